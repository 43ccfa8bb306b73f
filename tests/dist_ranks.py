"""P ranks of the row-sharded path as P Python threads of one process (a helper module of the tests, not a conftest; never imported
by the package).

ShardedGP takes rank=, world=, ops= and a caller's _lib.Collectives, so a rank needs no process group: every rank gets its own ops
object (its own handle of the library) and a Collectives whose two callbacks meet the other ranks' at one threading.Barrier.  A
callback first drains the rank's device work (ops.host_sync()), parks a clone of its send buffer in the rank's slot and waits; then
every rank writes torch.cat(slots) (all-gather) or the sum of the slots in rank order (all-reduce: the same order on every rank, so
the replicated results agree in their bits) into its own receive buffer, drains again and waits again, so that no slot is replaced
while a peer still reads it.  ctypes releases the GIL around the library call and the callbacks take it back; the library's error
string is thread_local.

Failures end the case for every rank: an exception inside a callback is printed and becomes status 2999 (an exception cannot cross
the C frame), which the rank's ops object raises from the library call; an exception in a body aborts the barrier, so the peers'
waits raise and end the same way.  The threads are joined with a time limit and one that is still alive after it is a failure.

Host only for now: the tests run it over the CPU twin of the ABI (tests/dist_stub_ops.StubOps).  With one HIP handle per thread on one
device the four-rank cases ended in an abandoned launch of the resident panel kernel (chain.hip chain_wait: the spin-wait hand-off
gave up, info = 0x7fffffff) followed by a memory fault; until that cause is found, run no device ops under this harness.

Only for P > 1 and only with these callbacks: collectives="rccl" and "ipc" block inside the library and must never run under it.
One rank with force_collectives=True passes collectives="torch" (the library's own copy path) and needs no harness."""
import threading
import time
import traceback

from fvgp_amd import _lib


class RanksFailed(AssertionError):
    """a rank raised or did not come back; .errors: {rank: exception}"""

    def __init__(self, msg, errors):
        super().__init__(msg)
        self.errors = errors


def _callbacks(rank, P, ops, slots, barrier):
    torch = ops.torch

    def park(ptr, count):
        ops.host_sync()
        slots[rank] = ops.wrap(ptr, count).clone()
        ops.host_sync()
        barrier.wait()

    def leave():
        ops.host_sync()
        barrier.wait()

    def all_gather(ctx, send, recv, count, stream):
        try:
            park(send, count)
            ops.wrap(recv, count * P).copy_(torch.cat(list(slots)))
            leave()
            return 0
        except Exception as e:                                 # noqa: BLE001 -- an exception cannot cross the C frame
            print(f"dist_ranks: all_gather callback of rank {rank} failed: {type(e).__name__}: {e}", flush=True)
            return 2999

    def all_reduce(ctx, buf, count, stream):
        try:
            park(buf, count)
            total = slots[0].clone()
            for s in slots[1:]:
                total += s
            ops.wrap(buf, count).copy_(total)
            leave()
            return 0
        except Exception as e:                                 # noqa: BLE001
            print(f"dist_ranks: all_reduce callback of rank {rank} failed: {type(e).__name__}: {e}", flush=True)
            return 2999

    return _lib.Collectives(None, _lib.ALL_GATHER_FN(all_gather), _lib.ALL_REDUCE_FN(all_reduce))


def run_ranks(P, make_ops, body, timeout=120, barrier_timeout=60):
    """body(rank, ops, collectives) in P threads, ops = make_ops(rank); returns the P results in rank order.  Raises RanksFailed
    (from the first exception that is not the echo of a peer's failure) when a rank raised or outlived `timeout` seconds."""
    assert P > 1, "the thread harness is for more than one rank"
    barrier = threading.Barrier(P, timeout=barrier_timeout)
    slots = [None] * P
    opss = [make_ops(r) for r in range(P)]
    colls = [_callbacks(r, P, opss[r], slots, barrier) for r in range(P)]       # kept alive here for the life of the ranks
    for o, c in zip(opss, colls):
        o._rank_collectives = c
    results, errors = [None] * P, {}

    def run(r):
        try:
            results[r] = body(r, opss[r], colls[r])
        except BaseException as e:                              # noqa: BLE001 -- reported by the caller's thread
            errors[r] = e
            e._rank_traceback = traceback.format_exc()
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,), name=f"rank{r}", daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    if alive:
        barrier.abort()
        raise RanksFailed(f"ranks {alive} of {P} were still running after {timeout} s", errors)
    if errors:
        # a peer's failure reaches the other ranks as a broken barrier -> status 2999 from their library call: name the cause first
        first = sorted(errors, key=lambda r: ("2999" in str(errors[r]) or isinstance(errors[r], threading.BrokenBarrierError), r))[0]
        text = "\n".join(f"rank {r}: {type(e).__name__}: {e}" for r, e in sorted(errors.items()))
        raise RanksFailed(f"{len(errors)} of {P} ranks failed\n{text}\n{errors[first]._rank_traceback}", errors) from errors[first]
    return results
