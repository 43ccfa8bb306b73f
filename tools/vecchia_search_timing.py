"""The neighbour search of the nearest-neighbour path on the device, brute entry against cell grid (fvgp_hip_nn_search against
fvgp_hip_nn_grid_build + fvgp_hip_nn_grid_search; VecchiaGP args["neighbor_search"]), one run:

    python tools/vecchia_search_timing.py [--out profiles/r21_vecchia_grid.txt] [--steps causal,predict,facade,big] [--windows 3]

    causal     the rows among themselves (c0 = 0), m = 32, N = 10^4, 3 10^4, 10^5, 3 10^5, 10^6: uniform rows at d = 1, 2, 3 in a random
               order and in a maxmin order (the first min(N, 16384) positions by fvgp_hip_nn_maxmin_order, so that ordering does not
               dominate the run), and one clustered set at d = 3 (a Gaussian mixture: 20 centres, sigma 0.01 of the box, random order).
               Per line: the brute entry, the grid build, the grid search, and whether the two index arrays are equal.  Below the table
               the "auto" threshold: the smallest measured N from which on build + search beats the brute entry on EVERY configuration.
    predict    1000 queries against N rows, every row a candidate (c0 < 0), d = 3, m = 32: brute, grid search (the grid is there already).
    facade     VecchiaGP(...) construction at d = 3, m = 32, ordering "random", with args["neighbor_search"] "brute" and "grid".
    big        N = 10^7, d = 3, m = 32, causal, random order: the grid route alone, once, if the device memory allows.
The brute entry is the reference: it is timed here, in the same run, never taken from an earlier record.  Every step runs in a process of
its own under its own time limit; a step that ends abnormally or runs out of time is written down as "not measured" and nothing is
started after it.  Wall clock around work that ends in a synchronisation: a warm-up, then the best of --windows with the spread
(max - min) / min; a brute search of 3 10^5 rows or more is timed once (its kernel is warm from the smaller sizes).  Nothing is asserted."""
import argparse
import os
import subprocess
import sys
import tempfile
import threading
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"causal": 540, "predict": 240, "facade": 300, "big": 300}      # seconds per step
SIZES = (10000, 30000, 100000, 300000, 1000000)
M = 32
MAXMIN_POINTS = 16384


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def best_ms(fn, windows, warm=True):
    if warm:
        fn()                                       # (code objects, the allocator)
    t = [wall_ms(fn)[0] for _ in range(windows)]
    return min(t), (max(t) - min(t)) / min(t)


def uniform(n, d, seed=20240601):
    return np.random.default_rng(seed + d).random((n, d))


def clustered(n, d=3, seed=20240602):
    """a Gaussian mixture: 20 centres uniform in the unit box, sigma 0.01, equal weights, in a random order"""
    rng = np.random.default_rng(seed)
    centres = rng.random((20, d))
    return centres[rng.integers(0, 20, n)] + 0.01 * rng.standard_normal((n, d))


def maxmin_order(H, x, scales):
    """x with its first min(n, MAXMIN_POINTS) positions in maxmin order, the rest behind them in a random order"""
    from fvgp_amd.gp_vecchia import first_point
    n = len(x)
    q = min(n, MAXMIN_POINTS)
    head, _ = H.nn_maxmin_order(H.to_device(x), first_point(x, scales), q, scales=scales, want_distances=False)
    rest = np.setdiff1d(np.arange(n, dtype=np.int64), head)
    rest = rest[np.random.default_rng(3).permutation(len(rest))]
    return np.ascontiguousarray(x[np.concatenate([head, rest])])


def time_pair(H, xd, scales, windows, c0=0, xq=None, brute=True):
    """(brute ms, spread, build ms, spread, search ms, spread, lists equal) for the rows of xd among themselves (or the queries xq)"""
    import torch
    n = xd.shape[0]
    xq = xd if xq is None else xq
    a = torch.empty((xq.shape[0], M), dtype=torch.int32, device=xd.device)
    b = torch.full_like(a, -2)
    tb = sb = float("nan")
    if brute:
        few = 1 if n >= 300000 else windows
        tb, sb = best_ms(lambda: H.nn_search(xq, xd, M, a, scales=scales, c0=c0), few, warm=n < 300000)
    tg, sg = best_ms(lambda: H.nn_grid_build(xd, scales), windows)
    grid = H.nn_grid_build(xd, scales)
    ts, ss = best_ms(lambda: H.nn_grid_search(xq, xd, M, b, grid, c0=c0), windows)
    same = bool(torch.equal(a, b)) if brute else None
    return tb, sb, tg, sg, ts, ss, same, grid


def step_causal(a, emit):
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    emit(f"causal  the rows among themselves (c0 = 0), m = {M}; ms, best of {a.windows} after a warm-up (spread); brute at N >= 300000: 1 run")
    emit("causal  configuration        d        N |      brute          |  grid build         |  grid search        | build+search | brute / grid | equal")
    wins = {n: True for n in SIZES}
    for n in SIZES:
        for name, d in (("uniform random", 1), ("uniform random", 2), ("uniform random", 3), ("uniform maxmin", 1), ("uniform maxmin", 2),
                        ("uniform maxmin", 3), ("clustered random", 3)):
            scales = np.array([0.3, 0.2, 0.4][:d])
            x = clustered(n) if name.startswith("clustered") else uniform(n, d)
            if name.endswith("maxmin"):
                x = maxmin_order(H, x, scales)
            xd = H.to_device(x)
            tb, sb, tg, sg, ts, ss, same, grid = time_pair(H, xd, scales, a.windows)
            wins[n] = wins[n] and (tg + ts < tb)
            emit(f"causal  {name:<17} d = {d}  {n:>8} | {tb:10.2f} ({sb:.3f}) | {tg:10.2f} ({sg:.3f}) | {ts:10.2f} ({ss:.3f}) | {tg + ts:10.2f}   | "
                 f"{tb / (tg + ts):9.2f}    | {same}   cells {'x'.join(map(str, grid.cells))}")
            del xd, grid
    ok = [n for n in SIZES if all(wins[k] for k in SIZES if k >= n)]
    emit(f"causal  build + search beats the brute entry on every configuration at N = {[n for n in SIZES if wins[n]]}")
    emit(f"causal  \"auto\" threshold (the smallest measured N from which on it wins on every configuration): "
         f"{ok[0] if ok else 'none: the grid loses at the largest size'}")
    H.close()


def step_predict(a, emit):
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    emit(f"predict  1000 queries against N rows, every row a candidate, d = 3, m = {M}; ms, best of {a.windows} (spread)")
    for n in SIZES:
        scales = np.array([0.3, 0.2, 0.4])
        xd = H.to_device(uniform(n, 3))
        xq = H.to_device(np.random.default_rng(9).random((1000, 3)) * 1.2 - 0.1)
        tb, sb, tg, sg, ts, ss, same, _ = time_pair(H, xd, scales, a.windows, c0=-1, xq=xq)
        emit(f"predict  N = {n:>8}: brute {tb:9.3f} ({sb:.3f}) | grid search {ts:9.3f} ({ss:.3f}) | brute / grid {tb / ts:8.1f} | equal {same}"
             f"   (grid build {tg:.2f}, made once per data set)")
    H.close()


def step_facade(a, emit):
    import fvgp_amd
    emit(f"facade  VecchiaGP(x, y, hps, noise, n_neighbors = {M}, ordering = 'random') at d = 3: construction (ordering, upload, search), ms")
    for n in (100000, 1000000):
        x = uniform(n, 3)
        y = np.sin(3.0 * x.sum(axis=1))
        times = {}
        for route in ("brute", "grid"):
            make = lambda: fvgp_amd.VecchiaGP(x, y, np.array([1.0, 0.3, 0.2, 0.4]), noise_variances=np.full(n, 0.01),      # noqa: E731
                                              kernel_function="matern32_ard", n_neighbors=M, args={"neighbor_search": route})
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                times[route] = best_ms(make, 1 if n >= 1000000 else a.windows)
        emit(f"facade  N = {n:>8}: brute {times['brute'][0]:10.1f} ({times['brute'][1]:.3f}) | grid {times['grid'][0]:10.1f} "
             f"({times['grid'][1]:.3f}) | brute / grid {times['brute'][0] / times['grid'][0]:6.2f}")


def step_big(a, emit):
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    n, d = 10 ** 7, 3
    need = _lib.nn_grid_bytes(n, d) + _lib.nn_grid_workspace_bytes(n, d) + n * (8 * d + 4 * M)
    free = torch.cuda.mem_get_info(0)[0]
    if need * 1.2 > free:
        emit(f"big  N = 10^7: not run, {need / 2 ** 30:.1f} GiB needed and {free / 2 ** 30:.1f} GiB free")
        return
    scales = np.array([0.3, 0.2, 0.4])
    xd = H.to_device(uniform(n, d))
    idx = torch.empty((n, M), dtype=torch.int32, device=xd.device)
    tg, grid = wall_ms(lambda: H.nn_grid_build(xd, scales))
    ts, _ = wall_ms(lambda: H.nn_grid_search(xd, xd, M, idx, grid, c0=0))
    emit(f"big  N = 10^7, d = 3, m = {M}, causal, uniform random, the grid route alone, 1 run without a warm-up: build {tg:.1f} ms, search "
         f"{ts:.1f} ms, cells {'x'.join(map(str, grid.cells))}; rows 10^7 - 5 .. 10^7 - 1 have {int((idx[-5:] >= 0).sum())} of {5 * M} neighbours")
    H.close()


STEPS = {"causal": step_causal, "predict": step_predict, "facade": step_facade, "big": step_big}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_vecchia_grid.txt"))
    ap.add_argument("--steps", default="causal,predict,facade,big")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a, lambda s: print(s, flush=True))
        return 0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    emit(f"# neighbour search of the nearest-neighbour path, brute entry against cell grid, one run; wall clock around work that ends in a "
         f"synchronisation, best of {a.windows} after a warm-up (spread = (max - min) / min) unless a line says otherwise; a step per "
         f"process, each under its own time limit")
    names = [s for s in a.steps.split(",") if s]
    for i, name in enumerate(names):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--windows", str(a.windows)]
        # the step's lines are passed on as they come (a long step is not silent), its time limit kept by a timer
        errfile = tempfile.TemporaryFile("w+")
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=errfile, text=True)
        late = []
        timer = threading.Timer(LIMITS[name], lambda: (late.append(1), proc.kill()))
        timer.start()
        for line in proc.stdout:
            emit(line.rstrip("\n"))
        rc = proc.wait()
        timer.cancel()
        errfile.seek(0)
        err = errfile.read()
        errfile.close()
        rc = 124 if late else rc
        if rc != 0:
            why = f"time limit of {LIMITS[name]} s" if rc == 124 else f"exit status {rc}: {err.strip().splitlines()[-1] if err.strip() else ''}"
            emit(f"{name}: not measured past this line ({why})")
            for rest in names[i + 1:]:
                emit(f"{rest}: not measured (not started after {name} ended abnormally)")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
