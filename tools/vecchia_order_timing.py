"""The maxmin ordering of the nearest-neighbour path on the device (fvgp_hip_nn_maxmin_order, VecchiaGP(ordering="maxmin")), one run:

    python tools/vecchia_order_timing.py [--out profiles/r20_vecchia_order.txt] [--steps order,accuracy] [--windows 3]

    order      Handle.nn_maxmin_order at d = 3: N = 2 10^4 and 10^5 with q = N, N = 10^6 with q = 65 536; the time and the microseconds per
               step, and beside each two floors measured in the same process: the per-step time of the same entry over 256 points (one
               workgroup that has next to nothing to do: what q launches back to back on this stream cost by themselves), and the bytes
               a step reads at most (8 (d + 1) N) over the rate of a device-to-device copy.  N = 10^6 with q = N runs only if the per-step
               time at q = 65 536 projects it under 60 s; else the projection is printed.
    accuracy   DESIGN 24's fixture (N = 20 000, Matern-5/2, d = 3, noise 0.01) at m = 16 / 32 / 64, ordering "random" (seed 0) against
               "maxmin": construction time, |log p - exact| / N against the dense GP.log_likelihood, and (sum log d) / N -- the ordering
               with the lower sum has the lower KL to the exact GP, by half the difference times N nats.
Every step runs in a process of its own under its own time limit; a step that ends abnormally or runs out of time is written down as
"not measured" and nothing is started after it.  Wall clock around work that ends in a synchronisation (the host enqueues every step's
launch, so its time is part of the ordering's): best of --windows, spread = (max - min) / min.  Nothing is asserted."""
import argparse
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"order": 420, "accuracy": 420}      # seconds per step
D = 3


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def best_ms(fn, windows):
    fn()                                           # (warm: code objects, the allocator)
    t = [wall_ms(fn)[0] for _ in range(windows)]
    return min(t), (max(t) - min(t)) / min(t)


def data(n, d=D, seed=20240501):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y


def step_order(a, emit):
    import torch
    from fvgp_amd import _lib
    from fvgp_amd.gp_vecchia import first_point
    H = _lib.Handle(0)
    sc = np.array([0.3, 0.3, 0.3])
    # floor 1: the launches themselves
    tiny = H.to_device(data(256)[0])
    ms, spread = best_ms(lambda: H.nn_maxmin_order(tiny, 0, scales=sc), a.windows)
    launch_us = ms * 1e3 / 256
    emit(f"order  floor, launches: N = q = 256 (one workgroup per step), {ms:.3f} ms = {launch_us:.2f} us per step (best of {a.windows}, "
         f"spread {spread:.3f})")
    # floor 2: the memory system
    src = torch.empty(1 << 25, dtype=torch.float64, device=tiny.device)
    dst = torch.empty_like(src)
    ms, spread = best_ms(lambda: dst.copy_(src), a.windows)
    rate = 2 * src.numel() * 8 / (ms * 1e-3)
    emit(f"order  floor, memory: device copy of {src.numel() * 8 >> 20} MiB, {ms:.3f} ms = {rate / 1e12:.2f} TB/s read + written (best of "
         f"{a.windows}, spread {spread:.3f})")
    del src, dst
    per_step = None
    for n, q in ((20000, 20000), (100000, 100000), (1000000, 65536)):
        x = data(n)[0]
        xd = H.to_device(x)
        first = first_point(x, sc)
        ms, spread = best_ms(lambda: H.nn_maxmin_order(xd, first, q=q, scales=sc), a.windows)
        per_step = ms * 1e3 / q
        stream_us = 8 * (D + 1) * n / rate * 1e6
        emit(f"order  N = {n:>8}, q = {q:>7}, d = {D}: {ms:10.1f} ms = {per_step:7.2f} us per step (best of {a.windows}, spread {spread:.3f}); "
             f"floors per step: launch {launch_us:.2f} us, {8 * (D + 1) * n / 1e6:.2f} MB at the copy's rate {stream_us:.2f} us")
    n = 1000000
    projected = per_step * n / 1e6
    if projected < 60.0:
        ms, (perm, dist) = wall_ms(lambda: H.nn_maxmin_order(xd, first, scales=sc))
        ok = len(np.unique(perm)) == n and bool(np.all(dist[2:] <= dist[1:-1]))
        emit(f"order  N = {n:>8}, q = {n:>7}, d = {D}: {ms / 1e3:10.2f} s = {ms * 1e3 / n:7.2f} us per step (1 run; projected {projected:.1f} s "
             f"from q = 65536); a permutation with non-increasing distances: {ok}")
    else:
        emit(f"order  N = {n:>8}, q = {n:>7}: not run, projected {projected:.1f} s from the per-step time at q = 65536 (the limit is 60 s)")
    H.close()


def step_accuracy(a, emit):
    import fvgp_amd
    n = 20000
    x, y = data(n)
    V = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="matern52_ard")
        exact = float(gp.log_likelihood(theta))
    emit(f"accuracy  N = {n}, matern52_ard, d = {D}, noise 0.01: dense log p = {exact:.6f}; construction = ordering, upload and search, "
         f"wall clock, best of {a.windows}")
    for m in (16, 32, 64):
        for ordering in ("random", "maxmin"):
            build = lambda: gp.vecchia(n_neighbors=m, ordering=ordering, seed=0)      # noqa: E731
            t_build, spread = best_ms(build, a.windows)
            vg = build()
            ll = vg.log_likelihood()
            sld = float(np.sum(np.log(vg.conditionals()["variance"])))
            emit(f"    m = {m:>2}, {ordering:>6}: construction {t_build:8.1f} ms (spread {spread:.3f}), log p = {ll:.6f}, "
                 f"gap |log p - exact| / N = {abs(ll - exact) / n:.3e}, (sum log d) / N = {sld / n:.6f}  (1 evaluation: deterministic)")


STEPS = {"order": step_order, "accuracy": step_accuracy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_vecchia_order.txt"))
    ap.add_argument("--steps", default="order,accuracy")
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
    emit(f"# maxmin ordering of the nearest-neighbour path, one run; wall clock around work that ends in a synchronisation, best of "
         f"{a.windows} after a warm-up (spread = (max - min) / min) unless a line says otherwise; a step per process, each under its own time limit")
    names = [s for s in a.steps.split(",") if s]
    for i, name in enumerate(names):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--windows", str(a.windows)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
            rc, out, err = res.returncode, res.stdout, res.stderr
        except subprocess.TimeoutExpired as e:
            rc, out, err = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), ""
        for line in out.splitlines():
            emit(line)
        if rc != 0:
            why = f"time limit of {LIMITS[name]} s" if rc == 124 else f"exit status {rc}: {err.strip().splitlines()[-1] if err.strip() else ''}"
            emit(f"{name}: not measured past this line ({why})")
            for rest in names[i + 1:]:
                emit(f"{rest}: not measured (not started after {name} ended abnormally)")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
