"""The nearest-neighbour (Vecchia) path on the device (fvgp_hip_nn_search, fvgp_hip_nn_conditionals, fvgp_hip_nn_loglik, VecchiaGP), one run:

    python tools/vecchia_timing.py [--out profiles/r17_vecchia.txt] [--steps search,conditionals,loglik,million] [--windows 3]

    search        fvgp_hip_nn_search of N = 10^5 and 10^6 points among themselves (causal), d = 3, m = 32
    conditionals  fvgp_hip_nn_conditionals over 10^5 rows at m = 16 / 32 / 64 (Matern-3/2, d = 3): rows per second, and the
                  factorisation's and substitutions' arithmetic (m^3 / 3 + 2 m^2 flop per row, padded m) as a fraction of 78.6 TFLOP/s,
                  the MI355X's vector-fp64 peak (256 CU x 4 SIMD x 16 lanes x 2 flop x 2.4 GHz)
    loglik        at N = 20 000 (Matern-5/2, d = 3, noise 0.01): VecchiaGP.log_likelihood at m = 16 / 32 / 64 beside the dense GP's
                  evaluation, and the gap |log p_vecchia - log p_exact| / N
    million       N = 10^6, m = 32 end to end: construction (the search) and one likelihood
Every step runs in a process of its own under its own time limit; a step that ends abnormally or runs out of time is written down as
"not measured" and nothing is started after it.  Device events (best of --windows, spread = (max - min) / min) for the kernels, wall
clock where the host takes part."""
import argparse
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"search": 240, "conditionals": 180, "loglik": 300, "million": 420}      # seconds per step
PEAK = 78.6e12


def event_ms(fn, windows):
    import torch
    t = []
    for i in range(windows + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            t.append(e0.elapsed_time(e1))
    return min(t), (max(t) - min(t)) / min(t)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def data(n, d=3, seed=20240501):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y


def step_search(a, emit):
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    sc = np.array([0.3, 0.3, 0.3])
    for n in (100000, 1000000):
        xd = H.to_device(data(n)[0])
        idx = torch.empty((n, 32), dtype=torch.int32, device=xd.device)
        ms, spread = event_ms(lambda: H.nn_search(xd, xd, 32, idx, scales=sc, c0=0), a.windows if n <= 100000 else 1)
        emit(f"search  N = {n:>8}, d = 3, m = 32, causal: {ms:10.1f} ms (spread {spread:.3f}), {n * (n - 1) / 2 / ms / 1e6:8.1f} G distances/s")
        del xd, idx
    H.close()


def step_conditionals(a, emit):
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    n = 100000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    xd, rd, vd = H.to_device(x), H.to_device(y - y.mean()), H.to_device(np.full(n, 0.01))
    mu, var = H.empty(1, n), H.empty(1, n)
    for m in (16, 32, 64):
        idx = torch.empty((n, m), dtype=torch.int32, device=xd.device)
        H.nn_search(xd, xd, m, idx, scales=theta[1:], c0=0)
        work = H.empty(max(1, _lib.nn_workspace_bytes(_lib.NN_CONDITIONALS, n, 1)) // 8)
        ms, spread = event_ms(lambda: H.nn_conditionals(1, xd, xd, theta, idx, m, rd, vd, mu, var, s=vd, work=work), a.windows)
        flop = n * (m ** 3 / 3.0 + 2.0 * m * m)
        emit(f"conditionals  matern32_ard, d = 3, {n} rows, m = {m:>2}: {ms:8.2f} ms (spread {spread:.3f}), {n / ms / 1e3:8.2f} M rows/s, "
             f"{flop / ms / 1e9:7.3f} TFLOP/s = {flop / ms * 1e3 / PEAK:.4f} of the vector-fp64 peak")
    H.close()


def step_loglik(a, emit):
    import fvgp_amd
    n = 20000
    x, y = data(n)
    V = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="matern52_ard")
        gp.log_likelihood(theta)
        t_dense = min(wall_ms(lambda: gp.log_likelihood(theta))[0] for _ in range(a.windows))
        exact = float(gp.log_likelihood(theta))
    emit(f"loglik  N = {n}, matern52_ard, d = 3, noise 0.01 (wall clock ms, best of {a.windows}): dense {t_dense:.1f} ms, log p = {exact:.6f}")
    for m in (16, 32, 64):
        t_build, vg = wall_ms(lambda: gp.vecchia(n_neighbors=m))
        vg.log_likelihood()
        t = min(wall_ms(vg.log_likelihood)[0] for _ in range(a.windows))
        ll = vg.log_likelihood()
        emit(f"    m = {m:>2}: construction (ordering, upload, search) {t_build:8.1f} ms, log_likelihood {t:7.2f} ms = {t / t_dense:.3f} x dense, "
             f"log p = {ll:.6f}, gap |log p - exact| / N = {abs(ll - exact) / n:.3e}")


def step_million(a, emit):
    import torch
    import fvgp_amd
    n = 1000000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t_build, vg = wall_ms(lambda: fvgp_amd.VecchiaGP(x, y, theta, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard",
                                                         n_neighbors=32))
    t_first, ll = wall_ms(vg.log_likelihood)
    t_ll = min(wall_ms(vg.log_likelihood)[0] for _ in range(a.windows))
    t_pred, _ = wall_ms(lambda: vg.posterior_mean(x[:1000] + 1e-3))
    free, total = torch.cuda.mem_get_info()
    emit(f"million  N = {n}, matern52_ard, d = 3, m = 32 (wall clock): construction {t_build / 1e3:.2f} s, first log_likelihood {t_first:.1f} ms, "
         f"then {t_ll:.1f} ms (log p = {ll:.3f}), posterior_mean at 1000 points {t_pred:.1f} ms; device memory in use "
         f"{(total - free) / 2 ** 30:.2f} GiB (allocator caches included)")


STEPS = {"search": step_search, "conditionals": step_conditionals, "loglik": step_loglik, "million": step_million}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_vecchia.txt"))
    ap.add_argument("--steps", default="search,conditionals,loglik,million")
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
    emit(f"# nearest-neighbour (Vecchia) timing, one run; device events, best of {a.windows} (spread = (max - min) / min) unless a line says "
         "wall clock; a step per process, each under its own time limit")
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
