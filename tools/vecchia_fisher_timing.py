"""The Fisher information of the nearest-neighbour likelihood on the device (fvgp_hip_nn_loglik_fisher,
VecchiaGP.neg_log_likelihood_gradient_and_fisher, train_gradient(method="fisher")), one run:

    python tools/vecchia_fisher_timing.py [--out profiles/r19_vecchia_fisher.txt] [--steps rows,full,train] [--windows 3]

    rows      10^5 rows, Matern-3/2, d = 3, m = 16 / 32 / 64: fvgp_hip_nn_loglik_fisher (value + gradient + Fisher rows and their sum) beside
              fvgp_hip_nn_loglik_grad (value + gradient) on the same inputs, rows per second each and their ratio
    full      N = 20 000, Matern-5/2, d = 3, m = 16 / 32 / 64: VecchiaGP.neg_log_likelihood_gradient_and_fisher beside
              neg_log_likelihood_and_gradient
    train     one 20 000-point problem, Matern-3/2, d = 3, m = 32, from theta = (3, 1.5, 1.5, 1.5): train_gradient(method="fisher") beside
              train_gradient(method="local"): iterations, device calls, wall time and the final objective
Every step runs in a process of its own under its own time limit; a step that ends abnormally or runs out of time is written down as
"not measured" and nothing is started after it.  Device events (best of --windows, spread = (max - min) / min) for the bare calls, wall
clock where the facade takes part."""
import argparse
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vecchia_timing import data, event_ms, wall_ms      # noqa: E402

LIMITS = {"rows": 180, "full": 180, "train": 240}      # seconds per step


def step_rows(a, emit):
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    n = 100000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    xd, rd, vd = H.to_device(x), H.to_device(y - y.mean()), H.to_device(np.full(n, 0.01))
    mu, var = H.empty(1, n), H.empty(1, n)
    score = torch.empty((1, n, 4), dtype=torch.float64, device=xd.device)
    rows = torch.empty((1, n, 10), dtype=torch.float64, device=xd.device)
    for m in (16, 32, 64):
        idx = torch.empty((n, m), dtype=torch.int32, device=xd.device)
        H.nn_search(xd, xd, m, idx, scales=theta[1:], c0=0)
        wg = H.empty(max(1, _lib.nn_grad_workspace_bytes(n, 1, 4)) // 8)
        wf = H.empty(max(1, _lib.nn_fisher_workspace_bytes(n, 1, 4)) // 8)
        tg, sg = event_ms(lambda: H.nn_loglik_grad(1, xd, theta, idx, m, rd, vd, mu, var, score, work=wg), a.windows)
        tf, sf = event_ms(lambda: H.nn_loglik_fisher(1, xd, theta, idx, m, rd, vd, mu, var, score, rows, work=wf), a.windows)
        emit(f"rows  matern32_ard, d = 3, {n} rows, m = {m:>2}: value + gradient {tg:7.2f} ms (spread {sg:.3f}) = {n / tg / 1e3:7.2f} M rows/s, "
             f"value + gradient + Fisher {tf:7.2f} ms (spread {sf:.3f}) = {n / tf / 1e3:7.2f} M rows/s, ratio {tf / tg:.2f}")
    H.close()


def step_full(a, emit):
    import fvgp_amd
    n = 20000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    sp = lambda t: (max(t) - min(t)) / min(t)      # noqa: E731
    emit(f"full  N = {n}, matern52_ard, d = 3, H = 4, noise 0.01 (wall clock, best of {a.windows})")
    for m in (16, 32, 64):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vg = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard", n_neighbors=m)
        vg.neg_log_likelihood_and_gradient()
        vg.neg_log_likelihood_gradient_and_fisher()
        tg = [wall_ms(vg.neg_log_likelihood_and_gradient)[0] for _ in range(a.windows)]
        tf = [wall_ms(vg.neg_log_likelihood_gradient_and_fisher)[0] for _ in range(a.windows)]
        emit(f"    m = {m:>2}: value + gradient + Fisher {min(tf):8.2f} ms (spread {sp(tf):.3f}); value + gradient {min(tg):8.2f} ms "
             f"(spread {sp(tg):.3f}), ratio {min(tf) / min(tg):.2f}")


def step_train(a, emit):
    import fvgp_amd
    n, m = 20000, 32
    x, y = data(n)
    start = np.array([3.0, 1.5, 1.5, 1.5])
    bounds = np.array([[0.01, 100.0]] + [[0.01, 10.0]] * 3)
    emit(f"train  N = {n}, matern32_ard, d = 3, m = {m}, noise 0.01, start {start.tolist()}, tolerance 1e-6 (wall clock, one run each)")

    def fresh():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fvgp_amd.VecchiaGP(x, y, np.array([1.0, 0.3, 0.3, 0.3]), noise_variances=np.full(n, 0.01), kernel_function="matern32_ard",
                                      n_neighbors=m)
    vg = fresh()
    vg.neg_log_likelihood_gradient_and_fisher()
    t0 = time.perf_counter()
    th = vg.train_gradient(bounds, init_hyperparameters=start, method="fisher", tolerance=1e-6, max_iter=200)
    tf = time.perf_counter() - t0
    hist = vg.fisher_history
    emit(f"    fisher : {len(hist) - 1:4d} iterations, {vg.fisher_evaluations:4d} device calls, {tf * 1e3:9.1f} ms, f {hist[0][1]:.4f} -> "
         f"{vg.neg_log_likelihood():.6f}, last decrement {hist[-1][2]:.2e}, theta {np.round(th, 5).tolist()}")
    vl = fresh()
    vl.neg_log_likelihood_and_gradient()
    calls = [0]
    inner = vl.neg_log_likelihood_and_gradient

    def counted(hps=None):
        calls[0] += 1
        return inner(hps)
    vl.neg_log_likelihood_and_gradient = counted
    t0 = time.perf_counter()
    tl_theta = vl.train_gradient(bounds, init_hyperparameters=start, method="local", tolerance=1e-6, max_iter=200)
    tl = time.perf_counter() - t0
    emit(f"    local  : L-BFGS-B, {calls[0]:4d} device calls, {tl * 1e3:9.1f} ms, f -> {vl.neg_log_likelihood():.6f}, theta "
         f"{np.round(tl_theta, 5).tolist()}")


STEPS = {"rows": step_rows, "full": step_full, "train": step_train}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_vecchia_fisher.txt"))
    ap.add_argument("--steps", default="rows,full,train")
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
    emit(f"# nearest-neighbour (Vecchia) Fisher information timing, one run; device events, best of {a.windows} (spread = (max - min) / min) "
         "unless a line says wall clock; a step per process, each under its own time limit")
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
