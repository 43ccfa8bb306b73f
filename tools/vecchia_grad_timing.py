"""The exact gradient of the nearest-neighbour likelihood on the device (fvgp_hip_nn_loglik_grad, VecchiaGP.neg_log_likelihood_and_gradient),
one run:

    python tools/vecchia_grad_timing.py [--out profiles/r18_vecchia_grad.txt] [--steps rows,full,million] [--windows 3]

    rows      10^5 rows, Matern-3/2, d = 3, m = 16 / 32 / 64: fvgp_hip_nn_loglik_grad (value + scores + gradient) beside fvgp_hip_nn_loglik
              (value only) on the same inputs, rows per second each and their ratio
    full      N = 20 000, Matern-5/2, d = 3, m = 16 / 32 / 64: VecchiaGP.neg_log_likelihood_and_gradient beside (a) log_likelihood and
              (b) 2 H log_likelihood calls, the central-difference route to the same H numbers
    million   the same three at N = 10^6, m = 32
Every step runs in a process of its own under its own time limit; a step that ends abnormally or runs out of time is written down as
"not measured" and nothing is started after it.  Device events (best of --windows, spread = (max - min) / min) for the bare calls, wall
clock where the facade takes part."""
import argparse
import os
import subprocess
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vecchia_timing import data, event_ms, wall_ms      # noqa: E402

LIMITS = {"rows": 180, "full": 240, "million": 420}      # seconds per step


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
    for m in (16, 32, 64):
        idx = torch.empty((n, m), dtype=torch.int32, device=xd.device)
        H.nn_search(xd, xd, m, idx, scales=theta[1:], c0=0)
        wv = H.empty(max(1, _lib.nn_workspace_bytes(_lib.NN_LOGLIK, n, 1)) // 8)
        wg = H.empty(max(1, _lib.nn_grad_workspace_bytes(n, 1, 4)) // 8)
        tv, sv = event_ms(lambda: H.nn_loglik(1, xd, theta, idx, m, rd, vd, mu, var, work=wv), a.windows)
        tg, sg = event_ms(lambda: H.nn_loglik_grad(1, xd, theta, idx, m, rd, vd, mu, var, score, work=wg), a.windows)
        emit(f"rows  matern32_ard, d = 3, {n} rows, m = {m:>2}: value {tv:7.2f} ms (spread {sv:.3f}) = {n / tv / 1e3:7.2f} M rows/s, "
             f"value + gradient {tg:7.2f} ms (spread {sg:.3f}) = {n / tg / 1e3:7.2f} M rows/s, ratio {tg / tv:.2f}")
    H.close()


def _full(vg, a, emit, label):
    H2 = 2 * len(vg.hyperparameters)
    vg.log_likelihood()
    vg.neg_log_likelihood_and_gradient()
    tv = [wall_ms(vg.log_likelihood)[0] for _ in range(a.windows)]
    tg = [wall_ms(vg.neg_log_likelihood_and_gradient)[0] for _ in range(a.windows)]
    tc = [wall_ms(lambda: [vg.log_likelihood() for _ in range(H2)])[0] for _ in range(a.windows)]
    sp = lambda t: (max(t) - min(t)) / min(t)      # noqa: E731
    emit(f"{label}: value + gradient {min(tg):8.2f} ms (spread {sp(tg):.3f}); (a) log_likelihood {min(tv):8.2f} ms (spread {sp(tv):.3f}), "
         f"ratio {min(tg) / min(tv):.2f}; (b) {H2} log_likelihood calls {min(tc):8.2f} ms (spread {sp(tc):.3f}), ratio {min(tg) / min(tc):.2f}")


def step_full(a, emit):
    import fvgp_amd
    n = 20000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    emit(f"full  N = {n}, matern52_ard, d = 3, H = 4, noise 0.01 (wall clock, best of {a.windows})")
    for m in (16, 32, 64):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vg = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard", n_neighbors=m)
        _full(vg, a, emit, f"    m = {m:>2}")


def step_million(a, emit):
    import fvgp_amd
    n = 1000000
    x, y = data(n)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vg = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard", n_neighbors=32)
    _full(vg, a, emit, f"million  N = {n}, matern52_ard, d = 3, H = 4, m = 32 (wall clock, best of {a.windows})")


STEPS = {"rows": step_rows, "full": step_full, "million": step_million}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_vecchia_grad.txt"))
    ap.add_argument("--steps", default="rows,full,million")
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
    emit(f"# nearest-neighbour (Vecchia) gradient timing, one run; device events, best of {a.windows} (spread = (max - min) / min) unless a "
         "line says wall clock; a step per process, each under its own time limit")
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
