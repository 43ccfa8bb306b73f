"""GP.posterior_gradients (one analytic device pass) against the finite-difference pair posterior_mean_grad + posterior_covariance_grad,
in one process, on the same GP and prediction points; and the gradient kernel's own rate.

    python tools/posterior_grad_timing.py [--sizes 500:3,4000:3,20000:3] [--points 1000] [--windows 5] [--out FILE]
    python tools/posterior_grad_timing.py --kernel-only [--calls 20] ...          (the ABI call alone, for a rocprofv3 --kernel-trace --stats run)

For every size (N, d): RBF at theta = [1, 0.3, ..], P uniform prediction points; every shape warmed up first; the two sides alternate,
each timed window is bracketed by device synchronisations, the best of `--windows` is kept and the spread (max - min) / min over the
windows is reported.  The kernel's rate: Handle.posterior_grad alone (both launches: the pass over W and the reduction of the slices)
between two device events, `--calls` calls per window, over the 8 N P bytes of W it reads once."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0          # MI355X HBM3E peak


def synth(n, d, seed=20240501):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    return x, np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)


def window(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500:3,4000:3,20000:3")
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="run the ABI call alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import fvgp_amd
    from fvgp_amd import _lib
    P = a.points
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# posterior_gradients timing: {torch.cuda.get_device_name(0)}, P = {P} points, RBF, best of {a.windows} synchronised windows "
         f"(spread = (max - min) / min), the two sides alternating; kernel = Handle.posterior_grad alone between device events, "
         f"{a.calls} calls per window, GB/s over 8 N P bytes")
    emit(f"{'N':>6} {'d':>2} | {'analytic ms':>11} {'spread':>6} | {'FD pair ms':>10} {'spread':>6} | {'ratio':>6} | {'kernel us':>9} {'GB/s':>7} {'% HBM':>5}")
    for spec in a.sizes.split(","):
        n, d = (int(v) for v in spec.split(":"))
        x, y = synth(n, d)
        th = np.array([1.0] + [0.3] * d)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=np.full(n, 0.01), kernel_function="rbf_ard")
        xp = np.random.default_rng(n).random((P, d))
        H = gp._H
        Pp = _lib.pad128(P)
        xpd = H.to_device(xp)
        W = H.empty(gp._np, Pp)
        H.kmat(0, gp._x_dev, xpd, th, W, pad=_lib.PAD_ZERO)
        H.potrs_cols(gp._L, n, W, Pp)
        work = H.empty(_lib.posterior_grad_workspace_bytes(n, P, d) // 8)
        A, q, dm, dv = H.empty(P), H.empty(P), H.empty(P, d), H.empty(P, d)

        def kern():
            for _ in range(a.calls):
                H.posterior_grad(0, gp._x_dev, th, xpd, gp._alpha, 1, 0, W, d, work, A, q, dm, dv)
        kern()
        tk = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            kern()
            e1.record()
            torch.cuda.synchronize()
            tk.append(e0.elapsed_time(e1) * 1e-3 / a.calls)
        gbs = 8.0 * n * P / min(tk) / 1e9
        if a.kernel_only:
            emit(f"{n:6d} {d:2d} | {'':>11} {'':>6} | {'':>10} {'':>6} | {'':>6} | {min(tk) * 1e6:9.1f} {gbs:7.0f} {100 * gbs / HBM_GBS:5.1f}")
            continue

        def new():
            gp.posterior_gradients(xp)

        def pair():
            gp.posterior_mean_grad(xp)
            gp.posterior_covariance_grad(xp)
        new(); pair()
        tn, tp = [], []
        for _ in range(a.windows):
            tn.append(window(new)); tp.append(window(pair))
        emit(f"{n:6d} {d:2d} | {min(tn) * 1e3:11.3f} {(max(tn) - min(tn)) / min(tn):6.3f} | {min(tp) * 1e3:10.3f} {(max(tp) - min(tp)) / min(tp):6.3f} | "
             f"{min(tp) / min(tn):6.2f} | {min(tk) * 1e6:9.1f} {gbs:7.0f} {100 * gbs / HBM_GBS:5.1f}")
        del gp, W
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
