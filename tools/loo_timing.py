"""Leave-one-out cross-validation (fvgp_hip_loo) against the marginal likelihood's value + gradient, in one process on the same data.

    python tools/loo_timing.py [--sizes 2000,8000,20000] [--dim 3] [--windows 5] [--out FILE]

For every N (RBF, theta = [1, 0.3, ..], noise 0.01): one factorisation (Handle.loglik) followed by
    value only        Handle.loo without the gradient (POTRI + the pass over the diagonal)
    value + gradient  Handle.loo
    likelihood v + g  Handle.loglik_grad (POTRI + the fused trace pass)
each shape warmed up first, the three alternating, every timed window bracketed by device synchronisations, the best of `--windows`
kept with the spread (max - min) / min.  The factorisation is timed the same way and is part of every figure.  The product's rate:
fvgp_hip_gemm on the same shape (np x np x np, lower tiles: np^3 flops) alone between two device events."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8000,20000")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    d = a.dim
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# LOO timing: {torch.cuda.get_device_name(0)}, RBF, d = {d}; factorisation + call, best of {a.windows} synchronised windows "
         f"(spread = (max - min) / min), alternating; product = S S^T (lower tiles, np^3 flops) alone between device events")
    emit(f"{'N':>6} | {'factor ms':>9} | {'LOO value ms':>12} {'spread':>6} | {'LOO v+g ms':>10} {'spread':>6} | {'lik v+g ms':>10} {'spread':>6} | "
         f"{'ratio':>5} | {'product ms':>10} {'TFLOP/s':>7}")
    for n in (int(v) for v in a.sizes.split(",")):
        rng = np.random.default_rng(20240501)
        x = rng.random((n, d))
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
        th = np.array([1.0] + [0.3] * d)
        np_, dim = _lib.pad128(n), _lib.loglik_dim(n, 1)
        xd, vd, yd = H.to_device(x), H.to_device(np.full(n, 0.01)), H.to_device((y - y.mean()).reshape(n, 1))
        KV, work, alpha = H.empty(dim, dim), H.empty(np_, np_), H.empty(np_, 1)
        ws = H.empty(_lib.loo_workspace_bytes(n) // 8)
        resid, var, u, md = H.empty(n), H.empty(n), H.empty(n), H.empty(n)

        def factor():
            assert H.loglik(0, xd, th, vd, yd, KV, alpha)[3] == 0

        def loo_value():
            factor()
            H.loo(None, None, None, alpha, 1, 0, KV, work, ws, resid, var, n=n)

        def loo_grad():
            factor()
            H.loo(0, xd, th, alpha, 1, 0, KV, work, ws, resid, var, u, md)

        def lik_grad():
            factor()
            H.loglik_grad(0, xd, th, alpha, 1, 0, KV, work)
        fns = (factor, loo_value, loo_grad, lik_grad)
        for f in fns:
            f()
        t = [[] for _ in fns]
        for _ in range(a.windows):
            for k, f in enumerate(fns):
                t[k].append(window(f))
        tp = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            H.gemm(0, 0, 1, np_, np_, np_, 1.0, KV, KV, 0.0, work)
            e1.record()
            torch.cuda.synchronize()
            tp.append(e0.elapsed_time(e1) * 1e-3)
        sp = lambda v: (max(v) - min(v)) / min(v)
        emit(f"{n:6d} | {min(t[0]) * 1e3:9.3f} | {min(t[1]) * 1e3:12.3f} {sp(t[1]):6.3f} | {min(t[2]) * 1e3:10.3f} {sp(t[2]):6.3f} | "
             f"{min(t[3]) * 1e3:10.3f} {sp(t[3]):6.3f} | {min(t[2]) / min(t[3]):5.2f} | {min(tp) * 1e3:10.3f} {float(np_) ** 3 / min(tp) / 1e12:7.1f}")
        del KV, work
    H.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
