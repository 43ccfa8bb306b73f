"""The exact log-likelihood Hessian (fvgp_hip_loglik_hess) against the finite-difference route, in one process on the same GP.

    python tools/loglik_hessian_timing.py [--sizes 2000,8000,20000] [--dim 3] [--windows 3] [--out FILE]

For every N (rbf_ard, theta = [1, 0.3, ..], noise 0.01) one GP and, at its hyperparameters,
    exact   GP.neg_log_likelihood_exact_hessian   one factorisation, POTRI, per hyperparameter two N^3 products and one trace pass
    FD      GP.neg_log_likelihood_hessian         H + 1 exact gradients (factorisation + POTRI + trace pass each), forward difference
each warmed up first, the two alternating, every timed window bracketed by device synchronisations, the best of `--windows` kept with
the spread (max - min) / min; the largest relative difference of the two results rides along.  The products' rate: fvgp_hip_gemm on
the two shapes of the driver (np x np x np, all tiles: 2 np^3 flops; lower tiles: np^3) alone between two device events.  The kernels'
rates: one exact call and one gradient call under torch.profiler, device time per launch by kernel name, against the bytes each kernel
must move (the lower 128-tiles of W read once per pass by the two trace kernels and written once by kmat_kernel; np^2 doubles written
by kmat_grad_kernel)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("hess_trace_kernel", "grad_trace_kernel", "kmat_grad_kernel", "kmat_kernel")


def window(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_times(fn):
    """{kernel: (launches, mean device seconds per launch)} of one call of fn, or a string saying why there is none"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            us = getattr(e, "self_device_time_total", None)
            if us is None:
                us = getattr(e, "self_cuda_time_total", 0.0)
            for k in KERNELS:
                if k in e.key and us > 0:
                    c, t = out.get(k, (0, 0.0))
                    out[k] = (c + e.count, t + us * 1e-6)
        return {k: (c, t / c) for k, (c, t) in out.items()} or "the profiler recorded no device kernels"
    except Exception as ex:                                       # a build of torch without the device profiler
        return f"{type(ex).__name__}: {ex}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,8000,20000")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import fvgp_amd
    from fvgp_amd import _lib
    d = a.dim
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# exact log-likelihood Hessian timing: {torch.cuda.get_device_name(0)}, rbf_ard, d = {d} (H = {d + 1}); best of {a.windows} "
         f"synchronised windows (spread = (max - min) / min), alternating")
    emit(f"{'N':>6} | {'exact ms':>9} {'spread':>6} | {'FD ms':>9} {'spread':>6} | {'exact/FD':>8} {'(3H+1)/(H+1)':>12} | {'max|dH|/max|H|':>14} | "
         f"{'T=W K_i ms':>10} {'TFLOP/s':>7} | {'G=T W ms':>9} {'TFLOP/s':>7}")
    ktab = []
    for n in (int(v) for v in a.sizes.split(",")):
        rng = np.random.default_rng(20240501)
        x = rng.random((n, d))
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
        th = np.array([1.0] + [0.3] * d)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=np.full(n, 0.01), kernel_function="rbf_ard")
        fns = (lambda: gp.neg_log_likelihood_exact_hessian(th), lambda: gp.neg_log_likelihood_hessian(th))
        res = [f() for f in fns]                                   # warm-up (allocates the third square)
        t = [[] for _ in fns]
        for _ in range(a.windows):
            for k, f in enumerate(fns):
                t[k].append(window(f)[0])
        diff = float(np.max(np.abs(res[0] - res[1])) / np.max(np.abs(res[0])))
        # the two products alone, on the GP's own scratch squares
        H = gp._H
        np_ = _lib.pad128(n)
        A, B, C = gp._work, gp._work2, gp._work3
        A.normal_()
        B.normal_()
        tp = [[], []]
        for _ in range(a.windows + 1):
            for k, lower in enumerate((0, 1)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                H.gemm(0, 0, lower, np_, np_, np_, 1.0, A, B, 0.0, C)
                e1.record()
                torch.cuda.synchronize()
                tp[k].append(e0.elapsed_time(e1) * 1e-3)
        tp = [min(v[1:]) for v in tp]
        sp = lambda v: (max(v) - min(v)) / min(v)
        nh = d + 1
        emit(f"{n:6d} | {min(t[0]) * 1e3:9.2f} {sp(t[0]):6.3f} | {min(t[1]) * 1e3:9.2f} {sp(t[1]):6.3f} | {min(t[0]) / min(t[1]):8.2f} "
             f"{(3 * nh + 1) / (nh + 1):12.2f} | {diff:14.2e} | {tp[0] * 1e3:10.3f} {2.0 * float(np_) ** 3 / tp[0] / 1e12:7.1f} | "
             f"{tp[1] * 1e3:9.3f} {float(np_) ** 3 / tp[1] / 1e12:7.1f}")
        kt = [kernel_times(fns[0]), kernel_times(lambda: gp.neg_log_likelihood_gradient(th))]
        T = np_ // 128
        low = T * (T + 1) // 2 * 128 * 128 * 8.0
        ktab.append((n, np_, low, kt))
        del gp, A, B, C
        torch.cuda.empty_cache()
    emit("# kernels: device time per launch (torch.profiler) and the rate against the bytes the kernel must move; "
         "exact = inside the exact call, grad = inside neg_log_likelihood_gradient")
    emit(f"{'N':>6} | {'kernel':>28} | {'launches':>8} | {'ms':>9} | {'GB/s':>8}")
    for n, np_, low, kt in ktab:
        for tag, r, names in (("exact", kt[0], ("hess_trace_kernel", "grad_trace_kernel", "kmat_grad_kernel", "kmat_kernel")),
                              ("grad", kt[1], ("grad_trace_kernel", "kmat_kernel"))):
            if isinstance(r, str):
                emit(f"{n:6d} | {tag + ': not measured':>28} | {r}")
                continue
            for k in names:
                if k not in r:
                    continue
                c, s = r[k]
                nbytes = float(np_) ** 2 * 8.0 if k == "kmat_grad_kernel" else low
                emit(f"{n:6d} | {tag + ' ' + k:>28} | {c:8d} | {s * 1e3:9.3f} | {nbytes / s / 1e9:8.0f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
