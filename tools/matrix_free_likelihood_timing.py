"""The stochastic log-likelihood of the matrix-free path on the device (fvgp_hip_kgrad_form, fvgp_hip_precond_probes, fvgp_hip_precond_apply,
fvgp_hip_pcg_lanczos, MatrixFreeGP.log_likelihood_estimate), one run:

    python tools/matrix_free_likelihood_timing.py [--rates 20000,100000] [--dense 20000] [--big 200000] [--rank 256] [--probes 16]
                                                  [--windows 3] [--limit 600] [--out FILE]

    rates   fvgp_hip_kgrad_form on an n x n form, d = 3, RBF and Matern-5/2, s = 1 and 16 columns: kernel evaluations per second (n^2 / time,
            an entry is evaluated once per group of columns), beside fvgp_hip_kmatvec on the same points and columns in the same run
    dense   at N = --dense (Matern-5/2, d = 3, noise 0.01): one value + gradient estimate (the preconditioner, alpha, --probes probes,
            the forms), with its standard errors, beside the dense GP's exact value + gradient and the difference between the two in
            standard errors
    big     at each N of --big (sizes no dense call holds), rank --rank: one value + gradient estimate; the probes' iteration limit is
            sized from a measured product so that the estimate ends within --limit seconds
Device events on the handle's stream for the kernels (best of --windows, spread = (max - min) / min); wall clock where the host takes part."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def describe(e):
    return (f"log likelihood {e['log_likelihood']:.3f} +- {e['std_error']:.3f}, log det {e['logdet']:.3f} +- {e['logdet_std_error']:.3f} "
            f"(preconditioner {e['logdet_preconditioner']:.3f}), gradient {np.array2string(e['neg_gradient'], precision=3)} +- "
            f"{np.array2string(e['neg_gradient_std_error'], precision=3)}, probe iterations {int(e['iterations'].min())} .. "
            f"{int(e['iterations'].max())}, recorded steps <= {int(e['lanczos_steps'].max())}, alpha iterations {e['alpha_iterations']}, "
            f"converged {e['converged']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", default="20000,100000")
    ap.add_argument("--dense", type=int, default=20000)
    ap.add_argument("--big", default="200000")
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--limit", type=float, default=600.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import fvgp_amd
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    d = 3
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    sizes = lambda s: [int(v) for v in s.split(",") if v]      # noqa: E731
    emit(f"# matrix-free likelihood timing: {torch.cuda.get_device_name(0)}, d = {d}, one run; device events, best of {a.windows} "
         f"(spread = (max - min) / min) unless a line says wall clock")

    # ---- rates ----------------------------------------------------------------------------------------------------------------
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    emit(f"{'kernel':>12} {'n':>7} {'s':>3} | {'form ms':>9} {'spread':>6} {'Gk/s':>7} | {'matvec ms':>9} {'spread':>6} {'Gk/s':>7} | {'form / matvec':>13}")
    for n in sizes(a.rates):
        x, _ = data(n)
        xd = H.to_device(x)
        rng = np.random.default_rng(1)
        U, W, Y = H.to_device(rng.standard_normal((n, 16))), H.to_device(rng.standard_normal((n, 16))), H.empty(n, 16)
        gwork = H.empty(max(1, _lib.kgrad_form_workspace_bytes(n, n) // 8))
        mwork = H.empty(max(1, _lib.kmatvec_workspace_bytes(n, n, 16) // 8))
        for kernel in ("rbf_ard", "matern52_ard"):
            kid = _lib.KERNEL_IDS[kernel]
            for s in (1, 16):
                fm, fs = event_ms(lambda: H.kgrad_form(kid, xd, U, xd, W, theta, s=s, work=gwork), a.windows)
                mm, ms = event_ms(lambda: H.kmatvec(kid, xd, xd, theta, W, Y, s=s, work=mwork), a.windows)
                emit(f"{kernel:>12} {n:>7} {s:>3} | {fm:>9.3f} {fs:>6.3f} {n * n / fm / 1e6:>7.1f} | {mm:>9.3f} {ms:>6.3f} {n * n / mm / 1e6:>7.1f} | "
                     f"{fm / mm:>13.2f}")
        del xd, U, W, Y, gwork, mwork
    torch.cuda.empty_cache()

    # ---- N = --dense beside the dense path ------------------------------------------------------------------------------------------
    if a.dense:
        n = a.dense
        x, y = data(n)
        V = np.full(n, 0.01)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="matern52_ard")
            gp.neg_log_likelihood_gradient(theta)                       # (first call: its scratch)
            t_val, val = wall_ms(lambda: gp.neg_log_likelihood(theta))
            t_grad, grad = wall_ms(lambda: gp.neg_log_likelihood_gradient(theta))
            mf = gp.matrix_free(args={"precond_rank": a.rank})
            t_est, e = wall_ms(lambda: mf.log_likelihood_estimate(theta, n_probes=a.probes, seed=0, gradient=True))
        emit(f"N = {n}, matern52_ard, noise 0.01, wall clock ms, one run -- dense: value {t_val:.1f}, gradient {t_grad:.1f} "
             f"(log likelihood {-float(val):.3f}, gradient {np.array2string(np.asarray(grad), precision=3)})")
        emit(f"    matrix-free rank {a.rank}, {a.probes} probes: value + gradient estimate {t_est:.1f} ms = {t_est / (t_val + t_grad):.1f} x dense; "
             + describe(e))
        emit(f"    estimate - exact, in reported standard errors: value {(e['log_likelihood'] + float(val)) / e['std_error']:.2f}, gradient "
             f"{np.array2string((e['neg_gradient'] - np.asarray(grad)) / e['neg_gradient_std_error'], precision=2)}")
        del gp, mf
        torch.cuda.empty_cache()

    # ---- sizes no dense call holds -------------------------------------------------------------------------------------------------------
    for n in sizes(a.big):
        x, y = data(n)
        V = np.full(n, 0.01)
        xd = H.to_device(x)
        B, Y = H.to_device(np.random.default_rng(2).standard_normal((n, 16))), H.empty(n, 16)
        H.kmatvec(2, xd, xd, theta, B, Y, s=16)
        t_mv, _ = wall_ms(lambda: H.kmatvec(2, xd, xd, theta, B, Y, s=16))
        del xd, B, Y
        # one probe block costs about (iterations + 2) products of 16 columns; alpha and the forms ride in the margin
        max_iter = max(8, min(1000, int(0.5 * a.limit * 1e3 / t_mv / max(1, (a.probes + 15) // 16)) - 4))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mf = fvgp_amd.MatrixFreeGP(x, y, theta, noise_variances=V, kernel_function="matern52_ard",
                                       args={"precond_rank": a.rank, "max_iter": max_iter})
            t_pre, _ = wall_ms(mf._preconditioner)
            t_est, e = wall_ms(lambda: mf.log_likelihood_estimate(n_probes=a.probes, seed=0, gradient=True))
        free, total = torch.cuda.mem_get_info()
        emit(f"N = {n}, matern52_ard, noise 0.01, rank {a.rank}, {a.probes} probes (wall clock, one run): one product of 16 columns "
             f"{t_mv:.1f} ms, preconditioner {t_pre / 1e3:.2f} s (achieved rank {mf._rank}), value + gradient estimate {t_est / 1e3:.2f} s "
             f"(iteration limit {max_iter}); " + describe(e) + f"; device memory in use {(total - free) / 2 ** 30:.2f} GiB (allocator caches "
             f"included)")
        del mf
        torch.cuda.empty_cache()
    H.close()


if __name__ == "__main__":
    main()
