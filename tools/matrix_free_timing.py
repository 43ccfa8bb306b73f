"""The matrix-free path on the device (fvgp_hip_kmatvec, fvgp_hip_pchol, fvgp_hip_precond_factor, fvgp_hip_pcg, MatrixFreeGP), one run:

    python tools/matrix_free_timing.py [--rates 20000,100000] [--dense 20000] [--big 200000,500000] [--ranks 128,256] [--windows 3]
                                       [--limit 240] [--out FILE]

    rates   fvgp_hip_kmatvec on an n x n product, d = 3, RBF and Matern-5/2, s = 1, 4, 8, 16 columns: kernel evaluations per second
            (n^2 / time, the kernel is evaluated once per group of columns) and the time per column relative to s = 1; beside it
            select_cross_kernel's rate from one fvgp_hip_select_batch at N = 20000, P = 100000, q = 16 less its q column solves (as
            tools/select_batch_timing.py measures it: a difference of two minima)
    dense   at N = --dense (Matern-5/2, d = 3, noise 0.01): the preconditioner's build, the alpha solve (iterations, ms), the mean at 1000
            points and the variances at 64, beside the dense GP's evaluation and the same predictions
    big     at each N of --big (sizes no dense call holds): time per product, the build and the alpha solve at each rank (iterations,
            seconds, converged), device memory in use.  One run each; the iteration limit of a solve is sized from the measured time per
            product so that it ends within --limit seconds
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", default="20000,100000")
    ap.add_argument("--dense", type=int, default=20000)
    ap.add_argument("--big", default="200000,500000")
    ap.add_argument("--ranks", default="128,256")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0)
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
    emit(f"# matrix-free timing: {torch.cuda.get_device_name(0)}, d = {d}, one run; device events, best of {a.windows} "
         f"(spread = (max - min) / min) unless a line says wall clock")

    # ---- rates ----------------------------------------------------------------------------------------------------------------
    th = {"rbf_ard": np.array([1.0, 0.3, 0.3, 0.3]), "matern52_ard": np.array([1.0, 0.3, 0.3, 0.3])}
    emit(f"{'kernel':>12} {'n':>7} {'s':>3} | {'ms':>9} {'spread':>6} | {'Gk/s':>7} | {'per column / s=1':>16}")
    for n in sizes(a.rates):
        x, _ = data(n)
        xd = H.to_device(x)
        B, Y = H.to_device(np.random.default_rng(1).standard_normal((n, 16))), H.empty(n, 16)
        work = H.empty(max(1, _lib.kmatvec_workspace_bytes(n, n, 16) // 8))      # (without it option "matvec_split" = 0 cannot split)
        for kernel in ("rbf_ard", "matern52_ard"):
            t1 = None
            for s in (1, 4, 8, 16):
                ms, sp = event_ms(lambda: H.kmatvec(_lib.KERNEL_IDS[kernel], xd, xd, th[kernel], B, Y, s=s, work=work), a.windows)
                t1 = ms if s == 1 else t1
                emit(f"{kernel:>12} {n:>7} {s:>3} | {ms:>9.3f} {sp:>6.3f} | {n * n / ms / 1e6:>7.1f} | {ms / s / t1:>16.3f}")
    if sizes(a.rates):
        n, P, q = 20000, 100000, 16
        x, y = data(n)
        np_, dim = _lib.pad128(n), _lib.loglik_dim(n, 1)
        xd, vd, yd = H.to_device(x), H.to_device(np.full(n, 0.01)), H.to_device((y - y.mean()).reshape(n, 1))
        KV, alpha = H.empty(dim, dim), H.empty(np_, 1)
        assert H.loglik(0, xd, th["rbf_ard"], vd, yd, KV, alpha)[3] == 0
        xc = H.to_device(np.random.default_rng(2).random((P, d)))
        var0 = H.to_device(np.full(P, 0.5))
        var, idx, pick = H.empty(P), torch.empty(q, dtype=torch.int64, device=var0.device), H.empty(q)
        work = H.empty(_lib.select_workspace_bytes(n, P, q) // 8)
        col = H.empty(np_, 1)

        def call():
            var.copy_(var0)
            H.select_batch(0, xd, th["rbf_ard"], KV, xc, var, q, idx, pick, work=work)

        def sweeps():
            for _ in range(q):
                H.kmat(0, xc[:1], xd, th["rbf_ard"], col.view(1, np_))
                H.potrs(KV, n, col, 1)
        tc, sc = event_ms(call, a.windows)
        ts, ss = event_ms(sweeps, a.windows)
        cross = max(tc - ts, 1e-6) / q
        emit(f"select_cross_kernel beside it (rbf_ard, N = {n}, P = {P}, q = {q}): call {tc:.2f} ms (spread {sc:.3f}), sweeps {ts:.2f} ms "
             f"(spread {ss:.3f}), cross {cross:.3f} ms / step = {n * P / cross / 1e6:.1f} Gk/s (a difference of two minima: includes the pick, "
             f"the downdate and launch gaps)")
        del KV, work, xc

    # ---- N = --dense beside the dense path ------------------------------------------------------------------------------------------
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    if a.dense:
        n = a.dense
        x, y = data(n)
        V = np.full(n, 0.01)
        xp = np.random.default_rng(3).random((1000, d))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t_dense, gp = wall_ms(lambda: fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="matern52_ard"))
            t_dm, dm = wall_ms(lambda: gp.posterior_mean(xp)["m(x)"])
            t_dv, dv = wall_ms(lambda: gp.posterior_covariance(xp[:64], variance_only=True)["v(x)"])
            t_eval, _ = wall_ms(lambda: gp.log_likelihood(theta))
        emit(f"N = {n}, matern52_ard, noise 0.01, wall clock ms -- dense: construction (one evaluation + uploads) {t_dense:.1f}, one more "
             f"evaluation {t_eval:.1f}, mean at 1000 points {t_dm:.1f}, variances at 64 points {t_dv:.1f}")
        for rank in sizes(a.ranks):
            mf = gp.matrix_free(args={"precond_rank": rank, "tol": 1e-10})
            t_pre, _ = wall_ms(mf._preconditioner)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t_alpha, _ = wall_ms(mf._ensure_alpha)
                t_mm, mm = wall_ms(lambda: mf.posterior_mean(xp)["m(x)"])
                t_mv, mv = wall_ms(lambda: mf.posterior_covariance(xp[:64], variance_only=True)["v(x)"])
            info = mf._alpha_info
            emit(f"    matrix-free rank {rank}: preconditioner {t_pre:.1f} (achieved rank {mf._rank}), alpha solve {t_alpha:.1f} "
                 f"({info['iterations']} iterations, relative residual {info['relative_residual']:.2e}, converged {info['converged']}), mean at "
                 f"1000 points {t_mm:.1f}, variances at 64 points {t_mv:.1f} (4 blocks of 16 solves); against dense: mean max diff "
                 f"{np.max(np.abs(mm - dm)):.2e}, variance max diff {np.max(np.abs(mv - dv)):.2e}; alpha solve / dense evaluation = "
                 f"{t_alpha / t_eval:.1f}")
            del mf
        del gp
        torch.cuda.empty_cache()

    # ---- sizes no dense call holds -------------------------------------------------------------------------------------------------------
    for n in sizes(a.big):
        x, y = data(n)
        V = np.full(n, 0.01)
        xd = H.to_device(x)
        B, Y = H.to_device((y - y.mean()).reshape(n, 1)), H.empty(n, 1)
        t_mv, _ = wall_ms(lambda: H.kmatvec(2, xd, xd, theta, B, Y, s=1))
        t_mv, _ = wall_ms(lambda: H.kmatvec(2, xd, xd, theta, B, Y, s=1))
        emit(f"N = {n}, matern52_ard, noise 0.01: one product (s = 1) {t_mv:.1f} ms = {n * n / t_mv / 1e6:.1f} Gk/s (wall clock, one run)")
        del xd, B, Y
        max_iter = max(8, min(1000, int(a.limit * 1e3 / t_mv) - 4))
        for rank in sizes(a.ranks):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                mf = fvgp_amd.MatrixFreeGP(x, y, theta, noise_variances=V, kernel_function="matern52_ard",
                                           args={"precond_rank": rank, "tol": 1e-10, "max_iter": max_iter})
                t_pre, _ = wall_ms(mf._preconditioner)
                t_alpha, _ = wall_ms(mf._ensure_alpha)
            info = mf._alpha_info
            free, total = torch.cuda.mem_get_info()
            emit(f"    rank {rank}: preconditioner {t_pre / 1e3:.2f} s (achieved rank {mf._rank}), alpha solve {t_alpha / 1e3:.2f} s, "
                 f"{info['iterations']} iterations (limit {max_iter}), relative residual {info['relative_residual']:.2e}, converged "
                 f"{info['converged']}; device memory in use {(total - free) / 2 ** 30:.2f} GiB (allocator caches included)")
            del mf
            torch.cuda.empty_cache()
    H.close()


if __name__ == "__main__":
    main()
