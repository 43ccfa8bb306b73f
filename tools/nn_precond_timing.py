"""The nearest-neighbour preconditioner of the matrix-free solves against the pivoted Cholesky, one run on the device:

    python tools/nn_precond_timing.py [--sizes 20000,200000,500000] [--ranks 128,256] [--neighbors 16,32] [--orderings random,maxmin]
                                      [--limit 60] [--windows 3] [--apply-only] [--out FILE]

At each N of --sizes (Matern-5/2, d = 3, noise 0.01, the data of tools/matrix_free_timing.py) and tol = 1e-10:
    pchol     per rank: the build (fvgp_hip_pchol + fvgp_hip_precond_factor), then alpha: iterations, seconds, residual, converged
    vecchia   per (m, ordering): the construction split into ordering, neighbour search, host transpose (download, stable sort, upload)
              and factor (fvgp_hip_nn_factor), then alpha: iterations, seconds, residual, converged
    apply     fvgp_hip_nn_precond_apply at s = 16 (two copies, gather, transpose; device events, best of --windows) with the bytes the
              gather and the transpose move at least -- lists, coefficients and one read of each operand row per entry: n (m (12 + 128) +
              384) and n 384 + nnz (16 + 128) -- and the call's GB/s over their sum.  The two kernels' own times are in a kernel trace of
              `--apply-only` (rocprofv3 --kernel-trace --stats -- python tools/nn_precond_timing.py --apply-only ...)
A solve's iteration limit is sized from the measured time per product so that it ends within --limit seconds: "converged" False with the
residual reached says that it did not.  One run each; wall clock where the host takes part."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOL = 1e-10


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


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


def data(n, d=3, seed=20240501):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    return x, np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,200000,500000")
    ap.add_argument("--ranks", default="128,256")
    ap.add_argument("--neighbors", default="16,32")
    ap.add_argument("--orderings", default="random,maxmin")
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--apply-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fvgp_amd
    from fvgp_amd import _lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    theta = np.array([1.0, 0.15, 0.15, 0.15])
    H = _lib.Handle(0)
    kid = _lib.KERNEL_IDS["matern52_ard"]
    say(f"# nn_precond_timing: matern52_ard d=3 theta={theta.tolist()} noise=0.01 tol={TOL:g} limit={a.limit:g}s")
    for n in map(int, a.sizes.split(",")):
        x, y = data(n)
        V = np.full(n, 0.01)
        xd, B, X = H.to_device(x), H.to_device(np.ones((n, 1))), H.empty(n, 1)
        t_mv = event_ms(lambda: H.kmatvec(kid, xd, xd, theta, B, X, s=1), 1)[0] * 1e-3
        iters = max(8, int(a.limit / t_mv))
        say(f"N={n}: product {t_mv * 1e3:.1f} ms, iteration limit {iters}")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if not a.apply_only:
                for q in map(int, a.ranks.split(",")):
                    gp = fvgp_amd.MatrixFreeGP(x, y, theta, noise_variances=V, kernel_function="matern52_ard",
                                               args={"precond_rank": q, "tol": TOL, "max_iter": iters, "max_restarts": 0})
                    tb, _ = wall(gp._preconditioner)
                    ts, _ = wall(gp._ensure_alpha)
                    i = gp._alpha_info
                    say(f"  pchol rank {q}: build {tb:.2f} s | alpha {i['iterations']} iterations {ts:.2f} s residual "
                        f"{i['relative_residual']:.1e} converged {i['converged']}")
                    del gp
            for ordering in a.orderings.split(","):
                for m in map(int, a.neighbors.split(",")):
                    gp = None
                    t_order, perm = wall(lambda: fvgp_amd.VecchiaGP._maxmin(_Shell(H, theta), x)[0] if ordering == "maxmin"
                                         else np.random.default_rng(0).permutation(n))
                    t_all, gp = wall(lambda: fvgp_amd.MatrixFreeGP(
                        x, y, theta, noise_variances=V, kernel_function="matern52_ard",
                        args={"preconditioner": "vecchia", "precond_neighbors": m, "precond_ordering": perm, "tol": TOL, "max_iter": iters,
                              "max_restarts": 0}))
                    t_tr, _ = wall(lambda: H.nn_transpose(gp._idx, m))
                    t_f, W = wall(gp.preconditioner_factor)
                    t_search = t_all - t_tr
                    R, Z = H.to_device(np.random.default_rng(1).standard_normal((n, 16))), H.empty(n, 16)
                    work = H.empty(_lib.nn_precond_apply_workspace_bytes(n) // 8)
                    ms, spread = event_ms(lambda: H.nn_precond_apply(W, R, Z, s=16, work=work), a.windows)
                    gb_g, gb_t = n * (m * (12 + 128) + 384) / 1e9, (n * 384 + W.nnz * (16 + 128)) / 1e9
                    say(f"  vecchia m={m} {ordering}: ordering {t_order:.2f} s, upload + search {t_search:.2f} s, host transpose {t_tr:.2f} s, "
                        f"factor {t_f * 1e3:.1f} ms | apply s=16 {ms:.3f} ms (spread {spread:.1%}): gather {gb_g:.3f} GB + transpose "
                        f"{gb_t:.3f} GB = {(gb_g + gb_t) / (ms * 1e-3):.0f} GB/s over the call, largest bucket "
                        f"{int(np.diff(W.tr_start.cpu().numpy()).max())}")
                    if not a.apply_only:
                        ts, _ = wall(gp._ensure_alpha)
                        i = gp._alpha_info
                        say(f"    alpha {i['iterations']} iterations {ts:.2f} s residual {i['relative_residual']:.1e} converged {i['converged']}")
                    del gp, W
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


class _Shell:
    """what VecchiaGP._maxmin reads of its object, so that the ordering can be timed apart from the search"""

    def __init__(self, H, theta):
        self._H, self._scales, self.args, self._ordering_rule = H, np.asarray(theta[1:], dtype=np.float64), {}, ("maxmin", 0)


if __name__ == "__main__":
    main()
