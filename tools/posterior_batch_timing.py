"""Batched posterior (mean + variance, and with the full covariance) against sequential single evaluations, in one process, on the same
thetas and prediction points.

    python tools/posterior_batch_timing.py [--sizes 500:1,2000:3,4000:3] [--batch 64] [--points 1000] [--windows 5] [--batch-only] [--out FILE]
    python tools/posterior_batch_timing.py --kernel-stats STATS.csv --calls K --sizes 2000:3 [--out FILE.csv]

For every size (N, d): B thetas log-uniform within x/ 2 of [1, 0.3, ..], P uniform prediction points; every shape warmed up first; the
two sides alternate, each timed window is bracketed by device synchronisations, the best of `--windows` is kept and the spread
(max - min) / min over the windows is reported.  Two ways to the same numbers:
  batch      : ONE Handle.posterior_batch call (fvgp_hip_posterior_batch), variance only / with S
  sequential : B x (Handle.loglik + Handle.posterior) (the single fused evaluation and the single posterior)
Reported: ms, predictions (theta x point) per second, the speed-up, and the largest relative difference of mean and variance between the
two.  The second form turns the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--batch-only` (K batched calls) into the
per-kernel table kept under profiles/, with the epilogue kernel's HBM rate (it reads B * P * N doubles once)."""
import argparse
import csv
import os
import sys
import time

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


def kernel_stats(path, calls, n, B, P, out):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            g = {k.lower(): v for k, v in r.items()}
            rows.append((g["name"], int(g["calls"]), int(float(g["totaldurationns"])), int(float(g["averagens"])), int(float(g["minns"])),
                         int(float(g["maxns"])), float(g["percentage"])))
    rows.sort(key=lambda r: -r[2])
    lines = [f"# rocprofv3 --kernel-trace --stats of tools/posterior_batch_timing.py --batch-only (N={n}, B={B}, P={P}; {calls} batched calls each of "
             f"variance only and with S)", "kernel,calls,total_ns,avg_ns,min_ns,max_ns,percent,ms_per_batched_call"]
    for name, c, tot, avg, mn, mx, pct in rows:
        short = name.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0]
        lines.append(f"\"{short}\",{c},{tot},{avg},{mn},{mx},{pct:.2f},{tot / 1e6 / (2 * calls):.3f}")
        if "post_epilogue_batch_kernel" in name:
            gbs = B * P * n * 8 / (mn * 1e-9) / 1e9
            lines.append(f"# post_epilogue_batch_kernel: {B * P * n * 8 / 1e9:.3f} GB read per launch, best {mn / 1e3:.1f} us = {gbs:.0f} GB/s "
                         f"({100 * gbs / HBM_GBS:.0f} % of {HBM_GBS:.0f} GB/s HBM)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500:1,2000:3,4000:3")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true", help="time the batched calls only (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv to summarise instead of timing")
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, P = a.batch, a.points
    if a.kernel_stats:
        n = int(a.sizes.split(",")[0].split(":")[0])
        return kernel_stats(a.kernel_stats, a.calls, n, B, P, a.out)
    import torch
    from fvgp_amd import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# posterior_batch timing: {torch.cuda.get_device_name(0)}, B = {B} thetas x P = {P} points, best of {a.windows} synchronised windows "
         f"(spread = (max - min) / min over them), the two sides alternating")
    emit(f"{'N':>5} {'d':>2} {'mode':>8} | {'batch ms':>9} {'spread':>6} {'pred/s':>10} | {'seq ms':>9} {'spread':>6} {'pred/s':>10} | {'x seq':>6} | "
         f"max rel diff mean / var")
    H = _lib.Handle(0)
    Pp = _lib.pad128(P)
    for spec in a.sizes.split(","):
        n, d = (int(v) for v in spec.split(":"))
        x, y = synth(n, d)
        ym = (y - y.mean()).reshape(n, 1)
        xp = np.random.default_rng(n).random((P, d))
        xd, Vd, ymd, xpd = H.to_device(x), H.to_device(np.full(n, 0.01)), H.to_device(ym), H.to_device(xp)
        dim, dim1, npd = _lib.loglik_batch_dim(n, 1), _lib.loglik_dim(n, 1), _lib.pad128(n)
        rng = np.random.default_rng(B * 1000 + n)
        th = np.array([1.0] + [0.3] * d)[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, d + 1)))
        KVb, mean, var, Sb = H.empty(B, dim + Pp, dim), H.empty(B, P, 1), H.empty(B, P), H.empty(B, Pp, Pp)
        KV1, alpha, kx, m1, v1, S1 = H.empty(dim1, dim1), H.empty(npd, 1), H.empty(npd, Pp), H.empty(P, 1), H.empty(P), H.empty(Pp, Pp)
        for with_S in (False, True):
            res = {}

            def batch():
                H.posterior_batch(0, xd, th, Vd, ymd, xpd, KVb, mean, var, Sb if with_S else None)

            def seq():
                ms, vs = [], []
                for t in th:
                    H.loglik(0, xd, t, Vd, ymd, KV1, alpha)
                    H.posterior(0, xd, t, KV1, alpha, 1, xpd, kx, m1, v1, S1 if with_S else None)
                    if "m" not in res:
                        ms.append(m1.cpu().numpy().copy()); vs.append(v1.cpu().numpy().copy())
                H.sync()
                if ms:
                    res["m"], res["v"] = np.stack(ms), np.stack(vs)
            mode = "with S" if with_S else "var only"
            batch()
            if a.batch_only:
                tb = [window(batch) for _ in range(a.windows)]
                emit(f"{n:5d} {d:2d} {mode:>8} | {min(tb) * 1e3:9.3f} {(max(tb) - min(tb)) / min(tb):6.3f} {B * P / min(tb):10.3e} |")
                continue
            seq()
            tb, ts = [], []
            for _ in range(a.windows):
                tb.append(window(batch)); ts.append(window(seq))
            dm = float(np.max(np.abs(mean.cpu().numpy() - res["m"]) / np.max(np.abs(res["m"]), axis=(1, 2), keepdims=True)))
            dv = float(np.max(np.abs(var.cpu().numpy() - res["v"]) / th[:, :1]))
            emit(f"{n:5d} {d:2d} {mode:>8} | {min(tb) * 1e3:9.3f} {(max(tb) - min(tb)) / min(tb):6.3f} {B * P / min(tb):10.3e} | "
                 f"{min(ts) * 1e3:9.3f} {(max(ts) - min(ts)) / min(ts):6.3f} {B * P / min(ts):10.3e} | {min(ts) / min(tb):6.2f} | {dm:.2e} / {dv:.2e}")
        del KVb, Sb
    H.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
