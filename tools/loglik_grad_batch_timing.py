"""Batched log-likelihood value + gradient against sequential evaluations, in one process, on the same thetas.

    python tools/loglik_grad_batch_timing.py [--sizes 500:1,2000:3,4000:3] [--batches 64] [--windows 5] [--batch-only] [--out FILE]

For every size (N, d) and batch size B: B thetas log-uniform within x/ 2 of [1, 0.3, ..]; every shape warmed up first; each timed
window is bracketed by device synchronisations and the best of `--windows` is kept.  Two ways to get the B values and gradients:
  batch  : ONE Handle.loglik_grad_batch call (fvgp_hip_loglik_grad_batch)
  handle : B sequential Handle.loglik + Handle.loglik_grad calls (the single fused evaluation, POTRI and the trace)
Reported: value+gradient evaluations per second, the speed-up of the batch over the sequential calls, and the largest relative
difference of the batched gradients from the sequential ones."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(n, d, seed=20240501):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    return x, np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)


def best(fn, windows):
    import torch
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500:1,2000:3,4000:3")
    ap.add_argument("--batches", default="64")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true", help="time the batched call only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fvgp_amd import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# loglik_grad_batch timing: {torch.cuda.get_device_name(0)}, best of {a.windows} synchronised windows")
    emit(f"{'N':>5} {'d':>2} {'B':>3} | {'batch ms':>9} {'eval/s':>9} | {'handle ms':>9} {'eval/s':>9} | {'x handle':>8} | max rel grad diff")
    H = _lib.Handle(0)
    for spec in a.sizes.split(","):
        n, d = (int(v) for v in spec.split(":"))
        x, y = synth(n, d)
        V = np.full(n, 0.01)
        ym = (y - y.mean()).reshape(n, 1)
        xd, Vd, ymd = H.to_device(x), H.to_device(V), H.to_device(ym)
        dim, npd = _lib.loglik_batch_dim(n, 1), _lib.pad128(n)
        KV1, W1, alpha = H.empty(_lib.loglik_dim(n, 1), _lib.loglik_dim(n, 1)), H.empty(npd, npd), H.empty(npd, 1)
        for B in (int(v) for v in a.batches.split(",")):
            rng = np.random.default_rng(B * 1000 + n)
            th = np.array([1.0] + [0.3] * d)[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, d + 1)))
            KV, W = H.empty(B, dim, dim), H.empty(B, npd, npd)
            res = {}

            def batch():
                res["b"] = H.loglik_grad_batch(0, xd, th, Vd, ymd, KV, W)[1]

            def handle():
                g = []
                for t in th:
                    H.loglik(0, xd, t, Vd, ymd, KV1, alpha)
                    g.append(H.loglik_grad(0, xd, t, alpha, 1, 0, KV1, W1))
                res["h"] = np.array(g)
            batch()
            tb = best(batch, a.windows)
            if a.batch_only:
                emit(f"{n:5d} {d:2d} {B:3d} | {tb * 1e3:9.3f} {B / tb:9.0f} |")
                continue
            handle()
            th_ = best(handle, a.windows)
            diff = float(np.max(np.abs(res["b"] - res["h"]) / np.max(np.abs(res["h"]), axis=1, keepdims=True)))
            emit(f"{n:5d} {d:2d} {B:3d} | {tb * 1e3:9.3f} {B / tb:9.0f} | {th_ * 1e3:9.3f} {B / th_:9.0f} | {th_ / tb:8.2f} | {diff:.2e}")
            del KV, W
    H.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
