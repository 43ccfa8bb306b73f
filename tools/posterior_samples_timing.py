"""Joint posterior samples on the device (fvgp_hip_posterior -> fvgp_hip_potrf -> fvgp_hip_mvn_sample) against the host route on the same
covariance, in one process on the same data.

    python tools/posterior_samples_timing.py [--sizes 2000,20000] [--points 1000,4000] [--samples 64,1024] [--dim 3] [--windows 5] [--out FILE]

For every N (RBF, theta = [1, 0.3, ..], noise 0.01) and P prediction points the GP is factored once (not timed); then, per number of samples,
    posterior       Handle.posterior with the full covariance S (P x P, stays on the device)
    factorisation   S + (noise + jitter) I -> L by Handle.potrf on a copy (the copy and the diagonal update are part of the figure; the
                    noise 0.01 of the data on the diagonal as posterior_samples(add_noise=True) adds it: the latent covariance of
                    thousands of points under a smooth kernel is not positive definite with a jitter of 1e-9, on either route)
    draw            Handle.mvn_sample: the normals, L Z on the MFMA kernel, the transposing epilogue
    host route      S to the host (Handle.to_host), numpy.linalg.cholesky of the same matrix @ Z with host-generated normals Z
each warmed up first, every timed window bracketed by device synchronisations, the best of `--windows` kept with the spread
(max - min) / min.  The generator's rate: Handle.normal_fill of a 4096 x 4096 block alone between two device events, in GB/s written."""
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


def best(fn, windows):
    fn()
    t = [window(fn) for _ in range(windows)]
    return min(t), (max(t) - min(t)) / min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,20000")
    ap.add_argument("--points", default="1000,4000")
    ap.add_argument("--samples", default="64,1024")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=1e-9)
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
    emit(f"# posterior samples timing: {torch.cuda.get_device_name(0)}, RBF, d = {d}, jitter = {a.jitter:g}; best of {a.windows} synchronised "
         f"windows (spread = (max - min) / min); host route = S to the host + numpy.linalg.cholesky(S + (0.01 + jitter) I) @ Z")
    zf = H.empty(4096, 4096)
    tf = []
    for _ in range(a.windows + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        H.normal_fill(zf, 1, 0)
        e1.record()
        torch.cuda.synchronize()
        tf.append(e0.elapsed_time(e1) * 1e-3)
    emit(f"# normal_fill 4096 x 4096: {min(tf[1:]) * 1e3:.3f} ms = {zf.numel() * 8 / min(tf[1:]) / 1e9:.0f} GB/s written")
    del zf
    emit(f"{'N':>6} {'P':>5} {'samples':>7} | {'posterior ms':>12} {'spread':>6} | {'factor ms':>9} {'spread':>6} | {'draw ms':>8} {'spread':>6} | "
         f"{'device ms':>9} | {'host ms':>9} {'spread':>6} | {'host/device':>11}")
    for n in (int(v) for v in a.sizes.split(",")):
        rng = np.random.default_rng(20240501)
        x = rng.random((n, d))
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
        th = np.array([1.0] + [0.3] * d)
        np_, dim = _lib.pad128(n), _lib.loglik_dim(n, 1)
        xd, vd, yd = H.to_device(x), H.to_device(np.full(n, 0.01)), H.to_device((y - y.mean()).reshape(n, 1))
        KV, alpha = H.empty(dim, dim), H.empty(np_, 1)
        assert H.loglik(0, xd, th, vd, yd, KV, alpha)[3] == 0
        for P in (int(v) for v in a.points.split(",")):
            Pp = _lib.pad128(P)
            xp = H.to_device(rng.random((P, d)))
            kx, mean, S, A = H.empty(np_, Pp), H.empty(P, 1), H.empty(Pp, Pp), H.empty(Pp, Pp)

            def posterior():
                H.posterior(0, xd, th, KV, alpha, 1, xp, kx, mean, None, S)

            def factor():
                A.copy_(S)
                A.diagonal()[:P].add_(a.jitter + 0.01)
                assert H.potrf(A, P) == 0
            t_post, s_post = best(posterior, a.windows)
            t_fac, s_fac = best(factor, a.windows)
            H.invalidate_factor()
            for ns in (int(v) for v in a.samples.split(",")):
                Y = H.empty(ns, P)
                work = H.empty(_lib.mvn_sample_workspace_bytes(P, ns) // 8)
                hrng = np.random.default_rng(1)

                def draw():
                    H.mvn_sample(A, P, Y, mean=mean.view(-1), seed=1, work=work)

                def host():
                    Sh = H.to_host(S[:P, :P])
                    Z = hrng.standard_normal((P, ns))
                    return (np.linalg.cholesky(Sh + (a.jitter + 0.01) * np.eye(P)) @ Z).T
                t_draw, s_draw = best(draw, a.windows)
                t_host, s_host = best(host, max(2, a.windows // 2))
                dev = t_post + t_fac + t_draw
                emit(f"{n:6d} {P:5d} {ns:7d} | {t_post * 1e3:12.3f} {s_post:6.3f} | {t_fac * 1e3:9.3f} {s_fac:6.3f} | {t_draw * 1e3:8.3f} {s_draw:6.3f} | "
                     f"{dev * 1e3:9.3f} | {(t_post + t_host) * 1e3:9.3f} {s_host:6.3f} | {(t_post + t_host) / dev:11.2f}")
                del Y, work
            del kx, S, A
        del KV
    H.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
