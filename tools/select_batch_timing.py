"""Greedy batch selection on the device (fvgp_hip_posterior variances -> fvgp_hip_select_batch) and, at P = 1000, the host route on the same
state (posterior covariance S to the host, pivoted Cholesky in numpy), in one process on the same data.

    python tools/select_batch_timing.py [--sizes 2000,20000] [--points 1000,100000] [--picks 16,64] [--dim 3] [--windows 5] [--out FILE]

For every N (RBF, theta = [1, 0.3, ..], data noise 0.01, candidate noise 0.05, criterion "variance") the GP is factored once (not
timed); then per P and q, each between two device events on the handle's stream, warmed up first, best of `--windows` with the spread
(max - min) / min:
    variances   the initial variances: fvgp_hip_posterior(var_out, S_out = NULL) over the candidates in chunks of 4096
    call        one fvgp_hip_select_batch (q steps, one enqueue)
    sweeps      what a step spends outside the candidates: q times the column k(X, x_j) (Handle.kmat into a row of n entries) and its
                one-right-hand-side solve (Handle.potrs), enqueued back to back through the public entries; per step
    cross       per step, by difference: (call - q sweeps) / q -- the cross pass with the pick and the downdate
    Gk/s        kernel evaluations per second of the cross pass: N P / `cross`
    host        (P <= --host-max only) Handle.posterior with S, S to the host, q steps of pivoted Cholesky on it in numpy
The variances are restored before every window of `call`."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, windows, before=None):
    import torch
    t = []
    for i in range(windows + 1):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            t.append(e0.elapsed_time(e1))
    return min(t), (max(t) - min(t)) / min(t)


def host_pivoted_cholesky(S, noise, q):
    d = np.maximum(np.diag(S).copy(), 0.0)
    G = np.zeros((q, len(d)))
    taken = np.zeros(len(d), dtype=bool)
    idx = []
    for t in range(q):
        j = int(np.argmax(np.where(taken, -np.inf, d)))
        c = (S[:, j] - G[:t].T @ G[:t, j]) / np.sqrt(d[j] + noise)
        G[t] = c
        d = np.maximum(d - c * c, 0.0)
        taken[j] = True
        idx.append(j)
    return np.array(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,20000")
    ap.add_argument("--points", default="1000,100000")
    ap.add_argument("--picks", default="16,64")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fvgp_amd import _lib
    H = _lib.Handle(0)
    d, CH = a.dim, 4096
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# select_batch timing: {torch.cuda.get_device_name(0)}, RBF, d = {d}, criterion variance, candidate noise 0.05; device events, "
         f"best of {a.windows} (spread = (max - min) / min); host = posterior with S + transfer + numpy pivoted Cholesky (wall clock); "
         f"cross = (call - q sweeps) / q, a difference of two minima (no spread of its own) that includes the pick, the downdate and launch gaps: "
         f"Gk/s is a rate of the cross kernel at P = 100000 only")
    emit(f"{'N':>6} {'P':>7} {'q':>3} | {'variances ms':>12} {'spread':>6} | {'call ms':>9} {'spread':>6} | {'sweeps ms/step':>14} {'spread':>6} | "
         f"{'cross ms/step':>13} {'spread':>6} | {'Gk/s':>7} | {'host ms':>9} {'spread':>6} | {'same picks':>10}")
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
            xc = H.to_device(rng.random((P, d)))
            noise = H.to_device(np.full(P, 0.05))
            var0, var = H.empty(P), H.empty(P)
            kx = H.empty(np_, _lib.pad128(min(P, CH)))

            def variances():
                for c0 in range(0, P, CH):
                    c1 = min(c0 + CH, P)
                    Pp = _lib.pad128(c1 - c0)
                    H.posterior(0, xd, th, KV, alpha, 1, xc[c0:c1], kx.view(-1)[:np_ * Pp].view(np_, Pp), var_out=var0[c0:c1])
            t_var, s_var = event_ms(variances, a.windows)
            for q in (int(v) for v in a.picks.split(",")):
                idx = torch.empty(q, dtype=torch.int64, device=var.device)
                pick = H.empty(q)
                work = H.empty(_lib.select_workspace_bytes(n, P, q) // 8)

                def call():
                    H.select_batch(0, xd, th, KV, xc, var, q, idx, pick, noise=noise, work=work)

                def restore():
                    var.copy_(var0)
                col = H.empty(np_, 1)

                def sweeps():
                    for _ in range(q):
                        H.kmat(0, xc[:1], xd, th, col.view(1, np_))
                        H.potrs(KV, n, col, 1)
                res = {"call": event_ms(call, a.windows, before=restore), "sweeps": event_ms(sweeps, a.windows)}
                t_cross = max(res["call"][0] - res["sweeps"][0], 1e-6) / q
                restore()
                call()
                H.sync()
                picks = idx.cpu().numpy()
                host_txt, same = f"{'-':>9} {'-':>6}", "-"
                if P <= a.host_max:
                    Pp = _lib.pad128(P)
                    S, k2 = H.empty(Pp, Pp), H.empty(np_, Pp)
                    got = {}

                    def host():
                        H.posterior(0, xd, th, KV, alpha, 1, xc, k2, None, None, S)
                        got["idx"] = host_pivoted_cholesky(H.to_host(S[:P, :P]), 0.05, q)
                    tw = []
                    host()
                    for _ in range(max(2, a.windows // 2)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        host()
                        tw.append((time.perf_counter() - t0) * 1e3)
                    host_txt = f"{min(tw):9.3f} {(max(tw) - min(tw)) / min(tw):6.3f}"
                    same = str(bool(np.array_equal(got["idx"], picks)))
                    del S, k2
                gk = n * P / (t_cross * 1e-3) / 1e9
                emit(f"{n:6d} {P:7d} {q:3d} | {t_var:12.3f} {s_var:6.3f} | {res['call'][0]:9.3f} {res['call'][1]:6.3f} | "
                     f"{res['sweeps'][0] / q:14.4f} {res['sweeps'][1]:6.3f} | {t_cross:13.4f} {'-':>6} | {gk:7.1f} | "
                     f"{host_txt} | {same:>10}")
                del work
            del kx, var0, var
        del KV
    H.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
