"""GP.remove_data by the factor update against update_gp_data(kept, append=False) on the same object, and where an update call's time goes.
   python tools/remove_data_timing.py [--sizes 2000,8000,20000,50000] [--ranks 1,4,16,64] [--runs 3]

Per N and k, removal of the k oldest, the k newest and k random points: median and spread (min .. max) of `runs` wall times of
remove_data (update route forced) and of the refactorisation of the kept points, both from the full state, host work included.
Then, per N, fvgp_hip_chol_update alone at k = 16 on a copy of the factor from row 0 (what removing the oldest costs): the time of a call,
the share of it that is the serial chain of diagonal steps -- N / 128 times the time of one diagonal step, measured as the update of a
128-row problem launched back to back -- and the panel steps' rate against one read and one write of the trailing triangle per pass."""
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fvgp_amd
from fvgp_amd import _lib

warnings.simplefilter("ignore")
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2000,8000,20000,50000")
ap.add_argument("--ranks", default="1,4,16,64")
ap.add_argument("--runs", type=int, default=3)
a = ap.parse_args()
sizes = [int(s) for s in a.sizes.split(",")]
ranks = [int(s) for s in a.ranks.split(",")]
th = np.array([1.0, 0.3, 0.3, 0.3])


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def stats(ts):
    return f"{np.median(ts):9.2f} ({min(ts):.2f} .. {max(ts):.2f})"


print(f"remove_data: update route vs refactorisation of the kept points, ms, median (min .. max) of {a.runs} runs")
print(f"{'N':>6} {'k':>3} {'which':>7} | {'update':>28} | {'refactor':>28} | ratio")
for n in sizes:
    rng = np.random.default_rng(n)
    x = rng.random((n, 3))
    y = np.sin(3 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    nv = np.full(n, 0.01)
    gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard", args={"remove_update_max_fraction": 1.0, "remove_update_cost_model": False})
    for k in ranks:
        for which in ("oldest", "newest", "random"):
            idx = {"oldest": np.arange(k), "newest": np.arange(n - k, n), "random": np.sort(rng.choice(n, k, replace=False))}[which]
            keep = np.setdiff1d(np.arange(n), idx)
            tu, tr = [], []
            for _ in range(a.runs + 1):                      # (the first run warms the allocator and is dropped)
                res = {}
                tu.append(timed(lambda: res.update(gp.remove_data(idx))))
                assert res["route"] == "update" and gp.point_number == n - k
                ll = gp.log_likelihood()
                gp.update_gp_data(x, y, nv, append=False)
                tr.append(timed(lambda: gp.update_gp_data(x[keep], y[keep], nv[keep], append=False)))
                assert abs(gp.log_likelihood() - ll) <= 1e-8 * abs(ll), (gp.log_likelihood(), ll)
                gp.update_gp_data(x, y, nv, append=False)
            tu, tr = tu[1:], tr[1:]
            print(f"{n:>6} {k:>3} {which:>7} | {stats(tu):>28} | {stats(tr):>28} | {np.median(tr) / np.median(tu):5.2f}x", flush=True)
    # the update kernel alone
    H = gp._H
    H.sync()
    k = 16
    Lc = gp._L[:gp._np, :gp._np].clone()
    W0 = H.to_device(0.01 * rng.standard_normal((n, k)))
    work = H.empty(_lib.CHOL_UPDATE_TABLE_BYTES // 8)
    ts = []
    for _ in range(a.runs + 1):
        W = W0.clone()
        ts.append(timed(lambda: H.chol_update(Lc, n, W, row0=0, work=work)))
    ts = ts[1:]
    D = Lc[:128, :128].clone()
    Wd = W0[:128].clone()
    reps = 200
    H.chol_update(D, 128, Wd, work=work)
    t_diag = timed(lambda: [H.chol_update(D, 128, Wd, work=work) for _ in range(reps)]) / reps
    nb = (n + 127) // 128
    chain = nb * t_diag
    rows_below = sum(max(0, n - 128 * (j + 1)) for j in range(nb))
    gbytes = 2 * 8 * 128 * rows_below / 1e9
    t = float(np.median(ts))
    print(f"{n:>6} chol_update k=16 from row 0: {stats(ts)} ms; one diagonal step {1e3 * t_diag:.1f} us, chain of {nb}: {chain:.2f} ms = "
          f"{100 * chain / t:.0f} % of the call; trailing triangle {gbytes:.2f} GB read + written: {gbytes / (t / 1e3):.0f} GB/s over the whole "
          f"call, {gbytes / (max(t - chain, 1e-6) / 1e3):.0f} GB/s over the call less the chain", flush=True)
    del gp, Lc, W0
    torch.cuda.empty_cache()
