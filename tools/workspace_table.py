#!/usr/bin/env python3
"""Record what every workspace size query of the C ABI returns over a grid that crosses every branch of the size arithmetic: per
query one line of tests/golden/workspace_bytes.json with the values of each argument and the results at their product.
tests/test_workspace_host.py holds the built library to the table, so a change of the host code that moves a size shows there.

    python tools/workspace_table.py [--rev REV] [--lib PATH] [--out PATH]

Without --lib the sources of REV (default HEAD) are exported into a temporary directory and built there (hipcc cross-compiles without
a GPU; the queries are host code and run on the CPU), so the table is that commit's and not the working tree's."""
import argparse
import ctypes
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

N = (1, 127, 128, 129, 257, 4095, 20000, 10 ** 6)      # both sides of a tile, of the batched limit (4096) and of the chunk (4096)
N0 = N + (0,)
# the solver queries park the split product's sums while mv_auto_split(n, n) > 1: two chunks at least (n > 4096) and fewer than 512
# blocks of 64 rows (n <= 32704)
N_SOLVER = N0 + (4096, 4097, 32704, 32705)
B3 = (1, 3, 64, 0)
D = (1, 4, 5, 16, 0, 17)


def axes():
    """symbol -> the values of each argument; a query is asked at their product, in itertools.product's order"""
    a = {}
    a["fvgp_hip_workspace_bytes"] = (N0, (0, 1, 129, -1))
    for s in ("fvgp_hip_loglik_batch_workspace_bytes", "fvgp_hip_loglik_grad_batch_workspace_bytes"):
        a[s] = (N0 + (4088, 4096), (1, 2, 8, 0), B3)
    a["fvgp_hip_posterior_batch_workspace_bytes"] = (N0 + (4088, 4096), (1, 8), B3, (128, 384, 100))
    a["fvgp_hip_loglik_hess_workspace_bytes"] = (N0, D)
    a["fvgp_hip_posterior_grad_workspace_bytes"] = (N0, (1, 65, 128, 0), (1, 3, 16, 17, 0))
    a["fvgp_hip_loo_workspace_bytes"] = (N0,)
    a["fvgp_hip_mvn_sample_workspace_bytes"] = (N0, (1, 3, 64, 129, 0))
    a["fvgp_hip_select_workspace_bytes"] = (N0, (1, 65, 4096, 4097, 0), (1, 5, 8, 0))
    a["fvgp_hip_kmatvec_workspace_bytes"] = (N0, (1, 4097, 20000, 0), (1, 3, 5, 16, 17, 0))
    for s in ("fvgp_hip_pchol_workspace_bytes", "fvgp_hip_precond_workspace_bytes"):
        a[s] = (N0 + (8192, 8193), (1, 5, 8, 64, 0))
    for s in ("fvgp_hip_pcg_workspace_bytes", "fvgp_hip_precond_apply_workspace_bytes"):
        a[s] = (N_SOLVER, (0, 1, 5, 8, -1))
    a["fvgp_hip_pcg_lanczos_workspace_bytes"] = (N_SOLVER, (0, 1, 8, -1), (0, 1, 30, -1))
    a["fvgp_hip_kgrad_form_workspace_bytes"] = (N_SOLVER, (1, 4097, 20000, 0))
    a["fvgp_hip_chol_update_workspace_bytes"] = (N0, (1, 2, 3, 128, 0))
    a["fvgp_hip_nn_workspace_bytes"] = ((0, 1, 2, 3, -1), N0, B3)
    for s in ("fvgp_hip_nn_grad_workspace_bytes", "fvgp_hip_nn_fisher_workspace_bytes"):
        a[s] = (N0, B3, (1, 2, 5, 0))
    for s in ("fvgp_hip_nn_grid_bytes", "fvgp_hip_nn_grid_workspace_bytes"):
        a[s] = (N0 + (2 ** 31 - 1, 2 ** 31), (1, 2, 3, 0, 4))
    for s in ("fvgp_hip_nn_factor_workspace_bytes", "fvgp_hip_nn_maxmin_workspace_bytes"):
        a[s] = (N0,)
    for s in ("fvgp_hip_nn_precond_apply_workspace_bytes", "fvgp_hip_pcg_nn_workspace_bytes"):
        a[s] = (N_SOLVER,)
    return a


def results(L, symbol, ax):
    """what the bound library `L` returns for `symbol` at every point of the product of the axes `ax`"""
    return [int(getattr(L, symbol)(*args)) for args in itertools.product(*ax)]


def table(L):
    """one record per query: {"symbol", "axes", "results"}"""
    return [{"symbol": s, "axes": [list(v) for v in ax], "results": results(L, s, ax)} for s, ax in sorted(axes().items())]


def load(path):
    sys.path.insert(0, ROOT)
    from fvgp_amd import _lib
    return _lib.bind(ctypes.CDLL(path))


def build_rev(rev, tmp):
    """export `rev` into `tmp`, build its library there and return the library's path"""
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    subprocess.run(["make", "-C", os.path.join(tmp, "fvgp_amd", "csrc"), "-j16"], check=True, capture_output=True)
    return os.path.join(tmp, "fvgp_amd", "csrc", "libfvgp_hip.so")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", default="HEAD", help="the commit whose sources are built (default HEAD)")
    ap.add_argument("--lib", help="a built libfvgp_hip.so to ask instead of building --rev")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.lib:
        rows = table(load(a.lib))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            rows = table(load(build_rev(a.rev, tmp)))
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{sum(len(r['results']) for r in rows)} results of {len(rows)} queries -> {a.out}")


if __name__ == "__main__":
    main()
