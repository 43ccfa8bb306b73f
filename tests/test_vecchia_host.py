"""CPU-only checks of the nearest-neighbour (Vecchia) path: the library exports what include/fvgp_hip_nn.h declares and the binding
table agrees with it; the numpy twin (vecchia_ref) against the exact GP in longdouble; the float64 twin's own error, which sets the
device tests' bars; the search twin's properties.  Run with -s for the record lines."""
import ctypes
import os
import re

import numpy as np
import pytest

import kernel_family_ref as kf
import test_host_logic as thl
import vecchia_ref as vr
from conftest import ROOT

LD = vr.LD


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_nn_header_is_exported_and_bound():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = _header("fvgp_hip_nn.h")
    declared = sorted(set(re.findall(r"\b(fvgp_hip_\w+)\s*\(", hdr)))
    assert declared and sorted(_lib.SYMBOLS_NN) == declared
    for s in declared:
        assert hasattr(L, s), f"libfvgp_hip.so does not export {s}"
    protos, structs = thl._parse_header(hdr)
    assert structs == {} and list(protos) == list(_lib._ABI_NN) == _lib.SYMBOLS_NN, "the table is written in the header's order"
    assert thl._abi_differences(protos, _lib._ABI_NN, _lib) == []
    # the comparison can fail: the int64_t causal offset declared as int, a table that lacks an entry
    mutant = {k: (r, list(a)) for k, (r, a) in _lib._ABI_NN.items()}
    args = mutant["fvgp_hip_nn_search"][1]
    assert len(args) == 11 and args[8] is ctypes.c_int64
    args[8] = ctypes.c_int
    del mutant["fvgp_hip_nn_loglik"]
    assert thl._abi_differences(protos, mutant, _lib) == [("fvgp_hip_nn_search", 8), ("fvgp_hip_nn_loglik", "missing")]
    for name, (restype, argtypes) in _lib._ABI_NN.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the first header and its table are what they were
    first, _ = thl._parse_header(_header("fvgp_hip.h"))
    assert len(first) == 100 and list(first) == _lib.SYMBOLS and not set(first) & set(protos)
    assert int(re.search(r"#define FVGP_NN_MAX_NEIGHBORS (\d+)", hdr).group(1)) == _lib.NN_MAX_NEIGHBORS == 64
    # host-side argument rules run without a device
    wb = L.fvgp_hip_nn_workspace_bytes
    assert wb(_lib.NN_SEARCH, 5, 1) == 0 and wb(3, 5, 1) == -1 and wb(_lib.NN_LOGLIK, 0, 1) == -1 and wb(_lib.NN_LOGLIK, 5, 0) == -1
    assert 0 < wb(_lib.NN_CONDITIONALS, 1000, 3) < wb(_lib.NN_LOGLIK, 1000, 3) and wb(_lib.NN_LOGLIK, 1000, 3) % 8 == 0
    assert L.fvgp_hip_nn_search(None, None, 1, None, 1, 1, None, 1, 0, None, 1) == -1


# ---- 2. the longdouble twin is the exact GP where the approximation is exact --------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kf.FAMILY))
@pytest.mark.parametrize("n", [1, 2, 33, 97])
def test_twin_with_all_earlier_points_is_the_exact_likelihood(name, n):
    d = 3
    x, theta, r, v = vr.case_data(name, d, n, seed=1)
    idx = vr.search_ref(x, x, max(n - 1, 1), vr.length_scales(name, theta, d), c0=0)
    assert all(sorted(j for j in idx[i] if j >= 0) == list(range(i)) for i in range(n))
    ll = vr.loglik_ref(name, x, theta, idx, r, v, LD)[0]
    exact = vr.dense_loglik_ld(name, x, theta, r, v)
    err = float(abs(ll - exact) / abs(exact))
    print(f"\nvecchia twin vs dense longdouble {name} n={n}: rel {err:.2e} (bar {1e-15 * n:.1e})")
    assert err <= 1e-15 * n


# ---- 3. the float64 twin's error: the bases of the device bars ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.ACC_CASES + (vr.EXACT_CASE,), ids=vr.case_id)
def test_float64_twin_error_is_recorded_and_small(case):
    b = vr.bases(case)
    print(f"\nvecchia base {vr.case_id(case)}: " + " ".join(f"{k}={b[k]:.2e}" for k in vr.FIGURES))
    # well-conditioned cases (noise 1e-2 sigma^2): a double-precision evaluation loses a few digits of sixteen, no more.  (The
    # likelihood's own figure is relative to a sum that can cancel; its parts cannot.)
    assert all(np.isfinite(b[k]) for k in vr.FIGURES)
    assert max(b["mu"], b["d"], b["fit"], b["logdet"]) < 1e-11


def test_floor_is_the_median_of_the_bases():
    med = {k: float(np.median([vr.bases(c)[k] for c in vr.ACC_CASES])) for k in vr.FIGURES}
    print("\nvecchia floor: " + " ".join(f"{k}={med[k]:.3e}" for k in vr.FIGURES))
    for k in vr.FIGURES:
        assert abs(med[k] / vr.FLOOR[k] - 1.0) < 0.01, (k, med[k], vr.FLOOR[k])
    # the cases cover what the device has code paths for
    assert {c[0] for c in vr.ACC_CASES} == set(kf.FAMILY) and {c[1] for c in vr.ACC_CASES} == set(kf.DIMS)
    assert {c[3] for c in vr.ACC_CASES} == {1, 15, 16, 17, 31, 32, 33, 63, 64}
    assert {c[2] for c in vr.ACC_CASES} == {1, 2, 70, 200} and {c[4] for c in vr.ACC_CASES} == {1, 3}
    assert vr.MARGIN == __import__("chol_update_ref").MARGIN


# ---- 4. the search twin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c0", [-1, 0, 40])
def test_search_twin_properties(c0):
    rng = np.random.default_rng(5 + c0)
    xr = rng.random((65, 3))
    xq = xr if c0 == 0 else rng.random((30, 3))
    for m, scales in ((1, None), (17, np.array([0.5, 2.0, 1.25])), (64, None)):
        vr.check_search_rows(vr.search_ref(xq, xr, m, scales, c0), xq, xr, m, scales, c0)


def test_search_twin_breaks_ties_by_index():
    # duplicated points: every copy of a point is at distance 0 from the others, the lower index first
    base = np.random.default_rng(9).integers(0, 4, (7, 2)).astype(np.float64)
    x = np.vstack([base, base, base[:3]])
    idx = vr.search_ref(x, x, 5, None, c0=-1)
    vr.check_search_rows(idx, x, x, 5, None, -1)
    for i in range(len(x)):
        same = [j for j in range(len(x)) if np.array_equal(x[j], x[i])]
        assert list(idx[i, :len(same)][:5]) == same[:5]
    # a regular grid: distances are small integers and many tie; causal lists hold the earlier points only
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), axis=-1).reshape(-1, 2)
    idx = vr.search_ref(g, g, 8, np.array([1.0, 2.0]), c0=0)
    vr.check_search_rows(idx, g, g, 8, np.array([1.0, 2.0]), 0)
    assert np.all(idx[0] == -1) and list(idx[1]) == [0] + [-1] * 7
    D = vr.distances(g, g, np.array([1.0, 2.0]))
    assert np.all(D == np.round(D * 4) / 4), "exactly representable distances"
    i = 17
    ties = [j for j in idx[i] if j >= 0 and D[i, j] == D[i, idx[i, 0]]]
    assert ties == sorted(ties)
