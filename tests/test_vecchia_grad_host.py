"""CPU-only checks of the nearest-neighbour likelihood's gradient: the library exports and binds the two new entries of
include/fvgp_hip_nn.h; the longdouble twin of the scores (vecchia_grad_ref) against differences of vecchia_ref.loglik_ref and against
the exact GP's gradient where the approximation is exact; the float64 twin's own error, which sets the device tests' bars.  Run with -s
for the record lines."""
import os
import re

import numpy as np
import pytest

import kernel_family_ref as kf
import test_host_logic as thl
import vecchia_grad_ref as vg
import vecchia_ref as vr
from conftest import ROOT

LD = vr.LD


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_gradient_entries_are_exported_and_bound():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fvgp_hip_nn.h")).read()
    protos, _ = thl._parse_header(hdr)
    for s in ("fvgp_hip_nn_loglik_grad", "fvgp_hip_nn_grad_workspace_bytes"):
        assert s in protos and s in _lib._ABI_NN and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is _lib._ABI_NN[s][0] and list(fn.argtypes) == _lib._ABI_NN[s][1]
    assert list(protos) == _lib.SYMBOLS_NN and thl._abi_differences(protos, _lib._ABI_NN, _lib) == []
    assert len(_lib._ABI_NN["fvgp_hip_nn_loglik_grad"][1]) == 21
    assert re.search(r"BIT CONTRACT: out_host, mu and var are bit for bit those of fvgp_hip_nn_loglik", hdr)


def test_gradient_workspace_rules():
    from fvgp_amd import _lib
    _lib.build()
    wb = _lib.lib().fvgp_hip_nn_grad_workspace_bytes
    assert wb(0, 1, 2) == -1 and wb(5, 0, 2) == -1 and wb(5, 1, 0) == -1 and wb(-3, 1, 2) == -1
    base = wb(1000, 3, 4)
    assert base > _lib.nn_workspace_bytes(_lib.NN_LOGLIK, 1000, 3) and base % 8 == 0
    assert wb(2000, 3, 4) > base and wb(1000, 4, 4) > base and wb(1000, 3, 5) > base
    assert _lib.nn_grad_workspace_bytes(1000, 3, 4) == base
    # the sums are per slice of 256 rows: row 257 opens a slice
    assert wb(257, 1, 4) > wb(256, 1, 4)


def test_gradient_call_refuses_a_null_handle_on_the_host():
    from fvgp_amd import _lib
    _lib.build()
    assert _lib.lib().fvgp_hip_nn_loglik_grad(None, 0, None, 1, 1, None, 2, 1, None, 1, 1, None, None, None, None, None, None, 0,
                                              None, None, None) == -1


# ---- 2. the longdouble twin against differences of the likelihood ----------------------------------------------------------------------------
def _richardson(name, x, theta, idx, r, v):
    """d log p / d theta_h by central differences of vecchia_ref.loglik_ref with steps 2^-12 theta_h and half of it, extrapolated"""
    out = np.zeros(len(theta), dtype=LD)
    for h in range(len(theta)):
        est = []
        for step in (LD(2) ** -12 * LD(theta[h]), LD(2) ** -13 * LD(theta[h])):
            tp, tm = np.asarray(theta, dtype=LD).copy(), np.asarray(theta, dtype=LD).copy()
            tp[h] += step
            tm[h] -= step
            est.append((_loglik_ld(name, x, tp, idx, r, v) - _loglik_ld(name, x, tm, idx, r, v)) / (LD(2) * step))
        out[h] = (LD(4) * est[1] - est[0]) / LD(3)
    return out


def _loglik_ld(name, x, theta_ld, idx, r, v):
    """vecchia_ref.loglik_ref at a longdouble theta (conditionals_ref rounds theta to float64: here it must not)"""
    x = np.asarray(x, dtype=np.float64)
    r, v = np.asarray(r, dtype=LD), np.asarray(v, dtype=LD)
    mu, d = np.zeros(len(x), dtype=LD), np.zeros(len(x), dtype=LD)
    for i in range(len(x)):
        c = np.array([j for j in idx[i] if 0 <= j < len(x)], dtype=np.int64)
        d[i] = kf.k_ref(name, x[i:i + 1], x[i:i + 1], theta_ld, LD)[0, 0] + v[i]
        if len(c):
            A = kf.k_ref(name, x[c], x[c], theta_ld, LD) + np.diag(v[c])
            k = kf.k_ref(name, x[c], x[i:i + 1], theta_ld, LD)[:, 0]
            w, z, _ = vr._chol_solve(A, k, r[c], LD)
            mu[i], d[i] = np.dot(w, z), d[i] - np.dot(w, w)
    return vr.loglik_terms(r, mu, d, LD)[0]


@pytest.mark.parametrize("case", [("matern32_ard", 2, 70, 15), ("rbf_ard", 3, 70, 33), ("matern52_iso", 4, 70, 32)],
                         ids=lambda c: "{}-d{}-n{}-m{}".format(*c))
def test_twin_is_the_derivative_of_the_likelihood(case):
    """the closed form against a Richardson central difference of loglik_ref in longdouble: 1e-11 of sum_i |score_ih| (truncation gave
    at most 5.9e-13 with these steps on five cases; the bar is about 17 times that, as other cases may truncate worse)"""
    name, d, n, m = case
    x, theta, r, v = vr.case_data(name, d, n)
    idx = vr.search_ref(x, x, m, vr.length_scales(name, theta, d), c0=0)
    # the longdouble theta of the differences and the float64 theta of the closed form are the same numbers
    assert float(_loglik_ld(name, x, np.asarray(theta, dtype=LD), idx, r, v)) == float(vr.loglik_ref(name, x, theta, idx, r, v, LD)[0])
    s = vg.scores_ref(name, x, theta, idx, r, v, LD)
    fd = _richardson(name, x, theta, idx, r, v)
    err = np.abs(np.sum(s, axis=0) - fd) / np.sum(np.abs(s), axis=0)
    print(f"\nvecchia grad twin vs Richardson {name} d={d} n={n} m={m}: " + " ".join(f"{float(e):.2e}" for e in err) + " (bar 1e-11)")
    assert np.all(err <= 1e-11)


@pytest.mark.parametrize("name", sorted(kf.FAMILY))
@pytest.mark.parametrize("n", [2, 33, 65])
def test_twin_with_all_earlier_points_is_the_exact_gradient(name, n):
    """m = n - 1: the scores add up to the dense 1/2 (alpha^T dK alpha - tr((K + V)^-1 dK)), held to 1e-15 n sum |terms|"""
    d = 3
    x, theta, r, v = vr.case_data(name, d, n, seed=1)
    idx = vr.search_ref(x, x, n - 1, vr.length_scales(name, theta, d), c0=0)
    g = np.sum(vg.scores_ref(name, x, theta, idx, r, v, LD), axis=0)
    exact, scale = vg.dense_grad_ld(name, x, theta, r, v)
    err = np.abs(g - exact) / scale
    print(f"\nvecchia grad twin vs dense longdouble {name} n={n}: " + " ".join(f"{float(e):.2e}" for e in err) + f" (bar {1e-15 * n:.1e})")
    assert np.all(err <= 1e-15 * n)


# ---- 3. the float64 twin's error: the bases of the device bars ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", vg.GRAD_CASES + (vr.EXACT_CASE,), ids=vr.case_id)
def test_float64_twin_error_is_recorded_and_finite(case):
    b = vg.bases(case)
    print(f"\nvecchia grad base {vr.case_id(case)}: " + " ".join(f"{k}={b[k]:.2e}" for k in vg.FIGURES))
    assert all(np.isfinite(b[k]) for k in vg.FIGURES)
    # well-conditioned cases (noise 1e-2 sigma^2): a double-precision evaluation loses a few digits of sixteen, no more
    assert max(b.values()) < 1e-10


def test_floor_is_the_median_of_the_bases():
    med = {k: float(np.median([vg.bases(c)[k] for c in vg.GRAD_CASES])) for k in vg.FIGURES}
    print("\nvecchia grad floor: " + " ".join(f"{k}={med[k]:.3e}" for k in vg.FIGURES))
    for k in vg.FIGURES:
        assert abs(med[k] / vg.FLOOR[k] - 1.0) < 0.01, (k, med[k], vg.FLOOR[k])
    # the cases cover what the device has code paths for
    C = vg.GRAD_CASES
    assert {c[0] for c in C} == set(kf.FAMILY) and {c[1] for c in C} == set(kf.DIMS)
    assert {c[3] for c in C} >= {1, 15, 16, 17, 31, 32, 33, 63, 64}
    assert {c[2] for c in C} == {1, 2, 70, 300} and {c[4] for c in C} == {1, 3}
    assert all(c[2] <= 70 for c in C if c[3] >= 63)
    assert vg.SLICE_CASE[2] > 256 and vg.SLICE_CASE[3] == 3 and sum(c[2] > 256 for c in C) == 1
    assert vg.MARGIN == vr.MARGIN
