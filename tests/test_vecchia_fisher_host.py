"""CPU-only checks of the Fisher information of the nearest-neighbour likelihood: the library exports and binds the two new entries of
include/fvgp_hip_nn.h; the longdouble twin of the rows (vecchia_fisher_ref) against the trace difference it collapses and against the
exact GP's Fisher matrix where the approximation is exact; every row positive semidefinite; the float64 twin's own error, which sets the
device tests' bars; projected Fisher scoring (fvgp_amd/fisher_scoring.py) on the twin's objective.  Run with -s for the record lines."""
import os
import re

import numpy as np
import pytest

import kernel_family_ref as kf
import test_host_logic as thl
import vecchia_fisher_ref as vf
import vecchia_grad_ref as vg
import vecchia_ref as vr
from conftest import ROOT

LD = vr.LD


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_fisher_entries_are_exported_and_bound():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fvgp_hip_nn.h")).read()
    protos, _ = thl._parse_header(hdr)
    for s in ("fvgp_hip_nn_loglik_fisher", "fvgp_hip_nn_fisher_workspace_bytes"):
        assert s in protos and s in _lib._ABI_NN and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is _lib._ABI_NN[s][0] and list(fn.argtypes) == _lib._ABI_NN[s][1]
    assert list(protos) == _lib.SYMBOLS_NN and thl._abi_differences(protos, _lib._ABI_NN, _lib) == []
    assert len(_lib._ABI_NN["fvgp_hip_nn_loglik_fisher"][1]) == 23
    assert re.search(r"BIT CONTRACT: out_host, mu, var, score and grad_host are bit for bit those of fvgp_hip_nn_loglik_grad", hdr)


def test_fisher_workspace_rules():
    from fvgp_amd import _lib
    _lib.build()
    wb = _lib.lib().fvgp_hip_nn_fisher_workspace_bytes
    assert wb(0, 1, 2) == -1 and wb(5, 0, 2) == -1 and wb(5, 1, 0) == -1 and wb(-3, 1, 2) == -1
    base = wb(1000, 3, 4)
    assert base > _lib.nn_grad_workspace_bytes(1000, 3, 4) and base % 8 == 0
    assert wb(2000, 3, 4) > base and wb(1000, 4, 4) > base and wb(1000, 3, 5) > base
    assert _lib.nn_fisher_workspace_bytes(1000, 3, 4) == base
    assert wb(257, 1, 4) > wb(256, 1, 4)          # the sums are per slice of 256 rows: row 257 opens a slice


def test_fisher_call_refuses_a_null_handle_on_the_host():
    from fvgp_amd import _lib
    _lib.build()
    assert _lib.lib().fvgp_hip_nn_loglik_fisher(None, 0, None, 1, 1, None, 2, 1, None, 1, 1, None, None, None, None, None, None, None, 0,
                                                None, None, None, None) == -1


# ---- 2. the longdouble twin against the definitions -------------------------------------------------------------------------------------------
def _scale(ref):
    """(H, H): max_i sqrt(ref_i,hh ref_i,kk), the scale of the `rows` figure"""
    diag = np.sqrt(np.einsum("ihh->ih", ref))
    return np.max(diag[:, :, None] * diag[:, None, :], axis=0)


@pytest.mark.parametrize("case", [("matern32_ard", 3, 40, 15), ("rbf_ard", 2, 40, 33), ("matern52_iso", 4, 40, 17)],
                         ids=lambda c: "{}-d{}-n{}-m{}".format(*c))
def test_twin_rows_are_the_trace_difference(case):
    """the row form against F(Sigma_ci + noise) - F(A), both longdouble: 1e-12 of the row scale, the float64 cancellation bound of the
    direct form (measured: at most a few 1e-18 in longdouble, 5e-15 in the float64 prototype)"""
    name, d, n, m = case
    x, theta, r, v = vr.case_data(name, d, n)
    idx = vr.search_ref(x, x, m, vr.length_scales(name, theta, d), c0=0)
    rows, direct = vf.fisher_rows_ref(name, x, theta, idx, v, LD), vf.direct_rows_ld(name, x, theta, idx, v)
    err = float(np.max(np.max(np.abs(rows - direct), axis=0) / _scale(direct)))
    print(f"\nvecchia fisher twin vs trace difference {name} d={d} n={n} m={m}: {err:.2e} (bar 1e-12)")
    assert err <= 1e-12


@pytest.mark.parametrize("n", [2, 33, 97])
def test_twin_with_all_earlier_points_is_the_dense_fisher_matrix(n):
    """m = n - 1 on the given order: the rows telescope to 1/2 tr((K + V)^-1 d_h K (K + V)^-1 d_k K), held to 1e-15 n of the scale"""
    name, d = "matern32_ard", 3
    x, theta, r, v = vr.case_data(name, d, n, seed=1)
    idx = vr.search_ref(x, x, n - 1, vr.length_scales(name, theta, d), c0=0)
    F = np.sum(vf.fisher_rows_ref(name, x, theta, idx, v, LD), axis=0)
    exact = vf.dense_fisher_ld(name, x, theta, v)
    dg = np.sqrt(np.diagonal(exact))
    err = float(np.max(np.abs(F - exact) / np.outer(dg, dg)))
    print(f"\nvecchia fisher twin vs dense longdouble n={n}: {err:.2e} (bar {1e-15 * n:.1e})")
    assert err <= 1e-15 * n


@pytest.mark.parametrize("case", vf.CASES, ids=vr.case_id)
def test_every_row_is_positive_semidefinite(case):
    worst = 0.0
    for ref in vf.reference(case):
        for Fi in np.asarray(ref, dtype=np.float64):
            lam, tr = np.linalg.eigvalsh(Fi)[0], np.trace(Fi)
            assert lam >= -1e-12 * tr, (lam, tr)
            worst = min(worst, lam / tr)
    print(f"\nvecchia fisher smallest eigenvalue / trace {vr.case_id(case)}: {worst:.2e}")


def test_batched_float64_objective_is_the_twin():
    """objective_f64 (what the optimiser test minimises) against the row-by-row twins in float64"""
    name, d, n, m = "matern32_ard", 3, 60, 17
    x, theta, r, v = vr.case_data(name, d, n)
    idx = vr.search_ref(x, x, m, vr.length_scales(name, theta, d), c0=0)
    f, g, F = vf.objective_f64(name, x, theta, idx, r, v)
    Fr = np.sum(vf.fisher_rows_ref(name, x, theta, idx, v, np.float64), axis=0)
    s = vg.scores_ref(name, x, theta, idx, r, v, np.float64)
    assert abs(f + float(vr.loglik_ref(name, x, theta, idx, r, v, np.float64)[0])) <= 1e-12 * abs(f)
    assert np.all(np.abs(g + np.sum(s, axis=0)) <= 1e-11 * np.sum(np.abs(s), axis=0))
    dg = np.sqrt(np.diagonal(Fr))
    assert np.all(np.abs(F - Fr) <= 1e-11 * np.outer(dg, dg))


# ---- 3. the float64 twin's error: the bases of the device bars ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", vf.CASES + (vf.EXACT_CASE,), ids=vr.case_id)
def test_float64_twin_error_is_recorded_and_finite(case):
    b = vf.bases(case)
    print(f"\nvecchia fisher base {vr.case_id(case)}: " + " ".join(f"{k}={b[k]:.2e}" for k in vf.FIGURES))
    assert all(np.isfinite(b[k]) for k in vf.FIGURES)
    # well-conditioned cases (noise 1e-2 sigma^2): a double-precision evaluation loses a few digits of sixteen, no more
    assert max(b.values()) < 1e-10


def test_floor_is_the_median_of_the_bases():
    med = {k: float(np.median([vf.bases(c)[k] for c in vf.CASES])) for k in vf.FIGURES}
    print("\nvecchia fisher floor: " + " ".join(f"{k}={med[k]:.3e}" for k in vf.FIGURES))
    for k in vf.FIGURES:
        assert abs(med[k] / vf.FLOOR[k] - 1.0) < 0.01, (k, med[k], vf.FLOOR[k])
    # the cases cover what the device has code paths for
    C = vf.CASES
    assert {c[0] for c in C} == set(kf.FAMILY) and {c[1] for c in C} == set(kf.DIMS) == {1, 2, 3, 4, 5, 16}
    assert {c[3] for c in C} == {1, 2, 15, 16, 17, 32, 33, 63, 64}
    assert all(70 <= c[2] <= 300 for c in C) and {c[4] for c in C} == {1, 3}
    assert vf.SLICE_CASE[2] > 256 and sum(c[2] > 256 for c in C) == 1
    assert {(c[0], c[1], c[2]) for c in C} <= {(c[0], c[1], c[2]) for c in vg.GRAD_CASES}
    assert vf.MARGIN == vr.MARGIN


# ---- 4. projected Fisher scoring on the twin's objective ------------------------------------------------------------------------------------
BOUNDS = np.array([[0.1, 10.0]] + [[0.05, 5.0]] * 3)


def _problem():
    """300 points, m = 17, Matern-3/2, d = 3: (objective theta -> (f, g, F), the number of its calls so far)"""
    name, d, n, m = "matern32_ard", 3, 300, 17
    x, theta, r, v = vr.case_data(name, d, n)
    idx = vr.search_ref(x, x, m, vr.length_scales(name, theta, d), c0=0)
    calls = []

    def objective(t):
        calls.append(np.array(t))
        return vf.objective_f64(name, x, t, idx, r, v)
    return objective, calls


def _inside(t):
    return np.all(np.asarray(t) >= BOUNDS[:, 0]) and np.all(np.asarray(t) <= BOUNDS[:, 1])


def test_fisher_scoring_on_the_twin_objective():
    from scipy.optimize import minimize
    from fvgp_amd.fisher_scoring import fisher_scoring
    objective, calls = _problem()
    start, tol = np.array([3.0, 1.5, 1.5, 1.5]), 1e-8
    theta, history, evaluations = fisher_scoring(objective, start, BOUNDS, max_iter=200, tolerance=tol)
    assert evaluations == len(calls) and len({c.tobytes() for c in calls}) == len(calls), "nothing is evaluated twice"
    fs = [h[1] for h in history]
    assert _inside(theta) and all(_inside(h[0]) for h in history)
    assert np.array_equal(history[0][0], start) and np.array_equal(history[-1][0], theta) and history[-1][3] == 0.0
    assert all(b <= a for a, b in zip(fs, fs[1:])), fs
    assert history[-1][2] < tol and len(history) - 1 < 200
    assert all(0.0 < h[3] <= 1.0 for h in history[:-1])
    n_fisher = len(calls)
    res = minimize(lambda t: objective(t)[:2], start, jac=True, method="L-BFGS-B", bounds=BOUNDS)
    print(f"\nfisher scoring on the twin: {len(history) - 1} iterations, {n_fisher} calls, f {fs[0]:.4f} -> {fs[-1]:.6f}, theta "
          f"{np.round(theta, 4)}; L-BFGS-B: {len(calls) - n_fisher} calls, f {res.fun:.6f}")
    assert fs[-1] <= res.fun + 1e-6 * abs(res.fun)


def test_fisher_scoring_keeps_a_pinned_component_on_its_bound():
    """sigma^2 starts on its upper bound with the gradient pointing outward (the likelihood wants more): it stays there while the
    other components move"""
    from fvgp_amd.fisher_scoring import fisher_scoring
    objective, calls = _problem()
    bounds = BOUNDS.copy()
    bounds[0] = [0.01, 0.05]
    start = np.array([0.05, 0.5, 0.5, 0.5])
    f0, g0, _ = objective(start)
    assert g0[0] < 0.0, "the construction: the gradient at the upper bound points outward"
    theta, history, _ = fisher_scoring(objective, start, bounds, max_iter=3, tolerance=1e-4)
    assert len(history) >= 2 and history[1][0][0] == 0.05 and not np.array_equal(history[1][0][1:], start[1:])
    assert history[1][1] < f0


def test_fisher_scoring_treats_an_infinite_trial_as_rejected():
    """f = (theta - 1)^2 with a wall: +inf past 1.5.  From 0 with a curvature that is too small the full step lands behind the wall and
    is halved, not raised"""
    from fvgp_amd.fisher_scoring import fisher_scoring

    def objective(t):
        if t[0] > 1.5:
            return np.inf, np.full(1, np.nan), np.full((1, 1), np.nan)
        return float((t[0] - 1.0) ** 2), np.array([2.0 * (t[0] - 1.0)]), np.array([[0.5]])
    theta, history, _ = fisher_scoring(objective, np.array([0.0]), np.array([[-5.0, 5.0]]), max_iter=50, tolerance=1e-10)
    assert abs(theta[0] - 1.0) < 1e-4 and all(np.isfinite(h[1]) for h in history) and history[0][3] < 1.0
