"""CPU-only checks of the nearest-neighbour preconditioner's numpy twin (nn_precond_ref) and of the binding's host part: the factor is
the exact inverse Cholesky factor where every earlier point is a neighbour; the transposed lists are a permutation of the valid entries
in ascending row order (the twin's loops and the binding's stable sort agree); the iteration counts of the two regimes the README row
speaks of -- the nearest-neighbour factor far ahead once the data outgrow the rank, the low-rank preconditioner ahead on a small smooth
problem; the new entries are declared, exported and bound.  Run with -s for the record lines  NP|..."""
import os
import re

import numpy as np

import kernel_family_ref as kf
import matrix_free_ref as mf
import nn_precond_ref as npr
import vecchia_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
NEW_ENTRIES = ("fvgp_hip_nn_factor_workspace_bytes", "fvgp_hip_nn_factor", "fvgp_hip_nn_precond_apply_workspace_bytes",
               "fvgp_hip_nn_precond_apply", "fvgp_hip_pcg_nn_workspace_bytes", "fvgp_hip_pcg_nn")


def test_new_entries_are_declared_exported_and_bound():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fvgp_hip_nn.h")).read()
    declared = set(re.findall(r"\b(fvgp_hip_\w+)\s*\(", hdr))
    for s in NEW_ENTRIES:
        assert s in declared and s in _lib._ABI_NN and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is _lib._ABI_NN[s][0] and list(fn.argtypes) == _lib._ABI_NN[s][1]
    # the sizing entries answer without a device
    assert L.fvgp_hip_nn_factor_workspace_bytes(0) == -1 and L.fvgp_hip_nn_factor_workspace_bytes(1000) >= 8 * 1000
    assert L.fvgp_hip_nn_precond_apply_workspace_bytes(0) == -1 and L.fvgp_hip_nn_precond_apply_workspace_bytes(1000) >= 3 * 16 * 8 * 1000
    assert L.fvgp_hip_pcg_nn_workspace_bytes(0) == -1
    assert L.fvgp_hip_pcg_nn_workspace_bytes(1000) == L.fvgp_hip_pcg_workspace_bytes(1000, 0) + 16 * 8 * 1000, "the solver's, and T"


def test_factor_is_the_exact_inverse_where_every_earlier_point_is_a_neighbour():
    """n = 65, m = 64 on the given order: W^T W (K + V) is the identity (1e-12 asked; the record line has what double gives)"""
    case = vr.EXACT_CASE
    name, d, n, m, _ = case
    x, theta, v, idx = npr.factor_inputs(case)
    assert n == 65 and m == 64 and np.array_equal(np.sort(idx[-1]), np.arange(64))
    K = kf.k_ref(name, x, x, theta, np.float64)
    coef, dinv = npr.factor_ref(K, v, idx, np.float64)
    W = npr.dense_w(idx, coef, dinv)
    assert np.allclose(W, np.tril(W)) and np.all(np.diag(W) > 0)
    err = float(np.max(np.abs(W.T @ W @ (K + np.diag(v)) - np.eye(n))))
    print(f"\nNP|exact|n={n} m={m} max|W^T W (K + V) - I|={err:.2e}")
    assert err <= 1e-12
    # and the apply in longdouble is that product
    R = np.random.default_rng(1).standard_normal((n, 3))
    Z, mag, indeg = npr.apply_ref(idx, coef, dinv, R)
    assert np.max(np.abs(Z - (W.T @ (W @ R)))) <= 1e-13 * np.max(mag) and np.array_equal(indeg, np.arange(n)[::-1].clip(max=64))


def test_transposed_lists_are_a_permutation_in_ascending_rows():
    from fvgp_amd import _lib
    # lists with -1 and out-of-range entries between the neighbours, a leading dimension of their own
    n, m = 97, 17
    idx = npr.junk_lists(n, m)
    assert np.any(idx < 0) and np.any(idx >= n)
    for ld in (m, m + 3):
        start, pos = npr.transpose_ref(idx, n, ld)
        npr.check_transposed(idx, n, start, pos, ld)
        padded = np.full((n, ld), -1, dtype=np.int64)
        padded[:, :m] = idx
        s2, p2 = _lib.nn_transpose_lists(padded, n)
        assert s2.dtype == p2.dtype == np.int64 and np.array_equal(s2, start) and np.array_equal(p2, pos)
    # 40 coincident points in the given order: every later copy lists the earlier ones, one bucket outgrows a workgroup's 256 rows
    x = npr.coincident_set()
    m = 16
    idx = vr.search_ref(x, x, m, None, c0=0)
    start, pos = npr.transpose_ref(idx, len(x))
    npr.check_transposed(idx, len(x), start, pos)
    s2, p2 = _lib.nn_transpose_lists(idx, len(x))
    assert np.array_equal(s2, start) and np.array_equal(p2, pos)
    assert np.all(idx[16:40] == np.arange(16)), "the coincident rows list the first m copies (ties go to the lower index)"


def _counts(fx):
    """(rank-128 iterations, nearest-neighbour iterations) of the twin on column 0 at tol 1e-9"""
    low = mf.fixture_pcg(fx, 0, mf.RANK, TOL)
    nn = npr.fixture_pcg_nn(fx, 0, TOL)
    assert low[3] == 0 and nn[3] == 0 and low[2] <= TOL and nn[2] <= TOL
    # the two solve the same system: the ordered solution, taken back, is the other one
    o = npr.ordered_fixture(fx)
    x_nn = np.empty_like(nn[0])
    x_nn[o["perm"]] = nn[0]
    assert np.linalg.norm(x_nn - low[0]) <= 1e-6 * np.linalg.norm(low[0])
    print(f"\nNP|iterations|{mf.fixture_id(fx)} rank{mf.RANK}={low[1]} nn{npr.NEIGHBORS}={nn[1]}")
    return low[1], nn[1]


def test_iterations_once_the_data_outgrow_the_rank():
    """the two 2000-point fixtures: the m = 32 factor under a random ordering needs at most a quarter of rank 128's iterations"""
    for fx in npr.BIG_FIXTURES:
        low, nn = _counts(fx)
        assert 4 * nn <= low, (fx, low, nn)


def test_iterations_where_the_low_rank_preconditioner_wins():
    """FIXTURES[0] (rbf, d = 2, length scale 0.25, n = 1000): globally smooth and small -- rank 128 is ahead, which is why it stays the
    default"""
    low, nn = _counts(mf.FIXTURES[0])
    assert low < nn, (low, nn)
