"""Host side of the rank-k factor update and the removal of data points (fvgp_amd/csrc/chol_update.hip): the ABI surface, the workspace
query, and the numpy twin of the device sweep (tests/chol_update_ref.py) against numpy.linalg.cholesky of the kept matrix."""
import ctypes

import numpy as np
import pytest

import chol_update_ref as cr
from conftest import load_golden
from oracle import fvgp_oracle as orc

FIXTURES = {"G2": ("G2_rbf_n512_d3.npz", orc.rbf_ard), "G3": ("G3_matern52_n512_d3.npz", orc.matern52_ard)}
_CACHE = {}


def _factor(tag):
    """(KV, L) of a golden problem, computed once"""
    if tag not in _CACHE:
        name, kern = FIXTURES[tag]
        fx = load_golden(name)
        KV = orc.addKV(kern(fx["x"], fx["x"], fx["theta"]), fx["noise_variances"])
        _CACHE[tag] = (KV, np.linalg.cholesky(KV))
    return _CACHE[tag]


def removal_sets(n):
    rng = np.random.default_rng(23)
    return {"first": [0], "last": [n - 1], "straddle128": [127, 128, 129], "first16": list(range(16)),
            "random17": sorted(rng.choice(n, 17, replace=False).tolist()), "random70": sorted(rng.choice(n, 70, replace=False).tolist()),
            "every_second": list(range(0, n, 2))}


def test_library_exports_the_update_entries():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    for s in ("fvgp_hip_chol_update", "fvgp_hip_chol_delete", "fvgp_hip_chol_update_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert len(L.fvgp_hip_chol_update.argtypes) == 10 and L.fvgp_hip_chol_update.restype is ctypes.c_int
    assert len(L.fvgp_hip_chol_delete.argtypes) == 8 and L.fvgp_hip_chol_delete.restype is ctypes.c_int
    assert L.fvgp_hip_chol_update_workspace_bytes.restype is ctypes.c_int64
    assert _lib.CHOL_UPDATE_MAX_RANK == 16 and _lib.CHOL_UPDATE_TABLE_BYTES == 128 * 16 * 2 * 8
    # a missing handle is argument 1, before anything else is looked at
    assert L.fvgp_hip_chol_update(None, None, 0, 0, None, 0, 0, 0, None, 0) == -1
    assert L.fvgp_hip_chol_delete(None, None, 0, 0, None, 0, None, 0) == -1


def test_workspace_query():
    from fvgp_amd import _lib
    ws = _lib.chol_update_workspace_bytes
    for n, k in ((0, 1), (-3, 1), (10, 0), (10, -1)):
        assert ws(n, k) == -1
    assert ws(1, 1) >= _lib.CHOL_UPDATE_TABLE_BYTES
    # the pieces: the coefficient table, k + n index words, W (n x k) and a strip of at most 1024 rows -- never n x n
    for n in (1, 300, 4096, 20000, 50000, 10 ** 6):
        for k in (1, 16, 64):
            b = ws(n, k)
            assert b % 16 == 0
            assert _lib.CHOL_UPDATE_TABLE_BYTES < b <= 8 * (n + 1) * (k + 1 + 1024 + 2) + _lib.CHOL_UPDATE_TABLE_BYTES + 64
    # linear in n: doubling n at most doubles what is beyond the table (the strip stops growing at 2^25 doubles)
    for n in (2048, 8192, 20000, 50000, 250000):
        a, b = ws(n, 16) - _lib.CHOL_UPDATE_TABLE_BYTES, ws(2 * n, 16) - _lib.CHOL_UPDATE_TABLE_BYTES
        assert a < b <= 2 * a + 64
    assert ws(10 ** 6, 16) < 1 << 30


@pytest.mark.parametrize("tag", ["G2", "G3"])
def test_twin_matches_the_factor_of_the_kept_matrix(tag):
    KV, L = _factor(tag)
    n = len(L)
    scale = np.max(np.abs(L))
    for name, R in removal_sets(n).items():
        Rr, S = cr.split_indices(n, R)
        ref = np.linalg.cholesky(KV[np.ix_(S, S)])
        got = cr.chol_delete(L, R)
        err = np.max(np.abs(got - ref))
        print(f"chol_update twin|{tag}|{name}|k={len(Rr)}|{err / scale:.3g}")
        assert err <= 1e-12 * scale, name
        assert np.array_equal(got, np.tril(got)) and np.all(np.diag(got) > 0)


@pytest.mark.parametrize("tag", ["G2", "G3"])
def test_compaction_identity(tag):
    """KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T, L[S,S] lower triangular, W zero above the first removed index"""
    KV, L = _factor(tag)
    n = len(L)
    for name, R in removal_sets(n).items():
        Rr, S = cr.split_indices(n, R)
        Lss, W = cr.compaction(L, R)
        assert np.array_equal(Lss, np.tril(Lss)) and np.all(np.diag(Lss) > 0)
        assert Lss.shape == (len(S), len(S)) and W.shape == (len(S), len(Rr))
        assert not np.any(W[:Rr[0]])
        assert np.max(np.abs(Lss @ Lss.T + W @ W.T - KV[np.ix_(S, S)])) <= 1e-12, name


def test_twin_update_is_a_plain_rank_k_update():
    """the sweep on operands that come from no removal: every pass boundary, a row0, columns of W that start at different rows"""
    rng = np.random.default_rng(5)
    for n, k in ((1, 1), (1, 3), (7, 17), (40, 33), (129, 16)):
        A = rng.standard_normal((n, n))
        L = np.linalg.cholesky(A @ A.T + n * np.eye(n))
        W = rng.standard_normal((n, k))
        row0 = n // 3
        W[:row0] = 0.0
        for p in range(k):
            W[:min(n, row0 + 2 * p), p] = 0.0
        ref = np.linalg.cholesky(L @ L.T + W @ W.T)
        for r0 in (0, row0):
            assert np.max(np.abs(cr.chol_update(L, W, row0=r0) - ref)) <= 1e-12 * np.max(np.abs(ref))
