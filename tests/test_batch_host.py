"""CPU-only checks of the batched log-likelihood's host side: the three entry points are exported with the right result types,
the per-problem square and workspace queries, and the facade's chunk planner."""
import ctypes

import numpy as np
import pytest

BATCH = ("fvgp_hip_loglik_batch", "fvgp_hip_loglik_batch_dim", "fvgp_hip_loglik_batch_workspace_bytes")


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def test_batch_symbols_exported_with_restypes(L):
    from fvgp_amd import _lib
    for s in BATCH:
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.fvgp_hip_loglik_batch.restype is ctypes.c_int
    assert L.fvgp_hip_loglik_batch_dim.restype is ctypes.c_int64
    assert L.fvgp_hip_loglik_batch_workspace_bytes.restype is ctypes.c_int64
    assert len(L.fvgp_hip_loglik_batch.argtypes) == 18


def test_batch_dim_query(L):
    from fvgp_amd import _lib
    for ncol in (1, 2, 8):
        for n in list(range(1, 300)) + list(range(3900, 4200)):
            want = L.fvgp_hip_loglik_dim(n, ncol)
            got = L.fvgp_hip_loglik_batch_dim(n, ncol)
            assert got == (want if want <= _lib.BATCH_MAX_DIM else 0), (n, ncol)
            assert _lib.loglik_batch_dim(n, ncol) == got
    assert L.fvgp_hip_loglik_batch_dim(4095, 1) == 4096 and L.fvgp_hip_loglik_batch_dim(4096, 1) == 0
    assert L.fvgp_hip_loglik_batch_dim(0, 1) == -1


def test_batch_workspace_query(L):
    # per problem: one 128 x 128 block inverse, the reciprocal pivots, the theta table row (1 + 16), two reductions, an info word
    for n, ncol, B in ((500, 1, 1), (2000, 1, 64), (4000, 3, 7), (128, 1, 3)):
        dim = L.fvgp_hip_loglik_batch_dim(n, ncol)
        assert L.fvgp_hip_loglik_batch_workspace_bytes(n, ncol, B) == B * (128 * 128 + dim + 17 + 2) * 8 + B * 4
    assert L.fvgp_hip_loglik_batch_workspace_bytes(500, 1, 0) == -1
    assert L.fvgp_hip_loglik_batch_workspace_bytes(5000, 1, 4) == -1
    # the single-evaluation query is what it was
    assert L.fvgp_hip_workspace_bytes(500, 0) > 0


@pytest.mark.parametrize("B,per,budget", [(1, 10, 5), (64, 8 << 20, 1 << 30), (64, 128 << 20, 1 << 30), (10, 3, 7), (7, 5, 100),
                                          (1000, 33, 1000)])
def test_chunk_planner(B, per, budget):
    from fvgp_amd.gp import _batch_chunks
    ch = _batch_chunks(B, per, budget)
    covered = [b for s, e in ch for b in range(s, e)]
    assert covered == list(range(B))
    for s, e in ch:
        assert e > s
        assert (e - s) * per <= budget or e - s == 1
    assert all(e - s == ch[0][1] - ch[0][0] for s, e in ch[:-1])


def test_default_budget():
    from fvgp_amd import gp
    assert gp.BATCH_MAX_BYTES >= 1 << 30
    assert np.all(np.diff([s for s, _ in gp._batch_chunks(100, 1 << 20, gp.BATCH_MAX_BYTES)]) > 0)
