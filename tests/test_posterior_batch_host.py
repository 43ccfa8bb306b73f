"""CPU-only checks of the batched posterior's host side: the two entry points are exported with the right types, the workspace query
follows its documented layout, the moment matching of GP.posterior_mixture, and the facade's planner of row and point chunks."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def test_posterior_batch_symbols_exported_with_restypes(L):
    from fvgp_amd import _lib
    for s in ("fvgp_hip_posterior_batch", "fvgp_hip_posterior_batch_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.fvgp_hip_posterior_batch.restype is ctypes.c_int
    assert L.fvgp_hip_posterior_batch_workspace_bytes.restype is ctypes.c_int64
    assert len(L.fvgp_hip_posterior_batch.argtypes) == 26
    assert len(L.fvgp_hip_posterior_batch_workspace_bytes.argtypes) == 4


def _documented(L, n, ncol, B):
    # per problem: every leaf inverse, reciprocal pivots, theta row (1 + 16), two reductions, an info word
    dim = L.fvgp_hip_loglik_batch_dim(n, ncol)
    return B * ((dim // 128) * 128 * 128 + dim + 17 + 2) * 8 + B * 4


def test_posterior_batch_workspace_query(L):
    from fvgp_amd import _lib
    for n, ncol, B, pc in ((500, 1, 1, 128), (2000, 1, 64, 1024), (4000, 3, 7, 384), (128, 1, 3, 128), (1, 1, 2, 256), (4095, 1, 5, 4096)):
        got = L.fvgp_hip_posterior_batch_workspace_bytes(n, ncol, B, pc)
        assert got > 0 and got == _documented(L, n, ncol, B), (n, ncol, B, pc)
        assert got == _lib.posterior_batch_workspace_bytes(n, ncol, B, pc)
        assert L.fvgp_hip_posterior_batch_workspace_bytes(n, ncol, B + 1, pc) > got
        # it holds at least what the value-only batch keeps, and the prediction rows are the caller's
        assert got >= L.fvgp_hip_loglik_batch_workspace_bytes(n, ncol, B)
        assert L.fvgp_hip_posterior_batch_workspace_bytes(n, ncol, B, pc + 128) == got
    for n, ncol in ((4096, 1), (5000, 1), (4090, 8), (0, 1)):
        assert L.fvgp_hip_posterior_batch_workspace_bytes(n, ncol, 4, 128) <= 0
    assert L.fvgp_hip_posterior_batch_workspace_bytes(500, 1, 0, 128) <= 0
    for pc in (0, 64, 129, -128):
        assert L.fvgp_hip_posterior_batch_workspace_bytes(500, 1, 4, pc) <= 0


def test_posterior_batch_argument_errors_need_no_device(L):
    # a NULL handle is argument 1: refused before anything touches a device
    args =[None, 0, None, 4, 1, None, 2, 1, None, 0, None, 0, 1, None, 1, None, 256, 128, 0, None, None, None, 0, 0, None, None]
    assert L.fvgp_hip_posterior_batch(*args) == -1


@pytest.mark.parametrize("shape", [(5,), (7, 3), (4, 2, 6)])
def test_mixture_moments_match_direct_evaluation(shape):
    from fvgp_amd.gp import _mixture_moments, _mixture_weights
    rng = np.random.default_rng(11)
    B = 9
    m = rng.standard_normal((B,) + shape)
    v = rng.random((B,) + shape) + 0.01
    raw = rng.random(B) * 5.0
    w = _mixture_weights(raw, B)
    np.testing.assert_allclose(w, raw / raw.sum(), rtol=1e-15)
    assert abs(w.sum() - 1.0) < 1e-15
    mean, var, within, between = _mixture_moments(m, v, w)
    mean_d = np.zeros(shape); second = np.zeros(shape); within_d = np.zeros(shape)
    for b in range(B):
        mean_d += w[b] * m[b]
        within_d += w[b] * v[b]
        second += w[b] * (v[b] + m[b] ** 2)
    np.testing.assert_allclose(mean, mean_d, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(var, second - mean_d ** 2, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(within, within_d, rtol=1e-13)
    np.testing.assert_allclose(within + between, var, rtol=1e-13, atol=1e-15)
    assert np.all(between > -1e-14)
    # a sampled mixture has these two moments
    s = np.concatenate([m[b].ravel()[0] + np.sqrt(v[b].ravel()[0]) * rng.standard_normal(int(200000 * w[b])) for b in range(B)])
    assert abs(s.mean() - mean.ravel()[0]) < 0.02 and abs(s.var() - var.ravel()[0]) < 0.05 * var.ravel()[0] + 0.02


def test_mixture_weights_rules():
    from fvgp_amd.gp import _mixture_moments, _mixture_weights
    np.testing.assert_array_equal(_mixture_weights(None, 4), np.full(4, 0.25))
    np.testing.assert_allclose(_mixture_weights([2.0, 0.0, 6.0], 3), [0.25, 0.0, 0.75])
    for bad in ([1.0, -0.1, 1.0], [0.0, 0.0, 0.0], [1.0, np.nan, 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError):
            _mixture_weights(bad, 3)
    # one member: the mixture is that member
    m, v = np.array([[1.0, -2.0]]), np.array([[0.5, 0.25]])
    mean, var, within, between = _mixture_moments(m, v, _mixture_weights(None, 1))
    np.testing.assert_array_equal(mean, m[0]); np.testing.assert_array_equal(var, v[0])
    np.testing.assert_array_equal(between, np.zeros(2))


@pytest.mark.parametrize("B", [1, 2, 7, 64])
@pytest.mark.parametrize("P", [1, 127, 128, 129, 300, 1000])
@pytest.mark.parametrize("want_S", [False, True])
def test_planner_covers_every_row_and_point_once(B, P, want_S):
    from fvgp_amd import _lib
    from fvgp_amd.gp import _posterior_batch_plan
    dim, ncol = 512, 2
    for budget in (1, 8 * (dim + 128) * dim, 3 * 8 * (dim + 256) * dim + 5, 8 << 30):
        for max_chunk in (128, 256, 4096):
            pc, bs, ps = _posterior_batch_plan(B, P, dim, ncol, want_S, budget, max_chunk)
            assert pc % 128 == 0 and pc >= 128
            hits = np.zeros((B, P), dtype=int)
            for b0, b1 in bs:
                assert 0 <= b0 < b1 <= B
                for p0, p1 in ps:
                    assert 0 <= p0 < p1 <= P and p1 - p0 <= pc
                    hits[b0:b1, p0:p1] += 1
            assert np.all(hits == 1)
            # the point spans are the ones the device call walks with kv_rows = dim + P_chunk
            assert ps == [(p0, min(P, p0 + pc)) for p0 in range(0, P, pc)]
            if want_S:
                assert pc == _lib.pad128(P) and len(ps) == 1          # the covariance needs every point in one chunk
            else:
                assert pc <= max(128, min(_lib.pad128(P), max_chunk))
            per = 8 * ((dim + pc) * dim + P * ncol + P + (_lib.pad128(P) ** 2 if want_S else 0))
            for b0, b1 in bs:
                assert b1 - b0 == 1 or (b1 - b0) * per <= budget


def test_planner_chunk_edges():
    from fvgp_amd.gp import _posterior_batch_plan
    # P = P_chunk - 1, P_chunk, P_chunk + 1 with the chunk capped at 256
    for P, spans in ((255, [(0, 255)]), (256, [(0, 256)]), (257, [(0, 256), (256, 257)])):
        pc, _, ps = _posterior_batch_plan(3, P, 640, 1, False, 8 << 30, 256)
        assert pc == 256 and ps == spans
    # a budget below one problem's scratch: the chunk shrinks to 128 and the problems go one by one
    pc, bs, ps = _posterior_batch_plan(3, 1000, 640, 1, False, 1000, 4096)
    assert pc == 128 and bs == [(0, 1), (1, 2), (2, 3)] and len(ps) == 8
