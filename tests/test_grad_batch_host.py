"""CPU-only checks of the batched gradient's host side: the two entry points are exported with the right types, the workspace query
follows its documented layout, the lockstep Adam matches sequential Adam trajectory for trajectory, and the multi-start draw."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def test_grad_batch_symbols_exported_with_restypes(L):
    from fvgp_amd import _lib
    for s in ("fvgp_hip_loglik_grad_batch", "fvgp_hip_loglik_grad_batch_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.fvgp_hip_loglik_grad_batch.restype is ctypes.c_int
    assert L.fvgp_hip_loglik_grad_batch_workspace_bytes.restype is ctypes.c_int64
    assert len(L.fvgp_hip_loglik_grad_batch.argtypes) == 25
    assert len(L.fvgp_hip_loglik_grad_batch_workspace_bytes.argtypes) == 3


def _documented(L, n, ncol, B):
    # per problem: every leaf inverse, reciprocal pivots, theta row (1 + 16), z and b, partial sums per lower tile for 17 hyperparameters,
    # two reductions, the gradient row, an info word
    dim = L.fvgp_hip_loglik_batch_dim(n, ncol)
    npd = (n + 127) // 128 * 128
    T = npd // 128
    return B * ((dim // 128) * 128 * 128 + dim + 17 + 2 * npd + T * (T + 1) // 2 * 17 + 2 + 17) * 8 + B * 4


def test_grad_batch_workspace_query(L):
    for n, ncol, B in ((500, 1, 1), (2000, 1, 64), (4000, 3, 7), (128, 1, 3), (1, 1, 2), (4095, 1, 5)):
        got = L.fvgp_hip_loglik_grad_batch_workspace_bytes(n, ncol, B)
        assert got > 0 and got == _documented(L, n, ncol, B), (n, ncol, B)
        assert L.fvgp_hip_loglik_grad_batch_workspace_bytes(n, ncol, B + 1) > got
        # it holds at least what the value-only batch keeps
        assert got >= L.fvgp_hip_loglik_batch_workspace_bytes(n, ncol, B)
    for n, ncol in ((4096, 1), (5000, 1), (4090, 8), (0, 1)):
        assert L.fvgp_hip_loglik_batch_dim(n, ncol) <= 0
        assert L.fvgp_hip_loglik_grad_batch_workspace_bytes(n, ncol, 4) <= 0
    assert L.fvgp_hip_loglik_grad_batch_workspace_bytes(500, 1, 0) <= 0


def _quadratic(A, c):
    def f(t):
        d = t - c
        return float(0.5 * d @ A @ d)

    def g(t):
        return A @ (t - c)
    return f, g


def _rosenbrock():
    def f(t):
        return float(np.sum(100.0 * (t[1:] - t[:-1] ** 2) ** 2 + (1.0 - t[:-1]) ** 2))

    def g(t):
        out = np.zeros_like(t)
        out[:-1] = -400.0 * t[:-1] * (t[1:] - t[:-1] ** 2) - 2.0 * (1.0 - t[:-1])
        out[1:] += 200.0 * (t[1:] - t[:-1] ** 2)
        return out
    return f, g


def _batched(f, g):
    return lambda X: (np.array([f(t) for t in X]), np.array([g(t) for t in X]))


@pytest.mark.parametrize("problem", ["quadratic", "rosenbrock"])
def test_adam_batch_matches_sequential(problem):
    from fvgp_amd.gp_training import adam_optimize, adam_optimize_batch
    rng = np.random.default_rng(5)
    if problem == "quadratic":
        M = rng.standard_normal((4, 4))
        f, g = _quadratic(M @ M.T + 4.0 * np.eye(4), rng.standard_normal(4))
        # starts near the minimum freeze early, the far ones late
        c = np.linalg.solve(M @ M.T + 4.0 * np.eye(4), (M @ M.T + 4.0 * np.eye(4)) @ np.zeros(4))
        X0 = np.vstack([rng.standard_normal(4) * s for s in (1e-4, 0.01, 1.0, 3.0, 10.0)]) + c
        kw = dict(lr=0.05, max_iter=400, tol=1e-3)
    else:
        f, g = _rosenbrock()
        X0 = rng.uniform(-1.5, 1.5, (6, 3))
        kw = dict(max_iter=300, tol=2e-3)
    xs, hists = adam_optimize_batch(_batched(f, g), X0, **kw)
    lengths = set()
    for s in range(len(X0)):
        x, h = adam_optimize(f, g, X0[s], **kw)
        np.testing.assert_allclose(xs[s], x, rtol=1e-12, atol=0)
        assert len(hists[s]["theta"]) == len(h["theta"])
        np.testing.assert_allclose(np.array(hists[s]["theta"]), np.array(h["theta"]), rtol=1e-12, atol=0)
        np.testing.assert_allclose(hists[s]["nlml"], h["nlml"], rtol=1e-12)
        np.testing.assert_allclose(hists[s]["grad_norm"], h["grad_norm"], rtol=1e-12)
        lengths.add(len(h["theta"]))
    assert len(lengths) > 1          # the trajectories froze at different steps


def test_adam_batch_only_evaluates_running_trajectories():
    from fvgp_amd.gp_training import adam_optimize_batch
    f, g = _quadratic(np.eye(2), np.zeros(2))
    sizes = []

    def fg(X):
        sizes.append(len(X))
        return _batched(f, g)(X)
    adam_optimize_batch(fg, np.array([[1e-5, 0.0], [1.0, 1.0], [3.0, -2.0]]), lr=0.1, max_iter=200, tol=1e-3)
    assert sizes[0] == 3 and sizes == sorted(sizes, reverse=True) and sizes[-1] < 3


def test_adam_start_points():
    from fvgp_amd.gp_training import adam_start_points
    bounds = np.array([[0.1, 5.0], [0.05, 2.0], [0.05, 2.0]])
    init = np.array([1.0, 0.3, 0.3])
    a = adam_start_points(init, bounds, 5, seed=3)
    b = adam_start_points(init, bounds, 5, seed=3)
    assert a.shape == (5, 3) and a.tobytes() == b.tobytes()
    assert np.array_equal(a[0], init)
    assert np.all((a >= bounds[:, 0]) & (a <= bounds[:, 1]))
    rs = np.random.RandomState(3)
    np.testing.assert_array_equal(a[1:], rs.uniform(low=bounds[:, 0], high=bounds[:, 1], size=(4, 3)))
    assert not np.array_equal(adam_start_points(init, bounds, 5, seed=4), a)
    np.random.seed(11)
    c = adam_start_points(init, bounds, 3)
    np.random.seed(11)
    np.testing.assert_array_equal(c[1:], np.random.uniform(low=bounds[:, 0], high=bounds[:, 1], size=(2, 3)))
