"""Batched log-likelihood (fvgp_hip_loglik_batch, Handle.loglik_batch, GP.log_likelihood_batch, train(batch_population)):
parity with the oracle, the reference's own values and the single evaluation; bitwise independence of the batch; edges; the
facade's semantics; training with a vectorised population."""
import warnings

import numpy as np
import pytest

from conftest import load_golden, synth
from oracle import fvgp_oracle as orc

pytestmark = pytest.mark.gpu

KERNELS = ["rbf_ard", "matern32_ard", "matern52_ard", "rbf_iso", "matern32_iso", "matern52_iso"]


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _terms(x, ym, V, theta, kernel):
    """oracle: {log-likelihood, log|KV|, quad / ncol} (gp_marginal_likelihood.py:137-179)"""
    KV = orc.addKV(orc.KERNELS[kernel](x, x, theta), V)
    L = orc.calculate_Chol_factor(KV)
    a = orc.calculate_Chol_solve(L, ym)
    ld = orc.calculate_Chol_logdet(L)
    quad = float(np.sum(ym * a)) / ym.shape[1]
    return np.array([-0.5 * (quad + ld + len(x) * np.log(2.0 * np.pi)), ld, quad])


def _thetas(theta, B, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(theta)[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, len(theta))))


def _batch(H, kernel, x, thetas, V, ym):
    from fvgp_amd import _lib
    n, ncol = x.shape[0], ym.shape[-1]
    dim = _lib.loglik_batch_dim(n, ncol)
    KV = H.empty(len(thetas), dim, dim)
    return H.loglik_batch(_lib.KERNEL_IDS[kernel], H.to_device(x), np.asarray(thetas), H.to_device(V), H.to_device(ym), KV)


def _single(H, kernel, x, theta, V, ym):
    from fvgp_amd import _lib
    n, ncol = ym.shape
    dim = _lib.loglik_dim(n, ncol)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), ncol)
    ll, logdet, quad, info = H.loglik(_lib.KERNEL_IDS[kernel], H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)
    return np.array([ll, logdet, quad]), info


def _ym(y):
    y2 = y.reshape(len(y), -1)
    return y2 - np.mean(y2)


def _cases():
    g1 = load_golden("G1_rbf_n500_d1.npz")
    x2, y2 = synth(2000, 3)
    yield "G1", g1["x"], _ym(g1["y"]), g1["noise_variances"], g1["theta"], "rbf_ard"
    yield "synth2000", x2, _ym(y2), np.full(2000, 0.01), np.array([1.0, 0.3, 0.3, 0.3]), "rbf_ard"


@pytest.mark.parametrize("case", ["G1", "synth2000"])
def test_batch_matches_oracle_and_single(H, case):
    name, x, ym, V, theta, kernel = [c for c in _cases() if c[0] == case][0]
    th = _thetas(theta, 64, 7)
    out, info = _batch(H, kernel, x, th, V, ym)
    assert np.all(info == 0)
    for b in range(64):
        ref = _terms(x, ym, V, th[b], kernel)
        np.testing.assert_allclose(out[b, 0], ref[0], rtol=1e-11)
        np.testing.assert_allclose(out[b, 1:], ref[1:], rtol=1e-10)
        single, sinfo = _single(H, kernel, x, th[b], V, ym)
        assert sinfo == 0
        np.testing.assert_allclose(out[b], single, rtol=1e-12)


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_all_kernels(H, kernel):
    x, y = synth(300, 2, seed=11)
    ym, V = _ym(y), np.full(300, 0.02)
    theta = np.array([1.3, 0.4, 0.25]) if kernel.endswith("ard") else np.array([1.3, 0.35])
    th = _thetas(theta, 64, 3)
    out, info = _batch(H, kernel, x, th, V, ym)
    assert np.all(info == 0)
    for b in range(64):
        ref = _terms(x, ym, V, th[b], kernel)
        np.testing.assert_allclose(out[b, 0], ref[0], rtol=1e-11)
        np.testing.assert_allclose(out[b, 1:], ref[1:], rtol=1e-10)


@pytest.mark.parametrize("name", ["G1_rbf_n500_d1.npz", "G2_rbf_n512_d3.npz", "G3_matern52_n512_d3.npz", "G6_rbf_2col_n300_d3.npz",
                                  "G5_fvgp_4x64.npz"])
def test_batch_matches_reference_logliks(H, name):
    fx = load_golden(name)
    out, info = _batch(H, str(fx["kernel"]), fx["x"], fx["thetas"], fx["noise_variances"], _ym(fx["y"]))
    assert np.all(info == 0)
    np.testing.assert_allclose(out[:, 0], fx["logliks"], rtol=1e-12)


def test_batch_bitwise_independent(H):
    fx = load_golden("G1_rbf_n500_d1.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 64, 5)
    full, _ = _batch(H, "rbf_ard", x, th, V, ym)
    again, _ = _batch(H, "rbf_ard", x, th, V, ym)
    rev, _ = _batch(H, "rbf_ard", x, th[::-1].copy(), V, ym)
    bad = th[:5].copy()
    bad[2, 0] = -1.0
    mixed, minfo = _batch(H, "rbf_ard", x, np.vstack([th[:2], bad[2:3], th[2:5]]), V, ym)
    assert minfo[2] != 0 and np.all(np.isnan(mixed[2]))
    for b in (0, 1, 17, 63):
        alone, _ = _batch(H, "rbf_ard", x, th[b:b + 1], V, ym)
        assert alone[0].tobytes() == full[b].tobytes()
    assert again.tobytes() == full.tobytes()
    assert rev[::-1].tobytes() == full.tobytes()
    assert np.vstack([mixed[:2], mixed[3:]]).tobytes() == full[:5].tobytes()


@pytest.mark.parametrize("n,ncol", [(1, 1), (128, 1), (512, 1), (300, 2)])
def test_batch_edges(H, n, ncol):
    if ncol == 2:
        fx = load_golden("G6_rbf_2col_n300_d3.npz")
        x, ym, V, theta = fx["x"], _ym(fx["y"]), fx["noise_variances"], fx["theta"]
    else:
        x, y = synth(n, 2, seed=n)
        ym, V, theta = _ym(y), np.full(n, 0.05), np.array([1.1, 0.3, 0.4])
    th = _thetas(theta, 9, n)
    out, info = _batch(H, "rbf_ard", x, th, V, ym)
    assert np.all(info == 0)
    for b in range(len(th)):
        ref = _terms(x, ym, V, th[b], "rbf_ard")
        np.testing.assert_allclose(out[b, 0], ref[0], rtol=1e-11)
        np.testing.assert_allclose(out[b, 1:], ref[1:], rtol=1e-10, atol=1e-300)


def test_batch_per_problem_targets(H):
    """vdiag / ymean of their own per problem (stride != 0): a theta-dependent noise and mean"""
    x, y = synth(400, 3, seed=4)
    th = _thetas(np.array([1.0, 0.3, 0.3, 0.3, 0.05]), 16, 9)
    V = np.stack([np.full(400, t[4]) * (1.0 + 0.5 * x[:, 0]) for t in th])
    Y = np.stack([(y - 0.1 * t[0]).reshape(-1, 1) for t in th])
    out, info = _batch(H, "rbf_ard", x, th, V, Y)
    assert np.all(info == 0)
    for b in range(len(th)):
        ref = _terms(x, Y[b], V[b], th[b][:4], "rbf_ard")
        np.testing.assert_allclose(out[b, 0], ref[0], rtol=1e-11)


def test_batch_scratch_contract(H):
    """the strict upper triangles are never read (NaN there changes nothing) and nothing outside the B squares is written"""
    import torch
    from fvgp_amd import _lib
    fx = load_golden("G2_rbf_n512_d3.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 6, 1)
    dim = _lib.loglik_batch_dim(512, 1)
    assert dim == 640
    ref, _ = _batch(H, "rbf_ard", x, th, V, ym)
    ld = dim + 6
    buf = H.empty(7, dim + 3, ld)
    buf.fill_(1234.5)
    up = torch.triu(torch.ones(dim, dim, dtype=torch.bool, device=buf.device), diagonal=1)
    for b in range(6):
        buf[b, :dim, :dim][up] = float("nan")
    KV = buf[:6, :dim, :]
    out, info = H.loglik_batch(0, H.to_device(x), th, H.to_device(V), H.to_device(ym), KV)
    torch.cuda.synchronize()
    assert out.tobytes() == ref.tobytes()
    assert bool((buf[:6, dim:, :] == 1234.5).all())
    assert bool((buf[:6, :dim, dim:] == 1234.5).all())
    assert bool((buf[6] == 1234.5).all())


def test_batch_error_codes(H):
    from fvgp_amd import _lib
    xd = H.to_device(np.random.default_rng(0).random((4096, 1)))
    th = np.array([[1.0, 0.3]])
    with pytest.raises(_lib.HipExtensionError, match="status -4"):
        H.loglik_batch(0, xd, th, H.to_device(np.full(4096, 0.01)), H.to_device(np.zeros((4096, 1))), H.empty(1, 128, 128))
    x = H.to_device(np.random.default_rng(0).random((100, 1)))
    with pytest.raises(_lib.HipExtensionError, match="status -13"):
        H.loglik_batch(0, x, th, H.to_device(np.full(100, 0.01)), H.to_device(np.zeros((100, 9))), H.empty(1, 256, 256))
    with pytest.raises(_lib.HipExtensionError, match="status -8"):
        H.loglik_batch(0, x, np.zeros((0, 2)), H.to_device(np.full(100, 0.01)), H.to_device(np.zeros((100, 1))), H.empty(1, 128, 128))


def test_batch_non_pd(H):
    fx = load_golden("G1_rbf_n500_d1.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 8, 2)
    clean, _ = _batch(H, "rbf_ard", x, th, V, ym)
    bad = th.copy()
    bad[3, 0] = -1.0
    out, info = _batch(H, "rbf_ard", x, bad, V, ym)
    _, sinfo = _single(H, "rbf_ard", x, bad[3], V, ym)
    assert sinfo == 1 and info[3] == sinfo
    assert np.all(np.isnan(out[3]))
    keep = [b for b in range(8) if b != 3]
    assert out[keep].tobytes() == clean[keep].tobytes() and np.all(info[keep] == 0)


# ---- facade ------------------------------------------------------------------------------------------------------------------
def _gp(fx, **kw):
    import fvgp_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"], **kw)


def _state(gp):
    return (gp.hyperparameters.copy(), gp.log_likelihood(), gp.KVinvY.copy(), np.array(gp.Chol_factor))


def test_facade_batch_matches_loop_and_keeps_state():
    fx = load_golden("G3_matern52_n512_d3.npz")
    gp = _gp(fx, noise_variances=fx["noise_variances"], kernel_function="matern52_ard")
    th = _thetas(fx["theta"], 20, 4)
    before = _state(gp)
    got = gp.log_likelihood_batch(th)
    after = _state(gp)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    np.testing.assert_allclose(got, [gp.log_likelihood(t) for t in th], rtol=1e-12)
    np.testing.assert_array_equal(gp.neg_log_likelihood_batch(th), -got)
    # a forced small budget (several chunks) gives the same bits as one chunk
    gp.args["batch_max_bytes"] = 3 * 640 * 640 * 8
    assert gp.log_likelihood_batch(th).tobytes() == got.tobytes()


def test_facade_batch_fallbacks_exact():
    fx = load_golden("G2_rbf_n512_d3.npz")
    th = _thetas(fx["theta"], 4, 8)
    from oracle.fvgp_oracle import rbf_ard
    gk = _gp(fx, noise_variances=fx["noise_variances"], kernel_function=lambda a, b, h: rbf_ard(a, b, h))
    np.testing.assert_array_equal(gk.log_likelihood_batch(th), [gk.log_likelihood(t) for t in th])

    def f_factor(KV):
        return np.linalg.cholesky(KV)

    def f_solve(L, b):
        return np.linalg.solve(L.T, np.linalg.solve(L, b))

    def f_logdet(L):
        return 2.0 * np.sum(np.log(np.diag(L)))
    gl = _gp(fx, noise_variances=fx["noise_variances"], kernel_function="rbf_ard", linalg_mode=[f_factor, f_solve, f_logdet])
    np.testing.assert_array_equal(gl.log_likelihood_batch(th), [gl.log_likelihood(t) for t in th])
    n = len(fx["x"])
    gm = _gp(fx, kernel_function="rbf_ard", noise_function=lambda x, h: np.diag(np.full(len(x), 0.01)) + 1e-4 * np.ones((len(x), len(x))))
    np.testing.assert_array_equal(gm.log_likelihood_batch(th), [gm.log_likelihood(t) for t in th])
    assert n == 512


def test_facade_batch_theta_dependent_noise():
    fx = load_golden("G1_rbf_n500_d1.npz")
    gp = _gp({"x": fx["x"], "y": fx["y"], "theta": np.array([1.0, 0.2, 0.01])}, kernel_function="rbf_ard",
             noise_function=lambda x, h: np.full(len(x), h[2]), prior_mean_function=lambda x, h: np.full(len(x), 0.1 * h[0]))
    th = _thetas(np.array([1.0, 0.2, 0.01]), 12, 6)
    np.testing.assert_allclose(gp.log_likelihood_batch(th), [gp.log_likelihood(t) for t in th], rtol=1e-12)


def test_facade_batch_non_pd_raises_like_single():
    fx = load_golden("G1_rbf_n500_d1.npz")
    gp = _gp(fx, noise_variances=fx["noise_variances"], kernel_function="rbf_ard")
    th = _thetas(fx["theta"], 6, 3)
    th[2, 0] = -1.0
    th[4, 0] = -2.0
    with pytest.raises(Exception) as single:
        gp.log_likelihood(th[2])
    with pytest.raises(Exception) as batch:
        gp.log_likelihood_batch(th)
    assert type(batch.value) is type(single.value)
    assert str(batch.value) == str(single.value)


def test_facade_batch_fvgp():
    import fvgp_amd
    fx = load_golden("G5_fvgp_4x64.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(fx["fvgp_x"], fx["fvgp_y"], init_hyperparameters=fx["theta"], noise_variances=fx["fvgp_noise"])
    th = np.vstack([fx["thetas"], _thetas(fx["theta"], 5, 1)])
    np.testing.assert_allclose(gp.log_likelihood_batch(th), [gp.log_likelihood(t) for t in th], rtol=1e-12)


# ---- training ----------------------------------------------------------------------------------------------------------------
def _train_gp(batch):
    import fvgp_amd
    x, y = synth(200, 2, seed=21)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(x, y, init_hyperparameters=np.array([1.0, 0.3, 0.3]), noise_variances=np.full(200, 0.01),
                           kernel_function="rbf_ard", args={"batch_population": True} if batch else None)


BOUNDS = np.array([[0.1, 5.0], [0.05, 2.0], [0.05, 2.0]])


def test_train_batch_population(monkeypatch):
    from fvgp_amd import GP
    gp1, gp2 = _train_gp(True), _train_gp(True)
    calls = {"n": 0}
    orig = GP.log_likelihood

    def counting(self, hyperparameters=None):
        if hyperparameters is not None:
            calls["n"] += 1
        return orig(self, hyperparameters)
    monkeypatch.setattr(GP, "log_likelihood", counting)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t1 = gp1.train(hyperparameter_bounds=BOUNDS, method="global", seed=3, max_iter=5)
        assert calls["n"] == 0
        t2 = gp2.train(hyperparameter_bounds=BOUNDS, method="global", seed=3, max_iter=5)
    monkeypatch.setattr(GP, "log_likelihood", orig)
    assert np.asarray(t1).tobytes() == np.asarray(t2).tobytes()
    # the same vectorised, deferred DE with an objective that loops over the single evaluation
    from scipy.optimize import differential_evolution
    gp3 = _train_gp(False)
    res = differential_evolution(lambda X: np.array([gp3.neg_log_likelihood(t) for t in X.T]), BOUNDS, maxiter=5, popsize=20,
                                 tol=1e-4, polish=False, x0=gp3.hyperparameters.reshape(1, -1), workers=1, seed=3, vectorized=True,
                                 updating="deferred")
    np.testing.assert_allclose(t1, res.x, rtol=1e-6)


def test_train_global_default_unchanged(monkeypatch):
    import scipy.optimize
    seen = {}
    real = scipy.optimize.differential_evolution

    def spy(func, bounds, **kw):
        seen.update(kw)
        return real(func, bounds, **kw)
    monkeypatch.setattr(scipy.optimize, "differential_evolution", spy)
    gp = _train_gp(False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.train(hyperparameter_bounds=BOUNDS, method="global", seed=3, max_iter=2)
    assert seen["workers"] == 1
    assert "vectorized" not in seen and "updating" not in seen
    assert set(seen) == {"maxiter", "popsize", "tol", "disp", "polish", "x0", "constraints", "workers", "seed"}
