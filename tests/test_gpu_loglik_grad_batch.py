"""Batched log-likelihood gradient (fvgp_hip_loglik_grad_batch, Handle.loglik_grad_batch, GP.neg_log_likelihood_gradient_batch,
train(method="adam") with adam_starts): the reference's gradients, parity with the single path, bitwise value parity with the batched
log-likelihood, batch independence, edges, the facade's semantics and multi-start Adam."""
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


def _thetas(theta, B, seed):
    rng = np.random.default_rng(seed)
    return np.asarray(theta)[None, :] * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), (B, len(theta))))


def _ym(y):
    y2 = y.reshape(len(y), -1)
    return y2 - np.mean(y2)


def _gbatch(H, kernel, x, thetas, V, ym, component=0, outs=False):
    from fvgp_amd import _lib
    n, ncol = x.shape[0], ym.shape[-1]
    dim, npd = _lib.loglik_batch_dim(n, ncol), _lib.pad128(n)
    B = len(thetas)
    KV, W = H.empty(B, dim, dim), H.empty(B, npd, npd)
    bo, do = (H.empty(B, n), H.empty(B, n)) if outs else (None, None)
    out, grad, info = H.loglik_grad_batch(_lib.KERNEL_IDS[kernel], H.to_device(x), np.asarray(thetas), H.to_device(V), H.to_device(ym),
                                          KV, W, component, bo, do)
    if outs:
        return out, grad, info, bo.cpu().numpy(), do.cpu().numpy()
    return out, grad, info


def _vbatch(H, kernel, x, thetas, V, ym):
    from fvgp_amd import _lib
    dim = _lib.loglik_batch_dim(x.shape[0], ym.shape[-1])
    return H.loglik_batch(_lib.KERNEL_IDS[kernel], H.to_device(x), np.asarray(thetas), H.to_device(V), H.to_device(ym),
                          H.empty(len(thetas), dim, dim))


def _single_grad(H, kernel, x, theta, V, ym, component=0):
    from fvgp_amd import _lib
    n, ncol = ym.shape
    dim, npd = _lib.loglik_dim(n, ncol), _lib.pad128(n)
    KV, W, alpha = H.empty(dim, dim), H.empty(npd, npd), H.empty(npd, ncol)
    kid = _lib.KERNEL_IDS[kernel]
    ll, logdet, quad, info = H.loglik(kid, H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)
    assert info == 0
    return H.loglik_grad(kid, H.to_device(x), theta, alpha, ncol, component, KV, W)


@pytest.mark.parametrize("name", ["G1_rbf_n500_d1.npz", "G2_rbf_n512_d3.npz", "G3_matern52_n512_d3.npz", "G4_default_n256_d2.npz",
                                  "G6_rbf_2col_n300_d3.npz"])
def test_grad_batch_matches_reference_gradients(name):
    """through the facade, as test_gpu_facade builds these GPs (G4: default kernel and noise)"""
    import fvgp_amd
    fx = load_golden(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name.startswith("G4"):
            gp = fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"])
        else:
            gp = fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"], noise_variances=fx["noise_variances"],
                             kernel_function=str(fx["kernel"]))
    th = np.vstack([fx["theta"], _thetas(fx["theta"], 3, 1)])
    for c, key in ((0, "grad"), (1, "grad_c1")):
        if key not in fx:
            continue
        g = gp.neg_log_likelihood_gradient_batch(th, component=c)
        np.testing.assert_allclose(g[0], fx[key], rtol=1e-8, atol=1e-9 * np.max(np.abs(fx[key])))


@pytest.mark.parametrize("kernel", KERNELS)
def test_grad_batch_all_kernels_match_single(H, kernel):
    x, y = synth(300, 2, seed=11)
    ym, V = _ym(y), np.full(300, 0.02)
    theta = np.array([1.3, 0.4, 0.25]) if kernel.endswith("ard") else np.array([1.3, 0.35])
    th = _thetas(theta, 8, 3)
    out, grad, info = _gbatch(H, kernel, x, th, V, ym)
    assert np.all(info == 0)
    for b in range(8):
        np.testing.assert_allclose(grad[b], _single_grad(H, kernel, x, th[b], V, ym), rtol=1e-9, atol=1e-12 * np.max(np.abs(grad[b])))


def test_grad_batch_synth2000_and_value_bits(H):
    x, y = synth(2000, 3)
    ym, V = _ym(y), np.full(2000, 0.01)
    th = _thetas(np.array([1.0, 0.3, 0.3, 0.3]), 16, 7)
    out, grad, info = _gbatch(H, "rbf_ard", x, th, V, ym)
    vout, vinfo = _vbatch(H, "rbf_ard", x, th, V, ym)
    assert np.all(info == 0) and np.all(vinfo == 0)
    assert out.tobytes() == vout.tobytes()
    for b in (0, 5, 15):
        np.testing.assert_allclose(grad[b], _single_grad(H, "rbf_ard", x, th[b], V, ym), rtol=1e-9, atol=1e-12 * np.max(np.abs(grad[b])))


def test_grad_batch_bitwise_independent(H):
    fx = load_golden("G1_rbf_n500_d1.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 64, 5)
    full = _gbatch(H, "rbf_ard", x, th, V, ym)
    again = _gbatch(H, "rbf_ard", x, th, V, ym)
    rev = _gbatch(H, "rbf_ard", x, th[::-1].copy(), V, ym)
    assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
    assert rev[0][::-1].tobytes() == full[0].tobytes() and rev[1][::-1].tobytes() == full[1].tobytes()
    bad = th[2:3].copy()
    bad[0, 0] = -1.0
    mixed = _gbatch(H, "rbf_ard", x, np.vstack([th[:2], bad, th[2:5]]), V, ym)
    assert mixed[2][2] != 0 and np.all(np.isnan(mixed[0][2])) and np.all(np.isnan(mixed[1][2]))
    keep = [0, 1, 3, 4, 5]
    assert mixed[0][keep].tobytes() == full[0][:5].tobytes() and mixed[1][keep].tobytes() == full[1][:5].tobytes()
    rep = _gbatch(H, "rbf_ard", x, np.vstack([th[17:18]] * 3), V, ym)
    for b in (0, 17, 63):
        alone = _gbatch(H, "rbf_ard", x, th[b:b + 1], V, ym)
        assert alone[0][0].tobytes() == full[0][b].tobytes() and alone[1][0].tobytes() == full[1][b].tobytes()
    for r in range(3):
        assert rep[1][r].tobytes() == full[1][17].tobytes()


@pytest.mark.parametrize("n,ncol,component", [(1, 1, 0), (128, 1, 0), (512, 1, 0), (300, 2, 1), (4095, 1, 0)])
def test_grad_batch_edges(H, n, ncol, component):
    if ncol == 2:
        fx = load_golden("G6_rbf_2col_n300_d3.npz")
        x, ym, V, theta = fx["x"], _ym(fx["y"]), fx["noise_variances"], fx["theta"]
    else:
        x, y = synth(n, 2, seed=n)
        ym, V, theta = _ym(y), np.full(n, 0.05), np.array([1.1, 0.3, 0.4])
    B = 3 if n == 4095 else 6
    th = _thetas(theta, B, n)
    out, grad, info = _gbatch(H, "rbf_ard", x, th, V, ym, component=component)
    vout, _ = _vbatch(H, "rbf_ard", x, th, V, ym)
    assert np.all(info == 0) and out.tobytes() == vout.tobytes()
    for b in range(B):
        ref = _single_grad(H, "rbf_ard", x, th[b], V, ym, component)
        np.testing.assert_allclose(grad[b], ref, rtol=1e-9, atol=1e-12 * max(1.0, np.max(np.abs(ref))))


def test_grad_batch_non_pd(H):
    fx = load_golden("G1_rbf_n500_d1.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 8, 2)
    clean = _gbatch(H, "rbf_ard", x, th, V, ym)
    bad = th.copy()
    bad[3, 0] = -1.0
    out, grad, info = _gbatch(H, "rbf_ard", x, bad, V, ym)
    _, vinfo = _vbatch(H, "rbf_ard", x, bad, V, ym)
    assert info[3] != 0 and info[3] == vinfo[3]
    assert np.all(np.isnan(out[3])) and np.all(np.isnan(grad[3]))
    keep = [b for b in range(8) if b != 3]
    assert out[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[1][keep].tobytes()
    assert np.all(info[keep] == 0)


def test_grad_batch_optional_outputs(H):
    fx = load_golden("G6_rbf_2col_n300_d3.npz")
    x, ym, V = fx["x"], _ym(fx["y"]), fx["noise_variances"]
    th = _thetas(fx["theta"], 4, 9)
    for c in (0, 1):
        out, grad, info, bo, do = _gbatch(H, "rbf_ard", x, th, V, ym, component=c, outs=True)
        assert np.all(info == 0)
        for b in range(4):
            KV = orc.addKV(orc.KERNELS["rbf_ard"](x, x, th[b]), V)
            inv = np.linalg.inv(KV)
            np.testing.assert_allclose(bo[b], (inv @ ym)[:, c], rtol=1e-8, atol=1e-10 * np.max(np.abs(bo[b])))
            np.testing.assert_allclose(do[b], np.diag(inv), rtol=1e-8)


def test_grad_batch_error_codes(H):
    from fvgp_amd import _lib
    x = H.to_device(np.random.default_rng(0).random((100, 1)))
    th = np.array([[1.0, 0.3]])
    V, ym = H.to_device(np.full(100, 0.01)), H.to_device(np.zeros((100, 1)))
    KV, W = H.empty(1, 128, 128), H.empty(1, 128, 128)

    def rc(**kw):
        a = dict(kernel_id=0, x=x, thetas=th, vdiag=V, ymean=ym, KV=KV, work=W, component=0)
        a.update(kw)
        with pytest.raises(_lib.HipExtensionError) as e:
            H.loglik_grad_batch(**a)
        return str(e.value)
    assert "status -4" in rc(x=H.to_device(np.random.default_rng(0).random((4096, 1))), vdiag=H.to_device(np.full(4096, 0.01)),
                             ymean=H.to_device(np.zeros((4096, 1))))
    assert "status -2" in rc(kernel_id=9)
    assert "status -7" in rc(thetas=np.array([[1.0]]))
    assert "status -8" in rc(thetas=np.zeros((0, 2)))
    assert "status -13" in rc(ymean=H.to_device(np.zeros((100, 9))), KV=H.empty(1, 256, 256))
    assert "status -14" in rc(component=1)
    assert "status -16" in rc(KV=H.empty(1, 128, 126))
    assert "status -19" in rc(work=H.empty(1, 128, 64))


# ---- facade ------------------------------------------------------------------------------------------------------------------
def _gp(fx, **kw):
    import fvgp_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"], **kw)


def _state(gp):
    return (gp.hyperparameters.copy(), gp.log_likelihood(), gp.KVinvY.copy(), gp.posterior_mean(gp.x_data[:7])["m(x)"].copy())


def test_facade_grad_batch_matches_loop_and_keeps_state():
    fx = load_golden("G3_matern52_n512_d3.npz")
    gp = _gp(fx, noise_variances=fx["noise_variances"], kernel_function="matern52_ard")
    th = _thetas(fx["theta"], 10, 4)
    before = _state(gp)
    got = gp.neg_log_likelihood_gradient_batch(th)
    f, g = gp.neg_log_likelihood_and_gradient_batch(th)
    after = _state(gp)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    loop = np.array([gp.neg_log_likelihood_gradient(t) for t in th])
    np.testing.assert_allclose(got, loop, rtol=1e-9, atol=1e-12 * np.max(np.abs(loop)))
    assert g.tobytes() == got.tobytes()
    np.testing.assert_allclose(f, [gp.neg_log_likelihood(t) for t in th], rtol=1e-12)
    gp.args["batch_max_bytes"] = 3 * (640 * 640 + 512 * 512) * 8
    assert gp.neg_log_likelihood_gradient_batch(th).tobytes() == got.tobytes()


def test_facade_grad_batch_theta_dependent_noise_and_mean():
    fx = load_golden("G1_rbf_n500_d1.npz")
    gp = _gp({"x": fx["x"], "y": fx["y"], "theta": np.array([1.0, 0.2, 0.01, 0.3])}, kernel_function="rbf_ard",
             noise_function=lambda x, h: np.full(len(x), h[2]) * (1.0 + 0.5 * x[:, 0]),
             prior_mean_function=lambda x, h: np.full(len(x), h[3] * h[0]))
    th = _thetas(np.array([1.0, 0.2, 0.01, 0.3]), 6, 6)
    loop = np.array([gp.neg_log_likelihood_gradient(t) for t in th])
    np.testing.assert_allclose(gp.neg_log_likelihood_gradient_batch(th), loop, rtol=1e-9, atol=1e-12 * np.max(np.abs(loop)))
    np.testing.assert_allclose(gp.neg_log_likelihood_gradient_batch(th, component=0), loop, rtol=1e-9, atol=1e-12 * np.max(np.abs(loop)))


def test_facade_grad_batch_fallbacks_exact():
    fx = load_golden("G2_rbf_n512_d3.npz")
    th = _thetas(fx["theta"], 3, 8)
    gk = _gp(fx, noise_variances=fx["noise_variances"], kernel_function=lambda a, b, h: orc.rbf_ard(a, b, h))
    assert gk.neg_log_likelihood_gradient_batch(th).tobytes() == np.array([gk.neg_log_likelihood_gradient(t) for t in th]).tobytes()
    gm = _gp(fx, kernel_function="rbf_ard", noise_function=lambda x, h: np.diag(np.full(len(x), 0.01)) + 1e-4 * np.ones((len(x), len(x))))
    assert gm.neg_log_likelihood_gradient_batch(th).tobytes() == np.array([gm.neg_log_likelihood_gradient(t) for t in th]).tobytes()


def test_facade_grad_batch_non_pd_raises_like_single():
    fx = load_golden("G1_rbf_n500_d1.npz")
    gp = _gp(fx, noise_variances=fx["noise_variances"], kernel_function="rbf_ard")
    th = _thetas(fx["theta"], 6, 3)
    th[2, 0] = -1.0
    th[4, 0] = -2.0
    with pytest.raises(Exception) as single:
        gp.neg_log_likelihood_gradient(th[2])
    with pytest.raises(Exception) as batch:
        gp.neg_log_likelihood_gradient_batch(th)
    assert type(batch.value) is type(single.value)
    assert str(batch.value) == str(single.value)


def test_facade_grad_batch_fvgp():
    import fvgp_amd
    fx = load_golden("G5_fvgp_4x64.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(fx["fvgp_x"], fx["fvgp_y"], init_hyperparameters=fx["theta"], noise_variances=fx["fvgp_noise"])
    th = _thetas(fx["theta"], 5, 1)
    loop = np.array([gp.neg_log_likelihood_gradient(t) for t in th])
    np.testing.assert_allclose(gp.neg_log_likelihood_gradient_batch(th), loop, rtol=1e-9, atol=1e-12 * np.max(np.abs(loop)))


# ---- training ----------------------------------------------------------------------------------------------------------------
BOUNDS = np.array([[0.1, 5.0], [0.05, 2.0], [0.05, 2.0]])


def _train_gp(args):
    import fvgp_amd
    x, y = synth(200, 2, seed=21)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(x, y, init_hyperparameters=np.array([1.0, 0.3, 0.3]), noise_variances=np.full(200, 0.01),
                           kernel_function="rbf_ard", args=args)


def test_train_adam_multistart(monkeypatch):
    from fvgp_amd import GP
    from fvgp_amd.gp_training import adam_optimize
    gp = _train_gp({"adam_starts": 4})
    calls = {"n": 0}
    orig = GP.neg_log_likelihood_gradient

    def counting(self, *a, **kw):
        calls["n"] += 1
        return orig(self, *a, **kw)
    monkeypatch.setattr(GP, "neg_log_likelihood_gradient", counting)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hps = gp.train(hyperparameter_bounds=BOUNDS, method="adam", seed=3, max_iter=30, accept_only_if_improved=False)
    monkeypatch.setattr(GP, "neg_log_likelihood_gradient", orig)
    assert calls["n"] == 0
    info = gp.adam_multistart_info
    assert info["x0"].shape == (4, 3) and np.array_equal(info["x0"][0], [1.0, 0.3, 0.3])
    ref = _train_gp(None)
    for s in range(4):
        x, _ = adam_optimize(ref.neg_log_likelihood, ref.neg_log_likelihood_gradient, info["x0"][s], max_iter=30)
        np.testing.assert_allclose(info["x"][s], x, rtol=1e-6)
    assert info["best"] == int(np.argmin(info["f(x)"]))
    np.testing.assert_array_equal(hps, info["x"][info["best"]])
    assert len(gp.adam_history["theta"]) >= 1


def test_train_adam_default_unchanged(monkeypatch):
    from fvgp_amd import gp_training
    seen = []
    real = gp_training.adam_optimize

    def spy(f, g, theta0, **kw):
        seen.append((f, g, np.array(theta0), kw))
        return real(f, g, theta0, **kw)
    monkeypatch.setattr(gp_training, "adam_optimize", spy)
    gp = _train_gp(None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.train(hyperparameter_bounds=BOUNDS, method="adam", max_iter=3, accept_only_if_improved=False)
    assert len(seen) == 1
    f, g, t0, kw = seen[0]
    assert f == gp.neg_log_likelihood and g == gp.neg_log_likelihood_gradient
    np.testing.assert_array_equal(t0, [1.0, 0.3, 0.3])
    assert set(kw) == {"max_iter", "callback"} and kw["max_iter"] == 3
    assert not hasattr(gp, "adam_multistart_info")
