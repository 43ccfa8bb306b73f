"""The exact Hessian of the negative log marginal likelihood on the device (fvgp_hip_loglik_hess, GP.neg_log_likelihood_exact_hessian,
GP.hyperparameter_laplace, args["exact_hessian"]) against the extended-precision reference tests/hessian_ref.py.

Inputs as tests/test_gpu_loo.py draws them (hessian_ref.case_inputs).  The bar is the project's gradient bar in a Hessian's form: every
raw entry within 1e-8 |H_ij| + 1e-9 max|H| of the longdouble value, the gradient alike; tests/test_hessian_host.py shows the float64
closed form itself at 2e-6 ... 4e-4 of that bar on every case here."""
import ctypes
import warnings

import numpy as np
import pytest

import hessian_ref as hr
from conftest import load_golden
from fvgp_amd._lib import KERNEL_IDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _report(entry, name, d, n, figure):
    print(f"HESS|{entry}|{name}|{d}|{n}|{figure:.3g}")


def _factor(H, name, x, ym, V, theta):
    """the factor of K + V as fvgp_hip_loglik leaves it, and KVinvY"""
    from fvgp_amd import _lib
    n, ncol = ym.shape
    dim = _lib.loglik_dim(n, ncol)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), ncol)
    info = H.loglik(KERNEL_IDS[name], H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)[3]
    assert info == 0
    return KV, alpha


def _hess(H, name, x, theta, KV, alpha, comp, poison_upper=False):
    """fvgp_hip_loglik_hess on a fresh copy of the factor (poison_upper: every entry strictly above its diagonal, inside the diagonal
    tiles too, filled with NaN first) and on scratches filled with NaN"""
    from fvgp_amd import _lib
    n, d = x.shape
    np_ = _lib.pad128(n)
    A = KV.clone()
    if poison_upper:
        i = H.torch.arange(A.shape[0], device=A.device)
        A[i[:, None] < i[None, :]] = float("nan")
    work, work2 = H.empty(np_, np_), H.empty(np_, np_)
    work.fill_(float("nan"))
    work2.fill_(float("nan"))
    ws = H.empty(_lib.loglik_hess_workspace_bytes(n, d) // 8)
    return H.loglik_hess(KERNEL_IDS[name], H.to_device(x), theta, alpha, alpha.shape[1], comp, A, work, work2, ws)


@pytest.mark.parametrize("name,n,d,ncol,comp,dup", hr.ABI_CASES)
def test_abi_against_extended_precision(H, name, n, d, ncol, comp, dup):
    (x, ym, V, theta), (g_r, raw_r) = hr.reference(name, n, d, ncol, comp, dup)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    g, raw = _hess(H, name, x, theta, KV, alpha, comp)
    f = lambda a: np.asarray(a, dtype=np.float64)
    bar = hr.hessian_bar(raw_r)
    ratios = {
        "hessian": float(np.max(np.abs(raw - f(raw_r)) / bar)),
        "gradient": float(np.max(np.abs(g - f(g_r)) / hr.hessian_bar(g_r))),
        "asymmetry": float(np.max(np.abs(raw - raw.T) / bar)),
    }
    for key, r in ratios.items():
        _report(f"{key} / bar", name, d, n, r)
    assert g.shape == theta.shape and raw.shape == (len(theta), len(theta))
    assert np.all(np.isfinite(raw)) and np.all(np.isfinite(g))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{worst}: {ratios[worst]:.3g} times its bar"


def test_determinism_and_the_undefined_triangle(H):
    """the same call twice gives the same bits; with the whole strict upper triangle of the factor filled with NaN, again the same"""
    name, n, d = "matern32_ard", 300, 3
    (x, ym, V, theta), _ = hr.reference(name, n, d, 1, 0, None)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    g0, r0 = _hess(H, name, x, theta, KV, alpha, 0)
    g1, r1 = _hess(H, name, x, theta, KV, alpha, 0)
    g2, r2 = _hess(H, name, x, theta, KV, alpha, 0, poison_upper=True)
    bits = lambda a: np.asarray(a).view(np.int64)
    assert np.all(np.isfinite(r0))
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(r0), bits(r1))
    assert np.array_equal(bits(g0), bits(g2)) and np.array_equal(bits(r0), bits(r2))


def test_bad_arguments_return_their_position_and_write_nothing(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    name, n, d = "rbf_ard", 96, 1
    (x, ym, V, theta), _ = hr.reference(name, n, d, 1, 0, None)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    np_ = _lib.pad128(n)
    work, work2 = H.empty(np_, np_), H.empty(np_, np_)
    nbytes = _lib.loglik_hess_workspace_bytes(n, d)
    ws = H.empty(nbytes // 8)
    xd = H.to_device(x)
    th = (ctypes.c_double * 2)(*theta)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(h=H._h, kid=KERNEL_IDS[name], x=p(xd), n=n, d=d, theta=th, ntheta=2, alpha=p(alpha), ncol=1, comp=0,
                KV=p(KV), ld=KV.stride(0), work=p(work), ldw=np_, work2=p(work2), ldw2=np_, ws=p(ws), ws_bytes=nbytes)
    bad = [("h", None, -1), ("kid", 6, -2), ("kid", -1, -2), ("x", None, -3), ("n", 0, -4), ("d", 0, -5), ("d", 17, -5), ("theta", None, -6),
           ("ntheta", 1, -7), ("alpha", None, -8), ("ncol", 0, -9), ("comp", 1, -10), ("comp", -1, -10), ("KV", None, -11), ("ld", np_ - 2, -12),
           ("ld", np_ + 1, -12), ("work", None, -13), ("ldw", np_ - 2, -14), ("work2", None, -15), ("ldw2", np_ + 1, -16), ("ws", None, -17),
           ("ws_bytes", nbytes - 8, -18), ("ws_bytes", 0, -18)]
    keys = list(good)
    kv_before = KV.clone()
    for key, value, status in bad:
        a = dict(good)
        a[key] = value
        g = (ctypes.c_double * 2)(7.0, 7.0)
        hs = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
        assert L.fvgp_hip_loglik_hess(*[a[k] for k in keys], g, hs) == status, (key, value)
        assert list(hs) == [7.0] * 4 and list(g) == [7.0] * 2, (key, value)
    g = (ctypes.c_double * 2)(7.0, 7.0)
    hs = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    assert L.fvgp_hip_loglik_hess(*[good[k] for k in keys], None, hs) == -19 and list(hs) == [7.0] * 4
    assert L.fvgp_hip_loglik_hess(*[good[k] for k in keys], g, None) == -20 and list(g) == [7.0] * 2
    H.sync()
    assert H.torch.equal(KV, kv_before)                          # nothing was launched either


# ---- facade -----------------------------------------------------------------------------------------------------------------------
def _g9():
    import fvgp_amd
    fx = load_golden("G9_derivatives_rbf_n256_d2.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"], noise_variances=fx["noise_variances"], kernel_function="rbf_ard")
    return gp, fx


def test_facade_on_the_reference_fixture():
    gp, fx = _g9()
    y = fx["y"] - np.mean(fx["y"])
    g_r, raw_r = hr.nll_hessian_ref("rbf_ard", fx["x"], y, fx["noise_variances"], fx["theta"])
    h_r = np.asarray((raw_r + raw_r.T) / 2, dtype=np.float64)
    state = (gp.hyperparameters.copy(), gp.log_likelihood(), gp.posterior_mean(fx["x_pred"])["m(x)"].copy())
    hess, g = gp.neg_log_likelihood_exact_hessian(return_gradient=True)
    ratio = float(np.max(np.abs(hess - h_r) / hr.hessian_bar(h_r)))
    ratio_g = float(np.max(np.abs(g - np.asarray(g_r, dtype=np.float64)) / hr.hessian_bar(g_r)))
    _report("facade hessian / bar", "rbf_ard", 2, 256, ratio)
    _report("facade gradient / bar", "rbf_ard", 2, 256, ratio_g)
    assert ratio <= 1.0 and ratio_g <= 1.0
    assert np.array_equal(hess, hess.T)
    assert np.array_equal(hess, gp.neg_log_likelihood_exact_hessian(fx["theta"]))
    g1 = gp.neg_log_likelihood_gradient()                      # another kernel, another order of the sums: the gradient's bar, not bits
    assert np.max(np.abs(g - g1) / hr.hessian_bar(g1)) <= 1.0
    fd = gp.neg_log_likelihood_hessian(fx["theta"])
    hs = np.max(np.abs(hess))
    _report("finite-difference route vs exact / max|H|", "rbf_ard", 2, 256, float(np.max(np.abs(fd - hess)) / hs))
    np.testing.assert_allclose(fd, hess, rtol=0, atol=1e-4 * hs)
    # another theta is evaluated on the scratch buffers; the state stays as it was, to the bit
    assert not np.array_equal(gp.neg_log_likelihood_exact_hessian(fx["theta2"]), hess)
    assert np.array_equal(gp.hyperparameters, state[0]) and gp.log_likelihood() == state[1]
    assert np.array_equal(gp.posterior_mean(fx["x_pred"])["m(x)"], state[2])


def _noise(x, h):
    return h[3] * (0.01 + 0.01 * x[:, 0])


def test_facade_refusals_name_the_finite_difference_route():
    import fvgp_amd
    from fvgp_amd import kernels
    fx = load_golden("G9_derivatives_rbf_n256_d2.npz")
    x, y, V, theta = fx["x"][:60], fx["y"][:60], fx["noise_variances"][:60], fx["theta"]
    route = "neg_log_likelihood_hessian"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        callable_gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function=lambda a, b, h: kernels.rbf_ard(a, b, h))
        linalg_gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="rbf_ard",
                                linalg_mode=[np.linalg.cholesky, lambda L, b: np.linalg.solve(L.T, np.linalg.solve(L, b)),
                                             lambda L: 2.0 * np.sum(np.log(np.diag(L)))])
        noise_gp = fvgp_amd.GP(x, y, init_hyperparameters=np.concatenate([theta, [1.3]]), kernel_function="rbf_ard", noise_function=_noise)
        sharded_gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="rbf_ard")
    sharded_gp._sharded = True           # the row-sharded mode's switch (a process group is not needed to be refused)
    for gp in (callable_gp, linalg_gp, noise_gp, sharded_gp):
        with pytest.raises(NotImplementedError, match=route):
            gp.neg_log_likelihood_exact_hessian()
        with pytest.raises(NotImplementedError, match=route):
            gp.hyperparameter_laplace()
    sharded_gp._sharded = False


# ---- Laplace approximation and Newton-type training (the case tests/test_hessian_host.py vets) ---------------------------------------
def _laplace_gp(**kw):
    import fvgp_amd
    x, y, V, bounds, start = hr.laplace_case()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=start, noise_variances=V, kernel_function="rbf_iso", **kw)
    return gp, x, bounds


def test_laplace_after_local_training():
    gp, x, bounds = _laplace_gp()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.train(hyperparameter_bounds=bounds, method="local", tolerance=1e-10)
    r = gp.hyperparameter_laplace(n_samples=16)
    lam = np.linalg.eigvalsh(r["covariance"])
    _report("laplace: lambda_min / lambda_max of the covariance", "rbf_iso", 1, 200, float(lam[0] / lam[-1]))
    assert lam[0] > 0.0
    assert np.max(np.abs(r["covariance"] @ r["hessian"] - np.eye(2))) <= 1e-8
    assert np.array_equal(r["mean"], gp.hyperparameters)
    expect = gp.log_likelihood() + np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(r["hessian"])[1]
    np.testing.assert_allclose(r["log_evidence"], expect, rtol=1e-10)
    assert r["samples"].shape == (16, 2) and np.all(r["samples"] > 0.0)
    mix = gp.posterior_mixture(x[::20], r["samples"])
    assert mix["m(x)"].shape == (10,) and np.all(np.isfinite(mix["m(x)"])) and np.all(mix["v(x)"] > 0.0)
    # away from the minimum the Hessian of this case is indefinite: no Laplace approximation there
    with pytest.raises(ValueError, match="not at a minimum"):
        gp.hyperparameter_laplace(hr.LAPLACE_NOT_A_MINIMUM)


def test_local_training_takes_the_exact_hessian(monkeypatch):
    import fvgp_amd
    gp, _, bounds = _laplace_gp(args={"exact_hessian": True})
    calls = []
    inner = fvgp_amd.GP.neg_log_likelihood_exact_hessian

    def spy(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)
    monkeypatch.setattr(fvgp_amd.GP, "neg_log_likelihood_exact_hessian", spy)
    start = gp.neg_log_likelihood()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hps = gp.train(hyperparameter_bounds=bounds, method="local", local_optimizer="trust-constr", max_iter=40)
    end = gp.neg_log_likelihood()
    _report("train trust-constr: Hessian calls", "rbf_iso", 1, 200, float(len(calls)))
    _report("train trust-constr: -log p start -> end", "rbf_iso", 1, 200, end - start)
    assert len(calls) >= 1
    assert end <= start
    assert np.all(hps >= bounds[:, 0]) and np.all(hps <= bounds[:, 1])
    # without the key nothing changes: no Hessian is handed over
    plain, _, _ = _laplace_gp()
    calls.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain.train(hyperparameter_bounds=bounds, method="local", local_optimizer="trust-constr", max_iter=5)
    assert calls == []
