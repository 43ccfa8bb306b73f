"""Leave-one-out cross-validation on the device (fvgp_hip_loo, GP.loo_*) against the extended-precision reference tests/loo_ref.py.

Inputs as the other GPU tests draw them: x uniform in the unit cube, sigma^2 = 1.2, length scales in [0.3, 0.6], noise 0.01 - 0.02 per
point, y centred; cond(KV) is 1e3 - 1e5 at these sizes, so the float64 closed form itself stays three orders inside the bars.
The bars are the project's existing ones: value rtol 1e-10 (the log-likelihood's), residuals and variances 1e-10 of their largest entry
(POSTERIOR_PARITY), gradient rtol 1e-8 + 1e-9 max|g|, u and diag M 1e-8 of their largest entry (b_out / diag_out of the batched gradient)."""
import functools
import warnings

import numpy as np
import pytest

import kernel_family_ref as kf
import loo_ref
from fvgp_amd._lib import KERNEL_IDS

pytestmark = pytest.mark.gpu

NAMES = list(KERNEL_IDS)
# (kernel, n, d, ncol, component)
ABI_CASES = ([(name, 300, 3, 1, 0) for name in NAMES]           # an interior off-diagonal tile, partial last tiles, both branches of the trace kernel
             + [("rbf_ard", 96, 1, 1, 0),                       # a single partial tile
                ("rbf_ard", 128, 2, 1, 0),                      # no padding rows
                ("rbf_ard", 200, 5, 1, 0),                      # the runtime-dimension instantiation
                ("rbf_ard", 1100, 2, 1, 0),                     # padded 1152 > POTRI's 1024-wide panel: two panels
                ("matern52_iso", 300, 3, 2, 1)])
# every (name, d) of the family grid that ABI_CASES does not hold, by rule, at n = 261: the smallest size with an interior tile strictly
# below the diagonal (tile (1, 0): the two-rows-per-trip path of the two-vector trace), partial edge tiles (tile row 2 has five rows),
# an odd n and padding to 384 -- the list tests/hessian_ref.py builds for the Hessian
FAMILY_CASES = [(name, 261, d, 1, 0) for name in NAMES for d in kf.DIMS if (name, d) not in {(c[0], c[2]) for c in ABI_CASES}]


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _report(entry, name, d, n, figure):
    print(f"LOO|{entry}|{name}|{d}|{n}|{figure:.3g}")


def _inputs(name, n, d, ncol=1, seed=None):
    rng = np.random.default_rng(31 * n + 7 * d + sorted(KERNEL_IDS).index(name) if seed is None else seed)
    x = rng.random((n, d))
    theta = np.concatenate([[1.2], rng.uniform(0.3, 0.6, kf.n_theta(name, d) - 1)])
    y = np.stack([np.sin((3.0 + c) * x.sum(axis=1)) + 0.1 * rng.standard_normal(n) for c in range(ncol)], axis=1)
    return x, y - y.mean(axis=0), rng.uniform(0.01, 0.02, n), theta


@functools.lru_cache(maxsize=None)
def _reference(name, n, d, ncol, comp):
    """the case's inputs and loo_closed on them, computed once"""
    x, ym, V, theta = _inputs(name, n, d, ncol)
    value, m_loo, v_loo, grad, u, md = loo_ref.loo_closed(name, x, ym[:, comp], V, theta)
    resid = ym[:, comp].astype(np.longdouble) - m_loo
    return (x, ym, V, theta), (value, resid, v_loo, grad, u, md)


def _factor(H, name, x, ym, V, theta):
    """the factor of K + V as fvgp_hip_loglik leaves it, and KVinvY"""
    from fvgp_amd import _lib
    n, ncol = ym.shape
    dim = _lib.loglik_dim(n, ncol)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), ncol)
    info = H.loglik(KERNEL_IDS[name], H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)[3]
    assert info == 0
    return KV, alpha


def _loo(H, name, x, theta, KV, alpha, comp, grad=True):
    """fvgp_hip_loo on a fresh copy of the factor; every output as host arrays, and the destroyed copy"""
    from fvgp_amd import _lib
    n = len(x)
    np_ = _lib.pad128(n)
    A, work = KV.clone(), H.empty(np_, np_)
    ws = H.empty(_lib.loo_workspace_bytes(n) // 8)
    resid, var = H.empty(n), H.empty(n)
    u, md = (H.empty(n), H.empty(n)) if grad else (None, None)
    if grad:
        out, g = H.loo(KERNEL_IDS[name], H.to_device(x), theta, alpha, alpha.shape[1], comp, A, work, ws, resid, var, u, md)
    else:
        out, g = H.loo(None, None, None, alpha, alpha.shape[1], comp, A, work, ws, resid, var, n=n)
    H.sync()
    host = lambda t: None if t is None else t.cpu().numpy()
    return out, g, host(resid), host(var), host(u), host(md), A


def bar_ratios(out, g, resid, var, u, md, ref):
    """the eight figures of a result (device, or the float64 twin of tests/test_loo_host.py) over their bars, against _reference's"""
    value, resid_r, var_r, grad_r, u_r, md_r = ref
    f = lambda a: np.asarray(a, dtype=np.float64)
    rel_max = lambda got, want: float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    return {
        "value": abs(out[0] - float(value)) / (1e-10 * abs(float(value))),
        "sum resid^2": abs(out[1] - float(np.sum(resid_r ** 2))) / (1e-10 * float(np.sum(resid_r ** 2))),
        "sum log q": abs(out[2] + float(np.sum(np.log(var_r)))) / (1e-10 * float(np.sum(np.abs(np.log(var_r))))),
        "resid": rel_max(resid, f(resid_r)) / 1e-10,
        "var": rel_max(var, f(var_r)) / 1e-10,
        "grad": float(np.max(np.abs(g[:len(grad_r)] - f(grad_r)) / (1e-8 * np.abs(f(grad_r)) + 1e-9 * np.max(np.abs(f(grad_r)))))),
        "u": rel_max(u, f(u_r)) / 1e-8,
        "diag M": rel_max(md, f(md_r)) / 1e-8,
    }


def _abi_case(H, name, n, d, ncol, comp):
    (x, ym, V, theta), ref = _reference(name, n, d, ncol, comp)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    out, g, resid, var, u, md, _ = _loo(H, name, x, theta, KV, alpha, comp)
    ratios = bar_ratios(out, g, resid, var, u, md, ref)
    for key, r in ratios.items():
        _report(f"{key} / bar", name, d, n, r)
    assert out[3] == 0
    assert g.shape == theta.shape
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{worst}: {ratios[worst]:.3g} times its bar"


@pytest.mark.parametrize("name,n,d,ncol,comp", ABI_CASES)
def test_abi_against_extended_precision(H, name, n, d, ncol, comp):
    _abi_case(H, name, n, d, ncol, comp)


@pytest.mark.parametrize("name,n,d,ncol,comp", FAMILY_CASES)
def test_abi_against_extended_precision_every_instantiation(H, name, n, d, ncol, comp):
    """the same eight ratios under the same bars on the rest of the (kind, D) grid: with ABI_CASES every instantiation of the two-vector
    gradient trace (grad_trace_kernel<KIND, D, TWO = true>) runs, its interior, edge and diagonal tiles each"""
    _abi_case(H, name, n, d, ncol, comp)


def _lower_tile_mask(dim, np_):
    t = np.arange(dim) // 128
    m = t[:, None] >= t[None, :]
    m[np_:, :] = False
    m[:, np_:] = False
    return m


def test_value_only_call_and_determinism(H):
    """the value-only call gives the bits of the full call's values and leaves exactly what fvgp_hip_potri leaves; two full calls on
    fresh copies of the same factor agree in every bit of every output"""
    from fvgp_amd import _lib
    name, n, d = "matern32_ard", 300, 3
    (x, ym, V, theta), _ = _reference(name, n, d, 1, 0)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    full = _loo(H, name, x, theta, KV, alpha, 0)
    again = _loo(H, name, x, theta, KV, alpha, 0)
    for a, b in zip(full[:6], again[:6]):
        assert np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))
    out_v, g_v, resid_v, var_v, _, _, A_v = _loo(H, name, x, theta, KV, alpha, 0, grad=False)
    assert g_v is None
    assert np.array_equal(out_v[:3].view(np.int64), full[0][:3].view(np.int64)) and out_v[3] == 0
    assert np.array_equal(resid_v.view(np.int64), full[2].view(np.int64))
    assert np.array_equal(var_v.view(np.int64), full[3].view(np.int64))
    np_ = _lib.pad128(n)
    P = KV.clone()
    H.potri(P, n, H.empty(np_, np_))
    H.sync()
    mask = _lower_tile_mask(KV.shape[0], np_)
    assert np.array_equal(A_v.cpu().numpy()[mask].view(np.int64), P.cpu().numpy()[mask].view(np.int64))


# ---- facade -----------------------------------------------------------------------------------------------------------------------
def _noise(x, h):
    return h[3] * (0.01 + 0.01 * x[:, 0])


def _noise_grad(x, h):
    g = np.zeros((len(h), len(x)))
    g[3] = 0.01 + 0.01 * x[:, 0]
    return g


def _mean(x, h):
    return h[4] * np.sin(2.0 * x[:, 0])


def _mean_grad(x, h):
    g = np.zeros((len(h), len(x)))
    g[4] = np.sin(2.0 * x[:, 0])
    return g


def _gp(name, with_models=False, **kw):
    import fvgp_amd
    x, ym, V, theta = _inputs(name, 150, 2, seed=1234)
    y = ym[:, 0] + 0.25
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if with_models:
            hps = np.concatenate([theta, [1.3, 0.4]])
            gp = fvgp_amd.GP(x, y, init_hyperparameters=hps, kernel_function=name, noise_function=_noise, noise_function_grad=_noise_grad,
                             prior_mean_function=_mean, prior_mean_function_grad=_mean_grad, **kw)
        else:
            gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function=name, **kw)
    return gp, x, y, V, theta


@pytest.mark.parametrize("name", ["rbf_ard", "matern32_ard"])
def test_facade_predictions(name):
    gp, x, y, V, theta = _gp(name)
    value, m_loo, v_loo, _, _, _ = loo_ref.loo_closed(name, x, y - np.mean(y), V, theta, want_grad=False)
    m_ref = np.asarray(m_loo + np.mean(y), dtype=np.float64)
    v_ref = np.asarray(v_loo, dtype=np.float64)
    state = (gp.hyperparameters.copy(), gp.log_likelihood(), gp.posterior_mean(x[:7])["m(x)"].copy())
    p = gp.loo_predictions()
    scale_m, scale_v = np.max(np.abs(m_ref)), np.max(v_ref)
    _report("facade mean / bar", name, 2, 150, float(np.max(np.abs(p["m_loo"] - m_ref)) / (1e-10 * scale_m)))
    _report("facade var / bar", name, 2, 150, float(np.max(np.abs(p["v_loo"] - v_ref)) / (1e-10 * scale_v)))
    assert np.max(np.abs(p["m_loo"] - m_ref)) <= 1e-10 * scale_m
    assert np.max(np.abs(p["v_loo"] - v_ref)) <= 1e-10 * scale_v
    assert np.max(np.abs(p["v_loo_latent"] - (v_ref - V))) <= 1e-10 * scale_v
    np.testing.assert_allclose(p["loo_log_predictive"], float(value), rtol=1e-10)
    np.testing.assert_allclose(np.sum(p["log_predictive"]), float(value), rtol=1e-10)
    np.testing.assert_allclose(p["nlpd"], -float(value) / 150, rtol=1e-10)
    np.testing.assert_allclose(p["rmse"], float(np.sqrt(np.mean((y - m_ref) ** 2))), rtol=1e-10)
    # None means the current hyperparameters; another theta is evaluated on the scratch and leaves the state alone
    q = gp.loo_predictions(hyperparameters=gp.hyperparameters.copy())
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert gp.loo_log_predictive(theta * 1.1) != p["loo_log_predictive"]
    assert gp.neg_loo_log_predictive() == -p["loo_log_predictive"]
    assert np.array_equal(gp.hyperparameters, state[0]) and gp.log_likelihood() == state[1]
    assert np.array_equal(gp.posterior_mean(x[:7])["m(x)"], state[2])


def test_facade_gradient_with_noise_and_mean_models():
    """hyperparameters [sigma^2, l_1, l_2, a, b] with V = a (0.01 + 0.01 x_0) and m = b sin(2 x_0): the reference differentiates both by hand"""
    name = "rbf_ard"
    gp, x, y, _, theta = _gp(name, with_models=True)
    hps = gp.hyperparameters.copy()
    r = y - _mean(x, hps)
    V = _noise(x, hps)
    value, _, _, gk, u, md = loo_ref.loo_closed(name, x, r, V, theta)
    alpha = loo_ref.spd_inverse(kf.k_ref(name, x, x, theta) + np.diag(V.astype(np.longdouble))) @ r.astype(np.longdouble)
    g_ref = np.concatenate([gk, [np.sum(_noise_grad(x, hps)[3] * (u * alpha - md)), np.sum(_mean_grad(x, hps)[4] * u)]])
    g_ref = -np.asarray(g_ref, dtype=np.float64)
    state = (hps.copy(), gp.log_likelihood(), gp.posterior_mean(x[:7])["m(x)"].copy())
    f, g = gp.neg_loo_log_predictive_and_gradient()
    ratio = float(np.max(np.abs(g - g_ref) / (1e-8 * np.abs(g_ref) + 1e-9 * np.max(np.abs(g_ref)))))
    _report("facade gradient / bar", name, 2, 150, ratio)
    assert ratio <= 1.0
    np.testing.assert_allclose(f, -float(value), rtol=1e-10)
    assert np.array_equal(g, gp.neg_loo_log_predictive_gradient(hps))
    assert np.array_equal(gp.hyperparameters, state[0]) and gp.log_likelihood() == state[1]
    assert np.array_equal(gp.posterior_mean(x[:7])["m(x)"], state[2])


def test_facade_kernel_callable():
    """values and predictions work through the value-only call; the gradient names its alternative"""
    import fvgp_amd
    from fvgp_amd import kernels
    native, x, y, V, theta = _gp("rbf_ard")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function=lambda a, b, h: kernels.rbf_ard(a, b, h))
    np.testing.assert_allclose(gp.loo_log_predictive(), native.loo_log_predictive(), rtol=1e-10)
    np.testing.assert_allclose(gp.loo_predictions()["m_loo"], native.loo_predictions()["m_loo"], rtol=0, atol=1e-9)
    with pytest.raises(NotImplementedError, match="named kernels"):
        gp.neg_loo_log_predictive_gradient()


def test_fvgp_has_one_term_per_point_and_task():
    import fvgp_amd
    rng = np.random.default_rng(77)
    x = rng.random((40, 2))
    y = np.stack([np.sin(3.0 * x.sum(axis=1) + 0.3 * t) + 0.1 * rng.standard_normal(40) for t in range(4)], axis=1)
    nv = rng.uniform(0.01, 0.02, (40, 4))
    theta = np.array([1.2, 0.4, 0.5, 2.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function="rbf_ard")
    value = loo_ref.loo_closed("rbf_ard", gp.x_data, gp.y_data[:, 0] - np.mean(gp.y_data), gp.noise_variances, theta, want_grad=False)[0]
    p = gp.loo_predictions()
    assert p["m_loo"].shape == (160,) and p["log_predictive"].shape == (160,)
    np.testing.assert_allclose(p["loo_log_predictive"], float(value), rtol=1e-10)


# ---- training ---------------------------------------------------------------------------------------------------------------------
BOUNDS = np.array([[0.1, 10.0], [0.05, 5.0], [0.05, 5.0]])


@pytest.mark.parametrize("method,kw", [("adam", {"max_iter": 30}), ("local", {})])
def test_training_on_the_loo_objective(method, kw):
    gp, _, _, _, theta = _gp("rbf_ard", args={"training_objective": "loo"})
    start = gp.neg_loo_log_predictive()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hps = gp.train(hyperparameter_bounds=BOUNDS, method=method, **kw)
    assert np.all(hps >= BOUNDS[:, 0]) and np.all(hps <= BOUNDS[:, 1])
    assert np.array_equal(hps, gp.hyperparameters)
    end = gp.neg_loo_log_predictive()
    _report(f"train {method}: -L_LOO start -> end", "rbf_ard", 2, 150, end - start)
    assert end <= start


def test_training_mcmc_and_refusals():
    gp, _, _, _, theta = _gp("rbf_ard", args={"training_objective": "loo"})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hps = gp.train(hyperparameter_bounds=BOUNDS, method="mcmc", max_iter=50, seed=3)
    assert hps.shape == (3,) and np.array_equal(hps, gp.hyperparameters)
    assert np.all(hps >= BOUNDS[:, 0]) and np.all(hps <= BOUNDS[:, 1])
    multi, _, _, _, _ = _gp("rbf_ard", args={"training_objective": "loo", "adam_starts": 4})
    with pytest.raises(ValueError, match="adam_starts"):
        multi.train(hyperparameter_bounds=BOUNDS, method="adam", max_iter=5)
    pop, _, _, _, _ = _gp("rbf_ard", args={"training_objective": "loo", "batch_population": True})
    with pytest.raises(ValueError, match="batch_population"):
        pop.train(hyperparameter_bounds=BOUNDS, method="global", max_iter=2)
