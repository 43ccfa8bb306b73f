"""GP.remove_data / fvGP.remove_data: after the call the object answers as a GP built on the kept points does -- pinned to the
reference's golden vectors where a round trip ends on a golden data set, to a fresh GP elsewhere.  Tolerances are those of
test_rank_n_append_equals_refactorisation (tests/test_gpu_facade.py)."""
import pickle
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import load_golden
from oracle import fvgp_oracle as orc

pytestmark = pytest.mark.gpu

# the update route is what most of these tests are about: they state a threshold that admits their removal sets (20 of 532 points) and
# switch the cost model off, which at these sizes sends everything but trailing points to the refactorisation
UPDATE = {"remove_update_max_fraction": 0.25, "remove_update_cost_model": False}


def _quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **k)


def _interleave(fx, n_extra=20, seed=3):
    """the golden data with extra points at scattered positions -- the first, the last, both sides of rows 128 and 256 -- and the
    positions of the extras"""
    x, y, nv = fx["x"], fx["y"], fx["noise_variances"]
    n = len(x) + n_extra
    rng = np.random.default_rng(seed)
    fixed = [0, n - 1, 127, 128, 129, 255, 256, 257]
    rest = rng.choice(np.setdiff1d(np.arange(n), fixed), n_extra - len(fixed), replace=False)
    pos = np.sort(np.concatenate([fixed, rest]))
    extra = np.zeros(n, dtype=bool)
    extra[pos] = True
    xa = np.empty((n,) + x.shape[1:]); ya = np.empty((n,) + y.shape[1:]); nva = np.empty(n)
    xa[~extra], ya[~extra], nva[~extra] = x, y, nv
    xa[extra] = rng.uniform(x.min(axis=0), x.max(axis=0), (n_extra, x.shape[1]))
    ya[extra] = rng.standard_normal((n_extra,) + y.shape[1:]) * np.std(y)
    nva[extra] = np.mean(nv)
    return xa, ya, nva, pos


def _meets_fixture(gp, fx):
    np.testing.assert_allclose(gp.log_likelihood(), fx["loglik"], rtol=1e-10)
    np.testing.assert_allclose(np.diag(gp.Chol_factor), fx["L_diag"], rtol=1e-10)
    assert np.max(np.abs(gp.KVinvY - fx["KVinvY"])) <= 1e-8 * np.max(np.abs(fx["KVinvY"]))
    np.testing.assert_allclose(gp.posterior_mean(fx["x_pred"])["m(x)"], fx["pm"], rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(gp.posterior_covariance(fx["x_pred"])["S"] - fx["pS"])) <= 1e-10
    np.testing.assert_allclose(gp.log_likelihood(fx["thetas"][0]), fx["logliks"][0], rtol=1e-10)


def _same_as(gp, fresh, xp, theta2=None):
    assert gp.point_number == fresh.point_number and np.array_equal(gp.x_data, fresh.x_data) and np.array_equal(gp.y_data, fresh.y_data)
    np.testing.assert_allclose(gp.log_likelihood(), fresh.log_likelihood(), rtol=1e-10)
    np.testing.assert_allclose(gp.logdet_KV, fresh.logdet_KV, rtol=1e-10)
    if fresh.Chol_factor is not None:
        np.testing.assert_allclose(np.diag(gp.Chol_factor), np.diag(fresh.Chol_factor), rtol=1e-10)
    assert np.max(np.abs(gp.KVinvY - fresh.KVinvY)) <= 1e-8 * np.max(np.abs(fresh.KVinvY))
    np.testing.assert_allclose(gp.posterior_mean(xp)["m(x)"], fresh.posterior_mean(xp)["m(x)"], rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(gp.posterior_covariance(xp)["S"] - fresh.posterior_covariance(xp)["S"])) <= 1e-10
    np.testing.assert_allclose(gp.m, fresh.m, rtol=1e-15)
    assert np.array_equal(gp.V, fresh.V)
    if theta2 is not None:
        np.testing.assert_allclose(gp.log_likelihood(theta2), fresh.log_likelihood(theta2), rtol=1e-10)


@pytest.mark.parametrize("name", ["G2_rbf_n512_d3.npz", "G6_rbf_2col_n300_d3.npz"])
def test_removing_interleaved_extras_lands_on_the_reference(name):
    import fvgp_amd
    fx = load_golden(name)
    xa, ya, nva, pos = _interleave(fx)
    gp = _quiet(fvgp_amd.GP, xa, ya, init_hyperparameters=fx["theta"], noise_variances=nva, kernel_function=str(fx["kernel"]), args=dict(UPDATE))
    ptr = gp._L.data_ptr()
    res = gp.remove_data(pos[::-1])                               # any order
    assert res["route"] == "update" and np.array_equal(res["removed"], pos) and len(res["kept"]) == len(fx["x"])
    assert gp._L.data_ptr() == ptr and gp.point_number == len(fx["x"])
    assert np.array_equal(gp.x_data, fx["x"]) and np.array_equal(gp.noise_variances, fx["noise_variances"])
    _meets_fixture(gp, fx)


def test_removal_refreshes_the_cholinv_inverse():
    import fvgp_amd
    fx = load_golden("G3_matern52_n512_d3.npz")
    xa, ya, nva, pos = _interleave(fx)
    gp = _quiet(fvgp_amd.GP, xa, ya, init_hyperparameters=fx["theta"], noise_variances=nva, kernel_function="matern52_ard",
                linalg_mode="CholInv", args=dict(UPDATE))
    assert gp.remove_data(pos)["route"] == "update"
    inv = np.linalg.inv(orc.addKV(orc.matern52_ard(fx["x"], fx["x"], fx["theta"]), fx["noise_variances"]))
    assert tuple(gp._KVinv.shape) == (512, 512)
    assert np.max(np.abs(gp._KVinv[:512, :512].cpu().numpy() - inv)) <= 1e-9 * np.max(np.abs(inv))
    pv = gp.posterior_covariance(fx["x_pred"], variance_only=True)
    assert pv["S"] is None and np.max(np.abs(pv["v(x)"] - fx["pv"])) <= 1e-10
    _meets_fixture(gp, fx)


def test_sliding_window_append_then_remove_oldest():
    import fvgp_amd
    fx = load_golden("G2_rbf_n512_d3.npz")
    x, y, nv, th = fx["x"], fx["y"], fx["noise_variances"], fx["theta"]
    n0, step = 260, 4
    gp = fvgp_amd.GP(x[:n0], y[:n0], init_hyperparameters=th, noise_variances=nv[:n0], kernel_function="rbf_ard", args=dict(UPDATE))
    for s in range(3):
        a = n0 + s * step
        gp.update_gp_data(x[a:a + step], y[a:a + step], noise_variances_new=nv[a:a + step])
        assert gp.remove_data(np.arange(step))["route"] == "update"
        assert gp.point_number == n0
    lo = 3 * step
    fresh = fvgp_amd.GP(x[lo:lo + n0], y[lo:lo + n0], init_hyperparameters=th, noise_variances=nv[lo:lo + n0], kernel_function="rbf_ard")
    _same_as(gp, fresh, fx["x_pred"], fx["thetas"][0])


def test_update_route_with_a_kernel_callable_and_with_matrix_noise():
    import fvgp_amd
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 200
    x, y, nv, th = fx["x"][:n], fx["y"][:n], fx["noise_variances"][:n], fx["theta"]
    R = np.array([0, 63, 64, 130, n - 1])
    keep = np.setdiff1d(np.arange(n), R)
    gp = _quiet(fvgp_amd.GP, x, y, init_hyperparameters=th, noise_variances=nv, kernel_function=orc.rbf_ard, args=dict(UPDATE))
    assert gp.remove_data(R)["route"] == "update"
    fresh = _quiet(fvgp_amd.GP, x[keep], y[keep], init_hyperparameters=th, noise_variances=nv[keep], kernel_function=orc.rbf_ard)
    _same_as(gp, fresh, fx["x_pred"], fx["thetas"][0])
    # a 2-d noise model: V[S,S] of the kept points is what the function gives on them (products only: the same bits)
    noise = lambda xx, h: 0.02 * np.eye(len(xx)) + 1e-3 * np.outer(xx[:, 0], xx[:, 0])
    gp = _quiet(fvgp_amd.GP, x, y, init_hyperparameters=th, noise_function=noise, kernel_function="rbf_ard", args=dict(UPDATE))
    assert np.ndim(gp.V) == 2
    assert gp.remove_data(R)["route"] == "update"
    fresh = _quiet(fvgp_amd.GP, x[keep], y[keep], init_hyperparameters=th, noise_function=noise, kernel_function="rbf_ard")
    _same_as(gp, fresh, fx["x_pred"], fx["thetas"][0])


def test_fall_back_routes_refactor():
    import fvgp_amd
    from fvgp_amd.gp_update import REMOVE_UPDATE_MAX_FRACTION
    # the default noise rule follows mean|y|: the noise of the kept points changes with the removal
    fx = load_golden("G4_default_n256_d2.npz")
    R = np.array([3, 128, 200])
    keep = np.setdiff1d(np.arange(len(fx["x"])), R)
    gp = _quiet(fvgp_amd.GP, fx["x"], fx["y"], init_hyperparameters=fx["theta"], args=dict(UPDATE))
    assert gp.remove_data(R)["route"] == "refactor"
    _same_as(gp, _quiet(fvgp_amd.GP, fx["x"][keep], fx["y"][keep], init_hyperparameters=fx["theta"]), fx["x_pred"])
    # user linear algebra: the factor is the user's object
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 200
    x, y, nv, th = fx["x"][:n], fx["y"][:n], fx["noise_variances"][:n], fx["theta"]
    calls = [lambda KV: sla.cho_factor(KV, lower=True), lambda f, b: sla.cho_solve(f, b), lambda f: 2.0 * np.sum(np.log(np.diag(f[0])))]
    keep = np.setdiff1d(np.arange(n), R[:2])
    gp = _quiet(fvgp_amd.GP, x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard", linalg_mode=calls, args=dict(UPDATE))
    assert gp.remove_data(R[:2])["route"] == "refactor"
    _same_as(gp, _quiet(fvgp_amd.GP, x[keep], y[keep], init_hyperparameters=th, noise_variances=nv[keep], kernel_function="rbf_ard",
                        linalg_mode=calls), fx["x_pred"])
    # more points than the threshold admits (the default one)
    k = int(REMOVE_UPDATE_MAX_FRACTION * n) + 1
    assert 0 < k < n
    gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard", args={"remove_update_cost_model": False})
    assert k > gp.args.get("remove_update_max_fraction", REMOVE_UPDATE_MAX_FRACTION) * n
    res = gp.remove_data(np.arange(k))
    assert res["route"] == "refactor"
    _same_as(gp, fvgp_amd.GP(x[k:], y[k:], init_hyperparameters=th, noise_variances=nv[k:], kernel_function="rbf_ard"), fx["x_pred"])


def test_default_cost_model_keeps_the_update_for_where_it_is_faster():
    """at a few hundred points a refactorisation costs less than the chain of diagonal steps behind an old point, while trailing points
    leave without any update: the defaults route accordingly, and both routes give the same GP"""
    import fvgp_amd
    from fvgp_amd.gp_update import refactor_ms, update_ms
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 300
    x, y, nv, th = fx["x"][:n], fx["y"][:n], fx["noise_variances"][:n], fx["theta"]
    assert update_ms(n, np.arange(6)) > refactor_ms(n - 6) > update_ms(n, [n - 1])
    assert update_ms(20000, np.arange(4)) < refactor_ms(20000) < update_ms(20000, np.arange(64))
    gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard")
    assert gp.remove_data(np.arange(6))["route"] == "refactor"
    assert gp.remove_data([n - 8, n - 7])["route"] == "update"                 # the last two of the 294 that remain
    keep = np.arange(6, n - 2)
    _same_as(gp, fvgp_amd.GP(x[keep], y[keep], init_hyperparameters=th, noise_variances=nv[keep], kernel_function="rbf_ard"), fx["x_pred"])


def test_fvgp_removes_positions():
    import fvgp_amd
    fx = load_golden("G5n_fvgp_4x64_nan.npz")
    X, Y, NV = fx["fvgp_x"], fx["fvgp_y"], fx["fvgp_noise"]
    nan_pos = np.flatnonzero(np.isnan(Y).any(axis=1))
    assert len(nan_pos) >= 1
    pos = np.unique(np.concatenate([[0, 17, 40, 63], nan_pos[:1]]))
    assert len(pos) == 5
    keep = np.setdiff1d(np.arange(len(X)), pos)
    gp = _quiet(fvgp_amd.fvGP, X, Y, init_hyperparameters=fx["theta"], noise_variances=NV, args=dict(UPDATE))
    res = gp.remove_data(pos)
    assert res["route"] == "update" and np.array_equal(res["removed"], pos) and np.array_equal(res["kept"], keep)
    assert len(res["removed_rows"]) == int(np.sum(~np.isnan(Y[pos])))
    fresh = _quiet(fvgp_amd.fvGP, X[keep], Y[keep], init_hyperparameters=fx["theta"], noise_variances=NV[keep])
    assert gp.fvgp_x_data.shape == fresh.fvgp_x_data.shape and gp.fvgp_y_data.shape == fresh.fvgp_y_data.shape
    assert gp.fvgp_noise_variances.shape == fresh.fvgp_noise_variances.shape
    assert np.array_equal(gp.fvgp_x_data, X[keep]) and np.array_equal(gp.x_data, fresh.x_data)
    assert np.array_equal(gp.x_out, fresh.x_out) and gp.input_set_dim == fresh.input_set_dim == X.shape[1]
    np.testing.assert_allclose(gp.log_likelihood(), fresh.log_likelihood(), rtol=1e-10)
    for kw in ({}, {"x_out": fx["x_out"]}):
        a, b = gp.posterior_mean(fx["x_pred"], **kw), fresh.posterior_mean(fx["x_pred"], **kw)
        assert a["m(x)"].shape == b["m(x)"].shape == (len(fx["x_pred"]), 4)
        np.testing.assert_allclose(a["m(x)"], b["m(x)"], rtol=1e-8, atol=1e-10)


def test_no_op_mask_and_errors_leave_the_object_alone():
    import fvgp_amd
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 300
    x, y, nv, th = fx["x"][:n], fx["y"][:n], fx["noise_variances"][:n], fx["theta"]
    make = lambda: fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard", args=dict(UPDATE))
    gp = make()
    L0, a0, ll0 = gp._L.clone(), gp._alpha.clone(), gp.log_likelihood()

    def untouched():
        import torch
        return (gp.point_number == n and len(gp.x_data) == n and torch.equal(torch.tril(gp._L), torch.tril(L0)) and torch.equal(gp._alpha, a0)
                and gp.log_likelihood() == ll0)
    for empty in ([], np.zeros(0, dtype=np.int64), np.zeros(n, dtype=bool)):
        res = gp.remove_data(empty)
        assert res["route"] is None and len(res["removed"]) == 0 and np.array_equal(res["kept"], np.arange(n))
        assert untouched()
    for bad, err in (([1, n], IndexError), ([-1], IndexError), (np.arange(n), ValueError), (np.ones(n, dtype=bool), ValueError),
                     (np.ones(n - 1, dtype=bool), ValueError), ([0.5], TypeError)):
        with pytest.raises(err):
            gp.remove_data(bad)
        assert untouched()
    # a boolean mask is the index form; duplicates collapse
    mask = np.zeros(n, dtype=bool)
    mask[[4, 130, 131]] = True
    other = make()
    r1, r2 = gp.remove_data(mask), other.remove_data([131, 4, 130, 4])
    assert r1["route"] == r2["route"] == "update" and np.array_equal(r1["removed"], r2["removed"]) and np.array_equal(r1["kept"], r2["kept"])
    assert np.array_equal(gp.KVinvY, other.KVinvY) and gp.log_likelihood() == other.log_likelihood()


def test_device_failure_after_the_factor_was_touched_restores_the_old_state():
    import fvgp_amd
    from fvgp_amd._lib import HipExtensionError
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 300
    x, y, nv, th = fx["x"][:n], fx["y"][:n], fx["noise_variances"][:n], fx["theta"]
    gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard", args=dict(UPDATE))
    ll0, a0, pm0 = gp.log_likelihood(), gp.KVinvY.copy(), gp.posterior_mean(fx["x_pred"])["m(x)"].copy()
    H = gp._H
    real = H.potrs

    def boom(*a, **k):
        raise HipExtensionError("injected failure after the factor was updated")
    try:
        H.potrs = boom
        with pytest.raises(HipExtensionError, match="injected"):
            gp.remove_data([2, 129])
    finally:
        H.potrs = real
    assert gp.point_number == n and np.array_equal(gp.x_data, x) and len(gp.noise_variances) == n
    np.testing.assert_allclose(gp.log_likelihood(), ll0, rtol=1e-10)
    assert np.max(np.abs(gp.KVinvY - a0)) <= 1e-8 * np.max(np.abs(a0))
    np.testing.assert_allclose(gp.posterior_mean(fx["x_pred"])["m(x)"], pm0, rtol=1e-8, atol=1e-10)
    # ... and the removal still works afterwards
    assert gp.remove_data([2, 129])["route"] == "update"
    keep = np.setdiff1d(np.arange(n), [2, 129])
    _same_as(gp, fvgp_amd.GP(x[keep], y[keep], init_hyperparameters=th, noise_variances=nv[keep], kernel_function="rbf_ard"), fx["x_pred"])


def test_pickle_after_a_removal():
    import fvgp_amd
    fx = load_golden("G2_rbf_n512_d3.npz")
    n = 300
    gp = fvgp_amd.GP(fx["x"][:n], fx["y"][:n], init_hyperparameters=fx["theta"], noise_variances=fx["noise_variances"][:n],
                     kernel_function="rbf_ard", args=dict(UPDATE))
    assert gp.remove_data([0, 128, 299])["route"] == "update"
    pm = gp.posterior_mean(fx["x_pred"])["m(x)"]
    gp2 = pickle.loads(pickle.dumps(gp))
    assert gp2.point_number == n - 3
    assert np.array_equal(gp2.posterior_mean(fx["x_pred"])["m(x)"], pm)
    np.testing.assert_allclose(gp2.log_likelihood(fx["thetas"][0]), gp.log_likelihood(fx["thetas"][0]), rtol=1e-12)
