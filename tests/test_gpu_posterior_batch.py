"""Batched posterior over hyperparameter ensembles (fvgp_hip_posterior_batch, Handle.posterior_batch, GP.posterior_mean_batch /
posterior_covariance_batch / posterior_mixture): the reference's posterior at every row, parity with the single path, bitwise parity of
the likelihood values with the batched log-likelihood, batch and chunk independence, edges, argument errors, the facade's semantics
and the speed against sequential single evaluations."""
import time
import warnings

import numpy as np
import pytest

from conftest import load_golden, synth
from oracle import fvgp_oracle as orc

pytestmark = pytest.mark.gpu

KERNELS = ["rbf_ard", "matern32_ard", "matern52_ard", "rbf_iso", "matern32_iso", "matern52_iso"]

# Largest relative difference between Handle.posterior_batch and Handle.loglik + Handle.posterior at the same theta over the six
# kernels of test_posterior_batch_all_kernels_match_single, measured on an MI355X (relative to max |mean| per row, and to sigma^2 for
# the variance and S): mean 1.4e-13, variance and S 4.3e-15 (profiles/r09_posterior_batch.txt).  The two are
# different schedules of the same sums; the test asserts ten times the measured figure.
SINGLE_PARITY_MEAN = 10 * 1.4e-13
SINGLE_PARITY_VAR = 10 * 4.3e-15


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


def _pbatch(H, kernel, x, thetas, V, ym, xp, pc=None, want_S=True, want_loglik=False):
    """one Handle.posterior_batch call -> dict of host arrays (S cut to P x P, Sfull the padded squares)"""
    from fvgp_amd import _lib
    n, ncol = x.shape[0], ym.shape[-1]
    dim, B, P = _lib.loglik_batch_dim(n, ncol), len(thetas), len(xp)
    pc = _lib.pad128(P) if pc is None else pc
    KV = H.empty(B, dim + pc, dim)
    mean, var = H.empty(B, P, ncol), H.empty(B, P)
    S = H.empty(B, _lib.pad128(P), _lib.pad128(P)) if want_S else None
    out, info = H.posterior_batch(_lib.KERNEL_IDS[kernel], H.to_device(x), np.asarray(thetas), H.to_device(V), H.to_device(ym),
                                  H.to_device(xp), KV, mean, var, S, want_loglik=want_loglik)
    r = {"mean": mean.cpu().numpy(), "var": var.cpu().numpy(), "out": out, "info": info}
    if want_S:
        r["Sfull"] = S.cpu().numpy()
        r["S"] = r["Sfull"][:, :P, :P]
    return r


def _single(H, kernel, x, theta, V, ym, xp):
    """Handle.loglik + Handle.posterior at one theta: (mean (P, ncol), var (P,), S (P, P))"""
    from fvgp_amd import _lib
    n, ncol = ym.shape
    P, dim, npd = len(xp), _lib.loglik_dim(n, ncol), _lib.pad128(n)
    kid = _lib.KERNEL_IDS[kernel]
    KV, alpha = H.empty(dim, dim), H.empty(npd, ncol)
    ll, logdet, quad, info = H.loglik(kid, H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)
    assert info == 0
    Pp = _lib.pad128(P)
    kx, mean, var, S = H.empty(npd, Pp), H.empty(P, ncol), H.empty(P), H.empty(Pp, Pp)
    H.posterior(kid, H.to_device(x), theta, KV, alpha, ncol, H.to_device(xp), kx, mean, var, S)
    H.sync()
    return mean.cpu().numpy(), var.cpu().numpy(), S[:P, :P].cpu().numpy()


def _same(a, b, keys=("mean", "var", "S")):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def _gp(fx, name):
    import fvgp_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name.startswith("G4"):
            return fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"])
        return fvgp_amd.GP(fx["x"], fx["y"], init_hyperparameters=fx["theta"], noise_variances=fx["noise_variances"],
                           kernel_function=str(fx["kernel"]))


def _oracle(fx, name):
    if name.startswith("G4"):
        return orc.OracleGP(fx["x"], fx["y"], fx["theta"])                    # default kernel and noise
    return orc.OracleGP(fx["x"], fx["y"], fx["theta"], fx["noise_variances"], kernel=str(fx["kernel"]))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G1_rbf_n500_d1.npz", "G2_rbf_n512_d3.npz", "G3_matern52_n512_d3.npz", "G4_default_n256_d2.npz",
                                  "G6_rbf_2col_n300_d3.npz"])
def test_posterior_batch_matches_reference(name):
    """through the facade, as test_gpu_facade builds these GPs; every one of the 8 rows against the oracle at that theta with the
    single posterior's tolerances, row 0 also against the stored fixture vectors"""
    fx = load_golden(name)
    gp, o = _gp(fx, name), _oracle(fx, name)
    th = np.vstack([fx["theta"], _thetas(fx["theta"], 7, 1)])
    xp = fx["x_pred"]
    pm = gp.posterior_mean_batch(xp, th)
    pc = gp.posterior_covariance_batch(xp, th)
    pv = gp.posterior_covariance_batch(xp, th, variance_only=True)
    assert set(pm) == {"x", "x_pred", "hyperparameters", "m(x)", "m(x)_flat"}
    assert set(pc) == {"x", "x_pred", "hyperparameters", "v(x)", "S"}
    assert pm["m(x)"].shape == (8,) + fx["pm"].shape and pm["m(x)_flat"].shape == (8,) + fx["pm_flat"].shape
    assert pc["v(x)"].shape == (8,) + fx["pv"].shape and pc["S"].shape == (8,) + fx["pS"].shape and pv["S"] is None
    for b in range(8):
        o.set_hyperparameters(th[b])
        rm, rc = o.posterior_mean(xp), o.posterior_covariance(xp)
        tol = 1e-10 * th[b, 0] + 1e-12
        dm = np.max(np.abs(pm["m(x)"][b] - rm["m(x)"]))
        ds, dv, dvo = (np.max(np.abs(pc["S"][b] - rc["S"])), np.max(np.abs(pc["v(x)"][b] - rc["v(x)"])),
                       np.max(np.abs(pv["v(x)"][b] - rc["v(x)"])))
        print(f"{name} row {b}: max|dm| {dm:.3e}  max|dS| {ds:.3e} max|dv| {dv:.3e} (variance only {dvo:.3e})  tol {tol:.3e}")
        np.testing.assert_allclose(pm["m(x)"][b], rm["m(x)"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(pm["m(x)_flat"][b], rm["m(x)_flat"], rtol=1e-8, atol=1e-10)
        assert ds <= tol and dv <= tol and dvo <= tol
    sig = fx["theta"][0]
    np.testing.assert_allclose(pm["m(x)"][0], fx["pm"], rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(pc["v(x)"][0] - fx["pv"])) <= 1e-10 * sig + 1e-12
    assert np.max(np.abs(pc["S"][0] - fx["pS"])) <= 1e-10 * sig + 1e-12
    assert np.max(np.abs(pv["v(x)"][0] - fx["pv"])) <= 1e-10 * sig + 1e-12


def test_posterior_batch_many_points_match_reference():
    """more than one tile of prediction points: synth(1000, 3), P = 300 uniform points, B = 4"""
    import fvgp_amd
    x, y = synth(1000, 3)
    nv = np.full(1000, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    xp = np.random.default_rng(3).random((300, 3))
    th = np.vstack([theta, _thetas(theta, 3, 1)])
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function="rbf_ard")
    o = orc.OracleGP(x, y, theta, nv, kernel="rbf_ard")
    pm, pc = gp.posterior_mean_batch(xp, th), gp.posterior_covariance_batch(xp, th)
    pv = gp.posterior_covariance_batch(xp, th, variance_only=True)
    for b in range(4):
        o.set_hyperparameters(th[b])
        rm, rc = o.posterior_mean(xp), o.posterior_covariance(xp)
        tol = 1e-10 * th[b, 0] + 1e-12
        print(f"synth1000 row {b}: max|dm| {np.max(np.abs(pm['m(x)'][b] - rm['m(x)'])):.3e} max|dS| {np.max(np.abs(pc['S'][b] - rc['S'])):.3e} tol {tol:.3e}")
        np.testing.assert_allclose(pm["m(x)"][b], rm["m(x)"], rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(pc["S"][b] - rc["S"])) <= tol
        assert np.max(np.abs(pc["v(x)"][b] - rc["v(x)"])) <= tol
        assert np.max(np.abs(pv["v(x)"][b] - rc["v(x)"])) <= tol


def test_posterior_batch_fvgp_multitask_reshape():
    """G5 (fvGP, x_out): shapes and values of the multi-task reshape, row 0 against the fixture, every row against the oracle"""
    import fvgp_amd
    fx = load_golden("G5_fvgp_4x64.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(fx["fvgp_x"], fx["fvgp_y"], init_hyperparameters=fx["theta"], noise_variances=fx["fvgp_noise"])
    o = orc.OracleGP(gp.x_data, gp.y_data, fx["theta"], gp.noise_variances, kernel="matern32_ard")
    xp, xo = fx["x_pred"], fx["x_out"]
    th = np.vstack([fx["theta"], _thetas(fx["theta"], 3, 1)])
    for kw in ({}, {"x_out": xo}):
        pm, pc = gp.posterior_mean_batch(xp, th, **kw), gp.posterior_covariance_batch(xp, th, **kw)
        assert pm["m(x)"].shape == (4, len(xp), 4) and pm["m(x)_flat"].shape == (4, 4 * len(xp))
        assert pc["S"].shape == (4, len(xp), len(xp), 4, 4) and pc["v(x)"].shape == (4, len(xp), 4)
        assert np.array_equal(pm["x_pred"], fx["pm_xpred"])
        np.testing.assert_allclose(pm["m(x)"][0], fx["pm"], rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(pc["S"][0] - fx["pS"])) <= 1e-10 and np.max(np.abs(pc["v(x)"][0] - fx["pv"])) <= 1e-10
        for b in range(4):
            o.set_hyperparameters(th[b])
            rm, rc = o.posterior_mean(xp, x_out=xo), o.posterior_covariance(xp, x_out=xo)
            tol = 1e-10 * th[b, 0] + 1e-12
            np.testing.assert_allclose(pm["m(x)"][b], rm["m(x)"], rtol=1e-8, atol=1e-10)
            assert np.max(np.abs(pc["S"][b] - rc["S"])) <= tol and np.max(np.abs(pc["v(x)"][b] - rc["v(x)"])) <= tol


# ---- the single path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_posterior_batch_all_kernels_match_single(H, kernel):
    x, y = synth(300, 2, seed=11)
    ym, V = _ym(y), np.full(300, 0.02)
    theta = np.array([1.3, 0.4, 0.25]) if kernel.endswith("ard") else np.array([1.3, 0.35])
    th = _thetas(theta, 8, 3)
    xp = np.random.default_rng(5).random((40, 2))
    r = _pbatch(H, kernel, x, th, V, ym, xp)
    assert np.all(r["info"] == 0)
    worst_m = worst_v = worst_s = 0.0
    for b in range(8):
        m, v, S = _single(H, kernel, x, th[b], V, ym, xp)
        worst_m = max(worst_m, float(np.max(np.abs(r["mean"][b] - m)) / np.max(np.abs(m))))
        worst_v = max(worst_v, float(np.max(np.abs(r["var"][b] - v)) / th[b, 0]))
        worst_s = max(worst_s, float(np.max(np.abs(r["S"][b] - S)) / th[b, 0]))
        # inside the reference tolerance in any case
        np.testing.assert_allclose(r["mean"][b], m, rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(r["var"][b] - v)) <= 1e-10 * th[b, 0] + 1e-12
        assert np.max(np.abs(r["S"][b] - S)) <= 1e-10 * th[b, 0] + 1e-12
    print(f"single parity {kernel}: mean {worst_m:.3e} var {worst_v:.3e} S {worst_s:.3e} (relative)")
    assert worst_m <= SINGLE_PARITY_MEAN and worst_v <= SINGLE_PARITY_VAR and worst_s <= SINGLE_PARITY_VAR


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def test_posterior_batch_loglik_bits(H):
    from fvgp_amd import _lib
    x, y = synth(2000, 3)
    ym, V = _ym(y), np.full(2000, 0.01)
    th = _thetas(np.array([1.0, 0.3, 0.3, 0.3]), 16, 7)
    xp = np.random.default_rng(2).random((200, 3))
    r = _pbatch(H, "rbf_ard", x, th, V, ym, xp, want_S=False, want_loglik=True)
    dim = _lib.loglik_batch_dim(2000, 1)
    vout, vinfo = H.loglik_batch(0, H.to_device(x), th, H.to_device(V), H.to_device(ym), H.empty(16, dim, dim))
    assert np.all(r["info"] == 0) and np.all(vinfo == 0)
    assert r["out"].tobytes() == vout.tobytes()


def test_posterior_batch_bitwise_independent(H):
    fx = load_golden("G1_rbf_n500_d1.npz")
    x, ym, V, xp = fx["x"], _ym(fx["y"]), fx["noise_variances"], fx["x_pred"]
    th = _thetas(fx["theta"], 64, 5)
    full = _pbatch(H, "rbf_ard", x, th, V, ym, xp)
    assert np.all(full["info"] == 0)
    assert _same(full, _pbatch(H, "rbf_ard", x, th, V, ym, xp))
    rev = _pbatch(H, "rbf_ard", x, th[::-1].copy(), V, ym, xp)
    assert all(rev[k][::-1].tobytes() == full[k].tobytes() for k in ("mean", "var", "S"))
    bad = th[2:3].copy()
    bad[0, 0] = -1.0
    mixed = _pbatch(H, "rbf_ard", x, np.vstack([th[:2], bad, th[2:5]]), V, ym, xp, want_loglik=True)
    assert mixed["info"][2] > 0 and np.all(np.isnan(mixed["mean"][2])) and np.all(np.isnan(mixed["var"][2]))
    assert np.all(np.isnan(mixed["Sfull"][2])) and np.all(np.isnan(mixed["out"][2]))
    keep = [0, 1, 3, 4, 5]
    assert np.all(mixed["info"][keep] == 0)
    assert all(mixed[k][keep].tobytes() == full[k][:5].tobytes() for k in ("mean", "var", "S"))
    rep = _pbatch(H, "rbf_ard", x, np.vstack([th[17:18]] * 3), V, ym, xp)
    for b in (0, 17, 63):
        alone = _pbatch(H, "rbf_ard", x, th[b:b + 1], V, ym, xp)
        assert all(alone[k][0].tobytes() == full[k][b].tobytes() for k in ("mean", "var", "S"))
    for r in range(3):
        assert all(rep[k][r].tobytes() == full[k][17].tobytes() for k in ("mean", "var", "S"))
    # S is bitwise symmetric, padding included
    assert full["Sfull"].tobytes() == np.ascontiguousarray(full["Sfull"].transpose(0, 2, 1)).tobytes()


def test_posterior_batch_point_chunks_same_bits(H):
    x, y = synth(700, 3)
    ym, V = _ym(y), np.full(700, 0.01)
    th = _thetas(np.array([1.0, 0.3, 0.3, 0.3]), 5, 9)
    xp = np.random.default_rng(4).random((300, 3))
    one = _pbatch(H, "matern52_ard", x, th, V, ym, xp, pc=384)
    for pc in (128, 256):
        parts = _pbatch(H, "matern52_ard", x, th, V, ym, xp, pc=pc, want_S=False)
        assert _same(parts, one, ("mean", "var"))
    # the variance is the diagonal of S to rounding, and S is symmetric
    assert np.max(np.abs(np.diagonal(one["S"], axis1=1, axis2=2) - one["var"])) <= 1e-12
    assert one["Sfull"].tobytes() == np.ascontiguousarray(one["Sfull"].transpose(0, 2, 1)).tobytes()


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def _ref_posterior(kernel, x, theta, V, ym, xp):
    """numpy / scipy: mean without the prior mean, S"""
    from scipy.linalg import cho_factor, cho_solve
    K = orc.KERNELS[kernel](x, x, theta) + np.diag(V)
    k = orc.KERNELS[kernel](x, xp, theta)
    c = cho_factor(K, lower=True)
    return k.T @ cho_solve(c, ym), orc.KERNELS[kernel](xp, xp, theta) - k.T @ cho_solve(c, k)


@pytest.mark.parametrize("n,ncol,d,P,B", [(300, 1, 2, 1, 3), (300, 1, 2, 129, 2), (256, 1, 3, 20, 3), (255, 1, 3, 20, 3), (257, 2, 3, 20, 3),
                                          (384, 8, 2, 17, 2), (383, 8, 2, 17, 2), (200, 1, 16, 9, 1), (1, 1, 1, 3, 2)])
def test_posterior_batch_edges(H, n, ncol, d, P, B):
    """P = 1 and P = 129, n = 128 k and 128 k +- 1 (the appended rows change place there), ncol = 8, B = 1, d = 16"""
    rng = np.random.default_rng(n + 7 * P)
    x = rng.random((n, d))
    ym = rng.standard_normal((n, ncol))
    ym -= ym.mean()
    V = np.full(n, 0.05)
    theta = np.array([1.2] + [0.5 * np.sqrt(d)] * d)
    th = _thetas(theta, B, 2)
    xp = rng.random((P, d))
    r = _pbatch(H, "rbf_ard", x, th, V, ym, xp)
    assert np.all(r["info"] == 0)
    for b in range(B):
        m, S = _ref_posterior("rbf_ard", x, th[b], V, ym, xp)
        np.testing.assert_allclose(r["mean"][b], m, rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(r["S"][b] - S)) <= 1e-10 * th[b, 0] + 1e-12
        assert np.max(np.abs(r["var"][b] - np.diag(S))) <= 1e-10 * th[b, 0] + 1e-12
    # padding of S is zero
    assert np.all(r["Sfull"][:, P:, :] == 0.0) and np.all(r["Sfull"][:, :, P:] == 0.0)


def test_posterior_batch_strided_targets_match_shared(H):
    """per-problem vdiag / ymean (strides n and n * ncol) against the shared ones, and really different targets per problem"""
    from fvgp_amd import _lib
    x, y = synth(300, 2, seed=4)
    ym, V = _ym(y), np.full(300, 0.02)
    th = _thetas(np.array([1.3, 0.4, 0.25]), 4, 3)
    xp = np.random.default_rng(6).random((10, 2))
    shared = _pbatch(H, "rbf_ard", x, th, V, ym, xp)
    own = _pbatch(H, "rbf_ard", x, th, np.stack([V] * 4), np.stack([ym] * 4), xp)
    assert _same(shared, own)
    Vs = np.stack([V * (1.0 + 0.5 * b) for b in range(4)])
    Ys = np.stack([ym * (1.0 - 0.2 * b) for b in range(4)])
    diff = _pbatch(H, "rbf_ard", x, th, Vs, Ys, xp)
    for b in range(4):
        alone = _pbatch(H, "rbf_ard", x, th[b:b + 1], Vs[b], Ys[b], xp)
        assert all(alone[k][0].tobytes() == diff[k][b].tobytes() for k in ("mean", "var", "S"))


def test_posterior_batch_argument_errors(H):
    """every documented argument error comes back with its number, nothing is launched"""
    import ctypes
    from fvgp_amd import _lib
    L = _lib.lib()
    n, d, P, B, ncol = 300, 2, 10, 2, 1
    dim = _lib.loglik_batch_dim(n, ncol)
    x, V, ym, xp = H.to_device(np.random.default_rng(0).random((n, d))), H.to_device(np.full(n, 0.1)), H.zeros(n, 1), H.zeros(P, d)
    KV, mean, var, S = H.zeros(B, dim + 128, dim), H.zeros(B, P, ncol), H.zeros(B, P), H.zeros(B, 128, 128)
    th = np.ascontiguousarray(np.tile([1.0, 0.3, 0.3], (B, 1)))
    tp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    p = _lib._ptr

    def call(**kw):
        a = dict(h=H._h, kid=0, x=p(x), n=n, d=d, th=tp, nt=3, B=B, vd=p(V), vds=0, ym=p(ym), yms=0, ncol=ncol, xp=p(xp), P=P,
                 KV=p(KV), rows=dim + 128, ld=dim, kvs=(dim + 128) * dim, mean=p(mean), var=p(var), S=p(S), lds=128, ss=128 * 128,
                 out=None, info=None)
        a.update(kw)
        return L.fvgp_hip_posterior_batch(*a.values())
    assert call() == 0
    odd = ctypes.c_void_p(KV.data_ptr() + 8)
    cases = [(dict(h=None), -1), (dict(x=None), -3), (dict(n=0), -4), (dict(n=5000), -4), (dict(n=4090, ncol=8), -4), (dict(th=None), -6),
             (dict(nt=2), -7), (dict(B=0), -8), (dict(vd=None), -9), (dict(vds=-1), -10), (dict(ym=None), -11), (dict(yms=-1), -12),
             (dict(ncol=0), -13), (dict(ncol=9), -13), (dict(xp=None), -14), (dict(P=0), -15), (dict(KV=None), -16), (dict(KV=odd), -16),
             (dict(rows=dim), -17), (dict(rows=dim + 64), -17), (dict(rows=dim + 129), -17), (dict(ld=dim - 2), -18), (dict(ld=dim + 1), -18),
             (dict(kvs=(dim + 128) * dim - 2), -19), (dict(kvs=(dim + 128) * dim + 1), -19), (dict(mean=None), -20),
             (dict(P=129), -22), (dict(S=ctypes.c_void_p(S.data_ptr() + 8)), -22), (dict(lds=126), -23), (dict(lds=129), -23),
             (dict(ss=128 * 128 - 2), -24), (dict(ss=128 * 128 + 1), -24)]
    mean.zero_(); var.zero_(); S.zero_(); KV.zero_()
    for kw, rc in cases:
        assert call(**kw) == rc, (kw, rc)
    assert call(P=129) == -22 and b"one chunk" in L.fvgp_hip_last_error_string()
    assert call(rows=dim) == -17 and b"kv_rows" in L.fvgp_hip_last_error_string()
    # nothing was launched by the refused calls
    H.sync()
    assert all(float(t.abs().sum()) == 0.0 for t in (mean, var, S, KV))
    assert call() == 0 and float(var.abs().sum()) > 0.0


# ---- the facade -------------------------------------------------------------------------------------------------------------------
def _state(gp):
    gp._H.sync()
    return (gp.hyperparameters.tobytes(), gp._L.cpu().numpy().tobytes(), gp._alpha.cpu().numpy().tobytes(),
            np.asarray(gp.KVinvY).tobytes(), gp.log_likelihood())


def _loop(gp, xp, th, x_out=None, variance_only=False, add_noise=False):
    """what the batch replaces: set_hyperparameters + posterior_* per row, on a copy of the GP's state"""
    keep = gp.hyperparameters.copy()
    ms, vs, Ss = [], [], []
    for t in th:
        gp.set_hyperparameters(np.asarray(t))
        ms.append(gp.posterior_mean(xp, x_out=x_out)["m(x)"])
        c = gp.posterior_covariance(xp, x_out=x_out, variance_only=variance_only, add_noise=add_noise)
        vs.append(c["v(x)"]); Ss.append(c["S"])
    gp.set_hyperparameters(keep)
    return np.stack(ms), np.stack(vs), np.stack(Ss)


def test_facade_state_untouched_and_rows_match_loop():
    fx = load_golden("G2_rbf_n512_d3.npz")
    gp = _gp(fx, "G2")
    th = np.vstack([fx["theta"], _thetas(fx["theta"], 5, 2)])
    xp = fx["x_pred"]
    m, v, S = _loop(gp, xp, th, add_noise=True)
    before = _state(gp)
    pm = gp.posterior_mean_batch(xp, th)
    pc = gp.posterior_covariance_batch(xp, th, add_noise=True)
    pv = gp.posterior_covariance_batch(xp, th, variance_only=True, add_noise=True)
    mix = gp.posterior_mixture(xp, th, add_noise=True)
    assert _state(gp) == before
    sig = np.max(th[:, 0])
    np.testing.assert_allclose(pm["m(x)"], m, rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(pc["v(x)"] - v)) <= 1e-10 * sig + 1e-12 and np.max(np.abs(pc["S"] - S)) <= 1e-10 * sig + 1e-12
    assert np.max(np.abs(pv["v(x)"] - v)) <= 1e-10 * sig + 1e-12 and pv["S"] is None
    # the mixture is the moment formula applied to the batched rows
    w = np.full(6, 1.0 / 6.0)
    mean = np.einsum("b,bp->p", w, pm["m(x)"])
    np.testing.assert_allclose(mix["m(x)"], mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(mix["v(x)"], np.einsum("b,bp->p", w, pv["v(x)"] + pm["m(x)"] ** 2) - mean ** 2, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(mix["v_within"] + mix["v_between"], mix["v(x)"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(mix["v_within"], np.einsum("b,bp->p", w, pv["v(x)"]), rtol=1e-13)
    w2 = np.arange(1.0, 7.0)
    mix2 = gp.posterior_mixture(xp, th, weights=w2)
    np.testing.assert_allclose(mix2["weights"], w2 / w2.sum(), rtol=1e-15)
    np.testing.assert_allclose(mix2["m(x)"], np.einsum("b,bp->p", w2 / w2.sum(), pm["m(x)"]), rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        gp.posterior_mixture(xp, th, weights=-w2)


def test_facade_chunking_returns_identical_arrays():
    import fvgp_amd
    x, y = synth(600, 2)
    theta = np.array([1.0, 0.3, 0.3])
    th = _thetas(theta, 7, 4)
    xp = np.random.default_rng(8).random((300, 2))

    def run(args):
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=np.full(600, 0.01), kernel_function="rbf_ard", args=args)
        return (gp.posterior_mean_batch(xp, th)["m(x)"], gp.posterior_covariance_batch(xp, th, variance_only=True)["v(x)"],
                gp.posterior_covariance_batch(xp[:100], th)["S"])
    dim = 640
    whole = run({})
    # two problems per call; then a budget below one problem's scratch: one by one, points in chunks of 128
    for budget in (2 * 8 * ((dim + 384) * dim + 300 * 2 + 128 * 128) + 64, 1000):
        part = run({"batch_max_bytes": budget})
        for a, b in zip(whole, part):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(NotImplementedError, match="posterior_chunk"):
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=np.full(600, 0.01), kernel_function="rbf_ard",
                         args={"posterior_chunk": 128})
        gp.posterior_covariance_batch(xp, th)


def test_facade_callables_depending_on_theta():
    """mean and noise callables that read theta are evaluated per row on the host; a kernel callable takes the one-by-one route"""
    import fvgp_amd
    x, y = synth(300, 2, seed=3)
    xp = np.random.default_rng(1).random((20, 2))

    def mean_fn(xx, hps):
        return hps[3] * np.ones(len(xx)) + 0.1 * xx[:, 0]

    def noise_fn(xx, hps):
        return np.full(len(xx), hps[4])
    theta = np.array([1.0, 0.3, 0.3, 0.2, 0.02])
    th = _thetas(theta, 5, 6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, kernel_function="rbf_ard", prior_mean_function=mean_fn, noise_function=noise_fn)
        m, v, S = _loop(gp, xp, th, add_noise=True)
        pm, pc = gp.posterior_mean_batch(xp, th), gp.posterior_covariance_batch(xp, th, add_noise=True)
        sig = np.max(th[:, 0])
        np.testing.assert_allclose(pm["m(x)"], m, rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(pc["v(x)"] - v)) <= 1e-10 * sig + 1e-12 and np.max(np.abs(pc["S"] - S)) <= 1e-10 * sig + 1e-12
        # a row whose noise is not a positive vector goes one by one, the others stay batched: same values as the loop
        def noise_mixed(xx, hps):
            return np.diag(np.full(len(xx), hps[4])) if hps[4] > theta[4] else np.full(len(xx), hps[4])
        gp2 = fvgp_amd.GP(x, y, init_hyperparameters=theta, kernel_function="rbf_ard", prior_mean_function=mean_fn, noise_function=noise_mixed)
        assert any(t[4] > theta[4] for t in th) and any(t[4] <= theta[4] for t in th)
        np.testing.assert_allclose(gp2.posterior_mean_batch(xp, th)["m(x)"], m, rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(gp2.posterior_covariance_batch(xp, th, variance_only=True)["v(x)"] - _loop(gp, xp, th)[1])) <= 1e-10 * sig + 1e-12
        # kernel callable: the fallback route gives the loop's values
        gpk = fvgp_amd.GP(x, y, init_hyperparameters=theta[:3], noise_variances=np.full(300, 0.02),
                          kernel_function=lambda a, b, h: orc.rbf_ard(a, b, h))
        thk = th[:3, :3]
        mk, vk, Sk = _loop(gpk, xp, thk)
        before = _state(gpk)
        np.testing.assert_allclose(gpk.posterior_mean_batch(xp, thk)["m(x)"], mk, rtol=1e-10, atol=1e-12)
        ck = gpk.posterior_covariance_batch(xp, thk)
        assert np.max(np.abs(ck["S"] - Sk)) <= 1e-10 and np.max(np.abs(ck["v(x)"] - vk)) <= 1e-10
        assert _state(gpk) == before


def test_facade_clipping_and_nonpd():
    """gp_posterior.py:248-259 per row: warn below -1e-4, clip to 0, write the clipped diagonal back into S (negative variances forced
    as tests/test_gpu_edge_cases.py forces them for the single path); a non-positive-definite row raises what the single call raises"""
    import fvgp_amd
    from fvgp_amd.gp_lin_alg import NonPositiveDefiniteError
    x, y = synth(300, 2, seed=5)
    theta = np.array([1.0, 0.6, 0.6])
    th = _thetas(theta, 4, 2)
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=np.full(300, 0.01), kernel_function="rbf_ard")
    xp = np.random.default_rng(8).random((6, 2))
    cleans = {vo: gp.posterior_covariance_batch(xp, th, variance_only=vo) for vo in (False, True)}
    real = gp._posterior_batch_core

    def inflated(*a):
        hp, x_orig, x_pred, x_out, A, v, S = real(*a)
        v[1] -= 10.0
        if S is not None:
            S[1] -= np.eye(len(xp)) * 10.0
        return hp, x_orig, x_pred, x_out, A, v, S
    gp._posterior_batch_core = inflated
    for variance_only in (False, True):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            pc = gp.posterior_covariance_batch(xp, th, variance_only=variance_only)
        clean = cleans[variance_only]
        assert any("Negative variances" in str(w.message) for w in caught)
        assert np.all(pc["v(x)"][1] == 0.0) and np.array_equal(pc["v(x)"][[0, 2, 3]], clean["v(x)"][[0, 2, 3]])
        if not variance_only:
            assert np.all(np.diag(pc["S"][1]) == 0.0)
            off = ~np.eye(len(xp), dtype=bool)
            assert np.array_equal(pc["S"][1][off], clean["S"][1][off]) and np.array_equal(pc["S"][[0, 2, 3]], clean["S"][[0, 2, 3]])
    gp._posterior_batch_core = real
    bad = th.copy()
    bad[1, 0] = -1.0
    with pytest.raises(NonPositiveDefiniteError) as e_batch:
        gp.posterior_mean_batch(xp, bad)
    with pytest.raises(NonPositiveDefiniteError) as e_single:
        gp.posterior_mean(xp, hyperparameters=bad[1])
    assert str(e_batch.value) == str(e_single.value)


# ---- speed ------------------------------------------------------------------------------------------------------------------------
def test_posterior_batch_not_slower_than_sequential(H):
    """N = 500, B = 64, P = 1000: one batched call (variance only, and with S) against B x (Handle.loglik + Handle.posterior) in this
    process, every shape warmed up, the two sides alternating, best of 5 synchronised windows"""
    import torch
    from fvgp_amd import _lib
    n, d, B, P = 500, 1, 64, 1000
    x, y = synth(n, d)
    ym, V = _ym(y), np.full(n, 0.01)
    th = _thetas(np.array([1.0, 0.3]), B, 1)
    xp = np.random.default_rng(0).random((P, d))
    xd, Vd, ymd, xpd = H.to_device(x), H.to_device(V), H.to_device(ym), H.to_device(xp)
    dim, npd, Pp = _lib.loglik_batch_dim(n, 1), _lib.pad128(n), _lib.pad128(P)
    KVb, mean, var, Sb = H.empty(B, dim + Pp, dim), H.empty(B, P, 1), H.empty(B, P), H.empty(B, Pp, Pp)
    KV1, alpha, kx, m1, v1, S1 = H.empty(dim, dim), H.empty(npd, 1), H.empty(npd, Pp), H.empty(P, 1), H.empty(P), H.empty(Pp, Pp)

    def batch(S):
        H.posterior_batch(0, xd, th, Vd, ymd, xpd, KVb, mean, var, S)

    def seq(S):
        for t in th:
            H.loglik(0, xd, t, Vd, ymd, KV1, alpha)
            H.posterior(0, xd, t, KV1, alpha, 1, xpd, kx, m1, v1 if S is None else None, S)
        H.sync()

    def window(fn, S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(S)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for with_S in (False, True):
        Sb_, S1_ = (Sb, S1) if with_S else (None, None)
        batch(Sb_); seq(S1_)
        tb, ts = [], []
        for _ in range(5):
            tb.append(window(batch, Sb_)); ts.append(window(seq, S1_))
        print(f"N=500 B=64 P=1000 {'with S' if with_S else 'variance only'}: batch {min(tb) * 1e3:.3f} ms, sequential {min(ts) * 1e3:.3f} ms, "
              f"x{min(ts) / min(tb):.2f}")
        assert min(tb) <= min(ts)
