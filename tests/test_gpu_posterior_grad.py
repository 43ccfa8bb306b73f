"""Exact posterior gradients in the prediction points (fvgp_hip_posterior_grad, Handle.posterior_grad, GP.posterior_gradients): the C
ABI against the host restatement kernels.kernel_dx within the summation bound, the facade against the Richardson derivative of the
REFERENCE's posterior (fixture G12) where the finite-difference methods fall short, bitwise independence of a point from the rest of
the call, the facade's semantics, and the time against the finite-difference pair."""
import time
import warnings

import numpy as np
import pytest

from conftest import load_golden, synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KERNELS = ["rbf_ard", "matern32_ard", "matern52_ard", "rbf_iso", "matern32_iso", "matern52_iso"]

# The facade tests hold every posterior path (single, chunked, CholInv: tests/test_gpu_facade.py) to 1e-10 sigma^2 (variance) and
# 1e-10 of the values' scale (mean) against the oracle; posterior_gradients is one more schedule of the same sums and is held to the
# same figure against posterior_mean / posterior_covariance.
POSTERIOR_PARITY = 1e-10


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def host_kernel(name, x1, x2, hps):
    from fvgp_amd import kernels as K
    hps = np.asarray(hps, dtype=np.float64)
    if name.endswith("_iso"):
        dist, length = K.get_distance_matrix(x1, x2), hps[1]
    else:
        dist, length = K.get_anisotropic_distance_matrix(x1, x2, hps[1:]), 1.0
    f = {"rbf": K.squared_exponential_kernel, "matern32": K.matern_kernel_diff1, "matern52": K.matern_kernel_diff2}[name.split("_")[0]]
    return hps[0] * f(dist, length)


def _richardson(fx, name, tag):
    vals, h = fx[f"{name}_{tag}_vals"], float(fx[f"{name}_{tag}_h"])
    return ((vals[:, 0] - 8.0 * vals[:, 1] + 8.0 * vals[:, 2] - vals[:, 3]) / (12.0 * h)).T, float(fx[f"{name}_{tag}_err"])


def _abi_case(H, name, n, d, P, ncol=1, component=0, n_dirs=None):
    """factor at a theta, W = KV^-1 k on the device, one Handle.posterior_grad call; everything back on the host"""
    from fvgp_amd import _lib
    kid = _lib.KERNEL_IDS[name]
    rng = np.random.default_rng(n * 7 + d)
    x = rng.random((n, d))
    y = np.stack([np.sin((3.0 + c) * x.sum(axis=1)) + 0.1 * rng.standard_normal(n) for c in range(ncol)], axis=1)
    theta = np.concatenate([[1.2], rng.uniform(0.3, 0.5, 1 if name.endswith("_iso") else d)])
    xp = rng.random((P, d))
    n_dirs = d if n_dirs is None else n_dirs
    npad, Pp = _lib.pad128(n), _lib.pad128(P)
    dim = _lib.loglik_dim(n, ncol)
    xd, xpd = H.to_device(x), H.to_device(xp)
    KV, alpha = H.empty(dim, dim), H.empty(npad, ncol)
    info = H.loglik(kid, xd, theta, H.to_device(np.full(n, 0.01)), H.to_device(y - y.mean()), KV, alpha)[3]
    assert info == 0
    W = H.empty(npad, Pp)
    H.kmat(kid, xd, xpd, theta, W, pad=_lib.PAD_ZERO)
    H.potrs_cols(KV, n, W, Pp)
    nbytes = _lib.posterior_grad_workspace_bytes(n, P, n_dirs)
    assert nbytes == -(-n // 256) * (2 + 2 * n_dirs) * P * 8
    work = H.empty(nbytes // 8)
    A, q, dm, dv = H.empty(P), H.empty(P), H.empty(P, n_dirs), H.empty(P, n_dirs)
    H.posterior_grad(kid, xd, theta, xpd, alpha, ncol, component, W, n_dirs, work, A, q, dm, dv)
    H.sync()
    out = {k: v.cpu().numpy() for k, v in (("A", A), ("q", q), ("dm", dm), ("dv", dv))}
    A2, dm2 = H.empty(P), H.empty(P, n_dirs)
    H.posterior_grad(kid, xd, theta, xpd, alpha, ncol, component, None, n_dirs, work, A2, None, dm2, None)
    H.sync()
    out["A_mean_only"], out["dm_mean_only"] = A2.cpu().numpy(), dm2.cpu().numpy()
    return x, xp, theta, alpha.cpu().numpy()[:n, component], W.cpu().numpy()[:n, :P], out


@pytest.mark.parametrize("name", KERNELS)
def test_abi_matches_kernel_dx_within_the_summation_bound(H, name):
    """Every output is a sum of N products term_i; a sum of N rounded terms in any order is within (N - 1) eps sum|term_i| of the exact
    one (the standard bound), and an entry of k or dk evaluated by two correct implementations differs by a few ulp of itself (the
    device's exp and rsq are good to about 1 ulp, the argument of exp carries the rounding of r^2): 32 eps sum|term_i| is allowed for
    that.  Bound: (N + 32) eps sum_i|term_i| per output, derived, not measured.  alpha and W are the device's own, downloaded.
    Sizes: n = 300 and 517 (not multiples of 128; 517 spans three slices of 256 rows), P = 1 and P = 130 (three waves' worth of points
    with a ragged last one), d = 2 and 3; with d = 3 only the two leading columns are differentiated in one case (n_dirs < d)."""
    from fvgp_amd import kernels as K
    for (n, d, P, nd) in ((300, 2, 1, None), (517, 3, 130, None), (517, 3, 1, 2), (128, 1, 130, None)):
        x, xp, theta, alpha, W, out = _abi_case(H, name, n, d, P, n_dirs=nd)
        nd = d if nd is None else nd
        k = host_kernel(name, xp, x, theta)                      # (P, N)
        dk = K.kernel_dx(name, xp, x, theta)[:nd]                # (nd, P, N)
        for tag, terms, got in (("A", k * alpha[None, :], out["A"]), ("q", k * W.T, out["q"]),
                                ("dm", np.transpose(dk * alpha[None, None, :], (1, 0, 2)), out["dm"]),
                                ("dv", np.transpose(-2.0 * dk * W.T[None, :, :], (1, 0, 2)), out["dv"])):
            want, bound = terms.sum(axis=-1), (n + 32) * EPS * np.abs(terms).sum(axis=-1)
            worst = float(np.max(np.abs(got - want) / bound))
            print(f"{name} n={n} d={d} P={P} {tag}: max |device - host| / bound = {worst:.3f}")
            assert got.shape == want.shape
            assert np.all(np.abs(got - want) <= bound), (name, n, d, P, tag, worst)
        # without W: the mean's two outputs alone, the same bits
        assert out["A_mean_only"].tobytes() == out["A"].tobytes() and out["dm_mean_only"].tobytes() == out["dm"].tobytes()


def test_abi_component_and_argument_errors(H):
    from fvgp_amd import _lib, kernels as K
    x, xp, theta, alpha1, W, out = _abi_case(H, "matern52_ard", 300, 2, 5, ncol=2, component=1)
    dk = K.kernel_dx("matern52_ard", xp, x, theta)
    terms = np.transpose(dk * alpha1[None, None, :], (1, 0, 2))
    assert np.all(np.abs(out["dm"] - terms.sum(axis=-1)) <= (300 + 32) * EPS * np.abs(terms).sum(axis=-1))
    xd, xpd = H.to_device(x), H.to_device(xp)
    al, Wd, work = H.zeros(384, 1), H.zeros(384, 128), H.empty(4096)
    A, q, dm, dv = H.empty(5), H.empty(5), H.empty(5, 2), H.empty(5, 2)
    with pytest.raises(_lib.HipExtensionError, match="-12"):
        H.posterior_grad(2, xd, theta, xpd, al, 1, 1, Wd, 2, work, A, q, dm, dv)
    with pytest.raises(_lib.HipExtensionError, match="-15"):
        H.posterior_grad(2, xd, theta, xpd, al, 1, 0, Wd, 3, work, A, q, dm, dv)
    with pytest.raises(_lib.HipExtensionError, match="-17"):
        H.posterior_grad(2, xd, theta, xpd, al, 1, 0, Wd, 2, H.empty(8), A, q, dm, dv)
    with pytest.raises(_lib.HipExtensionError, match="-14"):
        H.posterior_grad(2, xd, theta, xpd, al, 1, 0, H.zeros(384, 64), 2, work, A, q, dm, dv)
    with pytest.raises(_lib.HipExtensionError, match="-21"):
        H.posterior_grad(2, xd, theta, xpd, al, 1, 0, Wd, 2, work, A, q, dm, None)
    assert _lib.posterior_grad_workspace_bytes(0, 5, 2) == -1 and _lib.posterior_grad_workspace_bytes(10, 5, 17) == -1


def test_facade_matches_the_reference_richardson_where_finite_differences_do_not():
    """GP.posterior_gradients against the 4-point Richardson derivative of the REFERENCE's own posterior_mean / posterior_covariance
    (fixture G12: RBF and Matern-5/2, N = 256, d = 2, the G9 points).  Bound: 10 x the error estimate stored in the fixture (truncation
    h^4 F5 / 30 + round-off 1.5 delta / h of the Richardson value itself; the margin of 10 is for the device factor's own rounding).
    The existing finite-difference methods (kernel step 1e-8) miss that bound on the same inputs -- the gap this method closes --
    while both stay within the tolerances test_gpu_facade.py holds the finite-difference methods to against G9 / G9m."""
    import fvgp_amd
    fx = load_golden("G12_posterior_grad_richardson.npz")
    x, y, nv, th, xp = fx["x"], fx["y"], fx["noise_variances"], fx["theta"], fx["x_pred"]
    for name in ("rbf_ard", "matern52_ard"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function=name)
        r = gp.posterior_gradients(xp)
        assert r["dm/dx"].shape == (10, 2) and r["dv/dx"].shape == (10, 2) and r["m(x)"].shape == (10,) and r["v(x)"].shape == (10,)
        assert np.max(np.abs(r["m(x)"] - fx[f"{name}_m_0"])) <= 1e-10 and np.max(np.abs(r["v(x)"] - fx[f"{name}_v_0"])) <= 1e-10
        fd = {"m": gp.posterior_mean_grad(xp)["dm/dx"], "v": gp.posterior_covariance_grad(xp)["dv/dx"]}
        for tag in ("m", "v"):
            truth, err = _richardson(fx, name, tag)
            e_new = float(np.max(np.abs(r[f"d{tag}/dx"] - truth)))
            e_fd = float(np.max(np.abs(fd[tag] - truth)))
            print(f"{name} d{tag}/dx: bound {10 * err:.3e}; posterior_gradients off by {e_new:.3e}, finite differences by {e_fd:.3e}")
            assert e_new <= 10.0 * err
            assert e_fd > 10.0 * err
    # the reference's own finite-difference outputs (G9, G9m), within the tolerances of test_finite_difference_derivatives_match_the_reference
    f9 = load_golden("G9_derivatives_rbf_n256_d2.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(f9["x"], f9["y"], init_hyperparameters=f9["theta"], noise_variances=f9["noise_variances"], kernel_function="rbf_ard")
    r = gp.posterior_gradients(f9["x_pred"])
    np.testing.assert_allclose(r["dm/dx"], f9["dm_all"], rtol=0, atol=2e-5 * np.max(np.abs(f9["dm_all"])))
    np.testing.assert_allclose(r["dv/dx"], f9["dv_all"], rtol=0, atol=5e-5 * np.max(np.abs(f9["dS_dir0"])))
    np.testing.assert_allclose(gp.posterior_gradients(f9["x_pred"], hyperparameters=f9["theta2"])["dm/dx"], f9["dm_theta2"], rtol=0,
                               atol=2e-5 * np.max(np.abs(f9["dm_all"])))
    fm = load_golden("G9m_derivatives_fvgp_4x64.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = fvgp_amd.fvGP(fm["fvgp_x"], fm["fvgp_y"], init_hyperparameters=fm["theta"], noise_variances=fm["fvgp_noise"])
    r = gm.posterior_gradients(fm["x_pred"], x_out=fm["x_out"])
    assert r["dm/dx"].shape == fm["dm_all"].shape and r["dv/dx"].shape == fm["dv_all"].shape
    np.testing.assert_allclose(r["dm/dx"], fm["dm_all"], rtol=0, atol=2e-5 * np.max(np.abs(fm["dm_all"])))
    np.testing.assert_allclose(r["dv/dx"], fm["dv_all"], rtol=0, atol=5e-5 * np.max(np.abs(fm["dS_dir1"])))


def test_a_point_does_not_depend_on_the_rest_of_the_call():
    """The four outputs of a point are bitwise the same asked for alone, inside a 1000-point call and in a 4100-point call that is cut
    at the 4096-point chunk boundary (one point on each side of the cut): the data rows are split by n alone, every sum has a fixed
    order, and the solve runs every product on one launch shape.  m(x) and v(x) agree with posterior_mean / posterior_covariance within
    the parity the facade tests hold the posterior paths to."""
    import fvgp_amd
    n, d = 700, 3
    x, y = synth(n, d)
    th = np.array([1.1, 0.3, 0.35, 0.4])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard")
    xq = np.random.default_rng(3).random((4100, d))
    keys = ("m(x)", "v(x)", "dm/dx", "dv/dx")
    big = gp.posterior_gradients(xq)
    for j in (4095, 4097):
        alone = gp.posterior_gradients(xq[j:j + 1])
        mid = gp.posterior_gradients(xq[j - 500:j + 500])
        for k in keys:
            assert alone[k][0].tobytes() == mid[k][500].tobytes() == big[k][j].tobytes(), (j, k)
    pm = gp.posterior_mean(xq[:1000])["m(x)"]
    pv = gp.posterior_covariance(xq[:1000], variance_only=True)["v(x)"]
    em, ev = float(np.max(np.abs(big["m(x)"][:1000] - pm))), float(np.max(np.abs(big["v(x)"][:1000] - pv)))
    print(f"parity with posterior_mean {em:.3e} (bound {POSTERIOR_PARITY * np.max(np.abs(pm)):.3e}), "
          f"with posterior_covariance {ev:.3e} (bound {POSTERIOR_PARITY * th[0]:.3e})")
    assert em <= POSTERIOR_PARITY * np.max(np.abs(pm))
    assert ev <= POSTERIOR_PARITY * th[0]


def test_facade_semantics():
    import fvgp_amd
    n, d = 300, 2
    x, y = synth(n, d)
    nv = np.full(n, 0.01)
    th, th2 = np.array([1.0, 0.3, 0.4]), np.array([1.2, 0.35, 0.3])
    xp = np.random.default_rng(8).random((7, d))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard")
        gp2 = fvgp_amd.GP(x, y, init_hyperparameters=th2, noise_variances=nv, kernel_function="rbf_ard")
    keys = ("m(x)", "v(x)", "dm/dx", "dv/dx")
    # hyperparameters= : a scratch evaluation, the state untouched
    before = gp.posterior_gradients(xp)
    other = gp.posterior_gradients(xp, hyperparameters=th2)
    after = gp.posterior_gradients(xp)
    assert np.array_equal(gp.get_hyperparameters(), th)
    want = gp2.posterior_gradients(xp)
    for k in keys:
        assert before[k].tobytes() == after[k].tobytes()
        assert np.max(np.abs(other[k] - want[k])) <= 1e-9 * max(1.0, float(np.max(np.abs(want[k]))))
        assert np.max(np.abs(other[k] - before[k])) > 1e-4
    # variance=False skips the solve (the solve entry point is not called at all) and leaves the mean's outputs bit for bit
    calls = []
    real = gp._H.potrs_cols
    gp._H.potrs_cols = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        mo = gp.posterior_gradients(xp, variance=False)
        assert calls == []
        gp.posterior_gradients(xp)
        assert calls == [1]
    finally:
        gp._H.potrs_cols = real
    assert mo["v(x)"] is None and mo["dv/dx"] is None
    assert mo["m(x)"].tobytes() == before["m(x)"].tobytes() and mo["dm/dx"].tobytes() == before["dm/dx"].tobytes()
    # a user prior mean contributes its derivative (forward difference, step 1e-6), the default constant mean none
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gl = fvgp_amd.GP(x, y, init_hyperparameters=th, noise_variances=nv, kernel_function="rbf_ard",
                         prior_mean_function=lambda xx, hps: 0.5 * xx[:, 0] - 2.0 * xx[:, 1])
    rl = gl.posterior_gradients(xp)
    fd = gl.posterior_mean_grad(xp)["dm/dx"]
    assert np.max(np.abs(rl["dm/dx"] - fd)) <= 2e-5 * np.max(np.abs(fd))
    assert np.max(np.abs(rl["m(x)"] - gl.posterior_mean(xp)["m(x)"])) <= 1e-10
    # component with two columns of y
    y2 = np.stack([y, np.cos(4.0 * x.sum(axis=1))], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g2 = fvgp_amd.GP(x, y2, init_hyperparameters=th, noise_variances=nv, kernel_function="matern32_ard")
    pm = g2.posterior_mean(xp)["m(x)"]
    for c in (0, 1):
        rc = g2.posterior_gradients(xp, component=c)
        assert np.max(np.abs(rc["m(x)"] - pm[:, c])) <= POSTERIOR_PARITY * np.max(np.abs(pm))
        fdc = g2.posterior_mean_grad(xp, component=c)["dm/dx"]
        assert np.max(np.abs(rc["dm/dx"] - fdc)) <= 2e-5 * np.max(np.abs(fdc))
    assert np.max(np.abs(g2.posterior_gradients(xp, component=0)["dm/dx"] - g2.posterior_gradients(xp, component=1)["dm/dx"])) > 1e-3
    # fvGP: x_out shapes
    fm = load_golden("G9m_derivatives_fvgp_4x64.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = fvgp_amd.fvGP(fm["fvgp_x"], fm["fvgp_y"], init_hyperparameters=fm["theta"], noise_variances=fm["fvgp_noise"])
    Pm, Dm, No = len(fm["x_pred"]), fm["x_pred"].shape[1], len(fm["x_out"])
    r = gm.posterior_gradients(fm["x_pred"], x_out=fm["x_out"])
    assert r["dm/dx"].shape == (Pm, Dm, No) and r["dv/dx"].shape == (Pm, Dm, No)
    assert r["m(x)"].shape == (Pm, No) and r["v(x)"].shape == (Pm, No)
    assert np.max(np.abs(r["m(x)"] - gm.posterior_mean(fm["x_pred"], x_out=fm["x_out"])["m(x)"])) <= 1e-10
    assert gm.posterior_gradients(fm["x_pred"])["dm/dx"].shape == (Pm, Dm, No)         # x_out defaults to every task
    # what has no closed form or no single-device factor raises
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gh = fvgp_amd.GP(x[:50], y[:50], init_hyperparameters=th, noise_variances=nv[:50],
                         kernel_function=lambda a, b, h: host_kernel("rbf_ard", a, b, h))
        from scipy.linalg import cho_factor, cho_solve
        gc = fvgp_amd.GP(x[:50], y[:50], init_hyperparameters=th, noise_variances=nv[:50], kernel_function="rbf_ard",
                         linalg_mode=[lambda KV: cho_factor(KV, lower=True), lambda o, b: cho_solve(o, b),
                                      lambda o: 2.0 * np.sum(np.log(np.diag(o[0])))])
    with pytest.raises(NotImplementedError, match="posterior_mean_grad"):
        gh.posterior_gradients(xp)
    with pytest.raises(NotImplementedError, match="linalg_mode"):
        gc.posterior_gradients(xp)
    gp._sharded = True
    try:
        with pytest.raises(NotImplementedError, match="single-GPU"):
            gp.posterior_gradients(xp)
    finally:
        gp._sharded = False


def test_one_call_is_faster_than_the_finite_difference_pair():
    """N = 4000, d = 3, P = 1000: one posterior_gradients call against posterior_mean_grad(x) + posterior_covariance_grad(x), the path
    that gave these derivatives before, on the same build.  Every shape warmed up, the two sides alternating, each window bracketed by
    device synchronisations, best of five.  The analytic call's device passes are a subset of the pair's, so only ratio > 1 is asserted."""
    import torch
    import fvgp_amd
    n, d, P = 4000, 3, 1000
    x, y = synth(n, d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=np.array([1.0, 0.3, 0.3, 0.3]), noise_variances=np.full(n, 0.01), kernel_function="rbf_ard")
    xp = np.random.default_rng(4).random((P, d))

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def new():
        gp.posterior_gradients(xp)

    def pair():
        gp.posterior_mean_grad(xp)
        gp.posterior_covariance_grad(xp)
    new(); pair(); new(); pair()
    tn, tp = [], []
    for _ in range(5):
        tn.append(window(new)); tp.append(window(pair))
    print(f"N={n} d={d} P={P}: posterior_gradients {min(tn) * 1e3:.2f} ms (spread {(max(tn) - min(tn)) / min(tn):.2f}), "
          f"finite-difference pair {min(tp) * 1e3:.2f} ms (spread {(max(tp) - min(tp)) / min(tp):.2f}), ratio {min(tp) / min(tn):.2f}")
    assert min(tp) / min(tn) > 1.0
