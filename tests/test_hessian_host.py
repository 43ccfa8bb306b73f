"""The exact log-likelihood Hessian without a GPU: the extended-precision reference (tests/hessian_ref.py) against central differences
of the first derivatives it is built on, its float64 twin on every case the device test uses, the reference's own finite-difference
Hessian (fixture G9), the Laplace arithmetic, the choice of the Laplace / training case, and the ABI surface of fvgp_hip_loglik_hess."""
import ctypes

import numpy as np
import pytest

import hessian_ref as hr
import kernel_family_ref as kf
from conftest import load_golden

LD = np.longdouble


def _points(d, n=12, seed=0):
    """points from the unit cube with one duplicated point (rows 2 and 5); x against itself, so the diagonal is in"""
    rng = np.random.default_rng(100 * d + seed)
    x = rng.random((n, d))
    x[5] = x[2]
    return x


@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("name", hr.NAMES)
def test_second_derivatives_equal_central_differences_of_the_first(name, d):
    """relative step 1e-6 in longdouble, bar 1e-8 of the largest entry (truncation ~1e-12, rounding ~1e-13; measured: 3e-12)"""
    x = _points(d)
    theta = kf.case_theta(name, d, np.random.default_rng(d)).astype(LD)
    d2 = hr.d2k_dtheta2_ref(name, x, x, theta)
    nt = len(theta)
    assert d2.shape == (nt, nt, len(x), len(x))
    fd = np.empty_like(d2)
    for j in range(nt):
        h = LD(1e-6) * theta[j]
        tp, tm = theta.copy(), theta.copy()
        tp[j] += h
        tm[j] -= h
        fd[:, j] = (kf.dk_dtheta_ref(name, x, x, tp) - kf.dk_dtheta_ref(name, x, x, tm)) / (2 * h)
    err = float(np.max(np.abs(d2 - fd)) / np.max(np.abs(d2)))
    print(f"HESS|d2k vs central difference|{name}|{d}|{len(x)}|{err:.3g}")
    assert np.all(np.isfinite(d2.astype(np.float64)))
    assert np.all(d2[:, :, 2, 5] == 0) and np.all(d2[1:, 1:, np.arange(len(x)), np.arange(len(x))] == 0)   # coincident pairs: exactly 0
    assert err <= 1e-8
    assert np.array_equal(d2, np.transpose(d2, (1, 0, 2, 3)))


@pytest.mark.parametrize("name,d", [("rbf_ard", 2), ("matern32_iso", 3), ("matern52_ard", 3)])
def test_hessian_equals_central_difference_of_its_gradient(name, d):
    """n = 40, relative step 1e-6, bar 1e-8 max|H| (measured: 5e-12); H_ij and H_ji, built from T_i and T_j, agree far below it"""
    x, ym, V, theta = hr.case_inputs(name, 40, d, seed=13 * d + 1)
    g, raw = hr.nll_hessian_ref(name, x, ym[:, 0], V, theta)
    nt = len(theta)
    fd = np.empty((nt, nt), dtype=LD)
    for j in range(nt):
        h = LD(1e-6) * LD(theta[j])
        tp, tm = theta.astype(LD), theta.astype(LD)
        tp[j] += h
        tm[j] -= h
        fd[:, j] = (hr.nll_gradient_ref(name, x, ym[:, 0], V, tp) - hr.nll_gradient_ref(name, x, ym[:, 0], V, tm)) / (2 * h)
    scale = float(np.max(np.abs(raw)))
    err = float(np.max(np.abs(raw - fd))) / scale
    asym = float(np.max(np.abs(raw - raw.T))) / scale
    print(f"HESS|hessian vs central difference|{name}|{d}|40|{err:.3g} asymmetry {asym:.3g}")
    assert float(np.max(np.abs(g - hr.nll_gradient_ref(name, x, ym[:, 0], V, theta)))) <= 1e-17 * float(np.max(np.abs(g)))
    assert err <= 1e-8
    assert asym <= 1e-14


def test_family_cases_complete_the_grid():
    """ABI_CASES and FAMILY_CASES hold every (name, d) of the family grid, FAMILY_CASES each at n = 261 and none twice: 8 of the 15
    <KIND, D> cells before, 15 with the sweep"""
    have = [(c[0], c[2]) for c in hr.FAMILY_CASES]
    assert len(set(have)) == len(have) and all(c[1] == hr.FAMILY_N == 261 for c in hr.FAMILY_CASES)
    assert not set(have) & {(c[0], c[2]) for c in hr.ABI_CASES}
    assert set(have) | {(c[0], c[2]) for c in hr.ABI_CASES} == {(name, d) for name in kf.FAMILY for d in kf.DIMS}
    cells = lambda cases: {hr.cell(c[0], c[2])[:2] for c in cases}
    assert len(cells(hr.ABI_CASES)) == 8 and len(cells(hr.ABI_CASES + hr.FAMILY_CASES)) == 15


@pytest.mark.parametrize("name,n,d,ncol,comp,dup", hr.ABI_CASES + hr.FAMILY_CASES)
def test_float64_twin_sits_far_inside_the_device_bar(name, n, d, ncol, comp, dup):
    """the same formulas in float64 against longdouble on every case of the device tests: at most 1e-2 of the device's bar
    (|dH_ij| <= 1e-8 |H_ij| + 1e-9 max|H|, gradient alike), so the bar judges the device and not the conditioning of the case"""
    (x, ym, V, theta), (g, raw) = hr.reference(name, n, d, ncol, comp, dup)
    g64, raw64 = hr.nll_hessian_ref(name, x, ym[:, comp], V, theta, dtype=np.float64)
    f = lambda a: np.asarray(a, dtype=np.float64)
    rh = float(np.max(np.abs(raw64 - f(raw)) / hr.hessian_bar(raw)))
    rg = float(np.max(np.abs(g64 - f(g)) / hr.hessian_bar(g)))
    print(f"HESS|float64 twin / bar|{name}|{d}|{n}|hessian {rh:.3g} gradient {rg:.3g}")
    assert rh <= 1e-2 and rg <= 1e-2


def test_float64_twin_against_the_reference_finite_difference_hessian():
    """fixture G9 (rbf_ard, n = 256, d = 2): the reference's own forward-difference Hessian, at the bar tests/test_gpu_facade.py holds
    neg_log_likelihood_hessian to (1e-4 max|H|; measured: 0.05 of it).  y is centred: the default prior mean is mean(y)."""
    fx = load_golden("G9_derivatives_rbf_n256_d2.npz")
    y = fx["y"] - np.mean(fx["y"])
    g, raw = hr.nll_hessian_ref("rbf_ard", fx["x"], y, fx["noise_variances"], fx["theta"], dtype=np.float64)
    hs = float(np.max(np.abs(fx["hessian"])))
    err = float(np.max(np.abs(0.5 * (raw + raw.T) - fx["hessian"]))) / (1e-4 * hs)
    print(f"HESS|float64 twin vs G9 / bar|rbf_ard|2|256|{err:.3g}")
    assert err <= 1.0
    np.testing.assert_allclose(-g, fx["an_grad"], rtol=1e-8)          # the fixture holds the gradient of +log p


def test_laplace_arithmetic():
    from fvgp_amd.gp_hessian import laplace_from_hessian
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4, 4))
    H = A @ A.T + 4.0 * np.eye(4)
    theta, f = np.array([1.0, 2.0, 0.7, 1.5]), 12.5
    r = laplace_from_hessian(theta, f, H, n_samples=200, seed=3)
    assert set(r) == {"mean", "hessian", "covariance", "log_evidence", "samples"}
    assert np.max(np.abs(r["covariance"] @ H - np.eye(4))) <= 1e-12
    assert np.array_equal(r["covariance"], r["covariance"].T) and np.array_equal(r["mean"], theta)
    expect = -f + 2.0 * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(H)[1]
    assert abs(r["log_evidence"] - expect) <= 1e-12 * abs(expect)
    assert r["samples"].shape == (200, 4) and np.all(r["samples"] > 0.0)
    assert np.array_equal(r["samples"], laplace_from_hessian(theta, f, H, n_samples=200, seed=3)["samples"])
    assert not np.array_equal(r["samples"], laplace_from_hessian(theta, f, H, n_samples=200, seed=4)["samples"])
    # the draws have the covariance H^-1 (20 000 draws: the entries' standard error is about 1 % of the diagonal)
    big = laplace_from_hessian(theta, f, H, n_samples=20000, seed=1, bounds=np.array([[-50.0, 50.0]] * 4))["samples"]
    assert np.max(np.abs(np.cov(big.T) - r["covariance"])) <= 0.05 * np.max(np.diag(r["covariance"]))
    # bounds hold; no samples asked: an empty (0, H) block
    bounds = np.stack([theta - 0.3, theta + 0.3], axis=1)
    s = laplace_from_hessian(theta, f, H, n_samples=64, seed=0, bounds=bounds)["samples"]
    assert np.all(s >= bounds[:, 0]) and np.all(s <= bounds[:, 1])
    assert laplace_from_hessian(theta, f, H)["samples"].shape == (0, 4)
    # an indefinite Hessian is no minimum
    Hi = H.copy()
    Hi[0, 0] = -1.0
    with pytest.raises(ValueError, match="smallest eigenvalue.*not at a minimum of the negative log-likelihood"):
        laplace_from_hessian(theta, f, Hi)
    # bounds that the approximation cannot meet end after a bounded number of tries
    with pytest.raises(RuntimeError, match="outside the bounds"):
        laplace_from_hessian(theta, f, H, n_samples=4, bounds=np.stack([theta + 50.0, theta + 51.0], axis=1), max_tries=3)


def _nll64(x, y, V, theta):
    """-log p(y|theta) and its gradient in float64 for rbf_iso (the objective scipy minimises in the test below)"""
    K = kf.k_ref("rbf_iso", x, x, theta, np.float64) + np.diag(V)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    W = np.linalg.inv(K)
    dK = kf.dk_dtheta_ref("rbf_iso", x, x, theta, np.float64)
    B = W - np.outer(alpha, alpha)
    f = 0.5 * y @ alpha + np.sum(np.log(np.diag(L))) + 0.5 * len(x) * np.log(2.0 * np.pi)
    return f, np.array([0.5 * np.sum(B * dK[i]) for i in range(2)])


def test_laplace_case_has_an_interior_well_conditioned_minimum():
    """the case the device's Laplace / training test runs (hessian_ref.laplace_case), vetted here with the float64 twin and scipy: the
    minimiser lies strictly inside the bounds and lambda_min(H) > 1e-3 lambda_max(H); at LAPLACE_NOT_A_MINIMUM the Hessian has a
    negative eigenvalue"""
    from scipy.optimize import minimize
    x, y, V, bounds, start = hr.laplace_case()
    ym = y - np.mean(y)
    res = minimize(lambda t: _nll64(x, ym, V, t), start, jac=True, method="L-BFGS-B", bounds=bounds, tol=1e-12)
    th = res.x
    g, raw = hr.nll_hessian_ref("rbf_iso", x, ym, V, th, dtype=np.float64)
    lam = np.linalg.eigvalsh(0.5 * (raw + raw.T))
    print(f"HESS|laplace case|rbf_iso|1|200|theta {th} |g| {np.max(np.abs(g)):.3g} eigenvalues {lam}")
    assert np.all(th > bounds[:, 0] * 1.5) and np.all(th < bounds[:, 1] / 1.5)
    assert np.max(np.abs(g)) <= 1e-3
    assert lam[0] > 1e-3 * lam[-1] > 0.0
    # the point where the device test expects the Laplace approximation to be refused: the Hessian is indefinite there
    _, far = hr.nll_hessian_ref("rbf_iso", x, ym, V, hr.LAPLACE_NOT_A_MINIMUM, dtype=np.float64)
    lam_far = np.linalg.eigvalsh(0.5 * (far + far.T))
    print(f"HESS|laplace case, away from the minimum|rbf_iso|1|200|eigenvalues {lam_far}")
    assert lam_far[0] < -1e-3 * lam_far[-1] < 0.0


def test_library_exports_the_hessian_entries():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    for s in ("fvgp_hip_loglik_hess", "fvgp_hip_loglik_hess_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert len(L.fvgp_hip_loglik_hess.argtypes) == 20 and L.fvgp_hip_loglik_hess.restype is ctypes.c_int
    assert len(L.fvgp_hip_loglik_hess_workspace_bytes.argtypes) == 2 and L.fvgp_hip_loglik_hess_workspace_bytes.restype is ctypes.c_int64
    # rows of the second-derivative pass (1 + d + d (d + 1) / 2 sums per lower tile up to d = 4, d rows of 18 beyond), (d + 1) trace
    # passes of (d + 1) sums per lower tile, one padded vector
    for n, d in ((1, 1), (128, 3), (129, 4), (300, 5), (140, 16)):
        np_ = -(-n // 128) * 128
        nb = (np_ // 128) * (np_ // 128 + 1) // 2
        row = 1 + d + d * (d + 1) // 2 if d <= 4 else 18 * d
        assert _lib.loglik_hess_workspace_bytes(n, d) == (nb * row + (d + 1) ** 2 * nb + np_) * 8
    for n, d in ((0, 2), (10, 0), (10, 17)):
        assert _lib.loglik_hess_workspace_bytes(n, d) == -1
    g, hs = (ctypes.c_double * 3)(), (ctypes.c_double * 9)()
    assert L.fvgp_hip_loglik_hess(None, 0, None, 10, 2, None, 3, None, 1, 0, None, 128, None, 128, None, 128, None, 0, g, hs) == -1
    assert hasattr(_lib.Handle, "loglik_hess")
