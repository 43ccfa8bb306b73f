"""Leave-one-out cross-validation without a GPU: the extended-precision reference's closed forms (tests/loo_ref.py) against n brute-force
refits, its gradient against a central difference of the brute-force value, the float64 twin on the cases of the device test, the
facade's host assembly of the noise and mean terms against hand-differentiated references, and the ABI surface of fvgp_hip_loo."""
import ctypes

import numpy as np
import pytest

import kernel_family_ref as kf
import loo_ref
import test_gpu_loo as gl

LD = np.longdouble


def _case(name, n, d, seed):
    """inputs as the GPU tests draw them: x in the unit cube, sigma^2 = 1.2, length scales in [0.3, 0.6], noise 0.01 - 0.02, y centred"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    theta = np.concatenate([[1.2], rng.uniform(0.3, 0.6, kf.n_theta(name, d) - 1)])
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y - y.mean(), rng.uniform(0.01, 0.02, n), theta


CASES = [("rbf_ard", 40, 2), ("matern32_iso", 40, 3), ("matern52_ard", 96, 3), ("rbf_ard", 96, 1)]


@pytest.mark.parametrize("name,n,d", CASES)
def test_closed_form_equals_brute_force_refits(name, n, d):
    """value and means to 1e-13, variances to 1e-12 relative (measured: at most 1e-15 and 4e-14)"""
    x, y, V, theta = _case(name, n, d, 7 * n + d)
    vc, mc, sc, _, _, _ = loo_ref.loo_closed(name, x, y, V, theta, want_grad=False)
    vb, mb, sb = loo_ref.loo_brute(name, x, y, V, theta)
    e_val, e_m, e_v = float(abs(vc - vb)), float(np.max(np.abs(mc - mb))), float(np.max(np.abs(sc - sb) / sb))
    print(f"LOO|closed vs brute|{name}|{d}|{n}|value {e_val:.3g} mean {e_m:.3g} var {e_v:.3g}")
    assert e_val <= 1e-13 * max(1.0, float(abs(vb)))
    assert e_m <= 1e-13
    assert e_v <= 1e-12


@pytest.mark.parametrize("name,n,d", [("rbf_ard", 40, 2), ("matern32_iso", 40, 3), ("matern52_ard", 40, 3)])
def test_gradient_equals_central_difference_of_brute_force(name, n, d):
    """step 1e-7, to 1e-7 relative of max|g| (measured: at most 2e-9; the step's truncation error is 1e-14 f''' and the longdouble
    objective's rounding 1e-19 |L| / 1e-7)"""
    x, y, V, theta = _case(name, n, d, 11 * n + d)
    g = loo_ref.loo_closed(name, x, y, V, theta)[3]
    h = LD(1e-7)
    fd = np.zeros(len(theta), dtype=LD)
    for j in range(len(theta)):
        tp, tm = theta.astype(LD), theta.astype(LD)
        tp[j] += h
        tm[j] -= h
        fd[j] = (loo_ref.loo_brute(name, x, y, V, tp)[0] - loo_ref.loo_brute(name, x, y, V, tm)[0]) / (2 * h)
    err = float(np.max(np.abs(fd - g)) / np.max(np.abs(g)))
    print(f"LOO|gradient vs central difference|{name}|{d}|{n}|{err:.3g}")
    assert err <= 1e-7


def test_family_cases_complete_the_grid():
    """ABI_CASES and FAMILY_CASES of the device test hold every (name, d) of the family grid, FAMILY_CASES each at n = 261, none twice"""
    have = [(c[0], c[2]) for c in gl.FAMILY_CASES]
    assert len(set(have)) == len(have) and all(c[1] == 261 for c in gl.FAMILY_CASES)
    assert not set(have) & {(c[0], c[2]) for c in gl.ABI_CASES}
    assert set(have) | {(c[0], c[2]) for c in gl.ABI_CASES} == {(name, d) for name in kf.FAMILY for d in kf.DIMS}
    cells = lambda cases: {(kf.FAMILY[c[0]][0], c[2] if c[2] <= 4 else 0) for c in cases}
    assert len(cells(gl.ABI_CASES)) == 6 and len(cells(gl.ABI_CASES + gl.FAMILY_CASES)) == 15


@pytest.mark.parametrize("name,n,d,ncol,comp", [c for c in gl.ABI_CASES if c[1] <= 300] + gl.FAMILY_CASES)
def test_float64_twin_sits_far_inside_the_device_bars(name, n, d, ncol, comp):
    """the same closed forms in float64 against longdouble on the cases of the device test (the two-panel n = 1100 case left to the
    device: its longdouble reference alone takes most of a minute): every one of the eight figures at most 1e-2 of its bar -- the cap
    tests/test_hessian_host.py holds the Hessian's twin to --, so the bars judge the device and not the conditioning of the case"""
    (x, ym, V, theta), ref = gl._reference(name, n, d, ncol, comp)
    value, m_loo, v_loo, grad, u, md = loo_ref.loo_closed(name, x, ym[:, comp], V, theta, dtype=np.float64)
    resid = ym[:, comp] - m_loo
    out = [value, np.sum(resid ** 2), -np.sum(np.log(v_loo))]
    ratios = gl.bar_ratios(out, grad, resid, v_loo, u, md, ref)
    worst = max(ratios, key=ratios.get)
    print(f"LOO|float64 twin / bar|{name}|{d}|{n}|worst {worst} {ratios[worst]:.3g}")
    assert ratios[worst] <= 1e-2, f"{worst}: {ratios[worst]:.3g} of its bar"


def _noise(x, a):
    """a noise model with one hyperparameter: V_k = a (0.01 + 0.01 x_k0)"""
    return a * (LD("0.01") + LD("0.01") * x[:, 0])


def _mean(x, b):
    """a mean model with one hyperparameter: m_k = b sin(2 x_k0)"""
    return b * np.sin(2 * x[:, 0])


def _objective(name, x, yraw, theta):
    """L_LOO of a GP with hyperparameters [kernel..., a (noise), b (mean)], in longdouble"""
    nk = kf.n_theta(name, x.shape[1])
    xl = x.astype(LD)
    return loo_ref.loo_closed(name, x, yraw.astype(LD) - _mean(xl, theta[nk + 1]), _noise(xl, theta[nk]), theta[:nk], want_grad=False)[0]


@pytest.mark.parametrize("name", ["rbf_ard", "matern52_iso"])
def test_host_assembly_of_noise_and_mean_terms(name):
    """assemble_loo_gradient on float64 pieces (u, alpha, diag M rounded from the longdouble reference) with dV and dm differentiated by
    hand: against the same sum in longdouble to 1e-13 of max|g|, and against a central difference (step 1e-7) of the longdouble objective
    in all hyperparameters, noise and mean included, to 1e-7 of max|g|"""
    from fvgp_amd.gp_loo import assemble_loo_gradient
    n, d = 60, 2
    x, y, _, tk = _case(name, n, d, 5)
    nk = len(tk)
    theta = np.concatenate([tk, [1.3, 0.4]]).astype(LD)
    xl = x.astype(LD)
    r = y.astype(LD) - _mean(xl, theta[nk + 1])
    V = _noise(xl, theta[nk])
    _, _, _, gk, u, md = loo_ref.loo_closed(name, x, r, V, theta[:nk])
    alpha = loo_ref.spd_inverse(kf.k_ref(name, x, x, tk) + np.diag(V)) @ r
    H = nk + 2
    dV = np.zeros((H, n), dtype=LD)
    dV[nk] = LD("0.01") + LD("0.01") * xl[:, 0]
    dm = np.zeros((H, n), dtype=LD)
    dm[nk + 1] = np.sin(2 * xl[:, 0])
    exact = np.concatenate([gk, [0, 0]]) + dV @ (u * alpha - md) + dm @ u
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    got = assemble_loo_gradient(f64(np.concatenate([gk, [0, 0]])), f64(u), f64(alpha), f64(md), f64(dV), f64(dm))
    scale = float(np.max(np.abs(exact)))
    assert got.dtype == np.float64 and got.shape == (H,)
    assert float(np.max(np.abs(got - exact))) <= 1e-13 * scale
    h = LD(1e-7)
    fd = np.zeros(H, dtype=LD)
    for j in range(H):
        tp, tm = theta.copy(), theta.copy()
        tp[j] += h
        tm[j] -= h
        fd[j] = (_objective(name, x, y, tp) - _objective(name, x, y, tm)) / (2 * h)
    err = float(np.max(np.abs(fd - exact))) / scale
    print(f"LOO|assembly vs central difference|{name}|{d}|{n}|{err:.3g}")
    assert err <= 1e-7
    # the pieces alone: no noise or mean model leaves the kernel term as it is; a matrix-valued noise derivative is refused
    assert np.array_equal(assemble_loo_gradient(f64(gk), f64(u), f64(alpha), f64(md)), f64(gk))
    with pytest.raises(NotImplementedError, match="gradient-free"):
        assemble_loo_gradient(f64(gk), f64(u), f64(alpha), f64(md), dV=np.zeros((nk, n, n)))


def test_library_exports_the_loo_entries():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    for s in ("fvgp_hip_loo", "fvgp_hip_loo_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert len(L.fvgp_hip_loo.argtypes) == 22 and L.fvgp_hip_loo.restype is ctypes.c_int
    assert len(L.fvgp_hip_loo_workspace_bytes.argtypes) == 1 and L.fvgp_hip_loo_workspace_bytes.restype is ctypes.c_int64
    # three padded vectors (w, c, sqrt c) and four partial sums per 128 rows
    for n in (1, 128, 129):
        np_ = -(-n // 128) * 128
        assert _lib.loo_workspace_bytes(n) == (3 * np_ + 4 * (np_ // 128)) * 8
    assert _lib.loo_workspace_bytes(0) == -1
    out = (ctypes.c_double * 4)()
    assert L.fvgp_hip_loo(None, 0, None, 10, 2, None, 0, None, 1, 0, None, 128, None, 128, None, 0, out, None, None, None, None, None) == -1
