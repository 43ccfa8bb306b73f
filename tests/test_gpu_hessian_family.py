"""Every <KIND, D> instantiation of the Hessian's three templated kernels -- hess_trace_kernel, kmat_grad_kernel (csrc/hessian.hip) and
the two-vector gradient trace (grad_trace_kernel<KIND, D, TWO = true>, csrc/kmat.hip) -- through fvgp_hip_loglik_hess, against the
extended-precision references of tests/hessian_ref.py, which tests/test_hessian_host.py and tests/test_hessian_family_host.py prove
on the host.

1. the sweep: every (name, d) of the family grid that tests/test_gpu_hessian.py does not hold, n = 261, under that test's bar;
2. the second-derivative pass on its own: a factor scaled by 2^30 and b = 2^-30 u push the bracket n 2^-60 below the trace, and every
   returned g_i and raw H_ij is held to a derived magnitude-sum bound (hessian_ref.hess_trace_bound_factor);
3. the bracket on its own: the scaling the other way round, one case per cell, a bound assembled from the product's, the entries' and
   the trace's derived bounds (hessian_ref.bracket_bound_factors).

Every case prints its figures as `HESS|entry|kernel|d|n|figure` lines (pytest -s)."""
import ctypes

import numpy as np
import pytest

import hessian_ref as hr
from fvgp_amd._lib import KERNEL_IDS

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _report(entry, name, d, n, figure):
    print(f"HESS|{entry}|{name}|{d}|{n}|{figure:.3g}")


def _ratio(err, bound):
    """largest err / bound; an entry whose bound is 0 counts 0 where it is met exactly and inf where not"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def _factor(H, name, x, ym, V, theta):
    """the factor of K + V as fvgp_hip_loglik leaves it, and KVinvY"""
    from fvgp_amd import _lib
    n, ncol = ym.shape
    dim = _lib.loglik_dim(n, ncol)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), ncol)
    info = H.loglik(KERNEL_IDS[name], H.to_device(x), theta, H.to_device(V), H.to_device(ym), KV, alpha)[3]
    assert info == 0
    return KV, alpha


def _scratch(H, n, d):
    from fvgp_amd import _lib
    np_ = _lib.pad128(n)
    work, work2 = H.empty(np_, np_), H.empty(np_, np_)
    work.fill_(float("nan"))
    work2.fill_(float("nan"))
    return work, work2, H.empty(_lib.loglik_hess_workspace_bytes(n, d) // 8)


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,d,ncol,comp,dup", hr.FAMILY_CASES)
def test_sweep_against_extended_precision(H, name, n, d, ncol, comp, dup):
    """tests/test_gpu_hessian.py::test_abi_against_extended_precision on the rest of the grid: the raw Hessian, the gradient and the
    asymmetry under hessian_bar"""
    (x, ym, V, theta), (g_r, raw_r) = hr.reference(name, n, d, ncol, comp, dup)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    g, raw = H.loglik_hess(KERNEL_IDS[name], H.to_device(x), theta, alpha, ncol, comp, KV, *_scratch(H, n, d))
    f = lambda a: np.asarray(a, dtype=np.float64)
    bar = hr.hessian_bar(raw_r)
    ratios = {
        "hessian": float(np.max(np.abs(raw - f(raw_r)) / bar)),
        "gradient": float(np.max(np.abs(g - f(g_r)) / hr.hessian_bar(g_r))),
        "asymmetry": float(np.max(np.abs(raw - raw.T) / bar)),
    }
    for key, r in ratios.items():
        _report(f"sweep {key} / bar", name, d, n, r)
    assert g.shape == theta.shape and raw.shape == (len(theta), len(theta))
    assert np.all(np.isfinite(raw)) and np.all(np.isfinite(g))
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{worst}: {ratios[worst]:.3g} times its bar"


@pytest.mark.parametrize("name,d", [("matern32_ard", 4), ("matern52_iso", 16)])
def test_two_more_hyperparameters_than_the_kernel_owns(H, name, d):
    """ntheta = nk + 2: grad_host comes back +0.0 in the two extra places, and hess_host, with a canary behind its nk x nk block, keeps
    the canary; the block and the gradient have the bits of the call with ntheta = nk"""
    from fvgp_amd import _lib
    L = _lib.lib()
    n = hr.FAMILY_N
    (x, ym, V, theta), _ = hr.reference(name, n, d, 1, 0, None)
    nk = len(theta)
    KV, alpha = _factor(H, name, x, ym, V, theta)
    xd = H.to_device(x)
    g0, raw0 = H.loglik_hess(KERNEL_IDS[name], xd, theta, alpha, 1, 0, KV.clone(), *_scratch(H, n, d))
    work, work2, ws = _scratch(H, n, d)
    th = (ctypes.c_double * (nk + 2))(*theta, 0.5, 0.7)
    g = (ctypes.c_double * (nk + 2))(*([7.0] * (nk + 2)))
    hs = (ctypes.c_double * (nk * nk + 8))(*([7.0] * (nk * nk + 8)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    A = KV.clone()
    rc = L.fvgp_hip_loglik_hess(H._h, KERNEL_IDS[name], p(xd), n, d, th, nk + 2, p(alpha), 1, 0, p(A), A.stride(0), p(work), work.stride(0),
                                p(work2), work2.stride(0), p(ws), ws.numel() * 8, g, hs)
    assert rc == 0
    g, hs = np.array(g[:]), np.array(hs[:])
    assert np.all(g[nk:] == 0.0) and not np.any(np.signbit(g[nk:]))
    assert np.all(hs[nk * nk:] == 7.0)
    assert g[:nk].tobytes() == g0.tobytes() and hs[:nk * nk].tobytes() == raw0.tobytes()


# ---- 2. and 3.: the pass and the bracket, each on its own -------------------------------------------------------------------------------
def _scaled_call(H, name, d, shift, apart=False):
    """fvgp_hip_loglik_hess on the factor of pass_inputs' well-conditioned KV scaled by 2^shift, with alpha overwritten by b = 2^-shift u
    (apart: the factor of the SAME x, the call with the coincident pairs one ulp apart): (x of the call, theta, g, raw, W, b), W read back
    from the lower triangle of KV -- which the entry leaves holding (L L^T)^-1 -- and mirrored"""
    x, theta, V, y, u = hr.pass_inputs(name, d)
    n = len(x)
    KV, alpha = _factor(H, name, x, y, V, theta)
    KV.mul_(2.0 ** shift)                       # exact; the padding's identity stays diagonal
    H.invalidate_factor()                       # the factor was rewritten in place: the handle's diagonal-block inverses are stale
    b = u * 2.0 ** -shift
    alpha.zero_()
    alpha[:n, 0] = H.to_device(b)
    xc = hr.pass_inputs(name, d, apart=True)[0] if apart else x
    g, raw = H.loglik_hess(KERNEL_IDS[name], H.to_device(xc), theta, alpha, 1, 0, KV, *_scratch(H, n, d))
    Wd = KV[:n, :n].cpu().numpy()
    upper = np.triu(Wd, 1)
    assert np.array_equal(upper, np.tril(Wd, -1).T)                  # the stated contract: both triangles
    assert 2.0 ** -8 < np.median(np.diag(Wd)) * 4.0 ** shift < 2.0 ** 8     # ... of 4^-shift (K + V)^-1, V of the order of sigma^2
    return xc, theta, g, raw, np.tril(Wd) + np.tril(Wd, -1).T, b


@pytest.mark.parametrize("name,d", hr.PASS_CASES)
def test_second_derivative_pass_within_its_derived_bound(H, name, d):
    """every g_i and raw H_ij of the call whose bracket is n 2^-60 of the trace: finite, and within hess_trace_bound_factor(d) eps of
    the magnitude sums that enter it (+ 2^-20 of the bracket's magnitude); the same call with the two coincident pairs one ulp apart
    changes no result by more than that bound (the 1e150 * 0 of Matern 3/2's c2 on a coincident pair really adds 0)"""
    n = hr.PASS_N
    x, theta, g, raw, W, b = _scaled_call(H, name, d, hr.PASS_SHIFT)
    R = hr.pass_reference(name, x, theta, W, b)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(raw))
    assert g.shape == R["g"].shape and raw.shape == R["raw"].shape
    # the construction holds on the device's W as on the host's (tests/test_hessian_family_host.py): terms of one sign, and a bracket
    # that is nothing beside the trace (H_00, where d2K/ds2 = 0, is the bracket alone)
    off = np.ones(raw.shape, dtype=bool)
    off[0, 0] = False
    assert max(float(v[1] / abs(v[0])) for k, v in R["red"].items() if k[0] != "gs") <= 4.0
    assert float(np.max(R["bracket_mag"][off] / np.abs(R["raw"])[off])) <= 2.0 ** -40
    rg = _ratio(np.abs(g.astype(LD) - R["g"]), R["g_bound"])
    rh = _ratio(np.abs(raw.astype(LD) - R["raw"]), R["raw_bound"])
    _report("pass gradient / bound", name, d, n, rg)
    _report("pass hessian / bound", name, d, n, rh)
    _, _, g2, raw2, W2, _ = _scaled_call(H, name, d, hr.PASS_SHIFT, apart=True)
    assert W2.tobytes() == W.tobytes()
    assert np.all(np.isfinite(g2)) and np.all(np.isfinite(raw2))
    ra = max(_ratio(np.abs(g2 - g), R["g_bound"]), _ratio(np.abs(raw2 - raw), R["raw_bound"]))
    _report("pass one ulp apart / bound", name, d, n, ra)
    assert rg <= 1.0 and rh <= 1.0, f"gradient {rg:.3g}, hessian {rh:.3g} times the bound"
    assert ra <= 1.0, f"one ulp apart: {ra:.3g} times the bound"


@pytest.mark.parametrize("name,d", hr.BRACKET_CASES)
def test_bracket_within_its_derived_bound(H, name, d):
    """the raw Hessian of the call whose trace is n^-1 2^-60 of the bracket: -[1/2 tr(G_i K_j) - b^T K_j w_i] as kmat_grad_kernel, the
    two products, rowdot_scale_kernel and the two-vector trace compute it, within bracket_bound_factors eps (M1 + M2)"""
    n = hr.PASS_N
    x, theta, g, raw, W, b = _scaled_call(H, name, d, -hr.PASS_SHIFT)
    ref, bound = hr.bracket_reference(name, x, theta, W, b)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(raw))
    r = _ratio(np.abs(raw.astype(LD) - ref), bound)
    _report("bracket / bound", name, d, n, r)
    _report("bracket bound / abs H, largest", name, d, n, float(np.max(bound / np.abs(ref))))
    assert r <= 1.0, f"{r:.3g} times the bound"
