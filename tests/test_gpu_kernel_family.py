"""Conformance of the native kernel family: every entry point that launches a <KIND, D> instantiation (kmat_kernel, grad_trace_kernel,
kmat_batch_kernel, cross_batch_kernel, grad_trace_batch_kernel, posterior_grad_kernel) at every name of _lib.KERNEL_IDS and
d = 1, 2, 3, 4 (the dimensions with an instantiation of their own), 5 and 16 (both ends of the runtime-dimension path), against the
extended-precision reference of tests/kernel_family_ref.py, which tests/test_kernel_family_ref.py proves on the host.  Then the
argument checks of the gradient trace's leading dimension and the exported reductions that had no direct test.

Every case prints its worst figure as a line `KF|entry point|kernel|d|n|figure` (pytest -s): the numbers the next family member is
compared with."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import kernel_family_ref as ref
from fvgp_amd._lib import KERNEL_IDS
from oracle import fvgp_oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NAMES = list(KERNEL_IDS)
NOISE = 0.02
# one d per name at n = 517 (five tile rows: interior tile rows in the two-rows-per-trip path and in the edge path)
D517 = {"rbf_ard": 2, "matern32_ard": 4, "matern52_ard": 16, "rbf_iso": 16, "matern32_iso": 5, "matern52_iso": 3}
GT_CASES = ([(name, d, 300) for name in NAMES for d in ref.DIMS] + [(name, D517[name], 517) for name in NAMES]
            + [(name, 3, n) for name in NAMES for n in (1, 127, 128, 129)])
COLS_CASES = [(name, d, 300) for name in NAMES for d in ref.DIMS] + [(name, D517[name], 517) for name in NAMES]


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _ratio(err, bound):
    """largest err / bound; an entry whose bound is 0 (every term of its sum is 0: the length-scale derivative of a single point) counts
    0 where it is met exactly and inf where not"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def _report(entry, name, d, n, figure):
    print(f"KF|{entry}|{name}|{d}|{n}|{figure:.3g}")


# ---- kmat ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ref.DIMS)
@pytest.mark.parametrize("name", NAMES)
def test_kmat_against_extended_precision(H, name, d):
    """300 x 201 (three tile rows, two tile columns, ragged last ones), once into a tight buffer (odd leading dimension: scalar stores)
    and once into a padded one (the vector stores and the interior-tile path): |K - k_ref| <= 4 eps sigma^2 for d <= 5,
    (4 + 0.4 (d + 2)) eps sigma^2 at d = 16 (kernel_family_ref.k_bound_ulps)."""
    from fvgp_amd import _lib
    x1, x2, theta = ref.case(name, d, 300, 201)
    exact = ref.k_ref(name, x1, x2, theta)
    kid = KERNEL_IDS[name]
    K = H.to_device(np.full((300, 201), np.nan))
    H.kmat(kid, H.to_device(x1), H.to_device(x2), theta, K, pad=_lib.PAD_NONE)
    Kp = H.to_device(np.full((384, 256), np.nan))
    H.kmat(kid, H.to_device(x1), H.to_device(x2), theta, Kp, pad=_lib.PAD_ZERO)
    H.sync()
    got, gp = K.cpu().numpy(), Kp.cpu().numpy()
    ulps = max(float(np.max(np.abs(g - exact))) / (EPS * theta[0]) for g in (got, gp[:300, :201]))
    _report("kmat ulp sigma^2", name, d, 300, ulps)
    assert np.all(np.isfinite(got))
    assert ulps <= ref.k_bound_ulps(d)
    assert np.all(gp[300:, :] == 0) and np.all(gp[:, 201:] == 0)


# ---- grad_trace, called directly -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gt_case(name, d, n):
    """inputs of a gradient-trace case and its longdouble reference (computed once, shared by the direct and the slab test, never
    modified): W random symmetric, b random; want / scale: sum and sum of magnitudes of the terms, with b and without"""
    x, _, theta = ref.case(name, d, n)
    rng = np.random.default_rng(7 * n + d)
    W = rng.standard_normal((n, n))
    W = W + W.T
    b = rng.standard_normal(n)
    out = {"x": x, "theta": theta, "W": W, "b": b}
    for key, bb in (("b", b), ("nob", None)):
        terms = ref.grad_trace_terms(name, x, theta, W, bb)
        out["want_" + key] = terms.sum(axis=(1, 2))
        out["bound_" + key] = ref.grad_trace_bound_factor(d) * EPS * np.abs(terms).sum(axis=(1, 2))
    for v in out.values():
        v.setflags(write=False)
    return out


def _lower_on_device(H, W, n, ld, col0=0, ncols=None):
    """columns [col0, col0 + ncols) of the symmetric W in a NaN-filled (pad128(n), ld) device buffer, entries with row >= column only:
    whatever else the kernel loads is NaN and must not reach a sum"""
    from fvgp_amd import _lib
    ncols = n - col0 if ncols is None else min(ncols, n - col0)
    buf = np.full((_lib.pad128(n), ld), np.nan)
    i, j = np.tril_indices(n)
    keep = (j >= col0) & (j < col0 + ncols)
    buf[i[keep], j[keep] - col0] = W[i[keep], j[keep]]
    return H.to_device(buf)


@pytest.mark.parametrize("name,d,n", GT_CASES)
def test_grad_trace_direct(H, name, d, n):
    """fvgp_hip_grad_trace on a W whose strict upper triangle and padding are NaN on the device (only i >= j is read), without b, with a
    contiguous b and with b as a column of an (n, 3) array (ldb = 3); ntheta exactly the kernel's count and two more (the extra entries
    come back exactly 0).  Per component: |g - g_exact| <= (80 + d + 32 + 2 d) eps sum_jk |term_jk| (kernel_family_ref), derived."""
    from fvgp_amd import _lib
    c = _gt_case(name, d, n)
    nk = ref.n_theta(name, d)
    kid = KERNEL_IDS[name]
    npad = _lib.pad128(n)
    T = npad // 128
    xd = H.to_device(np.array(c["x"]))
    Wd = _lower_on_device(H, c["W"], n, npad)
    partial = H.empty(T * (T + 1) // 2 * (nk + 2) + 64)
    b3 = np.full((n, 3), np.nan)
    b3[:, 1] = c["b"]
    b3d = H.to_device(b3)
    theta2 = np.concatenate([c["theta"], [0.5, 0.7]])
    g_nob = H.grad_trace(kid, xd, c["theta"], Wd, None, partial)
    g_b = H.grad_trace(kid, xd, theta2, Wd, H.to_device(np.array(c["b"])), partial)
    g_s = H.grad_trace(kid, xd, c["theta"], Wd, b3d[:, 1], partial)
    assert b3d[:, 1].stride(0) == 3
    assert g_nob.shape == (nk,) and g_b.shape == (nk + 2,) and g_s.shape == (nk,)
    assert np.all(g_b[nk:] == 0.0) and not np.any(np.signbit(g_b[nk:]))
    assert g_s.tobytes() == g_b[:nk].tobytes()                       # the stride of b changes no arithmetic
    worst = 0.0
    for got, key in ((g_nob, "nob"), (g_b[:nk], "b")):
        assert np.all(np.isfinite(got)), (key, got)
        worst = max(worst, _ratio(np.abs(got - c["want_" + key]), c["bound_" + key]))
    _report("grad_trace / bound", name, d, n, worst)
    assert worst <= 1.0


@pytest.mark.parametrize("name,d,n", COLS_CASES)
def test_grad_trace_cols_slabs_add_up(H, name, d, n):
    """fvgp_hip_grad_trace_cols over slabs of 128 columns (the last one narrower) and of 256 columns (the last one with ncols running
    past the matrix), each slab in a NaN-filled buffer of its own with a leading dimension of 128 ceil(ncols / 128): the slabs' results
    add up to fvgp_hip_grad_trace's and to the reference within the bound of test_grad_trace_direct; the blocks of a slab that lie
    above the diagonal (tile row < tile column) write exact zeros to the partial sums."""
    from fvgp_amd import _lib
    c = _gt_case(name, d, n)
    nk = ref.n_theta(name, d)
    kid = KERNEL_IDS[name]
    npad = _lib.pad128(n)
    T = npad // 128
    xd, bd = H.to_device(np.array(c["x"])), H.to_device(np.array(c["b"]))
    g_full = H.grad_trace(kid, xd, c["theta"], _lower_on_device(H, c["W"], n, npad), bd, H.empty(T * (T + 1) // 2 * nk + 64))
    worst = 0.0
    for width in (128, 256):
        total = np.zeros(nk, dtype=LD)
        for col0 in range(0, n, width):
            ncols = min(width, n - col0) if width == 128 else width
            ld = _lib.pad128(ncols)
            Wd = _lower_on_device(H, c["W"], n, ld, col0, ncols)
            partial = H.to_device(np.full(T * (ld // 128) * nk + 64, np.nan))
            g = H.grad_trace_cols(kid, xd, c["theta"], Wd, col0, ncols, bd, partial)
            assert np.all(np.isfinite(g)), (width, col0, g)
            total += g
            part = partial.cpu().numpy()
            ntj = min(ld // 128, T - col0 // 128)
            for tjl in range(ntj):
                for ti in range(col0 // 128 + tjl):                  # tile rows above this tile column
                    blk = part[(tjl * T + ti) * nk:(tjl * T + ti + 1) * nk]
                    assert np.all(blk == 0.0) and not np.any(np.signbit(blk)), (width, col0, tjl, ti, blk)
        for want in (g_full, c["want_b"]):
            worst = max(worst, _ratio(np.abs(total - want), c["bound_b"]))
    _report("grad_trace_cols / bound", name, d, n, worst)
    assert worst <= 1.0


def test_grad_trace_leading_dimension_is_checked(H):
    """the gradient trace loads whole 128-column tile rows of W: a leading dimension below padded_dim(n) -- below 128 ceil(ncols / 128)
    for a slab -- is refused with -9 before anything is launched (the outputs keep their NaN)"""
    from fvgp_amd import _lib
    n = 300
    xd = H.to_device(np.random.default_rng(0).random((n, 2)))
    theta = np.array([1.0, 0.3, 0.4])
    partial = H.to_device(np.full(4096, np.nan))
    for ld in (300, 382):
        with pytest.raises(_lib.HipExtensionError, match="status -9"):
            H.grad_trace(0, xd, theta, H.zeros(384, ld), None, partial)
    with pytest.raises(_lib.HipExtensionError, match="status -9"):
        H.grad_trace(0, xd, theta, H.zeros(384, 385), None, partial)             # odd
    for ld, ncols in ((200, 200), (128, 129), (254, 172)):
        with pytest.raises(_lib.HipExtensionError, match="status -9"):
            H.grad_trace_cols(0, xd, theta, H.zeros(384, ld), 128, ncols, None, partial)
    with pytest.raises(_lib.HipExtensionError, match="status -10"):
        H.grad_trace_cols(0, xd, theta, H.zeros(384, 128), 64, 128, None, partial)
    H.sync()
    assert np.all(np.isnan(partial.cpu().numpy()))


# ---- the whole gradient pipelines ------------------------------------------------------------------------------------------------
def _data(name, d, n):
    x, _, theta = ref.case(name, d, n)
    rng = np.random.default_rng(n + d)
    y = np.sin(3.0 * x.sum(axis=1) / np.sqrt(d)) + 0.1 * rng.standard_normal(n)
    return x, y, theta


def _gradient_reference(name, x, ym, theta):
    """double: K and dK/dtheta from the extended-precision reference (rounded to double), KV^-1 and b from scipy's Cholesky"""
    n = len(x)
    KV = np.asarray(ref.k_ref(name, x, x, theta), dtype=np.float64) + NOISE * np.eye(n)
    cf = sla.cho_factor(KV, lower=True)
    inv = sla.cho_solve(cf, np.eye(n))
    b = sla.cho_solve(cf, ym[:, 0])
    dK = np.asarray(ref.dk_dtheta_ref(name, x, x, theta), dtype=np.float64)
    g = np.array([0.5 * np.sum((inv - np.outer(b, b)) * dK[i]) for i in range(len(dK))])
    return g, b, np.diag(inv).copy()


@pytest.mark.parametrize("d", ref.DIMS)
@pytest.mark.parametrize("name", NAMES)
def test_loglik_grad_and_batch_against_extended_precision_dk(H, name, d):
    """fvgp_hip_loglik + fvgp_hip_loglik_grad at one theta and fvgp_hip_loglik_grad_batch at B = 3 (the middle row that theta), n = 300,
    noise 0.02: gradients rtol 1e-8, atol 1e-9 max|g| (the project's bars); b_out and diag_out 1e-8 of their largest entry (the KVinvY
    bar)."""
    from fvgp_amd import _lib
    n = 300
    x, y, theta = _data(name, d, n)
    ym = (y - y.mean()).reshape(n, 1)
    rng = np.random.default_rng(d)
    th = np.vstack([theta * np.exp(rng.uniform(-0.3, 0.3, len(theta))), theta, theta * np.exp(rng.uniform(-0.3, 0.3, len(theta)))])
    refs = [_gradient_reference(name, x, ym, t) for t in th]
    kid = KERNEL_IDS[name]
    dim, npd = _lib.loglik_dim(n, 1), _lib.pad128(n)
    xd, vd, ymd = H.to_device(x), H.to_device(np.full(n, NOISE)), H.to_device(ym)
    KV, W, alpha = H.empty(dim, dim), H.empty(npd, npd), H.empty(npd, 1)
    assert H.loglik(kid, xd, theta, vd, ymd, KV, alpha)[3] == 0
    g1 = H.loglik_grad(kid, xd, theta, alpha, 1, 0, KV, W)
    bdim = _lib.loglik_batch_dim(n, 1)
    bo, do = H.empty(3, n), H.empty(3, n)
    out, gb, info = H.loglik_grad_batch(kid, xd, th, vd, ymd, H.empty(3, bdim, bdim), H.empty(3, npd, npd), 0, bo, do)
    assert np.all(info == 0)
    bo, do = bo.cpu().numpy(), do.cpu().numpy()
    worst = 0.0
    for got, (g, b, dg) in [(g1, refs[1])] + list(zip(gb, refs)):
        worst = max(worst, float(np.max(np.abs(got - g) / (1e-8 * np.abs(g) + 1e-9 * np.max(np.abs(g))))))
    _report("loglik_grad(+batch) / bar", name, d, n, worst)
    np.testing.assert_allclose(g1, refs[1][0], rtol=1e-8, atol=1e-9 * np.max(np.abs(refs[1][0])))
    for r in range(3):
        g, b, dg = refs[r]
        np.testing.assert_allclose(gb[r], g, rtol=1e-8, atol=1e-9 * np.max(np.abs(g)))
        assert np.max(np.abs(bo[r] - b)) <= 1e-8 * np.max(np.abs(b))
        assert np.max(np.abs(do[r] - dg)) <= 1e-8 * np.max(np.abs(dg))


# ---- posterior_grad --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n_dirs", [(4, 4), (5, 5), (16, 16), (16, 3)])
@pytest.mark.parametrize("name", NAMES)
def test_posterior_grad_in_higher_dimensions(H, name, d, n_dirs):
    """fvgp_hip_posterior_grad at d = 4 (its own instantiation), 5 and 16 (runtime dimension), n = 300, P = 130: the bound of
    test_gpu_posterior_grad.test_abi_matches_kernel_dx_within_the_summation_bound, (N + 32) eps sum_i |term_i| per output, with k and
    dk/dx* from the extended-precision closed forms; alpha and W are the device's own, downloaded."""
    from fvgp_amd import _lib
    n, P = 300, 130
    x, y, theta = _data(name, d, n)
    xp = np.random.default_rng(d + 1).random((P, d))
    kid = KERNEL_IDS[name]
    npad, Pp, dim = _lib.pad128(n), _lib.pad128(P), _lib.loglik_dim(n, 1)
    xd, xpd = H.to_device(x), H.to_device(xp)
    KV, alpha = H.empty(dim, dim), H.empty(npad, 1)
    assert H.loglik(kid, xd, theta, H.to_device(np.full(n, NOISE)), H.to_device((y - y.mean()).reshape(n, 1)), KV, alpha)[3] == 0
    W = H.empty(npad, Pp)
    H.kmat(kid, xd, xpd, theta, W, pad=_lib.PAD_ZERO)
    H.potrs_cols(KV, n, W, Pp)
    work = H.empty(_lib.posterior_grad_workspace_bytes(n, P, n_dirs) // 8)
    A, q, dm, dv = H.empty(P), H.empty(P), H.empty(P, n_dirs), H.empty(P, n_dirs)
    H.posterior_grad(kid, xd, theta, xpd, alpha, 1, 0, W, n_dirs, work, A, q, dm, dv)
    H.sync()
    al, Wh = np.asarray(alpha.cpu().numpy()[:n, 0], dtype=LD), np.asarray(W.cpu().numpy()[:n, :P], dtype=LD)
    k = ref.k_ref(name, xp, x, theta)                               # (P, N)
    dk = ref.dk_dx_ref(name, xp, x, theta)[:n_dirs]                 # (n_dirs, P, N)
    worst = 0.0
    for tag, terms, got in (("A", k * al[None, :], A), ("q", k * Wh.T, q),
                            ("dm", np.transpose(dk * al[None, None, :], (1, 0, 2)), dm),
                            ("dv", np.transpose(-2 * dk * Wh.T[None, :, :], (1, 0, 2)), dv)):
        got = got.cpu().numpy()
        want, bound = terms.sum(axis=-1), (n + 32) * EPS * np.abs(terms).sum(axis=-1)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        ratio = float(np.max(np.abs(got - want) / bound))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, d, n_dirs, tag, ratio)
    _report(f"posterior_grad n_dirs={n_dirs} / bound", name, d, n, worst)


# ---- the batched assemblies -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 5, 16])
@pytest.mark.parametrize("name", NAMES)
def test_loglik_batch_and_posterior_batch_in_higher_dimensions(H, name, d):
    """fvgp_hip_loglik_batch (kmat_batch_kernel) and fvgp_hip_posterior_batch (cross_batch_kernel) at B = 2, P = 20, n = 300 against
    orc.log_likelihood_once and orc.OracleGP with the bars of the batch tests: log-likelihood rtol 1e-10, mean rtol 1e-8 (atol 1e-10),
    variance and covariance 1e-10 sigma^2 (+ 1e-12)."""
    from fvgp_amd import _lib
    n, P, B = 300, 20, 2
    x, y, theta = _data(name, d, n)
    nv = np.full(n, NOISE)
    th = np.vstack([theta, theta * np.exp(np.random.default_rng(d).uniform(-0.3, 0.3, len(theta)))])
    xp = np.random.default_rng(d + 2).random((P, d))
    kid = KERNEL_IDS[name]
    ym = (y - y.mean()).reshape(n, 1)
    dim, Pp = _lib.loglik_batch_dim(n, 1), _lib.pad128(P)
    xd, vd, ymd = H.to_device(x), H.to_device(nv), H.to_device(ym)
    out, info = H.loglik_batch(kid, xd, th, vd, ymd, H.empty(B, dim, dim))
    assert np.all(info == 0)
    mean, var, S = H.empty(B, P, 1), H.empty(B, P), H.empty(B, Pp, Pp)
    pout, pinfo = H.posterior_batch(kid, xd, th, vd, ymd, H.to_device(xp), H.empty(B, dim + Pp, dim), mean, var, S, want_loglik=True)
    assert np.all(pinfo == 0)
    mean, var, S = mean.cpu().numpy(), var.cpu().numpy(), S.cpu().numpy()[:, :P, :P]
    worst = 0.0
    for r in range(B):
        ll = orc.log_likelihood_once(x, y, nv, th[r], name)[0]
        o = orc.OracleGP(x, y, th[r], nv, kernel=name)
        rm, rc = o.posterior_mean(xp)["m(x)"], o.posterior_covariance(xp)
        tol = 1e-10 * th[r, 0] + 1e-12
        worst = max(worst, abs(out[r, 0] - ll) / (1e-10 * abs(ll)), abs(pout[r, 0] - ll) / (1e-10 * abs(ll)),
                    float(np.max(np.abs(S[r] - rc["S"]))) / tol, float(np.max(np.abs(var[r] - rc["v(x)"]))) / tol,
                    float(np.max(np.abs(mean[r, :, 0] + y.mean() - rm) / (1e-8 * np.abs(rm) + 1e-10))))
        np.testing.assert_allclose(out[r, 0], ll, rtol=1e-10)
        np.testing.assert_allclose(pout[r, 0], ll, rtol=1e-10)
        np.testing.assert_allclose(mean[r, :, 0] + y.mean(), rm, rtol=1e-8, atol=1e-10)
        assert np.max(np.abs(var[r] - rc["v(x)"])) <= tol
        assert np.max(np.abs(S[r] - rc["S"])) <= tol
    _report("loglik_batch+posterior_batch / bar", name, d, n, worst)


# ---- the exported reductions ------------------------------------------------------------------------------------------------------
ROWS, COLS = (1, 127, 129, 300), (1, 5, 130)


def _f32(rng, *shape):
    """standard normals rounded to float32: 24-bit mantissas, so a product of two is exact in double and the any-order summation bound
    (m - 1) eps sum|term| of a sum of m exact terms is the whole error of a correct kernel (0 for m = 1)"""
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def _fixed(rng, *shape):
    """multiples of 1/256 in [-8, 8]: (W - b_i b_j) D is exact in double too"""
    return rng.integers(-2048, 2049, shape).astype(np.float64) / 256.0


def _embed(H, a, extra_rows=2, extra_cols=3):
    """a (r, c) in the top left corner of a NaN-filled (r + extra_rows, c + extra_cols) device array; returns (array, view of a):
    a leading dimension larger than the width, and junk that must not be read"""
    r, c = a.shape
    buf = np.full((r + extra_rows, c + extra_cols), np.nan)
    buf[:r, :c] = a
    big = H.to_device(buf)
    return big, big[:r, :c]


@pytest.mark.parametrize("rows", ROWS)
def test_dot_coldot_colsumsq(H, rows):
    rng = np.random.default_rng(rows)
    for c in (1, 3):
        a, b = _f32(rng, rows, c), _f32(rng, rows, c)
        terms = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
        got = H.dot(_embed(H, a)[1], _embed(H, b, 1, 5)[1], rows)
        assert abs(got - terms.sum()) <= (rows * c - 1) * EPS * np.abs(terms).sum(), ("dot", rows, c)
    for cols in COLS:
        a, b = _f32(rng, rows, cols), _f32(rng, rows, cols)
        out = H.to_device(np.full(cols + 3, 7.0))
        H.coldot(_embed(H, a)[1], _embed(H, b, 1, 5)[1], rows, cols, out)
        H.sync()
        terms = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
        got = out.cpu().numpy()
        assert np.all(np.abs(got[:cols] - terms.sum(axis=0)) <= (rows - 1) * EPS * np.abs(terms).sum(axis=0)), ("coldot", rows, cols)
        assert np.all(got[cols:] == 7.0)
        out = H.to_device(np.full(cols + 3, 7.0))
        H.colsumsq(_embed(H, a)[1], out)
        H.sync()
        terms = np.asarray(a, dtype=LD) ** 2
        got = out.cpu().numpy()
        assert np.all(np.abs(got[:cols] - terms.sum(axis=0)) <= (rows - 1) * EPS * terms.sum(axis=0)), ("colsumsq", rows, cols)
        assert np.all(got[cols:] == 7.0)


@pytest.mark.parametrize("n", ROWS)
def test_trace_dot(H, n):
    """sum_ij (W_ij - b_i b_j) D_ij without b, with a contiguous b and with b as a column of an (n, 3) array"""
    rng = np.random.default_rng(n + 50)
    W, D, b = _fixed(rng, n, n), _fixed(rng, n, n), _fixed(rng, n)
    Wd, Dd = _embed(H, W, 1, 3)[1], _embed(H, D, 2, 1)[1]
    b3 = np.full((n, 3), np.nan)
    b3[:, 2] = b
    for bd, bb in ((None, None), (H.to_device(b), b), (H.to_device(b3)[:, 2], b)):
        Wl = np.asarray(W, dtype=LD) - (0 if bb is None else np.outer(np.asarray(bb, dtype=LD), np.asarray(bb, dtype=LD)))
        terms = Wl * np.asarray(D, dtype=LD)
        got = H.trace_dot(Wd, Dd, bd, n)
        assert abs(got - terms.sum()) <= (n * n - 1) * EPS * np.abs(terms).sum(), (n, bb is None)


@pytest.mark.parametrize("n", ROWS)
def test_add_lower_and_symmetrize(H, n):
    """A[i][j] += alpha B[i][j] for j <= i < n: one rounding per entry, as numpy's A + alpha * B with alpha a power of two; the strict
    upper triangle and everything outside n x n keep their bits.  symmetrize: the upper triangle becomes bitwise the lower one, the lower
    triangle and everything outside n x n keep their bits."""
    rng = np.random.default_rng(n + 60)
    a, b = rng.standard_normal((n + 2, n + 3)), rng.standard_normal((n + 1, n + 5))
    il = np.tril_indices(n)
    for alpha in (1.0, -0.5):
        A = H.to_device(a)
        H.add_lower(A, n, H.to_device(b), alpha)
        H.sync()
        want = a.copy()
        want[:n, :n][il] = a[:n, :n][il] + alpha * b[:n, :n][il]
        assert A.cpu().numpy().tobytes() == want.tobytes(), (n, alpha)
    A = H.to_device(a)
    H.symmetrize(A, n)
    H.sync()
    want = a.copy()
    want[:n, :n] = np.tril(a[:n, :n]) + np.tril(a[:n, :n], -1).T
    assert A.cpu().numpy().tobytes() == want.tobytes(), n


@pytest.mark.parametrize("rows", ROWS)
def test_add_matrix(H, rows):
    """A += alpha B on the rectangle of B's shape, exact against numpy; everything outside the rectangle keeps its bits"""
    rng = np.random.default_rng(rows + 70)
    for cols in COLS:
        a, b = rng.standard_normal((rows + 2, cols + 3)), rng.standard_normal((rows, cols))
        for alpha in (1.0, -0.5):
            A = H.to_device(a)
            H.add_matrix(A, _embed(H, b, 1, 2)[1], alpha)
            H.sync()
            want = a.copy()
            want[:rows, :cols] = a[:rows, :cols] + alpha * b
            assert A.cpu().numpy().tobytes() == want.tobytes(), (rows, cols, alpha)


@pytest.mark.parametrize("n", [300, 1000])
def test_trsm_lower_t(H, n):
    """L^T X = B with 128 right-hand sides on the factor of B B^T + n I against scipy at the 1e-12 bar of test_potrf_solve_logdet; the
    padding rows of the right-hand side come back zero; a number of right-hand sides that is no multiple of 128 is refused (-6)"""
    from fvgp_amd import _lib
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n))
    M = G @ G.T + n * np.eye(n)
    npad = _lib.pad128(n)
    buf = np.zeros((npad, npad))
    buf[:n, :n] = np.tril(M)
    buf[n:, n:] = np.eye(npad - n)
    A = H.to_device(buf)
    assert H.potrf(A, n) == 0
    Lref = np.tril(sla.cho_factor(M, lower=True)[0])
    rhs = rng.standard_normal((n, 128))
    rb = np.full((npad, 128), 5.0)
    rb[:n] = rhs
    Bd = H.to_device(rb)
    H.trsm_lower_t(A, n, Bd, 128)
    H.sync()
    got = Bd.cpu().numpy()
    want = sla.solve_triangular(Lref.T, rhs, lower=False)
    assert np.max(np.abs(got[:n] - want)) / np.max(np.abs(want)) < 1e-12
    assert np.all(got[n:] == 0)
    with pytest.raises(_lib.HipExtensionError, match="status -6"):
        H.trsm_lower_t(A, n, H.zeros(npad, 128), 100)
