"""The nearest-neighbour (Vecchia) path on the device (include/fvgp_hip_nn.h, fvgp_amd/gp_vecchia.py): the search by property and, where
distances are exact, against the twin's lists; the conditionals and the likelihood against longdouble under bars that come from the
float64 twin (vecchia_ref: MARGIN * max(base, FLOOR)); the likelihood against the dense GP where the approximation is exact; the bit
contracts; failure reporting; the facade.  Run with -s for the record lines."""
import ctypes
import warnings

import numpy as np
import pytest

import vecchia_ref as vr
from vecchia_device import CANARY, _device_loglik, _frame_untouched, _framed, _kid

pytestmark = pytest.mark.gpu

ICANARY = -7777
LD = vr.LD


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _framed_idx(H, nq, m):
    """an int32 canary buffer with a frame of rows and columns around the (nq, m) result and an odd leading dimension: (buffer, view)"""
    t = H.torch
    odd = 3 if m % 2 == 0 else 4
    big = t.full((nq + 2, m + odd), ICANARY, dtype=t.int32, device=f"cuda:{H.device}")
    assert big.stride(0) % 2 == 1
    return big, big[1:1 + nq]


def _idx_frame_untouched(big, nq, m):
    a = big.cpu().numpy()
    return np.all(a[0] == ICANARY) and np.all(a[1 + nq:] == ICANARY) and np.all(a[:, m:] == ICANARY)


def _search(H, xq, xr, m, scales=None, c0=-1):
    """Handle.nn_search into a framed result: the (nq, m) lists on the host"""
    xqd = H.to_device(xq)
    xrd = xqd if xr is xq else H.to_device(xr)
    big, view = _framed_idx(H, len(xq), m)
    H.nn_search(xqd, xrd, m, view, scales=scales, c0=c0)
    H.sync()
    assert _idx_frame_untouched(big, len(xq), m)
    return view.cpu().numpy()[:, :m].copy()


# ---- 1. the search ------------------------------------------------------------------------------------------------------------------------
# (nq, nr, d, m, scaled, c0): the sizes around one block of 64 queries and one staged slice of 128 rows, every padded list size, the four
# dimensions' code paths; c0 = 0 searches the rows among themselves, c0 = 700 the last 300 of 1000 rows as appended ones
SEARCH_CASES = [(1, 1, 1, 1, False, -1), (2, 2, 3, 16, True, 0), (63, 64, 5, 17, False, -1), (64, 65, 16, 64, True, -1),
                (65, 63, 3, 64, False, -1), (257, 257, 3, 17, True, 0), (1000, 1000, 3, 16, True, 0), (300, 1000, 5, 64, False, 700),
                (257, 1000, 1, 64, True, -1), (1000, 2, 16, 1, False, -1), (64, 257, 5, 16, True, 0)]


@pytest.mark.parametrize("nq,nr,d,m,scaled,c0", SEARCH_CASES)
def test_search_properties(H, nq, nr, d, m, scaled, c0):
    rng = np.random.default_rng(100 * nq + nr + d + m)
    xr = rng.random((nr, d))
    if c0 == 0:
        nq = min(nq, nr)
        xq = xr[:nq] if nq < nr else xr
    elif c0 > 0:
        xq = xr[c0:]
        assert len(xq) == nq
    else:
        xq = rng.random((nq, d))
    scales = 0.2 + rng.random(d) if scaled else None
    idx = _search(H, xq, xr, m, scales, c0)
    vr.check_search_rows(idx, xq, xr, m, scales, c0)
    # a row alone has the bits it has in the larger call
    for i in sorted({0, nq // 2, nq - 1}):
        one = _search(H, xq[i:i + 1], xr, m, scales, c0 if c0 < 0 else c0 + i)
        assert np.array_equal(one[0], idx[i]), i


def test_search_across_the_launch_cut(H):
    """more than 65536 queries go in several launches: the causal offset moves with the cut, the rows on both sides of it are right"""
    nq, nr, m = 65536 + 70, 70000, 2
    rng = np.random.default_rng(77)
    xr = rng.random((nr, 1))
    idx = _search(H, xr[:nq], xr, m, None, 0)
    for s, e in ((0, 64), (65500, nq)):
        vr.check_search_rows(idx[s:e], xr[s:e], xr, m, None, s)
    far = _search(H, xr[:nq], xr[:5], m, np.array([0.5]), -1)
    vr.check_search_rows(far[65500:], xr[65500:nq], xr[:5], m, np.array([0.5]), -1)


def test_search_ties_equal_the_twin(H):
    # duplicated points and a regular grid: every distance is exactly representable, so the lists are the twin's
    base = np.random.default_rng(9).integers(0, 4, (40, 3)).astype(np.float64)
    x = np.vstack([base, base, base[:13]])
    for m, c0 in ((5, -1), (17, 0), (64, -1)):
        assert np.array_equal(_search(H, x, x, m, None, c0), vr.search_ref(x, x, m, None, c0)), (m, c0)
    g = np.stack(np.meshgrid(np.arange(13.0), np.arange(11.0), indexing="ij"), axis=-1).reshape(-1, 2)
    sc = np.array([1.0, 2.0])
    for m, c0 in ((8, 0), (33, -1), (64, 0)):
        idx = _search(H, g, g, m, sc, c0)
        assert np.array_equal(idx, vr.search_ref(g, g, m, sc, c0)), (m, c0)
        vr.check_search_rows(idx, g, g, m, sc, c0)
    q = g[:70] + 0.5
    assert np.array_equal(_search(H, q, g, 16, sc, -1), vr.search_ref(q, g, 16, sc, -1))


def test_search_argument_rules(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    x = H.to_device(np.random.default_rng(1).random((10, 3)))
    big, out = _framed_idx(H, 10, 4)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    bad = (ctypes.c_double * 3)(1.0, 0.0, 1.0)

    def call(**kw):
        a = dict(h=H._h, xq=P(x), nq=10, xr=P(x), nr=10, d=3, sc=None, m=4, c0=0, out=P(out), ld=out.stride(0))
        a.update(kw)
        return L.fvgp_hip_nn_search(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(xq=None)), (-3, dict(nq=0)), (-4, dict(xr=None)), (-5, dict(nr=0)), (-5, dict(nr=2 ** 31)),
                     (-6, dict(d=0)), (-6, dict(d=17)), (-7, dict(sc=bad)), (-8, dict(m=0)), (-8, dict(m=65)), (-10, dict(out=None)),
                     (-11, dict(ld=3))):
        assert call(**kw) == code, (code, kw)
    H.sync()
    assert np.all(big.cpu().numpy() == ICANARY)


# ---- 2. conditionals and likelihood against longdouble ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.ACC_CASES, ids=vr.case_id)
def test_conditionals_and_likelihood_against_longdouble(H, case):
    """Bars from the float64 twin, never from the device: every figure <= MARGIN * max(base, FLOOR) (vecchia_ref)."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    out, info, mu, var = _device_loglik(H, case)
    assert info == 0
    bars = vr.bars(case)
    worst = dict.fromkeys(vr.FIGURES, 0.0)
    for b in range(B):
        f = vr.figures(r, (out[b, 0], out[b, 1], out[b, 2], mu[b], var[b]), vr.reference(case)[b])
        worst = {k: max(worst[k], f[k]) for k in vr.FIGURES}
    print(f"\nvecchia device {vr.case_id(case)}: " + " ".join(f"{k}={worst[k]:.2e}/{bars[k]:.2e}" for k in vr.FIGURES))
    # the conditionals entry on the same inputs is the likelihood's first half, bit for bit
    xd = H.to_device(x)
    mu2, var2 = H.empty(B, n), H.empty(B, n)
    idx_d = H.torch.as_tensor(np.ascontiguousarray(idx), device=xd.device)
    vd = H.to_device(v)
    assert H.nn_conditionals(_kid(name), xd, xd, thetas, idx_d, m, H.to_device(r), vd, mu2, var2, s=vd) == 0
    assert np.array_equal(mu2.cpu().numpy(), mu) and np.array_equal(var2.cpu().numpy(), var)
    for k in vr.FIGURES:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])


def _facade_pair(case, **kw):
    """(VecchiaGP, y, x, theta, v) over a case's data with y = r + 0.7"""
    import fvgp_amd
    name, d, n, m, _ = case
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    gp = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, **kw)
    return gp, y, x, theta, v


def test_likelihood_is_the_dense_one_when_every_earlier_point_is_a_neighbour(H):
    """n = 65, m = 64 on the given order: the product of conditionals is the exact likelihood, so the new path must agree with the
    dense GP.log_likelihood on the same data under the accuracy bar of this case."""
    import fvgp_amd
    case = vr.EXACT_CASE
    name = case[0]
    vg, y, x, theta, v = _facade_pair(case, ordering="given")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=v, kernel_function=name)
    got, want = vg.log_likelihood(), gp.log_likelihood(theta)
    bar = vr.bars(case)["loglik"]
    exact = float(vr.dense_loglik_ld(name, x, theta, y - np.mean(y), v))
    print(f"\nvecchia exactness n=65 m=64: vecchia {got!r} dense {want!r} longdouble {exact!r} rel {abs(got - want) / abs(want):.2e}/{bar:.2e}")
    assert abs(got - want) <= bar * abs(want)
    assert abs(got - exact) <= bar * abs(exact)
    nb = vg.neighbors()
    assert all(sorted(nb[i][nb[i] >= 0]) == list(range(i)) for i in range(65))


def test_conditionals_argument_rules(H):
    """a bad argument returns minus its position before anything is launched: outputs and workspace stay as they were"""
    from fvgp_amd import _lib
    L = _lib.lib()
    n, m, B = 10, 4, 2
    t = H.torch
    x = H.to_device(np.random.default_rng(1).random((n, 3)))
    r, v = H.to_device(np.ones(n)), H.to_device(np.ones(n))
    idx = t.full((n, m), -1, dtype=t.int32, device=x.device)
    mbig, mu = _framed(H, B, n)
    vbig, var = _framed(H, B, n)
    wb = _lib.nn_workspace_bytes(_lib.NN_LOGLIK, n, B)
    work = t.full((wb // 8,), CANARY, dtype=t.float64, device=x.device)
    th = np.ones((B, 4))
    out = np.full((B, 3), CANARY)
    info = ctypes.c_int64(-5)
    P = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    tp = th.ctypes.data_as(_lib.P_d)

    def cond(**kw):
        a = dict(h=H._h, kid=1, xq=P(x), nq=n, xr=P(x), nr=n, d=3, th=tp, nt=4, B=B, idx=P(idx), ld=m, m=m, r=P(r), v=P(v), s=None,
                 mu=P(mu), var=P(var), w=P(work), wb=wb, info=ctypes.byref(info))
        a.update(kw)
        return L.fvgp_hip_nn_conditionals(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=6)), (-3, dict(xq=None)), (-4, dict(nq=0)), (-5, dict(xr=None)), (-6, dict(nr=0)),
                     (-7, dict(d=17)), (-8, dict(th=None)), (-9, dict(nt=3)), (-10, dict(B=0)), (-10, dict(B=65536)), (-11, dict(idx=None)),
                     (-12, dict(ld=3)), (-13, dict(m=0)), (-13, dict(m=65)), (-14, dict(r=None)), (-15, dict(v=None)), (-17, dict(mu=None)),
                     (-18, dict(var=None)), (-19, dict(w=None)), (-20, dict(wb=8)), (-21, dict(info=None))):
        assert cond(**kw) == code, (code, kw)

    def loglik(**kw):
        a = dict(h=H._h, kid=1, x=P(x), n=n, d=3, th=tp, nt=4, B=B, idx=P(idx), ld=m, m=m, r=P(r), v=P(v), mu=P(mu), var=P(var),
                 w=P(work), wb=wb, out=out.ctypes.data_as(_lib.P_d), info=ctypes.byref(info))
        a.update(kw)
        return L.fvgp_hip_nn_loglik(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=-1)), (-3, dict(x=None)), (-4, dict(n=0)), (-5, dict(d=0)), (-6, dict(th=None)),
                     (-7, dict(nt=3)), (-8, dict(B=0)), (-9, dict(idx=None)), (-10, dict(ld=3)), (-11, dict(m=65)), (-12, dict(r=None)),
                     (-13, dict(v=None)), (-14, dict(mu=None)), (-15, dict(var=None)), (-16, dict(w=None)),
                     (-17, dict(wb=_lib.nn_workspace_bytes(_lib.NN_CONDITIONALS, n, B))), (-18, dict(out=None)), (-19, dict(info=None))):
        assert loglik(**kw) == code, (code, kw)
    H.sync()
    assert info.value == -5 and np.all(out == CANARY) and np.all(work.cpu().numpy() == CANARY)
    assert np.all(mbig.cpu().numpy() == CANARY) and np.all(vbig.cpu().numpy() == CANARY)
    # and the good call: rows without neighbours return mu = 0 and d = k(x, x) + s
    assert loglik() == 0 and info.value == 0
    assert np.all(mu.cpu().numpy() == 0.0) and np.all(var.cpu().numpy() == 2.0)


# ---- 3. bit contracts ------------------------------------------------------------------------------------------------------------------------
def test_bit_contracts(H):
    case = ("matern52_ard", 3, 200, 33, 3)
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    out, info, mu, var = _device_loglik(H, case)
    out2, _, mu2, var2 = _device_loglik(H, case)
    assert info == 0 and np.array_equal(out, out2) and np.array_equal(mu, mu2) and np.array_equal(var, var2), "the likelihood twice"
    # every batch position, and each theta alone
    for b in range(B):
        o1, _, m1, v1 = _device_loglik(H, case, thetas=thetas[b:b + 1])
        assert np.array_equal(o1[0], out[b]) and np.array_equal(m1[0], mu[b]) and np.array_equal(v1[0], var[b]), b
    perm = np.array([2, 0, 1])
    o3, _, m3, v3 = _device_loglik(H, case, thetas=thetas[perm])
    assert np.array_equal(o3, out[perm]) and np.array_equal(m3, mu[perm]) and np.array_equal(v3, var[perm])
    # a row alone (one query against the same reference rows) has the bits it has in the call of 200 rows
    xd, rd, vd = H.to_device(x), H.to_device(r), H.to_device(v)
    for i in (0, 1, 33, 130, 199):
        idx_d = H.torch.as_tensor(np.ascontiguousarray(idx[i:i + 1]), device=xd.device)
        m1, v1 = H.empty(B, 1), H.empty(B, 1)
        assert H.nn_conditionals(_kid(name), xd[i:i + 1], xd, thetas, idx_d, m, rd, vd, m1, v1, s=vd[i:i + 1]) == 0
        assert np.array_equal(m1.cpu().numpy()[:, 0], mu[:, i]) and np.array_equal(v1.cpu().numpy()[:, 0], var[:, i]), i


# ---- 4. failure reporting ------------------------------------------------------------------------------------------------------------------------
def test_failure_is_reported_not_trapped(H):
    """zero noise and a duplicated point among a row's neighbours, with sigma^2 a power of four so that the arithmetic is exact: the
    block [[s, s], [s, s]] has the second pivot s - (s / sqrt(s))^2 = 0 exactly.  The call reports the smallest failing (b, row); frames
    stay intact and every other row is what it is in a call without the singular list.  A numerical condition: nothing faults."""
    import fvgp_amd
    name, d, n, m = "rbf_ard", 2, 40, 16
    x, theta, r, _ = vr.case_data(name, d, n)
    x = x.copy()
    x[7] = x[3]                                   # rows 3 and 7 coincide
    v0 = np.zeros(n)
    idx = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        prev = np.arange(i)[-3:][::-1]            # the three rows before it: none of these lists holds both 3 and 7
        idx[i, :len(prev)] = prev
    idx[20, :3] = [3, 7, 5]                       # row 20 lists both copies
    thetas = np.array([np.concatenate([[4.0], theta[1:]]), np.concatenate([[1.0], 1.5 * theta[1:]])])
    t = H.torch
    xd, rd, vd = H.to_device(x), H.to_device(r), H.to_device(v0)
    mbig, mu = _framed(H, 2, n)
    vbig, var = _framed(H, 2, n)
    out, info = H.nn_loglik(_kid(name), xd, thetas, t.as_tensor(idx, device=xd.device), m, rd, vd, mu, var)
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    assert _frame_untouched(mbig) and _frame_untouched(vbig)
    bad = ~(var > 0.0)
    assert bad[0, 20] and bad[1, 20] and bad.sum() == 2, "the singular row fails at both thetas, no other row does"
    assert info == 1 + 0 * n + 20
    assert np.all(np.isnan(out[:, 0]))
    out1, info1 = H.nn_loglik(_kid(name), xd, thetas[1:], t.as_tensor(idx, device=xd.device), m, rd, vd, H.empty(1, n), H.empty(1, n))
    assert info1 == 1 + 20 and np.isnan(out1[0, 0])
    # the other rows are what they are in a call whose row 20 lists one copy only
    idx2 = idx.copy()
    idx2[20, :3] = [3, 5, -1]
    mu2, var2 = H.empty(2, n), H.empty(2, n)
    out2, info2 = H.nn_loglik(_kid(name), xd, thetas, t.as_tensor(idx2, device=xd.device), m, rd, vd, mu2, var2)
    keep = np.arange(n) != 20
    assert info2 == 0 and np.all(np.isfinite(out2))
    assert np.array_equal(mu2.cpu().numpy()[:, keep], mu[:, keep]) and np.array_equal(var2.cpu().numpy()[:, keep], var[:, keep])
    # through the facade the same condition raises and names the data point: point 1 is a copy of point 0, its only neighbour
    xx = np.vstack([x[3:4], x[3:4], x[:3]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vg = fvgp_amd.VecchiaGP(xx, r[:5] + 1.0, thetas[0], kernel_function=name, n_neighbors=4, ordering="given")
    vg._V_dev.zero_()                              # (the facade refuses zero noise at the door: take it away behind it)
    with pytest.raises(fvgp_amd.NonPositiveDefiniteError, match="data point 1 "):
        vg.log_likelihood()
    assert np.isnan(vg.log_likelihood_batch(thetas[:1])[0])


# ---- 5. the facade ------------------------------------------------------------------------------------------------------------------------
FACADE_CASE = ("matern32_ard", 3, 200, 17, 1)


def test_facade_orders_and_predicts_like_the_twin(H):
    case = FACADE_CASE
    name, d, n, m, _ = case
    vg, y, x, theta, v = _facade_pair(case, seed=5)
    perm = vg.ordering
    assert sorted(perm) == list(range(n)) and not np.array_equal(perm, np.arange(n))
    r = y - np.mean(y)
    sc = vr.length_scales(name, theta, d)
    xo, ro, vo = x[perm], r[perm], v[perm]
    idx = vr.search_ref(xo, xo, m, sc, c0=0)
    nb = vg.neighbors()
    assert np.array_equal(nb[perm], np.where(idx >= 0, perm[np.clip(idx, 0, None)], -1))
    ll, _, _, mu, dd = vr.loglik_ref(name, xo, theta, idx, ro, vo, LD)
    tol = vr.MARGIN * 1e-12                       # (the accuracy proper is section 2's: here the plumbing)
    got = vg.log_likelihood()
    assert abs(got - float(ll)) <= tol * abs(float(ll)) and vg.neg_log_likelihood() == -got
    c = vg.conditionals()
    want_mu, want_d = np.empty(n), np.empty(n)
    want_mu[perm], want_d[perm] = np.asarray(mu, dtype=np.float64) + np.mean(y), np.asarray(dd, dtype=np.float64)
    assert np.max(np.abs(c["mean"] - want_mu)) <= tol * np.max(np.abs(y)) and np.max(np.abs(c["variance"] / want_d - 1)) <= tol
    assert abs(np.sum(c["log_predictive"]) - got) <= 1e-12 * abs(got)
    # batch rows are the single calls, bit for bit
    thetas = vr.batch_thetas(theta, 3)
    lb = vg.log_likelihood_batch(thetas)
    assert lb.shape == (3,) and all(lb[b] == vg.log_likelihood(thetas[b]) for b in range(3)) and lb[0] == got
    assert np.array_equal(vg.neg_log_likelihood_batch(thetas), -lb)
    # prediction at 37 points: the m nearest data points of each, under the same scales
    xp = np.random.default_rng(3).random((37, d))
    pidx = vr.search_ref(xp, xo, m, sc, c0=-1)
    pm, pv = vr.conditionals_ref(name, xp, xo, theta, pidx, ro, vo, None, LD)
    gm, gv = vg.posterior_mean(xp), vg.posterior_covariance(xp)
    assert np.array_equal(gm["x"], xp) and np.max(np.abs(gm["m(x)"] - (np.asarray(pm, dtype=np.float64) + np.mean(y)))) <= tol * np.max(np.abs(y))
    assert np.max(np.abs(gv["v(x)"] / np.asarray(pv, dtype=np.float64) - 1)) <= tol
    gn = vg.posterior_covariance(xp, add_noise=True)["v(x)"]
    assert np.allclose(gn - gv["v(x)"], np.mean(v), rtol=1e-9)
    assert vg.posterior_covariance(xp[5:6])["v(x)"][0] == gv["v(x)"][5] and vg.posterior_mean(xp[5:6])["m(x)"][0] == gm["m(x)"][5]


def test_facade_equals_the_dense_gp_with_every_point_a_neighbour(H):
    import fvgp_amd
    name, d, n, m = "matern52_ard", 2, 50, 64
    vg, y, x, theta, v = _facade_pair((name, d, n, m, 1), seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=v, kernel_function=name)
    xp = np.random.default_rng(4).random((37, d))
    bars = vr.bars(("matern52_ard", 2, 200, 33, 1))           # the accuracy case of this kernel and dimension
    dm, dv = gp.posterior_mean(xp)["m(x)"], gp.posterior_covariance(xp, variance_only=True)["v(x)"]
    gm, gv = vg.posterior_mean(xp)["m(x)"], vg.posterior_covariance(xp)["v(x)"]
    r = y - np.mean(y)
    print(f"\nvecchia m >= n vs dense: mean {np.max(np.abs(gm - dm)) / np.max(np.abs(r)):.2e}/{bars['mu']:.2e} "
          f"var {np.max(np.abs(gv / dv - 1)):.2e}/{bars['d']:.2e}")
    assert np.max(np.abs(gm - dm)) <= bars["mu"] * np.max(np.abs(r))
    assert np.max(np.abs(gv / dv - 1)) <= bars["d"]
    # the variance at a data point with the noise added, point for point
    assert vg.posterior_covariance(x, add_noise=True)["v(x)"].shape == (n,)


def test_facade_update_hyperparameters_training_and_handover(H):
    import fvgp_amd
    case = FACADE_CASE
    name, d, n, m, _ = case
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    k = 150
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = fvgp_amd.VecchiaGP(x[:k], y[:k], theta, noise_variances=v[:k], kernel_function=name, n_neighbors=m, seed=11)
        a.update_gp_data(x[k:], y[k:], noise_variances_new=v[k:])
        order = np.concatenate([np.random.default_rng(11).permutation(k), np.arange(k, n)])
        b = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, ordering=order)
    assert a.point_number == n and np.array_equal(a.ordering, b.ordering) and np.array_equal(a.neighbors(), b.neighbors())
    assert a.log_likelihood() == b.log_likelihood() and a._m == b._m
    # set_hyperparameters leaves the lists alone, refresh_neighbors rebuilds them under the new length scales
    before = b.neighbors()
    th2 = theta * np.array([1.0, 4.0, 0.25, 1.0])
    b.set_hyperparameters(th2)
    assert np.array_equal(b.neighbors(), before) and np.array_equal(b.hyperparameters, th2)
    b.refresh_neighbors()
    assert not np.array_equal(b.neighbors(), before)
    assert np.array_equal(b.neighbors()[b.ordering],
                          np.where((i := vr.search_ref(x[order], x[order], m, th2[1:], 0)) >= 0, order[np.clip(i, 0, None)], -1))
    # a short chain does not end above where it started; the lists stay fixed while it runs
    b.set_hyperparameters(theta)
    lists = b.neighbors()
    bounds = np.array([[0.1, 10.0]] + [[0.05, 5.0]] * d)
    start = b.neg_log_likelihood()
    np.random.seed(3)
    hps = b.train(bounds, method="mcmc", max_iter=25)
    assert hps.shape == theta.shape and np.array_equal(b.hyperparameters, hps) and np.array_equal(b.neighbors(), lists)
    assert -b.mcmc_info["max f(x)"] <= start
    hps = b.train(bounds, init_hyperparameters=theta, method="global", max_iter=2, pop_size=4, seed=1)
    assert b.neg_log_likelihood() <= start
    # GP.vecchia carries kernel and hyperparameters over
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x[:60], y[:60], init_hyperparameters=theta, noise_variances=v[:60], kernel_function=name)
    vg = gp.vecchia(n_neighbors=9)
    assert isinstance(vg, fvgp_amd.VecchiaGP) and vg._native.name == name and np.array_equal(vg.hyperparameters, gp.hyperparameters)
    assert vg.point_number == 60 and vg.n_neighbors == 9 and np.array_equal(vg._V, v[:60])
    big = gp.vecchia(x, y, v, n_neighbors=12, ordering="given")
    assert big.point_number == n and np.array_equal(big.ordering, np.arange(n))


def test_facade_refusals(H):
    import fvgp_amd
    name, d, n = "rbf_iso", 2, 30
    x, theta, r, v = vr.case_data(name, d, n)
    kw = dict(noise_variances=v, kernel_function=name)
    with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
        fvgp_amd.VecchiaGP(x, r, theta, noise_variances=v, kernel_function=lambda a, b, h: np.eye(len(a)))
    with pytest.raises(NotImplementedError, match="fvGP / x_out"):
        fvgp_amd.VecchiaGP(x, np.stack([r, r], axis=1), theta, **kw)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        fvgp_amd.VecchiaGP(x, r, theta, args={"process_group": True}, **kw)
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="n_neighbors must lie in 1 .. 64"):
            fvgp_amd.VecchiaGP(x, r, theta, n_neighbors=bad, **kw)
    with pytest.raises(NotImplementedError, match="input dimension <= 16"):
        fvgp_amd.VecchiaGP(np.zeros((5, 17)), np.zeros(5), np.ones(2), noise_variances=np.ones(5), kernel_function=name)
    with pytest.raises(ValueError, match="ordering"):
        fvgp_amd.VecchiaGP(x, r, theta, ordering=np.zeros(n, dtype=int), **kw)
    with pytest.raises(ValueError, match="neighbor_scales"):
        fvgp_amd.VecchiaGP(x, r, theta, args={"neighbor_scales": "nearest"}, **kw)
    with pytest.warns(UserWarning, match="No noise function or measurement noise provided"):
        vg = fvgp_amd.VecchiaGP(x, r + 2.0, theta, kernel_function=name, n_neighbors=5)
    assert np.allclose(vg._V, (np.mean(np.abs(r + 2.0)) / 100.0) ** 2)
    xp = x[:4] + 0.01
    with pytest.raises(NotImplementedError, match="MatrixFreeGP.*dense fvgp_amd.GP"):
        vg.posterior_covariance(xp, variance_only=False)
    with pytest.raises(NotImplementedError, match="x_out"):
        vg.posterior_mean(xp, x_out=np.array([0]))
    bounds = np.array([[0.1, 10.0], [0.05, 5.0]])
    for method in ("local", "adam", "hgdl"):
        with pytest.raises(NotImplementedError, match="gradient of the nearest-neighbour likelihood is not built yet"):
            vg.train(bounds, method=method)
    with pytest.raises(NotImplementedError, match="not built yet"):
        vg.neg_log_likelihood_gradient()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, r, init_hyperparameters=theta, noise_variances=v, kernel_function=lambda a, b, h: h[0] * np.exp(-kf_dist(a, b) / h[1]))
    with pytest.raises(NotImplementedError, match="kernel callable stays with the dense GP"):
        gp.vecchia()


def kf_dist(a, b):
    return np.sqrt(np.sum((a[:, None, :] - b[None, :, :]) ** 2, axis=2))
