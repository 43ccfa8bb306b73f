"""The maxmin ordering of the nearest-neighbour path on the device (include/fvgp_hip_nn.h: fvgp_hip_nn_maxmin_order): by
property under vecchia_order_ref.check_maxmin (distances in longdouble, a slack derived from the roundings of a double distance); element
for element against the twin where every distance is exact; the bit contracts; the argument rules; the facade (ordering="maxmin"); and
the reason it exists, the lower KL than random orderings, under a bar the twin sets.  Run with -s for the record lines."""
import ctypes
import warnings

import numpy as np
import pytest

import vecchia_order_ref as vo
import vecchia_ref as vr
from vecchia_device import CANARY, _frame_untouched, _framed

pytestmark = pytest.mark.gpu

ICANARY = -7777
LD = vr.LD


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _framed_perm(H, q):
    big = H.torch.full((q + 16,), ICANARY, dtype=H.torch.int64, device=f"cuda:{H.device}")
    return big, big[8:8 + q]


def _perm_frame_untouched(big):
    a = big.cpu().numpy()
    return np.all(a[:8] == ICANARY) and np.all(a[-8:] == ICANARY)


def _order(H, x, scales, first, q, want_dist=True):
    """the entry itself into canary-framed outputs: (perm (q,), dist2 (q,) or None) on the host"""
    from fvgp_amd import _lib
    n, d = x.shape
    xd = H.to_device(x)
    pbig, perm = _framed_perm(H, q)
    dbig, dist = _framed(H, q) if want_dist else (None, None)
    work = H.empty(_lib.nn_maxmin_workspace_bytes(n) // 8)
    sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
    rc = _lib.lib().fvgp_hip_nn_maxmin_order(H._h, _ptr(xd), n, d, None if sc is None else sc.ctypes.data_as(_lib.P_d), first, q, _ptr(perm),
                                             _ptr(dist), _ptr(work), work.numel() * 8)
    assert rc == 0, rc
    H.sync()
    assert _perm_frame_untouched(pbig) and (dbig is None or _frame_untouched(dbig))
    return perm.cpu().numpy().copy(), None if dist is None else dist.cpu().numpy().copy()


# ---- 1. by property ------------------------------------------------------------------------------------------------------------------------
# (n, d, q, scaled, first): the sizes around one wave, one 256-thread workgroup and one or two strips, the four dimensions' code paths,
# q < n, `first` at both ends
PROPERTY_CASES = [(1, 1, 1, False, 0), (2, 3, 2, True, 1), (3, 2, 3, False, 2), (63, 5, 63, True, 0), (64, 16, 64, False, 63),
                  (65, 3, 65, True, 7), (257, 1, 257, False, 256), (1000, 3, 1000, True, 500), (1000, 16, 100, True, 0),
                  (4097, 2, 300, False, 4096)]


@pytest.mark.parametrize("n,d,q,scaled,first", PROPERTY_CASES)
def test_order_properties(H, n, d, q, scaled, first):
    rng = np.random.default_rng(1000 * n + 10 * d + q)
    x = rng.random((n, d))
    scales = 0.2 + rng.random(d) if scaled else None
    perm, dist2 = _order(H, x, scales, first, q)
    vo.check_maxmin(perm, dist2, x, scales, first)
    only, none = _order(H, x, scales, first, q, want_dist=False)
    assert none is None and np.array_equal(only, perm)


# ---- 2. the twin's ordering, element for element, where distances are exact ---------------------------------------------------------------------
def test_order_equals_the_twin_on_exact_distances(H):
    # the duplicated integer lattice and the grid of test_search_ties_equal_the_twin: every tie rule, duplicates last in index order
    base = np.random.default_rng(9).integers(0, 4, (40, 3)).astype(np.float64)
    x = np.vstack([base, base, base[:13]])
    g = np.stack(np.meshgrid(np.arange(13.0), np.arange(11.0), indexing="ij"), axis=-1).reshape(-1, 2)
    # one column of 8200 distinct integers in a shuffled order: 33 strips of 256 points, every step's pick crosses them
    line = np.random.default_rng(4).permutation(8200).astype(np.float64).reshape(-1, 1)
    for x_, sc, first in ((x, None, 0), (x, None, 92), (g, np.array([1.0, 2.0]), 71), (line, None, 4100)):
        n = len(x_)
        perm, dist2 = _order(H, x_, sc, first, n)
        rp, rd = vo.maxmin_ref(x_, sc, first, n)
        assert np.array_equal(perm, rp) and np.array_equal(dist2, rd), (n, first)
    # the duplicates come last, each copy in index order
    perm, dist2 = _order(H, x, None, 0, len(x))
    distinct = len(np.unique(x, axis=0))
    assert np.all(dist2[distinct:] == 0.0) and np.all(dist2[1:distinct] > 0.0)
    assert list(perm[distinct:]) == sorted(perm[distinct:])
    vo.check_maxmin(perm, dist2, x, None, 0)


# ---- 3. the bit contracts -----------------------------------------------------------------------------------------------------------------------
def test_bit_contracts(H):
    rng = np.random.default_rng(31)
    n, d, q = 700, 3, 200
    x, sc = rng.random((n, d)), np.array([0.7, 1.3, 0.4])
    perm, dist2 = _order(H, x, sc, 5, q)
    again = _order(H, x, sc, 5, q)
    assert np.array_equal(again[0], perm) and np.array_equal(again[1], dist2)
    # the picks of a shorter call are the first of the longer one
    for qq in (1, 64, 65):
        p, d2 = _order(H, x, sc, 5, qq)
        assert np.array_equal(p, perm[:qq]) and np.array_equal(d2, dist2[:qq]), qq
    # APPENDED ROWS: mindist_t(i) depends on x[i] and the t earlier picks alone, so with rows appended to x nothing changes before
    # the first step T at which one of THEM is picked: positions < T hold the same picks and the same distances, bit for bit.
    full, fd = _order(H, x, sc, 5, n)
    extra = rng.random((90, d))
    p2, d2 = _order(H, np.vstack([x, extra]), sc, 5, n + 90)
    T = int(np.argmax(p2 >= n))
    assert 1 <= T < n and np.array_equal(p2[:T], full[:T]) and np.array_equal(d2[:T], fd[:T])
    # appended DUPLICATES tie with their originals until those are picked (the lower index wins) and have distance 0 afterwards: they
    # are picked last, T = n, and the whole ordering of x is a prefix
    p3, d3 = _order(H, np.vstack([x, x[:90]]), sc, 5, n + 90)
    assert np.array_equal(p3[:n], full) and np.array_equal(d3[:n], fd) and list(p3[n:]) == list(range(n, n + 90)) and np.all(d3[n:] == 0.0)


# ---- 4. the argument rules ------------------------------------------------------------------------------------------------------------------------
def test_order_argument_rules(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    n, d = 10, 3
    x = H.to_device(np.random.default_rng(1).random((n, d)))
    pbig, perm = _framed_perm(H, n)
    dbig, dist = _framed(H, n)
    work = H.empty(_lib.nn_maxmin_workspace_bytes(n) // 8)
    bad = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    inf = (ctypes.c_double * 3)(1.0, np.inf, 1.0)

    def call(**kw):
        a = dict(h=H._h, x=_ptr(x), n=n, d=d, sc=None, first=0, q=n, perm=_ptr(perm), dist=_ptr(dist), work=_ptr(work), wb=work.numel() * 8)
        a.update(kw)
        return L.fvgp_hip_nn_maxmin_order(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(x=None)), (-3, dict(n=0)), (-3, dict(n=2 ** 31)), (-4, dict(d=0)), (-4, dict(d=17)),
                     (-5, dict(sc=bad)), (-5, dict(sc=inf)), (-6, dict(first=-1)), (-6, dict(first=n)), (-7, dict(q=0)), (-7, dict(q=n + 1)),
                     (-8, dict(perm=None)), (-10, dict(work=None)), (-10, dict(work=ctypes.c_void_p(work.data_ptr() + 4))),
                     (-11, dict(wb=work.numel() * 8 - 8))):
        assert call(**kw) == code, (code, kw)
    H.sync()
    assert np.all(pbig.cpu().numpy() == ICANARY) and np.all(dbig.cpu().numpy() == CANARY)
    # the binding: shapes, defaults, refusals
    p, d2 = H.nn_maxmin_order(x, 3)
    assert p.dtype == np.int64 and p.shape == (n,) and d2.shape == (n,) and p[0] == 3 and d2[0] == np.inf and sorted(p) == list(range(n))
    p4, none = H.nn_maxmin_order(x, 3, q=4, want_distances=False)
    assert none is None and np.array_equal(p4, p[:4])
    with pytest.raises(ValueError, match="scales"):
        H.nn_maxmin_order(x, 0, scales=np.ones(2))
    with pytest.raises(_lib.HipExtensionError, match="status -7"):
        H.nn_maxmin_order(x, 0, q=n + 1)


# ---- 5. the facade ----------------------------------------------------------------------------------------------------------------------------
FACADE = ("matern32_ard", 3, 300, 17)


def _make(x, y, theta, v, name, m, **kw):
    import fvgp_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, **kw)


def _same_state(a, b):
    """two objects answer with the same bits"""
    assert np.array_equal(a.ordering, b.ordering) and np.array_equal(a.neighbors(), b.neighbors())
    assert a.log_likelihood() == b.log_likelihood()
    fa, ga = a.neg_log_likelihood_and_gradient()
    fb, gb = b.neg_log_likelihood_and_gradient()
    assert fa == fb and np.array_equal(ga, gb)
    ca, cb = a.conditionals(), b.conditionals()
    assert all(np.array_equal(ca[k], cb[k]) for k in ("mean", "variance", "log_predictive"))


def test_facade_maxmin_ordering(H):
    name, d, n, m = FACADE
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    a = _make(x, y, theta, v, name, m, ordering="maxmin")
    sc = vr.length_scales(name, theta, d)
    assert np.array_equal(a._scales, sc)
    first = vo.first_point(x, sc)
    perm, dist2 = _order(H, x, sc, first, n)
    vo.check_maxmin(a.ordering, dist2, x, a._scales, first)
    assert np.array_equal(a.ordering, perm) and a.ordering.dtype == np.int64
    assert np.array_equal(a.ordering_distances, np.sqrt(dist2)) and a.ordering_distances[0] == np.inf
    # the same state as an object handed that permutation; a rule without distances has None
    b = _make(x, y, theta, v, name, m, ordering=a.ordering)
    assert b.ordering_distances is None and _make(x, y, theta, v, name, m).ordering_distances is None
    _same_state(a, b)
    # per-point results come back in the caller's order: the twin's conditionals under that ordering
    xo, ro, vv = x[perm], r[perm], v[perm]
    idx = vr.search_ref(xo, xo, m, sc, c0=0)
    assert np.array_equal(a.neighbors()[perm], np.where(idx >= 0, perm[np.clip(idx, 0, None)], -1))
    ll, _, _, mu, dd = vr.loglik_ref(name, xo, theta, idx, ro, vv, LD)
    tol = vr.MARGIN * 1e-12                        # (the plumbing; the accuracy proper is test_gpu_vecchia.py's)
    c = a.conditionals()
    want_mu, want_d = np.empty(n), np.empty(n)
    want_mu[perm], want_d[perm] = np.asarray(mu, dtype=np.float64) + np.mean(y), np.asarray(dd, dtype=np.float64)
    assert np.max(np.abs(c["mean"] - want_mu)) <= tol * np.max(np.abs(y)) and np.max(np.abs(c["variance"] / want_d - 1)) <= tol
    assert abs(a.log_likelihood() - float(ll)) <= tol * abs(float(ll))

    # maxmin_points: the prefix of the full ordering, then the points left over in the stated random order
    p = _make(x, y, theta, v, name, m, ordering="maxmin", seed=4, args={"maxmin_points": 75})
    rest = np.setdiff1d(np.arange(n), perm[:75])
    assert np.array_equal(p.ordering[:75], perm[:75]) and np.array_equal(p.ordering[75:], rest[np.random.default_rng(4).permutation(n - 75)])
    assert np.array_equal(p.ordering_distances[:75], a.ordering_distances[:75]) and np.all(np.isnan(p.ordering_distances[75:]))
    _same_state(p, _make(x, y, theta, v, name, m, ordering=p.ordering))


def test_facade_maxmin_update_refresh_and_handover(H):
    import fvgp_amd
    name, d, n, m = FACADE
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    k = 250
    # append: the new points at the end, without an entry distance
    a = _make(x[:k], y[:k], theta, v[:k], name, m, ordering="maxmin")
    head = a.ordering.copy()
    a.update_gp_data(x[k:], y[k:], noise_variances_new=v[k:])
    assert np.array_equal(a.ordering, np.concatenate([head, np.arange(k, n)]))
    assert np.all(np.isfinite(a.ordering_distances[1:k])) and np.all(np.isnan(a.ordering_distances[k:])) and len(a.ordering_distances) == n
    _same_state(a, _make(x, y, theta, v, name, m, ordering=a.ordering))
    # replace: the rule runs again on the new data
    xr, yr, vv = x[:120][::-1].copy(), y[:120][::-1].copy(), v[:120][::-1].copy()
    a.update_gp_data(xr, yr, noise_variances_new=vv, append=False)
    fresh = _make(xr, yr, theta, vv, name, m, ordering="maxmin")
    assert a.point_number == 120 and np.array_equal(a.ordering_distances, fresh.ordering_distances)
    _same_state(a, fresh)
    # refresh_neighbors(reorder=True): the ordering under the new length scales, the state of a fresh object built there
    b = _make(x, y, theta, v, name, m, ordering="maxmin")
    before = b.ordering.copy()
    th2 = theta * np.array([1.0, 4.0, 0.25, 1.0])
    b.set_hyperparameters(th2)
    b.refresh_neighbors()
    assert np.array_equal(b.ordering, before)
    b.refresh_neighbors(reorder=True)
    fresh = _make(x, y, th2, v, name, m, ordering="maxmin")
    assert not np.array_equal(b.ordering, before) and np.array_equal(b.ordering_distances, fresh.ordering_distances)
    _same_state(b, fresh)
    rnd = _make(x, y, theta, v, name, m)
    with pytest.raises(ValueError, match="reorder"):
        rnd.refresh_neighbors(reorder=True)
    rnd.refresh_neighbors(reorder=False)
    # GP.vecchia passes the ordering through
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x[:60], y[:60], init_hyperparameters=theta, noise_variances=v[:60], kernel_function=name)
    vg = gp.vecchia(n_neighbors=9, ordering="maxmin")
    sc = vr.length_scales(name, theta, d)
    assert np.array_equal(vg.ordering, _order(H, x[:60], sc, vo.first_point(x[:60], sc), 60)[0]) and vg.ordering_distances is not None
    # "unit" scales order by the plain distance
    u = _make(x[:60], y[:60], theta, v[:60], name, 9, ordering="maxmin", args={"neighbor_scales": "unit"})
    assert np.array_equal(u.ordering, _order(H, x[:60], None, vo.first_point(x[:60], None), 60)[0])


def test_facade_maxmin_refusals(H):
    name, d, n, m = "rbf_iso", 2, 30, 5
    x, theta, r, v = vr.case_data(name, d, n)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[7, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            _make(xb, r, theta, v, name, m, ordering="maxmin")
    for bad in (0, n + 1, -2, 2.5, True):
        with pytest.raises(ValueError, match="maxmin_points"):
            _make(x, r, theta, v, name, m, ordering="maxmin", args={"maxmin_points": bad})
    assert _make(x, r, theta, v, name, m, ordering="maxmin", args={"maxmin_points": n}).ordering_distances[-1] >= 0.0
    with pytest.raises(ValueError, match="ordering must be .*'maxmin'"):
        _make(x, r, theta, v, name, m, ordering="minmax")


# ---- 6. what it buys, on the device ----------------------------------------------------------------------------------------------------------------
def test_maxmin_has_the_lower_kl_than_random_orderings_on_the_device(H):
    """sum log d of the maxmin object lies below that of each random-ordered object by more than HALF the margin the twin shows for the
    same seed (vecchia_order_ref.accuracy_case: computed from the twin alone, never from the device)."""
    name, d, n, m = vo.ACC
    x, theta, r, v, sc, twin_perm, mm, rnd = vo.accuracy_case()
    total = lambda g: float(np.sum(np.log(g.conditionals()["variance"])))      # noqa: E731
    a = _make(x, r, theta, v, name, m, ordering="maxmin")
    got = total(a)
    print(f"\nvecchia order device {name} d={d} n={n} m={m}: sum log d maxmin {got:.4f} (twin {float(mm):.4f}, same ordering: "
          f"{np.array_equal(a.ordering, twin_perm)})")
    for s in vo.ACC_SEEDS:
        g = _make(x, r, theta, v, name, m, ordering="random", seed=s)
        assert np.array_equal(g.ordering, np.random.default_rng(s).permutation(n))
        margin, want = total(g) - got, float(rnd[s] - mm)
        print(f"    seed {s}: random - maxmin {margin:.3f} (twin {want:.3f}, bar {want / 2:.3f})")
        assert margin > want / 2
