"""The cell-grid neighbour search on the device (include/fvgp_hip_nn.h: fvgp_hip_nn_grid_build, fvgp_hip_nn_grid_search; DESIGN 28;
VecchiaGP args["neighbor_search"]).  The reference is the brute entry, Handle.nn_search, on the same inputs, and the comparison is
np.array_equal: the grid route has to return the same lists element for element.  Results land in framed int32 canary buffers with an odd
leading dimension (those of test_gpu_vecchia.py) whose frame must stay untouched.  Shapes: the smallest at which the walk can go wrong --
one cell, several shells, both sides of the early-row cut (1024 or 4096 candidates), ties and rows on faces, queries outside the box, clusters."""
import ctypes

import numpy as np
import pytest

import vecchia_grid_ref as vg
import vecchia_ref as vr
from test_vecchia_grid_host import EDGES, edge_inputs

pytestmark = pytest.mark.gpu

ICANARY = -7777


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


def _run(H, call, nq, m):
    big, view = _framed_idx(H, nq, m)
    call(view)
    H.sync()
    assert _idx_frame_untouched(big, nq, m)
    return view.cpu().numpy()[:, :m].copy()


class Pair:
    """reference rows on the device with their grid: .grid(xq, m, c0) and .brute(xq, m, c0) -> (nq, m) lists on the host"""

    def __init__(self, H, xr, scales=None):
        self.H, self.xr, self.scales = H, xr, scales
        self.xrd = H.to_device(xr)
        self.g = H.nn_grid_build(self.xrd, scales)

    def _xq(self, xq):
        return self.xrd if xq is self.xr else self.H.to_device(xq)

    def grid(self, xq, m, c0=-1, g=None):
        xqd = self._xq(xq)
        return _run(self.H, lambda out: self.H.nn_grid_search(xqd, self.xrd, m, out, g or self.g, c0=c0), len(xq), m)

    def brute(self, xq, m, c0=-1):
        xqd = self._xq(xq)
        return _run(self.H, lambda out: self.H.nn_search(xqd, self.xrd, m, out, scales=self.scales, c0=c0), len(xq), m)

    def same(self, xq, m, c0=-1):
        """the grid's lists, after asserting that they are the brute entry's"""
        got, want = self.grid(xq, m, c0), self.brute(xq, m, c0)
        bad = np.flatnonzero(np.any(got != want, axis=1))
        assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]], want[bad[:2]])
        return got


# ---- 1. the edge shapes, the bit contracts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nr,d,m,scaled,c0", EDGES)
def test_grid_equals_brute_on_the_edge_shapes(H, nq, nr, d, m, scaled, c0):
    xq, xr, scales = edge_inputs(nq, nr, d, m, scaled, c0)
    p = Pair(H, xr, scales)
    idx = p.same(xq, m, c0)
    if (nq, nr) in ((257, 257), (63, 64)):
        vr.check_search_rows(idx, xq, xr, m, scales, c0)
    # a row alone has the bits it has in the larger call; a second call, and a grid built a second time, return the same bits
    for i in sorted({0, len(xq) // 2, len(xq) - 1}):
        assert np.array_equal(p.grid(xq[i:i + 1], m, c0 if c0 < 0 else c0 + i)[0], idx[i]), i
    assert np.array_equal(p.grid(xq, m, c0), idx)
    again = H.nn_grid_build(p.xrd, scales)
    assert np.array_equal(again.info, p.g.info) and np.array_equal(p.grid(xq, m, c0, g=again), idx)


# ---- 2. the early-row cut ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,c0,nq", [(2000, 0, 1000), (2000, 900, 400), (2000, 1024, 300), (2000, 1023, 2), (70000, 3900, 400), (70000, 4095, 2)])
def test_early_row_cut(H, nr, c0, nq):
    """causal queries with fewer than 1024 candidates (4096 from 65536 reference rows on) go to the brute kernel, the others to the grid: below the cut, across it, above it,
    and the two rows next to it; a row alone on either side has the bits of the larger call"""
    cut = vg.early_cut(nr)
    assert cut == (1024 if nr == 2000 else 4096)
    xr = np.random.default_rng(41).random((nr, 3))
    p = Pair(H, xr, np.array([0.5, 1.0, 2.0]))
    xq = xr[c0:c0 + nq]
    idx = p.same(xq, 32, c0)
    for i in sorted({0, max(0, min(nq - 1, cut - 1 - c0)), max(0, min(nq - 1, cut - c0)), nq - 1}):
        assert np.array_equal(p.grid(xq[i:i + 1], 32, c0 + i)[0], idx[i]), i


# ---- 3. one cell, ties, faces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [15, 16, 17])
def test_fewer_rows_than_neighbours(H, n):
    x = np.random.default_rng(n).random((n, 2))
    p = Pair(H, x)
    p.same(x, 16, -1)
    p.same(x, 16, 0)
    one = Pair(H, x[:1] * np.ones((n, 1)))                      # n copies of one point: one cell
    assert one.g.cells == (1, 1)
    one.same(x, 16, -1)


def test_ties_and_faces(H):
    base = np.random.default_rng(9).integers(0, 4, (40, 3)).astype(np.float64)
    x = np.vstack([base, base, base[:13]])
    p = Pair(H, x)
    for m, c0 in ((5, -1), (17, 0), (64, -1)):
        assert np.array_equal(p.same(x, m, c0), vr.search_ref(x, x, m, None, c0)), (m, c0)
    g = np.stack(np.meshgrid(np.arange(13.0), np.arange(11.0), indexing="ij"), axis=-1).reshape(-1, 2)
    sc = np.array([1.0, 2.0])
    p = Pair(H, g, sc)
    for m, c0 in ((8, 0), (33, -1), (64, 0)):
        assert np.array_equal(p.same(g, m, c0), vr.search_ref(g, g, m, sc, c0)), (m, c0)
    q = g[:70] + 0.5
    assert np.array_equal(p.same(q, 16, -1), vr.search_ref(q, g, 16, sc, -1))
    same = np.full((300, 3), 0.25)
    p = Pair(H, same)
    assert np.array_equal(p.same(same, 16, -1)[7], np.arange(16))
    p.same(same, 16, 0)
    rng = np.random.default_rng(12)
    flat = rng.random((700, 3))
    flat[:, 1] = 0.375                                          # one coordinate constant: one cell across it
    p = Pair(H, flat, np.array([1.0, 0.3, 2.0]))
    assert p.g.cells[1] == 1
    p.same(flat, 17, -1)
    p.same(flat + np.array([0.0, 0.01, 0.0]), 17, -1)
    # rows exactly on the box's faces and on a lattice whose lines the cell faces may share; queries on the faces too
    lat = rng.integers(0, 9, (900, 3)).astype(np.float64) * 0.125
    p = Pair(H, lat)
    p.same(lat, 16, -1)
    p.same(lat, 16, 0)
    faces = rng.random((60, 3))
    faces[np.arange(60), rng.integers(0, 3, 60)] = rng.integers(0, 2, 60).astype(np.float64)
    p.same(faces, 33, -1)


# ---- 4. queries outside the box, clusters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_queries_outside_the_box(H, d):
    rng = np.random.default_rng(50 + d)
    xr = rng.random((1500, d))
    xq = np.vstack([rng.random((25, d)) * 21.0 - 10.0, (rng.random((25, d)) - 0.5) * 3.0])
    xq[:2 * d] = 0.5
    for k in range(d):
        xq[2 * k, k], xq[2 * k + 1, k] = -10.0, 11.0            # straight out through every side
    p = Pair(H, xr, 0.2 + rng.random(d))
    vr.check_search_rows(p.same(xq, 16, -1), xq, xr, 16, p.scales, -1)


def test_two_distant_clusters(H):
    """two clusters of width 1e-6 at distance 1e3: nearly every row shares two cells.  Exactness is asserted, not speed."""
    rng = np.random.default_rng(60)
    x = np.vstack([rng.random((1000, 3)) * 1e-6, 1e3 + rng.random((1000, 3)) * 1e-6])[rng.permutation(2000)]
    p = Pair(H, x)
    p.same(x, 32, 0)
    p.same(x, 32, -1)
    p.same(rng.random((20, 3)) * 1e3, 32, -1)


# ---- 5. sizes where shells grow: causal rows past the cut, random and maxmin orders -------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 20000])
def test_causal_search_in_random_and_maxmin_order(H, n):
    rng = np.random.default_rng(n)
    x = rng.random((n, 3))
    p = Pair(H, x)
    p.same(x, 32, 0)
    perm, _ = H.nn_maxmin_order(p.xrd, 0, want_distances=False)
    p = Pair(H, np.ascontiguousarray(x[perm]))
    p.same(p.xr, 32, 0)


def test_more_queries_than_one_brute_launch(H):
    """the existing launch-cut case: the grid entry takes all its queries in one launch, the early rows in the brute entry's"""
    nq, nr, m = 65536 + 70, 70000, 2
    xr = np.random.default_rng(77).random((nr, 1))
    p = Pair(H, xr)
    idx = p.same(xr[:nq], m, 0)
    for s, e in ((4090, 4100), (65500, nq)):
        vr.check_search_rows(idx[s:e], xr[s:e], xr, m, None, s)
    p.same(xr[:nq], m, -1)


def test_build_worst_case(H):
    """10^5 identical points: one cell; the build is linear in the cell's occupancy, and a search answers"""
    x = np.full((100000, 3), 0.5)
    p = Pair(H, x)
    assert p.g.cells == (1, 1, 1)
    q = np.random.default_rng(1).random((64, 3))
    got = p.same(q, 8, -1)
    assert np.array_equal(got, np.tile(np.arange(8), (64, 1)))


# ---- 6. argument rules ------------------------------------------------------------------------------------------------------------------------
def test_argument_rules(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    n, d = 50, 3
    xh = np.random.default_rng(1).random((n, d))
    x = H.to_device(xh)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    bad = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    buf, work = H.empty(_lib.nn_grid_bytes(n, d) // 8), H.empty(_lib.nn_grid_workspace_bytes(n, d) // 8)
    info = np.zeros(_lib.NN_GRID_INFO)

    def build(**kw):
        a = dict(h=H._h, xr=P(x), nr=n, d=d, sc=None, grid=P(buf), gb=buf.numel() * 8, work=P(work), wb=work.numel() * 8,
                 info=info.ctypes.data_as(_lib.P_d))
        a.update(kw)
        return L.fvgp_hip_nn_grid_build(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(xr=None)), (-3, dict(nr=0)), (-3, dict(nr=2 ** 31)), (-4, dict(d=0)), (-4, dict(d=4)),
                     (-5, dict(sc=bad)), (-6, dict(grid=None)), (-6, dict(grid=ctypes.c_void_p(buf.data_ptr() + 4))),
                     (-7, dict(gb=buf.numel() * 8 - 8)), (-8, dict(work=None)), (-9, dict(wb=work.numel() * 8 - 8)), (-10, dict(info=None))):
        assert build(**kw) == code, (code, kw)
    for poison in (np.nan, np.inf):                             # a coordinate that is no number: a code, not a fault
        xb = xh.copy()
        xb[17, 1] = poison
        xbd = H.to_device(xb)
        assert build(xr=P(xbd)) == -11
    huge = H.to_device(np.array([[-1e308, 0.0, 0.0], [1e308, 0.0, 0.0]]))   # finite rows, a box whose extent is not
    assert build(xr=P(huge), nr=2) == -11
    assert build() == 0

    big, out = _framed_idx(H, n, 4)

    def search(**kw):
        a = dict(h=H._h, xq=P(x), nq=n, xr=P(x), nr=n, d=d, m=4, c0=-1, info=info.ctypes.data_as(_lib.P_d), grid=P(buf), out=P(out),
                 ld=out.stride(0))
        a.update(kw)
        return L.fvgp_hip_nn_grid_search(*a.values())
    other = info.copy()
    other[0] = 0.0
    for code, kw in ((-1, dict(h=None)), (-2, dict(xq=None)), (-3, dict(nq=0)), (-4, dict(xr=None)), (-5, dict(nr=0)), (-5, dict(nr=2 ** 31)),
                     (-6, dict(d=0)), (-6, dict(d=4)), (-8, dict(m=0)), (-8, dict(m=65)), (-9, dict(info=None)), (-9, dict(nr=n - 1)),
                     (-9, dict(d=2)), (-9, dict(info=other.ctypes.data_as(_lib.P_d))), (-10, dict(out=None)), (-11, dict(ld=3)),
                     (-12, dict(grid=None))):
        assert search(**kw) == code, (code, kw)
    H.sync()
    assert np.all(big.cpu().numpy() == ICANARY)
    assert search() == 0
    H.sync()
    assert _idx_frame_untouched(big, n, 4)
    with pytest.raises(ValueError):
        H.nn_grid_build(H.to_device(np.zeros((5, 4))))


# ---- 7. the facade ------------------------------------------------------------------------------------------------------------------------------
def _gp(x, y, route, **kw):
    import fvgp_amd
    d = x.shape[1]
    return fvgp_amd.VecchiaGP(x, y, np.array([1.0] + [0.3, 0.2, 0.4, 0.3, 0.25][:d]), noise_variances=np.full(len(x), 0.01),
                              kernel_function="matern32_ard", n_neighbors=16, args={"neighbor_search": route}, **kw)


def _same_state(a, b):
    assert a._grid is not None and b._grid is None
    assert np.array_equal(a.neighbors(), b.neighbors())
    assert a.log_likelihood() == b.log_likelihood()


def test_facade_routes_agree(H):
    rng = np.random.default_rng(8)
    n = 3000
    x = rng.random((n, 2))
    y = np.sin(4.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    grid, brute = _gp(x, y, "grid"), _gp(x, y, "brute")
    _same_state(grid, brute)
    xp = np.vstack([rng.random((70, 2)), rng.random((30, 2)) * 4.0 - 1.5])          # some of them outside the data's box
    assert np.array_equal(grid.posterior_mean(xp)["m(x)"], brute.posterior_mean(xp)["m(x)"])
    xn, yn = rng.random((50, 2)) * 1.2, rng.standard_normal(50)
    for gp in (grid, brute):
        gp.update_gp_data(xn, yn, np.full(50, 0.02), append=True)
    _same_state(grid, brute)
    assert grid.point_number == n + 50 and grid._grid.nr == n + 50
    assert np.array_equal(grid.posterior_mean(xp)["m(x)"], brute.posterior_mean(xp)["m(x)"])
    for gp in (grid, brute):
        gp.refresh_neighbors(np.array([1.0, 0.1, 0.6]))
    _same_state(grid, brute)
    x2, y2 = rng.random((n, 2)), rng.standard_normal(n)
    for gp in (grid, brute):
        gp.update_gp_data(x2, y2, np.full(n, 0.01), append=False)
    _same_state(grid, brute)
    assert grid._grid.nr == n


def test_facade_maxmin_dimension_rule_and_unknown_value(H):
    rng = np.random.default_rng(18)
    x = rng.random((3000, 2))
    y = np.cos(3.0 * x[:, 0]) + x[:, 1]
    grid, brute = _gp(x, y, "grid", ordering="maxmin"), _gp(x, y, "brute", ordering="maxmin")
    _same_state(grid, brute)
    for gp in (grid, brute):
        gp.refresh_neighbors(np.array([1.0, 0.5, 0.1]), reorder=True)
    _same_state(grid, brute)
    x5 = rng.random((400, 5))
    y5 = x5.sum(axis=1)
    with pytest.raises(ValueError, match="'brute'.*'auto'"):
        _gp(x5, y5, "grid")
    auto, brute5 = _gp(x5, y5, "auto"), _gp(x5, y5, "brute")
    assert auto._grid is None and np.array_equal(auto.neighbors(), brute5.neighbors()) and auto.log_likelihood() == brute5.log_likelihood()
    with pytest.raises(ValueError, match="neighbor_search"):
        _gp(x, y, "tree")
    import fvgp_amd
    dense = fvgp_amd.GP(x[:200], y[:200], init_hyperparameters=np.array([1.0, 0.3, 0.2]), noise_variances=np.full(200, 0.01),
                        kernel_function="matern32_ard")
    through = dense.vecchia(n_neighbors=8, args={"neighbor_search": "grid"})
    assert through._grid is not None and np.array_equal(through.neighbors(), dense.vecchia(n_neighbors=8).neighbors())
