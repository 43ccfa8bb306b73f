"""CPU-only checks of the cell-grid neighbour search (include/fvgp_hip_nn.h: fvgp_hip_nn_grid_build, fvgp_hip_nn_grid_search):
the numpy twin of the algorithm (vecchia_grid_ref: the device's cell assignment, the shell walk, the stop rule with its margin, the
early-row cut) returns vecchia_ref.search_ref's lists element for element -- on the device tests' shapes, on a sweep of small
configurations from a coarse lattice (ties, rows on cell faces) and on copies nudged by one ulp -- and a stop rule without its
ingredients does not; the sizing entries and the host-side argument rules of the library; the facade's argument."""
import ctypes

import numpy as np
import pytest

import vecchia_grid_ref as vg
import vecchia_ref as vr

# (nq, nr, d, m, scaled, c0): the device tests' edge shapes
EDGES = [(1, 1, 1, 1, False, -1), (2, 2, 3, 16, True, 0), (63, 64, 2, 17, False, -1), (65, 63, 3, 64, False, -1), (257, 257, 3, 17, True, 0),
         (1000, 1000, 3, 16, True, 0), (300, 1000, 2, 64, False, 700), (257, 1000, 1, 64, True, -1), (1000, 2, 3, 1, False, -1)]


def edge_inputs(nq, nr, d, m, scaled, c0):
    """the inputs of an edge shape, as tests/test_gpu_vecchia.py::test_search_properties draws them"""
    rng = np.random.default_rng(100 * nq + nr + d + m)
    xr = rng.random((nr, d))
    if c0 == 0:
        nq = min(nq, nr)
        xq = xr[:nq] if nq < nr else xr
    elif c0 > 0:
        xq = xr[c0:]
    else:
        xq = rng.random((nq, d))
    return xq, xr, (0.2 + rng.random(d) if scaled else None)


@pytest.mark.parametrize("nq,nr,d,m,scaled,c0", EDGES)
def test_twin_equals_the_brute_twin_on_the_edge_shapes(nq, nr, d, m, scaled, c0):
    xq, xr, scales = edge_inputs(nq, nr, d, m, scaled, c0)
    want = vr.search_ref(xq, xr, m, scales, c0)
    # early = 7: the causal shapes walk the grid for all rows but the first (the device's cut, 1024 at these sizes, would send them all to the brute search)
    for early in (None, 7):
        stats = {}
        got = vg.grid_search_ref(xq, xr, m, scales, c0, early=early, shuffle=np.random.default_rng(1), stats=stats)
        assert np.array_equal(got, want), early
    assert stats["walked"] >= len(xq) - 7


def lattice_case(seed):
    """a small configuration from a coarse lattice: (xq, xr, m, scales, c0, h) -- h a multiple of the lattice step in scaled units, so
    that rows and queries lie exactly on cell faces, or None for the build's own choice"""
    rng = np.random.default_rng(seed)
    d = int(rng.integers(1, 4))
    n = int(rng.integers(1, 201)) if seed % 4 else int(rng.integers(1, 40))
    m = int(rng.choice([1, 5, 16]))
    levels = int(rng.choice([2, 3, 5, 9, 17]))
    step = float(rng.choice([1.0, 0.25, 0.1, 3.0]))
    xr = rng.integers(0, levels, (n, d)).astype(np.float64) * step
    if rng.random() < 0.2:
        xr[:, int(rng.integers(0, d))] = step                   # one coordinate constant
    scales = None if rng.random() < 0.5 else np.array([1.0, 2.0, 0.5])[:d] * float(rng.choice([1.0, 0.7]))
    mode = int(rng.integers(0, 3))
    if mode == 0:
        xq, c0 = xr, 0
    elif mode == 1:
        k = int(rng.integers(0, n))
        xq, c0 = xr[k:], k
    else:                                                       # prediction: on the lattice, between its points, outside the box
        nq = int(rng.integers(1, 40))
        xq = (rng.integers(-2 * levels, 3 * levels, (nq, d)).astype(np.float64) * 0.5) * step
        c0 = -1
    h = None
    if rng.random() < 0.6:
        h = float(rng.choice([1.0, 2.0, 3.0])) * step * (1.0 if scales is None else float(1.0 / scales[0]))
    return xq, xr, m, scales, c0, h


def nudged(x, rng):
    """every coordinate moved by one ulp up or down, or left where it is"""
    up, down = np.nextafter(x, np.inf), np.nextafter(x, -np.inf)
    pick = rng.integers(0, 3, x.shape)
    return np.where(pick == 0, x, np.where(pick == 1, up, down))


SWEEP = 300


def test_twin_equals_the_brute_twin_on_a_sweep_of_lattice_configurations():
    """ties, duplicated rows, rows and queries exactly on cell faces and on the box's faces, queries outside the box, and a copy of each
    configuration nudged by +-1 ulp so that nothing is exactly on a face any more but everything is next to one"""
    stopped_early = 0
    for seed in range(SWEEP):
        xq, xr, m, scales, c0, h = lattice_case(seed)
        rng = np.random.default_rng(10_000 + seed)
        for copy in range(2):
            if copy:
                same = xq is xr
                xr = nudged(xr, rng)
                xq = xr if same else (xr[c0:] if c0 > 0 else nudged(xq, rng))
            stats = {}
            got = vg.grid_search_ref(xq, xr, m, scales, c0, early=int(rng.choice([0, 3, 50])), occupancy=int(rng.choice([1, 2, 4])),
                                     shuffle=rng, stats=stats, h=h)
            assert np.array_equal(got, vr.search_ref(xq, xr, m, scales, c0)), (seed, copy)
            stopped_early += stats["visited"] < stats["walked"] * len(xr)
    assert stopped_early > SWEEP // 2              # (the stop rule is at work in the sweep, not every walk covers the grid)


@pytest.mark.parametrize("wrong", ["no gap", "not strict"])
def test_the_sweep_catches_a_wrong_stop_rule(monkeypatch, wrong):
    """the sweep has teeth: a bound that forgets where the query lies in its cell, and a stop at equality, both return wrong lists"""
    if wrong == "no gap":
        monkeypatch.setattr(vg, "stop_bound", lambda cq, t, nc, h, R: ((R + 1) * h) ** 2)
    else:                                           # worst <= bound: an unvisited row at exactly the worst distance with a lower index
        real = vg.stop_bound
        monkeypatch.setattr(vg, "stop_bound", lambda cq, t, nc, h, R: np.nextafter(real(cq, t, nc, h, R) / vg.SHRINK, np.inf))
        monkeypatch.setattr(vg, "SLACK", 0.0)
    bad = 0
    for seed in range(SWEEP):
        xq, xr, m, scales, c0, h = lattice_case(seed)
        bad += not np.array_equal(vg.grid_search_ref(xq, xr, m, scales, c0, early=0, h=h), vr.search_ref(xq, xr, m, scales, c0))
    print(f"\nwrong stop rule ({wrong}): {bad} of {SWEEP} configurations differ")
    assert bad > 0


def test_twin_on_the_special_sets():
    """the device tests' tie sets, one cell, identical points, queries far outside, two distant clusters"""
    base = np.random.default_rng(9).integers(0, 4, (40, 3)).astype(np.float64)
    x = np.vstack([base, base, base[:13]])
    for m, c0 in ((5, -1), (17, 0), (64, -1)):
        assert np.array_equal(vg.grid_search_ref(x, x, m, None, c0, early=0), vr.search_ref(x, x, m, None, c0))
    g = np.stack(np.meshgrid(np.arange(13.0), np.arange(11.0), indexing="ij"), axis=-1).reshape(-1, 2)
    sc = np.array([1.0, 2.0])
    for m, c0 in ((8, 0), (33, -1), (64, 0)):
        assert np.array_equal(vg.grid_search_ref(g, g, m, sc, c0, early=0), vr.search_ref(g, g, m, sc, c0))
    q = g[:70] + 0.5
    assert np.array_equal(vg.grid_search_ref(q, g, 16, sc, -1), vr.search_ref(q, g, 16, sc, -1))
    same = np.full((300, 3), 0.25)
    assert np.array_equal(vg.grid_search_ref(same, same, 16, None, 0, early=0), vr.search_ref(same, same, 16, None, 0))
    rng = np.random.default_rng(3)
    for n in (15, 16, 17):                                      # n = m - 1, m, m + 1
        x = rng.random((n, 2))
        assert np.array_equal(vg.grid_search_ref(x, x, 16, None, -1), vr.search_ref(x, x, 16, None, -1))
    for d in (2, 3):
        xr = rng.random((400, d))
        xq = np.vstack([rng.random((25, d)) * 21.0 - 10.0, (rng.random((25, d)) - 0.5) * 3.0])
        xq[:2 * d] = 0.5
        for k in range(d):
            xq[2 * k, k], xq[2 * k + 1, k] = -10.0, 11.0                 # straight out through every side
        assert np.array_equal(vg.grid_search_ref(xq, xr, 16, None, -1), vr.search_ref(xq, xr, 16, None, -1))
    cl = np.vstack([rng.random((300, 3)) * 1e-6, 1e3 + rng.random((300, 3)) * 1e-6])[rng.permutation(600)]
    assert np.array_equal(vg.grid_search_ref(cl, cl, 32, None, 0, early=0), vr.search_ref(cl, cl, 32, None, 0))
    between = rng.random((20, 3)) * 1e3
    assert np.array_equal(vg.grid_search_ref(between, cl, 32, None, -1), vr.search_ref(between, cl, 32, None, -1))


def test_the_walk_looks_at_a_small_part_of_evenly_spread_rows():
    """n = 3000 uniform rows, d = 2, m = 5: a ball that holds m rows covers m / n of the box; the shells around it hold, at two rows per
    cell, a few dozen rows -- the twin must look at under a tenth of the rows per query, or the stop rule stops nothing"""
    rng = np.random.default_rng(5)
    xr, xq = rng.random((3000, 2)), rng.random((40, 2))
    stats = {}
    got = vg.grid_search_ref(xq, xr, 5, None, -1, stats=stats)
    assert np.array_equal(got, vr.search_ref(xq, xr, 5, None, -1))
    print(f"\ngrid twin n=3000 d=2 m=5: {stats['visited'] / 40:.1f} rows looked at per query")
    assert stats["visited"] < 0.1 * 3000 * 40


def test_cell_choice():
    h, nc = vg.choose_cells([1.0, 1.0, 1.0], 16000)
    assert nc == [20, 20, 20] and abs(h - 0.05) < 1e-12         # two rows per cell
    assert vg.choose_cells([0.0, 0.0], 100000) == (1.0, [1, 1])
    h, nc = vg.choose_cells([1.0, 0.0, 1.0], 20000)
    assert nc[1] == 1 and nc[0] == nc[2] and nc[0] in (100, 101)       # (h comes from exp and log: the ceiling may see 100 + an ulp)
    h, nc = vg.choose_cells([1.0, 1e-9], 200)                   # thinner than a cell: one cell across, the other dimension takes them all
    assert nc[1] == 1 and nc[0] in (100, 101)
    for ext, n in (([1.0, 1.0, 1.0], 5), ([1e-300, 1e300], 1000), ([3.0, 1.0, 2.0], 10 ** 9), ([1e308, 1e308, 1e308], 1000)):
        h, nc = vg.choose_cells(ext, n)
        assert int(np.prod(nc, dtype=object)) <= min(n, vg.MAX_CELLS) and all(c >= 1 for c in nc) and h > 0
        assert all(e * (1.0 / h) <= c for e, c in zip(ext, nc)) or nc == [1] * len(ext)
    with pytest.raises(ValueError):
        vg.build_ref(np.array([[0.0, np.nan]]))
    with pytest.raises(ValueError):
        vg.build_ref(np.zeros((3, 4)))


def test_library_sizing_and_host_side_argument_rules():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    gb, wb = L.fvgp_hip_nn_grid_bytes, L.fvgp_hip_nn_grid_workspace_bytes
    for f in (gb, wb):
        assert f(0, 3) == -1 and f(10, 0) == -1 and f(10, 4) == -1 and f(2 ** 31, 3) == -1
        assert f(1, 1) > 0 and f(1000, 3) % 8 == 0
    n = 10 ** 6
    assert gb(n, 3) >= 8 * 3 * n + 4 * n + 4 * (n + 1) and gb(n, 3) == _lib.nn_grid_bytes(n, 3)
    assert gb(10 ** 8, 1) - gb(10 ** 8 - 2, 1) == 2 * 12                 # past 2^24 rows the cell table stops growing
    assert wb(n, 3) >= 8 * n and wb(n, 2) == _lib.nn_grid_workspace_bytes(n, 2)
    info = (ctypes.c_double * _lib.NN_GRID_INFO)()
    assert L.fvgp_hip_nn_grid_build(None, None, 1, 1, None, None, 0, None, 0, info) == -1
    assert L.fvgp_hip_nn_grid_search(None, None, 1, None, 1, 1, 1, 0, info, None, None, 1) == -1
    assert _lib.NN_GRID_MAX_DIM == 3 and (vg.early_cut(65535), vg.early_cut(65536)) == (1024, 4096)


def test_facade_argument_is_checked_before_any_device_work():
    from fvgp_amd import gp_vecchia
    assert gp_vecchia.NEIGHBOR_SEARCH_DEFAULT in ("brute", "auto") and gp_vecchia.NEIGHBOR_SEARCH_AUTO_POINTS >= 1

    class Stub(gp_vecchia.VecchiaGP):
        def __init__(self, d, n, args):
            self.args, self.index_set_dim, self.point_number = args, d, n
    assert Stub(3, 10, {})._search_route() == "brute"              # (the default: "brute", or "auto" below its threshold)
    assert Stub(3, 10, {"neighbor_search": "grid"})._search_route() == "grid"
    assert Stub(3, gp_vecchia.NEIGHBOR_SEARCH_AUTO_POINTS, {"neighbor_search": "auto"})._search_route() == "grid"
    assert Stub(3, gp_vecchia.NEIGHBOR_SEARCH_AUTO_POINTS - 1, {"neighbor_search": "auto"})._search_route() == "brute"
    assert Stub(5, 10 ** 7, {"neighbor_search": "auto"})._search_route() == "brute"
    with pytest.raises(ValueError, match="'brute'.*'auto'"):
        Stub(5, 10, {"neighbor_search": "grid"})._search_route()
    with pytest.raises(ValueError, match="neighbor_search"):
        Stub(2, 10, {"neighbor_search": "tree"})._search_route()
