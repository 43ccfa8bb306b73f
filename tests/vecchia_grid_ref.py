"""The numpy twin of the cell-grid neighbour search (include/fvgp_hip_nn.h: fvgp_hip_nn_grid_build, fvgp_hip_nn_grid_search):
the same algorithm in float64 -- the cell assignment in the device's operations, the walk over growing shells of cells, the stop rule
with its margin, the early-row cut -- so that a wrong stop rule shows up without a device.  Its lists are held to
vecchia_ref.search_ref by array_equal (tests/test_vecchia_grid_host.py); the device's to the brute entry's (tests/test_gpu_vecchia_grid.py).
Distances are vecchia_ref.distances': the bound's derivation needs only that every operation rounds monotonically."""
import itertools
import math

import numpy as np

import vecchia_ref as vr

OCCUPANCY = 2             # NG_OCCUPANCY: target mean rows per cell
MAX_CELLS = 1 << 24       # NG_MAX_CELLS


def early_cut(nr):
    """ng_early: causal queries with fewer candidates than this go to the brute search"""
    return 1024 if nr < 65536 else 4096

SLACK = 2.0 ** -40        # NG_SLACK
SHRINK = 1.0 - 2.0 ** -20  # NG_SHRINK
BOUND_FLOOR = 1e-270      # NG_BOUND_FLOOR


def choose_cells(ext, nr, occupancy=OCCUPANCY):
    """(h, cells per dimension) for the scaled extents ext >= 0 of nr rows: ng_choose of csrc/nn_grid.hip"""
    d = len(ext)
    cap = min(nr, MAX_CELLS)
    target = float(max(1, min(cap, -(-nr // occupancy))))
    on = [e > 0.0 for e in ext]
    h = 0.0
    for _ in range(3):
        if not any(on):
            break
        logvol = sum(math.log(e) for e, o in zip(ext, on) if o)
        h = math.exp((logvol - math.log(target)) / sum(on))
        thin = [o and e < h for e, o in zip(ext, on)]
        if not any(thin):
            break
        on = [o and not t for o, t in zip(on, thin)]
    ok = lambda v: v > 0.0 and math.isfinite(v)      # noqa: E731
    if not any(on) or not ok(h) or not ok(1.0 / h):
        return 1.0, [1] * d
    for _ in range(400):
        invh = 1.0 / h
        if not ok(h) or not ok(invh):
            break
        nc, prod, fits = [1] * d, 1, True
        for k in range(d):
            t = ext[k] * invh
            if not t < MAX_CELLS:
                fits = False
                break
            nc[k] = max(1, int(math.ceil(t)))
            prod *= nc[k]
            if prod > cap:
                fits = False
                break
        if fits:
            return h, nc
        h *= 1.25
    return 1.0, [1] * d


class Grid:
    """build_ref's result: lo, inv (1 / scales), h, invh, nc (cells per dimension), buckets {cell tuple: row indices}"""


def cell_coordinate(g, x):
    """((x - lo) * (1 / scales)) * (1 / h), the device's operations in the device's order: (..., d)"""
    return ((np.asarray(x, dtype=np.float64) - g.lo) * g.inv) * g.invh


def cells_of(g, x):
    t = cell_coordinate(g, x)
    return np.fmin(np.fmax(t, 0.0), np.asarray(g.nc, dtype=np.float64) - 1.0).astype(np.int64), t


def build_ref(xr, scales=None, occupancy=OCCUPANCY, shuffle=None, h=None):
    """the grid over the rows of xr (h: the cells' scaled edge where the caller sets it -- the walk must be right for every edge, and a
    test can put cell faces on its lattice this way); shuffle (a numpy Generator): the rows of every bucket in a random order, as the device's atomics
    may leave them.  Raises ValueError where the device returns -11 (a box that is not finite)."""
    xr = np.asarray(xr, dtype=np.float64)
    nr, d = xr.shape
    if not 1 <= d <= 3:
        raise ValueError("the cell grid takes 1 .. 3 dimensions")
    g = Grid()
    g.inv = vr.inv_scales(scales, d)
    g.lo, hi = xr.min(axis=0), xr.max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = (hi - g.lo) * g.inv
    if not (np.all(np.isfinite(xr)) and np.all(np.isfinite(ext))):
        raise ValueError("the reference rows' bounding box is not finite")
    if h is None:
        g.h, g.nc = choose_cells([float(e) for e in ext], nr, occupancy)
    else:
        g.h, g.nc = float(h), [max(1, int(math.ceil(float(e) * (1.0 / h)))) for e in ext]
    g.invh = 1.0 / g.h
    cells, _ = cells_of(g, xr)
    g.buckets = {}
    for j, c in enumerate(map(tuple, cells)):
        g.buckets.setdefault(c, []).append(j)
    for c in g.buckets:
        rows = np.array(g.buckets[c], dtype=np.int64)
        g.buckets[c] = rows if shuffle is None else shuffle.permutation(rows)
    return g


def _shell(cq, nc, R):
    """the cells at Chebyshev distance exactly R from cq, clipped to the grid"""
    ranges = [range(max(c - R, 0), min(c + R, n - 1) + 1) for c, n in zip(cq, nc)]
    return [c for c in itertools.product(*ranges) if max(abs(a - b) for a, b in zip(c, cq)) == R]


def stop_bound(cq, t, nc, h, R):
    """the lower bound on the computed squared distance from a query with cell coordinate t in cell cq to every row in a cell outside
    shells 0 .. R, margin included; inf where no such cell exists"""
    bound = math.inf
    for k in range(len(nc)):
        slack = SLACK * (abs(t[k]) + (nc[k] + 2))
        if cq[k] + R + 1 <= nc[k] - 1:
            g = max(((cq[k] + 1) - t[k]) + R - slack, 0.0) * h
            bound = min(bound, g * g)
        if cq[k] - R - 1 >= 0:
            g = max((t[k] - cq[k]) + R - slack, 0.0) * h
            bound = min(bound, g * g)
    return bound * SHRINK


def grid_search_ref(xq, xr, m, scales=None, c0=-1, early=None, occupancy=OCCUPANCY, shuffle=None, stats=None, h=None):
    """int32 (nq, m): fvgp_hip_nn_grid_search's algorithm.  stats (a dict): receives "visited" (rows looked at by the grid walks) and
    "walked" (queries that took the grid)"""
    xq, xr = np.asarray(xq, dtype=np.float64), np.asarray(xr, dtype=np.float64)
    g = build_ref(xr, scales, occupancy, shuffle, h)
    nr = len(xr)
    early = early_cut(nr) if early is None else early
    out = np.full((len(xq), m), -1, dtype=np.int32)
    cqs, ts = cells_of(g, xq)
    visited = walked = 0
    for i in range(len(xq)):
        if c0 >= 0 and c0 + i < early:
            out[i] = vr.search_ref(xq[i:i + 1], xr, m, scales, c0 + i)[0]
            continue
        walked += 1
        lim = vr.candidates(i, nr, c0)
        dist = vr.distances(xq[i:i + 1], xr, scales)[0]
        cq, t = tuple(int(c) for c in cqs[i]), [float(v) for v in ts[i]]
        best = []                                  # (distance, index), sorted
        last = max(max(c, n - 1 - c) for c, n in zip(cq, g.nc))
        for R in range(max(g.nc)):
            if R > last:
                break
            for c in _shell(cq, g.nc, R):
                for j in g.buckets.get(c, ()):
                    if j >= lim:
                        continue
                    visited += 1
                    key = (float(dist[j]), int(j))
                    if len(best) < m or key < best[-1]:
                        best.append(key)
                        best.sort()
                        del best[m:]
            if len(best) < m:
                continue
            bound = stop_bound(cq, t, g.nc, g.h, R)
            if bound >= BOUND_FLOOR and best[-1][0] < bound:
                break
        out[i, :len(best)] = [j for _, j in best]
    if stats is not None:
        stats["visited"], stats["walked"] = visited, walked
    return out
