"""A numpy twin of the maxmin ordering of the nearest-neighbour path (a helper module of the tests, not a conftest; include/fvgp_hip_nn.h:
fvgp_hip_nn_maxmin_order), the checker both the twin and the device are held to, and the accuracy case the host and the device
tests share.

    maxmin_ref      the ordering step by step in float64: distances to the current pick only (O(n) memory), squares unfused as in
                    vecchia_ref.distances; where every distance is exactly representable it IS the device's result
    first_point     where the facade starts: the point nearest the mean of the scaled coordinates
    check_maxmin    the definition as properties, distances in longdouble, streaming as well
    logdet_of       sum_i log d_i of the longdouble twin's likelihood under an ordering: half its difference between two orderings is
                    their difference in KL(exact || Vecchia) (the kernel fixed), whatever y is
    accuracy_case   the case of the "maxmin beats random" tests and the twin's figures for it, computed once

Nothing here comes from the device."""
import functools

import numpy as np

import vecchia_ref as vr

LD = vr.LD
U = LD(2) ** -53                 # the unit roundoff of a double


def maxmin_ref(x, scales, first, q):
    """(perm (q,) int64, dist2 (q,) float64): perm[0] = first, perm[t] the point not picked yet with the largest squared scaled distance
    to its nearest earlier pick (ties to the lowest index), dist2[t] that distance, dist2[0] = inf"""
    x = np.asarray(x, dtype=np.float64)
    mind = np.full(len(x), np.inf)
    perm, dist2 = np.empty(q, dtype=np.int64), np.empty(q)
    j, dj = int(first), np.inf
    for t in range(q):
        perm[t], dist2[t] = j, dj
        mind = np.minimum(mind, vr.distances(x, x[j:j + 1], scales)[:, 0])
        mind[perm[:t + 1]] = -1.0                      # picked (a duplicate of a pick has 0, and is still to come)
        j = int(np.argmax(mind))                       # the first of the largest: the lowest index
        dj = mind[j]
    return perm, dist2


def first_point(x, scales):
    """the facade's rule: the point nearest, in the scaled coordinates, to their mean; ties to the lowest index"""
    x = np.asarray(x, dtype=np.float64)
    z = x if scales is None else x * vr.inv_scales(scales, x.shape[1])
    return int(np.argmin(np.sum((z - np.mean(z, axis=0)) ** 2, axis=1)))


def check_maxmin(perm, dist2, x, scales, first):
    """The definition of the maxmin ordering as properties of (perm, dist2), the first q = len(perm) positions; distances in longdouble
    with the exact 1 / scale, one pick at a time.

        perm[0] == first, dist2[0] == inf; every entry in 0 .. n - 1, none repeated;
        at every t >= 1:  mindist_t(perm[t]) * slack >= the largest mindist_t over the points not picked yet,
                          and where the two are EQUAL in longdouble, perm[t] is the lowest index that attains it;
        dist2[t] agrees with mindist_t(perm[t]) to a relative (d + 6) 2^-53;
        dist2[1:] never increases (exact for maxmin in any arithmetic that computes each mindist once).

    slack = 1 + (2 d + 12) 2^-53.  The device orders by distances in double.  A term ((x_ik - x_jk) * is_k)^2 carries three roundings
    before it is squared -- the difference, is_k = 1 / scale_k, the product -- so 6 units of 2^-53 relative after squaring (the fused
    multiply-add does not round the square itself); the d fused accumulates add one rounding each to a sum of non-negative terms, d units
    more.  One distance is therefore within (d + 6) 2^-53 of the exact one, which is the bar on dist2; a mindist is a minimum of such
    distances and inherits the bound; and the pick compares two of them, so the exact mindist of the device's pick can fall short of
    the exact maximum by twice that: (2 d + 12) 2^-53.  Nothing here is measured."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    perm, dist2 = np.asarray(perm), np.asarray(dist2)
    q = len(perm)
    assert len(dist2) == q and 1 <= q <= n
    assert perm[0] == first, ("first", int(perm[0]), first)
    assert np.all((perm >= 0) & (perm < n)), "an index outside 0 .. n - 1"
    assert len(np.unique(perm)) == q, "a repeated index"
    assert dist2[0] == np.inf
    assert np.all(dist2[2:] <= dist2[1:-1]), "the entry distances increase somewhere"
    xl = x.astype(LD)
    slack, tol = 1 + (2 * d + 12) * U, (d + 6) * U
    mind = np.full(n, np.inf, dtype=LD)
    free = np.ones(n, dtype=bool)
    for t in range(1, q):
        mind = np.minimum(mind, vr.distances(xl, xl[perm[t - 1]:perm[t - 1] + 1], scales, LD)[:, 0])
        free[perm[t - 1]] = False
        mine, best = mind[perm[t]], np.max(mind[free])
        assert mine * slack >= best, ("not the farthest point", t, int(perm[t]), float(mine), float(best))
        if mine == best:
            assert perm[t] == np.flatnonzero(free & (mind == best))[0], ("a tie not broken to the lowest index", t)
        assert abs(LD(dist2[t]) - mine) <= tol * mine, ("dist2", t, float(dist2[t]), float(mine))


# ---- the accuracy case -------------------------------------------------------------------------------------------------------------------
ACC = ("matern52_ard", 2, 400, 8)      # (kernel, d, n, m): vecchia_ref.case_data(kernel, d, n), the scales its length scales
ACC_SEEDS = (0, 1, 2, 3, 4)            # the random orderings: default_rng(s).permutation(n), what VecchiaGP(ordering="random", seed=s) draws


def logdet_of(name, x, theta, r, v, perm, m, scales):
    """sum_i log d_i (longdouble) of the twin's likelihood with the data in the ordering perm, m neighbours under `scales`"""
    xo = x[perm]
    idx = vr.search_ref(xo, xo, m, scales, c0=0)
    return vr.loglik_ref(name, xo, theta, idx, r[perm], v[perm], LD)[2]


@functools.lru_cache(maxsize=None)
def accuracy_case():
    """(x, theta, r, v, scales, maxmin perm, logdet under maxmin, {seed: logdet under that random ordering}) of ACC, all by the twin"""
    name, d, n, m = ACC
    x, theta, r, v = vr.case_data(name, d, n)
    scales = vr.length_scales(name, theta, d)
    perm, _ = maxmin_ref(x, scales, first_point(x, scales), n)
    mm = logdet_of(name, x, theta, r, v, perm, m, scales)
    rnd = {s: logdet_of(name, x, theta, r, v, np.random.default_rng(s).permutation(n), m, scales) for s in ACC_SEEDS}
    return x, theta, r, v, scales, perm, mm, rnd
