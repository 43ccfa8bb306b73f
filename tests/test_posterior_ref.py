"""The reference of the posterior tests proved on the host, before any kernel runs (tests/posterior_ref.py; the device side is
tests/test_gpu_posterior.py): every fixture has the condition number the caps assume; the longdouble posterior agrees with a second
formulation through potrs_ld; points far from the data give exactly mean 0 and variance sigma^2; both float64 twins stay inside the
derived caps on every family; the floor of the bars is what scipy's substitution attains on the benign family; the two twins are within
8 x of each other there; and the sampled points hold every class and every edge."""
import numpy as np
import pytest

import kernel_family_ref as kf
import posterior_ref as pr

EPS, LD = pr.EPS, pr.LD
FIXTURES = [(f, n) for f in "BG" for n in pr.GPU_N] + [("H", n) for n in pr.H_N] + [("M", 300)]
# the calls whose twins are measured: every class alone (the one-point route), few points, one tile and more, 1024-wide blocks
HOST_P = (1, 5, 300, 1100)
# the summation of the twins' mean is numpy's pairwise one over n terms: depth log2(n) + 8 at the most
TWIN_DEPTH = 20


_REFS = {}


def _reference(fam, n, P, first=0):
    key = (fam, n, P, first)
    if key not in _REFS:
        fx = pr.fixture(fam, n)
        xp, cls = pr.points(fx, P, first=first)
        idx = pr.sample_points(P, seed=n)
        _REFS[key] = pr.Reference(fx, xp[idx], [cls[i] for i in idx])
    return _REFS[key]


@pytest.mark.parametrize("fam,n", FIXTURES)
def test_fixtures_meet_the_conditions_the_caps_rest_on(fam, n):
    """cond_2(L) within 30 % of the value written down in posterior_ref.COND; L is the rounded longdouble factor of K + noise I, lower
    triangular with a positive diagonal; alpha solves (L L^T) alpha = y to the precision a rounded solution can"""
    fx = pr.fixture(fam, n)
    want = pr.COND[(fam, n)]
    print(f"POSTREF|{fam}|{n}|cond_2(L) {fx.cond:.4g}")
    assert 0.7 * want <= fx.cond <= 1.3 * want, fx.cond
    assert fx.L.dtype == np.float64 and fx.L.shape == (n, n) and not fx.L.flags.writeable
    assert np.array_equal(fx.L, np.tril(fx.L)) and np.all(np.diagonal(fx.L) > 0)
    assert fx.theta[0] == pr.SIG and len(fx.theta) == kf.n_theta(fx.kernel, fx.d)
    Ll = np.asarray(fx.L, dtype=LD)
    rows = pr.chol_ref.edge_rows(n)                                                    # complete rows of L L^T, as chol_ref.beta takes them
    resid = np.abs(Ll[rows] @ Ll.T - np.asarray(fx.KV[rows], dtype=LD))
    assert float(np.max(resid / (np.abs(Ll[rows]) @ np.abs(Ll).T))) <= 2 * EPS        # the rounding of the entries of L alone
    a = fx.alpha(pr.VEC_COLS)
    assert a.shape == (n, pr.VEC_COLS) and np.all(np.isfinite(a))
    back = Ll @ (Ll.T @ np.asarray(a, dtype=LD)) - np.asarray(fx.y[:, :pr.VEC_COLS], dtype=LD)
    scale = np.abs(Ll) @ (np.abs(Ll.T) @ np.abs(np.asarray(a, dtype=LD)))
    assert float(np.max(np.abs(back) / scale)) <= 2 * EPS
    if n <= 300:            # the two widths of the solve give a column the same bits
        assert np.array_equal(fx.alpha(pr.MAX_COLS)[:, :pr.VEC_COLS], a)


@pytest.mark.parametrize("fam,n", [("B", 1), ("B", 129), ("G", 300), ("H", 300), ("M", 300), ("G", 700)])
def test_longdouble_posterior_agrees_with_a_second_formulation(fam, n):
    """S = k** - w^T w against k** - k^T (K + V)^-1 k through potrs_ld: the two differ by the longdouble rounding of two different
    solves, at most 64 cond_2(L)^2 eps_ld relative to |w_p| |w_q| + sigma^2 -- the bound of the potrs formulation, whose error grows
    with cond_2(K + V) = cond_2(L)^2; measured: 4e-17 on H at n = 300 (a fifth of a float64 ulp), 1e-18 on G, and the substitution the
    reference uses errs like twin (a) with a unit roundoff 2048 times smaller: at most 0.2 in the units of nu (363 / 2048 on H), where
    no bar is below 64"""
    fx = pr.fixture(fam, n)
    R = _reference(fam, n, 300)
    S2 = pr.posterior_ld_potrs(fx, R.xs)
    d = np.abs(S2 - R.S) / (R.den_sig / LD(EPS))
    tol = 64 * pr.ts.EPS_LD * max(fx.cond, 1.0) ** 2
    print(f"POSTREF|{fam}|{n}|two formulations differ by {float(np.max(d)):.3g} (allowed {tol:.3g}, a float64 ulp is {EPS:.3g})")
    assert float(np.max(d)) <= tol
    assert np.array_equal(R.v, np.diagonal(R.S))
    # the mean is the plain sum
    m2 = np.einsum("ip,ic->pc", R.k, np.asarray(fx.alpha(R.ncol), dtype=LD))
    assert float(np.max(np.abs(m2 - R.m) / (R.den_mu / LD(EPS)))) <= 4 * pr.ts.EPS_LD * n


@pytest.mark.parametrize("fam,n", [("B", 1), ("B", 300), ("G", 129), ("H", 700), ("M", 300)])
def test_far_points_give_exactly_zero_and_sigma2(fam, n):
    """the unit cube shifted by +50: every cross covariance underflows (rbf: to 0 in longdouble too; matern52 at l = 0.1: to 0 in
    float64, to below 1e-800 in longdouble), so the mean is 0, the variance sigma^2 and S the prior covariance among the points"""
    fx = pr.fixture(fam, n)
    R = _reference(fam, n, 300)
    far = np.array([c == "far" for c in R.cls])
    assert far.sum() >= 3
    sig = LD(fx.theta[0])
    assert np.all(np.asarray(R.m[far], dtype=np.float64) == 0.0)
    assert np.all(R.v[far] == sig)
    kss = kf.k_ref(fx.kernel, R.xs[far], R.xs[far], fx.theta)
    assert np.array_equal(R.S[np.ix_(far, far)], kss)
    assert np.all(np.asarray(R.S[np.ix_(far, ~far)], dtype=np.float64) == 0.0)
    if fx.kernel.startswith("rbf"):
        assert np.all(R.k[:, far] == 0) and np.all(R.m[far] == 0)
    for nb in (None, 128, 2048):
        m, v, S = pr.posterior_twin(fx, R.xs, nb)
        assert np.all(m[far] == 0.0) and np.all(v[far] == fx.theta[0])


@pytest.mark.parametrize("fam,n", FIXTURES)
def test_twins_stay_inside_the_caps(fam, n):
    """scipy's substitution and the block-inverse twin at every width a route takes: nu, sig <= 64 cond_2(L), mu <= k_bound_ulps(d)
    + the depth of numpy's sum; on B twin (a) alone is under the floor of the bars in every class and measure"""
    fx = pr.fixture(fam, n)
    worst = {}
    for P in HOST_P if n < 1300 else (300, 1100):
        for first in range(len(pr.CLASSES) if P == 1 else 1):
            R = _reference(fam, n, P, first)
            for nb in (None, 128, 2048 if P <= 1024 else 1024):          # the widths the routes take at P points
                fig = R.twin(nb)
                for q in pr.MEASURES:
                    cap = pr.mu_cap(fx, TWIN_DEPTH) if q == "mu" else max(fx.cap_solve(), pr.FLOOR[q])
                    for c, val in fig[q].items():
                        worst[(nb, q)] = max(worst.get((nb, q), 0.0), val)
                        assert val <= cap, (P, nb, q, c, val, cap)
                        if c == "far" and q != "sig":
                            assert val == 0.0, (P, nb, q, val)
                        if fam == "B" and nb is None:
                            assert val <= pr.FLOOR[q], (P, q, c, val)
    print(f"POSTREF|{fam}|{n}|" + "|".join(f"{'scipy' if nb is None else nb} {q} {v:.3g}" for (nb, q), v in sorted(worst.items(), key=str)))


def test_the_floor_is_the_smallest_that_twin_a_passes_on_the_benign_family():
    """FLOOR is a whole number, at least 4 (the floor of the two earlier suites), and where it is above 4 the next smaller whole number
    would fail twin (a) somewhere on B: over every size the device tests use and the calls HOST_P (n = 1300: 300 and 1100 points)"""
    worst = {q: 0.0 for q in pr.MEASURES}
    for n in pr.GPU_N:
        for P in HOST_P if n < 1300 else (300, 1100):
            for first in range(len(pr.CLASSES) if P == 1 else 1):
                fig = _reference("B", n, P, first).twin(None)
                for q in pr.MEASURES:
                    worst[q] = max(worst[q], max(fig[q].values()))
    print("POSTREF|floor|" + "|".join(f"{q} twin (a) worst on B {v:.3g} floor {pr.FLOOR[q]}" for q, v in worst.items()))
    for q in pr.MEASURES:
        f = pr.FLOOR[q]
        assert f >= 4 and f == int(f)
        assert worst[q] <= f
        assert f == 4 or worst[q] > f - 1


@pytest.mark.parametrize("n", [129, 300, 700])
def test_the_two_twins_are_within_8x_of_each_other_on_the_benign_family(n):
    """twin (a) and twin (b) at the widths the routes take, per class and measure, after both are raised to the floor: below the floor
    a ratio means nothing (0.003 against 0.6 of an ulp in one class).  Twin (a) is under the floor on B, so what this asserts is that
    the block-inverse algorithm costs at most 8 floors there -- on the benign family the two terms of the bars cannot be told apart"""
    for P in HOST_P:
        R = _reference("B", n, P)
        a = R.twin(None)
        for nb in (128, 2048 if P <= 1024 else 1024):
            b = R.twin(nb)
            for q in pr.MEASURES:
                for c in a[q]:
                    lo, hi = sorted((max(a[q][c], pr.FLOOR[q]), max(b[q][c], pr.FLOOR[q])))
                    assert hi <= pr.MARGIN * lo, (P, nb, q, c, a[q][c], b[q][c])


@pytest.mark.parametrize("P", [1, 2, 4, 5, 127, 128, 129, 300, 512, 640, 1000, 1100, 4096])
def test_sampled_points_contain_every_class_and_every_edge(P):
    idx = pr.sample_points(P)
    Pp = -(-P // 128) * 128
    assert idx == sorted(set(idx)) and len(idx) <= pr.MAX_SAMPLE and all(0 <= p < P for p in idx)
    assert len(idx) == min(P, max(40, len(idx))) or len(idx) >= 40
    want = {0, P - 1, Pp // 2 - 1, Pp // 2}
    for b in range(128, Pp + 1, 128):
        want |= {b - 1, b}
    assert {p for p in want if 0 <= p < P} <= set(idx)
    assert {pr.class_of(p) for p in idx} == {pr.class_of(p) for p in range(min(P, 5))}
    fx = pr.fixture("B", 129)
    xp, cls = pr.points(fx, P)
    assert xp.shape == (P, 2) and cls == [pr.class_of(p) for p in range(P)]
    for p in idx:
        c = cls[p]
        at = np.any(np.all(xp[p] == fx.x, axis=1))
        near = np.any(np.all(xp[p] - 1e-7 == fx.x, axis=1)) or np.min(np.max(np.abs(fx.x - xp[p]), axis=1)) <= 1.0000001e-7
        if c == "data":
            assert at
        elif c == "near":
            assert near and not at
        elif c == "far":
            assert np.all(xp[p] >= 50.0)
        elif c == "rand":
            assert np.all((xp[p] >= 0) & (xp[p] < 1)) and not at
        else:
            two = 2.0 * xp[p][None, None, :] - fx.x[:, None, :] - fx.x[None, :, :]
            assert np.min(np.max(np.abs(two), axis=2)) <= 4 * EPS
    assert pr.points(fx, P)[0].tobytes() == xp.tobytes()                # deterministic
    shifted = pr.points(fx, 1, first=3)
    assert shifted[1] == ["far"] and np.all(shifted[0] >= 50.0)
