"""The reference of the triangular-solve tests proved on the host, before any kernel runs (tests/tri_solve_ref.py; the device side is
tests/test_gpu_tri_solve.py): the longdouble substitution reproduces a solution chosen in longdouble; every factor the device tests
use has the condition number their bars assume; and the bars are attainable -- LAPACK's substitution and the float64 twin of the device
algorithm at both block widths stay within 64 eps cond_2(L) of the longdouble solution and within a factor 8 of each other."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import tri_solve_ref as ref

EPS, LD = ref.EPS, ref.LD
NCOL = 16


@pytest.mark.parametrize("fam,n", [("W", 1), ("W", 129), ("G", 700), ("H", 2432)])
def test_substitution_reproduces_a_longdouble_solution(fam, n):
    """B = L X and B = L^T X formed in longdouble from a longdouble X (B is then not a float64 array, which fwd_ld / bwd_ld accept as
    an intermediate): the solve returns X to 4 eps_longdouble n, relative, per column"""
    L, _ = ref.fixture(fam, n)
    rng = np.random.default_rng(n)
    X = np.asarray(rng.standard_normal((n, 5)), dtype=LD) + np.asarray(rng.standard_normal((n, 5)), dtype=LD) * LD(2.0) ** -40
    Ll = np.asarray(L, dtype=LD)
    bound = 4 * ref.EPS_LD * n
    # the residual of the solve in the norm of the solution: |X_solved - X| <= bound |X| needs a well-conditioned system, so it is
    # asserted on the residual, which substitution keeps small whatever the condition
    for solve, op in ((ref.fwd_ld, Ll), (ref.bwd_ld, Ll.T)):
        B = op @ X
        got = solve(L, B)
        assert got.dtype == LD and got.shape == X.shape
        res = np.sqrt(np.sum((op @ got - B) ** 2, axis=0)) / (np.sqrt(np.sum(np.abs(op) ** 2)) * np.sqrt(np.sum(got ** 2, axis=0)))
        assert float(np.max(res)) <= bound
    Bp = Ll @ (Ll.T @ X)
    gp = ref.potrs_ld(L, Bp)
    res = np.sqrt(np.sum((Ll @ (Ll.T @ gp) - Bp) ** 2, axis=0)) / (np.sum(np.abs(Ll) ** 2) * np.sqrt(np.sum(gp ** 2, axis=0)))
    assert float(np.max(res)) <= bound
    if fam == "W":                                  # cond_2 = 2: the solution itself comes back
        assert ref.col_err(ref.fwd_ld(L, Ll @ X), X)[1] <= bound
        assert ref.col_err(gp, X)[1] <= bound


def test_substitution_takes_vectors_and_reads_the_lower_triangle_only():
    L, _ = ref.fixture("G", 100)
    junk = L + np.triu(np.full((100, 100), np.nan), 1)
    b = ref.rhs(100, 1, 3)[:, 0]
    y = ref.fwd_ld(junk, b)
    assert y.shape == (100,) and y.dtype == LD and np.all(np.isfinite(y))
    assert np.array_equal(y, ref.fwd_ld(L, b.reshape(100, 1))[:, 0])
    assert np.all(np.isfinite(ref.potrs_ld(junk, b)))
    with pytest.raises(TypeError):
        ref.fwd_ld(L.astype(np.float32), b)


@functools.lru_cache(maxsize=None)
def _errors(fam, n):
    """worst per-column errors of the three float64 algorithms against longdouble, forward solve and L L^T solve: computed once"""
    L, cond = ref.fixture(fam, n)
    B = ref.rhs(n, NCOL, 5)
    y = ref.fwd_ld(L, B)
    x = ref.bwd_ld(L, y)
    fwd = {"lapack": sla.solve_triangular(L, B, lower=True), "twin128": ref.blockinv_fwd(L, B, 128), "twin1024": ref.blockinv_fwd(L, B, 1024)}
    pot = {"lapack": sla.cho_solve((L, True), B), "twin128": ref.blockinv_potrs(L, B, 128), "twin1024": ref.blockinv_potrs(L, B, 1024)}
    return cond, {k: ref.col_err(v, y)[1] for k, v in fwd.items()}, {k: ref.col_err(v, x)[1] for k, v in pot.items()}


@pytest.mark.parametrize("fam,n", ref.GPU_FIXTURES)
def test_fixtures_meet_the_conditions_the_bars_rest_on(fam, n):
    L, cond = ref.fixture(fam, n)
    assert L.shape == (n, n) and L.dtype == np.float64 and not L.flags.writeable
    assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0)
    lo, hi = ref.COND_RANGE[fam]
    if n >= 700:
        assert lo <= cond <= hi, cond
    else:
        assert 1.0 <= cond <= hi, cond
    if fam in "GH" and n >= 700:                    # the grading of a covariance factor: the diagonal falls from 1 to sqrt(noise)
        d = np.diag(L)
        assert 0.99 <= d.max() <= 1.01 and d.min() <= 2e-3
    cond_, fwd, pot = _errors(fam, n)
    print(f"TSREF|{fam}|{n}|cond {cond:.3g}|fwd " + " ".join(f"{k} {v:.2g}" for k, v in fwd.items())
          + "|potrs " + " ".join(f"{k} {v:.2g}" for k, v in pot.items()))
    # errors below 4 eps count as 4 eps (the floor of the measured bar): at n = 1 a solve can be exact
    for errs, cap in ((fwd, 64 * EPS * cond), (pot, 64 * EPS * cond * cond)):
        assert max(errs.values()) <= cap, (errs, cap)
        floor = 4 * EPS if n < 700 else 0.0
        vals = [max(v, floor) for v in errs.values()]
        assert max(vals) <= 8 * min(vals), errs


def test_twin_doubling_handles_the_narrow_last_pair():
    """n = 2432 = 2 x 1024 + 384: the last 1024-block is 384 wide, doubled as (128 | 128) then (256 | 128) -- a pair whose second half is
    narrower.  Every block inverse times its block is the identity to eps cond of the block."""
    L, _ = ref.fixture("G", 2432)
    inv = ref.block_inverses(L, 1024)
    assert [w.shape[0] for w in inv] == [1024, 1024, 384]
    for W, J0 in zip(inv, range(0, 2432, 1024)):
        A = L[J0:J0 + len(W), J0:J0 + len(W)]
        assert np.array_equal(W, np.tril(W))
        assert np.max(np.abs(W @ A - np.eye(len(W)))) <= 64 * EPS * ref.cond2(A)


@pytest.mark.parametrize("nrhs", [1, 2, 3, 8, 31, 32, 33, 128, 129, 512, 640, 1152])
def test_edge_columns(nrhs):
    cols = ref.edge_columns(nrhs, seed=nrhs)
    assert len(cols) == min(nrhs, 32) and len(set(cols)) == len(cols) and cols == sorted(cols)
    assert cols[0] == 0 and cols[-1] == nrhs - 1
    for c in (1, 15, 16, 63, 64, 127, 128, nrhs // 2 - 1, nrhs // 2):
        assert c in cols or not 0 <= c < nrhs
    assert cols == ref.edge_columns(nrhs, seed=nrhs)


def test_col_err_sees_a_small_column():
    """the max-norm over a whole result hides a wrong column of small magnitude; the per-column measure does not"""
    refm = np.stack([np.ones(10), 1e-9 * np.ones(10)], axis=1)
    got = refm.copy()
    got[:, 1] *= 1.5
    assert np.max(np.abs(got - refm)) / np.max(np.abs(refm)) < 1e-9
    e, worst = ref.col_err(got, refm)
    assert e[0] == 0.0 and abs(worst - 0.5) < 1e-12
    assert ref.col_err(np.zeros((3, 1)), np.zeros((3, 1)))[1] == 0.0 and ref.col_err(np.ones((3, 1)), np.zeros((3, 1)))[1] == np.inf


def test_scaled_family_has_the_solution_of_the_unscaled_one():
    """family S: (D L)(y) = D B has the bits of L y = B under LAPACK's substitution too (a data-independent order of sums), and the
    L L^T solve returns D^-1 x"""
    n = 129
    L, _ = ref.fixture("W", n)
    D = ref.scaling_s(n, ref.SEED)
    assert np.all(np.frexp(D)[0] == 0.5) and D.min() >= 2.0 ** -20 and D.max() <= 2.0 ** 20
    B = ref.rhs(n, 3, 9)
    y = ref.fwd_ld(L, B)
    ys = ref.fwd_ld(D[:, None] * L, D[:, None] * B)
    assert np.array_equal(np.asarray(ys, dtype=np.float64), np.asarray(y, dtype=np.float64))
    xs = ref.potrs_ld(D[:, None] * L, D[:, None] * B)
    assert ref.col_err(D[:, None] * np.asarray(xs, dtype=np.float64), ref.potrs_ld(L, B))[1] <= 4 * EPS
