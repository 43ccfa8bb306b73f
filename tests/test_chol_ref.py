"""The reference of the Cholesky tests proved on the host, before any kernel runs (tests/chol_ref.py; the device side is
tests/test_gpu_chol.py): the longdouble factorisation returns a chosen factor; every matrix the device tests factor has the condition
number their caps assume; the caps are attainable -- LAPACK and the float64 twins of both panel solves stay under them on every fixture;
the sampled rows of the backward error speak for all rows; and a power-of-two scaling changes no bit of the twins' factors."""
import numpy as np
import pytest

import chol_ref as cr

EPS, LD = cr.EPS, cr.LD
FIXTURES = [(f, n) for f in "WGH" for n in (129, 700, 1300)] + [(f, n) for f in "GH" for n in (1281, 1408)]


def _dyadic_factor(n, seed):
    """a lower-triangular L of small integers over 16 (diagonal 16 .. 31 over 16): every entry of L L^T is a sum of at most n products
    of two 5-bit integers over 256, exactly representable in float64"""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-8, 9, (n, n)), -1) / 16.0
    L[np.arange(n), np.arange(n)] = rng.integers(16, 32, n) / 16.0
    return L


@pytest.mark.parametrize("n", [1, 2, 17, 129, 300])
def test_chol_ld_returns_a_chosen_factor(n):
    L = _dyadic_factor(n, n)
    A = L @ L.T
    assert np.array_equal(np.asarray(A, dtype=LD), np.asarray(L, dtype=LD) @ np.asarray(L, dtype=LD).T)      # the product is exact
    got = cr.chol_ld(A)
    assert got.dtype == LD and got.shape == (n, n) and np.array_equal(got, np.tril(got))
    assert cr.phi(got, np.asarray(L, dtype=LD)) <= 4 * cr.EPS_LD * n
    # only the lower triangle is read
    junk = np.tril(A) + np.triu(np.full((n, n), np.nan), 1)
    assert np.array_equal(cr.chol_ld(junk), got)
    with pytest.raises(TypeError):
        cr.chol_ld(A.astype(np.float32))


def test_chol_ld_names_the_failing_minor():
    A = _dyadic_factor(20, 3)
    A = A @ A.T
    A[7, 7] = -3.0
    with pytest.raises(np.linalg.LinAlgError, match="order 8 "):
        cr.chol_ld(A)


@pytest.mark.parametrize("fam,n", FIXTURES)
def test_fixtures_meet_the_conditions_the_caps_rest_on(fam, n):
    """cond_2 within 30 % of the value written down in chol_ref.COND; scipy's LAPACK and both twins under the derived caps the device
    tests use: beta <= 2 (n + 1) for substitution (scipy, the 16-tile twin), times max_k cond_2(Lhat_kk) for the product with the explicit
    128-inverse; phi <= 64 eps cond_2(A); lam <= n eps cond_2(A)"""
    R = cr.reference(fam, n)
    A = R.A
    assert A.shape == (n, n) and A.dtype == np.float64 and not A.flags.writeable and np.array_equal(A, A.T)
    want = cr.COND[(fam, n)]
    assert 0.7 * want <= R.cond <= 1.3 * want, R.cond
    rows = cr.edge_rows(n, (512, 1024), n)
    fig = {w: (R.beta(w, rows), R.phi(w), R.lam(w)) for w in ("scipy", 16, 128)}
    print(f"CHREF|{fam}|{n}|cond {R.cond:.3g}|block cond {R.block_cond():.3g}|"
          + "|".join(f"{w}: beta {b:.3g} phi {p:.3g} lam {l:.3g}" for w, (b, p, l) in fig.items()))
    for w, (b, p, l) in fig.items():
        assert b <= R.cap_beta(explicit=(w == 128)), (w, b)
        assert p <= R.cap_phi(), (w, p)
        assert l <= R.cap_lam(), (w, l)
    if fam == "W":                  # on the easy matrix the two panel solves cannot be told apart ...
        assert fig[128][0] <= 4 * max(fig[16][0], 4)
    if fam == "H" and n >= 700:     # ... on the hard covariance the explicit inverse costs two orders of magnitude of backward error
        assert fig[128][0] >= 20 * max(fig[16][0], fig["scipy"][0])


def test_sampled_rows_speak_for_all_rows():
    """beta over the at most 24 rows of edge_rows() (and the whole diagonal) is within a factor 4 of beta over every row, n = 700, for
    LAPACK and both twins on W and H (H: 8.4 / 13.9, 63.6 / 63.6, 4970 / 7050).  beta is a maximum over entries and has a heavy tail:
    on G the 16-tile twin has ONE row (496) at 338 where the 99th percentile of the rows is 12.3 and the sample gives 12.3 -- there the
    sample is asserted to be a lower bound and within a factor 4 of the 99th percentile, no more, which is why every device case also
    carries phi over all rows."""
    n = 700
    for fam in "WGH":
        R = cr.reference(fam, n)
        rows = cr.edge_rows(n, (512,), n)
        for w in ("scipy", 16, 128):
            some = R.beta(w, rows)
            diag, per = cr.beta_parts(R.A, R.factor(w), range(n))
            every, p99 = max(diag, float(per.max())), max(diag, float(np.quantile(per, 0.99)))
            print(f"CHREF|rows|{fam}|{w}|sampled {some:.3g}|all {every:.3g}|99th percentile of the rows {p99:.3g}")
            assert some <= every, (fam, w, some, every)
            if (fam, w) != ("G", 16):
                assert every <= 4 * some, (fam, w, some, every)
            else:                   # all but the tail: the sample and the 99th percentile of the rows within a factor 4 of each other
                assert p99 <= 4 * some and some <= 4 * p99, (some, p99, every)


@pytest.mark.parametrize("n,bounds", [(1, ()), (2, ()), (17, ()), (129, ()), (1300, (512, 1024)), (1300, (256, 512, 768, 1024, 1280)), (1408, (1024,))])
def test_edge_rows(n, bounds):
    rows = cr.edge_rows(n, bounds, seed=n)
    assert len(rows) == min(n, cr.MAX_ROWS) and len(set(rows)) == len(rows) and rows == sorted(rows)
    for r in [0, 1, 15, 16, 17, 127, 128, 129, n - 2, n - 1] + [b + s for b in bounds for s in (-1, 1)]:
        assert r in rows or not 0 <= r < n
    assert rows == cr.edge_rows(n, bounds, seed=n)
    if n == 1300:
        assert len(set(rows) - {0, 1, 15, 16, 17, 127, 128, 129, n - 2, n - 1} - {b + s for b in bounds for s in (-1, 1)}) >= 4      # random ones


def test_measures_see_a_small_row_and_a_wrong_tile():
    """the max-norm over a whole factor hides a wrong row of small magnitude and a wrong tile away from the sampled rows; phi does not,
    and beta sees a sampled row that is off by a few units of its own size"""
    R = cr.reference("H", 129)
    L = np.array(R.factor("scipy"))
    assert cr.phi(L, R.Lhat) <= R.cap_phi()
    bad = L.copy()
    i = int(np.argmin(np.linalg.norm(L, axis=1)))
    bad[i, :i + 1] *= 1.0 + 1e-6
    assert cr.phi(bad, R.Lhat) >= 0.9e-6
    tile = L.copy()
    tile[100:116, 32:48] *= 1.0 + 1e-9
    assert cr.phi(tile, R.Lhat) >= 1e-11 and cr.beta(R.A, tile, [100]) > 100 * cr.beta(R.A, L, [100])
    assert cr.beta(R.A, np.where(np.tril(np.ones_like(L)) > 0, L, np.nan), [5]) == cr.beta(R.A, L, [5])      # the upper triangle is not read
    assert cr.beta(R.A, np.full_like(L, np.nan), [5]) == np.inf and cr.phi(np.full_like(L, np.inf), R.Lhat) == np.inf
    assert cr.lam(L, R.Lhat) <= R.cap_lam() and cr.lam(2 * L, R.Lhat) > 100
    assert cr.lam_value(float(cr.logdet_ld(R.Lhat)), R.Lhat) <= cr.lam_floor(R.Lhat)


@pytest.mark.parametrize("fam", ["S", "U-", "U+"])
def test_scaled_families_reproduce_the_unscaled_bits(fam):
    """D G D and 2^(+-400) G: numpy's Cholesky and both twins return D times the factor of G bit for bit (no order of sums depends on
    the data), and so does chol_ld -- which is why reference() may scale Lhat(G) instead of factoring again"""
    import scipy.linalg as sla
    n = 300
    G, A, D = cr.matrix("G", n), cr.matrix(fam, n), cr.row_scale(fam, n)
    assert np.all(np.frexp(D)[0] == 0.5)
    if fam == "S":
        assert D.min() >= 2.0 ** -20 and D.max() <= 2.0 ** 20 and D.min() < D.max()
    assert np.array_equal(A, D[:, None] * G * D[None, :]) and np.all(np.isfinite(A))
    for tb in (16, 128):
        assert np.array_equal(cr.twin_chol(A, tb), D[:, None] * cr.twin_chol(G, tb))
    assert np.array_equal(sla.cholesky(A, lower=True), D[:, None] * sla.cholesky(G, lower=True))
    R, Rg = cr.reference(fam, n), cr.reference("G", n)
    assert np.array_equal(cr.chol_ld(A), R.Lhat) and R.cond == Rg.cond
    rows = cr.edge_rows(n, (), n)
    for w in ("scipy", 16, 128):                    # beta and phi are invariant under the scaling
        assert R.beta(w, rows) == Rg.beta(w, rows) and R.phi(w) == Rg.phi(w)
