"""tests/batch_ref.py on the host: the longdouble reference of the batched entries is right, the fixtures are what the caps assume,
every float64 twin stays under the derived caps the project states, and the conditions under which the device tests' measures mean
something hold -- all without a GPU."""
import numpy as np
import pytest

import batch_ref as br
import chol_ref
import kernel_family_ref as kf
import posterior_ref as pr
import tri_solve_ref as ts

LD, EPS, EPS_LD = br.LD, br.EPS, br.EPS_LD
FAMS = ("E", "G", "H", "M")
SMALL_N = (1, 124, 300)
GRAD_N = tuple(n for n in br.GPU_N if n != 1300)                    # the gradient and the posterior stop at 897
POST_CASES = [(n, ncol, P) for n, ncol in ((124, 8), (300, 1), (700, 1)) for P in (1, 20, 129, 300)]
INFO_CASES = [(513, j) for j in (0, 127, 128, 300, 512)] + [(124, 123)]


@pytest.mark.parametrize("fam", ["G", "H"])
@pytest.mark.parametrize("n", [124, 513])
def test_rbf_fixtures_are_chol_refs_matrices(fam, n):
    """k_ref at theta = (1, l, l) reproduces tri_solve_ref.covariance_g: the diagonal in its bits, the rest to the rounding of the two
    formulas.  covariance_g forms r^2 = |x|^2 + |x'|^2 - 2 x.x' from numbers below 2 in a handful of roundings (at most 8 eps absolute),
    which the division by 2 l^2 turns into 4 eps / l^2 relative in K; k_ref is good to longdouble, and exp adds a few eps to each."""
    ell, noise = chol_ref.PARAMS[fam]
    A, Kg = br.problem(fam, n).A, ts.covariance_g(n, br.SEED, ell, noise)
    assert np.array_equal(np.diagonal(A), np.diagonal(Kg))
    assert np.all(np.abs(A - Kg) <= (4.0 / ell ** 2 + 4.0) * EPS * Kg)


def test_scaled_fixtures_are_exact_scalings():
    g = br.problem("G", 124)
    for fam, e in br.U_EXP.items():
        u = br.problem(fam, 124)
        assert np.array_equal(u.A, np.ldexp(g.A, e)) and np.array_equal(u.y, np.ldexp(g.y, e // 2)) and np.array_equal(u.V, np.ldexp(g.V, e))
        assert np.all(np.isfinite(u.A)) and np.array_equal(np.ldexp(u.A, -e), g.A) and np.array_equal(np.ldexp(u.y, -e // 2), g.y)
        r, rg = br.reference(fam, 124), br.reference("G", 124)
        assert np.array_equal(r.Lhat, chol_ref.chol_ld(u.A))                 # the scaled factor IS chol_ld of the scaled matrix
        assert np.array_equal(r.z, rg.z)
        np.testing.assert_allclose(np.asarray(r.out(8)[2], dtype=np.float64), float(rg.out(8)[2]), rtol=0)


@pytest.mark.parametrize("key", sorted(br.COND))
def test_cond_bands(key):
    """the recorded cond_2 within 30 % (the caps phi <= 64 eps cond_2 and lam <= n eps cond_2 rest on them)"""
    fam, n = key
    c = chol_ref.cond2(br.problem(fam, n).A)
    assert 0.7 * br.COND[key] <= c <= 1.3 * br.COND[key], (key, c)


def test_cond_table_covers_every_device_case():
    assert {(f, n) for f in FAMS for n in br.GPU_N} <= set(br.COND)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("n", SMALL_N)
def test_reference_identities(fam, n):
    """Lhat Lhat^T = A and What Lhat = I to a few EPS_LD n, each counted against the magnitudes that enter the entry (componentwise: the
    inverse of an ill-conditioned factor has large entries); KVinv A = I the same way; z and alpha solve their systems"""
    r = br.reference(fam, n)
    A, L, W = np.asarray(r.p.A, dtype=LD), r.Lhat, r.What
    tol = 4 * EPS_LD * max(n, 2)
    assert np.all(np.abs(np.tril(L @ L.T - A)) <= tol * (np.abs(L) @ np.abs(L).T))
    assert np.all(np.abs(W @ L - np.eye(n, dtype=LD)) <= tol * (np.abs(W) @ np.abs(L)))
    assert np.all(np.triu(W, 1) == 0)
    assert np.all(np.abs(r.KVinv @ A - np.eye(n, dtype=LD)) <= 4 * tol * (np.abs(W).T @ np.abs(W) @ np.abs(A)))
    y = np.asarray(r.p.y, dtype=LD)
    assert np.all(np.abs(L @ r.z - y) <= tol * (np.abs(L) @ np.abs(r.z)))
    assert np.all(np.abs(r.alpha - r.KVinv @ y) <= tol * (np.abs(r.KVinv) @ np.abs(y)))
    np.testing.assert_allclose(np.asarray(r.dinv, dtype=np.float64), np.asarray(np.diagonal(r.KVinv), dtype=np.float64), rtol=1e-15)
    # the single-column substitution of chol_ref agrees with the many-column one
    assert np.array_equal(chol_ref.fwd_ld(L, r.p.y[:, 3]), r.z[:, 3])
    # the values: the closed form at n = 1, numpy's float64 route elsewhere (only as good as cond_2 eps)
    out = np.asarray(r.out(2), dtype=np.float64)
    if n == 1:
        a = r.p.A[0, 0]
        q = np.mean(r.p.y[0, :2] ** 2) / a
        # (log|KV| = 2 log sqrt(a) carries the longdouble rounding of the root: absolute EPS_LD, not relative, where a is near 1)
        np.testing.assert_allclose(out, [-0.5 * (q + np.log(a) + np.log(2 * np.pi)), np.log(a), q], rtol=4 * EPS, atol=4 * EPS_LD)
    else:
        rough = 64 * n * EPS * r.chol.cond
        np.testing.assert_allclose(out[1], np.linalg.slogdet(r.p.A)[1], rtol=0, atol=rough * n)
        np.testing.assert_allclose(out[2], np.mean(np.sum(r.p.y[:, :2] * np.linalg.solve(r.p.A, r.p.y[:, :2]), axis=0)), rtol=rough)


@pytest.mark.parametrize("fam,n,c", [("E", 60, 0), ("E", 124, 7), ("M", 60, 1), ("M", 124, 0)])
def test_reference_gradient_matches_central_difference(fam, n, c):
    """the reference gradient (of the NEGATIVE log-likelihood, component c) against a central difference of the longdouble
    log-likelihood.  The difference quotient sees A rounded to float64 at both ends: with a step h = 1e-4 theta_i that is
    eps |KVinv| |A| / h, about 1e-12 M_i / h ... and the truncation h^2 / 6 of a third derivative of the order of M_i / theta_i^3:
    1e-6 M_i covers both."""
    r = br.reference(fam, n)
    p = r.p
    g, M = r.grad(c)
    yc = p.y[:, c:c + 1]
    for i in range(len(p.theta)):
        h = 1e-4 * p.theta[i]
        tp, tm = p.theta.copy(), p.theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = -(br.loglik_ld(p.kernel, p.x, tp, p.V, yc) - br.loglik_ld(p.kernel, p.x, tm, p.V, yc)) / LD(tp[i] - tm[i])
        assert abs(fd - g[i]) <= 1e-6 * M[i], (i, float(fd), float(g[i]), float(M[i]))
        assert abs(g[i]) >= 1e-3 * M[i]                                   # so that the comparison says something


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("n", [n for n in GRAD_N if n > 1])
def test_twins_stay_under_the_derived_caps(fam, n):
    """beta <= 2 (n + 1) max_k cond_2(Lhat_kk) (twin "a": the explicit block inverse; scipy's substitution: 2 (n + 1)),
    phi <= 64 eps cond_2, lam <= n eps cond_2 -- the caps of chol_ref.Reference, with this module's fixtures and edge rows"""
    r = br.reference(fam, n)
    dim = 128 * (-(-(n + 1) // 128))
    for t in br.Reference.TWINS:
        m = r.twin_factor(t, 1, dim)
        assert m["beta"] <= r.chol.cap_beta(t == "a"), (t, m)
        assert m["phi"] <= r.chol.cap_phi(), (t, m)
        assert m["lam"] <= r.chol.cap_lam(), (t, m)
    bars = r.factor_bars(1, dim)
    assert all(np.isfinite(b) and b > 0 for _, b in bars.values())


def test_halving_bounds_and_inverse_twin():
    assert br.halving_bounds(128) == [] and br.halving_bounds(256) == [128]
    assert br.halving_bounds(384) == [128, 256]                              # 1 + 2
    assert br.halving_bounds(640) == [128, 256, 384, 512]                    # 2 + 3
    assert br.halving_bounds(768) == [128, 256, 384, 512, 640]               # 3 + 3, then 1 + 2 twice
    assert br.halving_bounds(1408)[:1] == [128] and 640 in br.halving_bounds(1408)      # 5 + 6
    r = br.reference("E", 300)
    W = br.inverse_twin(r.L("a"))
    assert np.all(np.triu(W, 1) == 0)
    assert br.row_err(W, r.What) <= 64 * EPS * r.chol.cond
    np.testing.assert_allclose(W @ r.L("a"), np.eye(300), atol=1e-9)


@pytest.mark.parametrize("n,ncol", [(n, c) for n in GRAD_N if n > 1 for c in ((1, 8) if n == 124 else (1, 2) if n == 513 else (1,))])
def test_gradients_are_not_degenerate(n, ncol):
    """every component of the reference gradient has |ghat_i| >= 1e-3 M_i on E and M (a relative figure means something there); on the
    ill-conditioned fixtures only the M_i-relative measure is used"""
    for fam in ("E", "M"):
        g, M = br.reference(fam, n).grad(ncol - 1)
        assert np.all(np.abs(g) >= 1e-3 * M), (fam, n, np.asarray(np.abs(g) / M, dtype=np.float64))


@pytest.mark.parametrize("n,ncol,P", POST_CASES)
def test_posterior_conditions(n, ncol, P):
    """no sampled point of class "near" has a reference variance below 10 eps sigma^2 (nu counts in units of eps sigma^2: below that
    the measure could not tell a right variance from 0); far points are exactly prior; the two formulations of the mean agree"""
    for fam in FAMS:
        r = br.reference(fam, n)
        xp, cls = br.points(r, P)
        idx = pr.sample_points(P)
        ref = br.PosteriorReference(r, xp[idx], [cls[i] for i in idx], ncol)
        sig = r.p.theta[0]
        for s, c in enumerate(ref.cls):
            if c == "near":
                assert ref.v[s] >= 10 * EPS * sig, (fam, n, P, s, float(ref.v[s]))
            if c == "far":           # (matern32 at l = 0.15: exp(-980), 0 in float64 and not in longdouble)
                assert np.all(np.asarray(ref.k[:, s], dtype=np.float64) == 0) and ref.v[s] == sig
                assert np.all(np.asarray(ref.m[s], dtype=np.float64) == 0)
        m2 = ref.k.T @ r.alpha[:, :ncol]
        assert np.all(np.abs(ref.m - m2) <= 64 * r.n * EPS_LD / EPS * ref.den_mu * r.chol.cond)
        bars = ref.bars()
        assert all(np.isfinite(b) for q in bars.values() for _, b in q.values())


@pytest.mark.parametrize("n,j", INFO_CASES)
def test_info_fixtures_fail_at_the_intended_minor(n, j):
    """V[j] = -10 on E: the leading minor of order j + 1 is the first that is not positive"""
    p = br.problem("E", n)
    A = p.A.copy()
    A[j, j] = p.theta[0] - 10.0
    with pytest.raises(np.linalg.LinAlgError, match=f"order {j + 1} "):
        chol_ref.chol_ld(A)
    if j:
        chol_ref.chol_ld(A[:j, :j])
