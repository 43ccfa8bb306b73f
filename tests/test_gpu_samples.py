"""Joint sampling on the device (fvgp_hip_normal_fill, fvgp_hip_mvn_sample, GP.posterior_samples / prior_samples) against the numpy twin of
the generator (tests/samples_ref.py) and host linear algebra.

Inputs as the other GPU tests draw them: n = 200 points uniform in the unit square, sigma^2 = 1.2, length scales in [0.3, 0.6], noise
0.01 - 0.02 per point, y centred.  Bars:
  normals against the twin   1e-13 absolute: |z| <= 8.7 (u1 >= 2^-54), log, sqrt and cos on both sides are within a few ulp (ulp(8) = 1.8e-15),
                             the rounding of 2 pi u2 moves the cosine by at most 7e-16, times 8.7
  the draw against numpy     rtol 1e-12, atol 1e-12 max|L| 8.7 sqrt(n): a forward sum of at most 300 terms in another order
  the facade identity        rtol 1e-9, atol 1e-9: with noise >= 0.01 and sigma^2 = 1.2 cond(S + noise) < P 1.2 / 0.01 = 1.6e4, so a Cholesky
                             factor moves by about 1e4 eps = 4e-12 relative between two factorisations
  statistics                 6 sigma per entry of the sample mean and covariance of 4096 draws
Every prefix / chunk / repeat comparison is bitwise."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import samples_ref as sr

pytestmark = pytest.mark.gpu

SEED, STREAM = 2 ** 40 + 7, 2 ** 33 + 1            # the high words of both count
CANARY = -7.25
ZMAX = 8.7


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _twin(rows, cols, row0=0, col0=0, seed=SEED, stream=STREAM):
    z = sr.normal_block(seed, stream, row0, col0, rows, cols)
    z.setflags(write=False)
    return z


def _fill(H, rows, cols, ld, row0=0, col0=0):
    """fvgp_hip_normal_fill into the leading rows x cols of a (rows + 1, ld) buffer of canaries; the whole buffer on the host"""
    buf = H.torch.full((rows + 1, ld), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    H.normal_fill(buf[:rows, :cols], SEED, STREAM, row0, col0)
    H.sync()
    return buf.cpu().numpy()


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (3, 5, 9), (130, 257, 257), (130, 257, 258)])
def test_fill_equals_the_twin_and_writes_nothing_else(H, rows, cols, ld):
    got = _fill(H, rows, cols, ld)
    err = float(np.max(np.abs(got[:rows, :cols] - _twin(rows, cols))))
    print(f"SAMPLES|fill vs twin|{rows}x{cols} ld {ld}|{err:.3g}")
    assert err <= 1e-13
    assert np.all(got[:rows, cols:] == CANARY) and np.all(got[rows] == CANARY)


def test_fill_of_a_sub_block_is_bitwise_the_block_of_the_large_fill(H):
    big = _fill(H, 130, 257, 257)[:130, :257]
    for ld in (90, 91, 157):            # 16-byte stores, 8-byte stores (odd leading dimension), a wider row
        sub = _fill(H, 40, 90, ld, row0=64, col0=100)
        assert np.array_equal(sub[:40, :90], big[64:104, 100:190])
        assert np.all(sub[:40, 90:] == CANARY) and np.all(sub[40] == CANARY)
    # the last row and sample index there is: 2^32 - 1
    edge = _fill(H, 1, 1, 1, row0=2 ** 32 - 1, col0=2 ** 32 - 1)[0, 0]
    assert abs(edge - float(sr.normal(SEED, STREAM, 2 ** 32 - 1, 2 ** 32 - 1))) <= 1e-13


def test_fill_refuses_bad_arguments_and_touches_nothing(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    buf = H.torch.full((4, 8), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    p = ctypes.c_void_p(buf.data_ptr())
    two32 = 2 ** 32
    cases = [((None, 2, 2, 8), 0, 0, -6), ((p, 0, 2, 8), 0, 0, -7), ((p, 2, 0, 8), 0, 0, -8), ((p, 2, 8, 7), 0, 0, -9),
             ((p, 2, 2, 8), two32 - 1, 0, -4), ((p, 2, 2, 8), -1, 0, -4), ((p, 2, 2, 8), 0, two32 - 1, -5), ((p, 2, 2, 8), 0, -1, -5)]
    for (z, rows, cols, ld), row0, col0, want in cases:
        assert L.fvgp_hip_normal_fill(H._h, SEED, STREAM, row0, col0, z, rows, cols, ld) == want
    H.sync()
    assert np.all(buf.cpu().numpy() == CANARY)


# ---- 2. the draw -----------------------------------------------------------------------------------------------------------------------
NS = (1, 127, 128, 129, 300)
NSAMP = (1, 5, 128, 300)


@functools.lru_cache(maxsize=None)
def _spd(n):
    """a random symmetric matrix with eigenvalues in [1, 1e3] and a mean vector"""
    rng = np.random.default_rng(1000 + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, 3.0, n) if n > 1 else np.array([2.5])
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2, rng.standard_normal(n)


_factors = {}


def _factor(H, n):
    """the padded factor as fvgp_hip_potrf leaves it (the strict upper triangle still holds the matrix), kept per n"""
    from fvgp_amd import _lib
    if n not in _factors:
        np_ = _lib.pad128(n)
        A = H.zeros(np_, np_)
        A[:n, :n] = H.to_device(_spd(n)[0])
        assert H.potrf(A, n) == 0
        H.sync()
        _factors[n] = A
    return _factors[n]


def _draw(H, L, n, nsamp, samp0=0, mean=None, want_z=True, pad=3):
    """fvgp_hip_mvn_sample into the leading n columns of an (nsamp + 1, n + pad) buffer of canaries: (Y, Z_out, the whole buffer)"""
    buf = H.torch.full((nsamp + 1, n + pad), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    Z = H.empty(n, nsamp) if want_z else None
    H.mvn_sample(L, n, buf[:nsamp, :n], mean=None if mean is None else H.to_device(mean), seed=SEED, stream=STREAM, samp0=samp0, Z_out=Z)
    H.sync()
    full = buf.cpu().numpy()
    return full[:nsamp, :n], (None if Z is None else Z.cpu().numpy()), full


@pytest.mark.parametrize("nsamp", NSAMP)
@pytest.mark.parametrize("n", NS)
def test_draw_equals_the_host_product(H, n, nsamp):
    L = _factor(H, n)
    mean = _spd(n)[1]
    Y, Z, full = _draw(H, L, n, nsamp, mean=mean)
    Lh = np.tril(L[:n, :n].cpu().numpy())
    ez = float(np.max(np.abs(Z - _twin(n, nsamp))))
    ref = mean[None, :] + (Lh @ Z).T
    atol = 1e-12 * float(np.max(np.abs(Lh))) * ZMAX * np.sqrt(n)
    ratio = float(np.max(np.abs(Y - ref) / (atol + 1e-12 * np.abs(ref))))
    print(f"SAMPLES|draw / bar|n {n} nsamp {nsamp}|{ratio:.3g}   normals vs twin {ez:.3g}")
    assert ez <= 1e-13
    assert ratio <= 1.0
    assert np.all(full[:nsamp, n:] == CANARY) and np.all(full[nsamp] == CANARY)
    # nothing above the diagonal of L, and nothing of its padding, reaches Y
    L2 = L.clone()
    iu = H.torch.triu_indices(L2.shape[0], L2.shape[1], 1)
    L2[iu[0], iu[1]] = float("nan")
    L2[n:, :] = float("nan")
    Y2, _, _ = _draw(H, L2, n, nsamp, mean=mean, want_z=False)
    assert np.array_equal(Y2, Y)
    # without a mean: the product alone, and Y is the mean added to it
    Y0, _, _ = _draw(H, L, n, nsamp, want_z=False)
    assert np.array_equal(mean[None, :] + Y0, Y)


@pytest.mark.parametrize("n", NS)
def test_a_sample_does_not_depend_on_its_call(H, n):
    L = _factor(H, n)
    mean = _spd(n)[1]
    Y, Z, _ = _draw(H, L, n, 300, mean=mean)
    one, z1, _ = _draw(H, L, n, 1, mean=mean)
    assert np.array_equal(one[0], Y[0]) and np.array_equal(z1[:, 0], Z[:, 0])
    tail, zt, _ = _draw(H, L, n, 200, samp0=100, mean=mean, pad=4)          # (another row alignment of Y too)
    assert np.array_equal(tail, Y[100:300]) and np.array_equal(zt, Z[:, 100:300])
    again, _, _ = _draw(H, L, n, 300, mean=mean, want_z=False)
    assert np.array_equal(again, Y)


def test_draw_refuses_bad_arguments(H):
    from fvgp_amd import _lib
    lib = _lib.lib()
    n, nsamp = 129, 5
    L = _factor(H, n)
    Y = H.torch.full((nsamp, n), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    wb = _lib.mvn_sample_workspace_bytes(n, nsamp)
    work = H.empty(wb // 8)
    pL, pY, pW = (ctypes.c_void_p(t.data_ptr()) for t in (L, Y, work))

    def call(L_=pL, n_=n, ldl=L.stride(0), samp0=0, ns=nsamp, Y_=pY, ldy=n, Z_=None, ldz=0, W_=pW, wb_=wb):
        return lib.fvgp_hip_mvn_sample(H._h, L_, n_, ldl, None, SEED, STREAM, samp0, ns, Y_, ldy, Z_, ldz, W_, wb_)
    assert call(L_=None) == -2 and call(n_=0) == -3 and call(ldl=128) == -4
    assert call(samp0=2 ** 32 - 4) == -8 and call(samp0=-1) == -8 and call(ns=0) == -9
    assert call(Y_=None) == -10 and call(ldy=n - 1) == -11 and call(Z_=pY, ldz=nsamp - 1) == -13
    assert call(W_=None) == -14 and call(wb_=wb - 8) == -15
    H.sync()
    assert np.all(Y.cpu().numpy() == CANARY)
    assert call() == 0


# ---- 3 - 5. the facade -----------------------------------------------------------------------------------------------------------------
def _inputs(n=200, d=2, seed=20260101):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    theta = np.concatenate([[1.2], rng.uniform(0.3, 0.6, d)])
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y - y.mean() + 0.25, rng.uniform(0.01, 0.02, n), theta


def _gp(kernel="rbf_ard", **kw):
    import fvgp_amd
    x, y, V, theta = _inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function=kernel, **kw)


def _identity(r, S, rtol=1e-9, atol=1e-9):
    """samples - m = (chol(S + jitter I) normals)^T"""
    P = S.shape[0]
    ref = (np.linalg.cholesky(S + r["jitter"] * np.eye(P)) @ r["normals"]).T
    got = r["samples"] - r["m(x)_flat"][None, :]
    print(f"SAMPLES|facade identity|P {P}|{float(np.max(np.abs(got - ref))):.3g}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol)


def test_posterior_samples_identity_state_and_determinism():
    # CPU check of the case (float64 S of the same inputs from tests/kernel_family_ref.py, the twin's normals): cond(S + noise) = 3.0, and a
    # symmetric relative perturbation of S by 1e-14 moves chol(S + jitter I) @ normals by 7.2e-15 (max |product| 0.53): far below 1e-10
    gp = _gp()
    xq = np.random.default_rng(77).random((130, 2))
    before = (gp.log_likelihood(), gp.hyperparameters.copy(), gp.Chol_factor, gp.KVinvY)
    m = gp.posterior_mean(xq)["m(x)_flat"]
    r = gp.posterior_samples(xq, 64, add_noise=True, return_normals=True)
    assert r["samples"].shape == (64, 130) and r["normals"].shape == (130, 64) and r["jitter"] == 1e-9
    assert "samples(x)" not in r and np.array_equal(r["x"], xq)
    assert float(np.max(np.abs(r["normals"] - _twin(130, 64, seed=0, stream=0)))) <= 1e-13
    _identity(r, gp.posterior_covariance(xq, add_noise=True)["S"])
    assert np.array_equal(r["m(x)_flat"], m)
    after = (gp.log_likelihood(), gp.hyperparameters, gp.Chol_factor, gp.KVinvY)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(gp.posterior_mean(xq)["m(x)_flat"], m)
    again = gp.posterior_samples(xq, 64, add_noise=True)
    assert np.array_equal(again["samples"], r["samples"]) and "normals" not in again
    assert np.array_equal(gp.posterior_samples(xq, 3, add_noise=True)["samples"], r["samples"][:3])      # a longer call extends a shorter one
    for kw in ({"seed": 1}, {"stream": 1}):
        other = gp.posterior_samples(xq, 64, add_noise=True, **kw)["samples"]
        assert not np.any(other == r["samples"])


def test_statistics_through_the_whole_path():
    # CPU check (float64 S of the same inputs, the twin's normals at this seed): the largest mean deviation is 1.5 and the largest
    # covariance deviation 2.9 of their standard errors, against the bar of 6; the smallest eigenvalue of S is 5.9e-9
    gp = _gp()
    xs = np.random.default_rng(5).random((32, 2))
    n_s = 4096
    r = gp.posterior_samples(xs, n_s, seed=2026, jitter=1e-9)
    S = gp.posterior_covariance(xs)["S"]
    m = gp.posterior_mean(xs)["m(x)_flat"]
    F = r["samples"]
    d = np.diag(S)
    mu = F.mean(axis=0)
    r_mean = float(np.max(np.abs(mu - m) / np.sqrt(d / n_s)))
    C = (F - mu).T @ (F - mu) / (n_s - 1)
    r_cov = float(np.max(np.abs(C - S) / np.sqrt((np.outer(d, d) + S ** 2) / n_s)))
    print(f"SAMPLES|statistics / sigma|mean {r_mean:.3g} covariance {r_cov:.3g}")
    assert r_mean <= 6.0
    assert r_cov <= 6.0


@pytest.mark.parametrize("P", [20, 129])
def test_prior_samples(P):
    # jitter 1e-3: cond(K + jitter I) is 1.1e4 at 20 and 7.6e4 at 129 of these points (1e-9 would leave 1e10 and a factor that two
    # factorisations agree on to 1e-6 only); CPU check: a relative perturbation of K by 1e-14 moves the product by 1.0e-12 / 6.2e-12
    from fvgp_amd import kernels
    gp = _gp()
    xp = np.random.default_rng(9).random((P, 2))
    r = gp.prior_samples(xp, 16, jitter=1e-3, return_normals=True, stream=5)
    assert r["samples"].shape == (16, P) and r["normals"].shape == (P, 16) and r["jitter"] == 1e-3
    assert np.array_equal(r["m(x)_flat"], np.full(P, np.mean(gp.y_data)))
    assert float(np.max(np.abs(r["normals"] - _twin(P, 16, seed=0, stream=5)))) <= 1e-13
    _identity(r, np.asarray(kernels.rbf_ard(xp, xp, gp.hyperparameters), dtype=np.float64))
    assert np.array_equal(gp.prior_samples(xp, 16, jitter=1e-3, stream=5)["samples"], r["samples"])


def test_fvgp_with_x_out():
    import fvgp_amd
    rng = np.random.default_rng(11)
    x = rng.random((100, 2))
    y = np.stack([np.sin(3.0 * x.sum(axis=1) + 0.3 * t) + 0.1 * rng.standard_normal(100) for t in range(2)], axis=1)
    nv = rng.uniform(0.01, 0.02, (100, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(x, y, init_hyperparameters=np.array([1.2, 0.4, 0.5, 2.0]), noise_variances=nv, kernel_function="rbf_ard")
    xq = rng.random((10, 2))
    r = gp.posterior_samples(xq, 8, add_noise=True, return_normals=True)
    assert r["samples"].shape == (8, 20) and r["samples(x)"].shape == (8, 10, 2) and r["normals"].shape == (20, 8)
    pm = gp.posterior_mean(xq)
    assert np.array_equal(r["m(x)_flat"], pm["m(x)_flat"])
    for s in range(8):                                              # ordered as m(x) is: [point, task] of the task-major flat vector
        assert np.array_equal(r["samples(x)"][s], r["samples"][s].reshape(10, 2, order="F"))
    _identity(r, gp.posterior_covariance(xq, add_noise=True)["S_flat"])
    p = gp.prior_samples(xq, 4, jitter=1e-3)
    assert p["samples"].shape == (4, 20) and p["samples(x)"].shape == (4, 10, 2)


def _callable_gp():
    from fvgp_amd import kernels
    return _gp(kernel=lambda a, b, h: kernels.rbf_ard(a, b, h))


@pytest.mark.parametrize("make,P", [(_callable_gp, 20), (lambda: _gp(linalg_mode="CholInv"), 20),
                                    (lambda: _gp(args={"posterior_chunk": 128}), 150)],
                         ids=["kernel callable", "CholInv", "more than posterior_chunk points"])
def test_modes(make, P):
    gp = make()
    xq = np.random.default_rng(13).random((P, 2))
    r = gp.posterior_samples(xq, 8, add_noise=True, return_normals=True, seed=4)
    assert r["samples"].shape == (8, P) and r["normals"].shape == (P, 8)
    np.testing.assert_allclose(r["m(x)_flat"], gp.posterior_mean(xq)["m(x)_flat"], rtol=1e-12, atol=1e-12)
    _identity(r, gp.posterior_covariance(xq, add_noise=True)["S"])
    p = gp.prior_samples(xq[:20], 4, jitter=1e-3)
    assert p["samples"].shape == (4, 20)


def test_linalg_callables_mode():
    import scipy.linalg as sla
    gp = _gp(linalg_mode=[lambda KV: sla.cho_factor(KV, lower=True), lambda f, b: sla.cho_solve(f, b),
                          lambda f: 2.0 * float(np.sum(np.log(np.diag(f[0]))))])
    xq = np.random.default_rng(13).random((20, 2))
    r = gp.posterior_samples(xq, 8, add_noise=True, return_normals=True)
    assert r["samples"].shape == (8, 20)
    _identity(r, gp.posterior_covariance(xq, add_noise=True)["S"])


def test_a_factorisation_that_cannot_succeed_raises():
    gp = _gp()
    xq = np.tile(np.random.default_rng(3).random((8, 2)), (4, 1))      # every point four times: S is singular
    ll = gp.log_likelihood()
    with pytest.raises(Exception, match=r"dpotrf info = \d+.*larger `jitter`"):
        gp.posterior_samples(xq, 4, jitter=0)
    assert gp.log_likelihood() == ll
    assert gp.posterior_samples(xq, 4, jitter=1e-6)["samples"].shape == (4, 32)
