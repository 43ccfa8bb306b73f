"""A numpy twin of the nearest-neighbour (Vecchia) path (a helper module of the tests, not a conftest): the search, the conditionals and
the likelihood of include/fvgp_hip_nn.h in a chosen number type, and the cases the host and the device tests share.

    search_ref          the m nearest candidates by a (distance, index) sort, distances in float64
    conditionals_ref    per row: A = K(x_c, x_c) + diag(v_c), k = K(x_c, x_i), a Cholesky in the number type, w = L^-1 k, z = L^-1 r_c,
                        mu = w^T z, d = k(x_i, x_i) + s_i - w^T w -- in longdouble (the reference) or float64 (the twin whose own error
                        against longdouble sets the device's bars); kernel entries from kernel_family_ref.k_ref
    loglik_ref          log p = -1/2 sum_i [(r_i - mu_i)^2 / d_i + log d_i + log 2 pi] and its two parts
    dense_loglik_ld     the exact GP's log-likelihood by a longdouble Cholesky of K + V (tests/test_vecchia_host.py holds the twin to it
                        with m >= n - 1, which is what makes the twin a reference)

THE BARS of tests/test_gpu_vecchia.py.  For every case of ACC_CASES and every figure (FIGURES), base = the larger of two float64 twin
runs against the longdouble run on the same inputs: one plain, one with every kernel entry perturbed by a uniform random error of up to
kernel_family_ref.k_bound_ulps(d) ulps of sigma^2 -- the device assembly's documented entry bound, which the m x m solves amplify.  The
device must stay within MARGIN * max(base, FLOOR[figure]); FLOOR is the median of the bases over ACC_CASES, computed and asserted by
tests/test_vecchia_host.py::test_floor_is_the_median_of_the_bases and recorded here:

    FLOOR = {"mu": 3.40e-14, "d": 7.05e-14, "loglik": 4.51e-15, "fit": 3.90e-15, "logdet": 9.57e-16}

MARGIN = 8 is the project's own (chol_update_ref.MARGIN), for a different but equally stable operation order.  Nothing here comes from
the device."""
import functools

import numpy as np

import kernel_family_ref as kf

LD = np.longdouble
EPS = kf.EPS
MARGIN = 8
FIGURES = ("mu", "d", "loglik", "fit", "logdet")
# the medians of the bases over ACC_CASES (test_vecchia_host.py asserts these are what bases() gives, to 1 %)
FLOOR = {"mu": 3.40e-14, "d": 7.05e-14, "loglik": 4.51e-15, "fit": 3.90e-15, "logdet": 9.57e-16}


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def inv_scales(scales, d, dtype=np.float64):
    """(d,): 1 / scale_k in dtype, ones for scales None -- the one place the twins of the search, the ordering and the grid take it from"""
    return np.ones(d, dtype=dtype) if scales is None else dtype(1) / np.asarray(scales, dtype=dtype)


def distances(xq, xr, scales=None, dtype=np.float64):
    """(nq, nr): sum_k ((xq_ik - xr_jk) * (1 / scale_k))^2 added in ascending k (float64: every operation as the device rounds it,
    except that the device fuses each square into the sum)"""
    xq, xr = np.asarray(xq, dtype=dtype), np.asarray(xr, dtype=dtype)
    inv = inv_scales(scales, xq.shape[1], dtype)
    out = np.zeros((len(xq), len(xr)), dtype=dtype)
    for k in range(xq.shape[1]):
        e = (xq[:, k][:, None] - xr[:, k][None, :]) * inv[k]
        out = out + e * e
    return out


def candidates(i, nr, c0):
    """number of candidates of query i: the reference rows j < min(nr, c0 + i), or all of them for c0 < 0"""
    return nr if c0 < 0 else min(nr, c0 + i)


def search_ref(xq, xr, m, scales=None, c0=-1):
    """int32 (nq, m): per query the min(m, candidates) nearest candidates sorted by (distance, index), then -1"""
    D = distances(xq, xr, scales)
    out = np.full((len(xq), m), -1, dtype=np.int32)
    for i in range(len(xq)):
        nc = candidates(i, len(xr), c0)
        order = np.lexsort((np.arange(nc), D[i, :nc]))[:m]
        out[i, :len(order)] = order
    return out


def check_search_rows(idx, xq, xr, m, scales, c0):
    """the properties of a search result (the twin's or the device's), distances in longdouble: every index a legal candidate, none
    repeated, the row sorted by (distance, index), exactly the candidates there are and then -1, and the largest chosen distance at most
    the smallest unchosen one times (1 + 4 * 2^-52)"""
    D = distances(xq, xr, scales, LD)
    for i in range(len(xq)):
        nc = candidates(i, len(xr), c0)
        k = min(m, nc)
        row = idx[i]
        assert np.all(row[k:] == -1) and np.all((row[:k] >= 0) & (row[:k] < nc)) and len(set(row[:k])) == k
        slack = 1 + LD(4) * LD(2) ** -52           # (the device orders by distances rounded to double)
        for a, b in zip(row[:k - 1], row[1:k]):
            assert D[i, a] <= D[i, b] * slack and (D[i, a] != D[i, b] or a < b), (i, a, b)
        rest = np.setdiff1d(np.arange(nc), row[:k])
        if k and len(rest):
            assert D[i, row[k - 1]] <= np.min(D[i, rest]) * slack


# ---- the conditionals -----------------------------------------------------------------------------------------------------------------
def _chol_solve(A, k, z, dtype):
    """column-by-column Cholesky of A in dtype and both substitutions: (w = L^-1 k, L^-1 z, the factor's diagonal)"""
    m = len(k)
    L = np.zeros((m, m), dtype=dtype)
    for j in range(m):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    w, zz = np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype)
    for i in range(m):
        w[i] = (k[i] - L[i, :i] @ w[:i]) / L[i, i]
        zz[i] = (z[i] - L[i, :i] @ zz[:i]) / L[i, i]
    return w, zz, np.diagonal(L).copy()


def conditionals_ref(name, xq, xr, theta, idx, r, v, s=None, dtype=LD, perturb=None):
    """(mu (nq,), d (nq,)) in dtype for the neighbour lists idx (entries outside 0 .. nr - 1 skipped).  perturb = (rng, ulps): every
    kernel entry gets a uniform error in +-ulps eps sigma^2 (the matrix symmetrically)."""
    xq, xr = np.asarray(xq, dtype=np.float64), np.asarray(xr, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    r, v = np.asarray(r, dtype=dtype), np.asarray(v, dtype=dtype)
    mu, d = np.zeros(len(xq), dtype=dtype), np.zeros(len(xq), dtype=dtype)
    amp = 0.0 if perturb is None else perturb[1] * EPS * float(theta[0])
    for i in range(len(xq)):
        c = np.array([j for j in idx[i] if 0 <= j < len(xr)], dtype=np.int64)
        kxx = kf.k_ref(name, xq[i:i + 1], xq[i:i + 1], theta, dtype)[0, 0]
        if perturb is not None:
            kxx = kxx + dtype(amp * perturb[0].uniform(-1.0, 1.0))
        if s is not None:
            kxx = kxx + dtype(s[i])
        if len(c) == 0:
            d[i] = kxx
            continue
        A = kf.k_ref(name, xr[c], xr[c], theta, dtype)
        k = kf.k_ref(name, xr[c], xq[i:i + 1], theta, dtype)[:, 0]
        if perturb is not None:
            E = np.tril(perturb[0].uniform(-1.0, 1.0, A.shape))
            A = A + (amp * (E + np.tril(E, -1).T)).astype(dtype)
            k = k + (amp * perturb[0].uniform(-1.0, 1.0, k.shape)).astype(dtype)
        A = A + np.diag(v[c])
        w, z, _ = _chol_solve(A, k, r[c], dtype)
        mu[i] = np.dot(w, z)
        d[i] = kxx - np.dot(w, w)
    return mu, d


def loglik_terms(r, mu, d, dtype=LD):
    """(log p, fit, logdet) from the conditionals, in dtype"""
    r, mu, d = np.asarray(r, dtype=dtype), np.asarray(mu, dtype=dtype), np.asarray(d, dtype=dtype)
    fit = np.sum((r - mu) ** 2 / d)
    logdet = np.sum(np.log(d))
    return -(fit + logdet + dtype(len(r)) * np.log(dtype(2) * dtype(np.pi))) / dtype(2), fit, logdet


def loglik_ref(name, x, theta, idx, r, v, dtype=LD, perturb=None):
    """(log p, fit, logdet, mu, d): the conditionals of x on itself with s = v, and their sums"""
    mu, d = conditionals_ref(name, x, x, theta, idx, r, v, s=np.asarray(v, dtype=dtype), dtype=dtype, perturb=perturb)
    return loglik_terms(r, mu, d, dtype) + (mu, d)


def dense_loglik_ld(name, x, theta, r, v):
    """the exact log-likelihood -1/2 (r^T (K + V)^-1 r + log det(K + V) + n log 2 pi) by a longdouble Cholesky"""
    A = kf.k_ref(name, x, x, theta, LD) + np.diag(np.asarray(v, dtype=LD))
    _, z, L_diag = _chol_solve(A, np.zeros(len(x), dtype=LD), np.asarray(r, dtype=LD), LD)
    fit, logdet = np.dot(z, z), LD(2) * np.sum(np.log(L_diag))
    return -(fit + logdet + LD(len(x)) * np.log(LD(2) * LD(np.pi))) / LD(2)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def case_data(name, d, n, seed=0, noise=1e-2):
    """x (n, d) from the unit cube, theta = kernel_family_ref.case_theta, centred data r, positive noise v of order noise sigma^2 (so the
    m x m blocks stay well conditioned)"""
    rng = np.random.default_rng(7000 + 100 * d + 10 * sorted(kf.FAMILY).index(name) + n + 1000003 * seed)
    x = rng.random((n, d))
    theta = kf.case_theta(name, d, rng)
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    r = y - np.mean(y)
    v = noise * theta[0] * (1.0 + rng.random(n))
    return x, theta, r, v


def length_scales(name, theta, d):
    return np.full(d, theta[1]) if kf.FAMILY[name][1] else np.asarray(theta[1:1 + d])


def batch_thetas(theta, B):
    """the B hyperparameter vectors of a case: theta itself first, then scaled copies"""
    return np.array([theta * f for f in (1.0, 1.3, 0.8)[:B]])


# (kernel, d, n, m, B): every kernel id, d in {1, 2, 3, 4, 5, 16}, m in {1, 15, 16, 17, 31, 32, 33, 63, 64}, n in {1, 2, 70, 200} (the
# first rows have fewer neighbours than m, the row count is no multiple of the waves per workgroup), B in {1, 3}
ACC_CASES = (
    ("rbf_ard", 1, 200, 1, 1), ("matern32_ard", 2, 200, 15, 3), ("matern52_ard", 3, 200, 16, 1), ("rbf_iso", 4, 200, 17, 1),
    ("matern32_iso", 5, 200, 31, 1), ("matern52_iso", 16, 200, 32, 3), ("rbf_ard", 16, 70, 33, 1), ("matern32_ard", 3, 70, 63, 1),
    ("matern52_ard", 5, 200, 64, 1), ("rbf_iso", 2, 70, 64, 3), ("matern32_iso", 1, 2, 16, 1), ("matern52_iso", 4, 1, 32, 1),
    ("matern32_ard", 1, 70, 32, 1), ("rbf_ard", 3, 2, 1, 3), ("matern52_ard", 2, 200, 33, 1), ("matern32_iso", 3, 70, 17, 1),
)
EXACT_CASE = ("matern32_ard", 3, 65, 64, 1)      # m = n - 1 on the given order: the nearest-neighbour likelihood IS the exact one


def case_id(case):
    return "{}-d{}-n{}-m{}-B{}".format(*case)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(x, thetas (B, H), r, v, idx): the inputs of one accuracy case, the same on the host and on the device; the neighbour lists are
    the twin's under the first theta's length scales"""
    name, d, n, m, B = case
    x, theta, r, v = case_data(name, d, n)
    idx = search_ref(x, x, m, length_scales(name, theta, d), c0=0)
    return x, batch_thetas(theta, B), r, v, idx


def figures(r, got, ref):
    """the five figures of (log p, fit, logdet, mu, d) `got` against the longdouble `ref`"""
    rel = lambda a, b: float(abs(LD(a) - b) / abs(b)) if b != 0 else float(abs(LD(a)))      # noqa: E731
    scale = max(float(np.max(np.abs(r))), np.finfo(np.float64).tiny)
    return {"mu": float(np.max(np.abs(np.asarray(got[3], dtype=LD) - ref[3]))) / scale,
            "d": float(np.max(np.abs(np.asarray(got[4], dtype=LD) - ref[4]) / np.abs(ref[4]))),
            "loglik": rel(got[0], ref[0]), "fit": rel(got[1], ref[1]), "logdet": rel(got[2], ref[2])}


@functools.lru_cache(maxsize=None)
def reference(case):
    """per b the longdouble (log p, fit, logdet, mu, d) of a case: computed once, shared, never changed"""
    name = case[0]
    x, thetas, r, v, idx = case_inputs(case)
    return tuple(loglik_ref(name, x, t, idx, r, v, LD) for t in thetas)


@functools.lru_cache(maxsize=None)
def bases(case):
    """{figure: base}: over the case's thetas, the larger of the plain and the perturbed float64 twin's figures against longdouble"""
    name, d = case[0], case[1]
    x, thetas, r, v, idx = case_inputs(case)
    out = dict.fromkeys(FIGURES, 0.0)
    for b, t in enumerate(thetas):
        ref = reference(case)[b]
        rng = np.random.default_rng(4242 + b)
        for run in (loglik_ref(name, x, t, idx, r, v, np.float64),
                    loglik_ref(name, x, t, idx, r, v, np.float64, perturb=(rng, kf.k_bound_ulps(d)))):
            f = figures(r, run, ref)
            out = {k: max(out[k], f[k]) for k in FIGURES}
    return out


def bars(case):
    """{figure: MARGIN * max(base, FLOOR)}: what the device may differ from longdouble by"""
    b = bases(case)
    return {k: MARGIN * max(b[k], FLOOR[k]) for k in FIGURES}
