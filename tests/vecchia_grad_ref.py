"""A numpy twin of the nearest-neighbour likelihood's exact gradient (a helper module of the tests, not a conftest): the per-row scores of
include/fvgp_hip_nn.h (fvgp_hip_nn_loglik_grad) in a chosen number type, built on vecchia_ref and kernel_family_ref, and the cases the
host and the device tests share.

    scores_ref      per row i with the neighbour list c: Sigma = K over (c, i), A = Sigma[c, c] + diag(v_c), k = Sigma[c, i], A = L L^T,
                    a = A^-1 k, beta = A^-1 r_c, e = r_i - k^T beta, d = Sigma[i, i] + v_i - k^T a, b = (-a, 1), g = (beta, 0),
                    q = (e / d) g + 1/2 (e^2 / d^2 - 1 / d) b,   score_h = b^T (dSigma / dtheta_h) q
    dense_grad_ld   the exact GP's d log p / d theta = 1/2 (alpha^T dK alpha - tr((K + V)^-1 dK)) by a longdouble Cholesky
                    (tests/test_vecchia_grad_host.py holds the twin to it with m = n - 1, and to differences of vecchia_ref.loglik_ref)

THE BARS of tests/test_gpu_vecchia_grad.py.  Two figures per case:
    score = max over h of max_i |s_ih - ref_ih| / max_i |ref_ih|
    grad  = max over h of |g_h - ref_h| / sum_i |ref_ih|          (a scale that cannot cancel; a gradient near an optimum can)
base = the larger of two float64 twin runs against the longdouble run on the same inputs: one plain, one with every kernel entry
perturbed by up to kernel_family_ref.k_bound_ulps(d) ulps of sigma^2 (as in vecchia_ref) and every derivative entry by a relative error of
up to (16 + d) eps -- half of kernel_family_ref.grad_trace_bound_factor's per-term allowance 32 + 2 d, which covers two evaluations.  The
device must stay within MARGIN * max(base, FLOOR[figure]), MARGIN = vecchia_ref.MARGIN; FLOOR is the median of the bases over GRAD_CASES,
computed and asserted by tests/test_vecchia_grad_host.py::test_floor_is_the_median_of_the_bases and recorded here.  Nothing here comes
from the device."""
import functools

import numpy as np

import kernel_family_ref as kf
import vecchia_ref as vr

LD = vr.LD
EPS = kf.EPS
MARGIN = vr.MARGIN
FIGURES = ("score", "grad")
# the medians of the bases over GRAD_CASES (test_vecchia_grad_host.py asserts these are what bases() gives, to 1 %)
FLOOR = {"score": 4.79e-13, "grad": 6.92e-14}


# ---- linear algebra in a number type ------------------------------------------------------------------------------------------------------
def _chol(A, dtype):
    m = len(A)
    L = np.zeros((m, m), dtype=dtype)
    for j in range(m):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def _solve(L, b):
    """(L L^T)^-1 b, b a vector or a matrix of columns"""
    y = np.array(b, dtype=L.dtype)
    m = len(L)
    for i in range(m):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


# ---- the scores ---------------------------------------------------------------------------------------------------------------------------
def scores_ref(name, x, theta, idx, r, v, dtype=LD, perturb=None):
    """(n, H) in dtype: row i is d log p(y_i | y_c(i)) / d theta for the neighbour lists idx (entries outside 0 .. n - 1 skipped).
    perturb = (rng, ulps, rel): every kernel entry gets a uniform error in +-ulps eps sigma^2 and every derivative entry a uniform
    relative error in +-rel (both symmetrically)."""
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    r, v = np.asarray(r, dtype=dtype), np.asarray(v, dtype=dtype)
    n, H = len(x), len(theta)
    out = np.zeros((n, H), dtype=dtype)
    half = dtype(1) / dtype(2)
    for i in range(n):
        c = np.array([j for j in idx[i] if 0 <= j < n], dtype=np.int64)
        m = len(c)
        pts = x[np.concatenate([c, [i]])]
        S = kf.k_ref(name, pts, pts, theta, dtype)
        dS = kf.dk_dtheta_ref(name, pts, pts, theta, dtype)
        if perturb is not None:
            rng, ulps, rel = perturb
            E = np.tril(rng.uniform(-1.0, 1.0, S.shape))
            S = S + (ulps * EPS * float(theta[0]) * (E + np.tril(E, -1).T)).astype(dtype)
            F = np.tril(rng.uniform(-1.0, 1.0, dS.shape))
            dS = dS * (dtype(1) + (rel * (F + np.transpose(np.tril(F, -1), (0, 2, 1)))).astype(dtype))
        dv = S[m, m] + v[i]
        b, g = np.zeros(m + 1, dtype=dtype), np.zeros(m + 1, dtype=dtype)
        b[m] = dtype(1)
        e = r[i]
        if m:
            L = _chol(S[:m, :m] + np.diag(v[c]), dtype)
            a, beta = _solve(L, S[:m, m]), _solve(L, r[c])
            b[:m], g[:m] = -a, beta
            e = r[i] - np.dot(S[:m, m], beta)
            dv = dv - np.dot(S[:m, m], a)
        q = (e / dv) * g + half * (e * e / (dv * dv) - dtype(1) / dv) * b
        out[i] = np.einsum("p,hpq,q->h", b, dS, q)
    return out


def dense_grad_ld(name, x, theta, r, v):
    """the exact d log p / d theta (H,) = 1/2 (alpha^T dK alpha - tr((K + V)^-1 dK)) by a longdouble Cholesky, and sum |terms|: the sum of
    the absolute values of every product that enters it (the scale its rounding is held to)"""
    n = len(x)
    L = _chol(kf.k_ref(name, x, x, theta, LD) + np.diag(np.asarray(v, dtype=LD)), LD)
    Ainv = _solve(L, np.eye(n, dtype=LD))
    alpha = Ainv @ np.asarray(r, dtype=LD)
    dK = kf.dk_dtheta_ref(name, x, x, theta, LD)
    W = np.outer(alpha, alpha) - Ainv
    return np.sum(W[None] * dK, axis=(1, 2)) / LD(2), np.sum(np.abs(W[None] * dK), axis=(1, 2)) / LD(2)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# (kernel, d, n, m, B): every kernel id, d over kernel_family_ref.DIMS, m in {1, 15, 16, 17, 31, 32, 33, 63, 64}, n in {1, 2, 70} (the first
# rows have fewer neighbours than m, the row count is no multiple of the waves per workgroup; n <= 70 keeps a longdouble reference at
# m >= 63 to seconds), B in {1, 3}, and one case of 300 rows with m = 3: its sums cross a 256-row slice
GRAD_CASES = (
    ("rbf_ard", 1, 70, 1, 1), ("matern32_ard", 2, 70, 15, 3), ("matern52_ard", 3, 70, 16, 1), ("rbf_iso", 4, 70, 17, 1),
    ("matern32_iso", 5, 70, 31, 1), ("matern52_iso", 16, 70, 32, 3), ("rbf_ard", 16, 70, 33, 1), ("matern32_ard", 3, 70, 63, 1),
    ("matern52_ard", 5, 70, 64, 1), ("rbf_iso", 2, 70, 64, 3), ("matern32_iso", 1, 2, 16, 1), ("matern52_iso", 4, 1, 32, 1),
    ("rbf_ard", 3, 2, 1, 3), ("matern52_ard", 2, 300, 3, 1),
)
SLICE_CASE = GRAD_CASES[-1]


def figures(got, ref):
    """the two figures of the (n, H) scores `got` (their column sums, or got = (scores, gradient) with the gradient given) against
    the longdouble scores `ref`"""
    s, g = got if isinstance(got, tuple) else (got, None)
    s = np.asarray(s, dtype=LD)
    g = np.sum(s, axis=0) if g is None else np.asarray(g, dtype=LD)
    tiny = LD(np.finfo(np.float64).tiny)
    smax = np.maximum(np.max(np.abs(ref), axis=0), tiny)         # (a column of zeros -- n = 1's length scales -- is held absolutely)
    ssum = np.maximum(np.sum(np.abs(ref), axis=0), tiny)
    zero = np.max(np.abs(ref), axis=0) == 0
    smax, ssum = np.where(zero, LD(1), smax), np.where(zero, LD(1), ssum)
    return {"score": float(np.max(np.max(np.abs(s - ref), axis=0) / smax)),
            "grad": float(np.max(np.abs(g - np.sum(ref, axis=0)) / ssum))}


@functools.lru_cache(maxsize=None)
def reference(case):
    """per b the longdouble (n, H) scores of a case: computed once, shared, never changed"""
    x, thetas, r, v, idx = vr.case_inputs(case)
    return tuple(scores_ref(case[0], x, t, idx, r, v, LD) for t in thetas)


@functools.lru_cache(maxsize=None)
def bases(case):
    """{figure: base}: over the case's thetas, the larger of the plain and the perturbed float64 twin's figures against longdouble"""
    name, d = case[0], case[1]
    x, thetas, r, v, idx = vr.case_inputs(case)
    out = dict.fromkeys(FIGURES, 0.0)
    for b, t in enumerate(thetas):
        ref = reference(case)[b]
        rng = np.random.default_rng(5151 + b)
        for run in (scores_ref(name, x, t, idx, r, v, np.float64),
                    scores_ref(name, x, t, idx, r, v, np.float64, perturb=(rng, kf.k_bound_ulps(d), (16 + d) * EPS))):
            f = figures(run, ref)
            out = {k: max(out[k], f[k]) for k in FIGURES}
    return out


def bars(case):
    """{figure: MARGIN * max(base, FLOOR)}: what the device may differ from longdouble by"""
    b = bases(case)
    return {k: MARGIN * max(b[k], FLOOR[k]) for k in FIGURES}
