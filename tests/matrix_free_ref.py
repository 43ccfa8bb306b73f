"""The numpy twin of the matrix-free solves (csrc/matrix_free.hip) and the fixtures its tests share (a helper module, not a conftest).

    kmatvec_ref      K B + diag(v) B in longdouble from kernel_family_ref.k_ref
    pchol_ref        the greedy pivoted Cholesky of K: argmax of the residual diagonal over the points not picked yet, ties to the lowest
                     index, c = (K[:, j] - G[:t]^T G[:t, j]) / sqrt(d_j), d <- max(d - c^2, 0), exhausted at d_j <= tol sigma^2
    woodbury_apply   (G^T G + D)^-1 R = D^-1 R - D^-1 G^T (I + G D^-1 G^T)^-1 G D^-1 R
    pcg_ref          the device's recurrence column by column: freeze at |r| <= tol |b|, after max_iter iterations or on breakdown, judge
                     on the true residual, restart from it at most max_restarts times

tests/test_matrix_free_host.py proves the twin against numpy.linalg and the fixtures' margins; tests/test_gpu_matrix_free.py holds the
device to the twin."""
import functools

import numpy as np

import kernel_family_ref as kf

LD = np.longdouble
EPS = kf.EPS
SIGMA2 = 1.3
CHUNK = 4096                  # FVGP_MATVEC_CHUNK


def theta_of(kernel, d, ell):
    """sigma^2 = 1.3, length scales from ell to 1.5 ell over the dimensions (one: ell)"""
    if kf.FAMILY[kernel][1]:
        return np.array([SIGMA2, ell])
    return np.concatenate([[SIGMA2], ell * np.linspace(1.0, 1.5, d)])


def kmatvec_ref(kernel, x1, x2, theta, B, vdiag=None):
    """(Y, |K| |B| + |v B|) in longdouble: the product and the magnitude sum its error bound scales with"""
    K = kf.k_ref(kernel, x1, x2, theta)
    B = np.asarray(B, dtype=LD)
    Y, mag = K @ B, np.abs(K) @ np.abs(B)
    if vdiag is not None:
        vb = np.asarray(vdiag, dtype=LD)[:, None] * B
        Y, mag = Y + vb, mag + np.abs(vb)
    return Y, mag


def kmatvec_bound(n2, B, mag):
    """the componentwise bound of the product: 4 ulp sigma^2 per entry of K times sum_j |B_jc|, plus Higham's gamma of a sum of
    n2 + 4 terms in any order on |K| |B| + |v_i B_ic|"""
    colsum = np.abs(np.asarray(B, dtype=LD)).sum(axis=0)
    return 4 * EPS * SIGMA2 * colsum[None, :] + (n2 + 4) * (EPS / 2) * mag


def k_double(kernel, x, theta):
    return np.asarray(kf.k_ref(kernel, x, x, theta), dtype=np.float64)


def pchol_ref(K, q, tol=0.0, sigma2=None):
    """(G (q, n), piv (q; -1 from the achieved rank on), d (n), rank, margins (q): lead of the pick over the runner-up)"""
    n = K.shape[0]
    sigma2 = float(K[0, 0]) if sigma2 is None else sigma2
    d = np.full(n, sigma2)
    G = np.zeros((q, n))
    piv = np.full(q, -1, dtype=np.int64)
    taken = np.zeros(n, dtype=bool)
    margins = np.full(q, np.inf)
    rank = 0
    for t in range(q):
        score = np.where(taken, -1.0, d)
        j = int(np.argmax(score))                 # (the first of equal maxima: ties to the lowest index)
        if taken[j] or d[j] <= tol * sigma2:
            break
        others = np.delete(score, j)
        if len(others):
            margins[t] = d[j] - others.max()
        c = (K[:, j] - G[:t].T @ G[:t, j]) / np.sqrt(d[j])
        G[t] = c
        d = np.maximum(d - c * c, 0.0)
        piv[t] = j
        taken[j] = True
        rank = t + 1
    return G, piv, d, rank, margins


def woodbury_apply(G, v, R):
    """(G^T G + diag(v))^-1 R; G None or of no rows: R / v"""
    R = np.asarray(R, dtype=np.float64)
    W = R / v[:, None] if R.ndim == 2 else R / v
    if G is None or len(G) == 0:
        return W
    C = np.eye(len(G)) + (G / v) @ G.T
    T = np.linalg.solve(C, G @ W)
    return W - (G.T @ T) / (v[:, None] if R.ndim == 2 else v)


def pcg_ref(A, b, v, G, tol, max_iter=1000, max_restarts=3, x0=None, precond=True):
    """one column of (A) x = b by the device's rules; A dense (K + diag(v)), the preconditioner (G, v) (precond=False: none, z = r).
    Returns (x, iters, true relative residual, status: 0 converged, 1 not converged, 2 breakdown)."""
    n = len(b)
    M = (lambda r: woodbury_apply(G, v, r)) if precond else (lambda r: r.copy())
    bn = np.sqrt(b @ b)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    if bn == 0.0:
        return np.zeros(n), 0, 0.0, 0
    r = b - A @ x if x0 is not None else b.copy()
    iters, restarts, code = 0, 0, 0
    active = np.sqrt(r @ r) > tol * bn
    while True:
        if active:
            z = M(r)
            rho = r @ z
            p = z.copy()
            if not rho > 0.0 or np.isinf(rho):
                active, code = False, 2
        while active:
            Ap = A @ p
            pap = p @ Ap
            if not pap > 0.0 or np.isinf(pap):
                active, code = False, 2
                break
            alpha = rho / pap
            x = x + alpha * p
            r = r - alpha * Ap
            iters += 1
            if np.sqrt(r @ r) <= tol * bn:
                active, code = False, 0
                break
            if iters >= max_iter:
                active, code = False, 1
                break
            z = M(r)
            rho_new = r @ z
            if not rho_new > 0.0 or np.isinf(rho_new):
                active, code = False, 2
                break
            p = z + (rho_new / rho) * p
            rho = rho_new
        r = b - A @ x
        relres = np.sqrt(r @ r) / bn
        if relres <= tol:
            return x, iters, relres, 0
        if code == 2:
            return x, iters, relres, 2
        if code == 1 or restarts >= max_restarts:
            return x, iters, relres, 1
        restarts += 1
        active = True


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
# (kernel, d, length scale, noise level, n, seed): every radial kind, ARD and isotropic, d = 1, 2, 3 and 5; points uniform in the unit cube,
# noise = level (1 + U[0, 1)).  The three d = 2 cases are the ones whose iteration counts motivated the preconditioner; every fixture here is
# a pivot fixture (the margins of test_matrix_free_host.py).
FIXTURES = (
    ("rbf_ard", 2, 0.25, 1e-2, 1000, 11),
    ("matern32_ard", 2, 0.3, 1e-2, 1000, 12),
    ("matern52_ard", 2, 0.3, 1e-3, 1000, 13),
    ("matern32_iso", 1, 0.3, 1e-2, 1001, 14),
    ("matern52_iso", 3, 0.3, 1e-2, 997, 15),
    ("rbf_iso", 3, 0.4, 1e-2, 1000, 16),
    ("matern32_ard", 5, 0.6, 1e-2, 1000, 17),
)
PRECOND_FIXTURES = FIXTURES[:3]
PIVOT_FIXTURES = FIXTURES
# The solution-accuracy fixtures: the first one converges in 2 iterations and overshoots tol = 1e-9 down to 5e-13, the rounding floor of a
# residual evaluated in double (about sqrt(n) eps |x| / |b| from the kernel entries' own rounding), where no double-precision residual can be
# confirmed to 10 % in longdouble.  A shorter length scale takes its place: 6 iterations, a final residual above 1e-10.
ACCURACY_FIXTURES = (("rbf_ard", 2, 0.12, 1e-2, 1000, 11),) + FIXTURES[1:]
RANK = 128


def fixture_id(fx):
    return f"{fx[0]}-d{fx[1]}-n{fx[4]}"


@functools.lru_cache(maxsize=None)
def fixture(fx):
    """the fixture's arrays, computed once and shared (read-only): x, V, theta, K (double), A = K + diag(V)"""
    kernel, d, ell, level, n, seed = fx
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    V = level * (1.0 + rng.random(n))
    theta = theta_of(kernel, d, ell)
    K_ld = kf.k_ref(kernel, x, x, theta)
    K = np.asarray(K_ld, dtype=np.float64)
    out = {"kernel": kernel, "x": x, "V": V, "theta": theta, "K": K, "K_ld": K_ld, "A": K + np.diag(V), "rhs": rng.standard_normal((n, 16))}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture_pchol(fx, q=RANK):
    f = fixture(fx)
    return pchol_ref(f["K"], q, tol=0.0, sigma2=SIGMA2)


@functools.lru_cache(maxsize=None)
def fixture_pcg(fx, col, rank, tol, precond=True):
    """the twin's solve of column `col` of the fixture's right-hand sides with the rank-`rank` preconditioner (0: Jacobi)"""
    f = fixture(fx)
    G = fixture_pchol(fx, rank)[0] if rank else None
    return pcg_ref(f["A"], f["rhs"][:, col], f["V"], G, tol, precond=precond)


def matvec_case(n1, n2, d, s, seed, square=False):
    """x1 (n1, d), x2 (n2, d) (square: x2 = x1, with two coincident points), B (n2, s) of full-mantissa entries scaled by rows over
    2^-20 .. 2^20, v (n1)"""
    rng = np.random.default_rng(seed)
    x2 = rng.random((n2, d))
    x1 = x2 if square else rng.random((n1, d))
    if square and n2 > 2:
        x2[n2 - 1] = x2[0]
    B = rng.standard_normal((n2, s)) * np.exp2(rng.integers(-20, 21, size=(n2, 1)).astype(np.float64))
    v = 0.01 * (1.0 + rng.random(n1))
    return x1, x2, B, v
