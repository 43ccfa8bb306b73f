"""An extended-precision reference of leave-one-out cross-validation for the native kernel family (a helper module of the tests, not a
conftest), written in numpy.longdouble from the closed forms below on top of kernel_family_ref.k_ref / dk_dtheta_ref, with its own
Cholesky factorisation and inverse (numpy.linalg has none for longdouble).

With KV = K(theta) + V, Q = KV^-1, q_i = Q_ii, r = y - m and alpha = Q r (Rasmussen & Williams 5.4.2):

    r_i - mu_i = alpha_i / q_i        sigma^2_i = 1 / q_i        L = sum_i (log q_i - alpha_i^2 / q_i) / 2 - n / 2 log 2 pi

(mu_i: the prediction of r_i from the other n - 1 points; sigma^2_i the variance of the noisy observation) and, with w = alpha / q,
c_i = (1 + alpha_i^2 / q_i) / (2 q_i), u = Q w and M = Q diag(c) Q,

    dL/dtheta_j = u^T dKV_j alpha - sum_kl M_kl (dKV_j)_kl          dL/dm-parameter = u^T dm

`loo_brute` computes the same quantities the long way: n factorisations of the (n - 1)-point problems."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import kernel_family_ref as kf

LD = np.longdouble
LOG_2PI = np.log(LD(2) * np.arccos(LD(-1)))


def cholesky(A):
    """lower Cholesky factor of a symmetric positive definite matrix, in the precision of A"""
    A = np.array(A)
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"not positive definite at column {j}")
        L[j:, j] = v / np.sqrt(v[0])
    return L


def matmul(A, B, lower_a=False):
    """A @ B in the precision of the operands.  numpy has no BLAS for longdouble: its product is a plain loop that wants contiguous
    operands, so the rows of A are dealt to a few threads (the loop releases the interpreter lock); the result does not depend on the
    split, every entry is the same sum in the same order.  lower_a: A is the transpose of a lower triangular matrix (zero left of
    its diagonal), the products with those zeros are skipped."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    n = A.shape[0]
    if n < 256:
        return A @ B
    out = np.empty((n, B.shape[1]), dtype=A.dtype)
    cuts = np.linspace(0, n, 33).astype(int)

    def rows(k):
        a, b = cuts[k], cuts[k + 1]
        out[a:b] = np.ascontiguousarray(A[a:b, a:]) @ B[a:] if lower_a else A[a:b] @ B
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(rows, range(32)))
    return out


def tri_inverse(L):
    """inverse of a lower triangular matrix by forward substitution: the columns are independent, so blocks of them are dealt to a
    few threads (every entry is the same sum in the same order whatever the split)"""
    n = len(L)
    X = np.zeros_like(L)
    nb = max(1, min(32, n // 32))
    cuts = np.linspace(0, n, nb + 1).astype(int)

    def cols(k):
        a, b = cuts[k], cuts[k + 1]
        for i in range(a, n):
            rhs = -(L[i, a:i] @ X[a:i, a:b])
            if i < b:
                rhs[i - a] += 1
            X[i, a:b] = rhs / L[i, i]
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(cols, range(nb)))
    return X


def spd_inverse(A):
    X = tri_inverse(cholesky(A))
    return matmul(X.T, X, lower_a=True)


def solve_spd(A, b):
    L = cholesky(A)
    n = len(A)
    z = np.zeros(n, dtype=A.dtype)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    xs = np.zeros(n, dtype=A.dtype)
    for i in range(n - 1, -1, -1):
        xs[i] = (z[i] - L[i + 1:, i] @ xs[i + 1:]) / L[i, i]
    return xs, L


def _kv(name, x, V, theta, dtype):
    K = kf.k_ref(name, x, x, theta[:kf.n_theta(name, x.shape[1])], dtype)
    V = np.asarray(V, dtype=dtype)
    return K + (np.diag(V) if V.ndim == 1 else V)


def loo_closed(name, x, y_minus_m, V, theta, dtype=LD, want_grad=True):
    """(value, m_loo, v_loo, gradient, u, diag M): the LOO log predictive probability, the n LOO predictions of y - m and their
    variances (noisy observation), dL/dtheta for the hyperparameters the kernel owns, and the two vectors a caller needs for noise
    and mean hyperparameters.  V: the noise variances (n,) or a noise covariance (n, n).  dtype=np.float64: the same formulas in double."""
    x = np.asarray(x, dtype=dtype)
    r = np.asarray(y_minus_m, dtype=dtype).reshape(-1)
    theta = np.asarray(theta, dtype=dtype)
    n = len(x)
    Q = spd_inverse(_kv(name, x, V, theta, dtype))
    q = np.diag(Q).copy()
    alpha = Q @ r
    value = np.sum(np.log(q) - alpha ** 2 / q) / 2 - dtype(n) / 2 * LOG_2PI.astype(dtype)
    m_loo = r - alpha / q
    v_loo = 1 / q
    if not want_grad:
        return value, m_loo, v_loo, None, None, None
    w = alpha / q
    c = (1 + alpha ** 2 / q) / (2 * q)
    u = Q @ w
    M = matmul(Q * c, Q)
    dK = kf.dk_dtheta_ref(name, x, x, theta[:kf.n_theta(name, x.shape[1])], dtype)
    B = np.outer(u, alpha) - M
    grad = np.array([np.sum(B * dK[j]) for j in range(len(dK))], dtype=dtype)
    return value, m_loo, v_loo, grad, u, np.diag(M).copy()


def loo_brute(name, x, y_minus_m, V, theta, dtype=LD):
    """(value, m_loo, v_loo) from n refits on n - 1 points each: the posterior of point i given the others, noise of point i added"""
    x = np.asarray(x, dtype=dtype)
    r = np.asarray(y_minus_m, dtype=dtype).reshape(-1)
    theta = np.asarray(theta, dtype=dtype)
    n = len(x)
    KV = _kv(name, x, V, theta, dtype)
    m = np.zeros(n, dtype=dtype)
    v = np.zeros(n, dtype=dtype)
    for i in range(n):
        keep = np.arange(n) != i
        A = KV[np.ix_(keep, keep)]
        k = KV[keep, i]
        s, L = solve_spd(A, k)
        m[i] = s @ r[keep]
        v[i] = KV[i, i] - k @ s
    value = np.sum(-np.log(v) / 2 - (r - m) ** 2 / (2 * v)) - dtype(n) / 2 * LOG_2PI.astype(dtype)
    return value, m, v
