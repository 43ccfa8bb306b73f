"""The numpy twin of the stochastic log-likelihood on the matrix-free path (csrc/matrix_free.hip; a helper module like
matrix_free_ref.py, not a conftest).

    probe_map, probes_ref   Z = D^1/2 eps + G^T eta from samples_ref.normal_block: eps = z(seed, 2 stream, i, col), eta = z(seed, 2 stream + 1, t, col)
    pcg_lanczos_ref   matrix_free_ref.pcg_ref's recurrence, column by column, that also records rho_0 and the alpha and beta of the FIRST
                      recurrence (before any restart) below index L
    lanczos_T         T[k, k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1}, T[k, k+1] = sqrt(beta_k) / alpha_k
    quadrature        rho_0 e_1^T log(T_m) e_1 by numpy.linalg.eigh on the dense T (scipy's eigh_tridiagonal did not converge on an 84-step T)
    logdet_precond    log det(G^T G + D) = sum log v + 2 sum log diag chol(I + G D^-1 G^T)
    kgrad_form_ref    sum_c U[:, c]^T (dK / dtheta_j) W[:, c] in longdouble from kernel_family_ref.dk_dtheta_ref, with |U|^T |dK_j| |W|
    estimate_ref      the assembled estimate: the keys of MatrixFreeGP.log_likelihood_estimate

tests/test_mf_likelihood_host.py proves the twin against dense linear algebra; tests/test_gpu_mf_likelihood.py holds the device to it."""
import functools

import numpy as np

import kernel_family_ref as kf
import matrix_free_ref as mf
import samples_ref

LD = np.longdouble
EPS = kf.EPS
PROBES = 16
SEED = 7                      # the seed of the fixture estimates, here and on the device
PROBE_TOL = 1e-6
STEPS = 64
GROUP = 4                     # probes per fvgp_hip_kgrad_form call of the trace (the spread of the group means is the standard error)
ESTIMATE_FIXTURES = (mf.FIXTURES[1], mf.FIXTURES[3], mf.FIXTURES[5])


def probe_map(eps, eta, G, v):
    """D^1/2 eps + G^T eta: the linear map [D^1/2, G^T] of the stacked normals (eps (n, c), eta (q, c)); G None or of no rows: D^1/2 eps"""
    Z = np.sqrt(v)[:, None] * eps
    if G is not None and len(G):
        Z = Z + G.T @ eta
    return Z


def probes_ref(seed, stream, col0, cols, G, v):
    """(n, cols) probes with covariance G^T G + diag(v): eps from the stream 2 stream, eta from 2 stream + 1, columns col0 .."""
    n, q = len(v), 0 if G is None else len(G)
    eps = samples_ref.normal_block(seed, 2 * stream, 0, col0, n, cols)
    eta = samples_ref.normal_block(seed, 2 * stream + 1, 0, col0, q, cols) if q else None
    return probe_map(eps, eta, G, v)


def pcg_lanczos_ref(A, b, v, G, tol, L, max_iter=1000, max_restarts=3):
    """one column by the device's rules (matrix_free_ref.pcg_ref, cold start) with the records of fvgp_hip_pcg_lanczos:
    (x, iters, true relative residual, status, alpha (steps,), beta (<= steps,), rho0).  alpha_k is recorded at iteration k < L of the
    first recurrence, beta_k when that recurrence goes on after iteration k."""
    n = len(b)
    M = lambda r: mf.woodbury_apply(G, v, r)                                      # noqa: E731
    bn = np.sqrt(b @ b)
    x = np.zeros(n)
    alphas, betas, rho0 = [], [], 0.0
    if bn == 0.0:
        return x, 0, 0.0, 0, np.array(alphas), np.array(betas), rho0
    r = b.copy()
    iters, restarts, code, first = 0, 0, 0, True
    active = np.sqrt(r @ r) > tol * bn
    while True:
        if active:
            z = M(r)
            rho = r @ z
            p = z.copy()
            if not rho > 0.0 or np.isinf(rho):
                active, code = False, 2
            elif first:
                rho0 = rho
        while active:
            Ap = A @ p
            pap = p @ Ap
            if not pap > 0.0 or np.isinf(pap):
                active, code = False, 2
                break
            alpha = rho / pap
            if first and iters < L:
                alphas.append(alpha)
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
            beta = rho_new / rho
            if first and iters <= L:
                betas.append(beta)
            p = z + beta * p
            rho = rho_new
        r = b - A @ x
        relres = np.sqrt(r @ r) / bn
        status = 0 if relres <= tol else 2 if code == 2 else 1 if (code == 1 or restarts >= max_restarts) else None
        if status is not None:
            return x, iters, relres, status, np.array(alphas), np.array(betas), rho0
        restarts += 1
        first = False
        active = True


def lanczos_T(alpha, beta, m=None):
    """the m x m Lanczos tridiagonal of M^-1/2 A M^-1/2 from the first m CG coefficients (m = len(alpha) when None)"""
    m = len(alpha) if m is None else m
    T = np.zeros((m, m))
    for k in range(m):
        T[k, k] = 1.0 / alpha[k] + (beta[k - 1] / alpha[k - 1] if k else 0.0)
        if k + 1 < m:
            T[k, k + 1] = T[k + 1, k] = np.sqrt(beta[k]) / alpha[k]
    return T


def quadrature(alpha, beta, rho0, m=None):
    """rho_0 e_1^T log(T_m) e_1 = rho_0 sum_i tau_i^2 log lambda_i: the probe's estimate of zhat^T log(Ahat) zhat; 0 for no steps"""
    m = len(alpha) if m is None else m
    if m == 0:
        return 0.0
    lam, Q = np.linalg.eigh(lanczos_T(alpha, beta, m))
    return float(rho0 * np.sum(Q[0] ** 2 * np.log(lam)))


def logdet_precond(G, v):
    """log det(G^T G + diag(v)) through the q x q matrix the device factors"""
    out = float(np.sum(np.log(v)))
    if G is not None and len(G):
        C = np.eye(len(G)) + (G / v) @ G.T
        out += 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(C)))))
    return out


def kgrad_form_ref(kernel, x1, U, x2, W, theta):
    """(out (H,), mag (H,)) in longdouble: out[j] = sum_c U[:, c]^T dK_j W[:, c] and mag[j] = sum_c |U[:, c]|^T |dK_j| |W[:, c]|"""
    dK = kf.dk_dtheta_ref(kernel, x1, x2, theta)
    U, W = np.asarray(U, dtype=LD), np.asarray(W, dtype=LD)
    out = np.array([np.sum(U * (dK[j] @ W)) for j in range(len(dK))], dtype=LD)
    mag = np.array([np.sum(np.abs(U) * (np.abs(dK[j]) @ np.abs(W))) for j in range(len(dK))], dtype=LD)
    return out, mag


def kgrad_entry_ulps(d):
    """allowed |dK_j device - dK_j exact| per entry in units of eps |dK_j| scale: kernel_family_ref.grad_trace_bound_factor's per-term part,
    32 + 2 d (a few ulp each for exp and sqrt, (d + 2) for the rounding of r^2 in the argument, d for the e_k^2)"""
    return 32 + 2 * d


def kgrad_form_bound(kernel, x1, U, x2, W, theta, mag):
    """the componentwise bound of the form, in the manner of matrix_free_ref.kmatvec_bound: the entry error of dK_j, (32 + 2 d) eps
    max |dK_j|, times sum_c sum_i |U_ic| sum_k |W_kc|, plus Higham's gamma of n2 + s + 4 terms (the s products of t, the n2 rows of a lane's
    sum, 4 for the entry's own products) on sum_c |U_c|^T |dK_j| |W_c|"""
    dK = kf.dk_dtheta_ref(kernel, x1, x2, theta)
    n2, s, d = len(x2), np.shape(U)[1], np.shape(x1)[1]
    au, aw = np.abs(np.asarray(U, dtype=LD)).sum(axis=0), np.abs(np.asarray(W, dtype=LD)).sum(axis=0)
    entry = np.array([kgrad_entry_ulps(d) * EPS * np.max(np.abs(dK[j])) * np.sum(au * aw) for j in range(len(dK))], dtype=LD)
    return entry + (n2 + s + 4) * (EPS / 2) * mag


def dk_double(kernel, x, theta):
    return np.asarray(kf.dk_dtheta_ref(kernel, x, x, theta), dtype=np.float64)


def estimate_ref(kernel, x, y, v, theta, rank, n_probes=PROBES, seed=SEED, gradient=False, tol=1e-10, probe_tol=PROBE_TOL, steps=STEPS,
                 K=None, G=None):
    """the estimate of MatrixFreeGP.log_likelihood_estimate on the host, the same keys; K (double) and G (rank, n) may be handed in"""
    n = len(y)
    K = mf.k_double(kernel, x, theta) if K is None else K
    A = K + np.diag(v)
    if G is None and rank:
        G = mf.pchol_ref(K, min(rank, n), tol=1e-12, sigma2=float(theta[0]))[0]
    ym = y - np.mean(y)
    alpha, it_a, _, st_a = mf.pcg_ref(A, ym, v, G, tol)
    Z = probes_ref(seed, 0, 0, n_probes, G, v)
    U, quad, its, steps_used, ok = np.empty_like(Z), np.empty(n_probes), [], [], st_a == 0
    for c in range(n_probes):
        u, it, _, st, al, be, rho0 = pcg_lanczos_ref(A, Z[:, c], v, G, probe_tol, steps)
        U[:, c], quad[c] = u, quadrature(al, be, rho0)
        its.append(it)
        steps_used.append(len(al))
        ok = ok and st == 0
    ldm = logdet_precond(G, v)
    logdet = ldm + float(np.mean(quad))
    ld_se = float(np.std(quad, ddof=1) / np.sqrt(n_probes)) if n_probes > 1 else float("nan")
    fit = 0.5 * float(ym @ alpha)
    out = {"log_likelihood": -(fit + 0.5 * logdet + 0.5 * n * np.log(2.0 * np.pi)), "std_error": 0.5 * ld_se, "logdet": logdet,
           "logdet_std_error": ld_se, "logdet_preconditioner": ldm, "data_fit": fit, "per_probe": quad,
           "iterations": np.array(its), "lanczos_steps": np.array(steps_used), "alpha_iterations": it_a, "converged": bool(ok)}
    if gradient:
        dK = dk_double(kernel, x, theta)
        Wm = mf.woodbury_apply(G, v, Z)
        a_term = np.array([alpha @ dK[j] @ alpha for j in range(len(dK))])
        sums, means = np.zeros(len(dK)), []
        for g0 in range(0, n_probes, GROUP):
            g1 = min(g0 + GROUP, n_probes)
            f = np.array([np.sum(U[:, g0:g1] * (dK[j] @ Wm[:, g0:g1])) for j in range(len(dK))])
            sums += f
            means.append(f / (g1 - g0))
        trace = sums / n_probes
        tr_se = np.std(np.array(means), axis=0, ddof=1) / np.sqrt(len(means)) if len(means) > 1 else np.full(len(dK), np.nan)
        out.update({"neg_gradient": -0.5 * a_term + 0.5 * trace, "neg_gradient_std_error": 0.5 * tr_se, "trace": trace,
                    "trace_std_error": tr_se, "alpha": alpha, "U": U, "W": Wm, "Z": Z})
    return out


def fixture_y(fx):
    """the fixture's observations: column 0 of its right-hand sides"""
    return np.array(mf.fixture(fx)["rhs"][:, 0])


@functools.lru_cache(maxsize=None)
def fixture_estimate(fx, rank=mf.RANK, seed=SEED):
    """the twin's estimate with gradient on a fixture of matrix_free_ref, computed once and shared (read-only)"""
    f = mf.fixture(fx)
    G = mf.pchol_ref(f["K"], rank, tol=1e-12, sigma2=mf.SIGMA2)[0] if rank else None
    return estimate_ref(f["kernel"], f["x"], fixture_y(fx), f["V"], f["theta"], rank, seed=seed, gradient=True, K=np.array(f["K"]), G=G)


@functools.lru_cache(maxsize=None)
def fixture_dense(fx):
    """(slogdet(A), the dense traces tr(A^-1 dK_j)) of a fixture"""
    f = mf.fixture(fx)
    Ainv = np.linalg.inv(f["A"])
    dK = dk_double(f["kernel"], f["x"], f["theta"])
    return float(np.linalg.slogdet(f["A"])[1]), np.array([np.sum(Ainv * dK[j]) for j in range(len(dK))])
