"""A numpy twin of the Fisher information of the nearest-neighbour likelihood (a helper module of the tests, not a conftest): the per-row
terms of include/fvgp_hip_nn.h (fvgp_hip_nn_loglik_fisher) in a chosen number type, built on vecchia_grad_ref and kernel_family_ref, and
the cases the host and the device tests share.

    fisher_rows_ref   per row i with the neighbour list c: Sigma = K over (c, i), A = Sigma[c, c] + diag(v_c) = L L^T, a = A^-1 Sigma[c, i],
                      d = Sigma[i, i] + v_i - Sigma[c, i]^T a, b = (-a, 1), and per hyperparameter h
                          t_h = (dSigma_h b) on c,   delta_h = b^T dSigma_h b,   u_h = L^-1 t_h,
                          F_i[h][k] = u_h^T u_k / d + 1/2 delta_h delta_k / d^2
    direct_rows_ld    the same term as the trace difference F(Sigma_ci + noise) - F(A), F(S)[h][k] = 1/2 tr(S^-1 d_h S S^-1 d_k S), longdouble
    dense_fisher_ld   the exact GP's 1/2 tr((K + V)^-1 d_h K (K + V)^-1 d_k K), longdouble
    objective_f64     (f, g, F) of the negative log-likelihood in float64, the rows batched: what the optimiser's host test minimises
                      (tests/test_vecchia_fisher_host.py holds it to fisher_rows_ref and vecchia_grad_ref.scores_ref)

THE BARS of tests/test_gpu_vecchia_fisher.py.  Every F_i is positive semidefinite, so neither scale below can cancel:
    rows  = max over (h, k) of max_i |F_i,hk - ref_i,hk| / max_i sqrt(ref_i,hh ref_i,kk)
    total = max over (h, k) of |F_hk - ref_hk| / sqrt(ref_hh ref_kk),       F = sum_i F_i
base = the larger of two float64 twin runs against the longdouble run on the same inputs: one plain, one with every kernel entry
perturbed by up to kernel_family_ref.k_bound_ulps(d) ulps of sigma^2 and every derivative entry by a relative error of up to (16 + d) eps
(as in vecchia_grad_ref).  The device must stay within MARGIN * max(base, FLOOR[figure]), MARGIN = vecchia_ref.MARGIN; FLOOR is the median
of the bases over CASES, computed and asserted by tests/test_vecchia_fisher_host.py::test_floor_is_the_median_of_the_bases and recorded
here.  Nothing here comes from the device."""
import functools

import numpy as np

import kernel_family_ref as kf
import vecchia_grad_ref as vg
import vecchia_ref as vr

LD = vr.LD
EPS = kf.EPS
MARGIN = vr.MARGIN
FIGURES = ("rows", "total")
# the medians of the bases over CASES (test_vecchia_fisher_host.py asserts these are what bases() gives, to 1 %)
FLOOR = {"rows": 2.00e-13, "total": 2.05e-14}


def _forward(L, T):
    """L^-1 T, T a matrix of columns"""
    y = np.array(T, dtype=L.dtype)
    for i in range(len(L)):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def _blocks(name, x, theta, dtype):
    """K (n, n) and dK / dtheta (H, n, n) over all of x in dtype: a row's Sigma and dSigma are gathered from them"""
    return kf.k_ref(name, x, x, theta, dtype), kf.dk_dtheta_ref(name, x, x, theta, dtype)


def _row_blocks(K, dK, c, i, theta, dtype, perturb):
    p = np.concatenate([c, [i]]).astype(np.int64)
    S, dS = K[np.ix_(p, p)], dK[:, p[:, None], p[None, :]]
    if perturb is not None:
        rng, ulps, rel = perturb
        E = np.tril(rng.uniform(-1.0, 1.0, S.shape))
        S = S + (ulps * EPS * float(theta[0]) * (E + np.tril(E, -1).T)).astype(dtype)
        F = np.tril(rng.uniform(-1.0, 1.0, dS.shape))
        dS = dS * (dtype(1) + (rel * (F + np.transpose(np.tril(F, -1), (0, 2, 1)))).astype(dtype))
    return S, dS


def fisher_rows_ref(name, x, theta, idx, v, dtype=LD, perturb=None):
    """(n, H, H) in dtype: row i is the term F_i of the Fisher information for the neighbour lists idx (entries outside 0 .. n - 1
    skipped).  perturb = (rng, ulps, rel) as in vecchia_grad_ref.scores_ref."""
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    v = np.asarray(v, dtype=dtype)
    n, H = len(x), len(theta)
    K, dK = _blocks(name, x, theta, dtype)
    out = np.zeros((n, H, H), dtype=dtype)
    half = dtype(1) / dtype(2)
    for i in range(n):
        c = np.array([j for j in idx[i] if 0 <= j < n], dtype=np.int64)
        m = len(c)
        S, dS = _row_blocks(K, dK, c, i, theta, dtype, perturb)
        dv = S[m, m] + v[i]
        b = np.zeros(m + 1, dtype=dtype)
        b[m] = dtype(1)
        U = np.zeros((0, H), dtype=dtype)
        if m:
            L = vg._chol(S[:m, :m] + np.diag(v[c]), dtype)
            a = vg._solve(L, S[:m, m])
            b[:m] = -a
            dv = dv - np.dot(S[:m, m], a)
            U = _forward(L, (dS[:, :m, :] @ b).T)                  # (m, H): column h is u_h
        delta = np.einsum("p,hpq,q->h", b, dS, b)
        out[i] = U.T @ U / dv + half * np.outer(delta, delta) / (dv * dv)
    return out


def _trace_form(S, dS):
    """F(S)[h][k] = 1/2 tr(S^-1 d_h S S^-1 d_k S) by a longdouble Cholesky"""
    L = vg._chol(S, LD)
    W = np.array([vg._solve(L, d) for d in dS])                    # S^-1 d_h S
    return np.einsum("hpq,kqp->hk", W, W) / LD(2)


def direct_rows_ld(name, x, theta, idx, v):
    """(n, H, H) longdouble: F(Sigma_ci + noise) - F(A) per row, the definition the row form collapses"""
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    v = np.asarray(v, dtype=LD)
    n, H = len(x), len(theta)
    K, dK = _blocks(name, x, theta, LD)
    out = np.zeros((n, H, H), dtype=LD)
    for i in range(n):
        c = np.array([j for j in idx[i] if 0 <= j < n], dtype=np.int64)
        m = len(c)
        S, dS = _row_blocks(K, dK, c, i, theta, LD, None)
        S = S + np.diag(np.concatenate([v[c], v[i:i + 1]]))
        out[i] = _trace_form(S, dS)
        if m:
            out[i] -= _trace_form(S[:m, :m], dS[:, :m, :m])
    return out


def dense_fisher_ld(name, x, theta, v):
    """(H, H) longdouble: the exact GP's Fisher information 1/2 tr((K + V)^-1 d_h K (K + V)^-1 d_k K)"""
    K, dK = _blocks(name, np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64), LD)
    return _trace_form(K + np.diag(np.asarray(v, dtype=LD)), dK)


def objective_f64(name, x, theta, idx, r, v):
    """(f, g (H,), F (H, H)) in float64: the negative nearest-neighbour log-likelihood, its gradient and the Fisher information, the rows
    with equally long lists batched through numpy's stacked solves; f = +inf (g, F NaN) where a block is not positive definite"""
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    r, v = np.asarray(r, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n, H = len(x), len(theta)
    K, dK = _blocks(name, x, theta, np.float64)
    idx = np.asarray(idx)
    counts = np.sum((idx >= 0) & (idx < n), axis=1)
    f, g, F = 0.5 * n * np.log(2.0 * np.pi), np.zeros(H), np.zeros((H, H))
    for m in np.unique(counts):
        rows = np.nonzero(counts == m)[0]
        c = np.array([[j for j in idx[i] if 0 <= j < n] for i in rows], dtype=np.int64).reshape(len(rows), m)
        p = np.concatenate([c, rows[:, None]], axis=1)
        S = K[p[:, :, None], p[:, None, :]]                        # (rows, m + 1, m + 1)
        dS = dK[:, p[:, :, None], p[:, None, :]]                   # (H, rows, m + 1, m + 1)
        b, gg = np.zeros((len(rows), m + 1)), np.zeros((len(rows), m + 1))
        b[:, m] = 1.0
        dv, e = S[:, m, m] + v[rows], r[rows].copy()
        UU = np.zeros((len(rows), H, H))
        if m:
            A = S[:, :m, :m] + np.eye(m) * v[c][:, None, :]
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                return np.inf, np.full(H, np.nan), np.full((H, H), np.nan)
            sol = np.linalg.solve(A, np.stack([S[:, :m, m], r[c]], axis=2))
            b[:, :m], gg[:, :m] = -sol[:, :, 0], sol[:, :, 1]
            dv = dv - np.einsum("rp,rp->r", S[:, :m, m], sol[:, :, 0])
            e = e - np.einsum("rp,rp->r", S[:, :m, m], sol[:, :, 1])
            T = np.einsum("hrpq,rq->rph", dS[:, :, :m, :], b)      # (rows, m, H)
            U = np.linalg.solve(L, T)
            UU = np.einsum("rph,rpk->rhk", U, U)
        if not np.all(dv > 0.0):
            return np.inf, np.full(H, np.nan), np.full((H, H), np.nan)
        q = (e / dv)[:, None] * gg + (0.5 * (e * e / (dv * dv) - 1.0 / dv))[:, None] * b
        f += 0.5 * float(np.sum(e * e / dv + np.log(dv)))
        g -= np.einsum("rp,hrpq,rq->h", b, dS, q)
        delta = np.einsum("rp,hrpq,rq->rh", b, dS, b)
        F += np.sum(UU / dv[:, None, None] + 0.5 * delta[:, :, None] * delta[:, None, :] / (dv * dv)[:, None, None], axis=0)
    return float(f), g, F


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# (kernel, d, n, m, B): the shapes of vecchia_grad_ref.GRAD_CASES with every kernel id, d over kernel_family_ref.DIMS (5: the first
# runtime-dimension instantiation, 16: the widest), m on both sides of each padded size, n in 70 .. 300 (row 0 has no neighbours, the rows
# i < m short lists, the row count is no multiple of the waves per workgroup; n = 70 keeps a longdouble reference at m >= 63 to seconds),
# B in {1, 3}, and one case of 300 rows with m = 2: its sums cross a 256-row slice
CASES = (
    ("rbf_ard", 1, 70, 1, 1), ("matern32_ard", 2, 70, 15, 3), ("matern52_ard", 3, 70, 16, 1), ("rbf_iso", 4, 70, 17, 1),
    ("matern32_iso", 5, 70, 32, 1), ("matern52_iso", 16, 70, 32, 3), ("rbf_ard", 16, 70, 33, 1), ("matern32_ard", 3, 70, 63, 1),
    ("matern52_ard", 5, 70, 64, 1), ("rbf_iso", 2, 70, 64, 3), ("matern52_ard", 2, 300, 2, 1),
)
SLICE_CASE = CASES[-1]
EXACT_CASE = vr.EXACT_CASE


def packed_to_full(rows, H):
    """(.., H (H + 1) / 2) packed lower triangles ((h, k <= h) at h (h + 1) / 2 + k) -> (.., H, H) symmetric"""
    rows = np.asarray(rows)
    out = np.zeros(rows.shape[:-1] + (H, H), dtype=rows.dtype)
    for h in range(H):
        for k in range(h + 1):
            out[..., h, k] = out[..., k, h] = rows[..., h * (h + 1) // 2 + k]
    return out


def figures(got, ref):
    """the two figures of the (n, H, H) rows `got` (their sum, or got = (rows, total) with the total given) against the longdouble rows
    `ref`; a hyperparameter whose reference diagonal is 0 everywhere (no row has a neighbour) is held absolutely"""
    rows, total = got if isinstance(got, tuple) else (got, None)
    rows = np.asarray(rows, dtype=LD)
    total = np.sum(rows, axis=0) if total is None else np.asarray(total, dtype=LD)
    diag = np.sqrt(np.einsum("ihh->ih", ref))                      # (n, H)
    rscale = np.max(diag[:, :, None] * diag[:, None, :], axis=0)
    tsum = np.sum(ref, axis=0)
    tdiag = np.sqrt(np.diagonal(tsum))
    tscale = np.outer(tdiag, tdiag)
    rscale, tscale = np.where(rscale == 0, LD(1), rscale), np.where(tscale == 0, LD(1), tscale)
    return {"rows": float(np.max(np.max(np.abs(rows - ref), axis=0) / rscale)), "total": float(np.max(np.abs(total - tsum) / tscale))}


@functools.lru_cache(maxsize=None)
def reference(case):
    """per b the longdouble (n, H, H) rows of a case: computed once, shared, never changed"""
    x, thetas, r, v, idx = vr.case_inputs(case)
    return tuple(fisher_rows_ref(case[0], x, t, idx, v, LD) for t in thetas)


@functools.lru_cache(maxsize=None)
def bases(case):
    """{figure: base}: over the case's thetas, the larger of the plain and the perturbed float64 twin's figures against longdouble"""
    name, d = case[0], case[1]
    x, thetas, r, v, idx = vr.case_inputs(case)
    out = dict.fromkeys(FIGURES, 0.0)
    for b, t in enumerate(thetas):
        ref = reference(case)[b]
        rng = np.random.default_rng(6161 + b)
        for run in (fisher_rows_ref(name, x, t, idx, v, np.float64),
                    fisher_rows_ref(name, x, t, idx, v, np.float64, perturb=(rng, kf.k_bound_ulps(d), (16 + d) * EPS))):
            f = figures(run, ref)
            out = {k: max(out[k], f[k]) for k in FIGURES}
    return out


def bars(case):
    """{figure: MARGIN * max(base, FLOOR)}: what the device may differ from longdouble by"""
    b = bases(case)
    return {k: MARGIN * max(b[k], FLOOR[k]) for k in FIGURES}
