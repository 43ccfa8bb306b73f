"""A numpy twin of the nearest-neighbour preconditioner (include/fvgp_hip_nn.h: fvgp_hip_nn_factor, fvgp_hip_nn_precond_apply,
fvgp_hip_pcg_nn) and the cases its host and device tests share (a helper module of the tests, not a conftest).

    factor_ref        per row i of the ordered data with the list c = idx[i] (entries outside 0 .. n - 1 skipped):  A = K_cc + diag(v_c),
                      k = K_ci, a column-by-column Cholesky in the number type, w = L^-1 k, a = L^-T w, d = K_ii + v_i - w^T w,
                      dinv = 1 / sqrt(d), coef[l] = -a_l dinv at the list's valid positions and 0 elsewhere.  longdouble is the reference,
                      float64 the twin whose own error against it -- plain, and with every kernel entry perturbed by the device assembly's
                      documented entry bound, as vecchia_ref does -- sets the device's bars
    dense_w           the factor as a dense lower-triangular matrix W: (K + V)^-1 ~ W^T W, exactly with m >= n - 1
    transpose_ref     the transposed lists by plain loops: bucket j holds the flat positions i ld + l with idx[i][l] == j in ascending i
    apply_ref         Z = W^T (W R) in longdouble and the magnitude sum |W^T| (|W| |R|) its error bound scales with
    apply_bound       Higham's gamma of m + in-degree + 2 terms on that magnitude sum (the kind of matrix_free_ref.kmatvec_bound)
    pcg_nn_ref        matrix_free_ref.pcg_ref -- the device's recurrence -- with z = W^T (W r) in the preconditioner's place

Nothing here comes from the device."""
import functools

import numpy as np

import kernel_family_ref as kf
import matrix_free_ref as mf
import vecchia_ref as vr

LD = np.longdouble
EPS = kf.EPS
MARGIN = vr.MARGIN
# the floors of the factor's two figures: vecchia_ref's own, "d" for dinv (a relative figure of the conditional variance's kind) and "mu"
# for coef (an absolute figure on a scale of order one: coef sqrt(d) = -a, the weights of the conditional mean)
FLOOR = {"coef": vr.FLOOR["mu"], "dinv": vr.FLOOR["d"]}
FIGURES = ("coef", "dinv")
# the two larger fixtures of the issue's table (matrix_free_ref's format): the data outgrow rank 128 and the nearest-neighbour count stays flat
BIG_FIXTURES = (("matern32_ard", 2, 0.1, 1e-2, 2000, 22), ("matern52_ard", 3, 0.15, 1e-2, 2000, 23))
NEIGHBORS = 32


# ---- the factor ------------------------------------------------------------------------------------------------------------------------
def factor_ref(K, v, idx, dtype=LD, perturb=None, sigma2=None):
    """(coef (n, m), dinv (n)) in dtype from the full kernel matrix K (n, n) of the ordered data, the noise v and the lists idx (n, m).
    perturb = (rng, ulps): every kernel entry a row uses gets a uniform error in +-ulps eps sigma^2 (its block symmetrically)."""
    n, m = idx.shape
    K, v = np.asarray(K, dtype=dtype), np.asarray(v, dtype=dtype)
    coef, dinv = np.zeros((n, m), dtype=dtype), np.zeros(n, dtype=dtype)
    amp = 0.0 if perturb is None else perturb[1] * EPS * float(sigma2)
    for i in range(n):
        at = np.array([l for l in range(m) if 0 <= idx[i, l] < n], dtype=np.int64)
        c = idx[i, at].astype(np.int64)
        kxx = K[i, i]
        if perturb is not None:
            kxx = kxx + dtype(amp * perturb[0].uniform(-1.0, 1.0))
        kxx = kxx + v[i]
        if len(c) == 0:
            dinv[i] = dtype(1) / np.sqrt(kxx)
            continue
        A, k = K[np.ix_(c, c)].copy(), K[c, i].copy()
        if perturb is not None:
            E = np.tril(perturb[0].uniform(-1.0, 1.0, A.shape))
            A = A + (amp * (E + np.tril(E, -1).T)).astype(dtype)
            k = k + (amp * perturb[0].uniform(-1.0, 1.0, k.shape)).astype(dtype)
        A = A + np.diag(v[c])
        mm = len(c)
        L = np.zeros((mm, mm), dtype=dtype)
        for j in range(mm):
            col = A[j:, j] - L[j:, :j] @ L[j, :j]
            L[j, j] = np.sqrt(col[0])
            L[j + 1:, j] = col[1:] / L[j, j]
        w = np.zeros(mm, dtype=dtype)
        for j in range(mm):
            w[j] = (k[j] - L[j, :j] @ w[:j]) / L[j, j]
        a = w.copy()
        for j in range(mm - 1, -1, -1):                     # L^T a = w, outer-product form as the device's backward pass
            a[j] = a[j] / L[j, j]
            a[:j] = a[:j] - L[j, :j] * a[j]
        dinv[i] = dtype(1) / np.sqrt(kxx - np.dot(w, w))
        coef[i, at] = -(a * dinv[i])
    return coef, dinv


def dense_w(idx, coef, dinv, dtype=np.float64):
    """W (n, n) lower triangular: row i holds coef[i][l] at column idx[i][l] and dinv[i] on the diagonal"""
    n, m = idx.shape
    W = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        for l in range(m):
            if 0 <= idx[i, l] < n:
                W[i, idx[i, l]] += coef[i, l]
        W[i, i] += dinv[i]
    return W


# ---- the transposed lists ----------------------------------------------------------------------------------------------------------------
def transpose_ref(idx, n, ld=None):
    """(tr_start (n + 1,), tr_pos (nnz,)) int64 by plain loops over the rows in ascending order; ld: the leading dimension the positions
    are counted in (default: idx's columns)"""
    rows, m = idx.shape
    ld = m if ld is None else ld
    buckets = [[] for _ in range(n)]
    for i in range(rows):
        for l in range(m):
            j = int(idx[i, l])
            if 0 <= j < n:
                buckets[j].append(i * ld + l)
    start = np.zeros(n + 1, dtype=np.int64)
    start[1:] = np.cumsum([len(b) for b in buckets])
    return start, np.array([p for b in buckets for p in b], dtype=np.int64)


def check_transposed(idx, n, start, pos, ld=None):
    """the properties of transposed lists (the twin's or the binding's): a permutation of the valid entries' positions, every bucket's
    entries point at its column, ascending inside the bucket"""
    rows, m = idx.shape
    ld = m if ld is None else ld
    valid = [(i * ld + l) for i in range(rows) for l in range(m) if 0 <= idx[i, l] < n]
    assert start.shape == (n + 1,) and start[0] == 0 and start[n] == len(pos) == len(valid) and np.all(np.diff(start) >= 0)
    assert sorted(pos.tolist()) == valid
    for j in range(n):
        b = pos[start[j]:start[j + 1]]
        assert np.all(idx[b // ld, b % ld] == j) and np.all(np.diff(b) > 0), j


def coincident_set(n=300, d=2, copies=40, seed=5):
    """x (n, d) from the unit cube whose rows 0 .. copies - 1 are ONE point: with more than m of them every later copy lists the first m,
    and in the given order the nearest-neighbour lists send one bucket far past the others"""
    x = np.random.default_rng(seed).random((n, d))
    x[:copies] = x[0]
    return x


def junk_lists(n, m, seed=3):
    """int32 (n, m): random earlier rows with -1, n, n + 7 and both ends of int32 scattered among them"""
    rng = np.random.default_rng(seed)
    idx = np.full((n, m), -1, dtype=np.int64)
    for i in range(n):
        k = min(i, m)
        idx[i, :k] = rng.choice(i, size=k, replace=False) if k else []
    junk = np.array([-1, -5, n, n + 7, 2 ** 31 - 1, -2 ** 31])
    mask = rng.random((n, m)) < 0.3
    idx[mask] = rng.choice(junk, size=int(mask.sum()))
    return idx.astype(np.int32)


# ---- the apply ---------------------------------------------------------------------------------------------------------------------------
def apply_ref(idx, coef, dinv, R):
    """(Z, mag, indeg): Z = W^T (W R) and mag = |W^T| (|W| |R|) in longdouble for the factor AS GIVEN (coef, dinv: any number type), and
    every column's in-degree"""
    n, m = idx.shape
    coef, dinv, R = np.asarray(coef, dtype=LD), np.asarray(dinv, dtype=LD), np.asarray(R, dtype=LD)
    idx = np.asarray(idx, dtype=np.int64)
    valid = (idx >= 0) & (idx < n)
    T, Tm = dinv[:, None] * R, np.abs(dinv)[:, None] * np.abs(R)
    for l in range(m):
        rows = np.flatnonzero(valid[:, l])
        T[rows] += coef[rows, l][:, None] * R[idx[rows, l]]
        Tm[rows] += np.abs(coef[rows, l])[:, None] * np.abs(R[idx[rows, l]])
    Z, Zm = dinv[:, None] * T, np.abs(dinv)[:, None] * Tm
    rows, ls = np.nonzero(valid)
    np.add.at(Z, idx[rows, ls], coef[rows, ls][:, None] * T[rows])
    np.add.at(Zm, idx[rows, ls], np.abs(coef[rows, ls])[:, None] * Tm[rows])
    return Z, Zm, np.bincount(idx[rows, ls], minlength=n)


def apply_bound(m, indeg, mag):
    """the componentwise bound of the two products done one after the other by fused multiply-adds: row j of Z is a sum of
    in-degree + 1 terms, each a sum of at most m + 1: gamma_k = k u / (1 - k u), k = m + in-degree + 2, on |W^T| (|W| |R|)"""
    k = (m + np.asarray(indeg, dtype=LD) + 2) * LD(EPS / 2)
    return (k / (1 - k))[:, None] * mag


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------
def pcg_nn_ref(A, b, apply, tol, **kw):
    """matrix_free_ref.pcg_ref on A x = b with z = apply(r) as the preconditioner: the recurrence is pcg_ref's own code, only the one
    function it calls for M^-1 r is exchanged for the call"""
    saved = mf.woodbury_apply
    mf.woodbury_apply = lambda G, v, r: apply(r)
    try:
        return mf.pcg_ref(A, b, None, None, tol, **kw)
    finally:
        mf.woodbury_apply = saved


def apply_double(W):
    """r -> W^T (W r) in float64 for a dense W"""
    return lambda r: W.T @ (W @ r)


@functools.lru_cache(maxsize=None)
def ordered_fixture(fx, m=NEIGHBORS, ordering="random", seed=0):
    """a matrix_free_ref fixture in a random ordering with its nearest-neighbour factor in float64: perm, the ordered x, V, A, rhs, the
    lists (the twin's search under the length scales), coef, dinv; computed once and shared (read-only)"""
    f = mf.fixture(fx)
    kernel, d = fx[0], fx[1]
    n = len(f["x"])
    perm = np.random.default_rng(seed).permutation(n) if ordering == "random" else np.arange(n)
    x, V = f["x"][perm], f["V"][perm]
    K = f["K"][np.ix_(perm, perm)]
    idx = vr.search_ref(x, x, m, vr.length_scales(kernel, f["theta"], d), c0=0)
    coef, dinv = factor_ref(K, V, idx, np.float64)
    out = {"perm": perm, "x": x, "V": V, "K": K, "A": K + np.diag(V), "rhs": f["rhs"][perm], "idx": idx, "coef": coef, "dinv": dinv,
           "theta": f["theta"], "kernel": kernel}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture_w(fx, m=NEIGHBORS):
    o = ordered_fixture(fx, m)
    return dense_w(o["idx"], o["coef"], o["dinv"])


@functools.lru_cache(maxsize=None)
def fixture_pcg_nn(fx, col, tol, m=NEIGHBORS):
    """the twin's solve of column `col` of the ordered fixture with its own float64 factor"""
    o = ordered_fixture(fx, m)
    return pcg_nn_ref(o["A"], o["rhs"][:, col], apply_double(fixture_w(fx, m)), tol)


# ---- the factor's cases and bars (vecchia_ref.ACC_CASES at B = 1) -----------------------------------------------------------------------------
def factor_inputs(case):
    """(x, theta, v, idx) of an accuracy case: vecchia_ref's, the first theta"""
    x, thetas, _, v, idx = vr.case_inputs(case)
    return x, thetas[0], v, idx


def factor_figures(got, ref, d_ref):
    """{"coef": max |coef - ref| sqrt(d) (the error of a = A^-1 k, of order one), "dinv": max relative error}"""
    coef, dinv = np.asarray(got[0], dtype=LD), np.asarray(got[1], dtype=LD)
    scale = np.sqrt(np.asarray(d_ref, dtype=LD))[:, None]
    return {"coef": float(np.max(np.abs(coef - ref[0]) * scale)) if coef.size else 0.0,
            "dinv": float(np.max(np.abs(dinv - ref[1]) / np.abs(ref[1])))}


@functools.lru_cache(maxsize=None)
def factor_reference(case):
    """the longdouble (coef, dinv, d) of a case"""
    name = case[0]
    x, theta, v, idx = factor_inputs(case)
    coef, dinv = factor_ref(kf.k_ref(name, x, x, theta, LD), v, idx, LD)
    return coef, dinv, 1 / (dinv * dinv)


@functools.lru_cache(maxsize=None)
def factor_bars(case):
    """{figure: MARGIN * max(base, FLOOR)}, base = the larger of the plain and the perturbed float64 twin's error against longdouble"""
    name, d = case[0], case[1]
    x, theta, v, idx = factor_inputs(case)
    ref = factor_reference(case)
    K = kf.k_ref(name, x, x, theta, np.float64)
    rng = np.random.default_rng(4242)
    base = dict.fromkeys(FIGURES, 0.0)
    for run in (factor_ref(K, v, idx, np.float64),
                factor_ref(K, v, idx, np.float64, perturb=(rng, kf.k_bound_ulps(d)), sigma2=theta[0])):
        f = factor_figures(run, ref, ref[2])
        base = {k: max(base[k], f[k]) for k in FIGURES}
    return {k: MARGIN * max(base[k], FLOOR[k]) for k in FIGURES}
