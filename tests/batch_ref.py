"""An extended-precision reference for the three batched entries -- fvgp_hip_loglik_batch, fvgp_hip_loglik_grad_batch and
fvgp_hip_posterior_batch -- and float64 twins of their linear algebra (a helper module of the tests, not a conftest): numpy only, no GPU.

It is put together from the references the suite has already: kernel_family_ref (k_ref, dk_dtheta_ref, grad_trace_terms), chol_ref
(chol_ld, beta, phi, lam, edge_rows, twin_chol, max_block_cond and the caps of chol_ref.Reference), tri_solve_ref (blockinv_fwd,
col_err, _tri_inv) and posterior_ref (smooth_y, points, sample_points, posterior_twin and the measures mu, nu, sig of its Reference).
New here: the fixtures written as (x, theta, V, y) -- the batched entries assemble K themselves --, substitution with a factor that
is in longdouble already on many columns at once (fwd_cols), the float64 twin of W = L^-1 by recursive halving (inverse_twin) and the
measures of z, W, KV^-1, b, diag(KV^-1) and the gradient.

The fixtures, deterministic from (family, n): x = default_rng(5).random((n, d)),

    E    rbf_ard, d = 2, sigma^2 = 1.3, l = 0.3, V = 1e-2 (1 + x_0 / 2)                      the benign one (cond_2 about 1e4 at most)
    G    rbf_ard, d = 2, sigma^2 = 1, l = 0.05, V = 1e-6        chol_ref's G: k_ref reproduces tri_solve_ref.covariance_g off the diagonal
    H    rbf_ard, d = 2, sigma^2 = 1, l = 0.1,  V = 1e-8        chol_ref's H, the harder one
    U-   G with sigma^2 and V times 2^-400 and y times 2^-200       U+   2^400, 2^200       (exact scalings: z and the measures are G's)
    M    matern32_iso, d = 3, sigma^2 = 1.7, l = 0.15, V = 1e-6 (1 + x_0 / 2)               not everything rests on RBF

y (n, 8) = amplitude posterior_ref.smooth_y(x, 8) + sqrt(noise) N(0, 1), per family its own amplitude and draw.  On E the smooth part is
3 K (1 + smooth_y / 2) instead: a well-determined GP has a gradient that is the small difference of its two traces (|ghat_i| down to
1e-6 M_i at n = 897 with the plain y), and a relative figure needs |ghat_i| >= 1e-3 M_i; with b = KV^-1 y close to a positive smooth
vector the terms b_j b_k dK_jk share a sign and the condition holds at every size (tests/test_batch_ref_host.py).

The reference of a problem, in longdouble: A = fl64(K) + diag(V) (K = k_ref rounded to float64: the matrix an exact assembly hands the
factorisation), Lhat = chol_ld(A), z = Lhat^-1 y, {log-likelihood, log|KV|, quad / ncol}, What = Lhat^-1, KVinv = What^T What,
alpha = KVinv y (b is a column of it), diag(KVinv), the gradient 1/2 sum_jk (KVinv_jk - b_j b_k) dK_jk/dtheta_i of the NEGATIVE
log-likelihood with its magnitude sum M_i = 1/2 sum_jk |...|, and for prediction points V^T = Lhat^-1 k(x, x*), mean = V z,
var and S (PosteriorReference).  Everything is computed once per process and read-only.

The float64 twins, from which every bar comes (never from the device).  Like the entries they start from (x, theta, V, y): both factor
A64 = k_ref(dtype=float64) + diag(V), the float64 assembly, and are measured against A and Lhat like the device (_Chol says why):

    "a"   chol_ref.twin_chol(A, 128) -- the explicit-inverse panel solve, which the batched path always takes --, z by
          tri_solve_ref.blockinv_fwd at 128, W = inverse_twin (the device's recursive halving, split mid = J0 + (blocks // 2) 128),
          KVinv = W^T W, b = W^T z, the trace in float64
    "c"   scipy's LAPACK: cholesky, solve_triangular, cho_solve
    posterior: posterior_ref.posterior_twin on each of the two factors (substitution by scipy on "c", blockinv_fwd at 128 on "a"),
          and for the mean also V z with both in float64 on "a", which is how the device forms it

The measures (eps = 2^-52; all differences in longdouble):

    beta, phi, lam     chol_ref's, beta over edge_rows(n, halving_bounds(dim)) and the whole diagonal
    z                  the worst relative 2-norm error of a column (tri_solve_ref.col_err)
    W, KVinv           the worst relative 2-norm error of a row of the lower triangle, over all rows (chol_ref.phi)
    resid              max_i max_j |KVinv A - I|_ij / max_j (|KVinv| |A|)_ij / eps over the complete rows i of edge_rows
    b2, diag2          relative 2-norm error of b and of diag(KVinv)
    bc                 max_j |b_j - bhat_j| / (|KVinv| |y_c|)_j / eps        dc      max_j |d_j - dhat_j| / dhat_j / eps
    grad               max_i |g_i - ghat_i| / M_i
    mu, nu, sig        posterior_ref's, per point class"""
import numpy as np

import chol_ref
import kernel_family_ref as kf
import posterior_ref as pr
import tri_solve_ref as ts

LD = ts.LD
EPS = ts.EPS
EPS_LD = ts.EPS_LD
TILE = 128
SEED = 5
MAX_COLS = 8
MARGIN = 8.0                     # a differently ordered float64 sum: the margin of the Cholesky, triangular-solve and posterior suites
FLOOR_EPS = 4.0                  # floor of a measure counted in units of eps; FLOOR_EPS * EPS for a relative one
U_EXP = chol_ref.U_EXP
# family -> (kernel, d, theta, noise, V varies with x, amplitude of y, y = amplitude K (1 + smooth_y / 2) instead of amplitude smooth_y)
FAMILY = {"E": ("rbf_ard", 2, (1.3, 0.3, 0.3), 1e-2, True, 3.0, True),
          "G": ("rbf_ard", 2, (1.0,) + 2 * (chol_ref.PARAMS["G"][0],), chol_ref.PARAMS["G"][1], False, 0.7, False),
          "H": ("rbf_ard", 2, (1.0,) + 2 * (chol_ref.PARAMS["H"][0],), chol_ref.PARAMS["H"][1], False, 1.4, False),
          "M": ("matern32_iso", 3, (1.7, 0.15), 1e-6, True, 0.9, False)}
# the sizes of the device tests (tests/test_gpu_batch_accuracy.py states which branch each reaches); 1300: the factor only
GPU_N = (1, 127, 128, 124, 300, 513, 700, 897, 1300)
# cond_2(A) of the fixtures, measured on the host (tests/test_batch_ref_host.py asserts a band of 30 % around each: the caps of the
# device tests rest on them).  G and H at 700 and 1300 are chol_ref.COND's: the matrices agree to the rounding of the two formulas.
COND = {("E", 1): 1.0, ("E", 124): 5.61e3, ("E", 127): 5.76e3, ("E", 128): 5.77e3, ("E", 300): 1.38e4, ("E", 513): 2.30e4,
        ("E", 700): 3.18e4, ("E", 897): 4.06e4, ("E", 1300): 5.92e4,
        ("G", 1): 1.0, ("G", 124): 5.34e3, ("G", 127): 5.46e3, ("G", 128): 5.46e3, ("G", 300): 2.46e5, ("G", 513): 6.15e6,
        ("G", 897): 1.77e7,
        ("H", 1): 1.0, ("H", 124): 1.36e6, ("H", 127): 1.56e6, ("H", 128): 1.57e6, ("H", 300): 1.94e9, ("H", 513): 3.09e9,
        ("H", 897): 5.56e9,
        ("M", 1): 1.0, ("M", 124): 406.0, ("M", 127): 414.0, ("M", 128): 414.0, ("M", 300): 1.01e3, ("M", 513): 6.81e3,
        ("M", 700): 9.39e3, ("M", 897): 1.27e4, ("M", 1300): 2.15e4}
COND.update({k: v for k, v in chol_ref.COND.items() if k[0] in "GH" and k[1] in GPU_N})


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
class Problem:
    """one (family, n): kernel, d, x (n, d), theta, V (n,), y (n, 8) and A = fl64(K) + diag(V), all float64 and read-only"""

    def __init__(self, fam, n):
        base = "G" if fam in U_EXP else fam
        self.fam, self.n = fam, n
        self.kernel, self.d, theta, self.noise, varies, amp, through_k = FAMILY[base]
        self.x = np.random.default_rng(SEED).random((n, self.d))
        theta = np.array(theta, dtype=np.float64)
        V = self.noise * (1.0 + 0.5 * self.x[:, 0]) if varies else np.full(n, self.noise)
        rng = np.random.default_rng(7919 * n + sorted(FAMILY).index(base))
        K = np.asarray(kf.k_ref(self.kernel, self.x, self.x, theta), dtype=np.float64)
        assert np.array_equal(K, K.T)
        smooth = K @ (1.0 + 0.5 * pr.smooth_y(self.x, MAX_COLS)) if through_k else pr.smooth_y(self.x, MAX_COLS)
        y = amp * smooth + np.sqrt(self.noise) * rng.standard_normal((n, MAX_COLS))
        if fam in U_EXP:                                   # exact: powers of two
            theta[0] = np.ldexp(theta[0], U_EXP[fam])
            V = np.ldexp(V, U_EXP[fam])
            y = np.ldexp(y, U_EXP[fam] // 2)
            K = np.ldexp(K, U_EXP[fam])
        self.theta, self.V, self.y = theta, V, y
        K[np.arange(n), np.arange(n)] += V
        self.A = K
        # what the twins factor: the same formulas in float64 (r^2 and the radial function rounded as a float64 assembly rounds them)
        K64 = kf.k_ref(self.kernel, self.x, self.x, theta, dtype=np.float64)
        K64 = np.tril(K64) + np.tril(K64, -1).T
        K64[np.arange(n), np.arange(n)] += V
        self.A64 = K64
        for a in (self.x, self.theta, self.V, self.y, self.A, self.A64):
            a.setflags(write=False)


_PROBLEMS = {}


def problem(fam, n):
    if (fam, n) not in _PROBLEMS:
        _PROBLEMS[(fam, n)] = Problem(fam, n)
    return _PROBLEMS[(fam, n)]


# ---- extended precision ---------------------------------------------------------------------------------------------------------
def fwd_cols(Lhat, B):
    """Lhat X = B for a factor that is in longdouble already and many columns at once, row by row (chol_ref.fwd_ld takes one column,
    tri_solve_ref.fwd_ld a float64 factor).  B (n, m), float64 or longdouble."""
    n = Lhat.shape[0]
    X = np.array(np.asarray(B).reshape(n, -1), dtype=LD)
    for i in range(n):
        if i:
            X[i] -= Lhat[i, :i] @ X[:i]
        X[i] /= Lhat[i, i]
    return X


def inverse_ld(Lhat):
    """What = Lhat^-1 in longdouble: substitution on the identity, a row touching the columns up to its own only"""
    n = Lhat.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = LD(1)
        if i:
            X[i, :i] = -(Lhat[i, :i] @ X[:i, :i])
        X[i, :i + 1] /= Lhat[i, i]
    return X


def gram_ld(What):
    """What^T What in longdouble for a lower-triangular What: 128 rows of the result at a time, each from the rows of What that are
    not zero in those columns (a third of the full product's work); symmetric in its bits"""
    n = What.shape[0]
    G = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, TILE):
        i1 = min(n, i0 + TILE)
        G[i0:i1, :i1] = What[i0:, i0:i1].T @ What[i0:, :i1]
    low = np.tril(G)
    return low + np.tril(G, -1).T


def loglik_ld(kernel, x, theta, V, y):
    """the log marginal likelihood of (x, theta, V, y) in longdouble from A = fl64(K) + diag(V); y (n, ncol), the quadratic form
    averaged over the columns as the entries do"""
    n = len(x)
    A = np.asarray(kf.k_ref(kernel, x, x, theta), dtype=np.float64)
    A[np.arange(n), np.arange(n)] += V
    Lhat = chol_ref.chol_ld(A)
    z = fwd_cols(Lhat, y)
    return -LD(0.5) * (np.sum(z * z) / LD(z.shape[1]) + chol_ref.logdet_ld(Lhat) + LD(n) * _log2pi())


def _log2pi():
    return np.log(LD(2) * np.arccos(LD(-1)))


# ---- the float64 twin of W = L^-1 ---------------------------------------------------------------------------------------------------
def halving_bounds(dim, split=lambda blocks: blocks // 2):
    """the sorted boundaries `mid` of the recursive halving over the 128-wide block columns of [0, dim)"""
    out = []

    def rec(J0, Jend):
        blocks = (Jend - J0) // TILE
        if blocks <= 1:
            return
        mid = J0 + split(blocks) * TILE
        out.append(mid)
        rec(J0, mid)
        rec(mid, Jend)
    rec(0, -(-dim // TILE) * TILE)
    return sorted(out)


def inverse_twin(L, split=lambda blocks: blocks // 2):
    """W = L^-1 in float64 as fvgp_hip_loglik_grad_batch forms it: the inverses of the 128-blocks on the diagonal, then over the padded
    size inv [[A, 0], [C, D]] = [[inv A, 0], [-inv(D) (C inv(A)), inv D]] with the split mid = J0 + split(blocks) 128 (the padding is
    an identity block, which changes no entry of the leading n x n part: the ranges are clipped to n)"""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = L.shape[0]
    W = np.zeros((n, n))
    for k0 in range(0, n, TILE):
        k1 = min(n, k0 + TILE)
        W[k0:k1, k0:k1] = ts._tri_inv(L[k0:k1, k0:k1])

    def rec(J0, Jend):
        blocks = (Jend - J0) // TILE
        if blocks <= 1:
            return
        mid = J0 + split(blocks) * TILE
        rec(J0, mid)
        rec(mid, Jend)
        e = min(n, Jend)
        if mid < e:
            X = L[mid:e, J0:mid] @ W[J0:mid, J0:mid]
            W[mid:e, J0:mid] = -(W[mid:e, mid:e] @ X)
    rec(0, -(-n // TILE) * TILE)
    return W


# ---- the measures -------------------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0.0, np.inf))
    r = np.where(np.isfinite(r), r, np.inf)
    return float(np.max(r))


def row_err(X, Xhat):
    """the worst relative 2-norm error of a row of the lower triangle, over all rows (chol_ref.phi; Xhat's upper part is not read)"""
    return chol_ref.phi(X, np.tril(Xhat))


def col_err(got, ref):
    return ts.col_err(np.asarray(got).reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1))[1]


def sym_from_lower(X):
    X = np.tril(np.asarray(X))
    return X + np.tril(X, -1).T


def resid(KVinv_low, A, rows):
    """max_i max_j |KVinv A - I|_ij / max_j (|KVinv| |A|)_ij in units of eps over the complete rows `rows`; KVinv given by its lower
    triangle.  Row by row and not entry by entry: where the entries of A fall to 1e-170 (RBF at l = 0.05) single denominators lie far
    below the scale of their row, and an entry-wise maximum follows the order of the sums (the other split of the inverse twin moved it
    by a factor of 17 on G at n = 700) instead of the size of the error."""
    X = np.asarray(sym_from_lower(KVinv_low), dtype=LD)[list(rows)]
    if not np.all(np.isfinite(X)):
        return float("inf")
    Al = np.asarray(A, dtype=LD)
    R = X @ Al
    R[np.arange(len(rows)), list(rows)] -= LD(1)
    return _ratio(np.max(np.abs(R), axis=1), np.max(np.abs(X) @ np.abs(Al), axis=1)) / EPS


def comp_err(got, ref, den):
    """max_j |got_j - ref_j| / den_j in units of eps"""
    got = np.asarray(got, dtype=LD)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return _ratio(np.abs(got - ref), den) / EPS


def grad_err(g, ghat, M):
    g = np.asarray(g, dtype=LD)
    if not np.all(np.isfinite(g)):
        return float("inf")
    return _ratio(np.abs(g - ghat), M)


def bar(twins, floor, cap=None):
    """MARGIN max(twins, floor), and the derived cap where there is one"""
    b = MARGIN * max(max(twins), floor)
    return b if cap is None else min(b, cap)


# ---- the reference of one problem ---------------------------------------------------------------------------------------------------
class _Chol(chol_ref.Reference):
    """chol_ref.Reference of A whose float64 factors -- scipy's and the twins' -- are those of the float64 assembly A64: a batched entry
    is handed (x, theta, V) and not a matrix, so what float64 arithmetic attains includes the rounding of the entries of K (the
    argument r^2 / 2 of an RBF entry is rounded relative to ITSELF, up to 400 at l = 0.05: a few hundred eps relative in a small entry,
    which beta counts in full where the matrix is nearly diagonal, n <= 128 on G).  Every measure stays against A and Lhat."""

    def __init__(self, A, A64, Lhat=None, cond=None):
        super().__init__(A, Lhat, cond)
        self.A64 = A64

    def factor(self, which):
        if which not in self._factors:
            if which == "scipy":
                import scipy.linalg as sla
                F = np.tril(sla.cholesky(self.A64, lower=True))
            else:
                F = chol_ref.twin_chol(self.A64, which)
            F.setflags(write=False)
            self._factors[which] = F
        return self._factors[which]


class Reference:
    """problem(fam, n) with its longdouble results and, as the tests ask, the figures of the twins.  chol: the chol_ref.Reference of A
    (Lhat, cond_2, beta, phi, lam and their caps) with the float64 factors of twin "a" = 128 and "c" = "scipy" taken of A64."""
    TWINS = ("a", "c")

    def __init__(self, fam, n):
        self.p = p = problem(fam, n)
        self.fam, self.n = fam, n
        if fam in U_EXP:                     # chol_ld scales exactly by a power of two (tests/test_chol_ref.py proves it)
            g = reference("G", n)
            self.chol = _Chol(p.A, p.A64, Lhat=np.ldexp(g.chol.Lhat, U_EXP[fam] // 2), cond=g.chol.cond)
        else:
            self.chol = _Chol(p.A, p.A64)
        self.Lhat = self.chol.Lhat
        self.z = fwd_cols(self.Lhat, p.y)
        self.z.setflags(write=False)
        self._c = {}

    def _once(self, key, make):
        if key not in self._c:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._c[key] = v
        return self._c[key]

    # -- longdouble
    def out(self, ncol):
        """{log-likelihood, log|KV|, quad / ncol} in longdouble"""
        logdet = chol_ref.logdet_ld(self.Lhat)
        quad = np.sum(self.z[:, :ncol] ** 2) / LD(ncol)
        return np.array([-LD(0.5) * (quad + logdet + LD(self.n) * _log2pi()), logdet, quad], dtype=LD)

    @property
    def What(self):
        return self._once("What", lambda: inverse_ld(self.Lhat))

    @property
    def KVinv(self):
        return self._once("KVinv", lambda: gram_ld(self.What))

    @property
    def alpha(self):
        """KVinv y (n, 8): b of component c is its column c"""
        return self._once("alpha", lambda: self.What.T @ self.z)

    @property
    def dinv(self):
        return self._once("dinv", lambda: np.sum(self.What * self.What, axis=0))

    def b_den(self, c):
        return self._once(("bden", c), lambda: np.abs(self.KVinv) @ np.abs(np.asarray(self.p.y[:, c], dtype=LD)))

    def grad(self, c):
        """(ghat (n_theta,), M (n_theta,)): the gradient of the negative log-likelihood and its magnitude sum"""
        def make():
            t = kf.grad_trace_terms(self.p.kernel, self.p.x, self.p.theta, self.KVinv, self.alpha[:, c])
            return np.sum(t, axis=(1, 2)), np.sum(np.abs(t), axis=(1, 2))
        return self._once(("grad", c), make)

    def rows(self, dim=None):
        """the rows beta and resid look at: both sides of every halving boundary of the dim the call has"""
        dim = -(-self.n // TILE) * TILE if dim is None else dim
        return chol_ref.edge_rows(self.n, bounds=halving_bounds(dim))

    # -- the twins
    def L(self, t):
        return self.chol.factor(TILE if t == "a" else "scipy")

    def twin_z(self, t):
        def make():
            if t == "a":
                return ts.blockinv_fwd(self.L(t), self.p.y, TILE)
            import scipy.linalg as sla
            return sla.solve_triangular(self.L(t), self.p.y, lower=True)
        return self._once(("z", t), make)

    def twin_W(self, t, split=None):
        def make():
            if t == "a":
                return inverse_twin(self.L(t)) if split is None else inverse_twin(self.L(t), split)
            import scipy.linalg as sla
            return np.tril(sla.solve_triangular(self.L(t), np.eye(self.n), lower=True))
        return make() if split is not None else self._once(("W", t), make)

    def twin_KVinv(self, t):
        def make():
            if t == "a":
                W = self.twin_W(t)
                return W.T @ W
            import scipy.linalg as sla
            X = sla.cho_solve((self.L(t), True), np.eye(self.n))
            return 0.5 * (X + X.T)
        return self._once(("KVinv", t), make)

    def twin_alpha(self, t):
        def make():
            if t == "a":
                return self.twin_W(t).T @ self.twin_z(t)
            import scipy.linalg as sla
            return sla.cho_solve((self.L(t), True), self.p.y)
        return self._once(("alpha", t), make)

    def twin_grad(self, t, c, KVinv=None):
        def make():
            Ki = self.twin_KVinv(t) if KVinv is None else KVinv
            terms = kf.grad_trace_terms(self.p.kernel, self.p.x, self.p.theta, Ki, self.twin_alpha(t)[:, c], dtype=np.float64)
            return np.sum(terms, axis=(1, 2))
        return make() if KVinv is not None else self._once(("grad", t, c), make)

    # -- measures of given results (the device's or a twin's) against the reference
    def measure_factor(self, L, z, dim=None):
        """{beta, phi, lam, z} of a factor (lower triangle read) and z (n, ncol)"""
        return {"beta": chol_ref.beta(self.p.A, L, self.rows(dim)), "phi": chol_ref.phi(L, self.Lhat),
                "lam": chol_ref.lam(L, self.Lhat), "z": col_err(z, self.z[:, :np.asarray(z).reshape(self.n, -1).shape[1]])}

    def measure_grad(self, c, W=None, KVinv=None, b=None, diag=None, g=None):
        """the measures of W, KVinv (lower triangles read), b, diag(KVinv) and the gradient, those that are given"""
        out = {}
        if W is not None:
            out["W"] = row_err(W, self.What)
        if KVinv is not None:
            out["KVinv"] = row_err(KVinv, self.KVinv)
            out["resid"] = resid(KVinv, self.p.A, self.rows())
        if b is not None:
            out["b2"] = col_err(b, self.alpha[:, c])
            out["bc"] = comp_err(b, self.alpha[:, c], self.b_den(c))
        if diag is not None:
            out["diag2"] = col_err(diag, self.dinv)
            out["dc"] = comp_err(diag, self.dinv, self.dinv)
        if g is not None:
            out["grad"] = grad_err(g, *self.grad(c))
        return out

    def twin_factor(self, t, ncol=MAX_COLS, dim=None):
        return self._once(("mf", t, ncol, dim), lambda: self.measure_factor(self.L(t), self.twin_z(t)[:, :ncol], dim))

    def twin_measures(self, t, c):
        return self._once(("mg", t, c), lambda: self.measure_grad(c, self.twin_W(t), self.twin_KVinv(t), self.twin_alpha(t)[:, c],
                                                                  np.diagonal(self.twin_KVinv(t)), self.twin_grad(t, c)))

    # -- the bars
    def floor(self, q):
        if q == "lam":
            return chol_ref.lam_floor(self.Lhat)
        return FLOOR_EPS if q in ("beta", "resid", "bc", "dc") else FLOOR_EPS * EPS

    def cap(self, q):
        """the derived caps the project states already (chol_ref.Reference): beta of the explicit-inverse panel solve, phi, lam"""
        return {"beta": self.chol.cap_beta(True), "phi": self.chol.cap_phi(), "lam": self.chol.cap_lam()}.get(q)

    def factor_bars(self, ncol=MAX_COLS, dim=None):
        """{measure: (worst twin, bar)}"""
        tw = [self.twin_factor(t, ncol, dim) for t in self.TWINS]
        return {q: (max(m[q] for m in tw), bar([m[q] for m in tw], self.floor(q), self.cap(q))) for q in tw[0]}

    def grad_bars(self, c):
        tw = [self.twin_measures(t, c) for t in self.TWINS]
        return {q: (max(m[q] for m in tw), bar([m[q] for m in tw], self.floor(q))) for q in tw[0]}


_REFS = {}


def reference(fam, n):
    if (fam, n) not in _REFS:
        _REFS[(fam, n)] = Reference(fam, n)
    return _REFS[(fam, n)]


# ---- the posterior ------------------------------------------------------------------------------------------------------------------
class _Twin:
    """what posterior_ref.points and posterior_ref.posterior_twin read of a fixture, with a float64 factor and alpha of a twin"""

    def __init__(self, r, t):
        p = r.p
        self.fam, self.n, self.kernel, self.d, self.x, self.theta = p.fam, p.n, p.kernel, p.d, p.x, p.theta
        self.L = None if t is None else r.L(t)
        self._alpha = None if t is None else r.twin_alpha(t)

    def alpha(self, ncol=MAX_COLS):
        return self._alpha[:, :ncol]


def points(r, P, seed=0):
    """posterior_ref.points on the problem of a Reference: (xpred (P, d), classes), point p of class posterior_ref.CLASSES[p % 5]"""
    return pr.points(_Twin(r, None), P, seed)


class PosteriorReference(pr.Reference):
    """posterior_ref.Reference -- its measures mu, nu, sig per point class and their denominators -- of the sampled points xs, with the
    posterior taken from the longdouble factor itself: V^T = Lhat^-1 k(x, x*), mean = V z, var and S = k** - V^T V"""

    def __init__(self, r, xs, cls, ncol):
        self.r, self.fx, self.xs, self.cls, self.ncol = r, _Twin(r, None), np.asarray(xs), list(cls), ncol
        p = r.p
        self.k = kf.k_ref(p.kernel, p.x, self.xs, p.theta)
        kss = kf.k_ref(p.kernel, self.xs, self.xs, p.theta)
        self.w = fwd_cols(r.Lhat, self.k)
        self.m = self.w.T @ r.z[:, :ncol]
        self.S = kss - self.w.T @ self.w
        self.v = np.diagonal(self.S).copy()
        sig = LD(p.theta[0])
        a = np.abs(r.alpha[:, :ncol])
        self.den_mu = LD(EPS) * (np.abs(self.k).T @ a + sig * np.sum(a, axis=0)[None, :])
        self.den_nu = LD(EPS) * sig
        wn = np.sqrt(np.sum(self.w * self.w, axis=0))
        self.den_sig = LD(EPS) * (np.outer(wn, wn) + sig)
        self._twin = {}

    def twin(self, t):
        """the measures of posterior_ref.posterior_twin on the factor of twin "a" (blockinv_fwd at 128) or "c" (scipy's substitution);
        "a" also with the mean as V z, both in float64, the worse of the two means"""
        if t not in self._twin:
            fx = _Twin(self.r, t)
            m, v, S = pr.posterior_twin(fx, self.xs, TILE if t == "a" else None, self.ncol)
            q = self.measure(m, v, S)
            if t == "a":
                p = self.r.p
                w = ts.blockinv_fwd(fx.L, kf.k_ref(p.kernel, p.x, self.xs, p.theta, dtype=np.float64), TILE)
                q2 = self.measure(m=w.T @ self.r.twin_z("a")[:, :self.ncol])
                q["mu"] = {c: max(q["mu"][c], q2["mu"][c]) for c in q["mu"]}
            self._twin[t] = q
        return self._twin[t]

    def bars(self):
        """{measure: {class: (worst twin, MARGIN max(twins, posterior_ref.FLOOR))}}"""
        a, c = self.twin("a"), self.twin("c")
        return {q: {k: (max(a[q][k], c[q][k]), MARGIN * max(a[q][k], c[q][k], pr.FLOOR[q])) for k in a[q]} for q in pr.MEASURES}
