"""An extended-precision reference for the Cholesky factorisation (a helper module of the tests, not a conftest): numpy only, no GPU.

chol_ld: a column-by-column Cholesky of a float64 matrix in numpy.longdouble (64-bit mantissa on x86-64).  The matrix is taken as
given and only its lower triangle is read: the result is the factor of exactly that matrix up to longdouble rounding, so it can judge
a float64 factorisation of any algorithm.  About 2 s at n = 1300: references are computed once per process (reference()).

The matrix families, deterministic from (family, n):

    W    B B^T + n I with B = default_rng(n).standard_normal((n, n)), the _spd(n, n) of test_gpu_primitives: cond_2 = 5
    G    RBF covariance exp(-|x - x'|^2 / (2 l^2)) + noise I on default_rng(5).random((n, 2)), l = 0.05, noise 1e-6 (cond_2 = 2.4e7 at
         n = 1300), built by tri_solve_ref.covariance_g -- the matrix tri_solve_ref.factor_g factors
    H    the harder one: l = 0.1, noise 1e-8 (8.0e9 at n = 1300)
    S    D G D with D = tri_solve_ref.scaling_s: powers of two 2^-20 .. 2^20.  Scaling by a power of two is exact, so chol(D G D) =
         D chol(G) -- in floating point too when the order of the sums does not depend on the data and nothing over- or underflows
    U-   2^-400 G        U+   2^400 G        (factor: 2^-200, 2^200 times that of G)

twin_chol: a float64 numpy twin of the two ways the device does the panel solve X = P inv(L_kk)^T -- right-looking, 128 columns at a
time; tb = 128: a product with the explicit inverse of the 128-block; tb = 16: substitution over 16-column tiles with the explicit
inverses of the 16 x 16 diagonal tiles.  The diagonal block itself is factored as the leaf kernel does it (leaf_twin: 16-column tiles,
the rows inside the block solved with explicit inverses of 4 x 4 diagonal blocks).  It shows what float64 arithmetic of each algorithm
attains, so the bar the device is held to never comes from the device.

The measures, all in longdouble, against A itself or against Lhat = chol_ld(A):

    beta    max |A - L L^T|_ij / (|L| |L|^T)_ij / eps over the complete rows edge_rows() and the whole diagonal: the componentwise
            backward error, which (unlike a forward comparison with LAPACK) tells substitution from a product with an explicit inverse
    phi     max_i ||L_i - Lhat_i||_2 / ||Lhat_i||_2 over ALL rows (row i of the lower triangle): a wrong tile cannot hide from it
    lam     |2 sum log L_ii - 2 sum log Lhat_ii|"""
import numpy as np

import tri_solve_ref as ref

LD = ref.LD
EPS = ref.EPS
EPS_LD = ref.EPS_LD
TILE = 128
SEED = 5
PARAMS = {"G": (0.05, 1e-6), "H": (0.1, 1e-8)}          # family -> (length scale, noise)
U_EXP = {"U-": -400, "U+": 400}
MAX_ROWS = 24
# cond_2 of the fixtures, measured on the host (tests/test_chol_ref.py asserts a band of 30 % around each: the caps of the device tests
# rest on them)
COND = {("W", 129): 5.07, ("W", 700): 4.91, ("W", 1300): 4.99,
        ("G", 129): 5.46e3, ("G", 700): 1.45e7, ("G", 1300): 2.44e7, ("G", 1281): 2.43e7, ("G", 1408): 2.65e7,
        ("H", 129): 1.57e6, ("H", 700): 4.44e9, ("H", 1300): 7.96e9, ("H", 1281): 7.86e9, ("H", 1408): 8.62e9}


# ---- the factorisation in extended precision --------------------------------------------------------------------------------------
def chol_ld(A):
    """the lower Cholesky factor of the float64 matrix A in longdouble, column by column; only the lower triangle of A is read"""
    A = np.asarray(A)
    if A.dtype != np.float64 or A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise TypeError("the matrix must be a square float64 array")
    n = A.shape[0]
    Al = np.asarray(np.tril(A), dtype=LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = Al[j:, j] - L[j:, :j] @ L[j, :j] if j else Al[:, 0].copy()
        if not c[0] > 0:
            raise np.linalg.LinAlgError(f"leading minor of order {j + 1} is not positive")
        d = np.sqrt(c[0])
        L[j, j] = d
        L[j + 1:, j] = c[1:] / d
    return L


def fwd_ld(Lhat, b):
    """Lhat y = b by forward substitution with a factor that is already in longdouble"""
    n = Lhat.shape[0]
    y = np.array(np.asarray(b).reshape(n), dtype=LD)
    for i in range(n):
        if i:
            y[i] -= Lhat[i, :i] @ y[:i]
        y[i] /= Lhat[i, i]
    return y


# ---- the matrix families ----------------------------------------------------------------------------------------------------------
def matrix(fam, n):
    """the float64 matrix of a family (symmetric; the device only ever sees its lower triangle)"""
    if fam == "W":
        B = np.random.default_rng(n).standard_normal((n, n))
        return B @ B.T + n * np.eye(n)
    if fam in PARAMS:
        return ref.covariance_g(n, SEED, *PARAMS[fam])
    G = ref.covariance_g(n, SEED, *PARAMS["G"])
    if fam == "S":
        D = scaling(n)
        return D[:, None] * G * D[None, :]
    if fam in U_EXP:
        return np.ldexp(G, U_EXP[fam])
    raise KeyError(fam)


def scaling(n):
    return ref.scaling_s(n, SEED)


def row_scale(fam, n):
    """the diagonal D with chol(matrix(fam, n)) = D chol(matrix("G", n)) for the scaled families (powers of two), else None"""
    if fam == "S":
        return scaling(n)
    if fam in U_EXP:
        return np.full(n, np.ldexp(1.0, U_EXP[fam] // 2))
    return None


def cond2(A):
    w = np.linalg.eigvalsh(A)
    return float(w[-1] / w[0])


# ---- the float64 twins ------------------------------------------------------------------------------------------------------------
def _solve_tiles(P, Lkk, tb):
    """X = P inv(Lkk)^T by substitution over tb-column tiles with the explicit inverses of Lkk's tb x tb diagonal tiles"""
    w = Lkk.shape[0]
    X = np.empty_like(P)
    for t0 in range(0, w, tb):
        t1 = min(w, t0 + tb)
        R = P[:, t0:t1] - X[:, :t0] @ Lkk[t0:t1, :t0].T if t0 else P[:, t0:t1]
        X[:, t0:t1] = R @ ref._tri_inv(Lkk[t0:t1, t0:t1]).T
    return X


def _right_looking(M, nb, factor_diag, solve):
    """blocked right-looking Cholesky of the symmetric M: nb columns at a time, the diagonal block by factor_diag, the rows below it by
    solve(P, L_pp), then one update of everything to the right"""
    w = M.shape[0]
    M = np.array(M)
    L = np.zeros((w, w))
    for p0 in range(0, w, nb):
        p1 = min(w, p0 + nb)
        Lpp = factor_diag(M[p0:p1, p0:p1])
        L[p0:p1, p0:p1] = Lpp
        if p1 < w:
            X = solve(M[p1:, p0:p1], Lpp)
            L[p1:, p0:p1] = X
            M[p1:, p1:] -= X @ X.T
    return L


def _tile_twin(T):
    """a 16 x 16 diagonal tile as leaf_body.h PanelBlock factors it: four columns at a time, the rows below the 4 x 4 diagonal block by
    ONE product with its explicit inverse (X^T = W R^T), a rank-4 update of the rest"""
    return _right_looking(T, 4, np.linalg.cholesky, lambda P, Lbb: P @ ref._tri_inv(Lbb).T)


def leaf_twin(B):
    """a 128 x 128 diagonal block as the leaf kernel factors it (leaf_body.h): 16-column tiles; the tiles below a diagonal tile by
    tile_trsm_acc -- four columns at a time, a product with the inverted 4 x 4 diagonal block, then a rank-4 update of the columns left"""
    return _right_looking(B, 16, _tile_twin, lambda P, Lpp: _solve_tiles(P, Lpp, 4))


def twin_chol(A, tb):
    """float64, right-looking, 128 columns at a time: the diagonal block by leaf_twin, the panel solve by a product with the explicit
    inverse of the block (tb = 128) or by substitution over its 16-column tiles with the tile inverses (tb = 16), one update of
    everything to the right.  The diagonal block is leaf_twin and not LAPACK's Cholesky because the rows INSIDE a diagonal block are
    solved with explicit 4 x 4 inverses on the device, which costs backward error that a substitution does not have (G, n = 129:
    beta = 113 against 1.7)."""
    if tb not in (16, TILE):
        raise ValueError("tb is 16 or 128")
    A = np.asarray(A, dtype=np.float64)
    M = np.tril(A) + np.tril(A, -1).T
    if tb == TILE:
        return _right_looking(M, TILE, leaf_twin, lambda P, Lkk: P @ ref._tri_inv(Lkk).T)
    return _right_looking(M, TILE, leaf_twin, lambda P, Lkk: _solve_tiles(P, Lkk, 16))


# ---- the measures -----------------------------------------------------------------------------------------------------------------
def edge_rows(n, bounds=(), seed=0):
    """at most 24 sorted row indices: 0, 1, 15, 16, 17, 127, 128, 129 (both sides of the first tile and block boundaries), n - 2, n - 1,
    the rows on both sides of every panel boundary in `bounds`, and seeded random ones"""
    if n <= 0:
        raise ValueError("n must be positive")
    want = min(n, MAX_ROWS)
    fixed = [0, 1, 15, 16, 17, 127, 128, 129, n - 2, n - 1]
    for b in bounds:
        fixed += [b - 1, b + 1]
    rows = []
    for r in fixed:
        if 0 <= r < n and r not in rows and len(rows) < want:
            rows.append(int(r))
    if len(rows) < want:
        for r in np.random.default_rng(7919 * n + seed).permutation(n):
            if len(rows) >= want:
                break
            if int(r) not in rows:
                rows.append(int(r))
    return sorted(rows)


def _low_ld(L):
    return np.asarray(np.tril(np.asarray(L)), dtype=LD)


def beta_parts(A, L, rows, ncols=None):
    """(the componentwise backward error of the whole diagonal, an array with that of each complete row of `rows`, entries j <= i), in
    units of eps; (inf, infs) when L is not finite.  An entry whose |L||L|^T is 0 counts 0 where A is met exactly and inf where not.
    ncols: only the entries of the first ncols columns (a factored panel: they need those columns of L only)."""
    rows = list(rows)
    Ll = _low_ld(L)
    n = Ll.shape[0]
    w = n if ncols is None else ncols
    if not np.all(np.isfinite(Ll[:, :w])):
        return float("inf"), np.full(len(rows), np.inf)
    Al = np.asarray(np.tril(np.asarray(A)), dtype=LD)
    Lab = np.abs(Ll)

    def ratio(num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0.0, np.inf))
        return float(np.max(r))

    den = np.sum(Ll[:w, :w] * Ll[:w, :w], axis=1)
    diag = ratio(np.abs(np.diagonal(Al)[:w] - den), den)
    per = np.zeros(len(rows))
    for k, i in enumerate(rows):
        m = min(i + 1, w)
        prod = Ll[:m, :m] @ Ll[i, :m]
        den = Lab[:m, :m] @ Lab[i, :m]
        per[k] = ratio(np.abs(Al[i, :m] - prod), den)
    return diag / EPS, per / EPS


def beta(A, L, rows, ncols=None):
    """the componentwise backward error in units of eps over the complete rows `rows` and the whole diagonal (beta_parts)"""
    diag, per = beta_parts(A, L, rows, ncols)
    return max(diag, float(np.max(per))) if len(per) else diag


def phi(L, Lhat, ncols=None):
    """the largest relative 2-norm error of a row of the lower triangle, over all rows; inf when L is not finite.  ncols: the rows of
    the first ncols columns only (a factored panel)."""
    Ll = _low_ld(L)
    if Ll.shape != Lhat.shape:
        raise ValueError(f"shapes differ: {Ll.shape} and {Lhat.shape}")
    Ll, Lh = Ll[:, :ncols], Lhat[:, :ncols]
    if not np.all(np.isfinite(Ll)):
        return float("inf")
    num = np.sqrt(np.sum((Ll - Lh) ** 2, axis=1))
    den = np.sqrt(np.sum(Lh ** 2, axis=1))
    return float(np.max(num / den))


def logdet_ld(Lhat, nlog=None):
    return LD(2) * np.sum(np.log(np.diagonal(Lhat)[:nlog]))


def lam(L, Lhat, nlog=None):
    d = np.asarray(np.diagonal(np.asarray(L))[:nlog], dtype=LD)
    if not np.all(d > 0):
        return float("inf")
    return float(abs(LD(2) * np.sum(np.log(d)) - logdet_ld(Lhat, nlog)))


def lam_value(value, Lhat, nlog=None):
    """a log-determinant computed elsewhere against that of Lhat"""
    return float(abs(LD(value) - logdet_ld(Lhat, nlog))) if np.isfinite(value) else float("inf")


def lam_floor(Lhat, nlog=None):
    """the rounding of n logarithms and of their sum: eps (n + sum |log Lhat_ii|)"""
    d = np.diagonal(Lhat)[:nlog]
    return EPS * float(len(d) + np.sum(np.abs(np.log(d))))


def max_block_cond(Lhat):
    """max_k cond_2 of the 128 x 128 diagonal blocks of Lhat (what a product with their explicit inverses pays)"""
    n = Lhat.shape[0]
    worst = 1.0
    for k0 in range(0, n, TILE):
        s = np.linalg.svd(np.asarray(Lhat[k0:k0 + TILE, k0:k0 + TILE], dtype=np.float64), compute_uv=False)
        worst = max(worst, float(s[0] / s[-1]))
    return worst


# ---- references, computed once per process and never modified ---------------------------------------------------------------------
class Reference:
    """one matrix A (float64), Lhat = chol_ld(A), cond_2(A), and -- as the tests ask -- the float64 factors of scipy's LAPACK and of
    both twins with their phi, lam and (per set of rows) beta"""

    def __init__(self, A, Lhat=None, cond=None):
        self.A = A
        self.n = A.shape[0]
        self.Lhat = chol_ld(A) if Lhat is None else Lhat
        self.cond = cond2(A) if cond is None else cond
        for a in (self.A, self.Lhat):
            a.setflags(write=False)
        self._factors, self._beta, self._phi, self._lam = {}, {}, {}, {}
        self._bcond = None

    def factor(self, which):
        """'scipy', 16 or 128"""
        if which not in self._factors:
            if which == "scipy":
                import scipy.linalg as sla
                F = np.tril(sla.cholesky(self.A, lower=True))
            else:
                F = twin_chol(self.A, which)
            F.setflags(write=False)
            self._factors[which] = F
        return self._factors[which]

    def beta(self, which, rows, ncols=None):
        key = (which, tuple(rows), ncols)
        if key not in self._beta:
            self._beta[key] = beta(self.A, self.factor(which), rows, ncols)
        return self._beta[key]

    def phi(self, which, ncols=None):
        if (which, ncols) not in self._phi:
            self._phi[(which, ncols)] = phi(self.factor(which), self.Lhat, ncols)
        return self._phi[(which, ncols)]

    def lam(self, which, nlog=None):
        if (which, nlog) not in self._lam:
            self._lam[(which, nlog)] = lam(self.factor(which), self.Lhat, nlog)
        return self._lam[(which, nlog)]

    def block_cond(self):
        if self._bcond is None:
            self._bcond = max_block_cond(self.Lhat)
        return self._bcond

    # the derived caps
    def cap_beta(self, explicit):
        return 2.0 * (self.n + 1) * (self.block_cond() if explicit else 1.0)

    def cap_phi(self):
        return 64 * EPS * self.cond

    def cap_lam(self):
        return self.n * EPS * self.cond


_REFS = {}


def reference(fam, n):
    """the Reference of a family's matrix.  Lhat of a scaled family is D Lhat(G), which IS chol_ld of the scaled matrix (every operation
    of chol_ld scales exactly by a power of two: tests/test_chol_ref.py proves it); its bars are those of G (beta and phi are invariant
    under the scaling), so cond is cond_2(G)."""
    key = (fam, n)
    if key not in _REFS:
        D = row_scale(fam, n)
        if D is None:
            _REFS[key] = Reference(matrix(fam, n))
        else:
            g = reference("G", n)
            _REFS[key] = Reference(matrix(fam, n), Lhat=np.asarray(D, dtype=LD)[:, None] * g.Lhat, cond=g.cond)
    return _REFS[key]
