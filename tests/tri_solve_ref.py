"""An extended-precision reference for the triangular solves (a helper module of the tests, not a conftest): numpy only, no GPU.

fwd_ld / bwd_ld / potrs_ld: row-by-row substitution in numpy.longdouble (64-bit mantissa on x86-64, about 2000 times finer than the
doubles it judges).  The inputs are float64 and are taken as given: the result is the solution of exactly that system up to
longdouble rounding, so it can judge a float64 solve of any algorithm.

The factor families, deterministic from (n, seed):

    W   well conditioned: diagonal 1 + U(0, 1), strict lower part 0.02 N(0, 1) / sqrt(n) (the factor of
        test_gpu_primitives.test_forward_sweep_in_one_launch); cond_2 = 2.0 at n = 2432
    G   covariance factor: numpy's Cholesky factor of exp(-|x - x'|^2 / (2 l^2)) + noise I on n uniform points of the unit square;
        the diagonal falls from 1 to about sqrt(noise).  (l = 0.05 at n = 2432 and l = 0.1 at n = 700, noise 1e-6: cond_2 about 6e3;
        the harder one, n = 2432, l = 0.1, noise 1e-8: about 1.2e5)
    S   scaled: D L_W and D B with D a diagonal of powers of two 2^-20 .. 2^20.  Scaling by a power of two is exact, so
        (D L_W) y = D B has the solution of L_W y = B, and (D L_W)(D L_W)^T x = D B has x = D^-1 (L_W L_W^T)^-1 B -- in floating point
        too when the order of the sums does not depend on the data.

blockinv_fwd / blockinv_bwd: a float64 numpy twin of the device algorithm -- left-looking block substitution with EXPLICIT inverses of
the nb-wide diagonal blocks (nb = 128: the leaf inverses; nb = 1024: built from them by the doubling recurrence
inv [[A, 0], [C, B]] = [[inv A, 0], [-inv(B) C inv(A), inv B]], the last block of a width that is no power of two in pairs whose second
half is the narrower one, as csrc/api.hip ensure_winv does).  It shows what float64 arithmetic of that algorithm attains, so the bar
the device is held to never comes from the device.

col_err: per-column 2-norm relative error.  edge_columns: the at most 32 columns that are checked in longdouble."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)
TILE = 128


# ---- substitution in extended precision ----------------------------------------------------------------------------------------
def _as2d(B, n):
    B = np.asarray(B)
    if B.dtype not in (np.float64, LD):
        raise TypeError("right-hand sides must be float64 (or an intermediate in longdouble)")
    B2 = B.reshape(n, -1)
    return np.array(B2, dtype=LD), B.shape


def _lower(L):
    L = np.asarray(L)
    if L.dtype != np.float64 or L.ndim != 2 or L.shape[0] != L.shape[1]:
        raise TypeError("the factor must be a square float64 array")
    return np.asarray(np.tril(L), dtype=LD)


def fwd_ld(L, B):
    """L Y = B by forward substitution in longdouble; only the lower triangle of L is read"""
    Ll = _lower(L)
    n = Ll.shape[0]
    X, shape = _as2d(B, n)
    for i in range(n):
        if i:
            X[i] -= Ll[i, :i] @ X[:i]
        X[i] /= Ll[i, i]
    return X.reshape(shape)


def bwd_ld(L, B):
    """L^T X = B by backward substitution in longdouble; only the lower triangle of L is read"""
    Ll = _lower(L)
    n = Ll.shape[0]
    X, shape = _as2d(B, n)
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            X[i] -= Ll[i + 1:, i] @ X[i + 1:]
        X[i] /= Ll[i, i]
    return X.reshape(shape)


def potrs_ld(L, B):
    """(L L^T) X = B; the intermediate stays in longdouble"""
    return bwd_ld(L, fwd_ld(L, B))


# ---- the factor families --------------------------------------------------------------------------------------------------------
def factor_w(n, seed):
    rng = np.random.default_rng(seed)
    L = np.tril(0.02 * rng.standard_normal((n, n)) / np.sqrt(n), -1)
    L[np.arange(n), np.arange(n)] = 1.0 + rng.random(n)
    return L


def covariance_g(n, seed, ell, noise):
    """the RBF covariance exp(-|x - x'|^2 / (2 l^2)) + noise I on n uniform points of the unit square (symmetric in its bits); shared
    with tests/chol_ref.py, whose fixtures are this matrix before it is factored"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 2))
    sq = np.sum(x * x, axis=1)
    r2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)
    K = np.exp(-r2 / (2.0 * ell * ell))
    K = 0.5 * (K + K.T)
    K[np.arange(n), np.arange(n)] = 1.0 + noise
    return K


def factor_g(n, seed, ell, noise):
    return np.linalg.cholesky(covariance_g(n, seed, ell, noise))


def scaling_s(n, seed):
    """the diagonal of D: powers of two 2^-20 .. 2^20"""
    rng = np.random.default_rng(seed + 7919)
    return np.ldexp(1.0, rng.integers(-20, 21, n))


def cond2(L):
    s = np.linalg.svd(L, compute_uv=False)
    return float(s[0] / s[-1])


def rhs(n, nrhs, seed):
    return np.random.default_rng(1000003 * seed + n).standard_normal((n, nrhs))


# ---- the float64 twin of the device algorithm -----------------------------------------------------------------------------------
def _tri_inv(A):
    """inverse of a lower-triangular block by substitution on the identity (float64)"""
    m = A.shape[0]
    X = np.eye(m)
    for i in range(m):
        if i:
            X[i] -= A[i, :i] @ X[:i]
        X[i] /= A[i, i]
    return X


def block_inverses(L, nb):
    """the inverses of the nb-wide diagonal blocks of L (the last one narrower), list of arrays: 128-blocks by substitution, wider ones
    by doubling from them.  A block of a width that is no power-of-two multiple of 128 is doubled in pairs (A: hs wide, B: what is
    left, at most hs) from its left edge, so its last pair has a narrower second half."""
    n = L.shape[0]
    if nb % TILE or nb & (nb - 1):
        raise ValueError("nb must be a power-of-two multiple of 128")
    out = []
    for J0 in range(0, n, nb):
        w = min(nb, n - J0)
        A = L[J0:J0 + w, J0:J0 + w]
        W = np.zeros((w, w))
        for k0 in range(0, w, TILE):
            k1 = min(w, k0 + TILE)
            W[k0:k1, k0:k1] = _tri_inv(A[k0:k1, k0:k1])
        hs = TILE
        while hs < nb:
            for s in range(0, w, 2 * hs):
                if s + hs >= w:
                    continue
                e = min(w, s + 2 * hs)
                T = A[s + hs:e, s:s + hs] @ W[s:s + hs, s:s + hs]
                W[s + hs:e, s:s + hs] = -(W[s + hs:e, s + hs:e] @ T)
            hs *= 2
        out.append(W)
    return out


def blockinv_fwd(L, B, nb):
    """L Y = B in float64: block J receives everything to its left in one product, then one product with inv(L_JJ)"""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = L.shape[0]
    X = np.array(np.asarray(B, dtype=np.float64).reshape(n, -1))
    for W, J0 in zip(block_inverses(L, nb), range(0, n, nb)):
        J1 = min(n, J0 + nb)
        t = X[J0:J1]
        if J0:
            t = t - L[J0:J1, :J0] @ X[:J0]
        X[J0:J1] = W @ t
    return X.reshape(np.shape(B))


def blockinv_bwd(L, B, nb):
    """L^T X = B in float64, from the last block to the first: block J receives everything below it, then inv(L_JJ)^T"""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = L.shape[0]
    X = np.array(np.asarray(B, dtype=np.float64).reshape(n, -1))
    inv = block_inverses(L, nb)
    for W, J0 in reversed(list(zip(inv, range(0, n, nb)))):
        J1 = min(n, J0 + nb)
        t = X[J0:J1]
        if J1 < n:
            t = t - L[J1:, J0:J1].T @ X[J1:]
        X[J0:J1] = W.T @ t
    return X.reshape(np.shape(B))


def blockinv_potrs(L, B, nb):
    return blockinv_bwd(L, blockinv_fwd(L, B, nb), nb)


# ---- the measure ----------------------------------------------------------------------------------------------------------------
def col_err(got, ref):
    """(per-column ||got - ref||_2 / ||ref||_2 as float64, its maximum); the difference is formed in longdouble.  A column whose
    reference is 0 counts 0 where it is met exactly and inf where not."""
    got = np.asarray(got, dtype=LD)
    ref = np.asarray(ref, dtype=LD)
    if got.shape != ref.shape:
        raise ValueError(f"shapes differ: {got.shape} and {ref.shape}")
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    num = np.sqrt(np.sum((got - ref) ** 2, axis=0))
    den = np.sqrt(np.sum(ref ** 2, axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0.0, np.inf))
    e = np.asarray(e, dtype=np.float64)
    return e, float(np.max(e)) if e.size else 0.0


def edge_columns(nrhs, seed=0):
    """at most 32 sorted column indices: the first and last column, the columns on both sides of the 16-, 64- and 128-column
    boundaries and of the middle (where a sweep is cut in two halves), and seeded random ones"""
    if nrhs <= 0:
        raise ValueError("nrhs must be positive")
    fixed = [0, 1, 15, 16, 63, 64, 127, 128, nrhs // 2 - 1, nrhs // 2, nrhs - 1]
    cols = {c for c in fixed if 0 <= c < nrhs}
    want = min(nrhs, 32)
    if len(cols) < want:
        rng = np.random.default_rng(977 * nrhs + seed)
        for c in rng.permutation(nrhs):
            if len(cols) >= want:
                break
            cols.add(int(c))
    return sorted(cols)


# ---- the fixtures the device tests use ------------------------------------------------------------------------------------------
SEED = 18
NOISE = 1e-6
# family -> allowed cond_2 at n >= 700 (tests/test_tri_solve_ref.py asserts it: the bars of the device tests rest on it)
COND_RANGE = {"W": (1.5, 3.0), "G": (2e3, 2e4), "H": (5e4, 5e5)}
VEC_N = (1, 100, 128, 129, 700)                 # vector path (1 .. 8 right-hand sides)
GEMM_N = (100, 700, 1300)                       # block substitution below 2048 rows
SWEEP_CASES = (("G", 2048), ("G", 2177), ("G", 2432), ("W", 2432), ("H", 2432))      # transposed sweep
POTRI_N = (129, 700, 1300)
GPU_FIXTURES = tuple(sorted({(f, n) for f in "WG" for n in VEC_N + GEMM_N + POTRI_N} | set(SWEEP_CASES)))

_FIXTURES = {}


def fixture(fam, n):
    """(L, cond_2(L)) of family W, G (length scale 0.05 from 2048 rows, 0.1 below; noise 1e-6) or H (the harder G: 0.1, 1e-8), computed
    once per process and read-only"""
    key = (fam, n)
    if key not in _FIXTURES:
        if fam == "W":
            L = factor_w(n, SEED)
        elif fam == "G":
            L = factor_g(n, SEED, 0.05 if n >= 2048 else 0.1, NOISE)
        elif fam == "H":
            L = factor_g(n, SEED, 0.1, 1e-8)
        else:
            raise KeyError(fam)
        L.setflags(write=False)
        _FIXTURES[key] = (L, cond2(L))
    return _FIXTURES[key]
