"""An extended-precision reference for the posterior (a helper module of the tests, not a conftest): numpy only, no GPU.

The inputs are taken as given: the reference is the exact posterior of the float64 numbers the device receives -- x, theta, the lower
triangle of L, alpha, xpred -- not of the unrounded problem, so every device error measured against it is the posterior's own:

    k    = kernel_family_ref.k_ref(x, xpred)  in longdouble (64-bit mantissa on x86-64)          k** = k_ref(xpred, xpred)
    w    = L^-1 k    row-by-row substitution in longdouble on the float64 L widened (tri_solve_ref.fwd_ld, all columns at once)
    m    = k^T alpha        S = k** - w^T w        v = diag S

The fixtures, deterministic from (family, n): x = default_rng(5).random((n, d)), sigma^2 = 1.7,

    B    rbf_ard, d = 2, l = 0.35, noise 0.01      the benign values of the older posterior tests
    G    rbf_ard, d = 2, l = 0.05, noise 1e-6      (the covariance of chol_ref's G times 1.7, noise unscaled)
    H    rbf_ard, d = 2, l = 0.1,  noise 1e-8      the harder one
    M    matern52_iso, d = 3, l = 0.1, noise 1e-4  the variance's base is sigma^2 for another radial kind

L is the rounded chol_ref.chol_ld of the float64 K + noise I (K = k_ref in float64, symmetric in its bits), alpha the rounded
tri_solve_ref.potrs_ld(L, y) for a smooth y of up to 128 columns.

The prediction points of a case come in five classes, point p being of class CLASSES[p % 5] (so every call with five or more points
holds every class, next to every edge of the sample):

    rand    from the unit cube
    data    an exact copy of a data point: the variance sigma^2 - |L^-1 k|^2 cancels down to about the noise
    near    a data point plus 1e-7 in every coordinate
    far     the unit cube shifted by +50: k underflows to 0, the exact answer is mean 0, variance sigma^2, S = k** among them
    mid     the midpoint of two data points

sample_points: the at most 64 points the longdouble reference covers when a call has many.  The device is called with all of them.

The float64 twins -- the same formulas in float64 with k_ref(dtype=float64) -- show what double arithmetic of each algorithm attains, so
the bar the device is held to never comes from the device: (a) substitution by scipy.linalg.solve_triangular, (b)
tri_solve_ref.blockinv_fwd at the block width nb of the route (128: the one-point sweep and block_inverses = 0; 2048 up to 1024 points and
1024 beyond: at a padded size up to nb that is ONE product with the explicit inverse of the whole factor, which LAPACK's substitution
does not model).

The measures, all in longdouble, the worst of each class (sigma^2 = theta[0], eps = 2^-52):

    mu     |m - m_ref| / (eps (sum_i |k_pi| |alpha_i| + sigma^2 sum_i |alpha_i|))     the second term: the project's bar on a kernel
                                                                                     entry is absolute, k_bound_ulps(d) eps sigma^2
    nu     |v - v_ref| / (eps sigma^2)
    sig    |S_pq - S_ref,pq| / (eps (|w_p| |w_q| + sigma^2))   over the sampled pairs, a pair counted under the classes of both points"""
import numpy as np

import chol_ref
import kernel_family_ref as kf
import tri_solve_ref as ts

LD = ts.LD
EPS = ts.EPS
TILE = 128
SEED = 5
SIG = 1.7
MAX_COLS = 128
VEC_COLS = 8
MAX_SAMPLE = 64
CLASSES = ("rand", "data", "near", "far", "mid")
MEASURES = ("mu", "nu", "sig")
# family -> (kernel, d, length scale, noise)
FAMILY = {"B": ("rbf_ard", 2, 0.35, 1e-2), "G": ("rbf_ard", 2, 0.05, 1e-6), "H": ("rbf_ard", 2, 0.1, 1e-8),
          "M": ("matern52_iso", 3, 0.1, 1e-4)}
# cond_2(L) of the fixtures, measured on the host (tests/test_posterior_ref.py asserts a band of 30 % around each: the caps of the
# device tests rest on them)
COND = {("B", 1): 1.0, ("B", 2): 1.27, ("B", 127): 95.5, ("B", 128): 95.6, ("B", 129): 95.9, ("B", 255): 135.0, ("B", 300): 147.0,
        ("B", 700): 224.0, ("B", 1300): 305.0,
        ("G", 1): 1.0, ("G", 2): 1.0, ("G", 127): 73.9, ("G", 128): 73.9, ("G", 129): 73.9, ("G", 255): 465.0, ("G", 300): 500.0,
        ("G", 700): 4.95e3, ("G", 1300): 6.45e3,
        ("H", 129): 1.25e3, ("H", 300): 5.71e4, ("H", 700): 8.69e4, ("H", 1300): 1.16e5,
        ("M", 300): 16.5}
# the floor of the bars, in the units of each measure: the smallest whole number, 4 at the least, under which scipy's float64
# substitution (twin (a)) alone stays in every class on the benign family B, over every size of GPU_N and the calls of
# tests/test_posterior_ref.py HOST_P.  Measured worst: mu 0.38 (n = 1), nu 5.44 (n = 128), sig 5.83 (n = 1300).
# tests/test_posterior_ref.py asserts that twin (a) passes it and that a floor above 4 less one would fail.
FLOOR = {"mu": 4.0, "nu": 6.0, "sig": 6.0}
MARGIN = 8.0            # a differently ordered float64 sum: the margin of the triangular-solve and Cholesky suites
# the sizes the device tests use (tests/test_posterior_ref.py proves the reference on the small ones and the conditions on all)
GPU_N = (1, 2, 127, 128, 129, 255, 300, 700, 1300)
H_N = (129, 300, 700, 1300)


def theta_of(fam):
    name, d, ell, _ = FAMILY[fam]
    return np.array([SIG] + [ell] * (kf.n_theta(name, d) - 1))


def smooth_y(x, ncol=MAX_COLS):
    """a smooth function of x per column, of order one: products of slow sines whose frequency and phase move with the column"""
    c = np.arange(ncol)[None, :]
    s = np.sum(x, axis=1)[:, None]
    return np.sin((1.0 + 0.05 * c) * 3.0 * x[:, :1] + 0.3 * c) * np.cos((2.0 - 0.01 * c) * s) + 0.1 * c / ncol


class Fixture:
    """one (family, n): x, theta, K + noise I, L (float64, lower), cond_2(L), alpha (n, up to 128 columns), all read-only"""

    def __init__(self, fam, n):
        self.fam, self.n = fam, n
        self.kernel, self.d, _, self.noise = FAMILY[fam]
        self.theta = theta_of(fam)
        self.x = np.random.default_rng(SEED).random((n, self.d))
        K = kf.k_ref(self.kernel, self.x, self.x, self.theta, dtype=np.float64)
        assert np.array_equal(K, K.T)
        self.KV = K + self.noise * np.eye(n)
        self.Lhat = chol_ref.chol_ld(self.KV)
        self.L = np.asarray(self.Lhat, dtype=np.float64)
        self.cond = ts.cond2(self.L)
        self.y = smooth_y(self.x)
        self._alpha = {}
        for a in (self.theta, self.x, self.KV, self.Lhat, self.L, self.y):
            a.setflags(write=False)

    def alpha(self, ncol=VEC_COLS):
        """(n, ncol) float64: the rounded potrs_ld(L, y[:, :ncol]).  Solved 8 or 128 columns at a time (a column's solution does not depend
        on its neighbours), so that the large fixtures, which only ever need 8, do not pay for 128"""
        width = VEC_COLS if ncol <= VEC_COLS else MAX_COLS
        if width not in self._alpha:
            a = np.asarray(ts.potrs_ld(self.L, self.y[:, :width]), dtype=np.float64)
            a.setflags(write=False)
            self._alpha[width] = a
        return self._alpha[width][:, :ncol]

    def cap_solve(self):
        """nu and sig: the triangular-solve cap 64 cond_2(L) (in eps), which enters the variance through 2 w^T dw"""
        return 64.0 * self.cond


_FIXTURES = {}


def fixture(fam, n):
    key = (fam, n)
    if key not in _FIXTURES:
        _FIXTURES[key] = Fixture(fam, n)
    return _FIXTURES[key]


# ---- prediction points ------------------------------------------------------------------------------------------------------------
def class_of(p):
    return CLASSES[p % len(CLASSES)]


def points(fx, P, seed=0, first=0):
    """(xpred (P, d), list of class names): point p is of class CLASSES[(first + p) % 5]"""
    rng = np.random.default_rng(7919 * fx.n + 31 * P + seed)
    n, d = fx.n, fx.d
    xp = np.empty((P, d))
    cls = []
    for p in range(P):
        c = class_of(first + p)
        j, k = int(rng.integers(n)), int(rng.integers(n))
        u = rng.random(d)
        if c == "rand":
            xp[p] = u
        elif c == "data":
            xp[p] = fx.x[j]
        elif c == "near":
            xp[p] = fx.x[j] + 1e-7
        elif c == "far":
            xp[p] = u + 50.0
        else:
            xp[p] = 0.5 * (fx.x[j] + fx.x[k])
        cls.append(c)
    xp.setflags(write=False)
    return xp, cls


def sample_points(P, seed=0):
    """at most 64 sorted point indices: the first five (one of every class), the last point, the points on both sides of every
    multiple of 128 (the tiles of S, the halves of a sweep in two; padded_dim(P) / 2 is one of them), and seeded random ones up to
    min(P, 40)"""
    if P <= 0:
        raise ValueError("P must be positive")
    Pp = -(-P // TILE) * TILE
    fixed = [0, P - 1, Pp // 2 - 1, Pp // 2]
    for b in range(TILE, Pp + 1, TILE):
        fixed += [b - 1, b]
    fixed += [1, 2, 3, 4]
    idx = []
    for p in fixed:
        if 0 <= p < P and p not in idx and len(idx) < MAX_SAMPLE:
            idx.append(int(p))
    want = min(P, 40)
    if len(idx) < want:
        for p in np.random.default_rng(977 * P + seed).permutation(P):
            if len(idx) >= want:
                break
            if int(p) not in idx:
                idx.append(int(p))
    return sorted(idx)


# ---- the posterior in extended precision and its float64 twins ---------------------------------------------------------------------
def posterior_ld(fx, xs, ncol=VEC_COLS):
    """(m (s, ncol), v (s,), S (s, s), w (n, s), k (n, s)) in longdouble for the points xs"""
    k = kf.k_ref(fx.kernel, fx.x, xs, fx.theta)
    kss = kf.k_ref(fx.kernel, xs, xs, fx.theta)
    w = ts.fwd_ld(fx.L, k)
    m = k.T @ np.asarray(fx.alpha(ncol), dtype=LD)
    S = kss - w.T @ w
    return m, np.diagonal(S).copy(), S, w, k


def posterior_ld_potrs(fx, xs):
    """the second formulation: S = k** - k^T (K + V)^-1 k through potrs_ld"""
    k = kf.k_ref(fx.kernel, fx.x, xs, fx.theta)
    kss = kf.k_ref(fx.kernel, xs, xs, fx.theta)
    return kss - k.T @ ts.potrs_ld(fx.L, k)


def posterior_twin(fx, xs, nb=None, ncol=VEC_COLS):
    """(m, v, S) in float64: nb None -- substitution by scipy's LAPACK (twin (a)); else tri_solve_ref.blockinv_fwd at block width nb
    (twin (b))"""
    k = kf.k_ref(fx.kernel, fx.x, xs, fx.theta, dtype=np.float64)
    kss = kf.k_ref(fx.kernel, xs, xs, fx.theta, dtype=np.float64)
    if nb is None:
        import scipy.linalg as sla
        w = sla.solve_triangular(fx.L, k, lower=True)
    else:
        w = ts.blockinv_fwd(fx.L, k, nb)
    m = k.T @ fx.alpha(ncol)
    S = kss - w.T @ w
    return m, fx.theta[0] - np.sum(w * w, axis=0), S


def w_norms(fx, xs):
    """|L^-1 k_p|_2 of every point of xs in float64 by scipy's substitution: the denominators of sig where all points are compared"""
    import scipy.linalg as sla
    k = kf.k_ref(fx.kernel, fx.x, xs, fx.theta, dtype=np.float64)
    return np.sqrt(np.sum(sla.solve_triangular(fx.L, k, lower=True) ** 2, axis=0))


# ---- the measures ------------------------------------------------------------------------------------------------------------------
def _worst(err, den, cls, axis_cls):
    """worst err / den per class; err, den longdouble arrays whose axis 0 (and axis 1 if axis_cls == 2) runs over the points"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(r), r, np.inf)
    out = {}
    cls = np.asarray(cls)
    for c in CLASSES:
        sel = cls == c
        if not np.any(sel):
            continue
        part = r[sel]
        if axis_cls == 2:
            part = np.maximum(part, r[:, sel].T) if part.size else part
        out[c] = float(np.max(part)) if part.size else 0.0
    return out


class Reference:
    """the longdouble posterior of the sampled points of one call, the denominators of the measures and (as asked) the figures of
    the twins; cls: the classes of the sampled points"""

    def __init__(self, fx, xs, cls, ncol=VEC_COLS):
        self.fx, self.xs, self.cls, self.ncol = fx, np.asarray(xs), list(cls), ncol
        self.m, self.v, self.S, self.w, self.k = posterior_ld(fx, self.xs, ncol)
        sig = LD(fx.theta[0])
        a = np.abs(np.asarray(fx.alpha(ncol), dtype=LD))
        self.den_mu = LD(EPS) * (np.abs(self.k).T @ a + sig * np.sum(a, axis=0)[None, :])
        self.den_nu = LD(EPS) * sig
        wn = np.sqrt(np.sum(self.w * self.w, axis=0))
        self.den_sig = LD(EPS) * (np.outer(wn, wn) + sig)
        self._twin = {}

    def measure(self, m=None, v=None, S=None, cols=None):
        """{measure: {class: worst}} of the outputs given (m (s, c), v (s,), S (s, s)); cols: the columns of the reference m holds"""
        out = {}
        if m is not None:
            cols = slice(None) if cols is None else cols
            m = np.asarray(m, dtype=LD).reshape(len(self.cls), -1)
            e = np.abs(m - self.m[:, cols])
            r = np.max(np.where(np.isfinite(e), e, np.inf) / self.den_mu[:, cols], axis=1)
            out["mu"] = _worst(r, np.ones_like(r), self.cls, 1)
        if v is not None:
            e = np.abs(np.asarray(v, dtype=LD) - self.v)
            out["nu"] = _worst(e, np.full(e.shape, self.den_nu), self.cls, 1)
        if S is not None:
            e = np.abs(np.asarray(S, dtype=LD) - self.S)
            out["sig"] = _worst(e, self.den_sig, self.cls, 2)
        return out

    def twin(self, nb):
        """the measures of twin (a) (nb None) or (b) at block width nb"""
        if nb not in self._twin:
            m, v, S = posterior_twin(self.fx, self.xs, nb, self.ncol)
            self._twin[nb] = self.measure(m, v, S)
        return self._twin[nb]

    def bars(self, nb):
        """{measure: {class: 8 max(twin (a), twin (b) at nb, floor)}}"""
        a, b = self.twin(None), self.twin(nb)
        return {q: {c: MARGIN * max(a[q][c], b[q][c], FLOOR[q]) for c in a[q]} for q in MEASURES}


def mu_cap(fx, depth):
    """mu <= k_bound_ulps(d) for the rounded kernel entries plus the depth of the route's summation"""
    return kf.k_bound_ulps(fx.d) + depth
