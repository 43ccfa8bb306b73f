"""An extended-precision reference of the second derivatives of the native kernel family and of the Hessian of the negative log
marginal likelihood (a helper module of the tests, not a conftest), written in numpy.longdouble from the closed forms below on top of
kernel_family_ref and loo_ref's linear algebra -- not from the device code (csrc/hessian.hip, csrc/radial.h).

kernel_family_ref's notation: D_k = x1_ik - x2_jk, s = theta[0], r^2 = sum_k (D_k / l_k)^2, phi and cf as tabulated there.  The one new
radial factor is c2 = -(1 / r) dcf/dr:

    kind       c2(r)
    rbf        s exp(-r^2 / 2)                 (= cf)
    matern32   3 sqrt3 s exp(-sqrt3 r) / r
    matern52   25/3 s exp(-sqrt5 r)

    d2k/ds2       = 0
    d2k/ds dl_k   = (cf / s) D_k^2 / l_k^3
    d2k/dl_k dl_m = c2 D_k^2 D_m^2 / (l_k^3 l_m^3) - 3 delta_km cf D_k^2 / l_k^4
    isotropic     : d2k/dl2 = c2 r^4 / l^2 - 3 cf r^2 / l^2          (the sums over the dimensions)

Matern 3/2's c2 D_k^2 D_m^2 goes to zero like r^3: a coincident pair contributes exactly 0 (the product is formed as
(3 sqrt3 s exp(-sqrt3 r)) * (D_k^2 D_m^2 / r) with 0 where r = 0).

With f = -log p(y|theta), KV = K + V, W = KV^-1, b = W (y - m), K_i = dK/dtheta_i, K_ij = d2K/dtheta_i dtheta_j, T_i = W K_i:

    g_i  = 1/2 sum_ab (W - b b^T)_ab (K_i)_ab
    H_ij = 1/2 sum_ab (W - b b^T)_ab (K_ij)_ab - [ 1/2 tr(G_i K_j) - b^T K_j w_i ],     G_i = W K_i W,  w_i = W K_i b = T_i b
    tr(G_i K_j) = tr(T_i T_j) = sum_ab (T_i)_ab (T_j)_ba

A kind without an entry in _C2 raises KeyError: a new kernel fails every test that needs its Hessian until its formula stands here.

Below the cases of the device tests: the second-derivative pass and the bracket each on its own (pass_reference, bracket_reference),
with the derived bounds they are held to (hess_trace_bound_factor, bracket_bound_factors) and their float64 twins."""
import functools

import numpy as np

import kernel_family_ref as kf
import loo_ref

LD = np.longdouble


# kind -> (r, s, number type) -> c2 r  (c2 with ONE factor r taken out, finite at r = 0)
def _c2r_rbf(r, s, T):
    return s * np.exp(-r * r / T(2)) * r


def _c2r_matern32(r, s, T):
    return T(3) * np.sqrt(T(3)) * s * np.exp(-np.sqrt(T(3)) * r)


def _c2r_matern52(r, s, T):
    return T(25) / T(3) * s * np.exp(-np.sqrt(T(5)) * r) * r


_C2 = {"rbf": _c2r_rbf, "matern32": _c2r_matern32, "matern52": _c2r_matern52}


class _Second:
    """the pieces every second derivative of one (name, x1, x2, theta) shares; pair(i, j) -> (n1, n2)"""

    def __init__(self, name, x1, x2, theta, T):
        kind, self.iso = kf.FAMILY[name]
        self.T = T
        iso, self.s, self.ls, delta, self.phi, self.cf = kf._setup(name, x1, x2, theta, T)
        self.d = delta.shape[2]
        self.D2 = delta ** 2                                           # (n1, n2, d)
        r2 = np.sum(self.D2 / self.ls ** 2, axis=2)
        self.r = np.sqrt(r2)
        self.c2r = _C2[kind](self.r, self.s, T)
        self.nt = kf.n_theta(name, self.d)
        # e_k = D_k^2 / l_k^3 and e_k / r (0 on a coincident pair: e_k <= r^2 / l_k there, so e_k e_m / r -> 0)
        self.e = self.D2 / self.ls ** 3
        with np.errstate(divide="ignore", invalid="ignore"):
            self.e_over_r = np.where(self.r[:, :, None] > 0, self.e / self.r[:, :, None], T(0))

    def _ll(self, k, m):
        out = self.c2r * self.e_over_r[:, :, k] * self.e[:, :, m]
        if k == m:
            out = out - self.T(3) * self.cf * self.D2[:, :, k] / self.ls[k] ** 4
        return out

    def pair(self, i, j):
        if i > j:
            i, j = j, i
        if i == 0 and j == 0:
            return np.zeros_like(self.phi)
        if i == 0:
            dl = self.cf / self.s * (np.sum(self.e, axis=2) if self.iso else self.e[:, :, j - 1])
            return dl
        if self.iso:
            out = np.zeros_like(self.phi)
            for k in range(self.d):
                for m in range(self.d):
                    out = out + self._ll(k, m)
            return out
        return self._ll(i - 1, j - 1)


def d2k_dtheta2_ref(name, x1, x2, theta, dtype=LD):
    """d2K/dtheta_i dtheta_j, shape (n_theta, n_theta, n1, n2), in longdouble (dtype=np.float64: the same formulas in double)"""
    S = _Second(name, x1, x2, theta, dtype)
    out = np.empty((S.nt, S.nt) + S.phi.shape, dtype=dtype)
    for i in range(S.nt):
        for j in range(i, S.nt):
            out[i, j] = out[j, i] = S.pair(i, j)
    return out


def nll_hessian_ref(name, x, y_minus_m, V, theta, dtype=LD):
    """(gradient, raw Hessian) of the negative log marginal likelihood in the hyperparameters the kernel owns: raw[i] is built from
    T_i = W K_i and w_i = T_i b, as the formulas in the module's head state it; it is not symmetrised.  V: noise variances (n,) or a
    covariance (n, n).  dtype=np.float64: the same formulas in double."""
    x = np.asarray(x, dtype=dtype)
    r = np.asarray(y_minus_m, dtype=dtype).reshape(-1)
    nt = kf.n_theta(name, x.shape[1])
    theta = np.asarray(theta, dtype=dtype)[:nt]
    W = loo_ref.spd_inverse(loo_ref._kv(name, x, V, theta, dtype))
    W = (W + W.T) / dtype(2)
    b = W @ r
    B = W - np.outer(b, b)
    dK = kf.dk_dtheta_ref(name, x, x, theta, dtype)
    half = dtype(1) / dtype(2)
    grad = np.array([half * np.sum(B * dK[i]) for i in range(nt)], dtype=dtype)
    S = _Second(name, x, x, theta, dtype)
    T = [loo_ref.matmul(W, np.ascontiguousarray(dK[i])) for i in range(nt)]
    raw = np.zeros((nt, nt), dtype=dtype)
    for i in range(nt):
        w_i = T[i] @ b
        for j in range(nt):
            a_ij = half * np.sum(B * S.pair(i, j))
            raw[i, j] = a_ij - (half * np.sum(T[i] * T[j].T) - b @ (dK[j] @ w_i))
    return grad, raw


def nll_gradient_ref(name, x, y_minus_m, V, theta, dtype=LD):
    """the gradient alone (no second derivatives, no products): what test 2 differences"""
    x = np.asarray(x, dtype=dtype)
    r = np.asarray(y_minus_m, dtype=dtype).reshape(-1)
    nt = kf.n_theta(name, x.shape[1])
    theta = np.asarray(theta, dtype=dtype)[:nt]
    W = loo_ref.spd_inverse(loo_ref._kv(name, x, V, theta, dtype))
    b = W @ r
    B = W - np.outer(b, b)
    dK = kf.dk_dtheta_ref(name, x, x, theta, dtype)
    return np.array([np.sum(B * dK[i]) / 2 for i in range(nt)], dtype=dtype)


# ---- the cases of the device ABI test (tests/test_gpu_hessian.py) and of the host test that vets them --------------------------------
NAMES = list(kf.FAMILY)
# (kernel, n, d, ncol, component, duplicated rows or None)
ABI_CASES = ([(name, 300, 3, 1, 0, None) for name in NAMES]     # an interior off-diagonal tile, partial last tiles, padding to 384
             + [("rbf_ard", 96, 1, 1, 0, None),                 # one partial tile
                ("matern32_ard", 128, 2, 1, 0, None),           # no padding rows; Matern 3/2's 1 / r on the diagonal
                ("matern32_ard", 300, 3, 1, 0, (3, 7)),         # a duplicated point
                ("rbf_ard", 200, 5, 1, 0, None),                # the runtime-dimension path, its low end
                ("matern52_ard", 140, 16, 1, 0, None),          # ... and its high end: 17 rows of G
                ("rbf_ard", 1100, 2, 1, 0, None),               # two POTRI panels, a 9 x 9-tile product
                ("matern52_iso", 300, 3, 2, 1, None)])          # a second y column


# The sweep of every instantiation (tests/test_gpu_hessian_family.py, vetted by tests/test_hessian_host.py): every name x every d of
# kf.DIMS whose (name, d) ABI_CASES does not hold, built by that rule.  n = 261 is the smallest size with an interior tile strictly below
# the diagonal (tile (1, 0): the two-rows-per-trip path), partial edge tiles (tile row 2 has five rows), an odd n (a lane's second column
# falls past the end) and padding to 384.  The longdouble reference of the slowest case (d = 16, 17 hyperparameters) takes about a second,
# so d = 16 stays at n = 261 for every kind.
FAMILY_N = 261


def family_cases(held):
    """(name, FAMILY_N, d, 1, 0, None) for every (name, d) of the grid that no case of `held` (tuples (name, n, d, ...)) has"""
    have = {(c[0], c[2]) for c in held}
    return [(name, FAMILY_N, d, 1, 0, None) for name in NAMES for d in kf.DIMS if (name, d) not in have]


FAMILY_CASES = family_cases(ABI_CASES)


def case_inputs(name, n, d, ncol=1, dup=None, seed=None):
    """x, centred y, noise variances and theta, drawn the way tests/test_gpu_loo.py::_inputs draws them; dup = (i, j): row j of x
    is row i again"""
    rng = np.random.default_rng(31 * n + 7 * d + sorted(kf.FAMILY).index(name) if seed is None else seed)
    x = rng.random((n, d))
    theta = np.concatenate([[1.2], rng.uniform(0.3, 0.6, kf.n_theta(name, d) - 1)])
    y = np.stack([np.sin((3.0 + c) * x.sum(axis=1)) + 0.1 * rng.standard_normal(n) for c in range(ncol)], axis=1)
    V = rng.uniform(0.01, 0.02, n)
    if dup is not None:
        x[dup[1]] = x[dup[0]]
    return x, y - y.mean(axis=0), V, theta


@functools.lru_cache(maxsize=None)
def reference(name, n, d, ncol, comp, dup):
    """one ABI case's inputs and nll_hessian_ref on them in longdouble, computed once per process"""
    x, ym, V, theta = case_inputs(name, n, d, ncol, dup)
    grad, raw = nll_hessian_ref(name, x, ym[:, comp], V, theta)
    return (x, ym, V, theta), (grad, raw)


def hessian_bar(ref):
    """the project's gradient bar, for a Hessian: |dH_ij| <= 1e-8 |H_ij| + 1e-9 max|H|"""
    ref = np.asarray(ref, dtype=np.float64)
    return 1e-8 * np.abs(ref) + 1e-9 * np.max(np.abs(ref))


# ---- the Laplace / training case (tests/test_gpu_hessian.py; vetted on the host by tests/test_hessian_host.py) ------------------------
def laplace_case():
    """n = 200, d = 1, rbf_iso: x, y, noise variances, bounds and the starting point of the local optimiser"""
    rng = np.random.default_rng(2024)
    x = np.sort(rng.random((200, 1)), axis=0)
    y = np.sin(6.0 * x[:, 0]) + 0.3 * np.cos(17.0 * x[:, 0]) + 0.2 * rng.standard_normal(200)
    V = np.full(200, 0.04)
    bounds = np.array([[0.01, 100.0], [0.005, 10.0]])
    return x, y, V, bounds, np.array([1.0, 0.5])


# a point of that case where the Hessian is indefinite (eigenvalues -8.5 and 43.7): hyperparameter_laplace must refuse it
LAPLACE_NOT_A_MINIMUM = np.array([1.0, 3.0])


# ---- the second-derivative pass and the bracket, each on its own (tests/test_gpu_hessian_family.py, tests/test_hessian_family_host.py) --
# fvgp_hip_loglik_hess takes ANY lower factor and ANY alpha and leaves W = (L L^T)^-1, both triangles, in KV.  A factor scaled by 2^30 and
# b = 2^-30 u makes W and b b^T both of order 2^-60, the bracket (two factors W) of order n 2^-60 relative to the second-derivative
# trace: the returned numbers are then hess_trace_kernel's sums and the host's assembly of them, and nothing else.  The other way round
# (factor 2^-30, b 2^30) the trace is n^-1 2^-60 of the bracket and the numbers are the bracket's chain.
PASS_N = 261
PASS_SHIFT = 30
PASS_CASES = [(name, d) for name in NAMES for d in kf.DIMS]
DUP_ROWS = (3, 7, 200)           # x[7] = x[3] lies in a diagonal tile, x[200] = x[3] in the interior tile (1, 0)
BRACKET_SLACK = 2.0 ** -20       # of the bracket's magnitude, in the pass test: a million times its float64 rounding, a billionth of the bound
SENSITIVITY_CAP = 4.0            # what hess_trace_bound_factor assumes of the terms' mean sensitivity to r^2 (asserted on the host)


def cell(name, d):
    """the <KIND, D> instantiation dispatch_kind_dim (csrc/kernel_family.h) picks and the host layout of the partial sums:
    (kind, D, layout, iso) -- D = 0 is the runtime dimension, layout 'packed' (one row of 1 + d + d (d + 1) / 2 per tile) up to d = 4
    and 'rows' (d rows of 18 per tile) beyond"""
    kind, iso = kf.FAMILY[name]
    return kind, (d if d <= 4 else 0), ("packed" if d <= 4 else "rows"), iso


def pass_inputs(name, d, apart=False):
    """x (two planted coincident pairs; apart: each copy moved off its original by one ulp of one coordinate), theta, noise of the order
    of sigma^2 (a well-conditioned KV), y, and u uniform in [0.5, 1.5): b = 2^-+PASS_SHIFT u, all positive, so that -b b^T dominates the
    off-diagonal of W and the terms of every length-scale sum have one sign"""
    x, _, theta = kf.case(name, d, PASS_N)
    x = x.copy()
    rng = np.random.default_rng(77 * d + sorted(kf.FAMILY).index(name))
    V = theta[0] * rng.uniform(0.5, 1.5, PASS_N)
    y = rng.standard_normal((PASS_N, 1))
    u = rng.uniform(0.5, 1.5, PASS_N)
    i0, i1, i2 = DUP_ROWS
    x[i1] = x[i0]
    x[i2] = x[i0]
    if apart:
        x[i1, 0] = np.nextafter(x[i0, 0], 2.0)
        x[i2, d - 1] = np.nextafter(x[i0, d - 1], -1.0)
    return x, theta, V, y, u


def hess_trace_bound_factor(d):
    """allowed |device - exact| / (eps magnitude) for every number the second-derivative pass returns, magnitude = the sum over the
    entries of wt (|W_ab| + |b_a b_b|) |factor_ab| of the sums that enter it (with the host's 1 / l factors).  Derived like
    kernel_family_ref.grad_trace_bound_factor, in units of eps = 2^-52 (one rounding is at most eps / 2):

    depth of the summation, 75: 64 fused adds per lane (32 rows x 2 columns in a diagonal or edge tile, 16 trips x 4 entries in an
      interior one), 6 shuffle steps, 3 adds over the waves: 73 roundings of partial sums, counted whole; the host's sums over the tiles,
      over the d^2 + d sums of an isotropic kernel and its products with 1 / l run in long double (together below eps / 8 up to d = 16)
      and the result is rounded to double once: 2.
    per term:
      1   W - b b: two roundings, each at most eps / 2 of |W| + |b b| -- why the magnitude carries |W| + |b b| and not |W - b b|
      8   the two e2 factors: e = (x - u) (1 / l) with a rounded 1 / l is three roundings, its square seven: 3.5 eps each, 7 for two,
          and the products c2 e2_k and wt (c2 e2_k) (the multiply by e2_m is fused into the add, counted in the depth)
      12  the radial factor: 4 eps each for exp_neg (below 1 ulp, with its products by the constants), the square root (sqrt_pos,
          1 ulp) and Matern 3/2's reciprocal (two Newton steps, 1 ulp, and the product sqrt3 cf y)
      SENSITIVITY_CAP (d + 4)   the argument: r^2 is a sum of d rounded squares, relative error (d + 2) eps as kernel_family_ref has
          it, and the product with sqrt3 / sqrt5 / 0.5 and the constant's own rounding 2 eps more; a relative error delta of r^2 changes
          phi, cf and c2 by at most (1/2 + max(r^2, sqrt5 r) / 2) delta relative (d ln / d ln r^2 of each of the nine functions is
          below that); weighted with the terms' magnitudes that sensitivity averages below SENSITIVITY_CAP = 4 for every sum of every
          case -- an assumption on the inputs, which tests/test_hessian_family_host.py asserts from the longdouble reference."""
    return 75 + (1 + 8 + 12) + SENSITIVITY_CAP * (d + 4)


def _bracket64(dK, W, b):
    """the bracket [1/2 tr(G_i K_j) - b^T K_j w_i] (nt, nt) and its magnitude sum, in float64 through BLAS: in the pass test it is
    n 2^-60 of the entries it is subtracted from, its own float64 rounding another 2^-45 of that"""
    dK, W, b = (np.asarray(a, dtype=np.float64) for a in (dK, W, b))
    nt = len(dK)
    T = [W @ dK[i] for i in range(nt)]
    out, mag = np.zeros((nt, nt)), np.zeros((nt, nt))
    for i in range(nt):
        w_i, aw_i = T[i] @ b, np.abs(T[i]) @ np.abs(b)
        for j in range(nt):
            out[i, j] = 0.5 * np.sum(T[i] * T[j].T) - b @ (dK[j] @ w_i)
            mag[i, j] = 0.5 * np.sum(np.abs(T[i] * T[j].T)) + np.abs(b) @ (np.abs(dK[j]) @ aw_i)
    return out, mag


class PassSums:
    """the sums hess_trace_kernel forms, over the FULL symmetric matrix (the kernel's weight 2 below the diagonal): gs = sum B phi,
    gl[k] = sum B cf e2_k, Q[k, m] = sum B c2 e2_k e2_m with B = W - b b^T and e2_k = D_k^2 / l_k^2, in the number type T; `terms` are
    generated one sum at a time.  plant: None, or ("weight", None): the mirror of tile (1, 0) dropped (weight 1 for 2 on its rows), or
    ("c2", delta): c2 (1 + delta)."""

    def __init__(self, name, x, theta, W, b, T=LD, plant=None):
        self.T, self.name = T, name
        S = _Second(name, x, x, theta, T)
        self.S, self.d, self.iso = S, S.d, S.iso
        W, b = np.asarray(W, dtype=T), np.asarray(b, dtype=T)
        self.B = W - np.outer(b, b)
        self.absB = np.abs(W) + np.abs(np.outer(b, b))
        self.e2 = S.D2 / S.ls ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            self.e2_over_r = np.where(S.r[:, :, None] > 0, self.e2 / S.r[:, :, None], T(0))
        self.c2r = S.c2r * (T(1) + T(plant[1])) if plant is not None and plant[0] == "c2" else S.c2r
        self.mask = None
        if plant is not None and plant[0] == "weight":
            self.mask = np.ones(W.shape, dtype=T)
            self.mask[:128, 128:256] = 0
        # the bound's assumption: d ln f / d ln r^2 of phi, cf, c2 is at most 1/2 + max(r^2, sqrt5 r) / 2
        self.sens = T(0.5) + np.maximum(S.r ** 2, np.sqrt(T(5)) * S.r) / T(2)

    def factors(self):
        """(key, factor (n, n)) for gs, gl_k, Q_km (k <= m)"""
        S = self.S
        yield ("gs",), S.phi
        for k in range(self.d):
            yield ("gl", k), S.cf * self.e2[:, :, k]
        for k in range(self.d):
            for m in range(k, self.d):
                yield ("Q", k, m), self.c2r * self.e2_over_r[:, :, k] * self.e2[:, :, m]

    def reduce(self):
        """{key: (sum, magnitude sum, mean sensitivity)}"""
        out = {}
        for key, f in self.factors():
            t = self.B * f if self.mask is None else self.B * f * self.mask
            mag = self.absB * np.abs(f)
            m = np.sum(mag)
            out[key] = (np.sum(t), m, (np.sum(mag * self.sens) / m if m > 0 else self.T(0)))
        return out


def _packed_index(d, k, m, transposed=False):
    """where Q_km (k <= m) stands in the kernel's row of d (d + 1) / 2 sums: row by row; transposed: column by column (the planted
    error of the host's unpacking)"""
    if transposed:
        return m * (m + 1) // 2 + k
    return k * d - k * (k - 1) // 2 + (m - k)


def assemble_pass(name, theta, red, T=LD, transposed=False):
    """the host's assembly (csrc/hessian.hip) of the reduced sums `red` ({key: value}) into (g, A): g_i and A_ij = 1/2 sum B K_ij.
    transposed: Q_km is read from the packed row at the transposed index."""
    kind, iso = kf.FAMILY[name]
    theta = np.asarray(theta, dtype=T)
    d = max(k[1] for k in red if k[0] == "gl") + 1
    s, ls = theta[0], (np.full(d, theta[1], dtype=T) if iso else theta[1:])
    gs = red[("gs",)]
    gl = np.array([red[("gl", k)] for k in range(d)], dtype=T)
    packed = np.zeros(d * (d + 1) // 2, dtype=T)
    for k in range(d):
        for m in range(k, d):
            packed[_packed_index(d, k, m)] = red[("Q", k, m)]
    Q = np.zeros((d, d), dtype=T)
    for k in range(d):
        for m in range(k, d):
            Q[k, m] = Q[m, k] = packed[_packed_index(d, k, m, transposed)]
    nk = 2 if iso else d + 1
    g, A = np.zeros(nk, dtype=T), np.zeros((nk, nk), dtype=T)
    half = T(1) / T(2)
    g[0] = half * gs
    if iso:
        g[1] = half * np.sum(gl) / ls[0]
        A[0, 1] = A[1, 0] = g[1] / s
        A[1, 1] = half * (np.sum(Q) - 3 * np.sum(gl)) / ls[0] ** 2
    else:
        g[1:] = half * gl / ls
        A[0, 1:] = A[1:, 0] = g[1:] / s
        A[1:, 1:] = half * (Q / np.outer(ls, ls) - 3 * np.diag(gl / ls ** 2))
    return g, A


def pass_bounds(name, theta, mags, bracket_mag, d):
    """the bounds of g_i and of the raw H_ij of the pass test from the magnitude sums `mags` ({key: magnitude}): the assembly with
    magnitudes for sums and + for -, so a diagonal length-scale entry (the difference of two sums) takes both and an isotropic entry
    all d^2 + d; times hess_trace_bound_factor(d) eps; plus BRACKET_SLACK of the bracket's magnitude"""
    iso = kf.FAMILY[name][1]
    theta = np.asarray(theta, dtype=LD)
    s, ls = theta[0], (np.full(d, theta[1], dtype=LD) if iso else theta[1:])
    Mgl = np.array([mags[("gl", k)] for k in range(d)], dtype=LD)
    MQ = np.zeros((d, d), dtype=LD)
    for k in range(d):
        for m in range(k, d):
            MQ[k, m] = MQ[m, k] = mags[("Q", k, m)]
    nk = 2 if iso else d + 1
    gm, Am = np.zeros(nk, dtype=LD), np.zeros((nk, nk), dtype=LD)
    gm[0] = mags[("gs",)] / 2
    if iso:
        gm[1] = np.sum(Mgl) / 2 / ls[0]
        Am[1, 1] = (np.sum(MQ) + 3 * np.sum(Mgl)) / 2 / ls[0] ** 2
    else:
        gm[1:] = Mgl / 2 / ls
        Am[1:, 1:] = (MQ / np.outer(ls, ls) + 3 * np.diag(Mgl / ls ** 2)) / 2
    Am[0, 1:] = Am[1:, 0] = gm[1:] / s
    feps = LD(hess_trace_bound_factor(d)) * LD(kf.EPS)
    return feps * gm, feps * Am + LD(BRACKET_SLACK) * np.asarray(bracket_mag, dtype=LD)


def pass_reference(name, x, theta, W, b):
    """the longdouble reference of the second-derivative pass on the device's own W (symmetric, as read back from KV) and b:
    dict with g, raw (the module's formula: 1/2 sum B K_ij through _Second.pair, minus the bracket), their bounds, the reduced sums with
    magnitudes and sensitivities, and the bracket"""
    P = PassSums(name, x, theta, W, b, LD)
    S, B = P.S, P.B
    half = LD(1) / LD(2)
    dK = kf.dk_dtheta_ref(name, x, x, theta)
    nt = len(dK)
    g = np.array([half * np.sum(B * dK[i]) for i in range(nt)], dtype=LD)
    brk, brk_mag = _bracket64(dK, W, b)
    raw = np.zeros((nt, nt), dtype=LD)
    for i in range(nt):
        for j in range(i, nt):
            raw[i, j] = raw[j, i] = half * np.sum(B * S.pair(i, j))
    raw = raw - brk.astype(LD)
    red = P.reduce()
    g_bound, raw_bound = pass_bounds(name, theta, {k: v[1] for k, v in red.items()}, brk_mag, P.d)
    return {"g": g, "raw": raw, "g_bound": g_bound, "raw_bound": raw_bound, "red": red, "bracket": brk, "bracket_mag": brk_mag}


def pass_twin(name, x, theta, W, b, bracket, plant=None):
    """the pass in float64: the same formulas in double, numpy's own summation order, the host's assembly in double; minus the given
    bracket.  plant: see PassSums, or ("transposed", None): the host's unpacking reads Q_km at the transposed packed index."""
    sums_plant = plant if plant is not None and plant[0] in ("weight", "c2") else None
    P = PassSums(name, x, theta, W, b, np.float64, sums_plant)
    red = {k: v[0] for k, v in P.reduce().items()}
    g, A = assemble_pass(name, theta, red, np.float64, transposed=plant is not None and plant[0] == "transposed")
    return g, A - np.asarray(bracket, dtype=np.float64)


# one case per <KIND, D> cell, ARD and isotropic alternating (and both ends of the runtime dimension): the bracket costs two 384^3 products
# per hyperparameter, and 15 cases cover the instantiations of kmat_grad_kernel and of the two-vector trace
def _bracket_cases():
    out = []
    for kind in dict.fromkeys(k for k, _ in kf.FAMILY.values()):
        for D in (1, 2, 3, 4, 0):
            iso = len(out) % 2 == 1
            name = next(nm for nm, (k, i) in kf.FAMILY.items() if k == kind and i == iso)
            out.append((name, D if D else (5 if iso else 16)))
    return out


BRACKET_CASES = _bracket_cases()


def bracket_bound_factors(d, np_):
    """(on M1 + M2, in eps) the allowance of the bracket 1/2 tr(G_i K_j) - b^T K_j w_i as kmat_grad_kernel, the two products,
    rowdot_scale_kernel and the two-vector trace compute it, with M1 = 1/2 sum (|W| |K_i| |W|)_ab |K_j|_ab and
    M2 = |b|^T |K_j| (|W| |K_i| |b|).  Every term is derived, none measured:
      2 (np + 3) / 2   the two products T = W K_i and G_i = T W: gemm_ref.bound, (K + S + 2) u each with K = np, S = 1 (K = 384 is below
                       the split's 512) -- the second product's bound is on |T| |W| <= |W| |K_i| |W|, and it carries the first one's error
      2 (32 + 2 d)     the entries of K_i (kmat_grad_kernel) and of K_j (the trace re-evaluates them): the per-term part of
                       kernel_family_ref.grad_trace_bound_factor
      80 + d           the trace's summation depth: the other part of that factor
      2                the two roundings of G_ab - (b_a w_b + w_a b_b)
      12               rowdot_scale_kernel: a lane's two fused adds at n <= 512, 6 shuffle steps, 2 adds over the waves, the scale, and the
                       rounding of each output: w_i enters M2 only, charged to both"""
    return (np_ + 3) + 2 * (32 + 2 * d) + (80 + d) + 2 + 12


def bracket_reference(name, x, theta, W, b, dtype=LD, plant=False):
    """the raw Hessian of the bracket test from the device's W (symmetric) and b: the module's formula in longdouble (the
    second-derivative trace, n^-1 2^-60 of the bracket, included), its bound per entry -- bracket_bound_factors eps (M1 + M2) plus
    BRACKET_SLACK of the trace's magnitude --, and, dtype=np.float64, the twin: the same formulas in double with BLAS products.
    plant (twin): the isotropic length-scale matrix of kmat_grad_kernel sums d - 1 of the d dimensions."""
    T = dtype
    W, b = np.asarray(W, dtype=T), np.asarray(b, dtype=T)
    S = _Second(name, x, x, theta, T)
    dK = kf.dk_dtheta_ref(name, x, x, theta, T)
    nt = len(dK)
    Ki = dK.copy()                                    # what kmat_grad_kernel assembles (the trace has its own K_j)
    if plant:
        assert S.iso
        Ki[1] = S.cf * np.sum(S.e[:, :, :S.d - 1], axis=2)
    mm = (lambda a, c: loo_ref.matmul(a, np.ascontiguousarray(c))) if T is LD else (lambda a, c: a @ c)
    B = W - np.outer(b, b)
    half = T(1) / T(2)
    aW, ab = np.abs(W), np.abs(b)
    raw, bound = np.zeros((nt, nt), dtype=T), np.zeros((nt, nt), dtype=LD)
    feps = LD(bracket_bound_factors(S.d, -(-len(b) // 128) * 128)) * LD(kf.EPS)
    for i in range(nt):
        G = mm(mm(W, Ki[i]), W)
        w_i = mm(W, Ki[i]) @ b
        if T is LD:
            aG = mm(mm(aW, np.abs(Ki[i])), aW)
            aw_i = mm(aW, np.abs(Ki[i])) @ ab
        for j in range(nt):
            a_ij = half * np.sum(B * S.pair(i, j))
            raw[i, j] = a_ij - (half * np.sum(G * dK[j]) - b @ (dK[j] @ w_i))
            if T is LD:
                M = half * np.sum(aG * np.abs(dK[j])) + ab @ (np.abs(dK[j]) @ aw_i)
                a_mag = half * np.sum((aW + np.outer(ab, ab)) * np.abs(S.pair(i, j)))
                bound[i, j] = feps * M + LD(BRACKET_SLACK) * a_mag
    return raw, bound
