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

A kind without an entry in _C2 raises KeyError: a new kernel fails every test that needs its Hessian until its formula stands here."""
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
