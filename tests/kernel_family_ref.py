"""An independent extended-precision reference of the native kernel family (a helper module of the tests, not a conftest).

Everything here is written from the closed forms below in numpy.longdouble (64-bit mantissa on x86-64: about 2000 times finer than
the doubles it judges), not from the project's device code (csrc/radial.h) or its host restatements (fvgp_amd/kernels.py,
oracle/fvgp_oracle.py).  With D_k = x1_ik - x2_jk, l_k the length scale of dimension k (theta[1 + k]; theta[1] for every dimension of
an isotropic kernel), r^2 = sum_k (D_k / l_k)^2 and s = theta[0] (the signal variance sigma^2):

    kind       phi(r)                                    cf(r)
    rbf        exp(-r^2 / 2)                             s phi(r)
    matern32   (1 + sqrt3 r) exp(-sqrt3 r)               3 s exp(-sqrt3 r)
    matern52   (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r)   5/3 s (1 + sqrt5 r) exp(-sqrt5 r)

    k = s phi(r)       dk/ds = phi(r)       dk/dl_k = cf(r) D_k^2 / l_k^3       dk/dx1_k = -cf(r) D_k / l_k^2

(dphi/dr = -r cf / s for all three, and dr/dl_k = -D_k^2 / (l_k^3 r), dr/dx1_k = D_k / (l_k^2 r): the 1 / r cancels, so every
derivative is finite at coincident points).  An isotropic kernel has one length scale: its derivative is the sum over the dimensions.

A family member is looked up by name in FAMILY and its radial kind in _RADIAL: a name or kind without an entry raises KeyError, so a
seventh kernel fails every test that needs it until its formula is written down here."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# name -> (radial kind, one length scale for every dimension)
FAMILY = {
    "rbf_ard": ("rbf", False), "matern32_ard": ("matern32", False), "matern52_ard": ("matern52", False),
    "rbf_iso": ("rbf", True), "matern32_iso": ("matern32", True), "matern52_iso": ("matern52", True),
}


def _rbf(r2, T):
    phi = np.exp(-r2 / T(2))
    return phi, phi


def _matern32(r2, T):
    a = np.sqrt(T(3)) * np.sqrt(r2)
    ea = np.exp(-a)
    return (T(1) + a) * ea, T(3) * ea


def _matern52(r2, T):
    a = np.sqrt(T(5)) * np.sqrt(r2)
    ea = np.exp(-a)
    return (T(1) + a + T(5) * r2 / T(3)) * ea, T(5) / T(3) * (T(1) + a) * ea


# kind -> (r^2, number type) -> (phi, cf / s)
_RADIAL = {"rbf": _rbf, "matern32": _matern32, "matern52": _matern52}


def n_theta(name, d):
    """hyperparameters the kernel owns: sigma^2, then one length scale or one per dimension"""
    return 2 if FAMILY[name][1] else d + 1


def _setup(name, x1, x2, theta, T):
    kind, iso = FAMILY[name]
    x1, x2, theta = np.asarray(x1, dtype=T), np.asarray(x2, dtype=T), np.asarray(theta, dtype=T)
    d = x1.shape[1]
    if x2.shape[1] != d or theta.shape != (n_theta(name, d),):
        raise ValueError(f"{name}: x1 {x1.shape}, x2 {x2.shape}, theta {theta.shape} do not fit")
    ls = np.full(d, theta[1], dtype=T) if iso else theta[1:]
    delta = x1[:, None, :] - x2[None, :, :]                        # (n1, n2, d)
    r2 = np.sum((delta / ls) ** 2, axis=2)
    phi, cf1 = _RADIAL[kind](r2, T)
    return iso, theta[0], ls, delta, phi, theta[0] * cf1


def k_ref(name, x1, x2, theta, dtype=LD):
    """K (n1, n2) in longdouble (dtype=np.float64: the same formulas in double, for judging the bounds on the host)"""
    _, s, _, _, phi, _ = _setup(name, x1, x2, theta, dtype)
    return s * phi


def dk_dtheta_ref(name, x1, x2, theta, dtype=LD):
    """dK/dtheta (n_theta, n1, n2) in longdouble"""
    iso, _, ls, delta, phi, cf = _setup(name, x1, x2, theta, dtype)
    dl = np.transpose(cf[:, :, None] * delta ** 2 / ls ** 3, (2, 0, 1))         # (d, n1, n2)
    if iso:
        dl = np.sum(dl, axis=0, keepdims=True)
    return np.concatenate([phi[None], dl], axis=0)


def dk_dx_ref(name, x1, x2, theta, dtype=LD):
    """d k(x1_p, x2_i) / d x1_pk, shape (d, n1, n2), in longdouble"""
    _, _, ls, delta, _, cf = _setup(name, x1, x2, theta, dtype)
    return np.transpose(-cf[:, :, None] * delta / ls ** 2, (2, 0, 1))


DIMS = (1, 2, 3, 4, 5, 16)      # the four dimensions with an instantiation of their own, and both ends of the runtime-dimension path


def case_theta(name, d, rng, sig=1.7):
    """sigma^2 and length scales for points from the unit cube, chosen so that the median entry of K stays above 0.1 sigma^2 (the
    off-diagonal entries then exercise the radial functions instead of underflowing to 0; tests/test_kernel_family_ref.py asserts
    it for every case the device tests use).  r^2 is about sum_k 1 / (6 l_k^2), so the scales grow with sqrt(d).  One per dimension:
    (0.2 + U(0, 1)) max(1, sqrt(d / 2)), 2.8 times the unit-cube draw at d = 16.  One for all dimensions: (0.3 + 0.3 U(0, 1)) sqrt(d)."""
    if FAMILY[name][1]:
        ls = (0.3 + 0.3 * rng.random(1)) * np.sqrt(d)
    else:
        ls = (0.2 + rng.random(d)) * max(1.0, np.sqrt(d / 2.0))
    return np.concatenate([[sig], ls])


def case(name, d, n1, n2=None):
    """the inputs of one conformance case, the same on the host and on the device: x1 (n1, d), x2 (n2, d) -- or None -- from the unit
    cube and theta = case_theta"""
    rng = np.random.default_rng(1000 * d + 10 * sorted(FAMILY).index(name) + (n1 % 7))
    x1 = rng.random((n1, d))
    x2 = None if n2 is None else rng.random((n2, d))
    return x1, x2, case_theta(name, d, rng)


def k_bound_ulps(d):
    """allowed |K_device - K_exact| in units of eps sigma^2.  d <= 5: the project's bar of 4.  Larger d: r^2 is a sum of d
    rounded squares of rounded scaled differences, relative error <= (d + 2) eps, and |dk| <= sup r^2 |phi'(r^2)| (d + 2) eps s with
    sup r^2 |dphi/d(r^2)| = 1/e = 0.37 (rbf), 0.40 (matern32, at sqrt3 r = 1.62), 0.40 (matern52): 0.4 (d + 2), plus the 4 for
    exp, sqrt and the polynomial -- 11.2 at d = 16."""
    return 4.0 if d <= 5 else 4.0 + 0.4 * (d + 2)


def grad_trace_terms(name, x, theta, W, b=None, dtype=LD):
    """the terms of 1/2 sum_jk (W_jk - b_j b_k) dK_jk/dtheta_i, shape (n_theta, n, n), longdouble; W symmetric"""
    W = np.asarray(W, dtype=dtype)
    if b is not None:
        b = np.asarray(b, dtype=dtype)
        W = W - np.outer(b, b)
    return dtype(0.5) * W[None] * dk_dtheta_ref(name, x, x, theta, dtype)


def grad_trace_bound_factor(d):
    """allowed |g_device - g_exact| / (eps sum_jk |term_jk|): 80 + d for the depth of the device's summation (64 fused adds per thread,
    6 shuffle steps, 3 adds over the waves, up to d for the isotropic fold; the sum over the tiles runs in long double) and 32 + 2 d per
    term for two correct evaluations of an entry (a few ulp each for exp and sqrt, (d + 2) for the rounding of r^2 in its argument,
    d for the e_k^2)"""
    return (80 + d) + (32 + 2 * d)
