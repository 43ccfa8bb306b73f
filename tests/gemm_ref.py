"""Operands and references for the tests of the fp64 GEMM entry (fvgp_hip_gemm): C = alpha * opA * opB + beta * C0.

Two families.

EXACT: integer entries, |a|, |b| <= 64, |c| <= 1024, alpha in {+-0.75, 1}, beta in {1.25, 1, 0}.  Every partial sum of products,
taken in any order, fused or not, split over K or not, is an integer of magnitude <= 64 * 64 * K (6.8e7 at K = 16400) and so a
double without rounding; alpha times it and beta times c are multiples of 1/4 far below 2^53, and so is their sum.  The correct
result therefore has ONE bit pattern, the float64 expression below gives it, and the assertion is np.array_equal: a wrong index,
a dropped or doubled k step, a swapped tile or a stale LDS buffer changes bits.

ROUNDING: full-mantissa normals, the rows of op(A) and the columns of op(B) scaled by 2^e, e uniform in -20 .. 20, so that a bound
which only holds in norm fails.  Reference in numpy.longdouble (64-bit mantissa on x86-64).  Componentwise bound

    |got - ref| <= (K + S + 2) u (|alpha| |opA| @ |opB| + |beta| |C0|),      u = 2^-53,

S the number of K slices (1 unsplit): Higham's gamma bound of a length-K dot product summed in any order ((K) u to first order,
fused multiply-adds included), S - 1 further additions of the slices, one rounding each for the alpha product, the beta product
and the final sum.  The bound is derived, not measured; `fraction` reports how much of it a result uses.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ALPHAS = (-0.75, 0.75, 1.0)
BETAS = (1.25, 1.0, 0.0)


def extended_precision():
    """numpy.longdouble is the 80-bit extended format (the rounding family's reference judges nothing otherwise)"""
    return np.finfo(LD).nmant == 63


def store(opA, opB, a_kmajor, b_nmajor):
    """op(A) (M, K) and op(B) (K, N) as the entry wants them stored: A (M, K) or, a_kmajor, (K, M); B (N, K) or, b_nmajor, (K, N)"""
    A = np.ascontiguousarray(opA.T) if a_kmajor else np.ascontiguousarray(opA)
    B = np.ascontiguousarray(opB) if b_nmajor else np.ascontiguousarray(opB.T)
    return A, B


def exact_case(M, N, K, seed):
    """(opA (M, K), opB (K, N), C0 (M, N)) of the exact family, float64 arrays of integers"""
    rng = np.random.default_rng(seed)
    opA = rng.integers(-64, 65, (M, K)).astype(np.float64)
    opB = rng.integers(-64, 65, (K, N)).astype(np.float64)
    C0 = rng.integers(-1024, 1025, (M, N)).astype(np.float64)
    return opA, opB, C0


def exact_ref(opA, opB, C0, alpha, beta):
    assert alpha in ALPHAS and beta in BETAS
    prod = opA @ opB if opA.shape[1] else np.zeros(C0.shape)
    return alpha * prod + beta * C0


def rounding_case(M, N, K, seed):
    """(opA, opB, C0) of the rounding family; C0 is of the size of a typical |opA| @ |opB| entry, so that neither term hides the other"""
    rng = np.random.default_rng(seed)

    def normals(shape):
        return rng.choice([-1.0, 1.0], shape) * (1.0 + rng.random(shape))          # 52 random mantissa bits, exponent 0

    sa = np.ldexp(1.0, rng.integers(-20, 21, M))
    sb = np.ldexp(1.0, rng.integers(-20, 21, N))
    opA = normals((M, K)) * sa[:, None]
    opB = normals((K, N)) * sb[None, :]
    C0 = normals((M, N)) * np.sqrt(K) * sa[:, None] * sb[None, :]
    return opA, opB, C0


def rounding_ref(opA, opB, C0, alpha, beta):
    """(ref, magnitude) in longdouble: ref = alpha opA opB + beta C0, magnitude = |alpha| |opA| |opB| + |beta| |C0|"""
    a, b = opA.astype(LD), opB.astype(LD)
    ref = LD(alpha) * (a @ b) + LD(beta) * C0.astype(LD)
    mag = LD(abs(alpha)) * (np.abs(a) @ np.abs(b)) + LD(abs(beta)) * np.abs(C0).astype(LD)
    return ref, mag


def bound(mag, K, slices=1):
    return LD(K + slices + 2) * LD(U) * mag


def fraction(got, ref, mag, K, slices=1):
    """the largest |got - ref| / bound over the entries (<= 1 passes); entries whose bound is 0 must be exact"""
    err = np.abs(got.astype(LD) - ref)
    bnd = bound(mag, K, slices)
    zero = bnd == 0
    if np.any(err[zero] != 0):
        return np.inf
    return float(np.max(err[~zero] / bnd[~zero])) if np.any(~zero) else 0.0


def tile_mask(M, N, lower):
    """True where the entry computes: everywhere, or (lower) in the 128 x 128 tiles with tile row >= tile column"""
    if not lower:
        return np.ones((M, N), dtype=bool)
    ti = np.arange(M)[:, None] // 128
    tj = np.arange(N)[None, :] // 128
    return tj <= ti
