"""The references of the GEMM entry's tests (tests/gemm_ref.py) proven on the host, without the device: the exact family's float64
reference is the integer product, a correct double-precision product of the rounding family stays inside the componentwise bound
the device tests assert, and a product that lost a single k step does not."""
import numpy as np
import pytest

import gemm_ref as ref

LD = np.longdouble


def _need_extended():
    if not ref.extended_precision():
        pytest.skip("numpy.longdouble is not the 80-bit extended format here: the reference would judge nothing")


@pytest.mark.parametrize("M,N,K", [(256, 384, 16), (384, 384, 528), (256, 384, 1040), (128, 128, 16400)])
@pytest.mark.parametrize("alpha,beta", [(-0.75, 1.25), (0.75, 1.0), (1.0, 0.0)])
def test_exact_family_reference_is_the_integer_product(M, N, K, alpha, beta):
    """float64 BLAS on the exact family equals the int64 product, and alpha, beta in quarters keep it exact: 4 * ref is the integer
    4 alpha (A B) + 4 beta C0"""
    opA, opB, C0 = ref.exact_case(M, N, K, seed=K + M)
    assert np.max(np.abs(opA)) <= 64 and np.max(np.abs(opB)) <= 64 and np.max(np.abs(C0)) <= 1024
    assert np.array_equal(opA, np.rint(opA)) and np.array_equal(opB, np.rint(opB)) and np.array_equal(C0, np.rint(C0))
    prod = opA.astype(np.int64) @ opB.astype(np.int64)
    assert np.array_equal(opA @ opB, prod.astype(np.float64))
    assert 64 * 64 * K < 2 ** 53 // 8
    want4 = int(4 * alpha) * prod + int(4 * beta) * C0.astype(np.int64)
    got = ref.exact_ref(opA, opB, C0, alpha, beta)
    assert np.array_equal(4.0 * got, want4.astype(np.float64))
    # any split of K gives the same bits
    h = (K // 32) * 16
    parts = alpha * (opA[:, :h] @ opB[:h]) + alpha * (opA[:, h:] @ opB[h:]) + beta * C0
    assert np.array_equal(parts, got)


def test_exact_family_with_no_k_at_all():
    opA, opB, C0 = ref.exact_case(128, 256, 0, seed=1)
    assert np.array_equal(ref.exact_ref(opA, opB, C0, -0.75, 1.25), 1.25 * C0)
    assert np.array_equal(ref.exact_ref(opA, opB, C0, 1.0, 0.0), np.zeros((128, 256)))


def test_stored_layouts():
    opA, opB, _ = ref.exact_case(128, 256, 32, seed=2)
    for akm in (0, 1):
        for bnm in (0, 1):
            A, B = ref.store(opA, opB, akm, bnm)
            assert A.shape == ((32, 128) if akm else (128, 32)) and B.shape == ((32, 256) if bnm else (256, 32))
            assert A.flags.c_contiguous and B.flags.c_contiguous
            assert np.array_equal(A.T if akm else A, opA) and np.array_equal(B if bnm else B.T, opB)


def test_tile_mask():
    m = ref.tile_mask(384, 256, 1)
    assert m[:128, :128].all() and not m[:128, 128:].any() and m[128:, :].all()
    assert ref.tile_mask(256, 384, 0).all()


@pytest.mark.parametrize("M,N,K,alpha,beta", [(256, 256, 528, -0.75, 1.25), (256, 256, 128, 0.75, 1.0), (128, 256, 1040, 1.0, 0.0)])
def test_rounding_family_numpy_product_is_inside_the_bound(M, N, K, alpha, beta):
    """numpy's own float64 product (BLAS: blocked, fused multiply-adds, its own order) stays inside the componentwise bound against
    longdouble with S = 1; so does the product added up from four K slices, with S = 4; the row and column scales span 2^40 each"""
    _need_extended()
    opA, opB, C0 = ref.rounding_case(M, N, K, seed=K)
    rows = np.max(np.abs(opA), axis=1); cols = np.max(np.abs(opB), axis=0)
    assert rows.max() / rows.min() >= 2.0 ** 30 and cols.max() / cols.min() >= 2.0 ** 30
    want, mag = ref.rounding_ref(opA, opB, C0, alpha, beta)
    assert want.dtype == LD and mag.dtype == LD
    got = alpha * (opA @ opB) + beta * C0
    f = ref.fraction(got, want, mag, K)
    assert 0.0 < f <= 1.0, f
    cuts = [0, 16 * (K // 64), 32 * (K // 64), 48 * (K // 64), K]
    split = sum(alpha * (opA[:, a:b] @ opB[a:b]) for a, b in zip(cuts[:-1], cuts[1:])) + beta * C0
    f = ref.fraction(split, want, mag, K, slices=4)
    assert 0.0 < f <= 1.0, f


@pytest.mark.parametrize("K", [16, 528, 1040])
def test_a_product_without_one_k_step_is_outside_the_bound(K):
    """sixteen k terms missing (one step of the kernels' K loop), anywhere in the range, and a single missing term: far outside"""
    _need_extended()
    M = N = 128
    opA, opB, C0 = ref.rounding_case(M, N, K, seed=7 + K)
    want, mag = ref.rounding_ref(opA, opB, C0, -0.75, 1.25)
    for k0 in sorted({0, 16 * (K // 32), K - 16}):
        keep = np.ones(K, dtype=bool); keep[k0:k0 + 16] = False
        got = -0.75 * (opA[:, keep] @ opB[keep]) + 1.25 * C0
        assert ref.fraction(got, want, mag, K, slices=64) > 1e8
    keep = np.ones(K, dtype=bool); keep[K // 2] = False
    got = -0.75 * (opA[:, keep] @ opB[keep]) + 1.25 * C0
    assert ref.fraction(got, want, mag, K, slices=64) > 1e8
    # and one entry of C0 taken from the neighbouring column
    got = -0.75 * (opA @ opB) + 1.25 * np.roll(C0, 1, axis=1)
    assert ref.fraction(got, want, mag, K, slices=64) > 1e8
