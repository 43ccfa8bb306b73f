"""The extended-precision reference of the kernel family (tests/kernel_family_ref.py) proven on the host, without the device: against
the oracle's analytic gradients where it has them, against central differences of its own K for every family member, and the bounds
the device tests assert (tests/test_gpu_kernel_family.py) shown to be met by correct double-precision evaluations."""
import numpy as np
import pytest

import kernel_family_ref as ref
from oracle import fvgp_oracle as orc

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _names():
    from fvgp_amd import _lib
    return list(_lib.KERNEL_IDS)


def test_the_reference_covers_the_family_by_name():
    """every name the ABI knows has a formula here and in the oracle; an unknown one fails loudly"""
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble is not the 80-bit extended format here: the reference would judge nothing"
    assert sorted(ref.FAMILY) == sorted(_names()) == sorted(orc.KERNELS)
    x = np.random.default_rng(0).random((3, 2))
    for f in (ref.k_ref, ref.dk_dtheta_ref, ref.dk_dx_ref):
        with pytest.raises(KeyError):
            f("matern12_ard", x, x, np.ones(3))


@pytest.mark.parametrize("d", [3, 16])
@pytest.mark.parametrize("name", sorted(orc.KERNEL_GRADS))
def test_dk_dtheta_matches_the_oracle_gradients(name, d):
    """the three kernels with a one-length-scale-per-dimension gradient in the oracle (trial run: 9e-16 of the largest entry)"""
    x1, x2, theta = ref.case(name, d, 60, 41)
    for a, b in ((x1, x2), (x1, x1)):                        # (x1, x1): coincident points, r = 0 on the diagonal
        want = orc.KERNEL_GRADS[name](a, b, theta)
        got = ref.dk_dtheta_ref(name, a, b, theta)
        assert got.shape == want.shape == (d + 1, len(a), len(b))
        for i in range(d + 1):
            err = float(np.max(np.abs(got[i] - want[i])) / np.max(np.abs(want[i])))
            assert err <= 1e-14, (name, d, i, err)


@pytest.mark.parametrize("d", [1, 3, 5, 16])
@pytest.mark.parametrize("name", sorted(ref.FAMILY))
def test_dk_dtheta_matches_central_differences_of_k_ref(name, d):
    """every family member, the isotropic sum included: central difference of k_ref in longdouble, step 1e-7 (truncation
    h^2 k''' / 6 ~ 1e-14 k / l^3, round-off 2^-64 / h ~ 5e-13; trial run 1.6e-12 of the largest entry): 1e-9 allowed"""
    x1, x2, theta = ref.case(name, d, 50, 37)
    got = ref.dk_dtheta_ref(name, x1, x2, theta)
    assert got.shape == (ref.n_theta(name, d), 50, 37)
    h = LD(1e-7)
    worst = 0.0
    for i in range(len(theta)):
        tp, tm = np.asarray(theta, dtype=LD), np.asarray(theta, dtype=LD)
        tp[i] += h
        tm[i] -= h
        fd = (ref.k_ref(name, x1, x2, tp) - ref.k_ref(name, x1, x2, tm)) / (2 * h)
        err = float(np.max(np.abs(got[i] - fd)) / np.max(np.abs(fd)))
        worst = max(worst, err)
        assert err <= 1e-9, (name, d, i, err)
    print(f"{name} d={d}: dk/dtheta vs central difference, worst {worst:.2e} of the largest entry")


@pytest.mark.parametrize("d", [1, 3, 5, 16])
@pytest.mark.parametrize("name", sorted(ref.FAMILY))
def test_dk_dx_matches_central_differences_of_k_ref(name, d):
    """the derivative in the first argument (what fvgp_hip_posterior_grad differentiates), the same way: step 1e-7, 1e-9 allowed"""
    x1, x2, theta = ref.case(name, d, 20, 37)
    got = ref.dk_dx_ref(name, x1, x2, theta)
    assert got.shape == (d, 20, 37)
    h = LD(1e-7)
    for k in range(d):
        xp, xm = np.asarray(x1, dtype=LD), np.asarray(x1, dtype=LD)
        xp[:, k] += h
        xm[:, k] -= h
        fd = (ref.k_ref(name, xp, x2, theta) - ref.k_ref(name, xm, x2, theta)) / (2 * h)
        err = float(np.max(np.abs(got[k] - fd)) / np.max(np.abs(fd)))
        assert err <= 1e-9, (name, d, k, err)


@pytest.mark.parametrize("d", ref.DIMS)
@pytest.mark.parametrize("name", sorted(ref.FAMILY))
def test_the_oracle_in_double_sits_within_the_k_bound(name, d):
    """orc.KERNELS in double against k_ref on the device test's own inputs: within the bound the device is held to (trial run:
    at most 2.0 eps sigma^2), so the bound is one a correct double evaluation meets; and the median entry of K is at least 0.1 sigma^2
    on every input set the device tests draw, so those cases test the radial functions and not an underflow to 0."""
    x1, x2, theta = ref.case(name, d, 300, 201)
    exact = ref.k_ref(name, x1, x2, theta)
    got = orc.KERNELS[name](x1, x2, theta)
    ulps = float(np.max(np.abs(got - exact)) / (EPS * theta[0]))
    print(f"{name} d={d}: oracle K within {ulps:.2f} eps sigma^2 (bound {ref.k_bound_ulps(d):.1f})")
    assert ulps <= ref.k_bound_ulps(d)
    assert float(np.median(exact)) >= 0.1 * theta[0]
    for n in (129, 300, 517):
        x, _, th = ref.case(name, d, n)
        assert float(np.median(ref.k_ref(name, x, x, th, np.float64))) >= 0.1 * th[0], (name, d, n)


def test_k_bound_values():
    assert [ref.k_bound_ulps(d) for d in (1, 5)] == [4.0, 4.0] and abs(ref.k_bound_ulps(16) - 11.2) < 1e-12
    assert ref.grad_trace_bound_factor(3) == 80 + 3 + 32 + 6 and ref.grad_trace_bound_factor(16) == 80 + 16 + 32 + 32


@pytest.mark.parametrize("d", [2, 5, 16])
@pytest.mark.parametrize("name", sorted(ref.FAMILY))
def test_a_double_gradient_trace_sits_within_the_summation_bound(name, d):
    """1/2 sum_jk (W_jk - b_j b_k) dK_jk/dtheta_i with every term evaluated and summed in double (numpy's pairwise sum) against the
    longdouble sum: within (80 + d + 32 + 2 d) eps sum|term|, the bound of the device tests"""
    n = 129
    x, _, theta = ref.case(name, d, n)
    rng = np.random.default_rng(d)
    W = rng.standard_normal((n, n))
    W = W + W.T
    b = rng.standard_normal(n)
    terms = ref.grad_trace_terms(name, x, theta, W, b)
    want, scale = terms.sum(axis=(1, 2)), np.abs(terms).sum(axis=(1, 2))
    terms64 = ref.grad_trace_terms(name, x, theta, W, b, dtype=np.float64)
    assert terms64.dtype == np.float64
    got = terms64.sum(axis=(1, 2))
    ratio = np.abs(got - want) / (ref.grad_trace_bound_factor(d) * EPS * scale)
    print(f"{name} d={d}: double gradient trace at {float(np.max(ratio)):.3f} of the bound")
    assert np.all(ratio <= 1.0), (name, d, ratio)
