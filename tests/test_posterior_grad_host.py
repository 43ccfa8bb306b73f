"""kernels.kernel_dx, the host restatement of the closed-form kernel derivative fvgp_hip_posterior_grad evaluates: against central
differences of the package's own host kernels (tolerance derived from the step), the exact RBF case, and -- with a numpy solve -- the
posterior derivatives it implies against the reference's Richardson ground truth (fixture G12).  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
from fvgp_amd import kernels as K

EPS = np.finfo(np.float64).eps
KERNELS = ["rbf_ard", "matern32_ard", "matern52_ard", "rbf_iso", "matern32_iso", "matern52_iso"]


def host_kernel(name, x1, x2, hps):
    """the named kernels from the package's host building blocks (the formulas of the module docstring)"""
    hps = np.asarray(hps, dtype=np.float64)
    if name.endswith("_iso"):
        dist, length = K.get_distance_matrix(x1, x2), hps[1]
    else:
        dist, length = K.get_anisotropic_distance_matrix(x1, x2, hps[1:]), 1.0
    f = {"rbf": K.squared_exponential_kernel, "matern32": K.matern_kernel_diff1, "matern52": K.matern_kernel_diff2}[name.split("_")[0]]
    return hps[0] * f(dist, length)


def _hps(name, d, rng):
    return np.concatenate([[1.3], rng.uniform(0.3, 0.6, 1 if name.endswith("_iso") else d)])


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("name", KERNELS)
def test_kernel_dx_matches_central_differences(name, d):
    """|kernel_dx - central difference| <= h^2 max|d3k| / 6 + eps max|k| / h, the textbook error of a central difference with step h:
    truncation plus the rounding of the two kernel values.  max|d3k| comes from the host kernels alone: twice the largest third central
    difference [k(+2t) - 2 k(+t) + 2 k(-t) - k(-2t)] / (2 t^3) at the coarse step t = 1e-3 (the factor 2 covers that estimate's own
    truncation; its round-off, 3 eps max|k| / t^3 = 7e-7, is far below the third derivatives met here, 1e1 .. 1e3).  Random points: no
    coincident pairs (Matern-3/2's third derivative jumps there)."""
    rng = np.random.default_rng(100 * d + len(name))
    xp, xd = rng.random((7, d)), rng.random((40, d))
    hps = _hps(name, d, rng)
    h = 1e-5
    got = K.kernel_dx(name, xp, xd, hps)
    assert got.shape == (d, 7, 40)
    t = 1e-3

    def at(k, s):
        q = np.array(xp)
        q[:, k] += s
        return host_kernel(name, q, xd, hps)

    for k in range(d):
        d3 = 2.0 * np.max(np.abs(at(k, 2 * t) - 2.0 * at(k, t) + 2.0 * at(k, -t) - at(k, -2 * t))) / (2.0 * t ** 3)
        tol = h * h * d3 / 6.0 + EPS * hps[0] / h
        a, b = np.array(xp), np.array(xp)
        a[:, k] += h
        b[:, k] -= h
        fd = (host_kernel(name, a, xd, hps) - host_kernel(name, b, xd, hps)) / (2.0 * h)
        err = np.max(np.abs(got[k] - fd))
        print(f"{name} d={d} k={k}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol


def test_kernel_dx_rbf_one_dimension_exact():
    """RBF, d = 1: dk/dx = -k D / l^2 with k from the host kernel, to a few ulp (8: the two evaluate exp at arguments that differ by
    an ulp of r^2 / 2 <= 4, and round the products in another order)"""
    rng = np.random.default_rng(5)
    xp, xd = rng.random((9, 1)), rng.random((50, 1))
    for name in ("rbf_ard", "rbf_iso"):
        hps = np.array([0.9, 0.37])
        want = -host_kernel(name, xp, xd, hps) * (xp[:, None, 0] - xd[None, :, 0]) / hps[1] ** 2
        got = K.kernel_dx(name, xp, xd, hps)[0]
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)) <= 8 * EPS


def test_kernel_dx_rejects_unknown_names():
    with pytest.raises(ValueError):
        K.kernel_dx("exponential", np.zeros((1, 1)), np.zeros((1, 1)), np.array([1.0, 1.0]))


def test_library_exports_the_entry_points_and_sizes_the_scratch():
    """fvgp_hip_posterior_grad, its size query and fvgp_hip_potrs_cols are exported and bound; the scratch is one partial per slice of
    256 data rows, sum and point: ceil(n / 256) (2 + 2 n_dirs) P doubles, -1 for arguments the call would refuse"""
    import ctypes
    from fvgp_amd import _lib
    for n, P, nd in ((1, 1, 1), (256, 130, 2), (257, 1000, 3), (20000, 4096, 16)):
        assert _lib.posterior_grad_workspace_bytes(n, P, nd) == -(-n // 256) * (2 + 2 * nd) * P * 8
    L = _lib.lib()
    for s in ("fvgp_hip_posterior_grad", "fvgp_hip_posterior_grad_workspace_bytes", "fvgp_hip_potrs_cols"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.fvgp_hip_posterior_grad_workspace_bytes.restype is ctypes.c_int64
    assert len(L.fvgp_hip_posterior_grad.argtypes) == 21
    assert hasattr(_lib.Handle, "posterior_grad") and hasattr(_lib.Handle, "potrs_cols")
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 17)):
        assert _lib.posterior_grad_workspace_bytes(*bad) == -1


def test_closed_form_posterior_derivatives_match_the_reference_richardson():
    """dm/dx = dk/dx^T alpha and dv/dx = -2 dk/dx^T KV^-1 k with kernel_dx and a numpy solve, against the 4-point Richardson derivative
    of the REFERENCE's posterior (fixture G12) within ten times the error estimate stored in the fixture: the formulas of
    GP.posterior_gradients are right before any device code runs."""
    fx = load_golden("G12_posterior_grad_richardson.npz")
    x, y, nv, th, xp = fx["x"], fx["y"], fx["noise_variances"], fx["theta"], fx["x_pred"]
    for name in ("rbf_ard", "matern52_ard"):
        KV = host_kernel(name, x, x, th) + np.diag(nv)
        k = host_kernel(name, x, xp, th)                       # (N, P)
        alpha = np.linalg.solve(KV, y - np.mean(y))
        W = np.linalg.solve(KV, k)
        dk = K.kernel_dx(name, xp, x, th)                      # (D, P, N)
        dm = np.einsum("dpn,n->pd", dk, alpha)
        dv = -2.0 * np.einsum("dpn,np->pd", dk, W)
        for tag, got in (("m", dm), ("v", dv)):
            vals, h, err = fx[f"{name}_{tag}_vals"], float(fx[f"{name}_{tag}_h"]), float(fx[f"{name}_{tag}_err"])
            rich = ((vals[:, 0] - 8.0 * vals[:, 1] + 8.0 * vals[:, 2] - vals[:, 3]) / (12.0 * h)).T     # (P, D)
            e = np.max(np.abs(got - rich))
            print(f"{name} d{tag}/dx: |closed form - Richardson| {e:.3e}, fixture estimate {err:.3e}")
            assert e <= 10.0 * err
