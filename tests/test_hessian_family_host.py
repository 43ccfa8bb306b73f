"""The two isolating tests of tests/test_gpu_hessian_family.py without a GPU: which <KIND, D> cells and host layouts their cases reach,
the float64 twin of the second-derivative pass inside the derived bound on all 36 cases, the two assumptions the bound rests on (terms
of one sign; the mean sensitivity to r^2), three planted errors each outside the bound wherever they act, the resolution of the bound in
a relative perturbation of c2, and the same for the bracket: twin inside, planted error outside.

W here is the float64 inverse of the case's KV with the device test's scaling applied (the device test reads the device's own W back)."""
import functools

import numpy as np
import pytest

import hessian_ref as hr
import kernel_family_ref as kf

LD = np.longdouble
KINDS = ("rbf", "matern32", "matern52")
# the smallest power of ten by which c2 may be off, relatively, for the pass bound to catch it on EVERY case of the kind -- measured on
# the float64 twin against longdouble; at d >= 2 with a length scale per dimension 1e-13 is caught too
C2_DELTA_CAUGHT = {"rbf": 1e-12, "matern32": 1e-12, "matern52": 1e-12}


def _host_w(name, d, shift):
    x, theta, V, _, u = hr.pass_inputs(name, d)
    KV = np.asarray(kf.k_ref(name, x, x, theta, np.float64)) + np.diag(V)
    W = np.linalg.inv(KV)
    return x, theta, (W + W.T) / 2 * 2.0 ** (-2 * shift), u * 2.0 ** -shift


@functools.lru_cache(maxsize=None)
def _pass(name, d):
    x, theta, W, b = _host_w(name, d, hr.PASS_SHIFT)
    return x, theta, W, b, hr.pass_reference(name, x, theta, W, b)


def _worst(got, R):
    g, raw = got
    return max(float(np.max(np.abs(g - R["g"]) / R["g_bound"])), float(np.max(np.abs(raw - R["raw"]) / R["raw_bound"])))


def test_cases_reach_every_cell_and_both_host_layouts():
    """the 36 cases of the pass test reach all 15 <KIND, D> cells, both layouts of the partial sums and ARD and isotropic in each; the
    15 cases of the bracket test one cell each, ARD and isotropic alternating; dispatch as csrc/kernel_family.h has it"""
    every = {(kind, D) for kind in KINDS for D in (0, 1, 2, 3, 4)}
    cells = [hr.cell(name, d) for name, d in hr.PASS_CASES]
    assert len(hr.PASS_CASES) == 36 and {c[:2] for c in cells} == every
    assert {(c[2], c[3]) for c in cells} == {(lay, iso) for lay in ("packed", "rows") for iso in (False, True)}
    assert {(c[0], c[2], c[3]) for c in cells} == {(k, lay, iso) for k in KINDS for lay in ("packed", "rows") for iso in (False, True)}
    assert hr.cell("rbf_ard", 4)[1:3] == (4, "packed") and hr.cell("rbf_ard", 5)[1:3] == (0, "rows") and hr.cell("rbf_iso", 16)[1:3] == (0, "rows")
    bcells = [hr.cell(name, d) for name, d in hr.BRACKET_CASES]
    assert len(bcells) == 15 and {c[:2] for c in bcells} == every
    assert [c[3] for c in bcells] == [i % 2 == 1 for i in range(15)]
    # the planted pairs: (3, 7) inside diagonal tile (0, 0), (200, 3) inside the interior tile (1, 0); n = 261 has that tile whole
    i0, i1, i2 = hr.DUP_ROWS
    assert i0 // 128 == i1 // 128 == 0 and i2 // 128 == 1 and 2 * 128 <= hr.PASS_N < 3 * 128 and hr.PASS_N % 2 == 1


@pytest.mark.parametrize("name,d", hr.PASS_CASES)
def test_pass_twin_inside_the_bound_and_the_bound_bites(name, d):
    x, theta, W, b, R = _pass(name, d)
    r = _worst(hr.pass_twin(name, x, theta, W, b, R["bracket"]), R)
    # one sign: the magnitude the bound is made of -- sum (|W| + |b b|) |factor| >= sum |terms| -- is at most 4 |sum| for every
    # length-scale sum, so the bound is a bound on the RELATIVE error of the sum
    one_sign = max(float(v[1] / abs(v[0])) for k, v in R["red"].items() if k[0] != "gs")
    sens = max(float(v[2]) for v in R["red"].values())
    off = np.ones(R["raw"].shape, dtype=bool)
    off[0, 0] = False                  # d2K/ds2 = 0: H_00 is the bracket alone, 2^-60 n of the other entries, under its own allowance
    brk = float(np.max(R["bracket_mag"][off] / np.abs(R["raw"])[off]))
    print(f"HESS|pass twin / bound|{name}|{d}|{hr.PASS_N}|{r:.3g} sum|terms| / |sum| {one_sign:.3g} sensitivity {sens:.3g} bracket / |H| {brk:.3g}")
    assert r <= 1.0
    assert one_sign <= 4.0
    assert sens <= hr.SENSITIVITY_CAP
    assert brk <= 2.0 ** -40
    assert np.all(np.isfinite(np.asarray(R["raw"], dtype=np.float64))) and np.all(R["raw_bound"] > 0) and np.all(R["g_bound"] > 0)


@pytest.mark.parametrize("name,d", hr.PASS_CASES)
def test_planted_errors_leave_the_bound(name, d):
    """weight 1 for 2 on the rows of the interior tile (every case); c2 (1 + delta), delta = C2_DELTA_CAUGHT (every case); Q_km read
    at the transposed packed index -- column by column for row by row -- at d = 4, and at d = 3, where the two orders differ in the
    one place (0, 2) <-> (1, 1); and the resolution: the smallest power of ten in c2 that leaves the bound"""
    x, theta, W, b, R = _pass(name, d)
    kind = kf.FAMILY[name][0]
    r_w = _worst(hr.pass_twin(name, x, theta, W, b, R["bracket"], ("weight", None)), R)
    r_c = _worst(hr.pass_twin(name, x, theta, W, b, R["bracket"], ("c2", C2_DELTA_CAUGHT[kind])), R)
    caught = next(e for e in range(-16, -8) if _worst(hr.pass_twin(name, x, theta, W, b, R["bracket"], ("c2", 10.0 ** e)), R) > 1.0)
    print(f"HESS|pass planted / bound|{name}|{d}|{hr.PASS_N}|weight {r_w:.3g} c2 (1 + {C2_DELTA_CAUGHT[kind]:g}) {r_c:.3g} smallest caught 1e{caught}")
    assert r_w > 1.0 and r_c > 1.0
    if d in (3, 4):
        r_t = _worst(hr.pass_twin(name, x, theta, W, b, R["bracket"], ("transposed", None)), R)
        print(f"HESS|pass planted / bound|{name}|{d}|{hr.PASS_N}|transposed index {r_t:.3g}")
        assert r_t > 1.0
    elif d < 3:                        # one order up to d = 2; beyond 4 the layout has no packed row
        assert all(hr._packed_index(d, k, m) == hr._packed_index(d, k, m, True) for k in range(d) for m in range(k, d))


def test_bound_factors():
    assert hr.hess_trace_bound_factor(1) == 75 + 21 + 4 * 5 and hr.hess_trace_bound_factor(16) == 75 + 21 + 4 * 20
    assert hr.bracket_bound_factors(3, 384) == 387 + 76 + 83 + 14
    assert [hr._packed_index(4, k, m) for k in range(4) for m in range(k, 4)] == list(range(10))
    assert sorted(hr._packed_index(4, k, m, True) for k in range(4) for m in range(k, 4)) == list(range(10))


@pytest.mark.parametrize("name,d", hr.BRACKET_CASES)
def test_bracket_twin_inside_and_planted_error_outside(name, d):
    """the float64 twin of the bracket's chain (BLAS products) inside the derived bound; kmat_grad_kernel's isotropic p0 summing d - 1 of
    the d dimensions outside it, on every isotropic case"""
    x, theta, W, b = _host_w(name, d, -hr.PASS_SHIFT)
    ref, bound = hr.bracket_reference(name, x, theta, W, b)
    twin, _ = hr.bracket_reference(name, x, theta, W, b, np.float64)
    r = float(np.max(np.abs(twin - ref) / bound))
    share = float(np.max(bound / np.abs(ref)))
    line = f"HESS|bracket twin / bound|{name}|{d}|{hr.PASS_N}|{r:.3g} bound / |H| {share:.3g}"
    assert np.all(bound > 0) and r <= 1.0
    if kf.FAMILY[name][1]:
        bad, _ = hr.bracket_reference(name, x, theta, W, b, np.float64, plant=True)
        rp = float(np.max(np.abs(bad - ref) / bound))
        line += f" planted {rp:.3g}"
        assert rp > 1.0
    print(line)
