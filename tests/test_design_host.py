"""The numpy twin of the greedy batch selection (tests/design_ref.py) against exact conditioning, the information-gain identity, the
gap precondition of the fixtures the GPU tests compare indices on, and the repeat and exhaustion rules.  No GPU."""
import numpy as np
import pytest

import design_ref as dr
from fvgp_amd import _lib, gp_design


def _case_a():
    rng = np.random.default_rng(11)
    n, d, P = 200, 2, 300
    x, V = rng.random((n, d)), rng.uniform(0.01, 0.02, n)
    theta = np.concatenate([[dr.SIGMA2], rng.uniform(0.3, 0.6, d)])
    return "rbf_ard", x, theta, V, rng.random((P, d)), np.full(P, 0.05), 12, 0


def _case_b():
    rng = np.random.default_rng(12)
    n, d, P = 130, 3, 257
    x, V = rng.random((n, d)), rng.uniform(0.01, 0.02, n)
    theta = np.concatenate([[dr.SIGMA2], rng.uniform(0.3, 0.6, d)])
    return "rbf_ard", x, theta, V, rng.random((P, d)), rng.uniform(0.02, 0.2, P), 16, 1


@pytest.mark.parametrize("case", [_case_a, _case_b], ids=["n200-d2-P300-q12-variance", "n130-d3-P257-q16-information"])
def test_twin_matches_brute_force_conditioning(case):
    """Append the picked points, with their noise, to the data: the oracle's posterior variance at every candidate is the twin's
    `var` to 1e-12 sigma^2 (the twin deviates by a few 1e-15 sigma^2: two Cholesky routes to the same number), and the last cumulative
    information gain is 1/2 (logdet KV_aug - logdet KV - sum log noise_selected) to 1e-11."""
    kernel, x, theta, V, xc, noise, q, crit = case()
    ref = dr.select_batch_ref(kernel, x, theta, V, xc, q, noise=noise, criterion=crit)
    assert ref["m"] == q and not ref["exhausted"]
    picks = ref["indices"]
    v_bf, logdet_aug = dr.brute_force_after(kernel, x, theta, V, xc, picks, noise)
    dev = float(np.max(np.abs(ref["var"] - np.maximum(v_bf, 0.0)))) / dr.SIGMA2
    print(f"DESIGN|twin_vs_brute_force|{kernel}|n={len(x)}|P={len(xc)}|q={q}|criterion={crit}|dev_over_sigma2={dev:.3e}")
    assert dev <= 1e-12
    gain = 0.5 * np.sum(np.log1p(ref["pick_var"] / noise[picks]))
    want = 0.5 * (logdet_aug - dr.logdet_KV(kernel, x, theta, V) - np.sum(np.log(noise[picks])))
    print(f"DESIGN|information_gain_identity|criterion={crit}|gain={gain:.12f}|logdet_route={want:.12f}|diff={abs(gain - want):.3e}")
    assert abs(gain - want) <= 1e-11
    # G is the pivoted factor: what the batch removes from every variance
    assert np.max(np.abs(ref["var0"] - np.sum(ref["G"] ** 2, axis=0) - ref["var"])) <= 1e-12 * dr.SIGMA2


def test_fixtures_do_not_sit_on_a_near_tie():
    """The GPU tests compare indices exactly, so at every step of every fixture the best admissible score must lead the second best
    by at least 1e-8 sigma^2, 100 x the 1e-10 sigma^2 the device's variances are held to; and no fixture may run out of candidates."""
    worst = np.inf
    for fx in dr.ALL_FIXTURES:
        _, ref = dr.run_fixture(fx)
        assert ref["m"] == fx["q"], dr.fixture_id(fx)
        gap = float(np.min(ref["gaps"]))
        worst = min(worst, gap)
        assert gap >= 1e-8 * dr.SIGMA2, (dr.fixture_id(fx), gap)
    _, _, ref = dr.fvgp_case()
    assert ref["m"] == 8 and float(np.min(ref["gaps"])) >= 1e-8 * dr.SIGMA2
    print(f"DESIGN|fixture_gaps|fixtures={len(dr.ALL_FIXTURES) + 1}|smallest_gap_over_sigma2={worst / dr.SIGMA2:.3e}")


def test_workspace_and_criteria_of_the_product():
    """what needs no GPU of the product: the criterion numbers the facade hands to the ABI are the twin's, GP carries select_batch,
    and the workspace is O(P q) -- the partial sums stop growing at 65 536 candidates, nothing grows like P^2."""
    import fvgp_amd
    assert gp_design.CRITERIA == {"variance": 0, "information": 1} and callable(fvgp_amd.GP.select_batch)
    L = _lib.lib()
    assert hasattr(L, "fvgp_hip_select_batch")
    wb = _lib.select_workspace_bytes
    assert wb(0, 5, 2) == -1 and wb(5, 0, 2) == -1 and wb(5, 5, 0) == -1
    for n, P, q in ((1, 1, 1), (513, 300, 17), (20000, 100000, 64), (20000, 1000000, 64)):
        need = (q * P + -(-n // 256) * min(P, 65536) + _lib.pad128(n)) * 8
        assert need <= wb(n, P, q) <= need + 8 * (3 * -(-P // 64) + P // 8 + 64), (n, P, q)
    assert wb(20000, 1000000, 64) - wb(20000, 500000, 64) <= 500000 * (64 * 8 + 2)      # linear in P beyond the block


def test_fixture_list_covers_the_shapes():
    ns = {fx["n"] for fx in dr.ABI_FIXTURES}
    Ps = {fx["P"] for fx in dr.ABI_FIXTURES}
    assert ns == {1, 127, 128, 129, 257, 513} and Ps == {1, 63, 64, 65, 300}
    assert {(fx["n"], fx["P"]) for fx in dr.ABI_FIXTURES} >= {(n, P) for n in ns for P in Ps}
    assert {fx["q"] for fx in dr.ABI_FIXTURES} >= {1, 5, 17}
    assert {(fx["kernel"], fx["d"]) for fx in dr.ABI_FIXTURES} >= {(k, d) for k in dr.KERNELS for d in (1, 2, 3, 5)}
    assert {fx["mode"] for fx in dr.ABI_FIXTURES} == set(dr.MODES)
    for v, key in ((ns, "n"), (Ps, "P")):
        for val in v:
            assert {fx["mode"] for fx in dr.ABI_FIXTURES if fx[key] == val} == set(dr.MODES), (key, val)


def test_repeat_and_exhaustion_rules():
    rng = np.random.default_rng(5)
    n, d, P = 60, 2, 40
    x, V = rng.random((n, d)), rng.uniform(0.01, 0.02, n)
    theta = np.array([dr.SIGMA2, 0.4, 0.5])
    xc = rng.random((P, d))
    noise = np.full(P, 0.05)
    a = dr.select_batch_ref("matern52_ard", x, theta, V, xc, 30, noise=noise)
    assert a["m"] == 30 and len(set(a["indices"].tolist())) == 30                      # without repeats the indices are distinct
    b = dr.select_batch_ref("matern52_ard", x, theta, V, xc, 30, noise=noise, allow_repeats=True)
    assert b["m"] == 30 and len(set(b["indices"].tolist())) < 30                       # with repeats and noise a point recurs
    v_bf, _ = dr.brute_force_after("matern52_ard", x, theta, V, xc, b["indices"], noise)
    assert np.max(np.abs(b["var"] - v_bf)) <= 1e-12 * dr.SIGMA2                        # ... and a repeat conditions as a measurement does
    # zero noise, every point twice: a picked point's twin drops to zero variance with it
    xc2 = np.vstack([xc[:10], xc[:10]])
    for repeats in (False, True):
        c = dr.select_batch_ref("matern52_ard", x, theta, V, xc2, len(xc2), noise=None, allow_repeats=repeats)
        assert c["exhausted"] and c["m"] <= len(xc2) // 2
        assert np.all(c["indices"][c["m"]:] == -1) and np.all(c["indices"][:c["m"]] >= 0)
        assert len(set((c["indices"][:c["m"]] % 10).tolist())) == c["m"]
