"""CPU-only checks of the cases that tests/test_gpu_vecchia_family.py runs on the device (vecchia_family_ref): the sweep reaches every
instantiation of nn_cond_kernel by a Python mirror of the dispatch; the float64 twin is inside the bars it sets, at every sweep case; a
list with gaps and its compacted form have the same longdouble reference; and the checks can fail -- the twin with a planted error is
over the bar in every case where the error can act.  Run with -s for the record lines."""
import contextlib

import numpy as np
import pytest

import kernel_family_ref as kf
import vecchia_family_ref as fam
import vecchia_fisher_ref as vf
import vecchia_grad_ref as vg
import vecchia_ref as vr

LD = vr.LD
LEVELS = ("value", "grad", "fisher")


# ---- 1. the sweep reaches every instantiation ---------------------------------------------------------------------------------------------
def test_sweep_reaches_every_cell_of_the_dispatch():
    C = fam.SWEEP_CASES
    cells = [fam.cell(c[0], c[1], c[3]) for c in C]
    every = {(k, D, M) for k in fam.KINDS for D in (0, 1, 2, 3, 4) for M in fam.PADS}
    assert len(C) == 54 and len(set(C)) == 54 and set(cells) == every and len(every) == 45
    # the mirror itself: the dimensions with an instantiation of their own, the runtime one, the three pads at their borders
    assert [fam.cell("rbf_ard", d, 1)[1] for d in (1, 2, 3, 4, 5, 16)] == [1, 2, 3, 4, 0, 0]
    assert [fam.cell("rbf_ard", 1, m)[2] for m in (1, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64]
    assert {kf.FAMILY[n][0] for n in kf.FAMILY} == set(fam.KINDS)
    # both ends of the runtime dimension, in every (kind, M)
    for d in (5, 16):
        assert {(k, M) for (k, D, M), c in zip(cells, C) if c[1] == d} == {(k, M) for k in fam.KINDS for M in fam.PADS}
    # one length scale and one per dimension: every (D, M) pair and every (kind, D) pair sees both
    iso = [kf.FAMILY[c[0]][1] for c in C]
    for pair in (lambda k, D, M: (D, M), lambda k, D, M: (k, D)):
        seen = {}
        for cl, i in zip(cells, iso):
            seen.setdefault(pair(*cl), set()).add(i)
        assert all(s == {False, True} for s in seen.values()), seen
    # m on both sides of each padded size, every listed value with both sorts of kernel; n with full and short lists, no multiple of 4
    for M in fam.PADS:
        ms = {c[3] for c, cl in zip(C, cells) if cl[2] == M}
        assert ms == set(fam.M_OF[M]) and max(ms) == M and min(ms) == {16: 1, 32: 17, 64: 33}[M]
        assert {c[2] for c, cl in zip(C, cells) if cl[2] == M} == {fam.N_OF[M]} and fam.N_OF[M] > M and fam.N_OF[M] % 4
    for m in {c[3] for c in C}:
        assert {i for c, i in zip(C, iso) if c[3] == m} == {False, True}, m
    assert {c[4] for c in C} == {1, 2} and {cl[2] for c, cl in zip(C, cells) if c[4] == 2} == set(fam.PADS)
    # the old lists and what rests on them stay as they were
    assert len(vr.ACC_CASES) == 16 and len(vg.GRAD_CASES) == 14 and len(vf.CASES) == 11 and vr.MARGIN == vg.MARGIN == vf.MARGIN == 8


def test_gapped_and_prediction_cases_cover_what_they_name():
    G = fam.GAP_CASES
    assert len(G) == 6 and sorted(g[1] for g in G) == [16, 16, 32, 32, 64, 64]
    for M in fam.PADS:
        assert {kf.FAMILY[g[0][0]][1] for g in G if g[1] == M} == {False, True}
    for gap in G:
        case, m = gap
        n, mc = case[2], case[3]
        idx, lists = fam.gapped_list(gap), vr.case_inputs(case)[4]
        assert idx.shape == (n, m) and idx.dtype == np.int32 and mc == {16: 10, 32: 20, 64: 40}[m]
        assert np.array_equal(fam.compacted(idx, n)[:, :mc], lists) and np.all(fam.compacted(idx, n)[:, mc:] == -1)
        hole = ~fam.in_range(idx, n)
        assert set(idx[hole]) == set(fam.junk(n).astype(np.int32)), "every sort of junk occurs"
        full = np.nonzero(fam.in_range(idx, n).sum(axis=1) == mc)[0]
        assert len(full) and np.all(hole[0]) and any(hole[i, :-1].any() and not hole[i, -1] for i in full), "gaps in the middle of a list"
    P = fam.PRED_CASES
    assert len(P) == 8 and {fam.cell(c[0], c[1], c[4])[2] for c in P} == set(fam.PADS)
    assert {c[2] for c in P} == {1, 5, 67} and {c[3] for c in P} == {1, 3, 80} and {c[1] for c in P} == {1, 3, 16}
    assert {c[5] for c in P} == {False, True} and {c[6] for c in P} == {1, 3} and all(c[2] != c[3] or c[2] == 1 for c in P)
    assert any(c[3] < c[4] and c[3] > 1 for c in P) and any(c[3] == 1 for c in P)


# ---- 2. the float64 twin against its own bars ---------------------------------------------------------------------------------------------
def _twin(name, x, theta, idx, r, v):
    """the float64 twin at the three levels: (value run, scores, Fisher rows)"""
    return (vr.loglik_ref(name, x, theta, idx, r, v, np.float64), vg.scores_ref(name, x, theta, idx, r, v, np.float64),
            vf.fisher_rows_ref(name, x, theta, idx, v, np.float64))


def _figures(r, runs, refs):
    """{level: figures} of _twin's three runs against the three longdouble references"""
    return {"value": vr.figures(r, runs[0], refs[0]), "grad": vg.figures(runs[1], refs[1]), "fisher": vf.figures(runs[2], refs[2])}


def _references(case, b=0):
    return vr.reference(case)[b], vg.reference(case)[b], vf.reference(case)[b]


def _bars(case):
    return {"value": vr.bars(case), "grad": vg.bars(case), "fisher": vf.bars(case)}


@pytest.mark.parametrize("case", fam.SWEEP_CASES, ids=vr.case_id)
def test_float64_twin_is_inside_the_bars_it_sets(case):
    """The twin is the bars' source, not an outlier: its plain run is within bar / MARGIN = max(base, FLOOR) at every figure of every
    level, and every bar is finite."""
    name = case[0]
    x, thetas, r, v, idx = vr.case_inputs(case)
    bars = _bars(case)
    for b, t in enumerate(thetas):
        plain = _figures(r, _twin(name, x, t, idx, r, v), _references(case, b))
        for lv in LEVELS:
            print(f"\nvecchia family twin {vr.case_id(case)} b={b} {lv}: " + " ".join(f"{k}={plain[lv][k]:.2e}/{bars[lv][k]:.2e}" for k in bars[lv]))
            for k, bar in bars[lv].items():
                assert np.isfinite(bar) and plain[lv][k] <= bar / vr.MARGIN, (lv, k, plain[lv][k], bar)


@pytest.mark.parametrize("case", fam.PRED_CASES, ids=fam.pred_id)
def test_float64_twin_is_inside_the_prediction_bars(case):
    r = fam.pred_inputs(case)[4]
    bars = fam.pred_bars(case)
    for b in range(case[6]):
        f = fam.pred_figures(r, fam.pred_run(case, b, np.float64), fam.pred_reference(case)[b])
        print(f"\nvecchia family twin {fam.pred_id(case)} b={b}: " + " ".join(f"{k}={f[k]:.2e}/{bars[k]:.2e}" for k in bars))
        for k, bar in bars.items():
            assert np.isfinite(bar) and f[k] <= bar / vr.MARGIN, (k, f[k], bar)


# ---- 3. gapped equals compact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", fam.GAP_CASES, ids=fam.gap_id)
def test_gapped_list_has_the_compact_reference(gap):
    """the three references skip entries outside 0 .. n - 1 wherever they stand: bit for bit the compact case's longdouble results"""
    case, m = gap
    x, thetas, r, v, _ = vr.case_inputs(case)
    idx = fam.gapped_list(gap)
    ll = vr.loglik_ref(case[0], x, thetas[0], idx, r, v, LD)
    ref = vr.reference(case)[0]
    assert all(np.array_equal(a, b) for a, b in zip(ll, ref))
    assert np.array_equal(vg.scores_ref(case[0], x, thetas[0], idx, r, v, LD), vg.reference(case)[0])
    assert np.array_equal(vf.fisher_rows_ref(case[0], x, thetas[0], idx, v, LD), vf.reference(case)[0])


# ---- 4. the checks can fail -----------------------------------------------------------------------------------------------------------------
# Three errors a kernel of this shape could make, planted into the float64 twin.  Where an error acts is a CONDITION on the case, never a
# measurement: `drop` (the last valid neighbour of every row dropped) acts where some row has a neighbour; `zero` (an entry to be skipped
# read as index 0) where some list holds such an entry; `short` (the second dimension left out of an isotropic kernel's length-scale derivative
# sum) is defined for the isotropic kernels, acts on the score and the Fisher rows, and is a no-op at d = 1.
ERRORS = ("drop", "zero", "short")


@contextlib.contextmanager
def _short_derivative():
    keep = kf.dk_dtheta_ref
    kf.dk_dtheta_ref = fam.dk_dtheta_short
    try:
        yield
    finally:
        kf.dk_dtheta_ref = keep


def _defined(error, name):
    return error != "short" or kf.FAMILY[name][1]


def _acts(error, name, d, idx, nr):
    ok = fam.in_range(idx, nr)
    return {"drop": bool(ok.any()), "zero": bool((~ok).any()), "short": kf.FAMILY[name][1] and d >= 2 and bool(ok.any())}[error]


def _planted_likelihood(error, name, x, theta, idx, r, v, refs):
    """{level: figures} of the float64 twin with `error` planted, against the longdouble references of the true lists"""
    n = len(x)
    if error == "short":
        with _short_derivative():
            runs = _twin(name, x, theta, idx, r, v)
        f = _figures(r, runs, refs)
        return {lv: f[lv] for lv in ("grad", "fisher")}
    bad = fam.drop_last(idx, n) if error == "drop" else fam.gaps_as_zero(idx, n)
    return _figures(r, _twin(name, x, theta, bad, r, v), refs)


def _over(figs, bars):
    """the figures that are over their bars"""
    return [k for k in bars if figs[k] > bars[k]]


def _check_likelihood(label, name, d, x, theta, idx, r, v, refs, bars):
    for error in ERRORS:
        if not _defined(error, name):
            continue
        got = _planted_likelihood(error, name, x, theta, idx, r, v, refs)
        if not _acts(error, name, d, idx, len(x)):
            for lv in got:
                assert not _over(got[lv], bars[lv]), ("a no-op stays inside the bars", error, lv)
            continue
        for lv in got:
            print(f"\nvecchia family planted {error} {label} {lv}: " + " ".join(f"{k}={got[lv][k]:.2e}/{bars[lv][k]:.2e}" for k in bars[lv]))
            assert _over(got[lv], bars[lv]), (error, lv, got[lv], bars[lv])


@pytest.mark.parametrize("case", fam.SWEEP_CASES, ids=vr.case_id)
def test_planted_errors_are_over_the_bar_in_the_sweep(case):
    name, d = case[0], case[1]
    x, thetas, r, v, idx = vr.case_inputs(case)
    refs, bars = _references(case), _bars(case)        # (before anything is planted: both are cached)
    _check_likelihood(vr.case_id(case), name, d, x, thetas[0], idx, r, v, refs, bars)


@pytest.mark.parametrize("gap", fam.GAP_CASES, ids=fam.gap_id)
def test_planted_errors_are_over_the_bar_in_the_gapped_cases(gap):
    case, m = gap
    x, thetas, r, v, _ = vr.case_inputs(case)
    refs, bars = _references(case), _bars(case)
    _check_likelihood(fam.gap_id(gap), case[0], case[1], x, thetas[0], fam.gapped_list(gap), r, v, refs, bars)


@pytest.mark.parametrize("case", fam.PRED_CASES, ids=fam.pred_id)
def test_planted_errors_are_over_the_bar_in_the_prediction_cases(case):
    """prediction has mu and d alone: `short` has nothing to act on and is not counted"""
    name, d, nq, nr = case[:4]
    idx, r = fam.pred_inputs(case)[3], fam.pred_inputs(case)[4]
    ref, bars = fam.pred_reference(case)[0], fam.pred_bars(case)
    for error, bad in (("drop", fam.drop_last(idx, nr)), ("zero", fam.gaps_as_zero(idx, nr))):
        f = fam.pred_figures(r, fam.pred_run(case, 0, np.float64, idx=bad), ref)
        if not _acts(error, name, d, idx, nr):
            assert np.array_equal(bad, idx) and not _over(f, bars)
            continue
        print(f"\nvecchia family planted {error} {fam.pred_id(case)}: " + " ".join(f"{k}={f[k]:.2e}/{bars[k]:.2e}" for k in bars))
        assert _over(f, bars), (error, f, bars)


def test_few_cases_are_excluded_from_the_sensitivity_check():
    """per planted error, over the cases of the three sections it is defined for: the share where it is a no-op stays below one in four"""
    lik = [(c[0], c[1], vr.case_inputs(c)[4], c[2]) for c in fam.SWEEP_CASES]
    lik += [(g[0][0], g[0][1], fam.gapped_list(g), g[0][2]) for g in fam.GAP_CASES]
    pred = [(c[0], c[1], fam.pred_inputs(c)[3], c[3]) for c in fam.PRED_CASES]
    for error in ERRORS:
        pool = [c for c in (lik if error == "short" else lik + pred) if _defined(error, c[0])]
        out = [c for c in pool if not _acts(error, *c)]
        print(f"\nvecchia family sensitivity {error}: {len(out)} of {len(pool)} cases excluded")
        assert len(pool) >= 30 and 4 * len(out) < len(pool), (error, len(out), len(pool))
