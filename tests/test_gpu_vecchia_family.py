"""Every instantiation of nn_cond_kernel<KIND, D, M, MODE> (csrc/nn.hip) and every list shape include/fvgp_hip_nn.h promises, on the
device (the cases: vecchia_family_ref; their host side: test_vecchia_family_host.py).  The references and the bars are the existing ones
-- longdouble, MARGIN * max(base, FLOOR) from the float64 twins of vecchia_ref, vecchia_grad_ref and vecchia_fisher_ref:
    1. the sweep: all 45 (kind, D, M) cells at the three levels of the likelihood, the runtime dimension at d = 5 and d = 16
    2. lists with junk between the neighbours, inside a canary buffer with an odd leading dimension; rows of junk alone; ld > m
    3. the conditionals entry in prediction mode: xq apart from xr, nq != nr, nr < m, nr == 1, s NULL and given
    4. B = 70 (the sums' (b, column) pairs cross their 64-thread blocks) and thetas wider than the kernel's own hyperparameters
Run with -s for the record lines  VF|case|level|figure=got/bar ..."""
import numpy as np
import pytest

import vecchia_family_ref as fam
import vecchia_fisher_ref as vf
import vecchia_grad_ref as vg
import vecchia_ref as vr
from vecchia_device import FISHER, GRAD, VALUE, _device, _device_fisher, _device_grad, _device_value, _frame_untouched, _framed, _kid, _same

pytestmark = pytest.mark.gpu

ICANARY = -7777
EPS = vr.EPS


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _record(label, level, figs, bars):
    print(f"\nVF|{label}|{level}|" + " ".join(f"{k}={figs[k]:.2e}/{bars[k]:.2e}" for k in bars))


def _judge(H, label, case, x, thetas, idx, m, r, v):
    """The three likelihood entries on (x, thetas, idx, m, r, v) against `case`'s longdouble references under `case`'s bars: info, the
    bit contracts between the levels, the nine figures.  Returns the Fisher call's results."""
    name = case[0]
    B, nth = thetas.shape
    out0, info0, mu0, var0 = _device_value(H, name, x, thetas, idx, m, r, v)
    out1, grad1, info1, mu1, var1, score1 = _device_grad(H, name, x, thetas, idx, m, r, v)
    fis = _device_fisher(H, name, x, thetas, idx, m, r, v)
    out, grad, fisher, info, mu, var, score, rows = fis
    assert info0 == 0 and info1 == 0 and info == 0
    assert _same(out0, out1) and _same(mu0, mu1) and _same(var0, var1), "value and gradient call"
    assert _same(out0, out) and _same(mu0, mu) and _same(var0, var), "value and Fisher call"
    assert _same(score1, score) and _same(grad1, grad), "gradient and Fisher call"
    worst = {"value": dict.fromkeys(vr.FIGURES, 0.0), "grad": dict.fromkeys(vg.FIGURES, 0.0), "fisher": dict.fromkeys(vf.FIGURES, 0.0)}
    for b in range(B):
        assert np.array_equal(fisher[b], fisher[b].T)
        f = {"value": vr.figures(r, (out[b, 0], out[b, 1], out[b, 2], mu[b], var[b]), vr.reference(case)[b]),
             "grad": vg.figures((score[b], grad[b]), vg.reference(case)[b]),
             "fisher": vf.figures((vf.packed_to_full(rows[b], nth), fisher[b]), vf.reference(case)[b])}
        worst = {lv: {k: max(worst[lv][k], f[lv][k]) for k in f[lv]} for lv in f}
    bars = {"value": vr.bars(case), "grad": vg.bars(case), "fisher": vf.bars(case)}
    for lv in worst:
        _record(label, lv, worst[lv], bars[lv])
    for lv in worst:
        for k in bars[lv]:
            assert worst[lv][k] <= bars[lv][k], (lv, k, worst[lv][k], bars[lv][k])
    return fis


# ---- 1. the sweep: every cell, every mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fam.SWEEP_CASES, ids=vr.case_id)
def test_every_instantiation_against_longdouble(H, case):
    """Bars from the float64 twins, never from the device (vecchia_ref, vecchia_grad_ref, vecchia_fisher_ref)."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    _judge(H, vr.case_id(case), case, x, thetas, idx, m, r, v)


# ---- 2. lists with gaps and strides -----------------------------------------------------------------------------------------------------------
def _framed_list(H, idx, pad, fill=None):
    """idx (n, m) inside an int32 canary buffer with a frame row above and below and `pad` more columns: (buffer, the (n, m + pad) view
    whose leading dimension is m + pad).  fill (n, pad): what the columns past m of the view's rows hold instead of the canary."""
    t = H.torch
    n, m = idx.shape
    big = t.full((n + 2, m + pad), ICANARY, dtype=t.int32, device=f"cuda:{H.device}")
    big[1:1 + n, :m] = t.as_tensor(np.ascontiguousarray(idx), device=big.device)
    if fill is not None:
        big[1:1 + n, m:] = t.as_tensor(np.ascontiguousarray(fill), device=big.device)
    return big, big[1:1 + n]


@pytest.mark.parametrize("gap", fam.GAP_CASES, ids=fam.gap_id)
def test_lists_with_gaps_against_the_compact_reference(H, gap):
    """(a) The neighbours of a compact case at sorted random positions among m = 16 / 32 / 64 columns, every sort of junk between them
    (negative, n and past it, both ends of int32), the list a view with an odd leading dimension: every figure within the COMPACT
    case's bars against the compact lists' longdouble reference.  (b) Rows of junk alone have the bits of rows with an empty list, and
    those are mu = 0, var = k(x, x) + v, the sigma^2 terms alone in the score and the Fisher row."""
    case, m = gap
    name, d, n, mc, _ = case
    x, thetas, r, v, _ = vr.case_inputs(case)
    idx = fam.gapped_list(gap)
    pad = 3 if m % 2 == 0 else 4
    big, view = _framed_list(H, idx, pad)
    assert view.stride(0) == m + pad and view.stride(0) % 2 == 1 and view.stride(0) > m
    before = big.cpu().numpy().copy()
    _judge(H, fam.gap_id(gap), case, x, thetas, view, m, r, v)
    after = big.cpu().numpy()
    assert np.array_equal(after, before) and np.all(after[:, m:] == ICANARY) and np.all(after[0] == ICANARY) and np.all(after[-1] == ICANARY)
    # (b) three rows of junk alone against the same rows emptied
    rows_j = [0, n // 2, n - 1]
    junk_rows = np.random.default_rng(31 + m).choice(fam.junk(n), size=(len(rows_j), m)).astype(np.int32)
    a, e = idx.copy(), idx.copy()
    a[rows_j], e[rows_j] = junk_rows, -1
    got = _device_fisher(H, name, x, thetas, a, m, r, v)
    want = _device_fisher(H, name, x, thetas, e, m, r, v)
    assert got[3] == 0 and want[3] == 0 and all(_same(g, w) for g, w in zip(got, want))
    out, grad, fisher, info, mu, var, score, rows = got
    th = thetas[0]
    for i in rows_j:
        dv = th[0] + v[i]
        assert mu[0, i] == 0.0 and var[0, i] == dv, i
        ed2, inv = (r[i] / dv) ** 2, 1.0 / dv
        assert abs(score[0, i, 0] - 0.5 * (ed2 - inv)) <= 4 * EPS * 0.5 * (ed2 + inv) and np.all(score[0, i, 1:] == 0.0), i
        assert abs(rows[0, i, 0] - 0.5 * inv * inv) <= 4 * EPS * 0.5 * inv * inv and np.all(rows[0, i, 1:] == 0.0), i


# m = 15 and m = 63: lane m of the padded block must not read column m of a wider list
STRIDE_CASES = (("rbf_ard", 3, 22, 15, 2), ("matern32_iso", 5, 70, 63, 1), ("matern52_ard", 2, 38, 32, 1))


@pytest.mark.parametrize("case", STRIDE_CASES, ids=vr.case_id)
def test_leading_dimension_past_m_changes_no_bit(H, case):
    """(c) The search's own lists with ld = m + 3 -- the three columns past m hold VALID indices, so that a read past m would show --
    through nn_conditionals and the three likelihood entries: the bits of the ld = m call."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    fill = (np.arange(n)[:, None] + 1 + np.arange(3)[None, :]) % n
    big, view = _framed_list(H, idx, 3, fill.astype(np.int32))
    assert view.stride(0) == m + 3
    before = big.cpu().numpy().copy()
    for level in (VALUE, GRAD, FISHER):
        wide = _device(H, level, name, x, thetas, view, m, r, v)
        tight = _device(H, level, name, x, thetas, idx, m, r, v)
        assert all(_same(a, b) for a, b in zip(wide, tight)), level
    xd, rd, vd = H.to_device(x), H.to_device(r), H.to_device(v)
    res = []
    for lists in (view, H.torch.as_tensor(np.ascontiguousarray(idx), device=xd.device)):
        mbig, mu = _framed(H, B, n)
        vbig, var = _framed(H, B, n)
        assert H.nn_conditionals(_kid(name), xd, xd, thetas, lists, m, rd, vd, mu, var, s=vd) == 0
        assert _frame_untouched(mbig) and _frame_untouched(vbig)
        res.append((mu.cpu().numpy(), var.cpu().numpy()))
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])
    assert _same(res[0][0], tight[4]) and _same(res[0][1], tight[5]), "and the conditionals entry is the likelihood's first half"
    assert np.array_equal(big.cpu().numpy(), before)


# ---- 3. prediction shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fam.PRED_CASES, ids=fam.pred_id)
def test_prediction_shapes_against_longdouble(H, case):
    """Handle.nn_conditionals with xq drawn apart from xr, the lists of vecchia_ref.search_ref over every reference row: mu and d within
    vecchia_family_ref.pred_bars (the recipe of vecchia_ref.bars; nothing in them comes from the device)."""
    name, d, nq, nr, m, with_s, B = case
    xq, xr, thetas, idx, r, v, s = fam.pred_inputs(case)
    xqd, xrd = H.to_device(xq), H.to_device(xr)
    mbig, mu = _framed(H, B, nq)
    vbig, var = _framed(H, B, nq)
    idx_d = H.torch.as_tensor(np.ascontiguousarray(idx), device=xqd.device)
    info = H.nn_conditionals(_kid(name), xqd, xrd, thetas, idx_d, m, H.to_device(r), H.to_device(v), mu, var,
                             s=H.to_device(s) if with_s else None)
    assert info == 0 and _frame_untouched(mbig) and _frame_untouched(vbig)
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    bars = fam.pred_bars(case)
    worst = dict.fromkeys(fam.PRED_FIGURES, 0.0)
    for b in range(B):
        f = fam.pred_figures(r, (mu[b], var[b]), fam.pred_reference(case)[b])
        worst = {k: max(worst[k], f[k]) for k in worst}
    _record(fam.pred_id(case), "pred", worst, bars)
    for k in bars:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])


# ---- 4. batch and hyperparameter-count edges ------------------------------------------------------------------------------------------------------
def test_seventy_thetas_are_seventy_single_calls(H):
    """B = 70, n = 6, m = 3: the (b, column) pairs of the sums -- 140 for the likelihood's pair, 210 for the gradient, 420 for the packed
    Fisher entries -- cross the 64-thread blocks of nn_total_kernel, gridDim.y = 70.  Rows on both sides of every block border are the
    single-theta calls bit for bit, at every level."""
    name, d, n, m, B = "matern52_ard", 2, 6, 3, 70
    x, theta, r, v = vr.case_data(name, d, n)
    idx = vr.search_ref(x, x, m, vr.length_scales(name, theta, d), c0=0)
    thetas = np.array([theta * (0.7 + 0.01 * b) for b in range(B)])
    full = [_device(H, level, name, x, thetas, idx, m, r, v) for level in (VALUE, GRAD, FISHER)]
    for level, res in zip((VALUE, GRAD, FISHER), full):
        info = res[1 + level]
        assert info == 0 and np.all(np.isfinite(res[0])), level
        assert all(_same(a, b) for a, b in zip(res[:level + 1], full[FISHER][:level + 1])), "the host results of a level are the Fisher call's"
    for b in (0, 31, 32, 63, 64, 69):
        for level in (VALUE, GRAD, FISHER):
            one = _device(H, level, name, x, thetas[b], idx, m, r, v)
            for k, (a, f) in enumerate(zip(one, full[level])):
                if k != 1 + level:                                   # (the info word has no batch position)
                    assert _same(a[0], f[b]), (b, level, k)


def _plus_zero(a):
    a = np.asarray(a)
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


@pytest.mark.parametrize("case", [("matern32_ard", 3, 22, 7, 2), ("rbf_iso", 5, 38, 17, 2)], ids=vr.case_id)
def test_hyperparameter_columns_past_the_kernels_own_are_zero(H, case):
    """ntheta two larger than the kernel's count: the extra score and gradient columns, and every packed or mirrored Fisher entry that
    touches one, are +0.0 (the sign bit too); everything else has the bits of the exact-count call."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    own = thetas.shape[1]
    wide = np.concatenate([thetas, np.array([[3.3, -1.0]] * B)], axis=1)
    nth = own + 2
    for level in (VALUE, GRAD, FISHER):
        e = _device(H, level, name, x, thetas, idx, m, r, v)
        w = _device(H, level, name, x, wide, idx, m, r, v)
        assert e[1 + level] == 0 and w[1 + level] == 0
        names = (("out", "info", "mu", "var"), ("out", "grad", "info", "mu", "var", "score"),
                 ("out", "grad", "fisher", "info", "mu", "var", "score", "rows"))[level]
        E, W = dict(zip(names, e)), dict(zip(names, w))
        assert _same(E["out"], W["out"]) and _same(E["mu"], W["mu"]) and _same(E["var"], W["var"]), level
        if level >= GRAD:
            assert W["score"].shape == (B, n, nth) and W["grad"].shape == (B, nth)
            assert _same(W["score"][..., :own], E["score"]) and _same(W["grad"][:, :own], E["grad"]), level
            assert _plus_zero(W["score"][..., own:]) and _plus_zero(W["grad"][:, own:]), level
        if level == FISHER:
            P = own * (own + 1) // 2
            assert W["rows"].shape == (B, n, nth * (nth + 1) // 2) and W["fisher"].shape == (B, nth, nth)
            assert _same(W["rows"][..., :P], E["rows"]) and _plus_zero(W["rows"][..., P:])
            assert _same(W["fisher"][:, :own, :own], E["fisher"])
            assert _plus_zero(W["fisher"][:, own:, :]) and _plus_zero(W["fisher"][:, :, own:])
