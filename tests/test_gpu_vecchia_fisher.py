"""The Fisher information of the nearest-neighbour likelihood on the device (include/fvgp_hip_nn.h: fvgp_hip_nn_loglik_fisher;
fvgp_amd/gp_vecchia.py): the rows and their sum against longdouble under bars that come from the float64 twin (vecchia_fisher_ref:
MARGIN * max(base, FLOOR)); the bit contracts; the sum against the dense GP's Fisher matrix where the approximation is exact; failure
reporting; the argument rules; the facade, Fisher-scoring training and the Laplace approximation.  Run with -s for the record lines."""
import ctypes

import numpy as np
import pytest

import vecchia_fisher_ref as vf
import vecchia_ref as vr
from vecchia_device import CANARY, _device_fisher, _device_grad, _frame_untouched, _framed, _same

pytestmark = pytest.mark.gpu

LD = vr.LD


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


# ---- 1. accuracy against longdouble ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vf.CASES, ids=vr.case_id)
def test_rows_and_sum_against_longdouble(H, case):
    """Bars from the float64 twin, never from the device: both figures <= MARGIN * max(base, FLOOR) (vecchia_fisher_ref)."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    nth = thetas.shape[1]
    out, grad, fisher, info, mu, var, score, rows = _device_fisher(H, name, x, thetas, idx, m, r, v)
    assert info == 0 and rows.shape == (B, n, nth * (nth + 1) // 2) and fisher.shape == (B, nth, nth)
    bars = vf.bars(case)
    worst = dict.fromkeys(vf.FIGURES, 0.0)
    for b in range(B):
        assert np.array_equal(fisher[b], fisher[b].T)
        f = vf.figures((vf.packed_to_full(rows[b], nth), fisher[b]), vf.reference(case)[b])
        worst = {k: max(worst[k], f[k]) for k in vf.FIGURES}
    print(f"\nvecchia fisher device {vr.case_id(case)}: " + " ".join(f"{k}={worst[k]:.2e}/{bars[k]:.2e}" for k in vf.FIGURES))
    # everything else is the gradient call's, bit for bit
    out0, grad0, info0, mu0, var0, score0 = _device_grad(H, name, x, thetas, idx, m, r, v)
    assert info0 == 0 and _same(out, out0) and _same(grad, grad0) and _same(mu, mu0) and _same(var, var0) and _same(score, score0)
    for k in vf.FIGURES:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])


# ---- 2. bit contracts ------------------------------------------------------------------------------------------------------------------------
def test_bit_contracts(H):
    case = ("matern52_ard", 3, 200, 33, 3)
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    first = _device_fisher(H, name, x, thetas, idx, m, r, v)
    out, grad, fisher, info, mu, var, score, rows = first
    again = _device_fisher(H, name, x, thetas, idx, m, r, v)
    assert info == 0 and all(_same(a, b) for a, b in zip(first, again)), "the call twice"
    g = _device_grad(H, name, x, thetas, idx, m, r, v)
    assert all(_same(a, b) for a, b in zip((out, grad, info, mu, var, score), g)), "out / grad / info / mu / var / score are nn_loglik_grad's"
    for b in range(B):
        one = _device_fisher(H, name, x, thetas[b], idx, m, r, v)
        assert all(_same(a[0], full[b]) for a, full in zip((one[0], one[1], one[2], one[4], one[5], one[6], one[7]),
                                                           (out, grad, fisher, mu, var, score, rows))), b
    perm = np.array([2, 0, 1])
    p = _device_fisher(H, name, x, thetas[perm], idx, m, r, v)
    assert all(_same(a, full[perm]) for a, full in zip((p[0], p[1], p[2], p[4], p[5], p[6], p[7]), (out, grad, fisher, mu, var, score, rows)))
    # a row alone: the call over the same rows with every other list emptied, and the row as the last one of a shorter call
    for i in (0, 1, 33, 130, 199):
        alone = np.full_like(idx, -1)
        alone[i] = idx[i]
        r1 = _device_fisher(H, name, x, thetas, alone, m, r, v)[7]
        assert _same(r1[:, i], rows[:, i]), i
        r2 = _device_fisher(H, name, x[:i + 1], thetas, idx[:i + 1], m, r[:i + 1], v[:i + 1])[7]
        assert _same(r2[:, i], rows[:, i]), i
    # the Fisher information is an expectation over the data: other data, the same bits (the scores change)
    other = np.cos(17.0 * np.arange(n)) * 3.0
    o = _device_fisher(H, name, x, thetas, idx, m, other, v)
    assert _same(o[7], rows) and _same(o[2], fisher) and _same(o[5], var) and not _same(o[6], score)


def _documented_sum(col):
    """the header's order in float64: slices of 256 rows (the last one padded with 0.0) by the halving tree, the slices to 0 ascending"""
    a = np.zeros((len(col) + 255) // 256 * 256)
    a[:len(col)] = col
    s = np.float64(0.0)
    for t in a.reshape(-1, 256):
        for off in (128, 64, 32, 16, 8, 4, 2, 1):
            t[:off] += t[off:2 * off]
        s += t[0]
    return s


@pytest.mark.parametrize("n", [1, 256, 257])
def test_summation_order(H, n):
    """grad and fisher are the documented sums of score and fisher_rows, bit for bit: a lone row, a full slice, a second slice of one row;
    with B = 2 and 3 / 6 columns, every stride of the partial sums.  (fit and logdet: the device's division and log are not numpy's.)"""
    name, d, m, B = "matern32_ard", 2, 2, 2
    rng = np.random.default_rng(2600 + n)
    x, r, v = rng.random((n, d)), rng.standard_normal(n), 0.01 + 0.05 * rng.random(n)
    thetas = np.array([[1.0, 0.3, 0.4], [1.7, 0.5, 0.2]])
    xd = H.to_device(x)
    idx = H.torch.empty((n, m), dtype=H.torch.int32, device=xd.device)
    H.nn_search(xd, xd, m, idx, c0=0)
    out, grad, fisher, info, mu, var, score, rows = _device_fisher(H, name, x, thetas, idx.cpu().numpy(), m, r, v)
    nth = thetas.shape[1]
    assert info == 0 and score.shape == (B, n, nth) and rows.shape == (B, n, nth * (nth + 1) // 2)
    for b in range(B):
        for h in range(nth):
            assert grad[b, h] == _documented_sum(score[b, :, h]), (b, h)
            for k in range(h + 1):
                assert fisher[b, h, k] == _documented_sum(rows[b, :, h * (h + 1) // 2 + k]), (b, h, k)
        assert np.array_equal(fisher[b], fisher[b].T), b


# ---- 3. exactness ------------------------------------------------------------------------------------------------------------------------------
def test_sum_is_the_dense_fisher_matrix_when_every_earlier_point_is_a_neighbour(H):
    """n = 65, m = 64 on the given order: the product of conditionals is the exact likelihood, so the rows telescope to the dense
    1/2 tr((K + V)^-1 d_h K (K + V)^-1 d_k K)."""
    case = vf.EXACT_CASE
    name, d, n, m, _ = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    assert all(set(idx[i][idx[i] >= 0]) == set(range(i)) for i in range(n)), "every earlier point is a neighbour"
    out, grad, fisher, info, *_ = _device_fisher(H, name, x, thetas, idx, m, r, v)
    exact = vf.dense_fisher_ld(name, x, thetas[0], v)
    dg = np.sqrt(np.diagonal(exact))
    err = float(np.max(np.abs(np.asarray(fisher[0], dtype=LD) - exact) / np.outer(dg, dg)))
    bar = vf.bars(case)["total"]
    print(f"\nvecchia fisher exactness n=65 m=64: device vs dense longdouble {err:.2e}/{bar:.2e}")
    assert info == 0 and err <= bar


# ---- 4. failure reporting ------------------------------------------------------------------------------------------------------------------------
def test_failure_is_reported_not_trapped(H):
    """The singular construction of test_gpu_vecchia_grad.py: zero noise and a duplicated point among row 20's neighbours, sigma^2 a
    power of four, so that the second pivot is exactly 0.  A numerical condition that the kernel reports: a NaN row of fisher_rows at
    both thetas, the gradient call's info, a NaN fisher_host; every other row is what it is in a call without the singular list."""
    name, d, n, m = "rbf_ard", 2, 40, 16
    x, theta, r, _ = vr.case_data(name, d, n)
    x = x.copy()
    x[7] = x[3]
    v0 = np.zeros(n)
    idx = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        prev = np.arange(i)[-3:][::-1]
        idx[i, :len(prev)] = prev
    idx[20, :3] = [3, 7, 5]
    thetas = np.array([np.concatenate([[4.0], theta[1:]]), np.concatenate([[1.0], 1.5 * theta[1:]])])
    out, grad, fisher, info, mu, var, score, rows = _device_fisher(H, name, x, thetas, idx, m, r, v0)
    bad = np.isnan(rows).any(axis=2)
    assert np.all(np.isnan(rows[:, 20])) and bad[0, 20] and bad[1, 20] and bad.sum() == 2
    assert info == 1 + 0 * n + 20 and np.all(np.isnan(fisher)) and np.all(np.isnan(grad)) and np.all(np.isnan(out[:, 0]))
    g = _device_grad(H, name, x, thetas, idx, m, r, v0)
    assert g[2] == info and all(_same(a, b) for a, b in zip((out, grad, info, mu, var, score), g))
    idx2 = idx.copy()
    idx2[20, :3] = [3, 5, -1]
    out2, grad2, fisher2, info2, mu2, var2, score2, rows2 = _device_fisher(H, name, x, thetas, idx2, m, r, v0)
    keep = np.arange(n) != 20
    assert info2 == 0 and np.all(np.isfinite(fisher2)) and np.all(np.isfinite(rows2))
    assert _same(rows2[:, keep], rows[:, keep])


# ---- 5. argument rules ------------------------------------------------------------------------------------------------------------------------
def test_argument_rules(H):
    """a bad argument returns minus its position before anything is launched: outputs, workspace and host results stay as they were"""
    from fvgp_amd import _lib
    L = _lib.lib()
    n, m, B, nth = 10, 4, 2, 4
    P_ = nth * (nth + 1) // 2
    t = H.torch
    x = H.to_device(np.random.default_rng(1).random((n, 3)))
    rr = np.linspace(-1.0, 1.0, n)
    r, v = H.to_device(rr), H.to_device(np.ones(n))
    idx = t.full((n, m), -1, dtype=t.int32, device=x.device)
    mbig, mu = _framed(H, B, n)
    vbig, var = _framed(H, B, n)
    sbig, score = _framed(H, B, n, nth)
    fbig, rows = _framed(H, B, n, P_)
    wb = _lib.nn_fisher_workspace_bytes(n, B, nth)
    work = t.full((wb // 8,), CANARY, dtype=t.float64, device=x.device)
    th = np.array([[1.0, 1.0, 1.0, 1.0], [3.0, 0.5, 2.0, 1.0]])
    out, grad, fisher = np.full((B, 3), CANARY), np.full((B, nth), CANARY), np.full((B, nth, nth), CANARY)
    info = ctypes.c_int64(-5)
    P = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    tp = th.ctypes.data_as(_lib.P_d)

    def call(**kw):
        a = dict(h=H._h, kid=1, x=P(x), n=n, d=3, th=tp, nt=nth, B=B, idx=P(idx), ld=m, m=m, r=P(r), v=P(v), mu=P(mu), var=P(var),
                 score=P(score), rows=P(rows), w=P(work), wb=wb, out=out.ctypes.data_as(_lib.P_d), grad=grad.ctypes.data_as(_lib.P_d),
                 fisher=fisher.ctypes.data_as(_lib.P_d), info=ctypes.byref(info))
        a.update(kw)
        return L.fvgp_hip_nn_loglik_fisher(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=-1)), (-2, dict(kid=6)), (-3, dict(x=None)), (-4, dict(n=0)), (-4, dict(n=2 ** 31)),
                     (-5, dict(d=0)), (-5, dict(d=17)), (-6, dict(th=None)), (-7, dict(nt=3)), (-8, dict(B=0)), (-8, dict(B=65536)),
                     (-9, dict(idx=None)), (-10, dict(ld=3)), (-11, dict(m=0)), (-11, dict(m=65)), (-12, dict(r=None)), (-13, dict(v=None)),
                     (-14, dict(mu=None)), (-15, dict(var=None)), (-16, dict(score=None)), (-17, dict(rows=None)), (-18, dict(w=None)),
                     (-18, dict(w=ctypes.c_void_p(work.data_ptr() + 4))), (-19, dict(wb=wb - 1)),
                     (-19, dict(wb=_lib.nn_grad_workspace_bytes(n, B, nth))), (-20, dict(out=None)), (-21, dict(grad=None)),
                     (-22, dict(fisher=None)), (-23, dict(info=None))):
        assert call(**kw) == code, (code, kw)
    H.sync()
    assert info.value == -5 and np.all(out == CANARY) and np.all(grad == CANARY) and np.all(fisher == CANARY)
    assert np.all(work.cpu().numpy() == CANARY) and all(np.all(b.cpu().numpy() == CANARY) for b in (mbig, vbig, sbig, fbig))
    # and the good call: rows without neighbours have 1/2 delta delta^T / d^2 alone, delta = (1, 0, ..), d = sigma^2 + v
    assert call() == 0 and info.value == 0
    f = rows.cpu().numpy()
    for b in range(B):
        want = 0.5 / (th[b, 0] + 1.0) ** 2
        assert np.all(np.abs(f[b, :, 0] - want) <= 4 * vr.EPS * want) and np.all(f[b, :, 1:] == 0.0)
        assert abs(fisher[b, 0, 0] - n * want) <= 16 * vr.EPS * n * want
        assert np.all(fisher[b].ravel()[1:] == 0.0)
    assert all(_frame_untouched(b) for b in (mbig, vbig, sbig, fbig))


# ---- 6. the facade ------------------------------------------------------------------------------------------------------------------------------
FACADE_CASE = ("matern32_ard", 3, 200, 17, 1)
BOUNDS = np.array([[0.1, 10.0]] + [[0.05, 5.0]] * 3)


def _facade(case=FACADE_CASE, **kw):
    import fvgp_amd
    name, d, n, m, _ = case
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    return fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, **kw), y, x, theta, v


def _inside(t):
    return np.all(np.asarray(t) >= BOUNDS[:, 0]) and np.all(np.asarray(t) <= BOUNDS[:, 1])


def test_facade_fisher_information_rows_and_batches(H):
    name, d, n, m, _ = FACADE_CASE
    gp, y, x, theta, v = _facade(seed=5)
    perm = gp.ordering
    F = gp.fisher_information()
    assert F.shape == (d + 1, d + 1) and np.array_equal(F, F.T) and np.linalg.eigvalsh(F)[0] > 0.0
    rows = gp.conditional_fisher()
    dg = np.sqrt(np.diag(F))
    assert rows.shape == (n, d + 1, d + 1) and np.all(np.abs(np.sum(rows, axis=0) - F) <= 1e-13 * np.outer(dg, dg))
    # the plumbing (ordering, packing): the twin's rows in the caller's order; the accuracy proper is section 1's
    xo, vo = x[perm], v[perm]
    idx = vr.search_ref(xo, xo, m, vr.length_scales(name, theta, d), c0=0)
    ref = np.empty((n, d + 1, d + 1))
    ref[perm] = np.asarray(vf.fisher_rows_ref(name, xo, theta, idx, vo, LD), dtype=np.float64)
    sd = np.sqrt(np.einsum("ihh->ih", ref))
    assert np.all(np.abs(rows - ref) <= vr.MARGIN * 1e-12 * np.max(sd[:, :, None] * sd[:, None, :], axis=0))
    f, g, F1 = gp.neg_log_likelihood_gradient_and_fisher()
    f0, g0 = gp.neg_log_likelihood_and_gradient()
    assert f == f0 and np.array_equal(g, g0) and np.array_equal(F1, F)
    # batch rows are the single calls bit for bit, whatever the chunking, and the state is untouched
    thetas = vr.batch_thetas(theta, 3)
    fb, G, FB = gp.neg_log_likelihood_gradient_and_fisher_batch(thetas)
    assert fb.shape == (3,) and G.shape == thetas.shape and FB.shape == (3, d + 1, d + 1)
    for b in range(3):
        f1, g1, F1 = gp.neg_log_likelihood_gradient_and_fisher(thetas[b])
        assert f1 == fb[b] and np.array_equal(g1, G[b]) and np.array_equal(F1, FB[b]), b
    assert np.array_equal(gp.hyperparameters, theta)
    nth = len(theta)
    gp.args["grad_batch_bytes"] = 8 * n * (2 + nth + nth * (nth + 1) // 2)          # one hyperparameter vector per call
    assert gp._fisher_chunk(nth) == 1
    f2, G2, FB2 = gp.neg_log_likelihood_gradient_and_fisher_batch(thetas)
    assert np.array_equal(f2, fb) and np.array_equal(G2, G) and np.array_equal(FB2, FB)


def test_facade_fisher_scoring(H):
    name, d, n, m, _ = FACADE_CASE
    gp, y, x, theta, v = _facade(seed=5)
    lists = gp.neighbors()
    start, tol = np.array([3.0, 1.5, 1.5, 1.5]), 1e-8
    hps = gp.train_gradient(BOUNDS, init_hyperparameters=start, method="fisher", tolerance=tol, max_iter=100)
    hist = gp.fisher_history
    fs = [h[1] for h in hist]
    assert hps.shape == theta.shape and np.array_equal(gp.hyperparameters, hps) and _inside(hps) and all(_inside(h[0]) for h in hist)
    assert all(b <= a for a, b in zip(fs, fs[1:])), fs
    assert hist[-1][2] < tol and np.array_equal(hist[-1][0], hps) and fs[-1] == gp.neg_log_likelihood()
    assert gp.fisher_evaluations >= len(hist) and np.array_equal(gp.neighbors(), lists)
    ref, *_ = _facade(seed=5)
    ref.train_gradient(BOUNDS, init_hyperparameters=start, method="local", tolerance=1e-10, max_iter=200)
    f_local = ref.neg_log_likelihood()
    print(f"\nvecchia fisher scoring: {len(hist) - 1} iterations, {gp.fisher_evaluations} device calls, f {fs[0]:.6f} -> {fs[-1]:.9f}; "
          f"L-BFGS-B f {f_local:.9f}")
    assert fs[-1] <= f_local + 1e-6 * abs(f_local)
    # a component on its bound with the gradient pointing outward stays there
    tight = BOUNDS.copy()
    tight[0] = [0.01, 0.05]
    edge = np.array([0.05, 0.5, 0.5, 0.5])
    assert gp.neg_log_likelihood_and_gradient(edge)[1][0] < 0.0
    gp.train_gradient(tight, init_hyperparameters=edge, method="fisher", max_iter=3)
    assert all(h[0][0] == 0.05 for h in gp.fisher_history) and gp.fisher_history[-1][1] < gp.fisher_history[0][1]


def test_facade_train_is_opt_in(H):
    on, y, x, theta, v = _facade(seed=5, args={"likelihood_gradient": True})
    f = on.neg_log_likelihood()
    hps = on.train(BOUNDS, method="fisher", max_iter=20)
    assert np.array_equal(on.hyperparameters, hps) and _inside(hps) and on.neg_log_likelihood() <= f
    off, *_ = _facade(seed=5)
    with pytest.raises(NotImplementedError, match="likelihood_gradient.*train_gradient"):
        off.train(BOUNDS, method="fisher")
    with pytest.raises(ValueError, match="'fisher'"):
        off.train_gradient(BOUNDS, method="mcmc")


def test_facade_hyperparameter_laplace(H, monkeypatch):
    gp, y, x, theta, v = _facade(seed=5)
    gp.train_gradient(BOUNDS, method="fisher", max_iter=50)
    nth = len(theta)
    wide = np.array([[1e-6, 1e3]] * nth)
    lap = gp.hyperparameter_laplace(n_samples=64, seed=3, bounds=wide)
    assert np.array_equal(lap["fisher"], gp.fisher_information()) and np.array_equal(lap["mean"], gp.hyperparameters)
    assert np.max(np.abs(lap["covariance"] @ lap["fisher"] - np.eye(nth))) <= 1e-10
    assert np.allclose(lap["std_error"], np.sqrt(np.diag(np.linalg.inv(lap["fisher"]))), rtol=1e-9, atol=0.0)
    s = lap["samples"]
    assert s.shape == (64, nth) and np.all(s >= wide[:, 0]) and np.all(s <= wide[:, 1])
    assert np.isfinite(lap["log_evidence"]) and gp.hyperparameter_laplace()["samples"].shape == (0, nth)
    # a Fisher matrix that is not positive definite raises, as the dense method does
    broken = lap["fisher"].copy()
    broken[1, 1] = -broken[1, 1]
    monkeypatch.setattr(gp, "neg_log_likelihood_gradient_and_fisher", lambda hps=None: (1.0, np.zeros(nth), broken))
    with pytest.raises(ValueError, match="not positive definite"):
        gp.hyperparameter_laplace()
