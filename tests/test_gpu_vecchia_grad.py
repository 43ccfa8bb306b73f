"""The exact gradient of the nearest-neighbour likelihood on the device (include/fvgp_hip_nn.h: fvgp_hip_nn_loglik_grad;
fvgp_amd/gp_vecchia.py): the scores and the gradient against longdouble under bars that come from the float64 twin (vecchia_grad_ref:
MARGIN * max(base, FLOOR)); the bit contracts; the gradient against the dense GP's where the approximation is exact; failure reporting;
the argument rules; the facade and gradient training.  Run with -s for the record lines."""
import ctypes
import warnings

import numpy as np
import pytest

import vecchia_grad_ref as vg
import vecchia_ref as vr
from vecchia_device import CANARY, _device_grad, _device_value, _frame_untouched, _framed, _same

pytestmark = pytest.mark.gpu

LD = vr.LD


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


# ---- 1. accuracy against longdouble ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vg.GRAD_CASES, ids=vr.case_id)
def test_scores_and_gradient_against_longdouble(H, case):
    """Bars from the float64 twin, never from the device: both figures <= MARGIN * max(base, FLOOR) (vecchia_grad_ref)."""
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    out, grad, info, mu, var, score = _device_grad(H, name, x, thetas, idx, m, r, v)
    assert info == 0 and score.shape == (B, n, thetas.shape[1])
    bars = vg.bars(case)
    worst = dict.fromkeys(vg.FIGURES, 0.0)
    for b in range(B):
        f = vg.figures((score[b], grad[b]), vg.reference(case)[b])
        worst = {k: max(worst[k], f[k]) for k in vg.FIGURES}
    print(f"\nvecchia grad device {vr.case_id(case)}: " + " ".join(f"{k}={worst[k]:.2e}/{bars[k]:.2e}" for k in vg.FIGURES))
    # the value, the means and the variances are those of the value-only call, bit for bit
    out0, info0, mu0, var0 = _device_value(H, name, x, thetas, idx, m, r, v)
    assert info0 == 0 and _same(out, out0) and _same(mu, mu0) and _same(var, var0)
    for k in vg.FIGURES:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])


# ---- 2. bit contracts ------------------------------------------------------------------------------------------------------------------------
def test_bit_contracts(H):
    case = ("matern52_ard", 3, 200, 33, 3)
    name, d, n, m, B = case
    x, thetas, r, v, idx = vr.case_inputs(case)
    out, grad, info, mu, var, score = _device_grad(H, name, x, thetas, idx, m, r, v)
    again = _device_grad(H, name, x, thetas, idx, m, r, v)
    assert info == 0 and all(_same(a, b) for a, b in zip((out, grad, info, mu, var, score), again)), "the call twice"
    for b in range(B):
        o1, g1, _, m1, v1, s1 = _device_grad(H, name, x, thetas[b], idx, m, r, v)
        assert _same(o1[0], out[b]) and _same(g1[0], grad[b]) and _same(s1[0], score[b]) and _same(m1[0], mu[b]) and _same(v1[0], var[b]), b
    perm = np.array([2, 0, 1])
    o3, g3, _, m3, v3, s3 = _device_grad(H, name, x, thetas[perm], idx, m, r, v)
    assert _same(o3, out[perm]) and _same(g3, grad[perm]) and _same(s3, score[perm]) and _same(m3, mu[perm]) and _same(v3, var[perm])
    # a row alone: the call over the same rows with every other list emptied, and the row moved to another position of a shorter call
    # (the rows up to it and their lists: n changes, the row's inputs do not)
    for i in (0, 1, 33, 130, 199):
        alone = np.full_like(idx, -1)
        alone[i] = idx[i]
        s1 = _device_grad(H, name, x, thetas, alone, m, r, v)[5]
        assert _same(s1[:, i], score[:, i]), i
        s2 = _device_grad(H, name, x[:i + 1], thetas, idx[:i + 1], m, r[:i + 1], v[:i + 1])[5]
        assert _same(s2[:, i], score[:, i]), i


# ---- 3. exactness ------------------------------------------------------------------------------------------------------------------------------
def test_gradient_is_the_dense_one_when_every_earlier_point_is_a_neighbour(H):
    """n = 65, m = 64 on the given order: the product of conditionals is the exact likelihood, so its gradient is the dense GP's."""
    import fvgp_amd
    case = vr.EXACT_CASE
    name, d, n, m, _ = case
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    gp_v = fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, ordering="given")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=v, kernel_function=name)
    f, g = gp_v.neg_log_likelihood_and_gradient()
    exact, _ = vg.dense_grad_ld(name, x, theta, y - np.mean(y), v)
    scale = np.sum(np.abs(vg.reference(case)[0]), axis=0)          # sum_i |score_ih|: the scale of the `grad` figure
    bar = vg.bars(case)["grad"]
    dense = np.asarray(gp.neg_log_likelihood_gradient(theta), dtype=np.float64)
    err = float(np.max(np.abs(LD(1) * (-g) - exact) / scale))
    err_dense = float(np.max(np.abs(LD(1) * (-dense) - exact) / scale))
    err_pair = float(np.max(np.abs(g - dense) / np.asarray(scale, dtype=np.float64)))
    print(f"\nvecchia grad exactness n=65 m=64: vecchia vs longdouble {err:.2e}/{bar:.2e}, dense GP vs longdouble {err_dense:.2e}, "
          f"vecchia vs dense GP {err_pair:.2e}")
    assert f == gp_v.neg_log_likelihood()
    assert err <= bar
    assert err_dense <= 1e-9                      # (the dense GP's accuracy is other tests' business)
    assert err_pair <= bar + err_dense


# ---- 4. failure reporting ------------------------------------------------------------------------------------------------------------------------
def test_failure_is_reported_not_trapped(H):
    """The singular construction of test_gpu_vecchia.py: zero noise and a duplicated point among row 20's neighbours, sigma^2 a power of
    four, so that the second pivot is exactly 0.  A numerical condition that the kernel reports: NaN scores for that row at both thetas,
    the same info, a NaN gradient; every other row is what it is in a call without the singular list.  Nothing faults."""
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
    out, grad, info, mu, var, score = _device_grad(H, name, x, thetas, idx, m, r, v0)
    bad = np.isnan(score).any(axis=2)
    assert np.all(np.isnan(score[:, 20])) and bad[0, 20] and bad[1, 20] and bad.sum() == 2
    assert info == 1 + 0 * n + 20 and np.all(np.isnan(grad)) and np.all(np.isnan(out[:, 0]))
    out0, info0, mu0, var0 = _device_value(H, name, x, thetas, idx, m, r, v0)
    assert info0 == info and _same(out, out0) and _same(mu, mu0) and _same(var, var0)
    idx2 = idx.copy()
    idx2[20, :3] = [3, 5, -1]
    out2, grad2, info2, mu2, var2, score2 = _device_grad(H, name, x, thetas, idx2, m, r, v0)
    keep = np.arange(n) != 20
    assert info2 == 0 and np.all(np.isfinite(grad2)) and np.all(np.isfinite(score2))
    assert _same(score2[:, keep], score[:, keep]) and _same(mu2[:, keep], mu[:, keep]) and _same(var2[:, keep], var[:, keep])


# ---- 5. argument rules ------------------------------------------------------------------------------------------------------------------------
def test_argument_rules(H):
    """a bad argument returns minus its position before anything is launched: outputs, workspace and host results stay as they were"""
    from fvgp_amd import _lib
    L = _lib.lib()
    n, m, B, nth = 10, 4, 2, 4
    t = H.torch
    x = H.to_device(np.random.default_rng(1).random((n, 3)))
    rr = np.linspace(-1.0, 1.0, n)
    r, v = H.to_device(rr), H.to_device(np.ones(n))
    idx = t.full((n, m), -1, dtype=t.int32, device=x.device)
    mbig, mu = _framed(H, B, n)
    vbig, var = _framed(H, B, n)
    sbig, score = _framed(H, B, n, nth)
    wb = _lib.nn_grad_workspace_bytes(n, B, nth)
    work = t.full((wb // 8,), CANARY, dtype=t.float64, device=x.device)
    th = np.array([[1.0, 1.0, 1.0, 1.0], [3.0, 0.5, 2.0, 1.0]])
    out, grad = np.full((B, 3), CANARY), np.full((B, nth), CANARY)
    info = ctypes.c_int64(-5)
    P = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    tp = th.ctypes.data_as(_lib.P_d)

    def call(**kw):
        a = dict(h=H._h, kid=1, x=P(x), n=n, d=3, th=tp, nt=nth, B=B, idx=P(idx), ld=m, m=m, r=P(r), v=P(v), mu=P(mu), var=P(var),
                 score=P(score), w=P(work), wb=wb, out=out.ctypes.data_as(_lib.P_d), grad=grad.ctypes.data_as(_lib.P_d),
                 info=ctypes.byref(info))
        a.update(kw)
        return L.fvgp_hip_nn_loglik_grad(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=-1)), (-2, dict(kid=6)), (-3, dict(x=None)), (-4, dict(n=0)), (-4, dict(n=2 ** 31)),
                     (-5, dict(d=0)), (-5, dict(d=17)), (-6, dict(th=None)), (-7, dict(nt=3)), (-8, dict(B=0)), (-8, dict(B=65536)),
                     (-9, dict(idx=None)), (-10, dict(ld=3)), (-11, dict(m=0)), (-11, dict(m=65)), (-12, dict(r=None)), (-13, dict(v=None)),
                     (-14, dict(mu=None)), (-15, dict(var=None)), (-16, dict(score=None)), (-17, dict(w=None)),
                     (-17, dict(w=ctypes.c_void_p(work.data_ptr() + 4))), (-18, dict(wb=_lib.nn_workspace_bytes(_lib.NN_LOGLIK, n, B))),
                     (-19, dict(out=None)), (-20, dict(grad=None)), (-21, dict(info=None))):
        assert call(**kw) == code, (code, kw)
    H.sync()
    assert info.value == -5 and np.all(out == CANARY) and np.all(grad == CANARY) and np.all(work.cpu().numpy() == CANARY)
    assert all(np.all(b.cpu().numpy() == CANARY) for b in (mbig, vbig, sbig))
    # and the good call: rows without neighbours have the sigma^2 term of d = sigma^2 + v alone,
    # d/d sigma^2 of -1/2 [r^2 / (sigma^2 + v) + log(sigma^2 + v)], and 0 for the length scales
    assert call() == 0 and info.value == 0
    s = score.cpu().numpy()
    for b in range(B):
        dv = LD(th[b, 0]) + LD(1)
        want = (np.asarray(rr, dtype=LD) ** 2 / dv ** 2 - 1 / dv) / 2
        assert np.max(np.abs(s[b, :, 0] - want)) <= 4 * vr.EPS * float(np.max(np.abs(want))) and np.all(s[b, :, 1:] == 0.0)
        assert abs(grad[b, 0] - float(np.sum(want))) <= 16 * vr.EPS * float(np.sum(np.abs(want))) and np.all(grad[b, 1:] == 0.0)
    assert _frame_untouched(mbig) and _frame_untouched(vbig) and _frame_untouched(sbig)


# ---- 6. the facade ------------------------------------------------------------------------------------------------------------------------------
FACADE_CASE = ("matern32_ard", 3, 200, 17, 1)


def _facade(case, **kw):
    import fvgp_amd
    name, d, n, m, _ = case
    x, theta, r, v = vr.case_data(name, d, n)
    y = r + 0.7
    return fvgp_amd.VecchiaGP(x, y, theta, noise_variances=v, kernel_function=name, n_neighbors=m, **kw), y, x, theta, v


def test_facade_value_gradient_scores_and_batches(H):
    case = FACADE_CASE
    name, d, n, m, _ = case
    gp, y, x, theta, v = _facade(case, seed=5)
    perm = gp.ordering
    r = y - np.mean(y)
    xo, ro, vo = x[perm], r[perm], v[perm]
    idx = vr.search_ref(xo, xo, m, vr.length_scales(name, theta, d), c0=0)
    ref = vg.scores_ref(name, xo, theta, idx, ro, vo, LD)
    tol = vr.MARGIN * 1e-12                       # (the accuracy proper is section 1's: here the plumbing)
    scale = np.asarray(np.sum(np.abs(ref), axis=0), dtype=np.float64)
    f, g = gp.neg_log_likelihood_and_gradient()
    assert f == gp.neg_log_likelihood() and g.shape == theta.shape
    assert np.all(np.abs(g + np.asarray(np.sum(ref, axis=0), dtype=np.float64)) <= tol * scale)
    s = gp.conditional_scores()
    want = np.empty((n, len(theta)))
    want[perm] = np.asarray(ref, dtype=np.float64)
    assert s.shape == (n, len(theta)) and np.all(np.abs(s - want) <= tol * np.max(np.abs(want), axis=0))
    assert np.all(np.abs(np.sum(s, axis=0) + g) <= 1e-12 * scale)
    # batch rows are the single calls bit for bit, whatever the chunking, and the state is untouched
    thetas = vr.batch_thetas(theta, 3)
    fb, G = gp.neg_log_likelihood_and_gradient_batch(thetas)
    assert fb.shape == (3,) and G.shape == thetas.shape and np.array_equal(gp.neg_log_likelihood_gradient_batch(thetas), G)
    for b in range(3):
        f1, g1 = gp.neg_log_likelihood_and_gradient(thetas[b])
        assert f1 == fb[b] and np.array_equal(g1, G[b]), b
    assert fb[0] == f and np.array_equal(G[0], g) and np.array_equal(gp.hyperparameters, theta)
    gp.args["grad_batch_bytes"] = 8 * n * (2 + len(theta))          # one hyperparameter vector per call
    assert gp._grad_chunk(len(theta)) == 1
    f2, G2 = gp.neg_log_likelihood_and_gradient_batch(thetas)
    assert np.array_equal(f2, fb) and np.array_equal(G2, G)


def test_facade_gradient_training(H):
    case = FACADE_CASE
    name, d, n, m, _ = case
    gp, y, x, theta, v = _facade(case, seed=5)
    lists = gp.neighbors()
    bounds = np.array([[0.1, 10.0]] + [[0.05, 5.0]] * d)
    inside = lambda t: np.all(np.asarray(t) >= bounds[:, 0]) and np.all(np.asarray(t) <= bounds[:, 1])      # noqa: E731
    start = gp.neg_log_likelihood()
    hps = gp.train_gradient(bounds, method="local", max_iter=15)
    assert hps.shape == theta.shape and np.array_equal(gp.hyperparameters, hps) and inside(hps)
    assert gp.neg_log_likelihood() <= start and np.array_equal(gp.neighbors(), lists)
    hps = gp.train_gradient(bounds, init_hyperparameters=theta, method="adam", max_iter=15, lr=0.05)
    assert np.array_equal(gp.hyperparameters, hps) and inside(hps) and gp.neg_log_likelihood() <= start
    assert 1 <= len(gp.adam_history["theta"]) <= 15 and all(inside(t) for t in gp.adam_history["theta"])
    assert np.array_equal(gp.neighbors(), lists)
    with pytest.raises(ValueError, match="'local' or 'adam'"):
        gp.train_gradient(bounds, method="mcmc")
    # a start on the boundary with a step that overshoots: the projection keeps every iterate inside
    edge = np.array([0.1, 0.05, 5.0, 0.05])
    gp.train_gradient(bounds, init_hyperparameters=edge, method="adam", max_iter=5, lr=1.0)
    assert all(inside(t) for t in gp.adam_history["theta"]) and inside(gp.hyperparameters)
    # multi-start
    multi, *_ = _facade(case, seed=5, args={"adam_starts": 3})
    hps = multi.train_gradient(bounds, init_hyperparameters=theta, method="adam", max_iter=15, lr=0.05, seed=1)
    mi = multi.adam_multistart_info
    assert mi["x0"].shape == (3, d + 1) and np.array_equal(mi["x0"][0], theta) and mi["x"].shape == (3, d + 1) and mi["f(x)"].shape == (3,)
    assert mi["best"] == int(np.argmin(mi["f(x)"])) and np.array_equal(hps, mi["x"][mi["best"]]) and all(inside(t) for t in mi["x"])
    assert all(inside(t) for t in multi.adam_history["theta"])
    assert multi.neg_log_likelihood() == mi["f(x)"][mi["best"]] <= start and np.array_equal(multi.neighbors(), lists)


def test_facade_fvgp_names_are_opt_in(H):
    case = FACADE_CASE
    name, d, n, m, _ = case
    bounds = np.array([[0.1, 10.0]] + [[0.05, 5.0]] * d)
    on, y, x, theta, v = _facade(case, seed=5, args={"likelihood_gradient": True})
    f, g = on.neg_log_likelihood_and_gradient()
    assert np.array_equal(on.neg_log_likelihood_gradient(), g) and np.array_equal(on.neg_log_likelihood_gradient(theta * 1.1),
                                                                                  on.neg_log_likelihood_and_gradient(theta * 1.1)[1])
    for method in ("local", "adam"):
        on.set_hyperparameters(theta)
        hps = on.train(bounds, method=method, max_iter=15)
        assert np.array_equal(on.hyperparameters, hps) and on.neg_log_likelihood() <= f
    for method in ("hgdl", "bo"):
        with pytest.raises(NotImplementedError, match="not built yet"):
            on.train(bounds, method=method)
    # without the flag the refusals of test_gpu_vecchia.py stand, and name the new route
    off, *_ = _facade(case, seed=5)
    for method in ("local", "adam", "hgdl"):
        with pytest.raises(NotImplementedError, match="gradient of the nearest-neighbour likelihood is not built yet"):
            off.train(bounds, method=method)
    with pytest.raises(NotImplementedError, match="not built yet.*likelihood_gradient"):
        off.neg_log_likelihood_gradient()
    with pytest.raises(NotImplementedError, match="train_gradient"):
        off.train(bounds, method="local")
