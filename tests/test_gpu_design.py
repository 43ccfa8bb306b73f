"""Greedy batch selection on the device (fvgp_hip_select_batch, Handle.select_batch, GP.select_batch): the C ABI against the numpy
twin of tests/design_ref.py on every shape at which the kernels take another path, bitwise independence of a candidate from the rest of
the call, exhaustion decided on the device, refused arguments, and the facade against exact conditioning with no reference in the loop."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import design_ref as dr

pytestmark = pytest.mark.gpu

CANARY = -7.25e300
ICANARY = -7777
# every posterior variance is held to 1e-10 sigma^2.  The twin sits at 1e-15 sigma^2 from exact conditioning
# (tests/test_design_host.py); the device differs from it by the order of sums over at most 513 terms and the 4-ulp kernel values.
BAR = 1e-10 * dr.SIGMA2


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _factor(H, kernel, x, theta, V):
    """the factor of K + diag(V) on the device, as the fused evaluation leaves it"""
    from fvgp_amd import _lib
    n = len(x)
    dim = _lib.loglik_dim(n, 1)
    xd = H.to_device(x)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), 1)
    y = np.sin(3.0 * x.sum(axis=1))[:, None]
    info = H.loglik(_lib.KERNEL_IDS[kernel], xd, theta, H.to_device(V), H.to_device(y - y.mean()), KV, alpha)[3]
    assert info == 0
    return xd, KV, alpha


def _initial_variances(H, kernel, xd, theta, KV, alpha, xcd):
    from fvgp_amd import _lib
    P = xcd.shape[0]
    var = H.empty(P)
    kx = H.empty(KV.shape[0], _lib.pad128(P))
    H.posterior(_lib.KERNEL_IDS[kernel], xd, theta, KV, alpha, 1, xcd, kx, var_out=var)
    return var


def _framed(H, shape, dtype=None):
    """a canary-filled buffer with a frame of 8 around the view the call gets: (buffer, view)"""
    t = H.torch
    if len(shape) == 1:
        big = t.full((shape[0] + 16,), ICANARY if dtype is not None else CANARY, dtype=dtype or t.float64, device=f"cuda:{H.device}")
        return big, big[8:8 + shape[0]]
    big = t.full((shape[0] + 2, shape[1] + 3), CANARY, dtype=t.float64, device=f"cuda:{H.device}")     # an odd leading dimension
    return big, big[1:1 + shape[0], :shape[1]]


def _frame_untouched(big, view_shape):
    a = big.cpu().numpy()
    if a.ndim == 1:
        fill = ICANARY if a.dtype == np.int64 else CANARY
        return np.all(a[:8] == fill) and np.all(a[8 + view_shape[0]:] == fill)
    return np.all(a[0] == CANARY) and np.all(a[1 + view_shape[0]:] == CANARY) and np.all(a[:, view_shape[1]:] == CANARY)


def _run(H, kernel, xd, theta, KV, xcd, var0, q, noise=None, criterion=0, allow_repeats=False, tol=1e-12):
    """one Handle.select_batch call with every output framed by canaries; the outputs on the host"""
    from fvgp_amd import _lib
    P = xcd.shape[0]
    vbig, var = _framed(H, (P,))
    var.copy_(var0)
    ibig, idx = _framed(H, (q,), dtype=H.torch.int64)
    pbig, pick = _framed(H, (q,))
    gbig, G = _framed(H, (q, P))
    nd = None if noise is None else H.to_device(noise)
    H.select_batch(_lib.KERNEL_IDS[kernel], xd, theta, KV, xcd, var, q, idx, pick, noise=nd, criterion=criterion,
                   allow_repeats=allow_repeats, tol=tol, G_out=G)
    H.sync()
    assert _frame_untouched(vbig, (P,)) and _frame_untouched(ibig, (q,)) and _frame_untouched(pbig, (q,)) and _frame_untouched(gbig, (q, P))
    return {"indices": idx.cpu().numpy(), "pick_var": pick.cpu().numpy(), "var": var.cpu().numpy(), "G": G.cpu().numpy()}


# ---- 1. the ABI against the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", dr.ABI_FIXTURES, ids=dr.fixture_id)
def test_abi_matches_the_twin(H, fx):
    """indices equal (the fixtures lead by >= 1e-8 sigma^2 at every step: tests/test_design_host.py); pick_var_out, the final var and
    G_out within 1e-10 sigma^2; nothing outside the output buffers changes."""
    from fvgp_amd import _lib
    (x, V, theta, xc, noise), ref = dr.run_fixture(fx)
    n, P, q = fx["n"], fx["P"], fx["q"]
    assert _lib.select_workspace_bytes(n, P, q) >= (q * P + -(-n // 256) * min(P, 65536) + _lib.pad128(n)) * 8
    xd, KV, alpha = _factor(H, fx["kernel"], x, theta, V)
    xcd = H.to_device(xc)
    var0 = _initial_variances(H, fx["kernel"], xd, theta, KV, alpha, xcd)
    got = _run(H, fx["kernel"], xd, theta, KV, xcd, var0, q, noise=noise, criterion=1 if fx["mode"] == "info" else 0)
    dev = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in ("pick_var", "var", "G")}
    dev["var0"] = float(np.max(np.abs(np.maximum(var0.cpu().numpy(), 0.0) - ref["var0"])))
    print(f"DESIGN|select_abi_vs_twin|{dr.fixture_id(fx)}|" + "|".join(f"{k}_dev_over_sigma2={v / dr.SIGMA2:.3e}" for k, v in dev.items()))
    assert np.array_equal(got["indices"], ref["indices"]), (got["indices"], ref["indices"])
    assert dev["pick_var"] <= BAR and dev["var"] <= BAR and dev["G"] <= BAR, dev


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bits_case():
    return dr.run_fixture(dr.BITS_FIXTURE)


def test_bits_do_not_depend_on_the_rest_of_the_call(H):
    """The same call twice; q = 5 as the prefix of q = 12; select_block = 128 (three blocks of the 300 candidates) against the default;
    a sub-list of the candidates that holds every pick (with the full call's initial variances, which are the caller's): all bitwise."""
    fx = dr.BITS_FIXTURE
    (x, V, theta, xc, noise), ref = _bits_case()
    xd, KV, alpha = _factor(H, fx["kernel"], x, theta, V)
    xcd = H.to_device(xc)
    var0 = _initial_variances(H, fx["kernel"], xd, theta, KV, alpha, xcd)
    full = _run(H, fx["kernel"], xd, theta, KV, xcd, var0, 12, noise=noise)
    assert np.array_equal(full["indices"], ref["indices"])
    again = _run(H, fx["kernel"], xd, theta, KV, xcd, var0, 12, noise=noise)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    pre = _run(H, fx["kernel"], xd, theta, KV, xcd, var0, 5, noise=noise)
    for k in ("indices", "pick_var", "G"):
        assert pre[k].tobytes() == full[k][:5].tobytes(), k
    H.set_option("select_block", 128)
    try:
        cut = _run(H, fx["kernel"], xd, theta, KV, xcd, var0, 12, noise=noise)
    finally:
        H.set_option("select_block", 65536)
    for k in full:
        assert full[k].tobytes() == cut[k].tobytes(), k
    picks = full["indices"]
    rest = np.setdiff1d(np.arange(300), picks)[::3]
    sub = np.sort(np.concatenate([picks, rest]))                      # 12 picks + 96 others, in their order
    s = _run(H, fx["kernel"], xd, theta, KV, H.to_device(xc[sub]), var0[H.torch.as_tensor(sub, device=var0.device)], 12, noise=noise[sub])
    assert np.array_equal(sub[s["indices"]], picks)
    assert s["pick_var"].tobytes() == full["pick_var"].tobytes()
    assert s["G"].tobytes() == np.ascontiguousarray(full["G"][:, sub]).tobytes()
    assert s["var"].tobytes() == full["var"][sub].tobytes()


# ---- 3. exhaustion on the device ------------------------------------------------------------------------------------------------------
def test_exhaustion_is_decided_on_the_device(H):
    """Every candidate twice, no noise: a pick takes its duplicate's variance with it, so at most P / 2 picks are made, -1 fills idx_out
    from the first exhausted step on, and var is what the call with exactly that many steps leaves.  tol = 1e-9: what is left of a
    conditioned-out duplicate is the rounding of sigma^2 - k^T KV^-1 k, about eps cond(KV) sigma^2 ~ 1e-12 sigma^2 at worst."""
    rng = np.random.default_rng(5)
    n, d = 60, 2
    x, V = rng.random((n, d)), rng.uniform(0.01, 0.02, n)
    theta = np.array([dr.SIGMA2, 0.4, 0.5])
    xc = rng.random((10, d))
    xc2 = np.vstack([xc, xc])
    xd, KV, alpha = _factor(H, "matern52_ard", x, theta, V)
    xcd = H.to_device(xc2)
    var0 = _initial_variances(H, "matern52_ard", xd, theta, KV, alpha, xcd)
    for repeats in (False, True):
        got = _run(H, "matern52_ard", xd, theta, KV, xcd, var0, 20, allow_repeats=repeats, tol=1e-9)
        idx = got["indices"]
        m = int(np.argmax(idx < 0))
        assert idx[0] >= 0 and 1 <= m <= 10 and np.all(idx[m:] == -1) and np.all(idx[:m] >= 0)
        assert len(set((idx[:m] % 10).tolist())) == m
        assert np.all(got["pick_var"][m:] == 0.0)
        assert np.all(got["G"][m:] == CANARY)                          # rows from the first exhausted step on are not written
        short = _run(H, "matern52_ard", xd, theta, KV, xcd, var0, m, allow_repeats=repeats, tol=1e-9)
        assert short["var"].tobytes() == got["var"].tobytes()
        assert short["indices"].tobytes() == idx[:m].tobytes()
        assert np.max(got["var"]) <= 1e-9 * float(np.max(var0.cpu().numpy())) + 1e-12


# ---- 4. bad arguments -------------------------------------------------------------------------------------------------------------------
def test_select_refuses_bad_arguments_and_touches_nothing(H):
    from fvgp_amd import _lib
    L = _lib.lib()
    t = H.torch
    n, d, P, q = 40, 2, 20, 4
    rng = np.random.default_rng(1)
    xd, xcd = H.to_device(rng.random((n, d))), H.to_device(rng.random((P, d)))
    fac = H.zeros(128, 128)
    noise = H.to_device(np.full(P, 0.05))
    var = t.full((P,), CANARY, dtype=t.float64, device=xd.device)
    idx = t.full((q,), ICANARY, dtype=t.int64, device=xd.device)
    pick = t.full((q,), CANARY, dtype=t.float64, device=xd.device)
    G = t.full((q, P), CANARY, dtype=t.float64, device=xd.device)
    nbytes = _lib.select_workspace_bytes(n, P, q)
    work = t.full((nbytes // 8 + 2,), CANARY, dtype=t.float64, device=xd.device)
    theta = (ctypes.c_double * 3)(1.2, 0.3, 0.4)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    good = dict(h=H._h, kid=0, x=ptr(xd), n=n, d=d, theta=theta, ntheta=3, L=ptr(fac), ldl=128, xc=ptr(xcd), P=P, noise=ptr(noise), var=ptr(var),
                q=q, crit=0, rep=0, tol=1e-12, work=ptr(work), wb=nbytes, idx=ptr(idx), pick=ptr(pick), G=ptr(G), ldg=P)
    cases = [("h", None, -1), ("kid", 6, -2), ("kid", -1, -2), ("x", None, -3), ("n", 0, -4), ("d", 0, -5), ("d", 17, -5), ("theta", None, -6),
             ("ntheta", 2, -7), ("L", None, -8), ("L", ctypes.c_void_p(fac.data_ptr() + 8), -8), ("ldl", 127, -9), ("ldl", 64, -9),
             ("xc", None, -10), ("P", 0, -11), ("var", None, -13), ("q", 0, -14), ("crit", 2, -15), ("tol", -1.0, -17),
             ("tol", float("nan"), -17), ("work", None, -18), ("work", ctypes.c_void_p(work.data_ptr() + 8), -18), ("wb", nbytes - 8, -19),
             ("idx", None, -20), ("pick", None, -21), ("ldg", P - 1, -23)]
    for key, val, want in cases + [("crit1_without_noise", None, -12)]:
        a = dict(good)
        if key == "crit1_without_noise":
            a["crit"], a["noise"] = 1, None
        else:
            a[key] = val
        rc = L.fvgp_hip_select_batch(a["h"], a["kid"], a["x"], a["n"], a["d"], a["theta"], a["ntheta"], a["L"], a["ldl"], a["xc"], a["P"],
                                     a["noise"], a["var"], a["q"], a["crit"], a["rep"], a["tol"], a["work"], a["wb"], a["idx"], a["pick"],
                                     a["G"], a["ldg"])
        assert rc == want, (key, val, rc, want)
    H.sync()
    for buf in (var, pick, G, work):
        assert np.all(buf.cpu().numpy() == CANARY)
    assert np.all(idx.cpu().numpy() == ICANARY)
    assert _lib.select_workspace_bytes(0, 5, 2) == -1 and _lib.select_workspace_bytes(5, 0, 2) == -1 and _lib.select_workspace_bytes(5, 5, 0) == -1
    with pytest.raises(_lib.HipExtensionError):
        H.set_option("select_block", 100)


# ---- 5. the facade: conditioning identity with no reference in the loop ------------------------------------------------------------------
def _gp(fx_inputs, kernel, **kw):
    import fvgp_amd
    x, V, theta, xc, noise = fx_inputs
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * np.random.default_rng(2).standard_normal(len(x))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=None if "noise_function" in kw else V.copy(),
                           kernel_function=kernel, **kw)


def test_facade_conditioning_identity():
    """select_batch, then update_gp_data with the picked points and noise_selected: the model's own posterior variance at the candidates
    is "v_after" to 1e-10 sigma^2 and half the growth of logdet_KV(), less 1/2 sum log noise, is the last "information_gain" to 1e-9
    relative; before the append the state and the cached results are bitwise what they were."""
    fx = dr.FACADE_FIXTURE
    inputs, ref = dr.run_fixture(fx)
    x, V, theta, xc, noise = inputs
    gp = _gp(inputs, fx["kernel"])
    xfix = np.random.default_rng(9).random((7, fx["d"]))
    before = (gp.log_likelihood(), gp.posterior_mean(xfix)["m(x)"], gp.posterior_covariance(xfix)["S"], gp.logdet_KV)
    r = gp.select_batch(xc, fx["q"], noise_variances=noise)
    after = (gp.log_likelihood(), gp.posterior_mean(xfix)["m(x)"], gp.posterior_covariance(xfix)["S"], gp.logdet_KV)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.array_equal(r["indices"], ref["indices"]) and not r["exhausted"]
    assert r["x"].tobytes() == xc[r["indices"]].tobytes() and r["x_pred"].tobytes() == xc.tobytes()
    assert r["noise_selected"].tobytes() == noise[r["indices"]].tobytes()
    assert r["v_before"].shape == r["v_after"].shape == (fx["P"],) and r["v_selected"].shape == r["information_gain"].shape == (fx["q"],)
    assert np.max(np.abs(r["v_before"] - ref["var0"])) <= BAR and np.all(np.diff(r["information_gain"]) > 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.update_gp_data(r["x"], np.zeros(len(r["x"])), noise_variances_new=r["noise_selected"])
    v = gp.posterior_covariance(xc, variance_only=True)["v(x)"]
    dev = float(np.max(np.abs(v - r["v_after"])))
    want = 0.5 * (gp.logdet_KV - before[3]) - 0.5 * np.sum(np.log(r["noise_selected"]))
    rel = abs(r["information_gain"][-1] - want) / abs(want)
    print(f"DESIGN|select_facade_conditioning|v_after_dev_over_sigma2={dev / dr.SIGMA2:.3e}|information_gain_rel={rel:.3e}")
    assert dev <= BAR
    assert rel <= 1e-9


# ---- 6. the facade in chunks, on an fvGP, its noise arguments and its refusals -----------------------------------------------------------
def test_facade_chunks_noise_arguments_and_fvgp():
    import fvgp_amd
    fx = dr.FACADE_FIXTURE
    inputs, ref = dr.run_fixture(fx)
    x, V, theta, xc, noise = inputs
    one = _gp(inputs, fx["kernel"]).select_batch(xc, fx["q"], noise_variances=noise)
    cut = _gp(inputs, fx["kernel"], args={"posterior_chunk": 128}).select_batch(xc, fx["q"], noise_variances=noise)   # 128 + 128 + 44 candidates
    assert np.array_equal(one["indices"], cut["indices"]) and np.array_equal(one["indices"], ref["indices"])
    assert np.max(np.abs(one["v_after"] - cut["v_after"])) <= BAR and np.max(np.abs(one["v_after"] - ref["var"])) <= BAR
    # a scalar, and the default (the model's noise at the candidates: the mean of the data's), against exact conditioning on the picks
    gp = _gp(inputs, fx["kernel"])
    for arg, value in ((0.03, 0.03), (None, float(np.mean(V)))):
        r = gp.select_batch(xc, 6, noise_variances=arg, criterion="information")
        assert np.all(r["noise_selected"] == value) and len(set(r["indices"].tolist())) == 6
        v_bf, _ = dr.brute_force_after(fx["kernel"], x, theta, V, xc, r["indices"], np.full(len(xc), value))
        assert np.max(np.abs(r["v_after"] - v_bf)) <= BAR
        assert np.isclose(r["information_gain"][-1], 0.5 * np.sum(np.log1p(r["v_selected"] / value)), rtol=1e-14)
    r0 = gp.select_batch(xc, 3, noise_variances=0.0)
    assert r0["information_gain"] is None and np.all(r0["v_after"][r0["indices"]] <= BAR)
    with pytest.raises(ValueError, match="information"):
        gp.select_batch(xc, 3, noise_variances=0.0, criterion="information")
    # repeats on the device: with noise a point recurs
    rr = gp.select_batch(xc[:40], 30, noise_variances=0.05, allow_repeats=True)
    assert len(rr["indices"]) == 30 and len(set(rr["indices"].tolist())) < 30
    # exhaustion through the facade: the warning names tol
    with pytest.warns(UserWarning, match="tol"):
        re = gp.select_batch(np.vstack([xc[:5], xc[:5]]), 10, noise_variances=0.0, tol=1e-9)
    assert re["exhausted"] and len(re["indices"]) <= 5
    # an fvGP with two tasks: the candidates are the product set
    (xd, y, nv, th, xq, x_out, nz), xprod, fref = dr.fvgp_case()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = fvgp_amd.fvGP(xd, y, init_hyperparameters=th, noise_variances=nv, kernel_function="matern32_ard")
    rm = gm.select_batch(xq, 8, x_out=x_out, noise_variances=nz)
    assert rm["x_pred"].shape == (80, 3) and np.array_equal(rm["x_pred"], xprod)
    assert np.array_equal(rm["indices"], fref["indices"]) and np.max(np.abs(rm["v_after"] - fref["var"])) <= BAR
    assert np.array_equal(gm.select_batch(xq, 8, noise_variances=nz)["indices"], rm["indices"])      # x_out defaults to every task
    # what has no factor on this device, or no kernel on it, raises and names the mode and the host route
    small = (x[:50], V[:50], theta, xc, noise)
    from scipy.linalg import cho_factor, cho_solve
    import oracle.fvgp_oracle as orc
    gh = _gp(small, lambda a, b, h: orc.rbf_ard(a, b, h))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gc = _gp(small, fx["kernel"], linalg_mode=[lambda KV: cho_factor(KV, lower=True), lambda o, b: cho_solve(o, b),
                                                   lambda o: 2.0 * np.sum(np.log(np.diag(o[0])))])
    with pytest.raises(NotImplementedError, match="kernel callable.*posterior_covariance"):
        gh.select_batch(xc, 3)
    with pytest.raises(NotImplementedError, match="linalg_mode.*posterior_covariance"):
        gc.select_batch(xc, 3)
    gp._sharded = True
    try:
        with pytest.raises(NotImplementedError, match="row-sharded.*posterior_covariance"):
            gp.select_batch(xc, 3)
    finally:
        gp._sharded = False
    gv = _gp(small, fx["kernel"], noise_function=lambda xx, hps: np.diag(np.full(len(xx), 0.01)))
    with pytest.raises(NotImplementedError, match="matrix-valued"):
        gv.select_batch(xc, 3)
