"""BASELINE.json configs at their full sizes, checked through size-independent properties (no oracle can
follow there): residual of the solve, L L^T against re-assembled entries, gradient against a directional
finite difference of the likelihood, PSD / symmetry of the posterior covariance."""
import warnings

import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu


def _entries_of_LLt(gp, pairs):
    """(L L^T)[i,j] for a few index pairs from the device factor."""
    import torch
    L = gp._L
    out = []
    for i, j in pairs:
        m = min(i, j) + 1
        out.append(float((L[i, :m] * L[j, :m]).sum().item()))
    return np.array(out)


def test_config2_n20000_rbf_posterior():
    """C2: N=20k d=3 RBF, dense K assembly + Cholesky + posterior at P=1000 on one MI355X."""
    import fvgp_amd
    import torch
    n = 20000
    x, y = synth(n, 3)
    nv = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function="rbf_ard")
    H = gp._H
    # residual of KV alpha = y - m with K re-assembled in full
    K = H.empty(n, n)
    H.kmat(0, gp._x_dev, gp._x_dev, theta, K)
    H.sync()
    alpha = gp._alpha[:n, 0]
    ym = H.to_device(y - np.mean(y))
    res = K @ alpha + H.to_device(nv) * alpha - ym
    assert float(res.norm() / ym.norm()) < 1e-9
    # L L^T against assembled entries
    rng = np.random.default_rng(1)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, (64, 2))] + [(n - 1, n - 1), (0, 0), (n - 1, 0)]
    got = _entries_of_LLt(gp, pairs)
    want = np.array([float(K[i, j].item()) + (nv[i] if i == j else 0.0) for i, j in pairs])
    assert np.max(np.abs(got - want)) < 1e-11
    # log-likelihood pieces are consistent: quad = ym . alpha
    quad = float((ym * alpha).sum().item())
    ll = -0.5 * (quad + gp.logdet_KV + n * np.log(2 * np.pi))
    np.testing.assert_allclose(gp.log_likelihood(), ll, rtol=1e-12)
    del K
    torch.cuda.empty_cache()
    # posterior at P = 1000
    xp = np.random.default_rng(2).random((1000, 3))
    pm = gp.posterior_mean(xp)["m(x)"]
    pc = gp.posterior_covariance(xp)
    S, v = pc["S"], pc["v(x)"]
    assert pm.shape == (1000,) and S.shape == (1000, 1000)
    assert np.max(np.abs(S - S.T)) < 1e-10
    assert np.min(np.linalg.eigvalsh(S)) > -1e-9
    assert np.all(v >= 0) and np.all(v <= theta[0] + 1e-12)
    truth = np.sin(3.0 * xp.sum(axis=1))
    assert np.sqrt(np.mean((pm - truth) ** 2)) < 0.05          # it actually regresses the synthetic function
    # mean = k^T alpha recomputed by hand for a few points
    kx = H.empty(n, 16)
    H.kmat(0, gp._x_dev, H.to_device(xp[:16]), theta, kx)
    H.sync()
    np.testing.assert_allclose(pm[:16], (kx.T @ alpha).cpu().numpy() + np.mean(y), rtol=1e-9, atol=1e-11)


def test_config2_n20000_against_the_oracle():
    """C2 at its FULL size against the oracle itself (the box's host runs N=20k in seconds): log-likelihood, log-det, KVinvY,
    posterior mean and covariance -- the same tolerances as the golden-vector tests."""
    import fvgp_amd
    from oracle import fvgp_oracle as orc
    n = 20000
    x, y = synth(n, 3)
    nv = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function="rbf_ard")
    ref = orc.OracleGP(x, y, theta, nv, kernel="rbf_ard")
    np.testing.assert_allclose(gp.log_likelihood(), ref.log_likelihood(), rtol=1e-10)
    np.testing.assert_allclose(gp.logdet_KV, ref.logdet_KV, rtol=1e-10)
    assert np.max(np.abs(gp.KVinvY - ref.KVinvY)) <= 1e-8 * np.max(np.abs(ref.KVinvY))
    np.testing.assert_allclose(gp._L.diagonal()[:n:97].cpu().numpy(), np.diag(ref.Chol_factor)[::97], rtol=1e-10)
    xp = np.random.default_rng(2).random((200, 3))
    np.testing.assert_allclose(gp.posterior_mean(xp)["m(x)"], ref.posterior_mean(xp)["m(x)"], rtol=1e-8, atol=1e-10)
    pc, rc = gp.posterior_covariance(xp), ref.posterior_covariance(xp)
    assert np.max(np.abs(pc["S"] - rc["S"])) <= 1e-10 * theta[0]
    assert np.max(np.abs(pc["v(x)"] - rc["v(x)"])) <= 1e-10 * theta[0]
    t2 = theta * np.array([1.3, 0.8, 1.1, 0.9])
    np.testing.assert_allclose(gp.log_likelihood(t2), ref.log_likelihood(t2), rtol=1e-10)


def test_headline_n50000_rbf():
    """The metric's own workload (BASELINE.json: N=50k d=3 RBF, bench.py's synthetic data and theta): residual of
    KV alpha = y - m with K re-assembled in full, entries of L L^T against assembled entries, the log-likelihood's pieces, and
    a second evaluation at another theta that must leave the state alone (gp_marginal_likelihood.py:137-179).  bench.py itself
    compares this workload with the oracle's value on the box's host (`headline_parity`)."""
    import fvgp_amd
    import torch
    n = 50000
    x, y = synth(n, 3)
    nv = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=nv, kernel_function="rbf_ard")
    H = gp._H
    K = H.empty(n, n)
    H.kmat(0, gp._x_dev, gp._x_dev, theta, K)
    H.sync()
    alpha = gp._alpha[:n, 0]
    ym = H.to_device(y - np.mean(y))
    res = K @ alpha + H.to_device(nv) * alpha - ym
    assert float(res.norm() / ym.norm()) < 1e-9
    rng = np.random.default_rng(1)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, (64, 2))] + [(n - 1, n - 1), (0, 0), (n - 1, 0), (n - 1, n - 2)]
    got = _entries_of_LLt(gp, pairs)
    want = np.array([float(K[i, j].item()) + (nv[i] if i == j else 0.0) for i, j in pairs])
    assert np.max(np.abs(got - want)) < 1e-11
    del K
    torch.cuda.empty_cache()
    quad = float((ym * alpha).sum().item())
    ll = -0.5 * (quad + gp.logdet_KV + n * np.log(2 * np.pi))
    np.testing.assert_allclose(gp.log_likelihood(), ll, rtol=1e-12)
    # log|KV| = 2 sum log L_ii from the factor itself
    np.testing.assert_allclose(gp.logdet_KV, 2.0 * float(torch.log(gp._L.diagonal()[:n]).sum().item()), rtol=1e-12)
    l2 = gp.log_likelihood(theta * 1.02)
    assert np.isfinite(l2) and l2 != ll
    np.testing.assert_allclose(gp.log_likelihood(theta), ll, rtol=1e-12)


def test_config3_n50000_matern52_value_and_gradient():
    """C3: N=50k d=3 Matern-5/2: log marginal likelihood + hyperparameter gradient on one MI355X."""
    import fvgp_amd
    n = 50000
    x, y = synth(n, 3)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    gp = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=np.full(n, 0.01), kernel_function="matern52_ard")
    g = gp.neg_log_likelihood_gradient(theta)
    assert g.shape == (4,) and np.all(np.isfinite(g))
    u = np.array([0.5, -0.3, 0.6, 0.2]); u /= np.linalg.norm(u)
    eps = 2e-5
    fd = (gp.neg_log_likelihood(theta + eps * u) - gp.neg_log_likelihood(theta - eps * u)) / (2 * eps)
    np.testing.assert_allclose(g @ u, fd, rtol=2e-6)
    # the state was not touched by the evaluations at other theta
    np.testing.assert_allclose(gp.log_likelihood(theta), gp.log_likelihood(), rtol=1e-12)


def test_config5_multitask_4x10000():
    """C5: fvGP, 4 tasks x 10 000 points, d=2 -> N=40 000 over the (x, task) index set, default kernel."""
    import fvgp_amd
    rng = np.random.default_rng(20240501)
    xm = rng.random((10000, 2))
    s = xm.sum(axis=1)
    ym = np.stack([np.sin(3 * s), np.cos(3 * s), np.linalg.norm(xm, axis=1), np.sin(3 * s) * np.cos(3 * s)], axis=1)
    ym = ym + 0.05 * rng.standard_normal(ym.shape)
    theta = np.array([1.0, 0.3, 0.3, 1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(xm, ym, init_hyperparameters=theta, noise_variances=np.full(ym.shape, 0.01))
    assert gp.x_data.shape == (40000, 3)
    assert np.array_equal(gp.x_data[10000:10005, :2], xm[:5]) and np.all(gp.x_data[10000:20000, 2] == 1.0)
    H, n = gp._H, 40000
    K = H.empty(n, n)
    H.kmat(1, gp._x_dev, gp._x_dev, theta, K)
    H.sync()
    alpha = gp._alpha[:n, 0]
    rhs = H.to_device(gp.y_data[:, 0] - np.mean(gp.y_data))
    res = K @ alpha + 0.01 * alpha - rhs
    assert float(res.norm() / rhs.norm()) < 1e-9
    del K
    xp = rng.random((32, 2))
    pm = gp.posterior_mean(xp)["m(x)"]
    assert pm.shape == (32, 4)
    s2 = xp.sum(axis=1)
    assert np.max(np.abs(pm[:, 0] - np.sin(3 * s2))) < 0.15 and np.max(np.abs(pm[:, 1] - np.cos(3 * s2))) < 0.15
    pc = gp.posterior_covariance(xp)
    assert pc["S"].shape == (32, 32, 4, 4) and pc["v(x)"].shape == (32, 4) and np.all(pc["v(x)"] >= 0)


def test_config5_shape_4x2500_against_the_oracle():
    """C5's shape at a quarter of its size (4 tasks x 2 500 points -> N = 10 000 over the index set; the oracle runs it in seconds)
    against the oracle's multi-task restatement: index-set transform, log-likelihood, gradient, posterior reshapes."""
    import fvgp_amd
    from oracle import fvgp_oracle as orc
    rng = np.random.default_rng(20240501)
    xm = rng.random((2500, 2))
    s = xm.sum(axis=1)
    ym = np.stack([np.sin(3 * s), np.cos(3 * s), np.linalg.norm(xm, axis=1), np.sin(3 * s) * np.cos(3 * s)], axis=1)
    ym = ym + 0.05 * rng.standard_normal(ym.shape)
    theta = np.array([1.0, 0.3, 0.3, 1.0])
    nvm = np.full(ym.shape, 0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.fvGP(xm, ym, init_hyperparameters=theta, noise_variances=nvm)
    xi, yi, nvi = orc.transform_index_set(xm, ym, nvm)
    assert np.array_equal(gp.x_data, xi) and np.array_equal(gp.y_data[:, 0], yi)
    ref = orc.OracleGP(xi, yi, theta, nvi, kernel="matern32_ard", x_out=np.arange(4))
    np.testing.assert_allclose(gp.log_likelihood(), ref.log_likelihood(), rtol=1e-10)
    t2 = theta * np.array([1.2, 0.9, 1.1, 0.8])
    np.testing.assert_allclose(gp.log_likelihood(t2), ref.log_likelihood(t2), rtol=1e-10)
    assert np.max(np.abs(gp.KVinvY - ref.KVinvY)) <= 1e-8 * np.max(np.abs(ref.KVinvY))
    g, g_ref = gp.neg_log_likelihood_gradient(theta), ref.neg_log_likelihood_gradient_potri(theta)
    np.testing.assert_allclose(g, g_ref, rtol=1e-7, atol=1e-8 * np.max(np.abs(g_ref)))
    xp = rng.random((16, 2))
    pm, rm = gp.posterior_mean(xp), ref.posterior_mean(xp)
    assert pm["m(x)"].shape == (16, 4)
    np.testing.assert_allclose(pm["m(x)"], rm["m(x)"], rtol=1e-8, atol=1e-10)
    pc, rc = gp.posterior_covariance(xp), ref.posterior_covariance(xp)
    assert pc["S"].shape == (16, 16, 4, 4)
    assert np.max(np.abs(pc["S"] - rc["S"])) <= 1e-10 * theta[0]
    assert np.max(np.abs(pc["v(x)"] - rc["v(x)"])) <= 1e-10 * theta[0]


def test_config4_size_n100000_two_drivers_agree():
    """C4's size (N=100k, an 80 GB matrix) on the one GPU of the test box: the single-GPU driver
    (fvgp_hip_loglik) and the row-sharded driver at world size 1 (fvgp_amd/dist.py: tall-panel chain on a
    second stream, sharded trailing update, (y-m)^T carried as a block row) are two independent schedules of
    the same factorisation; log-likelihood, log-det and data fit must agree, and a few entries of L L^T are
    checked against re-assembled K+V."""
    import torch
    from fvgp_amd import _lib
    from fvgp_amd.dist import ShardedGP
    from fvgp_amd.device import default_handle
    from oracle import fvgp_oracle as orc
    n = 100000
    x, y = synth(n, 3)
    nv = np.full(n, 0.01)
    theta = np.array([1.0, 0.3, 0.3, 0.3])
    H = default_handle()
    npad = _lib.pad128(n)
    KV = H.empty(npad, npad)
    alpha = H.empty(npad, 1)
    ll, logdet, quad, info = H.loglik(0, H.to_device(x), theta, H.to_device(nv), H.to_device((y - y.mean()).reshape(n, 1)), KV, alpha)
    assert info == 0 and np.isfinite(ll)
    rng = np.random.default_rng(3)
    pairs = [(int(i), int(j)) for i, j in zip(rng.integers(0, n, 12), rng.integers(0, n, 12))] + [(n - 1, n - 1), (n - 1, 0)]
    got = []
    for i, j in pairs:
        m = min(i, j) + 1
        got.append(float((KV[i, :m] * KV[j, :m]).sum().item()))
    want = np.array([orc.rbf_ard(x[i:i + 1], x[j:j + 1], theta)[0, 0] + (0.01 if i == j else 0.0) for i, j in pairs])
    assert np.max(np.abs(np.array(got) - want)) <= 1e-11
    del KV
    torch.cuda.empty_cache()
    gp = ShardedGP(x, y, nv, kernel="rbf_ard", panel=1024, rank=0, world=1)
    ll2, logdet2, quad2 = gp.log_likelihood(theta)
    np.testing.assert_allclose(logdet2, logdet, rtol=1e-12)
    np.testing.assert_allclose(quad2, quad, rtol=1e-9)
    np.testing.assert_allclose(ll2, ll, rtol=1e-11)
    del gp
    torch.cuda.empty_cache()


def _bench(args, tmp_path, timeout):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                         env=env, timeout=timeout, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain `bench.py --gpus 1` run: the headline only (no side records), --steps timed steps, ms_per_step; --dump-outputs
    writes the last step's outputs, the same ones for the same arguments (the inputs are seeded)."""
    n = 3000
    outs = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        line = _bench(["--steps", "3", "--warmup", "1", "--npoints", str(n), "--dump-outputs", str(d)], tmp_path, 300)
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "f64"
        assert line["metric"] == "log_marginal_likelihood_evals_per_sec" and line["unit"] == "evals/s" and line["higher_is_better"]
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-6 * 1e3
        assert not {"configs", "cpu_baseline", "headline_parity"} & set(line)
        files = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert set(files) == {"loglik", "logdet", "quad", "alpha", "factor_diag", "factor_lower_sample"}
        assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert files["loglik"][0] == line["loglik_last"] and files["alpha"].shape == (n,) and files["factor_diag"].shape == (n,)
        assert np.all(files["factor_diag"] > 0)
        np.testing.assert_allclose(files["logdet"][0], 2.0 * np.sum(np.log(files["factor_diag"])), rtol=1e-12)
        outs.append(files)
    for name in outs[0]:
        np.testing.assert_array_equal(outs[0][name], outs[1][name], err_msg=name)
    # the last timed step is theta_0 (1 + 0.02 (warmup + steps - 1)): the same value the oracle gives
    from oracle import fvgp_oracle as orc
    x, y = synth(n, 3)
    ref, _ = orc.log_likelihood_once(x, y, np.full(n, 0.01), np.array([1.0, 0.3, 0.3, 0.3]) * 1.06, "rbf_ard")
    assert abs(outs[0]["loglik"][0] - ref) <= 1e-10 * abs(ref)


def test_bench_full_run_keeps_the_cpu_leg_and_the_parity_check(tmp_path):
    """`--full` adds what a plain run leaves out: the CPU leg (the oracle on this host) and the headline's agreement with it."""
    line = _bench(["--steps", "2", "--warmup", "1", "--npoints", "3000", "--full"], tmp_path, 600)
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["oracle_n"] > 0
    assert line["headline_parity"]["ok"] and line["headline_parity"]["rel_diff"] <= 1e-10
