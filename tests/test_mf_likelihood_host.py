"""The numpy twin of the stochastic log-likelihood (tests/mf_likelihood_ref.py) against dense linear algebra: the Lanczos quadrature of
the recorded CG coefficients, the probes' covariance, log det of the preconditioner, the trace estimator, and the fixture / seed pairs
the device test leans on.  No GPU."""
import numpy as np
import pytest

import matrix_free_ref as mf
import mf_likelihood_ref as ml


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def test_abi_symbols_and_size_queries(L):
    from fvgp_amd import _lib
    for s in ("fvgp_hip_kgrad_form", "fvgp_hip_kgrad_form_workspace_bytes", "fvgp_hip_precond_probes", "fvgp_hip_precond_apply",
              "fvgp_hip_precond_apply_workspace_bytes", "fvgp_hip_pcg_lanczos", "fvgp_hip_pcg_lanczos_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert _lib.LANCZOS_MAX_STEPS == 256 and len(L.fvgp_hip_pcg_lanczos.argtypes) == len(L.fvgp_hip_pcg.argtypes) + 5
    # the records behind the solver's workspace: alpha and beta (16, L), rho0, and two rows for steps and first
    assert _lib.pcg_lanczos_workspace_bytes(1000, 128, 0) == _lib.pcg_workspace_bytes(1000, 128)
    assert _lib.pcg_lanczos_workspace_bytes(1000, 128, 64) == _lib.pcg_workspace_bytes(1000, 128) + 16 * (2 * 64 + 3) * 8
    assert _lib.pcg_lanczos_workspace_bytes(1000, 128, 257) == -1 and _lib.pcg_lanczos_workspace_bytes(0, 0, 1) == -1
    # the result and the blocks' sums, 17 doubles each; the parked chunk sums only while the launch would split by itself
    assert _lib.kgrad_form_workspace_bytes(130, 100) == (1 + 3) * 17 * 8
    assert _lib.kgrad_form_workspace_bytes(130, 2 * mf.CHUNK + 1) == ((1 + 3) * 17 + 3 * 130 * 17) * 8
    assert _lib.kgrad_form_workspace_bytes(200000, 200000) == (1 + 3125) * 17 * 8
    assert _lib.kgrad_form_workspace_bytes(0, 1) == -1 and _lib.precond_apply_workspace_bytes(0, 0) == -1
    assert _lib.precond_apply_workspace_bytes(10 ** 6, 256) < 1 << 30
    # refused before anything touches a device
    assert L.fvgp_hip_kgrad_form(None, 0, None, 0, None, 0, 0, None, 0, None, 0, None, 0, 0, None, 0, None) == -1
    assert L.fvgp_hip_precond_probes(None, 0, 0, 0, None, 0, 0, 0, None, None, 0, 0) == -1
    assert L.fvgp_hip_precond_apply(None, None, 0, 0, None, 0, 0, None, None, 0, 0, None, 0, None, 0) == -1


def _small_system(n=40, rank=8):
    f = mf.fixture(mf.FIXTURES[1])
    x, v, theta = f["x"][:n].copy(), f["V"][:n].copy(), f["theta"]
    K = mf.k_double(f["kernel"], x, theta)
    G = mf.pchol_ref(K, rank, sigma2=mf.SIGMA2)[0]
    return f["kernel"], x, v, theta, K, K + np.diag(v), G


def test_quadrature_of_the_recorded_coefficients_is_the_log_quadratic_form():
    """L = n on a 40-point system, the solve driven to 1e-14: rho_0 e_1^T log(T) e_1 = zhat^T log(Ahat) zhat from a dense
    eigendecomposition of Ahat = Lm^-1 A Lm^-T, zhat = Lm^-1 z, M = Lm Lm^T (any square root of M gives the same number), 1e-8 relative"""
    _, _, v, _, _, A, G = _small_system()
    n = len(v)
    M = G.T @ G + np.diag(v)
    Lm = np.linalg.cholesky(M)
    Ahat = np.linalg.solve(Lm, np.linalg.solve(Lm, A).T)
    lam, Q = np.linalg.eigh(0.5 * (Ahat + Ahat.T))
    Z = ml.probes_ref(3, 0, 0, 4, G, v)
    for c in range(4):
        zh = np.linalg.solve(Lm, Z[:, c])
        want = float(np.sum((Q.T @ zh) ** 2 * np.log(lam)))
        _, it, _, st, al, be, rho0 = ml.pcg_lanczos_ref(A, Z[:, c], v, G, 1e-14, n, max_iter=n)
        assert len(al) == it <= n and len(be) >= it - 1
        assert abs(rho0 - zh @ zh) <= 1e-12 * rho0
        got = ml.quadrature(al, be, rho0)
        print(c, "steps", it, "quadrature", got, "dense", want)
        assert abs(got - want) <= 1e-8 * abs(want)
        T = ml.lanczos_T(al, be)
        assert np.array_equal(T, T.T) and np.all(np.triu(T, 2) == 0.0)
    # a 1 x 1 T: one step gives rho_0 log(1 / alpha_0)
    assert ml.quadrature(np.array([0.5]), np.array([]), 3.0) == pytest.approx(3.0 * np.log(2.0), rel=1e-15)
    assert ml.quadrature(np.array([]), np.array([]), 3.0) == 0.0


def test_records_stop_at_L_and_at_the_first_restart():
    _, _, v, _, _, A, G = _small_system()
    z = ml.probes_ref(3, 0, 0, 1, G, v)[:, 0]
    full = ml.pcg_lanczos_ref(A, z, v, G, 1e-10, 64)
    cut = ml.pcg_lanczos_ref(A, z, v, G, 1e-10, 3)
    assert full[1] > 3 and len(cut[4]) == 3 and len(cut[5]) == 3
    assert np.array_equal(cut[4], full[4][:3]) and np.array_equal(cut[5], full[5][:3]) and cut[6] == full[6]
    assert np.array_equal(cut[0], full[0]) and cut[1] == full[1]                 # the solve does not depend on what is recorded
    ref = mf.pcg_ref(A, z, v, G, 1e-10)
    assert np.array_equal(ref[0], full[0]) and ref[1:] == full[1:4]              # ... and is matrix_free_ref's
    assert len(ml.pcg_lanczos_ref(A, z, v, G, 1e-10, 0)[4]) == 0


def test_probe_map_reproduces_the_preconditioner():
    """[D^1/2, G^T] [D^1/2, G^T]^T = G^T G + D as a matrix product (to the rounding of sqrt(v)^2), also without G"""
    _, _, v, _, _, _, G = _small_system()
    n, q = len(v), len(G)
    P = np.hstack([ml.probe_map(np.eye(n), np.zeros((q, n)), G, v), ml.probe_map(np.zeros((n, q)), np.eye(q), G, v)])
    M = G.T @ G + np.diag(v)
    assert np.max(np.abs(P @ P.T - M)) <= 4 * ml.EPS * np.max(np.abs(M))
    assert np.array_equal(ml.probe_map(np.eye(n), None, None, v), np.diag(np.sqrt(v)))
    # the two streams: eps and eta are different draws, and col0 shifts columns
    Z = ml.probes_ref(5, 2, 0, 6, G, v)
    assert np.array_equal(ml.probes_ref(5, 2, 2, 3, G, v), Z[:, 2:5])
    assert not np.array_equal(ml.probes_ref(5, 3, 0, 6, G, v), Z)


@pytest.mark.parametrize("fx", mf.FIXTURES[:4], ids=mf.fixture_id)
def test_logdet_of_the_preconditioner(fx):
    f = mf.fixture(fx)
    G = mf.fixture_pchol(fx)[0]
    want = np.linalg.slogdet(G.T @ G + np.diag(f["V"]))[1]
    assert abs(ml.logdet_precond(G, f["V"]) - want) <= 1e-10 * abs(want)
    assert ml.logdet_precond(None, f["V"]) == pytest.approx(np.sum(np.log(f["V"])), rel=1e-15)


def test_trace_term_with_dense_solves():
    """the assembled trace equals (1 / p) sum_c z_c^T A^-1 dK_j M^-1 z_c when its solves are driven to 1e-13"""
    kernel, x, v, theta, K, A, G = _small_system(n=120, rank=16)
    y = np.sin(5.0 * x[:, 0])
    e = ml.estimate_ref(kernel, x, y, v, theta, 16, n_probes=8, seed=4, gradient=True, probe_tol=1e-13, K=K, G=G)
    Z = ml.probes_ref(4, 0, 0, 8, G, v)
    assert np.array_equal(Z, e["Z"])
    M = G.T @ G + np.diag(v)
    dK = ml.dk_double(kernel, x, theta)
    U, W = np.linalg.solve(A, Z), np.linalg.solve(M, Z)
    for j in range(len(dK)):
        want = np.sum(U * (dK[j] @ W)) / 8
        assert abs(e["trace"][j] - want) <= 1e-9 * abs(want), (j, e["trace"][j], want)
    ref, mag = ml.kgrad_form_ref(kernel, x, U, x, W, theta)
    assert np.allclose(np.asarray(ref, dtype=np.float64) / 8, e["trace"], rtol=1e-9) and np.all(mag >= np.abs(ref))
    # the alpha term and the data fit
    alpha = np.linalg.solve(A, y - y.mean())
    assert abs(e["data_fit"] - 0.5 * (y - y.mean()) @ alpha) <= 1e-9 * abs(e["data_fit"])
    want_grad = np.array([-0.5 * alpha @ dK[j] @ alpha for j in range(len(dK))]) + 0.5 * e["trace"]
    assert np.allclose(e["neg_gradient"], want_grad, rtol=1e-7, atol=1e-9 * np.max(np.abs(want_grad)))


@pytest.mark.parametrize("fx", ml.ESTIMATE_FIXTURES, ids=mf.fixture_id)
def test_fixture_estimates_lie_within_three_standard_errors(fx):
    """rank 128, 16 probes, the seed the device test uses: log det within 3 of its reported standard errors of slogdet(A), every trace
    component within 3 of its standard errors of tr(A^-1 dK_j)"""
    e = ml.fixture_estimate(fx)
    logdet, traces = ml.fixture_dense(fx)
    z = (e["logdet"] - logdet) / e["logdet_std_error"]
    zt = (e["trace"] - traces) / e["trace_std_error"]
    print(mf.fixture_id(fx), "log det", e["logdet"], "dense", logdet, "standard error", e["logdet_std_error"], "z", z)
    print("   traces", e["trace"], "dense", traces, "z", zt, "iterations", e["iterations"].max(), "steps", e["lanczos_steps"].max())
    assert e["converged"] and e["lanczos_steps"].max() < ml.STEPS
    assert abs(z) <= 3.0
    assert np.all(np.abs(zt) <= 3.0)
    assert np.all(e["neg_gradient_std_error"] == 0.5 * e["trace_std_error"]) and e["std_error"] == 0.5 * e["logdet_std_error"]
