"""Every entry of the C ABI that takes a caller-owned workspace, held to its size query (tests/vecchia_device.py's frames, for workspaces):

  run A  the workspace is a 16-byte aligned view of EXACTLY the queried size inside a canary-filled tensor, 16 doubles of frame on
         each side -- the frames must be untouched afterwards: nothing is written past either end;
  run B  the workspace is twice that size and filled with NaN -- the outputs of A and B must be bit-equal: nothing depends on what the
         workspace held or on how large it is.

Shapes are the smallest that reach both sides of a tile edge (n = 129 and 300, P = 65, q = 5, k = 3, B = 2, m = 5, s = 3, nsamp = 3,
lanczos_steps = 7, d = 3 and for the Hessian also 5), one kernel id.  The three batched evaluations own their buffer and cannot be framed:
test_gpu_batch_accuracy.py, test_gpu_loglik_batch.py, test_gpu_loglik_grad_batch.py and test_gpu_posterior_batch.py cover them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = -7.25e300
FRAME = 16
KERNEL = "rbf_ard"
NS = (129, 300)
P, Q, K, B, M, S, NSAMP, LANCZOS = 65, 5, 3, 2, 5, 3, 3, 7


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _exact(H, nbytes):
    """(buffer, view): a 16-byte aligned view of exactly nbytes inside a canary-filled flat buffer"""
    assert nbytes > 0 and nbytes % 8 == 0
    big = H.torch.full((nbytes // 8 + 2 * FRAME,), CANARY, dtype=H.torch.float64, device=f"cuda:{H.device}")
    view = big[FRAME:FRAME + nbytes // 8]
    assert view.data_ptr() % 16 == 0 and view.numel() * 8 == nbytes
    return big, view


def _roomy(H, nbytes):
    return H.torch.full((2 * (nbytes // 8),), float("nan"), dtype=H.torch.float64, device=f"cuda:{H.device}")


def _frames_untouched(big):
    a = big.cpu().numpy()
    return bool(np.all(a[:FRAME] == CANARY) and np.all(a[-FRAME:] == CANARY))


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _hold(H, nbytes, call):
    """call(work) -> outputs, once per run; the frames of run A and the bit-equality of the two runs' outputs"""
    big, view = _exact(H, nbytes)
    a = [_host(t) for t in call(view)]
    H.sync()
    assert _frames_untouched(big), "the entry wrote outside a workspace of exactly the queried size"
    b = [_host(t) for t in call(_roomy(H, nbytes))]
    H.sync()
    assert len(a) == len(b) and len(a) > 0
    for i, (u, v) in enumerate(zip(a, b)):
        assert not np.any(np.isnan(u.astype(np.float64))), f"output {i} of run A holds NaN"
        assert np.array_equal(u, v), f"output {i} depends on the workspace's contents or size"


_PROBLEMS = {}


def _problem(H, n, d=3):
    """inputs of n points in d dimensions, the factor of K + V as Handle.loglik leaves it and KV^-1 y: computed once, never written"""
    from fvgp_amd import _lib
    if (n, d) not in _PROBLEMS:
        rng = np.random.default_rng(1000 * d + n)
        x = rng.random((n, d))
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
        p = {"n": n, "d": d, "kid": _lib.KERNEL_IDS[KERNEL], "theta": np.concatenate([[1.2], rng.uniform(0.3, 0.5, d)]),
             "x": x, "xd": H.to_device(x), "v": np.full(n, 0.01), "r": (y - y.mean()), "xp": rng.random((P, d)),
             "rhs": rng.standard_normal((n, S))}
        p["vd"], p["rd"] = H.to_device(p["v"]), H.to_device(p["r"])
        dim = _lib.loglik_dim(n, 1)
        p["KV"], p["alpha"] = H.empty(dim, dim), H.empty(_lib.pad128(n), 1)
        info = H.loglik(p["kid"], p["xd"], p["theta"], p["vd"], H.to_device(p["r"].reshape(n, 1)), p["KV"], p["alpha"])[3]
        assert info == 0
        _PROBLEMS[n, d] = p
    return _PROBLEMS[n, d]


def _lowrank(H, p):
    """the pivoted factor G (Q, n) of the problem and the factor C of its preconditioner, computed once"""
    from fvgp_amd import _lib
    if "G" not in p:
        G, piv = H.zeros(Q, p["n"]), H.torch.zeros(Q, dtype=H.torch.int64, device=p["xd"].device)
        assert H.pchol(p["kid"], p["xd"], p["theta"], Q, G, piv) == Q
        C = H.zeros(_lib.pad128(Q), _lib.pad128(Q))
        assert H.precond_factor(G, Q, p["n"], p["vd"], C) == 0
        p["G"], p["C"] = G, C
    return p["G"], p["C"]


def _lists(H, p):
    """the causal neighbour lists (n, M) of the problem's points in their order, on the device, computed once"""
    if "idx" not in p:
        idx = H.torch.full((p["n"], M), -1, dtype=H.torch.int32, device=p["xd"].device)
        H.nn_search(p["xd"], p["xd"], M, idx, c0=0)
        H.sync()
        p["idx"] = idx
    return p["idx"]


def _nn_factor(H, p):
    if "factor" not in p:
        factor, info = H.nn_factor(p["kid"], p["xd"], p["theta"], _lists(H, p), M, p["vd"])
        assert info == 0
        p["factor"] = factor
    return p["factor"]


def _thetas(p):
    return np.stack([p["theta"], 1.25 * p["theta"]])[:B]


def _lower(t, n):
    return np.tril(_host(t)[:n, :n])


# ---- the dense path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_loo(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    np_ = _lib.pad128(n)

    def call(ws):
        resid, var, u, md = H.zeros(n), H.zeros(n), H.zeros(n), H.zeros(n)
        out, g = H.loo(p["kid"], p["xd"], p["theta"], p["alpha"], 1, 0, p["KV"].clone(), H.zeros(np_, np_), ws, resid, var, u, md)
        return out, g, resid, var, u, md
    _hold(H, _lib.loo_workspace_bytes(n), call)


@pytest.mark.parametrize("n,d", [(n, d) for n in NS for d in (3, 5)])
def test_loglik_hess(H, n, d):
    from fvgp_amd import _lib
    p = _problem(H, n, d)
    np_ = _lib.pad128(n)

    def call(ws):
        return H.loglik_hess(p["kid"], p["xd"], p["theta"], p["alpha"], 1, 0, p["KV"].clone(), H.zeros(np_, np_), H.zeros(np_, np_), ws)
    _hold(H, _lib.loglik_hess_workspace_bytes(n, d), call)


@pytest.mark.parametrize("n", NS)
def test_posterior_grad(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    W = H.zeros(_lib.pad128(n), _lib.pad128(P))
    xpd = H.to_device(p["xp"])
    H.kmat(p["kid"], p["xd"], xpd, p["theta"], W, pad=_lib.PAD_ZERO)
    H.potrs_cols(p["KV"], n, W, _lib.pad128(P))

    def call(work):
        A, q, dm, dv = H.zeros(P), H.zeros(P), H.zeros(P, p["d"]), H.zeros(P, p["d"])
        H.posterior_grad(p["kid"], p["xd"], p["theta"], xpd, p["alpha"], 1, 0, W, p["d"], work, A, q, dm, dv)
        return A, q, dm, dv
    _hold(H, _lib.posterior_grad_workspace_bytes(n, P, p["d"]), call)


@pytest.mark.parametrize("n", NS)
def test_mvn_sample(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)

    def call(work):
        Y, Z = H.zeros(NSAMP, n), H.zeros(n, NSAMP)
        H.mvn_sample(p["KV"], n, Y, mean=p["rd"], seed=11, stream=3, Z_out=Z, work=work)
        return Y, Z
    _hold(H, _lib.mvn_sample_workspace_bytes(n, NSAMP), call)


@pytest.mark.parametrize("n", NS)
def test_select_batch(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    xcd = H.to_device(p["xp"])
    var0 = H.to_device(np.linspace(0.5, 1.0, P))

    def call(work):
        var, idx = var0.clone(), H.torch.zeros(Q, dtype=H.torch.int64, device=var0.device)
        pick, G = H.zeros(Q), H.zeros(Q, P)
        H.select_batch(p["kid"], p["xd"], p["theta"], p["KV"], xcd, var, Q, idx, pick, G_out=G, work=work)
        return var, idx, pick, G
    _hold(H, _lib.select_workspace_bytes(n, P, Q), call)


@pytest.mark.parametrize("n", NS)
def test_chol_update_and_delete(H, n):
    from fvgp_amd import _lib
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    np_ = _lib.pad128(n)
    host = np.eye(np_)
    host[:n, :n] = np.linalg.cholesky(A @ A.T + n * np.eye(n))
    W = rng.standard_normal((n, K))

    def update(ws):
        L = H.to_device(host)
        H.chol_update(L, n, H.to_device(W), work=ws)
        H.invalidate_factor()
        return (_lower(L, n),)
    _hold(H, _lib.CHOL_UPDATE_TABLE_BYTES, update)

    def delete(ws):
        L = H.to_device(host)
        H.chol_delete(L, n, [1, n // 2, n - 2], work=ws)
        H.invalidate_factor()
        return (_lower(L, n - K),)
    _hold(H, _lib.chol_update_workspace_bytes(n, K), delete)


# ---- the matrix-free path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_kmatvec_and_kgrad_form(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    U, W = H.to_device(p["rhs"]), H.to_device(p["rhs"][::-1].copy())

    def matvec(work):
        Y = H.zeros(n, S)
        H.kmatvec(p["kid"], p["xd"], p["xd"], p["theta"], U, Y, vdiag=p["vd"], work=work)
        return (Y,)
    _hold(H, _lib.kmatvec_workspace_bytes(n, n, S), matvec)
    _hold(H, _lib.kgrad_form_workspace_bytes(n, n), lambda work: (H.kgrad_form(p["kid"], p["xd"], U, p["xd"], W, p["theta"], work=work),))


@pytest.mark.parametrize("n", NS)
def test_pchol_and_precond_factor(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)

    def pchol(work):
        G, piv, resid = H.zeros(Q, n), H.torch.zeros(Q, dtype=H.torch.int64, device=p["xd"].device), H.zeros(n)
        rank = H.pchol(p["kid"], p["xd"], p["theta"], Q, G, piv, resid_diag_out=resid, work=work)
        return np.array([rank]), G, piv, resid
    _hold(H, _lib.pchol_workspace_bytes(n, Q), pchol)
    G, _ = _lowrank(H, p)

    def factor(work):
        C = H.zeros(_lib.pad128(Q), _lib.pad128(Q))
        info = H.precond_factor(G, Q, n, p["vd"], C, work=work)
        return np.array([info]), _lower(C, Q)
    _hold(H, _lib.precond_workspace_bytes(n, Q), factor)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("rank", [0, Q])
def test_pcg_and_lanczos(H, n, rank):
    from fvgp_amd import _lib
    p = _problem(H, n)
    G, C = _lowrank(H, p) if rank else (None, None)
    Bd = H.to_device(p["rhs"])

    def pcg(work):
        X = H.zeros(n, S)
        return (*H.pcg(p["kid"], p["xd"], p["theta"], p["vd"], Bd, X, G=G, q=rank, C=C, tol=1e-8, max_iter=200, work=work), X)
    _hold(H, _lib.pcg_workspace_bytes(n, rank), pcg)

    def lanczos(work):
        X = H.zeros(n, S)
        return (*H.pcg_lanczos(p["kid"], p["xd"], p["theta"], p["vd"], Bd, X, LANCZOS, G=G, q=rank, C=C, tol=1e-8, max_iter=200, work=work), X)
    _hold(H, _lib.pcg_lanczos_workspace_bytes(n, rank, LANCZOS), lanczos)


@pytest.mark.parametrize("n", NS)
def test_precond_apply(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    G, C = _lowrank(H, p)
    R = H.to_device(p["rhs"])

    def call(work):
        W = H.zeros(n, S)
        H.precond_apply(R, W, p["vd"], G=G, q=Q, C=C, work=work)
        return (W,)
    _hold(H, _lib.precond_apply_workspace_bytes(n, Q), call)


@pytest.mark.parametrize("n", NS)
def test_nn_precond_apply_and_pcg_nn(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    factor = _nn_factor(H, p)
    R = H.to_device(p["rhs"])

    def apply(work):
        Z = H.zeros(n, S)
        H.nn_precond_apply(factor, R, Z, work=work)
        return (Z,)
    _hold(H, _lib.nn_precond_apply_workspace_bytes(n), apply)

    def pcg(work):
        X = H.zeros(n, S)
        return (*H.pcg_nn(p["kid"], p["xd"], p["theta"], p["vd"], R, X, factor, tol=1e-8, max_iter=200, work=work), X)
    _hold(H, _lib.pcg_nn_workspace_bytes(n), pcg)


# ---- the nearest-neighbour path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_nn_conditionals_and_factor(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)
    idx = _lists(H, p)

    def conditionals(work):
        mu, var = H.zeros(B, n), H.zeros(B, n)
        info = H.nn_conditionals(p["kid"], p["xd"], p["xd"], _thetas(p), idx, M, p["rd"], p["vd"], mu, var, s=p["vd"], work=work)
        return np.array([info]), mu, var
    _hold(H, _lib.nn_workspace_bytes(_lib.NN_CONDITIONALS, n, B), conditionals)

    def factor(work):
        f, info = H.nn_factor(p["kid"], p["xd"], p["theta"], idx, M, p["vd"], transposed=(None, None, 0), work=work)
        return np.array([info]), f.coef, f.dinv
    _hold(H, _lib.nn_factor_workspace_bytes(n), factor)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_nn_loglik_levels(H, n, level):
    from fvgp_amd import _lib
    p = _problem(H, n)
    idx = _lists(H, p)
    nth = len(p["theta"])
    nbytes = (_lib.nn_workspace_bytes(_lib.NN_LOGLIK, n, B), _lib.nn_grad_workspace_bytes(n, B, nth), _lib.nn_fisher_workspace_bytes(n, B, nth))[level]

    def call(work):
        rows = [H.zeros(B, n), H.zeros(B, n), H.zeros(B, n, nth), H.zeros(B, n, nth * (nth + 1) // 2)][:2 + level]
        entry = (H.nn_loglik, H.nn_loglik_grad, H.nn_loglik_fisher)[level]
        host = entry(p["kid"], p["xd"], _thetas(p), idx, M, p["rd"], p["vd"], *rows, work=work)
        return (*(np.asarray(a) for a in host), *rows)
    _hold(H, nbytes, call)


@pytest.mark.parametrize("n", NS)
def test_nn_maxmin_order(H, n):
    from fvgp_amd import _lib
    p = _problem(H, n)

    def call(work):
        perm, dist = H.torch.zeros(n, dtype=H.torch.int64, device=p["xd"].device), H.zeros(n)
        H._call("fvgp_hip_nn_maxmin_order", _lib._ptr(p["xd"]), n, p["d"], None, 0, n, _lib._ptr(perm), _lib._ptr(dist), _lib._ptr(work),
                work.numel() * 8)
        H.sync()
        return perm, dist[1:]                       # (dist[0] is inf by definition)
    _hold(H, _lib.nn_maxmin_workspace_bytes(n), call)


@pytest.mark.parametrize("n", NS)
def test_nn_grid_build_and_search(H, n):
    """both buffers of the build are framed; the search then reads the framed grid"""
    from fvgp_amd import _lib
    p = _problem(H, n)
    gbytes, wbytes = _lib.nn_grid_bytes(n, p["d"]), _lib.nn_grid_workspace_bytes(n, p["d"])
    results = []
    for grid_buf, work in ((_exact(H, gbytes), _exact(H, wbytes)), ((None, _roomy(H, gbytes)), (None, _roomy(H, wbytes)))):
        info = np.zeros(_lib.NN_GRID_INFO)
        H._call("fvgp_hip_nn_grid_build", _lib._ptr(p["xd"]), n, p["d"], None, _lib._ptr(grid_buf[1]), grid_buf[1].numel() * 8,
                _lib._ptr(work[1]), work[1].numel() * 8, info.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        H.sync()
        idx = H.torch.full((n, M), -1, dtype=H.torch.int32, device=p["xd"].device)
        H.nn_grid_search(p["xd"], p["xd"], M, idx, _lib.NNGrid(grid_buf[1], info, n, p["d"]), c0=0)
        H.sync()
        for big in (grid_buf[0], work[0]):
            assert big is None or _frames_untouched(big), "the build or the search wrote outside a buffer of exactly the queried size"
        results.append((info, _host(idx)))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert np.array_equal(results[0][1], _host(_lists(H, p))), "the grid search gives nn_search's lists"
