"""Matrix-free solves on the device (fvgp_hip_kmatvec, fvgp_hip_pchol, fvgp_hip_precond_factor, fvgp_hip_pcg, MatrixFreeGP): the entries
and the product against longdouble, the bit contracts, the pivoted Cholesky and the conjugate gradients against the numpy twin of
tests/matrix_free_ref.py, refused arguments, and the facade against the dense GP."""
import ctypes
import warnings

import numpy as np
import pytest

import kernel_family_ref as kf
import matrix_free_ref as mf

pytestmark = pytest.mark.gpu

CANARY = -7.25e300
ICANARY = -7777
TOL = 1e-9
CHUNK = mf.CHUNK


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _kid(kernel):
    from fvgp_amd import _lib
    return _lib.KERNEL_IDS[kernel]


def _framed(H, shape, dtype=None):
    """a canary-filled buffer with a frame around the view the call gets and an odd leading dimension: (buffer, view)"""
    t = H.torch
    if len(shape) == 1:
        big = t.full((shape[0] + 16,), ICANARY if dtype is not None else CANARY, dtype=dtype or t.float64, device=f"cuda:{H.device}")
        return big, big[8:8 + shape[0]]
    odd = 3 if shape[1] % 2 == 0 else 4
    big = t.full((shape[0] + 2, shape[1] + odd), CANARY, dtype=t.float64, device=f"cuda:{H.device}")
    assert big.stride(0) % 2 == 1
    return big, big[1:1 + shape[0], :shape[1]]


def _frame_untouched(big, view_shape):
    a = big.cpu().numpy()
    if a.ndim == 1:
        fill = ICANARY if a.dtype == np.int64 else CANARY
        return np.all(a[:8] == fill) and np.all(a[8 + view_shape[0]:] == fill)
    return np.all(a[0] == CANARY) and np.all(a[1 + view_shape[0]:] == CANARY) and np.all(a[:, view_shape[1]:] == CANARY)


def _matvec(H, kernel, x1, x2, theta, B, v=None, split=0, x1d=None, x2d=None):
    """one Handle.kmatvec call into a framed Y with the given "matvec_split"; B on the host, (n2, s)"""
    from fvgp_amd import _lib
    n1, n2, s = len(x1), len(x2), B.shape[1]
    x1d = H.to_device(x1) if x1d is None else x1d
    x2d = x1d if x2 is x1 else (H.to_device(x2) if x2d is None else x2d)
    Bd = H.to_device(B)
    ybig, Y = _framed(H, (n1, s))
    work = H.empty(max(1, _lib.kmatvec_workspace_bytes(n1, n2, s) // 8))
    H.set_option("matvec_split", split)
    try:
        H.kmatvec(_kid(kernel), x1d, x2d, theta, Bd, Y, vdiag=None if v is None else H.to_device(v), work=work)
        H.sync()
    finally:
        H.set_option("matvec_split", 0)
    assert _frame_untouched(ybig, (n1, s))
    return Y.cpu().numpy()


# ---- 1. the entries of K through the product --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(kf.FAMILY))
def test_identity_columns_return_the_entries_of_k(H, kernel):
    """B = I returns K: every entry within the project's 4 ulp sigma^2 of the longdouble value, every kernel id, d = 1 .. 5,
    coincident points (the diagonal, and a repeated point) included; 70 columns go as four groups of 16 and one of 8"""
    for d in (1, 2, 3, 4, 5):
        x1, x2, _, _ = mf.matvec_case(70, 70, d, 1, 100 + d, square=True)
        theta = mf.theta_of(kernel, d, 0.3)
        Y = _matvec(H, kernel, x1, x1, theta, np.eye(70))
        K = kf.k_ref(kernel, x1, x1, theta)
        err = float(np.max(np.abs(Y - K)))
        print(kernel, d, "largest entry error / (eps sigma^2):", err / (kf.EPS * mf.SIGMA2))
        assert err <= 4 * kf.EPS * mf.SIGMA2
        assert Y[69, 0] == Y[0, 0] == Y[5, 5]                   # coincident points: the same value as the diagonal


# ---- 2. the product against longdouble ---------------------------------------------------------------------------------------------------
# (kernel, d, n1, n2, s, vdiag, matvec_split): every n1 of {1, 63, 64, 65, 300}, every n2 of {1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1,
# 2 CHUNK + 37}, every s of {1, 3, 8, 16, 17}, vdiag on and off (on needs n1 == n2), split forced (k), forbidden (1) and by the shape (0);
# the last two are the runtime-dimension kernels (d = 5) with wide column groups and parked chunk sums
PRODUCT_CASES = [
    ("rbf_ard", 1, 1, 1, 1, True, 0),
    ("matern32_ard", 2, 63, 255, 3, False, 0),
    ("matern52_ard", 3, 64, 256, 8, False, 1),
    ("rbf_iso", 4, 65, 257, 16, False, 2),
    ("matern32_iso", 5, 300, 300, 17, True, 0),
    ("matern52_iso", 2, 64, 64, 1, True, 0),
    ("matern32_ard", 3, 300, CHUNK - 1, 1, False, 1),
    ("rbf_ard", 2, 64, CHUNK, 17, False, 0),
    ("matern52_ard", 3, 63, CHUNK + 1, 8, False, 3),
    ("matern52_ard", 3, 65, 2 * CHUNK + 37, 17, False, 3),
    ("matern32_ard", 1, 65, 2 * CHUNK + 37, 3, False, 1),
    ("rbf_ard", 3, 1, 2 * CHUNK + 37, 16, False, 0),
    ("matern32_ard", 2, 257, 257, 5, True, 2),
    ("rbf_ard", 5, 65, 2 * CHUNK + 37, 8, False, 3),
    ("matern52_iso", 5, 1, CHUNK + 1, 16, False, 2),
]


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_product_against_longdouble(H, case):
    """|Y - Y_ref|_ic <= 4 eps sigma^2 sum_j |B_jc| + (n2 + 4) (eps / 2) (|K| |B| + |v_i B_ic|)_ic: the entry error of test 1 plus
    Higham's gamma for a length-n2 sum in any order.  B has full-mantissa entries scaled over 2^-20 .. 2^20 by row.
    OBSERVED on an MI355X (an observation, not a bound): the largest share of the bound used over these cases was 0.067 (n2 = 64, and
    0.065 at n2 = 1, where the bound is the entry error almost alone); the cases with 255 <= n2 <= 300 used 0.008 .. 0.015 of it, the
    cases from n2 = 4095 on at most 0.0006.  The largest entry error of test 1 was 1.9 eps sigma^2."""
    kernel, d, n1, n2, s, vd, split = case
    x1, x2, B, v = mf.matvec_case(n1, n2, d, s, 7 * n1 + n2 + s, square=vd)
    theta = mf.theta_of(kernel, d, 0.3)
    Y = _matvec(H, kernel, x1, x2, theta, B, v=v if vd else None, split=split)
    ref, mag = mf.kmatvec_ref(kernel, x1, x2, theta, B, v if vd else None)
    bound = mf.kmatvec_bound(n2, B, mag)
    share = float(np.max(np.abs(Y - ref) / bound))
    print(case, "largest share of the bound:", share)
    assert np.all(np.abs(Y - ref) <= bound), share


# ---- 3. the bit contract of the product --------------------------------------------------------------------------------------------------
def test_product_bits_do_not_depend_on_the_rest_of_the_call(H):
    """column c alone against inside s = 17 (groups 16 + 1 against a group of 1); row i in calls of 1, 65 and 300 rows; split (forced 2, 3
    and by the shape) against unsplit at n2 = 2 CHUNK + 37; the same call twice; split 3 against unsplit on the runtime-dimension kernel
    (d = 5, n1 = 65, s = 16)"""
    kernel, d, n2, s = "matern52_ard", 3, 2 * CHUNK + 37, 17
    x1, x2, B, _ = mf.matvec_case(300, n2, d, s, 4242)
    theta = mf.theta_of(kernel, d, 0.3)
    x2d = H.to_device(x2)
    full = _matvec(H, kernel, x1, x2, theta, B, split=1, x2d=x2d)
    assert np.array_equal(full, _matvec(H, kernel, x1, x2, theta, B, split=1, x2d=x2d))
    for k in (0, 2, 3):
        assert np.array_equal(full, _matvec(H, kernel, x1, x2, theta, B, split=k, x2d=x2d)), k
    for c in (0, 7, 15, 16):
        assert np.array_equal(full[:, c], _matvec(H, kernel, x1, x2, theta, B[:, c:c + 1].copy(), split=1, x2d=x2d)[:, 0]), c
    assert np.array_equal(full[:, 3:8], _matvec(H, kernel, x1, x2, theta, B[:, 3:8].copy(), split=0, x2d=x2d))     # a group of 8
    for rows in (1, 65):
        for i0 in (0, 131):
            got = _matvec(H, kernel, x1[i0:i0 + rows].copy(), x2, theta, B, split=0, x2d=x2d)
            assert np.array_equal(full[i0:i0 + rows], got), (rows, i0)
    x5, y5, B5, _ = mf.matvec_case(65, n2, 5, 16, 4243)
    th5 = mf.theta_of(kernel, 5, 0.3)
    assert np.array_equal(_matvec(H, kernel, x5, y5, th5, B5, split=1), _matvec(H, kernel, x5, y5, th5, B5, split=3))
    # with vdiag (n1 == n2): rows cannot be cut, columns can
    xs, _, Bs, v = mf.matvec_case(300, 300, d, 17, 99, square=True)
    sq = _matvec(H, kernel, xs, xs, theta, Bs, v=v)
    assert np.array_equal(sq[:, 16], _matvec(H, kernel, xs, xs, theta, Bs[:, 16:].copy(), v=v)[:, 0])


# ---- 4. the pivoted Cholesky against the twin -----------------------------------------------------------------------------------------------
def _pchol(H, kernel, x, theta, q, tol=0.0, xd=None):
    n = len(x)
    xd = H.to_device(np.array(x)) if xd is None else xd
    gbig, G = _framed(H, (q, n))
    pbig, piv = _framed(H, (q,), dtype=H.torch.int64)
    dbig, dres = _framed(H, (n,))
    rank = H.pchol(_kid(kernel), xd, theta, q, G, piv, tol=tol, resid_diag_out=dres)
    assert _frame_untouched(gbig, (q, n)) and _frame_untouched(pbig, (q,)) and _frame_untouched(dbig, (n,))
    return G, piv.cpu().numpy(), dres.cpu().numpy(), rank


@pytest.mark.parametrize("fx", mf.PIVOT_FIXTURES, ids=mf.fixture_id)
def test_pchol_matches_the_twin(H, fx):
    """pivots equal over the first 24 steps (the fixtures lead by >= 1e-9 sigma^2 there: tests/test_matrix_free_host.py), G within
    1e-10 sigma^2 of the twin over those steps, and the residual diagonal of a 24-step run; over the full run of q = 64: distinct pivots,
    G[t, piv[s]] = 0 for s < t, the residual diagonal >= 0 and equal to sigma^2 - sum_t G[t, i]^2"""
    f = mf.fixture(fx)
    Gt, pivt, _, _, _ = mf.fixture_pchol(fx)
    G, piv, dres, rank = _pchol(H, f["kernel"], f["x"], f["theta"], 64)
    G = G.cpu().numpy()
    assert rank == 64
    assert np.array_equal(piv[:24], pivt[:24])
    assert np.max(np.abs(G[:24] - Gt[:24])) <= 1e-10 * mf.SIGMA2
    _, piv24, d24, r24 = _pchol(H, f["kernel"], f["x"], f["theta"], 24)
    assert r24 == 24 and np.array_equal(piv24, pivt[:24])
    dt = mf.SIGMA2 - np.sum(Gt[:24] ** 2, axis=0)
    assert np.max(np.abs(d24 - np.maximum(dt, 0.0))) <= 1e-10 * mf.SIGMA2
    assert len(set(piv.tolist())) == 64 and piv.min() >= 0
    for t in range(1, 64):
        assert np.max(np.abs(G[t, piv[:t]])) <= 1e-12 * np.sqrt(mf.SIGMA2), t
    assert dres.min() >= 0.0
    assert np.max(np.abs(dres - (mf.SIGMA2 - np.sum(G.astype(np.longdouble) ** 2, axis=0)))) <= 1e-12 * mf.SIGMA2


def test_pchol_bits_exhaustion_and_the_solve_behind_it(H):
    """a point's column of G has the same bits when points that are never pivots leave the call; 40 points at rank 64, tol 1e-10, exhaust:
    piv_out is -1 from the achieved rank on, the rows there are exactly zero, and the solve preconditioned with it is still correct"""
    fx = mf.FIXTURES[1]
    f = mf.fixture(fx)
    G, piv, _, _ = _pchol(H, f["kernel"], f["x"], f["theta"], 24)
    G = G.cpu().numpy()
    keep = np.sort(np.concatenate([piv, np.setdiff1d(np.arange(0, len(f["x"]), 3), piv)]))
    Gs, pivs, _, _ = _pchol(H, f["kernel"], f["x"][keep].copy(), f["theta"], 24)
    assert np.array_equal(keep[pivs], piv)
    assert np.array_equal(Gs.cpu().numpy(), G[:, keep])

    n, q = 40, 64
    x, V, theta = f["x"][:n].copy(), f["V"][:n].copy(), mf.theta_of("rbf_ard", 2, 0.25)
    xd = H.to_device(x)
    Gd, piv, dres, rank = _pchol(H, "rbf_ard", x, theta, q, tol=1e-10, xd=xd)
    Gh = Gd.cpu().numpy()
    assert 0 < rank <= n < q
    assert np.all(piv[rank:] == -1) and np.all(piv[:rank] >= 0) and len(set(piv[:rank].tolist())) == rank
    assert np.all(Gh[rank:] == 0.0) and dres.max() <= 1e-10 * mf.SIGMA2
    Vd, C = H.to_device(V), H.empty(128, 128)
    assert H.precond_factor(Gd, q, n, Vd, C) == 0
    b = f["rhs"][:n, :2].copy()
    xbig, X = _framed(H, (n, 2))
    it, rr, st = H.pcg(_kid("rbf_ard"), xd, theta, Vd, H.to_device(b), X, G=Gd, q=q, C=C, tol=TOL)
    assert _frame_untouched(xbig, (n, 2))
    A = np.asarray(kf.k_ref("rbf_ard", x, x, theta), dtype=np.float64) + np.diag(V)
    want = np.linalg.solve(A, b)
    assert np.all(st == 0) and np.all(rr <= TOL)
    assert np.linalg.norm(X.cpu().numpy() - want) <= np.linalg.cond(A) * TOL * np.linalg.norm(want)


def test_pchol_and_selection_share_kernels_not_state(H):
    """fvgp_hip_pchol, fvgp_hip_select_batch and fvgp_hip_pchol again, back to back on one handle and in ONE workspace: the selection (the
    information criterion, noise, repeats allowed, one that exhausts with repeats off) leaves nothing behind that the second
    factorisation reads.  n = 65 is two 64-point partials with a ragged second one, and the point at index 64 is the second pivot.
    Both factorisations: piv equal to the twin's (its picks lead by >= 1e-9 sigma^2 after the first, a tie that goes to index 0),
    G within 1e-10 sigma^2 of it, rank 8; the second equal to the first bit for bit; the frames around every output untouched."""
    from fvgp_amd import _lib
    fx = mf.FIXTURES[2]
    f = mf.fixture(fx)
    kernel, theta, n, q, P = f["kernel"], f["theta"], 65, 8, 5
    x, V = f["x"][:n].copy(), f["V"][:n].copy()
    x[[13, 64]] = x[[64, 13]]
    Gt, pivt, _, rankt, margins = mf.pchol_ref(mf.k_double(kernel, x, theta), q, sigma2=mf.SIGMA2)
    assert rankt == q and pivt[1] == 64 and margins[1:].min() >= 1e-9 * mf.SIGMA2
    xd, Vd = H.to_device(x), H.to_device(V)
    dim = _lib.loglik_dim(n, 1)
    KV, alpha = H.empty(dim, dim), H.empty(_lib.pad128(n), 1)
    assert H.loglik(_kid(kernel), xd, theta, Vd, H.zeros(n, 1), KV, alpha)[3] == 0      # the factor of K + V for the selection
    xcd, noise = H.to_device(np.random.default_rng(65).random((P, 2))), H.to_device(np.full(P, 0.05))
    work = H.empty(max(_lib.pchol_workspace_bytes(n, q), _lib.select_workspace_bytes(n, P, q)) // 8)

    def pchol():
        gbig, G = _framed(H, (q, n))
        pbig, piv = _framed(H, (q,), dtype=H.torch.int64)
        rank = H.pchol(_kid(kernel), xd, theta, q, G, piv, work=work)
        return (gbig, (q, n)), (pbig, (q,)), G, piv, rank

    def select(**kw):
        vbig, var = _framed(H, (P,))
        var.fill_(mf.SIGMA2)
        ibig, idx = _framed(H, (q,), dtype=H.torch.int64)
        kbig, pick = _framed(H, (q,))
        sbig, Gs = _framed(H, (q, P))
        H.select_batch(_kid(kernel), xd, theta, KV, xcd, var, q, idx, pick, G_out=Gs, work=work, **kw)
        return [(vbig, (P,)), (ibig, (q,)), (kbig, (q,)), (sbig, (q, P))], idx

    fg1, fp1, G1, piv1, rank1 = pchol()
    frames, idx_info = select(noise=noise, criterion=1, allow_repeats=True)
    more, idx_plain = select()                                           # 5 candidates, 8 steps, no repeats: `done` is set
    fg2, fp2, G2, piv2, rank2 = pchol()
    H.sync()
    assert idx_info.cpu().numpy().min() >= 0 and np.array_equal(idx_plain.cpu().numpy()[P:], np.full(q - P, -1))
    for big, shape in [fg1, fp1, fg2, fp2] + frames + more:
        assert _frame_untouched(big, shape)
    for G, piv, rank in ((G1, piv1, rank1), (G2, piv2, rank2)):
        assert rank == q and np.array_equal(piv.cpu().numpy(), pivt)
        assert np.max(np.abs(G.cpu().numpy() - Gt)) <= 1e-10 * mf.SIGMA2
    assert np.array_equal(piv2.cpu().numpy(), piv1.cpu().numpy()) and np.array_equal(G2.cpu().numpy(), G1.cpu().numpy())


# ---- 5. conjugate gradients ------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _dev(H, fx, rank=mf.RANK):
    """the fixture on the device with its rank-128 preconditioner, built once per module"""
    if (fx, rank) not in _DEV:
        f = mf.fixture(fx)
        n = len(f["x"])
        xd, Vd = H.to_device(np.array(f["x"])), H.to_device(np.array(f["V"]))
        G = piv = C = None
        if rank:
            gbig, G = _framed(H, (rank, n))
            piv = H.torch.empty(rank, dtype=H.torch.int64, device=G.device)
            assert H.pchol(_kid(f["kernel"]), xd, f["theta"], rank, G, piv) >= 64      # (an exhausted tail is zero rows)
            C = H.empty(128, 128)
            assert H.precond_factor(G, rank, n, Vd, C) == 0
            assert _frame_untouched(gbig, (rank, n))
        _DEV[(fx, rank)] = (xd, Vd, G, C)
    return _DEV[(fx, rank)]


def _solve(H, fx, B, rank=mf.RANK, warm=None, **kw):
    f = mf.fixture(fx)
    n, s = B.shape
    xd, Vd, G, C = _dev(H, fx, rank)
    xbig, X = _framed(H, (n, s))
    if warm is not None:
        X.copy_(H.to_device(warm))
    it, rr, st = H.pcg(_kid(f["kernel"]), xd, f["theta"], Vd, H.to_device(B), X, G=G, q=rank, C=C, warm=warm is not None,
                       **{"tol": TOL, **kw})
    assert _frame_untouched(xbig, (n, s))
    return X.cpu().numpy(), it, rr, st


def _dense_solve(H, fx, B):
    """(K + V)^-1 B by the dense device path: the fused evaluation's factor and potrs, eight columns at a time"""
    from fvgp_amd import _lib
    f = mf.fixture(fx)
    n = len(f["x"])
    dim, npad = _lib.loglik_dim(n, 1), _lib.pad128(n)
    KV, alpha = H.empty(dim, dim), H.empty(npad, 1)
    y = B[:, :1]
    info = H.loglik(_kid(f["kernel"]), H.to_device(np.array(f["x"])), f["theta"], H.to_device(np.array(f["V"])), H.to_device(y), KV, alpha)[3]
    assert info == 0
    out = np.empty_like(B)
    out[:, 0] = alpha.cpu().numpy()[:n, 0]
    for a in range(1, B.shape[1], 8):
        b = min(a + 8, B.shape[1])
        R = H.zeros(npad, 8)
        R[:n, :b - a] = H.to_device(B[:, a:b])
        H.potrs(KV, n, R, b - a)
        H.sync()
        out[:, a:b] = R.cpu().numpy()[:n, :b - a]
    return out


_SOLVED = {}


def _solved(H, fx, s):
    """the device's solve of the fixture's first s right-hand sides at tol = 1e-9, once per module"""
    if (fx, s) not in _SOLVED:
        _SOLVED[(fx, s)] = _solve(H, fx, mf.fixture(fx)["rhs"][:, :s].copy())
    return _SOLVED[(fx, s)]


def _own_relres(fx, B, X):
    """|b - (K + V) x| / |b| per column in longdouble, K from the longdouble reference"""
    f = mf.fixture(fx)
    A_ld = f["K_ld"] + np.diag(f["V"].astype(np.longdouble))
    R = B.astype(np.longdouble) - A_ld @ X.astype(np.longdouble)
    return np.asarray(np.sqrt((R * R).sum(axis=0)) / np.sqrt((B.astype(np.longdouble) ** 2).sum(axis=0)), dtype=np.float64)


@pytest.mark.parametrize("s", (1, 5, 16))
@pytest.mark.parametrize("fx", mf.ACCURACY_FIXTURES, ids=mf.fixture_id)
def test_pcg_solves_the_accuracy_fixtures(H, fx, s):
    """tol = 1e-9: every column status 0; the reported (true) residual and the test's own longdouble residual both <= tol; the solution
    within cond(A) tol of the dense device solve; iterations <= 2 x the twin's with the same preconditioner"""
    f = mf.fixture(fx)
    B = f["rhs"][:, :s].copy()
    X, it, rr, st = _solved(H, fx, s)
    assert np.all(st == 0), st
    assert np.all(rr <= TOL), rr
    assert np.all(_own_relres(fx, B, X) <= TOL)
    want = _dense_solve(H, fx, B)
    ev = np.linalg.eigvalsh(f["A"])
    cond = ev[-1] / ev[0]
    for c in range(s):
        assert np.linalg.norm(X[:, c] - want[:, c]) <= cond * TOL * np.linalg.norm(want[:, c]), c
        twin = mf.fixture_pcg(fx, c, mf.RANK, TOL)
        assert twin[3] == 0 and it[c] <= 2 * twin[1], (c, it[c], twin[1])
    print(fx, s, "iterations", it.tolist(), "twin", [mf.fixture_pcg(fx, c, mf.RANK, TOL)[1] for c in range(s)])


@pytest.mark.parametrize("s", (1, 5, 16))
@pytest.mark.parametrize("fx", mf.ACCURACY_FIXTURES, ids=mf.fixture_id)
def test_pcg_reported_residual_is_confirmed_in_longdouble(H, fx, s):
    """the reported relres agrees with the test's own longdouble residual to within 10 % of it, column by column.  (Attainable only above the
    rounding floor of a residual evaluated in double: the 2-iteration RBF fixture of the pivot tests ends at 4.3e-13 .. 5.9e-13 and the
    device reports 5.8e-13 .. 7.8e-13 there, 34 % .. 43 % apart -- tests/matrix_free_ref.py, ACCURACY_FIXTURES, says what takes its place;
    on the six other fixtures the largest difference observed was 0.4 % of the residual, at matern32_iso, d = 1.)"""
    B = mf.fixture(fx)["rhs"][:, :s].copy()
    X, it, rr, st = _solved(H, fx, s)
    own = _own_relres(fx, B, X)
    print(fx, s, "largest |own - reported| / own:", float(np.max(np.abs(own - rr) / own)), "own", own.tolist(), "reported", rr.tolist())
    assert np.all(np.abs(own - rr) <= 0.1 * own), (own, rr)


def test_pcg_jacobi_bits_and_edge_cases(H):
    fx = mf.FIXTURES[2]                                          # Matern-5/2, cond 5e5
    f = mf.fixture(fx)
    B = f["rhs"].copy()
    n = len(B)
    # rank 0 (Jacobi) converges too, within twice the twin's count
    X0, it0, rr0, st0 = _solve(H, fx, B[:, :2].copy(), rank=0)
    assert np.all(st0 == 0) and np.all(rr0 <= TOL)
    assert all(it0[c] <= 2 * mf.fixture_pcg(fx, c, 0, TOL)[1] for c in range(2))
    assert it0[0] >= 4 * mf.fixture_pcg(fx, 0, mf.RANK, TOL)[1]       # ... and shows what the preconditioner is worth
    # bits: a column alone against inside s = 16; the same call twice; other check_every
    X, it, rr, st = _solve(H, fx, B)
    X2, it2, rr2, st2 = _solve(H, fx, B)
    assert np.array_equal(X, X2) and np.array_equal(it, it2) and np.array_equal(rr, rr2)
    for c in (0, 9, 15):
        Xc, itc, rrc, stc = _solve(H, fx, B[:, c:c + 1].copy(), check_every=3)
        assert np.array_equal(Xc[:, 0], X[:, c]) and itc[0] == it[c] and rrc[0] == rr[c] and stc[0] == 0, c
    # a zero column: x = 0 after 0 iterations, its neighbours unchanged
    Bz = B[:, :3].copy()
    Bz[:, 1] = 0.0
    Xz, itz, rrz, stz = _solve(H, fx, Bz)
    assert np.all(Xz[:, 1] == 0.0) and itz[1] == 0 and rrz[1] == 0.0 and stz[1] == 0
    assert np.array_equal(Xz[:, 0], X[:, 0]) and np.array_equal(Xz[:, 2], X[:, 2])
    # a warm start from the converged X ends with 0 further iterations
    Xw, itw, rrw, stw = _solve(H, fx, B[:, :5].copy(), warm=X[:, :5].copy())
    assert np.all(itw == 0) and np.all(stw == 0) and np.all(rrw <= TOL) and np.array_equal(Xw, X[:, :5])
    # max_iter = 2: status 1, an honest residual above tol, return code 0 (no exception)
    Xm, itm, rrm, stm = _solve(H, fx, B[:, :3].copy(), max_iter=2)
    assert np.all(stm == 1) and np.all(itm == 2) and np.all(rrm > TOL)
    A_ld = f["K_ld"] + np.diag(f["V"].astype(np.longdouble))
    R = B[:, :3].astype(np.longdouble) - A_ld @ Xm.astype(np.longdouble)
    own = np.asarray(np.sqrt((R * R).sum(axis=0)) / np.sqrt((B[:, :3].astype(np.longdouble) ** 2).sum(axis=0)), dtype=np.float64)
    assert np.all(np.abs(own - rrm) <= 1e-6 * own)
    assert n == 1000


def test_refused_arguments(H):
    """one case per documented code; nothing is launched and no buffer is touched"""
    from fvgp_amd import _lib
    L = _lib.lib()
    fx = mf.FIXTURES[0]
    f = mf.fixture(fx)
    n, d = f["x"].shape
    xd, Vd, G, C = _dev(H, fx)
    th = np.ascontiguousarray(f["theta"])
    tp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    bbig, B = _framed(H, (n, 4))
    ybig, Y = _framed(H, (n, 4))
    work = H.empty(max(_lib.pcg_workspace_bytes(n, mf.RANK), _lib.pchol_workspace_bytes(n, mf.RANK),
                       _lib.precond_workspace_bytes(n, mf.RANK)) // 8)
    wb = work.numel() * 8
    h = H._h

    def mv(**kw):
        a = dict(h=h, kid=0, x1=P(xd), n1=n, x2=P(xd), n2=n, d=d, th=tp, nt=len(th), v=P(Vd), B=P(B), ldb=B.stride(0), s=4, Y=P(Y),
                 ldy=Y.stride(0), w=P(work), wb=wb)
        a.update(kw)
        return L.fvgp_hip_kmatvec(*a.values())
    assert mv() == 0
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=77)), (-3, dict(x1=None)), (-4, dict(n1=0)), (-5, dict(x2=None)), (-6, dict(n2=0)),
                     (-7, dict(d=17)), (-8, dict(th=None)), (-9, dict(nt=1)), (-10, dict(n1=n - 1)), (-11, dict(B=None)), (-12, dict(ldb=3)),
                     (-13, dict(s=0)), (-14, dict(Y=None)), (-15, dict(ldy=3)), (-16, dict(w=ctypes.c_void_p(work.data_ptr() + 4))),
                     (-17, dict(wb=-8))):
        assert mv(**kw) == code, (code, kw)
    H.set_option("matvec_split", 2)
    try:
        assert mv(x1=P(xd), n1=n, n2=n, v=None, wb=8, s=4) == (-17 if n > CHUNK else 0)
        x2big = H.to_device(np.random.default_rng(0).random((CHUNK + 5, d)))
        Bbig = H.zeros(CHUNK + 5, 4)
        assert mv(x2=P(x2big), n2=CHUNK + 5, v=None, B=P(Bbig), ldb=4, wb=8) == -17      # a forced split without its workspace
    finally:
        H.set_option("matvec_split", 0)
    with pytest.raises(_lib.HipExtensionError):
        H.set_option("matvec_split", -1)

    rank = ctypes.c_int(-5)
    pbig, piv = _framed(H, (8,), dtype=H.torch.int64)
    gbig, Gs = _framed(H, (8, n))

    def pc(**kw):
        a = dict(h=h, kid=0, x=P(xd), n=n, d=d, th=tp, nt=len(th), q=8, tol=0.0, G=P(Gs), ldg=Gs.stride(0), piv=P(piv), dres=None,
                 w=P(work), wb=wb, rank=ctypes.byref(rank))
        a.update(kw)
        return L.fvgp_hip_pchol(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=-1)), (-3, dict(x=None)), (-4, dict(n=0)), (-5, dict(d=0)), (-6, dict(th=None)),
                     (-7, dict(nt=2)), (-8, dict(q=0)), (-9, dict(tol=-1.0)), (-9, dict(tol=float("nan"))), (-10, dict(G=None)),
                     (-11, dict(ldg=n - 1)), (-12, dict(piv=None)), (-14, dict(w=None)), (-15, dict(wb=64)), (-16, dict(rank=None))):
        assert pc(**kw) == code, (code, kw)
    assert rank.value == -5 and _frame_untouched(pbig, (8,)) and _frame_untouched(gbig, (8, n))
    assert np.all(Gs.cpu().numpy() == CANARY)

    info = ctypes.c_int(-5)
    C2 = H.empty(128, 128)

    def pf(**kw):
        a = dict(h=h, G=P(G), ldg=G.stride(0), q=mf.RANK, n=n, v=P(Vd), C=P(C2), ldc=128, w=P(work), wb=wb, info=ctypes.byref(info))
        a.update(kw)
        return L.fvgp_hip_precond_factor(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(G=None)), (-3, dict(ldg=n - 1)), (-4, dict(q=0)), (-4, dict(q=_lib.PCG_MAX_RANK + 1)),
                     (-5, dict(n=0)), (-6, dict(v=None)), (-7, dict(C=None)), (-8, dict(ldc=127)), (-8, dict(q=129, ldc=128)),
                     (-9, dict(w=None)), (-10, dict(wb=8)), (-11, dict(info=None))):
        assert pf(**kw) == code, (code, kw)
    assert info.value == -5

    it = (ctypes.c_int * 16)()
    st = (ctypes.c_int * 16)()
    rr = (ctypes.c_double * 16)()
    xbig, X = _framed(H, (n, 4))

    def cg(**kw):
        a = dict(h=h, kid=0, x=P(xd), n=n, d=d, th=tp, nt=len(th), v=P(Vd), G=P(G), ldg=G.stride(0), q=mf.RANK, C=P(C), ldc=C.stride(0),
                 B=P(B), ldb=B.stride(0), s=4, X=P(X), ldx=X.stride(0), warm=0, tol=1e-9, max_iter=10, check_every=8, max_restarts=3,
                 w=P(work), wb=wb, it=it, rr=rr, st=st)
        a.update(kw)
        return L.fvgp_hip_pcg(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=6)), (-3, dict(x=None)), (-4, dict(n=0)), (-5, dict(d=17)), (-6, dict(th=None)),
                     (-7, dict(nt=1)), (-8, dict(v=None)), (-10, dict(ldg=n - 1)), (-11, dict(q=-1)), (-11, dict(q=_lib.PCG_MAX_RANK + 1)),
                     (-12, dict(C=None)), (-13, dict(ldc=127)), (-14, dict(B=None)), (-15, dict(ldb=3)), (-16, dict(s=0)),
                     (-16, dict(s=17, ldb=17, ldx=17)), (-17, dict(X=None)), (-18, dict(ldx=3)), (-20, dict(tol=0.0)), (-21, dict(max_iter=0)),
                     (-22, dict(check_every=0)), (-23, dict(max_restarts=-1)), (-24, dict(w=None)), (-25, dict(wb=64)), (-26, dict(it=None)),
                     (-27, dict(rr=None)), (-28, dict(st=None))):
        assert cg(**kw) == code, (code, kw)
    H.sync()
    assert _frame_untouched(xbig, (n, 4)) and np.all(X.cpu().numpy() == CANARY)


# ---- 6. the facade against the dense GP --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade():
    import fvgp_amd
    rng = np.random.default_rng(606)
    n, d, P = 1500, 2, 37
    x = rng.random((n + 50, d))
    y = np.sin(3.0 * x.sum(axis=1)) + 0.05 * rng.standard_normal(n + 50)
    V = 1e-2 * (1.0 + rng.random(n + 50))
    theta = np.array([1.3, 0.3, 0.45])
    xp = rng.random((P, d))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x[:n], y[:n], init_hyperparameters=theta, noise_variances=V[:n], kernel_function="matern52_ard")
        gp_all = fvgp_amd.GP(x, y, init_hyperparameters=theta, noise_variances=V, kernel_function="matern52_ard")
    return {"gp": gp, "gp_all": gp_all, "x": x, "y": y, "V": V, "theta": theta, "xp": xp, "n": n, "tol": 1e-10}


def _bounds(fc, x, y, V, xp):
    """tol |k*| |y - m| / min V + 1e-8 relative for the mean, tol |k*|^2 / min V + 1e-10 sigma^2 for variances and covariances: both from
    |delta z| <= |r| / lambda_min and lambda_min >= min V"""
    ks = np.asarray(kf.k_ref("matern52_ard", xp, x, fc["theta"]), dtype=np.float64)
    kn = np.linalg.norm(ks, axis=1)
    return fc["tol"] * kn * np.linalg.norm(y - y.mean()) / V.min(), fc["tol"] * kn.max() ** 2 / V.min() + 1e-10 * fc["theta"][0]


def test_facade_matches_the_dense_gp(facade):
    import fvgp_amd
    fc = facade
    n, xp, gp = fc["n"], fc["xp"], fc["gp"]
    mfgp = gp.matrix_free()
    assert isinstance(mfgp, fvgp_amd.MatrixFreeGP) and mfgp._native.name == "matern52_ard"
    assert np.array_equal(mfgp.hyperparameters, gp.hyperparameters) and mfgp.point_number == n
    bm, bv = _bounds(fc, fc["x"][:n], fc["y"][:n], fc["V"][:n], xp)
    want = gp.posterior_mean(xp)["m(x)"]
    got = mfgp.posterior_mean(xp)
    assert got["converged"] and np.all(np.abs(got["m(x)"] - want) <= bm + 1e-8 * np.abs(want))
    cw = gp.posterior_covariance(xp)
    cg = mfgp.posterior_covariance(xp)                           # 37 points: blocks of 16 + 16 + 5
    assert np.max(np.abs(cg["v(x)"] - cw["v(x)"])) <= bv and np.max(np.abs(cg["S"] - cw["S"])) <= bv
    assert np.array_equal(cg["S"], cg["S"].T)
    vo = mfgp.posterior_covariance(xp, variance_only=True)
    assert vo["S"] is None and np.max(np.abs(vo["v(x)"] - cw["v(x)"])) <= bv
    an = mfgp.posterior_covariance(xp, variance_only=True, add_noise=True)
    aw = gp.posterior_covariance(xp, variance_only=True, add_noise=True)
    assert np.max(np.abs(an["v(x)"] - aw["v(x)"])) <= bv and np.all(an["v(x)"] > vo["v(x)"])
    # a point's variance has the same bits in a call of 1 and of 37 points
    for p in (0, 20, 36):
        one = mfgp.posterior_covariance(xp[p:p + 1], variance_only=True)["v(x)"]
        assert one[0] == vo["v(x)"][p] and mfgp.posterior_covariance(xp[p:p + 1])["v(x)"][0] == cg["v(x)"][p]
    # solve() leaves the prediction state alone
    alpha = mfgp._alpha.clone()
    out = mfgp.solve(np.ones(n))
    assert out["converged"] and out["x"].shape == (n,) and out["relative_residual"][0] <= fc["tol"]
    assert mfgp._alpha is not None and bool((mfgp._alpha == alpha).all())
    assert mfgp.solve(np.ones((n, 18)))["x"].shape == (n, 18)         # more than 16 columns go in blocks


def test_facade_update_warm_starts(facade):
    import fvgp_amd
    fc = facade
    n, xp = fc["n"], fc["xp"]
    x, y, V = fc["x"], fc["y"], fc["V"]
    mfgp = fc["gp"].matrix_free()
    mfgp.posterior_mean(xp)
    mfgp.update_gp_data(x[n:], y[n:], noise_variances_new=V[n:])
    warm_iters = mfgp._alpha_info["iterations"]
    fresh = fvgp_amd.MatrixFreeGP(x, y, fc["theta"], noise_variances=V, kernel_function="matern52_ard")
    bm, bv = _bounds(fc, x, y, V, xp)
    a, b = mfgp.posterior_mean(xp), fresh.posterior_mean(xp)
    want = fc["gp_all"].posterior_mean(xp)["m(x)"]
    assert np.all(np.abs(a["m(x)"] - want) <= bm + 1e-8 * np.abs(want)) and np.all(np.abs(b["m(x)"] - want) <= bm + 1e-8 * np.abs(want))
    va, vw = mfgp.posterior_covariance(xp, variance_only=True)["v(x)"], fc["gp_all"].posterior_covariance(xp, variance_only=True)["v(x)"]
    assert np.max(np.abs(va - vw)) <= bv
    print("alpha iterations: warm", warm_iters, "cold", b["iterations"])
    assert a["converged"] and b["converged"] and warm_iters <= b["iterations"]
    # more data than the GP holds, straight from the dense object
    big = fc["gp"].matrix_free(x, y, V)
    assert big.point_number == n + 50 and np.array_equal(big.posterior_mean(xp)["m(x)"], b["m(x)"])
    # new hyperparameters drop alpha and the preconditioner
    big.set_hyperparameters(fc["theta"] * 1.1)
    assert big._alpha is None and big._G is None


def test_facade_warns_and_refuses(facade):
    import fvgp_amd
    fc = facade
    n, xp = fc["n"], fc["xp"]
    x, y, V = fc["x"][:n], fc["y"][:n], fc["V"][:n]
    slow = fvgp_amd.MatrixFreeGP(x, y, fc["theta"], noise_variances=V, kernel_function="matern52_ard", args={"max_iter": 2, "tol": 1e-10})
    with pytest.warns(UserWarning, match="did not converge: relative residual"):
        out = slow.solve(y)
    assert out["converged"] is False and out["relative_residual"][0] > 1e-10
    with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
        fvgp_amd.MatrixFreeGP(x, y, fc["theta"], noise_variances=V, kernel_function=lambda a, b, h: np.zeros((len(a), len(b))))
    mfgp = fc["gp"].matrix_free(args={"z_max_bytes": 2 * n * 16 * 8})
    with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
        mfgp.posterior_mean(xp, x_out=np.zeros((2, 1)))
    for call in (mfgp.log_likelihood, mfgp.neg_log_likelihood_gradient, mfgp.train):
        with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
            call()
    with pytest.raises(MemoryError, match="smaller batches"):
        mfgp.posterior_covariance(xp)                            # 37 points against a budget of 16
    assert mfgp.posterior_covariance(xp[:16], variance_only=True)["v(x)"].shape == (16,)
    with pytest.warns(UserWarning, match="No noise function or measurement noise"):
        fvgp_amd.MatrixFreeGP(x, y, fc["theta"], kernel_function="matern52_ard")
