"""The nearest-neighbour preconditioner on the device (include/fvgp_hip_nn.h: fvgp_hip_nn_factor, fvgp_hip_nn_precond_apply,
fvgp_hip_pcg_nn; MatrixFreeGP(args={"preconditioner": "vecchia"}), VecchiaGP.matrix_free) against the numpy twin
nn_precond_ref:
    1. the factor over vecchia_ref.ACC_CASES and a list with gaps: longdouble under MARGIN * max(base, FLOOR), the bits of the conditionals
       entry's variance, a row alone against the row inside the call
    2. the apply: n in {1, 257, 4097} x m in {1, 17, 64} x s in {1, 5, 16} and the coincident-point set, a componentwise bound, the bit
       contracts, positions outside the factor
    3. the solver on the fixtures whose iteration counts motivated it
    4. refused arguments: one case per documented code of each new entry
    5. the facade against the dense GP
Run with -s for the record lines  NP|..."""
import ctypes
import warnings

import numpy as np
import pytest

import kernel_family_ref as kf
import matrix_free_ref as mf
import nn_precond_ref as npr
import vecchia_family_ref as fam
import vecchia_ref as vr
from vecchia_device import CANARY, _frame_untouched, _framed, _kid, _same

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = kf.EPS
TOL = 1e-9
ICANARY = -7777


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _int_tensor(H, a, dtype=None):
    return H.torch.as_tensor(np.array(a), dtype=dtype, device=f"cuda:{H.device}")      # (a copy: the shared fixtures are read-only)


# ---- 1. the factor ---------------------------------------------------------------------------------------------------------------------------
def _factor(H, name, x, theta, idx, m, v, pad=0):
    """Handle.nn_factor into canary-framed coef (n, m + pad) and dinv, the lists a view of leading dimension m + pad inside an int32
    canary buffer: (coef (n, m), dinv, info, the NNFactor); the frames and the columns past m are checked here"""
    n = len(x)
    big_i = H.torch.full((n + 2, m + pad), ICANARY, dtype=H.torch.int32, device=f"cuda:{H.device}")
    big_i[1:1 + n, :m] = _int_tensor(H, idx[:, :m], H.torch.int32)
    view = big_i[1:1 + n]
    big_c, coef = _framed(H, n, m + pad)
    big_d, dinv = _framed(H, n)
    before = big_i.cpu().numpy().copy()
    W, info = H.nn_factor(_kid(name), H.to_device(x), theta, view, m, H.to_device(v), coef=coef, dinv=dinv)
    assert _frame_untouched(big_c) and _frame_untouched(big_d) and np.array_equal(big_i.cpu().numpy(), before)
    c = coef.cpu().numpy()
    assert np.all(c[:, m:] == CANARY), "columns m .. ld of coef are not written"
    assert not np.any(c[:, :m] == CANARY) and not np.any(dinv.cpu().numpy() == CANARY)
    return c[:, :m].copy(), dinv.cpu().numpy(), info, W


def _conditional_variance(H, name, x, theta, idx, m, v):
    """var of the conditionals entry on the same inputs with s = v (the data values are zeros: var does not read them)"""
    n = len(x)
    xd, vd = H.to_device(x), H.to_device(v)
    mu, var = H.empty(1, n), H.empty(1, n)
    info = H.nn_conditionals(_kid(name), xd, xd, theta, _int_tensor(H, idx, H.torch.int32), m, H.zeros(n), vd, mu, var, s=vd)
    return var.cpu().numpy()[0], info


def _check_factor(H, label, name, x, theta, v, idx, m, ref, bars, pad=0):
    n = len(x)
    coef, dinv, info, _ = _factor(H, name, x, theta, idx, m, v, pad)
    assert info == 0
    figs = npr.factor_figures((coef, dinv), ref, ref[2])
    print(f"\nNP|factor|{label}|" + " ".join(f"{k}={figs[k]:.2e}/{bars[k]:.2e}" for k in bars))
    for k in bars:
        assert figs[k] <= bars[k], (k, figs[k], bars[k])
    valid = (idx >= 0) & (idx < n)
    assert np.all(coef[~valid] == 0.0) and not np.any(np.signbit(coef[~valid])), "+0.0 at skipped entries"
    # d_i has the bits of the conditionals entry's var: dinv is the correctly rounded 1 / sqrt of it (numpy's sqrt and division round
    # correctly, as the device's do), and squaring it back lands within the two roundings' reach of var
    var, vinfo = _conditional_variance(H, name, x, theta, idx, m, v)
    assert vinfo == 0 and np.array_equal(dinv, 1.0 / np.sqrt(var))
    assert np.all(np.abs(1.0 / (dinv * dinv) - var) <= 4 * EPS * var)
    # a row alone: its listed rows and itself are the whole data set, the list keeps its shape
    for i in sorted({0, n // 2, n - 1}):
        at = np.flatnonzero(valid[i])
        rows = np.concatenate([idx[i, at], [i]]).astype(np.int64)
        sub = np.full((len(rows), m), -1, dtype=np.int32)
        sub[-1, at] = np.arange(len(at))
        c1, d1, info1, _ = _factor(H, name, x[rows], theta, sub, m, v[rows])
        assert info1 == 0 and _same(c1[-1], coef[i]) and d1[-1] == dinv[i], i
    return coef, dinv


@pytest.mark.parametrize("case", vr.ACC_CASES, ids=vr.case_id)
def test_factor_against_longdouble(H, case):
    """coef and dinv within MARGIN = 8 times the larger of the float64 twin's and the perturbed twin's error (floors: vecchia_ref's), at
    B = 1: the first theta of the case"""
    name, d, n, m, _ = case
    x, theta, v, idx = npr.factor_inputs(case)
    _check_factor(H, vr.case_id(case), name, x, theta, v, idx, m, npr.factor_reference(case), npr.factor_bars(case))


def test_factor_on_a_list_with_gaps(H):
    """the neighbours of a compact case scattered over 64 columns with every sort of junk between them, idx and coef with an odd leading
    dimension: within the compact case's bars of the longdouble factor of the same list"""
    gap = fam.GAP_CASES[4]
    case, m = gap
    name = case[0]
    x, theta, v, _ = npr.factor_inputs(case)
    idx = fam.gapped_list(gap)
    assert m == 64 and np.any(idx >= len(x)) and np.any(idx < 0)
    coef, dinv = npr.factor_ref(kf.k_ref(name, x, x, theta, LD), v, idx, LD)
    _check_factor(H, fam.gap_id(gap), name, x, theta, v, idx, m, (coef, dinv, 1 / (dinv * dinv)), npr.factor_bars(case), pad=3)


def test_factor_failed_pivot_gives_a_nan_row_and_info(H):
    """a row that lists two coincident points without noise, sigma^2 = 1 (the block is [[1, 1], [1, 1]] and every operation exact: the
    second pivot is 0): NaN in that row alone, info names it; the rows around it are untouched by it"""
    rng = np.random.default_rng(9)
    n, m = 12, 16
    x = rng.random((n, 2))
    x[7] = x[3]
    v = np.full(n, 1e-2)
    v[[3, 7]] = 0.0
    theta = np.array([1.0, 0.4, 0.5])
    idx = vr.search_ref(x, x, m, None, c0=0)
    clean = np.where(np.isin(idx, (3, 7)), -1, idx)               # (no other row meets the two copies)
    bad = clean.copy()
    bad[8] = -1
    bad[8, [2, 5]] = (3, 7)
    coef, dinv, info, _ = _factor(H, "matern32_ard", x, theta, bad, m, v)
    assert info == 1 + 8 and np.isnan(dinv[8]) and np.all(np.isnan(coef[8]))
    c0, d0, info0, _ = _factor(H, "matern32_ard", x, theta, clean, m, v)
    ok = np.arange(n) != 8
    assert info0 == 0 and np.all(np.isfinite(d0)) and _same(coef[ok], c0[ok]) and _same(dinv[ok], d0[ok])


# ---- 2. the apply ------------------------------------------------------------------------------------------------------------------------------
def _synthetic_factor(n, m, seed):
    """lists of random earlier rows with junk between them -- and, from m = 2 on, row 0 in every later row's first column: a bucket of
    n - 1 entries -- with random coefficients over five binades"""
    rng = np.random.default_rng(seed)
    idx = npr.junk_lists(n, m, seed)
    if m > 1 and n > 1:
        idx[1:, 0] = 0
    coef = rng.standard_normal((n, m)) * np.exp2(rng.integers(-2, 3, size=(n, m)).astype(np.float64))
    coef[(idx < 0) | (idx >= n)] = 0.0
    return idx, coef, 0.5 + rng.random(n)


def _upload_factor(H, idx, coef, dinv, lists=None, pad=0):
    """an NNFactor of the host arrays with a leading dimension of m + pad; lists = (tr_start, tr_pos, nnz) on the host or None: the
    binding's own"""
    from fvgp_amd import _lib
    n, m = idx.shape
    t = H.torch
    idx_d = t.full((n, m + pad), ICANARY, dtype=t.int32, device=f"cuda:{H.device}")
    idx_d[:, :m] = _int_tensor(H, idx, t.int32)
    coef_d = H.torch.full((n, m + pad), CANARY, dtype=t.float64, device=idx_d.device)
    coef_d[:, :m] = H.to_device(coef)
    if lists is None:
        start, pos, nnz = H.nn_transpose(idx_d, m)
    else:
        start, pos, nnz = _int_tensor(H, lists[0], t.int64), _int_tensor(H, np.concatenate([lists[1], [0]]), t.int64), lists[2]
    return _lib.NNFactor(idx_d, m, coef_d, H.to_device(dinv), start, pos, nnz)


def _apply(H, W, R, s):
    n = R.shape[0]
    big, Z = _framed(H, n, 16)
    H.nn_precond_apply(W, H.to_device(R), Z, s=s)
    H.sync()
    assert _frame_untouched(big)
    z = Z.cpu().numpy()
    assert np.all(z[:, s:] == CANARY), "columns past s are not written"
    return z[:, :s].copy()


def _check_apply(H, label, idx, coef, dinv, seed, pad=0):
    n, m = idx.shape
    R = np.random.default_rng(seed).standard_normal((n, 16)) * np.exp2(np.random.default_rng(seed + 1).integers(-8, 9, size=(n, 1)).astype(np.float64))
    W = _upload_factor(H, idx, coef, dinv, pad=pad)
    ld = m + pad
    start, pos = npr.transpose_ref(idx, n, ld)
    assert np.array_equal(W.tr_start.cpu().numpy(), start) and np.array_equal(W.tr_pos.cpu().numpy()[:W.nnz], pos) and W.nnz == len(pos)
    Z16 = _apply(H, W, R, 16)
    want, mag, indeg = npr.apply_ref(idx, coef, dinv, R)
    bound = npr.apply_bound(m, indeg, mag)
    err = np.abs(Z16.astype(LD) - want)
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    print(f"\nNP|apply|{label}|n={n} m={m} max in-degree={int(indeg.max())} worst error/bound={worst:.3f}")
    assert np.all(err <= bound)
    # bits: the same call twice; fewer columns; a column alone
    assert np.array_equal(_apply(H, W, R, 16), Z16)
    for s in (1, 5):
        assert np.array_equal(_apply(H, W, R[:, :s].copy(), s), Z16[:, :s]), s
    assert np.array_equal(_apply(H, W, R[:, 9:10].copy(), 1)[:, 0], Z16[:, 9])
    return W, R, Z16, (start, pos)


@pytest.mark.parametrize("m", (1, 17, 64))
@pytest.mark.parametrize("n", (1, 257, 4097))
def test_apply_against_longdouble_and_its_bit_contracts(H, n, m):
    """Z = W^T (W R) within gamma(m + in-degree + 2) of |W^T| (|W| |R|), componentwise; s = 1, 5, 16 and a column alone give the same
    bits; positions outside the factor and whatever lies past tr_start[n] are never read"""
    idx, coef, dinv = _synthetic_factor(n, m, 100 * n + m)
    W, R, Z16, (start, pos) = _check_apply(H, f"n{n}-m{m}", idx, coef, dinv, seed=n + m, pad=3 if m % 2 == 0 else 0)
    ld = W.idx.stride(0)
    # planted: positions at and past n ld and a negative one inside every third bucket, garbage behind the lists' end
    s2, p2 = [0], []
    for j in range(n):
        b = pos[start[j]:start[j + 1]].tolist()
        if j % 3 == 0:
            b = [-3] + b[:len(b) // 2] + [n * ld, n * ld + 5 + j, 2 ** 62] + b[len(b) // 2:]
        p2 += b
        s2.append(len(p2))
    if len(p2) + 4 <= n * ld:
        garbage = [2 ** 40, -1, 0, n * ld - 1]
        W2 = _upload_factor(H, idx, coef, dinv, lists=(np.array(s2), np.array(p2 + garbage, dtype=np.int64), len(p2) + len(garbage)), pad=ld - m)
        assert np.array_equal(_apply(H, W2, R, 16), Z16), "skipped, not read"


def test_apply_on_coincident_points(H):
    """40 coincident points first in the order, m = 64: the nearest-neighbour lists themselves send one bucket past a workgroup's 256 rows"""
    x = npr.coincident_set(n=1000)
    idx = vr.search_ref(x, x, 64, None, c0=0)
    rng = np.random.default_rng(77)
    coef = np.where(idx >= 0, rng.standard_normal(idx.shape), 0.0)
    _, _, _, (start, _) = _check_apply(H, "coincident", idx, coef, 0.5 + rng.random(len(x)), seed=78)
    assert np.max(np.diff(start)) > 256


# ---- 3. the solver ---------------------------------------------------------------------------------------------------------------------------
SOLVER_FIXTURES = npr.BIG_FIXTURES + (mf.ACCURACY_FIXTURES[1],)
_DEV = {}


def _dev(H, fx):
    """the ordered fixture on the device with its m = 32 factor (the device's own), once per module"""
    if fx not in _DEV:
        o = npr.ordered_fixture(fx)
        xd, Vd = H.to_device(np.array(o["x"])), H.to_device(np.array(o["V"]))
        W, info = H.nn_factor(_kid(o["kernel"]), xd, o["theta"], _int_tensor(H, o["idx"], H.torch.int32), npr.NEIGHBORS, Vd)
        assert info == 0
        _DEV[fx] = (xd, Vd, W)
    return _DEV[fx]


def _solve(H, fx, B, warm=None, **kw):
    o = npr.ordered_fixture(fx)
    n, s = B.shape
    xd, Vd, W = _dev(H, fx)
    xbig, X = _framed(H, n, s)
    if warm is not None:
        X.copy_(H.to_device(warm))
    it, rr, st = H.pcg_nn(_kid(o["kernel"]), xd, o["theta"], Vd, H.to_device(B), X, W, warm=warm is not None, **{"tol": TOL, **kw})
    assert _frame_untouched(xbig)
    return X.cpu().numpy(), it, rr, st


def _dense_solve(H, fx, B):
    """(K + V)^-1 B of the ordered fixture by the dense device path: the fused evaluation's factor and potrs, eight columns at a time"""
    from fvgp_amd import _lib
    o = npr.ordered_fixture(fx)
    n = len(o["x"])
    dim, npad = _lib.loglik_dim(n, 1), _lib.pad128(n)
    KV, alpha = H.empty(dim, dim), H.empty(npad, 1)
    info = H.loglik(_kid(o["kernel"]), H.to_device(np.array(o["x"])), o["theta"], H.to_device(np.array(o["V"])), H.to_device(B[:, :1]), KV, alpha)[3]
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


def _own_relres(fx, B, X):
    """|b - (K + V) x| / |b| per column in longdouble, K from the longdouble reference in the ordering"""
    o, f = npr.ordered_fixture(fx), mf.fixture(fx)
    A_ld = f["K_ld"][np.ix_(o["perm"], o["perm"])] + np.diag(o["V"].astype(LD))
    R = B.astype(LD) - A_ld @ X.astype(LD)
    return np.asarray(np.sqrt((R * R).sum(axis=0)) / np.sqrt((B.astype(LD) ** 2).sum(axis=0)), dtype=np.float64)


@pytest.mark.parametrize("fx", SOLVER_FIXTURES, ids=mf.fixture_id)
def test_pcg_nn_solves_the_fixtures(H, fx):
    """tol = 1e-9, s = 16: every column status 0; the reported residual and the test's own longdouble residual <= tol; the solution within
    cond(A) tol of the dense device solve; iterations <= 2 x the twin's with the same factor; a column alone has the bits it has inside
    s = 16"""
    o = npr.ordered_fixture(fx)
    B = np.array(o["rhs"])
    X, it, rr, st = _solve(H, fx, B)
    assert np.all(st == 0), st
    assert np.all(rr <= TOL), rr
    assert np.all(_own_relres(fx, B, X) <= TOL)
    want = _dense_solve(H, fx, B)
    ev = np.linalg.eigvalsh(o["A"])
    cond = ev[-1] / ev[0]
    twins = [npr.fixture_pcg_nn(fx, c, TOL) for c in range(16)]
    for c in range(16):
        assert np.linalg.norm(X[:, c] - want[:, c]) <= cond * TOL * np.linalg.norm(want[:, c]), c
        assert twins[c][3] == 0 and it[c] <= 2 * twins[c][1], (c, it[c], twins[c][1])
    print(f"\nNP|solver|{mf.fixture_id(fx)}|iterations {it.tolist()} twin {[t[1] for t in twins]}")
    for c in (0, 9):
        Xc, itc, rrc, stc = _solve(H, fx, B[:, c:c + 1].copy(), check_every=3)
        assert np.array_equal(Xc[:, 0], X[:, c]) and itc[0] == it[c] and rrc[0] == rr[c] and stc[0] == 0, c
    X2, it2, rr2, _ = _solve(H, fx, B)
    assert np.array_equal(X, X2) and np.array_equal(it, it2) and np.array_equal(rr, rr2)


def test_pcg_nn_against_the_device_rank_128_run(H):
    """the first 2000-point fixture, column 0: at most a quarter of the iterations the device's own rank-128 solve takes"""
    fx = npr.BIG_FIXTURES[0]
    o = npr.ordered_fixture(fx)
    n = len(o["x"])
    xd, Vd, _ = _dev(H, fx)
    B = np.array(o["rhs"][:, :1])
    _, it, _, st = _solve(H, fx, B)
    G = H.empty(mf.RANK, n)
    piv = H.torch.empty(mf.RANK, dtype=H.torch.int64, device=G.device)
    assert H.pchol(_kid(o["kernel"]), xd, o["theta"], mf.RANK, G, piv) == mf.RANK
    C = H.empty(128, 128)
    assert H.precond_factor(G, mf.RANK, n, Vd, C) == 0
    X = H.empty(n, 1)
    it_low, rr_low, st_low = H.pcg(_kid(o["kernel"]), xd, o["theta"], Vd, H.to_device(B), X, G=G, q=mf.RANK, C=C, tol=TOL)
    print(f"\nNP|solver|{mf.fixture_id(fx)}|device iterations: rank {mf.RANK} = {int(it_low[0])}, nearest-neighbour m = {npr.NEIGHBORS}: {int(it[0])}")
    assert st[0] == 0 and st_low[0] == 0 and 4 * it[0] <= it_low[0]


def test_pcg_nn_edge_cases(H):
    fx = mf.ACCURACY_FIXTURES[1]
    o = npr.ordered_fixture(fx)
    B = np.array(o["rhs"])
    X, it, rr, st = _solve(H, fx, B)
    # a zero column: x = 0 after 0 iterations, its neighbours unchanged
    Bz = B[:, :3].copy()
    Bz[:, 1] = 0.0
    Xz, itz, rrz, stz = _solve(H, fx, Bz)
    assert np.all(Xz[:, 1] == 0.0) and itz[1] == 0 and rrz[1] == 0.0 and stz[1] == 0
    assert np.array_equal(Xz[:, 0], X[:, 0]) and np.array_equal(Xz[:, 2], X[:, 2])
    # a warm start from the converged X ends with 0 further iterations
    Xw, itw, rrw, stw = _solve(H, fx, B[:, :5].copy(), warm=X[:, :5].copy())
    assert np.all(itw == 0) and np.all(stw == 0) and np.all(rrw <= TOL) and np.array_equal(Xw, X[:, :5])
    # max_iter = 2: status 1 and an honest residual above tol
    Xm, itm, rrm, stm = _solve(H, fx, B[:, :3].copy(), max_iter=2)
    assert np.all(stm == 1) and np.all(itm == 2) and np.all(rrm > TOL)
    own = _own_relres(fx, B[:, :3], Xm)
    assert np.all(np.abs(own - rrm) <= 1e-6 * own)


# ---- 4. refused arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(H):
    """one case per documented code of fvgp_hip_nn_factor, fvgp_hip_nn_precond_apply and fvgp_hip_pcg_nn; nothing is launched: every
    output keeps its canary"""
    from fvgp_amd import _lib
    L = _lib.lib()
    t = H.torch
    n, d, m, ld, s = 50, 2, 4, 5, 3
    dev = f"cuda:{H.device}"
    x, v = H.to_device(np.random.default_rng(0).random((n, d))), H.to_device(np.full(n, 0.01))
    idx = t.full((n, ld), -1, dtype=t.int32, device=dev)
    theta = np.array([1.0, 0.3, 0.3])
    tp = theta.ctypes.data_as(_lib.P_d)
    outs = {k: t.full(shape, CANARY, dtype=t.float64, device=dev) for k, shape in
            (("coef", (n, ld)), ("dinv", (n,)), ("Z", (n, s)), ("X", (n, s)))}
    R = H.to_device(np.random.default_rng(1).standard_normal((n, s)))
    start, pos = t.zeros(n + 1, dtype=t.int64, device=dev), t.zeros(1, dtype=t.int64, device=dev)
    wf = H.empty(max(2, _lib.nn_factor_workspace_bytes(n) // 8))
    wa = H.empty(max(2, _lib.nn_precond_apply_workspace_bytes(n) // 8))
    wp = H.empty(max(2, _lib.pcg_nn_workspace_bytes(n) // 8))
    info = ctypes.c_int64(0)
    iters, status, relres = (ctypes.c_int * 16)(), (ctypes.c_int * 16)(), (ctypes.c_double * 16)()
    p = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    bad = lambda a: ctypes.c_void_p(a.data_ptr() + 4)      # noqa: E731

    def run(fn, base, cases):
        keys = list(base)
        assert fn(*base.values()) == 0, (fn.__name__, "the base call is legal")
        H.sync()
        for o in outs.values():
            o.fill_(CANARY)
        H.sync()
        seen = []
        for code, key, value in cases:
            a = dict(base)
            assert key in keys
            a[key] = value
            assert fn(*a.values()) == code, (fn.__name__, code, key)
            seen.append(code)
        H.sync()
        assert all(bool((o == CANARY).all()) for o in outs.values()), "nothing was launched"
        return seen

    factor = {"h": H._h, "kid": 1, "x": p(x), "n": n, "d": d, "theta": tp, "ntheta": 3, "idx": p(idx), "ld": ld, "m": m, "v": p(v),
              "coef": p(outs["coef"]), "ldc": ld, "dinv": p(outs["dinv"]), "work": p(wf), "wb": wf.numel() * 8, "info": ctypes.byref(info)}
    seen = run(L.fvgp_hip_nn_factor, factor, [
        (-1, "h", None), (-2, "kid", 99), (-3, "x", None), (-4, "n", 0), (-4, "n", 2 ** 31), (-5, "d", 17), (-6, "theta", None),
        (-7, "ntheta", 2), (-8, "idx", None), (-9, "ld", m - 1), (-10, "m", 0), (-10, "m", 65), (-11, "v", None), (-12, "coef", None),
        (-13, "ldc", m - 1), (-14, "dinv", None), (-15, "work", None), (-15, "work", bad(wf)), (-16, "wb", wf.numel() * 8 - 8),
        (-17, "info", None)])
    assert set(seen) == set(range(-17, 0))

    W = {"idx": p(idx), "ld": ld, "m": m, "coef": p(outs["coef"]), "dinv": p(outs["dinv"]), "start": p(start), "pos": p(pos), "nnz": 0}
    apply = {"h": H._h, "n": n, **W, "R": p(R), "ldr": s, "s": s, "Z": p(outs["Z"]), "ldz": s, "work": p(wa), "wb": wa.numel() * 8}
    outs["coef"].zero_()
    outs["dinv"].fill_(1.0)
    assert L.fvgp_hip_nn_precond_apply(*apply.values()) == 0
    H.sync()
    assert np.array_equal(outs["Z"].cpu().numpy(), R.cpu().numpy()), "W = I"
    seen = run(L.fvgp_hip_nn_precond_apply, apply, [
        (-1, "h", None), (-2, "n", 0), (-2, "n", 2 ** 31), (-3, "idx", None), (-4, "ld", m - 1), (-5, "m", 0), (-5, "m", 65),
        (-6, "coef", None), (-7, "dinv", None), (-8, "start", None), (-9, "pos", None), (-10, "nnz", -1), (-10, "nnz", n * ld + 1),
        (-11, "R", None), (-12, "ldr", s - 1), (-13, "s", 0), (-13, "s", 17), (-14, "Z", None), (-15, "ldz", s - 1), (-16, "work", None),
        (-16, "work", bad(wa)), (-17, "wb", wa.numel() * 8 - 8)])
    assert set(seen) == set(range(-17, 0))

    outs["coef"].zero_()
    outs["dinv"].fill_(1.0)
    B = H.zeros(n, s)
    pcg = {"h": H._h, "kid": 1, "x": p(x), "n": n, "d": d, "theta": tp, "ntheta": 3, "v": p(v), **W, "B": p(B), "ldb": s, "s": s,
           "X": p(outs["X"]), "ldx": s, "warm": 0, "tol": 1e-9, "max_iter": 10, "check_every": 2, "max_restarts": 1, "work": p(wp),
           "wb": wp.numel() * 8, "iters": iters, "relres": relres, "status": status}
    seen = run(L.fvgp_hip_pcg_nn, pcg, [
        (-1, "h", None), (-2, "kid", 99), (-3, "x", None), (-4, "n", 0), (-5, "d", 17), (-6, "theta", None), (-7, "ntheta", 2),
        (-8, "v", None), (-9, "idx", None), (-10, "ld", m - 1), (-11, "m", 0), (-11, "m", 65), (-12, "coef", None), (-13, "dinv", None),
        (-14, "start", None), (-15, "pos", None), (-16, "nnz", -1), (-16, "nnz", n * ld + 1), (-17, "B", None), (-18, "ldb", s - 1),
        (-19, "s", 0), (-19, "s", 17), (-20, "X", None), (-21, "ldx", s - 1), (-23, "tol", 0.0), (-24, "max_iter", 0),
        (-25, "check_every", 0), (-26, "max_restarts", -1), (-27, "work", None), (-27, "work", bad(wp)), (-28, "wb", wp.numel() * 8 - 8),
        (-29, "iters", None), (-30, "relres", None), (-31, "status", None)])
    assert set(seen) == set(range(-31, 0)) - {-22}
    # the binding's own refusals
    with pytest.raises(ValueError, match="leading dimension"):
        H.nn_factor(1, x, theta, idx, m, v, coef=H.empty(n, ld + 1))


# ---- 5. the facade -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade():
    import fvgp_amd
    rng = np.random.default_rng(707)
    n, d, P = 600, 2, 21
    x = rng.random((n + 40, d))
    y = np.sin(3.0 * x.sum(axis=1)) + 0.05 * rng.standard_normal(n + 40)
    V = 1e-2 * (1.0 + rng.random(n + 40))
    theta = np.array([1.3, 0.3, 0.45])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x[:n], y[:n], init_hyperparameters=theta, noise_variances=V[:n], kernel_function="matern52_ard")
    return {"gp": gp, "x": x, "y": y, "V": V, "theta": theta, "xp": rng.random((P, d)), "n": n}


def _vecchia_mf(fc, n=None, **args):
    import fvgp_amd
    n = fc["n"] if n is None else n
    return fvgp_amd.MatrixFreeGP(fc["x"][:n], fc["y"][:n], fc["theta"], noise_variances=fc["V"][:n], kernel_function="matern52_ard",
                                 args={"preconditioner": "vecchia", **args})


def test_facade_matches_the_dense_gp(facade):
    fc = facade
    n, xp, gp, sig = fc["n"], fc["xp"], fc["gp"], fc["theta"][0]
    for ordering in ("random", "maxmin"):
        big = _vecchia_mf(fc, precond_ordering=ordering)
        assert big.preconditioner == "vecchia" and big.precond_neighbors == 32 and not np.array_equal(big.ordering, np.arange(n))
        assert np.array_equal(big.x_data, fc["x"][:n]) and np.array_equal(big.y_data, fc["y"][:n]), "the caller's order"
        got = big.posterior_mean(xp)
        assert got["converged"] and np.max(np.abs(got["m(x)"] - gp.posterior_mean(xp)["m(x)"])) <= 1e-7 * sig
        v = big.posterior_covariance(xp, variance_only=True)["v(x)"]
        assert np.max(np.abs(v - gp.posterior_covariance(xp, variance_only=True)["v(x)"])) <= 1e-7 * sig
        # solve(b) in the caller's order: against numpy on the caller's matrix
        A = np.asarray(kf.k_ref("matern52_ard", fc["x"][:n], fc["x"][:n], fc["theta"]), dtype=np.float64) + np.diag(fc["V"][:n])
        b = np.random.default_rng(1).standard_normal((n, 2))
        out = big.solve(b)
        assert out["converged"] and np.max(out["relative_residual"]) <= big.tol
        assert np.linalg.norm(A @ out["x"] - b) <= 1e-8 * np.linalg.norm(b)
        assert big.solve(b[:, 0])["x"].shape == (n,)
        print(f"\nNP|facade|{ordering}|alpha iterations {got['iterations']}")


def test_facade_default_is_the_pivoted_cholesky_bit_for_bit(facade):
    import fvgp_amd
    fc = facade
    n, xp = fc["n"], fc["xp"]
    mk = lambda args: fvgp_amd.MatrixFreeGP(fc["x"][:n], fc["y"][:n], fc["theta"], noise_variances=fc["V"][:n],      # noqa: E731
                                            kernel_function="matern52_ard", args=args)
    a, b = mk(None), mk({"preconditioner": "pchol"})
    assert a.preconditioner == b.preconditioner == "pchol"
    ma, mb = a.posterior_mean(xp), b.posterior_mean(xp)
    assert np.array_equal(ma["m(x)"], mb["m(x)"]) and ma["iterations"] == mb["iterations"]
    assert np.array_equal(a.posterior_covariance(xp, variance_only=True)["v(x)"], b.posterior_covariance(xp, variance_only=True)["v(x)"])
    assert np.array_equal(a.solve(np.ones(n))["x"], b.solve(np.ones(n))["x"])
    with pytest.raises(ValueError, match="'pchol' or 'vecchia'"):
        mk({"preconditioner": "jacobi"})
    with pytest.raises(ValueError, match="n_neighbors must lie in 1 .. 64"):
        mk({"preconditioner": "vecchia", "precond_neighbors": 65})
    with pytest.raises(ValueError, match="ordering must be"):
        mk({"preconditioner": "vecchia", "precond_ordering": "sorted"})
    with pytest.raises(NotImplementedError, match="vecchia"):
        a.neighbors()


def test_facade_hyperparameters_updates_and_the_shared_lists(facade):
    import fvgp_amd
    fc = facade
    n, xp, x, y, V = fc["n"], fc["xp"], fc["x"], fc["y"], fc["V"]
    big = _vecchia_mf(fc)
    big.posterior_mean(xp)
    nb, idx, tr = big.neighbors(), big._idx, big._transposed
    d0 = big.preconditioner_factor().dinv.cpu().numpy().copy()
    assert nb.shape == (n, 32) and np.all(nb < n)
    # new hyperparameters: the lists and their transpose stay, the factor is made again, lazily
    big.set_hyperparameters(fc["theta"] * 1.1)
    assert big._W is None and big._idx is idx and big._transposed is tr and np.array_equal(big.neighbors(), nb)
    assert not np.array_equal(big.preconditioner_factor().dinv.cpu().numpy(), d0)
    big.set_hyperparameters(fc["theta"])
    assert np.array_equal(big.preconditioner_factor().dinv.cpu().numpy(), d0)
    # appended data: the structure is rebuilt, alpha warm-starts
    big.posterior_mean(xp)
    big.update_gp_data(x[n:], y[n:], noise_variances_new=V[n:])
    warm = big._alpha_info["iterations"]
    fresh = _vecchia_mf(fc, n=n + 40)
    a, b = big.posterior_mean(xp), fresh.posterior_mean(xp)
    print(f"\nNP|facade|alpha iterations: warm {warm} cold {b['iterations']}")
    assert big.point_number == n + 40 and big.neighbors().shape == (n + 40, 32) and a["converged"] and warm <= b["iterations"]
    assert np.max(np.abs(a["m(x)"] - b["m(x)"])) <= 1e-7 * fc["theta"][0]
    # VecchiaGP.matrix_free: the exact answer beside the approximation, over the same ordering and lists
    nn = fvgp_amd.VecchiaGP(x[:n], y[:n], fc["theta"], noise_variances=V[:n], kernel_function="matern52_ard", n_neighbors=16, ordering="maxmin")
    exact = nn.matrix_free()
    assert isinstance(exact, fvgp_amd.MatrixFreeGP) and exact._idx is nn._idx and exact.ordering is nn.ordering and exact.precond_neighbors == 16
    assert np.array_equal(exact.neighbors(), nn.neighbors())
    want = fc["gp"].posterior_mean(xp)["m(x)"]
    assert np.max(np.abs(exact.posterior_mean(xp)["m(x)"] - want)) <= 1e-7 * fc["theta"][0]
    assert np.max(np.abs(nn.posterior_mean(xp)["m(x)"] - want)) > 1e-7 * fc["theta"][0], "the approximation is one"
    with pytest.raises(ValueError, match="'vecchia' here"):
        nn.matrix_free(args={"preconditioner": "pchol"})


def test_facade_refuses_the_likelihood_and_names_a_failed_conditional(facade):
    fc = facade
    n = fc["n"]
    big = _vecchia_mf(fc, stochastic_likelihood=True)
    bounds = np.array([[0.1, 10.0], [0.05, 2.0], [0.05, 2.0]])
    calls = [big.log_likelihood_estimate, big.stochastic_log_likelihood, big.stochastic_neg_log_likelihood,
             big.stochastic_neg_log_likelihood_gradient, big.stochastic_neg_log_likelihood_and_gradient, big.log_likelihood,
             big.neg_log_likelihood, big.neg_log_likelihood_gradient, lambda: big.train_stochastic(bounds), lambda: big.train(bounds)]
    for call in calls:
        with pytest.raises(NotImplementedError, match=r'preconditioner="pchol".*VecchiaGP.*deterministic likelihood'):
            call()
    # a duplicated point with noise that vanishes beside sigma^2 = 1, one neighbour per row (the conditional variance of the second copy
    # in the ordering is then (1 + 1e-300) - 1 * 1 = 0 exactly): it fails, named by the caller's index
    import fvgp_amd
    from fvgp_amd.gp_lin_alg import NonPositiveDefiniteError
    x, V = fc["x"][:n].copy(), fc["V"][:n].copy()
    x[411] = x[77]
    V[[77, 411]] = 1e-300
    bad = fvgp_amd.MatrixFreeGP(x, fc["y"][:n], np.array([1.0, 0.3, 0.45]), noise_variances=V, kernel_function="matern52_ard",
                                args={"preconditioner": "vecchia", "precond_ordering": np.arange(n)[::-1].copy(), "precond_neighbors": 1})
    with pytest.raises(NonPositiveDefiniteError, match="data point 77 "):
        bad.posterior_mean(fc["xp"])
