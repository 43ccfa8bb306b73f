"""The stochastic log-likelihood on the matrix-free path (fvgp_hip_kgrad_form, fvgp_hip_precond_probes, fvgp_hip_precond_apply,
fvgp_hip_pcg_lanczos, MatrixFreeGP.log_likelihood_estimate / train_stochastic): the form against longdouble, the probes, the apply and the
recorded coefficients against the numpy twin of tests/mf_likelihood_ref.py, the bit contracts, the estimate against slogdet and the
dense GP's gradient, training, the opt-in for the fvgp.GP method names, and refused arguments."""
import ctypes
import warnings

import numpy as np
import pytest

import kernel_family_ref as kf
import matrix_free_ref as mf
import mf_likelihood_ref as ml

pytestmark = pytest.mark.gpu

CANARY = -7.25e300
CHUNK = mf.CHUNK
# The recorded coefficients and the estimates against the twin, RELATIVE.  Measured once on an MI355X over the three fixtures (the prints
# of the tests below): alpha, beta, rho_0 differed from the twin by at most 7.0e-13 (matern32_ard, 15 steps), 1.2e-10 (matern32_iso, 3
# steps) and 1.2e-11 (rbf_iso, 4 steps); the estimates by at most 3.8e-13 (value, log det, data fit: 2e-14; gradient 3.8e-13; standard
# errors 1.7e-12), 3.8e-10 (the log det's standard error; gradient 3.2e-12) and 4.9e-11 in the same order.  Each bound is ten times the
# largest observation and never above RTOL_CAP; what is checked beyond the three fixtures (one-step and Jacobi records) is held to the cap.
RTOL_CAP = 1e-6
LANCZOS_OBSERVED = 1.2e-10
ESTIMATE_OBSERVED = 3.9e-10
LANCZOS_RTOL = min(10 * LANCZOS_OBSERVED, RTOL_CAP)
ESTIMATE_RTOL = min(10 * ESTIMATE_OBSERVED, RTOL_CAP)


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def _kid(kernel):
    from fvgp_amd import _lib
    return _lib.KERNEL_IDS[kernel]


def _framed(H, shape):
    """a canary-filled buffer with a frame around the view the call gets and an odd leading dimension: (buffer, view)"""
    t = H.torch
    odd = 3 if shape[1] % 2 == 0 else 4
    big = t.full((shape[0] + 2, shape[1] + odd), CANARY, dtype=t.float64, device=f"cuda:{H.device}")
    assert big.stride(0) % 2 == 1
    return big, big[1:1 + shape[0], :shape[1]]


def _frame_untouched(big, view_shape):
    a = big.cpu().numpy()
    return np.all(a[0] == CANARY) and np.all(a[1 + view_shape[0]:] == CANARY) and np.all(a[:, view_shape[1]:] == CANARY)


def _framed_copy(H, a):
    """the host array inside a frame on the device (a strided view with an odd leading dimension)"""
    big, view = _framed(H, a.shape)
    view.copy_(H.to_device(a))
    return big, view


# ---- 1. the form against longdouble --------------------------------------------------------------------------------------------------------
def form_case(kernel, d, n1, n2, s, square, seed):
    """x1 (n1, d), x2 (n2, d) with one coincident pair (square: x2 = x1, W = U, and two coincident points among them), U (n1, s), W (n2, s)
    of full-mantissa entries scaled by rows over 2^-10 .. 2^10, theta of matrix_free_ref"""
    rng = np.random.default_rng(seed)
    x2 = rng.random((n2, d))
    x1 = x2 if square else rng.random((n1, d))
    if square and n2 > 2:
        x2[n2 - 1] = x2[0]
    if not square:
        x2[n2 // 2] = x1[0]
    W = rng.standard_normal((n2, s)) * np.exp2(rng.integers(-10, 11, size=(n2, 1)).astype(np.float64))
    U = W if square else rng.standard_normal((n1, s)) * np.exp2(rng.integers(-10, 11, size=(n1, 1)).astype(np.float64))
    return x1, x2, U, W, mf.theta_of(kernel, d, 0.3)


def _form(H, kernel, x1, x2, U, W, theta, split=0, work=None, fill=None):
    """one Handle.kgrad_form call with the given "matvec_split"; U and W go as strided views inside frames"""
    from fvgp_amd import _lib
    x1d = H.to_device(x1)
    x2d = x1d if x2 is x1 else H.to_device(x2)
    ubig, Ud = _framed_copy(H, U)
    wbig, Wd = (ubig, Ud) if W is U else _framed_copy(H, W)
    if work is None:
        work = H.empty(max(1, _lib.kgrad_form_workspace_bytes(len(x1), len(x2)) // 8))
    if fill is not None:
        work.fill_(fill)
    H.set_option("matvec_split", split)
    try:
        out = H.kgrad_form(_kid(kernel), x1d, Ud, x2d, Wd, theta, work=work)
    finally:
        H.set_option("matvec_split", 0)
    assert _frame_untouched(ubig, U.shape) and _frame_untouched(wbig, W.shape)
    assert np.array_equal(Ud.cpu().numpy(), U) and np.array_equal(Wd.cpu().numpy(), W)
    return out[:kf.n_theta(kernel, x1.shape[1])]


# (kernel, d, n1, n2, s, x1 = x2 and U = W): every kernel id, d = 1 .. 4 and 5 (the runtime-dimension instantiation), the shapes
# (1, 1), (63, 65), (64, 257), (257, 255), (300, 4097), (130, 8193) -- one row, ragged blocks, more than one block, a ragged last slice, one
# chunk and a bit, two chunks and a bit (the split launch) -- s of {1, 3, 4, 16}, and s = 9: two groups (8 + 1), the second ADDED to the first;
# the last two are the runtime-dimension kernels with wide column groups and parked chunk sums (the register-tight instantiations)
FORM_CASES = [
    ("rbf_ard", 1, 1, 1, 1, False),
    ("matern32_ard", 2, 63, 65, 3, False),
    ("matern52_ard", 3, 64, 257, 4, False),
    ("rbf_iso", 4, 257, 255, 16, False),
    ("matern32_iso", 5, 300, 4097, 3, False),
    ("matern52_iso", 2, 130, 8193, 16, False),
    ("matern52_ard", 5, 257, 257, 4, True),
    ("matern32_ard", 3, 300, 300, 1, True),
    ("rbf_ard", 2, 65, 300, 9, False),
    ("matern32_iso", 1, 64, 257, 1, False),
    ("rbf_iso", 3, 63, 65, 4, False),
    ("matern52_iso", 4, 1, 1, 3, False),
    ("matern52_ard", 5, 65, 2 * CHUNK + 37, 16, False),
    ("rbf_ard", 5, 130, CHUNK + 1, 9, False),
]


@pytest.mark.parametrize("case", FORM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_form_against_longdouble(H, case):
    """|out_j - ref_j| <= (32 + 2 d) eps max|dK_j| sum_c sum|U_c| sum|W_c| + (n2 + s + 4) (eps / 2) sum_c |U_c|^T |dK_j| |W_c|
    (mf_likelihood_ref.kgrad_form_bound): the entry error of dK_j plus Higham's gamma of a lane's sum.
    OBSERVED on an MI355X (an observation, not a bound): the largest share of the bound used over these cases was 0.011 (n1 = n2 = 1,
    where the bound is the entry error alone; 0.008 at the other single entry); the cases with 65 <= n2 <= 300 used 9e-5 .. 2.5e-3 of it, the
    cases from n2 = 4097 on at most 1.3e-5."""
    kernel, d, n1, n2, s, square = case
    x1, x2, U, W, theta = form_case(kernel, d, n1, n2, s, square, 11 * n1 + n2 + s)
    got = _form(H, kernel, x1, x2, U, W, theta)
    ref, mag = ml.kgrad_form_ref(kernel, x1, U, x2, W, theta)
    bound = ml.kgrad_form_bound(kernel, x1, U, x2, W, theta, mag)
    err = np.abs(got - ref)
    share = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
    print(case, "largest share of the bound:", share)
    assert np.all(err <= bound), (share, got, ref)


def test_form_bits(H):
    """the same call twice; whatever the workspace held before; unsplit (1), forced splits (2, 3) and the split by the shape (0), with and
    without room for the parked chunk sums; nothing behind the result's entries is written.  (The column groups are part of the value --
    include/fvgp_hip.h -- so a sum of one-column calls on the host is NOT asserted equal.)  The same at d = 5, n1 = 65, s = 16: the
    runtime-dimension kernel with the widest column group."""
    from fvgp_amd import _lib
    for kernel, d, n1, n2, s in (("matern52_ard", 5, 65, 2 * CHUNK + 37, 16), ("matern52_ard", 3, 130, 2 * CHUNK + 37, 9)):
        x1, x2, U, W, theta = form_case(kernel, d, n1, n2, s, False, 77)
        full = _form(H, kernel, x1, x2, U, W, theta, split=1, fill=0.0)
        assert np.array_equal(full, _form(H, kernel, x1, x2, U, W, theta, split=1, fill=float("nan")))
        for k in (0, 2, 3):
            assert np.array_equal(full, _form(H, kernel, x1, x2, U, W, theta, split=k, fill=CANARY)), (d, k)
        small = H.empty((1 + (n1 + 63) // 64) * 17)               # no room for the chunk sums: one workgroup walks the chunks
        assert np.array_equal(full, _form(H, kernel, x1, x2, U, W, theta, split=3, work=small, fill=CANARY)), d
    # zero columns change nothing: 9 columns against the same 9 inside wider arrays is not a contract, but U = 0 columns are
    U0, W0 = U.copy(), W.copy()
    U0[:, 8] = 0.0
    assert np.array_equal(_form(H, kernel, x1, x2, U0, W0, theta), _form(H, kernel, x1, x2, U0[:, :8].copy(), W0[:, :8].copy(), theta))
    # the host result: only the kernel's own entries are written
    L = _lib.lib()
    out = np.full(d + 1 + 4, CANARY)
    th = np.ascontiguousarray(theta)
    x1d, x2d, Ud, Wd = H.to_device(x1), H.to_device(x2), H.to_device(U), H.to_device(W)
    work = H.empty(_lib.kgrad_form_workspace_bytes(n1, n2) // 8)
    rc = L.fvgp_hip_kgrad_form(H._h, _kid(kernel), ctypes.c_void_p(x1d.data_ptr()), n1, ctypes.c_void_p(x2d.data_ptr()), n2, d,
                               th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(th), ctypes.c_void_p(Ud.data_ptr()), s,
                               ctypes.c_void_p(Wd.data_ptr()), s, s, ctypes.c_void_p(work.data_ptr()), work.numel() * 8,
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == 0 and np.array_equal(out[:d + 1], full) and np.all(out[d + 1:] == CANARY)


# ---- the fixtures on the device ------------------------------------------------------------------------------------------------------------
_DEV = {}


def _dev(H, fx, rank=mf.RANK):
    """the fixture on the device with its rank-128 preconditioner (pchol_tol 1e-12, as the facade builds it), once per module:
    (x, V, G, C, G on the host)"""
    if (fx, rank) not in _DEV:
        f = mf.fixture(fx)
        n = len(f["x"])
        xd, Vd = H.to_device(np.array(f["x"])), H.to_device(np.array(f["V"]))
        G = C = Gh = None
        if rank:
            gbig, G = _framed(H, (rank, n))
            piv = H.torch.empty(rank, dtype=H.torch.int64, device=G.device)
            assert H.pchol(_kid(f["kernel"]), xd, f["theta"], rank, G, piv, tol=1e-12) >= 64
            C = H.empty(128, 128)
            assert H.precond_factor(G, rank, n, Vd, C) == 0
            assert _frame_untouched(gbig, (rank, n))
            Gh = G.cpu().numpy()
        _DEV[(fx, rank)] = (xd, Vd, G, C, Gh)
    return _DEV[(fx, rank)]


# ---- 2. the probes ---------------------------------------------------------------------------------------------------------------------------
def _probes(H, fx, s, rank=mf.RANK, seed=ml.SEED, stream=0, col0=0):
    xd, Vd, G, C, _ = _dev(H, fx, rank)
    n = xd.shape[0]
    zbig, Z = _framed(H, (n, s))
    H.precond_probes(Z, Vd, G=G, q=rank, seed=seed, stream=stream, col0=col0)
    H.sync()
    assert _frame_untouched(zbig, (n, s))
    return Z.cpu().numpy()


def test_probes_against_the_twin(H):
    """|Z - Z_twin| <= 1e-13 (sqrt(v_i) + sum_t |G[t][i]|) per entry; columns 0 .. 4 of a 16-column call equal a 5-column call, col0
    shifts columns, the stream separates draws, rank 0 is D^1/2 eps; the frame around Z stays untouched"""
    fx = mf.FIXTURES[1]
    f = mf.fixture(fx)
    Gh = _dev(H, fx)[4]
    Z = _probes(H, fx, 16)
    ref = ml.probes_ref(ml.SEED, 0, 0, 16, Gh, f["V"])
    scale = np.sqrt(f["V"]) + np.abs(Gh).sum(axis=0)
    print("probes: largest |Z - twin| / (sqrt v + sum |G|):", float(np.max(np.abs(Z - ref) / scale[:, None])))
    assert np.all(np.abs(Z - ref) <= 1e-13 * scale[:, None])
    assert np.array_equal(_probes(H, fx, 5), Z[:, :5])
    assert np.array_equal(_probes(H, fx, 7, col0=9), Z[:, 9:16])
    assert np.array_equal(_probes(H, fx, 1, col0=15)[:, 0], Z[:, 15])
    other = _probes(H, fx, 3, stream=1)
    assert np.all(np.abs(other - ml.probes_ref(ml.SEED, 1, 0, 3, Gh, f["V"])) <= 1e-13 * scale[:, None]) and not np.array_equal(other, Z[:, :3])
    Z0 = _probes(H, fx, 4, rank=0)
    ref0 = ml.probes_ref(ml.SEED, 0, 0, 4, None, f["V"])
    assert np.all(np.abs(Z0 - ref0) <= 1e-13 * np.sqrt(f["V"])[:, None])
    # the sample covariance of 16 probes is no test of M; their second moment against diag(M) within 5 sigma of a chi^2_16 mean is
    m2 = (Z ** 2).mean(axis=1) / (f["V"] + (Gh ** 2).sum(axis=0))
    assert abs(m2.mean() - 1.0) <= 5.0 * np.sqrt(2.0 / 16.0 / len(m2))


# ---- 3. the preconditioner on its own -------------------------------------------------------------------------------------------------------
def _apply(H, fx, R, rank=mf.RANK, inplace=False):
    xd, Vd, G, C, _ = _dev(H, fx, rank)
    n, s = R.shape
    rbig, Rd = _framed_copy(H, R)
    if inplace:
        H.precond_apply(Rd, Rd, Vd, G=G, q=rank, C=C)
        H.sync()
        assert _frame_untouched(rbig, (n, s))
        return Rd.cpu().numpy()
    wbig, Wd = _framed(H, (n, s))
    H.precond_apply(Rd, Wd, Vd, G=G, q=rank, C=C)
    H.sync()
    assert _frame_untouched(wbig, (n, s)) and np.array_equal(Rd.cpu().numpy(), R)
    return Wd.cpu().numpy()


@pytest.mark.parametrize("fx", mf.PRECOND_FIXTURES, ids=mf.fixture_id)
def test_apply_against_woodbury(H, fx):
    """W = M^-1 R against matrix_free_ref.woodbury_apply, column by column: |dW| <= 64 eps cond(M) |W| in the 2-norm -- both sides solve
    with M in double, each is within a small multiple of eps cond(M) of the exact W (the bound the solver's own accuracy tests lean on:
    a preconditioner applied to rounding); a column alone has the bits it has inside s = 16; in place works; rank 0 is R / v"""
    f = mf.fixture(fx)
    Gh = _dev(H, fx)[4]
    R = np.array(f["rhs"])
    W = _apply(H, fx, R)
    ref = mf.woodbury_apply(Gh, f["V"], R)
    ev = np.linalg.eigvalsh(Gh.T @ Gh + np.diag(f["V"]))
    cond = ev[-1] / ev[0]
    rel = np.linalg.norm(W - ref, axis=0) / np.linalg.norm(ref, axis=0)
    print(mf.fixture_id(fx), "apply: largest |dW| / |W|:", float(rel.max()), "eps cond(M):", kf.EPS * cond)
    assert np.all(rel <= 64 * kf.EPS * cond)
    for c in (0, 9, 15):
        assert np.array_equal(_apply(H, fx, R[:, c:c + 1].copy())[:, 0], W[:, c]), c
    assert np.array_equal(_apply(H, fx, R[:, :5].copy(), inplace=True), W[:, :5])
    assert np.array_equal(_apply(H, fx, R[:, :3].copy(), rank=0), R[:, :3] / f["V"][:, None])


# ---- 4. the solver with its coefficients recorded ------------------------------------------------------------------------------------------
def _lanczos(H, fx, B, L, rank=mf.RANK, tol=ml.PROBE_TOL, **kw):
    f = mf.fixture(fx)
    n, s = B.shape
    xd, Vd, G, C, _ = _dev(H, fx, rank)
    xbig, X = _framed(H, (n, s))
    out = H.pcg_lanczos(_kid(f["kernel"]), xd, f["theta"], Vd, H.to_device(B), X, L, G=G, q=rank, C=C, tol=tol, **kw)
    assert _frame_untouched(xbig, (n, s))
    return (X.cpu().numpy(),) + out


def _plain(H, fx, B, rank=mf.RANK, tol=ml.PROBE_TOL):
    f = mf.fixture(fx)
    n, s = B.shape
    xd, Vd, G, C, _ = _dev(H, fx, rank)
    X = H.empty(n, s)
    return (X,) + H.pcg(_kid(f["kernel"]), xd, f["theta"], Vd, H.to_device(B), X, G=G, q=rank, C=C, tol=tol)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


@pytest.mark.parametrize("fx", ml.ESTIMATE_FIXTURES, ids=mf.fixture_id)
def test_lanczos_records_against_the_twin(H, fx):
    """X, iterations and residuals have the bits of fvgp_hip_pcg for L = 0, 1 and 64; the recorded alpha, beta and rho_0 of four columns lie
    within LANCZOS_RTOL (relative) of the twin's first recurrence run with the device's G; steps = min(L, iterations); a column's records
    are the same alone and inside s = 16; entries never recorded are 0"""
    f = mf.fixture(fx)
    B = np.array(f["rhs"])
    Gh = _dev(H, fx)[4]
    Xp, itp, rrp, stp = _plain(H, fx, B)
    Xp = Xp.cpu().numpy()
    runs = {L: _lanczos(H, fx, B, L) for L in (0, 1, 64)}
    for L, (X, it, rr, st, al, be, steps, rho0) in runs.items():
        assert np.array_equal(X, Xp) and np.array_equal(it, itp) and np.array_equal(rr, rrp) and np.array_equal(st, stp), L
        assert np.all(st == 0)
        if L:
            assert np.array_equal(steps, np.minimum(L, it)) and al.shape == be.shape == (16, L)      # (no column restarts at this tolerance)
    X, it, rr, st, al, be, steps, rho0 = runs[64]
    _, _, _, _, al1, be1, steps1, rho01 = runs[1]
    assert np.array_equal(al1[:, 0], al[:, 0]) and np.array_equal(rho01, rho0) and np.all(steps1 == 1)
    assert np.array_equal(be1[:, 0], np.where(it > 1, be[:, 0], 0.0))
    worst = 0.0
    for c in range(4):
        _, itt, _, stt, alt, bet, rhot = ml.pcg_lanczos_ref(np.array(f["A"]), B[:, c], f["V"], Gh, ml.PROBE_TOL, 64)
        assert stt == 0 and it[c] == itt and steps[c] == len(alt)
        m = len(alt)
        assert np.all(al[c, m:] == 0.0) and np.all(be[c, len(bet):] == 0.0)
        worst = max(worst, _rel(al[c, :m], alt), _rel(be[c, :len(bet)], bet), _rel(rho0[c], rhot))
        q_dev, q_twin = ml.quadrature(al[c, :m], be[c, :m], rho0[c]), ml.quadrature(alt, bet, rhot)
        assert abs(q_dev - q_twin) <= LANCZOS_RTOL * rho0[c]
    print(mf.fixture_id(fx), "records: largest relative difference to the twin:", worst, "iterations", it.tolist())
    assert worst <= LANCZOS_RTOL
    for c in (0, 9, 15):
        Xc, itc, rrc, stc, alc, bec, stepc, rhoc = _lanczos(H, fx, B[:, c:c + 1].copy(), 64, check_every=3)
        assert np.array_equal(Xc[:, 0], X[:, c]) and itc[0] == it[c] and rrc[0] == rr[c]
        assert np.array_equal(alc[0], al[c]) and np.array_equal(bec[0], be[c]) and stepc[0] == steps[c] and rhoc[0] == rho0[c], c


def test_lanczos_one_step_and_edge_cases(H):
    """the RBF fixture at rank 128 converges in ONE iteration: a 1 x 1 T whose quadrature is rho_0 log(1 / alpha_0); a zero column records
    nothing and leaves its neighbours' records alone; rank 0 (Jacobi) records its first L = 8 steps and solves on"""
    fx = mf.FIXTURES[0]
    Z = _probes(H, fx, 4)
    X, it, rr, st, al, be, steps, rho0 = _lanczos(H, fx, Z, 64)
    assert np.all(st == 0) and np.all(it == 1) and np.all(steps == 1) and np.all(be == 0.0) and np.all(al[:, 1:] == 0.0)
    f = mf.fixture(fx)
    Gh = _dev(H, fx)[4]
    for c in range(4):
        _, itt, _, _, alt, bet, rhot = ml.pcg_lanczos_ref(np.array(f["A"]), Z[:, c], f["V"], Gh, ml.PROBE_TOL, 64)
        assert itt == 1 and len(bet) == 0
        print("one step, column", c, "relative differences to the twin: alpha", _rel(al[c, 0], alt[0]), "rho0", _rel(rho0[c], rhot))
        assert _rel(al[c, 0], alt[0]) <= RTOL_CAP and _rel(rho0[c], rhot) <= RTOL_CAP
        q = ml.quadrature(al[c, :1], be[c, :0], rho0[c])
        assert np.isfinite(q) and q == pytest.approx(rho0[c] * np.log(1.0 / al[c, 0]), rel=1e-12, abs=1e-300)
    # a zero column between two others
    fx = mf.FIXTURES[2]
    B = np.array(mf.fixture(fx)["rhs"][:, :3])
    full = _lanczos(H, fx, B, 8)
    B[:, 1] = 0.0
    X, it, rr, st, al, be, steps, rho0 = _lanczos(H, fx, B, 8)
    assert it[1] == 0 and steps[1] == 0 and rho0[1] == 0.0 and np.all(al[1] == 0.0) and np.all(X[:, 1] == 0.0)
    for c in (0, 2):
        assert np.array_equal(al[c], full[4][c]) and np.array_equal(be[c], full[5][c]) and rho0[c] == full[7][c]
    assert np.all(steps[[0, 2]] == np.minimum(8, it[[0, 2]]))
    # Jacobi: more iterations than L = 8 records; the solve goes on to its tolerance
    X0, it0, rr0, st0, al0, be0, steps0, rho00 = _lanczos(H, fx, np.array(mf.fixture(fx)["rhs"][:, :2]), 8, rank=0)
    assert np.all(st0 == 0) and np.all(it0 > 8) and np.all(steps0 == 8) and np.all(al0 > 0.0) and np.all(be0 > 0.0)
    f2 = mf.fixture(fx)
    _, itt, _, _, alt, bet, rhot = ml.pcg_lanczos_ref(np.array(f2["A"]), np.array(f2["rhs"][:, 0]), f2["V"], None, ml.PROBE_TOL, 8)
    assert len(alt) == 8 and len(bet) == 8
    print("Jacobi, 8 steps: relative differences to the twin: alpha", _rel(al0[0], alt), "beta", _rel(be0[0], bet), "rho0", _rel(rho00[0], rhot))
    assert max(_rel(al0[0], alt), _rel(be0[0], bet), _rel(rho00[0], rhot)) <= RTOL_CAP


# ---- 5. the estimate -------------------------------------------------------------------------------------------------------------------------
_GPS = {}


def _gps(fx):
    """(MatrixFreeGP, dense GP) over a fixture with y = column 0 of its right-hand sides, once per module"""
    if fx not in _GPS:
        import fvgp_amd
        f = mf.fixture(fx)
        x, y, V = np.array(f["x"]), ml.fixture_y(fx), np.array(f["V"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dense = fvgp_amd.GP(x, y, init_hyperparameters=np.array(f["theta"]), noise_variances=V, kernel_function=f["kernel"])
        _GPS[fx] = (fvgp_amd.MatrixFreeGP(x, y, np.array(f["theta"]), noise_variances=V, kernel_function=f["kernel"]), dense)
    return _GPS[fx]


@pytest.mark.parametrize("fx", ml.ESTIMATE_FIXTURES, ids=mf.fixture_id)
def test_estimate_against_dense_values_and_the_twin(H, fx):
    """rank 128, 16 probes, the seed tests/test_mf_likelihood_host.py checked: the device's log det within 4 of its own standard errors of
    slogdet(K + V), every gradient component within 4 standard errors of the dense GP's neg_log_likelihood_gradient, and the estimate within
    ESTIMATE_RTOL (relative) of the twin's, run with the device's G"""
    f = mf.fixture(fx)
    big, dense = _gps(fx)
    e = big.log_likelihood_estimate(n_probes=ml.PROBES, seed=ml.SEED, gradient=True)
    logdet, _ = ml.fixture_dense(fx)
    assert e["converged"] and e["lanczos_steps"].max() < ml.STEPS
    z = (e["logdet"] - logdet) / e["logdet_std_error"]
    g_dense = np.asarray(dense.neg_log_likelihood_gradient(hyperparameters=np.array(f["theta"])))
    zg = (e["neg_gradient"] - g_dense) / e["neg_gradient_std_error"]
    print(mf.fixture_id(fx), "log det", e["logdet"], "dense", logdet, "se", e["logdet_std_error"], "z", z)
    print("   gradient", e["neg_gradient"], "dense", g_dense, "se", e["neg_gradient_std_error"], "z", zg)
    assert abs(z) <= 4.0
    assert np.all(np.abs(zg) <= 4.0)
    nll = float(dense.neg_log_likelihood(hyperparameters=np.array(f["theta"])))
    assert abs(-e["log_likelihood"] - nll) <= 4.0 * e["std_error"] + 1e-9 * abs(nll)
    # the twin with the device's preconditioner
    Gh = big._G.cpu().numpy()
    t = ml.estimate_ref(f["kernel"], f["x"], ml.fixture_y(fx), f["V"], f["theta"], mf.RANK, seed=ml.SEED, gradient=True,
                        K=np.array(f["K"]), G=Gh)
    diffs = {k: _rel(e[k], t[k]) for k in ("log_likelihood", "logdet", "logdet_preconditioner", "data_fit", "neg_gradient", "trace",
                                           "logdet_std_error", "neg_gradient_std_error")}
    diffs["per_probe"] = float(np.max(np.abs(e["per_probe"] - t["per_probe"])) / abs(t["logdet"]))
    print("   relative differences to the twin:", diffs)
    assert np.array_equal(e["iterations"], t["iterations"]) and np.array_equal(e["lanczos_steps"], t["lanczos_steps"])
    assert max(diffs.values()) <= ESTIMATE_RTOL, diffs


def test_estimate_state_and_bits(H):
    fx = ml.ESTIMATE_FIXTURES[0]
    big, _ = _gps(fx)
    a = big.log_likelihood_estimate(n_probes=8, seed=3, gradient=True)
    hps, alpha, G = big._hps, big._alpha, big._G
    alpha_bits, G_bits = alpha.clone(), G.clone()
    theta = big.hyperparameters * np.array([1.1, 0.9, 1.05])
    b = big.log_likelihood_estimate(theta, n_probes=8, seed=3, gradient=True)
    assert big._hps is hps and big._alpha is alpha and big._G is G
    assert bool((big._alpha == alpha_bits).all()) and bool((big._G == G_bits).all())
    assert b["log_likelihood"] != a["log_likelihood"]
    # the same call, the same bits; through the object's own state too
    b2 = big.log_likelihood_estimate(theta, n_probes=8, seed=3, gradient=True)
    a2 = big.log_likelihood_estimate(n_probes=8, seed=3, gradient=True)
    for first, second in ((a, a2), (b, b2)):
        for k in ("log_likelihood", "logdet", "std_error", "data_fit"):
            assert first[k] == second[k], k
        assert np.array_equal(first["per_probe"], second["per_probe"]) and np.array_equal(first["neg_gradient"], second["neg_gradient"])
    other = big.log_likelihood_estimate(n_probes=8, seed=4)
    assert other["logdet"] != a["logdet"] and other["data_fit"] == a["data_fit"]
    assert "neg_gradient" not in other
    # 20 probes go through the solver as 16 + 4, and the first 8 are the 8 above
    more = big.log_likelihood_estimate(n_probes=20, seed=3)
    assert np.array_equal(more["per_probe"][:8], a["per_probe"]) and more["per_probe"].shape == (20,)
    # the wrappers
    v, g = big.stochastic_neg_log_likelihood_and_gradient(n_probes=8, seed=3)
    assert v == -a["log_likelihood"] and np.array_equal(g, a["neg_gradient"])
    assert big.stochastic_log_likelihood(n_probes=8, seed=3) == a["log_likelihood"]
    assert big.stochastic_neg_log_likelihood(theta, n_probes=8, seed=3) == -b["log_likelihood"]
    assert np.array_equal(big.stochastic_neg_log_likelihood_gradient(theta, n_probes=8, seed=3), b["neg_gradient"])


def test_estimate_warns_when_probes_do_not_converge_and_raises_on_breakdown(H):
    import fvgp_amd
    from fvgp_amd.gp_lin_alg import NonPositiveDefiniteError
    fx = ml.ESTIMATE_FIXTURES[0]
    f = mf.fixture(fx)
    x, y, V = np.array(f["x"][:300]), ml.fixture_y(fx)[:300], np.array(f["V"][:300])
    slow = fvgp_amd.MatrixFreeGP(x, y, np.array(f["theta"]), noise_variances=V, kernel_function=f["kernel"],
                                 args={"max_iter": 2, "precond_rank": 0, "tol": 1e-10})
    with pytest.warns(UserWarning, match="did not converge"):
        out = slow.log_likelihood_estimate(n_probes=4)
    assert out["converged"] is False and np.all(out["lanczos_steps"] == 2)
    bad = fvgp_amd.MatrixFreeGP(x, y, np.array([-1.0, 0.3, 0.3]), noise_variances=1e-6 * V, kernel_function=f["kernel"],
                                args={"precond_rank": 0})
    with pytest.raises(NonPositiveDefiniteError):
        bad.log_likelihood_estimate(n_probes=4)


# ---- 6. training --------------------------------------------------------------------------------------------------------------------------------
def test_train_stochastic_lowers_the_exact_likelihood(H):
    """n = 600, d = 2, Matern-5/2, data drawn from a known theta; 30 Adam steps from 1.5 theta: the EXACT dense negative log-likelihood at
    the final theta is below the one at the start, and every iterate stays inside the bounds"""
    import fvgp_amd
    rng = np.random.default_rng(600)
    n, d = 600, 2
    theta = np.array([1.0, 0.3, 0.4])
    x = rng.random((n, d))
    V = np.full(n, 0.01)
    K = mf.k_double("matern52_ard", x, theta) + np.diag(V)
    y = np.linalg.cholesky(K) @ rng.standard_normal(n)
    start = 1.5 * theta
    bounds = np.array([[0.1, 10.0], [0.05, 0.59], [0.05, 5.0]])          # the second length scale's bound is close: clipping is exercised
    start = np.clip(start, bounds[:, 0], bounds[:, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dense = fvgp_amd.GP(x, y, init_hyperparameters=start, noise_variances=V, kernel_function="matern52_ard")
    big = fvgp_amd.MatrixFreeGP(x, y, start, noise_variances=V, kernel_function="matern52_ard")
    seen = []
    got, history = big.train_stochastic(bounds, max_iter=30, lr=1e-2, tolerance=1e-8, n_probes=16, seed=1,
                                        callback=lambda th, fval, g, t: seen.append(th.copy()))
    assert len(history["nlml"]) == 30 and len(seen) == 30
    assert np.array_equal(big.hyperparameters, got) and big._alpha is None
    for th in seen + [got]:
        assert np.all(th >= bounds[:, 0]) and np.all(th <= bounds[:, 1])
    before, after = float(dense.neg_log_likelihood(hyperparameters=start)), float(dense.neg_log_likelihood(hyperparameters=got))
    print("exact negative log-likelihood: start", before, "after 30 steps", after, "theta", got, "drawn from", theta)
    assert after < before
    assert history["nlml"][-1] < history["nlml"][0]


# ---- 7. the fvgp.GP method names ------------------------------------------------------------------------------------------------------------------
def test_opt_in_for_the_gp_method_names(H):
    import fvgp_amd
    fx = ml.ESTIMATE_FIXTURES[1]
    f = mf.fixture(fx)
    x, y, V = np.array(f["x"]), ml.fixture_y(fx), np.array(f["V"])
    plain, _ = _gps(fx)
    for call in (plain.log_likelihood, plain.neg_log_likelihood, plain.neg_log_likelihood_gradient, plain.train, plain.neg_log_likelihood_hessian):
        with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
            call()
    with pytest.raises(NotImplementedError, match="stochastic_likelihood"):
        plain.log_likelihood()
    opted = fvgp_amd.MatrixFreeGP(x, y, np.array(f["theta"]), noise_variances=V, kernel_function=f["kernel"],
                                  args={"stochastic_likelihood": True})
    e = plain.log_likelihood_estimate(gradient=True)
    assert opted.log_likelihood() == e["log_likelihood"] == -opted.neg_log_likelihood()
    assert np.array_equal(opted.neg_log_likelihood_gradient(), e["neg_gradient"])
    assert opted.log_likelihood(np.array(f["theta"]) * 1.05) == plain.stochastic_log_likelihood(np.array(f["theta"]) * 1.05)
    with pytest.raises(NotImplementedError, match="dense fvgp_amd.GP"):
        opted.neg_log_likelihood_hessian()
    bounds = np.array([[0.1, 10.0], [0.01, 10.0]])
    got = opted.train(hyperparameter_bounds=bounds, max_iter=2)
    assert got.shape == (2,) and np.array_equal(opted.hyperparameters, got) and not np.array_equal(got, f["theta"])


# ---- 8. refused arguments -------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(H):
    """one case per documented code of the four entries; nothing is launched and no buffer is touched"""
    from fvgp_amd import _lib
    L = _lib.lib()
    fx = mf.FIXTURES[0]
    f = mf.fixture(fx)
    n, d = f["x"].shape
    xd, Vd, G, C, _ = _dev(H, fx)
    th = np.ascontiguousarray(f["theta"])
    tp = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    bbig, B = _framed(H, (n, 4))
    ybig, Y = _framed(H, (n, 4))
    work = H.empty(max(_lib.pcg_lanczos_workspace_bytes(n, mf.RANK, 64), _lib.kgrad_form_workspace_bytes(n, n),
                       _lib.precond_apply_workspace_bytes(n, mf.RANK)) // 8)
    wb = work.numel() * 8
    h = H._h
    out = np.full(8, CANARY)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def form(**kw):
        a = dict(h=h, kid=0, x1=P(xd), n1=n, x2=P(xd), n2=n, d=d, th=tp, nt=len(th), U=P(B), ldu=B.stride(0), W=P(Y), ldw=Y.stride(0), s=4,
                 w=P(work), wb=wb, out=op)
        a.update(kw)
        return L.fvgp_hip_kgrad_form(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=6)), (-3, dict(x1=None)), (-4, dict(n1=0)), (-5, dict(x2=None)), (-6, dict(n2=0)),
                     (-7, dict(d=17)), (-8, dict(th=None)), (-9, dict(nt=1)), (-10, dict(U=None)), (-11, dict(ldu=3)), (-12, dict(W=None)),
                     (-13, dict(ldw=3)), (-14, dict(s=0)), (-14, dict(s=17, ldu=17, ldw=17)), (-15, dict(w=None)),
                     (-15, dict(w=ctypes.c_void_p(work.data_ptr() + 4))), (-16, dict(wb=64)), (-17, dict(out=None))):
        assert form(**kw) == code, (code, kw)
    assert np.all(out == CANARY)

    def probes(**kw):
        a = dict(h=h, seed=1, stream=0, col0=0, G=P(G), ldg=G.stride(0), q=mf.RANK, n=n, v=P(Vd), Z=P(Y), ldz=Y.stride(0), s=4)
        a.update(kw)
        return L.fvgp_hip_precond_probes(*a.values())
    for code, kw in ((-1, dict(h=None)), (-3, dict(stream=1 << 63)), (-4, dict(col0=-1)), (-4, dict(col0=(1 << 32) - 3)), (-6, dict(ldg=n - 1)),
                     (-7, dict(q=-1)), (-7, dict(q=_lib.PCG_MAX_RANK + 1)), (-8, dict(n=0)), (-9, dict(v=None)), (-10, dict(Z=None)),
                     (-11, dict(ldz=3)), (-12, dict(s=0)), (-12, dict(s=17, ldz=17))):
        assert probes(**kw) == code, (code, kw)

    def apply(**kw):
        a = dict(h=h, G=P(G), ldg=G.stride(0), q=mf.RANK, C=P(C), ldc=C.stride(0), n=n, v=P(Vd), R=P(B), ldr=B.stride(0), s=4, W=P(Y),
                 ldw=Y.stride(0), w=P(work), wb=wb)
        a.update(kw)
        return L.fvgp_hip_precond_apply(*a.values())
    for code, kw in ((-1, dict(h=None)), (-3, dict(ldg=n - 1)), (-4, dict(q=-1)), (-4, dict(q=_lib.PCG_MAX_RANK + 1)), (-5, dict(C=None)),
                     (-6, dict(ldc=127)), (-7, dict(n=0)), (-8, dict(v=None)), (-9, dict(R=None)), (-10, dict(ldr=3)), (-11, dict(s=0)),
                     (-11, dict(s=17, ldr=17, ldw=17)), (-12, dict(W=None)), (-13, dict(ldw=3)), (-14, dict(w=None)), (-15, dict(wb=64))):
        assert apply(**kw) == code, (code, kw)

    it = (ctypes.c_int * 16)()
    st = (ctypes.c_int * 16)()
    rr = (ctypes.c_double * 16)()
    steps = (ctypes.c_int * 16)()
    rho0 = (ctypes.c_double * 16)()
    al = (ctypes.c_double * (16 * 64))()
    be = (ctypes.c_double * (16 * 64))()

    def cg(**kw):
        a = dict(h=h, kid=0, x=P(xd), n=n, d=d, th=tp, nt=len(th), v=P(Vd), G=P(G), ldg=G.stride(0), q=mf.RANK, C=P(C), ldc=C.stride(0),
                 B=P(B), ldb=B.stride(0), s=4, X=P(Y), ldx=Y.stride(0), warm=0, tol=1e-9, max_iter=10, check_every=8, max_restarts=3,
                 w=P(work), wb=wb, it=it, rr=rr, st=st, L=64, al=al, be=be, steps=steps, rho0=rho0)
        a.update(kw)
        return L.fvgp_hip_pcg_lanczos(*a.values())
    for code, kw in ((-1, dict(h=None)), (-2, dict(kid=6)), (-3, dict(x=None)), (-4, dict(n=0)), (-5, dict(d=17)), (-6, dict(th=None)),
                     (-7, dict(nt=1)), (-8, dict(v=None)), (-10, dict(ldg=n - 1)), (-11, dict(q=-1)), (-12, dict(C=None)), (-13, dict(ldc=127)),
                     (-14, dict(B=None)), (-15, dict(ldb=3)), (-16, dict(s=0)), (-17, dict(X=None)), (-18, dict(ldx=3)), (-20, dict(tol=0.0)),
                     (-21, dict(max_iter=0)), (-22, dict(check_every=0)), (-23, dict(max_restarts=-1)), (-24, dict(w=None)),
                     (-25, dict(wb=_lib.pcg_workspace_bytes(n, mf.RANK))), (-26, dict(it=None)), (-27, dict(rr=None)), (-28, dict(st=None)),
                     (-29, dict(L=-1)), (-29, dict(L=_lib.LANCZOS_MAX_STEPS + 1)), (-30, dict(al=None)), (-31, dict(be=None)),
                     (-32, dict(steps=None)), (-33, dict(rho0=None))):
        assert cg(**kw) == code, (code, kw)
    H.sync()
    for big, shape in ((bbig, (n, 4)), (ybig, (n, 4))):
        assert _frame_untouched(big, shape)
    assert np.all(Y.cpu().numpy() == CANARY) and np.all(B.cpu().numpy() == CANARY)
