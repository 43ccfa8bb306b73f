"""Every path of the Cholesky factorisation (fvgp_hip_potrf, _potrf_dev, _panel_potrf_dev and the fused fvgp_hip_loglik; csrc/api.hip
potrf_driver / panel_factor_any, csrc/chain.hip, csrc/leaf.hip) against the extended-precision reference of tests/chol_ref.py, which
tests/test_chol_ref.py proves on the host -- on the easy matrix the older tests use (W, cond_2 = 5), on RBF covariances (G: noise 1e-6,
cond_2 = 2.4e7; H: noise 1e-8, 8.0e9) and on power-of-two scalings of G (S: D G D with D = 2^-20 .. 2^20; U: 2^-400 G and 2^400 G).

The matrix is uploaded into a buffer of padded_dim(n) rows whose strict upper triangle (inside the diagonal blocks too) and whose
padding rows are NaN on entry; a leading dimension above the minimum is a strided view into a wider NaN-filled tensor.

On every case: (a) beta, the componentwise backward error |A - L L^T| / (|L||L|^T) in units of eps over at most 24 complete rows (both
sides of the tile, block and panel boundaries of the case, the last rows, random ones) and the whole diagonal; (b) phi, the relative
2-norm error of every row of L against the longdouble factor; (c) lam, the error of 2 sum log L_ii (fvgp_hip_logdet, and the device
value of potrf_dev); (d) info = 0; (e) the strict upper triangle and every column beyond padded_dim(n) keep their bits and L is finite,
so the NaN was never read; (f) the padding rows come back as identity; (g) a second identical call gives the same bits; (h) potrs with
one right-hand side agrees with scipy to 64 eps cond_2(A), so the block inverses belong to this factor.

Bars, none of them from the device.  Derived caps: beta <= 2 (n + 1) where the panel solve X = P inv(L_kk)^T is a substitution over
16 x 16 tiles with the tile inverses, times max_k cond_2(Lhat_kk) where it is a product with the explicit 128 x 128 inverse; phi <=
64 eps cond_2(A); lam <= n eps cond_2(A).  Measured bars: 8 max(scipy's LAPACK, the float64 twin of the path's panel solve, floor) on the
same rows against the same longdouble factor, floor = 4 (beta), 4 eps (phi), eps (n + sum |log Lhat_ii|) (lam).

Every case prints `CH|path|family|n|beta dev/scipy/twin|phi ...|lam ...|ratios` (pytest -s)."""
import contextlib

import numpy as np
import pytest
import scipy.linalg as sla

import chol_ref as cr
import tri_solve_ref as ref

pytestmark = pytest.mark.gpu

EPS, LD = cr.EPS, cr.LD
N = 1300                    # padded_dim 1408, 11 block columns: the smallest size with three panels of 512
# csrc/common.h: every key a case of this module sets, and the library's default
DEFAULTS = dict(outer_block=1024, outer_block_big=2048, big_threshold=24576, inner_block=512, lookahead=1, leaf_tiles=1, leaf_tiles_rows=4096,
                panel_recursive=1, panel_chain=1, panel_chain_min=4096, outer_block_small=512, small_threshold=12288, lookahead_min=1 << 40,
                cols_split=1, cols_split_rows=8192, chain_wide=1, wide_block=4096, wide_block_big=4096, wide_threshold=1 << 30, wide_inner=2048,
                wide_inner_rows=16384, chain_ahead=0, chain_single_rows=80, chain_sleep_rows=96)
B256 = (256, 512, 768, 1024, 1280)
_LA = dict(chain_wide=0, lookahead_min=0, outer_block=256, outer_block_big=0, outer_block_small=0, panel_chain_min=0)
# name -> (options, twins whose larger figure is the measured bar, panel boundaries at padded_dim 1408).  Why each option set reaches the
# path named (api.hip potrf_driver = D, panel_factor_any = P, panel_factor = F, trailing_update = T; chain.hip launch_panel_chain = C):
PATHS = {
    # D: `wide` (panel_chain && chain_wide && np < lookahead_min) gives ONE panel of wide_block = 4096 >= np, la is false, chain_alone = 1;
    # P: chain_alone && chain_wide -> C; 11 block rows <= chain_single_rows: one workgroup per compute unit.  The resident kernel solves by
    # tile substitution (chain.hip trsm_sub / the follow mode): twin 16.
    "1 default": ({}, (16,), ()),
    # D: `wide` with wide_block 512 -> panels [0, 512), [512, 1024), [1024, 1408); each C over every row below, then timed_update with
    # K = 512 (T: 28 and 6 tiles but K < 1024: no split)
    "2 wide 512": (dict(wide_block=512, wide_block_big=512), (16,), (512, 1024)),
    # D: panels [0, 1024), [1024, 1408); T: the one update has M = N = 384: 6 tiles <= 64, K = 1024 >= 1024, role 1, chain_alone && chain_wide:
    # split = min(256 / 6, 1024 / 512) = 2
    "3 split-K": (dict(wide_block=1024, wide_block_big=1024), (16,), (1024,)),
    # P: chain_alone, inner = 256 > 0, Jend - J0 = 1024 (384) > inner, np - J0 >= wide_inner_rows = 0: C per 256 columns, T with role 0 between
    "4 sub-panels": (dict(wide_block=1024, wide_block_big=1024, wide_inner=256, wide_inner_rows=0), (16,), B256),
    # C: rows <= chain_single_rows is false (pad_lds = 0: several workgroups per compute unit), sleep_rows = 0: no product yields
    "5 tall mode": (dict(chain_single_rows=0, chain_sleep_rows=0), (16,), ()),
    # C: chain_alone == 1 && n2 == rows: g.ahead = chain_ahead
    "5 tall mode ahead 3": (dict(chain_single_rows=0, chain_sleep_rows=0, chain_ahead=3), (16,), ()),
    # schedule 2: chain_wide = 0, panel_chain = 0, lookahead_min = 4608 > np: la false, panels of outer_block_small = 512 (np <=
    # small_threshold); P: panel_chain == 0 -> panel_factor_nested -> recursive halving down to F per 128 columns; F: leaf_tiles && R <= 1280
    # <= leaf_tiles_rows = 4096 -> launch_trsm_tiles (substitution with the tile inverses): twin 16
    "6 steps": (dict(schedule=2), (16,), (512, 1024)),
    # panel_factor_nested with panel_recursive = 0: F over sub-panels of inner_block = 256 < 512, T role 0 between
    "6 steps inner 256": (dict(schedule=2, panel_recursive=0, inner_block=256), (16,), B256),
    # F: tiles = 0 -> `launch_gemm(... P, lda, h->linv + kb * LEAF_DOUBLES ...)`, the product with the explicit 128-inverse: twin 128
    "6 steps explicit": (dict(schedule=2, leaf_tiles=0), (128,), (512, 1024)),
    # F: tiles = (R <= 512): the product with the explicit inverse for the block columns 0 .. 5, substitution for 6 .. 9: the larger twin
    "6 steps switch 512": (dict(schedule=2, leaf_tiles_rows=512), (16, 128), (512, 1024)),
    # D: chain_wide = 0 -> not `wide`: panels of 512, la false (np < lookahead_min), chain_alone = 1; P: panel_chain && np - J0 >= 0 -> C per panel
    "7 resident per panel": (dict(chain_wide=0, panel_chain=1, panel_chain_min=0), (16,), (512, 1024)),
    # D: six panels of 256 (big and small widths off), la = lookahead && npan > 2 && np >= 0, chain_alone = 0; can_split where the two
    # streams run side by side: the next panel's square is updated first, C with cols_tag, the rows below beside it.  can_split also
    # needs chain_streams_concurrent(h) == 1, a probe at run time that the test cannot read: on a machine where it returns 0 this case
    # is the same as "8 look-ahead" below.  (Either way every tile is updated once with the same K, so equal figures for the two cases
    # do not tell which route ran.)
    "8 look-ahead split": (dict(_LA, cols_split=1, cols_split_rows=100000), (16,), B256),
    # the whole column update (timed_update) before P -> C on the side stream
    "8 look-ahead": (dict(_LA, cols_split=0), (16,), B256),
    # P: panel_chain == 0 -> panel_factor_nested on the side stream (F: substitution, as path 6)
    "8 look-ahead steps": (dict(_LA, panel_chain=0), (16,), B256),
}
SCALED_PATHS = ("1 default", "6 steps")
SIZE_PATHS = ("1 default", "6 steps", "6 steps explicit")
SIZES = (1, 2, 16, 17, 127, 128, 129, 1281, 1408)       # 1281: one valid row in the last block; 1408: no padding


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@contextlib.contextmanager
def _schedule(H, opts):
    """sets a case's options (`schedule` first: it writes four of the other keys) and puts EVERY schedule key back to the library
    default afterwards: the handle is shared by the module"""
    try:
        if "schedule" in opts:
            H.set_option("schedule", opts["schedule"])
        for k, v in opts.items():
            if k != "schedule":
                H.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            H.set_option(k, v)
        H.set_option("schedule", 0)


class _Record:
    """collects a test's figures (printed whether they pass or not) and its failed checks (asserted at the end)"""

    def __init__(self):
        self.lines, self.fails = [], []

    def check(self, ok, path, what):
        if not ok:
            self.fails.append(f"{path}: {what}")

    def measure(self, path, fam, n, kind, dev, e_sp, e_tw, floor, cap, unit=""):
        """one of beta / phi / lam under its cap and its measured bar; returns the text of the figure and the ratio"""
        base = max(e_sp, e_tw, floor)
        self.check(dev <= cap, f"{path} {fam} n={n}", f"{kind} {dev:.3g} above the derived cap {cap:.3g}")
        self.check(dev <= 8 * base, f"{path} {fam} n={n}", f"{kind} {dev:.3g} above 8 x max(scipy {e_sp:.3g}, twin {e_tw:.3g}, floor {floor:.3g}) = {8 * base:.3g}")
        return f"{kind} {dev:.3g}/{e_sp:.3g}/{e_tw:.3g}", dev / base

    def line(self, path, fam, n, figs):
        self.lines.append(f"CH|{path}|{fam}|{n}|" + "|".join(f for f, _ in figs) + "|ratios " + " ".join(f"{r:.3g}" for _, r in figs))

    def finish(self):
        for ln in self.lines:
            print(ln)
        assert not self.fails, "\n".join(self.fails[:40])


# ---- device buffers ------------------------------------------------------------------------------------------------------------------
def _image(A, n, extra=0, identity=False):
    """host image of the matrix buffer: padded_dim(n) rows, the lower triangle of A, NaN everywhere else -- the strict upper triangle
    (inside the diagonal blocks too), the padding rows (fvgp_hip_potrf writes the identity there itself; identity = True: the caller
    supplies it) and the `extra` columns beyond padded_dim(n)"""
    from fvgp_amd._lib import pad128
    npad = pad128(n)
    buf = np.full((npad, npad + extra), np.nan)
    il = np.tril_indices(n)
    buf[:n, :n][il] = A[il]
    if identity:
        pl = np.tril_indices(npad)
        keep = pl[0] >= n
        buf[pl[0][keep], pl[1][keep]] = 0.0
        buf[np.arange(n, npad), np.arange(n, npad)] = 1.0
    return buf


def _upload(H, img, npad):
    wide = H.to_device(img)
    view = wide[:, :npad]
    assert view.stride(0) == img.shape[1]
    return wide, view


def _outside_kept(got, img, npad):
    """(e): the strict upper triangle of the npad x npad square and every column beyond it, bit for bit"""
    iu = np.triu_indices(npad, 1)
    return got[:, :npad][iu].tobytes() == img[:, :npad][iu].tobytes() and got[:, npad:].tobytes() == img[:, npad:].tobytes()


def _padding_is_identity(got, n, npad):
    pad = got[n:npad, :npad]
    rows = np.arange(n, npad)
    return bool(np.all(np.tril(pad, n - 1) == 0.0)) and bool(np.all(pad[rows - n, rows] == 1.0))


_SOLVES = {}


def _solve_ref(fam, n):
    """(b, scipy's float64 solution of G-or-whatever x = b): the scaled families solve D A_G D x = D b, whose solution is D^-1 x_G"""
    base = "G" if cr.row_scale(fam, n) is not None else fam
    if (base, n) not in _SOLVES:
        A = cr.reference(base, n).A
        b = np.random.default_rng(n + 1).standard_normal(n)
        _SOLVES[(base, n)] = (b, sla.cho_solve(sla.cho_factor(A, lower=True), b))
    return _SOLVES[(base, n)]


def _potrf_once(H, img, n, npad, rhs=None):
    """one fvgp_hip_potrf on a fresh upload: (info, the whole buffer as it came back, fvgp_hip_logdet, potrs of rhs)"""
    wide, view = _upload(H, img, npad)
    info = H.potrf(view, n)
    logdet, x = float("nan"), None
    if info == 0:
        logdet = H.logdet(view, n)
        if rhs is not None:
            b = np.zeros((npad, 1))
            b[:n, 0] = rhs
            B = H.to_device(b)
            H.potrs(view, n, B, 1)
            H.sync()
            x = B.cpu().numpy()[:n, 0]
    H.sync()
    return info, wide.cpu().numpy(), logdet, x


def _judge(rec, path, fam, n, R, twins, bounds, got, img, npad, info, logdets, x=None, ncols=None, nlog=None, seed=0):
    """checks (a) .. (f) and (h) on one factor as it came back; logdets: {name: value} of 2 sum log L_ii over the first nlog rows.
    Returns the lower triangle (n x n, zeros above)."""
    tag = f"{path} {fam} n={n}"
    w = n if ncols is None else ncols
    rec.check(info == 0, tag, f"(d) info = {info}")
    rec.check(_outside_kept(got, img, npad), tag, "(e) an entry above the diagonal or beyond padded_dim(n) changed")
    L = np.tril(got[:n, :n])
    L[:, w:] = 0.0
    finite = bool(np.all(np.isfinite(L)))
    rec.check(finite, tag, "(e) L is not finite")
    if ncols is None:
        rec.check(_padding_is_identity(got, n, npad), tag, "(f) the padding rows are not identity")
    rows = cr.edge_rows(n, [b for b in bounds if b < n], seed)
    explicit = 128 in twins
    figs = []
    b_tw = max(R.beta(t, rows, ncols) for t in twins)
    figs.append(rec.measure(path, fam, n, "beta", cr.beta(R.A, L, rows, ncols), R.beta("scipy", rows, ncols), b_tw, 4.0, R.cap_beta(explicit)))
    p_tw = max(R.phi(t, ncols) for t in twins)
    figs.append(rec.measure(path, fam, n, "phi", cr.phi(L, R.Lhat, ncols), R.phi("scipy", ncols), p_tw, 4 * EPS, R.cap_phi()))
    nl = w if nlog is None else nlog
    l_tw = max(R.lam(t, nl) for t in twins)
    for name, value in logdets.items():
        figs.append(rec.measure(path, fam, n, f"lam({name})", cr.lam_value(value, R.Lhat, nl), R.lam("scipy", nl), l_tw, cr.lam_floor(R.Lhat, nl), R.cap_lam()))
    if x is not None:
        D = cr.row_scale(fam, n)
        _, want = _solve_ref(fam, n)
        xs = x if D is None else D * x
        err = float(np.linalg.norm(xs - want) / np.linalg.norm(want)) if np.all(np.isfinite(xs)) else np.inf
        rec.check(err <= 64 * EPS * R.cond, tag, f"(h) potrs is {err:.3g} from scipy, above 64 eps cond = {64 * EPS * R.cond:.3g}")
    rec.line(path, fam, n, figs)
    return L


def _factor_and_judge(H, rec, path, fam, n, twins, bounds, extra=0):
    """fvgp_hip_potrf twice on fresh uploads of the family's matrix, every check; returns the lower triangle"""
    from fvgp_amd._lib import pad128
    R = cr.reference(fam, n)
    npad = pad128(n)
    img = _image(R.A, n, extra)
    D = cr.row_scale(fam, n)
    b, _ = _solve_ref(fam, n)
    info, got, logdet, x = _potrf_once(H, img, n, npad, b if D is None else D * b)
    info2, again, _, _ = _potrf_once(H, img, n, npad)
    rec.check(info2 == info and got.tobytes() == again.tobytes(), f"{path} {fam} n={n}", "(g) a second identical call gives other bits")
    name = path + (f" ld+{extra}" if extra else "")
    return _judge(rec, name, fam, n, R, twins, bounds, got, img, npad, info, {"logdet": logdet}, x, seed=n)


# ---- paths 1 .. 8 at n = 1300 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["W", "G", "H"])
@pytest.mark.parametrize("path", list(PATHS))
def test_path(H, path, fam):
    """fvgp_hip_potrf at n = 1300 under the option set of PATHS[path] (the comment there says which condition routes it); on G once more
    with a leading dimension 128 above the minimum, which must give the same bits"""
    opts, twins, bounds = PATHS[path]
    rec = _Record()
    with _schedule(H, opts):
        L = _factor_and_judge(H, rec, path, fam, N, twins, bounds)
        if fam == "G":
            Lw = _factor_and_judge(H, rec, path, fam, N, twins, bounds, extra=128)
            rec.check(L.tobytes() == Lw.tobytes(), f"{path} {fam}", "the leading dimension changes the bits of L")
    rec.finish()


@pytest.mark.parametrize("fam", ["S", "U-", "U+"])
@pytest.mark.parametrize("path", SCALED_PATHS)
def test_scaled_matrix_gives_the_scaled_factor(H, path, fam):
    """D G D (S: D = 2^-20 .. 2^20 row by row) and 2^-400 G, 2^400 G: beta and phi are invariant under the scaling and keep their bars
    (Lhat = D Lhat(G), exactly), and L equals D L(G) of the same path bit for bit: no step of the factorisation depends on the data"""
    from fvgp_amd._lib import pad128
    opts, twins, bounds = PATHS[path]
    rec = _Record()
    with _schedule(H, opts):
        L = _factor_and_judge(H, rec, path, fam, N, twins, bounds)
        info, got, _, _ = _potrf_once(H, _image(cr.reference("G", N).A, N), N, pad128(N))
        Lg = np.tril(got[:N, :N])
        D = cr.row_scale(fam, N)
        same = info == 0 and L.tobytes() == (D[:, None] * Lg).tobytes()
        print(f"CH|{path}|{fam}|{N}|bits equal to the scaled factor of G: {same}")
        rec.check(same, f"{path} {fam}", "L is not the scaled L of G bit for bit")
    rec.finish()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(H, n):
    """H at the smallest legal sizes, around the 16-tile and the 128-block, with one valid row in the last block (1281) and without
    padding (1408), under the default path, the launch-per-step path and its explicit-inverse variant"""
    rec = _Record()
    for path in SIZE_PATHS:
        opts, twins, bounds = PATHS[path]
        with _schedule(H, opts):
            _factor_and_judge(H, rec, path, "H", n, twins, bounds)
    rec.finish()


# ---- path 9: fvgp_hip_potrf_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["G", "H"])
def test_potrf_dev(H, fam):
    """info and log-det stay on the device (n_logdet = n and n - 5; once with a leading dimension 128 above the minimum); the default
    schedule, so the whole buffer is bit-identical to path 1.  potrs follows every call: the block inverses and the factor they are
    cached for (linv_L, set by the enqueue-only branch of potrf_driver) belong to this factor."""
    import torch
    from fvgp_amd._lib import pad128
    rec = _Record()
    R = cr.reference(fam, N)
    npad = pad128(N)
    b, _ = _solve_ref(fam, N)
    with _schedule(H, {}):
        for nlog, extra in ((N, 0), (N - 5, 0), (N, 128)):
            img = _image(R.A, N, extra)
            _, base, _, _ = _potrf_once(H, img, N, npad)
            wide, view = _upload(H, img, npad)
            info = torch.full((1,), 7, dtype=torch.int32, device=view.device)
            ld = H.to_device(np.full(1, np.nan))
            H.potrf_dev(view, N, nlog, info, ld)
            rhs = np.zeros((npad, 1))
            rhs[:N, 0] = b
            B = H.to_device(rhs)
            H.potrs(view, N, B, 1)
            H.sync()
            got, x = wide.cpu().numpy(), B.cpu().numpy()[:N, 0]
            name = f"9 potrf_dev n_logdet={nlog}" + (f" ld+{extra}" if extra else "")
            rec.check(got.tobytes() == base.tobytes(), f"{name} {fam}", "the buffer differs in bits from fvgp_hip_potrf (path 1)")
            _judge(rec, name, fam, N, R, (16,), (), got, img, npad, int(info.item()),
                   {"device": float(ld.item()), "logdet": H.logdet(view, nlog)}, x, nlog=nlog, seed=N)
    rec.finish()


# ---- path 10: fvgp_hip_panel_potrf_dev --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [1, 2, 0])
def test_panel_potrf_dev(H, chain):
    """T = the first 512 columns of the padded H (all 1408 rows, ldt = 1408, n_valid = 512): the result is Lhat[:, :512], so the reference
    is free.  panel_chain 1: the resident kernel with a workgroup per block, 2: not alone, 0: api.hip panel_factor_nested -> panel_factor
    with leaf_tiles and R <= leaf_tiles_rows -> launch_trsm_tiles.  All three substitute: twin 16."""
    import torch
    from fvgp_amd._lib import pad128
    rec = _Record()
    R = cr.reference("H", N)
    npad, w = pad128(N), 512
    img = _image(R.A, N, identity=True)
    outs = []
    with _schedule(H, dict(panel_chain=chain)):
        for _ in range(2):
            wide, view = _upload(H, img, npad)
            info = torch.full((1,), 9, dtype=torch.int32, device=view.device)
            ld = H.to_device(np.full(1, np.nan))
            H.panel_potrf_dev(wide[:, :w], w, npad, w, info, ld)
            H.sync()
            outs.append((wide.cpu().numpy(), int(info.item()), float(ld.item())))
    got, info, logdet = outs[0]
    tag = f"10 panel_potrf_dev panel_chain={chain}"
    rec.check(outs[1][0].tobytes() == got.tobytes() and outs[1][1:] == outs[0][1:], tag, "(g) a second identical call gives other bits")
    rec.check(got[:, w:].tobytes() == img[:, w:].tobytes(), tag, "(e) columns beyond the panel changed")
    rec.check(bool(np.all(got[N:, :w] == 0.0)), tag, "the panel's padding rows are not zero")
    _judge(rec, tag, "H", N, R, (16,), (), got, img, npad, info, {"device": logdet}, ncols=w, seed=N)
    rec.finish()


def test_panel_potrf_dev_identity_padding_inside_the_panel(H):
    """w = 512, n_valid = 500, the identity on the 12 padding rows supplied by the caller: the leading 500 x 500 of G at n = 1300 (the
    covariance of its first 500 points), so the reference is the leading 500 rows of Lhat(G, 1300)"""
    import torch
    rec = _Record()
    n, w = 500, 512
    big = cr.reference("G", N)
    A = np.array(big.A[:n, :n])
    R = cr.Reference(A, Lhat=np.array(big.Lhat[:n, :n]))
    assert cr.phi(cr.chol_ld(A), R.Lhat) <= 4 * cr.EPS_LD * n
    img = _image(A, n, identity=True)
    wide, view = _upload(H, img, w)
    info = torch.full((1,), 9, dtype=torch.int32, device=view.device)
    ld = H.to_device(np.full(1, np.nan))
    with _schedule(H, {}):
        H.panel_potrf_dev(view, w, w, n, info, ld)
        H.sync()
    got = wide.cpu().numpy()
    _judge(rec, "10 panel_potrf_dev n_valid=500", "G", n, R, (16,), (), got, img, w, int(info.item()), {"device": float(ld.item())}, seed=n)
    rec.finish()


# ---- info ---------------------------------------------------------------------------------------------------------------------------------
BAD_DIAGONALS = (1, 4, 5, 16, 17, 128, 129, 512, 513, 1299, 1300)
NAN_PAIRS = ((277, 274), (350, 290), (900, 300))        # inside one 16-tile, inside one 128-block, across panels


def _lapack_info(A):
    return int(sla.lapack.dpotrf(np.tril(A), lower=1, clean=0, overwrite_a=0)[1])


def _broken_matrices(n, fit=None):
    """(what, matrix, expected info, compare with LAPACK) on W: a negative diagonal at p, a pivot that only fails after the updates, two
    bad diagonals, a NaN below the diagonal.  fit: only positions up to this column (a panel)."""
    lim = n if fit is None else fit
    out = []
    if n != N:                           # (no padding rows at n = 1408: the last pivot of the last block)
        A = cr.matrix("W", n)
        A[n - 1, n - 1] = -3.0
        return [(f"n = {n}: A[{n - 1},{n - 1}] = -3", A, n, True)]
    R = cr.reference("W", n)
    for p in BAD_DIAGONALS:
        if p <= lim:
            A = np.array(R.A)
            A[p - 1, p - 1] = -3.0
            out.append((f"A[{p - 1},{p - 1}] = -3", A, p, True))
    for p in (130, 700):                 # the pivot becomes -Lhat_pp^2 once the columns before it are applied: far from rounding
        if p <= lim:
            A = np.array(R.A)
            A[p - 1, p - 1] -= 2.0 * float(R.Lhat[p - 1, p - 1]) ** 2
            out.append((f"pivot {p} fails after the updates", A, p, True))
    second = 901 if fit is None else 401
    A = np.array(R.A)
    A[200, 200] = A[second - 1, second - 1] = -3.0
    out.append((f"bad diagonals at 201 and {second}", A, 201, True))
    for i, j in NAN_PAIRS if fit is None else ((277, 274), (350, 290), (450, 100)):
        A = np.array(R.A)
        A[i, j] = np.nan                 # every pivot before i + 1 is computed from finite entries (OpenBLAS reports 0 here: no comparison)
        out.append((f"NaN at A[{i},{j}]", A, i + 1, False))
    return out


INFO_PATHS = ("1 default", "2 wide 512", "6 steps", "8 look-ahead split")


@pytest.mark.parametrize("path", INFO_PATHS)
def test_info(H, path):
    """info = the order of the first leading minor that is not positive, as LAPACK's dpotrf (a NaN below the diagonal at (i, j): i + 1);
    after every failed factorisation G factors on the same handle with info 0 and the bits it had before: flags, tags, the info word
    and the inverse cache are clean"""
    from fvgp_amd._lib import pad128
    rec = _Record()
    npad = pad128(N)
    gimg = _image(cr.reference("G", N).A, N)
    with _schedule(H, PATHS[path][0]):
        info, gbase, _, _ = _potrf_once(H, gimg, N, npad)
        assert info == 0
        cases = [(N,) + c for c in _broken_matrices(N)] + [(1408,) + c for c in _broken_matrices(1408)]
        for n, what, A, want, lapack in cases:
            if lapack:
                assert _lapack_info(A) == want, what
            info, _, _, _ = _potrf_once(H, _image(A, n), n, pad128(n))
            rec.check(info == want, f"{path} {what}", f"info = {info}, expected {want}")
            info, after, _, _ = _potrf_once(H, gimg, N, npad)
            rec.check(info == 0 and after.tobytes() == gbase.tobytes(), f"{path} after {what}", f"G: info {info}, same bits: {after.tobytes() == gbase.tobytes()}")
    print(f"CH|info|{path}|{len(cases)} broken matrices")
    rec.finish()


@pytest.mark.parametrize("entry", ["potrf_dev", "panel_potrf_dev"])
def test_info_stays_on_the_device(H, entry):
    """the same broken matrices through fvgp_hip_potrf_dev (the last pivot at n = 1408, without padding rows, included), and those that
    fit in the first 512 columns through fvgp_hip_panel_potrf_dev (T = those columns over all 1408 rows)"""
    import torch
    from fvgp_amd._lib import pad128
    rec = _Record()
    w = 512
    panel = entry == "panel_potrf_dev"

    def run(A):
        n = A.shape[0]
        npad = pad128(n)
        wide, view = _upload(H, _image(A, n, identity=panel), npad)
        info = torch.full((1,), 7, dtype=torch.int32, device=view.device)
        if panel:
            H.panel_potrf_dev(wide[:, :w], w, npad, w, info, None)
        else:
            H.potrf_dev(view, n, 0, info, None)
        H.sync()
        return int(info.item()), wide.cpu().numpy()

    with _schedule(H, {}):
        G = cr.reference("G", N).A
        info, gbase = run(G)
        assert info == 0
        cases = _broken_matrices(N, fit=w if panel else None) + ([] if panel else _broken_matrices(1408))
        for what, A, want, _ in cases:
            info, _ = run(A)
            rec.check(info == want, f"{entry} {what}", f"info = {info}, expected {want}")
            info, after = run(G)
            rec.check(info == 0 and after.tobytes() == gbase.tobytes(), f"{entry} after {what}", f"G: info {info}, same bits: {after.tobytes() == gbase.tobytes()}")
    print(f"CH|info|{entry}|{len(cases)} broken matrices")
    rec.finish()


# ---- the fused evaluation ---------------------------------------------------------------------------------------------------------------
_KMAT = {}


def _assembled(H, fam, n):
    """the matrix fvgp_hip_kmat assembles from the evaluation's arguments, downloaded, as a Reference (computed once per (family, n))"""
    from fvgp_amd import _lib
    if (fam, n) not in _KMAT:
        ell, noise = cr.PARAMS[fam]
        x = np.random.default_rng(cr.SEED).random((n, 2))
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * np.random.default_rng(cr.SEED + 1).standard_normal(n)
        y -= y.mean()
        theta = np.array([1.0, ell, ell])
        npad = _lib.pad128(n)
        K = H.to_device(np.full((npad, npad), np.nan))
        xd, vd = H.to_device(x), H.to_device(np.full(n, noise))
        H.kmat(0, xd, xd, theta, K, vdiag=vd, uplo=_lib.LOWER, pad=_lib.PAD_IDENTITY)
        H.sync()
        low = np.tril(K.cpu().numpy()[:n, :n])
        A = low + np.tril(low, -1).T
        assert np.max(np.abs(A - cr.matrix(fam, n))) <= 1e-11           # the same covariance as the fixture, up to the rounding of r^2
        _KMAT[(fam, n)] = (cr.Reference(A), x, y, theta, noise)
    return _KMAT[(fam, n)]


@pytest.mark.parametrize("fam", ["G", "H"])
@pytest.mark.parametrize("n,rows", [(1300, 1408), (1408, 1536), (1408, 1408)])
def test_fused_evaluation(H, fam, n, rows):
    """fvgp_hip_loglik, kernel id 0, on the points, length scale and noise of G and H, y = sin(3 sum x) + 0.1 N(0, 1), centred: the forward
    solve rides in appended rows through the panel solves of the default path -- in the padding rows (n = 1300), in an extra block row
    (n = 1408 with a scratch of loglik_dim = 1536 rows: np_force) or not at all (n = 1408 with padded_dim rows: a sweep of its own).
    The reference matrix is what fvgp_hip_kmat assembles from the same arguments: evaluate.hip fvgp_hip_loglik_rows fills a KmatDesc by
    kmat_desc_from_theta with uplo = FVGP_LOWER, pad = 1 and calls launch_kmat, the launch behind fvgp_hip_kmat(LOWER, PAD_IDENTITY).
    The L left in the scratch by (a) and (b), the log-det by (c); the quadratic form against |Lhat^-1 y|^2 in longdouble under
    8 max(scipy's, the twin's, 4 eps) relative; alpha against tri_solve_ref.potrs_ld on the device's own factor under the bars of the
    solves suite (cap 64 eps cond_2(L)^2; 8 max(scipy's cho_solve, the block-inverse twin at 128, 4 eps))."""
    from fvgp_amd import _lib
    rec = _Record()
    R, x, y, theta, noise = _assembled(H, fam, n)
    npad = _lib.pad128(n)
    assert _lib.loglik_dim(n, 1) == (1408 if n == 1300 else 1536)
    tag = f"loglik scratch {rows}"
    outs = []
    with _schedule(H, {}):
        for _ in range(2):
            KV = H.to_device(np.full((rows, rows), np.nan))
            alpha = H.to_device(np.full((npad, 1), np.nan))
            ll, logdet, quad, info = H.loglik(0, H.to_device(x), theta, H.to_device(np.full(n, noise)), H.to_device(y.reshape(n, 1)), KV, alpha)
            H.sync()
            outs.append((KV.cpu().numpy(), alpha.cpu().numpy()[:n, 0], logdet, quad, info))
    got, a, logdet, quad, info = outs[0]
    rec.check(all(o[0].tobytes() == got.tobytes() and o[1].tobytes() == a.tobytes() and o[2:] == outs[0][2:] for o in outs[1:]), tag,
              "(g) a second identical call gives other bits")
    rec.check(info == 0, tag, f"(d) info = {info}")
    L = np.tril(got[:n, :n])
    finite = bool(np.all(np.isfinite(L)) and np.all(np.isfinite(a)))
    rec.check(finite, tag, "L or alpha is not finite")
    rec.check(_padding_is_identity(got, n, npad), tag, "(f) the padding rows are not identity")
    rowsE = cr.edge_rows(n, (), n)
    figs = [rec.measure(tag, fam, n, "beta", cr.beta(R.A, L, rowsE), R.beta("scipy", rowsE), R.beta(16, rowsE), 4.0, R.cap_beta(False)),
            rec.measure(tag, fam, n, "phi", cr.phi(L, R.Lhat), R.phi("scipy"), R.phi(16), 4 * EPS, R.cap_phi()),
            rec.measure(tag, fam, n, "lam", cr.lam_value(logdet, R.Lhat), R.lam("scipy"), R.lam(16), cr.lam_floor(R.Lhat), R.cap_lam())]
    z = cr.fwd_ld(R.Lhat, y)
    q_ld = np.sum(z * z)
    q_err = lambda q: float(abs(LD(q) - q_ld) / q_ld)       # noqa: E731
    q_ref = {w: q_err(np.sum(sla.solve_triangular(R.factor(w), y, lower=True) ** 2)) for w in ("scipy", 16)}
    figs.append(rec.measure(tag, fam, n, "quad", q_err(quad) if np.isfinite(quad) else np.inf, q_ref["scipy"], q_ref[16], 4 * EPS, 64 * EPS * R.cond))
    if finite:
        want = ref.potrs_ld(L, y)
        cond_l = ref.cond2(L)
        e_sp = ref.col_err(sla.cho_solve((L, True), y), want)[1]
        e_tw = ref.col_err(ref.blockinv_potrs(L, y, 128), want)[1]
        figs.append(rec.measure(tag, fam, n, "alpha", ref.col_err(a, want)[1], e_sp, e_tw, 4 * EPS, 64 * EPS * cond_l ** 2))
    rec.line(tag, fam, n, figs)
    rec.finish()
