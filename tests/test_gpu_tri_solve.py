"""Every path of the triangular solves (csrc/tri_solve.hip, csrc/sweep.hip, fvgp_hip_panel_trsm) against the extended-precision reference
of tests/tri_solve_ref.py, which tests/test_tri_solve_ref.py proves on the host: the vector path at 1 .. 8 columns (C = 1, 2, 4, 8, the
one-launch sweeps on and off), block substitution on GEMMs under three outer blocks, the transposed sweep with the 1024-wide inverted
blocks (full, one whole block short, and the narrow last pair of the doubling at padded_dim 2432; in two halves and in one; with
and without the block inverses), its fallback above 1024 columns, panel_trsm and both POTRI schedules -- on well-conditioned factors (W), on
covariance factors whose diagonal falls from 1 to sqrt(noise) (G, and a harder H) and on row-scaled ones (S).

The factor is uploaded as given (nothing is factored on the device) into a buffer of padded_dim(n) rows: identity on the padding
diagonal, NaN in the whole strict upper triangle; a leading dimension above the minimum is a strided view into a wider NaN-filled tensor.

On every case: (a) the per-column error of the edge columns against longdouble, under the derived cap 64 eps cond_2(L) (cond^2 where the
solve is with L L^T) and under the measured bar 8 max(error of scipy's float64 solve, error of the float64 twin at the path's block width,
4 eps), both reference errors taken over the same columns against the same longdouble solution -- neither comes from the device; (b) all
other columns against scipy's float64 solve at twice the cap; (c) the padding rows of B come back exactly zero from a non-zero fill; (d)
what lies outside the nrhs columns of a wide B keeps its bits; (e) the whole L buffer, NaNs included, keeps its bits; (f) the result is
finite, so the NaN triangle was never read; (g) a second identical call gives the same bits.

Every case prints `TS|path|device worst|scipy|twin|device / max(scipy, twin, 4 eps)` (pytest -s)."""
import numpy as np
import pytest
import scipy.linalg as sla

import tri_solve_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
DEFAULTS = dict(outer_block=1024, block_inverses=1, fwd_sweep=1, bwd_sweep=1, potri_kminor=1, posterior_halves=1)   # csrc/common.h
KIND = {"potrs": "potrs", "potrs_cols": "potrs", "trsm_lower": "fwd", "trsm_lower_t": "bwd"}
POWER = {"potrs": 2, "fwd": 1, "bwd": 1}
FILL = 7.0


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


class _Options:
    """sets options for a block and puts every one of the module's options back to the library default afterwards"""

    def __init__(self, H, **opts):
        self.H, self.opts = H, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.H.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.H.set_option(k, v)


class _Record:
    """collects the figures of a test's cases (printed whether they pass or not) and the failed checks (asserted at the end)"""

    def __init__(self):
        self.worst, self.fails = {}, []

    def figure(self, path, dev, e_sp, e_tw):
        floor = max(e_sp, e_tw, 4 * EPS)
        w = self.worst.setdefault(path, [0.0, 0.0, 0.0, 0.0])
        if not dev / floor <= w[3]:
            w[:] = [dev, e_sp, e_tw, dev / floor]

    def check(self, ok, path, what):
        if not ok:
            self.fails.append(f"{path}: {what}")

    def finish(self):
        for path, (dev, e_sp, e_tw, ratio) in self.worst.items():
            print(f"TS|{path}|device {dev:.3g}|scipy {e_sp:.3g}|twin {e_tw:.3g}|ratio {ratio:.3g}")
        assert not self.fails, "\n".join(self.fails[:40])


# ---- references, computed once per (fixture, kind) and never modified -----------------------------------------------------------------
class _System:
    """right-hand sides B (n, width) of one fixture and one kind of solve, scipy's float64 solution of all of them, and -- column by
    column, as the cases ask -- the longdouble solution and the error of the float64 twin"""

    def __init__(self, fam, n, kind, width):
        self.L, self.cond = ref.fixture(fam, n)
        self.kind, self.n = kind, n
        self.B = ref.rhs(n, width, {"fwd": 1, "bwd": 2, "potrs": 3}[kind])
        L = self.L
        if kind == "fwd":
            self.sp = sla.solve_triangular(L, self.B, lower=True)
        elif kind == "bwd":
            self.sp = sla.solve_triangular(L, self.B, lower=True, trans="T")
        else:
            self.sp = sla.cho_solve((L, True), self.B)
        self.B.setflags(write=False)
        self.sp.setflags(write=False)
        self._ld, self._tw = {}, {}

    def ld(self, cols):
        miss = [c for c in cols if c not in self._ld]
        if miss:
            sol = {"fwd": ref.fwd_ld, "bwd": ref.bwd_ld, "potrs": ref.potrs_ld}[self.kind](self.L, self.B[:, miss])
            for k, c in enumerate(miss):
                self._ld[c] = sol[:, k]
        return np.stack([self._ld[c] for c in cols], axis=1)

    def twin_err(self, nb, cols):
        miss = [c for c in cols if (nb, c) not in self._tw]
        if miss:
            sol = {"fwd": ref.blockinv_fwd, "bwd": ref.blockinv_bwd, "potrs": ref.blockinv_potrs}[self.kind](self.L, self.B[:, miss], nb)
            e = ref.col_err(sol, self.ld(miss))[0]
            for k, c in enumerate(miss):
                self._tw[(nb, c)] = float(e[k])
        return max(self._tw[(nb, c)] for c in cols)


_SYSTEMS = {}


def _system(fam, n, kind, width):
    key = (fam, n, kind, width)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = _System(fam, n, kind, width)
    return _SYSTEMS[key]


# ---- device buffers ------------------------------------------------------------------------------------------------------------------
def _factor_buffer(L, extra=0):
    """host image of the factor buffer: padded_dim(n) rows, identity on the padding diagonal, NaN in the strict upper triangle (padding
    included) and in the `extra` columns beyond padded_dim(n)"""
    from fvgp_amd._lib import pad128
    n = L.shape[0]
    npad = pad128(n)
    buf = np.full((npad, npad + extra), np.nan)
    blk = buf[:, :npad]
    blk[np.tril_indices(npad)] = 0.0
    il = np.tril_indices(n)
    blk[:n, :n][il] = L[il]
    blk[np.arange(n, npad), np.arange(n, npad)] = 1.0
    return buf


def _same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


class _Factor:
    """a factor on the device (wide tensor, view of the leading padded_dim(n) columns) and a copy to compare its bits with"""

    def __init__(self, H, L, extra=0):
        from fvgp_amd._lib import pad128
        self.n, self.npad = L.shape[0], pad128(L.shape[0])
        self.wide = H.to_device(_factor_buffer(L, extra))
        self.view = self.wide[:, :self.npad]
        self.keep = self.wide.clone()
        H.invalidate_factor()
        assert self.view.stride(0) == self.npad + extra

    def unchanged(self):
        return _same_bits(self.wide, self.keep)


def _rhs_buffer(rhs, npad, extra):
    n, nrhs = rhs.shape
    buf = np.full((npad, nrhs + extra), np.nan)
    buf[:n, :nrhs] = rhs
    buf[n:, :nrhs] = FILL
    return buf


def _call(H, entry, F, rhs, extra=0):
    """one solve of `rhs` (n, nrhs) in a (padded_dim(n), nrhs + extra) buffer; returns the whole buffer as it came back and its image
    before the call"""
    nrhs = rhs.shape[1]
    before = _rhs_buffer(rhs, F.npad, extra)
    wide = H.to_device(before)
    view = wide[:, :nrhs]
    assert view.stride(0) == nrhs + extra
    getattr(H, entry)(F.view, F.n, view, nrhs)
    H.sync()
    return wide.cpu().numpy(), before


def _solve_and_check(H, rec, path, entry, F, S, nrhs, extra=0, nb=128, cond=None, seed=0):
    """the solve twice, checks (a) .. (g); returns the (n, nrhs) result"""
    n, kind = F.n, S.kind
    rhs = S.B[:, :nrhs]
    got, before = _call(H, entry, F, rhs, extra)
    again, _ = _call(H, entry, F, rhs, extra)
    X = got[:n, :nrhs]
    rec.check(got.tobytes() == again.tobytes(), path, "(g) a second identical call gives other bits")
    rec.check(got[:, nrhs:].tobytes() == before[:, nrhs:].tobytes(), path, "(d) B was written outside its nrhs columns")
    rec.check(bool(np.all(got[n:, :nrhs] == 0.0)), path, "(c) padding rows of B are not zero")
    rec.check(F.unchanged(), path, "(e) the factor buffer changed")
    finite = bool(np.all(np.isfinite(X)))
    rec.check(finite, path, "(f) the result is not finite")
    cond = S.cond if cond is None else cond
    cap = 64 * EPS * cond ** POWER[kind]
    cols = ref.edge_columns(nrhs, seed)
    want = S.ld(cols)
    dev = ref.col_err(X[:, cols], want)[1] if finite else np.inf
    e_sp = ref.col_err(S.sp[:, cols], want)[1]
    e_tw = S.twin_err(nb, cols)
    rec.figure(path, dev, e_sp, e_tw)
    bar = 8 * max(e_sp, e_tw, 4 * EPS)
    rec.check(dev <= cap, path, f"(a) edge columns {dev:.3g} above the cap {cap:.3g}")
    rec.check(dev <= bar, path, f"(a) edge columns {dev:.3g} above 8 x max(scipy {e_sp:.3g}, twin {e_tw:.3g}, 4 eps) = {bar:.3g}")
    rest = np.setdiff1d(np.arange(nrhs), cols)
    if len(rest) and finite:
        d = np.linalg.norm(X[:, rest] - S.sp[:, rest], axis=0) / np.linalg.norm(S.sp[:, rest], axis=0)
        rec.check(float(np.max(d)) <= 2 * cap, path, f"(b) other columns {np.max(d):.3g} from scipy, above {2 * cap:.3g}")
    return X


# ---- the vector path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.VEC_N)
@pytest.mark.parametrize("fam", ["W", "G"])
def test_vector_path(H, fam, n):
    """fvgp_hip_potrs and fvgp_hip_trsm_lower at 1 .. 8 columns: the one-launch sweeps (1), the step kernels instantiated for C = 2 (2), 4
    (3, 4) and 8 (5, 7, 8), ldb = nrhs and nrhs + 6.  n = 1 is the smallest legal size, n = 128 a single block with no rows below, 129 two
    blocks with 127 padding rows, 700 six blocks.  One column also with the step kernels in place of either sweep: the backward sweep
    gives the bits of the steps (every sum in the same order), the forward one another order of the same sums, within the bar."""
    rec = _Record()
    F = _Factor(H, ref.fixture(fam, n)[0])
    with _Options(H):
        for entry in ("potrs", "trsm_lower"):
            S = _system(fam, n, KIND[entry], 8)
            for nrhs in (1, 2, 3, 4, 5, 7, 8):
                for extra in (0, 6):
                    _solve_and_check(H, rec, f"{entry} vec {fam} n={n}", entry, F, S, nrhs, extra, seed=n)
            for extra in (0, 6):
                base = _solve_and_check(H, rec, f"{entry} vec {fam} n={n}", entry, F, S, 1, extra, seed=n)
                H.set_option("fwd_sweep", 0)
                steps = _solve_and_check(H, rec, f"{entry} vec fwd steps {fam} n={n}", entry, F, S, 1, extra, seed=n)
                H.set_option("fwd_sweep", 1)
                if entry == "potrs":
                    H.set_option("bwd_sweep", 0)
                    steps = _solve_and_check(H, rec, f"{entry} vec bwd steps {fam} n={n}", entry, F, S, 1, extra, seed=n)
                    H.set_option("bwd_sweep", 1)
                    rec.check(steps.tobytes() == base.tobytes(), f"{entry} n={n}", "the backward sweep and the backward steps differ in bits")
    rec.finish()


@pytest.mark.parametrize("n", [129, 700])
def test_results_do_not_depend_on_what_the_scratch_held(H, n):
    """the step kernels read every column of the handle's scratch (Yres[k0 * C + e] in bwd_step_kernel, also the columns a call with
    fewer right-hand sides than C never wrote): after a solve of 8 columns of NaN on the same handle, a solve of 3 columns (C = 4: one
    column of the scratch is stale) and of 1 column (the sweeps, and the C = 1 steps) return the bits they returned before it"""
    L, _ = ref.fixture("G", n)
    F = _Factor(H, L)
    B = ref.rhs(n, 3, 11)
    nan8 = np.full((n, 8), np.nan)
    with _Options(H):
        for sweeps in (1, 0):
            H.set_option("fwd_sweep", sweeps)
            H.set_option("bwd_sweep", sweeps)
            for entry in ("potrs", "trsm_lower"):
                for nrhs in (3, 1):
                    clean = _call(H, entry, F, B[:, :nrhs])[0]
                    poisoned = _call(H, entry, F, nan8)[0]
                    assert np.all(np.isnan(poisoned[:n]))            # (the padding rows too: 0 x NaN of the rows above)
                    after = _call(H, entry, F, B[:, :nrhs])[0]
                    assert np.all(np.isfinite(after)), (entry, nrhs, sweeps)
                    assert after.tobytes() == clean.tobytes(), (entry, nrhs, sweeps)
    assert F.unchanged()


# ---- block substitution on GEMMs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.GEMM_N)
@pytest.mark.parametrize("fam", ["W", "G"])
def test_gemm_path_below_2048_rows(H, fam, n):
    """fvgp_hip_potrs, _potrs_cols, _trsm_lower, _trsm_lower_t with 128 and 256 columns, ldb = nrhs and nrhs + 128, under outer blocks of
    128, 512 and 1024 (n = 1300: 11 blocks, so three, one whole and one ragged, and two outer blocks).  potrs may take the 64-tile
    kernel where potrs_cols forces the 128-tile one: both hold the bar.  potrs_cols with 256 columns returns, column by column, the
    bits of two calls with 128 columns each (its contract)."""
    rec = _Record()
    F = _Factor(H, ref.fixture(fam, n)[0])
    with _Options(H):
        for outer in (128, 512, 1024):
            H.set_option("outer_block", outer)
            for entry in ("potrs", "potrs_cols", "trsm_lower", "trsm_lower_t"):
                S = _system(fam, n, KIND[entry], 256)
                for nrhs in (128, 256):
                    for extra in (0, 128):
                        X = _solve_and_check(H, rec, f"{entry} gemm outer={outer} {fam} n={n}", entry, F, S, nrhs, extra, seed=n)
                        if entry == "potrs_cols" and nrhs == 256:
                            for c0 in (0, 128):
                                part = _call(H, entry, F, S.B[:, c0:c0 + 128], extra)[0][:n, :128]
                                rec.check(part.tobytes() == np.ascontiguousarray(X[:, c0:c0 + 128]).tobytes(), f"potrs_cols outer={outer} n={n}",
                                          f"columns {c0}.. of a 256-column call differ in bits from a 128-column call")
    rec.finish()


# ---- the transposed sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,n", ref.SWEEP_CASES)
def test_transposed_sweep(H, fam, n):
    """fvgp_hip_trsm_lower with 128 .. 1024 columns against padded_dim(n) >= 2048: 2048 (two full 1024-blocks), 2304 (a last block of
    256) and 2432 (a last block of 384 = 256 + 128: the pair with a narrower second half in the doubling).  512, 768 and 1024 columns
    run as two halves on two streams, 128 and 640 do not; every count under both settings of posterior_halves and of block_inverses
    (0: the same sweep substitutes by 128-blocks, the twin at 128 is its bar).  Once per n the factor sits in a buffer 128 columns
    wider than padded_dim(n)."""
    rec = _Record()
    L = ref.fixture(fam, n)[0]
    S = _system(fam, n, "fwd", 1152 if n == 2432 else 1024)
    F = _Factor(H, L)
    with _Options(H):
        for binv, nb in ((1, 1024), (0, 128)):
            H.set_option("block_inverses", binv)
            for nrhs in (128, 512, 640, 768, 1024):
                for halves in (1, 0):
                    H.set_option("posterior_halves", halves)
                    _solve_and_check(H, rec, f"trsm_lower sweep binv={binv} halves={halves} {fam} n={n}", "trsm_lower", F, S, nrhs, nb=nb, seed=n)
            H.set_option("posterior_halves", 1)
        H.set_option("block_inverses", 1)
        if n == 2432 and fam == "G":            # above 1024 columns: block substitution on GEMMs under outer_block
            _solve_and_check(H, rec, f"trsm_lower 1152 columns (fallback) {fam} n={n}", "trsm_lower", F, S, 1152, nb=128, seed=n)
        if fam == "G":
            del F
            F = _Factor(H, L, extra=128)
            for nrhs, extra in ((128, 0), (512, 128)):
                _solve_and_check(H, rec, f"trsm_lower sweep ldl=padded+128 {fam} n={n}", "trsm_lower", F, S, nrhs, extra, nb=1024, seed=n)
    rec.finish()


@pytest.mark.parametrize("fam", ["G", "H"])
def test_backward_and_full_solves_at_2432(H, fam):
    """fvgp_hip_trsm_lower_t and fvgp_hip_potrs (and _potrs_cols) with 128 and 384 columns at n = 2432 on the covariance factor; the harder
    one (cond_2 = 1.2e5) once per entry at 384 columns; once with the factor in a wider buffer"""
    rec = _Record()
    n = 2432
    L = ref.fixture(fam, n)[0]
    F = _Factor(H, L)
    with _Options(H):
        for entry in ("trsm_lower_t", "potrs", "potrs_cols"):
            S = _system(fam, n, KIND[entry], 384)
            for nrhs in ((128, 384) if fam == "G" else (384,)):
                _solve_and_check(H, rec, f"{entry} gemm {fam} n={n}", entry, F, S, nrhs, seed=n)
        if fam == "G":
            del F
            F = _Factor(H, L, extra=128)
            for entry in ("trsm_lower_t", "potrs"):
                _solve_and_check(H, rec, f"{entry} gemm ldl=padded+128 {fam} n={n}", entry, F, _system(fam, n, KIND[entry], 384), 128, 128, seed=n)
    rec.finish()


# ---- panel_trsm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [128, 384])
def test_panel_trsm(H, nd):
    """X = P L^-T with L the leading nd x nd of the covariance factor (itself the factor of the leading covariance), rows 128 and 640,
    ldp = nd and nd + 128.  Row i of X solves L x = P_i^T: the reference is the longdouble substitution on the transposed system, the
    measure the error per ROW of X.  rows = 0 returns 0 and touches nothing."""
    rec = _Record()
    D = np.array(ref.fixture("G", 700)[0][:nd, :nd])
    cond = ref.cond2(D)
    F = _Factor(H, D)
    cap = 64 * EPS * cond
    for rows in (128, 640):
        P = ref.rhs(rows, nd, 13 + nd)
        rcols = ref.edge_columns(rows, nd)
        want = ref.fwd_ld(D, np.ascontiguousarray(P.T[:, rcols]))
        sp = sla.solve_triangular(D, P.T, lower=True)
        e_sp = ref.col_err(sp[:, rcols], want)[1]
        e_tw = ref.col_err(ref.blockinv_fwd(D, np.ascontiguousarray(P.T[:, rcols]), 128), want)[1]
        for extra in (0, 128):
            path = f"panel_trsm nd={nd} rows={rows}"
            before = np.full((rows, nd + extra), np.nan)
            before[:, :nd] = P
            outs = []
            for _ in range(2):
                wide = H.to_device(before)
                H.panel_trsm(F.view, nd, wide[:, :nd], rows)
                H.sync()
                outs.append(wide.cpu().numpy())
            got = outs[0]
            rec.check(got.tobytes() == outs[1].tobytes(), path, "(g) a second identical call gives other bits")
            rec.check(got[:, nd:].tobytes() == before[:, nd:].tobytes(), path, "(d) P was written outside its nd columns")
            rec.check(F.unchanged(), path, "(e) the diagonal block changed")
            X = got[:, :nd]
            finite = bool(np.all(np.isfinite(X)))
            rec.check(finite, path, "(f) the result is not finite")
            dev = ref.col_err(X.T[:, rcols], want)[1] if finite else np.inf
            rec.figure(path, dev, e_sp, e_tw)
            bar = 8 * max(e_sp, e_tw, 4 * EPS)
            rec.check(dev <= cap and dev <= bar, path, f"(a) edge rows {dev:.3g}: cap {cap:.3g}, 8 x max(scipy {e_sp:.3g}, twin {e_tw:.3g}, 4 eps) = {bar:.3g}")
            rest = np.setdiff1d(np.arange(rows), rcols)
            if finite:
                d = np.linalg.norm(X.T[:, rest] - sp[:, rest], axis=0) / np.linalg.norm(sp[:, rest], axis=0)
                rec.check(float(np.max(d)) <= 2 * cap, path, f"(b) other rows {np.max(d):.3g} from scipy, above {2 * cap:.3g}")
        wide = H.to_device(before)
        H.panel_trsm(F.view, nd, wide[:, :nd], 0)
        H.sync()
        rec.check(wide.cpu().numpy().tobytes() == before.tobytes() and F.unchanged(), f"panel_trsm nd={nd}", "rows = 0 wrote something")
    rec.finish()


# ---- POTRI ----------------------------------------------------------------------------------------------------------------------------
_POTRI = {}


def _potri_refs(fam, n):
    if (fam, n) not in _POTRI:
        L, cond = ref.fixture(fam, n)
        cols = ref.edge_columns(n, n)
        E = np.zeros((n, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        want = ref.potrs_ld(L, E)
        sp = sla.cho_solve((L, True), E)
        tail = lambda M: max(ref.col_err(M[j:, k], want[j:, k])[1] for k, j in enumerate(cols))      # noqa: E731
        tw = {nb: tail(ref.blockinv_potrs(L, E, nb)) for nb in (128, 1024)}
        _POTRI[(fam, n)] = dict(cols=cols, want=want, e_sp=tail(sp), e_tw=tw, inv=np.linalg.inv(L @ L.T), cond=cond)
    return _POTRI[(fam, n)]


@pytest.mark.parametrize("kminor", [1, 0])
@pytest.mark.parametrize("n", ref.POTRI_N)
@pytest.mark.parametrize("fam", ["W", "G"])
def test_potri(H, fam, n, kminor):
    """fvgp_hip_potri, both schedules (potri_kminor = 1: from the 1024-wide inverted blocks; 0: from the 128-blocks under outer_block), with
    ldl = ldw = padded_dim(n) and both 128 above it, the work buffer filled with NaN.  Column j of the returned lower triangle, rows >= j,
    against potrs_ld(L, e_j) for the edge columns j (cap 64 eps cond_2(L)^2 and the measured bar; scipy's figure is cho_solve of e_j);
    every column of the triangle against numpy's float64 inverse of L L^T at the cap; the extra columns of both buffers keep their bits;
    a second run gives the same bits; after symmetrize the upper triangle is the transposed lower one, bit for bit."""
    from fvgp_amd._lib import pad128
    rec = _Record()
    R = _potri_refs(fam, n)
    L, cond, cols = ref.fixture(fam, n)[0], R["cond"], R["cols"]
    npad = pad128(n)
    cap = 64 * EPS * cond * cond
    nb = 1024 if kminor else 128
    with _Options(H, potri_kminor=kminor):
        for extra in (0, 128):
            path = f"potri kminor={kminor} {fam} n={n}"
            outs = []
            for _ in range(2):
                F = _Factor(H, L, extra)
                work0 = np.full((npad, npad + extra), np.nan)
                work = H.to_device(work0)
                H.potri(F.view, n, work[:, :npad])
                H.sync()
                outs.append((F.wide.cpu().numpy(), work.cpu().numpy()))
            got, wgot = outs[0]
            low = np.tril(got[:n, :n])
            rec.check(np.tril(outs[1][0][:n, :n]).tobytes() == low.tobytes(), path, "(g) a second identical call gives other bits")
            if extra:
                rec.check(bool(np.all(np.isnan(got[:, npad:])) and np.all(np.isnan(wgot[:, npad:]))), path, "(d) columns beyond padded_dim(n) were written")
            finite = bool(np.all(np.isfinite(got[:n, :n][np.tril_indices(n)])))
            rec.check(finite, path, "(f) the lower triangle is not finite")
            dev = max(ref.col_err(low[j:, j], R["want"][j:, k])[1] for k, j in enumerate(cols)) if finite else np.inf
            rec.figure(path, dev, R["e_sp"], R["e_tw"][nb])
            bar = 8 * max(R["e_sp"], R["e_tw"][nb], 4 * EPS)
            rec.check(dev <= cap, path, f"(a) edge columns {dev:.3g} above the cap {cap:.3g}")
            rec.check(dev <= bar, path, f"(a) edge columns {dev:.3g} above 8 x max(scipy {R['e_sp']:.3g}, twin {R['e_tw'][nb]:.3g}, 4 eps) = {bar:.3g}")
            if finite:
                inv = np.tril(R["inv"])
                d = np.linalg.norm(low - inv, axis=0) / np.linalg.norm(inv, axis=0)
                rec.check(float(np.max(d)) <= cap, path, f"(b) the triangle is {np.max(d):.3g} from numpy's inverse, above the cap {cap:.3g}")
            H.symmetrize(F.view, n)
            H.sync()
            full = F.wide.cpu().numpy()[:n, :n]
            rec.check(np.tril(full).tobytes() == low.tobytes() and np.ascontiguousarray(full.T).tobytes() == full.tobytes(), path,
                      "symmetrize: the upper triangle is not the transposed lower one")
            H.invalidate_factor()
    rec.finish()


# ---- family S -------------------------------------------------------------------------------------------------------------------------
def test_scaled_rows(H):
    """family S: the factor D L_W and the right-hand sides D B, D powers of two 2^-20 .. 2^20.  The forward solve has the solution of
    (L_W, B) itself and the L L^T solve D^-1 times it (multiply the returned rows by D), exactly, so each must hold the bar of the same
    call on (L_W, B) -- with row magnitudes spread over 2^40, which a max-norm over the whole result cannot see.  Whether the bits equal
    those of the unscaled call is printed, not asserted."""
    rec = _Record()
    for entry, n, nrhs, nb in (("trsm_lower", 700, 3, 128), ("trsm_lower", 2432, 128, 1024), ("potrs", 700, 1, 128)):
        L, cond = ref.fixture("W", n)
        D = ref.scaling_s(n, ref.SEED)
        S = _system("W", n, KIND[entry], 128 if nrhs == 128 else 8)
        plain = _solve_and_check(H, rec, f"{entry} unscaled W n={n} nrhs={nrhs}", entry, _Factor(H, L), S, nrhs, nb=nb, seed=n)
        F = _Factor(H, D[:, None] * L)
        got, before = _call(H, entry, F, D[:, None] * S.B[:, :nrhs])
        path = f"{entry} scaled S n={n} nrhs={nrhs}"
        rec.check(F.unchanged(), path, "(e) the factor buffer changed")
        rec.check(bool(np.all(got[n:] == 0.0)), path, "(c) padding rows of B are not zero")
        X = got[:n] * D[:, None] if entry == "potrs" else got[:n]
        finite = bool(np.all(np.isfinite(X)))
        rec.check(finite, path, "(f) the result is not finite")
        cols = list(range(nrhs)) if nrhs <= 8 else ref.edge_columns(nrhs, n)
        want = S.ld(cols)
        dev = ref.col_err(X[:, cols], want)[1] if finite else np.inf
        e_sp, e_tw = ref.col_err(S.sp[:, cols], want)[1], S.twin_err(nb, cols)
        rec.figure(path, dev, e_sp, e_tw)
        cap, bar = 64 * EPS * cond ** POWER[KIND[entry]], 8 * max(e_sp, e_tw, 4 * EPS)
        rec.check(dev <= cap and dev <= bar, path, f"(a) {dev:.3g}: cap {cap:.3g}, 8 x max(scipy {e_sp:.3g}, twin {e_tw:.3g}, 4 eps) = {bar:.3g}")
        # component by component: the largest error of an entry in units of the largest entry of its column
        comp = float(np.max(np.abs(X[:, cols] - np.asarray(want, dtype=np.float64)) / np.max(np.abs(np.asarray(want, dtype=np.float64)), axis=0)))
        rec.check(comp <= cap, path, f"an entry is off by {comp:.3g} of its column's largest, above {cap:.3g}")
        print(f"TS|{path}|bits equal to the unscaled call: {X.tobytes() == np.ascontiguousarray(plain).tobytes()}")
    rec.finish()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_alone(H):
    """the status of each refused call (HipExtensionError), and after it every buffer bit for bit as it was"""
    from fvgp_amd import _lib
    n = 300
    npad = _lib.pad128(n)
    F = _Factor(H, ref.fixture("W", n)[0])
    image = np.full((npad, 384), 3.0)
    cases = []
    for entry in ("potrs", "potrs_cols", "trsm_lower", "trsm_lower_t"):
        cases.append((entry, 384, 0, -6))
    for entry in ("potrs", "trsm_lower"):
        cases += [(entry, 384, 9, -6), (entry, 384, 100, -6), (entry, 2, 3, -7)]
    for entry in ("potrs_cols", "trsm_lower_t"):
        cases += [(entry, 384, 100, -6), (entry, 384, 8, -6), (entry, 128, 256, -7)]
    for entry, width, nrhs, status in cases:
        B = H.to_device(image[:, :width])
        with pytest.raises(_lib.HipExtensionError, match=f"status {status}\\b"):
            getattr(H, entry)(F.view, n, B, nrhs)
        H.sync()
        assert B.cpu().numpy().tobytes() == np.ascontiguousarray(image[:, :width]).tobytes(), (entry, nrhs)
        assert F.unchanged(), (entry, nrhs)
    # the factor's leading dimension: odd, and below padded_dim(n)
    for ld in (npad + 1, npad - 2):
        bad = H.to_device(np.full((npad, ld), 2.0))
        keep = bad.clone()
        for entry, nrhs in (("potrs", 3), ("potrs_cols", 128), ("trsm_lower", 128), ("trsm_lower_t", 128)):
            B = H.to_device(image[:, :128])
            with pytest.raises(_lib.HipExtensionError, match="status -4\\b"):
                getattr(H, entry)(bad, n, B, nrhs)
            H.sync()
            assert B.cpu().numpy().tobytes() == np.ascontiguousarray(image[:, :128]).tobytes() and _same_bits(bad, keep), (entry, ld)
        work = H.to_device(np.full((npad, npad), 5.0))
        with pytest.raises(_lib.HipExtensionError, match="status -4\\b"):
            H.potri(bad, n, work)
        H.sync()
        assert _same_bits(bad, keep) and bool((work == 5.0).all())
    # panel_trsm: a diagonal block that is no multiple of 128, rows that are none, a panel narrower than the block
    D = H.to_device(np.full((256, 256), 2.0))
    keepD = D.clone()
    for nd, pshape, rows, status in ((100, (128, 128), 128, -3), (256, (128, 256), 100, -6), (256, (128, 128), 128, -7)):
        P = H.to_device(np.full(pshape, 4.0))
        with pytest.raises(_lib.HipExtensionError, match=f"status {status}\\b"):
            H.panel_trsm(D, nd, P, rows)
        H.sync()
        assert bool((P == 4.0).all()) and _same_bits(D, keepD), (nd, rows)
    H.invalidate_factor()
