"""Every path of fvgp_hip_posterior (csrc/evaluate.hip) against the extended-precision reference of tests/posterior_ref.py, which
tests/test_posterior_ref.py proves on the host, and fvgp_hip_coldot / fvgp_hip_colsumsq / fvgp_hip_dot (the variance's other route,
sigma^2 - k^T KV^-1 k of gp.py's cholinv mode) against longdouble sums.

L and alpha are uploaded as given -- nothing is factored on the device: L in a buffer of padded_dim(n) rows with identity on the padding
diagonal and NaN in the whole strict upper triangle, alpha with zero padding rows (what fvgp_hip_loglik leaves), H.invalidate_factor()
after every upload, kx NaN-filled on entry, every output in a buffer of sentinels.

Every call is judged by _judge: (a) mu, nu, sig of the sampled points per class under the derived caps and under the bars 8 max(twin (a),
twin (b) at the route's block width, floor) -- neither comes from the device; (b) the points far from the data: mean 0 and variance
sigma^2 exactly, on ALL of them; (c) the variance against the diagonal of S of the same call, all points, within the bar; (d) S
bitwise symmetric over [:P, :P] and finite although L's upper triangle and kx were NaN; (e) the sentinels behind P in mean_out and
var_out and in the columns of S_out from padded_dim(P) on; (f) L and alpha bit for bit as uploaded.

rows_sumsq_base_kernel is launched with the padded row count by all three of its callers, so its odd tail is not reachable from the
entry (rows_dot_kernel's is, at every odd n).  route() restates the host logic of fvgp_hip_posterior, trsm_fwd_gemm_t and the K split
of S -= V^T V: LATTICE is checked against it by test_the_lattice_reaches_every_route.  Every case prints `PO|path|measure|class|device|twin a|twin b|device / max(twins, floor)`
(pytest -s)."""
import ctypes

import numpy as np
import pytest

import posterior_ref as pr

pytestmark = pytest.mark.gpu

EPS, LD = pr.EPS, pr.LD
DEFAULTS = dict(block_inverses=1, posterior_halves=1, posterior_block=2048, fwd_sweep=1)         # csrc/common.h
SENT = -7.25
ALL = ("m", "v", "S")
OUTPUTS = (("m",), ("v",), ("S",), ("m", "S"), ALL)         # ("m", "S") is what gp.py asks for


def pad128(n):
    return -(-n // 128) * 128


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


class _Options:
    """sets options for a block and puts every one of the module's options back to the library default in a finally"""

    def __init__(self, H, opts):
        self.H, self.opts = H, opts or {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.H.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.H.set_option(k, v)


# ---- the routes of csrc/evaluate.hip, restated ------------------------------------------------------------------------------------
def s_split(n, P):
    """(K split of S -= V^T V, whether the search loop ran) as fvgp_hip_posterior chooses it"""
    npad, Pp = pad128(n), pad128(P)
    tr = Pp // 128
    tiles = tr * (tr + 1) // 2
    split = 1 if tiles >= 512 else 64 // ((tiles + 7) // 8)
    max_split = max(npad // 512, 1)
    searched = False
    if tiles >= 512:
        best = float((tiles + 511) // 512)
        for sp in range(2, min(8, max_split) + 1):
            searched = True
            rounds = ((tiles * sp + 511) // 512) / sp
            if rounds < best * 0.97:
                best, split = rounds, sp
            if best <= 1.15 * tiles / 512.0:
                break
    return min(split, max_split), searched


def route(n, P, ncol, opts=None, outs=ALL):
    """(set of the branches one call takes, block width of the float64 twin (b), depth of the mean's summation in units of eps)"""
    o = dict(DEFAULTS, **(opts or {}))
    npad, Pp = pad128(n), pad128(P)
    tags = set()
    if P == 1 and o["fwd_sweep"] and ncol <= 8:
        # `if (P == 1 && h->fwd_sweep && ncol <= FVGP_MAX_RHS_VEC)`: dot_rows_kernel per column, launch_fwd_sweep, rows_sumsq_base
        tags.add("one-point")
        if "m" in outs:
            tags.add("dot_rows")
        if "v" in outs:
            tags.add("one-point var")
        if "S" in outs:
            tags.add("one-point S")
        # dot_rows_kernel, 1024 threads: ceil(n / 1024) fused adds, 6 shuffle steps, 16 wave sums in sequence
        return tags, 128, -(-n // 1024) + 6 + 16
    tags.add("many-point")
    depth = 0
    if "m" in outs:
        if ncol <= 8:
            C = 1 if ncol <= 1 else 2 if ncol <= 2 else 4 if ncol <= 4 else 8
            tags.add(f"rows_dot<{C}>")
            tags.add("rows_dot odd tail" if n % 2 else "rows_dot even")
            # rows_dot_kernel, 256 threads two elements at a time: 2 ceil(n / 512) fused adds, 6 shuffle steps, 2 levels of wave sums
            depth = 2 * -(-n // 512) + 6 + 2
        else:
            tags.add("mean GEMM")
            # the bound of tests/gemm_ref.py for K = padded_dim(n), unsplit: (K + 1 + 2) u = (K + 3) / 2 eps
            depth = (npad + 3) / 2
    nb = 128
    if "v" in outs or "S" in outs:
        winv = bool(o["block_inverses"])
        WB = o["posterior_block"] if Pp <= 1024 else 1024
        nb = WB if winv else 128
        tags.add(f"blocks {WB}" if winv else "steps 128")
        if npad >= 256 and winv:
            tags.add("doubling")
        if npad > WB:
            tags.add("outer blocks > 1")
        halves = bool(o["posterior_halves"]) and winv and 512 <= Pp <= 1024 and Pp % 256 == 0
        tags.add("halves" if halves else "whole")
        if "S" in outs:
            split, searched = s_split(n, P)
            tags.add("S split > 1" if split > 1 else "S unsplit")
            if searched:
                tags.add("S split search")
            tags.add("mirror")
        if "v" in outs:
            tags.add("rows_sumsq_base")
    return tags, nb, depth


# ---- the lattice --------------------------------------------------------------------------------------------------------------------
def _case(fam, n, P, ncol=1, opts=None, outs=ALL, el=0, ek=0, es=0, first=0):
    o = "-".join(f"{k}{v}" for k, v in (opts or {}).items())
    name = f"{fam}-n{n}-P{P}-c{ncol}" + (f"-{o}" if o else "") + ("" if outs == ALL else "-" + "".join(outs)) \
        + (f"-ld+{el},{ek},{es}" if el or ek or es else "") + (f"-first{first}" if first else "")
    return pytest.param(fam, n, P, ncol, opts or {}, outs, (el, ek, es), first, id=name)


def _lattice():
    cases = []
    for fam in "BG":
        # every n with the one-point route (all five classes, one call each) ...
        for n in pr.GPU_N:
            for first in range(5):
                cases.append(_case(fam, n, 1, 1 + (n + first) % 8 if first == 0 else 1, first=first))
        # ... and with many points; P and ncol walk their axes along n
        cases += [
            _case(fam, 1, 5, 1),                                  # one data point: L = (l_11), 127 padding rows
            _case(fam, 2, 2, 2),                                  # rows_dot<2>
            _case(fam, 127, 127, 3),                              # rows_dot<4> at 3 columns, odd n: the odd tail
            _case(fam, 128, 128, 4),                              # no padding rows at all, posterior_prepare returns early
            _case(fam, 129, 129, 5, el=6, ek=2, es=4),            # rows_dot<8> at 5; two blocks, 127 padding rows; wide ldl, ldk, lds
            _case(fam, 255, 300, 8),                              # rows_dot<8> full
            _case(fam, 129, 1, 2, el=6, ek=2, es=4),              # the one-point route strides kx by ldk and S by lds: both above 128
            _case(fam, 129, 1, 1, el=6, ek=2, es=4, first=1),
            _case(fam, 300, 1, 1, opts=dict(fwd_sweep=0)),        # one point through the many-point route
            _case(fam, 300, 1, 9),                                # the widened GEMM route at one point
            _case(fam, 300, 5, 128),                              # ... at 128 columns
            _case(fam, 300, 300, 1),
            _case(fam, 300, 300, 1, opts=dict(block_inverses=0)),     # the 128-step substitution
            _case(fam, 300, 512, 9),                              # padded 512: two halves on two streams
            _case(fam, 300, 512, 1, opts=dict(posterior_halves=0)),
            _case(fam, 300, 640, 1),                              # padded 640 is no multiple of 256: one sweep
            _case(fam, 700, 1000, 2),                             # padded 1024: two halves of 512
            _case(fam, 700, 1100, 1),                             # padded 1152: 1024-wide blocks, one outer block
            _case(fam, 1300, 300, 8),                             # 1408 padded rows: S split 2 (max_split), one 2048-block
            _case(fam, 1300, 300, 1, opts=dict(posterior_block=1024)),     # two outer blocks of 1024
            _case(fam, 1300, 1100, 1, es=2),                      # 1024-blocks by the number of points, two outer blocks
        ]
        for outs in OUTPUTS[:-1]:
            cases.append(_case(fam, 300, 300, 3, outs=outs))
            cases.append(_case(fam, 129, 1, 3, outs=outs, first=1))
    cases.append(_case("G", 1300, 4096, 1))                       # 528 output tiles: the split search runs and picks 2
    # H on the routes that substitute: one point, few points, halves, whole
    for n in pr.H_N:
        for first in range(5):
            cases.append(_case("H", n, 1, 1, first=first))
    cases += [_case("H", 129, 5, 1), _case("H", 300, 5, 2), _case("H", 300, 300, 1), _case("H", 300, 512, 1),
              _case("H", 300, 300, 1, opts=dict(block_inverses=0)), _case("H", 700, 1000, 1), _case("H", 1300, 300, 1),
              _case("H", 1300, 1100, 1)]
    # another radial kind, d = 3
    cases += [_case("M", 300, 300, 2), _case("M", 300, 1, 1, first=3), _case("M", 300, 1, 1, first=1)]
    return cases


LATTICE = _lattice()
ROUTES = {"one-point", "dot_rows", "one-point var", "one-point S", "many-point", "rows_dot<1>", "rows_dot<2>", "rows_dot<4>",
          "rows_dot<8>", "rows_dot odd tail", "rows_dot even", "mean GEMM", "blocks 2048", "blocks 1024", "steps 128", "doubling",
          "outer blocks > 1", "halves", "whole", "S split > 1", "S unsplit", "S split search", "mirror", "rows_sumsq_base"}


def test_the_lattice_reaches_every_route():
    """the case list itself: every branch route() knows is taken on B and on G, every value of every axis of the issue's table appears on
    both, H runs one point, few points, halves and whole, and the figures the comments of evaluate.hip state come out of s_split"""
    reach = {f: set() for f in "BGHM"}
    axes = {f: {k: set() for k in ("n", "P", "ncol", "outs", "opts", "ld", "ld one-point")} for f in "BGHM"}
    for p in LATTICE:
        fam, n, P, ncol, opts, outs, ld, first = p.values
        tags = route(n, P, ncol, opts, outs)[0]
        reach[fam] |= tags
        a = axes[fam]
        a["n"].add(n); a["P"].add(P); a["ncol"].add(ncol); a["outs"].add(outs); a["opts"] |= set(opts.items())
        a["ld one-point" if "one-point" in tags else "ld"] |= {i for i, e in enumerate(ld) if e}
        if P == 1 and "one-point" in tags:
            a["P"].add("sweep")
    assert reach["B"] | {"S split search"} == ROUTES and reach["G"] == ROUTES
    for fam in "BG":
        a = axes[fam]
        assert a["n"] == set(pr.GPU_N)
        assert a["P"] >= {1, "sweep", 2, 5, 127, 128, 129, 300, 512, 640, 1000, 1100}
        assert a["ncol"] >= {1, 2, 3, 4, 5, 8, 9, 128}
        assert a["outs"] == set(OUTPUTS)
        assert a["opts"] >= {("block_inverses", 0), ("posterior_halves", 0), ("posterior_block", 1024), ("fwd_sweep", 0)}
        assert a["ld"] == {0, 1, 2} and a["ld one-point"] == {0, 1, 2}
    assert 4096 in axes["G"]["P"]
    assert reach["H"] >= {"one-point", "whole", "halves", "steps 128", "blocks 2048", "blocks 1024", "outer blocks > 1"}
    assert "rows_sumsq_base" in reach["M"] and "one-point var" in reach["M"]
    # the host's choice of the K split
    assert s_split(20000, 1000) == (12, False)          # "36 tiles -> 5 -> 12 slices, not 14"
    assert s_split(1300, 300) == (2, False) and s_split(700, 300) == (1, False)
    assert s_split(1300, 4096) == (2, True) and s_split(1300, 4000) == (2, True) and s_split(300, 4096) == (1, False)
    assert route(300, 512, 1)[0] >= {"halves"} and route(300, 640, 1)[0] >= {"whole"} and route(700, 1000, 1)[0] >= {"halves"}
    assert route(300, 512, 1, dict(block_inverses=0))[0] >= {"whole", "steps 128"}
    assert route(700, 1100, 1)[1] == 1024 and route(700, 1000, 1)[1] == 2048 and route(129, 1, 1)[1] == 128
    assert "doubling" not in route(128, 128, 1)[0]


# ---- device buffers -----------------------------------------------------------------------------------------------------------------
def _factor_buffer(L, extra=0):
    """host image of the factor buffer: padded_dim(n) rows, identity on the padding diagonal, NaN in the strict upper triangle (padding
    included) and in the `extra` columns beyond padded_dim(n)"""
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


class _Data:
    """one fixture on the device: x, the factor (wide tensor and a view of padded_dim(n) columns), alpha per column count, and copies to
    compare the bits with.  H.invalidate_factor() follows the upload."""

    def __init__(self, H, fx, extra=0):
        self.H, self.fx, self.n, self.npad = H, fx, fx.n, pad128(fx.n)
        self.x = H.to_device(fx.x)
        self.wide = H.to_device(_factor_buffer(fx.L, extra))
        self.L = self.wide[:, :self.npad]
        self.keep = self.wide.clone()
        H.invalidate_factor()
        assert self.L.stride(0) == self.npad + extra
        self._alpha = {}

    def alpha(self, ncol):
        if ncol not in self._alpha:
            a = np.zeros((self.npad, ncol))
            a[:self.n] = self.fx.alpha(ncol)
            d = self.H.to_device(a)
            self._alpha[ncol] = (d, d.clone())
        return self._alpha[ncol][0]

    def unchanged(self):
        return _same_bits(self.wide, self.keep) and all(_same_bits(a, k) for a, k in self._alpha.values())


_DATA = {}


def _data(H, fam, n, extra=0):
    """cached per (fixture, extra): at most a handful of factors of up to 16 MB"""
    key = (fam, n, extra)
    if key not in _DATA or _DATA[key].H is not H:
        _DATA[key] = _Data(H, pr.fixture(fam, n), extra)
    else:
        H.invalidate_factor()           # the cached inverses belong to whatever factor the last test used
    return _DATA[key]


class _Out:
    pass


def _call(H, D, xp, ncol, outs=ALL, ek=0, es=0, sync=True):
    """one posterior of the points xp: kx NaN-filled, every output asked for in a buffer of sentinels.  Returns m (P, ncol), v (P,),
    S (padded_dim(P), padded_dim(P)) -- None where not asked for -- and whether the sentinels survived"""
    import torch
    from fvgp_amd import _lib
    P = xp.shape[0]
    Pp = pad128(P)
    kid = _lib.KERNEL_IDS[D.fx.kernel]
    xpd = H.to_device(xp)
    kx = torch.full((D.npad, Pp + ek), float("nan"), dtype=torch.float64, device=D.x.device)
    mbuf = torch.full((P * ncol + 16,), SENT, dtype=torch.float64, device=D.x.device) if "m" in outs else None
    vbuf = torch.full((P + 16,), SENT, dtype=torch.float64, device=D.x.device) if "v" in outs else None
    Sbuf = torch.full((Pp, Pp + es), SENT, dtype=torch.float64, device=D.x.device) if "S" in outs else None
    H.posterior(kid, D.x, D.fx.theta, D.L, D.alpha(ncol), ncol, xpd, kx,
                mean_out=None if mbuf is None else mbuf[:P * ncol].view(P, ncol), var_out=None if vbuf is None else vbuf[:P],
                S_out=None if Sbuf is None else Sbuf[:, :Pp])
    if sync:
        H.sync()
    r = _Out()
    r.P, r.Pp, r.ncol = P, Pp, ncol
    r.m = r.v = r.S = None
    r.tails = True
    if mbuf is not None:
        a = H.to_host(mbuf)
        r.m, r.tails = a[:P * ncol].reshape(P, ncol).copy(), r.tails and bool(np.all(a[P * ncol:] == SENT))
    if vbuf is not None:
        a = H.to_host(vbuf)
        r.v, r.tails = a[:P].copy(), r.tails and bool(np.all(a[P:] == SENT))
    if Sbuf is not None:
        a = H.to_host(Sbuf)
        r.S, r.tails = a[:, :Pp], r.tails and bool(np.all(a[:, Pp:] == SENT))
    return r


def _bits(r):
    return tuple(None if a is None else a.tobytes() for a in (r.m, r.v, None if r.S is None else r.S[:r.P, :r.P]))


# ---- references, computed once per call shape and never modified ---------------------------------------------------------------------
_REFS = {}


def _reference(fam, n, P, first, ncol):
    """(xpred, classes, sampled indices, Reference of the sampled points with 8 or 128 columns of alpha)"""
    width = pr.VEC_COLS if ncol <= pr.VEC_COLS else pr.MAX_COLS
    key = (fam, n, P, first, width)
    if key not in _REFS:
        fx = pr.fixture(fam, n)
        xp, cls = pr.points(fx, P, first=first)
        idx = pr.sample_points(P, seed=n)
        _REFS[key] = (xp, cls, idx, pr.Reference(fx, xp[idx], [cls[i] for i in idx], width))
    return _REFS[key]


class _Record:
    """collects the figures of a test's cases (printed whether they pass or not) and the failed checks (asserted at the end)"""

    def __init__(self):
        self.rows, self.fails = [], []

    def check(self, ok, path, what):
        if not ok:
            self.fails.append(f"{path}: {what}")

    def finish(self):
        print()
        for row in self.rows:
            print("PO|" + "|".join(row))
        assert not self.fails, "\n".join(self.fails[:40])


def _judge(rec, path, D, r, fam, n, P, first, opts, outs):
    """checks (a) .. (f) of one call's outputs"""
    fx = D.fx
    xp, cls, idx, R = _reference(fam, n, P, first, r.ncol)
    _, nb, depth = route(n, P, r.ncol, opts, outs)
    sig2 = fx.theta[0]
    rec.check(r.tails, path, "(e) a sentinel behind an output was overwritten")
    rec.check(D.unchanged(), path, "(f) L or alpha changed")
    finite = all(a is None or bool(np.all(np.isfinite(a[:P]))) for a in (r.m, r.v)) and (r.S is None or bool(np.all(np.isfinite(r.S))))
    rec.check(finite, path, "(d) an output is not finite")
    if not finite:
        return
    # (a) accuracy of the sampled points
    fig = R.measure(None if r.m is None else r.m[idx], None if r.v is None else r.v[idx],
                    None if r.S is None else r.S[np.ix_(idx, idx)], cols=slice(0, r.ncol))
    bars, ta, tb = R.bars(nb), R.twin(None), R.twin(nb)
    for q, per in fig.items():
        cap = pr.mu_cap(fx, depth) if q == "mu" else max(fx.cap_solve(), pr.FLOOR[q])
        worst = max(per, key=lambda c: per[c] / bars[q][c])
        rec.rows.append((path, q, worst, f"device {per[worst]:.3g}", f"twin a {ta[q][worst]:.3g}", f"twin b({nb}) {tb[q][worst]:.3g}",
                         f"ratio {per[worst] / (bars[q][worst] / pr.MARGIN):.3g}"))
        for c, val in per.items():
            rec.check(val <= cap, path, f"(a) {q} {c} {val:.3g} above the cap {cap:.3g}")
            rec.check(val <= bars[q][c], path,
                      f"(a) {q} {c} {val:.3g} above 8 x max(twin a {ta[q][c]:.3g}, twin b({nb}) {tb[q][c]:.3g}, {pr.FLOOR[q]}) = {bars[q][c]:.3g}")
    # (b) far from the data, all points
    far = np.array([c == "far" for c in cls])
    if r.m is not None:
        rec.check(bool(np.all(r.m[far] == 0.0)), path, "(b) the mean of a far point is not 0")
    if r.v is not None:
        rec.check(bool(np.all(r.v[far] == sig2)), path, "(b) the variance of a far point is not sigma^2 exactly")
    if r.S is not None:
        Sp = r.S[:P, :P]
        rec.check(bool(np.all(Sp[far][:, ~far] == 0.0)), path, "(b) the covariance of a far point with a near one is not 0")
        # (d)
        rec.check(Sp.tobytes() == np.ascontiguousarray(Sp.T).tobytes(), path, "(d) S is not symmetric in its bits")
        if r.v is not None:
            # (c) all points: the sampled ones carry the bar of their class, the others that of the class's sampled members
            dv = np.abs(r.v - np.diagonal(Sp)) / (EPS * sig2)
            for c in set(cls):
                sel = np.array([k == c for k in cls])
                rec.check(float(np.max(dv[sel])) <= bars["nu"][c], path,
                          f"(c) variance and diagonal of S differ by {np.max(dv[sel]):.3g} eps sigma^2 in class {c}, bar {bars['nu'][c]:.3g}")


def _run_case(H, rec, fam, n, P, ncol, opts, outs, ld, first, path=None, repeat=True):
    el, ek, es = ld
    D = _data(H, fam, n, el)
    xp = _reference(fam, n, P, first, ncol)[0]
    path = path or f"{fam} n={n} P={P} c={ncol} {sorted(route(n, P, ncol, opts, outs)[0] - {'many-point', 'mirror', 'doubling'})}"
    with _Options(H, opts):
        r = _call(H, D, xp, ncol, outs, ek, es)
        _judge(rec, path, D, r, fam, n, P, first, opts, outs)
        if repeat:
            again = _call(H, D, xp, ncol, outs, ek, es)
            rec.check(_bits(again) == _bits(r), path, "a second identical call gives other bits")
    return r


@pytest.mark.parametrize("fam,n,P,ncol,opts,outs,ld,first", LATTICE)
def test_posterior_routes(H, fam, n, P, ncol, opts, outs, ld, first):
    """one case of the lattice: checks (a) .. (f), and the same call again gives the same bits (the first call built the block inverses,
    the second found them)"""
    rec = _Record()
    _run_case(H, rec, fam, n, P, ncol, opts, outs, ld, first)
    rec.finish()


# ---- the same output has the same bits whatever else is asked for and whatever ran before ---------------------------------------------
FILLER = ("B", 1300, 1100)          # 1408 x 1152 padded: both outer blocks of the sweep, S split in 2 x 1152^2 doubles


@pytest.mark.parametrize("fam,n,P,ncol", [("G", 300, 300, 3), ("G", 129, 1, 3), ("B", 128, 128, 4), ("B", 300, 512, 9), ("G", 1300, 300, 1),
                                          ("H", 300, 5, 2)])
def test_bits_do_not_depend_on_the_outputs_asked_for_or_on_history(H, fam, n, P, ncol):
    """mean, variance and S each have the same bits in every combination of outputs (one point: dot_rows / the sweep; many: rows_dot or
    the GEMM route, rows_sumsq_base, the split product), as the first call on a factor or the third, after posterior_prepare or
    without it (128 rows: it returns before building anything), and after unrelated larger calls that leave the handle's scratch, its 128-block inverses and its wide inverses full of
    other numbers (FILLER: a posterior on another factor with more rows, more points and a larger split-K workspace than any case here,
    then a solve of eight columns of NaN through the vector path's scratch)"""
    rec = _Record()
    path = f"{fam} n={n} P={P} c={ncol}"
    D = _data(H, fam, n)
    xp = _reference(fam, n, P, 0, ncol)[0]
    with _Options(H, {}):
        base = _call(H, D, xp, ncol)                    # first call on the factor: builds the inverses
        _judge(rec, path, D, base, fam, n, P, 0, {}, ALL)
        for outs in OUTPUTS:
            r = _call(H, D, xp, ncol, outs)             # second .. sixth
            for k, name in enumerate(ALL):
                if name in outs:
                    rec.check(_bits(r)[k] == _bits(base)[k], path, f"{name} asked for as {outs} has other bits than in {ALL}")
                else:
                    rec.check(_bits(r)[k] is None, path, f"{name} came back unasked")
        H.invalidate_factor()
        H.posterior_prepare(D.L, n)
        r = _call(H, D, xp, ncol)
        rec.check(_bits(r) == _bits(base), path, "other bits after posterior_prepare")
        # an unrelated larger call on another factor, then NaN through the vector path's scratch
        other = _data(H, *FILLER[:2])
        xo = _reference(*FILLER, 0, 1)[0]
        _call(H, other, xo, 1)
        nan8 = H.to_device(np.full((other.npad, 8), np.nan))
        H.potrs(other.L, other.n, nan8, 8)
        H.sync()
        H.invalidate_factor()
        r = _call(H, D, xp, ncol)
        rec.check(_bits(r) == _bits(base), path, "other bits after an unrelated call filled the scratch")
        for outs in (("v",), ("m", "S")):
            H.invalidate_factor()
            r = _call(H, D, xp, ncol, outs)             # first call on the factor again, with fewer outputs
            for k, name in enumerate(ALL):
                if name in outs:
                    rec.check(_bits(r)[k] == _bits(base)[k], path, f"{name} as the first call on a factor ({outs}) has other bits")
    rec.finish()


@pytest.mark.parametrize("fam,n,P", [("B", 300, 512), ("G", 300, 512), ("H", 300, 512), ("G", 700, 1000), ("G", 1300, 300), ("H", 1300, 300)])
def test_halves_and_block_widths_agree_within_the_bar(H, fam, n, P):
    """posterior_halves 0 / 1 (another launch shape of the same products) and posterior_block 1024 / 2048 (another level of the
    doubling; at 1408 padded rows two outer blocks against one) are each held to the reference by _judge, and against each other to ONE
    bar -- per class the larger of the two routes' bars -- over ALL points: the variances in units of eps sigma^2, every entry of
    S[:P, :P] in units of eps (|w_p| |w_q| + sigma^2) with |w_p| from scipy's float64 substitution of all P points (a denominator, good
    to a relative 1e-12), an entry under the larger bar of its two classes.  The bars come from the sampled points of each class.

    The halves must give the BITS of the whole sweep: each half runs the launches of the whole at half the rows and half the workgroup
    slots, fill_split(tiles / 2, 256) = fill_split(tiles, 512) gives every output tile the same K slices (tri_solve.hip), and a row's
    sums do not depend on its neighbours.

    tests/test_gpu_primitives.py holds both pairs to 1e-11 sigma^2 = 4.5e4 eps sigma^2 on a benign factor.  Measured here, 1024- against
    2048-wide blocks, worst entry of S in eps sigma^2 (the PO|...|pair lines): the same bits at 384 padded rows (the doubling stops at
    the same level), 169 on G at n = 700, P = 1000, 780 on G and 657 on H at n = 1300 -- 1.7e-13 sigma^2"""
    rec = _Record()
    D = _data(H, fam, n)
    fx = D.fx
    xp, cls, idx, R = _reference(fam, n, P, 0, 1)
    sig2 = fx.theta[0]
    got = {}
    variants = {"default": {}, "halves0": dict(posterior_halves=0), "block1024": dict(posterior_block=1024)}
    for name, opts in variants.items():
        got[name] = _run_case(H, rec, fam, n, P, 1, opts, ALL, (0, 0, 0), 0, path=f"{fam} n={n} P={P} {name}", repeat=False)
    rec.check(_bits(got["halves0"]) == _bits(got["default"]), f"{fam} n={n} P={P}", "posterior_halves 0 and 1 give different bits")
    wn = pr.w_norms(fx, xp)
    den = EPS * (np.outer(wn, wn) + sig2)
    cls = np.asarray(cls)
    for name in ("halves0", "block1024"):
        nb_a, nb_b = route(n, P, 1)[1], route(n, P, 1, variants[name])[1]
        ba, bb = R.bars(nb_a), R.bars(nb_b)
        a, b = got["default"], got[name]
        if not all(np.all(np.isfinite(t)) for t in (a.S, b.S, a.v, b.v)):
            continue
        bar_nu = np.array([max(ba["nu"][c], bb["nu"][c]) for c in cls])
        bar_sig = np.array([max(ba["sig"][c], bb["sig"][c]) for c in cls])
        dv = np.abs(a.v - b.v) / (EPS * sig2)
        dS = np.abs(a.S[:P, :P] - b.S[:P, :P]) / den
        rv, rS = dv / bar_nu, dS / np.maximum.outer(bar_sig, bar_sig)
        pv, (p1, p2) = int(np.argmax(rv)), np.unravel_index(int(np.argmax(rS)), rS.shape)
        full = float(np.max(np.abs(a.S[:P, :P] - b.S[:P, :P]))) / (EPS * sig2)
        rec.rows.append((f"{fam} n={n} P={P} default against {name}", "pair", f"S {full:.3g} eps sigma^2 (all entries)",
                         f"nu {dv[pv]:.3g} of a bar {bar_nu[pv]:.3g} ({cls[pv]})",
                         f"sig {dS[p1, p2]:.3g} of a bar {max(bar_sig[p1], bar_sig[p2]):.3g} ({cls[p1]}, {cls[p2]})"))
        rec.check(rv[pv] <= 1.0, f"{fam} n={n} P={P} {name}",
                  f"variances differ by {dv[pv]:.3g} eps sigma^2 at point {pv} ({cls[pv]}), bar {bar_nu[pv]:.3g}")
        rec.check(rS[p1, p2] <= 1.0, f"{fam} n={n} P={P} {name}",
                  f"S differs by {dS[p1, p2]:.3g} at ({p1}, {p2}) ({cls[p1]}, {cls[p2]}), bar {max(bar_sig[p1], bar_sig[p2]):.3g}")
    rec.finish()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(H):
    """every status of the entry's argument checks, in the order of the checks, each with kx, mean_out, var_out and S_out left as they
    were; ncol = 129 is -11; set_option("posterior_block", 512) is refused and leaves the option alone"""
    import torch
    from fvgp_amd import _lib
    lib = _lib.lib()
    fx = pr.fixture("B", 129)
    D = _data(H, "B", 129)
    P, ncol = 5, 2
    npad, Pp = D.npad, 128
    xp = H.to_device(pr.points(fx, P)[0])
    theta = np.ascontiguousarray(fx.theta)
    tp = theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    dev = D.x.device
    kx = torch.full((npad * Pp + 2,), SENT, dtype=torch.float64, device=dev)
    m = torch.full((P * 129,), SENT, dtype=torch.float64, device=dev)
    v = torch.full((P,), SENT, dtype=torch.float64, device=dev)
    S = torch.full((Pp * Pp + 2,), SENT, dtype=torch.float64, device=dev)
    alpha129 = H.zeros(npad, 129)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(h=H._h, kid=0, x=p(D.x), n=fx.n, d=2, theta=tp, nt=3, L=p(D.L), ldl=D.L.stride(0), alpha=p(D.alpha(ncol)), ncol=ncol,
                xp=p(xp), P=P, kx=p(kx), ldk=Pp, m=p(m), v=p(v), S=p(S), lds=Pp)
    off8 = lambda t: ctypes.c_void_p(t.data_ptr() + 8)
    refusals = [(-1, dict(h=None)), (-3, dict(x=None)), (-4, dict(n=0)), (-4, dict(n=-5)), (-6, dict(theta=None)),
                (-8, dict(L=None)), (-8, dict(L=off8(D.wide))), (-9, dict(ldl=npad - 2)), (-9, dict(ldl=npad + 1)),
                (-10, dict(alpha=None)), (-11, dict(ncol=0)), (-11, dict(ncol=129, alpha=p(alpha129))), (-12, dict(xp=None)),
                (-13, dict(P=0)), (-14, dict(kx=None)), (-14, dict(kx=off8(kx))), (-15, dict(ldk=Pp - 2)), (-15, dict(ldk=Pp + 1)),
                (-19, dict(lds=Pp - 2)), (-19, dict(lds=Pp + 1)), (-19, dict(S=off8(S))),
                # behind the entry's own checks: the kernel's (csrc/kmat.hip kmat_desc_from_theta)
                (-2, dict(kid=99)), (-7, dict(d=0)), (-9, dict(nt=2))]
    for want, change in refusals:
        a = dict(good, **change)
        rc = lib.fvgp_hip_posterior(a["h"], a["kid"], a["x"], a["n"], a["d"], a["theta"], a["nt"], a["L"], a["ldl"], a["alpha"], a["ncol"],
                                    a["xp"], a["P"], a["kx"], a["ldk"], a["m"], a["v"], a["S"], a["lds"])
        assert rc == want, (change, rc)
        H.sync()
        for t in (kx, m, v, S):
            assert bool(torch.all(t == SENT)), (change, "something was written")
        assert D.unchanged()
    # an S that is not asked for excuses its leading dimension
    a = dict(good, S=None, lds=0)
    assert lib.fvgp_hip_posterior(a["h"], a["kid"], a["x"], a["n"], a["d"], a["theta"], a["nt"], a["L"], a["ldl"], a["alpha"], a["ncol"],
                                  a["xp"], a["P"], a["kx"], a["ldk"], a["m"], a["v"], a["S"], a["lds"]) == 0
    H.sync()
    assert bool(torch.all(S == SENT)) and not bool(torch.any(m[:P * ncol] == SENT)) and bool(torch.all(m[P * ncol:] == SENT))
    for bad in (512, 0, 4096, 1536):
        with pytest.raises(_lib.HipExtensionError):
            H.set_option("posterior_block", bad)
    # the refused values left the option alone: 2048-wide blocks give the bits of a fresh default call
    rec = _Record()
    r1 = _run_case(H, rec, "B", 300, 300, 1, {}, ALL, (0, 0, 0), 0)
    H.set_option("posterior_block", 2048)
    r2 = _run_case(H, rec, "B", 300, 300, 1, {}, ALL, (0, 0, 0), 0)
    rec.check(_bits(r1) == _bits(r2), "B n=300", "a refused posterior_block changed the block width")
    rec.finish()


# ---- the column reductions of the variance's other route --------------------------------------------------------------------------------
def _reduction_cap(depth, terms):
    """(depth + 2) eps sum |terms|: `depth` rounded additions on the longest path of the kernel's summation, one rounding for the
    product that a fused multiply-add does not round, one to spare for the final store"""
    return LD(depth + 2) * LD(EPS) * np.sum(np.abs(terms), axis=0)


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 300])
@pytest.mark.parametrize("cols", [1, 31, 32, 33, 300])
def test_coldot_and_colsumsq_against_longdouble(H, rows, cols):
    """out[p] = sum_i A[i][p] B[i][p] and sum_i V[i][p]^2 at 1, 7, 8, 9, 300 rows (eight row groups per column: fewer rows than groups, one
    each, a ragged second round) and 1, 31, 32, 33, 300 columns (32 columns per workgroup), tight and in a wide leading dimension, the
    output followed by sentinels.  coldot_kernel / colsumsq_kernel: thread (tx, ty) adds rows ty, ty + 8, .. by fma -- ceil(rows / 8)
    additions -- and thread (tx, 0) adds the eight partial sums in sequence -- 8 more: depth ceil(rows / 8) + 8.  Mixed signs in A, B:
    the bound is on sum |terms|, which a cancelling sum does not shrink"""
    import torch
    rng = np.random.default_rng(1000 * rows + cols)
    A = rng.standard_normal((rows, cols)) * np.exp(3 * rng.standard_normal((rows, cols)))
    B = rng.standard_normal((rows, cols))
    depth = -(-rows // 8) + 8
    for extra in (0, 5):
        wideA = H.to_device(np.concatenate([A, np.full((rows, extra), np.nan)], axis=1))
        wideB = H.to_device(np.concatenate([B, np.full((rows, extra + 2), np.nan)], axis=1))
        dA, dB = wideA[:, :cols], wideB[:, :cols]
        assert dA.stride(0) == cols + extra and dB.stride(0) == cols + extra + 2
        out = torch.full((cols + 8,), SENT, dtype=torch.float64, device=dA.device)
        H.coldot(dA, dB, rows, cols, out)
        H.sync()
        got = H.to_host(out)
        terms = np.asarray(A, dtype=LD) * np.asarray(B, dtype=LD)
        err = np.abs(np.asarray(got[:cols], dtype=LD) - np.sum(terms, axis=0))
        assert np.all(got[cols:] == SENT)
        assert np.all(err <= _reduction_cap(depth, terms)), float(np.max(err / (LD(EPS) * np.sum(np.abs(terms), axis=0))))
        out = torch.full((cols + 8,), SENT, dtype=torch.float64, device=dA.device)
        H.colsumsq(dA, out)
        H.sync()
        got = H.to_host(out)
        terms = np.asarray(A, dtype=LD) ** 2
        err = np.abs(np.asarray(got[:cols], dtype=LD) - np.sum(terms, axis=0))
        assert np.all(got[cols:] == SENT) and np.all(got[:cols] >= 0)
        assert np.all(err <= _reduction_cap(depth, terms)), float(np.max(err / (LD(EPS) * np.sum(terms, axis=0))))


@pytest.mark.parametrize("n", [1, 7, 300, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("c", [1, 3])
def test_dot_against_longdouble(H, n, c):
    """fvgp_hip_dot = dot_rows_kernel (the one-point posterior mean runs on it too): one workgroup of 1024 threads, thread t adds the
    elements t, t + 1024, .. of the n c products by fma -- ceil(n c / 1024) additions --, 6 shuffle steps, then thread 0 adds the 16 wave
    sums in sequence: depth ceil(n c / 1024) + 6 + 16.  Tight and in wide leading dimensions"""
    rng = np.random.default_rng(77 * n + c)
    a = rng.standard_normal((n, c)) * np.exp(3 * rng.standard_normal((n, c)))
    b = rng.standard_normal((n, c))
    depth = -(-n * c // 1024) + 6 + 16
    terms = (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)).reshape(-1, 1)
    want, cap = np.sum(terms), _reduction_cap(depth, terms)[0]
    for extra in (0, 3):
        da = H.to_device(np.concatenate([a, np.full((n, extra), np.nan)], axis=1))[:, :c]
        db = H.to_device(np.concatenate([b, np.full((n, extra + 1), np.nan)], axis=1))[:, :c]
        got = H.dot(da, db, n)
        assert abs(LD(got) - want) <= cap, float(abs(LD(got) - want) / (LD(EPS) * np.sum(np.abs(terms))))
    from fvgp_amd import _lib
    with pytest.raises(_lib.HipExtensionError):
        H.dot(da, db, 0)
