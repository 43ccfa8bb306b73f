"""The linear algebra behind the three batched entries -- fvgp_hip_loglik_batch, fvgp_hip_loglik_grad_batch, fvgp_hip_posterior_batch
(csrc/batch_api.hip: batch_recursion with leaf_batch_kernel and the panel TRSM by the explicit block inverse, one lower-tile update per
halving, W = L^-1 by a second halving, KV^-1 = W^T W, the solve-only pass of later prediction chunks) -- against the extended-precision
reference of tests/batch_ref.py, which tests/test_batch_ref_host.py proves on the host.

Fixtures (batch_ref.FAMILY): E benign (noise 1e-2), G and H the ill-conditioned RBF covariances of chol_ref (cond_2 up to 2.4e7 and
8.0e9), U- and U+ their scalings by 2^-400 and 2^400, M a matern32_iso at d = 3.  One call takes one kernel and one x for all its
problems, so each shape makes three calls: rbf_ard with one row per RBF fixture (each row its own theta, V and y: non-zero strides),
matern32_iso with the row M twice (its own copies of V and y; the rows must agree in their bits), and B = 1 (stride 0) on H.  The
factor and gradient tests have one case per (shape, fixture): the device runs once per shape and each case pays for one longdouble
reference only.

KV and work are views with ld = dim + 2 and an even stride above the minimum inside a wider tensor that holds a sentinel; the tiles no
launch may touch -- strictly above the block diagonal in KV, strictly below it in work -- hold NaN.  After every call these tiles and
everything outside the squares must have kept their bits.

Bars (batch_ref.bar), none of them from the device: device <= 8 max(twin "a", twin "c", floor), and the derived caps of chol_ref where
one exists (beta <= 2 (n + 1) max_k cond_2(Lhat_kk), phi <= 64 eps cond_2, lam <= n eps cond_2).  Twin "a" is the float64 numpy copy of
the device's algorithm (explicit block inverses, recursive halving), twin "c" scipy's LAPACK.  Floors: 4 for a measure counted in eps
(beta, resid, bc, dc), 4 eps for a relative one, chol_ref.lam_floor, posterior_ref.FLOOR.  On E the values also keep the tolerances of
the older batch tests (rtol 1e-11 for the value, 1e-10 for log|KV| and the quadratic form).

Every figure prints as `BA|entry|fixture|n|measure|device|twin|ratio` (pytest -s), ratio = device / bar, before anything is asserted."""
import numpy as np
import pytest

import batch_ref as br
import posterior_ref as pr

pytestmark = pytest.mark.gpu

EPS, LD, TILE = br.EPS, br.LD, br.TILE
SENT = 1234.5
RBF = ("E", "G", "H")
# (n, ncol): the smallest shapes that reach each branch of batch_recursion (batch_api.hip) over dim / 128 block columns
SHAPES = [
    (1, 1),        # dim 128: one block column, `blocks <= 1` at the top: no recursion, no update; the leaf has nvalid = 1
    (127, 1),      # dim 128: the appended row 127 is the tile's last row: z comes out of the leaf alone, no TRSM
    (128, 1),      # dim 256 > np = 128: the appended row is row 0 of a second block column whose leaf has nvalid = 0
    (124, 8),      # dim 256: the appended rows 124 .. 131 straddle the tile boundary; component 7 is row 131, past np = 128
    (300, 1),      # dim 384: 3 blocks, odd halving 1 + 2 (mid = 128, then 256)
    (513, 2),      # dim 640: 5 blocks, 2 + 3; one valid row in the last block column
    (700, 1),      # dim 768: 6 blocks, 3 + 3, then 1 + 2 twice
    (897, 1),      # dim 1024: 8 blocks, the full binary tree
    (1300, 1),     # dim 1408: 11 blocks, 5 + 6; chol_ref.COND applies; log-likelihood only
]
GRAD_SHAPES = SHAPES[:-1]
# (n, ncol, P, P_chunk, with S): P = 129 and 300 at P_chunk = 128 send the second (and third) chunk through the solve-only pass
POST_CASES = [(n, ncol, P, 128, P == 20) for n, ncol in ((124, 8), (300, 1), (700, 1)) for P in (1, 20, 129, 300)]
_fail, _slot = [], {}


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _say(entry, fam, n, q, dev, twin, bar):
    """one BA line; a figure above its bar is kept for the assertion at the end of the test"""
    ratio = dev / bar if bar > 0 else (0.0 if dev == 0 else float("inf"))
    print(f"BA|{entry}|{fam}|{n}|{q}|{dev:.3e}|{twin:.3e}|{ratio:.3f}")
    if not ratio <= 1.0:
        _fail.append(f"{entry} {fam} n={n} {q}: device {dev:.3e} > bar {bar:.3e} (twins {twin:.3e})")


def _cached(key, make):
    """the device results of the shape in hand, shared by the cases of its fixtures (one slot: the cases of a shape follow each other)"""
    if _slot.get("key") != key:
        _slot.clear()
        _slot.update(key=key, value=make())
    return _slot["value"]


def _done():
    bad, _fail[:] = list(_fail), []
    assert not bad, "\n".join(bad)


def _inputs(H, fams, n, ncol):
    from fvgp_amd import _lib
    ps = [br.problem(f, n) for f in fams]
    assert all(p.kernel == ps[0].kernel and np.array_equal(p.x, ps[0].x) for p in ps)
    return dict(kernel_id=_lib.KERNEL_IDS[ps[0].kernel], x=H.to_device(ps[0].x), thetas=np.stack([p.theta for p in ps]),
                vdiag=H.to_device(np.stack([p.V for p in ps])), ymean=H.to_device(np.stack([p.y[:, :ncol] for p in ps])))


class _Scratch:
    """B squares of `rows` x dim (ld = dim + 2, two rows more per problem than needed, one problem more than needed) as a view into a
    sentinel-filled tensor; NaN in the tiles strictly above (upper=True) or strictly below the block diagonal of the leading sq x sq"""

    def __init__(self, H, B, rows, dim, sq, upper=True):
        import torch
        self.torch, self.B, self.rows, self.dim = torch, B, rows, dim
        self.buf = H.empty(B + 1, rows + 2, dim + 2)
        self.buf.fill_(SENT)
        t = torch.arange(sq, device=self.buf.device) // TILE
        dead = (t[None, :] > t[:, None]) if upper else (t[None, :] < t[:, None])
        self.buf[:B, :sq, :sq][:, dead] = float("nan")
        self.keep = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)       # what no launch may touch
        live = torch.zeros(rows, dim, dtype=torch.bool, device=self.buf.device)
        live[:sq, :sq] = ~dead
        if upper:
            live[sq:, :] = True                  # the prediction rows under a square
        self.keep[:B, :rows, :dim] = ~live
        self.before = self.buf.clone()
        self.view = self.buf[:B, :rows, :]
        assert self.view.stride(1) == dim + 2 and self.view.stride(0) % 2 == 0 and self.view.stride(0) > rows * (dim + 2)

    def untouched(self):
        i64 = self.torch.int64
        return bool((self.buf.view(i64) == self.before.view(i64))[self.keep].all())

    def host(self, b):
        return self.buf[b, :self.rows, :self.dim].cpu().numpy()


def _loglik(H, fams, n, ncol):
    """one fvgp_hip_loglik_batch call -> (out (B, 3), info, [L (n, n) lower], [z (n, ncol)])"""
    from fvgp_amd import _lib
    dim = _lib.loglik_batch_dim(n, ncol)
    s = _Scratch(H, len(fams), dim, dim, dim)
    out, info = H.loglik_batch(KV=s.view, **_inputs(H, fams, n, ncol))
    H.sync()
    assert s.untouched(), f"loglik_batch wrote outside the lower tiles of its squares ({fams}, n = {n})"
    sq = [s.host(b) for b in range(len(fams))]
    return out, info, [np.tril(a[:n, :n]) for a in sq], [a[n:n + ncol, :n].T.copy() for a in sq]


def _plain_loglik(H, fams, n, ncol):
    from fvgp_amd import _lib
    dim = _lib.loglik_batch_dim(n, ncol)
    return H.loglik_batch(KV=H.empty(len(fams), dim, dim), **_inputs(H, fams, n, ncol))


def _check_values(entry, fam, n, ncol, out, r):
    """{log-likelihood, log|KV|, quad / ncol} against the reference: relative to the magnitudes that enter each, bars from the twins'
    own values"""
    ref = r.out(ncol)
    den = np.array([0.5 * (abs(ref[2]) + abs(ref[1]) + r.n * np.log(2 * np.pi)), abs(ref[1]), abs(ref[2])], dtype=LD)
    den[1] = max(den[1], LD(r.floor("lam") / EPS))          # log|KV| near 0 (n = 1): the rounding of the logarithms is the scale
    den[0] = max(den[0], den[1])
    tw = []
    for t in br.Reference.TWINS:
        L, z = r.L(t), r.twin_z(t)[:, :ncol]
        ld = 2.0 * np.sum(np.log(np.diagonal(L)))
        q = np.sum(z * z) / ncol
        tw.append(np.abs(np.array([-0.5 * (q + ld + r.n * np.log(2 * np.pi)), ld, q], dtype=LD) - ref) / den)
    dev = np.abs(np.asarray(out, dtype=LD) - ref) / den
    for i, q in enumerate(("value", "logdet", "quad")):
        d = float(dev[i]) if np.isfinite(out[i]) else float("inf")
        _say(entry, fam, n, q, d, float(max(t[i] for t in tw)), br.bar([float(t[i]) for t in tw], br.FLOOR_EPS * EPS))
    if fam == "E":
        ref64 = np.asarray(ref, dtype=np.float64)
        np.testing.assert_allclose(out[0], ref64[0], rtol=1e-11)
        np.testing.assert_allclose(out[1:], ref64[1:], rtol=1e-10, atol=1e-300)


# ---- fvgp_hip_loglik_batch ------------------------------------------------------------------------------------------------------------
def _loglik_case(H, n, ncol):
    """the three calls of a shape -> {fixture: (out row, L, z)}, "H/B1" the call with B = 1"""
    res = {}
    for fams in (RBF + ("U-", "U+"), ("M", "M"), ("H",)):
        out, info, Ls, zs = _loglik(H, fams, n, ncol)
        assert np.all(info == 0) and np.all(np.isfinite(out)), (fams, info, out)
        if fams == ("M", "M"):
            assert out[0].tobytes() == out[1].tobytes() and Ls[0].tobytes() == Ls[1].tobytes() and zs[0].tobytes() == zs[1].tobytes()
        for b, fam in enumerate(fams):
            res[fam if len(fams) > 1 else fam + "/B1"] = (out[b], Ls[b], zs[b])
    return res


@pytest.mark.parametrize("fam", RBF + ("U-", "U+", "M"))
@pytest.mark.parametrize("n,ncol", SHAPES)
def test_loglik_batch_factor_and_values(H, n, ncol, fam):
    """L and z^T read back from KV: beta, phi, lam, z; the three outputs; U- and U+ under G's scale-free bars, finite, info = 0.  The
    device runs once per shape (all fixtures); a case measures one fixture, H also its B = 1 call."""
    from fvgp_amd import _lib
    dim = _lib.loglik_batch_dim(n, ncol)
    res = _cached(("loglik", n, ncol), lambda: _loglik_case(H, n, ncol))
    r = br.reference(fam, n)
    for key in (fam, "H/B1") if fam == "H" else (fam,):
        out, L, z = res[key]
        entry = "loglik_batch" + key[len(fam):]
        assert np.all(np.isfinite(L)) and np.all(np.isfinite(z))
        got = r.measure_factor(L, z, dim)
        for q, (twin, bar) in r.factor_bars(ncol, dim).items():
            _say(entry, fam, n, q, got[q], twin, bar)
        _check_values(entry, fam, n, ncol, out, r)
    _done()


# ---- fvgp_hip_loglik_grad_batch -------------------------------------------------------------------------------------------------------
def _grad(H, fams, n, ncol, c):
    from fvgp_amd import _lib
    dim, npd, B = _lib.loglik_batch_dim(n, ncol), _lib.pad128(n), len(fams)
    kv, wk = _Scratch(H, B, dim, dim, dim), _Scratch(H, B, npd, npd, npd, upper=False)
    bo, do = H.empty(B, n), H.empty(B, n)
    out, grad, info = H.loglik_grad_batch(KV=kv.view, work=wk.view, component=c, b_out=bo, diag_out=do, **_inputs(H, fams, n, ncol))
    H.sync()
    assert kv.untouched(), f"loglik_grad_batch wrote outside the lower tiles of KV ({fams}, n = {n})"
    assert wk.untouched(), f"loglik_grad_batch wrote outside the upper tiles of work ({fams}, n = {n})"
    res = []
    for b in range(B):
        res.append(dict(KVinv=np.tril(kv.host(b)[:n, :n]), W=np.triu(wk.host(b)[:n, :n]).T.copy(), b=bo[b].cpu().numpy(),
                        diag=do[b].cpu().numpy(), g=grad[b]))
    return out, grad, info, res


def _grad_case(H, n, ncol):
    """the three calls of a shape for component 0 and ncol - 1 -> {(component, fixture): results}, "H/B1" the call with B = 1"""
    res = {}
    for c in sorted({0, ncol - 1}):
        for fams in (RBF, ("M", "M"), ("H",)):
            out, grad, info, rs = _grad(H, fams, n, ncol, c)
            vout, vinfo = _plain_loglik(H, fams, n, ncol)
            assert np.all(info == 0) and np.all(vinfo == 0), (fams, info, vinfo)
            assert out.tobytes() == vout.tobytes(), f"out differs from loglik_batch's in its bits ({fams}, n = {n}, component {c})"
            if fams == ("M", "M"):
                assert all(rs[0][k].tobytes() == rs[1][k].tobytes() for k in rs[0])
            for b, fam in enumerate(fams):
                res[(c, fam if len(fams) > 1 else fam + "/B1")] = rs[b]
    return res


@pytest.mark.parametrize("fam", RBF + ("M",))
@pytest.mark.parametrize("n,ncol", GRAD_SHAPES)
def test_grad_batch_inverse_and_gradient(H, n, ncol, fam):
    """for component 0 and ncol - 1: out bit-equal to loglik_batch; W^T (upper tiles of work), KV^-1 (lower tiles of KV), b_out,
    diag_out and the gradient against the reference.  The device runs once per shape; a case measures one fixture, H also its B = 1
    call."""
    res = _cached(("grad", n, ncol), lambda: _grad_case(H, n, ncol))
    r = br.reference(fam, n)
    for c in sorted({0, ncol - 1}):
        for key in (fam, "H/B1") if fam == "H" else (fam,):
            rs = res[(c, key)]
            assert all(np.all(np.isfinite(v)) for v in rs.values())
            got = r.measure_grad(c, **rs)
            for q, (twin, bar) in r.grad_bars(c).items():
                _say(f"loglik_grad_batch/c{c}" + key[len(fam):], fam, n, q, got[q], twin, bar)
    _done()


# ---- fvgp_hip_posterior_batch ---------------------------------------------------------------------------------------------------------
def _posterior(H, fams, n, ncol, xp, pc, want_S, inputs=None):
    from fvgp_amd import _lib
    dim, B, P = _lib.loglik_batch_dim(n, ncol), len(fams), len(xp)
    Pp = _lib.pad128(P)
    kv = _Scratch(H, B, dim + pc, dim, dim)
    mean, var = H.empty(B, P, ncol), H.empty(B, P)
    S = H.empty(B, Pp, Pp) if want_S else None
    out, info = H.posterior_batch(xpred=H.to_device(xp), KV=kv.view, mean_out=mean, var_out=var, S_out=S, want_loglik=True,
                                  **(_inputs(H, fams, n, ncol) if inputs is None else inputs))
    H.sync()
    assert kv.untouched(), f"posterior_batch wrote outside its squares and prediction rows ({fams}, n = {n}, P = {P})"
    return dict(out=out, info=info, mean=mean.cpu().numpy(), var=var.cpu().numpy(), S=None if S is None else S.cpu().numpy()[:, :P, :P])


def _measure_posterior(entry, fam, n, ref, m, v, S):
    got, bars = ref.measure(m, v, S), ref.bars()
    for q in got:
        for k, d in got[q].items():
            _say(entry, fam, n, f"{q}.{k}", d, *bars[q][k])
    return bars


@pytest.mark.parametrize("n,ncol,P,pc,want_S", POST_CASES)
def test_posterior_batch_mean_variance_covariance(H, n, ncol, P, pc, want_S):
    """mean, variance and S per point class against the reference; far points exactly prior; S bitwise symmetric and finite; the
    variance against diag(S) of the same call; the points of later chunks (the solve-only pass) against the reference on their own"""
    for fams in (RBF, ("M", "M"), ("H",)):
        r0 = br.reference(fams[0], n)
        xp, cls = br.points(r0, P)
        res = _posterior(H, fams, n, ncol, xp, pc, want_S)
        vout, _ = _plain_loglik(H, fams, n, ncol)
        assert np.all(res["info"] == 0) and res["out"].tobytes() == vout.tobytes()
        if fams == ("M", "M"):
            assert all(res[k][0].tobytes() == res[k][1].tobytes() for k in ("mean", "var") + (("S",) if want_S else ()))
            fams = ("M",)
        tag = "" if len(fams) > 1 or fams == ("M",) else "/B1"
        idx = pr.sample_points(P)
        late = [i for i in idx if i >= pc]
        far = np.array([c == "far" for c in cls])
        for b, fam in enumerate(fams):
            r = br.reference(fam, n)
            m, v, S = res["mean"][b], res["var"][b], None if not want_S else res["S"][b]
            assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
            assert np.all(m[far] == 0.0) and np.all(v[far] == r.p.theta[0])
            ref = br.PosteriorReference(r, xp[idx], [cls[i] for i in idx], ncol)
            bars = _measure_posterior("posterior_batch" + tag, fam, n, ref, m[idx], v[idx], None if S is None else S[np.ix_(idx, idx)])
            if S is not None:
                assert np.all(np.isfinite(S)) and S.tobytes() == S.T.copy().tobytes()
                dv = np.abs(np.asarray(v, dtype=LD) - np.diagonal(S)) / (EPS * r.p.theta[0])
                for k in sorted(set(cls)):
                    sel = np.array([c == k for c in cls])
                    _say("posterior_batch" + tag, fam, n, f"var-diagS.{k}", float(np.max(dv[sel])), *bars["nu"][k])
            if late and fam in ("G", "H"):
                ref2 = br.PosteriorReference(r, xp[late], [cls[i] for i in late], ncol)
                _measure_posterior("posterior_batch/solve_only" + tag, fam, n, ref2, m[late], v[late], None)
    _done()


# ---- info -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ncol,js", [(513, 1, (0, 127, 128, None, 300, 512)), (124, 8, (123, None))])
def test_info_names_the_first_bad_pivot(H, n, ncol, js):
    """E with V[j_b] = -10 in problem b (None: clean): info[b] = j_b + 1 exactly and NaN results in all three entries; the clean
    problem's results are those of its solo call in their bits"""
    from fvgp_amd import _lib
    p = br.problem("E", n)
    B, clean = len(js), js.index(None)
    V = np.tile(p.V, (B, 1))
    for b, j in enumerate(js):
        if j is not None:
            V[b, j] = -10.0
    want = np.array([0 if j is None else j + 1 for j in js])
    bad = want != 0
    xp, _ = br.points(br.reference("E", n), 20)

    def inputs(rows):
        return dict(kernel_id=_lib.KERNEL_IDS[p.kernel], x=H.to_device(p.x), thetas=np.tile(p.theta, (len(rows), 1)),
                    vdiag=H.to_device(V[rows]), ymean=H.to_device(np.stack([p.y[:, :ncol]] * len(rows))))

    def run(rows):
        dim, npd, Bs = _lib.loglik_batch_dim(n, ncol), _lib.pad128(n), len(rows)
        out, info = H.loglik_batch(KV=H.empty(Bs, dim, dim), **inputs(rows))
        bo, do = H.empty(Bs, n), H.empty(Bs, n)
        gout, grad, ginfo = H.loglik_grad_batch(KV=H.empty(Bs, dim, dim), work=H.empty(Bs, npd, npd), component=ncol - 1, b_out=bo,
                                                diag_out=do, **inputs(rows))
        post = _posterior(H, rows, n, ncol, xp, 128, True, inputs(rows))
        return dict(out=out, info=info, gout=gout, grad=grad, ginfo=ginfo, b=bo.cpu().numpy(), diag=do.cpu().numpy(), pout=post["out"],
                    pinfo=post["info"], mean=post["mean"], var=post["var"], S=post["S"])

    full, solo = run(list(range(B))), run([clean])
    for k in ("info", "ginfo", "pinfo"):
        print(f"BA|info|E|{n}|{k}|{full[k].tolist()}|{want.tolist()}|-")
        assert np.array_equal(full[k], want), (k, full[k], want)
    for k in ("out", "gout", "grad", "pout", "mean", "var", "S"):
        assert np.all(np.isnan(full[k][bad])), k
        assert full[k][clean].tobytes() == solo[k][0].tobytes(), k
        assert np.all(np.isfinite(full[k][clean])), k
    for k in ("b", "diag"):
        assert full[k][clean].tobytes() == solo[k][0].tobytes(), k


# ---- the split of B into groups of 65535 ----------------------------------------------------------------------------------------------
def test_group_split_of_the_batch(H):
    """B = 65537 problems of n = 1: two groups (65535 + 2) with their pointer offsets.  Every row against the closed form
    -1/2 (y^2 / (s + v) + log(s + v) + log 2 pi) to 4 eps relative; the rows 65534 .. 65536 equal to their solo calls in their bits.
    s + v lies in [1.1, 3.1] and |y| <= 1, so every term of the sum is positive and the value stays away from 0."""
    import torch
    B = 65537
    rng = np.random.default_rng(65537)
    x = np.array([[0.25, 0.75]])
    thetas = np.column_stack([1.0 + rng.random(B), 0.1 + rng.random(B), 0.1 + rng.random(B)])
    V = 0.1 + rng.random((B, 1))
    Y = rng.uniform(-1.0, 1.0, (B, 1, 1))
    xd, Vd, Yd = H.to_device(x), H.to_device(V), H.to_device(Y)
    KV = H.empty(B, TILE, TILE)                                        # 8.6 GB
    try:
        out, info = H.loglik_batch(0, xd, thetas, Vd, Yd, KV)
    finally:
        del KV
        torch.cuda.empty_cache()
    assert np.all(info == 0)
    a = np.asarray(thetas[:, 0], dtype=LD) + np.asarray(V[:, 0], dtype=LD)
    a = np.asarray(np.asarray(a, dtype=np.float64), dtype=LD)          # the entry adds in float64: A = fl(s + v)
    ref = -LD(0.5) * (np.asarray(Y[:, 0, 0], dtype=LD) ** 2 / a + np.log(a) + br._log2pi())
    err = np.abs(np.asarray(out[:, 0], dtype=LD) - ref) / np.abs(ref) / EPS
    worst = int(np.argmax(err))
    print(f"BA|loglik_batch/groups|closed form|1|value|{float(err[worst]):.3f} eps at row {worst}|-|{float(err[worst]) / 4:.3f}")
    print(f"BA|loglik_batch/groups|closed form|1|value, second group|{float(np.max(err[65535:])):.3f} eps|-|{float(np.max(err[65535:])) / 4:.3f}")
    assert np.all(np.isfinite(out)) and float(err[worst]) <= 4.0
    for b in (65534, 65535, 65536):
        alone, ainfo = H.loglik_batch(0, xd, thetas[b:b + 1], Vd[b:b + 1], Yd[b:b + 1], H.empty(1, TILE, TILE))
        assert ainfo[0] == 0 and alone[0].tobytes() == out[b].tobytes(), b
