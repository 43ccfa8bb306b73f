"""Cases, bars and the one runner of the row-sharded tests (a helper module of the tests, not a conftest): no new reference.

The longdouble reference and the float64 twins are batch_ref's (problem / reference / points / PosteriorReference / loglik_ld), the
factor measures chol_ref's.  Here: the geometry table -- the smallest (world, panel, n) that reaches each branch of
fvgp_amd/csrc/dist_driver.h, each reason derived from the driver's arithmetic --, the selection of the twins, and run() with full_body(), which
drive ShardedGP through every entry on any ops factory: the CPU twin of the ABI (tests/dist_stub_ops.StubOps, the same driver over host
loops; tests/test_sharded_host.py) or the HIP kernels (tests/test_gpu_sharded_accuracy.py: the one-rank geometries only).  More than one
rank runs as threads of this process under tests/dist_ranks.py -- on the host only: with one HIP handle per thread in one process the
four-rank cases ended in an abandoned launch of the resident panel kernel (the spin-wait hand-off of chain.hip chain_wait gave up and
stored info = 0x7fffffff) and a memory fault, and until that cause is found no multi-rank case may run on a device under the harness.

Twins.  The factor: chol_ref.twin_chol(A64, 16) -- fvgp_hip_panel_potrf_dev substitutes over 16-column tiles while at most
leaf_tiles_rows = 4096 rows lie below a block (api.hip panel_factor: `tiles = leaf_tiles && R <= leaf_tiles_rows`), which every case here
is; tests/test_gpu_chol.py assigns the same twin to that entry (its path 10) -- and scipy's LAPACK; beta capped by 2 (n + 1) (no explicit
128-inverse), phi by 64 eps cond_2, lam by n eps cond_2.  The scalars, alpha, diag(KV^-1), the gradient and the posterior: batch_ref's
twins "a" and "c".  The kernel-id cases, which have no batch_ref fixture: scipy and schedule_twin, the float64 copy of the sharded
schedule itself.  Bars: batch_ref.bar = 8 max(twins, floor), never from a device figure.

Every figure prints as `SD|entry|world|panel|fixture|n|measure|device|twin|ratio`, ratio = device / bar, before anything is asserted;
the failures of a case are collected and raised together (done())."""
import threading

import numpy as np

import batch_ref as br
import chol_ref
import kernel_family_ref as kf
import posterior_ref as pr

EPS, LD, TILE = br.EPS, br.LD, br.TILE
INPLACE, FORCED = "in place", "forced"          # one rank: the panels factored in A itself / through the panel buffers and collectives

# (world, mode, panel, n): np = padded n, nblk = np / 128 blocks dealt block b -> rank b mod P, nbw = blocks of a panel,
# per = ceil((panel / 128) / P) blocks of a diagonal block a rank sends at most
GEOMETRY = [
    (1, INPLACE, 128, 1),     # one block, one panel, n_valid = 1; `!general`: panel_potrf on A itself, no update
    (1, INPLACE, 256, 300),   # np = 384: panels [0, 256), [256, 384): the ragged last one w = 128 with n_valid = 300 - 256 = 44; the in-place `update`
    (1, INPLACE, 512, 300),   # one panel clipped by bnd() to np: w = 384 < NB, n_valid = 300
    (1, FORCED, 128, 300),    # per = 1, nbw = 1 = P, b0 % 1 == 0: every panel's all-gather lands in D in place; Dfac; the library's copy path
    (1, FORCED, 256, 513),    # np = 640: per = 2, so the gather is staged (G) and block-copied on every panel; last panel w = 128, n_valid = 1
    (2, None, 256, 300),      # panel 0: per = 1, nbw = 2 = P, b0 = 0: in place; panel 1: nbw = 1 != P: staged.  Rank 1's second local block
                              # is global block 3 >= nblk = 3: zero rows (assemble's `rows <= 0`)
    (2, None, 128, 513),      # nblk = 5 (odd): rank 0 owns 3 blocks, rank 1 two and one past the matrix; every panel narrower than P blocks
    (3, None, 128, 700),      # panel 1 (b0 = 1, b1 = 2): L0 = 2 / 3 = 0, on rank 0 la = ceil(1 / 3) = 1 > L0: local block 0 lies above the panel
                              # and is zeroed in `low`; again at b0 = 4 (L0 = 1, la = 2)
    (3, None, 256, 513),      # np = 640: per = 1, nbw = 2 != P; panel 0 holds blocks 0, 1: rank 2 has la = lb = 0, sends nothing; rank 2 owns
                              # block 2 and block 5 >= nblk = 5
    (3, None, 512, 700),      # np = 768: per = 2; of panel 0's blocks 0 .. 3 rank 0 sends two, ranks 1 and 2 one each; last panel w = 256
    (4, None, 512, 897),      # np = 1024: per = 1, nbw = 4 = P, b0 = 0 and 4: both panels gathered in place (the 8 x 1024 layout scaled down)
    (4, None, 128, 129),      # nblk = 2, nb_max = 1: ranks 2 and 3 hold blocks 2, 3 >= nblk: nv = 0, x_loc is None
    (3, None, 128, 1),        # nblk = 1: ranks 1 and 2 own nothing; a single entry
    (2, None, 256, 128),      # np = 128 < NB: w clipped to 128, n_valid = w
    (2, None, 256, 127),      # the same with n_valid = w - 1
]
HARD = [(1, FORCED, 128, 300), (3, None, 128, 700), (3, None, 512, 700)]
# (geometry, fixture, ncol) of the factor / value / backward-solve test
FACTOR_CASES = ([(g, "E", 1) for g in GEOMETRY] + [(g, f, 1) for g in HARD for f in ("G", "H")]
                + [((2, None, 256, 300), f, 1) for f in ("U-", "U+")] + [((2, None, 128, 513), "M", 1), ((1, INPLACE, 256, 300), "M", 1)]
                + [((2, None, 128, 300), "E", 8), ((3, None, 256, 513), "E", 8)])
OTHER_KERNELS = [("matern32_ard", 1), ("matern52_ard", 4), ("rbf_iso", 5), ("matern52_iso", 16)]      # the names no fixture uses, one d each

_fail = []
_print_lock = threading.Lock()


def case_id(geom, fam=None, ncol=None):
    world, mode, panel, n = geom
    s = f"P{world}{'' if mode is None else '-' + mode.replace(' ', '')}-nb{panel}-n{n}"
    return s + ("" if fam is None else f"-{fam}") + ("" if ncol in (None, 1) else f"-c{ncol}")


def say(entry, geom, fam, q, dev, twin, bar):
    """one SD line; a figure above its bar is kept for done()"""
    world, mode, panel, n = geom
    ratio = dev / bar if bar > 0 else (0.0 if dev == 0 else float("inf"))
    with _print_lock:
        print(f"SD|{entry}|{world}{'' if mode is None else ' ' + mode}|{panel}|{fam}|{n}|{q}|{dev:.3e}|{twin:.3e}|{ratio:.3f}", flush=True)
        if not ratio <= 1.0:
            _fail.append(f"{entry} {case_id(geom, fam)} {q}: device {dev:.3e} > bar {bar:.3e} (twins {twin:.3e})")


def check(ok, what):
    if not ok:
        _fail.append(what)


def done():
    bad, _fail[:] = list(_fail), []
    assert not bad, "\n".join(bad)


def bounds_of(geom):
    """the panel and 128-block boundaries inside the matrix"""
    _, _, panel, n = geom
    return sorted({b for b in list(range(TILE, n, TILE)) + list(range(panel, n, panel))})


# ---- running a case -----------------------------------------------------------------------------------------------------------------
def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def run(geom, make_ops, body, close_ops=None):
    """body(gp_factory, rank) on every rank of the geometry -> the list of the ranks' results.  gp_factory(**kw) builds the rank's
    ShardedGP(x, y, V, kernel=...) with rank, world, panel, ops and collectives filled in."""
    from fvgp_amd.dist import ShardedGP
    import dist_ranks
    world, mode, panel, n = geom
    made = []
    _fail[:] = []                                            # what a case that raised before done() left behind is not this case's

    def ops_of(r):
        made.append(make_ops(r))
        return made[-1]

    def rank_body(r, ops, coll):
        def factory(x, y, V, kernel):
            return ShardedGP(x, y, V, kernel=kernel, ops=ops, panel=panel, rank=r, world=world, collectives=coll,
                             force_collectives=(mode == FORCED))
        return body(factory, r)

    try:
        if world == 1:
            return [rank_body(0, ops_of(0), "torch")]
        return dist_ranks.run_ranks(world, ops_of, rank_body)
    finally:
        if close_ops is not None:
            for o in made:
                close_ops(o)


def poison(gp):
    """NaN in what the driver states is written before it is read, or never read: the panel buffers and, in the rank's rows of A,
    everything to the right of each block's diagonal tile"""
    nan = float("nan")
    for t in list(gp._T) + list(gp._recv) + [gp._Dfac, gp._gather]:
        if t is not None:
            t.fill_(nan)
    for l in range(gp.nb_max):
        c = (l * gp.P + gp.p + 1) * TILE
        if c < gp.np_:
            gp.A[l * TILE:(l + 1) * TILE, c:].fill_(nan)


def gathered_nans(gp):
    """NaN in what the last all-gather into each recv buffer wrote: rows that lie above a panel on some rank are solved and gathered
    like the rest, and the driver zeroes them first (`la > L0`) so that nothing stale travels"""
    bad = 0
    for i in range(2 if gp.general else 0):
        Js = [J for J in range(gp.npan - 1) if J % 2 == i]          # the last panel gathers nothing
        if Js:
            w, L0 = gp.bnd[Js[-1] + 1] - gp.bnd[Js[-1]], (gp.bnd[Js[-1] + 1] // TILE) // gp.P
            bad += int(gp._recv[i][:gp.P * (gp.nb_max - L0) * TILE * w].isnan().sum())
    return bad


def full_body(p, ncol, theta=None, slabs=(), components=(0,), xpred=None, want_diag=True, want_factor=True, kernel=None, V=None,
              poisoned=False, repeat=False, refusal=False):
    """the body that drives every entry once: evaluate (+ alpha), the gathered factor, log_likelihood (+ the refusals after it), the
    gradient at each (component, slab) twice, the posterior with and without S.  Everything comes back as host arrays."""
    theta = p.theta if theta is None else theta

    def body(factory, rank):
        gp = factory(p.x, p.y[:, :ncol], np.array(p.V if V is None or np.ndim(V) == 2 else V), p.kernel if kernel is None else kernel)
        gp.set_targets(p.y[:, :ncol], p.V if V is None else V)
        if poisoned:
            poison(gp)
        out = {"scalars": np.array(gp.evaluate(theta, want_alpha=True)), "alpha": host(gp.alpha)[:p.n, :ncol]}
        if poisoned:
            out["gathered_nan"] = gathered_nans(gp)
        if want_factor:
            out["L"] = gp.factor_matrix()
        for c in components:
            for slab in slabs:
                if callable(gp.kernel_callable):
                    break
                g, dg = gp.gradient(component=c, slab=slab, want_diag=True)
                g2, dg2 = gp.gradient(component=c, slab=slab, want_diag=True)
                out[("grad", c, slab)] = (g, dg, g.tobytes() == g2.tobytes() and dg.tobytes() == dg2.tobytes())
        if want_diag and not slabs and not callable(gp.kernel_callable):
            out["diag"] = gp.gradient(component=0, slab=2048, want_diag=True)[1]
        if callable(gp.kernel_callable):
            try:
                gp.gradient()
                out["grad_refused"] = False
            except NotImplementedError:
                out["grad_refused"] = True
        if xpred is not None:
            m, S = gp.posterior(xpred)
            m2, S2 = gp.posterior(xpred, want_cov=False)
            out["post"] = (m, S, m.tobytes() == m2.tobytes() and S2 is None)
        if repeat:                                   # theta, 1.3 theta, theta again on the one object
            gp.evaluate(1.3 * theta, want_alpha=True)
            out["again"] = (np.array(gp.evaluate(theta, want_alpha=True)), host(gp.alpha)[:p.n, :ncol])
        if refusal:
            out["ll_only"] = np.array(gp.log_likelihood(theta))
            out["refused"] = _refusals(gp)
        return out
    return body


def _refusals(gp):
    """after log_likelihood (keep_factor = 0): the methods through `theta is None`, the ABI entry with status -2 on real buffers"""
    res = {}
    for name, call in (("posterior", lambda: gp.posterior(gp.x_host[:1])), ("gradient", gp.gradient)):
        try:
            call()
            res[name] = "ran"
        except AssertionError:
            res[name] = "AssertionError"
    o = gp.ops
    assert gp._desc.keep_factor == 0 and gp.theta is None
    alpha, ws = o.zeros(gp.np_, TILE), o.zeros(o.dist_scratch(gp._desc, 0))
    try:
        o.solve_dist(gp._desc, alpha, ws)
        res["abi"] = "ran"
    except RuntimeError as e:
        res["abi"] = "-2" if "status -2" in str(e) else str(e)
    res["alpha_untouched"] = bool((alpha == 0).all())
    return res


# ---- judging ------------------------------------------------------------------------------------------------------------------------
def ranks_agree(entry, geom, fam, results, keys=None):
    """the replicated outputs of all ranks are equal in their bits"""
    def flat(v):
        if isinstance(v, np.ndarray):
            return v.tobytes()
        if isinstance(v, (tuple, list)):
            return tuple(flat(a) for a in v)
        return v
    for k in results[0]:
        if keys is not None and k not in keys:
            continue
        for r, res in enumerate(results[1:], 1):
            check(flat(res[k]) == flat(results[0][k]), f"{entry} {case_id(geom, fam)}: rank {r} differs from rank 0 in the bits of {k}")


def judge_values(entry, geom, fam, ncol, out, r):
    """{log-likelihood, log|KV|, quad / ncol}: relative to the magnitudes that enter each; bars from the twins' own values"""
    ref = r.out(ncol)
    den = np.array([0.5 * (abs(ref[2]) + abs(ref[1]) + r.n * np.log(2 * np.pi)), abs(ref[1]), abs(ref[2])], dtype=LD)
    # the scale of log|KV| is never below n + sum |log L_ii| (lam_floor / eps: the rounding of the n logarithms and of their sum): what
    # matters at n = 1, where log|KV| is near 0; at the larger n it applies too and makes this bar about four times the factor's lam bar
    # (both about 1e-14 relative)
    den[1] = max(den[1], LD(r.floor("lam") / EPS))
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
        say(entry, geom, fam, q, d, float(max(t[i] for t in tw)), br.bar([float(t[i]) for t in tw], br.FLOOR_EPS * EPS))
    if fam == "E":                                           # the older tolerance of tests/test_gpu_dist.py stays
        check(abs(out[0] - float(ref[0])) <= 1e-10 * abs(float(ref[0])), f"{entry} {case_id(geom, fam)}: value off by more than 1e-10 relative")


def judge_factor(entry, geom, fam, L, r):
    """beta over edge_rows(n, the case's panel and block boundaries) and the whole diagonal, phi over all rows, lam"""
    n = r.n
    check(L.shape == (n, n) and bool(np.all(np.isfinite(L))), f"{entry} {case_id(geom, fam)}: the factor is not finite")
    rows = chol_ref.edge_rows(n, bounds=bounds_of(geom))
    C = r.chol
    fig = {"beta": lambda F: chol_ref.beta(r.p.A, F, rows), "phi": lambda F: chol_ref.phi(F, r.Lhat), "lam": lambda F: chol_ref.lam(F, r.Lhat)}
    cap = {"beta": C.cap_beta(False), "phi": C.cap_phi(), "lam": C.cap_lam()}
    for q, f in fig.items():
        tw = [f(C.factor(t)) for t in (16, "scipy")]
        say(entry, geom, fam, q, f(L), max(tw), br.bar(tw, r.floor(q), cap[q]))


def judge_solve(entry, geom, fam, r, c, alpha=None, diag=None, g=None):
    got = r.measure_grad(c, b=None if alpha is None else alpha[:, c], diag=diag, g=g)
    bars = r.grad_bars(c)
    for q, v in got.items():
        say(entry, geom, fam, q, v, *bars[q])
    if fam == "E" and alpha is not None:                     # tests/test_gpu_dist.py: 1e-8 on KVinvY
        ref = np.asarray(r.alpha[:, c], dtype=np.float64)
        check(np.max(np.abs(alpha[:, c] - ref)) <= 1e-8 * np.max(np.abs(ref)), f"{entry} {case_id(geom, fam)}: KVinvY off by more than 1e-8")
    if fam == "E" and g is not None:
        gh = np.asarray(r.grad(c)[0], dtype=np.float64)
        check(bool(np.all(np.abs(g - gh) <= 1e-8 * np.abs(gh) + 1e-9 * np.max(np.abs(gh)))), f"{entry} {case_id(geom, fam)}: gradient off by more than 1e-8")


def posterior_case(r, npred):
    """(xpred, sampled indices, the classes of all points) for batch_ref.points(r, npred)"""
    xp, cls = br.points(r, npred)
    idx = pr.sample_points(npred)
    return xp, idx, cls


def judge_posterior(entry, geom, fam, r, ncol, xp, idx, cls, m, S):
    check(bool(np.all(np.isfinite(m)) and np.all(np.isfinite(S))), f"{entry} {case_id(geom, fam)}: the posterior is not finite")
    ref = br.PosteriorReference(r, xp[idx], [cls[i] for i in idx], ncol)
    Ss = S[np.ix_(idx, idx)]
    got, bars = ref.measure(m[idx], np.diagonal(Ss).copy(), Ss), ref.bars()
    for q in got:
        for k, d in got[q].items():
            say(entry, geom, fam, f"{q}.{k}", d, *bars[q][k])


def judge_full(entry, geom, fam, ncol, results, r, xpred_case=None):
    """everything full_body returned on rank 0 against the reference; all ranks against rank 0 in their bits"""
    res = results[0]
    ranks_agree(entry, geom, fam, results)
    judge_values(entry, geom, fam, ncol, res["scalars"], r)
    if "L" in res:
        judge_factor(entry, geom, fam, res["L"], r)
    for c in sorted({0, ncol - 1}):
        judge_solve(entry, geom, fam, r, c, alpha=res["alpha"], diag=res.get("diag") if c == 0 else None)
    slabs = {}
    for k, v in res.items():
        if isinstance(k, tuple) and k[0] == "grad":
            _, c, slab = k
            g, dg, same = v
            check(same, f"{entry} {case_id(geom, fam)}: the gradient at slab {slab} differs between two identical calls")
            judge_solve(f"{entry}/c{c}/slab{slab}", geom, fam, r, c, diag=dg, g=g)
            slabs.setdefault(c, []).append(g)
    for c, gs in slabs.items():                              # all slabs within the bar of each other: relative to M like the measure
        M = r.grad(c)[1]
        spread = max(br.grad_err(a, np.asarray(b, dtype=LD), M) for a in gs for b in gs)
        say(f"{entry}/c{c}", geom, fam, "slab spread", spread, *r.grad_bars(c)["grad"])
    if "post" in res:
        xp, idx, cls = xpred_case
        m, S, same = res["post"]
        check(same, f"{entry} {case_id(geom, fam)}: want_cov=False changes the mean's bits or returns a covariance")
        judge_posterior(f"{entry}/P{len(xp)}", geom, fam, r, ncol, xp, idx, cls, m, S)
    if "gathered_nan" in res:
        check(all(o["gathered_nan"] == 0 for o in results), f"{entry} {case_id(geom, fam)}: NaN among the gathered panel rows: "
              f"{[o['gathered_nan'] for o in results]}")
    if "again" in res:
        s, a = res["again"]
        check(s.tobytes() == res["scalars"].tobytes() and a.tobytes() == res["alpha"].tobytes(),
              f"{entry} {case_id(geom, fam)}: theta after 1.3 theta does not give the first result's bits")
    if "ll_only" in res:
        check(res["ll_only"].tobytes() == res["scalars"].tobytes(), f"{entry} {case_id(geom, fam)}: log_likelihood differs from evaluate in its bits")
        want = {"posterior": "AssertionError", "gradient": "AssertionError", "abi": "-2", "alpha_untouched": True}
        check(res["refused"] == want, f"{entry} {case_id(geom, fam)}: after keep_factor = 0: {res['refused']}")


# ---- not positive definite ----------------------------------------------------------------------------------------------------------
def npd_rows(geom):
    """i0 in the first panel; the first row of a later panel (owned by rank 1 where there is one); the last row"""
    _, _, panel, n = geom
    return [77, panel, n - 1]


def npd_body(p, i0s):
    """V[i0] = -(sigma^2 + 1) for each i0 in turn, then the fixture's own V on the same object"""
    def body(factory, rank):
        gp = factory(p.x, p.y[:, :1], np.array(p.V), p.kernel)
        out = {"raised": []}
        for i0 in i0s:
            V = np.array(p.V)
            V[i0] = -(p.theta[0] + 1.0)
            gp.set_targets(p.y[:, :1], V)
            try:
                gp.evaluate(p.theta, want_alpha=True)
                out["raised"].append("nothing")
            except np.linalg.LinAlgError as e:
                out["raised"].append(str(e))
        gp.set_targets(p.y[:, :1], p.V)
        out["scalars"] = np.array(gp.evaluate(p.theta, want_alpha=True))
        out["alpha"] = host(gp.alpha)[:p.n, :1]
        out["L"] = gp.factor_matrix()
        return out
    return body


def chol_ld_order(p, i0):
    """the order chol_ld names for the fixture with V[i0] = -(sigma^2 + 1)"""
    A = np.array(p.A)
    A[i0, i0] = np.asarray(kf.k_ref(p.kernel, p.x[i0:i0 + 1], p.x[i0:i0 + 1], p.theta), dtype=np.float64)[0, 0] - (p.theta[0] + 1.0)
    try:
        chol_ref.chol_ld(A)
    except np.linalg.LinAlgError as e:
        return int(str(e).split("order ")[1].split()[0])
    return 0


# ---- every kernel id ----------------------------------------------------------------------------------------------------------------
class KernelProblem:
    """kernel_family_ref.case(name, d, 300) with V = 1e-2 and a smooth y: what full_body reads of a problem"""

    def __init__(self, name, d, n=300):
        self.kernel, self.d, self.n = name, d, n
        self.x, _, self.theta = kf.case(name, d, n)
        self.V = np.full(n, 1e-2)
        self.y = pr.smooth_y(self.x, 1) + 0.1 * np.random.default_rng(n + d).standard_normal((n, 1))


def schedule_twin(A64, y):
    """(L, z) in float64 as the sharded schedule forms them: L = chol_ref.twin_chol(A64, 16) -- right-looking, 128 columns at a time,
    the panel solve by substitution over 16-column tiles --, and z^T as the appended block row that rides through the same panel
    solves and trailing updates: per 128 columns z_p^T = r_p inv(L_pp)^T by chol_ref._solve_tiles, then r -= z_p^T L[below, p]^T.
    scipy's substitution is another float64 algorithm; this one is the device's, so the bar of the scalars counts what its own
    order of sums attains (tests/test_sharded_host.py proves it a valid solve)."""
    L = chol_ref.twin_chol(A64, 16)
    n = len(L)
    r = np.array(np.asarray(y, dtype=np.float64).reshape(n, -1).T)
    z = np.zeros_like(r)
    for p0 in range(0, n, TILE):
        p1 = min(n, p0 + TILE)
        z[:, p0:p1] = chol_ref._solve_tiles(r[:, p0:p1], L[p0:p1, p0:p1], 16)
        if p1 < n:
            r[:, p1:] -= z[:, p0:p1] @ L[p1:, p0:p1].T
    return L, z.T.copy()


def kernel_matrices(p):
    """(A = fl64(K) + diag(V) of the exact kernel, A64 = the float64 assembly) of a KernelProblem"""
    i = np.arange(p.n)
    A = np.asarray(kf.k_ref(p.kernel, p.x, p.x, p.theta), dtype=np.float64)
    A[i, i] += p.V
    A64 = kf.k_ref(p.kernel, p.x, p.x, p.theta, dtype=np.float64)
    A64[i, i] += p.V
    return A, A64


def judge_kernel(entry, geom, p, out):
    """the three scalars against batch_ref.loglik_ld; the bar from scipy's float64 value of the same problem and from the float64
    twin of the sharded schedule (schedule_twin)"""
    import scipy.linalg as sla
    n = p.n
    A = np.asarray(kf.k_ref(p.kernel, p.x, p.x, p.theta), dtype=np.float64)
    A[np.arange(n), np.arange(n)] += p.V
    Lhat = chol_ref.chol_ld(A)
    z = br.fwd_cols(Lhat, p.y)
    logdet, quad = chol_ref.logdet_ld(Lhat), np.sum(z * z)
    ref = np.array([-LD(0.5) * (quad + logdet + LD(n) * br._log2pi()), logdet, quad], dtype=LD)
    assert abs(ref[0] - br.loglik_ld(p.kernel, p.x, p.theta, p.V, p.y)) <= 4 * br.EPS_LD * abs(ref[0])
    A64 = kf.k_ref(p.kernel, p.x, p.x, p.theta, dtype=np.float64)
    A64[np.arange(n), np.arange(n)] += p.V
    L = sla.cholesky(A64, lower=True)
    zs = sla.solve_triangular(L, p.y, lower=True)
    ld, q = 2.0 * np.sum(np.log(np.diagonal(L))), np.sum(zs * zs)
    den = np.array([0.5 * (abs(ref[2]) + abs(ref[1]) + n * np.log(2 * np.pi)), abs(ref[1]), abs(ref[2])], dtype=LD)
    Ls, zt = schedule_twin(A64, p.y)
    lds, qs = 2.0 * np.sum(np.log(np.diagonal(Ls))), np.sum(zt * zt)
    tw = [np.abs(np.array([-0.5 * (b + a + n * np.log(2 * np.pi)), a, b], dtype=LD) - ref) / den for a, b in ((ld, q), (lds, qs))]
    dev = np.abs(np.asarray(out, dtype=LD) - ref) / den
    for i, name in enumerate(("value", "logdet", "quad")):
        d = float(dev[i]) if np.isfinite(out[i]) else float("inf")
        say(entry, geom, p.kernel, name, d, float(max(t[i] for t in tw)), br.bar([float(t[i]) for t in tw], br.FLOOR_EPS * EPS))
