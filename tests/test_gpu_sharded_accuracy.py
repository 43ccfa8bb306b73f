"""The row-sharded evaluation -- fvgp_hip_loglik_dist, _solve_dist, _posterior_dist, _grad_dist (csrc/dist.hip over csrc/dist_driver.h)
sequenced by fvgp_amd.dist.ShardedGP -- against the extended-precision reference of tests/batch_ref.py, at the smallest geometries that
reach each branch of the driver (tests/sharded_ref.py: the table, the twins, the bars; tests/test_sharded_host.py proves them on the CPU
twin of the ABI, every multi-rank geometry included).

On the device only the one-rank geometries run here: in place (the panels factored in A itself) and forced (force_collectives: the panel
buffers, Dfac, the staged and the in-place gather, the library's own copy path).  The multi-rank rows of the table ran as threads with
one handle each (tests/dist_ranks.py) and the four-rank cases ended in an abandoned panel kernel and a memory fault whose cause is not
found, so no multi-rank case runs on a device from this file; the spawned-process tests of tests/test_gpu_dist.py remain the device's
multi-rank coverage.

Fixtures (batch_ref.FAMILY): E on every geometry, the ill-conditioned G and H on the forced one, U- and U+ (G scaled by 2^-400 and 2^400)
and ncol = 8 on (1 forced, 256, 300), M (matern32_iso, d = 3) in place; the gradient on E, H and M at every geometry with n >= 300.  With a
named kernel one rank assembles through kmat_lower only: kmat_rows + dist_diag_kernel have no extended-precision check on the device.

Every figure prints as `SD|entry|world|panel|fixture|n|measure|device|twin|ratio` (pytest -s) before anything is asserted."""
import numpy as np
import pytest

import batch_ref as br
import kernel_family_ref as kf
import sharded_ref as sr

pytestmark = pytest.mark.gpu

FORCED, INPLACE = sr.FORCED, sr.INPLACE


def _one_rank(cases):
    return [c for c in cases if (c[0][0] if isinstance(c[0], tuple) else c[0]) == 1]


BIG = _one_rank([g for g in sr.GEOMETRY if g[3] >= 300])
# the issue's U-, U+ and ncol = 8 cases sit on multi-rank geometries (tests/test_sharded_host.py runs them there on the CPU twin): here
# they go through the panel buffers of one rank
FACTOR_CASES = _one_rank(sr.FACTOR_CASES) + [((1, FORCED, 256, 300), f, 1) for f in ("U-", "U+")] + [((1, FORCED, 256, 300), "E", 8)]
GRAD_CASES = [(g, f) for g in BIG for f in ("E", "H", "M")]
POST_CASES = [((1, INPLACE, 256, 300), "E"), ((1, FORCED, 128, 300), "E"), ((1, FORCED, 128, 300), "H")]
STALE = [(1, FORCED, 128, 300), (1, FORCED, 256, 513)]


def _ops(rank):
    from fvgp_amd import _lib
    from fvgp_amd.dist import HipOps
    return HipOps(_lib.Handle(0))


def _close(ops):
    ops.close()
    ops.H.close()


def _run(geom, body):
    return sr.run(geom, _ops, body, _close)


# ---- 1. factor, value, backward solve -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,fam,ncol", FACTOR_CASES, ids=[sr.case_id(*c) for c in FACTOR_CASES])
def test_factor_value_and_backward_solve(geom, fam, ncol):
    """the gathered factor (beta, phi, lam), the three scalars, alpha and diag(KV^-1); log_likelihood (keep_factor = 0) returns
    evaluate's scalars in their bits -- the two differ only in what chain() copies back into A, and the appended rows the scalars are
    read from are copied back by both --, after which the solve, posterior and gradient are refused"""
    r = br.reference(fam, geom[3])
    res = _run(geom, sr.full_body(r.p, ncol, refusal=True))
    sr.judge_full("factor", geom, fam, ncol, res, r)
    sr.done()


# ---- 2. gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,fam", GRAD_CASES, ids=[sr.case_id(*c) for c in GRAD_CASES])
def test_gradient_over_slabs(geom, fam):
    """slab 128 and 256 (several slabs, the last ragged), np (one slab) and 2048 (wider than the matrix); components 0 and 1 of
    ncol = 2 (the b term is added on rank 0 only); all slabs within the bar of each other, the same slab twice equal in its bits"""
    n = geom[3]
    r = br.reference(fam, n)
    npad = -(-n // 128) * 128
    res = _run(geom, sr.full_body(r.p, 2, slabs=tuple(sorted({128, 256, npad, 2048})), components=(0, 1), want_factor=False))
    sr.judge_full("grad", geom, fam, 2, res, r)
    sr.done()


# ---- 3. posterior ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npred", [1, 128, 129])
@pytest.mark.parametrize("geom,fam", POST_CASES, ids=[sr.case_id(*c) for c in POST_CASES])
def test_posterior(geom, fam, npred):
    """mean, variance (the diagonal of S) and S per point class; want_cov=False returns the same mean in its bits and None"""
    r = br.reference(fam, geom[3])
    pc = sr.posterior_case(r, npred)
    res = _run(geom, sr.full_body(r.p, 1, xpred=pc[0], want_factor=False, want_diag=False))
    sr.judge_full("posterior", geom, fam, 1, res, r, pc)
    sr.done()


# ---- 4. pre-assembled rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["callable", "noise matrix"])
@pytest.mark.parametrize("geom", [(1, FORCED, 128, 300), (1, INPLACE, 256, 300)], ids=sr.case_id)
def test_preassembled_rows(geom, how):
    """a host kernel callable (the k_pre / kk_pre branch of the posterior; gradient() raises NotImplementedError) and the noise as an
    (n, n) diagonal matrix through set_targets: value, alpha and posterior within the bars of fixture E"""
    r = br.reference("E", 300)
    p = r.p
    pc = sr.posterior_case(r, 129)
    kw = {}
    if how == "callable":
        kw["kernel"] = lambda a, b, h: np.asarray(kf.k_ref(p.kernel, a, b, h, dtype=np.float64))
    else:
        kw["V"] = np.diag(p.V)
    res = _run(geom, sr.full_body(p, 1, xpred=pc[0], want_diag=False, **kw))
    if how == "callable":
        assert all(o.pop("grad_refused") for o in res)
    sr.judge_full(f"preassembled/{how}", geom, "E", 1, res, r, pc)
    sr.done()


# ---- 5. every kernel id through the sharded assembly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(1, INPLACE, 128, 300), (1, FORCED, 256, 300)], ids=sr.case_id)
@pytest.mark.parametrize("name,d", sr.OTHER_KERNELS)
def test_every_kernel_id(name, d, geom):
    """the four names no fixture uses through kmat_lower, in place and through the panel buffers (kmat_rows + dist_diag_kernel assemble
    only where there is more than one rank: on the CPU twin in tests/test_sharded_host.py).  The bar is 8 times the worse of two float64
    values of the same problem: scipy's, and sharded_ref.schedule_twin's -- the float64 copy of the sharded schedule (twin_chol at 16,
    z as the appended row through the panel solves), which tests/test_sharded_host.py proves a valid solve.  With scipy alone the
    in-place matern52_ard case is a schedule's rounding above the bar (quad 1.758e-14 on an MI355X against 8 x 2.127e-15; the
    schedule twin itself gives 1.891e-14 on the host, cond_2 = 2.3e4)."""
    p = sr.KernelProblem(name, d)
    res = _run(geom, sr.full_body(p, 1, want_factor=False, want_diag=False))
    sr.ranks_agree("kernels", geom, name, res)
    sr.judge_kernel("kernels", geom, p, res[0]["scalars"])
    sr.done()


# ---- 6. nothing stale is read ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", STALE, ids=sr.case_id)
def test_nothing_stale_is_read(geom):
    """NaN in T, recv, gather, Dfac and right of every block's diagonal tile in A before the first evaluation: finite results, in their
    bits those of an untouched object; theta, 1.3 theta, theta on one object: the third result is the first in its bits"""
    r = br.reference("E", geom[3])
    clean = _run(geom, sr.full_body(r.p, 1, want_diag=False))
    dirty = _run(geom, sr.full_body(r.p, 1, want_diag=False, poisoned=True, repeat=True))
    sr.judge_full("stale", geom, "E", 1, dirty, r)
    for k in ("scalars", "alpha", "L"):
        sr.check(bool(np.all(np.isfinite(dirty[0][k]))), f"stale {sr.case_id(geom)}: a NaN arrived in {k}")
        sr.check(dirty[0][k].tobytes() == clean[0][k].tobytes(), f"stale {sr.case_id(geom)}: {k} differs from the untouched object's bits")
    sr.done()


# ---- 7. not positive definite ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(1, FORCED, 128, 300)], ids=sr.case_id)
def test_not_positive_definite(geom):
    """V[i0] = -(sigma^2 + 1) in the first panel, in the first row of a later panel and at n - 1: the rank
    raises LinAlgError naming the order i0 + 1 (what chol_ld raises: tests/test_sharded_host.py); a valid evaluation on the same objects
    then meets its bars"""
    r = br.reference("E", geom[3])
    i0s = sr.npd_rows(geom)
    res = _run(geom, sr.npd_body(r.p, i0s))
    for rank, out in enumerate(res):
        got = [s.split("-th")[0] for s in out["raised"]]
        print(f"SD|npd|{geom[0]}|{geom[2]}|E|{geom[3]}|orders named by rank {rank}|{got}|{[i + 1 for i in i0s]}|-")
        sr.check(got == [str(i0 + 1) for i0 in i0s], f"npd {sr.case_id(geom)}: rank {rank} raised {out['raised']}")
    sr.judge_full("npd/after", geom, "E", 1, res, r)
    sr.done()
