"""The thread harness of the row-sharded tests (tests/dist_ranks.py), the geometry table and the bars of tests/sharded_ref.py, proved on
the host: every geometry runs on the CPU twin of the ABI (tests/dist_stub_ops.StubOps -- the same fvgp_amd/csrc/dist_driver.h over host
loops) and is held to the measures and bars the device is held to in tests/test_gpu_sharded_accuracy.py.  No GPU."""
import time
import types

import numpy as np
import pytest

import batch_ref as br
import sharded_ref as sr
from conftest import synth
from oracle import fvgp_oracle as orc


def _stub(rank):
    from dist_stub_ops import StubOps
    return StubOps()


@pytest.mark.parametrize("geom", sr.GEOMETRY, ids=[sr.case_id(g) for g in sr.GEOMETRY])
def test_every_geometry_on_the_cpu_twin(geom):
    """fixture E through evaluate, the gathered factor, alpha, diag(KV^-1), one ragged-slab gradient and a posterior; log_likelihood
    bitwise and the refusals after it; every rank's replicated outputs equal in their bits"""
    world, mode, panel, n = geom
    r = br.reference("E", n)
    pc = sr.posterior_case(r, 5)
    res = sr.run(geom, _stub, sr.full_body(r.p, 1, slabs=(256,) if n >= 300 else (), xpred=pc[0], refusal=True))
    sr.judge_full("host", geom, "E", 1, res, r, pc)
    sr.done()


OTHER_FACTOR_CASES = [c for c in sr.FACTOR_CASES if (c[1], c[2]) != ("E", 1)]


@pytest.mark.parametrize("geom,fam,ncol", OTHER_FACTOR_CASES, ids=[sr.case_id(*c) for c in OTHER_FACTOR_CASES])
def test_hard_fixtures_through_the_multi_rank_composition(geom, fam, ncol):
    """what the device runs on one rank only: the ill-conditioned G and H, U- and U+ (G scaled by 2^-400 and 2^400: nothing may over- or
    underflow in the row sums of squares or the log-determinants, every measure under G's bars), M, and ncol = 8 (alpha judged at
    columns 0 and 7) through the gathers, updates and sweeps of two and three ranks"""
    r = br.reference(fam, geom[3])
    res = sr.run(geom, _stub, sr.full_body(r.p, ncol, refusal=True))
    assert all(np.all(np.isfinite(o[k])) for o in res for k in ("scalars", "alpha", "L", "diag"))
    sr.judge_full("host/factor", geom, fam, ncol, res, r)
    sr.done()


def test_stale_buffers_and_repeat_on_the_cpu_twin():
    """(3, 128, 700), the `la > L0` geometry: NaN in every panel buffer and right of the diagonal tiles changes no bit; theta after
    1.3 theta gives the first result's bits"""
    geom = (3, None, 128, 700)
    r = br.reference("E", 700)
    clean = sr.run(geom, _stub, sr.full_body(r.p, 1, want_diag=False))
    dirty = sr.run(geom, _stub, sr.full_body(r.p, 1, want_diag=False, poisoned=True, repeat=True))
    sr.judge_full("host/poisoned", geom, "E", 1, dirty, r)
    for k in ("scalars", "alpha", "L"):
        assert np.all(np.isfinite(dirty[0][k])) and dirty[0][k].tobytes() == clean[0][k].tobytes(), k
    sr.done()


def test_agrees_with_the_process_group_case():
    """world 3, n = 900, panel 128, matern52_ard: a shape of tests/test_dist_cpu.py (ranks as gloo processes there, threads here) against
    the dense oracle within that test's tolerances"""
    n, d, theta = 900, 3, np.array([1.1, 0.3, 0.35, 0.4])
    x, y = synth(n, d)
    p = types.SimpleNamespace(x=x, y=(y - np.mean(y))[:, None], V=np.full(n, 0.01), theta=theta, kernel="matern52_ard", n=n)
    xp = np.random.default_rng(7).random((130, d))
    res = sr.run((3, None, 128, n), _stub, sr.full_body(p, 1, slabs=(256,), xpred=xp, want_factor=False))
    sr.ranks_agree("host/gloo shape", (3, None, 128, n), "matern52_ard", res)
    sr.done()
    out = res[0]
    gp = orc.OracleGP(x, y, theta, np.full(n, 0.01), kernel="matern52_ard")
    np.testing.assert_allclose(out["scalars"][0], gp.log_likelihood(), rtol=1e-10)
    np.testing.assert_allclose(out["scalars"][1], gp.logdet_KV, rtol=1e-10)
    assert np.max(np.abs(out["alpha"] - gp.KVinvY.reshape(n, -1))) <= 1e-8 * np.max(np.abs(gp.KVinvY))
    m, S, _ = out["post"]
    np.testing.assert_allclose(m, gp.posterior_mean(xp)["m(x)_flat"].reshape(len(xp), -1) - np.mean(y), rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(S - gp.posterior_covariance(xp)["S"])) <= 1e-10 * theta[0]
    g_ref = gp.neg_log_likelihood_gradient(theta, component=0)
    np.testing.assert_allclose(out[("grad", 0, 256)][0], g_ref, rtol=1e-8, atol=1e-9 * np.max(np.abs(g_ref)))


def test_a_failing_rank_ends_the_case_for_all():
    """rank 1 raises before its first collective: the peers' waits break, run_ranks raises naming rank 1's exception, well inside the
    barrier's time limit"""
    import dist_ranks
    p = br.problem("E", 300)

    def body(factory, rank):
        if rank == 1:
            raise ValueError("rank 1 gives up")
        gp = factory(p.x, p.y[:, :1], p.V, p.kernel)
        return gp.evaluate(p.theta)

    t0 = time.monotonic()
    with pytest.raises(dist_ranks.RanksFailed) as e:
        sr.run((3, None, 128, 300), _stub, body)
    assert time.monotonic() - t0 < 30.0
    assert isinstance(e.value.__cause__, ValueError) and isinstance(e.value.errors[1], ValueError)
    assert set(e.value.errors) == {0, 1, 2}


@pytest.mark.parametrize("geom", [(3, None, 128, 700), (1, sr.FORCED, 128, 300)], ids=sr.case_id)
def test_not_positive_definite_names_the_order_chol_ld_names(geom):
    """V[i0] = -(sigma^2 + 1): chol_ld raises at order i0 + 1, and so does every rank of the CPU twin; the same objects then meet the
    bars of the clean fixture"""
    r = br.reference("E", geom[3])
    i0s = sr.npd_rows(geom)
    assert i0s[0] < geom[2] <= i0s[1] < i0s[2] and (geom[0] == 1 or (i0s[1] // 128) % geom[0] != 0)
    for i0 in i0s:
        assert sr.chol_ld_order(r.p, i0) == i0 + 1
    res = sr.run(geom, _stub, sr.npd_body(r.p, i0s))
    for rank, out in enumerate(res):
        assert [s.split("-th")[0] for s in out["raised"]] == [str(i0 + 1) for i0 in i0s], (rank, out["raised"])
    sr.judge_full("host/after npd", geom, "E", 1, res, r)
    sr.done()


@pytest.mark.parametrize("name,d", sr.OTHER_KERNELS)
def test_every_kernel_id_through_the_rank_assembly(name, d):
    """the four names no fixture uses at (3, 128, 300): the driver's per-block kmat_rows and diag calls on three ranks"""
    geom = (3, None, 128, 300)
    p = sr.KernelProblem(name, d)
    res = sr.run(geom, _stub, sr.full_body(p, 1, want_factor=False, want_diag=False))
    sr.ranks_agree("host/kernels", geom, name, res)
    sr.judge_kernel("host/kernels", geom, p, res[0]["scalars"])
    sr.done()


@pytest.mark.parametrize("name,d", sr.OTHER_KERNELS)
def test_schedule_twin_is_a_valid_float64_solve(name, d):
    """sharded_ref.schedule_twin, the float64 copy of the sharded schedule that the bars of the kernel-id cases count beside scipy:
    its factor is chol_ref.twin_chol(A64, 16) in its bits, its z solves L z = y to 4 n eps componentwise (the backward error of a
    substitution, with the tile inverses' share), and against the longdouble z it stays under 64 eps cond_2 like scipy's.  What it
    attains in the three scalars is printed beside scipy's figure."""
    import scipy.linalg as sla
    import chol_ref
    p = sr.KernelProblem(name, d)
    A, A64 = sr.kernel_matrices(p)
    L, z = sr.schedule_twin(A64, p.y)
    assert L.tobytes() == chol_ref.twin_chol(A64, 16).tobytes()
    LD = br.LD
    Ll, zl = np.asarray(L, dtype=LD), np.asarray(z, dtype=LD)
    back = np.max(np.abs(Ll @ zl - p.y) / (np.abs(Ll) @ np.abs(zl) + np.abs(p.y))) / br.EPS
    zhat = br.fwd_cols(chol_ref.chol_ld(A), p.y)
    cond = chol_ref.cond2(A)
    zs = sla.solve_triangular(sla.cholesky(A64, lower=True), p.y, lower=True)
    err, err_s = br.col_err(z, zhat), br.col_err(zs, zhat)
    q = float(np.sum(zhat * zhat))
    print(f"SD|host/schedule twin|-|128|{name}|{p.n}|backward error of z in eps|{float(back):.3e}|-|{float(back) / (4 * p.n):.3f}")
    print(f"SD|host/schedule twin|-|128|{name}|{p.n}|z|{err:.3e}|{err_s:.3e}|{err / (64 * br.EPS * cond):.3f}")
    print(f"SD|host/schedule twin|-|128|{name}|{p.n}|quad|{abs(float(np.sum(zl * zl)) - q) / q:.3e}|{abs(float(np.sum(zs * zs)) - q) / q:.3e}|-")
    assert back <= 4 * p.n and err <= 64 * br.EPS * cond and err_s <= 64 * br.EPS * cond
