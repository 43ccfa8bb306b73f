"""The numpy twin of the matrix-free solves (tests/matrix_free_ref.py) against numpy.linalg, and the margins of the fixtures the device
tests lean on: pivots that lead their runner-up, a preconditioner that earns its place, condition numbers at which tol = 1e-9 is
attainable.  No GPU."""
import numpy as np
import pytest

import matrix_free_ref as mf

TOL = 1e-9


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def test_abi_symbols_and_size_queries(L):
    from fvgp_amd import _lib
    for s in ("fvgp_hip_kmatvec", "fvgp_hip_kmatvec_workspace_bytes", "fvgp_hip_pchol", "fvgp_hip_pchol_workspace_bytes",
              "fvgp_hip_precond_factor", "fvgp_hip_precond_workspace_bytes", "fvgp_hip_pcg", "fvgp_hip_pcg_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert _lib.MATVEC_CHUNK == mf.CHUNK
    # per-chunk sums of the split form: chunks x rows x group width (17 columns go as 16 + 1, 3 columns in a group of 4)
    assert _lib.kmatvec_workspace_bytes(300, 2 * mf.CHUNK + 37, 17) == 3 * 300 * 16 * 8
    assert _lib.kmatvec_workspace_bytes(300, mf.CHUNK, 3) == 1 * 300 * 4 * 8
    assert _lib.kmatvec_workspace_bytes(0, 5, 1) == -1 and _lib.pchol_workspace_bytes(10, 0) == -1
    assert _lib.precond_workspace_bytes(20000, 128) == 3 * 128 * 128 * 8
    assert _lib.pcg_workspace_bytes(0, 0) == -1 and _lib.pcg_workspace_bytes(1000, 128) > 4 * 1000 * 16 * 8
    # O(n): a million points at rank 256 stay below 1 GB of solver workspace
    assert _lib.pcg_workspace_bytes(10 ** 6, 256) < 1 << 30


@pytest.mark.parametrize("fx", mf.PIVOT_FIXTURES, ids=mf.fixture_id)
def test_pchol_twin_reproduces_the_residual_diagonal(fx):
    f = mf.fixture(fx)
    G, piv, d, rank, _ = mf.fixture_pchol(fx)
    n = len(f["x"])
    assert rank == mf.RANK and len(set(piv.tolist())) == mf.RANK
    R = f["K"] - G.T @ G
    assert np.max(np.abs(np.diag(R) - d)) <= 1e-12 * mf.SIGMA2, np.max(np.abs(np.diag(R) - d))
    assert np.linalg.eigvalsh(R).min() >= -1e-12 * mf.SIGMA2 * n
    for t in range(1, 64):                                   # a pivot's column is eliminated by its own step
        assert np.max(np.abs(G[t, piv[:t]])) <= 1e-12 * np.sqrt(mf.SIGMA2)


@pytest.mark.parametrize("fx", mf.PIVOT_FIXTURES, ids=mf.fixture_id)
def test_pivot_margins(fx):
    """what the device comparison needs: at each of the first 24 steps after step 0 the pick leads the runner-up by >= 1e-9 sigma^2"""
    margins = mf.fixture_pchol(fx)[4]
    print(fx, "smallest margin over steps 1..24:", margins[1:25].min())
    assert margins[1:25].min() >= 1e-9 * mf.SIGMA2, margins[1:25]


@pytest.mark.parametrize("fx", mf.FIXTURES[:4], ids=mf.fixture_id)
def test_woodbury_apply_equals_a_dense_solve(fx):
    f = mf.fixture(fx)
    G = mf.fixture_pchol(fx)[0]
    M = G.T @ G + np.diag(f["V"])
    R = f["rhs"][:, :3]
    want = np.linalg.solve(M, R)
    got = mf.woodbury_apply(G, f["V"], R)
    # M is conditioned like sigma^2 n / min V at the worst: a relative 1e-8 covers both routes' rounding
    assert np.linalg.norm(got - want) <= 1e-8 * np.linalg.norm(want)
    assert np.array_equal(mf.woodbury_apply(None, f["V"], R), R / f["V"][:, None])


@pytest.mark.parametrize("fx", mf.ACCURACY_FIXTURES, ids=mf.fixture_id)
def test_pcg_twin_reaches_the_dense_solution_and_the_fixture_is_well_conditioned(fx):
    """cond(A) <= 1e6, so that tol = 1e-9 is attainable in double; and no column's final residual below 5e-12, ten times the rounding floor
    of a residual evaluated in double on these fixtures (about sqrt(n) eps |x| / |b| = 5e-13 with |x| / |b| near 1 / min V): a solve that
    overshoots tol by more lands where the device's reported value cannot be confirmed to 10 %"""
    f = mf.fixture(fx)
    assert min(mf.fixture_pcg(fx, c, mf.RANK, TOL)[2] for c in range(16)) >= 5e-12
    ev = np.linalg.eigvalsh(f["A"])
    cond = ev[-1] / ev[0]
    print(fx, "cond", cond)
    assert cond <= 1e6
    x, iters, relres, status = mf.fixture_pcg(fx, 0, mf.RANK, TOL)
    want = np.linalg.solve(f["A"], f["rhs"][:, 0])
    assert status == 0 and relres <= TOL
    assert np.linalg.norm(x - want) <= cond * TOL * np.linalg.norm(want)
    xj, itj, rrj, stj = mf.fixture_pcg(fx, 0, 0, TOL)              # Jacobi
    assert stj == 0 and np.linalg.norm(xj - want) <= cond * TOL * np.linalg.norm(want)
    print(fx, "iterations rank 128:", iters, "Jacobi:", itj)


@pytest.mark.parametrize("fx", mf.PRECOND_FIXTURES, ids=mf.fixture_id)
def test_the_preconditioner_earns_its_place(fx):
    it128 = mf.fixture_pcg(fx, 0, mf.RANK, TOL)[1]
    it0 = mf.fixture_pcg(fx, 0, 0, TOL, precond=False)[1]
    print(fx, "rank 128:", it128, "no preconditioner:", it0)
    assert it0 >= 4 * it128


def test_pcg_twin_rules():
    fx = mf.FIXTURES[2]
    f = mf.fixture(fx)
    G = mf.fixture_pchol(fx)[0]
    b = f["rhs"][:, 1]
    assert mf.pcg_ref(f["A"], np.zeros(len(b)), f["V"], G, TOL)[1:] == (0, 0.0, 0)
    x, it, rr, st = mf.pcg_ref(f["A"], b, f["V"], G, TOL, max_iter=2)
    assert st == 1 and it == 2 and rr > TOL
    x, it, rr, st = mf.fixture_pcg(fx, 1, mf.RANK, TOL)
    assert mf.pcg_ref(f["A"], b, f["V"], G, TOL, x0=x)[1] == 0       # a warm start from the solution iterates no further
    Aneg = f["A"] - 2.0 * np.eye(len(b)) * np.linalg.eigvalsh(f["A"])[-1]
    assert mf.pcg_ref(Aneg, b, f["V"], None, TOL)[3] == 2           # not positive definite: breakdown


def test_kmatvec_bound_holds_for_a_double_product():
    """the bound of the device test judged on the host: the same product in plain double in numpy's own order stays inside it"""
    x1, x2, B, v = mf.matvec_case(65, 300, 3, 5, 7)
    theta = mf.theta_of("matern52_ard", 3, 0.3)
    Y, mag = mf.kmatvec_ref("matern52_ard", x1, x2, theta, B)
    got = np.asarray(mf.kf.k_ref("matern52_ard", x1, x2, theta), dtype=np.float64) @ B
    assert np.all(np.abs(got - Y) <= mf.kmatvec_bound(300, B, mag))
