"""Host side of the rank-k factor update and the removal of data points (fvgp_amd/csrc/chol_update.hip): the ABI surface, the workspace
query, and the numpy twin of the device sweep (tests/chol_update_ref.py) against numpy.linalg.cholesky of the kept matrix.

Then the proof of the extended-precision reference that tests/test_gpu_chol_update_accuracy.py judges the device with, on the cases of
that file (the lists live in chol_update_ref): the Householder route agrees with a plain sweep of rotations in longdouble to U / 16
(U = 2^-53); nothing simpler could serve (a fresh factorisation and the formed-matrix route are beyond 1e4 U on H where the twin is
within its cap); the twin stays under the caps on every case, so a bad twin can never widen a device bar; seeded defects in a copy of
the twin ARE flagged by the device bar; what the measures cannot see by design; and the bit property of the scaled families."""
import ctypes

import numpy as np
import pytest

import chol_ref
import chol_update_ref as cr
from conftest import load_golden
from oracle import fvgp_oracle as orc

FIXTURES = {"G2": ("G2_rbf_n512_d3.npz", orc.rbf_ard), "G3": ("G3_matern52_n512_d3.npz", orc.matern52_ard)}
_CACHE = {}


def _factor(tag):
    """(KV, L) of a golden problem, computed once"""
    if tag not in _CACHE:
        name, kern = FIXTURES[tag]
        fx = load_golden(name)
        KV = orc.addKV(kern(fx["x"], fx["x"], fx["theta"]), fx["noise_variances"])
        _CACHE[tag] = (KV, np.linalg.cholesky(KV))
    return _CACHE[tag]


def removal_sets(n):
    rng = np.random.default_rng(23)
    return {"first": [0], "last": [n - 1], "straddle128": [127, 128, 129], "first16": list(range(16)),
            "random17": sorted(rng.choice(n, 17, replace=False).tolist()), "random70": sorted(rng.choice(n, 70, replace=False).tolist()),
            "every_second": list(range(0, n, 2))}


def test_library_exports_the_update_entries():
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    for s in ("fvgp_hip_chol_update", "fvgp_hip_chol_delete", "fvgp_hip_chol_update_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert len(L.fvgp_hip_chol_update.argtypes) == 10 and L.fvgp_hip_chol_update.restype is ctypes.c_int
    assert len(L.fvgp_hip_chol_delete.argtypes) == 8 and L.fvgp_hip_chol_delete.restype is ctypes.c_int
    assert L.fvgp_hip_chol_update_workspace_bytes.restype is ctypes.c_int64
    assert _lib.CHOL_UPDATE_MAX_RANK == 16 and _lib.CHOL_UPDATE_TABLE_BYTES == 128 * 16 * 2 * 8
    # a missing handle is argument 1, before anything else is looked at
    assert L.fvgp_hip_chol_update(None, None, 0, 0, None, 0, 0, 0, None, 0) == -1
    assert L.fvgp_hip_chol_delete(None, None, 0, 0, None, 0, None, 0) == -1


def test_workspace_query():
    from fvgp_amd import _lib
    ws = _lib.chol_update_workspace_bytes
    for n, k in ((0, 1), (-3, 1), (10, 0), (10, -1)):
        assert ws(n, k) == -1
    assert ws(1, 1) >= _lib.CHOL_UPDATE_TABLE_BYTES
    # the pieces: the coefficient table, k + n index words, W (n x k) and a strip of at most 1024 rows -- never n x n
    for n in (1, 300, 4096, 20000, 50000, 10 ** 6):
        for k in (1, 16, 64):
            b = ws(n, k)
            assert b % 16 == 0
            assert _lib.CHOL_UPDATE_TABLE_BYTES < b <= 8 * (n + 1) * (k + 1 + 1024 + 2) + _lib.CHOL_UPDATE_TABLE_BYTES + 64
    # linear in n: doubling n at most doubles what is beyond the table (the strip stops growing at 2^25 doubles)
    for n in (2048, 8192, 20000, 50000, 250000):
        a, b = ws(n, 16) - _lib.CHOL_UPDATE_TABLE_BYTES, ws(2 * n, 16) - _lib.CHOL_UPDATE_TABLE_BYTES
        assert a < b <= 2 * a + 64
    assert ws(10 ** 6, 16) < 1 << 30


@pytest.mark.parametrize("tag", ["G2", "G3"])
def test_twin_matches_the_factor_of_the_kept_matrix(tag):
    KV, L = _factor(tag)
    n = len(L)
    scale = np.max(np.abs(L))
    for name, R in removal_sets(n).items():
        Rr, S = cr.split_indices(n, R)
        ref = np.linalg.cholesky(KV[np.ix_(S, S)])
        got = cr.chol_delete(L, R)
        err = np.max(np.abs(got - ref))
        print(f"chol_update twin|{tag}|{name}|k={len(Rr)}|{err / scale:.3g}")
        assert err <= 1e-12 * scale, name
        assert np.array_equal(got, np.tril(got)) and np.all(np.diag(got) > 0)


@pytest.mark.parametrize("tag", ["G2", "G3"])
def test_compaction_identity(tag):
    """KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T, L[S,S] lower triangular, W zero above the first removed index"""
    KV, L = _factor(tag)
    n = len(L)
    for name, R in removal_sets(n).items():
        Rr, S = cr.split_indices(n, R)
        Lss, W = cr.compaction(L, R)
        assert np.array_equal(Lss, np.tril(Lss)) and np.all(np.diag(Lss) > 0)
        assert Lss.shape == (len(S), len(S)) and W.shape == (len(S), len(Rr))
        assert not np.any(W[:Rr[0]])
        assert np.max(np.abs(Lss @ Lss.T + W @ W.T - KV[np.ix_(S, S)])) <= 1e-12, name


def test_twin_update_is_a_plain_rank_k_update():
    """the sweep on operands that come from no removal: every pass boundary, a row0, columns of W that start at different rows"""
    rng = np.random.default_rng(5)
    for n, k in ((1, 1), (1, 3), (7, 17), (40, 33), (129, 16)):
        A = rng.standard_normal((n, n))
        L = np.linalg.cholesky(A @ A.T + n * np.eye(n))
        W = rng.standard_normal((n, k))
        row0 = n // 3
        W[:row0] = 0.0
        for p in range(k):
            W[:min(n, row0 + 2 * p), p] = 0.0
        ref = np.linalg.cholesky(L @ L.T + W @ W.T)
        for r0 in (0, row0):
            assert np.max(np.abs(cr.chol_update(L, W, row0=r0) - ref)) <= 1e-12 * np.max(np.abs(ref))


# ---- the extended-precision reference and the bars of the device suite -------------------------------------------------------------------
U = cr.U


def _groups():
    """the cases of the device suite by the first word of their id (a test per group keeps each one short)"""
    out = {}
    for case in cr.update_cases() + cr.delete_cases():
        out.setdefault(("update " if len(case) == 6 else "delete ") + case[0].split("|")[0].split(" ")[0], []).append(case)
    return out


GROUPS = _groups()


def test_case_ids_name_every_route():
    """read from the ids alone: every instantiation of both kernels through both entries, the second strip, a skipped later pass, 1 / 63 /
    64 / 65 rows below the first block, 127 and 128 points after a removal"""
    up = [c[0] for c in cr.update_cases()]
    de = [c[0] for c in cr.delete_cases()]
    for ids in (up, de):
        for kp in (1, 2, 4, 8, 16):
            assert any(i.endswith(f"|KP{kp}") or f"|KP{kp} " in i or f"+{kp}" in i.split("|")[-1] for i in ids), kp
    assert len(set(up)) == len(up) and len(set(de)) == len(de)
    assert any("strips=2" in i for i in de) and any("+skip" in i for i in de)
    for below in (1, 63, 64, 65):
        assert any(f"below={below}|" in i for i in up)
    assert any("m=127|" in i for i in de) and any("m=128|" in i for i in de)
    assert cr.instantiation(17) == "KP16+1" and cr.instantiation(24) == "KP16+8" and cr.instantiation(48) == "KP16+16+16"
    assert cr.instantiation(3) == "KP4" and cr.instantiation(9) == "KP16"


def test_scaled_families_have_the_scaled_factor_of_g():
    for fam in ("S", "U-", "U+"):
        D = chol_ref.row_scale(fam, cr.N_MAIN)
        assert np.array_equal(cr.factor(fam, cr.N_MAIN), D[:, None] * cr.factor("G", cr.N_MAIN))
        for k in cr.SCALE_K:
            assert np.array_equal(cr.update_problem(fam, cr.N_MAIN, k).W, D[:, None] * cr.update_problem("G", cr.N_MAIN, k).W)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_reference_routes_agree_and_twin_is_under_its_caps(group):
    """per case: phi(update_ld, update_givens_ld) <= U / 16 (neither rounded); update_ld rounded to float64 has rho <= 2 U; the twin has
    phi <= 256 U and rho <= 64 U"""
    fails = []
    for case in GROUPS[group]:
        P = cr.case_problem(case)
        agree = cr.phi_ld(cr.update_givens_ld(P.L, P.W), P.Lhat)
        rounded = cr.rho(np.asarray(P.Lhat, dtype=np.float64), P.gram, P.nu, P.rows)
        tp, tr, tl = P.twin_figs
        print(f"CU host|{case[0]}|routes {agree / U:.3g}|rho rounded {rounded / U:.3g}|twin phi {tp / U:.3g} rho {tr / U:.3g} lam {tl:.3g}")
        for ok, what in ((agree <= U / 16, f"the two longdouble routes differ by {agree / U:.3g} U"), (rounded <= 2 * U, f"rho of the rounded reference {rounded / U:.3g} U"),
                         (tp <= cr.CAP_PHI, f"twin phi {tp / U:.3g} U above the cap"), (tr <= cr.CAP_RHO, f"twin rho {tr / U:.3g} U above the cap")):
            if not ok:
                fails.append(f"{case[0]}: {what}")
    assert not fails, "\n".join(fails)


def test_chain_and_split_routes_twin_is_under_its_caps():
    """the chained removal (H, n = 700, eight times four points) and the routes of the device suite's route test, each against delete_ld of
    the ORIGINAL factor for the union"""
    L = cr.factor("H", cr.N_CHAIN)
    sets, union = cr.chain_sets()
    assert len(union) == 32 and len(set(union)) == 32
    P = cr.delete_problem("H", cr.N_CHAIN, union)
    figs = P.figures(cr.twin_chain(L, sets))
    print(f"CU host|chain|twin phi {figs[0] / U:.3g} rho {figs[1] / U:.3g} lam {figs[2]:.3g}|at once phi {P.twin_figs[0] / U:.3g}")
    assert figs[0] <= cr.CAP_PHI and figs[1] <= cr.CAP_RHO
    for fam in ("G", "H"):
        R = cr.delete_sets(cr.N_MAIN)[cr.ROUTE_SET]
        P = cr.delete_problem(fam, cr.N_MAIN, R)
        for name, steps in cr.route_steps(R).items():
            figs = P.figures(cr.twin_chain(cr.factor(fam, cr.N_MAIN), steps))
            print(f"CU host|route {name}|{fam}|twin phi {figs[0] / U:.3g} rho {figs[1] / U:.3g}")
            assert figs[0] <= cr.CAP_PHI and figs[1] <= cr.CAP_RHO


def test_nothing_simpler_serves_as_the_reference():
    """H, n = 300: against the exact update, a fresh factorisation of the kept matrix and the Cholesky factor of the FORMED L L^T + W W^T
    (formed and factored in longdouble, rounded) are both beyond 1e4 U, while the twin is under its cap: forming the matrix costs cond,
    the orthogonal update sqrt(cond)"""
    n = cr.N_MAIN
    for name in ("first2", "straddle128", "scattered17"):
        R = cr.delete_sets(n)[name]
        P = cr.delete_problem("H", n, R)
        _, S = cr.split_indices(n, R)
        fresh = np.linalg.cholesky(chol_ref.matrix("H", n)[np.ix_(S, S)])
        Ll, Wl = np.asarray(P.L, dtype=cr.LD), np.asarray(P.W, dtype=cr.LD)
        formed = chol_ref.chol_ld(np.asarray(Ll @ Ll.T + Wl @ Wl.T, dtype=np.float64))
        e_fresh, e_formed = cr.phi(fresh, P.Lhat), cr.phi(np.asarray(formed, dtype=np.float64), P.Lhat)
        print(f"CU host|H|{name}|fresh {e_fresh / U:.3g}|formed {e_formed / U:.3g}|twin {P.twin_figs[0] / U:.3g}")
        assert e_fresh > 1e4 * U and e_formed > 1e4 * U and P.twin_figs[0] <= cr.CAP_PHI


def _defective(L, W, defect):
    """a copy of chol_update_ref.chol_update (row0 = 0) with one seeded defect: 'cs0' -- column 1 is rotated with column 0's (c, s);
    'late' -- the first pass starts one 128-block late; 'strip' -- the 64 rows 192 .. 255 are left out of the first block column's panel
    step"""
    L = np.tril(np.array(L, dtype=np.float64))
    W = np.array(W, dtype=np.float64)
    n, k = W.shape
    for p0 in range(0, k, cr.MAX_RANK):
        Wp = W[:, p0:p0 + cr.MAX_RANK]
        kp = Wp.shape[1]
        keep = (L[192:256, :128].copy(), Wp[192:256].copy()) if defect == "strip" and p0 == 0 else None
        for j in range(128 if defect == "late" and p0 == 0 else 0, n):
            if j == 128 and keep is not None:
                L[192:256, :128], Wp[192:256] = keep
            l = L[j, j]
            r = np.sqrt(l * l + np.cumsum(Wp[j] * Wp[j]))
            rprev = np.concatenate([[l], r[:-1]])
            c, s = rprev / r, Wp[j] / r
            if defect == "cs0" and kp > 1:
                c[1], s[1] = c[0], s[0]
            col = L[j + 1:, j].copy()
            for p in range(kp):
                sw = s[p] * Wp[j + 1:, p]
                Wp[j + 1:, p] = c[p] * Wp[j + 1:, p] - s[p] * col
                col = c[p] * col + sw
            L[j + 1:, j] = col
            L[j, j] = r[-1]
    return L


@pytest.mark.parametrize("fam", ["G", "H"])
def test_seeded_defects_are_flagged_by_the_device_bar(fam):
    """the copy without a defect IS the twin; each defect puts phi or rho above MARGIN max(twin, floor), the bar the device is held to"""
    for k in (2, 17):
        P = cr.update_problem(fam, cr.N_MAIN, k)
        assert np.array_equal(_defective(P.L, P.W, None), P.twin)
        bp, br, _ = P.bases()
        for defect in ("cs0", "late", "strip"):
            fp, fr, _ = P.figures(_defective(P.L, P.W, defect))
            print(f"CU host|defect {defect}|{fam}|k={k}|phi {fp / bp:.3g} x base|rho {fr / br:.3g} x base")
            assert fp > cr.MARGIN * bp and fr > cr.MARGIN * br, defect


def test_what_the_measures_cannot_see():
    """by design phi and rho are relative to a whole row: ONE entry of a small off-diagonal block (far-apart points, the smallest entry
    of the last row) off by 64 units of its last place moves neither by a tenth of the floor"""
    P = cr.update_problem("H", cr.N_MAIN, 2)
    n = P.n
    j = int(np.argmin(np.abs(P.twin[n - 1, :n - 1]) + (P.twin[n - 1, :n - 1] == 0)))
    bent = np.array(P.twin)
    bent[n - 1, j] *= 1 + 64 * 2 * U
    assert bent[n - 1, j] != P.twin[n - 1, j] and abs(P.twin[n - 1, j]) < 1e-6 * np.linalg.norm(P.twin[n - 1])
    fp, fr, _ = P.figures(bent)
    assert abs(fp - P.twin_figs[0]) <= 0.1 * cr.FLOOR_PHI and abs(fr - P.twin_figs[1]) <= 0.1 * cr.FLOOR_RHO


@pytest.mark.parametrize("fam", ["S", "U-", "U+"])
def test_twin_of_a_scaled_problem_is_the_scaled_twin(fam):
    """update(D L, D W) == D update(L, W) bit for bit for D a vector of powers of two: the sums have a fixed order and (c, s) are ratios
    of one row's entries, so only an absolute threshold or an under- / overflow could break it"""
    D = chol_ref.row_scale(fam, cr.N_MAIN)
    for k in cr.SCALE_K:
        assert np.array_equal(cr.update_problem(fam, cr.N_MAIN, k).twin, D[:, None] * cr.update_problem("G", cr.N_MAIN, k).twin)
        # ... and so is the exact result, which is why the scaled families keep the bars of G
        assert np.array_equal(cr.update_problem(fam, cr.N_MAIN, k).Lhat, np.asarray(D, dtype=cr.LD)[:, None] * cr.update_problem("G", cr.N_MAIN, k).Lhat)
