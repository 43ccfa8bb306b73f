"""The cases that point the nearest-neighbour references at the whole of nn_cond_kernel<KIND, D, M, MODE> (csrc/nn.hip) -- a helper module
of the tests, not a conftest.  Nothing new is measured against: the longdouble references, the float64 twins and the bars
MARGIN * max(base, FLOOR) are those of vecchia_ref (value), vecchia_grad_ref (score) and vecchia_fisher_ref (Fisher), whose ACC_CASES,
GRAD_CASES, CASES, FLOOR and MARGIN stay as they are.  What is here:

    SWEEP_CASES     (kernel, d, n, m, B), built by a rule: every cell (kind, D, M) of the dispatch, the runtime dimension at both of its
                    ends (54 cases for 45 cells); cell() is the Python mirror of dispatch_kind_dim / dispatch_pad
    GAP_CASES       (compact case, m): a compact case's lists scattered over m = 16 / 32 / 64 columns with junk between (gapped_list),
                    judged against the compact case's own reference and bars
    PRED_CASES      (kernel, d, nq, nr, m, s given, B): the conditionals entry in prediction mode (xq apart from xr, nq != nr, nr < m,
                    nr == 1); pred_bars is the project's recipe for mu and d, written once
    the planted errors of tests/test_vecchia_family_host.py: drop_last, gaps_as_zero, dk_dtheta_short

Nothing here comes from the device."""
import functools

import numpy as np

import kernel_family_ref as kf
import vecchia_ref as vr

LD = vr.LD
MARGIN = vr.MARGIN

KINDS = ("rbf", "matern32", "matern52")
PADS = (16, 32, 64)                              # the padded block sizes M of dispatch_pad
M_OF = {16: (1, 7, 15, 16), 32: (17, 25, 31, 32), 64: (33, 48, 63, 64)}
# the smallest row counts with rows that own a full list and rows that do not, none a multiple of the four waves of a workgroup
N_OF = {16: 22, 32: 38, 64: 70}
DIMS = kf.DIMS                                   # 1 .. 4: an instantiation each; 5 and 16: both ends of the runtime dimension (D = 0)


def cell(name, d, m):
    """(kind, D, M): the instantiation a call dispatches to -- dispatch_kind_dim (D = 0 is the runtime dimension) and dispatch_pad"""
    return kf.FAMILY[name][0], d if d <= 4 else 0, 16 if m <= 16 else 32 if m <= 32 else 64


def _sweep():
    """With ik, jd, iM the positions of kind, d and M: iso for odd ik + jd + iM (so every (D, M) pair sees both over the kinds and every
    (kind, D) pair over the M), m = M_OF[M][(jd + iM) mod 4] (the kind has no part in it: every m meets kernels of both sorts),
    B = 2 where ik + jd + iM is a multiple of 4, else 1."""
    out = []
    for ik, kind in enumerate(KINDS):
        for jd, d in enumerate(DIMS):
            for iM, M in enumerate(PADS):
                t = ik + jd + iM
                out.append((kind + ("_iso" if t % 2 else "_ard"), d, N_OF[M], M_OF[M][(jd + iM) % 4], 2 if t % 4 == 0 else 1))
    return tuple(out)


SWEEP_CASES = _sweep()


# ---- lists with gaps ------------------------------------------------------------------------------------------------------------------
# (compact case, m): the compact case's lists hold 10 / 20 / 40 neighbours (the rows i < 10 / 20 / 40 fewer, row 0 none); each M once
# with one length scale and once with one per dimension
GAP_CASES = (
    (("rbf_ard", 3, 22, 10, 1), 16), (("matern32_iso", 2, 22, 10, 1), 16), (("matern52_ard", 5, 38, 20, 1), 32),
    (("rbf_iso", 16, 38, 20, 1), 32), (("matern32_ard", 2, 70, 40, 1), 64), (("matern52_iso", 4, 70, 40, 1), 64),
)


def gap_id(gap):
    return vr.case_id(gap[0]) + "-gaps{}".format(gap[1])


def junk(n):
    """what a list may hold in place of a neighbour: every one outside 0 .. n - 1, both ends of int32 among them"""
    return np.array([-1, -5, n, n + 1000, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def gapped_list(gap):
    """int32 (n, m): row i's valid entries, in their order, at sorted random positions among m columns, junk everywhere else"""
    case, m = gap
    n = case[2]
    idx = vr.case_inputs(case)[4]
    rng = np.random.default_rng(8800 + 10 * m + n)
    out = rng.choice(junk(n), size=(n, m))
    for i in range(n):
        valid = idx[i][(idx[i] >= 0) & (idx[i] < n)]
        out[i, np.sort(rng.choice(m, size=len(valid), replace=False))] = valid
    return out.astype(np.int32)


def compacted(idx, nr):
    """the in-range entries of every row moved to the front in their order, -1 behind them"""
    out = np.full_like(idx, -1)
    for i, row in enumerate(idx):
        keep = row[(row >= 0) & (row < nr)]
        out[i, :len(keep)] = keep
    return out


# ---- prediction shapes ----------------------------------------------------------------------------------------------------------------
# (kernel, d, nq, nr, m, s given, B): nq in {1, 5, 67}, nr in {1, 3, 80} (1 and 3 are fewer reference rows than any list is long), s NULL
# and given, B in {1, 3}, d in {1, 3, 16}, every M
PRED_CASES = (
    ("rbf_ard", 1, 1, 1, 16, False, 1), ("matern32_iso", 3, 5, 3, 16, True, 3), ("matern52_ard", 16, 67, 80, 64, False, 1),
    ("rbf_iso", 3, 67, 80, 33, True, 3), ("matern32_ard", 16, 5, 80, 32, True, 1), ("matern52_iso", 1, 67, 80, 17, False, 3),
    ("rbf_ard", 3, 67, 3, 1, True, 1), ("matern32_ard", 3, 1, 80, 64, False, 3),
)
PRED_FIGURES = ("mu", "d")


def pred_id(case):
    return "{}-d{}-nq{}-nr{}-m{}-s{:d}-B{}".format(*case)


@functools.lru_cache(maxsize=None)
def pred_inputs(case):
    """(xq, xr, thetas (B, H), idx, r, v, s or None): reference rows and queries drawn apart from the unit cube, the lists the twin's
    search over every reference row under the first theta's length scales"""
    name, d, nq, nr, m, with_s, B = case
    rng = np.random.default_rng(9900 + 100 * d + 10 * sorted(kf.FAMILY).index(name) + nq + 7 * nr + m)
    xr, xq = rng.random((nr, d)), rng.random((nq, d))
    theta = kf.case_theta(name, d, rng)
    r = np.sin(3.0 * xr.sum(axis=1)) + 0.1 * rng.standard_normal(nr)
    v = 1e-2 * theta[0] * (1.0 + rng.random(nr))
    s = 1e-2 * theta[0] * (1.0 + rng.random(nq)) if with_s else None
    idx = vr.search_ref(xq, xr, m, vr.length_scales(name, theta, d), c0=-1)
    return xq, xr, vr.batch_thetas(theta, B), idx, r, v, s


def pred_figures(r, got, ref):
    """vecchia_ref's figures of the conditionals alone: `got` = (mu, d) against the longdouble `ref`"""
    scale = max(float(np.max(np.abs(r))), np.finfo(np.float64).tiny)
    return {"mu": float(np.max(np.abs(np.asarray(got[0], dtype=LD) - ref[0]))) / scale,
            "d": float(np.max(np.abs(np.asarray(got[1], dtype=LD) - ref[1]) / np.abs(ref[1])))}


def pred_run(case, b, dtype=LD, perturb=None, idx=None):
    """(mu, d) of the case's theta b in dtype, over the case's lists or over `idx`"""
    xq, xr, thetas, own, r, v, s = pred_inputs(case)
    return vr.conditionals_ref(case[0], xq, xr, thetas[b], own if idx is None else idx, r, v, s=s, dtype=dtype, perturb=perturb)


@functools.lru_cache(maxsize=None)
def pred_reference(case):
    """per b the longdouble (mu, d): computed once, shared, never changed"""
    return tuple(pred_run(case, b) for b in range(case[6]))


@functools.lru_cache(maxsize=None)
def pred_bases(case):
    """vecchia_ref.bases for a prediction case: over the thetas, the larger of the plain float64 twin and the one with every kernel
    entry perturbed by up to kernel_family_ref.k_bound_ulps(d) ulps of sigma^2, against longdouble"""
    r = pred_inputs(case)[4]
    out = dict.fromkeys(PRED_FIGURES, 0.0)
    for b in range(case[6]):
        rng = np.random.default_rng(4242 + b)
        for run in (pred_run(case, b, np.float64), pred_run(case, b, np.float64, perturb=(rng, kf.k_bound_ulps(case[1])))):
            f = pred_figures(r, run, pred_reference(case)[b])
            out = {k: max(out[k], f[k]) for k in PRED_FIGURES}
    return out


def pred_bars(case):
    """{figure: MARGIN * max(base, vecchia_ref.FLOOR[figure])}: what the device may differ from longdouble by"""
    b = pred_bases(case)
    return {k: MARGIN * max(b[k], vr.FLOOR[k]) for k in PRED_FIGURES}


# ---- planted errors: what a wrong kernel would compute, for the host test that shows the checks can fail --------------------------------------
def in_range(idx, nr):
    idx = np.asarray(idx)
    return (idx >= 0) & (idx < nr)


def drop_last(idx, nr):
    """the last valid neighbour of every row dropped"""
    out = np.array(idx)
    for i in range(len(out)):
        pos = np.nonzero(in_range(out[i], nr))[0]
        if len(pos):
            out[i, pos[-1]] = -1
    return out


def gaps_as_zero(idx, nr):
    """every entry that is to be skipped read as index 0"""
    return np.where(in_range(idx, nr), idx, 0).astype(np.asarray(idx).dtype)


def dk_dtheta_short(name, x1, x2, theta, dtype=LD):
    """kernel_family_ref.dk_dtheta_ref with the second dimension left out of an isotropic kernel's length-scale derivative sum (at d = 1
    there is none to leave out)"""
    iso, _, ls, delta, phi, cf = kf._setup(name, x1, x2, theta, dtype)
    dl = np.transpose(cf[:, :, None] * delta ** 2 / ls ** 3, (2, 0, 1))
    if iso:
        dl = np.sum(np.delete(dl, 1, axis=0) if len(dl) > 1 else dl, axis=0, keepdims=True)
    return np.concatenate([phi[None], dl], axis=0)
