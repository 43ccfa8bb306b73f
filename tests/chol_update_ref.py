"""A numpy twin of the rank-k Cholesky update the device runs (fvgp_amd/csrc/chol_update.hip), a helper module of the tests (not a
conftest), and the identity that turns the removal of data points into such an update.

With KV = L L^T, R the sorted removed indices and S the kept ones in their original order,

    KV[S,S] = L[S,S] L[S,S]^T + L[S,R] L[S,R]^T

L[S,S] is lower triangular with a positive diagonal, so the factor of the kept points is chol(L[S,S] L[S,S]^T + W W^T), W = L[S,R]:
a positive rank-|R| update.  `chol_update` is the sweep of the kernels, operation for operation up to fused multiply-adds: passes of at
most 16 columns of W; in a pass column j of L is rotated against the columns p of W in turn with

    q_p = L_jj^2 + sum_{u <= p} W_ju^2,   r_p = sqrt(q_p),   c_p = r_{p-1} / r_p,   s_p = W_jp / r_p      (r_{-1} = L_jj)
    rows i > j:  (L_ij, W_ip) <- (c_p L_ij + s_p W_ip,  c_p W_ip - s_p L_ij),         L_jj <- r_{kp-1}

The extended-precision reference (update_ld, delete_ld) is the EXACT update of the float64 inputs in numpy.longdouble by orthogonal
transforms of [L | W], one Householder reflector per row -- another algorithm than the sweep of rotations, and one that never forms
L L^T + W W^T: the orthogonal update is accurate to sqrt(cond), anything that forms the matrix only to cond, which on the covariance
families of tests/chol_ref.py is up to six orders of magnitude worse than the code under test (tests/test_chol_update_host.py asserts
it).  update_givens_ld, the plain sweep of single rotations in longdouble, exists only to prove update_ld on the host.

The measures, all in longdouble against Lhat = update_ld(L, W) and the inputs, in units of U = 2^-53:

    phi    max_i ||L'_i - Lhat_i||_2 / ||Lhat_i||_2 over ALL rows (chol_ref.phi)
    rho    max_{i >= j} |L L^T + W W^T - L' L'^T|_ij / (nu_i nu_j), nu_i = ||(L_i,:, W_i,:)||_2: the row-norm-wise backward error.  (Not
           chol_ref's componentwise beta: its denominator (|L||L|^T)_ij collapses for far-apart points and the twin itself scores 6e2 ..
           2e5 there.)  Over every row up to RHO_ALL_ROWS rows, beyond that over rho_rows(n): both sides of every 128- and 1024-row
           boundary, the first and last rows and seeded random ones -- phi still sees every row.
    lam    |2 sum log L'_ii - 2 sum log Lhat_ii|  (chol_ref.lam)

What they cannot see, by design: both are relative to a whole ROW.  One element of a small off-diagonal block (far-apart points, an
entry many orders below its row's norm) that is off by 64 units of its own last place moves neither.

The fixtures are the factors numpy.linalg.cholesky(chol_ref.matrix(fam, n)) of the families W, G, H, S, U-, U+ of tests/chol_ref.py
and the operand classes of operand(); the case lists at the end are shared by tests/test_chol_update_host.py (which holds the twin to
caps on every case, so that a bad twin can never widen a device bar) and tests/test_gpu_chol_update_accuracy.py.
"""
import zlib

import numpy as np

import chol_ref

MAX_RANK = 16
LD = chol_ref.LD
U = 2.0 ** -53                      # the unit of every figure of this suite
FLOOR_PHI = FLOOR_RHO = 4 * U       # the floors of the device bar: device <= MARGIN max(twin, floor)
MARGIN = 8
CAP_PHI, CAP_RHO = 256 * U, 64 * U  # the caps on the twin (host test): measured worst 48.8 and 14.3 on W / G / H, k <= 33
RHO_ALL_ROWS = 700


def split_indices(n, removed):
    """(R, S): the sorted unique removed indices and the kept ones, in order"""
    R = np.unique(np.asarray(removed, dtype=np.int64))
    keep = np.ones(n, dtype=bool)
    keep[R] = False
    return R, np.flatnonzero(keep)


def compaction(L, removed):
    """(L[S,S], W = L[S,R]) of a lower-triangular factor: the operands of the update that removes `removed`"""
    L = np.tril(L)
    R, S = split_indices(len(L), removed)
    return L[np.ix_(S, S)].copy(), L[np.ix_(S, R)].copy()


def chol_update(L, W, row0=0):
    """chol(L L^T + W W^T) by the kernels' sweep; rows < row0 of W are taken to be zero (columns left of row0 are skipped).  Returns a new
    array; only the lower triangle of L is read."""
    L = np.tril(np.array(L, dtype=np.float64))
    W = np.array(W, dtype=np.float64).reshape(len(L), -1)
    n, k = W.shape
    for p0 in range(0, k, MAX_RANK):
        Wp = W[:, p0:p0 + MAX_RANK]
        kp = Wp.shape[1]
        for j in range(row0, n):
            l = L[j, j]
            q = l * l + np.cumsum(Wp[j] * Wp[j])
            r = np.sqrt(q)
            rprev = np.concatenate([[l], r[:-1]])
            c, s = rprev / r, Wp[j] / r
            col = L[j + 1:, j].copy()
            for p in range(kp):
                sw = s[p] * Wp[j + 1:, p]
                Wp[j + 1:, p] = c[p] * Wp[j + 1:, p] - s[p] * col
                col = c[p] * col + sw
            L[j + 1:, j] = col
            L[j, j] = r[-1]
    return L


def chol_delete(L, removed):
    """the factor of the kept points from the factor of all of them"""
    Lss, W = compaction(L, removed)
    R, _ = split_indices(len(L), removed)
    return chol_update(Lss, W, row0=int(R[0]) if len(R) and R[0] < len(Lss) else len(Lss))


# ---- the exact update in extended precision ----------------------------------------------------------------------------------------
def _operands_ld(L, W):
    L, W = np.asarray(L), np.asarray(W)
    if L.dtype != np.float64 or W.dtype != np.float64 or L.ndim != 2 or L.shape[0] != L.shape[1]:
        raise TypeError("the factor (square) and the update must be float64 arrays")
    return np.array(np.tril(L), dtype=LD), np.array(W.reshape(len(L), -1), dtype=LD)


def update_ld(L, W):
    """chol(L L^T + W W^T) of the float64 inputs in longdouble: for every row j ONE Householder reflector takes (L_jj, W_j,:) to
    (-r, 0), r = ||(L_jj, W_j,:)||, and is applied to the rows below of [L_:,j | W]; the column is then negated.  u = v + r e_1 with
    v_1 = L_jj > 0, so nothing cancels.  A row of W that is zero needs no reflector (it would be the identity after the negation)."""
    Ll, Wl = _operands_ld(L, W)
    n = len(Ll)
    for j in range(n):
        w = Wl[j]
        if not np.any(w):
            continue
        l = Ll[j, j]
        r = np.sqrt(l * l + w @ w)
        u0 = l + r                                      # u = (l + r, w), u.u = 2 r (l + r)
        if j + 1 < n:
            col = Ll[j + 1:, j]
            tau = (u0 * col + Wl[j + 1:] @ w) / (r * u0)            # 2 (u.x) / (u.u) for every row x below
            Ll[j + 1:, j] = tau * u0 - col                          # -(x_1 - tau u_1)
            Wl[j + 1:] -= tau[:, None] * w[None, :]
        Ll[j, j] = r
        Wl[j] = 0
    return Ll


def update_givens_ld(L, W):
    """the same update by the textbook sweep, one rotation at a time, in longdouble"""
    Ll, Wl = _operands_ld(L, W)
    n, k = Wl.shape
    for j in range(n):
        for p in range(k):
            w = Wl[j, p]
            if w == 0:
                continue
            l = Ll[j, j]
            r = np.sqrt(l * l + w * w)
            c, s = l / r, w / r
            col, wc = Ll[j + 1:, j].copy(), Wl[j + 1:, p].copy()
            Ll[j + 1:, j] = c * col + s * wc
            Wl[j + 1:, p] = c * wc - s * col
            Ll[j, j] = r
            Wl[j, p] = 0
    return Ll


def delete_ld(L, removed):
    return update_ld(*compaction(L, removed))


# ---- the measures ------------------------------------------------------------------------------------------------------------------
def rho_rows(n):
    """None (every row) up to RHO_ALL_ROWS rows, else at most 64 sorted rows: the ends, both sides of every 128-row boundary near the
    1024-row strip and the first blocks, seeded random ones"""
    if n <= RHO_ALL_ROWS:
        return None
    fixed = [0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1151, 1152, 1153, n - 2, n - 1]
    rows = {r for r in fixed if 0 <= r < n}
    for r in np.random.default_rng(7919 * n).permutation(n):
        if len(rows) >= 64:
            break
        rows.add(int(r))
    return sorted(rows)


def gram_low(L, W=None, rows=None):
    """the rows `rows` (None: all) of L L^T (+ W W^T) in longdouble; only entries j <= i are meant to be read"""
    Ll = np.asarray(np.tril(np.asarray(L)), dtype=LD)
    n = len(Ll)
    Wl = None if W is None else np.asarray(np.asarray(W).reshape(n, -1), dtype=LD)
    if rows is not None:
        G = Ll[rows] @ Ll.T
        return G if Wl is None else G + Wl[rows] @ Wl.T
    G = np.zeros((n, n), dtype=LD)
    B = 128
    for i0 in range(0, n, B):
        i1 = min(n, i0 + B)
        for j0 in range(0, i1, B):
            j1 = min(n, j0 + B)
            G[i0:i1, j0:j1] = Ll[i0:i1, :j1] @ Ll[j0:j1, :j1].T             # columns beyond j1 of rows < j1 are zero
        if Wl is not None:
            G[i0:i1, :i1] += Wl[i0:i1] @ Wl[:i1].T
    return G


def row_norms(L, W):
    Ll, Wl = _operands_ld(L, W)
    return np.sqrt(np.sum(Ll * Ll, axis=1) + np.sum(Wl * Wl, axis=1))


def rho(Lnew, gram, nu, rows=None):
    """the row-norm-wise backward error of Lnew against gram = gram_low(L, W, rows) and nu = row_norms(L, W); inf when not finite"""
    Lnew = np.asarray(Lnew)
    if not np.all(np.isfinite(np.tril(Lnew))):
        return float("inf")
    n = len(nu)
    idx = np.arange(n) if rows is None else np.asarray(rows)
    M = np.abs(gram - gram_low(Lnew, None, rows)) / (nu[idx][:, None] * nu[None, :])
    M[np.arange(n)[None, :] > idx[:, None]] = 0
    return float(np.max(M))


def phi(Lnew, Lhat):
    """chol_ref.phi of a float64 result"""
    return chol_ref.phi(np.asarray(Lnew, dtype=np.float64), Lhat)


def phi_ld(A, B):
    """chol_ref.phi between two longdouble factors, neither of them rounded"""
    return chol_ref.phi(np.asarray(A, dtype=LD), np.asarray(B, dtype=LD))


def lam(Lnew, Lhat):
    return chol_ref.lam(np.asarray(Lnew, dtype=np.float64), Lhat)


def lam_value(value, Lhat):
    return chol_ref.lam_value(value, Lhat)


# ---- fixtures: factors and operand classes ---------------------------------------------------------------------------------------------
FAMILIES = ("W", "G", "H", "S", "U-", "U+")
CLASSES = ("dense", "tiny", "huge", "zero_col", "spike", "staggered", "own_cols", "twin_cols")
_FACTORS = {}


def factor(fam, n):
    """numpy.linalg.cholesky(chol_ref.matrix(fam, n)), once per process, read-only"""
    if (fam, n) not in _FACTORS:
        L = np.linalg.cholesky(chol_ref.matrix(fam, n))
        L.setflags(write=False)
        _FACTORS[fam, n] = L
    return _FACTORS[fam, n]


def base_family(fam):
    """the family whose factor, scaled row-wise by chol_ref.row_scale (powers of two), is this family's"""
    return "G" if fam in ("S", "U-", "U+") else fam


def _seed(cls, n, k):
    return [zlib.crc32(cls.encode()), n, k]


def spike_rows(n, k):
    """the row of column p's single non-zero: 0, 127, 128, n - 1, then 1, 129, 63, 64, 255, 256, ... as far as they exist"""
    want = [0, 127, 128, n - 1, 1, 129, 63, 64, 255, 256, 191, 192, 193, n - 2, 2, 130]
    rows = []
    for r in want + list(range(3, n)):
        if 0 <= r < n and r not in rows:
            rows.append(r)
    return [rows[p % len(rows)] for p in range(k)]


# `huge` is dense 2^30 on W.  On the covariance families the EXACT problem at 2^30 is so ill conditioned (cond grows with the square of
# the scale) that the two longdouble routes themselves part by up to 8 U on H (0.064 U on G), above the U / 16 the reference is proven
# to: there the scale is the largest power at which they agree -- 2^16 on G, 2^3 on H (measured: 0.053 U and 0.044 U at k = 17)
HUGE_EXP = {"W": 30, "G": 16, "H": 3}


def operand(cls, L, k, row0=0, huge_exp=30):
    """W (n x k, float64) of a class, deterministic from (class, n, k); every class but own_cols is scaled row-wise by diag L (exactly so
    on the scaled families: their diagonal is a power of two times G's); rows above row0 are zero"""
    n = len(L)
    base = "dense" if cls in ("tiny", "huge") else cls
    rng = np.random.default_rng(_seed(base, n, k))
    if cls == "own_cols":
        cols = np.unique(np.linspace(0, n - 1, k).astype(int)) if k > 1 else np.array([n // 2])
        if len(cols) != k:
            raise ValueError("own_cols needs k <= n distinct columns")
        W = np.tril(L)[:, cols].copy()
    else:
        W = rng.standard_normal((n, k))
        if cls == "tiny":
            W = np.ldexp(W, -30)
        elif cls == "huge":
            W = np.ldexp(W, huge_exp)
        elif cls == "zero_col":
            W[:, k // 2] = 0.0
        elif cls == "spike":
            S = np.zeros((n, k))
            for p, r in enumerate(spike_rows(n, k)):
                S[r, p] = W[r, p]
            W = S
        elif cls == "staggered":
            for p in range(k):
                W[:(37 * p) % n, p] = 0.0
        elif cls == "twin_cols":
            if k < 2:
                raise ValueError("twin_cols needs two columns")
            W[:, 1] = W[:, 0]
        elif cls != "dense":
            raise KeyError(cls)
        W *= np.diag(L)[:, None]
    W[:row0] = 0.0
    return W


# ---- a problem with its exact result and the twin's figures, computed once per process ---------------------------------------------------
class Problem:
    """one update (L, W, row0): Lhat = update_ld, the Gram rows and row norms rho needs, the twin's result and its phi / rho / lam"""

    def __init__(self, L, W, row0=0, twin=None):
        self.L, self.W, self.row0 = L, W, int(row0)
        self.n, self.k = W.shape
        self.Lhat = update_ld(L, W)
        self.rows = rho_rows(self.n)
        self.gram = gram_low(L, W, self.rows)
        self.nu = row_norms(L, W)
        self.twin = chol_update(L, W, row0=row0) if twin is None else twin
        self.twin_figs = self.figures(self.twin)
        for a in (self.Lhat, self.gram, self.nu, self.twin):
            a.setflags(write=False)

    def figures(self, Lnew):
        """(phi, rho, lam) of a float64 result"""
        Lnew = np.tril(np.asarray(Lnew, dtype=np.float64))
        return phi(Lnew, self.Lhat), rho(Lnew, self.gram, self.nu, self.rows), lam(Lnew, self.Lhat)

    def floors(self):
        return FLOOR_PHI, FLOOR_RHO, chol_ref.lam_floor(self.Lhat)

    def bases(self):
        """max(twin, floor) per measure: MARGIN times this is the device bar"""
        return tuple(max(t, f) for t, f in zip(self.twin_figs, self.floors()))


_PROBLEMS = {}


def update_problem(fam, n, k, cls="dense", row0=0):
    key = ("u", fam, n, k, cls, row0)
    if key not in _PROBLEMS:
        L = factor(fam, n)
        _PROBLEMS[key] = Problem(L, operand(cls, L, k, row0, HUGE_EXP.get(fam, 30)), row0)
    return _PROBLEMS[key]


def delete_problem(fam, n, removed, L=None, key=None):
    """the update that removes `removed` from factor(fam, n) (or from the factor L given, cached under `key`)"""
    R, _ = split_indices(n, removed)
    key = ("d", fam, n, tuple(R.tolist())) if key is None else key
    if key not in _PROBLEMS:
        L = factor(fam, n) if L is None else L
        Lss, W = compaction(L, R)
        m = len(Lss)
        _PROBLEMS[key] = Problem(Lss, W, int(R[0]) if R[0] < m else m)
    return _PROBLEMS[key]


# ---- the cases, shared by the host and the device tests ---------------------------------------------------------------------------------
def instantiation(k):
    """how k columns are served: the template arguments of its passes, e.g. 17 -> 'KP16+1'"""
    kp = [min(MAX_RANK, k - p0) for p0 in range(0, k, MAX_RANK)]
    return "KP" + "+".join(str(1 if q == 1 else 2 if q == 2 else 4 if q <= 4 else 8 if q <= 8 else 16) for q in kp)


KP_LIST = (1, 2, 3, 4, 5, 8, 9, 16)
MULTI_PASS = (17, 18, 24, 33, 48)
N_MAIN, N_EDGE, N_CHAIN, N_STRIP = 300, 193, 700, 1300
SMALL_SIZES = (1, 2, 127, 128, 129, 191, 192, 193)          # rows below the first block: 129 -> 1, 191 -> 63, 192 -> 64, 193 -> 65
ROW0_K = (2, 8, 17)
CLASS_K = (2, 5, 17)
SCALE_K = (2, 17)


def row0_list(n):
    return (0, 1, 127, 128, 129, 130, n - 1, n)


def update_cases():
    """(id, fam, n, k, class, row0) of every update the device tests judge by value"""
    out = []
    for fam in ("G", "H"):
        for k in KP_LIST + MULTI_PASS:
            out.append((f"inst|{fam}|n={N_MAIN}|k={k}|{instantiation(k)}", fam, N_MAIN, k, "dense", 0))
    for k in KP_LIST:
        out.append((f"edge nr=1|G|n={N_EDGE}|k={k}|{instantiation(k)}", "G", N_EDGE, k, "dense", 0))
    for fam in ("W", "G"):
        for n in SMALL_SIZES:
            for k in (2, 5, 17):
                out.append((f"size below={max(n - 128, 0)}|{fam}|n={n}|k={k}|{instantiation(k)}", fam, n, k, "dense", 0))
    for k in ROW0_K:
        for row0 in row0_list(N_MAIN):
            out.append((f"row0={row0}|H|n={N_MAIN}|k={k}|{instantiation(k)}", "H", N_MAIN, k, "dense", row0))
    for fam in ("G", "H"):
        for cls in CLASSES:
            for k in CLASS_K:
                out.append((f"class {cls}|{fam}|n={N_MAIN}|k={k}|{instantiation(k)}", fam, N_MAIN, k, cls, 0))
    for k in CLASS_K:
        out.append((f"class huge|W|n={N_MAIN}|k={k}|{instantiation(k)}", "W", N_MAIN, k, "huge", 0))
    for fam in FAMILIES:
        for k in SCALE_K:
            out.append((f"family|{fam}|n={N_MAIN}|k={k}|{instantiation(k)}", fam, N_MAIN, k, "dense", 0))
    for k in (2, 33):
        out.append((f"family|H|n={N_CHAIN}|k={k}|{instantiation(k)}", "H", N_CHAIN, k, "dense", 0))
    return out


def delete_sets(n):
    """the removal sets at n = 300; mixed19: 16 scattered and the last 3 (the second pass starts at row m: skipped); late33: 33 points
    whose 17th lies behind row 256 + 16 (the second pass starts in the third block, the third pass of one column runs too)"""
    rng = np.random.default_rng(9)
    s17 = sorted(rng.choice(n, 17, replace=False).tolist())
    s18 = sorted(rng.choice(n, 18, replace=False).tolist())
    s16 = sorted(rng.choice(n - 3, 16, replace=False).tolist())
    front = sorted(rng.choice(250, 16, replace=False).tolist())
    back = sorted((n - 25 + rng.choice(20, 17, replace=False)).tolist())        # the second pass starts at row >= n - 25 - 16 > 256
    return {"first": [0], "last": [n - 1], "straddle128": [127, 128, 129], "first2": [0, 1], "first16": list(range(16)),
            "scattered17": s17, "scattered18": s18, "every_second": list(range(0, n, 2)), "tail5": list(range(n - 5, n)),
            "mixed19": s16 + [n - 3, n - 2, n - 1], "late33": front + back}


CROSSINGS = ((2, (0,)), (2, (1,)), (129, (0,)), (129, (128,)), (130, (5, 128, 129)), (257, (256,)), (257, (0,)))
# n = 1300, m = 1297: two strips; m - first = 1024: exactly one; 1025: a second strip of one row; the rows around the strip's end
STRIP_SETS = {"two strips": (0, 640, 1290), "one strip of 1024": (273, 700, 1290), "second strip of 1 row": (272, 700, 1290),
              "straddle 1024": (1023, 1024, 1025)}
ROUTE_SET = "scattered17"


def passes_of(n, removed):
    """how the device serves a removal, for the case id: the instantiation, 'skip' for a pass that starts at row m, the strips"""
    R, S = split_indices(n, removed)
    m = len(S)
    if R[0] >= m:
        return "trailing"
    parts = []
    for p0 in range(0, len(R), MAX_RANK):
        q = min(MAX_RANK, len(R) - p0)
        parts.append("skip" if R[p0] - p0 >= m else str(1 if q == 1 else 2 if q == 2 else 4 if q <= 4 else 8 if q <= 8 else 16))
    strips = -(-(m - int(R[0])) // 1024)
    return "KP" + "+".join(parts) + (f" strips={strips}" if strips > 1 else "")


def delete_cases():
    """(id, fam, n, R) of every removal the device tests judge by value"""
    out = []
    for fam in ("G", "H"):
        for name, R in delete_sets(N_MAIN).items():
            out.append((f"set {name}|{fam}|n={N_MAIN}|k={len(R)}|{passes_of(N_MAIN, R)}", fam, N_MAIN, tuple(R)))
    for fam in ("W", "G"):
        for n, R in CROSSINGS:
            out.append((f"crossing m={n - len(R)}|{fam}|n={n}|k={len(R)}|{passes_of(n, R)} R={list(R)}", fam, n, R))
    for name, R in STRIP_SETS.items():
        out.append((f"strip {name}|H|n={N_STRIP}|k=3|{passes_of(N_STRIP, R)}", "H", N_STRIP, R))
    return out


def case_problem(case):
    """the Problem of an entry of update_cases() or delete_cases()"""
    if len(case) == 6:
        return update_problem(*case[1:])
    return delete_problem(*case[1:])


def chain_sets(n=N_CHAIN, steps=8, each=4):
    """eight successive removals of four scattered points, as indices into what is left at each step, and their union in the original
    numbering"""
    rng = np.random.default_rng(41)
    alive = np.arange(n)
    sets = []
    for _ in range(steps):
        pick = np.sort(rng.choice(len(alive), each, replace=False))
        sets.append(pick.tolist())
        alive = np.delete(alive, pick)
    union = np.setdiff1d(np.arange(n), alive)
    return sets, union.tolist()


def route_steps(R):
    """the same removal three ways, each a list of successive index sets into what is left: at once; one point at a time, highest
    first (the indices in front keep their numbers); in two halves, the upper half first"""
    R = sorted(R)
    h = len(R) // 2
    return {"at once": [R], "one at a time": [[r] for r in R[::-1]], "two halves": [R[h:], R[:h]]}


def twin_chain(L, sets):
    for R in sets:
        L = chol_delete(L, R)
    return L
