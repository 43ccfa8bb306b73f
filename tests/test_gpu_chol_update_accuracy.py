"""fvgp_hip_chol_update / fvgp_hip_chol_delete (csrc/chol_update.hip) and GP.remove_data against the extended-precision reference of
tests/chol_update_ref.py, which tests/test_chol_update_host.py proves on the host: the EXACT update of the float64 inputs by Householder
reflectors in longdouble, never forming L L^T + W W^T (a fresh factorisation of the kept matrix is up to six orders of magnitude less
accurate than the code under test on the covariance families G and H of tests/chol_ref.py).

Bar, never from the device: device <= 8 max(twin, floor) for phi (row-wise forward error, every row), rho (row-norm-wise backward error)
and lam (log-determinant), the twin being the float64 numpy sweep of chol_update_ref on the same inputs against the same exact result;
floors 4 U, 4 U (U = 2^-53) and chol_ref.lam_floor.  The host test caps the twin on every case (phi <= 256 U, rho <= 64 U).

The factor is uploaded with NaN in the strict upper triangle and in every column beyond padded_dim(n), W with NaN beyond its k columns:
a result that is finite, with those bits unchanged, shows they were neither read nor written.  The cases come from chol_update_ref
(update_cases, delete_cases); their ids name the template instantiations (KP1 .. KP16 per pass), the strips and the skipped passes.

Every case prints `CU|route|family|n|k|class|phi dev/twin|rho dev/twin|lam dev/twin|ratios` (pytest -s)."""
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

import chol_ref
import chol_update_ref as cu
import tri_solve_ref as ref

pytestmark = pytest.mark.gpu

U, LD = cu.U, cu.LD
UPDATE_CASES = cu.update_cases()
DELETE_CASES = cu.delete_cases()
# as UPDATE of tests/test_gpu_remove_data.py: a threshold that admits the sets, the cost model off
UPDATE_ARGS = {"remove_update_max_fraction": 0.25, "remove_update_cost_model": False}


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


class _Record:
    """collects a test's record lines (printed whether they pass or not) and its failed checks (asserted together at the end)"""

    def __init__(self):
        self.lines, self.fails = [], []

    def check(self, ok, tag, what):
        if not ok:
            self.fails.append(f"{tag}: {what}")

    def judge(self, tag, P, Lnew, logdet=None):
        """phi, rho and lam of a device result under 8 max(twin, floor); `tag` is route|family|n|k|class.  Returns the ratios."""
        dev = list(P.figures(Lnew))
        if logdet is not None:
            dev[2] = cu.lam_value(logdet, P.Lhat)
        ratios = [d / b for d, b in zip(dev, P.bases())]
        tw = P.twin_figs
        self.lines.append(f"CU|{tag}|phi {dev[0] / U:.3g}/{tw[0] / U:.3g}|rho {dev[1] / U:.3g}/{tw[1] / U:.3g}|lam {dev[2]:.3g}/{tw[2]:.3g}"
                          f"|ratios {ratios[0]:.3g} {ratios[1]:.3g} {ratios[2]:.3g}")
        for name, r, d, b in zip(("phi", "rho", "lam"), ratios, dev, P.bases()):
            self.check(r <= cu.MARGIN, tag, f"{name} {d:.3g} above {cu.MARGIN} x max(twin, floor) = {cu.MARGIN * b:.3g}")
        return ratios

    def note(self, text):
        self.lines.append("CU|" + text)

    def finish(self):
        for ln in self.lines:
            print(ln)
        assert not self.fails, "\n".join(self.fails[:40])


def _tag(case, cls=None):
    """route|family|n|k|class of a case id `what|family|n=..|k=..|instantiation`"""
    what, fam, n, k, inst = case[0].split("|")
    return f"{what} {inst}|{fam}|{n[2:]}|{k[2:]}|{cls if cls is not None else (case[4] if len(case) == 6 else 'removal')}"


# ---- device buffers ------------------------------------------------------------------------------------------------------------------
def _image(L, ld=None):
    """host image of a factor buffer: padded_dim(n) rows of `ld` columns; the lower triangle of L, identity padding on and below the
    diagonal, NaN everywhere else -- the strict upper triangle (of the padding rows too) and every column beyond padded_dim(n)"""
    from fvgp_amd._lib import pad128
    n = len(L)
    npad = pad128(n)
    ld = ld or npad
    buf = np.full((npad, ld), np.nan)
    il = np.tril_indices(npad)
    sq = np.eye(npad)
    sq[:n, :n] = np.tril(L)
    buf[:, :npad][il] = sq[il]
    return buf


def _bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _upper(npad, ld):
    return np.triu(np.ones((npad, ld), dtype=bool), 1)


def _run_update(H, L, W, row0=0, ldl=None, ldw=None):
    """one fvgp_hip_chol_update on fresh uploads: (the whole buffer as it came back, its image before, the columns of W's buffer beyond
    k -- NaN on entry)"""
    n, k = W.shape
    img = _image(L, ldl)
    Wimg = np.full((n, ldw or k), np.nan)
    Wimg[:, :k] = W
    buf, Wd = H.to_device(img), H.to_device(Wimg)
    assert buf.stride(0) == img.shape[1] and Wd.stride(0) == Wimg.shape[1]
    H.chol_update(buf, n, Wd, k=k, row0=row0)
    H.sync()
    return buf.cpu().numpy(), img, Wd.cpu().numpy()[:, k:]


def _check_update_untouched(rec, tag, got, img, n, row0, junk):
    """the strict upper triangle and every column beyond padded_dim(n), the padding rows, the columns left of row0's block (with
    row0 = n: everything) and W's columns beyond k keep their bits; the n x n lower triangle is finite"""
    up = _upper(*img.shape)
    rec.check(_bits(got[up], img[up]), tag, "an entry above the diagonal or beyond padded_dim(n) changed")
    rec.check(_bits(got[n:], img[n:]), tag, "a padding row changed")
    rec.check(bool(np.all(np.isnan(junk))), tag, "a column of W beyond k was written")
    rec.check(bool(np.all(np.isfinite(np.tril(got[:n, :n])))), tag, "L is not finite (junk was read)")
    if row0 >= n:
        rec.check(_bits(got, img), tag, "row0 = n changed the buffer")
    else:
        c0 = row0 // 128 * 128
        rec.check(_bits(np.tril(got[:n, :c0]), np.tril(img[:n, :c0])), tag, "a column left of row0's block changed")


def _run_deletes(H, L, steps, ldl=None):
    """successive fvgp_hip_chol_delete calls in ONE buffer (each `steps` entry indexes what the one before left), then invalidate_factor:
    (device buffer, the whole buffer downloaded, its image before, the points left)"""
    n = len(L)
    img = _image(L, ldl)
    buf = H.to_device(img)
    for R in steps:
        H.chol_delete(buf, n, R)
        n -= len(R)
    H.invalidate_factor()
    H.sync()
    return buf, buf.cpu().numpy(), img, n


def _check_delete_layout(rec, tag, got, img, n, m):
    """what a factor of m points looks like: rows m .. padded_dim(n) - 1 identity on and below the diagonal, exactly; the strict upper
    triangle of the m rows and every column beyond padded_dim(n) keep their bits; the m x m lower triangle finite"""
    npad = img.shape[0]
    pad = np.tril(got[m:npad, :npad], m)
    rec.check(np.array_equal(pad, np.eye(npad)[m:]), tag, f"rows {m} .. {npad - 1} are not the identity padding")
    up = _upper(m, img.shape[1])
    up[:, npad:] = True
    rec.check(_bits(got[:m][up], img[:m][up]), tag, "an entry above the diagonal or beyond padded_dim(n) changed")
    rec.check(_bits(got[m:, npad:], img[m:, npad:]), tag, "a column beyond padded_dim(n) changed")
    rec.check(bool(np.all(np.isfinite(np.tril(got[:m, :m])))), tag, "L is not finite (junk was read)")


# ---- fvgp_hip_chol_update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update(H, case):
    """every case of chol_update_ref.update_cases(): the instantiations KP 1 / 2 / 4 / 8 / 16 of both kernels and the multi-pass counts on G
    and H, the panel's row edge (n = 193: a last workgroup of one row; 1 / 63 / 64 / 65 rows below the first block), row0 on both sides of
    the block boundary and at n - 1 and n, every operand class, every family.  Values under the bar, what must not be touched, and a
    second identical call gives the same bits."""
    _, fam, n, k, cls, row0 = case
    P = cu.update_problem(fam, n, k, cls, row0)
    rec = _Record()
    tag = _tag(case)
    got, img, junk = _run_update(H, P.L, P.W, row0)
    Lnew = np.tril(got[:n, :n])
    rec.judge(tag, P, Lnew)
    _check_update_untouched(rec, tag, got, img, n, row0, junk)
    again, _, _ = _run_update(H, P.L, P.W, row0)
    rec.check(_bits(again, got), tag, "a second identical call gives other bits")
    rec.finish()


@pytest.mark.parametrize("k", [2, 17])
@pytest.mark.parametrize("fam", ["G", "H"])
def test_update_leading_dimensions(H, fam, k):
    """ldw in {k, k + 1, k + 7} x ldl in {padded_dim(n), padded_dim(n) + 2, 512} with NaN in every column beyond k of W and beyond
    padded_dim(n) of L: under the bar, the junk untouched, and the same bits whatever the leading dimensions"""
    n = cu.N_MAIN
    P = cu.update_problem(fam, n, k)
    rec = _Record()
    base = None
    for ldl in (384, 386, 512):
        for ldw in (k, k + 1, k + 7):
            tag = f"ldl={ldl} ldw={ldw} {cu.instantiation(k)}|{fam}|{n}|{k}|dense"
            got, img, junk = _run_update(H, P.L, P.W, 0, ldl, ldw)
            Lnew = np.tril(got[:n, :n])
            rec.judge(tag, P, Lnew)
            _check_update_untouched(rec, tag, got, img, n, 0, junk)
            rec.check(junk.shape[1] == ldw - k, tag, "the junk columns of W")
            base = Lnew if base is None else base
            rec.check(_bits(Lnew, base), tag, "the leading dimensions change the bits of L")
    rec.finish()


@pytest.mark.parametrize("k", cu.SCALE_K)
@pytest.mark.parametrize("fam", ["S", "U-", "U+"])
def test_update_of_a_scaled_problem_is_the_scaled_update(H, fam, k):
    """D L and D W with D powers of two (S: 2^-20 .. 2^20 row by row; U: 2^-200, 2^200): the device result is D times the device result
    on G, bit for bit -- the sums have a fixed order and (c, s) are ratios of one row's entries, so only an absolute threshold or an
    under- / overflow could break it"""
    n = cu.N_MAIN
    Ps, Pg = cu.update_problem(fam, n, k), cu.update_problem("G", n, k)
    D = chol_ref.row_scale(fam, n)
    assert np.array_equal(Ps.L, D[:, None] * Pg.L) and np.array_equal(Ps.W, D[:, None] * Pg.W)
    rec = _Record()
    tag = f"scaled {cu.instantiation(k)}|{fam}|{n}|{k}|dense"
    gs, _, _ = _run_update(H, Ps.L, Ps.W)
    gg, _, _ = _run_update(H, Pg.L, Pg.W)
    same = _bits(np.tril(gs[:n, :n]), D[:, None] * np.tril(gg[:n, :n]))
    rec.note(f"{tag}|bits equal to the scaled result on G: {same}")
    rec.check(same, tag, "the result is not D times the result on G bit for bit")
    rec.finish()


@pytest.mark.parametrize("k", [2, 8])
def test_leading_rows_do_not_depend_on_what_follows(H, k):
    """row i of the result depends on rows <= i only: the update of n = 300 and that of its leading 129 rows agree bit for bit on those
    rows (H, row0 = 5), at k = 2 and 8 -- the counts the older test of this property does not run"""
    n = cu.N_MAIN
    P = cu.update_problem("H", n, k, "dense", 5)
    big, _, _ = _run_update(H, P.L, P.W, 5)
    small, _, _ = _run_update(H, P.L[:129, :129], P.W[:129].copy(), 5)
    assert _bits(np.tril(big[:129, :129]), np.tril(small[:129, :129]))


# ---- fvgp_hip_chol_delete ------------------------------------------------------------------------------------------------------------------
def _potrs_ld(Lhat, B):
    """(Lhat Lhat^T) X = B by substitution in longdouble with the exact factor: chol_ref.fwd_ld column by column, then its transpose"""
    n = Lhat.shape[0]
    X = np.empty(B.shape, dtype=LD)
    for c in range(B.shape[1]):
        y = chol_ref.fwd_ld(Lhat, B[:, c])
        for i in range(n - 1, -1, -1):
            if i + 1 < n:
                y[i] -= Lhat[i + 1:, i] @ y[i + 1:]
            y[i] /= Lhat[i, i]
        X[:, c] = y
    return X


def _check_serves_as_a_factor(H, rec, tag, P, buf, m, solves=True):
    """after invalidate_factor: fvgp_hip_logdet under the lam bar; fvgp_hip_potrs with 1, 3 and 8 right-hand sides against longdouble
    substitution with the exact factor, under the bar of the solves suite (tests/test_gpu_chol.py, alpha: 8 max(scipy's cho_solve, the
    block-inverse twin at 128, 4 eps) per column and the cap 64 eps cond_2(L)^2, both on the twin's float64 factor); junk in the
    padding rows of the right-hand side comes back zero"""
    from fvgp_amd._lib import pad128
    lam_dev = cu.lam_value(H.logdet(buf, m), P.Lhat)
    base = P.bases()[2]
    rec.check(lam_dev <= cu.MARGIN * base, tag, f"logdet {lam_dev:.3g} above {cu.MARGIN} x max(twin, floor) = {cu.MARGIN * base:.3g}")
    cap = 64 * ref.EPS * ref.cond2(P.twin) ** 2 if solves else 0.0
    worst = 0.0
    for nrhs in (1, 3, 8) if solves else ():
        rhs = ref.rhs(m, nrhs, 23)
        want = _potrs_ld(P.Lhat, rhs)
        B = np.full((pad128(m), nrhs), 7.0)
        B[:m] = rhs
        Bd = H.to_device(B)
        H.potrs(buf, m, Bd, nrhs)
        H.sync()
        out = Bd.cpu().numpy()
        rec.check(bool(np.all(out[m:] == 0)), tag, f"potrs nrhs={nrhs}: the padding rows are not zero")
        e_dev = ref.col_err(out[:m], want)[1] if np.all(np.isfinite(out[:m])) else np.inf
        e_sp = ref.col_err(sla.cho_solve((P.twin, True), rhs), want)[1]
        e_tw = ref.col_err(ref.blockinv_potrs(P.twin, rhs, 128), want)[1]
        b = max(e_sp, e_tw, 4 * ref.EPS)
        worst = max(worst, e_dev / b)
        rec.check(e_dev <= 8 * b and e_dev <= cap, tag,
                  f"potrs nrhs={nrhs}: {e_dev:.3g} above 8 x max(scipy {e_sp:.3g}, twin {e_tw:.3g}, 4 eps) or the cap {cap:.3g}")
    rec.note(f"{tag}|logdet lam {lam_dev:.3g} ratio {lam_dev / base:.3g}|potrs worst ratio {worst:.3g}")


@pytest.mark.parametrize("case", DELETE_CASES, ids=[c[0] for c in DELETE_CASES])
def test_delete(H, case):
    """every case of chol_update_ref.delete_cases(): the sets at n = 300 on G and H (a two-column pass, a skipped later pass, a later
    pass two blocks behind the first), the removals that cross a padded_dim boundary (m = 127, 128, 256, 1), and at n = 1300 the
    compaction in two strips, in exactly one, with a second strip of one row and around row 1024.  The result must be exactly what a
    factor of m points looks like, and serve as one; a second identical call gives the same bits."""
    _, fam, n, R = case
    R = list(R)
    P = cu.delete_problem(fam, n, R)
    rec = _Record()
    tag = _tag(case)
    buf, got, img, m = _run_deletes(H, cu.factor(fam, n), [R])
    rec.judge(tag, P, np.tril(got[:m, :m]))
    _check_delete_layout(rec, tag, got, img, n, m)
    _check_serves_as_a_factor(H, rec, tag, P, buf, m, solves=n <= cu.N_MAIN)          # (the solves at n = 300 and below: seconds at 1300)
    _, again, _, _ = _run_deletes(H, cu.factor(fam, n), [R])
    rec.check(_bits(again, got), tag, "a second identical call gives other bits")
    rec.finish()


@pytest.mark.parametrize("name", ["two strips", "second strip of 1 row"])
def test_compaction_is_a_pure_permutation(H, name):
    """n = 1300: a factor whose removed columns are zero below the diagonal has W = 0, every rotation is c = 1, s = 0, and the result is
    tril(L)[S, S] bit for bit -- through two strips whose source and destination overlap; and a removal of trailing points alone leaves
    the kept triangle where it is"""
    n = cu.N_STRIP
    R = list(cu.STRIP_SETS[name])
    L = np.array(cu.factor("H", n))
    for r in R:
        L[r + 1:, r] = 0.0
    _, S = cu.split_indices(n, R)
    rec = _Record()
    tag = f"permutation {name}|H|{n}|3|zero W"
    _, got, img, m = _run_deletes(H, L, [R])
    rec.check(_bits(np.tril(got[:m, :m]), np.tril(L)[np.ix_(S, S)]), tag, "the compacted triangle is not tril(L)[S, S] bit for bit")
    _check_delete_layout(rec, tag, got, img, n, m)
    tail = [n - 3, n - 2, n - 1]
    _, got, img, m = _run_deletes(H, L, [tail])
    rec.check(_bits(got[:m], img[:m]), tag, "removing trailing points changed the kept rows")
    _check_delete_layout(rec, tag + " trailing", got, img, n, m)
    rec.note(f"{tag}|bit for bit: {not rec.fails}")
    rec.finish()


@pytest.mark.parametrize("ldl", [386, 512])
@pytest.mark.parametrize("fam", ["G", "H"])
def test_delete_wide_leading_dimension(H, fam, ldl):
    """n = 300 in a buffer of 386 and of 512 columns, NaN beyond column 384: the same bits as with the minimal leading dimension, the
    junk untouched"""
    n = cu.N_MAIN
    rec = _Record()
    for name in ("scattered18", "mixed19"):
        R = cu.delete_sets(n)[name]
        P = cu.delete_problem(fam, n, R)
        tag = f"ldl={ldl} set {name} {cu.passes_of(n, R)}|{fam}|{n}|{len(R)}|removal"
        _, got, img, m = _run_deletes(H, cu.factor(fam, n), [R], ldl)
        _, base, _, _ = _run_deletes(H, cu.factor(fam, n), [R])
        rec.judge(tag, P, np.tril(got[:m, :m]))
        _check_delete_layout(rec, tag, got, img, n, m)
        rec.check(_bits(np.tril(got[:, :384]), np.tril(base)), tag, "the leading dimension changes the bits")
    rec.finish()


@pytest.mark.parametrize("fam", ["G", "H"])
def test_delete_routes_agree_within_the_bar(H, fam):
    """the same 17 points at once, one at a time (highest first) and in two halves: each against delete_ld of the ORIGINAL factor, the
    base being the twin run the same way"""
    n = cu.N_MAIN
    R = cu.delete_sets(n)[cu.ROUTE_SET]
    exact = cu.delete_problem(fam, n, R)
    rec = _Record()
    for name, steps in cu.route_steps(R).items():
        P = _with_twin(exact, cu.twin_chain(cu.factor(fam, n), steps))
        tag = f"route {name}|{fam}|{n}|{len(R)}|removal"
        _, got, img, m = _run_deletes(H, cu.factor(fam, n), steps)
        rec.judge(tag, P, np.tril(got[:m, :m]))
        _check_delete_layout(rec, tag, got, img, n, m)
    rec.finish()


class _WithTwin:
    """an exact Problem judged against another twin result (the twin run along the same route)"""

    def __init__(self, P, twin):
        self.P, self.Lhat = P, P.Lhat
        self.twin = twin
        self.twin_figs = P.figures(twin)

    def figures(self, Lnew):
        return self.P.figures(Lnew)

    def bases(self):
        return tuple(max(t, f) for t, f in zip(self.twin_figs, self.P.floors()))


def _with_twin(P, twin):
    return _WithTwin(P, twin)


def test_delete_chain(H):
    """eight successive removals of four scattered points in one buffer (H, n = 700): the exact result is delete_ld of the ORIGINAL factor
    for the union, the base the twin chained the same way -- error that grows faster than the twin's fails"""
    n = cu.N_CHAIN
    sets, union = cu.chain_sets()
    L = cu.factor("H", n)
    P = _with_twin(cu.delete_problem("H", n, union), cu.twin_chain(L, sets))
    rec = _Record()
    tag = f"chain 8 x 4|H|{n}|32|removal"
    buf, got, img, m = _run_deletes(H, L, sets)
    rec.judge(tag, P, np.tril(got[:m, :m]), logdet=H.logdet(buf, m))
    _check_delete_layout(rec, tag, got, img, n, m)
    rec.finish()


# ---- the facade --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scattered17", "mixed19"])
def test_remove_data_hands_over_the_right_factor(name):
    """a GP on the recipe of H (RBF, l = 0.1, noise 1e-8, 700 points of the unit square), where a fresh factorisation could not be the
    yardstick: Chol_factor after remove_data is within the phi bar of delete_ld(Chol_factor before, R), logdet_KV within the lam bar"""
    import fvgp_amd
    n = cu.N_CHAIN
    ell, noise = chol_ref.PARAMS["H"]
    x = np.random.default_rng(chol_ref.SEED).random((n, 2))
    y = np.sin(3.0 * x.sum(axis=1))
    rng = np.random.default_rng(9)
    R = sorted(rng.choice(n, 17, replace=False).tolist()) if name == "scattered17" else \
        sorted(rng.choice(n - 3, 16, replace=False).tolist()) + [n - 3, n - 2, n - 1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = fvgp_amd.GP(x, y, init_hyperparameters=np.array([1.0, ell, ell]), noise_variances=np.full(n, noise), kernel_function="rbf_ard",
                         args=dict(UPDATE_ARGS))
    before = np.tril(np.array(gp.Chol_factor, dtype=np.float64))
    assert before.shape == (n, n)
    assert np.max(np.abs(before - cu.factor("H", n))) <= 1e-5                # the factor of H up to what its conditioning allows
    res = gp.remove_data(R)
    assert res["route"] == "update" and gp.point_number == n - len(R)
    after = np.tril(np.array(gp.Chol_factor, dtype=np.float64))
    P = cu.delete_problem("H", n, R, L=before, key=("facade", name))
    rec = _Record()
    tag = f"facade {name} {cu.passes_of(n, R)}|H|{n}|{len(R)}|removal"
    rec.check(after.shape == (n - len(R),) * 2, tag, f"Chol_factor has shape {after.shape}")
    if not rec.fails:
        rec.judge(tag, P, after, logdet=float(gp.logdet_KV))
    rec.finish()
