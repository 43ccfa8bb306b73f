"""fvgp_hip_gemm, the one exported door to the fp64 MFMA product kernels (fvgp_amd/csrc/gemm.hip), on every kernel it can pick,
in every operand layout and at the edges of each, against the references of tests/gemm_ref.py: the exact family (integer operands,
one correct bit pattern, np.array_equal) and the rounding family (longdouble reference, componentwise gamma bound).

Which kernel a call reaches is decided by three rules, mirrored by `route` below and named in every case id:
  * fvgp_hip_gemm splits K over gridDim.y when K >= 1024, C is 16-byte aligned with an even ldc and the launch has fewer than
    256 tiles: split = min(64 / ceil(tiles / 8), K / 256) slices of ceil(K / 16 / split) steps, then launch_splitk_reduce;
  * gemm_takes_small_tiles sends an unsplit (M,K)-stored A with at most `small_tile_max` (160) tiles and K <= 512 to the 64-tile
    kernels: gemm_f64_small_kernel<64,64,BNM>, the one-stage gemm_f64_k128_kernel<64> for B (N,K), K == 128 and option
    `k128_kernels`, and gemm_f64_small_kernel<128,32,1> for C == B stored (K,N) with M == 128;
  * everything else runs gemm_f64_kernel<AKM,BNM,0> on 128-tiles, its blockIdx -> tile map read from the XCD-balanced table when
    option `tile_tables` is set and the grid of whole super-tiles has at least 64 blocks, computed by formula otherwise.
So `small_tile_max` = 0 (or a_kmajor = 1, or K > 512) puts a small shape on the 128-tile kernel and `k128_kernels` = 0 takes
K == 128 off the one-stage kernel."""
import contextlib
import functools
import re

import numpy as np
import pytest

import gemm_ref as ref

pytestmark = pytest.mark.gpu

DEFAULTS = dict(small_tile_max=160, tile_tables=1, k128_kernels=1)
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
BIG = dict(small_tile_max=0)           # the 128-tile kernel at any shape
WORST = {}                             # kernel variant -> worst observed fraction of the rounding bound


@pytest.fixture(scope="module")
def H():
    from fvgp_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@contextlib.contextmanager
def options(H, opts):
    try:
        for k, v in opts.items():
            H.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            H.set_option(k, v)


def grid_tiles(tm, tn, lower):
    """gemm_grid_tiles: the 128-tile kernel's grid, whole super-tiles of 8 x min(8, tn) tiles"""
    SN = min(tn, 8)
    sm, sn = (tm + 7) // 8, (tn + SN - 1) // SN
    if lower and SN == 8:
        nst = sm * (sm + 1) // 2 if sm <= sn else sn * (sn + 1) // 2 + (sm - sn) * sn
    else:
        nst = sm * sn
    return nst * 8 * SN


def route(akm, bnm, lower, M, N, K, opts=None, c_is_b=False, c_splittable=True):
    """(kernel the call reaches, number of K slices), by the rules of fvgp_hip_gemm, gemm_takes_small_tiles and launch_gemm"""
    o = dict(DEFAULTS); o.update(opts or {})
    tm, tn = M // 128, N // 128
    if K >= 1024 and c_splittable:
        tiles = tm * (tm + 1) // 2 if lower else tm * tn
        split = 1 if tiles >= 256 else 64 // ((tiles + 7) // 8)
        split = min(split, K // 256)
        if split > 1:
            return f"split{split}+tile128<{akm},{bnm}>", split
    small = not akm and tm * tn <= o["small_tile_max"] and K <= 512 and (not c_is_b or (bnm and M == 128))
    if small:
        if bnm:
            return ("small<128,32,1>" if c_is_b else "small<64,64,1>"), 1
        return ("k128<64>" if K == 128 and o["k128_kernels"] else "small<64,64,0>"), 1
    table = o["tile_tables"] and grid_tiles(tm, tn, lower) >= 64
    return f"tile128<{akm},{bnm}>/" + ("table" if table else "formula"), 1


@functools.lru_cache(maxsize=None)
def exact(M, N, K):
    return ref.exact_case(M, N, K, seed=1000 + M + 3 * N + 7 * K)          # shared by the cases of a shape: nobody writes to it


@functools.lru_cache(maxsize=None)
def exact_want(M, N, K, alpha, beta):
    return ref.exact_ref(*exact(M, N, K), alpha, beta)


def expect(want, C0, mask):
    """the computed tiles from the reference, every other entry as it was"""
    return np.where(mask, want, C0)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def pattern(shape, seed):
    """a recognisable non-zero fill for what a call must leave alone"""
    return np.random.default_rng(seed).integers(1, 1 << 20, shape).astype(np.float64) + 0.5


def run(H, akm, bnm, lower, M, N, K, alpha, beta, opA, opB, C0, opts=None, place="tight"):
    """one call of the entry; returns C on the host.  place: "tight"; "odd" (odd ldc) and "off8" (C 8 bytes off 16-byte alignment):
    the two placements the entry documents as taking the unsplit product"""
    A, B = ref.store(opA, opB, akm, bnm)
    dA, dB = H.to_device(A), H.to_device(B)
    if place == "tight":
        dC = H.to_device(C0)
    elif place == "odd":
        dC = H.to_device(np.concatenate([C0, pattern((M, 1), 5)], axis=1))[:, :N]
        assert dC.stride(0) % 2 == 1
    else:
        dC = H.to_device(np.concatenate([pattern((M, 1), 6), C0, pattern((M, 1), 7)], axis=1))[:, 1:N + 1]
        assert dC.stride(0) % 2 == 0 and dC.data_ptr() % 16 == 8
    with options(H, opts or {}):
        H.gemm(akm, bnm, lower, M, N, K, alpha, dA, dB, beta, dC)
        H.sync()
    return H.to_host(dC)


# ---- exact family: every kernel x layout x lower x K ----------------------------------------------------------------------------
def _lattice():
    cases = []
    for akm, bnm in LAYOUTS:
        for lower in (0, 1):
            for K in (16, 32, 48, 128, 176, 528):       # one, two, three steps of the double-buffered loop; K == 128; odd and even step counts
                M, N = (384, 384) if lower else (256, 384)
                seen = set()
                for opts in (BIG, {}, dict(k128_kernels=0)):
                    kern = route(akm, bnm, lower, M, N, K, opts)[0]
                    if kern not in seen:
                        seen.add(kern)
                        cases.append(pytest.param(akm, bnm, lower, K, opts, kern, id=f"{kern}-lower{lower}-K{K}"))
    return cases


LATTICE = _lattice()


def test_the_lattice_reaches_every_kernel():
    """the case list itself: each instantiation behind the entry appears, the 128-tile kernel in all four layouts and at every K"""
    kerns = {}
    for p in LATTICE:
        kerns.setdefault(p.values[5], set()).add(p.values[3])
    for akm, bnm in LAYOUTS:
        assert kerns[f"tile128<{akm},{bnm}>/formula"] == {16, 32, 48, 128, 176, 528}
    assert kerns["small<64,64,0>"] == {16, 32, 48, 128, 176} and kerns["small<64,64,1>"] == {16, 32, 48, 128, 176}
    assert kerns["k128<64>"] == {128}


@pytest.mark.parametrize("akm,bnm,lower,K,opts,kern", LATTICE)
def test_exact_every_kernel_layout_and_k(H, akm, bnm, lower, K, opts, kern):
    """All four layouts x lower x K in {16, 32, 48, 128, 176, 528}, alpha / beta = -0.75 / 1.25, on the 128-tile kernel (option
    small_tile_max = 0; the K loop by LDS-DMA in layout (0,0), through registers in the others) and, where the dispatch sends the
    shape there at the defaults (A stored (M,K), 6 or 9 tiles, K <= 512), on small<64,64,0>, small<64,64,1> and k128<64> (K == 128,
    B (N,K); k128_kernels = 0 gives small<64,64,0> at K == 128 too).  Bit-exact; with `lower` the tiles above the diagonal keep C0."""
    M, N = (384, 384) if lower else (256, 384)
    opA, opB, C0 = exact(M, N, K)
    got = run(H, akm, bnm, lower, M, N, K, -0.75, 1.25, opA, opB, C0, opts)
    assert np.array_equal(got, expect(exact_want(M, N, K, -0.75, 1.25), C0, ref.tile_mask(M, N, lower)))


# ---- exact family: split-K ----------------------------------------------------------------------------------------------------------
SPLIT = [(akm, bnm, 0, 256, 384, 1040) for akm, bnm in LAYOUTS] + \
        [(0, 0, 1, 384, 384, 1024), (1, 1, 1, 384, 384, 1024), (0, 0, 0, 128, 128, 16400), (1, 1, 0, 128, 128, 16400)]


def _split_id(c, place):
    akm, bnm, lower, M, N, K = c
    return f"{route(akm, bnm, lower, M, N, K, c_splittable=place == 'tight')[0]}-lower{lower}-{M}x{N}x{K}-C_{place}"


@pytest.mark.parametrize("case,place", [pytest.param(c, p, id=_split_id(c, p)) for c in SPLIT for p in ("tight", "odd", "off8")])
def test_exact_split_k(H, case, place):
    """K >= 1024 with 6 tiles (256 x 384, and 384 x 384 lower) or one (128 x 128): fvgp_hip_gemm splits K.  256 x 384 x 1040: 4 slices
    of 17, 17, 17 and 14 steps; 384 x 384 x 1024 lower: 4 of 16; 128 x 128 x 16400: 64 slices of 17 steps of which 61 .. 63 start
    past K and are empty (they must contribute zeros, not stale scratch).  beta = 1.25, and beta = 0 over a C full of NaN.
    With C at an odd ldc or 8 bytes off alignment the entry takes the unsplit 128-tile kernel instead: same bits in this family."""
    akm, bnm, lower, M, N, K = case
    kern, S = route(akm, bnm, lower, M, N, K, c_splittable=place == "tight")
    assert (S > 1) == (place == "tight") and (kern.startswith("split") or kern.startswith("tile128"))
    if place == "tight":
        assert S == (64 if K == 16400 else 4)
    opA, opB, C0 = exact(M, N, K)
    mask = ref.tile_mask(M, N, lower)
    got = run(H, akm, bnm, lower, M, N, K, -0.75, 1.25, opA, opB, C0, place=place)
    assert np.array_equal(got, expect(exact_want(M, N, K, -0.75, 1.25), C0, mask))
    nan = np.full((M, N), np.nan)
    got = run(H, akm, bnm, lower, M, N, K, 0.75, 0.0, opA, opB, nan, place=place)
    assert np.array_equal(got[mask], exact_want(M, N, K, 0.75, 0.0)[mask]) and np.all(np.isnan(got[~mask]))


# ---- exact family: beta = 0 must not read C -------------------------------------------------------------------------------------------
def _beta0():
    cases = []
    for akm, bnm in LAYOUTS:
        cases.append((akm, bnm, 176, BIG))
    cases += [(0, 0, 176, {}), (0, 1, 176, {}), (0, 0, 128, {}), (0, 0, 128, dict(k128_kernels=0)), (0, 1, 128, {})]
    return [pytest.param(a, b, K, o, id=f"{route(a, b, 0, 256, 384, K, o)[0]}-K{K}") for a, b, K, o in cases]


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("akm,bnm,K,opts", _beta0())
def test_exact_beta_zero_over_nan(H, akm, bnm, K, opts, lower):
    """beta == 0 over a C full of NaN, unsplit: the 128-tile kernel's epilogue (store_tile) has one branch that reads C (beta != 0,
    the lattice above) and one that must not (here), in all four layouts; the 64-tile kernels and the one-stage kernel skip their
    up-front fetch of C.  0 * NaN anywhere would leave NaN.  Tiles a `lower` call does not compute stay NaN."""
    M, N = (384, 384) if lower else (256, 384)
    opA, opB, _ = exact(M, N, K)
    mask = ref.tile_mask(M, N, lower)
    got = run(H, akm, bnm, lower, M, N, K, 0.75, 0.0, opA, opB, np.full((M, N), np.nan), opts)
    assert np.array_equal(got[mask], exact_want(M, N, K, 0.75, 0.0)[mask]) and np.all(np.isnan(got[~mask]))


# ---- exact family: tile maps on the device --------------------------------------------------------------------------------------------
MAPS = [(1, 9, 9), (1, 12, 12), (1, 11, 8), (1, 3, 9), (0, 9, 3), (0, 3, 9), (0, 17, 9)]
MAP_MODES = {"table": dict(small_tile_max=0, tile_tables=1), "formula": dict(small_tile_max=0, tile_tables=0), "default": {}}


def _map_id(lower, tm, tn, mode):
    return f"{route(0, 0, lower, tm * 128, tn * 128, 32, MAP_MODES[mode])[0]}-lower{lower}-{tm}x{tn}tiles-{mode}"


@pytest.mark.parametrize("lower,tm,tn,mode", [pytest.param(l, tm, tn, m, id=_map_id(l, tm, tn, m)) for l, tm, tn in MAPS for m in MAP_MODES])
def test_exact_tile_maps(H, lower, tm, tn, mode):
    """blockIdx -> tile on the device, K = 32 so that a tile is cheap and every tile has its own data: a tile computed twice, not at
    all or from another tile's operands changes bits.  `lower` with 9 x 9 and 12 x 12 tiles (triangular enumeration of the 8 x 8
    super-tiles, ragged last super-tile), 11 x 8 (more super-rows than super-columns) and 3 x 9 (tiles_m != tiles_n, one super-tile);
    full grids of 9 x 3 (super-tiles 8 x 3: 48 blocks, under the 64 a table needs -- formula in both settings), 3 x 9 and 17 x 9.
    Each on the 128-tile kernel (small_tile_max = 0) with the XCD-balanced table and with the formula map, and at the defaults, where
    at most 160 tiles and K <= 512 send it to the 64-tile kernels' own plain grid (B (N,K) and B (K,N))."""
    M, N, K = tm * 128, tn * 128, 32
    opA, opB, C0 = exact(M, N, K)
    want = expect(exact_want(M, N, K, -0.75, 1.25), C0, ref.tile_mask(M, N, lower))
    kern = route(0, 0, lower, M, N, K, MAP_MODES[mode])[0]
    if mode == "default":
        assert kern == "small<64,64,0>" and route(0, 1, lower, M, N, K)[0] == "small<64,64,1>"
    else:
        assert kern == "tile128<0,0>/" + ("table" if mode == "table" and (tm, tn) != (9, 3) else "formula")
    for bnm in ((0, 1) if mode == "default" else (0,)):
        got = run(H, 0, bnm, lower, M, N, K, -0.75, 1.25, opA, opB, C0, MAP_MODES[mode])
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"first wrong entry at {bad[0]}, tiles {sorted({(int(i) // 128, int(j) // 128) for i, j in bad})[:8]}"


# ---- exact family: in place over B (K, N) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 1.25])
def test_exact_in_place_over_the_kn_operand(H, beta):
    """b_nmajor = 1, C == B, M = K = 128, N = 384: gemm_takes_small_tiles lets this aliasing onto small tiles only for M == 128, and
    launch_gemm then picks gemm_f64_small_kernel<128,32,1>, whose workgroup owns 32 whole columns of B and C"""
    M, N, K = 128, 384, 128
    assert route(0, 1, 0, M, N, K, c_is_b=True)[0] == "small<128,32,1>"
    opA, opB, _ = exact(M, N, K)
    dA, dB = H.to_device(opA), H.to_device(opB)
    H.gemm(0, 1, 0, M, N, K, -0.75, dA, dB, beta, dB)
    H.sync()
    assert np.array_equal(H.to_host(dB), -0.75 * (opA @ opB) + beta * opB)
    assert np.array_equal(H.to_host(dA), opA)


# ---- exact family: pitched operands and the footprint of C ---------------------------------------------------------------------------------
def _pitched():
    cases = [(akm, bnm, 176, BIG) for akm, bnm in LAYOUTS]
    cases += [(0, 0, 176, {}), (0, 1, 176, {}), (0, 0, 128, {}), (0, 0, 1040, {}), (1, 1, 1040, {}), (0, 1, 1040, {}), (1, 0, 1040, {})]
    return [pytest.param(a, b, K, o, id=f"{route(a, b, 0, 256, 384, K, o)[0]}-K{K}") for a, b, K, o in cases]


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("akm,bnm,K,opts", _pitched())
def test_exact_pitched_operands_and_footprint(H, akm, bnm, K, opts, lower):
    """A, B and C are column slices, at even column offsets, of wider arrays filled with a pattern: three different leading
    dimensions, all above the tight ones; C also has rows of its parent above and below it.  On the 128-tile kernel (all four
    layouts), the 64-tile and one-stage kernels and split-K (whose reduction writes C in 16-byte pairs).  Every element of C's
    parent outside the M x N window -- and, with `lower`, every tile above the diagonal inside it -- keeps its bits."""
    M, N = (384, 384) if lower else (256, 384)
    opA, opB, C0 = exact(M, N, K)
    A, B = ref.store(opA, opB, akm, bnm)
    pa = pattern((A.shape[0], A.shape[1] + 10), 11); pa[:, 2:2 + A.shape[1]] = A
    pb = pattern((B.shape[0], B.shape[1] + 24), 12); pb[:, 4:4 + B.shape[1]] = B
    pc = pattern((M + 5, N + 38), 13); pc[3:3 + M, 6:6 + N] = C0
    dpa, dpb, dpc = H.to_device(pa), H.to_device(pb), H.to_device(pc)
    dA, dB, dC = dpa[:, 2:2 + A.shape[1]], dpb[:, 4:4 + B.shape[1]], dpc[3:3 + M, 6:6 + N]
    lds = (dA.stride(0), dB.stride(0), dC.stride(0))
    assert len(set(lds)) == 3 and lds[0] > A.shape[1] and lds[1] > B.shape[1] and lds[2] > N
    assert all(t.data_ptr() % 16 == 0 for t in (dA, dB, dC))
    with options(H, opts):
        H.gemm(akm, bnm, lower, M, N, K, -0.75, dA, dB, 1.25, dC)
        H.sync()
    want = pc.copy()
    want[3:3 + M, 6:6 + N] = expect(exact_want(M, N, K, -0.75, 1.25), C0, ref.tile_mask(M, N, lower))
    assert same_bits(H.to_host(dpc), want)
    assert same_bits(H.to_host(dpa), pa) and same_bits(H.to_host(dpb), pb)


# ---- exact family: any non-zero `lower` is the lower-tile form -----------------------------------------------------------------------------
@pytest.mark.parametrize("akm,bnm,K,opts", [pytest.param(a, b, K, o, id=f"{route(a, b, 1, 384, 384, K, o)[0]}-K{K}") for a, b, K, o in
                                            [(0, 0, 176, BIG), (1, 1, 176, BIG), (0, 0, 176, {}), (0, 1, 176, {}), (0, 0, 128, {}),
                                             (0, 0, 1024, {}), (1, 1, 1024, {})]])
def test_exact_lower_is_normalised(H, akm, bnm, K, opts):
    """lower = 2 and lower = 5 give lower = 1's bits and leave the same tiles alone, on the 128-tile, 64-tile, one-stage and split-K
    paths.  (Inside, lower == 2 is the row-sharded predicate of fvgp_hip_syrk_rowshard, which builds its own descriptor; passed
    through unchanged it computed tile column 0 only, and lower >= 3 computed every tile.)"""
    M = N = 384
    opA, opB, C0 = exact(M, N, K)
    want = expect(exact_want(M, N, K, -0.75, 1.25), C0, ref.tile_mask(M, N, 1))
    for lower in (1, 2, 5):
        got = run(H, akm, bnm, lower, M, N, K, -0.75, 1.25, opA, opB, C0, opts)
        assert np.array_equal(got, want), f"lower = {lower}"


# ---- exact family: K == 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("akm,bnm,opts", [pytest.param(a, b, o, id=route(a, b, 0, 256, 384, 0, o)[0]) for a, b, o in
                                          [(a, b, BIG) for a, b in LAYOUTS] + [(0, 0, {}), (0, 1, {})]])
def test_exact_k_zero_is_beta_c(H, akm, bnm, opts, lower):
    """K == 0 (BLAS semantics: C = beta C on the computed tiles).  Both kernels guard their prologue loads by nk > 0 and never enter
    the K loop (gemm_f64_kernel: `if (nk > 0)` around the first fetch, the LDS-DMA loop fetches only under `more`;
    gemm_f64_small_kernel likewise), so A and B are never read -- they are real allocations all the same.  beta = 0 over NaN
    gives zeros."""
    M, N = (384, 384) if lower else (256, 384)
    _, _, C0 = exact(M, N, 16)
    mask = ref.tile_mask(M, N, lower)
    dA, dB = H.to_device(pattern((384, 16), 1)), H.to_device(pattern((384, 16), 2))
    with options(H, opts):
        dC = H.to_device(C0)
        H.gemm(akm, bnm, lower, M, N, 0, -0.75, dA, dB, 1.25, dC)
        dZ = H.to_device(np.full((M, N), np.nan))
        H.gemm(akm, bnm, lower, M, N, 0, -0.75, dA, dB, 0.0, dZ)
        H.sync()
    assert np.array_equal(H.to_host(dC), expect(1.25 * C0, C0, mask))
    z = H.to_host(dZ)
    assert np.all(z[mask] == 0.0) and np.all(np.isnan(z[~mask]))


# ---- the leading-dimension limit ----------------------------------------------------------------------------------------------------------------
def raw_gemm(H, akm, bnm, lower, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc):
    """the status code of the entry itself (Handle.gemm raises on a non-zero one); A, B, C are addresses or None"""
    from fvgp_amd import _lib
    return _lib.lib().fvgp_hip_gemm(H._h, akm, bnm, lower, M, N, K, float(alpha), A, lda, B, ldb, float(beta), C, ldc)


def test_leading_dimension_limit(H):
    """lda = ldb = 2^21 - 2 is accepted and 2^21 returns -9.  A tile's 128 rows are addressed by 32-bit byte offsets from its first
    row in the LDS-DMA loop of layout (0,0): the largest is (127 (2^21 - 2) + 14) 8 = 2 130 704 512, plus the K position (K - 16) 8
    = 128 and the 16 bytes fetched, below 2^31; gemm_f64_small_kernel and the 128-tile kernel's first fetch add (m0 + row) * lda
    to a 64-bit pointer in 64-bit arithmetic, so nothing of theirs can wrap.  A and B are the columns 0 .. 31 and 32 .. 63 of the
    same 128 rows of one 2 GB buffer of which only those columns are ever written or read."""
    import torch
    LD_OK, LD_BAD = (1 << 21) - 2, 1 << 21
    assert (127 * LD_OK + 14) * 8 + (32 - 16) * 8 + 16 < 2 ** 31 <= 128 * LD_BAD * 8
    M = N = 128; K = 32
    opA, opB, C0 = exact(M, N, K)
    A, B = ref.store(opA, opB, 0, 0)
    want = exact_want(M, N, K, -0.75, 1.25)
    big = torch.empty(128 * LD_BAD, dtype=torch.float64, device="cuda")
    try:
        dA = torch.as_strided(big, (M, K), (LD_OK, 1), 0)
        dB = torch.as_strided(big, (N, K), (LD_OK, 1), K)
        dA.copy_(H.to_device(A)); dB.copy_(H.to_device(B))
        for opts, kern in ((BIG, "tile128<0,0>/formula"), ({}, "small<64,64,0>")):
            assert route(0, 0, 0, M, N, K, opts)[0] == kern
            dC = H.to_device(C0)
            with options(H, opts):
                H.gemm(0, 0, 0, M, N, K, -0.75, dA, dB, 1.25, dC)
                H.sync()
            assert np.array_equal(H.to_host(dC), want), kern
        dC = H.to_device(C0)
        p = big.data_ptr()
        assert raw_gemm(H, 0, 0, 0, M, N, K, -0.75, p, LD_BAD, p + 8 * K, LD_OK, 1.25, dC.data_ptr(), N) == -9
        assert raw_gemm(H, 0, 0, 0, M, N, K, -0.75, p, LD_OK, p + 8 * K, LD_BAD, 1.25, dC.data_ptr(), N) == -9
        H.sync()
        assert np.array_equal(H.to_host(dC), C0)
    finally:
        del big
        torch.cuda.empty_cache()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing(H):
    """-5 for M or N not a multiple of 128 or K not of 16, -9 for an odd lda or ldb or an A or B 8 bytes off 16-byte alignment,
    -9 / -11 / -14 for a null A / B / C, whatever kernel the shape would have reached (unsplit and split K); C keeps its bits"""
    for K in (176, 1040):
        M, N = 256, 384
        opA, opB, C0 = exact(M, N, K)
        dA = H.to_device(np.concatenate([opA, opA[:, :2]], axis=1))          # (M, K + 2): room for a shifted and an odd-pitched view
        dB = H.to_device(np.concatenate([opB.T, opB.T[:, :2]], axis=1))
        dC = H.to_device(C0)
        a, b, c, ld = dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), K + 2
        assert a % 16 == 0 and b % 16 == 0

        def rc(M=M, N=N, K=K, A=a, lda=ld, B=b, ldb=ld, C=c):
            return raw_gemm(H, 0, 0, 0, M, N, K, -0.75, A, lda, B, ldb, 1.25, C, N)

        assert rc(M=M - 1) == -5 and rc(M=M - 64) == -5 and rc(N=N - 8) == -5 and rc(N=N - 64) == -5
        assert rc(K=K - 1) == -5 and rc(K=K - 8) == -5
        assert rc(lda=ld - 1) == -9 and rc(ldb=ld - 1) == -9
        assert rc(A=a + 8) == -9 and rc(B=b + 8) == -9
        assert rc(A=None) == -9 and rc(B=None) == -11 and rc(C=None) == -14
        H.sync()
        assert np.array_equal(H.to_host(dC), C0)
        assert rc() == 0                                                     # the same call with nothing wrong runs
        H.sync()
        assert np.array_equal(H.to_host(dC), exact_want(M, N, K, -0.75, 1.25))


def test_handle_gemm_raises_with_the_status(H):
    from fvgp_amd._lib import HipExtensionError
    t = H.zeros(128, 128)
    with pytest.raises(HipExtensionError, match=re.escape("status -5")):
        H.gemm(0, 0, 0, 128, 128, 8, 1.0, t, t, 0.0, H.zeros(128, 128))


# ---- rounding family: one case per kernel ----------------------------------------------------------------------------------------------------
ROUNDING = [(akm, bnm, 528, {}) for akm, bnm in LAYOUTS] + \
           [(0, 0, 176, {}), (0, 1, 176, {}), (0, 0, 128, {}), (0, 0, 1040, {}), (1, 1, 1040, {})]


@pytest.mark.parametrize("akm,bnm,K,opts", [pytest.param(a, b, K, o, id=f"{route(a, b, 0, 256, 256, K, o)[0]}-K{K}") for a, b, K, o in ROUNDING])
def test_rounding_componentwise_bound(H, akm, bnm, K, opts):
    """256 x 256, alpha / beta = -0.75 / 1.25, full-mantissa operands with rows and columns scaled over 2^-20 .. 2^20, against
    longdouble: |got - ref| <= (K + S + 2) u (|alpha| |opA| |opB| + |beta| |C0|) in every entry.  K = 528 is past the small-tile
    rule's 512 (the 128-tile kernel, four layouts); K = 176 and 128 with A (M,K) and 4 tiles take small<64,64,0>, small<64,64,1> and
    k128<64>; K = 1040 with 4 tiles splits into S = 4 slices (the facade's layout (1,1), and (0,0))."""
    if not ref.extended_precision():
        pytest.skip("numpy.longdouble is not the 80-bit extended format here: the reference would judge nothing")
    M = N = 256
    kern, S = route(akm, bnm, 0, M, N, K, opts)
    want_kern = {528: f"tile128<{akm},{bnm}>/formula", 176: f"small<64,64,{bnm}>", 128: "k128<64>", 1040: f"split4+tile128<{akm},{bnm}>"}[K]
    assert kern == want_kern and S == (4 if K == 1040 else 1)
    opA, opB, C0 = ref.rounding_case(M, N, K, seed=31 * K + 2 * akm + bnm)
    got = run(H, akm, bnm, 0, M, N, K, -0.75, 1.25, opA, opB, C0, opts)
    want, mag = ref.rounding_ref(opA, opB, C0, -0.75, 1.25)
    f = ref.fraction(got, want, mag, K, S)
    WORST[kern] = max(WORST.get(kern, 0.0), f)
    print(f"gemm rounding: {kern} K={K} S={S}: worst |err| / bound = {f:.4f}")
    assert f <= 1.0, (kern, f)
    assert f > 0.0, "a double-precision product of full-mantissa operands that equals the longdouble one in every entry is not one"


def test_rounding_report():
    """the observed fractions of the bound per kernel variant (observations, not the assertion), printed for the record"""
    for kern in sorted(WORST):
        print(f"gemm rounding, worst fraction of the bound: {kern}: {WORST[kern]:.4f}")
    assert all(f <= 1.0 for f in WORST.values())
