// Host side of the C ABI: triangular solves with a factor (vector sweeps, block substitution on GEMMs, the transposed sweep of the
// posterior) and POTRI.
#include "common.h"

// B (np x ldb), nrhs columns: in-place solve, vector path (nrhs <= 8)
int potrs_vec(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb, bool backward) {
    const int64_t np = pad128(n);
    int rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    rc = ensure_scratch(h, np); if (rc) return rc;
    const int c = (int)nrhs;
    double *Y = h->vec;
    if (h->fwd_sweep && c == 1) {               // one launch for the whole sweep (B is not touched)
        rc = launch_fwd_sweep(h, L, ldl, np, h->linv, B, ldb, Y); if (rc) return rc;
    } else
    for (int64_t k0 = 0; k0 < np; k0 += TILE) {
        rc = launch_fwd_step(h, L, ldl, np, k0, h->linv + (k0 / TILE) * LEAF_DOUBLES, B, ldb, Y, c);
        if (rc) return rc;
    }
    if (!backward) {
        // forward result lives in Y (np x rhs_width(c)); copy back to B
        return launch_copy_cols(h, Y, rhs_width(c), B, ldb, np, c, np, c);
    }
    if (h->bwd_sweep && c == 1) return launch_bwd_sweep(h, L, ldl, np, h->linv, Y, B, ldb, c);        // one launch for the whole sweep
    for (int64_t k0 = np - TILE; k0 >= 0; k0 -= TILE) {
        rc = launch_bwd_step(h, L, ldl, np, k0, h->linv + (k0 / TILE) * LEAF_DOUBLES, Y, B, ldb, c);
        if (rc) return rc;
    }
    return 0;
}

// B (np x ldb), nrhs (multiple of 128) columns: forward block substitution on MFMA GEMMs, two block sizes like
// the factorisation: 128-row steps inside an outer block of `outer_block` rows (updates confined to that block,
// K = 128), then ONE update of everything below with K = outer_block -- the read-modify-write passes over B
// drop by outer_block/128.
static int trsm_fwd_gemm(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t ncols, int64_t ldb) {
    const int64_t np = pad128(n), NB = h->outer_block;
    int rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    for (int64_t J0 = 0; J0 < np; J0 += NB) {
        const int64_t Jend = (J0 + NB < np) ? J0 + NB : np;
        for (int64_t k0 = J0; k0 < Jend; k0 += TILE) {
            double *Bk = B + k0 * ldb;
            // X_k = inv(L_kk) B_k
            rc = launch_gemm(h, gemm_desc(0, 1, TILE, ncols, TILE, 1.0, h->linv + (k0 / TILE) * LEAF_DOUBLES, TILE, Bk, ldb, 0.0, Bk, ldb)); if (rc) return rc;
            const int64_t r0 = k0 + TILE, R = Jend - r0;
            if (R <= 0) continue;
            // rest of the outer block: B[r0:Jend] -= L[r0:Jend, k] X_k
            rc = launch_gemm(h, gemm_desc(0, 1, R, ncols, TILE, -1.0, L + r0 * ldl + k0, ldl, Bk, ldb, 1.0, B + r0 * ldb, ldb)); if (rc) return rc;
        }
        if (np > Jend) {   // everything below: B[Jend:] -= L[Jend:, J0:Jend] X[J0:Jend]
            rc = launch_gemm(h, gemm_desc(0, 1, np - Jend, ncols, Jend - J0, -1.0, L + Jend * ldl + J0, ldl, B + J0 * ldb, ldb, 1.0, B + Jend * ldb, ldb));
            if (rc) return rc;
        }
    }
    return 0;
}

// The same substitution on the TRANSPOSED right-hand sides: BT (rows x np, row-major, rows a multiple of 128) holds B^T and
// leaves (L^-1 B)^T.  Every product is then the (M,K) x (N,K) layout of the factorisation's own panel TRSM and trailing
// update -- X_k^T = B_k^T inv(L_kk)^T in place, BT[:, block] -= X^T L[block, k]^T -- i.e. the kernels with the 16-byte
// fragment reads, and what follows (V^T V, row sums) reads contiguous rows.
// The block itself is then ONE product with the inverse of its NB x NB diagonal block (ensure_winv) instead of NB / 128
// steps of two latency-bound launches each.  NB = 2048 up to 1024 rows, where the sweep is a chain of dependent launches and
// half as many are worth the larger block products (N = 20k: P = 8 .. 64 2.53 -> 1.68 ms, 600 5.8 -> 5.4, 1000 8.4 -> 8.1);
// 1024 beyond (flop-bound: P = 2000 / 4000 +0.7 % with 2048).
// LEFT-looking over the outer blocks: block J first receives everything to its left in one product,
//     BT[:, J] -= BT[:, 0:J0] L[J, 0:J0]^T          (rows/128 x NB/128 output tiles, K = J0),
// with K split over enough workgroups to fill the chip (deterministic two-pass reduction).  A right-looking sweep has
// (rows/128) x (remaining blocks) tiles of K = NB per step instead: 1192, 1128, .. tiles on 512 slots lose a quarter of
// the time to partly filled rounds (measured at N = 20k, P = 1000: 7.3 ms for 3.9e11 flops); here every launch is one round.
// `slots`: the workgroups one launch should bring (512 = the whole chip; 256 when two halves of the rows run side by side on two
// streams, trsm_fwd_gemm_t below); scratch: trsm_fwd_scratch(rows, slots) doubles.
// workgroups per output tile of a launch with fewer tiles than slots (split K): s slices take ceil(tiles s / slots) / s rounds of the
// unsplit tile's time; the floor slots / tiles leaves up to a third of the chip idle (192 tiles: 384 of 512), a larger s in two
// rounds can beat it (192 tiles x 5 = 960: 0.4 instead of 0.5).  A small charge per slice for the partial sums' traffic.
static int64_t fill_split(int64_t tiles, int64_t slots) {
    if (tiles >= slots) return 1;
    int64_t best = slots / tiles;
    double cost = 1.0 / (double)best + 0.012 * (double)best;
    for (int64_t sp = best + 1; sp <= 8; ++sp) {
        const double c = (double)((tiles * sp + slots - 1) / slots) / (double)sp + 0.012 * (double)sp;
        if (c < cost - 1e-9) { cost = c; best = sp; }
    }
    return best;
}

static int64_t trsm_fwd_scratch(int64_t rows, int64_t slots, int64_t NB) {
    const int64_t tiles = (rows / TILE) * (NB / TILE);
    const int64_t want = fill_split(tiles, slots);
    return rows * NB + want * rows * NB;
}

// one outer block [J0, J0 + NB) of the sweep for `rows` rows of BT
static int trsm_fwd_gemm_t_block(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *BT, int64_t rows, int64_t ldbt,
                                 int64_t slots, double *scratch, int64_t J0, int64_t NB, int64_t WB) {
    const int64_t np = pad128(n);
    const bool winv = h->block_inverses != 0;
    int rc = 0;
    // scratch: tmp (rows x NB: block J with everything to its left applied) and the split-K partials behind it
    const int64_t tiles = (rows / TILE) * (NB / TILE);
    const int64_t want = fill_split(tiles, slots);                       // workgroups per output tile that fill the launch's share of the chip
    const int64_t tmp_d = rows * NB;
    double *tmp = scratch, *ws = scratch + tmp_d;
    {
        const int64_t Jend = (J0 + NB < np) ? J0 + NB : np, w = Jend - J0;
        bool in_tmp = false;
        if (J0 > 0) {
            // BT[:, J] -= BT[:, 0:J0] L[J, 0:J0]^T
            GemmDesc u = gemm_desc(0, 0, rows, w, J0, -1.0, BT, ldbt, L + J0 * ldl, ldl, 1.0, BT + J0, ldbt);
            int64_t split = want;
            const int64_t max_split = J0 / 512 > 0 ? J0 / 512 : 1;          // at least 512 of K per workgroup
            if (split > max_split) split = max_split;
            if (split > 1) {
                u.split = (int)split; u.split_ws = ws;
                if (winv) { u.split_out = tmp; u.split_ldo = w; in_tmp = true; }   // the reduction drops the block where the next product reads it
            }
            rc = launch_gemm(h, u); if (rc) return rc;
        }
        if (winv) {
            if (!in_tmp) { rc = launch_copy_cols(h, BT + J0, ldbt, tmp, w, rows, w, rows, w); if (rc) return rc; }
            // X_J^T = B_J^T inv(L_JJ)^T   (NB < WB: a diagonal sub-block of the WB-wide inverses)
            GemmDesc d = gemm_desc(0, 0, rows, w, w, 1.0, tmp, w, h->winv + J0 * WB + J0 % WB, WB, 0.0, BT + J0, ldbt);
            int64_t split = want;
            if (split > w / TILE) split = w / TILE;
            if (split > 1) {
                d.split = (int)split; d.split_ws = ws;
                // inv(L_JJ) is lower triangular: tile column tj of the product stops at K = 128 (tj + 1), 44 % of the flops never
                // issued (the sums are the same bit for bit: the terms left out are products with explicit zeros).  Slices of whole
                // 128-blocks only.  C2 posterior covariance 7.8 -> 7.46 ms.
                d.split_tri = ((w / 16 + split - 1) / split * 16) % 128 == 0;
            }
            return launch_gemm(h, d);
        }
        for (int64_t k0 = J0; k0 < Jend; k0 += TILE) {
            // X_k^T = B_k^T inv(L_kk)^T, in place (a workgroup owns whole rows)
            rc = launch_gemm(h, gemm_desc(0, 0, rows, TILE, TILE, 1.0, BT + k0, ldbt, h->linv + (k0 / TILE) * LEAF_DOUBLES, TILE, 0.0, BT + k0, ldbt));
            if (rc) return rc;
            const int64_t r0 = k0 + TILE, R = Jend - r0;
            if (R <= 0) continue;
            // rest of the outer block: BT[:, r0:Jend] -= X_k^T L[r0:Jend, k]^T
            rc = launch_gemm(h, gemm_desc(0, 0, rows, R, TILE, -1.0, BT + k0, ldbt, L + r0 * ldl + k0, ldl, 1.0, BT + r0, ldbt)); if (rc) return rc;
        }
    }
    return 0;
}

// With 512 or more rows (posterior covariance at P >= 512 points) the rows are cut in two halves that run the same sweep side
// by side on the two streams of the handle, each with launches of 256 workgroups: a step of the sweep is three dependent
// launches with two reductions between them (~66 us of fixed cost per block, 10 blocks at N = 20k), and the other half's
// product fills the chip while they run.
int trsm_fwd_gemm_t(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *BT, int64_t rows, int64_t ldbt, int64_t block) {
    const bool winv = h->block_inverses != 0;
    // up to 1024 points the sweep is a chain of dependent launches: 2048-wide blocks, half as many (`posterior_block`).  The block
    // width is a function of the call alone (number of rows, the option, `block` of the caller): the same call gives the same bits
    // whether it is the first on a factor or the tenth.  The last doubling level of the inverted blocks costs 1.3 ms at N = 20k, once
    // per factor: a posterior pays it on its first call (the sweeps that follow gain 0.4 ms each at P = 1000, 0.85 at P <= 64);
    // fvgp_hip_trsm_lower, whose callers solve once per factor (the new rows of an append), asks for 1024.
    const int64_t WB = block ? block : (rows <= 1024 ? h->posterior_block : 1024);
    const int64_t NB = WB;
    int rc = winv ? ensure_winv(h, L, n, ldl, WB, NB) : ensure_linv(h, L, n, ldl); if (rc) return rc;
    const bool halves = h->posterior_halves && winv && rows >= 512 && rows <= 1024 && rows % 256 == 0;    // (2048 rows: +3 %)
    const int64_t np = pad128(n);
    if (!halves) {
        rc = ensure_scratch(h, (trsm_fwd_scratch(rows, 512, NB) + 7) / 8); if (rc) return rc;
        for (int64_t J0 = 0; J0 < np && !rc; J0 += NB) rc = trsm_fwd_gemm_t_block(h, L, n, ldl, BT, rows, ldbt, 512, h->vec, J0, NB, WB);
        return rc;
    }
    const int64_t r2 = rows / 2, sc = trsm_fwd_scratch(r2, 256, NB);
    rc = ensure_scratch(h, (2 * sc + 7) / 8); if (rc) return rc;
    rc = fvgp_ensure_side(h); if (rc) return rc;
    hipStream_t mainS = h->stream, sideS = h->side;
    HIPCHK(hipEventRecord(h->ev_cols, mainS));
    HIPCHK(hipStreamWaitEvent(sideS, h->ev_cols, 0));
    for (int64_t J0 = 0; J0 < np && !rc; J0 += NB) {          // the two halves are enqueued block by block (a launch costs the host ~17 us)
        rc = trsm_fwd_gemm_t_block(h, L, n, ldl, BT, r2, ldbt, 256, h->vec, J0, NB, WB);
        if (rc) break;
        h->stream = sideS;
        rc = trsm_fwd_gemm_t_block(h, L, n, ldl, BT + r2 * ldbt, r2, ldbt, 256, h->vec + sc, J0, NB, WB);
        h->stream = mainS;
    }
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev_panel, sideS));
    HIPCHK(hipStreamWaitEvent(mainS, h->ev_panel, 0));
    return 0;
}

// backward half, same two block sizes, from the last outer block to the first
static int trsm_bwd_gemm(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t ncols, int64_t ldb) {
    const int64_t np = pad128(n), NB = h->outer_block;
    int rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    const int64_t npan = (np + NB - 1) / NB;
    for (int64_t J = npan - 1; J >= 0; --J) {
        const int64_t J0 = J * NB, Jend = (J0 + NB < np) ? J0 + NB : np;
        for (int64_t k0 = Jend - TILE; k0 >= J0; k0 -= TILE) {
            double *Bk = B + k0 * ldb;
            // X_k = inv(L_kk)^T Y_k
            rc = launch_gemm(h, gemm_desc(1, 1, TILE, ncols, TILE, 1.0, h->linv + (k0 / TILE) * LEAF_DOUBLES, TILE, Bk, ldb, 0.0, Bk, ldb)); if (rc) return rc;
            if (k0 == J0) continue;
            // rest of the outer block: Y[J0:k0] -= L[k, J0:k0]^T X_k
            rc = launch_gemm(h, gemm_desc(1, 1, k0 - J0, ncols, TILE, -1.0, L + k0 * ldl + J0, ldl, Bk, ldb, 1.0, B + J0 * ldb, ldb)); if (rc) return rc;
        }
        if (J0 > 0) {   // everything above: Y[0:J0] -= L[J0:Jend, 0:J0]^T X[J0:Jend]
            rc = launch_gemm(h, gemm_desc(1, 1, J0, ncols, Jend - J0, -1.0, L + J0 * ldl, ldl, B + J0 * ldb, ldb, 1.0, B, ldb)); if (rc) return rc;
        }
    }
    return 0;
}

extern "C" {

int fvgp_hip_potrs(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!B) return -5;
    if (nrhs <= 0) return -6;
    if (ldb < nrhs) return -7;
    // refused before anything is written: the padding rows of B keep their bits
    if (nrhs > FVGP_MAX_RHS_VEC && (nrhs % 128 || (ldb & 1) || ((uintptr_t)B & 15))) { fvgp_set_error("potrs with nrhs > 8 needs nrhs % 128 == 0, even ldb, 16-byte aligned B"); return -6; }
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n);
    if (np > n) { rc = launch_copy_cols(h, B, ldb, B + n * ldb, ldb, 0, 0, np - n, nrhs); if (rc) return rc; }
    if (nrhs <= FVGP_MAX_RHS_VEC) return potrs_vec(h, L, n, ldl, B, nrhs, ldb, true);
    rc = trsm_fwd_gemm(h, L, n, ldl, B, nrhs, ldb);
    if (rc) return rc;
    return trsm_bwd_gemm(h, L, n, ldl, B, nrhs, ldb);
}

// potrs with the launch shape of every product fixed (the 128-tile kernel): a column's bits do not depend on nrhs
int fvgp_hip_potrs_cols(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!B) return -5;
    if (nrhs <= 0 || nrhs % 128 || (ldb & 1) || ((uintptr_t)B & 15)) { fvgp_set_error("potrs_cols needs nrhs % 128 == 0, even ldb, 16-byte aligned B"); return -6; }
    if (ldb < nrhs) return -7;
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n);
    if (np > n) { rc = launch_copy_cols(h, B, ldb, B + n * ldb, ldb, 0, 0, np - n, nrhs); if (rc) return rc; }
    const int64_t keep = h->small_tile_max;
    h->small_tile_max = -1;
    rc = trsm_fwd_gemm(h, L, n, ldl, B, nrhs, ldb);
    if (!rc) rc = trsm_bwd_gemm(h, L, n, ldl, B, nrhs, ldb);
    h->small_tile_max = keep;
    return rc;
}

int fvgp_hip_trsm_lower(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!B) return -5;
    if (nrhs <= 0) return -6;
    if (ldb < nrhs) return -7;
    // refused before anything is written: the padding rows of B keep their bits
    if (nrhs > FVGP_MAX_RHS_VEC && (nrhs % 128 || (ldb & 1) || ((uintptr_t)B & 15))) { fvgp_set_error("trsm with nrhs > 8 needs nrhs % 128 == 0, even ldb, 16-byte aligned B"); return -6; }
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n);
    if (np > n) { rc = launch_copy_cols(h, B, ldb, B + n * ldb, ldb, 0, 0, np - n, nrhs); if (rc) return rc; }
    if (nrhs <= FVGP_MAX_RHS_VEC) return potrs_vec(h, L, n, ldl, B, nrhs, ldb, false);
    if (h->block_inverses && nrhs <= 1024 && np >= 2048) {
        // few columns against a long factor (the new rows of an append, gp_lin_alg.py:1310-1477; the callables' posterior): the
        // posterior's block sweep on the TRANSPOSED right-hand sides (N / 1024 steps with inverted diagonal blocks instead of
        // N / 128 steps of two latency-bound launches: append of 4 points at N = 20k 10.0 -> 7 ms), two transposes around it
        const size_t need = (size_t)nrhs * np;
        if (need > h->tr_ws_cap) {
            if (h->tr_ws) HIPCHK(hipFree(h->tr_ws));
            h->tr_ws = nullptr; h->tr_ws_cap = 0;
            HIPCHK(hipMalloc((void **)&h->tr_ws, need * sizeof(double)));
            h->tr_ws_cap = need;
        }
        rc = launch_transpose(h, B, ldb, h->tr_ws, np, np, nrhs); if (rc) return rc;
        rc = trsm_fwd_gemm_t(h, L, n, ldl, h->tr_ws, nrhs, np, 1024); if (rc) return rc;
        return launch_transpose(h, h->tr_ws, np, B, ldb, nrhs, np);
    }
    return trsm_fwd_gemm(h, L, n, ldl, B, nrhs, ldb);
}

int fvgp_hip_trsm_lower_t(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *B, int64_t nrhs, int64_t ldb) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (!B) return -5;
    if (nrhs <= 0) return -6;
    if (ldb < nrhs) return -7;
    if (nrhs % 128 || (ldb & 1) || ((uintptr_t)B & 15)) { fvgp_set_error("trsm_lower_t needs nrhs % 128 == 0, even ldb, 16-byte aligned B"); return -6; }
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n);
    if (np > n) { rc = launch_copy_cols(h, B, ldb, B + n * ldb, ldb, 0, 0, np - n, nrhs); if (rc) return rc; }
    return trsm_bwd_gemm(h, L, n, ldl, B, nrhs, ldb);
}

int fvgp_hip_logdet(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, double *out_host) {
    if (!h) return -1;
    if (!L) return -2;
    if (n <= 0) return -3;
    if (ldl < n) return -4;
    if (!out_host) return -5;
    HIPCHK(hipSetDevice(h->device));
    int rc = launch_diag_logsum(h, L, n, ldl, h->red);
    if (rc) return rc;
    return fvgp_read_back(h, h->red, out_host, 1);
}

// POTRI on the factorisation's own product layout.  Every product of dtrtri and of W^T W is arranged as (M,K) x (N,K) --
// both operands k-minor, the layout of the trailing update and of its K loop (16-byte swizzled fragment reads, LDS-DMA
// staging, no vector-ALU work) -- by keeping transposes where the textbook schedule reads an operand k-major:
//   dtrtri, 1024-wide panels from the bottom-right corner, W_JJ from the doubled block inverses (ensure_winv):
//        X^T  = W_JJ^T L_2J^T            A = W_JJ^T (transposed copy of the block), B = L_2J          -> work[J, 2]
//        W_2J = -W_22 X                  A = W_22 (k <= row), B = X^T                                 -> over L_2J
//   W^T W = (W^T)(W^T)^T with W^T written into `work` (upper tiles, diagonal tiles transposed), the result straight into L.
// Against the round-2 schedule ((K,N) and (K,M) operands on the 8-byte fragment reads, 14 latency-bound launches per panel
// for W_JJ, ragged K in 438 launches): the same N^3 2/3 flops on the faster kernel in 3 launches per panel.
static int potri_kminor(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *work, int64_t ldw) {
    const int64_t np = pad128(n), WB = 1024;
    int rc = ensure_winv(h, L, n, ldl); if (rc) return rc;
    rc = ensure_scratch(h, (WB * WB + 7) / 8); if (rc) return rc;
    double *Ujj = h->vec;                                   // W_JJ^T of the panel at hand
    const int64_t npan = (np + WB - 1) / WB;
    for (int64_t J = npan - 1; J >= 0; --J) {
        const int64_t J0 = J * WB, Jend = (J0 + WB < np) ? J0 + WB : np, w = Jend - J0, R = np - Jend;
        const double *Wjj = h->winv + J0 * WB;
        if (R > 0) {
            rc = launch_transpose_lower_tiles(h, Wjj, WB, Ujj, WB, w); if (rc) return rc;
            double *XT = work + J0 * ldw + Jend;            // w x R, in the (free) upper part of work
            // X^T = W_JJ^T L_2J^T   (W_JJ^T upper: k >= row tile)
            rc = launch_gemm(h, gemm_desc(0, 0, w, R, w, 1.0, Ujj, WB, L + Jend * ldl + J0, ldl, 0.0, XT, ldw).k_begin(0, TILE, 0)); if (rc) return rc;
            // W_2J = -W_22 X   (W_22 lower: k <= row tile), over L_2J
            GemmDesc u = gemm_desc(0, 0, R, w, R, -1.0, L + Jend * ldl + Jend, ldl, XT, ldw, 0.0, L + Jend * ldl + J0, ldl).k_end(TILE, TILE, 0);
            u.rev_m = 1;    // K grows with the row tile: the long rows start first
            rc = launch_gemm(h, u); if (rc) return rc;
        }
        rc = launch_copy_lower_tiles(h, Wjj, WB, L + J0 * ldl + J0, ldl, w); if (rc) return rc;
    }
    rc = launch_transpose_lower_tiles(h, L, ldl, work, ldw, np); if (rc) return rc;
    // KV^-1 = W^T W = (W^T)(W^T)^T, lower tiles, k >= row tile
    rc = launch_gemm(h, gemm_desc(0, 0, np, np, np, 1.0, work, ldw, work, ldw, 0.0, L, ldl).lower_tiles().k_begin(0, TILE, 0)); if (rc) return rc;
    h->winv_ok = false; h->linv_L = nullptr;   // L is gone
    return 0;
}

int fvgp_hip_potri(fvgp_handle *h, double *L, int64_t n, int64_t ldl, double *work, int64_t ldw) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    rc = check_square(work, n, ldw, 5, 3, 6);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (h->potri_kminor) return potri_kminor(h, L, n, ldl, work, ldw);
    const int64_t np = pad128(n);
    const int64_t NB = h->outer_block;
    rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    // ---- W = inv(L), written over L panel by panel from the bottom-right corner (dtrtri, lower):
    //        W_JJ  = inv(L_JJ)                               (block rows of 128 from the leaf inverses)
    //        W_2J  = -W_22 * (L_2J * W_JJ)                   (two large GEMMs per panel)
    //      `work` holds W_JJ and the intermediate L_2J * W_JJ.
    const int64_t npan = (np + NB - 1) / NB;
    for (int64_t J = npan - 1; J >= 0; --J) {
        const int64_t J0 = J * NB, Jend = (J0 + NB < np) ? J0 + NB : np, w = Jend - J0;
        double *Wjj = work + J0 * ldw + J0;
        const double *Ljj = L + J0 * ldl + J0;
        for (int64_t i0 = 0; i0 < w; i0 += TILE) {
            const double *li = h->linv + ((J0 + i0) / TILE) * LEAF_DOUBLES;
            rc = launch_copy_cols(h, li, TILE, Wjj + i0 * ldw + i0, ldw, TILE, TILE, TILE, TILE); if (rc) return rc;
            if (i0 == 0) continue;
            double *Wi = Wjj + i0 * ldw;
            // T = L_JJ[i][0:i] * W_JJ[0:i][0:i]   (W lower-triangular: k starts at the column tile)
            rc = launch_gemm(h, gemm_desc(0, 1, TILE, i0, i0, 1.0, Ljj + i0 * ldl, ldl, Wjj, ldw, 0.0, Wi, ldw).k_begin(0, 0, TILE)); if (rc) return rc;
            // W_JJ[i][0:i] = -inv(L_ii) * T  (in place: each tile reads only its own columns)
            rc = launch_gemm(h, gemm_desc(0, 1, TILE, i0, TILE, -1.0, li, TILE, Wi, ldw, 0.0, Wi, ldw)); if (rc) return rc;
        }
        const int64_t R = np - Jend;
        if (R > 0) {
            double *L2J = L + Jend * ldl + J0, *T = work + Jend * ldw + J0;
            // T = L_2J * W_JJ -> work   (W_JJ lower: k >= column tile)
            rc = launch_gemm(h, gemm_desc(0, 1, R, w, w, 1.0, L2J, ldl, Wjj, ldw, 0.0, T, ldw).k_begin(0, 0, TILE)); if (rc) return rc;
            // W_2J = -W_22 * T -> over L_2J   (W_22 lower: k <= row tile)
            GemmDesc u = gemm_desc(0, 1, R, w, R, -1.0, L + Jend * ldl + Jend, ldl, T, ldw, 0.0, L2J, ldl).k_end(TILE, TILE, 0);
            u.rev_m = 1;    // K grows with the row tile: start the long rows first so the launch has no long tail
            rc = launch_gemm(h, u); if (rc) return rc;
        }
        // W_JJ over L_JJ (its 128-tiles above the block diagonal are never read)
        rc = launch_copy_lower_tiles(h, Wjj, ldw, L + J0 * ldl + J0, ldl, w); if (rc) return rc;
    }
    // ---- KV^-1 = W^T W, lower tiles, k >= row tile; into work, then back over L
    rc = launch_gemm(h, gemm_desc(1, 1, np, np, np, 1.0, L, ldl, L, ldl, 0.0, work, ldw).lower_tiles().k_begin(0, TILE, 0)); if (rc) return rc;
    rc = launch_copy_lower_tiles(h, work, ldw, L, ldl, np); if (rc) return rc;
    h->winv_ok = false; h->linv_L = nullptr;   // L is gone
    return 0;
}

}  // extern "C"
