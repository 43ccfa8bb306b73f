// Host side of the C ABI (include/fvgp_hip.h), first unit: the handle, its options and profile, the buffers a handle grows on demand
// (ensure_*) and the blocked Cholesky drivers with their entries.  The other entries: tri_solve.hip (solves, POTRI), evaluate.hip (fused
// single evaluations), batch_api.hip (batched evaluations), blas_api.hip (thin products, reductions, diagnostics).  No torch types.
#include "common.h"
#include "kernel_family.h"
#include <string.h>

// ---------------------------------------------------------------------------------------
static thread_local std::string g_err;
void fvgp_set_error(const std::string &s) { g_err = s; }
int fvgp_hip_fail(hipError_t e, const char *what, int line) {
    g_err = std::string("HIP error '") + hipGetErrorString(e) + "' at api line " + std::to_string(line) + ": " + what;
    return 1000 + (int)e;
}

extern "C" {

int fvgp_hip_version(void) { return 100; }
const char *fvgp_hip_last_error_string(void) { return g_err.c_str(); }
int64_t fvgp_hip_workspace_bytes(int64_t n, int64_t npred) {
    // what a handle allocates on the device for problems of n points (and npred prediction points):
    // inverted 128 x 128 diagonal blocks + per-leaf log-det partials + the solve / posterior scratch + reductions
    if (n <= 0 || npred < 0) return -1;
    const int64_t np = pad128(n), nblk = np / TILE, pp = pad128(npred);
    int64_t vec = np * 16 + pp * 16 > np * 8 ? np * 16 + pp * 16 : np * 8;      // posterior mean widening vs vector sweeps
    int64_t winv = 0;
    if (npred > 0) {
        // posterior: inverted diagonal blocks (np x WB; 2048 wide up to 1024 points, 1024 beyond), their doubling
        // scratch (np x WB/4), one block of the transposed right-hand sides + its split-K partials, split-K partials of S -= V^T V
        const int64_t WB = pp <= 1024 ? 2048 : 1024;
        winv = np * WB;
        const int64_t tiles = (pp / TILE) * (WB / TILE), want = tiles >= 512 ? 1 : 512 / tiles;
        const int64_t stiles = (pp / TILE) * (pp / TILE + 1) / 2, swant = stiles >= 512 ? 1 : 64 / ((stiles + 7) / 8);      // S -= V^T V: lower tiles
        const int64_t cand[3] = {np * (WB / 4) + 1024, (1 + want) * pp * WB + 64, swant * pp * pp + 64};
        for (int64_t c : cand) if (c > vec) vec = c;
    }
    // + the per-CU yield counters, the backward sweep's granules (16 bytes per row) and ticket, the resident panel kernel's flag words
    const int64_t round3 = (int64_t)CU_YIELD_KEYS * CU_YIELD_STRIDE * (int64_t)sizeof(int) + np * 16 + 2 * (int64_t)sizeof(int) + 80 * 16 * (int64_t)sizeof(unsigned long long);
    return (nblk * LEAF_DOUBLES + nblk * TILE + (npred > 0 ? vec : np * 8) + winv + RED_SLOTS) * (int64_t)sizeof(double) + (int64_t)sizeof(int) + round3;
}

int64_t fvgp_hip_padded_dim(int64_t n) { return pad128(n); }
int64_t fvgp_hip_loglik_dim(int64_t n, int ncol) {
    if (n <= 0 || ncol < 1) return -1;
    return (pad128(n) - n) >= ncol ? pad128(n) : pad128(n + ncol);
}

int fvgp_hip_create(fvgp_handle **out, int device, void *stream) {
    if (!out) return -1;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { fvgp_set_error("no such HIP device"); return -2; }
    HIPCHK(hipSetDevice(device));
    fvgp_handle *h = new fvgp_handle();
    h->device = device;
    h->stream = (hipStream_t)stream;
    HIPCHK(hipMalloc((void **)&h->red, RED_SLOTS * sizeof(double)));
    HIPCHK(hipMalloc((void **)&h->dinfo, 64));
    HIPCHK(hipMalloc((void **)&h->cu_yield, (size_t)CU_YIELD_KEYS * CU_YIELD_STRIDE * sizeof(int)));
    HIPCHK(hipMemset(h->cu_yield, 0, (size_t)CU_YIELD_KEYS * CU_YIELD_STRIDE * sizeof(int)));
    HIPCHK(hipHostMalloc((void **)&h->hpin, RED_SLOTS * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, device));
    *out = h;
    return 0;
}

int fvgp_hip_destroy(fvgp_handle *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);      // the look-ahead / chain stream may still read the buffers freed below
    for (auto e : h->ev) (void)hipEventDestroy(e);
    if (h->ev_panel) (void)hipEventDestroy(h->ev_panel);
    for (auto e : h->ev_stage) if (e) (void)hipEventDestroy(e);
    for (auto e : h->rs_ev) (void)hipEventDestroy(e);
    if (h->ev_cols) (void)hipEventDestroy(h->ev_cols);
    gemm_release_tables(h);
    (void)fvgp_hip_comm_destroy(h);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->linv) (void)hipFree(h->linv);
    if (h->winv) (void)hipFree(h->winv);
    if (h->logdet_parts) (void)hipFree(h->logdet_parts);
    if (h->red) (void)hipFree(h->red);
    if (h->dinfo) (void)hipFree(h->dinfo);
    if (h->cu_yield) (void)hipFree(h->cu_yield);
    if (h->tr_ws) (void)hipFree(h->tr_ws);
    if (h->sweep_gran) (void)hipFree(h->sweep_gran);
    if (h->sweep_ticket) (void)hipFree(h->sweep_ticket);
    if (h->chain_flags) (void)hipFree(h->chain_flags);
    if (h->chain_vhash) (void)hipFree(h->chain_vhash);
    if (h->vec) (void)hipFree(h->vec);
    if (h->hpin) (void)hipHostFree(h->hpin);
    if (h->bat_ws) (void)hipFree(h->bat_ws);
    delete h;
    return 0;
}

int fvgp_hip_stream_create(void **out_stream, int device, int high_priority, const uint32_t *cu_mask, int mask_words) {
    if (!out_stream) return -1;
    if (cu_mask && mask_words < 1) return -5;
    HIPCHK(hipSetDevice(device));
    hipStream_t s = nullptr;
    if (cu_mask) {
        HIPCHK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask_words, cu_mask));
    } else {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, high_priority ? hi : lo));
    }
    *out_stream = s;
    return 0;
}

int fvgp_hip_stream_destroy(void *stream) {
    if (!stream) return -1;
    HIPCHK(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int fvgp_hip_sync(fvgp_handle *h) {
    if (!h) return -1;
    HIPCHK(hipStreamSynchronize(h->stream));
    return fvgp_ipc_check(h);
}

int fvgp_hip_set_option(fvgp_handle *h, const char *key, int64_t value) {
    if (!h) return -1;
    if (!key) return -2;
    if (!strcmp(key, "outer_block")) {
        if (value < 128 || value % 128) { fvgp_set_error("outer_block must be a positive multiple of 128"); return -3; }
        h->outer_block = value;
        return 0;
    }
    if (!strcmp(key, "schedule")) {
        // THE schedule switch: one of the three factorisation schedules, each with the settings it was tuned with; every other
        // schedule key below is a measurement knob underneath one of them
        if (value == 0) { h->chain_wide = 1; h->lookahead_min = (int64_t)1 << 40; h->panel_chain = 1; h->lookahead = 1; }            // wide: 4096-wide panels, each alone on the chip
        else if (value == 1) { h->chain_wide = 0; h->lookahead_min = 4608; h->panel_chain = 1; h->lookahead = 1; }                  // lookahead: 2048/1024/512 panels, the next one under the update (the row-sharded driver's form)
        else if (value == 2) { h->chain_wide = 0; h->lookahead_min = 4608; h->panel_chain = 0; h->lookahead = 1; }                  // narrow: the same panels, three launches per 128 columns instead of the resident kernel
        else { fvgp_set_error("schedule: 0 = wide (default), 1 = lookahead, 2 = narrow"); return -3; }
        return 0;
    }
    if (!strcmp(key, "profile")) { h->profile = value ? 1 : 0; return 0; }
    if (!strcmp(key, "lookahead")) { h->lookahead = value ? 1 : 0; return 0; }
    if (!strcmp(key, "outer_block_big")) {
        if (value != 0 && (value < 128 || value % 128)) { fvgp_set_error("outer_block_big must be 0 or a multiple of 128"); return -3; }
        h->outer_block_big = value; return 0;
    }
    if (!strcmp(key, "big_threshold")) { h->big_threshold = value; return 0; }
    if (!strcmp(key, "tile_tables")) { h->tile_tables = value ? 1 : 0; return 0; }
    if (!strcmp(key, "chain_stamps")) { h->chain_stamps = reinterpret_cast<unsigned long long *>((uintptr_t)value); h->chain_seq = 0; return 0; }
    if (!strcmp(key, "leaf_stamps")) { h->leaf_stamps = reinterpret_cast<unsigned long *>((uintptr_t)value); return 0; }
    if (!strcmp(key, "small_tile_max")) { h->small_tile_max = value; return 0; }
    if (!strcmp(key, "small_tile_max_update")) { h->small_tile_max_update = value; return 0; }
    if (!strcmp(key, "inner_block")) {
        if (value != 0 && (value < 128 || value % 128)) { fvgp_set_error("inner_block must be 0 or a multiple of 128"); return -3; }
        h->inner_block = value; return 0;
    }
    if (!strcmp(key, "panel_recursive")) { h->panel_recursive = value ? 1 : 0; return 0; }
    if (!strcmp(key, "leaf_tiles")) { h->leaf_tiles = value ? 1 : 0; return 0; }
    if (!strcmp(key, "leaf_tiles_rows")) { h->leaf_tiles_rows = value; return 0; }
    if (!strcmp(key, "k128_kernels")) { h->k128_kernels = value ? 1 : 0; return 0; }
    if (!strcmp(key, "block_inverses")) { h->block_inverses = value ? 1 : 0; return 0; }
    if (!strcmp(key, "potri_kminor")) { h->potri_kminor = value ? 1 : 0; return 0; }
    if (!strcmp(key, "leaf_yield")) { h->leaf_yield = (int)value; return 0; }
    if (!strcmp(key, "chain_yield")) { h->chain_yield = (int)value; return 0; }
    if (!strcmp(key, "lookahead_min")) { h->lookahead_min = value; return 0; }
    if (!strcmp(key, "panel_chain")) { if (value < 0 || value > 3) return -3; h->panel_chain = (int)value; return 0; }
    if (!strcmp(key, "panel_chain_min")) { h->panel_chain_min = value; return 0; }
    if (!strcmp(key, "chain_wide")) { h->chain_wide = (int)value; return 0; }
    if (!strcmp(key, "chain_sleep_rows")) { h->chain_sleep_rows = (int)value; return 0; }
    if (!strcmp(key, "chain_ahead")) { if (value < 0 || value > 8) return -3; h->chain_ahead = (int)value; return 0; }
    if (!strcmp(key, "chain_single_rows")) { h->chain_single_rows = (int)value; return 0; }
    if (!strcmp(key, "wide_block") || !strcmp(key, "wide_block_big")) {
        if (value < TILE || value % TILE || value / TILE > FVGP_CHAIN_MAX_BLOCKS) { fvgp_set_error("wide_block: a multiple of 128, at most 4096"); return -2; }
        (key[10] ? h->wide_block_big : h->wide_block) = value; return 0;
    }
    if (!strcmp(key, "wide_threshold")) { h->wide_threshold = value; return 0; }
    if (!strcmp(key, "wide_inner")) { if (value % TILE) return -2; h->wide_inner = value; return 0; }
    if (!strcmp(key, "wide_inner_rows")) { h->wide_inner_rows = value; return 0; }
    if (!strcmp(key, "cols_split")) { h->cols_split = value ? 1 : 0; return 0; }
    if (!strcmp(key, "chain_verify")) { h->chain_verify = value ? 1 : 0; return 0; }
    if (!strcmp(key, "cols_split_rows")) { h->cols_split_rows = value; return 0; }
    if (!strcmp(key, "bwd_sweep")) { h->bwd_sweep = (int)value; return 0; }
    if (!strcmp(key, "fwd_sweep")) { h->fwd_sweep = (int)value; return 0; }
    if (!strcmp(key, "posterior_halves")) { h->posterior_halves = (int)value; return 0; }
    if (!strcmp(key, "posterior_block")) { if (value != 1024 && value != 2048) return -3; h->posterior_block = value; return 0; }
    if (!strcmp(key, "select_block")) {
        if (value < 64 || value % 64 || value > 65536) { fvgp_set_error("select_block: a multiple of 64, at most 65536"); return -3; }
        h->select_block = value; return 0;
    }
    if (!strcmp(key, "matvec_split")) {
        if (value < 0 || value > 65535) { fvgp_set_error("matvec_split: 0 (by the shape), 1 (never) or the number of chunk ranges, at most 65535"); return -3; }
        h->matvec_split = value; return 0;
    }
    if (!strcmp(key, "outer_block_small")) { if (value < 0 || value % TILE) return -3; h->outer_block_small = value; return 0; }
    if (!strcmp(key, "small_threshold")) { h->small_threshold = value; return 0; }
    fvgp_set_error(std::string("unknown option ") + key);
    return -2;
}

int fvgp_hip_invalidate_factor(fvgp_handle *h) {
    if (!h) return -1;
    h->winv_ok = false; h->linv_L = nullptr;
    return 0;
}

int fvgp_hip_chain_verify_counts(fvgp_handle *h, int64_t *out2_host) {
    if (!h) return -1;
    if (!out2_host) return -2;
    HIPCHK(hipSetDevice(h->device));
    unsigned long long w[2];
    const int rc = chain_verify_counts(h, w);
    out2_host[0] = (int64_t)w[0]; out2_host[1] = (int64_t)w[1];
    return rc;
}

int fvgp_hip_get_profile(fvgp_handle *h, double *out) {
    if (!h) return -1;
    if (!out) return -2;
    if (h->rs_used > 0) {
        // the row-sharded driver enqueues its trailing updates one ABI call at a time: their events are read here
        HIPCHK(hipStreamSynchronize(h->stream));
        h->prof_launches = (double)h->rs_flops.size(); h->prof_ms = 0; h->prof_flops = 0;
        for (size_t i = 0; i < h->rs_flops.size(); ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, h->rs_ev[2 * i], h->rs_ev[2 * i + 1]));
            h->prof_ms += ms; h->prof_flops += h->rs_flops[i];
        }
        h->rs_used = 0; h->rs_flops.clear();
    }
    out[0] = h->prof_launches; out[1] = h->prof_ms; out[2] = h->prof_flops; out[3] = h->prof_total_ms;
    out[4] = h->prof_kmat_ms; out[5] = h->prof_kmat_bytes; out[6] = h->prof_tail_ms; out[7] = h->prof_host_enqueue_ms;
    return 0;
}

int fvgp_hip_get_profile_ex(fvgp_handle *h, double *out16) {
    int rc = fvgp_hip_get_profile(h, out16); if (rc) return rc;
    for (int i = 8; i < 16; ++i) out16[i] = 0.0;
    out16[8] = h->prof_bytes;
    return 0;
}

}  // extern "C"

// the high-priority second stream (look-ahead panel chain) and the two events that order it against the main stream
int fvgp_ensure_side(fvgp_handle *h) {
    if (h->side) return 0;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi));
    HIPCHK(hipEventCreateWithFlags(&h->ev_panel, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_cols, hipEventDisableTiming));
    return 0;
}

// ---------------------------------------------------------------------------------------
static int ensure_blocks(fvgp_handle *h, int64_t nblk) {
    if ((size_t)nblk > h->linv_blocks) {
        if (h->linv) HIPCHK(hipFree(h->linv));
        h->linv = nullptr; h->linv_blocks = 0; h->winv_ok = false; h->linv_L = nullptr;
        HIPCHK(hipMalloc((void **)&h->linv, (size_t)nblk * LEAF_DOUBLES * sizeof(double)));
        h->linv_blocks = (size_t)nblk;
    }
    if ((size_t)nblk > h->logdet_cap) {
        if (h->logdet_parts) HIPCHK(hipFree(h->logdet_parts));
        h->logdet_parts = nullptr; h->logdet_cap = 0;
        HIPCHK(hipMalloc((void **)&h->logdet_parts, (size_t)nblk * TILE * sizeof(double)));
        h->logdet_cap = (size_t)nblk;
    }
    return 0;
}

int ensure_scratch(fvgp_handle *h, int64_t np) {
    size_t need = (size_t)np * 8;
    if (need > h->vec_cap) {
        if (h->vec) HIPCHK(hipFree(h->vec));
        h->vec = nullptr; h->vec_cap = 0;
        HIPCHK(hipMalloc((void **)&h->vec, need * sizeof(double)));
        h->vec_cap = need;
    }
    return 0;
}

// diagonal-block inverses for factor L: reuse those left by potrf, else recompute (batched)
int ensure_linv(fvgp_handle *h, const double *L, int64_t n, int64_t ldl) {
    const int64_t np = pad128(n), nblk = np / TILE;
    if (h->linv_L == L && h->linv_n == n && h->linv_ld == ldl && (size_t)nblk <= h->linv_blocks) return 0;
    int rc = ensure_blocks(h, nblk);
    if (rc) return rc;
    rc = launch_leaf_inverse_batched(h, L, ldl, nblk, h->linv);
    if (rc) return rc;
    h->winv_ok = false; h->linv_L = L; h->linv_n = n; h->linv_ld = ldl;
    return 0;
}

// inverses of the WB x WB diagonal blocks of L (WB = 1024: POTRI, posterior at more than 1024 points; 2048: posterior up to 1024
// points), from the 128-block inverses by doubling:
//     inv [[A, 0], [C, B]] = [[inv A, 0], [-inv(B) C inv(A), inv B]]      at block sizes 128 -> 256 -> 512 -> 1024 (-> 2048),
// every level two strided-batch GEMM launches over all full WB-blocks (T = C inv(A) into the handle scratch, then
// -inv(B) T into place) plus single launches for the pairs of a narrower last block.  O(N WB^2) flops, a few hundred
// microseconds; kept until the factor changes or the other width is asked for.
// `upto` <= WB: the doubling stops at upto x upto blocks (they sit on the diagonal of the WB-wide layout); a later call with a
// larger `upto` only adds the missing levels.
int ensure_winv(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, int64_t WB, int64_t upto) {
    if (upto <= 0 || upto > WB) upto = WB;
    int rc = ensure_linv(h, L, n, ldl); if (rc) return rc;
    if (h->winv_ok && h->winv_w == WB && h->winv_level >= upto) return 0;
    const bool extend = h->winv_ok && h->winv_w == WB;          // the lower levels are there
    h->winv_ok = false;
    const int64_t np = pad128(n), nblk = np / TILE;
    const size_t need = (size_t)np * WB;
    if (need > h->winv_cap) {
        if (h->winv) HIPCHK(hipFree(h->winv));
        h->winv = nullptr; h->winv_cap = 0;
        HIPCHK(hipMalloc((void **)&h->winv, need * sizeof(double)));
        h->winv_cap = need;
    }
    double *W = h->winv;
    if (!extend) { rc = launch_winv_seed(h, h->linv, nblk, W, WB); if (rc) return rc; }
    rc = ensure_scratch(h, np * (WB / 32) + 128); if (rc) return rc;   // T: at most np/2 x WB/2 doubles
    double *T = h->vec;
    const int64_t nfull = np / WB, t0 = nfull * WB, wt = np - t0;
    for (int64_t hs = extend ? h->winv_level : TILE; hs < upto; hs *= 2) {
        const int64_t ny = WB / (2 * hs);
        if (nfull > 0) {
            const int64_t pairL = 2 * hs * ldl + 2 * hs, pairW = 2 * hs * WB + 2 * hs, hh = hs * hs;      // from one pair (A, C, B) to the next
            // T[y, z] = C inv(A)
            rc = launch_gemm(h, gemm_desc(0, 1, hs, hs, hs, 1.0, L + hs * ldl, ldl, W, WB, 0.0, T, hs)
                                    .batched_y(ny, pairL, pairW, hh).batched(nfull, WB * ldl + WB, WB * WB, ny * hh)); if (rc) return rc;
            // W21[y, z] = -inv(B) T
            rc = launch_gemm(h, gemm_desc(0, 1, hs, hs, hs, -1.0, W + hs * WB + hs, WB, T, hs, 0.0, W + hs * WB, WB)
                                    .batched_y(ny, pairW, hh, pairW).batched(nfull, WB * WB, ny * hh, WB * WB)); if (rc) return rc;
        }
        double *Tt = T + nfull * ny * hs * hs;                           // the last, narrower block: its pairs one by one
        for (int64_t s = 0; s + hs < wt; s += 2 * hs) {
            const int64_t wb = (wt - s - hs < hs) ? wt - s - hs : hs;
            const double *C21 = L + (t0 + s + hs) * ldl + t0 + s;
            double *W11 = W + (t0 + s) * WB + s, *W21 = W + (t0 + s + hs) * WB + s;
            rc = launch_gemm(h, gemm_desc(0, 1, wb, hs, hs, 1.0, C21, ldl, W11, WB, 0.0, Tt, hs)); if (rc) return rc;                  // T = C inv(A)
            rc = launch_gemm(h, gemm_desc(0, 1, wb, hs, wb, -1.0, W21 + hs, WB, Tt, hs, 0.0, W21, WB)); if (rc) return rc;             // W21 = -inv(B) T
        }
    }
    h->winv_ok = true; h->winv_w = WB; h->winv_level = upto;
    return 0;
}

int check_square(const void *A, int64_t n, int64_t ld, int argA, int argn, int argld) {
    if (!A) return -argA;
    if (n <= 0) return -argn;
    if (ld < pad128(n) || (ld & 1)) { fvgp_set_error("leading dimension must be even and >= padded_dim(n)"); return -argld; }
    if ((uintptr_t)A & 15) { fvgp_set_error("matrix base must be 16-byte aligned"); return -argA; }
    return 0;
}

// the run of checks behind a known kernel id: the inputs' dimension, theta (on the host) and its length
int check_kernel_args(int kernel_id, int d, const double *theta, int ntheta, int arg_d, int arg_theta, int arg_ntheta) {
    if (d < 1 || d > FVGP_MAX_DIM) { fvgp_set_error("input dimension out of range"); return -arg_d; }
    if (!theta) return -arg_theta;
    if (ntheta < kernel_param_count(kernel_id, d)) { fvgp_set_error("too few hyperparameters for this kernel"); return -arg_ntheta; }
    return 0;
}

// ---------------------------------------------------------------------------------------
// one (sub-)panel of the blocked Cholesky, 128 columns at a time: leaf (potf2 + trtri in LDS) -> panel TRSM as a
// GEMM with inv(L_kk) -> update of the remaining columns of this (sub-)panel (K = 128)
static int panel_factor(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda, int64_t J0, int64_t Jend) {
    int rc;
    for (int64_t k0 = J0; k0 < Jend; k0 += TILE) {
        const int64_t kb = k0 / TILE;
        const int64_t nv = n - k0;
        const int64_t r0 = k0 + TILE, R = np - r0;
        // few rows below = the chain is what the factorisation waits for: the leaf then skips the triangular inverse of its
        // block (19 of 103 thousand cycles) and the TRSM substitutes with the 16 x 16 tile inverses; with many rows the
        // product with the full inverse is the cheaper TRSM and the leaf is hidden under the trailing update anyway
        const int tiles = (h->leaf_tiles && R <= h->leaf_tiles_rows) ? 1 : 0;
        rc = launch_leaf(h, A + k0 * lda + k0, lda, h->linv + kb * LEAF_DOUBLES, h->logdet_parts + kb * TILE, (int)k0, 1,
                         nv >= TILE ? TILE : (nv > 0 ? (int)nv : 0), tiles);
        if (rc) return rc;
        if (R <= 0) continue;
        // panel TRSM in place: A[r0:, k0:k0+128] <- A[r0:, k0:k0+128] * inv(L_kk)^T
        double *P = A + r0 * lda + k0;
        if (tiles) {        // by substitution with the inverses of the diagonal block's 16 x 16 tiles (all the leaf left)
            rc = launch_trsm_tiles(h, P, lda, R, A + k0 * lda + k0, lda, h->linv + kb * LEAF_DOUBLES);
        } else {
            rc = launch_gemm(h, gemm_desc(0, 0, R, TILE, TILE, 1.0, P, lda, h->linv + kb * LEAF_DOUBLES, TILE, 0.0, P, lda));
        }
        if (rc) return rc;
        // update of the rest of the outer panel: A[r0:, r0:Jend] -= P P[0:Jend-r0]^T (lower tiles)
        const int64_t W = Jend - r0;
        if (W > 0) {
            rc = launch_gemm(h, gemm_desc(0, 0, R, W, TILE, -1.0, P, lda, P, lda, 1.0, A + r0 * lda + r0, lda).lower_tiles());
            if (rc) return rc;
        }
    }
    return 0;
}

// trailing update with the factored panel [J0, Jend): block columns [c0, c1) of the trailing matrix
// (rows c0..np), lower tiles only:  A[c0:, c0:c1] -= L[c0:, J0:Jend] L[c0:c1, J0:Jend]^T
static int trailing_update(fvgp_handle *h, double *A, int64_t np, int64_t lda, int64_t J0, int64_t Jend, int64_t c0, int64_t c1, int role = 1,
                           bool *big_kernel = nullptr) {
    if (big_kernel) *big_kernel = false;
    if (c1 <= c0 || np <= c0) return 0;
    const double *Lc = A + c0 * lda + J0;
    GemmDesc s = gemm_desc(0, 0, np - c0, c1 - c0, Jend - J0, -1.0, Lc, lda, Lc, lda, 1.0, A + c0 * lda + c0, lda).lower_tiles().with_role(role);
    // the last update behind a wide panel may have a handful of tiles and K = 4096 (N = 4096 with its extra block row: ONE tile, 0.2 ms
    // on four compute units): split K so that the launch fills the chip once, partial tiles summed in a fixed order
    const int64_t tm = s.M / TILE, tn = s.N / TILE, tiles = tn * (tn + 1) / 2 + (tm - tn) * tn;
    if (role == 1 && h->chain_alone && h->chain_wide && tiles > 0 && tiles <= 64 && s.K >= 1024) {
        int64_t split = 256 / tiles;
        if (split > s.K / 512) split = s.K / 512;
        if (split > 1) {
            int rc = ensure_scratch(h, (split * s.M * s.N + 7) / 8); if (rc) return rc;
            s.split = (int)split; s.split_ws = h->vec;
            if (big_kernel) *big_kernel = true;
            return launch_gemm(h, s);
        }
    }
    if (big_kernel) *big_kernel = !gemm_takes_small_tiles(h, s);
    return launch_gemm(h, s);
}

// a panel wider than `inner_block` is factored in sub-panels of that width: 128-column steps inside a sub-panel,
// then one update of the remaining columns of the panel with K = inner_block -- a third block size between the
// leaf (128) and the trailing update (panel width), so that wide panels do not pay for their width in K = 128 work
// One 128-column step of the chain without the in-panel update: leaf, then the TRSM of every row below.
static int panel_step(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda, int64_t k0) {
    return panel_factor(h, A, n, np, lda, k0, k0 + TILE);
}

// Recursive panel: left half, ONE update of the right half's columns with K = width of the left half, right half.  Against
// the right-looking loop of panel_factor (after every 128 columns an update of ALL remaining columns of the panel with
// K = 128) the same flops make 2/3 of the read-modify-write passes over the panel's columns at the 512 level and run at
// K = 256 / 512 / 1024 where they can; the update right before a leaf only touches the columns that leaf needs.
static int panel_factor_recursive(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda, int64_t J0, int64_t Jend) {
    const int64_t blocks = (Jend - J0) / TILE;
    if (blocks <= 1) return panel_step(h, A, n, np, lda, J0);
    const int64_t mid = J0 + (blocks / 2) * TILE;
    int rc = panel_factor_recursive(h, A, n, np, lda, J0, mid); if (rc) return rc;
    rc = trailing_update(h, A, np, lda, J0, mid, mid, Jend, 0); if (rc) return rc;
    return panel_factor_recursive(h, A, n, np, lda, mid, Jend);
}

static int panel_factor_nested(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda, int64_t J0, int64_t Jend) {
    if (h->panel_recursive) return panel_factor_recursive(h, A, n, np, lda, J0, Jend);
    const int64_t inner = h->inner_block;
    if (inner <= 0 || Jend - J0 <= inner) return panel_factor(h, A, n, np, lda, J0, Jend);
    for (int64_t s0 = J0; s0 < Jend; s0 += inner) {
        const int64_t s1 = (s0 + inner < Jend) ? s0 + inner : Jend;
        int rc = panel_factor(h, A, n, np, lda, s0, s1); if (rc) return rc;
        if (s1 < Jend) { rc = trailing_update(h, A, np, lda, s0, s1, s1, Jend, 0); if (rc) return rc; }
    }
    return 0;
}

// one panel, every row from its first column down: the resident panel kernel (chain.hip) while enough rows remain for a
// trailing update to run beside it, else the three launches per 128 columns
static int panel_factor_any(fvgp_handle *h, double *A, int64_t n, int64_t np, int64_t lda, int64_t J0, int64_t Jend) {
    // (the resident kernel has flag words for 32 block columns: a wider panel -- `outer_block` above 4096 -- takes the nested chain)
    if (h->panel_chain && (np - J0 >= h->panel_chain_min || (h->chain_alone && h->chain_wide)) && (Jend - J0) / TILE <= FVGP_CHAIN_MAX_BLOCKS) {
        // a tall panel (alone on the chip): sub-panels of `wide_inner` columns by the resident kernel, the rest of the panel's columns
        // brought up to date by the trailing update's kernel with K = wide_inner in between -- three quarters of the panel's flops
        // move from the resident kernel's products (0.7 of the MFMA rate) to that kernel (0.92)
        const int64_t inner = h->wide_inner;
        if (h->chain_alone && inner > 0 && Jend - J0 > inner && np - J0 >= h->wide_inner_rows) {
            for (int64_t s0 = J0; s0 < Jend; s0 += inner) {
                const int64_t s1 = (s0 + inner < Jend) ? s0 + inner : Jend;
                int rc = launch_panel_chain(h, A, n, np, lda, s0, s1); if (rc) return rc;
                if (s1 < Jend) { rc = trailing_update(h, A, np, lda, s0, s1, s1, Jend, 0); if (rc) return rc; }
            }
            return 0;
        }
        return launch_panel_chain(h, A, n, np, lda, J0, Jend);
    }
    return panel_factor_nested(h, A, n, np, lda, J0, Jend);
}

// algorithmic bytes of a lower-tile update: every C tile read and written once, the panel's rows (the B operand is the top of A) read once
static double lower_bytes(int64_t M, int64_t N, int64_t K) {
    const double tm = (double)(M / TILE), tn = (double)(N / TILE);
    const double tiles = tn * (tn + 1.0) * 0.5 + (tm - tn) * tn;
    return tiles * 128.0 * 128.0 * 8.0 * 2.0 + (double)M * (double)K * 8.0;
}

static double lower_flops(int64_t M, int64_t N, int64_t K) {     // algorithmic flops of a lower-tile update
    const double tm = (double)(M / TILE), tn = (double)(N / TILE);
    const double tiles = tn * (tn + 1.0) * 0.5 + (tm - tn) * tn;
    return tiles * 128.0 * 128.0 * 2.0 * (double)K;
}

// ---------------------------------------------------------------------------------------
// blocked right-looking Cholesky, three block sizes:
//   128        : panel_factor above;
//   inner_block: a wide outer panel is factored in sub-panels of this width, each followed by one update of the rest
//                of the outer panel with K = inner_block (panel_factor_nested);
//   outer NB   : one trailing SYRK per outer panel with K = NB (outer_block, or outer_block_big while more than
//                big_threshold rows remain), which carries ~all the flops and keeps the C-tile read-modify-write
//                traffic at 8/NB bytes per flop.
// look-ahead (option "lookahead"): the trailing update of panel J is split into the block columns of
// panel J+1 (done first) and the rest; panel J+1 is then factored on a second, high-priority stream
// while the rest of the update runs on the main stream.
// np_force != 0: the padded matrix has np_force rows (fvgp_hip_loglik appends (y-m)^T in a block row of its own when n leaves no padding rows)
// skip_inverses: the caller launches the batched block inverses itself (fvgp_hip_loglik: after it has taken the appended rows out again)
int potrf_driver(fvgp_handle *h, double *A, int64_t n, int64_t lda, int *info_host, int *info_dev, bool enqueue_only, int64_t np_force, bool skip_inverses) {
    const int64_t np = np_force ? np_force : pad128(n), nblk = np / TILE;
    int rc = ensure_blocks(h, nblk);
    if (rc) return rc;
    h->winv_ok = false; h->linv_L = nullptr;
    HIPCHK(hipMemsetAsync(h->dinfo, 0, sizeof(int), h->stream));
    const int64_t NB = h->outer_block;
    size_t nev = 0;
    h->ev_flops.clear(); h->ev_bytes.clear();
    hipEvent_t e_begin = nullptr, e_end = nullptr;
    auto get_event = [&](hipEvent_t *e) -> int {
        if (nev >= h->ev.size()) { hipEvent_t x; HIPCHK(hipEventCreate(&x)); h->ev.push_back(x); }
        *e = h->ev[nev++];
        return 0;
    };
    const bool profile = h->profile && !enqueue_only;
    if (profile) { rc = get_event(&e_begin); if (rc) return rc; HIPCHK(hipEventRecord(e_begin, h->stream)); }
    auto timed_update = [&](int64_t J0, int64_t Jend, int64_t c0, int64_t c1) -> int {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (profile) { int r = get_event(&e0); if (r) return r; HIPCHK(hipEventRecord(e0, h->stream)); }
        bool big = false;
        int r = trailing_update(h, A, np, lda, J0, Jend, c0, c1, 1, &big);
        if (r) return r;
        if (profile) {
            // only launches of the kernel the roofline names count (sub-round updates run the small-tile kernel): 0 flops = skipped
            r = get_event(&e1); if (r) return r; HIPCHK(hipEventRecord(e1, h->stream));
            h->ev_flops.push_back(big ? lower_flops(np - c0, c1 - c0, Jend - J0) : 0.0);
            h->ev_bytes.push_back(big ? lower_bytes(np - c0, c1 - c0, Jend - J0) : 0.0);
        }
        return 0;
    };

    // panel boundaries: width NB, or the wider `outer_block_big` while more than `big_threshold` rows remain
    // (a wider panel halves the C read-modify-write passes of the trailing update; its longer factorisation
    // chain only stays hidden behind the update while the trailing matrix is large)
    // matrices too short for look-ahead (no trailing update to hide a panel behind): ONE resident kernel per 4096 columns, a workgroup per
    // 128 x 128 block (chain.hip) -- 36 us per 128 columns instead of the ~50 us of three launches, and no update launches in between
    const bool wide = h->panel_chain && h->chain_wide && np < h->lookahead_min;
    std::vector<int64_t> bnd;
    for (int64_t J0 = 0; J0 < np;) {
        bnd.push_back(J0);
        if (wide) { const int64_t w = np - J0 > h->wide_threshold ? h->wide_block_big : h->wide_block; J0 = (J0 + w < np) ? J0 + w : np; continue; }
        // three widths: `outer_block_big` (2048) while the trailing update hides any chain, NB (1024), and `outer_block_small`
        // (512) for the last `small_threshold` rows, where the chain is what the factorisation waits for: a 512-wide panel's
        // update tiles retire twice as often (K = 512), so the chain's many-workgroup kernels find slots sooner (N=8k -4 %,
        // N=12k -3 %, N=20k +-0 with 512 throughout)
        int64_t w = (h->outer_block_big > NB && np - J0 > h->big_threshold) ? h->outer_block_big : NB;
        if (h->outer_block_small > 0 && h->outer_block_small < w && np - J0 <= h->small_threshold) w = h->outer_block_small;
        J0 = (J0 + w < np) ? J0 + w : np;
    }
    bnd.push_back(np);
    const size_t npan = bnd.size() - 1;
    // a switch between the two streams costs ~12 us (event wait): below ~6k rows the panels are too short to pay for it
    // (measured: N=4000 2.78 ms with, 2.68 without; N=8000 7.48 / 7.58; N=12000 16.4 / 16.9)
    const bool la = h->lookahead && npan > 2 && np >= h->lookahead_min;
    h->chain_alone = la ? 0 : 1;            // (chain.hip: no trailing update runs beside the panel kernels of this factorisation)
    const bool can_split = la && h->cols_split && h->panel_chain && np - bnd[1] >= h->panel_chain_min && chain_streams_concurrent(h) == 1;
    if (!la) {
        for (size_t J = 0; J < npan; ++J) {
            rc = panel_factor_any(h, A, n, np, lda, bnd[J], bnd[J + 1]); if (rc) return rc;
            if (np > bnd[J + 1]) { rc = timed_update(bnd[J], bnd[J + 1], bnd[J + 1], np); if (rc) return rc; }
        }
    } else {
        rc = fvgp_ensure_side(h); if (rc) return rc;
        hipStream_t mainS = h->stream, sideS = h->side;
        rc = panel_factor_any(h, A, n, np, lda, bnd[0], bnd[1]); if (rc) return rc;      // panel 0 on the main stream
        for (size_t J = 0; J + 1 < npan; ++J) {
            const int64_t J0 = bnd[J], Jend = bnd[J + 1], Nend = bnd[J + 2];           // next panel = [Jend, Nend)
            // (1) main: bring the next panel's block columns up to date with panel J
            // `cols_split`: while few rows remain (the chain is what the factorisation waits for) only the next panel's SQUARE is
            // updated before its chain starts; the rows below it follow on the main stream beside the chain, whose block rows
            // below the square wait for a flag in memory that a one-thread kernel raises behind that update (chain.hip) -- the
            // update of (rows below) x (panel) leaves the critical path: one launch + one stream hand-over per panel
            const bool split = can_split && np - Jend >= h->panel_chain_min && np - Jend <= h->cols_split_rows && np > Nend &&
                               (Nend - Jend) / TILE <= FVGP_CHAIN_MAX_BLOCKS;
            unsigned long long cols_tag = 0;
            if (split) {
                // rows and columns [Jend, Nend): lower tiles
                const double *Ln = A + Jend * lda + J0;
                rc = launch_gemm(h, gemm_desc(0, 0, Nend - Jend, Nend - Jend, Jend - J0, -1.0, Ln, lda, Ln, lda, 1.0, A + Jend * lda + Jend, lda)
                                        .lower_tiles().with_role(1)); if (rc) return rc;
            } else {
                rc = timed_update(J0, Jend, Jend, Nend); if (rc) return rc;
            }
            HIPCHK(hipEventRecord(h->ev_cols, mainS));
            // (2) side: factor the next panel as soon as (1) is done ...
            HIPCHK(hipStreamWaitEvent(sideS, h->ev_cols, 0));
            h->stream = sideS;
            if (split) { rc = launch_panel_chain(h, A, n, np, lda, Jend, Nend, &cols_tag); }
            else rc = panel_factor_any(h, A, n, np, lda, Jend, Nend);
            h->stream = mainS;
            if (rc) return rc;
            HIPCHK(hipEventRecord(h->ev_panel, sideS));
            if (split) {
                // rows [Nend, np) x columns [Jend, Nend): every tile
                rc = launch_gemm(h, gemm_desc(0, 0, np - Nend, Nend - Jend, Jend - J0, -1.0, A + Nend * lda + J0, lda, A + Jend * lda + J0, lda,
                                              1.0, A + Nend * lda + Jend, lda).with_role(1)); if (rc) return rc;
                rc = launch_chain_cols_ready(h, cols_tag); if (rc) return rc;
            }
            // (3) ... while main applies panel J to everything right of the next panel
            if (np > Nend) { rc = timed_update(J0, Jend, Nend, np); if (rc) return rc; }
            // the next iteration's updates use panel J+1: wait for its factorisation
            HIPCHK(hipStreamWaitEvent(mainS, h->ev_panel, 0));
        }
    }
    if (h->leaf_tiles || h->panel_chain) {
        // the chain only needed the inverses of the 16 x 16 diagonal tiles; the 128 x 128 block inverses the sweeps, the
        // posterior and POTRI use come from one launch over all blocks (a few tens of microseconds on the whole chip
        // instead of 8 us per block on the chain's critical path)
        if (!skip_inverses) { rc = launch_leaf_inverse_batched(h, A, lda, nblk, h->linv); if (rc) return rc; }
    }
    if (enqueue_only) {          // no host round trip: info stays on the device, nothing is timed
        if (info_dev) HIPCHK(hipMemcpyAsync(info_dev, h->dinfo, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        h->winv_ok = false; h->linv_L = skip_inverses ? nullptr : A; h->linv_n = n; h->linv_ld = lda;
        return 0;
    }
    if (h->profile) { rc = get_event(&e_end); if (rc) return rc; HIPCHK(hipEventRecord(e_end, h->stream)); }
    int *hinfo = reinterpret_cast<int *>(h->hpin + RED_SLOTS - 2);
    HIPCHK(hipMemcpyAsync(hinfo, h->dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int info = *hinfo;
    if (info == 0x7fffffff) { fvgp_set_error("panel chain: a workgroup waited longer than 3 s for a hand-off and the launch was abandoned"); return 1999; }
    if (info > n) info = 0;   // cannot happen: the padding is an identity block
    if (info_host) *info_host = info;
    h->winv_ok = false; h->linv_L = skip_inverses ? nullptr : A; h->linv_n = n; h->linv_ld = lda;
    if (h->profile) {
        h->prof_launches = 0; h->prof_ms = 0; h->prof_flops = 0; h->prof_bytes = 0;
        for (size_t i = 0; i < h->ev_flops.size(); ++i) {
            if (h->ev_flops[i] <= 0.0) continue;
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, h->ev[1 + 2 * i], h->ev[2 + 2 * i]));
            h->prof_ms += ms; h->prof_flops += h->ev_flops[i]; h->prof_bytes += h->ev_bytes[i]; h->prof_launches += 1.0;
        }
        float tot = 0.f;
        HIPCHK(hipEventElapsedTime(&tot, e_begin, e_end));
        h->prof_total_ms = tot;
    }
    return 0;
}


int fvgp_read_back(fvgp_handle *h, const double *dev, double *host, int count) {
    HIPCHK(hipMemcpyAsync(h->hpin, dev, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < count; ++i) host[i] = h->hpin[i];
    return fvgp_ipc_check(h);       // (direct collectives: a poll that gave up left stale data behind it -- never hand that to the host)
}

extern "C" {

int fvgp_hip_potrf(fvgp_handle *h, double *A, int64_t n, int64_t lda, int *info_host) {
    if (!h) return -1;
    int rc = check_square(A, n, lda, 2, 3, 4);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    rc = launch_pad_identity(h, A, n, pad128(n), lda);
    if (rc) return rc;
    return potrf_driver(h, A, n, lda, info_host);
}

int fvgp_hip_potrf_dev(fvgp_handle *h, double *A, int64_t n, int64_t lda, int64_t n_logdet, int *info_dev, double *logdet_dev) {
    if (!h) return -1;
    int rc = check_square(A, n, lda, 2, 3, 4);
    if (rc) return rc;
    if (n_logdet < 0 || n_logdet > n) return -5;
    if (!info_dev) return -6;
    HIPCHK(hipSetDevice(h->device));
    rc = launch_pad_identity(h, A, n, pad128(n), lda);
    if (rc) return rc;
    rc = potrf_driver(h, A, n, lda, nullptr, info_dev, true);
    if (rc) return rc;
    if (logdet_dev && n_logdet > 0) return launch_diag_logsum(h, A, n_logdet, lda, logdet_dev);
    return 0;
}

int fvgp_hip_panel_potrf_dev(fvgp_handle *h, double *T, int64_t w, int64_t rows, int64_t ldt, int64_t n_valid,
                             int *info_dev, double *logdet_dev) {
    if (!h) return -1;
    if (!T) return -2;
    if (w <= 0 || w % TILE) { fvgp_set_error("panel_potrf_dev: the panel width must be a positive multiple of 128"); return -3; }
    if (rows < w || rows % TILE) return -4;
    if (ldt < w || (ldt & 1) || ((uintptr_t)T & 15)) return -5;
    if (n_valid < 0 || n_valid > w) return -6;
    if (!info_dev) return -7;
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_blocks(h, w / TILE);
    if (rc) return rc;
    h->winv_ok = false; h->linv_L = nullptr;
    HIPCHK(hipMemsetAsync(h->dinfo, 0, sizeof(int), h->stream));
    // the row-sharded driver's stacked panel: ONE resident kernel with a workgroup per block (8-rank emulation at N = 50 000: 93.2 ms
    // against 96.0 with the launch-per-step chain; with a workgroup per block ROW below the square, panel_chain = 2, 100.6)
    if (h->panel_chain >= 1 && w / TILE <= FVGP_CHAIN_MAX_BLOCKS && rows / TILE <= 1024) { h->chain_alone = h->panel_chain == 2 ? 0 : 2; rc = launch_panel_chain(h, T, n_valid, rows, ldt, 0, w); }      // (2: a workgroup per block, but NOT alone: the rank's trailing update runs beside it)
    else rc = panel_factor_nested(h, T, n_valid, rows, ldt, 0, w);   // leaf / TRSM of every row below / in-panel update per 128 columns, in sub-panels of `inner_block`
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(info_dev, h->dinfo, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    if (logdet_dev && n_valid > 0) return launch_diag_logsum(h, T, n_valid, ldt, logdet_dev);
    return 0;
}

}  // extern "C"
