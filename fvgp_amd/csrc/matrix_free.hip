// Solves with K(theta) + V without the matrix: the product with a block of vectors, the pivoted-Cholesky preconditioner and
// the preconditioned conjugate gradients whose scalars stay on the device.
//
// fvgp_hip_kmatvec   Y = K(x1, x2) B + diag(v) B.  select_cross_kernel widened: lanes along 64 output rows, the x2 rows and S entries of
//     B per row staged in LDS (slice_sum.h, broadcast reads), S accumulator pairs per lane filled by the same row loop (slice_rows),
//     so one exp (plus the rsq of the Matern kinds) serves S columns.  The order of every sum is a function of n2 alone: x2 is cut
//     into chunks of MATVEC_CHUNK rows, a chunk into slices of SLICE_ROWS; wave w sums rows [64 w, 64 w + 64) of every slice of the
//     chunk into an even-row and an odd-row accumulator; the chunk's sum is (((e0 + o0) + (e1 + o1)) + (e2 + o2)) + (e3 + o3); chunk
//     sums are added to 0 in ascending order; v_i B_ic enters as the last fused multiply-add.  A workgroup that walks all chunks
//     (gridDim.y == 1) and a launch that deals chunk ranges over gridDim.y, parks the per-chunk sums and adds them in a second pass
//     give the same bits.
// fvgp_hip_pchol     greedy pivoted Cholesky of K(x, x), q steps enqueued at once: selection's greedy pivot core (pivot.h) with the
//     data as their own candidates, no conditioning (pivot_downdate_kernel<KIND, CROSS = false>) and no noise.
// fvgp_hip_precond_factor   C = I + G D^-1 G^T in fixed-order chunks of PF_CHUNK points, factored by potrf_driver.
// fvgp_hip_pcg       s <= 16 independent recurrences that share the matvec; every vector kernel reads the per-column state
//     (active, alpha, beta) from device memory, the host reads the status words every `check_every` iterations.
// The stochastic log-likelihood:
// fvgp_hip_kgrad_form       sum_c U[:, c]^T (dK / dtheta_j) W[:, c] for every j in ONE pass over the kernel entries: kmatvec_kernel's shape
//     (lanes along 64 rows of x1, x2 rows and S entries of W per row staged in LDS, U[i, 0 .. S) in registers), per entry one
//     radial_grad, S fused multiply-adds for t = sum_c U[i][c] W[k][c] and one per hyperparameter.  Sums as in the product; the rows of
//     a block by a halving tree, the blocks in ascending order by one small kernel: no atomics.
// fvgp_hip_precond_probes   Z = D^1/2 eps + G^T eta from the normals of normal.h;  fvgp_hip_precond_apply   the solver's M^-1 on its own;
// fvgp_hip_pcg_lanczos      the solver with the coefficients of every column's first recurrence recorded (one driver serves both entries).
#include "radial.h"
#include "kernel_family.h"
#include "slice_sum.h"
#include "pivot.h"
#include "normal.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int MATVEC_CHUNK = FVGP_MATVEC_CHUNK;      // x2 rows per chunk sum (a multiple of SLICE_ROWS)
constexpr int MV_MAXS = 16;                          // widest column group
constexpr int PCG_LD = FVGP_PCG_MAX_RHS;             // row stride of the solver's own vectors
constexpr int PF_CHUNK = 8192;                       // points per partial Gram sum of precond_factor
constexpr int PT_CHUNK = 4096;                       // points per partial of G (D^-1 R)
constexpr int DOT_ROWS = 1024;                       // rows per partial of the dot products
static_assert(MATVEC_CHUNK % SLICE_ROWS == 0, "a chunk is whole slices");

// ---------------------------------------------------------------------------------------------------------------- the product
struct MvArgs {
    const double *x1, *x2, *B, *v;
    double *Y, *part;                        // part: nullptr (the workgroup adds its chunks itself) or (nchunks, n1, S) chunk sums
    long n1, n2, ldb, ldy, nchunks, cpy;     // cpy: chunks per blockIdx.y
    int d, c0, sc;                           // columns [c0, c0 + sc) of B and Y, sc <= S
    double sig;
    double il[FVGP_MAX_DIM];
};

template <int KIND, int D, int S>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void kmatvec_kernel(MvArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    __shared__ __attribute__((aligned(16))) double sm[SLICE_ROWS * (DD + S)];     // (>= 3 * 64 * S: the parked sums of waves 1 .. 3)
    double *sx = sm, *sb = sm + SLICE_ROWS * DD;
    const int d = D ? D : a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long loc = (long)blockIdx.x * 64 + lane;
    const long i = loc < a.n1 ? loc : a.n1 - 1;
    double u[DD], il[DD];                                     // (il: a copy, so that the address of the kernel's arguments is never taken)
#pragma unroll
    for (int k = 0; k < DD; ++k) { u[k] = k < d ? a.x1[i * d + k] : 0.0; il[k] = a.il[k]; }
    const long ch0 = (long)blockIdx.y * a.cpy, ch1 = ch0 + a.cpy < a.nchunks ? ch0 + a.cpy : a.nchunks;
    double tot[S];
#pragma unroll
    for (int c = 0; c < S; ++c) tot[c] = 0.0;

    for (long ch = ch0; ch < ch1; ++ch) {
        double s0[S], s1[S];                                  // even and odd rows of this wave's share of the chunk
#pragma unroll
        for (int c = 0; c < S; ++c) { s0[c] = 0.0; s1[c] = 0.0; }
        const long rbeg = ch * MATVEC_CHUNK, rend = rbeg + MATVEC_CHUNK < a.n2 ? rbeg + MATVEC_CHUNK : a.n2;
        for (long row0 = rbeg; row0 < rend; row0 += SLICE_ROWS) {
            __syncthreads();                                  // the last slice's rows (or the parked sums) have been read
            slice_stage_cols<DD, S>(sx, sb, a.x2, a.B, a.ldb, a.c0, a.sc, a.n2, d, row0, tid);
            __syncthreads();
            const int r0 = wave * SLICE_WAVE_ROWS, rows = slice_wave_rows(a.n2, row0, wave);
            slice_rows<KIND, DD, S>(sx, sb, r0, rows, d, u, il, a.sig, s0, s1);
        }
        __syncthreads();                                      // every wave is done with the staged rows
        if (wave > 0) {
#pragma unroll
            for (int c = 0; c < S; ++c) slice_parked(sm, S, wave, lane)[c * 64] = s0[c] + s1[c];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < S; ++c) {
                double t = s0[c] + s1[c];
#pragma unroll
                for (int ww = 1; ww < 4; ++ww) t += slice_parked(sm, S, ww, lane)[c * 64];      // ((wave 0 + wave 1) + wave 2) + wave 3
                if (a.part) { if (loc < a.n1) a.part[(ch * a.n1 + loc) * S + c] = t; }
                else tot[c] += t;
            }
        }
    }
    if (a.part || wave != 0 || loc >= a.n1) return;
#pragma unroll
    for (int c = 0; c < S; ++c)
        if (c < a.sc) a.Y[loc * a.ldy + a.c0 + c] = a.v ? fma(a.v[loc], a.B[loc * a.ldb + a.c0 + c], tot[c]) : tot[c];
}

// the second pass of a split launch: one thread per (row, column), the chunk sums added to 0 in ascending order
__global__ __launch_bounds__(256) void kmatvec_reduce_kernel(MvArgs a, int S) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n1 * a.sc) return;
    const long loc = e / a.sc;
    const int c = (int)(e - loc * a.sc);
    double tot = 0.0;
    for (long ch = 0; ch < a.nchunks; ++ch) tot += a.part[(ch * a.n1 + loc) * S + c];
    a.Y[loc * a.ldy + a.c0 + c] = a.v ? fma(a.v[loc], a.B[loc * a.ldb + a.c0 + c], tot) : tot;
}

inline int64_t mv_chunks(int64_t n2) { return (n2 + MATVEC_CHUNK - 1) / MATVEC_CHUNK; }
inline int mv_group(int left) { return left >= MV_MAXS ? MV_MAXS : left > 4 ? 8 : left > 1 ? 4 : 1; }      // the narrowest group that holds what is left
inline int64_t mv_split_doubles(int64_t n1, int64_t n2, int s) { return mv_chunks(n2) * n1 * mv_group(s); }
// the launches' gridDim.y when nothing is forced: chunk ranges are dealt out only while the 64-row blocks alone cannot fill the chip
inline int64_t mv_auto_split(int64_t n1, int64_t n2) {
    const int64_t bx = (n1 + 63) / 64, nch = mv_chunks(n2);
    if (nch < 2 || bx >= 512) return 1;
    const int64_t gy = (1024 + bx - 1) / bx;
    return gy < nch ? gy : nch;
}

template <int KIND, int D, int S>
void mv_launch(fvgp_handle *h, const MvArgs &a, dim3 grid) {
    hipLaunchKernelGGL((kmatvec_kernel<KIND, D, S>), grid, dim3(256), 0, h->stream, a);
}

// Y[:, 0 .. s) = K B + diag(v) B.  k: x1, n1, x2, n2, d, kind, sig, invl, vdiag.  work_doubles < what a forced split needs: -1 unless
// `fallback` (then the unsplit form, which has the same bits)
int launch_kmatvec(fvgp_handle *h, const KmatDesc &k, const double *B, int64_t ldb, int s, double *Y, int64_t ldy, double *work,
                   int64_t work_doubles, bool fallback) {
    MvArgs a;
    a.x1 = k.x1; a.x2 = k.x2; a.B = B; a.v = k.vdiag; a.Y = Y;
    a.n1 = k.n1; a.n2 = k.n2; a.ldb = ldb; a.ldy = ldy; a.nchunks = mv_chunks(k.n2);
    a.d = k.d; a.sig = k.sig;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
    int64_t gy = h->matvec_split == 0 ? mv_auto_split(k.n1, k.n2) : h->matvec_split;
    if (gy > a.nchunks) gy = a.nchunks;
    if (gy > 65535) gy = 65535;
    const int64_t bx = (k.n1 + 63) / 64;
    for (int c0 = 0; c0 < s;) {
        const int left = s - c0;
        const int S = mv_group(left);
        a.c0 = c0; a.sc = left < S ? left : S;
        bool split = gy > 1;
        if (split && (!work || work_doubles < a.nchunks * k.n1 * S)) {
            if (h->matvec_split > 1 && !fallback) { fvgp_set_error("kmatvec: work smaller than fvgp_hip_kmatvec_workspace_bytes(n1, n2, s)"); return -1; }
            split = false;
        }
        a.part = split ? work : nullptr;
        a.cpy = split ? (a.nchunks + gy - 1) / gy : a.nchunks;
        const dim3 grid((unsigned)bx, split ? (unsigned)((a.nchunks + a.cpy - 1) / a.cpy) : 1u);
        dispatch_kind_dim(k.kind, k.d, [&](auto KIND, auto D) {
            constexpr int KK = decltype(KIND)::value, DV = decltype(D)::value;
            switch (S) {
                case 16: mv_launch<KK, DV, 16>(h, a, grid); break;
                case 8: mv_launch<KK, DV, 8>(h, a, grid); break;
                case 4: mv_launch<KK, DV, 4>(h, a, grid); break;
                default: mv_launch<KK, DV, 1>(h, a, grid); break;
            }
        });
        HIPCHK(hipGetLastError());
        if (split) {
            hipLaunchKernelGGL(kmatvec_reduce_kernel, dim3((unsigned)((k.n1 * a.sc + 255) / 256)), dim3(256), 0, h->stream, a, S);
            HIPCHK(hipGetLastError());
        }
        c0 += a.sc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------ the gradient's bilinear form
constexpr int KG_H = 1 + FVGP_MAX_DIM;               // stride of every per-hyperparameter sum (sigma^2, then the length scales)

struct KgArgs {
    const double *x1, *x2, *U, *W;
    double *park, *bpart;                    // park: nullptr (the workgroup adds its chunks itself) or (nchunks, n1, KG_H) chunk sums; bpart (blocks, KG_H)
    long n1, n2, ldu, ldw, nchunks, cpy;     // cpy: chunks per blockIdx.y
    int d, c0, sc, iso;                      // columns [c0, c0 + sc) of U and W, sc <= S
    double sig;
    double il[FVGP_MAX_DIM];
};

// the lane's sums of one row of x1 (length scales already times 1 / l) added over the block's 64 lanes by the halving tree; lane 0 writes
template <int DD>
__device__ __forceinline__ void kg_block_sum(double (&tot)[DD + 1], int nh, int lane, double *out) {
#pragma unroll
    for (int hh = 0; hh < DD + 1; ++hh)
        if (hh < nh) {
            double w = tot[hh];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
            if (lane == 0) out[hh] = w;
        }
}

template <int KIND, int D, int S>   // D == 0: runtime dimension (<= FVGP_MAX_DIM)
__global__ __launch_bounds__(256) void kgrad_form_kernel(KgArgs a) {
    constexpr int DD = D ? D : FVGP_MAX_DIM;
    constexpr int NH = DD + 1;                                                    // accumulators per chain: sigma^2 and DD length scales (iso: one)
    __shared__ __attribute__((aligned(16))) double sm[SLICE_ROWS * (DD + S)];     // (>= 3 * 64 * NH: the parked sums of waves 1 .. 3)
    double *sx = sm, *sw = sm + SLICE_ROWS * DD;
    const int d = D ? D : a.d;
    const int nh = a.iso ? 2 : d + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long loc = (long)blockIdx.x * 64 + lane;
    const long i = loc < a.n1 ? loc : a.n1 - 1;
    double u[DD], il[DD], uc[S];
#pragma unroll
    for (int k = 0; k < DD; ++k) { u[k] = k < d ? a.x1[i * d + k] : 0.0; il[k] = a.il[k]; }
#pragma unroll
    for (int c = 0; c < S; ++c) uc[c] = (loc < a.n1 && c < a.sc) ? a.U[i * a.ldu + a.c0 + c] : 0.0;
    const long ch0 = (long)blockIdx.y * a.cpy, ch1 = ch0 + a.cpy < a.nchunks ? ch0 + a.cpy : a.nchunks;
    double tot[NH];
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) tot[hh] = 0.0;

    for (long ch = ch0; ch < ch1; ++ch) {
        double g0[NH], g1[NH];                                // even and odd rows of this wave's share of the chunk
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) { g0[hh] = 0.0; g1[hh] = 0.0; }
        // one entry: row r of the staged slice into the chain g
        auto entry = [&](const int r, double (&g)[NH]) {
            const double *xr = sx + r * DD, *wr = sw + r * S;
            double e2[DD], r2 = 0.0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (k < d) { const double e = (u[k] - xr[k]) * il[k]; e2[k] = e * e; r2 += e2[k]; }
                else e2[k] = 0.0;
            }
            double phi, cf, t = 0.0;
            radial_grad<KIND>(r2, a.sig, phi, cf);
#pragma unroll
            for (int c = 0; c < S; ++c) t = fma(uc[c], wr[c], t);
            g[0] = fma(phi, t, g[0]);
            const double wc = cf * t;
            if (a.iso) g[1] = fma(wc, r2, g[1]);
            else {
#pragma unroll
                for (int k = 0; k < DD; ++k) if (k < d) g[1 + k] = fma(wc, e2[k], g[1 + k]);
            }
        };
        const long rbeg = ch * MATVEC_CHUNK, rend = rbeg + MATVEC_CHUNK < a.n2 ? rbeg + MATVEC_CHUNK : a.n2;
        for (long row0 = rbeg; row0 < rend; row0 += SLICE_ROWS) {
            __syncthreads();                                  // the last slice's rows (or the parked sums) have been read
            slice_stage_cols<DD, S>(sx, sw, a.x2, a.W, a.ldw, a.c0, a.sc, a.n2, d, row0, tid);
            __syncthreads();
            const int r0 = wave * SLICE_WAVE_ROWS, rows = slice_wave_rows(a.n2, row0, wave);
            int r = 0;
            for (; r + 1 < rows; r += 2) { entry(r0 + r, g0); entry(r0 + r + 1, g1); }
            if (r < rows) entry(r0 + r, g0);
        }
        __syncthreads();                                      // every wave is done with the staged rows
        if (wave > 0) {
#pragma unroll
            for (int hh = 0; hh < NH; ++hh) if (hh < nh) slice_parked(sm, NH, wave, lane)[hh * 64] = g0[hh] + g1[hh];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int hh = 0; hh < NH; ++hh)
                if (hh < nh) {
                    double t = g0[hh] + g1[hh];
#pragma unroll
                    for (int ww = 1; ww < 4; ++ww) t += slice_parked(sm, NH, ww, lane)[hh * 64];      // ((wave 0 + wave 1) + wave 2) + wave 3
                    if (a.park) { if (loc < a.n1) a.park[(ch * a.n1 + loc) * KG_H + hh] = t; }
                    else tot[hh] += t;
                }
        }
    }
    if (a.park || wave != 0) return;
    if (loc >= a.n1) {                                        // (a lane past n1 repeats the last row with U = 0: its sums count as 0 whatever they are)
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) tot[hh] = 0.0;
    }
#pragma unroll
    for (int hh = 1; hh < NH; ++hh) if (hh < nh) tot[hh] *= il[hh - 1];
    kg_block_sum<DD>(tot, nh, lane, a.bpart + (long)blockIdx.x * KG_H);
}

// the second pass of a split launch: one wave per 64 rows, a lane adds its row's chunk sums to 0 in ascending order, then as above
__global__ __launch_bounds__(64) void kgrad_rows_kernel(KgArgs a) {
    const int lane = threadIdx.x, nh = a.iso ? 2 : a.d + 1;
    const long loc = (long)blockIdx.x * 64 + lane;
    double tot[KG_H];
#pragma unroll
    for (int hh = 0; hh < KG_H; ++hh) {
        double t = 0.0;
        if (hh < nh && loc < a.n1)
            for (long ch = 0; ch < a.nchunks; ++ch) t += a.park[(ch * a.n1 + loc) * KG_H + hh];
        tot[hh] = hh >= 1 && hh < nh ? t * a.il[hh - 1] : t;
    }
    kg_block_sum<FVGP_MAX_DIM>(tot, nh, lane, a.bpart + (long)blockIdx.x * KG_H);
}

// out[j] = (first ? 0 : out[j]) + the blocks' sums added to 0 in ascending order; one thread per hyperparameter
__global__ __launch_bounds__(64) void kgrad_sum_kernel(const double *bpart, long nblocks, int nh, int first, double *out) {
    const int hh = threadIdx.x;
    if (hh >= nh) return;
    double acc = 0.0;
    for (long b = 0; b < nblocks; ++b) acc += bpart[b * KG_H + hh];
    out[hh] = first ? acc : out[hh] + acc;
}

template <int KIND, int D, int S>
void kg_launch(fvgp_handle *h, const KgArgs &a, dim3 grid) {
    hipLaunchKernelGGL((kgrad_form_kernel<KIND, D, S>), grid, dim3(256), 0, h->stream, a);
}

inline int64_t kg_base_doubles(int64_t n1) { return (1 + (n1 + 63) / 64) * KG_H; }

// ------------------------------------------------------------------------------------------------------ the probes
struct ProbeArgs {
    uint32_t k0, k1, e0, e1, g0, g1;         // the key (seed) and the two streams' words: 2 stream (eps) and 2 stream + 1 (eta)
    const double *G, *v;
    double *Z;
    long ldg, n, ldz, col0;
    int q, s;
};

// a workgroup takes 256 points, a thread one of them and all s columns; eta goes through LDS 16 rows of G at a time
__global__ __launch_bounds__(256) void precond_probes_kernel(ProbeArgs a) {
    __shared__ double se[16][PCG_LD];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + tid;
    const bool live = i < a.n;
    double acc[PCG_LD];
    const double sv = live ? sqrt(a.v[i]) : 0.0;
#pragma unroll
    for (int c = 0; c < PCG_LD; ++c)
        acc[c] = (live && c < a.s) ? sv * normal_at(a.k0, a.k1, a.e0, a.e1, (uint32_t)i, (uint32_t)(a.col0 + c)) : 0.0;
    for (int t0 = 0; t0 < a.q; t0 += 16) {
        __syncthreads();
        {
            const int tt = tid >> 4, c = tid & 15;
            se[tt][c] = (t0 + tt < a.q && c < a.s) ? normal_at(a.k0, a.k1, a.g0, a.g1, (uint32_t)(t0 + tt), (uint32_t)(a.col0 + c)) : 0.0;
        }
        __syncthreads();
        const int tn = a.q - t0 < 16 ? a.q - t0 : 16;
        if (live)
            for (int tt = 0; tt < tn; ++tt) {
                const double g = a.G[(long)(t0 + tt) * a.ldg + i];
#pragma unroll
                for (int c = 0; c < PCG_LD; ++c) acc[c] = fma(g, se[tt][c], acc[c]);
            }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < PCG_LD; ++c) if (c < a.s) a.Z[i * a.ldz + c] = acc[c];
}

// rows x s doubles from src (ld lds) into dst (ld ldd): the block fvgp_hip_precond_apply moves into and out of the solver's layout
__global__ __launch_bounds__(256) void mf_copy_cols_kernel(const double *src, long lds, double *dst, long ldd, long rows, int s) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(e & 15);
    const long i = e >> 4;
    if (i < rows && c < s) dst[i * ldd + c] = src[i * lds + c];
}

// ------------------------------------------------------------------------------------------------------ the pivoted Cholesky
__global__ __launch_bounds__(256) void mf_zero_rows_kernel(double *A, long ld, long rows, long cols) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cols) return;
    const long r = e / cols;
    A[r * ld + (e - r * cols)] = 0.0;
}

// ------------------------------------------------------------------------------------------------------ the preconditioner
// partial Gram sums of one chunk of PF_CHUNK points: part[chunk][a][b] = sum_i G[a,i] G[b,i] / v_i for b <= a, 16 x 16 per workgroup,
// every thread its own entry, points in ascending order
__global__ __launch_bounds__(256) void pf_gram_kernel(const double *G, long ldg, int q, long n, const double *v, double *part) {
    __shared__ double sa[16][65], sb[16][65];
    const int nt = (q + 15) / 16, ta = blockIdx.x / nt, tb = blockIdx.x % nt;
    if (tb > ta) return;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long i0 = (long)blockIdx.y * PF_CHUNK, i1 = i0 + PF_CHUNK < n ? i0 + PF_CHUNK : n;
    double acc = 0.0;
    for (long ib = i0; ib < i1; ib += 64) {
        for (int e = tid; e < 16 * 64; e += 256) {
            const int rr = e >> 6, kk = e & 63;
            const long i = ib + kk;
            const int ra = ta * 16 + rr, rb = tb * 16 + rr;
            sa[rr][kk] = i < i1 && ra < q ? G[(long)ra * ldg + i] / v[i] : 0.0;
            sb[rr][kk] = i < i1 && rb < q ? G[(long)rb * ldg + i] : 0.0;
        }
        __syncthreads();
#pragma unroll 16
        for (int kk = 0; kk < 64; ++kk) acc = fma(sa[ty][kk], sb[tx][kk], acc);
        __syncthreads();
    }
    const int ra = ta * 16 + ty, rb = tb * 16 + tx;
    if (ra < q && rb <= ra) part[((long)blockIdx.y * q + ra) * q + rb] = acc;
}

// C[a][b] = C[b][a] = (a == b) + the chunks' sums in ascending order
__global__ __launch_bounds__(256) void pf_finish_kernel(const double *part, long nchunks, int q, double *C, long ldc) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)q * q) return;
    const int ra = (int)(e / q), rb = (int)(e - (long)ra * q);
    if (rb > ra) return;
    double s = 0.0;
    for (long c = 0; c < nchunks; ++c) s += part[(c * q + ra) * q + rb];
    s += ra == rb ? 1.0 : 0.0;
    C[(long)ra * ldc + rb] = s;
    C[(long)rb * ldc + ra] = s;
}

// ------------------------------------------------------------------------------------------------------ conjugate gradients
// per-column state of the recurrences, on the device
struct PcgState {
    double rho[PCG_LD], alpha[PCG_LD], beta[PCG_LD], rn2[PCG_LD], bnorm[PCG_LD], relres[PCG_LD];
    int active[PCG_LD], code[PCG_LD], iters[PCG_LD], restart[PCG_LD];      // code: 0 residual met, 1 iteration limit, 2 breakdown
};
enum { SC_INIT = 0, SC_RHO0 = 1, SC_ALPHA = 2, SC_RNORM = 3, SC_BETA = 4, SC_TRUE = 5, SC_RESTART = 6 };

// what fvgp_hip_pcg_lanczos records of every column's first recurrence, on the device behind the solver's workspace; alpha == nullptr: nothing
struct PcgRec {
    double *alpha, *beta, *rho0;             // (PCG_LD, L), (PCG_LD, L), (PCG_LD)
    int *steps, *first;                      // alphas recorded; 1 until the column's first restart
    int L;
};

struct PcgVec {
    double *R, *Z, *P, *AP;                  // (n, PCG_LD)
    double *X; long ldx;
    const double *B; long ldb;
    const double *v;
    PcgState *st;
    double *part0, *part1;                   // (nblk, PCG_LD) partial dot products
    long n;
    int s;
};

// the block's share of sum_i a_i b_i for every column: thread (g, c) adds rows g, g + 16, .. of the DOT_ROWS, then a tree over g
__device__ __forceinline__ void dot_block(double acc, double *out, int tid, bool live) {
    __shared__ double sh[256];
    sh[tid] = acc;
    __syncthreads();
    for (int off = 128; off >= 16; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    if (tid < 16 && live) out[(long)blockIdx.x * PCG_LD + tid] = sh[tid];
}

// what = 0: R = B, part0 = b.b;  1: R = B - AP, part0 = b.b, part1 = r.r (warm start);  2: R = B - AP for frozen columns, part1 = r.r
__global__ __launch_bounds__(256) void pcg_resid_kernel(PcgVec a, int what) {
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    const long r0 = (long)blockIdx.x * DOT_ROWS, r1 = r0 + DOT_ROWS < a.n ? r0 + DOT_ROWS : a.n;
    double bb = 0.0, rr = 0.0;
    const bool live = c < a.s;
    if (live)
        for (long i = r0 + g; i < r1; i += 16) {
            const double b = a.B[i * a.ldb + c];
            double r = b;
            if (what) r = b - a.AP[i * PCG_LD + c];
            if (what == 0) a.X[i * a.ldx + c] = 0.0;
            a.R[i * PCG_LD + c] = r;
            bb = fma(b, b, bb); rr = fma(r, r, rr);
        }
    if (what != 2) dot_block(bb, a.part0, tid, live);
    if (what != 0) { __syncthreads(); dot_block(rr, a.part1, tid, live); }
}

// part0 = sum_i a_i b_i per column
__global__ __launch_bounds__(256) void pcg_dot_kernel(const double *A, const double *Bv, long n, int s, double *part) {
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    const long r0 = (long)blockIdx.x * DOT_ROWS, r1 = r0 + DOT_ROWS < n ? r0 + DOT_ROWS : n;
    double acc = 0.0;
    if (c < s)
        for (long i = r0 + g; i < r1; i += 16) acc = fma(A[i * PCG_LD + c], Bv[i * PCG_LD + c], acc);
    dot_block(acc, part, tid, c < s);
}

// active columns: x += alpha p, r -= alpha Ap, part0 = r.r
__global__ __launch_bounds__(256) void pcg_axpy_kernel(PcgVec a) {
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    const long r0 = (long)blockIdx.x * DOT_ROWS, r1 = r0 + DOT_ROWS < a.n ? r0 + DOT_ROWS : a.n;
    double rr = 0.0;
    const bool live = c < a.s && a.st->active[c];
    if (live) {
        const double al = a.st->alpha[c];
        for (long i = r0 + g; i < r1; i += 16) {
            const double p = a.P[i * PCG_LD + c];
            a.X[i * a.ldx + c] = fma(al, p, a.X[i * a.ldx + c]);
            const double r = fma(-al, a.AP[i * PCG_LD + c], a.R[i * PCG_LD + c]);
            a.R[i * PCG_LD + c] = r;
            rr = fma(r, r, rr);
        }
    }
    dot_block(rr, a.part0, tid, c < a.s);
}

// active columns: p = z + beta p (beta == 0: p = z)
__global__ __launch_bounds__(256) void pcg_dir_kernel(PcgVec a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(e & 15);
    const long i = e >> 4;
    if (i >= a.n || c >= a.s || !a.st->active[c]) return;
    const double be = a.st->beta[c], z = a.Z[i * PCG_LD + c];
    a.P[i * PCG_LD + c] = be == 0.0 ? z : fma(be, a.P[i * PCG_LD + c], z);
}

// a warm start whose right-hand side is zero: x = 0
__global__ __launch_bounds__(256) void pcg_zero_cols_kernel(PcgVec a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(e & 15);
    const long i = e >> 4;
    if (i < a.n && c < a.s && a.st->bnorm[c] == 0.0) a.X[i * a.ldx + c] = 0.0;
}

// one workgroup: the partials of every column added in an order n alone fixes (thread (g, c): blocks g, g + 16, ..; a tree over g),
// then the column's scalar step
__global__ __launch_bounds__(256) void pcg_scalar_kernel(PcgVec a, long nblk, int mode, double tol, int max_iter, PcgRec rec) {
    __shared__ double sh[2][256];
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    double s0 = 0.0, s1 = 0.0;
    if (c < a.s)
        for (long b = g; b < nblk; b += 16) { s0 += a.part0[b * PCG_LD + c]; s1 += a.part1[b * PCG_LD + c]; }
    sh[0][tid] = s0; sh[1][tid] = s1;
    __syncthreads();
    for (int off = 128; off >= 16; off >>= 1) {
        if (tid < off) { sh[0][tid] += sh[0][tid + off]; sh[1][tid] += sh[1][tid + off]; }
        __syncthreads();
    }
    if (tid >= a.s) return;
    PcgState &st = *a.st;
    const double v0 = sh[0][tid], v1 = sh[1][tid];
    switch (mode) {
        case SC_INIT: {                                       // v0 = b.b, v1 = r.r (cold start: the caller points part1 at part0)
            const double bn = sqrt(v0);
            st.bnorm[c] = bn; st.rn2[c] = v1; st.iters[c] = 0; st.code[c] = 0; st.beta[c] = 0.0; st.alpha[c] = 0.0; st.rho[c] = 0.0;
            st.relres[c] = 0.0; st.restart[c] = 0;
            st.active[c] = (bn > 0.0 && sqrt(v1) > tol * bn) || !(v1 == v1) ? 1 : 0;
            if (rec.alpha) { rec.first[c] = 1; rec.steps[c] = 0; rec.rho0[c] = 0.0; }
            break;
        }
        case SC_RHO0:                                         // v0 = r.z
            if (st.active[c]) {
                st.rho[c] = v0; st.beta[c] = 0.0;
                if (!(v0 > 0.0) || isinf(v0)) { st.active[c] = 0; st.code[c] = 2; }
                else if (rec.alpha) rec.rho0[c] = v0;
            }
            break;
        case SC_ALPHA:                                        // v0 = p.Ap
            if (st.active[c]) {
                if (!(v0 > 0.0) || isinf(v0)) { st.active[c] = 0; st.code[c] = 2; }
                else {
                    st.alpha[c] = st.rho[c] / v0;
                    if (rec.alpha && rec.first[c] && st.iters[c] < rec.L) { rec.alpha[c * rec.L + st.iters[c]] = st.alpha[c]; rec.steps[c] = st.iters[c] + 1; }
                }
            }
            break;
        case SC_RNORM:                                        // v0 = r.r
            if (st.active[c]) {
                st.rn2[c] = v0; st.iters[c] += 1;
                if (sqrt(v0) <= tol * st.bnorm[c]) { st.active[c] = 0; st.code[c] = 0; }
                else if (st.iters[c] >= max_iter) { st.active[c] = 0; st.code[c] = 1; }
            }
            break;
        case SC_BETA:                                         // v0 = r.z
            if (st.active[c]) {
                if (!(v0 > 0.0) || isinf(v0)) { st.active[c] = 0; st.code[c] = 2; }
                else {
                    st.beta[c] = v0 / st.rho[c]; st.rho[c] = v0;
                    if (rec.alpha && rec.first[c] && st.iters[c] <= rec.L) rec.beta[c * rec.L + st.iters[c] - 1] = st.beta[c];
                }
            }
            break;
        case SC_TRUE:                                         // v1 = |b - A x|^2
            st.relres[c] = st.bnorm[c] > 0.0 ? sqrt(v1) / st.bnorm[c] : 0.0;
            st.rn2[c] = v1;
            break;
        default:                                              // SC_RESTART: v0 = r.z of the true residual
            if (st.restart[c]) {
                if (rec.alpha) rec.first[c] = 0;
                st.restart[c] = 0; st.rho[c] = v0; st.beta[c] = 0.0; st.code[c] = 0;
                if (!(v0 > 0.0) || isinf(v0)) st.code[c] = 2; else st.active[c] = 1;
            }
            break;
    }
}

// T partials of one chunk of PT_CHUNK points: part[chunk][t][c] = sum_i G[t,i] R[i,c] / v_i.  The chunk goes through LDS in pieces of
// 256 points (column-major, so that the lanes of a wave read neighbouring words); wave w takes rows t = w, w + 4, ..; a lane adds its
// four points in ascending order, the wave's lanes are added by the shuffle tree, pieces in ascending order
__global__ __launch_bounds__(256) void pcg_gr_kernel(const double *G, long ldg, int q, PcgVec a, double *part) {
    __shared__ double sr[PCG_LD][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long i0 = (long)blockIdx.x * PT_CHUNK, i1 = i0 + PT_CHUNK < a.n ? i0 + PT_CHUNK : a.n;
    double *out = part + (long)blockIdx.x * q * PCG_LD;
    for (long ib = i0; ib < i1; ib += 256) {
        __syncthreads();
        for (int e = tid; e < 256 * PCG_LD; e += 256) {
            const int rr = e >> 4, cc = e & 15;
            const long i = ib + rr;
            sr[cc][rr] = i < i1 && cc < a.s ? a.R[i * PCG_LD + cc] / a.v[i] : 0.0;
        }
        __syncthreads();
        for (int t = wave; t < q; t += 4) {
            double gk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const long i = ib + lane + 64 * k; gk[k] = i < i1 ? G[(long)t * ldg + i] : 0.0; }
            for (int c = 0; c < a.s; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = fma(gk[k], sr[c][lane + 64 * k], acc);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
                if (lane == 0) { double *o = out + (long)t * PCG_LD + c; *o = ib == i0 ? acc : *o + acc; }
            }
        }
    }
}

// T[t][c] = the chunks' partials in ascending order (T: padded_dim(q) rows of PCG_LD, the padding stays zero)
__global__ __launch_bounds__(256) void pcg_gr_finish_kernel(const double *part, long nchunks, int q, int s, double *T) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= q * PCG_LD) return;
    const int c = e & 15;
    if (c >= s) return;
    double acc = 0.0;
    for (long k = 0; k < nchunks; ++k) acc += part[k * q * PCG_LD + e];
    T[e] = acc;
}

// z_i = (r_i - sum_t G[t,i] T[t]) / v_i (q == 0: the Jacobi preconditioner r_i / v_i) and part0 = r.z; one thread per point
__global__ __launch_bounds__(256) void pcg_apply_kernel(const double *G, long ldg, int q, const double *T, PcgVec a) {
    __shared__ double sp[4][PCG_LD];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[PCG_LD], rz[PCG_LD];
#pragma unroll
    for (int c = 0; c < PCG_LD; ++c) { acc[c] = 0.0; rz[c] = 0.0; }
    if (i < a.n) {
        for (int t = 0; t < q; ++t) {
            const double g = G[(long)t * ldg + i];
            const double *tt = T + t * PCG_LD;
#pragma unroll
            for (int c = 0; c < PCG_LD; ++c) acc[c] = fma(g, tt[c], acc[c]);
        }
        const double iv = a.v[i];
#pragma unroll
        for (int c = 0; c < PCG_LD; ++c)
            if (c < a.s) {
                const double r = a.R[i * PCG_LD + c], z = (r - acc[c]) / iv;
                a.Z[i * PCG_LD + c] = z;
                rz[c] = r * z;
            }
    }
    // the block's r.z: lanes by the shuffle tree, then the four waves in order
#pragma unroll
    for (int c = 0; c < PCG_LD; ++c) {
        double w = rz[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
        if (lane == 0) sp[wave][c] = w;
    }
    __syncthreads();
    if (threadIdx.x < PCG_LD) {
        const int c = threadIdx.x;
        a.part0[(long)blockIdx.x * PCG_LD + c] = ((sp[0][c] + sp[1][c]) + sp[2][c]) + sp[3][c];
    }
}

struct PcgLayout { int64_t R, Z, P, AP, T, tpart, part0, part1, state, mv, total; int64_t nblk, tchunks, mv_doubles; };
PcgLayout pcg_layout(int64_t n, int q) {
    PcgLayout l;
    const int64_t qp = q > 0 ? pad128(q) : 0;
    l.nblk = (n + 255) / 256;                 // the apply kernel's blocks (>= the DOT_ROWS blocks of the other partials)
    l.tchunks = (n + PT_CHUNK - 1) / PT_CHUNK;
    l.mv_doubles = mv_auto_split(n, n) > 1 ? mv_split_doubles(n, n, MV_MAXS) : 0;
    int64_t o = 0;
    l.R = o; o += n * PCG_LD; l.Z = o; o += n * PCG_LD; l.P = o; o += n * PCG_LD; l.AP = o; o += n * PCG_LD;
    l.T = o; o += qp * PCG_LD;
    l.tpart = o; o += l.tchunks * q * PCG_LD;
    l.part0 = o; o += l.nblk * PCG_LD; l.part1 = o; o += l.nblk * PCG_LD;
    l.state = o; o += even_up((int64_t)((sizeof(PcgState) + 7) / 8));
    l.mv = o; o += l.mv_doubles;
    l.total = o;
    return l;
}

// Z = M^-1 R for the solver's own vectors, part0 = r.z (blocks of 256 points): G (D^-1 R) in chunks, one potrs per column, the apply kernel.
// T: pad128(q) rows of PCG_LD whose padding is zero
int pcg_precond(fvgp_handle *h, const double *G, int64_t ldg, int q, const double *C, int64_t ldc, const PcgVec &a, double *T, double *tpart,
                int64_t tchunks) {
    hipStream_t st = h->stream;
    if (q > 0) {
        hipLaunchKernelGGL(pcg_gr_kernel, dim3((unsigned)tchunks), dim3(256), 0, st, G, (long)ldg, q, a, tpart);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pcg_gr_finish_kernel, dim3((unsigned)((q * PCG_LD + 255) / 256)), dim3(256), 0, st, tpart, (long)tchunks, q, a.s, T);
        HIPCHK(hipGetLastError());
        // one right-hand side at a time: a column's sweeps are then the same launches whatever s is
        for (int c = 0; c < a.s; ++c) { const int r = potrs_vec(h, C, q, ldc, T + c, 1, PCG_LD, true); if (r) return r; }
    }
    hipLaunchKernelGGL(pcg_apply_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, G, (long)ldg, q, T, a);
    HIPCHK(hipGetLastError());
    return 0;
}

inline int64_t pcg_rec_doubles(int L) { return L > 0 ? (int64_t)PCG_LD * (2 * L + 3) : 0; }      // alpha, beta, rho0, and steps and first (ints) in two rows

struct ApplyLayout { int64_t R, Z, T, tpart, part0, total, tchunks; };
ApplyLayout apply_layout(int64_t n, int q) {
    ApplyLayout l;
    const int64_t qp = q > 0 ? pad128(q) : 0;
    l.tchunks = (n + PT_CHUNK - 1) / PT_CHUNK;
    int64_t o = 0;
    l.R = o; o += n * PCG_LD; l.Z = o; o += n * PCG_LD;
    l.T = o; o += qp * PCG_LD;
    l.tpart = o; o += l.tchunks * q * PCG_LD;
    l.part0 = o; o += (n + 255) / 256 * PCG_LD;
    l.total = o;
    return l;
}

// the one driver of fvgp_hip_pcg (L == 0) and fvgp_hip_pcg_lanczos
int pcg_driver(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
               const double *vdiag, const double *G, int64_t ldg, int q, const double *C, int64_t ldc,
               const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
               double tol, int max_iter, int check_every, int max_restarts,
               double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host,
               int L, double *alpha_host, double *beta_host, int *steps_host, double *rho0_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n <= 0) return -4;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 5, 6, 7); if (rc) return rc;
    if (!vdiag) { fvgp_set_error("pcg: the noise variances are the Jacobi part of the preconditioner and must be given"); return -8; }
    if (!G) q = 0;
    if (q < 0 || q > FVGP_PCG_MAX_RANK) { fvgp_set_error("pcg: rank outside 0 .. FVGP_PCG_MAX_RANK"); return -11; }
    if (q > 0) {
        if (ldg < n) return -10;
        rc = check_square(C, q, ldc, 12, 11, 13);
        if (rc) return rc;
    }
    if (!B) return -14;
    if (s < 1 || s > FVGP_PCG_MAX_RHS) { fvgp_set_error("pcg: 1 .. FVGP_PCG_MAX_RHS right-hand sides per call"); return -16; }
    if (ldb < s) return -15;
    if (!X) return -17;
    if (ldx < s) return -18;
    if (!(tol > 0.0)) return -20;
    if (max_iter < 1) return -21;
    if (check_every < 1) return -22;
    if (max_restarts < 0) return -23;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("pcg: work must be 16-byte aligned"); return -24; }
    if (L < 0 || L > FVGP_LANCZOS_MAX_STEPS) { fvgp_set_error("pcg_lanczos: lanczos_steps outside 0 .. FVGP_LANCZOS_MAX_STEPS"); return -29; }
    if (work_bytes < (pcg_layout(n, q).total + pcg_rec_doubles(L)) * (int64_t)sizeof(double)) {
        fvgp_set_error(L ? "pcg_lanczos: work smaller than fvgp_hip_pcg_lanczos_workspace_bytes(n, rank, lanczos_steps)"
                         : "pcg: work smaller than fvgp_hip_pcg_workspace_bytes(n, rank)");
        return -25;
    }
    if (!iters_host) return -26;
    if (!relres_host) return -27;
    if (!status_host) return -28;
    if (L > 0) {
        if (!alpha_host) return -30;
        if (!beta_host) return -31;
        if (!steps_host) return -32;
        if (!rho0_host) return -33;
    }
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    k.x1 = x; k.n1 = n; k.x2 = x; k.n2 = n; k.vdiag = vdiag;
    const PcgLayout lay = pcg_layout(n, q);
    PcgRec rec{};                                                 // L == 0: every pointer NULL, the scalar kernel records nothing
    if (L > 0) {
        double *rw = work + lay.total;
        rec.alpha = rw; rec.beta = rw + (int64_t)PCG_LD * L; rec.rho0 = rw + 2 * (int64_t)PCG_LD * L;
        rec.steps = reinterpret_cast<int *>(rw + 2 * (int64_t)PCG_LD * L + PCG_LD); rec.first = rec.steps + PCG_LD;
        rec.L = L;
        HIPCHK(hipMemsetAsync(rw, 0, (size_t)pcg_rec_doubles(L) * sizeof(double), h->stream));
    }
    PcgVec a;
    a.R = work + lay.R; a.Z = work + lay.Z; a.P = work + lay.P; a.AP = work + lay.AP;
    a.X = X; a.ldx = ldx; a.B = B; a.ldb = ldb; a.v = vdiag;
    a.st = reinterpret_cast<PcgState *>(work + lay.state);
    a.part0 = work + lay.part0; a.part1 = work + lay.part1;
    a.n = n; a.s = s;
    double *T = work + lay.T, *tpart = work + lay.tpart, *mvws = lay.mv_doubles ? work + lay.mv : nullptr;
    const int64_t qp = q > 0 ? pad128(q) : 0;
    const long nblk = (long)((n + DOT_ROWS - 1) / DOT_ROWS), nblk_apply = (long)((n + 255) / 256);
    const dim3 gdot((unsigned)nblk), gdir((unsigned)((n * PCG_LD + 255) / 256));
    hipStream_t st = h->stream;

    auto matvec = [&](const double *V, int64_t ldv) -> int {     // AP = (K + D) V
        return launch_kmatvec(h, k, V, ldv, s, a.AP, PCG_LD, mvws, lay.mv_doubles, true);
    };
    auto scalar = [&](const PcgVec &v, long nb, int mode) -> int {
        hipLaunchKernelGGL(pcg_scalar_kernel, dim3(1), dim3(256), 0, st, v, nb, mode, tol, max_iter, rec);
        HIPCHK(hipGetLastError());
        return 0;
    };
    auto precond = [&]() -> int { return pcg_precond(h, G, ldg, q, C, ldc, a, T, tpart, lay.tchunks); };
    PcgVec a1 = a; a1.part1 = a.part0;                            // (a scalar step that reads one partial array)

    if (qp) HIPCHK(hipMemsetAsync(T, 0, (size_t)qp * PCG_LD * sizeof(double), st));
    if (warm) {
        rc = matvec(X, ldx); if (rc) return rc;
        hipLaunchKernelGGL(pcg_resid_kernel, gdot, dim3(256), 0, st, a, 1);
        HIPCHK(hipGetLastError());
        rc = scalar(a, nblk, SC_INIT); if (rc) return rc;
        hipLaunchKernelGGL(pcg_zero_cols_kernel, gdir, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(pcg_resid_kernel, gdot, dim3(256), 0, st, a, 0);
        HIPCHK(hipGetLastError());
        rc = scalar(a1, nblk, SC_INIT); if (rc) return rc;
    }
    rc = precond(); if (rc) return rc;
    rc = scalar(a1, nblk_apply, SC_RHO0); if (rc) return rc;
    hipLaunchKernelGGL(pcg_dir_kernel, gdir, dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());

    PcgState hs;
    int restarts[PCG_LD] = {0};
    bool final_col[PCG_LD] = {false};
    // no column iterates more than max_iter times in all; each restart round ends when every column is frozen
    for (;;) {
        for (int it = 0;; ++it) {
            if (it % check_every == 0) {
                HIPCHK(hipMemcpyAsync(&hs, a.st, sizeof(hs), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                bool any = false;
                for (int c = 0; c < s; ++c) any = any || hs.active[c];
                if (!any) break;
            }
            rc = matvec(a.P, PCG_LD); if (rc) return rc;
            hipLaunchKernelGGL(pcg_dot_kernel, gdot, dim3(256), 0, st, a.P, a.AP, (long)n, s, a.part0);
            HIPCHK(hipGetLastError());
            rc = scalar(a1, nblk, SC_ALPHA); if (rc) return rc;
            hipLaunchKernelGGL(pcg_axpy_kernel, gdot, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            rc = scalar(a1, nblk, SC_RNORM); if (rc) return rc;
            rc = precond(); if (rc) return rc;
            rc = scalar(a1, nblk_apply, SC_BETA); if (rc) return rc;
            hipLaunchKernelGGL(pcg_dir_kernel, gdir, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
        }
        // every column is frozen: the true residual b - A x decides
        rc = matvec(X, ldx); if (rc) return rc;
        hipLaunchKernelGGL(pcg_resid_kernel, gdot, dim3(256), 0, st, a, 2);
        HIPCHK(hipGetLastError());
        rc = scalar(a, nblk, SC_TRUE); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(&hs, a.st, sizeof(hs), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool again = false;
        for (int c = 0; c < s; ++c) {
            if (final_col[c]) continue;
            iters_host[c] = hs.iters[c]; relres_host[c] = hs.relres[c];
            if (hs.relres[c] <= tol) { status_host[c] = 0; final_col[c] = true; }
            else if (hs.code[c] == 2) { status_host[c] = 2; final_col[c] = true; }
            else if (hs.code[c] == 1 || restarts[c] >= max_restarts || !(hs.relres[c] == hs.relres[c])) { status_host[c] = 1; final_col[c] = true; }
            else { restarts[c] += 1; hs.restart[c] = 1; again = true; }
        }
        if (!again) break;
        HIPCHK(hipMemcpyAsync(a.st->restart, hs.restart, sizeof(hs.restart), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                         // (hs is on the stack: the copy must have read it before it changes)
        rc = precond(); if (rc) return rc;
        rc = scalar(a1, nblk_apply, SC_RESTART); if (rc) return rc;
        hipLaunchKernelGGL(pcg_dir_kernel, gdir, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    if (L > 0) {
        HIPCHK(hipMemcpyAsync(alpha_host, rec.alpha, (size_t)s * L * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(beta_host, rec.beta, (size_t)s * L * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rho0_host, rec.rho0, (size_t)s * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(steps_host, rec.steps, (size_t)s * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t fvgp_hip_kmatvec_workspace_bytes(int64_t n1, int64_t n2, int s) {
    if (n1 < 1 || n2 < 1 || s < 1) return -1;
    return mv_split_doubles(n1, n2, s) * (int64_t)sizeof(double);
}

int fvgp_hip_kmatvec(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2, int d,
                     const double *theta, int ntheta, const double *vdiag, const double *B, int64_t ldb, int s,
                     double *Y, int64_t ldy, double *work, int64_t work_bytes) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x1) return -3;
    if (n1 <= 0) return -4;
    if (!x2) return -5;
    if (n2 <= 0) return -6;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 7, 8, 9); if (rc) return rc;
    if (vdiag && n1 != n2) { fvgp_set_error("kmatvec: vdiag needs n1 == n2"); return -10; }
    if (!B) return -11;
    if (s < 1) return -13;
    if (ldb < s) return -12;
    if (!Y) return -14;
    if (ldy < s) return -15;
    if (work && ((uintptr_t)work & 7)) return -16;
    if (work_bytes < 0) return -17;
    if ((n1 + 63) / 64 > 0x7fffffffLL) return -4;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    k.x1 = x1; k.n1 = n1; k.x2 = x2; k.n2 = n2; k.vdiag = vdiag;
    rc = launch_kmatvec(h, k, B, ldb, s, Y, ldy, work, work ? work_bytes / 8 : 0, false);
    return rc == -1 ? -17 : rc;
}

int64_t fvgp_hip_pchol_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 1) return -1;
    return (pivot_layout(0, n, 2).end + even_up(n)) * (int64_t)sizeof(double);      // the core's pieces, then the residual diagonal
}

int fvgp_hip_pchol(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                   int q, double tol, double *G, int64_t ldg, int64_t *piv_out, double *resid_diag_out,
                   double *work, int64_t work_bytes, int *rank_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x) return -3;
    if (n <= 0) return -4;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 5, 6, 7); if (rc) return rc;
    if (q < 1) return -8;
    if (!(tol >= 0.0)) return -9;
    if (!G) return -10;
    if (ldg < n) return -11;
    if (!piv_out) return -12;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("pchol: work must be 16-byte aligned"); return -14; }
    if (work_bytes < fvgp_hip_pchol_workspace_bytes(n, q)) { fvgp_set_error("pchol: work smaller than fvgp_hip_pchol_workspace_bytes(n, q)"); return -15; }
    if (!rank_host) return -16;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    const PivotLayout lay = pivot_layout(0, n, 2);
    // selection's run with the data as their own candidates: no conditioning, no noise, d = sigma^2 at the start, G the caller's
    PivotArgs a{};
    a.x = x; a.xc = x; a.var = work + lay.end; a.G = G; a.ldg_in = ldg;
    a.slot = work + lay.slot; a.best = work + lay.best;
    a.st = reinterpret_cast<PivotState *>(work + lay.state);
    a.taken = reinterpret_cast<unsigned char *>(work + lay.taken);
    a.idx = reinterpret_cast<long long *>(piv_out);
    a.n = n; a.P = n; a.cn = n; a.d = d; a.q = q; a.sig = k.sig; a.tol = tol;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
    const unsigned nb = (unsigned)((n + 255) / 256);
    // the rows an exhausted run never reaches are zero rows: G is cleared first, inside its (q, n) view only
    for (int64_t r0 = 0; r0 < q; r0 += 1024) {
        const int64_t rows = q - r0 < 1024 ? q - r0 : 1024;
        hipLaunchKernelGGL(mf_zero_rows_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, h->stream, G + r0 * ldg, (long)ldg,
                           (long)rows, (long)n);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(pivot_init_kernel, dim3(nb), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < q; ++t) {
        a.t = t;
        hipLaunchKernelGGL(pivot_pick_kernel, dim3(1), dim3(256), 0, h->stream, a);
        HIPCHK(hipGetLastError());
        dispatch_kind(k.kind, [&](auto KIND) {
            hipLaunchKernelGGL((pivot_downdate_kernel<decltype(KIND)::value, false>), dim3(nb), dim3(256), 0, h->stream, a, 0L);
        });
        HIPCHK(hipGetLastError());
    }
    if (resid_diag_out)
        HIPCHK(hipMemcpyAsync(resid_diag_out, a.var, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    long long done = 0;                                           // 0, or 1 + the step that found nothing left to pick
    HIPCHK(hipMemcpyAsync(&done, &a.st->done, sizeof(done), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *rank_host = done ? (int)done - 1 : q;
    return 0;
}

int64_t fvgp_hip_precond_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 1) return -1;
    return (n + PF_CHUNK - 1) / PF_CHUNK * (int64_t)q * q * (int64_t)sizeof(double);
}

int fvgp_hip_precond_factor(fvgp_handle *h, const double *G, int64_t ldg, int q, int64_t n, const double *vdiag,
                            double *C, int64_t ldc, double *work, int64_t work_bytes, int *info_host) {
    if (!h) return -1;
    if (!G) return -2;
    if (q < 1 || q > FVGP_PCG_MAX_RANK) { fvgp_set_error("precond_factor: rank outside 1 .. FVGP_PCG_MAX_RANK"); return -4; }
    if (n <= 0) return -5;
    if (ldg < n) return -3;
    if (!vdiag) return -6;
    int rc = check_square(C, q, ldc, 7, 4, 8);
    if (rc) return rc;
    if (!work || ((uintptr_t)work & 7)) return -9;
    if (work_bytes < fvgp_hip_precond_workspace_bytes(n, q)) { fvgp_set_error("precond_factor: work smaller than fvgp_hip_precond_workspace_bytes(n, q)"); return -10; }
    if (!info_host) return -11;
    HIPCHK(hipSetDevice(h->device));
    const int64_t nch = (n + PF_CHUNK - 1) / PF_CHUNK;
    if (nch > 65535) { fvgp_set_error("precond_factor: n too large"); return -5; }
    const int nt = (q + 15) / 16;
    hipLaunchKernelGGL(pf_gram_kernel, dim3((unsigned)(nt * nt), (unsigned)nch), dim3(256), 0, h->stream, G, (long)ldg, q, (long)n, vdiag, work);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pf_finish_kernel, dim3((unsigned)(((int64_t)q * q + 255) / 256)), dim3(256), 0, h->stream, work, (long)nch, q, C, (long)ldc);
    HIPCHK(hipGetLastError());
    rc = launch_pad_identity(h, C, q, pad128(q), ldc); if (rc) return rc;
    return potrf_driver(h, C, q, ldc, info_host);
}

int64_t fvgp_hip_pcg_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 0) return -1;
    return pcg_layout(n, q).total * (int64_t)sizeof(double);
}

int fvgp_hip_pcg(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                 const double *vdiag, const double *G, int64_t ldg, int q, const double *C, int64_t ldc,
                 const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                 double tol, int max_iter, int check_every, int max_restarts,
                 double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host) {
    return pcg_driver(h, kernel_id, x, n, d, theta, ntheta, vdiag, G, ldg, q, C, ldc, B, ldb, s, X, ldx, warm, tol, max_iter, check_every,
                      max_restarts, work, work_bytes, iters_host, relres_host, status_host, 0, nullptr, nullptr, nullptr, nullptr);
}

int64_t fvgp_hip_pcg_lanczos_workspace_bytes(int64_t n, int q, int lanczos_steps) {
    if (n < 1 || q < 0 || lanczos_steps < 0 || lanczos_steps > FVGP_LANCZOS_MAX_STEPS) return -1;
    return (pcg_layout(n, q).total + pcg_rec_doubles(lanczos_steps)) * (int64_t)sizeof(double);
}

int fvgp_hip_pcg_lanczos(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                         const double *vdiag, const double *G, int64_t ldg, int q, const double *C, int64_t ldc,
                         const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                         double tol, int max_iter, int check_every, int max_restarts,
                         double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host,
                         int lanczos_steps, double *alpha_host, double *beta_host, int *steps_host, double *rho0_host) {
    return pcg_driver(h, kernel_id, x, n, d, theta, ntheta, vdiag, G, ldg, q, C, ldc, B, ldb, s, X, ldx, warm, tol, max_iter, check_every,
                      max_restarts, work, work_bytes, iters_host, relres_host, status_host, lanczos_steps, alpha_host, beta_host, steps_host,
                      rho0_host);
}

int64_t fvgp_hip_kgrad_form_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 1 || n2 < 1) return -1;
    const int64_t park = (n1 + 63) / 64 < 512 && mv_chunks(n2) > 1 ? mv_chunks(n2) * n1 * KG_H : 0;
    return (kg_base_doubles(n1) + park) * (int64_t)sizeof(double);
}

int fvgp_hip_kgrad_form(fvgp_handle *h, int kernel_id, const double *x1, int64_t n1, const double *x2, int64_t n2, int d,
                        const double *theta, int ntheta, const double *U, int64_t ldu, const double *W, int64_t ldw, int s,
                        double *work, int64_t work_bytes, double *out_host) {
    if (!h) return -1;
    if (!kernel_id_known(kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!x1) return -3;
    if (n1 <= 0 || (n1 + 63) / 64 > 0x7fffffffLL) return -4;
    if (!x2) return -5;
    if (n2 <= 0) return -6;
    int rc = check_kernel_args(kernel_id, d, theta, ntheta, 7, 8, 9); if (rc) return rc;
    if (!U) return -10;
    if (s < 1 || s > FVGP_PCG_MAX_RHS) { fvgp_set_error("kgrad_form: 1 .. FVGP_PCG_MAX_RHS columns per call"); return -14; }
    if (ldu < s) return -11;
    if (!W) return -12;
    if (ldw < s) return -13;
    if (!work || ((uintptr_t)work & 7)) return -15;
    if (work_bytes < kg_base_doubles(n1) * (int64_t)sizeof(double)) { fvgp_set_error("kgrad_form: work smaller than fvgp_hip_kgrad_form_workspace_bytes(n1, n2)"); return -16; }
    if (!out_host) return -17;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    KgArgs a;
    a.x1 = x1; a.x2 = x2; a.U = U; a.W = W;
    a.n1 = n1; a.n2 = n2; a.ldu = ldu; a.ldw = ldw; a.nchunks = mv_chunks(n2);
    a.d = d; a.iso = k.iso ? 1 : 0; a.sig = k.sig;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
    const int nh = kernel_param_count(kernel_id, d);
    const int64_t bx = (n1 + 63) / 64;
    double *out = work, *bpart = work + KG_H, *park = work + kg_base_doubles(n1);
    a.bpart = bpart;
    // the chunk ranges are dealt over gridDim.y by the product's rule, where `work` has room for the chunk sums (the bits are the same)
    int64_t gy = h->matvec_split == 0 ? mv_auto_split(n1, n2) : h->matvec_split;
    if (gy > a.nchunks) gy = a.nchunks;
    if (gy > 65535) gy = 65535;
    const bool split = gy > 1 && work_bytes / 8 >= kg_base_doubles(n1) + a.nchunks * n1 * KG_H;
    a.park = split ? park : nullptr;
    a.cpy = split ? (a.nchunks + gy - 1) / gy : a.nchunks;
    const dim3 grid((unsigned)bx, split ? (unsigned)((a.nchunks + a.cpy - 1) / a.cpy) : 1u);
    for (int c0 = 0; c0 < s;) {
        const int left = s - c0;
        const int S = mv_group(left);
        a.c0 = c0; a.sc = left < S ? left : S;
        dispatch_kind_dim(k.kind, d, [&](auto KIND, auto D) {
            constexpr int KK = decltype(KIND)::value, DV = decltype(D)::value;
            switch (S) {
                case 16: kg_launch<KK, DV, 16>(h, a, grid); break;
                case 8: kg_launch<KK, DV, 8>(h, a, grid); break;
                case 4: kg_launch<KK, DV, 4>(h, a, grid); break;
                default: kg_launch<KK, DV, 1>(h, a, grid); break;
            }
        });
        HIPCHK(hipGetLastError());
        if (split) {
            hipLaunchKernelGGL(kgrad_rows_kernel, dim3((unsigned)bx), dim3(64), 0, h->stream, a);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(kgrad_sum_kernel, dim3(1), dim3(64), 0, h->stream, (const double *)bpart, (long)bx, nh, c0 == 0 ? 1 : 0, out);
        HIPCHK(hipGetLastError());
        c0 += a.sc;
    }
    HIPCHK(hipMemcpyAsync(out_host, out, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int fvgp_hip_precond_probes(fvgp_handle *h, uint64_t seed, uint64_t stream, int64_t col0, const double *G, int64_t ldg, int q,
                            int64_t n, const double *vdiag, double *Z, int64_t ldz, int s) {
    constexpr int64_t TWO32 = (int64_t)1 << 32;
    if (!h) return -1;
    if (stream >> 63) { fvgp_set_error("precond_probes: the streams 2 stream and 2 stream + 1 must fit 64 bits"); return -3; }
    if (s < 1 || s > FVGP_PCG_MAX_RHS) { fvgp_set_error("precond_probes: 1 .. FVGP_PCG_MAX_RHS columns per call"); return -12; }
    if (col0 < 0 || col0 > TWO32 || s > TWO32 - col0) { fvgp_set_error("precond_probes: column indices must stay below 2^32"); return -4; }
    if (!G) q = 0;
    if (q < 0 || q > FVGP_PCG_MAX_RANK) { fvgp_set_error("precond_probes: rank outside 0 .. FVGP_PCG_MAX_RANK"); return -7; }
    if (n <= 0 || n > TWO32) return -8;
    if (q > 0 && ldg < n) return -6;
    if (!vdiag) return -9;
    if (!Z) return -10;
    if (ldz < s) return -11;
    HIPCHK(hipSetDevice(h->device));
    ProbeArgs a;
    const uint64_t se = 2 * stream, sg = 2 * stream + 1;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.e0 = (uint32_t)se; a.e1 = (uint32_t)(se >> 32); a.g0 = (uint32_t)sg; a.g1 = (uint32_t)(sg >> 32);
    a.G = G; a.v = vdiag; a.Z = Z; a.ldg = ldg; a.n = n; a.ldz = ldz; a.col0 = col0; a.q = q; a.s = s;
    hipLaunchKernelGGL(precond_probes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

int64_t fvgp_hip_precond_apply_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 0) return -1;
    return apply_layout(n, q).total * (int64_t)sizeof(double);
}

int fvgp_hip_precond_apply(fvgp_handle *h, const double *G, int64_t ldg, int q, const double *C, int64_t ldc, int64_t n,
                           const double *vdiag, const double *R, int64_t ldr, int s, double *W, int64_t ldw,
                           double *work, int64_t work_bytes) {
    if (!h) return -1;
    if (!G) q = 0;
    if (q < 0 || q > FVGP_PCG_MAX_RANK) { fvgp_set_error("precond_apply: rank outside 0 .. FVGP_PCG_MAX_RANK"); return -4; }
    if (n <= 0) return -7;
    if (q > 0) {
        if (ldg < n) return -3;
        const int rc = check_square(C, q, ldc, 5, 4, 6);
        if (rc) return rc;
    }
    if (!vdiag) return -8;
    if (!R) return -9;
    if (s < 1 || s > FVGP_PCG_MAX_RHS) { fvgp_set_error("precond_apply: 1 .. FVGP_PCG_MAX_RHS columns per call"); return -11; }
    if (ldr < s) return -10;
    if (!W) return -12;
    if (ldw < s) return -13;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("precond_apply: work must be 16-byte aligned"); return -14; }
    if (work_bytes < fvgp_hip_precond_apply_workspace_bytes(n, q)) { fvgp_set_error("precond_apply: work smaller than fvgp_hip_precond_apply_workspace_bytes(n, rank)"); return -15; }
    HIPCHK(hipSetDevice(h->device));
    const ApplyLayout lay = apply_layout(n, q);
    PcgVec a{};
    a.R = work + lay.R; a.Z = work + lay.Z; a.v = vdiag; a.part0 = work + lay.part0; a.n = n; a.s = s;
    const int64_t qp = q > 0 ? pad128(q) : 0;
    const dim3 gcopy((unsigned)((n * PCG_LD + 255) / 256));
    if (qp) HIPCHK(hipMemsetAsync(work + lay.T, 0, (size_t)qp * PCG_LD * sizeof(double), h->stream));
    hipLaunchKernelGGL(mf_copy_cols_kernel, gcopy, dim3(256), 0, h->stream, R, (long)ldr, a.R, (long)PCG_LD, (long)n, s);
    HIPCHK(hipGetLastError());
    const int rc = pcg_precond(h, G, ldg, q, C, ldc, a, work + lay.T, work + lay.tpart, lay.tchunks); if (rc) return rc;
    hipLaunchKernelGGL(mf_copy_cols_kernel, gcopy, dim3(256), 0, h->stream, (const double *)a.Z, (long)PCG_LD, W, (long)ldw, (long)n, s);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
