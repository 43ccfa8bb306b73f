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
#include "radial.h"
#include "kernel_family.h"
#include "slice_sum.h"
#include "pivot.h"
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
__global__ __launch_bounds__(256) void pcg_scalar_kernel(PcgVec a, long nblk, int mode, double tol, int max_iter) {
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
            break;
        }
        case SC_RHO0:                                         // v0 = r.z
            if (st.active[c]) { st.rho[c] = v0; st.beta[c] = 0.0; if (!(v0 > 0.0) || isinf(v0)) { st.active[c] = 0; st.code[c] = 2; } }
            break;
        case SC_ALPHA:                                        // v0 = p.Ap
            if (st.active[c]) {
                if (!(v0 > 0.0) || isinf(v0)) { st.active[c] = 0; st.code[c] = 2; }
                else st.alpha[c] = st.rho[c] / v0;
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
                else { st.beta[c] = v0 / st.rho[c]; st.rho[c] = v0; }
            }
            break;
        case SC_TRUE:                                         // v1 = |b - A x|^2
            st.relres[c] = st.bnorm[c] > 0.0 ? sqrt(v1) / st.bnorm[c] : 0.0;
            st.rn2[c] = v1;
            break;
        default:                                              // SC_RESTART: v0 = r.z of the true residual
            if (st.restart[c]) {
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
    if (work_bytes < fvgp_hip_pcg_workspace_bytes(n, q)) { fvgp_set_error("pcg: work smaller than fvgp_hip_pcg_workspace_bytes(n, rank)"); return -25; }
    if (!iters_host) return -26;
    if (!relres_host) return -27;
    if (!status_host) return -28;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    k.x1 = x; k.n1 = n; k.x2 = x; k.n2 = n; k.vdiag = vdiag;
    const PcgLayout lay = pcg_layout(n, q);
    PcgVec a;
    a.R = work + lay.R; a.Z = work + lay.Z; a.P = work + lay.P; a.AP = work + lay.AP;
    a.X = X; a.ldx = ldx; a.B = B; a.ldb = ldb; a.v = vdiag;
    a.st = reinterpret_cast<PcgState *>(work + lay.state);
    a.part0 = work + lay.part0; a.part1 = work + lay.part1;
    a.n = n; a.s = s;
    double *T = work + lay.T, *tpart = work + lay.tpart, *mvws = lay.mv_doubles ? work + lay.mv : nullptr;
    const int64_t qp = q > 0 ? pad128(q) : 0;
    const long nblk = (long)((n + DOT_ROWS - 1) / DOT_ROWS), nblk_apply = (long)((n + 255) / 256);
    const dim3 gdot((unsigned)nblk), gapply((unsigned)nblk_apply), gdir((unsigned)((n * PCG_LD + 255) / 256));
    hipStream_t st = h->stream;

    auto matvec = [&](const double *V, int64_t ldv) -> int {     // AP = (K + D) V
        return launch_kmatvec(h, k, V, ldv, s, a.AP, PCG_LD, mvws, lay.mv_doubles, true);
    };
    auto scalar = [&](const PcgVec &v, long nb, int mode) -> int {
        hipLaunchKernelGGL(pcg_scalar_kernel, dim3(1), dim3(256), 0, st, v, nb, mode, tol, max_iter);
        HIPCHK(hipGetLastError());
        return 0;
    };
    auto precond = [&]() -> int {                                // Z = M^-1 R, part0 = r.z (nblk_apply partials)
        if (q > 0) {
            hipLaunchKernelGGL(pcg_gr_kernel, dim3((unsigned)lay.tchunks), dim3(256), 0, st, G, (long)ldg, q, a, tpart);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(pcg_gr_finish_kernel, dim3((unsigned)((q * PCG_LD + 255) / 256)), dim3(256), 0, st, tpart, (long)lay.tchunks, q, s, T);
            HIPCHK(hipGetLastError());
            // one right-hand side at a time: a column's sweeps are then the same launches whatever s is
            for (int c = 0; c < s; ++c) { const int r = potrs_vec(h, C, q, ldc, T + c, 1, PCG_LD, true); if (r) return r; }
        }
        hipLaunchKernelGGL(pcg_apply_kernel, gapply, dim3(256), 0, st, G, (long)ldg, q, T, a);
        HIPCHK(hipGetLastError());
        return 0;
    };
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
    return 0;
}

}  // extern "C"
