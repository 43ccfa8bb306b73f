// The two passes over the entries of K(x1, x2) that the matrix-free path makes; the solver that calls the first is
// matrix_free.hip.  The two kernels walk the chunks of x2 in the same way and are nevertheless written out twice: a walk shared through
// an inlined function changed the registers of both (profiles/r17_matvec_walk_ab.txt).
// fvgp_hip_kmatvec   Y = K(x1, x2) B + diag(v) B.  select_cross_kernel widened: lanes along 64 output rows, the x2 rows and S entries of
//     B per row staged in LDS, S accumulator pairs per lane filled by slice_rows, so one exp (plus the rsq of the Matern kinds) serves S
//     columns.  The order of every sum is a function of n2 alone; v_i B_ic enters as the last fused multiply-add.  A
//     workgroup that walks all chunks (gridDim.y == 1) and a launch that deals chunk ranges over gridDim.y, parks the per-chunk sums and
//     adds them in a second pass give the same bits.
// fvgp_hip_kgrad_form   sum_c U[:, c]^T (dK / dtheta_j) W[:, c] for every j in ONE pass over the kernel entries: the same walk (W staged,
//     U[i, 0 .. S) in registers), per entry one radial_grad, S fused multiply-adds for t = sum_c U[i][c] W[k][c] and one per
//     hyperparameter; the rows of a block by a halving tree, the blocks in ascending order by one small kernel: no atomics.
// Both entries split by ONE rule (mv_plan): the chunk ranges dealt over gridDim.y, the chunk sums parked or not.
#include "radial.h"
#include "kernel_family.h"
#include "reduce.h"
#include "slice_sum.h"
#include <math.h>

namespace {

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

// ---------------------------------------------------------------------------------------------------------------- the one split plan
// what MvArgs and KgArgs both take from the kernel's description (each struct keeps its own field order: DESIGN 21 on the kernels' registers)
template <class A>
void kmat_fill(A &a, const KmatDesc &k) {
    a.x1 = k.x1; a.x2 = k.x2; a.n1 = k.n1; a.n2 = k.n2; a.nchunks = mv_chunks(k.n2); a.d = k.d; a.sig = k.sig;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
}

// gy chunk ranges of cpy chunks over gridDim.y: gy from "matvec_split" or the shape; split (the chunk sums parked, a second pass) only
// where the caller's `room` doubles hold `per` of them for every (chunk, row), else one workgroup walks all chunks: the same bits
struct MvPlan { int64_t gy, cpy; bool split; dim3 grid; };
MvPlan mv_plan(const fvgp_handle *h, int64_t n1, int64_t n2, int64_t room, int per) {
    const int64_t nchunks = mv_chunks(n2);
    MvPlan p;
    p.gy = h->matvec_split == 0 ? mv_auto_split(n1, n2) : h->matvec_split;
    if (p.gy > nchunks) p.gy = nchunks;
    if (p.gy > 65535) p.gy = 65535;
    p.split = p.gy > 1 && room >= nchunks * n1 * per;
    p.cpy = p.split ? (nchunks + p.gy - 1) / p.gy : nchunks;
    p.grid = dim3((unsigned)((n1 + 63) / 64), p.split ? (unsigned)((nchunks + p.cpy - 1) / p.cpy) : 1u);
    return p;
}

// f(std::integral_constant<int, S>) for the column group mv_group chose
template <class F>
inline void dispatch_group(int S, F &&f) {
    switch (S) {
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 1>{}); break;
    }
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
            const double w = wave_sum(tot[hh]);
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

// fvgp_hip_kgrad_form's workspace: the result row, a row of sums per block of 64 rows; `full`: what the size query adds behind them for
// the split plan, every chunk's sums where the product deals chunk ranges by itself (the entry hands the plan what it finds there)
struct KgWs { double *out, *bpart; };
inline KgWs kg_layout(Carve &c, int64_t n1, int64_t n2, bool full) {
    const KgWs l{c.take<double>(KG_H, sizeof(double)), c.take<double>((n1 + 63) / 64 * KG_H, sizeof(double))};
    if (full && (n1 + 63) / 64 < 512 && mv_chunks(n2) > 1) c.take<double>(mv_chunks(n2) * n1 * KG_H, sizeof(double));
    return l;
}

}  // namespace

// Y[:, 0 .. s) = K B + diag(v) B.  k: x1, n1, x2, n2, d, kind, sig, invl, vdiag.  work_doubles < what a forced split needs: -1 unless
// `fallback` (then the unsplit form, which has the same bits)
int launch_kmatvec(fvgp_handle *h, const KmatDesc &k, const double *B, int64_t ldb, int s, double *Y, int64_t ldy, double *work,
                   int64_t work_doubles, bool fallback) {
    MvArgs a;
    kmat_fill(a, k);
    a.B = B; a.ldb = ldb; a.v = k.vdiag; a.Y = Y; a.ldy = ldy;
    for (int c0 = 0; c0 < s; c0 += a.sc) {
        const int S = mv_group(s - c0);
        a.c0 = c0; a.sc = s - c0 < S ? s - c0 : S;
        const MvPlan p = mv_plan(h, k.n1, k.n2, work ? work_doubles : 0, S);
        if (p.gy > 1 && !p.split && h->matvec_split > 1 && !fallback) {
            fvgp_set_error("kmatvec: work smaller than fvgp_hip_kmatvec_workspace_bytes(n1, n2, s)");
            return -1;
        }
        a.part = p.split ? work : nullptr;
        a.cpy = p.cpy;
        dispatch_kind_dim(k.kind, k.d, [&](auto KIND, auto D) {
            dispatch_group(S, [&](auto SS) {
                hipLaunchKernelGGL((kmatvec_kernel<decltype(KIND)::value, decltype(D)::value, decltype(SS)::value>), p.grid, dim3(256), 0, h->stream, a);
            });
        });
        HIPCHK(hipGetLastError());
        if (p.split) HIPLAUNCH(kmatvec_reduce_kernel, dim3((unsigned)((k.n1 * a.sc + 255) / 256)), dim3(256), h->stream, a, S);
    }
    return 0;
}

extern "C" {

int64_t fvgp_hip_kmatvec_workspace_bytes(int64_t n1, int64_t n2, int s) {
    if (n1 < 1 || n2 < 1 || s < 1) return -1;
    return carve_bytes(mv_park_layout, n1, n2, s);
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
    rc = launch_kmatvec(h, k, B, ldb, s, Y, ldy, work, work_bytes / 8, false);
    return rc == -1 ? -17 : rc;
}

int64_t fvgp_hip_kgrad_form_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 1 || n2 < 1) return -1;
    return carve_bytes(kg_layout, n1, n2, true);
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
    Carve c(work); const KgWs l = kg_layout(c, n1, n2, false);
    if (work_bytes < c.bytes()) { fvgp_set_error("kgrad_form: work smaller than fvgp_hip_kgrad_form_workspace_bytes(n1, n2)"); return -16; }
    if (!out_host) return -17;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    k.x1 = x1; k.n1 = n1; k.x2 = x2; k.n2 = n2;
    const int nh = kernel_param_count(kernel_id, d);
    const long bx = (long)((n1 + 63) / 64);
    // the product's plan, split where `work` has room for the chunk sums behind the blocks' (the bits are the same either way)
    const int64_t left = (work_bytes - c.bytes()) / (int64_t)sizeof(double);
    double *out = l.out, *bpart = l.bpart, *park = c.take<double>(left, sizeof(double));
    const MvPlan p = mv_plan(h, n1, n2, left, KG_H);
    KgArgs a;
    kmat_fill(a, k);
    a.cpy = p.cpy;
    a.W = W; a.ldw = ldw; a.park = p.split ? park : nullptr;
    a.U = U; a.ldu = ldu; a.iso = k.iso ? 1 : 0; a.bpart = bpart;
    for (int c0 = 0; c0 < s; c0 += a.sc) {
        const int S = mv_group(s - c0);
        a.c0 = c0; a.sc = s - c0 < S ? s - c0 : S;
        dispatch_kind_dim(k.kind, d, [&](auto KIND, auto D) {
            dispatch_group(S, [&](auto SS) {
                hipLaunchKernelGGL((kgrad_form_kernel<decltype(KIND)::value, decltype(D)::value, decltype(SS)::value>), p.grid, dim3(256), 0, h->stream, a);
            });
        });
        HIPCHK(hipGetLastError());
        if (p.split) HIPLAUNCH(kgrad_rows_kernel, dim3((unsigned)bx), dim3(64), h->stream, a);
        HIPLAUNCH(kgrad_sum_kernel, dim3(1), dim3(64), h->stream, (const double *)bpart, bx, nh, c0 == 0 ? 1 : 0, out);
    }
    HIPCHK(hipMemcpyAsync(out_host, out, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
