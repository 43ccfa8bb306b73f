// Solves with K(theta) + V without the matrix: the pivoted-Cholesky preconditioner and the preconditioned conjugate gradients
// whose scalars stay on the device.  The product with a block of vectors, launch_kmatvec, and the gradient's bilinear form are matvec.hip.
//
// fvgp_hip_pchol     greedy pivoted Cholesky of K(x, x), q steps enqueued at once: selection's greedy pivot core (pivot.h) with the
//     data as their own candidates, no conditioning (pivot_downdate_kernel<KIND, CROSS = false>) and no noise.
// fvgp_hip_precond_factor   C = I + G D^-1 G^T in fixed-order chunks of PF_CHUNK points, factored by potrf_driver.
// fvgp_hip_pcg       s <= 16 independent recurrences that share the matvec; every vector kernel reads the per-column state
//     (active, alpha, beta) from device memory, the host reads the status words every `check_every` iterations.
// The stochastic log-likelihood:
// fvgp_hip_precond_probes   Z = D^1/2 eps + G^T eta from the normals of normal.h;  fvgp_hip_precond_apply   the solver's M^-1 on its own;
// fvgp_hip_pcg_lanczos      the solver with the coefficients of every column's first recurrence recorded (one driver serves both entries).
#include "radial.h"
#include "kernel_family.h"
#include "reduce.h"
#include "slice_sum.h"
#include "pivot.h"
#include "normal.h"
#include "../../include/fvgp_hip_nn.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int PCG_LD = FVGP_PCG_MAX_RHS;             // row stride of the solver's own vectors
constexpr int PF_CHUNK = 8192;                       // points per partial Gram sum of precond_factor
constexpr int PT_CHUNK = 4096;                       // points per partial of G (D^-1 R)
constexpr int DOT_ROWS = 1024;                       // rows per partial of the dot products

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

// sh[a][c] <- the sum over g of sh[a][16 g + c] for the NA arrays at once: a halving tree over g, 256 threads
template <int NA>
__device__ __forceinline__ void tree_over_g(double (&sh)[NA][256], int tid) {
    __syncthreads();
    for (int off = 128; off >= 16; off >>= 1) {
        if (tid < off)
            for (int a = 0; a < NA; ++a) sh[a][tid] += sh[a][tid + off];
        __syncthreads();
    }
}

// the block's share of sum_i a_i b_i for every column: thread (g, c) adds rows g, g + 16, .. of the DOT_ROWS, then the tree over g
__device__ __forceinline__ void dot_block(double acc, double *out, int tid, bool live) {
    __shared__ double sh[1][256];
    sh[0][tid] = acc;
    tree_over_g(sh, tid);
    if (tid < 16 && live) out[(long)blockIdx.x * PCG_LD + tid] = sh[0][tid];
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
    tree_over_g(sh, tid);
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
                acc = wave_sum(acc);
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
        const double w = wave_sum(rz[c]);
        if (lane == 0) sp[wave][c] = w;
    }
    __syncthreads();
    if (threadIdx.x < PCG_LD) {
        const int c = threadIdx.x;
        a.part0[(long)blockIdx.x * PCG_LD + c] = ((sp[0][c] + sp[1][c]) + sp[2][c]) + sp[3][c];
    }
}

// a piece of `rows` rows of PCG_LD doubles (128 bytes each: every such piece begins 16-byte aligned behind others of its kind)
inline double *mf_rows(Carve &c, int64_t rows) { return c.take<double>(rows * PCG_LD, sizeof(double)); }
// the pieces the entries of this unit share: R and Z (n rows), behind them the solver's P and AP; the intermediate T = W R of the
// nearest-neighbour preconditioner; part0 (r.z by blocks of 256 points: >= the DOT_ROWS blocks of the solver's other partials)
inline void vec_layout(Carve &c, int64_t n, bool solver, PcgVec &a) {
    a.R = mf_rows(c, n); a.Z = mf_rows(c, n);
    if (solver) { a.P = mf_rows(c, n); a.AP = mf_rows(c, n); }
}
inline double *nn_t_layout(Carve &c, int64_t n) { return mf_rows(c, n); }
inline void part0_layout(Carve &c, int64_t n, PcgVec &a) { a.part0 = mf_rows(c, (n + 255) / 256); }

// the low-rank preconditioner's pieces: T (pad128(q) rows whose padding stays zero), the chunks' partials of G (D^-1 R), part0
struct PrecondWs { double *T, *tpart; int64_t qp, tchunks; };
PrecondWs precond_layout(Carve &c, int64_t n, int q, PcgVec &a) {
    PrecondWs l;
    l.qp = q > 0 ? pad128(q) : 0;
    l.tchunks = (n + PT_CHUNK - 1) / PT_CHUNK;
    l.T = mf_rows(c, l.qp); l.tpart = mf_rows(c, l.tchunks * q);
    part0_layout(c, n, a);
    return l;
}

// before the first pcg_precond on a workspace: the padding of T is zeroed
int precond_begin(fvgp_handle *h, const PrecondWs &l) {
    if (l.qp) HIPCHK(hipMemsetAsync(l.T, 0, (size_t)l.qp * PCG_LD * sizeof(double), h->stream));
    return 0;
}

// Z = M^-1 R for the solver's own vectors, part0 = r.z: G (D^-1 R) in chunks, one potrs per column, the apply kernel
int pcg_precond(fvgp_handle *h, const double *G, int64_t ldg, int q, const double *C, int64_t ldc, const PcgVec &a, const PrecondWs &l) {
    double *T = l.T, *tpart = l.tpart;
    if (q > 0) {
        HIPLAUNCH(pcg_gr_kernel, dim3((unsigned)l.tchunks), dim3(256), h->stream, G, (long)ldg, q, a, tpart);
        HIPLAUNCH(pcg_gr_finish_kernel, dim3((unsigned)((q * PCG_LD + 255) / 256)), dim3(256), h->stream, tpart, (long)l.tchunks, q, a.s, T);
        // one right-hand side at a time: a column's sweeps are then the same launches whatever s is
        for (int c = 0; c < a.s; ++c) { const int r = potrs_vec(h, C, q, ldc, T + c, 1, PCG_LD, true); if (r) return r; }
    }
    HIPLAUNCH(pcg_apply_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), h->stream, G, (long)ldg, q, T, a);
    return 0;
}

// ------------------------------------------------------------------------------- the nearest-neighbour preconditioner
// the sparse inverse Cholesky factor W of fvgp_hip_nn_factor and its transposed lists (include/fvgp_hip_nn.h): idx and coef (n, ld), row i
// of W is coef[i][.] at the columns idx[i][.] and dinv[i] on the diagonal; bucket j of tr_pos holds the flat positions of column j's
// entries in ascending row
struct NnFactor {
    const int *idx; const double *coef, *dinv; const int64_t *tr_start, *tr_pos;
    long n, ld, nnz; int m;
};

// T = W R.  A row of the solver's vectors is PCG_LD doubles = 128 bytes: 16 lanes take a row, one column each, so that every wave
// instruction reads four whole rows; the 16 lanes of a row read the same list entry and coefficient (one address, a broadcast)
__global__ __launch_bounds__(256) void nn_gather_kernel(NnFactor f, const double *R, int s, double *T) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(e & 15);
    const long i = e >> 4;
    if (i >= f.n || c >= s) return;
    const int *li = f.idx + i * f.ld;
    const double *ci = f.coef + i * f.ld;
    double acc = f.dinv[i] * R[i * PCG_LD + c];
    for (int l = 0; l < f.m; ++l) {
        const long j = li[l];
        if (j >= 0 && j < f.n) acc = fma(ci[l], R[j * PCG_LD + c], acc);
    }
    T[i * PCG_LD + c] = acc;
}

// Z = W^T T and part0 = r.z per 256 rows, where pcg_apply_kernel leaves it.  Thread (g, c) of a workgroup takes the rows g, g + 16, .. of
// its 256 and column c; a row walks its own bucket in ascending order and nothing else: the loop is bounded by the bucket's length (clipped
// to the list), a position outside the factor is skipped, no workgroup waits for another.  r.z: the thread's rows by fma in ascending
// order, then the tree over g
__global__ __launch_bounds__(256) void nn_transpose_kernel(NnFactor f, const double *T, PcgVec a) {
    const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
    const long r0 = (long)blockIdx.x * 256, r1 = r0 + 256 < f.n ? r0 + 256 : f.n;
    const int64_t npos = (int64_t)f.n * f.ld;
    double rz = 0.0;
    if (c < a.s)
        for (long j = r0 + g; j < r1; j += 16) {
            int64_t e0 = f.tr_start[j], e1 = f.tr_start[j + 1];
            e0 = e0 < 0 ? 0 : e0; e1 = e1 > f.nnz ? f.nnz : e1;
            double z = f.dinv[j] * T[j * PCG_LD + c];
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t pos = f.tr_pos[e];
                if (pos >= 0 && pos < npos) z = fma(f.coef[pos], T[(pos / f.ld) * PCG_LD + c], z);
            }
            a.Z[j * PCG_LD + c] = z;
            rz = fma(a.R[j * PCG_LD + c], z, rz);
        }
    dot_block(rz, a.part0, tid, true);
}

// Z = W^T (W R) for the solver's own vectors, part0 = r.z: the two launches in stream order
int nn_precond(fvgp_handle *h, const NnFactor &f, const PcgVec &a, double *T) {
    HIPLAUNCH(nn_gather_kernel, dim3((unsigned)((f.n * PCG_LD + 255) / 256)), dim3(256), h->stream, f, (const double *)a.R, a.s, T);
    HIPLAUNCH(nn_transpose_kernel, dim3((unsigned)((f.n + 255) / 256)), dim3(256), h->stream, f, (const double *)T, a);
    return 0;
}

// the factor's arguments as the two entries take them, positions p0 .. p0 + 7 of the entry: 0, or minus the position of the first bad one
int nn_factor_check(const char *who, int64_t n, const int *idx, int64_t ld, int m, const double *coef, const double *dinv,
                    const int64_t *tr_start, const int64_t *tr_pos, int64_t nnz, int p0) {
    if (!idx) return -p0;
    if (m < 1 || m > FVGP_NN_MAX_NEIGHBORS) { fvgp_set_error(std::string(who) + ": 1 .. FVGP_NN_MAX_NEIGHBORS neighbours"); return -(p0 + 2); }
    if (ld < m) return -(p0 + 1);
    if (!coef) return -(p0 + 3);
    if (!dinv) return -(p0 + 4);
    if (!tr_start) return -(p0 + 5);
    if (!tr_pos) return -(p0 + 6);
    if (nnz < 0 || nnz > n * ld) { fvgp_set_error(std::string(who) + ": nnz outside 0 .. n ld"); return -(p0 + 7); }
    return 0;
}

// the solver's workspace: its vectors (into a), the low-rank preconditioner's pieces, the second partials, the state, the split product's
// parking room while the product deals chunk ranges by itself, nn: the intermediate T of the nearest-neighbour preconditioner, L > 0:
// the Lanczos record -- alpha and beta (PCG_LD, L), rho0, steps and first (PCG_LD ints each) and PCG_LD doubles that nothing uses
// (the size has always counted the two rows of ints as rows of doubles)
struct PcgWs { PrecondWs pre; double *mv, *nnT; int64_t mv_doubles; PcgRec rec; size_t rec_bytes; };
PcgWs pcg_layout(Carve &c, int64_t n, int q, bool nn, int L, PcgVec &a) {
    PcgWs l{};
    vec_layout(c, n, true, a);
    l.pre = precond_layout(c, n, q, a);
    a.part1 = mf_rows(c, (n + 255) / 256); a.st = c.take<PcgState>(1);
    l.mv_doubles = mv_auto_split(n, n) > 1 ? mv_split_doubles(n, n, MV_MAXS) : 0;
    l.mv = l.mv_doubles ? mv_park_layout(c, n, n, MV_MAXS) : nullptr;
    l.nnT = nn ? nn_t_layout(c, n) : nullptr;
    if (L > 0) {                                                  // L == 0: every pointer NULL, the scalar kernel records nothing
        const int64_t at = c.bytes();
        l.rec.alpha = mf_rows(c, L); l.rec.beta = mf_rows(c, L); l.rec.rho0 = mf_rows(c, 1);
        l.rec.steps = c.take<int>(PCG_LD, sizeof(int)); l.rec.first = c.take<int>(PCG_LD, sizeof(int));
        mf_rows(c, 1); l.rec.L = L; l.rec_bytes = (size_t)(c.bytes() - at);
    }
    return l;
}

// fvgp_hip_precond_apply's workspace: R and Z, the low-rank preconditioner's pieces
PrecondWs apply_layout(Carve &c, int64_t n, int q, PcgVec &a) {
    vec_layout(c, n, false, a);
    return precond_layout(c, n, q, a);
}

// fvgp_hip_nn_precond_apply's: R and Z, T, part0
double *nn_apply_layout(Carve &c, int64_t n, PcgVec &a) {
    vec_layout(c, n, false, a);
    double *T = nn_t_layout(c, n);
    part0_layout(c, n, a);
    return T;
}

// what the two solver entries ask of the driver: the arguments of fvgp_hip_pcg_lanczos (include/fvgp_hip.h); fvgp_hip_pcg leaves L = 0
struct PcgCall {
    int kernel_id; const double *x; int64_t n; int d; const double *theta; int ntheta; const double *vdiag, *G; int64_t ldg; int q;
    const double *C; int64_t ldc; const double *B; int64_t ldb; int s; double *X; int64_t ldx; int warm; double tol;
    int max_iter, check_every, max_restarts; double *work; int64_t work_bytes; int *iters_host; double *relres_host; int *status_host;
    int L; double *alpha_host, *beta_host; int *steps_host; double *rho0_host;
    const NnFactor *nn = nullptr;            // fvgp_hip_pcg_nn: the sparse factor in the place of (G, C); its entry has checked it
};

// the one driver of fvgp_hip_pcg (L == 0), fvgp_hip_pcg_lanczos and fvgp_hip_pcg_nn (p.nn: only the preconditioner's launches differ)
int pcg_driver(fvgp_handle *h, PcgCall p) {
    if (!h) return -1;
    if (!kernel_id_known(p.kernel_id)) { fvgp_set_error("unknown kernel id"); return -2; }
    if (!p.x) return -3;
    if (p.n <= 0) return -4;
    int rc = check_kernel_args(p.kernel_id, p.d, p.theta, p.ntheta, 5, 6, 7); if (rc) return rc;
    if (!p.vdiag) { fvgp_set_error("pcg: the noise variances are the Jacobi part of the preconditioner and must be given"); return -8; }
    if (!p.G) p.q = 0;
    if (p.q < 0 || p.q > FVGP_PCG_MAX_RANK) { fvgp_set_error("pcg: rank outside 0 .. FVGP_PCG_MAX_RANK"); return -11; }
    if (p.q > 0) {
        if (p.ldg < p.n) return -10;
        rc = check_square(p.C, p.q, p.ldc, 12, 11, 13);
        if (rc) return rc;
    }
    if (!p.B) return -14;
    if (p.s < 1 || p.s > FVGP_PCG_MAX_RHS) { fvgp_set_error("pcg: 1 .. FVGP_PCG_MAX_RHS right-hand sides per call"); return -16; }
    if (p.ldb < p.s) return -15;
    if (!p.X) return -17;
    if (p.ldx < p.s) return -18;
    if (!(p.tol > 0.0)) return -20;
    if (p.max_iter < 1) return -21;
    if (p.check_every < 1) return -22;
    if (p.max_restarts < 0) return -23;
    if (!p.work || ((uintptr_t)p.work & 15)) { fvgp_set_error("pcg: work must be 16-byte aligned"); return -24; }
    if (p.L < 0 || p.L > FVGP_LANCZOS_MAX_STEPS) { fvgp_set_error("pcg_lanczos: lanczos_steps outside 0 .. FVGP_LANCZOS_MAX_STEPS"); return -29; }
    Carve c(p.work); PcgVec a;
    const PcgWs lay = pcg_layout(c, p.n, p.q, p.nn, p.L, a);
    if (p.work_bytes < c.bytes()) {
        fvgp_set_error(p.nn ? "pcg_nn: work smaller than fvgp_hip_pcg_nn_workspace_bytes(n)"
                       : p.L ? "pcg_lanczos: work smaller than fvgp_hip_pcg_lanczos_workspace_bytes(n, rank, lanczos_steps)"
                         : "pcg: work smaller than fvgp_hip_pcg_workspace_bytes(n, rank)");
        return -25;
    }
    if (!p.iters_host) return -26;
    if (!p.relres_host) return -27;
    if (!p.status_host) return -28;
    if (p.L > 0) {
        if (!p.alpha_host) return -30;
        if (!p.beta_host) return -31;
        if (!p.steps_host) return -32;
        if (!p.rho0_host) return -33;
    }
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(p.kernel_id, p.d, p.theta, p.ntheta, &k); if (rc) return rc;
    k.x1 = p.x; k.n1 = p.n; k.x2 = p.x; k.n2 = p.n; k.vdiag = p.vdiag;
    const PcgRec &rec = lay.rec;
    if (p.L > 0) HIPCHK(hipMemsetAsync(rec.alpha, 0, lay.rec_bytes, h->stream));
    a.X = p.X; a.ldx = p.ldx; a.B = p.B; a.ldb = p.ldb; a.v = p.vdiag;
    a.n = p.n; a.s = p.s;
    rc = precond_begin(h, lay.pre); if (rc) return rc;
    double *mvws = lay.mv;
    const long nblk = (long)((p.n + DOT_ROWS - 1) / DOT_ROWS), nblk_apply = (long)((p.n + 255) / 256);
    const dim3 gdot((unsigned)nblk), gdir((unsigned)((p.n * PCG_LD + 255) / 256));
    hipStream_t st = h->stream;

    auto matvec = [&](const double *V, int64_t ldv) -> int {     // AP = (K + D) V
        return launch_kmatvec(h, k, V, ldv, p.s, a.AP, PCG_LD, mvws, lay.mv_doubles, true);
    };
    auto scalar = [&](const PcgVec &v, long nb, int mode) -> int {
        HIPLAUNCH(pcg_scalar_kernel, dim3(1), dim3(256), st, v, nb, mode, p.tol, p.max_iter, rec);
        return 0;
    };
    auto precond = [&]() -> int {
        return p.nn ? nn_precond(h, *p.nn, a, lay.nnT) : pcg_precond(h, p.G, p.ldg, p.q, p.C, p.ldc, a, lay.pre);
    };
    PcgVec a1 = a; a1.part1 = a.part0;                            // (a scalar step that reads one partial array)

    if (p.warm) {
        rc = matvec(p.X, p.ldx); if (rc) return rc;
        HIPLAUNCH(pcg_resid_kernel, gdot, dim3(256), st, a, 1);
        rc = scalar(a, nblk, SC_INIT); if (rc) return rc;
        HIPLAUNCH(pcg_zero_cols_kernel, gdir, dim3(256), st, a);
    } else {
        HIPLAUNCH(pcg_resid_kernel, gdot, dim3(256), st, a, 0);
        rc = scalar(a1, nblk, SC_INIT); if (rc) return rc;
    }
    rc = precond(); if (rc) return rc;
    rc = scalar(a1, nblk_apply, SC_RHO0); if (rc) return rc;
    HIPLAUNCH(pcg_dir_kernel, gdir, dim3(256), st, a);

    PcgState hs;
    int restarts[PCG_LD] = {0};
    bool final_col[PCG_LD] = {false};
    // no column iterates more than max_iter times in all; each restart round ends when every column is frozen
    for (;;) {
        for (int it = 0;; ++it) {
            if (it % p.check_every == 0) {
                HIPCHK(hipMemcpyAsync(&hs, a.st, sizeof(hs), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                bool any = false;
                for (int c = 0; c < p.s; ++c) any = any || hs.active[c];
                if (!any) break;
            }
            rc = matvec(a.P, PCG_LD); if (rc) return rc;
            HIPLAUNCH(pcg_dot_kernel, gdot, dim3(256), st, a.P, a.AP, (long)p.n, p.s, a.part0);
            rc = scalar(a1, nblk, SC_ALPHA); if (rc) return rc;
            HIPLAUNCH(pcg_axpy_kernel, gdot, dim3(256), st, a);
            rc = scalar(a1, nblk, SC_RNORM); if (rc) return rc;
            rc = precond(); if (rc) return rc;
            rc = scalar(a1, nblk_apply, SC_BETA); if (rc) return rc;
            HIPLAUNCH(pcg_dir_kernel, gdir, dim3(256), st, a);
        }
        // every column is frozen: the true residual b - A x decides
        rc = matvec(p.X, p.ldx); if (rc) return rc;
        HIPLAUNCH(pcg_resid_kernel, gdot, dim3(256), st, a, 2);
        rc = scalar(a, nblk, SC_TRUE); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(&hs, a.st, sizeof(hs), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool again = false;
        for (int c = 0; c < p.s; ++c) {
            if (final_col[c]) continue;
            p.iters_host[c] = hs.iters[c]; p.relres_host[c] = hs.relres[c];
            if (hs.relres[c] <= p.tol) { p.status_host[c] = 0; final_col[c] = true; }
            else if (hs.code[c] == 2) { p.status_host[c] = 2; final_col[c] = true; }
            else if (hs.code[c] == 1 || restarts[c] >= p.max_restarts || !(hs.relres[c] == hs.relres[c])) { p.status_host[c] = 1; final_col[c] = true; }
            else { restarts[c] += 1; hs.restart[c] = 1; again = true; }
        }
        if (!again) break;
        HIPCHK(hipMemcpyAsync(a.st->restart, hs.restart, sizeof(hs.restart), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                         // (hs is on the stack: the copy must have read it before it changes)
        rc = precond(); if (rc) return rc;
        rc = scalar(a1, nblk_apply, SC_RESTART); if (rc) return rc;
        HIPLAUNCH(pcg_dir_kernel, gdir, dim3(256), st, a);
    }
    if (p.L > 0) {
        HIPCHK(hipMemcpyAsync(p.alpha_host, rec.alpha, (size_t)p.s * p.L * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(p.beta_host, rec.beta, (size_t)p.s * p.L * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(p.rho0_host, rec.rho0, (size_t)p.s * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(p.steps_host, rec.steps, (size_t)p.s * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

// fvgp_hip_pchol's workspace: the core's pieces, then the residual diagonal
void pchol_layout(Carve &c, int64_t n, PivotArgs &a) {
    pivot_layout(c, n, 2, a);
    a.var = c.take<double>(n);
}

// fvgp_hip_precond_factor's: the partial Gram sums of the nch chunks
double *pf_layout(Carve &c, int64_t n, int q, int64_t &nch) { nch = (n + PF_CHUNK - 1) / PF_CHUNK; return c.take<double>(nch * q * q, sizeof(double)); }

}  // namespace

extern "C" {

int64_t fvgp_hip_pchol_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 1) return -1;
    return carve_bytes_for<PivotArgs>(pchol_layout, n);
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
    // selection's run with the data as their own candidates: no conditioning, no noise, d = sigma^2 at the start, G the caller's
    Carve c(work); PivotArgs a{};
    pchol_layout(c, n, a);
    if (work_bytes < c.bytes()) { fvgp_set_error("pchol: work smaller than fvgp_hip_pchol_workspace_bytes(n, q)"); return -15; }
    if (!rank_host) return -16;
    HIPCHK(hipSetDevice(h->device));
    KmatDesc k{};
    rc = kmat_desc_from_theta(kernel_id, d, theta, ntheta, &k); if (rc) return rc;
    a.x = x; a.xc = x; a.G = G; a.ldg_in = ldg;
    a.idx = reinterpret_cast<long long *>(piv_out);
    a.n = n; a.P = n; a.cn = n; a.d = d; a.q = q; a.sig = k.sig; a.tol = tol;
    for (int i = 0; i < FVGP_MAX_DIM; ++i) a.il[i] = k.invl[i];
    const unsigned nb = (unsigned)((n + 255) / 256);
    // the rows an exhausted run never reaches are zero rows: G is cleared first, inside its (q, n) view only
    for (int64_t r0 = 0; r0 < q; r0 += 1024) {
        const int64_t rows = q - r0 < 1024 ? q - r0 : 1024;
        HIPLAUNCH(mf_zero_rows_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), h->stream, G + r0 * ldg, (long)ldg,
                  (long)rows, (long)n);
    }
    HIPLAUNCH(pivot_init_kernel, dim3(nb), dim3(256), h->stream, a);
    for (int t = 0; t < q; ++t) {
        a.t = t;
        HIPLAUNCH(pivot_pick_kernel, dim3(1), dim3(256), h->stream, a);
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
    return carve_bytes_for<int64_t>(pf_layout, n, q);
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
    Carve c(work); int64_t nch;
    double *gram = pf_layout(c, n, q, nch);
    if (work_bytes < c.bytes()) { fvgp_set_error("precond_factor: work smaller than fvgp_hip_precond_workspace_bytes(n, q)"); return -10; }
    if (!info_host) return -11;
    HIPCHK(hipSetDevice(h->device));
    if (nch > 65535) { fvgp_set_error("precond_factor: n too large"); return -5; }
    const int nt = (q + 15) / 16;
    HIPLAUNCH(pf_gram_kernel, dim3((unsigned)(nt * nt), (unsigned)nch), dim3(256), h->stream, G, (long)ldg, q, (long)n, vdiag, gram);
    HIPLAUNCH(pf_finish_kernel, dim3((unsigned)(((int64_t)q * q + 255) / 256)), dim3(256), h->stream, gram, (long)nch, q, C, (long)ldc);
    rc = launch_pad_identity(h, C, q, pad128(q), ldc); if (rc) return rc;
    return potrf_driver(h, C, q, ldc, info_host);
}

int64_t fvgp_hip_pcg_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 0) return -1;
    return carve_bytes_for<PcgVec>(pcg_layout, n, q, false, 0);
}

int fvgp_hip_pcg(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                 const double *vdiag, const double *G, int64_t ldg, int q, const double *C, int64_t ldc,
                 const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                 double tol, int max_iter, int check_every, int max_restarts,
                 double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host) {
    return pcg_driver(h, PcgCall{kernel_id, x, n, d, theta, ntheta, vdiag, G, ldg, q, C, ldc, B, ldb, s, X, ldx, warm, tol, max_iter, check_every,
                                 max_restarts, work, work_bytes, iters_host, relres_host, status_host, 0, nullptr, nullptr, nullptr, nullptr});
}

int64_t fvgp_hip_pcg_lanczos_workspace_bytes(int64_t n, int q, int lanczos_steps) {
    if (n < 1 || q < 0 || lanczos_steps < 0 || lanczos_steps > FVGP_LANCZOS_MAX_STEPS) return -1;
    return carve_bytes_for<PcgVec>(pcg_layout, n, q, false, lanczos_steps);
}

int fvgp_hip_pcg_lanczos(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                         const double *vdiag, const double *G, int64_t ldg, int q, const double *C, int64_t ldc,
                         const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                         double tol, int max_iter, int check_every, int max_restarts,
                         double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host,
                         int lanczos_steps, double *alpha_host, double *beta_host, int *steps_host, double *rho0_host) {
    return pcg_driver(h, PcgCall{kernel_id, x, n, d, theta, ntheta, vdiag, G, ldg, q, C, ldc, B, ldb, s, X, ldx, warm, tol, max_iter, check_every,
                                 max_restarts, work, work_bytes, iters_host, relres_host, status_host, lanczos_steps, alpha_host, beta_host,
                                 steps_host, rho0_host});
}

int64_t fvgp_hip_pcg_nn_workspace_bytes(int64_t n) {
    if (n < 1) return -1;
    return carve_bytes_for<PcgVec>(pcg_layout, n, 0, true, 0);
}

int fvgp_hip_pcg_nn(fvgp_handle *h, int kernel_id, const double *x, int64_t n, int d, const double *theta, int ntheta,
                    const double *vdiag, const int *idx, int64_t ld, int m, const double *coef, const double *dinv,
                    const int64_t *tr_start, const int64_t *tr_pos, int64_t nnz,
                    const double *B, int64_t ldb, int s, double *X, int64_t ldx, int warm,
                    double tol, int max_iter, int check_every, int max_restarts,
                    double *work, int64_t work_bytes, int *iters_host, double *relres_host, int *status_host) {
    if (!h) return -1;
    if (n >= 1) { const int rc = nn_factor_check("pcg_nn", n, idx, ld, m, coef, dinv, tr_start, tr_pos, nnz, 9); if (rc) return rc; }
    const NnFactor f{idx, coef, dinv, tr_start, tr_pos, (long)n, (long)ld, (long)nnz, m};
    const int rc = pcg_driver(h, PcgCall{kernel_id, x, n, d, theta, ntheta, vdiag, nullptr, 0, 0, nullptr, 0, B, ldb, s, X, ldx, warm, tol, max_iter,
                                         check_every, max_restarts, work, work_bytes, iters_host, relres_host, status_host, 0, nullptr, nullptr,
                                         nullptr, nullptr, &f});
    // the driver numbers its errors by the positions of fvgp_hip_pcg: from B on this entry's are three further
    return rc <= -14 && rc > -1000 ? rc - 3 : rc;
}

int64_t fvgp_hip_nn_precond_apply_workspace_bytes(int64_t n) {
    if (n < 1) return -1;
    return carve_bytes_for<PcgVec>(nn_apply_layout, n);
}

int fvgp_hip_nn_precond_apply(fvgp_handle *h, int64_t n, const int *idx, int64_t ld, int m, const double *coef, const double *dinv,
                              const int64_t *tr_start, const int64_t *tr_pos, int64_t nnz, const double *R, int64_t ldr, int s,
                              double *Z, int64_t ldz, double *work, int64_t work_bytes) {
    if (!h) return -1;
    if (n < 1 || n > 0x7fffffffLL) return -2;
    int rc = nn_factor_check("nn_precond_apply", n, idx, ld, m, coef, dinv, tr_start, tr_pos, nnz, 3); if (rc) return rc;
    if (!R) return -11;
    if (s < 1 || s > FVGP_PCG_MAX_RHS) { fvgp_set_error("nn_precond_apply: 1 .. FVGP_PCG_MAX_RHS columns per call"); return -13; }
    if (ldr < s) return -12;
    if (!Z) return -14;
    if (ldz < s) return -15;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("nn_precond_apply: work must be 16-byte aligned"); return -16; }
    Carve c(work); PcgVec a{};
    double *T = nn_apply_layout(c, n, a);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("nn_precond_apply: work smaller than fvgp_hip_nn_precond_apply_workspace_bytes(n)"); return -17;
    }
    HIPCHK(hipSetDevice(h->device));
    const NnFactor f{idx, coef, dinv, tr_start, tr_pos, (long)n, (long)ld, (long)nnz, m};
    a.n = n; a.s = s;
    const dim3 gcopy((unsigned)((n * PCG_LD + 255) / 256));
    HIPLAUNCH(mf_copy_cols_kernel, gcopy, dim3(256), h->stream, R, (long)ldr, a.R, (long)PCG_LD, (long)n, s);
    rc = nn_precond(h, f, a, T); if (rc) return rc;
    HIPLAUNCH(mf_copy_cols_kernel, gcopy, dim3(256), h->stream, (const double *)a.Z, (long)PCG_LD, Z, (long)ldz, (long)n, s);
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
    HIPLAUNCH(precond_probes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), h->stream, a);
    return 0;
}

int64_t fvgp_hip_precond_apply_workspace_bytes(int64_t n, int q) {
    if (n < 1 || q < 0) return -1;
    return carve_bytes_for<PcgVec>(apply_layout, n, q);
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
    Carve c(work); PcgVec a{};
    const PrecondWs lay = apply_layout(c, n, q, a);
    if (work_bytes < c.bytes()) { fvgp_set_error("precond_apply: work smaller than fvgp_hip_precond_apply_workspace_bytes(n, rank)"); return -15; }
    HIPCHK(hipSetDevice(h->device));
    a.v = vdiag; a.n = n; a.s = s;
    int rc = precond_begin(h, lay); if (rc) return rc;
    const dim3 gcopy((unsigned)((n * PCG_LD + 255) / 256));
    HIPLAUNCH(mf_copy_cols_kernel, gcopy, dim3(256), h->stream, R, (long)ldr, a.R, (long)PCG_LD, (long)n, s);
    rc = pcg_precond(h, G, ldg, q, C, ldc, a, lay); if (rc) return rc;
    HIPLAUNCH(mf_copy_cols_kernel, gcopy, dim3(256), h->stream, (const double *)a.Z, (long)PCG_LD, W, (long)ldw, (long)n, s);
    return 0;
}

}  // extern "C"
