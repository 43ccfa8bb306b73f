// Vector triangular sweeps (HBM-bound work).
//
// potrs with a handful of right-hand sides (y has 1..few columns, fvgp/gp_kv.py:592) is
// bandwidth work: L is streamed exactly once per direction.  Both sweeps use the inverted
// 128x128 diagonal blocks left behind by the factorisation, so a block step is
//   forward :  y_k = inv(L_kk) b_k ;  b[r > k] -= L[r, k-block] y_k      (column panel, rows below)
//   backward:  x_k = inv(L_kk)^T y_k ; y[c < k] -= L[k-block, c]^T x_k   (row panel, columns left)
// Each workgroup recomputes the 128-vector of its step from the L2-resident diagonal
// inverse (128 KiB) instead of waiting on a second launch, so one launch = one block step.
#include "common.h"

namespace {

// wave-wide sum of R independent values per column: all R rows are in flight before any reduction
template <int C, int R>
__device__ __forceinline__ void wave_reduce(double (&acc)[R][C]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int cc = 0; cc < C; ++cc) acc[rr][cc] += __shfl_down(acc[rr][cc], off, 64);
}

template <int C>
__global__ __launch_bounds__(256) void fwd_step_kernel(const double *L, long ldl, long np, long k0, const double *linv,
                                                       double *B, long ldb, double *Y, int c_used) {
    __shared__ double sb[128 * C];
    __shared__ double sy[128 * C];
    constexpr int R = 8;                       // rows below in flight per wave and pass
    constexpr int RY = 16;                     // rows of the diagonal inverse in flight per wave and pass
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // like the backward step, a chain of memory round trips: the first pass over the rows below does not depend on y, so
    // its loads go out before anything else
    const long r0 = k0 + 128;
    const long stride = (long)gridDim.x * 4 * R;
    const long rb0 = r0 + ((long)blockIdx.x * 4 + wave) * R;
    double2_t lf[R];
    if (rb0 < np) {
#pragma unroll
        for (int rr = 0; rr < R; ++rr) lf[rr] = *reinterpret_cast<const double2_t *>(L + (rb0 + rr) * ldl + k0 + 2 * lane);
    }
    for (int e = tid; e < 128 * C; e += 256) {
        const int i = e / C, cc = e - i * C;
        sb[e] = cc < c_used ? B[(k0 + i) * ldb + cc] : 0.0;
    }
    __syncthreads();
    // y = Linv * b : wave handles 32 rows, 16 at a time; lanes hold 2 columns each
    {
        double b0[C], b1[C];
#pragma unroll
        for (int cc = 0; cc < C; ++cc) { b0[cc] = sb[(2 * lane) * C + cc]; b1[cc] = sb[(2 * lane + 1) * C + cc]; }
        for (int i0 = wave * 32; i0 < wave * 32 + 32; i0 += RY) {
            double2_t l2[RY];
#pragma unroll
            for (int rr = 0; rr < RY; ++rr) l2[rr] = *reinterpret_cast<const double2_t *>(linv + (i0 + rr) * 128 + 2 * lane);
            double acc[RY][C];
#pragma unroll
            for (int rr = 0; rr < RY; ++rr)
#pragma unroll
                for (int cc = 0; cc < C; ++cc) acc[rr][cc] = l2[rr][0] * b0[cc] + l2[rr][1] * b1[cc];
            wave_reduce<C, RY>(acc);
            if (lane == 0)
#pragma unroll
                for (int rr = 0; rr < RY; ++rr)
#pragma unroll
                    for (int cc = 0; cc < C; ++cc) sy[(i0 + rr) * C + cc] = acc[rr][cc];
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int e = tid; e < 128 * C; e += 256) {
            const int i = e / C, cc = e - i * C;
            if (cc < c_used) Y[(k0 + i) * C + cc] = sy[e];
        }
    }
    // rows below: each wave takes R consecutive rows per pass
    double y0[C], y1[C];
#pragma unroll
    for (int cc = 0; cc < C; ++cc) { y0[cc] = sy[(2 * lane) * C + cc]; y1[cc] = sy[(2 * lane + 1) * C + cc]; }
    for (long rb = rb0; rb < np; rb += stride) {   // np - r0 is a multiple of 128
        double2_t l2[R];
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
            l2[rr] = rb == rb0 ? lf[rr] : *reinterpret_cast<const double2_t *>(L + (rb + rr) * ldl + k0 + 2 * lane);
        double acc[R][C];
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int cc = 0; cc < C; ++cc) acc[rr][cc] = l2[rr][0] * y0[cc] + l2[rr][1] * y1[cc];
        wave_reduce<C, R>(acc);
        if (lane == 0)
#pragma unroll
            for (int rr = 0; rr < R; ++rr)
#pragma unroll
                for (int cc = 0; cc < C; ++cc) if (cc < c_used) B[(rb + rr) * ldb + cc] -= acc[rr][cc];
    }
}

// One block step of the backward sweep.  A step is a chain of dependent memory round trips (y_k, the diagonal inverse, the
// row panel), not bandwidth, so each phase has ALL its loads in flight at once: the 128 x 128 inverse as 64 loads per thread,
// the row panel with the 128 rows split over the four waves (32 loads per thread, two columns each) and the four partial
// sums combined through LDS -- three round trips per step instead of thirteen.  Workgroup b owns columns [128 b, 128 b + 128).
template <int C>
__global__ __launch_bounds__(256) void bwd_step_kernel(const double *L, long ldl, long np, long k0, const double *linv,
                                                       double *Yres, double *X, long ldx, int c_used) {
    __shared__ double sy[128 * C];
    __shared__ double sxv[2][128 * C];
    __shared__ double sp[4][128 * C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the row panel does not depend on x: its loads go out first and fly during the x phase
    const long c2 = (long)blockIdx.x * 128 + 2 * lane;
    const bool have = c2 < k0;
    double2_t l2[32];
    if (have) {
#pragma unroll
        for (int u = 0; u < 32; ++u) l2[u] = *reinterpret_cast<const double2_t *>(L + (k0 + wave * 32 + u) * ldl + c2);
    }
    for (int e = tid; e < 128 * C; e += 256) sy[e] = Yres[k0 * C + e];
    // x = Linv^T y : thread (i, half) walks half of column i of Linv (coalesced across i)
    {
        const int i = tid & 127, half = tid >> 7;
        double l[64];
#pragma unroll
        for (int u = 0; u < 64; ++u) l[u] = linv[(half * 64 + u) * 128 + i];      // Linv[j][i] = 0 for j < i
        __syncthreads();
        double acc[C];
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = 0.0;
#pragma unroll
        for (int u = 0; u < 64; ++u)
#pragma unroll
            for (int cc = 0; cc < C; ++cc) acc[cc] = fma(l[u], sy[(half * 64 + u) * C + cc], acc[cc]);
#pragma unroll
        for (int cc = 0; cc < C; ++cc) sxv[half][i * C + cc] = acc[cc];
    }
    __syncthreads();
    for (int e = tid; e < 128 * C; e += 256) sxv[0][e] += sxv[1][e];
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int e = tid; e < 128 * C; e += 256) {
            const int i = e / C, cc = e - i * C;
            if (cc < c_used) X[(k0 + i) * ldx + cc] = sxv[0][e];
        }
    }
    // columns to the left: this wave's 32 rows of the panel times x, two adjacent columns per lane
    double a0[C], a1[C];
#pragma unroll
    for (int cc = 0; cc < C; ++cc) { a0[cc] = 0.0; a1[cc] = 0.0; }
    if (have) {
#pragma unroll
        for (int u = 0; u < 32; ++u)
#pragma unroll
            for (int cc = 0; cc < C; ++cc) {
                const double xv = sxv[0][(wave * 32 + u) * C + cc];
                a0[cc] = fma(l2[u][0], xv, a0[cc]);
                a1[cc] = fma(l2[u][1], xv, a1[cc]);
            }
    }
#pragma unroll
    for (int cc = 0; cc < C; ++cc) { sp[wave][(2 * lane) * C + cc] = a0[cc]; sp[wave][(2 * lane + 1) * C + cc] = a1[cc]; }
    __syncthreads();
    for (int e = tid; e < 128 * C; e += 256) {
        const long col = (long)blockIdx.x * 128 + e / C;
        if (col < k0) Yres[(long)blockIdx.x * 128 * C + e] -= (sp[0][e] + sp[1][e]) + (sp[2][e] + sp[3][e]);
    }
}

// The whole backward sweep in ONE launch (one right-hand side).  The per-block launches above are a chain of N/128 dependent
// kernels of 7-11 us each (x_k by everybody, one read of the row panel, one boundary); here workgroup c owns the 128 columns of
// block c for the whole sweep: it keeps y_c in LDS, walks down the column of L below its block -- the next 128 x 128 block is in
// flight before the x it meets has arrived -- and, once the block right under the diagonal is in, multiplies by the inverse of
// its diagonal block (fetched like one more block of the column) and PUBLISHES x_c to the workgroups left of it.  The hand-off
// is the one form that needs neither fence nor flag (MI355X_MICROARCH.md, inter-workgroup visibility, "granule"): every
// published double travels as ONE naturally aligned 16-byte {value, tag} written by one sc1 (write-through) store and polled by
// sc1 loads until its tag is this launch's -- a stale line shows an old tag and is read again, so nothing depends on when
// another compute unit's caches notice the store.  The tag is a per-handle launch counter, never reused; the stored word is the
// tag XOR a hash of the value, so a granule whose halves come from two different stores does not pass either.  Columns are handed out
// by a ticket in the order the workgroups start (c = nb - 1 - ticket), so a workgroup only ever waits for workgroups that started
// before it: no assumption on the dispatch order, no need for the whole grid to be resident.  Every sum is formed in the order
// the step kernels use (four row quarters of a block, ((0+1)+(2+3)); two halves of the inverse), so the results are
// bit-identical to theirs -- which is how the tests would see a stale read.  Spins are bounded (seconds): a workgroup that gives
// up publishes NaN.
//
// The two sweep kernels keep the poll loop, the publish and (backward) the block load written out in their bodies: each sits at 256 VGPRs
// with part of its state parked in AGPRs, and with those moved into shared device functions the generated code came out differently
// and every hop of the sweep 40-90 ns slower (potrs with one right-hand side +2.1 % at N = 4096, +1.3 % at N = 16384; the backward
// block load through load_wave_rows, ONE scalar instruction more, +1.2 %).  Shared is what leaves the two kernels' instructions as
// they are: the constants of the protocol -- the multiplier of the hash that ties a granule's tag word to its value, the polls after
// which a workgroup gives up --, the ticket, and the forward sweep's loads.
constexpr unsigned long long GRANULE_HASH = 0x9E3779B97F4A7C15ull;
constexpr int GRANULE_SPINS = 1 << 22;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// this workgroup's place in the order the workgroups start (one thread calls it) ...
__device__ __forceinline__ int sweep_ticket_take(int *ticket) { return atomicAdd(ticket, 1); }
// ... and the last workgroup to finish leaves both ticket words zero for the next launch (one thread calls it)
__device__ __forceinline__ void sweep_ticket_done(int *ticket) {
    if (atomicAdd(ticket + 1, 1) == (int)gridDim.x - 1) { atomicExch(ticket, 0); atomicExch(ticket + 1, 0); }
}

// l2 <- 32 rows of 128 doubles from `first` on (wave-uniform), row stride `stride`: lane l takes columns 2 l, 2 l + 1 of each (one buffer
// descriptor, the lane's 16 bytes as the only vector offset, the row as a scalar offset: 32 64-bit addresses would cost as many
// registers as the data)
__device__ __forceinline__ void load_wave_rows(u32x4 (&l2)[32], const double *first, const long stride, const int lane) {
    const double *base = uniform_ptr(first);
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(base), 0, 0xffffffff, 0x00020000);
    const int rowb = (int)(stride * 8);
#pragma unroll
    for (int u = 0; u < 32; ++u) l2[u] = __builtin_amdgcn_raw_buffer_load_b128(src, 16 * lane, u * rowb, 0);
}

struct BwdSweepArgs {
    const double *L; long ldl; long np;
    const double *linv;           // 128 x 128 inverses of the diagonal blocks, block b at linv + b * 128 * 128 (row-major, zeros above)
    const double *Y;              // np residuals y = L^-1 b
    double *X; long ldx;
    double *gran;                 // np granules of {value, tag} (16 bytes each)
    unsigned long long tag;
    int *ticket;                  // {next column ticket, finished workgroups}; the last workgroup zeroes both
};

__global__ __launch_bounds__(256) void bwd_sweep_kernel(BwdSweepArgs g) {      // 1 workgroup per CU: the next block is in flight beside the current one
    __shared__ double sy[128];
    __shared__ double sx[128];
    __shared__ double sxv[2][128];
    __shared__ double sp[4][128];
    __shared__ int s_c, s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = (int)(g.np / 128);
    if (tid == 0) { s_c = nb - 1 - sweep_ticket_take(g.ticket); s_fail = 0; }
    __syncthreads();
    const int c = s_c;
    const __amdgpu_buffer_rsrc_t gsrc = __builtin_amdgcn_make_buffer_rsrc(g.gran, 0, 0xffffffff, 0x00020000);
    // (a buffer descriptor per block, the lane's 16 bytes as the only vector offset, the row as a scalar offset: 32 64-bit
    // addresses would cost as many registers as the data)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int rowb = (int)(g.ldl * 8);
    u32x4 l2[32];
    auto load_block = [&](const int I) {
        const double *base = uniform_ptr(g.L + ((long)I * 128 + wave_u * 32) * g.ldl + (long)c * 128);
        const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(base), 0, 0xffffffff, 0x00020000);
#pragma unroll
        for (int u = 0; u < 32; ++u) l2[u] = __builtin_amdgcn_raw_buffer_load_b128(src, 16 * lane, u * rowb, 0);
    };
    // the inverse of the diagonal block is the last "block" of the column: thread (i, half) takes half of column i of inv(L_cc)
    // (coalesced across i)
    // (registers of its own, requested before anything else: behind the last block of the column its round trip -- 128 KB, 2.6 us -- sat on
    // the path from x_{c+1} to x_c, a third of every hop of the sweep; one workgroup per compute unit has the registers)
    double2_t li[32];
    {
        const double *inv = g.linv + (long)c * 128 * 128 + (tid >> 7) * 64 * 128 + (tid & 127);
#pragma unroll
        for (int u = 0; u < 32; ++u) li[u] = (double2_t){inv[(2 * u) * 128], inv[(2 * u + 1) * 128]};
    }
    if (c < nb - 1) load_block(nb - 1);
    if (tid < 128) sy[tid] = g.Y[(long)c * 128 + tid];
    __syncthreads();
    for (int I = nb - 1; I > c; --I) {
        // ---- x_I: a thread per granule ------------------------------------------------------------------------------------
        if (tid < 128) {
            const int off = (int)(((long)I * 128 + tid) * 16);
            u32x4 v;
            int spins = 0;
            for (;;) {
                v = __builtin_amdgcn_raw_buffer_load_b128(gsrc, off, 0, 16);          // sc1: served past this CU's L1
                // the second word is tag ^ mix(value bits): a granule torn between its 8-byte halves (new tag beside a stale value, or
                // the other way round; never observed on gfx950, not promised by the ISA either) decodes to a wrong tag and is read again
                const unsigned long long vb = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
                const unsigned long long t = ((unsigned long long)v[2] | ((unsigned long long)v[3] << 32)) ^ (vb * GRANULE_HASH);
                if (t == g.tag) break;
                if (++spins > GRANULE_SPINS) { s_fail = 1; break; }
                // only the workgroup right behind the frontier is waited for: the further left, the rarer the polls (every
                // poll is a trip past the L1 that the producer's store and the critical poll share the fabric with)
                __builtin_amdgcn_s_sleep(2);
                for (int k = I - 1 - c < 24 ? I - 1 - c : 24; k > 0; --k) __builtin_amdgcn_s_sleep(6);
                asm volatile("" ::: "memory");
            }
            const unsigned long long bits = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
            double xv;
            __builtin_memcpy(&xv, &bits, 8);
            sx[tid] = xv;
        }
        __syncthreads();
        // ---- y_c -= L[I, c]^T x_I: this wave's 32 rows of the block, two adjacent columns per lane ----------------------
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const double xv = sx[wave * 32 + u];
            double2_t lv;
            __builtin_memcpy(&lv, &l2[u], 16);
            a0 = fma(lv[0], xv, a0);
            a1 = fma(lv[1], xv, a1);
        }
        if (I - 1 > c) load_block(I - 1);      // the next block of the column is on its way while the partial sums are combined
        sp[wave][2 * lane] = a0; sp[wave][2 * lane + 1] = a1;
        __syncthreads();
        if (tid < 128) sy[tid] -= (sp[0][tid] + sp[1][tid]) + (sp[2][tid] + sp[3][tid]);
        __syncthreads();
    }
    // ---- x_c = inv(L_cc)^T y_c : thread (i, half) walks half of column i of the inverse ---------------------------------------
    {
        const int i = tid & 127, half = tid >> 7;
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            acc = fma(li[u][0], sy[half * 64 + 2 * u], acc);
            acc = fma(li[u][1], sy[half * 64 + 2 * u + 1], acc);
        }
        sxv[half][i] = acc;
    }
    __syncthreads();
    if (tid < 128) {
        const double xv = s_fail ? __builtin_nan("") : sxv[0][tid] + sxv[1][tid];
        unsigned long long bits;
        __builtin_memcpy(&bits, &xv, 8);
        const unsigned long long tw = g.tag ^ (bits * GRANULE_HASH);        // tag and value vouch for each other (torn granules)
        const u32x4 v = {(unsigned)bits, (unsigned)(bits >> 32), (unsigned)tw, (unsigned)(tw >> 32)};
        __builtin_amdgcn_raw_buffer_store_b128(v, gsrc, (int)(((long)c * 128 + tid) * 16), 0, 16);      // one sc1 store per granule
        g.X[((long)c * 128 + tid) * g.ldx] = xv;
    }
    if (tid == 0) sweep_ticket_done(g.ticket);
}

// Sums of 32 per-lane values over the 64 lanes of a wave by halving: at distance 32, 16, 8, 4, 2 a lane keeps one half of its
// list and adds the partner's copy of that half (31 exchanges instead of 32 x 6), distance 1 completes the pair.  Row
// u = 16 b5 + 8 b4 + 4 b3 + 2 b2 + b1 (b_k = bit k of the lane) ends up, complete, in both lanes of its pair.  Fixed order.
__device__ __forceinline__ double wave_sums32(const double (&a)[32][1], const int lane) {
    double v16[16], v8[8], v4[4], v2[2];
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const double keep = b5 ? a[16 + k][0] : a[k][0], give = b5 ? a[k][0] : a[16 + k][0]; v16[k] = keep + __shfl_xor(give, 32, 64); }
#pragma unroll
    for (int k = 0; k < 8; ++k) { const double keep = b4 ? v16[8 + k] : v16[k], give = b4 ? v16[k] : v16[8 + k]; v8[k] = keep + __shfl_xor(give, 16, 64); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double keep = b3 ? v8[4 + k] : v8[k], give = b3 ? v8[k] : v8[4 + k]; v4[k] = keep + __shfl_xor(give, 8, 64); }
#pragma unroll
    for (int k = 0; k < 2; ++k) { const double keep = b2 ? v4[2 + k] : v4[k], give = b2 ? v4[k] : v4[2 + k]; v2[k] = keep + __shfl_xor(give, 4, 64); }
    const double keep = b1 ? v2[1] : v2[0], give = b1 ? v2[0] : v2[1];
    const double v1 = keep + __shfl_xor(give, 2, 64);
    return v1 + __shfl_xor(v1, 1, 64);
}

// The forward sweep L y = b in ONE launch (one right-hand side): the mirror image of bwd_sweep_kernel.  Workgroup r owns block ROW r
// of L -- 128 contiguous rows, streamed left to right, the next 128 x 128 block in flight before the y it meets has arrived -- and
// keeps, per thread, the partial sums of its wave's 32 rows over the two columns its lane reads; they are reduced across the
// lanes once, when the row is through (every sum in a fixed order: nothing depends on timing).  Then t = b_r - sum, y_r =
// inv(L_rr) t with the inverse fetched like one more block of the row, and y_r is PUBLISHED to the workgroups right of it as
// 16-byte {value, tag ^ hash(value)} granules exactly as the backward sweep hands its x to the left.  Rows are handed out by a
// ticket in start order (r = ticket): a workgroup only waits for workgroups that started before it.  Replaces N/128 dependent
// launches of 8-20 us each (the path of a size that leaves no padding row for the fused solve, n % 128 == 0: N = 4096 2.91 ms
// against 2.46 at N = 4000, same factorisation).
struct FwdSweepArgs {
    const double *L; long ldl; long np;
    const double *linv;
    const double *B; long ldb;    // right-hand side, column 0 (np rows, padding rows zero)
    double *Y;                    // np doubles: y = L^-1 b
    double *gran;
    unsigned long long tag;
    int *ticket;
};

__global__ __launch_bounds__(256) void fwd_sweep_kernel(FwdSweepArgs g) {
    __shared__ double sy[2][128];
    __shared__ double ssum[128];
    __shared__ double st[128];
    __shared__ int s_r, s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_r = sweep_ticket_take(g.ticket); s_fail = 0; }
    __syncthreads();
    const int r = s_r;
    const __amdgpu_buffer_rsrc_t gsrc = __builtin_amdgcn_make_buffer_rsrc(g.gran, 0, 0xffffffff, 0x00020000);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    u32x4 l2[32];
    // this wave's 32 rows of a 128 x 128 block
    auto load_rows = [&](const double *blk, const long stride) { load_wave_rows(l2, blk + (long)wave_u * 32 * stride, stride, lane); };
    const double *Lrow = g.L + (long)r * 128 * g.ldl;
    const double *inv = g.linv + (long)r * 128 * 128;
    // (the inverse of the diagonal block in registers of its own, requested first: see bwd_sweep_kernel)
    u32x4 li[32];
    load_wave_rows(li, inv + (long)wave_u * 32 * 128, 128, lane);
    if (r > 0) load_rows(Lrow, g.ldl);
    const double bval = tid < 128 ? g.B[((long)r * 128 + tid) * g.ldb] : 0.0;
    double acc[32][1];
#pragma unroll
    for (int u = 0; u < 32; ++u) acc[u][0] = 0.0;
    for (int c = 0; c < r; ++c) {
        if (tid < 128) {
            const int off = (int)(((long)c * 128 + tid) * 16);
            u32x4 v;
            int spins = 0;
            for (;;) {
                v = __builtin_amdgcn_raw_buffer_load_b128(gsrc, off, 0, 16);          // sc1: served past this CU's L1
                const unsigned long long vb = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
                const unsigned long long t = ((unsigned long long)v[2] | ((unsigned long long)v[3] << 32)) ^ (vb * GRANULE_HASH);
                if (t == g.tag) break;
                if (++spins > GRANULE_SPINS) { s_fail = 1; break; }
                __builtin_amdgcn_s_sleep(2);
                for (int k = r - 1 - c < 24 ? r - 1 - c : 24; k > 0; --k) __builtin_amdgcn_s_sleep(6);      // far behind the frontier: rare polls
                asm volatile("" ::: "memory");
            }
            const unsigned long long bits = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
            double yv;
            __builtin_memcpy(&yv, &bits, 8);
            sy[c & 1][tid] = yv;
        }
        __syncthreads();
        const double y0 = sy[c & 1][2 * lane], y1 = sy[c & 1][2 * lane + 1];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            double2_t lv;
            __builtin_memcpy(&lv, &l2[u], 16);
            acc[u][0] = fma(lv[0], y0, acc[u][0]);
            acc[u][0] = fma(lv[1], y1, acc[u][0]);
        }
        if (c + 1 < r) load_rows(Lrow + (long)(c + 1) * 128, g.ldl);      // on its way while the next y is awaited
    }
    const int urow = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    {
        const double tot = wave_sums32(acc, lane);
        if (!(lane & 1)) ssum[wave * 32 + urow] = tot;
    }
    __syncthreads();
    if (tid < 128) st[tid] = bval - ssum[tid];
    __syncthreads();
    {
        const double t0 = st[2 * lane], t1 = st[2 * lane + 1];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            double2_t lv;
            __builtin_memcpy(&lv, &li[u], 16);
            acc[u][0] = fma(lv[1], t1, lv[0] * t0);
        }
    }
    {
        const double tot = wave_sums32(acc, lane);
        if (!(lane & 1)) ssum[wave * 32 + urow] = tot;
    }
    __syncthreads();
    if (tid < 128) {
        const double yv = s_fail ? __builtin_nan("") : ssum[tid];
        unsigned long long bits;
        __builtin_memcpy(&bits, &yv, 8);
        const unsigned long long tw = g.tag ^ (bits * GRANULE_HASH);
        const u32x4 v = {(unsigned)bits, (unsigned)(bits >> 32), (unsigned)tw, (unsigned)(tw >> 32)};
        __builtin_amdgcn_raw_buffer_store_b128(v, gsrc, (int)(((long)r * 128 + tid) * 16), 0, 16);      // one sc1 store per granule
        g.Y[(long)r * 128 + tid] = yv;
    }
    if (tid == 0) sweep_ticket_done(g.ticket);
}

}  // namespace

int launch_fwd_step(fvgp_handle *h, const double *L, int64_t ldl, int64_t np, int64_t k0, const double *linv_k,
                    double *B, int64_t ldb, double *Y, int c) {
    long rows = np - k0 - 128;
    long blocks = rows > 0 ? (rows + 31) / 32 : 1;   // 8 rows per wave-pass, 4 waves
    if (blocks > 2048) blocks = 2048;
    return dispatch_rhs_width(c, [&](auto C) {
        HIPLAUNCH((fwd_step_kernel<decltype(C)::value>), dim3((unsigned)blocks), dim3(256), h->stream, L, (long)ldl, (long)np, (long)k0, linv_k, B, (long)ldb, Y, c);
        return 0;
    });
}

int launch_bwd_step(fvgp_handle *h, const double *L, int64_t ldl, int64_t np, int64_t k0, const double *linv_k,
                    double *Yres, double *X, int64_t ldx, int c) {
    const long blocks = k0 > 0 ? k0 / 128 : 1;       // one workgroup per 128 columns to the left (k0 is a multiple of 128)
    return dispatch_rhs_width(c, [&](auto C) {
        HIPLAUNCH((bwd_step_kernel<decltype(C)::value>), dim3((unsigned)blocks), dim3(256), h->stream, L, (long)ldl, (long)np, (long)k0, linv_k, Yres, X, (long)ldx, c);
        return 0;
    });
}

// granules (16 bytes per row, tags of earlier launches never match) and the ticket words of the one-launch sweeps
static int sweep_buffers(fvgp_handle *h, int64_t np) {
    const size_t need = (size_t)np * 2;                              // doubles: 16 bytes per granule
    if (need > h->sweep_gran_cap) {
        if (h->sweep_gran) HIPCHK(hipFree(h->sweep_gran));
        h->sweep_gran = nullptr; h->sweep_gran_cap = 0;
        HIPCHK(hipMalloc((void **)&h->sweep_gran, need * sizeof(double)));
        HIPCHK(hipMemset(h->sweep_gran, 0, need * sizeof(double)));
        h->sweep_gran_cap = need;
    }
    if (!h->sweep_ticket) {
        HIPCHK(hipMalloc((void **)&h->sweep_ticket, 2 * sizeof(int)));
        HIPCHK(hipMemset(h->sweep_ticket, 0, 2 * sizeof(int)));
    }
    return 0;
}

// one sweep kernel over the np / 128 blocks of L (g: BwdSweepArgs or FwdSweepArgs without its last three fields): the handle's granules,
// a tag of its own and the ticket words go in here
template <class Args>
static int launch_sweep(fvgp_handle *h, void (*kernel)(Args), int64_t np, Args g) {
    int rc = sweep_buffers(h, np); if (rc) return rc;
    g.gran = h->sweep_gran; g.tag = ++h->sweep_tag; g.ticket = h->sweep_ticket;
    HIPLAUNCH(kernel, dim3((unsigned)(np / 128)), dim3(256), h->stream, g);
    return 0;
}

// the whole backward sweep in one launch (bwd_sweep_kernel, one right-hand side); Yres is only read
int launch_bwd_sweep(fvgp_handle *h, const double *L, int64_t ldl, int64_t np, const double *linv, const double *Yres, double *X, int64_t ldx, int c) {
    if (c != 1) { fvgp_set_error("bwd_sweep: one right-hand side"); return -9; }
    return launch_sweep(h, bwd_sweep_kernel, np, BwdSweepArgs{L, (long)ldl, (long)np, linv, Yres, X, (long)ldx});
}

// the whole forward sweep in one launch (fwd_sweep_kernel, one right-hand side): Y (np doubles) <- L^-1 B[:, 0]; B is only read
int launch_fwd_sweep(fvgp_handle *h, const double *L, int64_t ldl, int64_t np, const double *linv, const double *B, int64_t ldb, double *Y) {
    return launch_sweep(h, fwd_sweep_kernel, np, FwdSweepArgs{L, (long)ldl, (long)np, linv, B, (long)ldb, Y});
}
