// Joint Gaussian draws on the device: a counter-based normal generator and Y = mean + (L Z)^T from a Cholesky factor
// (fvgp_hip_normal_fill, fvgp_hip_mvn_sample).
//
// The generator has no state: z(seed, stream, i, j) is Philox4x32-10 (Salmon et al., SC 2011; the Random123 constants) on the counter
// (i, j, lo32(stream), hi32(stream)) with the key (lo32(seed), hi32(seed)), its four output words w0..w3 turned into two uniforms of 53
// bits in (0, 1] and one Box-Muller cosine branch:
//     u1 = (((w0 | w1 << 32) >> 11) + 0.5) 2^-53      u2 likewise from w2, w3      z = sqrt(-2 ln u1) cos(2 pi u2)
// ONE counter per element: element (i, j) depends on nothing but its four arguments -- not on its neighbours, the launch shape or how a
// caller cuts a request into calls.  tests/samples_ref.py is the numpy twin.
//
// The draw: Z (padded, zero padding) into the caller's scratch; the diagonal 128-tiles of L copied there with everything above the
// diagonal (and every column from n on) zeroed, since L itself is const and its strict upper triangle holds whatever the factored matrix
// held; C = D Z, one strided-batch product over the diagonal tiles, then C += L Z over the tiles below the diagonal with the K range of
// tile row ti ending at the diagonal tile -- both on the 128-tile MFMA kernel through GemmDesc with an explicit K range (never the
// 64-tile kernel, never split K); a transposing epilogue adds the mean and writes sample-major.  Every sum of an output element sees
// its row of L and its column of Z only, in an order fixed by the row: a sample's bits do not depend on nsamp, samp0 or its neighbours.
#include "common.h"
#include "normal.h"
#include <math.h>

namespace {

struct FillArgs {
    uint32_t k0, k1, s0, s1;
    long row0, col0;
    double *Z; long ld; int vec;            // rows_all x cols_all are written: the normals where r < rows, c < cols, zero elsewhere
    long rows, cols, rows_all, cols_all;
    double *Z2; long ld2; int vec2;         // or nullptr: the rows x cols normals once more (the caller's copy)
    long col_blocks;
};

// two neighbouring elements of a row: one 16-byte store where the row's base allows it
__device__ __forceinline__ void put2(double *Z, long ld, int vec, long r, long c, long cend, double v0, double v1) {
    double *p = Z + r * ld + c;
    if (vec && c + 1 < cend) *reinterpret_cast<double2_t *>(p) = (double2_t){v0, v1};
    else { p[0] = v0; if (c + 1 < cend) p[1] = v1; }
}

// a workgroup fills 4 rows x 128 columns; a wave one row of them (64 lanes x 16 bytes, contiguous)
__global__ __launch_bounds__(256) void normal_fill_kernel(FillArgs g) {
    const long rb = (long)blockIdx.x / g.col_blocks, cb = (long)blockIdx.x % g.col_blocks;
    const long r = rb * 4 + (threadIdx.x >> 6), c = cb * 128 + 2 * (threadIdx.x & 63);
    if (r >= g.rows_all || c >= g.cols_all) return;
    double v0 = 0.0, v1 = 0.0;
    if (r < g.rows) {
        const uint32_t i = (uint32_t)(g.row0 + r);
        if (c < g.cols) v0 = normal_at(g.k0, g.k1, g.s0, g.s1, i, (uint32_t)(g.col0 + c));
        if (c + 1 < g.cols) v1 = normal_at(g.k0, g.k1, g.s0, g.s1, i, (uint32_t)(g.col0 + c + 1));
    }
    put2(g.Z, g.ld, g.vec, r, c, g.cols_all, v0, v1);
    if (g.Z2 && r < g.rows && c < g.cols) put2(g.Z2, g.ld2, g.vec2, r, c, g.cols, v0, v1);
}

// D[b] = the b-th diagonal 128-tile of L with the entries above the diagonal and the columns from n on zeroed; those entries of L are
// not loaded
__global__ __launch_bounds__(256) void diag_tiles_lower_kernel(const double *L, long ldl, long n, double *D) {
    const long b = blockIdx.x, base = b * TILE;
    const double *Lb = L + base * ldl + base;
    double *Db = D + b * (long)LEAF_DOUBLES;
    const int c = 2 * (threadIdx.x & 63);
    for (int r = threadIdx.x >> 6; r < TILE; r += 4) {
        const double v0 = (c <= r && base + c < n) ? Lb[r * ldl + c] : 0.0;
        const double v1 = (c + 1 <= r && base + c + 1 < n) ? Lb[r * ldl + c + 1] : 0.0;
        *reinterpret_cast<double2_t *>(Db + r * TILE + c) = (double2_t){v0, v1};
    }
}

// Y[s][p] = mean[p] + C[p][s], s < nsamp, p < n: 64 x 64 pieces through LDS, 16-byte loads of C (padded: whole pieces exist) and
// 16-byte stores into Y where its rows allow them
__global__ __launch_bounds__(256) void sample_epilogue_kernel(const double *C, long ldc, const double *mean, long n, long nsamp,
                                                              double *Y, long ldy, int vec) {
    __shared__ double t[64][65];
    const long p0 = (long)blockIdx.x * 64, s0 = (long)blockIdx.y * 64;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    for (int rr = hi; rr < 64; rr += 8) {
        const double2_t v = *reinterpret_cast<const double2_t *>(C + (p0 + rr) * ldc + s0 + 2 * lo);
        t[rr][2 * lo] = v[0]; t[rr][2 * lo + 1] = v[1];
    }
    __syncthreads();
    const long p = p0 + 2 * lo;
    if (p >= n) return;
    const double m0 = mean ? mean[p] : 0.0, m1 = (mean && p + 1 < n) ? mean[p + 1] : 0.0;
    for (int ss = hi; ss < 64; ss += 8) {
        const long s = s0 + ss;
        if (s >= nsamp) break;
        put2(Y, ldy, vec, s, p, n, m0 + t[2 * lo][ss], m1 + t[2 * lo + 1][ss]);
    }
}

constexpr int64_t TWO_32 = (int64_t)1 << 32;

int vec_ok(const double *p, int64_t ld) { return (((uintptr_t)p & 15) == 0 && (ld & 1) == 0) ? 1 : 0; }

int launch_normal_fill(fvgp_handle *h, uint64_t seed, uint64_t stream, int64_t row0, int64_t col0, double *Z, int64_t ld,
                       int64_t rows, int64_t cols, int64_t rows_all, int64_t cols_all, double *Z2, int64_t ld2) {
    FillArgs g;
    g.k0 = (uint32_t)seed; g.k1 = (uint32_t)(seed >> 32); g.s0 = (uint32_t)stream; g.s1 = (uint32_t)(stream >> 32);
    g.row0 = row0; g.col0 = col0;
    g.Z = Z; g.ld = ld; g.vec = vec_ok(Z, ld);
    g.rows = rows; g.cols = cols; g.rows_all = rows_all; g.cols_all = cols_all;
    g.Z2 = Z2; g.ld2 = ld2; g.vec2 = Z2 ? vec_ok(Z2, ld2) : 0;
    g.col_blocks = (cols_all + 127) / 128;
    const int64_t blocks = (rows_all + 3) / 4 * g.col_blocks;
    if (blocks > 0x7fffffffLL) { fvgp_set_error("normal_fill: more than 2^31 workgroups; fill the block in pieces"); return -7; }
    hipLaunchKernelGGL(normal_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, g);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int fvgp_hip_normal_fill(fvgp_handle *h, uint64_t seed, uint64_t stream, int64_t row0, int64_t col0,
                         double *Z, int64_t rows, int64_t cols, int64_t ldz) {
    if (!h) return -1;
    if (!Z || ((uintptr_t)Z & 7)) return -6;
    if (rows < 1) return -7;
    if (cols < 1) return -8;
    if (ldz < cols) return -9;
    if (row0 < 0 || row0 > TWO_32 || rows > TWO_32 - row0) { fvgp_set_error("normal_fill: row indices must stay below 2^32"); return -4; }
    if (col0 < 0 || col0 > TWO_32 || cols > TWO_32 - col0) { fvgp_set_error("normal_fill: column indices must stay below 2^32"); return -5; }
    HIPCHK(hipSetDevice(h->device));
    return launch_normal_fill(h, seed, stream, row0, col0, Z, ldz, rows, cols, rows, cols, nullptr, 0);
}

// fvgp_hip_mvn_sample's scratch: Z and C = L Z (padded n by padded nsamp each), the masked diagonal tiles D
struct SampleWs { double *Z, *C, *D; };
static SampleWs sample_layout(Carve &c, int64_t n, int64_t nsamp) {
    const int64_t np = pad128(n), sp = pad128(nsamp);
    return {c.take<double>(np * sp), c.take<double>(np * sp), c.take<double>(np * TILE)};
}

int64_t fvgp_hip_mvn_sample_workspace_bytes(int64_t n, int64_t nsamp) {
    if (n < 1 || nsamp < 1) return -1;
    return carve_bytes(sample_layout, n, nsamp);
}

int fvgp_hip_mvn_sample(fvgp_handle *h, const double *L, int64_t n, int64_t ldl, const double *mean,
                        uint64_t seed, uint64_t stream, int64_t samp0, int64_t nsamp,
                        double *Y, int64_t ldy, double *Z_out, int64_t ldz, double *work, int64_t work_bytes) {
    if (!h) return -1;
    int rc = check_square(L, n, ldl, 2, 3, 4);
    if (rc) return rc;
    if (n > TWO_32) { fvgp_set_error("mvn_sample: n must stay below 2^32"); return -3; }
    if (ldl >= ((int64_t)1 << 21)) { fvgp_set_error("mvn_sample: ldl must be below 2^21"); return -4; }
    if (mean && ((uintptr_t)mean & 7)) return -5;
    if (nsamp < 1 || pad128(nsamp) >= ((int64_t)1 << 21)) { fvgp_set_error("mvn_sample: 1 <= nsamp, padded below 2^21 per call"); return -9; }
    if (samp0 < 0 || samp0 > TWO_32 || nsamp > TWO_32 - samp0) { fvgp_set_error("mvn_sample: sample indices must stay below 2^32"); return -8; }
    if (!Y || ((uintptr_t)Y & 7)) return -10;
    if (ldy < n) return -11;
    if (Z_out && ((uintptr_t)Z_out & 7)) return -12;
    if (Z_out && ldz < nsamp) return -13;
    if (!work || ((uintptr_t)work & 15)) { fvgp_set_error("mvn_sample: work must be 16-byte aligned"); return -14; }
    Carve c(work); const SampleWs l = sample_layout(c, n, nsamp);
    if (work_bytes < c.bytes()) {
        fvgp_set_error("mvn_sample: work smaller than fvgp_hip_mvn_sample_workspace_bytes(n, nsamp)"); return -15;
    }
    HIPCHK(hipSetDevice(h->device));
    const int64_t np = pad128(n), sp = pad128(nsamp), nb = np / TILE;
    double *Z = l.Z, *C = l.C, *D = l.D;

    rc = launch_normal_fill(h, seed, stream, 0, samp0, Z, sp, n, nsamp, np, sp, Z_out, ldz); if (rc) return rc;
    hipLaunchKernelGGL(diag_tiles_lower_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, L, (long)ldl, (long)n, D);
    HIPCHK(hipGetLastError());
    // C[b] = D[b] Z[b]: the diagonal tiles, one problem of the strided batch each (tile row b of C, block row b of Z)
    rc = launch_gemm(h, gemm_desc(0, 1, TILE, sp, TILE, 1.0, D, TILE, Z, sp, 0.0, C, sp).k_end(TILE)
                            .batched(nb, LEAF_DOUBLES, (int64_t)TILE * sp, (int64_t)TILE * sp));
    if (rc) return rc;
    // C += L Z over the tiles of L below the diagonal: tile row ti of the rows from 128 on ends its K range at 128 (ti + 1)
    if (nb > 1) {
        rc = launch_gemm(h, gemm_desc(0, 1, np - TILE, sp, np - TILE, 1.0, L + (int64_t)TILE * ldl, ldl, Z, sp, 1.0, C + (int64_t)TILE * sp, sp)
                                .k_end(TILE, TILE, 0));
        if (rc) return rc;
    }
    hipLaunchKernelGGL(sample_epilogue_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((nsamp + 63) / 64)), dim3(256), 0, h->stream,
                       (const double *)C, (long)sp, mean, (long)n, (long)nsamp, Y, (long)ldy, vec_ok(Y, ldy));
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
