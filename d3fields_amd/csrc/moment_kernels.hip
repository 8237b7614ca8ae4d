// moment_kernels.hip -- d3f_row_moments: weighted mean and centred scatter matrix of M rows of C channels (gfx950).
//
// The device half of a PCA fit (d3fields_amd/pca.py): wsum = sum w_m, mean_c = sum w_m x_mc / wsum and
// scatter_ij = sum_m w_m (x_mi - mean_i)(x_mj - mean_j) in float64, rows read as stored (fp32, or fp16 widened exactly, row
// stride >= C).  Dense arithmetic over every row (a row with w = 0 still multiplies: 0 * NaN = NaN), no atomics, a fixed
// summation order that depends on (M, C) alone: two runs are bit-identical, and the scatter is bitwise symmetric because only
// the lower triangle is computed and then mirrored.
//
// Four launches on one stream:
//   moment_sums_kernel      column sums sum w, sum w x_c of a row slab: one thread per channel, fmaf chains of kMomSumChain rows in
//                           fp32 folded into float64; one partial per slab in the workspace.
//   moment_mean_kernel      folds the slabs in order: wsum, mean (float64) and the shift m32 = fp32(mean).
//   moment_scatter_kernel   v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain per entry).  A workgroup owns a pair of 64-channel
//                           panels (I, J <= I) and a row slab; per stage of kMomRows rows it writes d = x - m32 (I panel) and w * d
//                           (J panel) into LDS in MFMA fragment order (linear, conflict-free reads), next stage's loads in flight
//                           meanwhile.  Each of the four waves owns 2 x 2 tiles of 16 x 16; the fp32 accumulators are flushed
//                           into float64 registers after every stage (chains of kMomRows = 64 rows), and the slab's float64 tile
//                           goes to the workspace.  Diagonal workgroups also accumulate sum w d (an MFMA against ones).
//   moment_fold_kernel      folds the slabs of a panel pair in order, subtracts the exact shift correction wsum * delta delta^T
//                           (delta = sum w d / wsum = mean - m32 up to rounding) and writes both triangles.
// Rows past a slab's end and channels past C enter as exact zeros (0 * 0).  16-byte (fp16: 8-byte) loads when the base pointer
// and the row stride allow; scalar loads otherwise.
#include "d3f_internal.h"
#include "d3f_device.h"

namespace d3f {

typedef _Float16 mom_f16x4 __attribute__((ext_vector_type(4)));

constexpr int kMomPanel = 64;                    // channels per panel
constexpr int kMomRows = 64;                     // rows per LDS stage = length of an fp32 chain before its float64 flush
constexpr int kMomBlock = 256;                   // four waves, 2 x 2 tiles of 16 x 16 each
constexpr int kMomSumChain = 32;                 // rows per fp32 chain of the column sums
constexpr int kMomSumSlabs = 2048;               // workgroups the column sums aim for
constexpr int kMomScatterGroups = 1024;          // workgroups the scatter pass aims for
constexpr int kMomMaxSlabs = 256;

static int64_t mom_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

MomentPlan moment_plan(int64_t M, int C)
{
    MomentPlan p;
    p.panels = (C + kMomPanel - 1) / kMomPanel;
    p.pairs = p.panels * (p.panels + 1) / 2;
    p.cpad = p.panels * kMomPanel;
    const int chunks = (C + kMomBlock - 1) / kMomBlock;
    int64_t want = mom_ceil(kMomSumSlabs, chunks);
    p.sum_rows = mom_ceil(mom_ceil(M, want), kMomSumChain) * kMomSumChain;
    p.sum_slabs = mom_ceil(M, p.sum_rows);
    want = mom_ceil(kMomScatterGroups, p.pairs);
    if (want > kMomMaxSlabs) want = kMomMaxSlabs;
    p.slab_rows = mom_ceil(mom_ceil(M, want), kMomRows) * kMomRows;
    p.slabs = mom_ceil(M, p.slab_rows);
    Carve c;
    p.off_wsum = c.take(8, 8);                                                          // double
    p.off_wsum_part = c.take(p.sum_slabs * 8, 8);                                       // double [sum_slabs]
    p.off_sum_part = c.take(p.sum_slabs * p.cpad * 8, 8);                               // double [sum_slabs][cpad]
    p.off_col_part = c.take(p.slabs * p.cpad * 8, 8);                                   // double [slabs][cpad]
    p.off_tiles = c.take(p.slabs * p.pairs * (int64_t)(kMomPanel * kMomPanel) * 8, 8);  // double [slabs][pairs][64][64]
    c.take((16 - c.at % 16) % 16, 1);                                                   // m32 starts at a multiple of 16 (the doubles so far may be an odd number)
    p.off_m32 = c.take((int64_t)p.cpad * 4, 4);                                         // float [cpad]
    c.take((256 - c.at % 256) % 256, 1);                                                // the whole is a multiple of 256
    p.bytes = c.at;
    return p;
}

int64_t row_moments_workspace_bytes(int64_t M, int C) { return moment_plan(M, C).bytes; }

struct MomentArgs {
    const char *rows;
    const float *w;                              // NULL: all ones
    int64_t M, stride;
    int C, cpad, half, vec, panels, pairs;
    int64_t sum_slabs, sum_rows, slabs, slab_rows;
    double *wsum, *wsum_part, *sum_part, *col_part, *tiles;
    float *m32;
    double *wsum_out, *mean_out, *scatter_out;
};

__device__ __forceinline__ float mom_load1(const MomentArgs &A, int64_t row, int c)
{
    const int64_t e = row * A.stride + c;
    return A.half ? (float)reinterpret_cast<const _Float16 *>(A.rows)[e] : reinterpret_cast<const float *>(A.rows)[e];
}

// pass 1: grid (channel chunks of kMomBlock, sum_slabs)
__global__ __launch_bounds__(kMomBlock) void moment_sums_kernel(const MomentArgs A)
{
    const int c = blockIdx.x * kMomBlock + threadIdx.x;
    const bool live = c < A.C;
    const int cc = live ? c : A.C - 1;           // idle lanes re-read the last channel and store nothing
    const int64_t r0 = (int64_t)blockIdx.y * A.sum_rows;
    const int64_t r1 = r0 + A.sum_rows < A.M ? r0 + A.sum_rows : A.M;
    double sx = 0.0, sw = 0.0;
    for (int64_t r = r0; r < r1; r += kMomSumChain) {
        float cx = 0.0f, cw = 0.0f;
        if (r + kMomSumChain <= r1) {
            float x[8], w[8];
#pragma unroll 1
            for (int k = 0; k < kMomSumChain; k += 8) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    x[i] = mom_load1(A, r + k + i, cc);
                    w[i] = A.w ? A.w[r + k + i] : 1.0f;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    cx = fmaf(w[i], x[i], cx);
                    cw = cw + w[i];
                }
            }
        } else {
            for (int64_t q = r; q < r1; ++q) {
                const float w = A.w ? A.w[q] : 1.0f;
                cx = fmaf(w, mom_load1(A, q, cc), cx);
                cw = cw + w;
            }
        }
        sx += (double)cx;
        sw += (double)cw;
    }
    if (live) A.sum_part[(int64_t)blockIdx.y * A.cpad + c] = sx;
    if (c == 0) A.wsum_part[blockIdx.y] = sw;
}

// folds pass 1: grid cpad / kMomBlock
__global__ __launch_bounds__(kMomBlock) void moment_mean_kernel(const MomentArgs A)
{
    const int c = blockIdx.x * kMomBlock + threadIdx.x;
    if (c >= A.cpad) return;
    double sw = 0.0, sx = 0.0;
    for (int64_t s = 0; s < A.sum_slabs; ++s) sw += A.wsum_part[s];
    if (c < A.C)
        for (int64_t s = 0; s < A.sum_slabs; ++s) sx += A.sum_part[s * A.cpad + c];
    const double mean = sx / sw;
    A.m32[c] = c < A.C ? (float)mean : 0.0f;
    if (c < A.C) A.mean_out[c] = mean;
    if (c == 0) { A.wsum[0] = sw; A.wsum_out[0] = sw; }
}

// channels c .. c+3 of a row (c a multiple of 4), widened to fp32; zero past C or for a row past the slab
__device__ __forceinline__ f32x4 mom_load4(const MomentArgs &A, int64_t row, int c, bool row_ok)
{
    f32x4 r = (f32x4)0.0f;
    if (!row_ok || c >= A.C) return r;
    const int64_t e = row * A.stride + c;
    if (A.vec && c + 4 <= A.C) {
        if (A.half) r = __builtin_convertvector(*reinterpret_cast<const mom_f16x4 *>(A.rows + e * 2), f32x4);
        else r = *reinterpret_cast<const f32x4 *>(A.rows + e * 4);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c + i < A.C) r[i] = A.half ? (float)reinterpret_cast<const _Float16 *>(A.rows)[e + i] : reinterpret_cast<const float *>(A.rows)[e + i];
    }
    return r;
}

// d = x - m32 on the live channels of a quad, exact zero on the padding
__device__ __forceinline__ f32x4 mom_centre(const MomentArgs &A, f32x4 x, f32x4 m, int c, bool row_ok)
{
    f32x4 d;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = (row_ok && c + i < A.C) ? x[i] - m[i] : 0.0f;
    return d;
}

// pass 2: grid (pairs, slabs)
__global__ __launch_bounds__(kMomBlock, 2) void moment_scatter_kernel(const MomentArgs A)
{
    // fragment order: [4-row step][16-channel tile][lane]: row 4 step + (lane >> 4), channel 16 tile + (lane & 15)
    __shared__ f32x4 Da[kMomRows * kMomPanel / 4];           // d of the I panel (the MFMA's A operand)
    __shared__ f32x4 Wb[kMomRows * kMomPanel / 4];           // w * d of the J panel (the B operand)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    const bool diag = I == J;
    const int64_t r0 = (int64_t)blockIdx.y * A.slab_rows;
    const int64_t r1 = r0 + A.slab_rows < A.M ? r0 + A.slab_rows : A.M;
    // loader: this thread's channel quad g of both panels, rows (threadIdx.x >> 4) + 16 q of a stage
    const int g = threadIdx.x & 15, lr = threadIdx.x >> 4;
    const int ci = I * kMomPanel + 4 * g, cj = J * kMomPanel + 4 * g;
    const f32x4 mi = *reinterpret_cast<const f32x4 *>(A.m32 + ci), mj = *reinterpret_cast<const f32x4 *>(A.m32 + cj);
    const int ti = 2 * (wv >> 1), tj = 2 * (wv & 1);         // this wave's tiles: (ti, ti + 1) x (tj, tj + 1)
    const bool cols = diag && ti == 0;                       // ... and the column sums of its J tiles

    double acc[2][2][4], col[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[a][b][i] = 0.0;
    col[0] = col[1] = 0.0;

    f32x4 xi[4], xj[4];
    float w[4];
    auto fetch = [&](int64_t base) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = base + lr + 16 * q;
            const bool ok = row < r1;
            xi[q] = mom_load4(A, row, ci, ok);
            xj[q] = diag ? xi[q] : mom_load4(A, row, cj, ok);
            w[q] = ok ? (A.w ? A.w[row] : 1.0f) : 0.0f;
        }
    };
    fetch(r0);
    for (int64_t base = r0; base < r1; base += kMomRows) {
        __syncthreads();                                     // the previous stage has been read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = lr + 16 * q;
            const bool ok = base + row < r1;
            const f32x4 di = mom_centre(A, xi[q], mi, ci, ok);
            const f32x4 dj = mom_centre(A, xj[q], mj, cj, ok);
            f32x4 wd;
#pragma unroll
            for (int i = 0; i < 4; ++i) wd[i] = ok ? w[q] * dj[i] : 0.0f;
            const int slot = (((row >> 2) * 4 + (g >> 2)) * 64 + (row & 3) * 16 + (g & 3) * 4) >> 2;
            Da[slot] = di;
            Wb[slot] = wd;
        }
        __syncthreads();
        if (base + kMomRows < r1) fetch(base + kMomRows);    // in flight under the MFMAs
        f32x4 t[2][2], tc[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) t[a][b] = (f32x4)0.0f;
        tc[0] = tc[1] = (f32x4)0.0f;
        const float *da = reinterpret_cast<const float *>(Da), *wb = reinterpret_cast<const float *>(Wb);
#pragma unroll 4
        for (int s = 0; s < kMomRows / 4; ++s) {
            const float a0 = da[(s * 4 + ti) * 64 + lane], a1 = da[(s * 4 + ti + 1) * 64 + lane];
            const float b0 = wb[(s * 4 + tj) * 64 + lane], b1 = wb[(s * 4 + tj + 1) * 64 + lane];
            t[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, t[0][0], 0, 0, 0);
            t[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, t[0][1], 0, 0, 0);
            t[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, t[1][0], 0, 0, 0);
            t[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, t[1][1], 0, 0, 0);
            if (cols) {                                      // wave-uniform: 1 * (w d) summed over the rows, every output row alike
                tc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b0, tc[0], 0, 0, 0);
                tc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b1, tc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[a][b][i] += (double)t[a][b][i];
        col[0] += (double)tc[0][0];
        col[1] += (double)tc[1][0];
    }
    // this lane's entries: panel row 16 (ti + a) + 4 (lane >> 4) + i, panel column 16 (tj + b) + (lane & 15)
    double *tile = A.tiles + ((int64_t)blockIdx.y * A.pairs + blockIdx.x) * (kMomPanel * kMomPanel);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                tile[(16 * (ti + a) + 4 * (lane >> 4) + i) * kMomPanel + 16 * (tj + b) + (lane & 15)] = acc[a][b][i];
    if (cols && lane < 16) {
        double *cp = A.col_part + (int64_t)blockIdx.y * A.cpad + J * kMomPanel;
        cp[16 * tj + lane] = col[0];
        cp[16 * (tj + 1) + lane] = col[1];
    }
}

// pass 3: grid (pairs, 4): a quarter of a pair's 64 x 64 tile per workgroup
__global__ __launch_bounds__(kMomBlock) void moment_fold_kernel(const MomentArgs A)
{
    __shared__ double delta[2][kMomPanel];
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    const double wsum = A.wsum[0];
    if (threadIdx.x < 2 * kMomPanel) {
        const int side = threadIdx.x >> 6, c = (side ? J : I) * kMomPanel + (threadIdx.x & 63);
        double s = 0.0;
        for (int64_t k = 0; k < A.slabs; ++k) s += A.col_part[k * A.cpad + c];
        delta[side][threadIdx.x & 63] = s / wsum;
    }
    __syncthreads();
    for (int e = blockIdx.y * 1024 + threadIdx.x; e < (int)(blockIdx.y + 1) * 1024; e += kMomBlock) {
        const int i = e >> 6, j = e & 63;
        const int gi = I * kMomPanel + i, gj = J * kMomPanel + j;
        if (gi >= A.C || gj >= A.C || (I == J && j > i)) continue;
        double s = 0.0;
        for (int64_t k = 0; k < A.slabs; ++k) s += A.tiles[(k * A.pairs + blockIdx.x) * (kMomPanel * kMomPanel) + e];
        const double v = s - (wsum * delta[0][i]) * delta[1][j];
        A.scatter_out[(int64_t)gi * A.C + gj] = v;
        A.scatter_out[(int64_t)gj * A.C + gi] = v;
    }
}

hipError_t launch_row_moments(const void *rows, bool half, int64_t M, int C, int64_t row_stride, const float *weights, double *wsum_out,
                              double *mean_out, double *scatter_out, void *workspace, hipStream_t s)
{
    const MomentPlan p = moment_plan(M, C);
    MomentArgs A;
    A.rows = static_cast<const char *>(rows);
    A.w = weights;
    A.M = M; A.stride = row_stride;
    A.C = C; A.cpad = p.cpad; A.half = half ? 1 : 0;
    A.vec = (reinterpret_cast<uintptr_t>(rows) % (half ? 8 : 16) == 0 && row_stride % 4 == 0) ? 1 : 0;
    A.panels = p.panels; A.pairs = p.pairs;
    A.sum_slabs = p.sum_slabs; A.sum_rows = p.sum_rows; A.slabs = p.slabs; A.slab_rows = p.slab_rows;
    A.wsum = static_cast<double *>(ws_at(workspace, p.off_wsum));
    A.wsum_part = static_cast<double *>(ws_at(workspace, p.off_wsum_part));
    A.sum_part = static_cast<double *>(ws_at(workspace, p.off_sum_part));
    A.col_part = static_cast<double *>(ws_at(workspace, p.off_col_part));
    A.tiles = static_cast<double *>(ws_at(workspace, p.off_tiles));
    A.m32 = static_cast<float *>(ws_at(workspace, p.off_m32));
    A.wsum_out = wsum_out; A.mean_out = mean_out; A.scatter_out = scatter_out;
    hipLaunchKernelGGL(moment_sums_kernel, dim3((unsigned)((C + kMomBlock - 1) / kMomBlock), (unsigned)p.sum_slabs), dim3(kMomBlock), 0, s, A);
    hipLaunchKernelGGL(moment_mean_kernel, dim3((unsigned)((p.cpad + kMomBlock - 1) / kMomBlock)), dim3(kMomBlock), 0, s, A);
    hipLaunchKernelGGL(moment_scatter_kernel, dim3((unsigned)p.pairs, (unsigned)p.slabs), dim3(kMomBlock), 0, s, A);
    hipLaunchKernelGGL(moment_fold_kernel, dim3((unsigned)p.pairs, 4), dim3(kMomBlock), 0, s, A);
    return hipGetLastError();
}

} // namespace d3f
