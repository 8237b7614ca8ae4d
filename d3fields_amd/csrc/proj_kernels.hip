// proj_kernels.hip -- d3f_project_maps: a channel map through a linear head, [V,fh,fw,C] -> [V,fh,fw,k] (gfx950).
//
// Fusion is linear in the channel vector, so a query of k projected channels may project the MAPS once per observation and
// query the k-channel result through the ordinary kernel families ("Projected queries").  This file is that one
// streaming pass: a skinny GEMM  dst[t, j] = sum_c src[t, c] * W[j, c]  over every texel t, read as stored (fp32, or fp16
// widened exactly, explicit strides), dense multiply-accumulate over ALL channels (fp32 products in short fp32 chains, chain
// sums added in float64 and rounded to fp32 once; a NaN texel makes its k outputs NaN, zero weights included), no atomics, a
// fixed summation order per instance (two runs are bit-identical).
//
// Two instances:
//   project_lanes_kernel (k <= 4)   16 lanes share a texel, each lane owns 4 consecutive channels of every 64 (one 16-byte load
//       per texel and step, 256 contiguous bytes per texel), four texels per lane group and W read once per step from LDS for
//       the four of them; k partial sums per texel and lane, folded over the 16 lanes by DPP (two quad permutes, row half
//       mirror, row mirror).  k/2 flop per byte: the vector ALUs idle behind HBM.
//   project_mfma_kernel (5 <= k <= 64)  v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain per output and 16-channel step): 16 texels x 16
//       outputs per tile, ceil(k/16) tiles per texel group, two texel groups per wave and eight waves against one W fragment.  Lane l loads the 16
//       bytes (4 channels) of texel l & 15 at channel quad l >> 4 of a 16-channel step and feeds them to four MFMAs; W waits
//       in LDS in exactly that fragment order, so its reads are linear.  From k ~ 16 the vector ALUs would need more issue
//       cycles than HBM leaves (2k flop per 4 bytes against 64 flop/clk/SIMD).  Measured: k = 3 streams at 1.0x a
//       bare read of a dense map (3x on a 50 MB map: 192 workgroups do not hide the load latency of its 16 serial steps); this
//       instance takes 2x at k = 16 and 3x at k = 64, bound by instruction issue and MFMA dependencies, not by HBM.
// In both, every product and the short chains are fp32; the step sums of a lane are added in float64 and rounded to fp32 once (a
// single fp32 chain over 1024 channels rounds every small term at the size of the running total and misses the per-entry pin).
// Channels past C and outputs past k are zero-padded in LDS (and the texel lanes past C load nothing): 0 * 0 adds an exact zero.
#include "d3f_internal.h"
#include "d3f_device.h"

namespace d3f {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct ProjArgs {
    const char *data;       // source map, element (v,y,x,c) at data[(v*sv + y*sy + x*sx + c) * esize]
    const float *W;         // [k,C]
    float *dst;             // [T,k]
    int64_t sv, sy, sx, T;  // strides in elements; T = V*fh*fw texels
    int fh, fw, C, k;
    int half;               // fp16 storage
    int vec;                // every 4-channel group of every texel is one aligned vector load
    int chunk;              // channels of W resident in LDS at a time
};

constexpr int kProjLaneK = 4;                    // project_lanes_kernel: k <= 4
constexpr int kProjLaneChunk = 2048;             // its W chunk: 4 x 2048 floats = 32 KB
constexpr int kProjMfmaFloats = 16384;           // project_mfma_kernel: 64 KB of W fragments
constexpr int kProjMfmaBlock = 512;              // ... shared by eight waves

__device__ __forceinline__ int64_t proj_texel_offset(const ProjArgs &A, int64_t t)
{
    t = t < A.T ? t : A.T - 1;                   // lanes past the end re-read the last texel and store nothing
    const int64_t hw = (int64_t)A.fh * A.fw;
    const int64_t v = t / hw, r = t - v * hw;
    const int64_t y = r / A.fw, x = r - y * A.fw;
    return v * A.sv + y * A.sy + x * A.sx;
}

// channels c .. c+3 of the texel at element offset `off` (c is a multiple of 4), widened to fp32; zero past C
__device__ __forceinline__ f32x4 proj_load4(const ProjArgs &A, int64_t off, int c)
{
    f32x4 r = (f32x4)0.0f;
    if (c >= A.C) return r;
    if (A.vec && c + 4 <= A.C) {
        if (A.half) r = __builtin_convertvector(__builtin_nontemporal_load(reinterpret_cast<const f16x4 *>(A.data + (off + c) * 2)), f32x4);
        else r = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(A.data + (off + c) * 4));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c + i < A.C)
                r[i] = A.half ? (float)reinterpret_cast<const _Float16 *>(A.data)[off + c + i] : reinterpret_cast<const float *>(A.data)[off + c + i];
    }
    return r;
}

template <int CTRL> __device__ __forceinline__ float proj_dpp_add(float v)
{
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(float, o);
}

__global__ __launch_bounds__(kBlock, 3) void project_lanes_kernel(const ProjArgs A)
{
    __shared__ float Ws[kProjLaneK * kProjLaneChunk];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, q = lane & 15;
    const int C = A.C, k = A.k, CC = A.chunk;
    const bool one_chunk = C <= CC;
    const int64_t tiles = (A.T + 63) / 64;
    bool staged = false;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * 64 + (wv * 4 + g) * 4;
        int64_t off[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) off[t] = proj_texel_offset(A, t0 + t);
        double acc[4][kProjLaneK];               // a step's four products are an fp32 fmaf chain from zero; step sums add up in float64
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < kProjLaneK; ++kk) acc[t][kk] = 0.0;
        for (int c0 = 0; c0 < C; c0 += CC) {
            const int cend = min(CC, (C - c0 + 63) / 64 * 64);         // channels of this chunk, padded to whole steps
            if (!(one_chunk && staged)) {
                __syncthreads();
                for (int i = threadIdx.x; i < k * cend; i += kBlock) {
                    const int kk = i / cend, cc = i - kk * cend;
                    Ws[kk * CC + cc] = c0 + cc < C ? A.W[(int64_t)kk * C + c0 + cc] : 0.0f;
                }
                __syncthreads();
                staged = true;
            }
#pragma unroll 1
            for (int cs = 4 * q; cs < cend; cs += 64) {
                f32x4 x[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) x[t] = proj_load4(A, off[t], c0 + cs);
#pragma unroll
                for (int kk = 0; kk < kProjLaneK; ++kk) {
                    if (kk < k) {
                        const f32x4 w = *reinterpret_cast<const f32x4 *>(&Ws[kk * CC + cs]);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            float s = x[t].x * w.x;
                            s = fmaf(x[t].y, w.y, s);
                            s = fmaf(x[t].z, w.z, s);
                            s = fmaf(x[t].w, w.w, s);
                            acc[t][kk] += (double)s;
                        }
                    }
                }
            }
        }
        // fold the 16 lanes of a texel: xor 1, xor 2 (quad permutes), then the mirrored half (8) and row (16); both sides of
        // every pair add the same two numbers, so all 16 lanes end with the same sum
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int kk = 0; kk < kProjLaneK; ++kk) {
                if (kk < k) {
                    float s = (float)acc[t][kk];
                    s = proj_dpp_add<0xB1>(s);      // quad_perm [1,0,3,2]
                    s = proj_dpp_add<0x4E>(s);      // quad_perm [2,3,0,1]
                    s = proj_dpp_add<0x141>(s);     // row_half_mirror
                    s = proj_dpp_add<0x140>(s);     // row_mirror
                    if (q == 0 && t0 + t < A.T) A.dst[(t0 + t) * k + kk] = s;
                }
            }
    }
}

__global__ __launch_bounds__(kProjMfmaBlock, 4) void project_mfma_kernel(const ProjArgs A)
{
    __shared__ f32x4 Wf[kProjMfmaFloats / 4];    // fragment order: [step][tile][lane] -> W[16 tile + (lane & 15)][16 step + 4 (lane >> 4) + 0..3]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = lane & 15, ls = lane >> 4;
    const int C = A.C, k = A.k, CC = A.chunk;
    const int nt = (k + 15) >> 4;
    const bool one_chunk = C <= CC;
    const int64_t tiles = (A.T + 255) / 256;
    bool staged = false;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * 256 + wv * 32;                         // eight waves x two groups of 16 texels
        int64_t off[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) off[m] = proj_texel_offset(A, t0 + m * 16 + lc);
        f64x4 acc[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) acc[m][w] = (f64x4)0.0;
        for (int c0 = 0; c0 < C; c0 += CC) {
            const int S = (min(CC, C - c0) + 15) >> 4;                   // 16-channel steps of this chunk
            if (!(one_chunk && staged)) {
                __syncthreads();
                float *Wl = reinterpret_cast<float *>(Wf);
                for (int i = threadIdx.x; i < S * nt * 256; i += kProjMfmaBlock) {
                    const int i4 = i & 3, ln = (i >> 2) & 63, sw = i >> 8;
                    const int s = sw / nt, w = sw - s * nt;
                    const int j = 16 * w + (ln & 15), c = c0 + 16 * s + 4 * (ln >> 4) + i4;
                    Wl[i] = (j < k && c < C) ? A.W[(int64_t)j * C + c] : 0.0f;
                }
                __syncthreads();
                staged = true;
            }
            f32x4 a[2], an[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) an[m] = a[m] = proj_load4(A, off[m], c0 + 4 * ls);
            for (int s = 0; s < S; ++s) {
                if (s + 1 < S) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) an[m] = proj_load4(A, off[m], c0 + 16 * (s + 1) + 4 * ls);
                }
                // the 16 channels of a step are one fmaf chain from zero on the matrix cores; the step sums are added in float64
                // (one chain over C = 1024 channels would round every small term at the size of the running total)
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (w < nt) {
                        const f32x4 b = Wf[(s * nt + w) * 64 + lane];
                        f32x4 blk[2];
#pragma unroll
                        for (int m = 0; m < 2; ++m) blk[m] = (f32x4)0.0f;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int m = 0; m < 2; ++m) blk[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][i], b[i], blk[m], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < 2; ++m) acc[m][w] += __builtin_convertvector(blk[m], f64x4);
                    }
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) a[m] = an[m];
            }
        }
        // this lane's results: texels t0 + 16 m + 4 ls + i, output 16 w + lc
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int j = 16 * w + lc;
                if (w < nt && j < k) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int64_t t = t0 + m * 16 + 4 * ls + i;
                        if (t < A.T) A.dst[t * k + j] = (float)acc[m][w][i];
                    }
                }
            }
    }
}

hipError_t launch_project_maps(const void *data, int V, int fh, int fw, int C, int64_t sv, int64_t sy, int64_t sx, bool half, const float *W,
                               int k, float *dst, hipStream_t s)
{
    ProjArgs A;
    A.data = static_cast<const char *>(data);
    A.W = W;
    A.dst = dst;
    A.sv = sv; A.sy = sy; A.sx = sx;
    A.T = (int64_t)V * fh * fw;
    A.fh = fh; A.fw = fw; A.C = C; A.k = k;
    A.half = half ? 1 : 0;
    const uintptr_t need = half ? 8 : 16;
    A.vec = (reinterpret_cast<uintptr_t>(data) % need == 0 && sv % 4 == 0 && sy % 4 == 0 && sx % 4 == 0) ? 1 : 0;
    if (k <= kProjLaneK) {
        A.chunk = kProjLaneChunk;
        const int64_t tiles = (A.T + 63) / 64;
        hipLaunchKernelGGL(project_lanes_kernel, dim3((unsigned)(tiles < 256 * 3 ? tiles : 256 * 3)), dim3(kBlock), 0, s, A);
    } else {
        const int nt = (k + 15) / 16;
        A.chunk = kProjMfmaFloats / 16 / nt / 16 * 16;             // 16 * nt * chunk floats of fragments fit the 64 KB
        const int64_t tiles = (A.T + 255) / 256;
        hipLaunchKernelGGL(project_mfma_kernel, dim3((unsigned)(tiles < 256 * 2 ? tiles : 256 * 2)), dim3(kProjMfmaBlock), 0, s, A);
    }
    return hipGetLastError();
}

} // namespace d3f
