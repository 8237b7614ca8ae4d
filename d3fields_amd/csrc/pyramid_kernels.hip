// pyramid_kernels.hip -- a baked field at half the resolution (include/d3fields_hip_pyramid.h, d3f_volume_coarsen_select and
// d3f_volume_coarsen_rows).
//
// The contract (restated in tests/pyramid_cases.py).  Fine grid nx x ny x nz, flat index q = (x*ny + y)*nz + z; coarse grid of ceil(n/2) per
// axis, flat index Q = (X*cy + Y)*cz + Z.  The children of (X, Y, Z) are (2X + i, 2Y + j, 2Z + k), i, j, k in {0, 1}, inside the fine volume,
// numbered c = 4i + 2j + k: ascending c is ascending fine flat index.  float32, one rounding per operation, nothing contracted (the build has
// -ffp-contract=off and this file names no contracted operation):
//   select  a child is USABLE iff valid != 0 and dist is not NaN; dist of a child that is not valid is never read.  children = the usable
//           bits, count their number, valid = count >= min_children, dist = sum * (1.0f / (float)count) with sum one accumulator from +0 over
//           the usable children in ascending c; 1e3 where not valid.
//   rows    child c of a listed Q CONTRIBUTES iff bit c of children[Q] is set, the child lies inside and the source is dense or
//           slot[child] >= 0.  n_r contributors: every channel is acc * (1.0f / (float)n_r), acc one accumulator from +0 over the contributors
//           in ascending c.  n_r == 0: the fill row, known = 0.
// A child that does not contribute is loaded as +0 and added all the same: acc starts at +0 and x + (+0) has the bits of x for every x but
// -0, which a sum that started at +0 never is.  So all eight loads of a step are issued together and the adds carry no branch.
//
//   coarsen_select_kernel  one lane per coarse voxel, Z along the lanes: eight valid bytes, up to eight distances, three stores
//   coarsen_rows_kernel    the two forms of merge_rows_kernel: one lane per listed voxel decides, writes out_known and the sets of up to 16
//                          channels; for the wider sets sixteen lanes take one voxel along the channels.  They get the voxel and its mask by
//                          shuffles and read the eight slots themselves.  WIDE: the launch has a set wider than 16 channels.  HALF: it has a
//                          set stored as IEEE half (a step is one 16-byte load of eight channels per child, widened exactly by
//                          volume_rows.h's widen); the float32-only instance carries no conversion.
// A streaming pass: eight rows read for one written.  No LDS, no atomics, no workspace, nothing waits for another workgroup: two runs give
// identical bytes.  Every output is written completely; the caller's buffers may hold anything.
#include "d3f_internal.h"
#include "volume_rows.h"      // widen: a stored half to float32, exactly

namespace d3f {

namespace {

constexpr int kNoVoxel = -2, kOutside = -1;      // the mask a lane holds: past the list / a listed entry outside the coarse volume
constexpr float kSentinel = 1e3f;

__global__ __launch_bounds__(kBlock) void coarsen_select_kernel(const CoarsenSelectArgs P)
{
    const int64_t Q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (Q >= P.nc) return;
    const int Z = (int)(Q % P.cz), XY = (int)(Q / P.cz), Y = XY % P.cy, X = XY / P.cy;
    float d[8];
    unsigned mask = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int x = 2 * X + (c >> 2), y = 2 * Y + ((c >> 1) & 1), z = 2 * Z + (c & 1);
        d[c] = 0.0f;
        if (x < P.nx && y < P.ny && z < P.nz) {
            const int64_t q = ((int64_t)x * P.ny + y) * P.nz + z;
            if (P.valid[q] != 0) {
                const float t = P.dist[q];
                if (t == t) {
                    d[c] = t;
                    mask |= 1u << c;
                }
            }
        }
    }
    const int count = __popc(mask);
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (mask & (1u << c)) sum = sum + d[c];
    const bool ok = count >= P.min_children;
    float out = kSentinel;
    if (ok) {
        const float inv = 1.0f / (float)count;
        out = sum * inv;
    }
    P.out_dist[Q] = out;
    P.out_valid[Q] = ok ? 1 : 0;
    P.out_children[Q] = (uint8_t)mask;
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------
struct CoarsenRows {
    const uint8_t *children;
    const int32_t *voxels;
    const int32_t *slot;
    uint8_t *out_known;
    int64_t m, nc;
    int32_t nx, ny, nz, cy, cz;
    int32_t n_sets, banded;
    CoarsenSet sets[D3F_MAX_MAPS];
};

struct Kids {
    int32_t row[8];        // the source row of child c (a voxel or a slot), -1: it does not contribute
    int n;
};

// mask: children[Q] (0..255), or kOutside
__device__ __forceinline__ Kids kids_of(const CoarsenRows &P, int mask, int Q)
{
    Kids k;
    k.n = 0;
    const int Z = Q % P.cz, XY = Q / P.cz, Y = XY % P.cy, X = XY / P.cy;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int x = 2 * X + (c >> 2), y = 2 * Y + ((c >> 1) & 1), z = 2 * Z + (c & 1);
        int32_t r = -1;
        if (mask > 0 && (mask & (1 << c)) && x < P.nx && y < P.ny && z < P.nz) {
            const int32_t q = (x * P.ny + y) * P.nz + z;             // (at most 2^31 - 1 fine voxels)
            r = !P.banded ? q : P.slot ? P.slot[q] : -1;
            if (r < 0) r = -1;
        }
        k.row[c] = r;
        k.n += r >= 0;
    }
    return k;
}

template <bool HALF>
__device__ __forceinline__ const void *row_at(const void *data, int64_t row, int64_t stride)
{
    return static_cast<const char *>(data) + row * stride * (HALF ? 2 : 4);
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// channels [first, C) in steps of `lanes` vectors / floats of output row `o`.  A half set that moves as vectors has C % 8 == 0 and steps by
// eight channels, a float32 set by four.
template <bool HALF>
__device__ __forceinline__ void mean_row(const CoarsenSet &S, float *__restrict__ o, const Kids &kids, int first, int lanes)
{
    if (kids.n == 0) {
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes)
                *reinterpret_cast<float4 *>(o + k) = S.fill ? make_float4(S.fill[k], S.fill[k + 1], S.fill[k + 2], S.fill[k + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = S.fill ? S.fill[k] : 0.0f;
        }
        return;
    }
    const float inv = 1.0f / (float)kids.n;
    const void *row[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) row[c] = kids.row[c] >= 0 ? row_at<HALF>(S.data, kids.row[c], S.stride) : nullptr;
    if (S.vec) {
        if constexpr (HALF) {
            for (int k = 8 * first; k < S.C; k += 8 * lanes) {
                uint4 r[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)      // (a packed word of zeros is two halves of +0)
                    r[c] = row[c] ? *reinterpret_cast<const uint4 *>(static_cast<const _Float16 *>(row[c]) + k) : make_uint4(0u, 0u, 0u, 0u);
                float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    lo = add4(lo, make_float4(widen(r[c].x & 0xffffu), widen(r[c].x >> 16), widen(r[c].y & 0xffffu), widen(r[c].y >> 16)));
                    hi = add4(hi, make_float4(widen(r[c].z & 0xffffu), widen(r[c].z >> 16), widen(r[c].w & 0xffffu), widen(r[c].w >> 16)));
                }
                *reinterpret_cast<float4 *>(o + k) = scale4(lo, inv);
                *reinterpret_cast<float4 *>(o + k + 4) = scale4(hi, inv);
            }
        } else {
            for (int k = 4 * first; k < S.C; k += 4 * lanes) {
                float4 v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = row[c] ? *reinterpret_cast<const float4 *>(static_cast<const float *>(row[c]) + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int c = 0; c < 8; ++c) acc = add4(acc, v[c]);
                *reinterpret_cast<float4 *>(o + k) = scale4(acc, inv);
            }
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                v[c] = 0.0f;
                if (row[c]) {
                    if constexpr (HALF)
                        v[c] = (float)static_cast<const _Float16 *>(row[c])[k];
                    else
                        v[c] = static_cast<const float *>(row[c])[k];
                }
            }
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc = acc + v[c];
            o[k] = acc * inv;
        }
    }
}

// the storage of one set is the same in every lane: a branch per set, outside the channel loop
template <bool HALF>
__device__ __forceinline__ void mean_set(const CoarsenSet &S, float *__restrict__ o, const Kids &kids, int first, int lanes)
{
    if (HALF && S.f16 != 0)
        mean_row<true>(S, o, kids, first, lanes);
    else
        mean_row<false>(S, o, kids, first, lanes);
}

template <bool WIDE, bool HALF>
__global__ __launch_bounds__(kBlock) void coarsen_rows_kernel(const CoarsenRows P)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int mask = kNoVoxel;
    int q32 = 0;
    if (j < P.m) {
        const int64_t Q = P.voxels ? (int64_t)P.voxels[j] : j;
        const bool inside = Q >= 0 && Q < P.nc;
        mask = inside ? (int)P.children[Q] : kOutside;
        q32 = inside ? (int)Q : 0;
        const Kids kids = kids_of(P, mask, q32);
        P.out_known[j] = kids.n > 0 ? 1 : 0;
        for (int s = 0; s < P.n_sets; ++s)
            if (P.sets[s].C <= kVolNarrowMax) mean_set<HALF>(P.sets[s], P.sets[s].out + j * P.sets[s].C, kids, 0, 1);
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = j - lane;
        for (int round = 0; round < 16; ++round) {
            if (wave_first + 4 * round >= P.m) break;            // wave-uniform: no voxel left
            const int from = 4 * round + group;
            const int mask_g = __shfl(mask, from, 64);
            const int q_g = __shfl(q32, from, 64);
            if (mask_g == kNoVoxel) continue;
            const Kids kids = kids_of(P, mask_g, q_g);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C > kVolNarrowMax) mean_set<HALF>(P.sets[s], P.sets[s].out + (wave_first + from) * P.sets[s].C, kids, sub, 16);
        }
    }
}

}  // namespace

hipError_t launch_coarsen_select(const CoarsenSelectArgs &A, hipStream_t s)
{
    const int64_t blocks = (A.nc + kBlock - 1) / kBlock;         // nc <= 2^31 - 1: below 2^23
    hipLaunchKernelGGL(coarsen_select_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_coarsen_rows(const CoarsenRowsArgs &A, hipStream_t s)
{
    CoarsenRows P;
    P.children = A.children;
    P.voxels = A.voxels;
    P.slot = A.slot;
    P.out_known = A.out_known;
    P.m = A.m;
    P.nc = A.nc;
    P.nx = A.nx; P.ny = A.ny; P.nz = A.nz; P.cy = A.cy; P.cz = A.cz;
    P.n_sets = A.n_sets;
    P.banded = A.banded ? 1 : 0;
    bool wide = false, half = false;
    for (int i = 0; i < A.n_sets; ++i) {
        P.sets[i] = A.sets[i];
        wide = wide || A.sets[i].C > kVolNarrowMax;
        half = half || A.sets[i].f16 != 0;
    }
    const int64_t blocks = (A.m + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (wide) {
        if (half)
            hipLaunchKernelGGL((coarsen_rows_kernel<true, true>), grid, block, 0, s, P);
        else
            hipLaunchKernelGGL((coarsen_rows_kernel<true, false>), grid, block, 0, s, P);
    } else {
        if (half)
            hipLaunchKernelGGL((coarsen_rows_kernel<false, true>), grid, block, 0, s, P);
        else
            hipLaunchKernelGGL((coarsen_rows_kernel<false, false>), grid, block, 0, s, P);
    }
    return hipGetLastError();
}

}  // namespace d3f
