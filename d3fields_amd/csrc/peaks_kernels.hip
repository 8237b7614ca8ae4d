// peaks_kernels.hip -- where is this descriptor?  Exact, order-independent non-maximum suppression through the band's slot volume
// (include/d3fields_hip.h, the peaks block).
//
// Definitions (the contract; restated in tests/peaks_cases.py).  A volume nx x ny x nz, z fastest, flat index (x*ny + y)*nz + z, extents in
// [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels.  slot: NULL, or an int32 volume as d3f_band_mark writes it (-1 = no row); with NULL, row m
// is voxel m and M = nx*ny*nz.  mask: NULL, or one byte per voxel (non-zero = takes part).  score: float32, row m column q at
// score[m*stride_row + q], 0 <= q < K <= stride_row.  radius r in [1, D3F_PEAKS_MAX_RADIUS = 8].  threshold: not NaN, +Inf = none.
//   TAKES PART  for column q, voxel v with row m = slot[v]: m >= 0, mask[v] != 0 (when given), score[m, q] < +Inf (false for NaN and +Inf;
//               -Inf takes part).
//   PEAK        v takes part, score[m, q] <= threshold, and for every OTHER voxel u that takes part with |u_a - v_a| <= r on all three axes
//               the pair (score_u, flat_u) is lexicographically greater than (score_v, flat_v).  The box is spatial and clipped to the
//               volume: (x, y, nz-1) and (x, y+1, 0) are no neighbours.  Scores compare as IEEE floats (-0.0 == +0.0).  The threshold
//               filters peaks; a voxel above it still suppresses others.
//   out[m*out_stride + q] = score[m, q] where the voxel of row m is a peak of column q, +Inf otherwise, for every row and column; the padding
//   between K and the stride is not touched.  out_count[q] (may be NULL, zeroed by the entry point) = the number of peaks of column q.
//   Minima only.  Two peaks of one column differ by more than r on some axis; a constant volume has exactly one peak, voxel 0.
//
// THE KEY.  Per (voxel, column) a 64-bit key: high word = the float mapped to an order-preserving uint32 (-0.0 first made +0.0: b = bits,
// b ^ 0xffffffff if the sign is set, b | 0x80000000 otherwise), low word = the flat index; all ones = does not take part (no key of a voxel
// that takes part has a high word of all ones: the largest is that of FLT_MAX, 0xff7fffff).  The lexicographic minimum of (score, flat) over a box
// is then a u64 minimum, which is associative and commutative: the minimum over the box is exactly the x-minimum of the y-minima of the
// z-minima, in any order of execution.  v is a peak iff the low word of its box minimum is v itself (and its score passes the threshold).
//
//   peaks_kernel   one workgroup per (tile of T^3 voxels, chunk of CK columns); T, CK and the padded line length come from peaks_plan.
//                  1. with a slot volume: a tile none of whose voxels has a row writes nothing and leaves before any score load;
//                  2. the tile and a halo of r are staged as keys in LDS through the slot indirection, columns fastest, so the CK
//                     columns of a row are one contiguous load; a position outside the volume holds all ones;
//                  3. z, then y window minima in place, one thread per (line, column) walking its line forwards: out[i] = min in[i .. i+2r]
//                     is written at i after it was read, and nothing later reads below i + 1;
//                  4. one thread per (tile voxel, column) takes the x window minimum, compares its low word with the own flat index, loads
//                     the score of a peak again for the threshold and the output, and writes out for every voxel that has a row;
//                  5. peaks are counted per column in LDS (integer adds) and added to out_count once per workgroup and column.
// No float atomics, no workspace, nothing waits for another workgroup, every loop bound is known at launch (T, r, CK), no scratch.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr uint64_t kNoKey = ~0ull;
constexpr int kPeaksMaxKeys = 8188;          // with the column counters just under 64 KiB per workgroup: two workgroups per CU
constexpr int kPeaksMaxChunk = 8;            // columns per workgroup at most

struct PeaksArgs {
    const int32_t *slot;
    const uint8_t *mask;
    const float *score;
    float *out;
    int32_t *out_count;
    int64_t stride_row, out_stride;
    int nx, ny, nz, K, radius, tile, log_ck, hzp, tiles_y, tiles_z;
    float threshold;
};

__device__ __forceinline__ uint64_t peak_key(float s, int32_t flat)
{
    uint32_t b = s == 0.0f ? 0u : __float_as_uint(s);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | (uint32_t)flat;
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(kBlock) void peaks_kernel(PeaksArgs p)
{
    extern __shared__ uint64_t key[];
    __shared__ int cnt[kPeaksMaxChunk];
    const int tid = threadIdx.x;
    const int T = p.tile, r = p.radius, lg = p.log_ck, cmask = (1 << lg) - 1;
    const int h = T + 2 * r, hzp = p.hzp, win = 2 * r;
    const int b = blockIdx.x;
    const int tz = b % p.tiles_z, txy = b / p.tiles_z;
    const int x0 = (txy / p.tiles_y) * T, y0 = (txy % p.tiles_y) * T, z0 = tz * T;
    const int q0 = (int)blockIdx.y << lg;

    if (p.slot) {                                   // 1. a tile without a stored voxel has no row to write
        int has = 0;
        for (int i = tid; i < T * T * T; i += kBlock) {
            const int z = z0 + i % T, y = y0 + (i / T) % T, x = x0 + i / (T * T);
            if (x < p.nx && y < p.ny && z < p.nz) has |= p.slot[(x * p.ny + y) * p.nz + z] >= 0;
        }
        if (!__syncthreads_or(has)) return;
    }

    const int staged = (h * h * h) << lg;           // 2. keys of the tile and its halo
    for (int e = tid; e < staged; e += kBlock) {
        const int c = e & cmask, i = e >> lg;
        const int lz = i % h, lxy = i / h, ly = lxy % h, lx = lxy / h;
        const int x = x0 - r + lx, y = y0 - r + ly, z = z0 - r + lz, q = q0 + c;
        uint64_t k = kNoKey;
        if ((unsigned)x < (unsigned)p.nx && (unsigned)y < (unsigned)p.ny && (unsigned)z < (unsigned)p.nz && q < p.K) {
            const int32_t v = (x * p.ny + y) * p.nz + z;
            const int32_t m = p.slot ? p.slot[v] : v;
            if (m >= 0 && (!p.mask || p.mask[v] != 0)) {
                const float s = p.score[(int64_t)m * p.stride_row + q];
                if (s < INFINITY) k = peak_key(s, v);
            }
        }
        key[((((lx * h) + ly) * hzp + lz) << lg) | c] = k;
    }
    if (tid < kPeaksMaxChunk) cnt[tid] = 0;
    __syncthreads();

    for (int t = tid; t < (h * h) << lg; t += kBlock) {            // 3a. z: lines (lx, ly), outputs 0 .. T-1
        const int base = (((t >> lg) * hzp) << lg) | (t & cmask);
        for (int z = 0; z < T; ++z) {
            uint64_t m = key[base + (z << lg)];
            for (int k = 1; k <= win; ++k) m = min_u64(m, key[base + ((z + k) << lg)]);
            key[base + (z << lg)] = m;
        }
    }
    __syncthreads();

    for (int t = tid; t < (h * T) << lg; t += kBlock) {            // 3b. y: lines (lx, z < T)
        const int l = t >> lg, z = l % T, lx = l / T;
        const int base = ((lx * h * hzp + z) << lg) | (t & cmask), stride = hzp << lg;
        for (int y = 0; y < T; ++y) {
            uint64_t m = key[base + y * stride];
            for (int k = 1; k <= win; ++k) m = min_u64(m, key[base + (y + k) * stride]);
            key[base + y * stride] = m;
        }
    }
    __syncthreads();

    for (int e = tid; e < (T * T * T) << lg; e += kBlock) {        // 4. x, and the verdict of one (voxel, column)
        const int c = e & cmask, i = e >> lg;
        const int lz = i % T, ly = (i / T) % T, lx = i / (T * T);
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz, q = q0 + c;
        if (x >= p.nx || y >= p.ny || z >= p.nz || q >= p.K) continue;
        const int32_t v = (x * p.ny + y) * p.nz + z;
        const int32_t row = p.slot ? p.slot[v] : v;
        if (row < 0) continue;
        const int base = ((ly * hzp + lz) << lg) | c, stride = (h * hzp) << lg;
        uint64_t m = key[base + lx * stride];
        for (int k = 1; k <= win; ++k) m = min_u64(m, key[base + (lx + k) * stride]);
        float o = INFINITY;
        if ((uint32_t)m == (uint32_t)v) {                              // (all ones never equals a flat index: those stay below 2^31)
            const float s = p.score[(int64_t)row * p.stride_row + q];
            if (s <= p.threshold) {
                o = s;
                if (p.out_count) atomicAdd(&cnt[c], 1);
            }
        }
        p.out[(int64_t)row * p.out_stride + q] = o;
    }
    if (p.out_count) {                                                  // 5. one integer add per workgroup and column
        __syncthreads();
        if (tid <= cmask && q0 + tid < p.K && cnt[tid] > 0) atomicAdd(p.out_count + q0 + tid, cnt[tid]);
    }
}

}  // namespace

// Tile edge, column chunk and padded z line of a launch.  Radii up to 4 use tiles of 8^3 voxels, larger ones 4^3 (a halo of 8 round 8^3 would be
// 24^3 keys); the chunk is the largest power of two <= 8 that the columns can fill and whose keys fit kPeaksMaxKeys; the z line is padded to an odd
// length where that still fits, so that the 8-byte accesses of the z pass (one line per lane) fall on distinct banks.
PeaksPlan peaks_plan(int nx, int ny, int nz, int K, int radius)
{
    PeaksPlan pl{};
    pl.tile = radius <= 4 ? 8 : 4;
    const int h = pl.tile + 2 * radius;
    int lg = 0;
    while (lg < 3 && (1 << lg) < K && ((int64_t)h * h * h << (lg + 1)) <= kPeaksMaxKeys) ++lg;
    pl.log_ck = lg;
    pl.hzp = ((int64_t)h * h * (h | 1) << lg) <= kPeaksMaxKeys ? (h | 1) : h;
    pl.lds_bytes = (int64_t)h * h * pl.hzp * 8 << lg;
    pl.tiles_y = (ny + pl.tile - 1) / pl.tile;
    pl.tiles_z = (nz + pl.tile - 1) / pl.tile;
    pl.tiles = (int64_t)((nx + pl.tile - 1) / pl.tile) * pl.tiles_y * pl.tiles_z;
    pl.chunks = ((int64_t)K + (1 << lg) - 1) >> lg;
    return pl;
}

hipError_t launch_volume_peaks(const int32_t *slot, const uint8_t *mask, int nx, int ny, int nz, const float *score, int K, int64_t stride_row, int radius,
                               float threshold, float *out, int64_t out_stride, int32_t *out_count, hipStream_t s)
{
    const PeaksPlan pl = peaks_plan(nx, ny, nz, K, radius);
    PeaksArgs a{slot, mask, score, out, out_count, stride_row, out_stride, nx, ny, nz, K, radius, pl.tile, pl.log_ck, pl.hzp, pl.tiles_y, pl.tiles_z, threshold};
    hipLaunchKernelGGL(peaks_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.chunks), dim3(kBlock), (size_t)pl.lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace d3f
