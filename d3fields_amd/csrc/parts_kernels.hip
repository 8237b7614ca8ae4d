// parts_kernels.hip -- which part is this?  Descriptor-gated links between neighbouring voxels of the baked field (include/d3fields_hip.h, the
// links block).
//
// Definitions (the contract; restated in tests/parts_cases.py).  A volume nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, extents in
// [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels.  site: one byte per voxel; valid: NULL or one byte per voxel; slot: NULL or the int32 volume
// of a band (-1 = no row).  One set of rows of C floats: the row of voxel v is data + v*stride_voxel, with a slot volume data + slot[v]*stride_voxel.
//   MEMBER      site[v] != 0, valid[v] != 0 (when given), slot[v] >= 0 (when given).
//   OFFSETS     (dx, dy, dz) over {-1,0,1}^3 in lexicographic order, the 13 that precede (0,0,0): j = 9*(dx+1) + 3*(dy+1) + (dz+1), j = 0..12.
//               Bits 0..8 are dx = -1, bits 9..11 are (0,-1,*), bit 12 is (0,0,-1): every one is a neighbour of LOWER flat index.
//   out[v]      uint16; bit j is set iff  v is a member,  u = v + offset j lies inside the volume (spatially: nothing wraps through memory),
//               |dx|+|dy|+|dz| <= 1 / 2 / 3 for connectivity 6 / 18 / 26,  u is a member,  and the rule accepts (row_v, row_u) = (a, b).
//               Bits 13..15 are 0.  Every voxel of the volume is written.  A pair is evaluated once, by its higher voxel.
//   D3F_LINK_L2      s <= threshold   (the caller passes the squared radius; false for a NaN s; +Inf accepts every s that is not NaN)
//   D3F_LINK_COSINE  na > 0 && nb > 0 && dot >= 0 && (double)dot*dot >= ((double)t*t) * ((double)na*nb),  t = threshold in [0, 1]: float64
//                    products, each rounded once, no square root, no division
//   D3F_LINK_ARGMAX  best(a) == best(b),  best(r): `best = 0; for c in 1..C-1: if r[c] > r[best]: best = c` (the vote rule of d3f_volume_pool: the
//                    first channel that holds the maximum; a NaN never wins, a NaN at channel 0 stays).  threshold is not used.
// THE SUMMATION ORDER.  Every sum has ONE float32 accumulator that starts at +0.0f and takes the channels in ascending order c = 0 .. C-1:
//   s   = fl(s   + fl(d * d)),  d = fl(a_c - b_c)          dot = fl(dot + fl(a_c * b_c))
//   na  = fl(na  + fl(a_c * a_c))                          nb  = fl(nb  + fl(b_c * b_c))
// every operation one IEEE float32 operation, nothing fused (the build has -ffp-contract=off and this file names no fused operation).  The
// thirteen pairs of a lane are thirteen independent chains, which is all the instruction-level parallelism the loop needs; the channel chunks of
// the staging below do not change the order (a padding channel beyond C adds fl(s + 0.0f) = s).  The vector and the scalar row path give the
// same bits.
//
//   links_kernel<RULE, VEC>   one workgroup of 256 lanes per tile of D3F_LINK_TILE_X x _Y x _Z = 4 x 4 x 16 voxels, one lane per voxel, z fastest.
//                  1. the row index (or -1) of every voxel of the tile's BOX -- the tile and the halo x-1, y-1 .. y+1, z-1 .. z+1, 5 x 6 x 18 rows
//                     -- goes to LDS; a tile none of whose own voxels is a member writes zeros and leaves before any row load;
//                  2. the rows of the box are staged through LDS in chunks of 16 channels (16-byte loads where C % 4 == 0, stride_voxel % 4 == 0
//                     and data is 16-byte aligned, scalar loads otherwise; a non-member's row and the channels beyond C are zeros), every row
//                     is loaded once per tile instead of 14 times;
//                  3. every lane carries the partial sums of its 13 pairs in registers across the chunks, takes the verdicts and writes one uint16.
//   links_argmax_kernel       the same tiles; one lane per box row walks its row for the first maximum, then 13 integer comparisons per voxel.
// LDS: 540 rows x 20 floats (16 and 4 of padding) and 540 int32: 45 360 bytes.  No atomics, no scratch, no workspace, nothing waits for another
// workgroup, every loop bound is known at launch.  Every output is a function of the input alone.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int kLinkTX = D3F_LINK_TILE_X, kLinkTY = D3F_LINK_TILE_Y, kLinkTZ = D3F_LINK_TILE_Z;
constexpr int kLinkBX = kLinkTX + 1, kLinkBY = kLinkTY + 2, kLinkBZ = kLinkTZ + 2;
constexpr int kLinkBoxRows = kLinkBX * kLinkBY * kLinkBZ;
constexpr int kLinkChunk = 16;                 // channels per staging round
constexpr int kLinkRowFloats = kLinkChunk + 4; // the LDS row: 16-byte aligned, consecutive rows on different banks
static_assert(kLinkTX * kLinkTY * kLinkTZ == kBlock, "one lane per voxel of the tile");
static_assert(kLinkBoxRows * (kLinkRowFloats + 1) * 4 <= 65536, "two workgroups per CU");

struct LinkArgs {
    const uint8_t *site, *valid;
    const int32_t *slot;
    const float *data;
    int64_t stride;
    uint16_t *out;
    int nx, ny, nz, C, tiles_y, tiles_z;
    uint32_t conn_mask;
    float threshold;
};

// the box row of offset j relative to a lane's own
__device__ __forceinline__ constexpr int link_delta(int j) { return ((j / 9 - 1) * kLinkBY + ((j / 3) % 3 - 1)) * kLinkBZ + (j % 3 - 1); }

struct LinkTile {
    int x0, y0, z0;      // the tile's first voxel
    int own;             // the lane's own box row
    int32_t v;           // its flat index, -1 outside the volume
};

// 1. of the header: mrow[] and whether the tile holds a member.  Ends with a barrier.
__device__ __forceinline__ bool link_box(const LinkArgs &p, int32_t *mrow, LinkTile &t)
{
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int tz = b % p.tiles_z, txy = b / p.tiles_z;
    t.x0 = (txy / p.tiles_y) * kLinkTX, t.y0 = (txy % p.tiles_y) * kLinkTY, t.z0 = tz * kLinkTZ;
    int has = 0;
    for (int i = tid; i < kLinkBoxRows; i += kBlock) {
        const int lz = i % kLinkBZ, lxy = i / kLinkBZ, ly = lxy % kLinkBY, lx = lxy / kLinkBY;
        const int x = t.x0 - 1 + lx, y = t.y0 - 1 + ly, z = t.z0 - 1 + lz;
        int32_t m = -1;
        if ((unsigned)x < (unsigned)p.nx && (unsigned)y < (unsigned)p.ny && (unsigned)z < (unsigned)p.nz) {
            const int32_t v = (x * p.ny + y) * p.nz + z;
            if (p.site[v] != 0 && (!p.valid || p.valid[v] != 0)) m = p.slot ? p.slot[v] : v;
        }
        mrow[i] = m;
        if (lx >= 1 && ly >= 1 && ly <= kLinkTY && lz >= 1 && lz <= kLinkTZ) has |= m >= 0;
    }
    const int lz = tid % kLinkTZ, ly = (tid / kLinkTZ) % kLinkTY, lx = tid / (kLinkTZ * kLinkTY);
    const int x = t.x0 + lx, y = t.y0 + ly, z = t.z0 + lz;
    t.own = ((lx + 1) * kLinkBY + ly + 1) * kLinkBZ + lz + 1;
    t.v = x < p.nx && y < p.ny && z < p.nz ? (x * p.ny + y) * p.nz + z : -1;
    return __syncthreads_or(has) != 0;
}

template <int RULE, bool VEC>
__global__ __launch_bounds__(kBlock) void links_kernel(LinkArgs p)
{
    __shared__ __attribute__((aligned(16))) float rows[kLinkBoxRows * kLinkRowFloats];
    __shared__ int32_t mrow[kLinkBoxRows];
    const int tid = threadIdx.x;
    LinkTile t;
    if (!link_box(p, mrow, t)) {
        if (t.v >= 0) p.out[t.v] = 0;
        return;
    }
    const bool member = t.v >= 0 && mrow[t.own] >= 0;
    float acc[13], nb[13], na = 0.0f;      // L2: acc = s; COSINE: acc = dot
#pragma unroll
    for (int j = 0; j < 13; ++j) acc[j] = nb[j] = 0.0f;
    for (int c0 = 0; c0 < p.C; c0 += kLinkChunk) {
        if (c0 > 0) __syncthreads();                                  // the chunk before has been read
        if (VEC) {
            for (int e = tid; e < kLinkBoxRows * (kLinkChunk / 4); e += kBlock) {
                const int i = e / (kLinkChunk / 4), c = c0 + 4 * (e % (kLinkChunk / 4));
                const int32_t m = mrow[i];
                float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (m >= 0 && c < p.C) val = *reinterpret_cast<const float4 *>(p.data + (int64_t)m * p.stride + c);
                *reinterpret_cast<float4 *>(rows + i * kLinkRowFloats + 4 * (e % (kLinkChunk / 4))) = val;
            }
        } else {
            for (int e = tid; e < kLinkBoxRows * kLinkChunk; e += kBlock) {
                const int i = e / kLinkChunk, k = e % kLinkChunk, c = c0 + k;
                const int32_t m = mrow[i];
                rows[i * kLinkRowFloats + k] = m >= 0 && c < p.C ? p.data[(int64_t)m * p.stride + c] : 0.0f;
            }
        }
        __syncthreads();
        if (member) {
            const float *a = rows + t.own * kLinkRowFloats;
#pragma unroll 1      // (unrolled, the 52 row loads of a chunk are hoisted into some 240 registers)
            for (int u = 0; u < kLinkChunk; u += 4) {
                const float4 av = *reinterpret_cast<const float4 *>(a + u);
#pragma unroll
                for (int j = 0; j < 13; ++j) {
                    const float4 bv = *reinterpret_cast<const float4 *>(a + link_delta(j) * kLinkRowFloats + u);
                    if (RULE == D3F_LINK_L2) {
                        const float d0 = av.x - bv.x, d1 = av.y - bv.y, d2 = av.z - bv.z, d3 = av.w - bv.w;
                        acc[j] = acc[j] + d0 * d0;
                        acc[j] = acc[j] + d1 * d1;
                        acc[j] = acc[j] + d2 * d2;
                        acc[j] = acc[j] + d3 * d3;
                    } else {
                        acc[j] = acc[j] + av.x * bv.x;
                        acc[j] = acc[j] + av.y * bv.y;
                        acc[j] = acc[j] + av.z * bv.z;
                        acc[j] = acc[j] + av.w * bv.w;
                        nb[j] = nb[j] + bv.x * bv.x;
                        nb[j] = nb[j] + bv.y * bv.y;
                        nb[j] = nb[j] + bv.z * bv.z;
                        nb[j] = nb[j] + bv.w * bv.w;
                    }
                }
                if (RULE == D3F_LINK_COSINE) {
                    na = na + av.x * av.x;
                    na = na + av.y * av.y;
                    na = na + av.z * av.z;
                    na = na + av.w * av.w;
                }
            }
        }
    }
    if (t.v < 0) return;
    uint32_t bits = 0;
    if (member) {
        const double tt = (double)p.threshold * (double)p.threshold;
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            bool ok;
            if (RULE == D3F_LINK_L2)
                ok = acc[j] <= p.threshold;
            else
                ok = na > 0.0f && nb[j] > 0.0f && acc[j] >= 0.0f && (double)acc[j] * (double)acc[j] >= tt * ((double)na * (double)nb[j]);
            if (ok && mrow[t.own + link_delta(j)] >= 0) bits |= 1u << j;
        }
    }
    p.out[t.v] = (uint16_t)(bits & p.conn_mask);
}

__global__ __launch_bounds__(kBlock) void links_argmax_kernel(LinkArgs p)
{
    __shared__ int32_t best[kLinkBoxRows];
    __shared__ int32_t mrow[kLinkBoxRows];
    LinkTile t;
    if (!link_box(p, mrow, t)) {
        if (t.v >= 0) p.out[t.v] = 0;
        return;
    }
    for (int i = threadIdx.x; i < kLinkBoxRows; i += kBlock) {
        const int32_t m = mrow[i];
        int b = -1;
        if (m >= 0) {
            const float *row = p.data + (int64_t)m * p.stride;
            float top = row[0];
            b = 0;
            for (int c = 1; c < p.C; ++c) {
                const float r = row[c];
                if (r > top) {
                    top = r;
                    b = c;
                }
            }
        }
        best[i] = b;
    }
    __syncthreads();
    if (t.v < 0) return;
    uint32_t bits = 0;
    const int mine = best[t.own];
    if (mine >= 0) {
#pragma unroll
        for (int j = 0; j < 13; ++j)
            if (best[t.own + link_delta(j)] == mine) bits |= 1u << j;
    }
    p.out[t.v] = (uint16_t)(bits & p.conn_mask);
}

}  // namespace

hipError_t launch_volume_links(const uint8_t *site, const uint8_t *valid, const int32_t *slot, int nx, int ny, int nz, const float *data, int C, int64_t stride,
                               bool vec, int rule, float threshold, int connectivity, uint16_t *out, hipStream_t s)
{
    const int tiles_y = (ny + kLinkTY - 1) / kLinkTY, tiles_z = (nz + kLinkTZ - 1) / kLinkTZ;
    const int64_t tiles = (int64_t)((nx + kLinkTX - 1) / kLinkTX) * tiles_y * tiles_z;
    // bits by |dx|+|dy|+|dz|: 1 -> {4, 10, 12}, 2 -> {1, 3, 5, 7, 9, 11}, 3 -> {0, 2, 6, 8}
    const uint32_t conn_mask = connectivity == 6 ? 0x1410u : connectivity == 18 ? 0x1ebau : 0x1fffu;
    LinkArgs a{site, valid, slot, data, stride, out, nx, ny, nz, C, tiles_y, tiles_z, conn_mask, threshold};
    const dim3 grid((unsigned)tiles), block(kBlock);
    if (rule == D3F_LINK_ARGMAX)
        hipLaunchKernelGGL(links_argmax_kernel, grid, block, 0, s, a);
    else if (rule == D3F_LINK_L2) {
        if (vec)
            hipLaunchKernelGGL((links_kernel<D3F_LINK_L2, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((links_kernel<D3F_LINK_L2, false>), grid, block, 0, s, a);
    } else {
        if (vec)
            hipLaunchKernelGGL((links_kernel<D3F_LINK_COSINE, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((links_kernel<D3F_LINK_COSINE, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace d3f
