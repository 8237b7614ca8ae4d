// flow_kernels.hip -- how did it move?  Dense descriptor flow between two baked fields on the same grid (include/d3fields_hip.h, the flow block;
// DESIGN.md section 25).
//
// Definitions (the contract; restated in tests/flow_cases.py).  A volume nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, extents in
// [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels.  Two fields A and B on that grid, each with site (one byte per voxel), slot (NULL or the int32
// volume of a band, -1 = no row) and ONE set of rows of C floats (the same C): the row of voxel v is data + v*stride_voxel, with a slot volume
// data + slot[v]*stride_voxel.  Either field may be dense or banded, independently of the other.
//   MEMBER      of A: site_a[v] != 0 and slot_a[v] >= 0 (when given); of B likewise.
//   CANDIDATES  of v: u = v + (dx, dy, dz), |dx|, |dy|, |dz| <= r, r in 1..D3F_FLOW_MAX_RADIUS, u inside the volume (spatially: nothing wraps
//               through memory) and a member of B.
//   COST        s(v, u): ONE float32 accumulator that starts at +0.0f and takes the channels in ascending order c = 0 .. C-1,
//               s = fl(s + fl(d * d)),  d = fl(a_c - b_c),  every operation one IEEE float32 operation, nothing fused (the build has
//               -ffp-contract=off and this file names no fused operation): the L2 chain of parts_kernels.hip word for word.
//   TAKES PART  iff s is finite (not NaN, not +Inf) and s <= max_cost2 (the caller passes the SQUARED radius; +Inf: no threshold).
//   WINNER      the candidate with the lexicographically smallest key (s, d2, j), d2 = dx^2 + dy^2 + dz^2,
//               j = ((dx + r)*(2r + 1) + (dy + r))*(2r + 1) + (dz + r): for a fixed v, ascending j is ascending flat index of u.  s >= +0, d2 <= 48
//               and j < 729, so the key packs exactly into 64 bits, bits(s) << 16 | d2 << 10 | j, and the smallest integer is the winner.
//   OUTPUTS     every voxel of the volume is written.  target int32: the flat index of the winner, or -1; cost float32: the winner's s, or +Inf.
//               -1 and +Inf go together: a non-member of A, or a member with no candidate that takes part.
//   AXIS COST   optional, float32 [n, 6]: for a voxel with target t the costs s(v, t -+ e) in the order x-, x+, y-, y+, z-, z+; +Inf where the
//               neighbour lies outside the volume, is no member of B or has a non-finite s.  Neither the window nor max_cost2 applies.  A voxel
//               without a target gets six +Inf.  The same chain.
//
//   flow_kernel<W, VEC>   one workgroup of 256 lanes per tile of D3F_LINK_TILE_X x _Y x _Z = 4 x 4 x 16 voxels of A, one lane per voxel, z fastest.
//                  The window of (2r+1)^3 offsets is cut into sub-windows of W^3 offsets (W = 3 at r = 1, 5 at r = 2, 4 at r = 3 -- two per
//                  axis --, 5 at r = 4 -- two per axis), one PASS each; offsets of the last sub-window of an axis that lie beyond +r are
//                  computed and not looked at.  A tile none of whose voxels is a member of A writes -1 / +Inf and leaves before any row load.
//                  Per pass:
//                  1. the B row index (or -1) of every voxel of the pass's BOX -- the tile shifted by the sub-window's first offset, plus W-1
//                     voxels along every axis, (3+W) x (3+W) x (15+W) rows -- goes to LDS; a box without a member of B ends the pass;
//                  2. the B rows of the box are staged through LDS in chunks of 8 channels (16-byte loads where C % 4 == 0, both strides are
//                     multiples of 4 and both bases 16-byte aligned, scalar loads otherwise; a non-member's row and the channels beyond C are
//                     zeros, which add fl(s + 0.0f) = s), every B row is loaded once per tile and pass instead of once per pair;
//                  3. every lane reads its own 8 channels of A from memory and carries the W^3 partial sums of its offsets in registers across the
//                     chunks: W^3 independent chains;
//                  4. every offset that takes part is folded into the lane's running best 64-bit key.  The key is a total order, so the merge
//                     across passes is exact whatever their order.
//   flow_axis_kernel      one lane per voxel: seven direct row reads and six chains for a voxel with a target.
// WORKGROUP ORDER.  Tiles are numbered with z SLOWEST (b = tz * tiles_xy + tx * tiles_y + ty).  Consecutive workgroups go to consecutive XCDs; with z
// fastest and a volume four tiles high, the tiles that hold a horizontal surface (a table top) are every fourth workgroup and land on two of the
// eight XCDs.  Counters showed exactly that on the 200 x 175 x 55 bake.
// LDS at W = 5: 1280 rows x 12 floats (8 and 4 of padding: 16-byte aligned rows) and 1280 int32, 66 560 bytes: two workgroups per CU, which is
// what the ~125 accumulators per lane allow in registers as well; at 16 channels per chunk the box alone would be 100 KB and one workgroup of
// four waves would own a CU.  No atomics, no scratch, no workspace, nothing waits for another workgroup, every loop bound is known at launch.
// Every output is a function of the input alone.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int kFlowTX = D3F_LINK_TILE_X, kFlowTY = D3F_LINK_TILE_Y, kFlowTZ = D3F_LINK_TILE_Z;
constexpr int kFlowChunk = 8;                    // channels per staging round
constexpr int kFlowRowFloats = kFlowChunk + 4;   // the LDS row: 16-byte aligned
static_assert(kFlowTX * kFlowTY * kFlowTZ == kBlock, "one lane per voxel of the tile");

struct FlowArgs {
    const uint8_t *site_a, *site_b;
    const int32_t *slot_a, *slot_b;
    const float *data_a, *data_b;
    int64_t stride_a, stride_b;
    int32_t *target;
    float *cost, *axis;
    int nx, ny, nz, C, r, tiles_y, tiles_xy;
    float max_cost2;
};

__device__ __forceinline__ int32_t flow_row(const uint8_t *site, const int32_t *slot, int32_t v)
{
    if (site[v] == 0) return -1;
    return slot ? slot[v] : v;
}

template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void flow_kernel(FlowArgs p)
{
    constexpr int BX = kFlowTX + W - 1, BY = kFlowTY + W - 1, BZ = kFlowTZ + W - 1, NB = BX * BY * BZ, NO = W * W * W;
    static_assert(NB * (kFlowRowFloats + 1) * 4 <= 81920, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) float rows[NB * kFlowRowFloats];
    __shared__ int32_t mrow[NB];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int tz = b / p.tiles_xy, txy = b % p.tiles_xy;      // z slowest: see the note on workgroup order in the header of this file
    const int x0 = (txy / p.tiles_y) * kFlowTX, y0 = (txy % p.tiles_y) * kFlowTY, z0 = tz * kFlowTZ;
    const int lz = tid % kFlowTZ, ly = (tid / kFlowTZ) % kFlowTY, lx = tid / (kFlowTZ * kFlowTY);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    const int32_t v = x < p.nx && y < p.ny && z < p.nz ? (x * p.ny + y) * p.nz + z : -1;
    const int32_t arow = v >= 0 ? flow_row(p.site_a, p.slot_a, v) : -1;
    const bool member = arow >= 0;
    if (!__syncthreads_or(member)) {
        if (v >= 0) {
            p.target[v] = -1;
            p.cost[v] = __builtin_inff();
        }
        return;
    }
    const int r = p.r, side = 2 * r + 1, passes = (side + W - 1) / W;
    const float *arow_ptr = p.data_a + (int64_t)(member ? arow : 0) * p.stride_a;
    const int own = (lx * BY + ly) * BZ + lz;           // the box row of the sub-window's first offset
    unsigned long long best = ~0ull;
    for (int pass = 0; pass < passes * passes * passes; ++pass) {
        const int lox = -r + W * (pass / (passes * passes)), loy = -r + W * ((pass / passes) % passes), loz = -r + W * (pass % passes);
        __syncthreads();                                                  // the pass before has been read
        int has = 0;
        for (int i = tid; i < NB; i += kBlock) {
            const int bz = i % BZ, bxy = i / BZ, by = bxy % BY, bx = bxy / BY;
            const int ux = x0 + lox + bx, uy = y0 + loy + by, uz = z0 + loz + bz;
            int32_t m = -1;
            if ((unsigned)ux < (unsigned)p.nx && (unsigned)uy < (unsigned)p.ny && (unsigned)uz < (unsigned)p.nz)
                m = flow_row(p.site_b, p.slot_b, (ux * p.ny + uy) * p.nz + uz);
            mrow[i] = m;
            has |= m >= 0;
        }
        if (!__syncthreads_or(has)) continue;
        float acc[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) acc[j] = 0.0f;
        for (int c0 = 0; c0 < p.C; c0 += kFlowChunk) {
            if (c0 > 0) __syncthreads();                                  // the chunk before has been read
            if (VEC) {
                for (int e = tid; e < NB * (kFlowChunk / 4); e += kBlock) {
                    const int i = e / (kFlowChunk / 4), k = 4 * (e % (kFlowChunk / 4)), c = c0 + k;
                    const int32_t m = mrow[i];
                    float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (m >= 0 && c < p.C) val = *reinterpret_cast<const float4 *>(p.data_b + (int64_t)m * p.stride_b + c);
                    *reinterpret_cast<float4 *>(rows + i * kFlowRowFloats + k) = val;
                }
            } else {
                for (int e = tid; e < NB * kFlowChunk; e += kBlock) {
                    const int i = e / kFlowChunk, k = e % kFlowChunk, c = c0 + k;
                    const int32_t m = mrow[i];
                    rows[i * kFlowRowFloats + k] = m >= 0 && c < p.C ? p.data_b[(int64_t)m * p.stride_b + c] : 0.0f;
                }
            }
            __syncthreads();
            if (member) {
                const float *bbase = rows + own * kFlowRowFloats;
#pragma unroll 1      // (one group of four channels at a time keeps the row loads of a group out of the accumulators' registers)
                for (int u = 0; u < kFlowChunk; u += 4) {
                    float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    const int c = c0 + u;
                    if (VEC) {
                        if (c < p.C) av = *reinterpret_cast<const float4 *>(arow_ptr + c);
                    } else {
                        if (c < p.C) av.x = arow_ptr[c];
                        if (c + 1 < p.C) av.y = arow_ptr[c + 1];
                        if (c + 2 < p.C) av.z = arow_ptr[c + 2];
                        if (c + 3 < p.C) av.w = arow_ptr[c + 3];
                    }
#pragma unroll
                    for (int j = 0; j < NO; ++j) {
                        const int delta = ((j / (W * W)) * BY + (j / W) % W) * BZ + j % W;
                        const float4 bv = *reinterpret_cast<const float4 *>(bbase + delta * kFlowRowFloats + u);
                        const float d0 = av.x - bv.x, d1 = av.y - bv.y, d2 = av.z - bv.z, d3 = av.w - bv.w;
                        acc[j] = acc[j] + d0 * d0;
                        acc[j] = acc[j] + d1 * d1;
                        acc[j] = acc[j] + d2 * d2;
                        acc[j] = acc[j] + d3 * d3;
                    }
                }
            }
        }
        if (member) {
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                const int jx = j / (W * W), jy = (j / W) % W, jz = j % W;
                const int ox = lox + jx, oy = loy + jy, oz = loz + jz;
                const float s = acc[j];
                const bool in = ox <= r && oy <= r && oz <= r && mrow[own + (jx * BY + jy) * BZ + jz] >= 0;
                if (in && s <= p.max_cost2 && s < __builtin_inff()) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 16) | (unsigned long long)((ox * ox + oy * oy + oz * oz) << 10) |
                                                   (unsigned long long)(((ox + r) * side + (oy + r)) * side + (oz + r));
                    if (key < best) best = key;
                }
            }
        }
    }
    if (v < 0) return;
    int32_t target = -1;
    float cost = __builtin_inff();
    if (best != ~0ull) {
        const int j = (int)(best & 1023u);
        const int ox = j / (side * side) - r, oy = (j / side) % side - r, oz = j % side - r;
        target = v + (ox * p.ny + oy) * p.nz + oz;
        cost = __uint_as_float((unsigned)(best >> 16));
    }
    p.target[v] = target;
    p.cost[v] = cost;
}

__global__ __launch_bounds__(kBlock) void flow_axis_kernel(FlowArgs p, int32_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t v = (int32_t)i;
    float out[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = __builtin_inff();
    const int32_t t = p.target[v];
    if (t >= 0) {
        const int tz = t % p.nz, txy = t / p.nz, ty = txy % p.ny, tx = txy / p.ny;
        const int coord[3] = {tx, ty, tz}, extent[3] = {p.nx, p.ny, p.nz}, step[3] = {p.ny * p.nz, p.nz, 1};
        const float *a = p.data_a + (int64_t)(p.slot_a ? p.slot_a[v] : v) * p.stride_a;
        const float *brow[6];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int sign = (k & 1) ? 1 : -1, cc = coord[k >> 1] + sign;
            int32_t m = -1;
            if (cc >= 0 && cc < extent[k >> 1]) m = flow_row(p.site_b, p.slot_b, t + sign * step[k >> 1]);
            brow[k] = m >= 0 ? p.data_b + (int64_t)m * p.stride_b : nullptr;
            any |= m >= 0;
        }
        if (any) {
            float s[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] = 0.0f;
            for (int c = 0; c < p.C; ++c) {
                const float ac = a[c];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (brow[k]) {
                        const float d = ac - brow[k][c];
                        s[k] = s[k] + d * d;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (brow[k] && s[k] < __builtin_inff()) out[k] = s[k];
        }
    }
    float *o = p.axis + (int64_t)v * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = out[k];
}

template <int W>
void flow_launch(const FlowArgs &a, bool vec, dim3 grid, hipStream_t s)
{
    if (vec)
        hipLaunchKernelGGL((flow_kernel<W, true>), grid, dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL((flow_kernel<W, false>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace

hipError_t launch_volume_flow(const uint8_t *site_a, const int32_t *slot_a, const float *data_a, int64_t stride_a, const uint8_t *site_b, const int32_t *slot_b,
                              const float *data_b, int64_t stride_b, int C, bool vec, int nx, int ny, int nz, int radius, float max_cost2, int32_t *out_target,
                              float *out_cost, float *out_axis_cost, hipStream_t s)
{
    const int tiles_y = (ny + kFlowTY - 1) / kFlowTY, tiles_z = (nz + kFlowTZ - 1) / kFlowTZ;
    const int tiles_xy = ((nx + kFlowTX - 1) / kFlowTX) * tiles_y;
    const int64_t tiles = (int64_t)tiles_xy * tiles_z;
    FlowArgs a{site_a, site_b, slot_a, slot_b, data_a, data_b, stride_a, stride_b, out_target, out_cost, out_axis_cost, nx, ny, nz, C, radius, tiles_y, tiles_xy,
               max_cost2};
    const dim3 grid((unsigned)tiles);
    if (radius == 1)
        flow_launch<3>(a, vec, grid, s);
    else if (radius == 3)
        flow_launch<4>(a, vec, grid, s);
    else
        flow_launch<5>(a, vec, grid, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out_axis_cost) return e;
    const int32_t n = nx * ny * nz;
    hipLaunchKernelGGL(flow_axis_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, n);
    return hipGetLastError();
}

// the axis pass alone, over targets that another kernel wrote (the seeded flow: flow_seeded_kernels.hip); flow_axis_kernel reads nothing else of A
// than slot and rows
hipError_t launch_flow_axis(const int32_t *slot_a, const float *data_a, int64_t stride_a, const uint8_t *site_b, const int32_t *slot_b, const float *data_b,
                            int64_t stride_b, int C, int nx, int ny, int nz, const int32_t *target, float *out_axis_cost, hipStream_t s)
{
    FlowArgs a{nullptr, site_b, slot_a, slot_b, data_a, data_b, stride_a, stride_b, const_cast<int32_t *>(target), nullptr, out_axis_cost, nx, ny, nz, C, 0, 0, 0,
               0.0f};
    const int32_t n = nx * ny * nz;
    hipLaunchKernelGGL(flow_axis_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, n);
    return hipGetLastError();
}

}  // namespace d3f
