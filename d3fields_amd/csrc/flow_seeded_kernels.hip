// flow_seeded_kernels.hip -- the dense descriptor flow with every member's window centred on a per-voxel predicted offset
// (include/d3fields_hip_pyramid.h, d3f_volume_flow_seeded).
//
// The contract is flow_kernels.hip's word for word (restated in tests/pyramid_cases.py on top of tests/flow_cases.py) with one change:
//   CANDIDATES  of member v of A: u = v + seed[v] + (dx, dy, dz), |dx|, |dy|, |dz| <= r, u inside the volume (spatially: nothing wraps) and a
//               member of B.  seed int32 [n, 3] in voxels, nullptr: zeros.  The seed of a non-member of A is never read.
//   KEY         (s, d2, j) with d2 and j taken from (dx, dy, dz), the offset from the SEEDED centre; packed as bits(s) << 16 | d2 << 10 | j.
//   RANGE       a member whose seed has a component outside [-D3F_FLOW_SEED_MAX, D3F_FLOW_SEED_MAX] has no candidate; tested before any
//               address arithmetic, so that no sum of coordinates leaves 32 bits.
//   COST        s(v, u): ONE float32 accumulator from +0.0f, channels ascending, s = fl(s + fl(d * d)), d = fl(a_c - b_c), nothing contracted
//               (the build has -ffp-contract=off and this file names no contracted operation).
// With a zero seed target and cost are flow_kernel's byte for byte.  The axis costs come from flow_axis_kernel (launch_flow_axis).
//
// The LDS box of flow_kernel holds ONE window per tile; with a seed per voxel there is no such box, so this is another kernel.
//   flow_seeded_kernel<VEC>   ONE LANE PER CANDIDATE.  A wave takes 64 consecutive voxels (flat order, so a run along z), one per lane: the lane
//               reads its voxel's site, slot and -- a member only -- seed, and the ballot of the members is the wave's work list.  The members
//               are taken in turn: at r = 1 (27 candidates) two at a time, one per half of the wave; at r >= 2 one at a time in rounds of 64
//               candidates.  The member's coordinates, row and seed reach the lanes by shuffles.  Every lane runs its candidate's chain over
//               the channels sequentially (16-byte loads of its B row where VEC; all lanes of a member read the same A row at the same
//               address), forms the packed key, and the minimum across the member's lanes -- xor shuffles; the key is a total order, so the
//               order of the reduction does not matter -- goes back to the member's own lane.  A wave without members writes -1 / +Inf
//               and leaves.  Each B row is read once per pair, through L2.
// No LDS, no atomics, no workspace, nothing waits for another workgroup, every output is a function of the input alone.
#include "d3f_internal.h"
#include "d3fields_hip_pyramid.h"      // D3F_FLOW_SEED_MAX

namespace d3f {

namespace {

constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ int32_t seeded_row(const uint8_t *site, const int32_t *slot, int32_t v)
{
    if (site[v] == 0) return -1;
    return slot ? slot[v] : v;
}

__device__ __forceinline__ unsigned long long shuffle_xor_key(unsigned long long key, int mask)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long shuffle_key(unsigned long long key, int from)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)key, from, 64), hi = (unsigned)__shfl((int)(unsigned)(key >> 32), from, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// s(a, b) over C channels; all lanes of a member pass the same `a`
template <bool VEC>
__device__ __forceinline__ float chain(const float *__restrict__ a, const float *__restrict__ b, int C)
{
    float s = 0.0f;
    if (VEC) {
        for (int c = 0; c < C; c += 4) {
            const float4 av = *reinterpret_cast<const float4 *>(a + c), bv = *reinterpret_cast<const float4 *>(b + c);
            const float d0 = av.x - bv.x, d1 = av.y - bv.y, d2 = av.z - bv.z, d3 = av.w - bv.w;
            s = s + d0 * d0;
            s = s + d1 * d1;
            s = s + d2 * d2;
            s = s + d3 * d3;
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float d = a[c] - b[c];
            s = s + d * d;
        }
    }
    return s;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void flow_seeded_kernel(const FlowSeededArgs p, int32_t n)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int32_t v = i < n ? (int32_t)i : -1;
    int32_t arow = -1;
    int x = 0, y = 0, z = 0, sx = 0, sy = 0, sz = 0;
    bool in_range = true;
    if (v >= 0) {
        arow = seeded_row(p.site_a, p.slot_a, v);
        if (arow >= 0) {
            z = v % p.nz;
            const int xy = v / p.nz;
            y = xy % p.ny;
            x = xy / p.ny;
            if (p.seed) {
                const int32_t *sd = p.seed + 3 * (int64_t)v;
                sx = sd[0]; sy = sd[1]; sz = sd[2];
                in_range = sx >= -D3F_FLOW_SEED_MAX && sx <= D3F_FLOW_SEED_MAX && sy >= -D3F_FLOW_SEED_MAX && sy <= D3F_FLOW_SEED_MAX && sz >= -D3F_FLOW_SEED_MAX &&
                           sz <= D3F_FLOW_SEED_MAX;
            }
        }
    }
    // the window's centre; a member out of range is no work (and its centre is never formed)
    const bool work = arow >= 0 && in_range;
    const int cx = work ? x + sx : 0, cy = work ? y + sy : 0, cz = work ? z + sz : 0;      // |.| < 2^15 + 2^14
    unsigned long long todo = __ballot(work);
    unsigned long long best = kNoKey;
    const int r = p.r, side = 2 * r + 1, total = side * side * side;
    const bool pairs = total <= 32;                                                          // r = 1: two members share the wave
    while (todo) {                                                                           // wave-uniform
        const int m0 = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        int m1 = m0;
        if (pairs && todo) {
            m1 = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
        }
        const bool second = pairs && lane >= 32;
        const int from = second ? m1 : m0;
        const bool idle = second && m1 == m0;                                                // an odd member out: the upper half has none
        const int mx = __shfl(cx, from, 64), my = __shfl(cy, from, 64), mz = __shfl(cz, from, 64);
        const int32_t mrow = __shfl(arow, from, 64);
        const float *a = p.data_a + (int64_t)mrow * p.stride_a;
        unsigned long long key = kNoKey;
        const int step = pairs ? 32 : 64, sub = pairs ? (lane & 31) : lane;
        for (int j0 = 0; j0 < total; j0 += step) {                                           // wave-uniform
            const int j = j0 + sub;
            if (j < total && !idle) {
                const int dx = j / (side * side) - r, dy = (j / side) % side - r, dz = j % side - r;
                const int ux = mx + dx, uy = my + dy, uz = mz + dz;
                if ((unsigned)ux < (unsigned)p.nx && (unsigned)uy < (unsigned)p.ny && (unsigned)uz < (unsigned)p.nz) {
                    const int32_t brow = seeded_row(p.site_b, p.slot_b, (ux * p.ny + uy) * p.nz + uz);
                    if (brow >= 0) {
                        const float s = chain<VEC>(a, p.data_b + (int64_t)brow * p.stride_b, p.C);
                        if (s <= p.max_cost2 && s < __builtin_inff()) {
                            const unsigned long long k = ((unsigned long long)__float_as_uint(s) << 16) | (unsigned long long)((dx * dx + dy * dy + dz * dz) << 10) |
                                                         (unsigned long long)j;
                            if (k < key) key = k;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) {
            if (pairs && w == 32) break;                                                     // a half of the wave is one member
            const unsigned long long other = shuffle_xor_key(key, w);
            if (other < key) key = other;
        }
        // every lane of a half (of the wave at r >= 2) now holds that member's key; the member's own lane may sit in the other half
        const unsigned long long key0 = shuffle_key(key, 0), key1 = shuffle_key(key, 32);
        if (lane == m0)
            best = key0;
        else if (lane == m1)
            best = key1;
    }
    if (v < 0) return;
    int32_t target = -1;
    float cost = __builtin_inff();
    if (best != kNoKey) {
        const int j = (int)(best & 1023u);
        const int dx = j / (side * side) - r, dy = (j / side) % side - r, dz = j % side - r;
        target = ((cx + dx) * p.ny + (cy + dy)) * p.nz + (cz + dz);
        cost = __uint_as_float((unsigned)(best >> 16));
    }
    p.target[v] = target;
    p.cost[v] = cost;
}

}  // namespace

hipError_t launch_flow_seeded(const FlowSeededArgs &A, hipStream_t s)
{
    const int32_t n = A.nx * A.ny * A.nz;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (A.vec)
        hipLaunchKernelGGL((flow_seeded_kernel<true>), grid, block, 0, s, A, n);
    else
        hipLaunchKernelGGL((flow_seeded_kernel<false>), grid, block, 0, s, A, n);
    return hipGetLastError();
}

}  // namespace d3f
