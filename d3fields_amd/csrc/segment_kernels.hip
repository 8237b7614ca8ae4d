// segment_kernels.hip -- can I go straight?  Exact grid segments through a free volume and shortcuts of voxel rows (include/d3fields_hip.h,
// the segment block).
//
// Definitions (the contract; restated in tests/segment_cases.py).  Voxel centres sit at the integer coordinates of index space.  free: uint8
// [nx, ny, nz], z fastest, non-zero = traversable.  The SEGMENT of two voxels a, b is {a + t (b - a), 0 <= t <= 1}.  It TOUCHES a voxel v
//   strict (default)             when the closed cube [v - 1/2, v + 1/2]^3 meets it (the supercover: where the segment passes exactly through
//                                an edge or a corner of the lattice, every cube round that point counts),
//   D3F_SEGMENT_CUT_CORNERS      when the open cube meets it.
// The ends are integers, so the segment never runs inside a face plane and the two rules differ only at isolated edge and corner crossings.
// Every touched voxel lies in the box spanned by a and b: nothing outside the volume is ever read.
//
// THE WALK, all in int32 ((2k + 1) * n < 2^29 for extents up to 16384).  n_i = |b_i - a_i|, s_i = sign(b_i - a_i), k_i = 0, cur = a.  Axis i
// crosses its next plane at t_i = (2 k_i + 1) / (2 n_i); two such values are compared by cross-multiplication.  Event 0 touches {a}.  Every
// further event takes the set E of the axes with k_i < n_i that share the smallest t_i; under the strict rule with |E| >= 2 it touches
// cur + sum of s_i e_i over every non-empty proper subset of E (2 side voxels for |E| = 2, 6 for |E| = 3); then cur and k advance on all of E
// and the event touches the new cur.  At most n_x + n_y + n_z + 1 events; their union is the touched set of the rule, in non-decreasing t.
//
// Per segment: clear = every touched voxel is free; last = cur of the last event before the first event that touches a non-free voxel (b if
// clear, -1 if event 0 is blocked); blocked = the smallest flat index among the non-free voxels of that event (-1 if clear); with a value
// volume, min_value / min_voxel over the voxels of the events before the blocking one: among equal minima the earliest event, then the
// smallest flat index inside it (INT32_MAX / -1 if event 0 is blocked).  An end outside the volume: clear 0, -1, -1, INT32_MAX, -1.
//
//   segment_kernel<strict>   one lane per segment runs the walk: byte loads of free, word loads of value when given.
//   shorten_kernel<strict>   one wave per row, four rows per workgroup.  From anchor i the candidates j = min(L - 1, i + max_span) .. i + 1 are
//                            taken in chunks of 64 from the far end inwards, one candidate per lane, each lane running the same walk; a ballot
//                            picks the largest clear j of the first chunk that has one, which is the largest clear j overall; without one the
//                            next anchor is i + 1.  Lane 0 writes the anchor; the wave pads the row's tail with -1.
// No LDS, no atomics, no workspace; nothing waits for another wave; the loops are bounded by nx + ny + nz events, ceil(max_span / 64)
// chunks and L anchors, all known at launch.  Control flow around the ballot is wave-uniform: a lane without a candidate skips the walk and
// still votes.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int32_t kSegInf = 0x7fffffff;
constexpr int kShortenRows = kBlock / 64;      // rows (waves) per workgroup

struct SegResult {
    int32_t last, blocked, min_value, min_voxel;
    bool clear;
};

// the walk of one segment.  STRICT: the closed-cube rule; VALUE: keep the minimum of `value` (otherwise value is never read)
template <bool STRICT, bool VALUE>
__device__ __forceinline__ SegResult segment_walk(const uint8_t *__restrict__ free, const int32_t *__restrict__ value, int ny, int nz, int32_t n_voxels,
                                                  int32_t a, int32_t b, int max_events)
{
    SegResult R{-1, -1, kSegInf, -1, false};
    if ((uint32_t)a >= (uint32_t)n_voxels || (uint32_t)b >= (uint32_t)n_voxels) return R;
    const int plane = ny * nz;
    const int ax = a / plane, ay = (a - ax * plane) / nz, az = a - ax * plane - ay * nz;
    const int bx = b / plane, by = (b - bx * plane) / nz, bz = b - bx * plane - by * nz;
    const int n0 = abs(bx - ax), n1 = abs(by - ay), n2 = abs(bz - az);
    const int d0 = bx < ax ? -plane : plane, d1 = by < ay ? -nz : nz, d2 = bz < az ? -1 : 1;      // flat-index steps (unused where n_i = 0)
    int k0 = 0, k1 = 0, k2 = 0;
    int32_t cur = a;
    // event 0
    if (free[a] == 0) {
        R.blocked = a;
        return R;
    }
    if (VALUE) {
        R.min_value = value[a];
        R.min_voxel = a;
    }
    for (int e = 0; e < max_events; ++e) {
        const bool l0 = k0 < n0, l1 = k1 < n1, l2 = k2 < n2;
        if (!(l0 || l1 || l2)) break;
        // numerators of t_i over the common denominator 2 n_0 n_1 n_2 are not needed: compare pairwise, (2 k_i + 1) n_j against (2 k_j + 1) n_i
        const int c0 = 2 * k0 + 1, c1 = 2 * k1 + 1, c2 = 2 * k2 + 1;
        // le_ij: t_i <= t_j among live axes (a dead axis is later than every live one)
        const bool le01 = l0 && (!l1 || c0 * n1 <= c1 * n0), le10 = l1 && (!l0 || c1 * n0 <= c0 * n1);
        const bool le02 = l0 && (!l2 || c0 * n2 <= c2 * n0), le20 = l2 && (!l0 || c2 * n0 <= c0 * n2);
        const bool le12 = l1 && (!l2 || c1 * n2 <= c2 * n1), le21 = l2 && (!l1 || c2 * n1 <= c1 * n2);
        const unsigned E = (le01 && le02 ? 1u : 0u) | (le10 && le12 ? 2u : 0u) | (le20 && le21 ? 4u : 0u);
        int32_t bad = -1, ev_min = kSegInf, ev_at = -1;
#pragma unroll
        for (unsigned m = 1; m < 8; ++m) {              // subsets in ascending m; the flat index is not monotone in m, so ties compare indices
            if ((m & ~E) != 0 || (m != E && !STRICT)) continue;
            const int32_t v = cur + ((m & 1u) ? d0 : 0) + ((m & 2u) ? d1 : 0) + ((m & 4u) ? d2 : 0);
            if (free[v] == 0) {
                if (bad < 0 || v < bad) bad = v;
            } else if (VALUE) {
                const int32_t x = value[v];
                if (ev_at < 0 || x < ev_min || (x == ev_min && v < ev_at)) {
                    ev_min = x;
                    ev_at = v;
                }
            }
        }
        if (bad >= 0) {
            R.last = cur;
            R.blocked = bad;
            return R;
        }
        if (VALUE && ev_min < R.min_value) {           // strictly: among equal minima the earliest event stays
            R.min_value = ev_min;
            R.min_voxel = ev_at;
        }
        if (E & 1u) {
            cur += d0;
            ++k0;
        }
        if (E & 2u) {
            cur += d1;
            ++k1;
        }
        if (E & 4u) {
            cur += d2;
            ++k2;
        }
    }
    R.clear = cur == b;      // always true after n_x + n_y + n_z events; a shorter bound would report "not clear" rather than lie
    R.last = cur;
    return R;
}

template <bool STRICT, bool VALUE>
__global__ __launch_bounds__(kBlock) void segment_kernel(const uint8_t *__restrict__ free, const int32_t *__restrict__ value, int ny, int nz, int32_t n_voxels,
                                                         const int32_t *__restrict__ a, const int32_t *__restrict__ b, int64_t n, int max_events,
                                                         uint8_t *__restrict__ out_clear, int32_t *__restrict__ out_last, int32_t *__restrict__ out_blocked,
                                                         int32_t *__restrict__ out_min_value, int32_t *__restrict__ out_min_voxel)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const SegResult R = segment_walk<STRICT, VALUE>(free, value, ny, nz, n_voxels, a[i], b[i], max_events);
    if (out_clear) out_clear[i] = R.clear ? 1 : 0;
    if (out_last) out_last[i] = R.last;
    if (out_blocked) out_blocked[i] = R.blocked;
    if (VALUE) {
        if (out_min_value) out_min_value[i] = R.min_value;
        if (out_min_voxel) out_min_voxel[i] = R.min_voxel;
    }
}

template <bool STRICT>
__global__ __launch_bounds__(kBlock) void shorten_kernel(const uint8_t *__restrict__ free, int ny, int nz, int32_t n_voxels, const int32_t *__restrict__ voxels,
                                                         const int32_t *__restrict__ length, int64_t n, int row_len, int max_span, int max_events,
                                                         int32_t *__restrict__ out_index, int32_t *__restrict__ out_voxels, int32_t *__restrict__ out_count)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kShortenRows + (threadIdx.x >> 6);
    if (r >= n) return;                                  // the whole wave leaves
    const int32_t *row = voxels + r * row_len;
    int32_t *oi = out_index ? out_index + r * row_len : nullptr;
    int32_t *ov = out_voxels ? out_voxels + r * row_len : nullptr;
    const int L = min(max(length[r], 0), row_len);
    int count = 0;
    if (L >= 1) {
        if (lane == 0) {
            if (oi) oi[0] = 0;
            if (ov) ov[0] = row[0];
        }
        count = 1;
    }
    int i = 0;
    for (int anchors = 1; anchors < L && i < L - 1; ++anchors) {      // every anchor advances i by at least 1: at most L - 1 rounds
        const int32_t pi = row[i];
        const int far = i + min(max_span, L - 1 - i);                  // (no i + max_span: max_span may be INT32_MAX)
        int next = i + 1;
        for (int top = far; top > i; top -= 64) {                      // ceil((far - i) / 64) chunks, the far end first
            const int j = top - lane;
            bool clear = false;
            if (j > i) clear = segment_walk<STRICT, false>(free, nullptr, ny, nz, n_voxels, pi, row[j], max_events).clear;
            const unsigned long long votes = __ballot(clear);
            if (votes != 0) {
                next = top - (int)__builtin_ctzll(votes);              // the lowest lane holds the largest j
                break;
            }
        }
        i = next;
        if (lane == 0) {
            if (oi) oi[count] = i;
            if (ov) ov[count] = row[i];
        }
        ++count;
    }
    for (int k = count + lane; k < row_len; k += 64) {
        if (oi) oi[k] = -1;
        if (ov) ov[k] = -1;
    }
    if (lane == 0) out_count[r] = count;
}

}  // namespace

hipError_t launch_volume_segments(const uint8_t *free, const int32_t *value, int nx, int ny, int nz, const int32_t *a, const int32_t *b, int64_t n, bool strict,
                                  uint8_t *out_clear, int32_t *out_last, int32_t *out_blocked, int32_t *out_min_value, int32_t *out_min_voxel, hipStream_t s)
{
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    const int32_t n_voxels = (int32_t)((int64_t)nx * ny * nz);
    const int max_events = nx + ny + nz;
#define D3F_SEG_LAUNCH(STRICT, VALUE)                                                                                                                      \
    hipLaunchKernelGGL((segment_kernel<STRICT, VALUE>), grid, block, 0, s, free, value, ny, nz, n_voxels, a, b, n, max_events, out_clear, out_last, out_blocked, \
                       out_min_value, out_min_voxel)
    if (strict) {
        if (value)
            D3F_SEG_LAUNCH(true, true);
        else
            D3F_SEG_LAUNCH(true, false);
    } else {
        if (value)
            D3F_SEG_LAUNCH(false, true);
        else
            D3F_SEG_LAUNCH(false, false);
    }
#undef D3F_SEG_LAUNCH
    return hipGetLastError();
}

hipError_t launch_path_shorten(const uint8_t *free, int nx, int ny, int nz, const int32_t *voxels, const int32_t *length, int64_t n, int row_len, int max_span,
                               bool strict, int32_t *out_index, int32_t *out_voxels, int32_t *out_count, hipStream_t s)
{
    const dim3 grid((unsigned)((n + kShortenRows - 1) / kShortenRows)), block(kBlock);
    const int32_t n_voxels = (int32_t)((int64_t)nx * ny * nz);
    const int max_events = nx + ny + nz;
    if (strict)
        hipLaunchKernelGGL(shorten_kernel<true>, grid, block, 0, s, free, ny, nz, n_voxels, voxels, length, n, row_len, max_span, max_events, out_index, out_voxels,
                           out_count);
    else
        hipLaunchKernelGGL(shorten_kernel<false>, grid, block, 0, s, free, ny, nz, n_voxels, voxels, length, n, row_len, max_span, max_events, out_index,
                           out_voxels, out_count);
    return hipGetLastError();
}

}  // namespace d3f
