// ccl_kernels.hip -- connected components of a site volume (include/d3fields_hip.h, ABI 15).
//
// Definitions (the contract; restated in tests/ccl_cases.py).  site: uint8 [nx, ny, nz], z fastest, non-zero = site.  Two sites are
// NEIGHBOURS if their integer coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1 for connectivity 6 / 18 / 26.
// Neighbourhood is spatial: (x, y, nz-1) and (x, y+1, 0) are adjacent in memory and are not neighbours.  A COMPONENT is a class of the
// transitive closure; its ROOT is its smallest flat index, its SIZE its voxel count, its BOX the inclusive min / max of x, y, z.
// found = the number of components; the KEPT ones (size >= min_voxels) are numbered 1..K in ascending order of root.
//
// Union-find on one int32 parent volume, the voxel's flat index v along the lanes in every kernel (a wave = 64 consecutive v, whatever
// nz is: lines shorter than 64 share a wave, longer ones span several):
//   ccl_init_kernel     one ballot of the site bytes per wave; a site's first parent is the start of its z run INSIDE the wave (clz of the
//                       masked word, cut at the start of its own line: lane - z): parent <= v, -1 for a non-site.  Zeroes size[] and counts.
//   ccl_merge_kernel    every site unites itself with its neighbours of lower flat index: v-1 across a wave boundary of its own line,
//                       and the lines (x, y-1), (x-1, y), (x-1, y-1), (x-1, y+1) at the z offsets the connectivity allows.  Unite = walk
//                       both to their roots, link the larger root to the smaller with an agent-scope atomic min; lock-free, no waiting.
//   ccl_flatten_kernel  (next launch) every site walks to its root and stores it; integer atomic adds give size[] and found, aggregated
//                       first in the wave (one add per distinct root), then across the turns of a wave and the waves of a workgroup for the
//                       root that holds most of them.  With ccl_box_kernel the only kernel whose workgroup takes iters * 256 voxels (iters =
//                       ceil(n / 131072), at most 64) instead of 256.
//   ccl_flag_kernel     rank[v] = 1 for a root with size >= min_voxels; launch_exclusive_scan_u32 turns it into the number - 1.
//   ccl_label_kernel    out_label, out_count, and {root, size, empty box} of the stats rows below the capacity.
//   ccl_box_kernel      (stats_capacity > 0) the boxes, in the turns of the flatten kernel: each lane grows its own box of the wave's main label
//                       across the turns, then one min / max reduction over the lanes and integer atomics, skipped where the row already
//                       holds the value.
// Parents never rise: every store to parent[] is the init value (<= v) or an atomic min, so a walk strictly descends and terminates.
// Coherence inside the merge launch: parents are read with relaxed agent-scope atomic loads, and the algorithm is also indifferent to a
// stale value -- a parent once stored is an ancestor for good (whoever lowers parent[a] from p to b goes on to unite p with b), and the
// only decisive step is the atomic min, whose return value says whether `a` still was a root.  Flatten runs after the kernel boundary.
// Integer min / max / add only: every output is a function of the input alone, two launches give identical bytes.
// d3f_volume_components_linked (section 24) swaps the first two kernels for ccl_linked_init_kernel / ccl_linked_merge_kernel, which follow the bits of a
// link volume instead of plain adjacency; everything from the flatten kernel on is shared.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int64_t kCclFlattenSpan = 131072;      // ccl_flatten_kernel and ccl_box_kernel: iters = ceil(n / span) turns per workgroup, capped at 64

__device__ __forceinline__ int ccl_load(const int32_t *parent, int a)
{
    return __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int ccl_find(const int32_t *parent, int a)
{
    for (int p = ccl_load(parent, a); p != a; p = ccl_load(parent, a)) a = p;      // p < a: strictly descending
    return a;
}

// max(a, b) strictly falls from one turn to the next: at most v turns
__device__ __forceinline__ void ccl_unite(int32_t *parent, int a, int b)
{
    for (;;) {
        a = ccl_find(parent, a);
        b = ccl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;      // a was a root and now hangs under b
        a = old;                   // a had been linked to old < a meanwhile (its parent is min(old, b) now): old and b remain to be united
    }
}

__global__ __launch_bounds__(kBlock) void ccl_init_kernel(const uint8_t *__restrict__ site, int32_t *__restrict__ parent, int32_t *__restrict__ size,
                                                          int32_t *__restrict__ count, int nz, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool s = v < n && site[v] != 0;
    const unsigned long long word = __ballot(s);
    if (v == 0) count[0] = count[1] = 0;
    if (v >= n) return;
    size[v] = 0;
    int p = -1;
    if (s) {
        const int z = (int)((uint32_t)v % (uint32_t)nz);
        const unsigned long long gaps = ~word & ((1ull << lane) - 1ull);      // the non-sites below this lane
        const int run = gaps ? 64 - __builtin_clzll(gaps) : 0;               // the lane after the highest of them
        const int line = lane - z;                                           // where this lane's own line begins (< 0: in an earlier wave)
        p = (int)v - (lane - max(run, max(line, 0)));
    }
    parent[v] = p;
}

// the neighbouring line at flat offset `at` (its voxel of equal z), WIDE: dz in {-1, 0, 1}, else dz = 0.  down: v-1 is a site of v's line, so
// v and v-1 are one component and every union v-1 makes need not be made again.
template <bool WIDE>
__device__ __forceinline__ void ccl_line(const uint8_t *__restrict__ site, int32_t *parent, int v, int at, int z, int nz, bool down)
{
    const bool c0 = site[at] != 0;
    const bool cm = z > 0 && site[at - 1] != 0;
    if (!WIDE) {
        if (c0 && !(down && cm)) ccl_unite(parent, v, at);      // down && cm: v-1 ~ at-1, and at-1 ~ at is a run
        return;
    }
    const bool cp = z + 1 < nz && site[at + 1] != 0;
    if (c0) {                                                    // at-1, at, at+1: one run as far as they are sites
        if (!down) ccl_unite(parent, v, at);                     // (down: v-1 sees `at` at its dz = +1)
    } else {
        if (cm && !down) ccl_unite(parent, v, at - 1);           // (down: v-1 sees at-1 at its dz = 0)
        if (cp) ccl_unite(parent, v, at + 1);
    }
}

template <int CONN>
__global__ __launch_bounds__(kBlock) void ccl_merge_kernel(const uint8_t *__restrict__ site, int32_t *parent, int ny, int nz, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || site[i] == 0) return;
    const int v = (int)i;
    const uint32_t l = (uint32_t)v / (uint32_t)nz;
    const int z = (int)((uint32_t)v - l * (uint32_t)nz);
    const uint32_t x = l / (uint32_t)ny;
    const int y = (int)(l - x * (uint32_t)ny);
    const bool down = z > 0 && site[v - 1] != 0;
    if (down && (v & 63) == 0) ccl_unite(parent, v, v - 1);      // the run goes on across the wave boundary of ccl_init_kernel
    const int plane = ny * nz;
    if (y > 0) ccl_line<CONN != 6>(site, parent, v, v - nz, z, nz, down);
    if (x > 0) {
        ccl_line<CONN != 6>(site, parent, v, v - plane, z, nz, down);
        if (CONN != 6) {
            if (y > 0) ccl_line<CONN == 26>(site, parent, v, v - plane - nz, z, nz, down);
            if (y + 1 < ny) ccl_line<CONN == 26>(site, parent, v, v - plane + nz, z, nz, down);
        }
    }
}

// ---- components over a link volume (d3f_volume_components_linked) ----
// links: uint16 [nx, ny, nz] as d3f_volume_links writes it -- bit j of voxel v names the neighbour at offset j = 9*(dx+1) + 3*(dy+1) + (dz+1),
// j = 0..12, all of lower flat index.  Two sites are united iff the higher one's bit is set, the connectivity allows the offset (conn_mask),
// and the neighbour lies inside the volume and is a site: a bit that fails one of these is ignored and never followed, so a caller's own bits
// cannot cause a read outside the volume.  Only the first two kernels differ from the site-only labelling; parents still never rise.

// v is tied to v - 1 by bit 12: the same test in both kernels
__device__ __forceinline__ bool ccl_link_down(const uint8_t *__restrict__ site, const uint16_t *__restrict__ links, int64_t v, int z, uint32_t conn_mask)
{
    return z > 0 && (links[v] & conn_mask & 0x1000u) != 0 && site[v - 1] != 0;
}

// ccl_init_kernel with runs of "bit 12 set" instead of runs of sites: a site's first parent is the lowest voxel it reaches through consecutive
// bit-12 links INSIDE the wave (a link needs z > 0, so a run never crosses a line start).
__global__ __launch_bounds__(kBlock) void ccl_linked_init_kernel(const uint8_t *__restrict__ site, const uint16_t *__restrict__ links, int32_t *__restrict__ parent,
                                                                 int32_t *__restrict__ size, int32_t *__restrict__ count, int nz, uint32_t conn_mask, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool s = v < n && site[v] != 0;
    const bool tied = s && ccl_link_down(site, links, v, (int)((uint32_t)v % (uint32_t)nz), conn_mask);
    const unsigned long long word = __ballot(tied);
    if (v == 0) count[0] = count[1] = 0;
    if (v >= n) return;
    size[v] = 0;
    int p = -1;
    if (s) {
        const unsigned long long loose = ~word & ((2ull << lane) - 1ull);      // the lanes up to this one that are not tied to the lane below
        const int start = loose ? 63 - __builtin_clzll(loose) : 0;            // the highest of them begins the run (none: the run enters from the wave below)
        p = (int)v - (lane - start);
    }
    parent[v] = p;
}

__global__ __launch_bounds__(kBlock) void ccl_linked_merge_kernel(const uint8_t *__restrict__ site, const uint16_t *__restrict__ links, int32_t *parent, int ny,
                                                                  int nz, uint32_t conn_mask, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || site[i] == 0) return;
    const int v = (int)i;
    const uint32_t bits = links[v] & conn_mask;
    if (bits == 0) return;
    const uint32_t l = (uint32_t)v / (uint32_t)nz;
    const int z = (int)((uint32_t)v - l * (uint32_t)nz);
    const uint32_t x = l / (uint32_t)ny;
    const int y = (int)(l - x * (uint32_t)ny);
    if ((v & 63) == 0 && ccl_link_down(site, links, v, z, conn_mask)) ccl_unite(parent, v, v - 1);      // the run goes on across the wave boundary of the init kernel
    const int plane = ny * nz;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int dx = j / 9 - 1, dy = (j / 3) % 3 - 1, dz = j % 3 - 1;
        if (!((bits >> j) & 1u)) continue;
        if (dx < 0 && x == 0) continue;
        if ((unsigned)(y + dy) >= (unsigned)ny || (unsigned)(z + dz) >= (unsigned)nz) continue;
        const int u = v + dx * plane + dy * nz + dz;
        if (site[u] != 0) ccl_unite(parent, v, u);
    }
}

// A workgroup takes iters * 256 consecutive voxels, 256 at a time.  Sizes: a wave keeps ONE (root, count) pair in registers across its turns -- the
// root with the most voxels so far; any other root of a turn costs one atomic add of its own -- and the four pairs of a workgroup are joined
// through LDS, so the voxels of a large component arrive as one add per workgroup, not one per wave: those adds all hit one word.
__global__ __launch_bounds__(kBlock) void ccl_flatten_kernel(int32_t *parent, int32_t *__restrict__ size, int32_t *__restrict__ count, int iters, int64_t n)
{
    __shared__ int s_root[kBlock / 64], s_count[kBlock / 64], s_roots[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kBlock * iters + threadIdx.x;
    int held = -1, held_count = 0, roots = 0;                   // the same in every lane of the wave
    for (int i = 0; i < iters; ++i) {
        const int64_t v = base + (int64_t)i * kBlock;
        int r = -1;
        if (v < n) {
            r = parent[v];
            if (r >= 0) {
                // another lane may store its root into a word of this walk meanwhile: that is an ancestor too, and a root's word never changes
                for (int p = parent[r]; p != r; p = parent[r]) r = p;
                parent[v] = r;
            }
        }
        roots += (int)__builtin_popcountll(__ballot(r >= 0 && r == (int)v));
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {                                          // one turn per distinct root of the 64 voxels (usually one or two)
            const int rl = __shfl(r, (int)__builtin_ctzll(todo));
            const unsigned long long same = __ballot(r == rl) & todo;
            const int c = (int)__builtin_popcountll(same);
            if (rl == held) {
                held_count += c;
            } else if (c > held_count) {
                if (held_count > 0 && lane == 0) atomicAdd(size + held, held_count);
                held = rl;
                held_count = c;
            } else if (lane == 0) {
                atomicAdd(size + rl, c);
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        s_root[wave] = held;
        s_count[wave] = held_count;
        s_roots[wave] = roots;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            total += s_roots[w];
            int c = s_count[w];
            if (c == 0) continue;
            for (int u = w + 1; u < kBlock / 64; ++u)
                if (s_root[u] == s_root[w]) {
                    c += s_count[u];
                    s_count[u] = 0;
                }
            atomicAdd(size + s_root[w], c);
        }
        if (total > 0) atomicAdd(count + 1, total);            // found
    }
}

__global__ __launch_bounds__(kBlock) void ccl_flag_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size, uint32_t *__restrict__ rank,
                                                          int min_voxels, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < n) rank[v] = parent[v] == (int)v && size[v] >= min_voxels;
}

__global__ __launch_bounds__(kBlock) void ccl_label_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size, const uint32_t *__restrict__ rank,
                                                           int32_t *__restrict__ label, int32_t *__restrict__ count, int32_t *__restrict__ stats,
                                                           int capacity, int min_voxels, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    const int r = parent[v];
    int k = 0, sz = 0;
    if (r >= 0) {
        sz = size[r];
        if (sz >= min_voxels) k = (int)rank[r] + 1;
    }
    label[v] = k;
    const bool root = k > 0 && r == (int)v;
    if (root && k <= capacity) {
        int32_t *row = stats + (int64_t)(k - 1) * 8;
        row[0] = r;
        row[1] = sz;
        row[2] = row[3] = row[4] = 0x7fffffff;
        row[5] = row[6] = row[7] = -1;
    }
    if (v == n - 1) count[0] = (int)rank[v] + (root ? 1 : 0);      // (count[1] = found: ccl_flatten_kernel)
}

__device__ __forceinline__ int ccl_wave_min(int a)
{
    for (int o = 32; o > 0; o >>= 1) a = min(a, __shfl_xor(a, o));
    return a;
}

// the wave's box of component k (each lane's own partial box; the identity where it has none) into the stats row: one min / max reduction over
// the lanes, then six lanes issue integer atomics, skipped where the row already holds a value at least as extreme.  Called by whole waves.
__device__ __forceinline__ void ccl_box_flush(int32_t *stats, int k, int lane, int x0, int y0, int z0, int x1, int y1, int z1)
{
    x0 = ccl_wave_min(x0), y0 = ccl_wave_min(y0), z0 = ccl_wave_min(z0);
    x1 = -ccl_wave_min(-x1), y1 = -ccl_wave_min(-y1), z1 = -ccl_wave_min(-z1);
    if (lane < 6) {
        int32_t *word = stats + (int64_t)(k - 1) * 8 + 2 + lane;
        const int mine = lane == 0 ? x0 : lane == 1 ? y0 : lane == 2 ? z0 : lane == 3 ? x1 : lane == 4 ? y1 : z1;
        // a stale value is a box not yet grown that far: it can only cost an atomic that changes nothing, never drop one
        const int have = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < 3) {
            if (mine < have) __hip_atomic_fetch_min(word, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (mine > have) __hip_atomic_fetch_max(word, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The turns of ccl_flatten_kernel: a wave HOLDS one label -- the one with the most voxels so far -- and every lane grows its own partial box of
// it in registers across the turns; the cross-lane reduction and the atomics happen once, when the label is given up or the wave ends.  Any
// other label of a turn is reduced and sent at once.
__global__ __launch_bounds__(kBlock) void ccl_box_kernel(const int32_t *__restrict__ label, int32_t *stats, int capacity, int ny, int nz, int iters, int64_t n)
{
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kBlock * iters + threadIdx.x;
    const int big = 0x7fffffff;
    int held = 0, held_count = 0;                               // the same in every lane of the wave
    int bx0 = big, by0 = big, bz0 = big, bx1 = -1, by1 = -1, bz1 = -1;
    for (int t = 0; t < iters; ++t) {
        const int64_t i = base + (int64_t)t * kBlock;
        int k = 0, x = 0, y = 0, z = 0;
        if (i < n) {
            k = label[i];
            if (k > capacity) k = 0;
            if (k > 0) {
                const uint32_t l = (uint32_t)i / (uint32_t)nz;
                z = (int)((uint32_t)i - l * (uint32_t)nz);
                x = (int)(l / (uint32_t)ny);
                y = (int)(l - (uint32_t)x * (uint32_t)ny);
            }
        }
        unsigned long long todo = __ballot(k > 0);
        while (todo) {                                          // uniform over the wave: every lane takes part in the reductions
            const int kl = __shfl(k, (int)__builtin_ctzll(todo));
            const bool in = k == kl;
            const unsigned long long same = __ballot(in);
            const int c = (int)__builtin_popcountll(same);
            if (kl != held && c > held_count) {
                if (held_count > 0) ccl_box_flush(stats, held, lane, bx0, by0, bz0, bx1, by1, bz1);
                held = kl;
                held_count = 0;
                bx0 = by0 = bz0 = big;
                bx1 = by1 = bz1 = -1;
            }
            if (kl == held) {
                held_count += c;
                if (in) {
                    bx0 = min(bx0, x), by0 = min(by0, y), bz0 = min(bz0, z);
                    bx1 = max(bx1, x), by1 = max(by1, y), bz1 = max(bz1, z);
                }
            } else {
                ccl_box_flush(stats, kl, lane, in ? x : big, in ? y : big, in ? z : big, in ? x : -1, in ? y : -1, in ? z : -1);
            }
            todo &= ~same;
        }
    }
    if (held_count > 0) ccl_box_flush(stats, held, lane, bx0, by0, bz0, bx1, by1, bz1);
}

}  // namespace

// parent, size, rank: int32 [n] each, back to back, then the scratch of the scan
CclLayout ccl_layout(int64_t n)
{
    CclLayout L;
    Carve c;
    L.parent = c.take(4 * n, 4);
    L.size = c.take(4 * n, 4);
    L.rank = c.take(4 * n, 4);
    L.scan = c.take(scan_scratch_bytes(n), 4);
    L.total = c.at;
    return L;
}

// flatten, count, number, label and box: everything after the merge kernel, the same for both labellings
static hipError_t ccl_finish(int ny, int nz, int64_t n, int min_voxels, void *workspace, const CclLayout &L, int32_t *out_label, int32_t *out_count,
                             int32_t *out_stats, int capacity, hipStream_t s)
{
    int32_t *parent = static_cast<int32_t *>(ws_at(workspace, L.parent)), *size = static_cast<int32_t *>(ws_at(workspace, L.size));
    uint32_t *rank = static_cast<uint32_t *>(ws_at(workspace, L.rank));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    // about 512 workgroups, at most 64 turns each: few enough adds on the word of a component that spans the volume, enough waves to hide the walks
    const int iters = (int)std::min<int64_t>(64, (n + kCclFlattenSpan - 1) / kCclFlattenSpan);
    const int64_t span = (int64_t)kBlock * iters;
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)((n + span - 1) / span)), block, 0, s, parent, size, out_count, iters, n);
    hipLaunchKernelGGL(ccl_flag_kernel, grid, block, 0, s, parent, size, rank, min_voxels, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan_u32(rank, rank, n, ws_at(workspace, L.scan), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ccl_label_kernel, grid, block, 0, s, parent, size, rank, out_label, out_count, out_stats, capacity, min_voxels, n);
    if (capacity > 0) hipLaunchKernelGGL(ccl_box_kernel, dim3((unsigned)((n + span - 1) / span)), block, 0, s, out_label, out_stats, capacity, ny, nz, iters, n);
    return hipGetLastError();
}

hipError_t launch_volume_components(const uint8_t *site, int nx, int ny, int nz, int connectivity, int min_voxels, int32_t *out_label, int32_t *out_count,
                                    int32_t *out_stats, int capacity, void *workspace, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz;
    const CclLayout L = ccl_layout(n);
    int32_t *parent = static_cast<int32_t *>(ws_at(workspace, L.parent)), *size = static_cast<int32_t *>(ws_at(workspace, L.size));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(ccl_init_kernel, grid, block, 0, s, site, parent, size, out_count, nz, n);
    if (connectivity == 6)
        hipLaunchKernelGGL(ccl_merge_kernel<6>, grid, block, 0, s, site, parent, ny, nz, n);
    else if (connectivity == 18)
        hipLaunchKernelGGL(ccl_merge_kernel<18>, grid, block, 0, s, site, parent, ny, nz, n);
    else
        hipLaunchKernelGGL(ccl_merge_kernel<26>, grid, block, 0, s, site, parent, ny, nz, n);
    return ccl_finish(ny, nz, n, min_voxels, workspace, L, out_label, out_count, out_stats, capacity, s);
}

hipError_t launch_volume_components_linked(const uint8_t *site, const uint16_t *links, int nx, int ny, int nz, int connectivity, int min_voxels,
                                           int32_t *out_label, int32_t *out_count, int32_t *out_stats, int capacity, void *workspace, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz;
    const CclLayout L = ccl_layout(n);
    int32_t *parent = static_cast<int32_t *>(ws_at(workspace, L.parent)), *size = static_cast<int32_t *>(ws_at(workspace, L.size));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    const uint32_t conn_mask = connectivity == 6 ? 0x1410u : connectivity == 18 ? 0x1ebau : 0x1fffu;      // bits by |dx|+|dy|+|dz| (parts_kernels.hip)
    hipLaunchKernelGGL(ccl_linked_init_kernel, grid, block, 0, s, site, links, parent, size, out_count, nz, conn_mask, n);
    hipLaunchKernelGGL(ccl_linked_merge_kernel, grid, block, 0, s, site, links, parent, ny, nz, conn_mask, n);
    return ccl_finish(ny, nz, n, min_voxels, workspace, L, out_label, out_count, out_stats, capacity, s);
}

}  // namespace d3f
