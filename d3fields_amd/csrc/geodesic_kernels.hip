// geodesic_kernels.hip -- cost-to-go through free space: exact shortest paths on the voxel lattice (include/d3fields_hip.h, the geodesic
// block).
//
// Definitions (the contract; restated in tests/geodesic_cases.py).  free: uint8 [nx, ny, nz], z fastest, non-zero = traversable.
// NEIGHBOURS: coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1 for connectivity 6 / 18 / 26; nothing wraps
// through memory.  A MOVE between neighbours u, v exists when both are free and costs w[|u - v|_1 - 1] + penalty[v], w = (w1, w2, w3)
// integers with 1 <= w1 <= w2 <= w3 <= 255, penalty an optional int32 volume charged for entering v (NULL: zero; a negative entry is read
// as 0).  cost[v] (int32) = the minimum over all move sequences from any seed to v of the summed move costs; a seed has cost 0 and its own
// penalty is not charged; a candidate is formed in unsigned arithmetic (it never wraps) and discarded above max_cost; an unreached voxel
// holds INT32_MAX.  next[v] = among the neighbours u with cost[u] + w(u, v) + penalty[v] == cost[v] the one with the smallest flat index;
// v itself for a seed, -1 where unreached.  dist[v] = (float)cost[v] * (step / (float)w1), +inf where unreached.
//
// Block-based fast iterative method with integer costs.  The volume is cut into tiles of kGeoTX x kGeoTY x kGeoTZ voxels:
//   geo_init_kernel     cost = INT32_MAX everywhere, every tile flag and both list counts 0 (every workspace word is written here or below)
//   geo_seed_kernel     cost = 0 at the accepted seeds; the seed's own tile and every tile that holds one of its 26 neighbours are flagged (a seed on a
//                       tile face, edge or corner is seen by up to 8 tiles).  Plain stores of one value: duplicates are harmless.
//   geo_compact_kernel  flagged tiles -> the tile list: one ballot per wave, one integer atomic add per wave on the list's count, the flags
//                       cleared for the next round.  The ORDER of the list depends on how the adds land; no output does (see below).
//   geo_tile_kernel     one workgroup per listed tile (surplus workgroups of the launch exit on the device count): the tile plus a one-voxel
//                       halo of cost into LDS, free / penalty of the own voxels into registers; Jacobi passes over the own voxels against
//                       their up to 26 neighbours from LDS until a pass changes nothing or kGeoInnerCap passes ran; own voxels that fell
//                       are written back; the tile flags the neighbour tiles that touch a voxel that fell (a 27-bit mask, OR-ed through
//                       LDS), and itself if the capped last pass still changed something.
//   geo_pending_kernel  out_pending = the count of the list for the round after the last, which also moves into slot 0 for the next call.
//   geo_finish_kernel   one thread per voxel: next by the rule above from the final costs, and dist.
//   geo_follow_kernel   one lane per start: walks next for at most max_steps steps.
// Only the owner writes a tile's costs: no atomic on a cost word.  A non-free voxel holds INT32_MAX for good, and INT32_MAX + w + penalty
// exceeds every legal max_cost in uint32, so "the neighbour is free" needs no test of its own.
// Why it is exact despite the races: every stored value is INT32_MAX or the cost of a real path; values only fall; a halo word read while
// its owner rewrites it is an old or a new value of that kind (aligned 32-bit words do not tear); whoever lowers a voxel -- the seed kernel (INT32_MAX -> 0)
// or a tile run -- flags every tile that holds a neighbour of it, so every tile whose neighbourhood changed runs again after the kernel boundary.
// The process therefore ends only where no move can lower any voxel, and with w1 >= 1 that state is the unique shortest-path solution: the same bytes on every run, whatever the order of tiles, rounds or list entries.
// Nothing waits for another workgroup; every loop has a bound known at launch (the inner cap, the tile size, ceil(tiles / grid)).
#include "d3f_internal.h"

namespace d3f {

namespace {

// Tile shape, row padding, inner cap and grid were chosen by measurement: 8 x 8 x 8 needs the fewest rounds (the front moves a tile
// per round on every axis), and beats 4 x 4 x 32 and 4 x 8 x 16 once its LDS rows are padded.
constexpr int kGeoTX = 8, kGeoTY = 8, kGeoTZ = 8;
constexpr int kGeoHX = kGeoTX + 2, kGeoHY = kGeoTY + 2, kGeoHZ = kGeoTZ + 2;
constexpr int kGeoHalo = kGeoHX * kGeoHY * kGeoHZ;                     // words loaded per tile
// words between two z rows in LDS.  A 32-lane half wave reads four rows of 8 words (y .. y + 3) at one offset; with 24 words between rows they start
// at banks 0, 24, 16, 8 of the 32 a ds_read_b32 sees: no bank conflict.  The unpadded 10 puts the fourth row onto six banks of the first.
constexpr int kGeoRow = 24;
static_assert(kGeoRow >= kGeoHZ, "a row holds the tile's z extent and both halo words");
constexpr int kGeoSY = kGeoRow, kGeoSX = kGeoHY * kGeoRow;             // LDS strides of y and x
constexpr int kGeoLds = kGeoHX * kGeoSX;                               // words of LDS
constexpr int kGeoInnerCap = 8;
constexpr int kGeoMaxGrid = 4096;                                      // workgroups of one tile launch; a workgroup takes ceil(listed / grid) tiles
constexpr uint32_t kGeoInf = 0x7fffffffu;
constexpr int kGeoHeaderWords = 16;                                    // count[0], count[1], padding
static_assert(kGeoTX * kGeoTY * kGeoTZ == 2 * kBlock && kGeoTX % 2 == 0, "two voxels per lane: local x and x + kGeoTX / 2");

// the tile offsets (bit (dx+1)*9 + (dy+1)*3 + (dz+1)) that hold a neighbour of one of the tile's voxels under a connectivity, plus the tile itself
constexpr uint32_t geo_tile_mask(int conn)
{
    const int reach = conn == 6 ? 1 : conn == 18 ? 2 : 3;
    uint32_t m = 0;
    for (int b = 0; b < 27; ++b) {
        const int dx = b / 9 - 1, dy = (b / 3) % 3 - 1, dz = b % 3 - 1;
        const int l1 = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
        if (l1 <= reach) m |= 1u << b;
    }
    return m;
}

struct GeoTiles {
    int nx, ny, nz;
    int tx, ty, tz;      // tiles along each axis
};

// the tiles that hold the voxel at local (x, y, z) of a tile or one of its 26 neighbours: bit (dx+1)*9 + (dy+1)*3 + (dz+1), the tile itself included.
// THE invariant of the solve: whoever lowers a voxel -- the seed kernel or a tile run -- flags every tile of this mask (a tile run may drop the offsets
// its connectivity cannot reach, and its own bit), so every tile that can see the new value runs after the kernel boundary.
__device__ __forceinline__ uint32_t geo_touch_mask(int x, int y, int z)
{
    const uint32_t mz = 2u | (z == 0 ? 1u : 0u) | (z == kGeoTZ - 1 ? 4u : 0u);
    const uint32_t myz = (y == 0 ? mz : 0u) | (mz << 3) | (y == kGeoTY - 1 ? mz << 6 : 0u);
    return (x == 0 ? myz : 0u) | (myz << 9) | (x == kGeoTX - 1 ? myz << 18 : 0u);
}

// stores the flags of the tiles in `mask` around tile (bx, by, bz) that exist; called by up to 27 lanes or in a loop of 27
__device__ __forceinline__ void geo_flag_tile(uint32_t *flags, const GeoTiles &G, uint32_t mask, int bit, int bx, int by, int bz)
{
    if (!((mask >> bit) & 1u)) return;
    const int ax = bx + bit / 9 - 1, ay = by + (bit / 3) % 3 - 1, az = bz + bit % 3 - 1;
    if (ax >= 0 && ax < G.tx && ay >= 0 && ay < G.ty && az >= 0 && az < G.tz) flags[(ax * G.ty + ay) * G.tz + az] = 1;
}

__global__ __launch_bounds__(kBlock) void geo_init_kernel(int32_t *__restrict__ cost, uint32_t *__restrict__ header, uint32_t *__restrict__ flags, int64_t n,
                                                          int64_t tiles)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < n) cost[v] = (int32_t)kGeoInf;
    if (v < tiles) flags[v] = 0;
    if (v < kGeoHeaderWords) header[v] = 0;
}

__global__ __launch_bounds__(kBlock) void geo_seed_kernel(const uint8_t *__restrict__ free, const int32_t *__restrict__ seeds, int64_t n_seeds,
                                                          int32_t *__restrict__ cost, uint32_t *__restrict__ flags, GeoTiles G, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_seeds) return;
    const int s = seeds[i];
    if (s < 0 || (int64_t)s >= n || free[s] == 0) return;
    cost[s] = 0;
    // the seed was lowered (INT32_MAX -> 0) here, not by a tile run: its own tile and every tile that holds one of its 26 neighbours must run.
    // (The connectivity is not known yet: a tile flagged for a neighbour the connectivity cannot reach runs once and changes nothing.)
    const uint32_t l = (uint32_t)s / (uint32_t)G.nz;
    const int z = (int)((uint32_t)s - l * (uint32_t)G.nz);
    const int x = (int)(l / (uint32_t)G.ny);
    const int y = (int)(l - (uint32_t)x * (uint32_t)G.ny);
    const uint32_t mask = geo_touch_mask(x % kGeoTX, y % kGeoTY, z % kGeoTZ);
    for (int bit = 0; bit < 27; ++bit) geo_flag_tile(flags, G, mask, bit, x / kGeoTX, y / kGeoTY, z / kGeoTZ);
}

// count_ran: the list length of the tile round that just ran, or nullptr (after the seeds).  A round that ran no tile set no flag: nothing to read.
__global__ __launch_bounds__(kBlock) void geo_compact_kernel(uint32_t *__restrict__ flags, uint32_t *__restrict__ list, uint32_t *count_out,
                                                             const uint32_t *__restrict__ count_ran, int64_t tiles)
{
    if (count_ran && *count_ran == 0) return;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool f = t < tiles && flags[t] != 0;
    const unsigned long long word = __ballot(f);
    if (word == 0) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count_out, (uint32_t)__builtin_popcountll(word));
    base = __shfl(base, 0);
    if (f) {
        flags[t] = 0;
        list[base + (uint32_t)__builtin_popcountll(word & ((1ull << lane) - 1ull))] = (uint32_t)t;
    }
}

struct GeoRelax {
    const uint8_t *free;
    const int32_t *penalty;      // or nullptr
    int32_t *cost;               // read (halo: possibly while its owner writes) and written (own voxels)
    const uint32_t *list;
    const uint32_t *count;       // the list's length
    uint32_t *count_next;        // zeroed here for the compaction that follows
    uint32_t *flags;
    GeoTiles G;
    uint32_t w1, w2, w3, max_cost;
};

// the cheapest candidate for the voxel at LDS word c: min over the classes of (cheapest neighbour + the class weight), + the voxel's penalty.
// uint32 throughout: at most (2^31 - 1) + 255 + (2^31 - 1) < 2^32.
template <int CONN>
__device__ __forceinline__ uint32_t geo_candidate(const uint32_t *s, int c, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t pen)
{
    uint32_t m = min(min(s[c - 1], s[c + 1]), min(min(s[c - kGeoSY], s[c + kGeoSY]), min(s[c - kGeoSX], s[c + kGeoSX]))) + w1;
    if (CONN != 6) {
        uint32_t e = min(min(s[c - kGeoSY - 1], s[c - kGeoSY + 1]), min(s[c + kGeoSY - 1], s[c + kGeoSY + 1]));
        e = min(e, min(min(s[c - kGeoSX - 1], s[c - kGeoSX + 1]), min(s[c + kGeoSX - 1], s[c + kGeoSX + 1])));
        e = min(e, min(min(s[c - kGeoSX - kGeoSY], s[c - kGeoSX + kGeoSY]), min(s[c + kGeoSX - kGeoSY], s[c + kGeoSX + kGeoSY])));
        m = min(m, e + w2);
    }
    if (CONN == 26) {
        uint32_t k = min(min(s[c - kGeoSX - kGeoSY - 1], s[c - kGeoSX - kGeoSY + 1]), min(s[c - kGeoSX + kGeoSY - 1], s[c - kGeoSX + kGeoSY + 1]));
        k = min(k, min(min(s[c + kGeoSX - kGeoSY - 1], s[c + kGeoSX - kGeoSY + 1]), min(s[c + kGeoSX + kGeoSY - 1], s[c + kGeoSX + kGeoSY + 1])));
        m = min(m, k + w3);
    }
    return m + pen;
}

template <int CONN>
__global__ __launch_bounds__(kBlock) void geo_tile_kernel(GeoRelax P)
{
    __shared__ uint32_t s_cost[kGeoLds];
    __shared__ uint32_t s_mask;
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.count_next = 0;      // nobody reads it in this launch
    const uint32_t listed = *P.count;
    const int t = threadIdx.x;
    const int lz = t % kGeoTZ, ly = (t / kGeoTZ) % kGeoTY, lx = t / (kGeoTZ * kGeoTY);      // the lane's voxels: local x = lx and lx + kGeoTX / 2
    const int nx = P.G.nx, ny = P.G.ny, nz = P.G.nz;
    for (uint32_t i = blockIdx.x; i < listed; i += gridDim.x) {     // at most ceil(tiles / gridDim.x) turns
        const uint32_t tile = P.list[i];
        const uint32_t txy = tile / (uint32_t)P.G.tz;
        const int bz = (int)(tile - txy * (uint32_t)P.G.tz);
        const int bx = (int)(txy / (uint32_t)P.G.ty);
        const int by = (int)(txy - (uint32_t)bx * (uint32_t)P.G.ty);
        const int x0 = bx * kGeoTX, y0 = by * kGeoTY, z0 = bz * kGeoTZ;
        for (int k = t; k < kGeoHalo; k += kBlock) {
            const int hz = k % kGeoHZ, r = k / kGeoHZ;
            const int hy = r % kGeoHY, hx = r / kGeoHY;
            const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
            uint32_t c = kGeoInf;                                    // outside the volume: no neighbour, nothing wraps
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) c = (uint32_t)P.cost[((int64_t)gx * ny + gy) * nz + gz];
            s_cost[r * kGeoRow + hz] = c;
        }
        if (t == 0) s_mask = 0;
        int64_t v[2];
        int at[2];
        bool open[2];
        uint32_t pen[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gx = x0 + lx + j * (kGeoTX / 2), gy = y0 + ly, gz = z0 + lz;
            const bool in = gx < nx && gy < ny && gz < nz;
            v[j] = in ? ((int64_t)gx * ny + gy) * nz + gz : -1;
            at[j] = (lx + j * (kGeoTX / 2) + 1) * kGeoSX + (ly + 1) * kGeoSY + lz + 1;
            open[j] = in && P.free[v[j]] != 0;
            pen[j] = 0;
            if (open[j] && P.penalty) pen[j] = (uint32_t)max(P.penalty[v[j]], 0);
        }
        __syncthreads();
        uint32_t own[2] = {s_cost[at[0]], s_cost[at[1]]};
        const uint32_t first[2] = {own[0], own[1]};
        int again = 0;
        for (int pass = 0; pass < kGeoInnerCap; ++pass) {
            uint32_t now[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                now[j] = own[j];
                if (open[j]) {
                    const uint32_t c = geo_candidate<CONN>(s_cost, at[j], P.w1, P.w2, P.w3, pen[j]);
                    if (c <= P.max_cost && c < own[j]) now[j] = c;
                }
            }
            __syncthreads();                                         // every read of this pass is done
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (now[j] < own[j]) s_cost[at[j]] = now[j];
            const int fell = now[0] < own[0] || now[1] < own[1];
            own[0] = now[0];
            own[1] = now[1];
            again = __syncthreads_or(fell);
            if (!again) break;
        }
        uint32_t touch = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (own[j] < first[j]) {                                 // (only a voxel inside the volume can fall)
                P.cost[v[j]] = (int32_t)own[j];
                touch |= geo_touch_mask(lx + j * (kGeoTX / 2), ly, lz);
            }
        touch &= ~(1u << 13);
        if (again) touch |= 1u << 13;                                // the capped last pass still changed something: run this tile again
        for (int o = 32; o > 0; o >>= 1) touch |= (uint32_t)__shfl_xor((int)touch, o);
        if ((t & 63) == 0 && touch) atomicOr(&s_mask, touch);
        __syncthreads();
        if (t < 27) geo_flag_tile(P.flags, P.G, s_mask & geo_tile_mask(CONN), t, bx, by, bz);
        __syncthreads();                                             // s_cost and s_mask are free for the next turn
    }
}

__global__ void geo_pending_kernel(uint32_t *header, int slot, int32_t *__restrict__ out_pending)
{
    const uint32_t c = header[slot];
    header[0] = c;
    out_pending[0] = (int32_t)c;
}

template <int CONN>
__global__ __launch_bounds__(kBlock) void geo_finish_kernel(const uint8_t *__restrict__ free, const int32_t *__restrict__ penalty, const int32_t *__restrict__ cost,
                                                            int32_t *__restrict__ out_next, float *__restrict__ out_dist, int nx, int ny, int nz, uint32_t w1,
                                                            uint32_t w2, uint32_t w3, float scale, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = (uint32_t)cost[i];
    if (out_dist) out_dist[i] = c == kGeoInf ? __builtin_inff() : (float)(int32_t)c * scale;
    if (!out_next) return;
    int best = -1;
    if (c == 0) {
        best = (int)i;                                               // w1 >= 1: only a seed costs nothing
    } else if (c != kGeoInf && free[i] != 0) {
        const int v = (int)i;
        const uint32_t l = (uint32_t)v / (uint32_t)nz;
        const int z = (int)((uint32_t)v - l * (uint32_t)nz);
        const int x = (int)(l / (uint32_t)ny);
        const int y = (int)(l - (uint32_t)x * (uint32_t)ny);
        const uint32_t pen = penalty ? (uint32_t)max(penalty[i], 0) : 0u;
        const int plane = ny * nz;
        // descending flat index, the last match kept: the smallest flat index wins
#pragma unroll
        for (int dx = 1; dx >= -1; --dx)
#pragma unroll
            for (int dy = 1; dy >= -1; --dy)
#pragma unroll
                for (int dz = 1; dz >= -1; --dz) {
                    const int l1 = (dx != 0) + (dy != 0) + (dz != 0);
                    if (l1 == 0 || l1 > (CONN == 6 ? 1 : CONN == 18 ? 2 : 3)) continue;
                    if (x + dx < 0 || x + dx >= nx || y + dy < 0 || y + dy >= ny || z + dz < 0 || z + dz >= nz) continue;
                    const int u = v + dx * plane + dy * nz + dz;
                    const uint32_t cu = (uint32_t)cost[u];           // a non-free or unreached u holds INT32_MAX: the sum then exceeds every cost
                    if (cu + (l1 == 1 ? w1 : l1 == 2 ? w2 : w3) + pen == c) best = u;
                }
    }
    out_next[i] = best;
}

__global__ __launch_bounds__(kBlock) void geo_follow_kernel(const int32_t *__restrict__ next, int64_t n_voxels, const int32_t *__restrict__ starts, int64_t n,
                                                            int max_steps, int32_t *__restrict__ out_voxels, int32_t *__restrict__ out_length,
                                                            uint8_t *__restrict__ out_reached)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int32_t *row = out_voxels + i * max_steps;
    int s = starts[i];
    int length = 0;
    bool reached = false;
    if (s >= 0 && (int64_t)s < n_voxels && next[s] >= 0) {
        while (length < max_steps) {
            row[length++] = s;
            const int to = next[s];
            if (to == s) {
                reached = true;
                break;
            }
            if (to < 0 || (int64_t)to >= n_voxels) break;            // not a next volume of geo_finish_kernel: stop rather than index with it
            s = to;
        }
    }
    for (int k = length; k < max_steps; ++k) row[k] = -1;
    out_length[i] = length;
    out_reached[i] = reached ? 1 : 0;
}

GeoTiles geo_tiles(int nx, int ny, int nz)
{
    return GeoTiles{nx, ny, nz, (nx + kGeoTX - 1) / kGeoTX, (ny + kGeoTY - 1) / kGeoTY, (nz + kGeoTZ - 1) / kGeoTZ};
}

int64_t geo_tile_count(const GeoTiles &G) { return (int64_t)G.tx * G.ty * G.tz; }

unsigned geo_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

// the header (two list counts, padded to 16 words), then one flag word and one list word per tile, back to back
GeoLayout geodesic_layout(int nx, int ny, int nz)
{
    GeoLayout L;
    Carve c;
    L.tiles = geo_tile_count(geo_tiles(nx, ny, nz));
    L.header = c.take(4 * kGeoHeaderWords, 4);
    L.flags = c.take(4 * L.tiles, 4);
    L.list = c.take(4 * L.tiles, 4);
    L.total = c.at;
    return L;
}

hipError_t launch_geodesic_init(const uint8_t *free, int nx, int ny, int nz, const int32_t *seeds, int64_t n_seeds, int32_t *out_cost, void *workspace,
                                hipStream_t s)
{
    const GeoTiles G = geo_tiles(nx, ny, nz);
    const GeoLayout L = geodesic_layout(nx, ny, nz);
    const int64_t n = (int64_t)nx * ny * nz, tiles = L.tiles;
    uint32_t *header = static_cast<uint32_t *>(ws_at(workspace, L.header));
    uint32_t *flags = static_cast<uint32_t *>(ws_at(workspace, L.flags));
    uint32_t *list = static_cast<uint32_t *>(ws_at(workspace, L.list));
    hipLaunchKernelGGL(geo_init_kernel, dim3(geo_blocks(std::max<int64_t>(std::max(n, tiles), kGeoHeaderWords))), dim3(kBlock), 0, s, out_cost, header, flags, n,
                       tiles);
    if (n_seeds > 0) hipLaunchKernelGGL(geo_seed_kernel, dim3(geo_blocks(n_seeds)), dim3(kBlock), 0, s, free, seeds, n_seeds, out_cost, flags, G, n);
    hipLaunchKernelGGL(geo_compact_kernel, dim3(geo_blocks(tiles)), dim3(kBlock), 0, s, flags, list, header, (const uint32_t *)nullptr, tiles);
    return hipGetLastError();
}

hipError_t launch_geodesic_relax(const uint8_t *free, const int32_t *penalty, int nx, int ny, int nz, int connectivity, const int32_t *w, int32_t max_cost,
                                 int rounds, int32_t *cost, int32_t *out_pending, void *workspace, hipStream_t s)
{
    GeoRelax P;
    P.free = free;
    P.penalty = penalty;
    P.cost = cost;
    P.G = geo_tiles(nx, ny, nz);
    const GeoLayout L = geodesic_layout(nx, ny, nz);
    const int64_t tiles = L.tiles;
    uint32_t *header = static_cast<uint32_t *>(ws_at(workspace, L.header));
    P.flags = static_cast<uint32_t *>(ws_at(workspace, L.flags));
    uint32_t *list = static_cast<uint32_t *>(ws_at(workspace, L.list));
    P.list = list;
    P.w1 = (uint32_t)w[0];
    P.w2 = (uint32_t)w[1];
    P.w3 = (uint32_t)w[2];
    P.max_cost = (uint32_t)max_cost;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, kGeoMaxGrid)), block(kBlock);
    for (int r = 0; r < rounds; ++r) {
        P.count = header + (r & 1);
        P.count_next = header + ((r + 1) & 1);
        if (connectivity == 6)
            hipLaunchKernelGGL(geo_tile_kernel<6>, grid, block, 0, s, P);
        else if (connectivity == 18)
            hipLaunchKernelGGL(geo_tile_kernel<18>, grid, block, 0, s, P);
        else
            hipLaunchKernelGGL(geo_tile_kernel<26>, grid, block, 0, s, P);
        hipLaunchKernelGGL(geo_compact_kernel, dim3(geo_blocks(tiles)), block, 0, s, P.flags, list, P.count_next, P.count, tiles);
    }
    hipLaunchKernelGGL(geo_pending_kernel, dim3(1), dim3(1), 0, s, header, rounds & 1, out_pending);
    return hipGetLastError();
}

hipError_t launch_geodesic_finish(const uint8_t *free, const int32_t *penalty, int nx, int ny, int nz, int connectivity, const int32_t *w, float step,
                                  const int32_t *cost, int32_t *out_next, float *out_dist, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz;
    const float scale = step / (float)w[0];
    const dim3 grid(geo_blocks(n)), block(kBlock);
    const uint32_t w1 = (uint32_t)w[0], w2 = (uint32_t)w[1], w3 = (uint32_t)w[2];
    if (connectivity == 6)
        hipLaunchKernelGGL(geo_finish_kernel<6>, grid, block, 0, s, free, penalty, cost, out_next, out_dist, nx, ny, nz, w1, w2, w3, scale, n);
    else if (connectivity == 18)
        hipLaunchKernelGGL(geo_finish_kernel<18>, grid, block, 0, s, free, penalty, cost, out_next, out_dist, nx, ny, nz, w1, w2, w3, scale, n);
    else
        hipLaunchKernelGGL(geo_finish_kernel<26>, grid, block, 0, s, free, penalty, cost, out_next, out_dist, nx, ny, nz, w1, w2, w3, scale, n);
    return hipGetLastError();
}

hipError_t launch_volume_follow(const int32_t *next, int64_t n_voxels, const int32_t *starts, int64_t n, int max_steps, int32_t *out_voxels, int32_t *out_length,
                                uint8_t *out_reached, hipStream_t s)
{
    hipLaunchKernelGGL(geo_follow_kernel, dim3(geo_blocks(n)), dim3(kBlock), 0, s, next, n_voxels, starts, n, max_steps, out_voxels, out_length, out_reached);
    return hipGetLastError();
}

}  // namespace d3f
