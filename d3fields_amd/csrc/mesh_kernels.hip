// mesh_kernels.hip -- iso-surface extraction (marching cubes) of a float32 volume [nx, ny, nz] (z fastest) and a separable
// Gaussian filter of such a volume.  Volume, vertices and triangles stay on the device; the output is deterministic.
//
// Extraction.  A vertex sits on a grid edge (lower endpoint p, axis a) whose endpoints straddle iso under inside = value < iso,
// when at least one of the (up to four) cells round the edge emits; a cell emits when its eight corners are finite and, with a
// valid array, valid.  key = 3 * flat(p) + a, t = (iso - va) / (vb - va) in fp32 with the IEEE division; vertices leave in
// ascending key order, triangles by cell (= flat index of the cell's lowest corner), inside a cell in the order of mc_table.h.
//
// One lane per lattice point, flat index along the lanes (so the eight corner rows a wave reads are eight runs of 64
// consecutive floats), 1024 consecutive points per workgroup in four rounds of 256.  The lane owns the three edges leaving its
// point and the cell whose lowest corner the point is.
//   count     forms the case, counts the lane's vertices and triangles, reduces them over the workgroup and writes TWO words
//             per workgroup -- nothing per cell is ever written;
//   scan      scan_kernels.hip, over the workgroup totals (one more element at the end receives the grand total);
//   vertices  recomputes and writes key / t at workgroup offset + rank inside the workgroup: ascending by construction;
//   triangles recomputes the case and turns each triangle corner's edge key into its vertex index by a binary search over the
//             key array -- only over the span of the workgroup that owns the key's point (the scanned vertex offsets bound it), a
//             handful of steps.  No dense edge -> vertex map, no staged 64-bit keys.
// The 256 x 15-byte triangle table sits in LDS: it is indexed by the lane's own case, so scalar (constant) loads cannot serve it.
#include "d3f_internal.h"
#define D3F_MC_TABLE_ATTR static __device__ const
#include "mc_table.h"

namespace d3f {

namespace {

constexpr int kMeshRounds = 4;
constexpr int kMeshPerBlock = kBlock * kMeshRounds;      // 1024 points per workgroup

struct MeshParams {
    const float *vol;
    const uint8_t *valid;      // nullptr: every point is valid
    int32_t nx, ny, nz;
    int64_t n;                 // points
    int64_t sx, sy;            // strides of x and y in elements (z: 1)
    float iso;
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool point_good(const MeshParams &P, int64_t q, float v) { return finite_f(v) && (!P.valid || P.valid[q] != 0); }

// all eight corners of the cell with lowest corner (cx, cy, cz) are good; the cell must exist
__device__ bool cell_good(const MeshParams &P, int cx, int cy, int cz)
{
    const int64_t base = ((int64_t)cx * P.ny + cy) * P.nz + cz;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t q = base + (c & 1) * P.sx + ((c >> 1) & 1) * P.sy + ((c >> 2) & 1);
        ok = ok && point_good(P, q, P.vol[q]);
    }
    return ok;
}

// does any existing cell round the edge (point (ix, iy, iz), axis a) emit?  (rare path: the lane's own cell did not decide it)
__device__ bool edge_has_cell(const MeshParams &P, int ix, int iy, int iz, int a)
{
    for (int k = 0; k < 4; ++k) {
        const int d1 = k & 1, d2 = k >> 1;
        int cx = ix, cy = iy, cz = iz;
        if (a == 0) { cy -= d1; cz -= d2; } else if (a == 1) { cx -= d1; cz -= d2; } else { cx -= d1; cy -= d2; }
        if (cx < 0 || cy < 0 || cz < 0 || cx > P.nx - 2 || cy > P.ny - 2 || cz > P.nz - 2) continue;
        if (cell_good(P, cx, cy, cz)) return true;
    }
    return false;
}

struct PointEval {
    float va;          // value at the point
    float vb[3];       // value at the upper endpoint of the edge along x / y / z (read only where the edge exists)
    uint32_t vmask;    // bit a: the edge along axis a carries a vertex
    uint32_t mc_case;  // 8-bit case of the lane's cell, 0 when the cell does not exist or does not emit
};

// the lane's three edges and its cell from the same eight corner reads (the vertex pass needs the cell too: an emitting cell
// settles its three edges without a look at the neighbours)
__device__ __forceinline__ PointEval eval_point(const MeshParams &P, int64_t i, int ix, int iy, int iz)
{
    PointEval r;
    const bool hx = ix + 1 < P.nx, hy = iy + 1 < P.ny, hz = iz + 1 < P.nz;
    float v[8];
    bool g[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool there = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
        const int64_t q = i + (c & 1) * P.sx + ((c >> 1) & 1) * P.sy + ((c >> 2) & 1);
        v[c] = there ? P.vol[q] : 0.0f;
        g[c] = there && point_good(P, q, v[c]);
    }
    const bool cell = g[0] && g[1] && g[2] && g[3] && g[4] && g[5] && g[6] && g[7];      // implies hx && hy && hz
    uint32_t mc = 0;
    if (cell) {
#pragma unroll
        for (int c = 0; c < 8; ++c) mc |= (v[c] < P.iso ? 1u : 0u) << c;
        if (mc == 255u) mc = 0u;
    }
    r.mc_case = mc;
    r.va = v[0];
    r.vb[0] = v[1];
    r.vb[1] = v[2];
    r.vb[2] = v[4];
    const bool in0 = v[0] < P.iso;
    uint32_t straddle = 0;
    if (g[0]) {
        if (g[1] && (v[1] < P.iso) != in0) straddle |= 1u;
        if (g[2] && (v[2] < P.iso) != in0) straddle |= 2u;
        if (g[4] && (v[4] < P.iso) != in0) straddle |= 4u;
    }
    uint32_t vmask = straddle;
    if (straddle && !cell) {          // rare: a straddling edge next to a cell that does not emit (or the volume's upper faces)
        vmask = 0;
        for (int a = 0; a < 3; ++a)
            if (((straddle >> a) & 1u) && edge_has_cell(P, ix, iy, iz, a)) vmask |= 1u << a;
    }
    r.vmask = vmask;
    return r;
}

__device__ __forceinline__ void split_index(const MeshParams &P, int64_t i, int &ix, int &iy, int &iz)
{
    const uint32_t u = (uint32_t)i, nz = (uint32_t)P.nz, ny = (uint32_t)P.ny;
    const uint32_t xy = u / nz;
    iz = (int)(u - xy * nz);
    ix = (int)(xy / ny);
    iy = (int)(xy - (uint32_t)ix * ny);
}

// exclusive rank of `mine` over the 256 lanes of the workgroup (+ the workgroup's total); wave_tot: kBlock / 64 words of LDS
__device__ __forceinline__ uint32_t block_rank(uint32_t mine, uint32_t *wave_tot, uint32_t &total)
{
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if ((threadIdx.x & 63) >= off) incl += up;
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                   // the previous round's readers are done with wave_tot
    if ((threadIdx.x & 63) == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) before += wave_tot[w];
        total += wave_tot[w];
    }
    return before;
}

__global__ __launch_bounds__(kBlock) void mesh_count_kernel(MeshParams P, uint32_t *__restrict__ vsum, uint32_t *__restrict__ tsum,
                                                           int64_t nblocks)
{
    __shared__ uint8_t tri_count[256];
    __shared__ uint32_t wave_tot[2 * (kBlock / 64)];
    tri_count[threadIdx.x] = kMcTriCount[threadIdx.x];
    __syncthreads();
    uint32_t nv = 0, nt = 0;
    for (int r = 0; r < kMeshRounds; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMeshPerBlock + r * kBlock + threadIdx.x;
        if (i < P.n) {
            int ix, iy, iz;
            split_index(P, i, ix, iy, iz);
            const PointEval e = eval_point(P, i, ix, iy, iz);
            nv += __popc(e.vmask);
            nt += tri_count[e.mc_case];
        }
    }
    // sixteen bits each: at most 3 * 4 vertices and 5 * 4 triangles per lane, 3072 / 5120 per workgroup
    uint32_t both = nv | (nt << 16);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) both += __shfl_xor(both, off, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = both;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += wave_tot[w];
        vsum[blockIdx.x] = s & 0xffffu;
        tsum[blockIdx.x] = s >> 16;
        if (blockIdx.x == 0) {          // the element past the last workgroup: the exclusive scan leaves the grand total there
            vsum[nblocks] = 0u;
            tsum[nblocks] = 0u;
        }
    }
}

__global__ void mesh_totals_kernel(const uint32_t *__restrict__ voff, const uint32_t *__restrict__ toff, int64_t nblocks,
                                   int64_t *__restrict__ counts)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = (int64_t)voff[nblocks];
        counts[1] = (int64_t)toff[nblocks];
    }
}

__device__ __forceinline__ float edge_t(float iso, float va, float vb)
{
    float t = (iso - va) / (vb - va);
    if (!(t >= 0.0f && t <= 1.0f)) {          // a difference overflowed (|values| near FLT_MAX): the same quotient of quarters
        t = (iso * 0.25f - va * 0.25f) / (vb * 0.25f - va * 0.25f);
        t = t >= 0.0f ? (t <= 1.0f ? t : 1.0f) : 0.0f;
    }
    return t + 0.0f;                          // -0 (va == iso, vb < iso) -> +0
}

__global__ __launch_bounds__(kBlock) void mesh_vertices_kernel(MeshParams P, const uint32_t *__restrict__ voff, int64_t capacity,
                                                              int64_t *__restrict__ keys, float *__restrict__ ts)
{
    __shared__ uint32_t wave_tot[kBlock / 64];
    uint32_t base = voff[blockIdx.x];
    if (voff[blockIdx.x + 1] == base) return;          // the count pass found no vertex in this workgroup's points
    for (int r = 0; r < kMeshRounds; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMeshPerBlock + r * kBlock + threadIdx.x;
        PointEval e;
        e.vmask = 0;
        if (i < P.n) {
            int ix, iy, iz;
            split_index(P, i, ix, iy, iz);
            e = eval_point(P, i, ix, iy, iz);
        }
        uint32_t total;
        uint32_t at = base + block_rank(__popc(e.vmask), wave_tot, total);
        base += total;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if ((e.vmask >> a) & 1u) {
                if ((int64_t)at < capacity) {
                    keys[at] = 3 * i + a;
                    ts[at] = edge_t(P.iso, e.va, e.vb[a]);
                }
                ++at;
            }
    }
}

// index of `key` in keys[lo, hi): it is there by construction
__device__ __forceinline__ int32_t find_key(const int64_t *__restrict__ keys, uint32_t lo, uint32_t hi, int64_t key)
{
    while (lo + 1 < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= key) lo = mid; else hi = mid;
    }
    return (int32_t)lo;
}

__global__ __launch_bounds__(kBlock) void mesh_triangles_kernel(MeshParams P, const uint32_t *__restrict__ voff,
                                                               const uint32_t *__restrict__ toff, int64_t nblocks,
                                                               int64_t vertex_capacity, int64_t capacity,
                                                               const int64_t *__restrict__ keys, int32_t *__restrict__ tris)
{
    __shared__ uint8_t tri_count[256];
    __shared__ uint8_t tri_edges[256][3 * D3F_MC_MAX_TRIANGLES + 1];
    __shared__ uint32_t wave_tot[kBlock / 64];
    if ((int64_t)voff[nblocks] > vertex_capacity) return;      // the key array is incomplete: the caller re-runs with the true counts
    if (toff[blockIdx.x + 1] == toff[blockIdx.x]) return;      // the count pass found no triangle in this workgroup's cells
    tri_count[threadIdx.x] = kMcTriCount[threadIdx.x];
    for (int k = 0; k < 3 * D3F_MC_MAX_TRIANGLES; ++k) tri_edges[threadIdx.x][k] = kMcTriEdges[threadIdx.x][k];
    __syncthreads();
    uint32_t base = toff[blockIdx.x];
    for (int r = 0; r < kMeshRounds; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMeshPerBlock + r * kBlock + threadIdx.x;
        uint32_t mc = 0;
        if (i < P.n) {
            int ix, iy, iz;
            split_index(P, i, ix, iy, iz);
            mc = eval_point(P, i, ix, iy, iz).mc_case;
        }
        const uint32_t mine = tri_count[mc];
        uint32_t total;
        const uint32_t at = base + block_rank(mine, wave_tot, total);
        base += total;
        for (uint32_t k = 0; k < mine; ++k) {
            if ((int64_t)(at + k) >= capacity) break;
            int32_t idx[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t e = tri_edges[mc][3 * k + c];
                const uint32_t a = e >> 2, j = e & 3u;
                // offsets of the edge's lower endpoint along the other two axes, ascending: (j & 1, j >> 1)
                const int64_t su = a == 0 ? P.sy : P.sx, sw = a == 2 ? P.sy : 1;
                const int64_t q = i + (j & 1u) * su + (j >> 1) * sw;
                const int64_t b = q / kMeshPerBlock;
                idx[c] = find_key(keys, voff[b], voff[b + 1], 3 * q + (int64_t)a);
            }
            int32_t *o = tris + 3 * (int64_t)(at + k);
            o[0] = idx[0];
            o[1] = idx[1];
            o[2] = idx[2];
        }
    }
}

MeshParams mesh_params(const float *vol, const uint8_t *valid, int nx, int ny, int nz, float iso)
{
    MeshParams P;
    P.vol = vol;
    P.valid = valid;
    P.nx = nx;
    P.ny = ny;
    P.nz = nz;
    P.n = (int64_t)nx * ny * nz;
    P.sx = (int64_t)ny * nz;
    P.sy = nz;
    P.iso = iso;
    return P;
}

}  // namespace

int64_t mesh_blocks(int64_t n) { return (n + kMeshPerBlock - 1) / kMeshPerBlock; }

// two arrays of (workgroups + 1) words (vertex and triangle totals, scanned in place) + the scan's own scratch
MeshLayout mesh_layout(int64_t n)
{
    MeshLayout L;
    Carve c;
    L.blocks = mesh_blocks(n);
    L.voff = c.take((L.blocks + 1) * 4);
    L.toff = c.take((L.blocks + 1) * 4);
    L.scan = c.take(scan_scratch_bytes(L.blocks + 1));
    L.total = c.at;
    return L;
}

// counts_out: 2 x int64 on the device (vertices, triangles).  keys == nullptr: count only.
hipError_t launch_mesh(const float *vol, const uint8_t *valid, int nx, int ny, int nz, float iso, int64_t vertex_capacity,
                       int64_t triangle_capacity, int64_t *keys, float *ts, int32_t *tris, int64_t *counts_out, void *workspace,
                       bool extract, hipStream_t s)
{
    const MeshParams P = mesh_params(vol, valid, nx, ny, nz, iso);
    const MeshLayout L = mesh_layout(P.n);
    const int64_t nb = L.blocks;
    uint32_t *voff = static_cast<uint32_t *>(ws_at(workspace, L.voff));
    uint32_t *toff = static_cast<uint32_t *>(ws_at(workspace, L.toff));
    void *scratch = ws_at(workspace, L.scan);
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, P, voff, toff, nb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan_u32(voff, voff, nb + 1, scratch, s);
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan_u32(toff, toff, nb + 1, scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mesh_totals_kernel, dim3(1), dim3(64), 0, s, voff, toff, nb, counts_out);
    if (extract) {
        hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, P, voff, vertex_capacity, keys, ts);
        hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, P, voff, toff, nb, vertex_capacity,
                           triangle_capacity, keys, tris);
    }
    return hipGetLastError();
}

// ---- separable Gaussian filter -----------------------------------------------------------------------------------------------
// scipy.ndimage.gaussian_filter(mode='reflect'): weights exp(-k^2 / 2 sigma^2) normalised to sum 1 (computed on the host in
// double, rounded to fp32), radius int(truncate * sigma + 0.5), boundary (d c b a | a b c d | d c b a); axes in scipy's order
// x, y, z.  A pass sees the volume as [outer][len][inner] and filters along len: x = [1][nx][ny*nz], y = [nx][ny][nz] -- both
// stage a tile of (32 + 2 r) rows x 64 consecutive inner elements in LDS, so every global read and write is a run of 64
// floats -- and z = [nx*ny][nz][1], where the taps of a lane are neighbours in its own row and come from the cache.
// Accumulation: centre first, then pairs outwards, acc = fmaf(w_k, below + above, acc).

namespace {

constexpr int kGaussRows = 32;      // output rows of an LDS tile

struct GaussWeights {
    float w[kGaussMaxRadius + 1];
    int32_t radius;
};

__device__ __forceinline__ int reflect_index(int j, int len)
{
    const int period = 2 * len;
    j %= period;
    if (j < 0) j += period;
    return j < len ? j : period - 1 - j;
}

__global__ __launch_bounds__(kBlock) void gauss_strided_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t outer,
                                                              int len, int64_t inner, GaussWeights W, int row_tiles,
                                                              int64_t inner_tiles)
{
    extern __shared__ float tile[];      // [kGaussRows + 2 r][64]
    const int r = W.radius;
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    int64_t b = blockIdx.x;
    const int64_t it = b % inner_tiles;
    b /= inner_tiles;
    const int rt = (int)(b % row_tiles);
    const int64_t o = b / row_tiles;
    const int64_t col = it * 64 + lane;
    const bool live = col < inner;
    const int row0 = rt * kGaussRows;
    const float *s = src + o * len * inner + col;
    for (int a = group; a < kGaussRows + 2 * r; a += kBlock / 64) {
        const int j = reflect_index(row0 - r + a, len);
        tile[a * 64 + lane] = live ? s[(int64_t)j * inner] : 0.0f;
    }
    __syncthreads();
    float *d = dst + o * len * inner + col;
    for (int l = group; l < kGaussRows; l += kBlock / 64) {
        if (row0 + l >= len || !live) continue;
        const float *c = tile + (l + r) * 64 + lane;
        float acc = W.w[0] * c[0];
        for (int k = 1; k <= r; ++k) acc = fmaf(W.w[k], c[-k * 64] + c[k * 64], acc);
        d[(int64_t)(row0 + l) * inner] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void gauss_contiguous_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n, int len,
                                                                 GaussWeights W)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int r = W.radius;
    const uint32_t row = (uint32_t)i / (uint32_t)len;
    const int z = (int)((uint32_t)i - row * (uint32_t)len);
    const float *s = src + (int64_t)row * len;
    float acc = W.w[0] * s[z];
    if (z - r >= 0 && z + r < len) {
        for (int k = 1; k <= r; ++k) acc = fmaf(W.w[k], s[z - k] + s[z + k], acc);
    } else {
        for (int k = 1; k <= r; ++k) acc = fmaf(W.w[k], s[reflect_index(z - k, len)] + s[reflect_index(z + k, len)], acc);
    }
    dst[i] = acc;
}

hipError_t gauss_strided(const float *src, float *dst, int64_t outer, int len, int64_t inner, const GaussWeights &W, hipStream_t s)
{
    const int row_tiles = (len + kGaussRows - 1) / kGaussRows;
    const int64_t inner_tiles = (inner + 63) / 64;
    const int64_t blocks = outer * row_tiles * inner_tiles;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = (size_t)(kGaussRows + 2 * W.radius) * 64 * sizeof(float);
    hipLaunchKernelGGL(gauss_strided_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, s, src, dst, outer, len, inner, W, row_tiles,
                       inner_tiles);
    return hipGetLastError();
}

}  // namespace

// weights[0 .. radius]: the normalised half kernel (host array); tmp: one volume of floats; src != dst
hipError_t launch_volume_gaussian(const float *src, float *dst, int nx, int ny, int nz, const float *weights, int radius, float *tmp,
                                  hipStream_t s)
{
    GaussWeights W;
    for (int k = 0; k <= kGaussMaxRadius; ++k) W.w[k] = k <= radius ? weights[k] : 0.0f;
    W.radius = radius;
    const int64_t n = (int64_t)nx * ny * nz;
    hipError_t e = gauss_strided(src, dst, 1, nx, (int64_t)ny * nz, W, s);      // along x
    if (e != hipSuccess) return e;
    e = gauss_strided(dst, tmp, nx, ny, nz, W, s);                             // along y
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gauss_contiguous_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tmp, dst, n, nz, W);
    return hipGetLastError();
}

}  // namespace d3f
