// edt_kernels.hip -- the exact Euclidean distance transform of a site volume (include/d3fields_hip.h, ABI 14).
// For every voxel v: the squared integer distance to the nearest site and the flat index of one such site.
//
// Separable, z then y then x; every pass carries the winning SITE, never a distance -- the distance of the next pass is formed again
// from the site's coordinates, so the two intermediate volumes are small:
//   z pass   A[v] int16: z of the nearest site in v's own z line (-1: none within the cap).  64 lanes hold 64 consecutive z, ONE ballot
//            of the site bytes gives the line as a word, clz / ctz of the masked word the nearest site below and above: no loop over
//            the line.  Lines of at most 32 voxels share a wave (64 / W lines of W = 2^k >= nz lanes); a line longer than 64 keeps
//            its words in LDS and a lane walks words only while they are empty.
//   y pass   B[v] int32: (sy << 14) | sz of the nearest site in v's own yz plane (-1: none), from f[j] = (z - A[x,j,z])^2
//   x pass   the outputs, from f[j] = (y - sy_j)^2 + (z - sz_j)^2 of B[j,y,z]
// y and x pass are ONE kernel (edt_line_kernel): a workgroup takes T = 64 or 32 neighbouring lines (consecutive z, the memory's
// fastest index, so a row of the tile is one coalesced 256- or 128-byte access) and keeps f of the whole lines in LDS, lane index
// fastest: entry j of lane l at word j * T + l, consecutive lanes on consecutive banks.  The threads of the workgroup are T lanes
// x blockDim / T segments; segment s computes the outputs i = s, s + segments, ...  Per output the DIRECT minimum over j, walked
// outwards from i (j = i, i -+ 1, i -+ 2, ...) and stopped at the first d with d^2 >= best: f >= 0, so no farther j can win.  That
// is exact, needs no division, and the lanes of a wave (same i, neighbouring z) stop within a few steps of one another.  The cap is
// the same rule with best starting at cap + 1.  Only f lives in LDS (4 n bytes per lane); the winner's site is read again from the
// pass's input.  Lines too long for 160 KiB (n > 1280) run the same loop on global memory (LDS = false).
// Every voxel is written by one lane from a fixed candidate order (lower j first at equal d): no atomics, two runs agree bit for bit.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr uint32_t kEdtNone = 0x7fffffffu;      // f of a line entry without a site; f + d^2 stays below 2^32 (d <= 16383)
constexpr int kEdtFar = 32768;                  // "no site on this side" of the z pass: above every |dz|
constexpr int kEdtMaxWords = 256;               // 16384 / 64

// the nearest set bit to position z given the nearest below-or-at (zb) and at-or-above (za), -1 for none; the lower one at a tie
__device__ __forceinline__ int16_t edt_pick(int z, int zb, int za, uint32_t best0)
{
    const int db = zb >= 0 ? z - zb : kEdtFar, da = za >= 0 ? za - z : kEdtFar;
    const int d = db <= da ? db : da;
    const int s = db <= da ? zb : za;
    return (d == kEdtFar || (uint32_t)(d * d) >= best0) ? (int16_t)-1 : (int16_t)s;
}

// nz <= 64: a wave holds 64 >> logw lines of w = 1 << logw lanes each
__global__ __launch_bounds__(kBlock) void edt_z_short_kernel(const uint8_t *__restrict__ site, int16_t *__restrict__ A, int nz, int logw, int64_t nlines,
                                                            uint32_t best0)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int w = 1 << logw, seg = lane >> logw, zl = lane & (w - 1);
    const int64_t line = wave * (64 >> logw) + seg;
    const bool active = line < nlines && zl < nz;
    const bool s = active && site[line * nz + zl] != 0;
    unsigned long long word = __ballot(s) >> (seg << logw);
    if (w < 64) word &= (1ull << w) - 1ull;
    if (!active) return;
    const unsigned long long below = word & ((2ull << zl) - 1ull), above = (word >> zl) << zl;
    const int zb = below ? 63 - __builtin_clzll(below) : -1, za = above ? __builtin_ctzll(above) : -1;
    A[line * nz + zl] = edt_pick(zl, zb, za, best0);
}

// nz > 64: one wave per line, the line's ballot words in LDS
__global__ __launch_bounds__(kBlock) void edt_z_long_kernel(const uint8_t *__restrict__ site, int16_t *__restrict__ A, int nz, int64_t nlines, uint32_t best0)
{
    __shared__ unsigned long long words[kBlock / 64][kEdtMaxWords];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t line = (int64_t)blockIdx.x * (kBlock / 64) + wv;
    const bool live = line < nlines;
    const int nwords = (nz + 63) >> 6;
    for (int c = 0; c < nwords; ++c) {
        const int z = c * 64 + lane;
        const bool s = live && z < nz && site[line * nz + z] != 0;
        const unsigned long long word = __ballot(s);
        if (lane == 0) words[wv][c] = word;
    }
    __syncthreads();
    if (!live) return;
    for (int c = 0; c < nwords; ++c) {
        const int z = c * 64 + lane;
        if (z >= nz) break;
        const unsigned long long own = words[wv][c];
        unsigned long long below = own & ((2ull << lane) - 1ull), above = (own >> lane) << lane;
        int kb = c, ka = c;
        while (!below && kb > 0) below = words[wv][--kb];
        while (!above && ka < nwords - 1) above = words[wv][++ka];
        const int zb = below ? kb * 64 + 63 - __builtin_clzll(below) : -1, za = above ? ka * 64 + __builtin_ctzll(above) : -1;
        A[line * nz + z] = edt_pick(z, zb, za, best0);
    }
}

struct EdtPass {
    const void *in;        // PASS 1: A int16; PASS 2: B int32
    int32_t *packed;       // PASS 1: B
    int32_t *d2, *nearest; // PASS 2 (each may be nullptr)
    float *dist;
    int n, ny, nz;         // n: the length of a line of this pass
    int64_t nlines, stride;
    uint32_t best0;        // min(cap + 1, kEdtNone): a candidate wins only below it
    int32_t cap;
    float step;
};

// f of entry j of the line at `base`: the squared distance, inside the dimensions already passed, from this line to that entry's site
template <int PASS>
__device__ __forceinline__ uint32_t edt_f(const EdtPass &P, int64_t at, int y, int z)
{
    if (PASS == 1) {
        const int s = static_cast<const int16_t *>(P.in)[at];
        const int dz = z - s;
        return s < 0 ? kEdtNone : (uint32_t)(dz * dz);
    }
    const int p = static_cast<const int32_t *>(P.in)[at];
    const int dy = y - (p >> 14), dz = z - (p & 16383);
    return p < 0 ? kEdtNone : (uint32_t)(dy * dy + dz * dz);
}

template <int PASS, int T, bool LDS>
__global__ __launch_bounds__(1024) void edt_line_kernel(const EdtPass P)
{
    extern __shared__ uint32_t edt_lds[];      // [n][T] (LDS only)
    const int lane = threadIdx.x % T, seg = threadIdx.x / T, nseg = blockDim.x / T;
    const int64_t L = (int64_t)blockIdx.x * T + lane;
    const bool active = L < P.nlines;
    const int n = P.n;
    // PASS 1: lines along y, L = x * nz + z; PASS 2: lines along x, L = y * nz + z (the flat index of the line's first voxel)
    const uint32_t q = (uint32_t)(active ? L : 0) / (uint32_t)P.nz;
    const int z = (int)((uint32_t)(active ? L : 0) - q * (uint32_t)P.nz);
    const int y = (int)q;                      // (PASS 2 only)
    const int64_t base = PASS == 1 ? (int64_t)q * P.ny * P.nz + z : L;
    const int64_t stride = P.stride;
    if (LDS) {
        for (int j = seg; j < n; j += nseg) edt_lds[j * T + lane] = active ? edt_f<PASS>(P, base + j * stride, y, z) : kEdtNone;
        __syncthreads();
    }
    if (!active) return;
    auto f = [&](int j) -> uint32_t { return LDS ? edt_lds[j * T + lane] : edt_f<PASS>(P, base + j * stride, y, z); };
    for (int i = seg; i < n; i += nseg) {
        uint32_t best = P.best0;
        int bj = -1;
        {
            const uint32_t c = f(i);
            if (c < best) { best = c; bj = i; }
        }
        const int reach = max(i, n - 1 - i);
        for (int d = 1; d <= reach && (uint32_t)(d * d) < best; ++d) {
            const uint32_t dd = (uint32_t)(d * d);
            if (i - d >= 0) {
                const uint32_t c = f(i - d) + dd;
                if (c < best) { best = c; bj = i - d; }
            }
            if (i + d < n) {
                const uint32_t c = f(i + d) + dd;
                if (c < best) { best = c; bj = i + d; }
            }
        }
        const int64_t at = base + i * stride;
        if (PASS == 1) {
            int32_t out = -1;
            if (bj >= 0) out = (bj << 14) | (int32_t)static_cast<const int16_t *>(P.in)[base + bj * stride];
            P.packed[at] = out;
        } else {
            const int32_t d2 = bj >= 0 ? (int32_t)best : P.cap;
            if (P.d2) P.d2[at] = d2;
            if (P.nearest) {
                int32_t out = -1;
                if (bj >= 0) {
                    const int p = static_cast<const int32_t *>(P.in)[base + bj * stride];
                    out = (bj * P.ny + (p >> 14)) * P.nz + (p & 16383);
                }
                P.nearest[at] = out;
            }
            if (P.dist) P.dist[at] = d2 == 0x7fffffff ? __builtin_inff() : sqrtf((float)d2) * P.step;
        }
    }
}

template <int PASS, int T, bool LDS>
hipError_t launch_line(const EdtPass &P, int threads, size_t lds, hipStream_t s)
{
    const int64_t blocks = (P.nlines + T - 1) / T;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(edt_line_kernel<PASS, T, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((edt_line_kernel<PASS, T, LDS>), dim3((unsigned)blocks), dim3(threads), lds, s, P);
    return hipGetLastError();
}

// n <= 256: 64 lines per workgroup within 64 KiB; n <= 512: 32 lines within 64 KiB; n <= 1280: 32 lines in up to 160 KiB (one workgroup of
// 1024 threads per CU); longer: global memory
template <int PASS>
hipError_t launch_pass(const EdtPass &P, hipStream_t s)
{
    if (P.n <= 256) return launch_line<PASS, 64, true>(P, 512, (size_t)P.n * 64 * 4, s);
    if (P.n <= 512) return launch_line<PASS, 32, true>(P, 512, (size_t)P.n * 32 * 4, s);
    if (P.n <= 1280) return launch_line<PASS, 32, true>(P, 1024, (size_t)P.n * 32 * 4, s);
    return launch_line<PASS, 64, false>(P, 512, 0, s);
}

}  // namespace

// B int32 [n] then A int16 [n], an even count of them
EdtLayout edt_layout(int64_t n)
{
    EdtLayout L;
    Carve c;
    L.B = c.take(4 * n, 4);
    L.A = c.take(2 * n, 4);
    L.total = c.at;
    return L;
}

hipError_t launch_volume_edt(const uint8_t *site, int nx, int ny, int nz, float step, int32_t cap, int32_t *out_d2, int32_t *out_nearest, float *out_dist,
                             void *workspace, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz;
    const EdtLayout L = edt_layout(n);
    int32_t *B = static_cast<int32_t *>(ws_at(workspace, L.B));
    int16_t *A = static_cast<int16_t *>(ws_at(workspace, L.A));
    const uint32_t best0 = cap == 0x7fffffff ? kEdtNone : (uint32_t)cap + 1u;
    const int64_t zlines = (int64_t)nx * ny;
    if (nz <= 64) {
        int logw = 0;
        while ((1 << logw) < nz) ++logw;
        const int64_t waves = (zlines + (64 >> logw) - 1) / (64 >> logw);
        hipLaunchKernelGGL(edt_z_short_kernel, dim3((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, s, site, A, nz, logw, zlines, best0);
    } else {
        hipLaunchKernelGGL(edt_z_long_kernel, dim3((unsigned)((zlines + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, s, site, A, nz, zlines, best0);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    EdtPass P = {};
    P.ny = ny;
    P.nz = nz;
    P.best0 = best0;
    P.cap = cap;
    P.step = step;
    P.in = A;
    P.packed = B;
    P.n = ny;
    P.nlines = (int64_t)nx * nz;
    P.stride = nz;
    e = launch_pass<1>(P, s);
    if (e != hipSuccess) return e;
    P.in = B;
    P.packed = nullptr;
    P.d2 = out_d2;
    P.nearest = out_nearest;
    P.dist = out_dist;
    P.n = nx;
    P.nlines = (int64_t)ny * nz;
    P.stride = (int64_t)ny * nz;
    return launch_pass<2>(P, s);
}

}  // namespace d3f
