// warp_kernels.hip -- where is it now?  A baked field moved by the rigid motions of its parts (include/d3fields_hip.h, d3f_volume_warp_select and
// d3f_volume_warp_rows).
//
// The contract (restated in tests/warp_cases.py).  Coordinates are voxel index units, the flat index is (x*ny + y)*nz + z.  owner: int32
// [nx, ny, nz]; pose: float64 [K, 15] as d3f_part_motion writes it (R row-major, src, dst; q = R (p - src) + dst).  Part k (1..K) MOVES iff the 15
// entries of its row are finite; a voxel is moving when its owner is a moving part; every other voxel is background and stays where it is.
// Inverse map of destination voxel q under part k, float64, one rounding per operation, nothing fused (the build has -ffp-contract=off and this
// file names no fused operation):
//   u = q - dst;  p_i = ((R_0i*u_0 + R_1i*u_1) + R_2i*u_2) + src_i;  inside: 0 <= p_a <= n_a - 1 on the three axes (NaN is not inside);
//   i_a = min(floor(p_a), n_a - 2);  t_a = float32(p_a - i_a);  the nearest corner is i_a + (t_a > 0.5f).
// Candidate k exists when p is inside, cell_valid[i] is set, the nearest corner's owner is exactly k and the interpolated distance is not NaN.
// Interpolation: the weights of corner_weights (volume_cell.h), acc = w0*v0, then acc = acc + w_c*v_c for c = 1..7, every product and sum rounded
// to float32.  Candidate 0, the background: the voxel itself with dist[q] when valid[q], q is not moving and dist[q] is not NaN.
// Winner: candidates in the order 0, 1, ..., K; a later one replaces the best only if its distance is strictly smaller.
//
//   warp_box_init_kernel    the 12 words of every part's two boxes: lo = INT32_MAX, hi = INT32_MIN
//   warp_owner_box_kernel   one lane per voxel: the inclusive box of every part's owner == k voxels (integer atomic min / max)
//   warp_select_kernel      one workgroup per tile of 4 x 8 x 8 destination voxels, one lane per voxel, z along the lanes.  Culling, 64 parts per wave
//                           step: a lane inverse-maps the eight corners of the tile's box under its part, and the part survives when the bounding box of
//                           the eight images, grown by one voxel, meets the part's owner box.  The map is affine, so the image of every voxel of the tile
//                           lies in that bounding box, and a candidate's nearest corner -- an owner == k voxel -- within half a voxel of the image:
//                           a culled part has no candidate in the tile, whatever R is.  One ballot per step; the survivors' indices go to LDS in
//                           ascending order, so the walk below takes the candidates in the contract's order.  Each lane then walks the survivors.
//   warp_rows_kernel        the rows of listed destination voxels: the two phases of volume_kernels.hip -- one lane per voxel for the sets of up to
//                           16 channels, sixteen lanes per voxel along the channels for the wider ones -- with the chain above instead of the fused one.
//                           A background voxel is a row copy; a moved one recomputes p, i, t by the same expressions and blends eight corner rows.
// No float atomic, no spinning, nothing waits for another workgroup; integer atomic min / max for the boxes only, so the bytes do not depend on
// the order in which anything lands.  Every output is written completely; the caller's buffers may hold anything.
#include "d3f_internal.h"
#include "volume_cell.h"      // corner_weights, corner_offset

namespace d3f {

namespace {

constexpr int kPoseRow = D3F_MOTION_POSE_DOUBLES;
constexpr int kTileX = 4, kTileY = 8, kTileZ = 8;
constexpr int kWords = D3F_WARP_MAX_PARTS / 64;
static_assert(kPoseRow == 15 && kTileX * kTileY * kTileZ == kBlock && kWords * 64 == D3F_WARP_MAX_PARTS && D3F_WARP_MAX_PARTS <= 65536,
              "R, src, dst; one lane per voxel of a tile; whole ballot words; survivor indices fit 16 bits");

constexpr int32_t kBoxEmptyLo = 0x7fffffff, kBoxEmptyHi = -0x7fffffff - 1;

struct Pose {
    double R[9], src[3], dst[3];
};

// part k (0-based row); true iff it moves
__device__ __forceinline__ bool load_pose(const double *__restrict__ pose, int k, Pose &P)
{
    const double inf = __builtin_huge_val();
    const double *r = pose + (int64_t)k * kPoseRow;
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        P.R[a] = r[a];
        finite = finite && fabs(P.R[a]) < inf;      // a NaN compares false
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        P.src[a] = r[9 + a];
        P.dst[a] = r[12 + a];
        finite = finite && fabs(P.src[a]) < inf && fabs(P.dst[a]) < inf;
    }
    return finite;
}

__device__ __forceinline__ void inverse_map(const Pose &P, double qx, double qy, double qz, double (&p)[3])
{
    const double u0 = qx - P.dst[0], u1 = qy - P.dst[1], u2 = qz - P.dst[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = ((P.R[i] * u0 + P.R[3 + i] * u1) + P.R[6 + i] * u2) + P.src[i];
}

struct Where {
    int ix, iy, iz;
    float tx, ty, tz;
};

// the cell and the fractions of an image point; false: not inside
__device__ __forceinline__ bool locate_image(const double (&p)[3], int nx, int ny, int nz, Where &w)
{
    const bool inside = p[0] >= 0.0 && p[0] <= (double)(nx - 1) && p[1] >= 0.0 && p[1] <= (double)(ny - 1) && p[2] >= 0.0 && p[2] <= (double)(nz - 1);
    if (!inside) return false;
    w.ix = min((int)floor(p[0]), nx - 2);
    w.iy = min((int)floor(p[1]), ny - 2);
    w.iz = min((int)floor(p[2]), nz - 2);
    w.tx = (float)(p[0] - (double)w.ix);
    w.ty = (float)(p[1] - (double)w.iy);
    w.tz = (float)(p[2] - (double)w.iz);
    return true;
}

// the chain of the contract: two roundings per corner
__device__ __forceinline__ float blend_plain(const float (&w)[8], const float (&v)[8])
{
    float acc = w[0] * v[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) acc = acc + w[c] * v[c];
    return acc;
}

__device__ __forceinline__ float4 blend_plain4(const float (&w)[8], const float4 (&v)[8])
{
    float4 acc = make_float4(w[0] * v[0].x, w[0] * v[0].y, w[0] * v[0].z, w[0] * v[0].w);
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        acc.x = acc.x + w[c] * v[c].x;
        acc.y = acc.y + w[c] * v[c].y;
        acc.z = acc.z + w[c] * v[c].z;
        acc.w = acc.w + w[c] * v[c].w;
    }
    return acc;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// One word of a box takes in v.  The word only ever falls (rises), so a relaxed read that is not below (above) v already proves the min (max)
// would change nothing, and a stale read costs one needless operation at worst.  Thousands of min / max operations on one address serialise:
// unfiltered they are the whole cost of the box pass (measured: DESIGN.md 28.1).
__device__ __forceinline__ void box_min(int32_t *box, int v)
{
    if (v < __hip_atomic_load(box, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(box, v);
}

__device__ __forceinline__ void box_max(int32_t *box, int v)
{
    if (v > __hip_atomic_load(box, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(box, v);
}

// box (lo[3], hi[3]) of part k (1-based; 0: this lane adds nothing) takes in voxel (x, y, z).  Every lane of the wave calls this together.  Where the
// lanes that add all name one part -- the common case: parts are large against 64 voxels -- the wave folds first and one lane does the six words.
__device__ __forceinline__ void box_add(int32_t *boxes, int which, int k, int x, int y, int z)
{
    const bool adds = k > 0;
    const unsigned long long any = __ballot(adds);
    if (any == 0) return;
    const int kf = __shfl(k, __ffsll((long long)any) - 1, 64);
    int32_t *box = boxes + ((int64_t)(adds ? k : kf) - 1) * 12 + which;
    if (__ballot(adds && k != kf) == 0) {
        const int lx = wave_min(adds ? x : kBoxEmptyLo), ly = wave_min(adds ? y : kBoxEmptyLo), lz = wave_min(adds ? z : kBoxEmptyLo);
        const int hx = wave_max(adds ? x : kBoxEmptyHi), hy = wave_max(adds ? y : kBoxEmptyHi), hz = wave_max(adds ? z : kBoxEmptyHi);
        if ((threadIdx.x & 63) == 0) {
            box_min(box + 0, lx);
            box_min(box + 1, ly);
            box_min(box + 2, lz);
            box_max(box + 3, hx);
            box_max(box + 4, hy);
            box_max(box + 5, hz);
        }
    } else if (adds) {
        box_min(box + 0, x);
        box_min(box + 1, y);
        box_min(box + 2, z);
        box_max(box + 3, x);
        box_max(box + 4, y);
        box_max(box + 5, z);
    }
}

__global__ __launch_bounds__(kBlock) void warp_box_init_kernel(int32_t *__restrict__ boxes, int K)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < K * 12) boxes[i] = (i % 6) < 3 ? kBoxEmptyLo : kBoxEmptyHi;
}

__global__ __launch_bounds__(kBlock) void warp_owner_box_kernel(const int32_t *__restrict__ owner, int32_t *__restrict__ boxes, int K, int ny, int nz, int64_t n)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int k = 0, x = 0, y = 0, z = 0;
    if (q < n) {
        k = owner[q];
        if (k < 1 || k > K) k = 0;
        const uint32_t u = (uint32_t)q, xy = u / (uint32_t)nz;
        z = (int)(u - xy * (uint32_t)nz);
        x = (int)(xy / (uint32_t)ny);
        y = (int)(xy - (uint32_t)x * (uint32_t)ny);
    }
    box_add(boxes, 0, k, x, y, z);
}

struct WarpSelect {
    const float *dist;
    const uint8_t *valid, *cell;
    const int32_t *owner;
    const double *pose;
    int32_t *out_source;
    float *out_dist;
    uint8_t *out_valid;
    int32_t *boxes;
    int32_t nx, ny, nz, K;
    int32_t tiles_y, tiles_z;
};

__global__ __launch_bounds__(kBlock) void warp_select_kernel(const WarpSelect P)
{
    __shared__ unsigned long long s_moving[kWords], s_survive[kWords];
    __shared__ int s_first[kWords + 1];
    __shared__ uint16_t s_list[D3F_WARP_MAX_PARTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nx = P.nx, ny = P.ny, nz = P.nz, K = P.K;
    const uint32_t b = blockIdx.x;
    const uint32_t bxy = b / (uint32_t)P.tiles_z;
    const int x0 = (int)(bxy / (uint32_t)P.tiles_y) * kTileX, y0 = (int)(bxy % (uint32_t)P.tiles_y) * kTileY, z0 = (int)(b - bxy * (uint32_t)P.tiles_z) * kTileZ;
    const int words = (K + 63) >> 6;

    // ---- which parts move, and which of them can reach this tile: 64 parts per wave step ----
    {
        const double cx[2] = {(double)x0, (double)min(x0 + kTileX - 1, nx - 1)}, cy[2] = {(double)y0, (double)min(y0 + kTileY - 1, ny - 1)},
                     cz[2] = {(double)z0, (double)min(z0 + kTileZ - 1, nz - 1)};
        for (int s = wave; s < words; s += kBlock / 64) {
            const int j = s * 64 + lane;
            bool moving = false, survive = false;
            if (j < K) {
                Pose R;
                moving = load_pose(P.pose, j, R);
                if (moving) {
                    const double big = __builtin_huge_val();
                    double lo[3] = {big, big, big}, hi[3] = {-big, -big, -big};
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        double p[3];
                        inverse_map(R, cx[c >> 2], cy[(c >> 1) & 1], cz[c & 1], p);
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            lo[a] = p[a] < lo[a] ? p[a] : lo[a];
                            hi[a] = p[a] > hi[a] ? p[a] : hi[a];
                        }
                    }
                    const int32_t *box = P.boxes + (int64_t)j * 12;
                    survive = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) survive = survive && lo[a] - 1.0 <= (double)box[3 + a] && hi[a] + 1.0 >= (double)box[a];      // (NaN: culled)
                }
            }
            const unsigned long long mv = __ballot(moving), sv = __ballot(survive);
            if (lane == 0) {
                s_moving[s] = mv;
                s_survive[s] = sv;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {                                           // exclusive prefix of the survivors per word: kWords == 64 == one wave
        int c = lane < words ? __popcll(s_survive[lane]) : 0;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        s_first[lane] = incl - c;
        if (lane == 63) s_first[kWords] = incl;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += kBlock) {
        const unsigned long long word = s_survive[j >> 6], bit = 1ull << (j & 63);
        if (word & bit) s_list[s_first[j >> 6] + __popcll(word & (bit - 1))] = (uint16_t)j;
    }
    __syncthreads();
    const int survivors = s_first[kWords];

    // ---- one lane per destination voxel ----
    const int x = x0 + (threadIdx.x >> 6), y = y0 + ((threadIdx.x >> 3) & 7), z = z0 + (threadIdx.x & 7);
    const bool in = x < nx && y < ny && z < nz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const int64_t q = ((int64_t)x * ny + y) * nz + z;
    int best = -1;
    float best_d = 1e3f;
    if (in) {
        const int o = P.owner[q];
        const bool q_moving = o >= 1 && o <= K && ((s_moving[(o - 1) >> 6] >> ((o - 1) & 63)) & 1ull) != 0;
        if (P.valid[q] != 0 && !q_moving) {
            const float d = P.dist[q];
            if (d == d) {
                best = 0;
                best_d = d;
            }
        }
    }
    for (int s = 0; s < survivors; ++s) {
        const int k = __builtin_amdgcn_readfirstlane((int)s_list[s]);      // the same in every lane: the pose comes through scalar loads
        Pose R;
        load_pose(P.pose, k, R);
        if (!in) continue;
        double p[3];
        inverse_map(R, (double)x, (double)y, (double)z, p);
        Where w;
        if (!locate_image(p, nx, ny, nz, w)) continue;
        if (P.cell[((int64_t)w.ix * (ny - 1) + w.iy) * (nz - 1) + w.iz] == 0) continue;
        const int nearx = w.ix + (w.tx > 0.5f ? 1 : 0), neary = w.iy + (w.ty > 0.5f ? 1 : 0), nearz = w.iz + (w.tz > 0.5f ? 1 : 0);
        if (P.owner[((int64_t)nearx * ny + neary) * nz + nearz] != k + 1) continue;
        const int64_t base = ((int64_t)w.ix * ny + w.iy) * nz + w.iz;
        float wt[8], v[8];
        corner_weights(w.tx, w.ty, w.tz, wt);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = P.dist[base + corner_offset(c, sx, sy)];
        const float d = blend_plain(wt, v);
        if (d == d && (best < 0 || d < best_d)) {
            best = k + 1;
            best_d = d;
        }
    }
    if (in) {
        P.out_source[q] = best;
        P.out_dist[q] = best_d;
        P.out_valid[q] = best >= 0 ? 1 : 0;
    }
    if (K > 0) box_add(P.boxes, 6, in && best > 0 ? best : 0, x, y, z);
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------
constexpr int kNoVoxel = -2, kFill = -1, kCopy = 0, kBlend = 1;      // what a listed voxel's rows are

struct WarpRows {
    const int32_t *source;
    const double *pose;
    const int32_t *voxels;     // or nullptr: every voxel in flat order
    const int32_t *slot;       // a banded source: the row of a stored voxel, -1 elsewhere; nullptr with no stored voxel at all (nothing of the band is read)
    const uint8_t *cell_band;
    uint8_t *out_known;
    int64_t m, n;
    int32_t nx, ny, nz, K;
    int32_t n_sets, banded;
    VolSet sets[D3F_MAX_MAPS];
};

// channels [first, C) in steps of `lanes` vectors / floats of row `o`
__device__ __forceinline__ void warp_row(const VolSet &S, float *__restrict__ o, int kind, const int64_t (&row)[8], const float (&w)[8], int first, int lanes)
{
    if (kind == kFill) {
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes)
                *reinterpret_cast<float4 *>(o + k) = S.fill ? make_float4(S.fill[k], S.fill[k + 1], S.fill[k + 2], S.fill[k + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = S.fill ? S.fill[k] : 0.0f;
        }
    } else if (kind == kCopy) {
        const float *r = S.data + row[0] * S.stride;
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes) *reinterpret_cast<float4 *>(o + k) = *reinterpret_cast<const float4 *>(r + k);
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = r[k];
        }
    } else {
        const float *r[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) r[c] = S.data + row[c] * S.stride;
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes) {
                float4 v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(r[c] + k);
                *reinterpret_cast<float4 *>(o + k) = blend_plain4(w, v);
            }
        } else {
            for (int k = first; k < S.C; k += lanes) {
                float v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = r[c][k];
                o[k] = blend_plain(w, v);
            }
        }
    }
}

// the row indices of a voxel of kind kCopy (row[0]; at: the voxel's own row) or kBlend (at: the cell's corner (0,0,0); in a band every corner has a slot)
__device__ __forceinline__ void row_indices(const WarpRows &P, int kind, int64_t at, int64_t sx, int64_t sy, int64_t (&row)[8])
{
#pragma unroll
    for (int c = 0; c < 8; ++c) row[c] = 0;
    if (kind == kCopy) {
        row[0] = at;
    } else if (kind == kBlend) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t v = at + corner_offset(c, sx, sy);
            row[c] = P.banded ? (int64_t)P.slot[v] : v;
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void warp_rows_kernel(const WarpRows P)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    int kind = kNoVoxel;
    int64_t at = 0;
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;
    if (j < P.m) {
        kind = kFill;
        const int64_t q = P.voxels ? (int64_t)P.voxels[j] : j;
        const int src = q >= 0 && q < P.n ? P.source[q] : -1;
        if (src == 0) {
            at = !P.banded ? q : P.slot ? (int64_t)P.slot[q] : -1;
            if (at >= 0) kind = kCopy;
        } else if (src >= 1 && src <= P.K) {
            const uint32_t u = (uint32_t)q, xy = u / (uint32_t)P.nz;
            const int z = (int)(u - xy * (uint32_t)P.nz), x = (int)(xy / (uint32_t)P.ny);
            const int y = (int)(xy - (uint32_t)x * (uint32_t)P.ny);
            Pose R;
            load_pose(P.pose, src - 1, R);
            double p[3];
            inverse_map(R, (double)x, (double)y, (double)z, p);
            Where w;
            if (locate_image(p, P.nx, P.ny, P.nz, w) && (!P.banded || (P.cell_band && P.cell_band[((int64_t)w.ix * (P.ny - 1) + w.iy) * (P.nz - 1) + w.iz] != 0))) {
                kind = kBlend;
                at = ((int64_t)w.ix * P.ny + w.iy) * P.nz + w.iz;
                tx = w.tx;
                ty = w.ty;
                tz = w.tz;
            }
        }
        P.out_known[j] = kind != kFill ? 1 : 0;
        bool narrow = false;
        for (int s = 0; s < P.n_sets; ++s) narrow = narrow || P.sets[s].C <= kVolNarrowMax;
        if (narrow) {
            float w[8];
            int64_t row[8];
            corner_weights(tx, ty, tz, w);
            row_indices(P, kind, at, sx, sy, row);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C <= kVolNarrowMax) warp_row(P.sets[s], P.sets[s].out + j * P.sets[s].C, kind, row, w, 0, 1);
        }
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = j - lane;
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.m) break;                  // wave-uniform: no voxel left
            const int from = 4 * r + group;
            const int kind_g = __shfl(kind, from, 64);
            const int at_lo = __shfl((int)(uint32_t)(at & 0xffffffffLL), from, 64), at_hi = __shfl((int)(at >> 32), from, 64);
            const float gx = __shfl(tx, from, 64), gy = __shfl(ty, from, 64), gz = __shfl(tz, from, 64);
            if (kind_g == kNoVoxel) continue;
            const int64_t at_g = ((int64_t)at_hi << 32) | (int64_t)(uint32_t)at_lo;
            float w[8];
            int64_t row[8];
            corner_weights(gx, gy, gz, w);
            row_indices(P, kind_g, at_g, sx, sy, row);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C > kVolNarrowMax) warp_row(P.sets[s], P.sets[s].out + (wave_first + from) * P.sets[s].C, kind_g, row, w, sub, 16);
        }
    }
}

}  // namespace

hipError_t launch_warp_select(const WarpSelectArgs &A, hipStream_t s)
{
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    if (A.K > 0) {
        hipLaunchKernelGGL(warp_box_init_kernel, dim3((unsigned)((A.K * 12 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, A.out_boxes, A.K);
        hipLaunchKernelGGL(warp_owner_box_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, A.owner, A.out_boxes, A.K, A.ny, A.nz, n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    WarpSelect P;
    P.dist = A.dist;
    P.valid = A.valid;
    P.cell = A.cell_valid;
    P.owner = A.owner;
    P.pose = A.pose;
    P.out_source = A.out_source;
    P.out_dist = A.out_dist;
    P.out_valid = A.out_valid;
    P.boxes = A.out_boxes;
    P.nx = A.nx; P.ny = A.ny; P.nz = A.nz; P.K = A.K;
    const int64_t tiles_x = (A.nx + kTileX - 1) / kTileX;
    P.tiles_y = (A.ny + kTileY - 1) / kTileY;
    P.tiles_z = (A.nz + kTileZ - 1) / kTileZ;
    const int64_t tiles = tiles_x * P.tiles_y * P.tiles_z;      // a tile holds at least 4 x 2 x 2 voxels (every extent >= 2): below 2^28
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_select_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_warp_rows(const WarpRowsArgs &A, hipStream_t s)
{
    WarpRows P;
    P.source = A.source;
    P.pose = A.pose;
    P.voxels = A.voxels;
    P.slot = A.slot;
    P.cell_band = A.cell_band;
    P.out_known = A.out_known;
    P.m = A.m;
    P.n = (int64_t)A.nx * A.ny * A.nz;
    P.nx = A.nx; P.ny = A.ny; P.nz = A.nz; P.K = A.K;
    P.n_sets = A.n_sets;
    P.banded = A.banded ? 1 : 0;
    bool wide = false;
    for (int i = 0; i < A.n_sets; ++i) {
        P.sets[i] = A.sets[i];
        wide = wide || A.sets[i].C > kVolNarrowMax;
    }
    const int64_t blocks = (A.m + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (wide)
        hipLaunchKernelGGL(warp_rows_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    else
        hipLaunchKernelGGL(warp_rows_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

}  // namespace d3f
