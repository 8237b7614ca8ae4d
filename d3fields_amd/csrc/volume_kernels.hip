// volume_kernels.hip -- trilinear lookups in a BAKED field: the regular volume of a grid query (dist, valid, channel sets; flat
// index (ix*ny + iy)*nz + iz, z fastest) read back at arbitrary points, and the gradient of that lookup w.r.t. the point.
//
// The contract (include/d3fields_hip.h, ABI 11), all in fp32:
//   g = (p - origin) / h per axis;  inside = 0 <= g <= n - 1;  i = min(floor(g), n - 2), t = g - i;
//   valid = inside && cell[i] (one byte per CELL, the AND of its eight corners: volume_cell_valid_kernel, once per volume);
//   w(dx,dy,dz) = (dx ? tx : 1-tx) * (dy ? ty : 1-ty) * (dz ? tz : 1-tz);  out = w0 v0, then fma(w_c, v_c, out), c = dx*4 + dy*2 + dz;
//   not valid: dist 1e3, a set's fill row, NO corner read (an invalid voxel may hold NaN).
//
// Phase A, one lane per point (256 points per workgroup, 64 per wave): the three divisions, the cell byte, dist, and every set
// of up to kVolNarrowMax channels -- corner rows as 16-byte vectors where the set allows it.  That is the whole NARROW instance.
// Phase B (the WIDE instance only): the wave walks its 64 points four at a time; a group of sixteen lanes takes one point, gets
// its cell index and (tx, ty, tz) from the lane that located it (four __shfl) and forms the weights itself (fifteen VALU
// instructions, cheaper than eight more shuffles); lanes run along the channels, 16 lanes x 16 bytes = 64 channels per step, so
// a corner row is read as runs of 256 bytes.  The divisions are thus done once per point by ONE lane of the wave, not by sixteen.
// Rows that cannot move as vectors (C % 4 != 0, an unaligned stride) take the same walk with one float per lane.
//
// Backward: the same two phases.  d out / d t_x = sum over the four (dy,dz) of wy wz (v[1,dy,dz] - v[0,dy,dz]), likewise y and z;
// a lane sums grad * that over its channels, a group folds its sixteen partial sums (__shfl_xor), the lane that located the point
// adds them to its own (phase A) sums and writes the row: three plain stores per point, no atomics.
#include "d3f_internal.h"
#include "volume_cell.h"      // corner_weights, corner_offset, blend

namespace d3f {

namespace {

constexpr int kNotValid = -1;      // Cell::base of a point outside the volume or in a cell with an invalid corner
constexpr int kNoPoint = -2;       // ... of a lane past the last point

struct Cell {
    int32_t base;                  // flat index of the cell's corner (0,0,0), < nx*ny*nz <= 2^31 - 1
    float tx, ty, tz;
};

__device__ __forceinline__ Cell locate(const VolParams &P, int64_t i)
{
    const float *p = P.pts + 3 * i;
    const float gx = (p[0] - P.ox) / P.h, gy = (p[1] - P.oy) / P.h, gz = (p[2] - P.oz) / P.h;
    Cell c;
    c.base = kNotValid;
    c.tx = c.ty = c.tz = 0.0f;
    // (NaN fails every comparison)
    const bool inside = gx >= 0.0f && gx <= (float)(P.nx - 1) && gy >= 0.0f && gy <= (float)(P.ny - 1) && gz >= 0.0f && gz <= (float)(P.nz - 1);
    if (inside) {
        const int ix = min((int)floorf(gx), P.nx - 2), iy = min((int)floorf(gy), P.ny - 2), iz = min((int)floorf(gz), P.nz - 2);
        c.tx = gx - (float)ix;
        c.ty = gy - (float)iy;
        c.tz = gz - (float)iz;
        const int64_t cell = ((int64_t)ix * (P.ny - 1) + iy) * (P.nz - 1) + iz;
        if (P.cell[cell] != 0) c.base = (ix * P.ny + iy) * P.nz + iz;
    }
    return c;
}

__device__ __forceinline__ float4 blend4(const float (&w)[8], const float4 (&v)[8])
{
    float4 acc = make_float4(w[0] * v[0].x, w[0] * v[0].y, w[0] * v[0].z, w[0] * v[0].w);
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        acc.x = fmaf(w[c], v[c].x, acc.x);
        acc.y = fmaf(w[c], v[c].y, acc.y);
        acc.z = fmaf(w[c], v[c].z, acc.z);
        acc.w = fmaf(w[c], v[c].w, acc.w);
    }
    return acc;
}

__device__ __forceinline__ float fill_of(const VolSet &S, int ch) { return S.fill ? S.fill[ch] : 0.0f; }

// channels [first, C) in steps of `lanes` vectors / floats of the row of point i: lanes = 1 is phase A, 16 is phase B
__device__ __forceinline__ void sample_row(const VolSet &S, int64_t i, int32_t base, const float (&w)[8], int64_t sx, int64_t sy, int first, int lanes)
{
    float *o = S.out + i * S.C;
    if (base < 0) {
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes)
                *reinterpret_cast<float4 *>(o + k) = make_float4(fill_of(S, k), fill_of(S, k + 1), fill_of(S, k + 2), fill_of(S, k + 3));
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = fill_of(S, k);
        }
        return;
    }
    const float *row[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) row[c] = S.data + ((int64_t)base + corner_offset(c, sx, sy)) * S.stride;
    if (S.vec) {
        for (int k = 4 * first; k < S.C; k += 4 * lanes) {
            float4 v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(row[c] + k);
            *reinterpret_cast<float4 *>(o + k) = blend4(w, v);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = row[c][k];
            o[k] = blend(w, v);
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void volume_sample_kernel(VolParams P)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    Cell me;
    me.base = kNoPoint;
    me.tx = me.ty = me.tz = 0.0f;
    if (i < P.n) {
        me = locate(P, i);
        float w[8];
        corner_weights(me.tx, me.ty, me.tz, w);
        float d = 1e3f;
        if (me.base >= 0) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = P.dist[(int64_t)me.base + corner_offset(c, sx, sy)];
            d = blend(w, v);
        }
        P.out_dist[i] = d;
        P.out_valid[i] = me.base >= 0 ? 1 : 0;
        for (int s = 0; s < P.n_sets; ++s)
            if (P.sets[s].C <= kVolNarrowMax) sample_row(P.sets[s], i, me.base, w, sx, sy, 0, 1);
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = i - lane;
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.n) break;                  // wave-uniform: no point left
            const int src = 4 * r + group;
            const int32_t base = __shfl(me.base, src, 64);
            const float tx = __shfl(me.tx, src, 64), ty = __shfl(me.ty, src, 64), tz = __shfl(me.tz, src, 64);
            if (base == kNoPoint) continue;
            float w[8];
            corner_weights(tx, ty, tz, w);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C > kVolNarrowMax) sample_row(P.sets[s], wave_first + src, base, w, sx, sy, sub, 16);
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
struct FaceWeights {
    float yz[4], xz[4], xy[4];      // products of the two OTHER axes' weights, index = first * 2 + second
};

__device__ __forceinline__ FaceWeights face_weights(float tx, float ty, float tz)
{
    const float ax[2] = {1.0f - tx, tx}, ay[2] = {1.0f - ty, ty}, az[2] = {1.0f - tz, tz};
    FaceWeights f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f.yz[j] = ay[j >> 1] * az[j & 1];
        f.xz[j] = ax[j >> 1] * az[j & 1];
        f.xy[j] = ax[j >> 1] * ay[j & 1];
    }
    return f;
}

// acc += g * d blend / d (tx, ty, tz) for one channel with corner values v
__device__ __forceinline__ void add_derivative(const FaceWeights &f, const float (&v)[8], float g, float (&acc)[3])
{
    float dx = f.yz[0] * (v[4] - v[0]);
    dx = fmaf(f.yz[1], v[5] - v[1], dx);
    dx = fmaf(f.yz[2], v[6] - v[2], dx);
    dx = fmaf(f.yz[3], v[7] - v[3], dx);
    float dy = f.xz[0] * (v[2] - v[0]);
    dy = fmaf(f.xz[1], v[3] - v[1], dy);
    dy = fmaf(f.xz[2], v[6] - v[4], dy);
    dy = fmaf(f.xz[3], v[7] - v[5], dy);
    float dz = f.xy[0] * (v[1] - v[0]);
    dz = fmaf(f.xy[1], v[3] - v[2], dz);
    dz = fmaf(f.xy[2], v[5] - v[4], dz);
    dz = fmaf(f.xy[3], v[7] - v[6], dz);
    acc[0] = fmaf(g, dx, acc[0]);
    acc[1] = fmaf(g, dy, acc[1]);
    acc[2] = fmaf(g, dz, acc[2]);
}

// the point is valid and S.grad is not null
__device__ __forceinline__ void backward_row(const VolSet &S, int64_t i, int32_t base, const FaceWeights &f, int64_t sx, int64_t sy, int first, int lanes,
                                             float (&acc)[3])
{
    const float *g = S.grad + i * S.C;
    const float *row[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) row[c] = S.data + ((int64_t)base + corner_offset(c, sx, sy)) * S.stride;
    if (S.vec) {
        for (int k = 4 * first; k < S.C; k += 4 * lanes) {
            float4 v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(row[c] + k);
            const float4 gk = *reinterpret_cast<const float4 *>(g + k);
            const float a[8] = {v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x};
            const float b[8] = {v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y};
            const float c2[8] = {v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z};
            const float d[8] = {v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w};
            add_derivative(f, a, gk.x, acc);
            add_derivative(f, b, gk.y, acc);
            add_derivative(f, c2, gk.z, acc);
            add_derivative(f, d, gk.w, acc);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = row[c][k];
            add_derivative(f, v, g[k], acc);
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void volume_backward_kernel(VolParams P)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    Cell me;
    me.base = kNoPoint;
    me.tx = me.ty = me.tz = 0.0f;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (i < P.n) {
        me = locate(P, i);
        if (me.base >= 0) {
            const FaceWeights f = face_weights(me.tx, me.ty, me.tz);
            if (P.grad_dist) {
                float v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = P.dist[(int64_t)me.base + corner_offset(c, sx, sy)];
                add_derivative(f, v, P.grad_dist[i], acc);
            }
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C <= kVolNarrowMax && P.sets[s].grad) backward_row(P.sets[s], i, me.base, f, sx, sy, 0, 1, acc);
        }
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = i - lane;
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.n) break;                  // wave-uniform: no point left
            const int src = 4 * r + group;
            const int32_t base = __shfl(me.base, src, 64);
            const float tx = __shfl(me.tx, src, 64), ty = __shfl(me.ty, src, 64), tz = __shfl(me.tz, src, 64);
            float part[3] = {0.0f, 0.0f, 0.0f};
            if (base >= 0) {
                const FaceWeights f = face_weights(tx, ty, tz);
                for (int s = 0; s < P.n_sets; ++s)
                    if (P.sets[s].C > kVolNarrowMax && P.sets[s].grad) backward_row(P.sets[s], wave_first + src, base, f, sx, sy, sub, 16, part);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) part[a] += __shfl_xor(part[a], off, 64);      // every lane of the group holds the sum
                const float mine = __shfl(part[a], (lane & 3) * 16, 64);                            // group (lane & 3) worked on point 4 r + (lane & 3)
                if ((lane >> 2) == r) acc[a] += mine;
            }
        }
    }
    if (i < P.n) {
        float *o = P.grad_pts + 3 * i;
        o[0] = P.rh * acc[0];
        o[1] = P.rh * acc[1];
        o[2] = P.rh * acc[2];
    }
}

// ---- bake time: one byte per cell --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void volume_cell_valid_kernel(const uint8_t *__restrict__ valid, uint8_t *__restrict__ cell, int nx, int ny, int nz,
                                                                  int64_t ncells)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // flat cell index along the lanes: eight runs of consecutive bytes per wave
    if (i >= ncells) return;
    const uint32_t u = (uint32_t)i, cz_n = (uint32_t)(nz - 1), cy_n = (uint32_t)(ny - 1);
    const uint32_t xy = u / cz_n;
    const uint32_t cz = u - xy * cz_n, cx = xy / cy_n;
    const uint32_t cy = xy - cx * cy_n;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const int64_t base = ((int64_t)cx * ny + cy) * nz + cz;
    uint8_t ok = 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok &= valid[base + corner_offset(c, sx, sy)] != 0 ? 1 : 0;
    cell[i] = ok;
}

bool any_wide(const VolParams &P, bool backward)
{
    for (int s = 0; s < P.n_sets; ++s)
        if (P.sets[s].C > kVolNarrowMax && (!backward || P.sets[s].grad)) return true;
    return false;
}

}  // namespace

hipError_t launch_volume_cell_valid(const uint8_t *valid, uint8_t *cell, int nx, int ny, int nz, hipStream_t s)
{
    const int64_t ncells = (int64_t)(nx - 1) * (ny - 1) * (nz - 1);
    hipLaunchKernelGGL(volume_cell_valid_kernel, dim3((unsigned)((ncells + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, valid, cell, nx, ny, nz, ncells);
    return hipGetLastError();
}

hipError_t launch_volume_sample(const VolParams &P, hipStream_t s)
{
    const int64_t blocks = (P.n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (any_wide(P, false))
        hipLaunchKernelGGL(volume_sample_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    else
        hipLaunchKernelGGL(volume_sample_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_volume_backward(const VolParams &P, hipStream_t s)
{
    const int64_t blocks = (P.n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (any_wide(P, true))
        hipLaunchKernelGGL(volume_backward_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    else
        hipLaunchKernelGGL(volume_backward_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

}  // namespace d3f
