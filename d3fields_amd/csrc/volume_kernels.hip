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
#include "volume_rows.h"      // locate, sample_row, face_weights, add_derivative, backward_row (shared with band_kernels.hip)

namespace d3f {

namespace {

// the eight corner rows of the cell at voxel `base` of a DENSE set: one row per voxel
struct DenseRows {
    const VolSet &S;
    int32_t base;
    int64_t sx, sy;
    template <class T>      // float, or _Float16 for a half set: the stride counts elements
    __device__ __forceinline__ void operator()(const T *(&row)[8]) const
    {
#pragma unroll
        for (int c = 0; c < 8; ++c) row[c] = reinterpret_cast<const T *>(S.data) + ((int64_t)base + corner_offset(c, sx, sy)) * S.stride;
    }
};

template <bool F16>
__device__ __forceinline__ void sample_row(const VolSet &S, int64_t i, int32_t base, const float (&w)[8], int64_t sx, int64_t sy, int first, int lanes)
{
    sample_row<F16>(S, i, base >= 0, w, first, lanes, DenseRows{S, base, sx, sy});
}

// F16: some set of the launch is stored as half (volume_rows.h); the <.., false> instances are the float32-only code
template <bool WIDE, bool F16>
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
            if (P.sets[s].C <= kVolNarrowMax) sample_row<F16>(P.sets[s], i, me.base, w, sx, sy, 0, 1);
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
                if (P.sets[s].C > kVolNarrowMax) sample_row<F16>(P.sets[s], wave_first + src, base, w, sx, sy, sub, 16);
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// the point is valid and S.grad is not null
template <bool F16>
__device__ __forceinline__ void backward_row(const VolSet &S, int64_t i, int32_t base, const FaceWeights &f, int64_t sx, int64_t sy, int first, int lanes,
                                             float (&acc)[3])
{
    backward_row<F16>(S, i, f, first, lanes, acc, DenseRows{S, base, sx, sy});
}

template <bool WIDE, bool F16>
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
                if (P.sets[s].C <= kVolNarrowMax && P.sets[s].grad) backward_row<F16>(P.sets[s], i, me.base, f, sx, sy, 0, 1, acc);
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
                    if (P.sets[s].C > kVolNarrowMax && P.sets[s].grad) backward_row<F16>(P.sets[s], wave_first + src, base, f, sx, sy, sub, 16, part);
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

bool any_f16(const VolParams &P, bool backward)
{
    for (int s = 0; s < P.n_sets; ++s)
        if (P.sets[s].f16 && (!backward || P.sets[s].grad)) return true;
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
    const bool wide = any_wide(P, false), f16 = any_f16(P, false);
    auto kernel = wide ? (f16 ? volume_sample_kernel<true, true> : volume_sample_kernel<true, false>)
                       : (f16 ? volume_sample_kernel<false, true> : volume_sample_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

hipError_t launch_volume_backward(const VolParams &P, hipStream_t s)
{
    const int64_t blocks = (P.n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool wide = any_wide(P, true), f16 = any_f16(P, true);
    auto kernel = wide ? (f16 ? volume_backward_kernel<true, true> : volume_backward_kernel<true, false>)
                       : (f16 ? volume_backward_kernel<false, true> : volume_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return hipGetLastError();
}

}  // namespace d3f
