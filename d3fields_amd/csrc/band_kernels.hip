// band_kernels.hip -- a baked field whose channel rows exist only near the surface (include/d3fields_hip.h, ABI 13; DESIGN.md
// section 15).  dist / valid / cell_valid stay dense; a set's rows are COMPACTED: one int32 slot per voxel names the row of a stored
// voxel (-1: none), rows are [M, C] in ascending flat voxel index.
//
// Marking (d3f_band_mark), all order-preserving, no atomics:
//   band_cell_kernel   cell_band[cell] = cell_valid[cell] && any of the eight corners has fabsf(dist) < band (strict; NaN is no seed;
//                      a valid cell has eight valid corners, so `valid` itself is not read, nor is dist of an invalid cell)
//   band_flag_kernel   stored[q] = OR of cell_band over the up to eight cells voxel q is a corner of (clipped at the faces), written as
//                      0 / 1 words INTO the slot volume, which
//   launch_exclusive_scan_u32 (recursive, caller scratch) turns in place into the rank of every voxel among the stored ones, and
//   band_slot_kernel   slot[q] = stored ? rank : -1 (the flag is formed again from the cell bytes -- eight byte loads, cheaper than
//                      a second word volume), voxels[rank] = q below the capacity, and the lane of the last voxel writes the count.
//
// Lookups (d3f_band_sample / d3f_band_sample_backward): the two phases of volume_kernels.hip with the SAME chain (volume_rows.h);
// only the eight row pointers differ: rows + slot[corner] * stride.  in_band = valid && cell_band[cell]; a point that is valid but
// not in the band gets dist (and the dist term of the gradient) and every set's fill row, and no slot or row is read for it.
// Phase B: a group of sixteen lanes gets `base` of an IN-BAND point (kNotValid for any other) and (tx, ty, tz) from the locating
// lane -- the four shuffles of the dense kernel -- and loads the point's eight slots itself: all sixteen lanes read the same eight
// words (DESIGN.md 15 says why they are not shuffled).
#include "d3f_internal.h"
#include "volume_rows.h"

namespace d3f {

namespace {

// ---- marking ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void band_cell_kernel(const float *__restrict__ dist, const uint8_t *__restrict__ cell_valid,
                                                          uint8_t *__restrict__ cell_band, int nx, int ny, int nz, int64_t ncells, float band)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // flat cell index along the lanes, as volume_cell_valid_kernel
    if (i >= ncells) return;
    uint8_t keep = 0;
    if (cell_valid[i] != 0) {
        const uint32_t u = (uint32_t)i, cz_n = (uint32_t)(nz - 1), cy_n = (uint32_t)(ny - 1);
        const uint32_t xy = u / cz_n;
        const uint32_t cz = u - xy * cz_n, cx = xy / cy_n;
        const uint32_t cy = xy - cx * cy_n;
        const int64_t sx = (int64_t)ny * nz, sy = nz;
        const int64_t base = ((int64_t)cx * ny + cy) * nz + cz;
#pragma unroll
        for (int c = 0; c < 8; ++c) keep |= fabsf(dist[base + corner_offset(c, sx, sy)]) < band ? 1 : 0;      // (NaN compares false)
    }
    cell_band[i] = keep;
}

// is voxel q a corner of a kept cell?
__device__ __forceinline__ uint32_t voxel_stored(const uint8_t *__restrict__ cell_band, int64_t q, int nx, int ny, int nz)
{
    const uint32_t u = (uint32_t)q, unz = (uint32_t)nz, uny = (uint32_t)ny;
    const uint32_t xy = u / unz;
    const int iz = (int)(u - xy * unz), ix = (int)(xy / uny);
    const int iy = (int)(xy - (uint32_t)ix * uny);
    uint32_t stored = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cx = ix - (c >> 2), cy = iy - ((c >> 1) & 1), cz = iz - (c & 1);      // the cell whose corner c this voxel is
        if (cx >= 0 && cx <= nx - 2 && cy >= 0 && cy <= ny - 2 && cz >= 0 && cz <= nz - 2)
            stored |= cell_band[((int64_t)cx * (ny - 1) + cy) * (nz - 1) + cz] != 0 ? 1u : 0u;
    }
    return stored;
}

__global__ __launch_bounds__(kBlock) void band_flag_kernel(const uint8_t *__restrict__ cell_band, uint32_t *__restrict__ flag, int nx, int ny, int nz,
                                                          int64_t n)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < n) flag[q] = voxel_stored(cell_band, q, nx, ny, nz);
}

// slot holds the exclusive scan of the flags on entry
__global__ __launch_bounds__(kBlock) void band_slot_kernel(const uint8_t *__restrict__ cell_band, int32_t *__restrict__ slot, int32_t *__restrict__ voxels,
                                                          int64_t capacity, int64_t *__restrict__ count, int nx, int ny, int nz, int64_t n)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const uint32_t rank = (uint32_t)slot[q];
    const uint32_t stored = voxel_stored(cell_band, q, nx, ny, nz);
    slot[q] = stored ? (int32_t)rank : -1;
    if (stored && (int64_t)rank < capacity) voxels[rank] = (int32_t)q;
    if (q == n - 1) *count = (int64_t)rank + stored;
}

// ---- lookups ------------------------------------------------------------------------------------------------------------------
// the eight corner rows of a cell in a COMPACTED set: one row per stored voxel, named by the voxel's slot
struct BandRows {
    const VolSet &S;
    const int32_t (&slot)[8];
    template <class T>      // float, or _Float16 for a half set: the stride counts elements
    __device__ __forceinline__ void operator()(const T *(&row)[8]) const
    {
#pragma unroll
        for (int c = 0; c < 8; ++c) row[c] = reinterpret_cast<const T *>(S.data) + (int64_t)slot[c] * S.stride;
    }
};

// base: the cell of an in-band point, so every corner has a slot >= 0
__device__ __forceinline__ void load_slots(const BandParams &B, int32_t base, int64_t sx, int64_t sy, int32_t (&slot)[8])
{
#pragma unroll
    for (int c = 0; c < 8; ++c) slot[c] = B.slot[(int64_t)base + corner_offset(c, sx, sy)];
}

__device__ __forceinline__ bool any_narrow(const VolParams &P, bool backward)
{
    bool any = false;
    for (int s = 0; s < P.n_sets; ++s) any |= P.sets[s].C <= kVolNarrowMax && (!backward || P.sets[s].grad);
    return any;
}

// F16: some set of the launch is stored as half (volume_rows.h); the <.., false> instances are the float32-only code
// (four workgroups per CU hold the float32 instances at 128 VGPRs; an instance with both row forms would spill there, so it asks for three)
template <bool WIDE, bool F16>
__global__ __launch_bounds__(kBlock, F16 ? 3 : 4) void band_sample_kernel(BandParams B)
{
    const VolParams &P = B.V;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    Cell me;
    me.base = kNoPoint;
    me.tx = me.ty = me.tz = 0.0f;
    int32_t band_base = kNoPoint;      // what phase B sees of a point: its base where in the band, kNotValid elsewhere
    if (i < P.n) {
        int64_t cell = 0;
        me = locate(P, i, cell);
        float w[8];
        corner_weights(me.tx, me.ty, me.tz, w);
        float d = 1e3f;
        bool in_band = false;
        if (me.base >= 0) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = P.dist[(int64_t)me.base + corner_offset(c, sx, sy)];
            d = blend(w, v);
            in_band = B.cell_band != nullptr && B.cell_band[cell] != 0;
        }
        P.out_dist[i] = d;
        P.out_valid[i] = me.base >= 0 ? 1 : 0;
        B.out_in_band[i] = in_band ? 1 : 0;
        band_base = in_band ? me.base : kNotValid;
        if (any_narrow(P, false)) {
            int32_t slot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (in_band) load_slots(B, me.base, sx, sy, slot);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C <= kVolNarrowMax) sample_row<F16>(P.sets[s], i, in_band, w, 0, 1, BandRows{P.sets[s], slot});
        }
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = i - lane;
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.n) break;                  // wave-uniform: no point left
            const int src = 4 * r + group;
            const int32_t base = __shfl(band_base, src, 64);
            const float tx = __shfl(me.tx, src, 64), ty = __shfl(me.ty, src, 64), tz = __shfl(me.tz, src, 64);
            if (base == kNoPoint) continue;
            float w[8];
            corner_weights(tx, ty, tz, w);
            int32_t slot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (base >= 0) load_slots(B, base, sx, sy, slot);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C > kVolNarrowMax) sample_row<F16>(P.sets[s], wave_first + src, base >= 0, w, sub, 16, BandRows{P.sets[s], slot});
        }
    }
}

template <bool WIDE, bool F16>
__global__ __launch_bounds__(kBlock) void band_backward_kernel(BandParams B)
{
    const VolParams &P = B.V;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    Cell me;
    me.base = kNoPoint;
    me.tx = me.ty = me.tz = 0.0f;
    int32_t band_base = kNoPoint;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (i < P.n) {
        int64_t cell = 0;
        me = locate(P, i, cell);
        band_base = kNotValid;
        if (me.base >= 0) {
            const FaceWeights f = face_weights(me.tx, me.ty, me.tz);
            if (P.grad_dist) {                                     // the dist term: every valid point, in the band or not
                float v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = P.dist[(int64_t)me.base + corner_offset(c, sx, sy)];
                add_derivative(f, v, P.grad_dist[i], acc);
            }
            if (B.cell_band != nullptr && B.cell_band[cell] != 0) {
                band_base = me.base;
                if (any_narrow(P, true)) {
                    int32_t slot[8];
                    load_slots(B, me.base, sx, sy, slot);
                    for (int s = 0; s < P.n_sets; ++s)
                        if (P.sets[s].C <= kVolNarrowMax && P.sets[s].grad) backward_row<F16>(P.sets[s], i, f, 0, 1, acc, BandRows{P.sets[s], slot});
                }
            }
        }
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = i - lane;
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.n) break;                  // wave-uniform: no point left
            const int src = 4 * r + group;
            const int32_t base = __shfl(band_base, src, 64);
            const float tx = __shfl(me.tx, src, 64), ty = __shfl(me.ty, src, 64), tz = __shfl(me.tz, src, 64);
            float part[3] = {0.0f, 0.0f, 0.0f};
            if (base >= 0) {
                const FaceWeights f = face_weights(tx, ty, tz);
                int32_t slot[8];
                load_slots(B, base, sx, sy, slot);
                for (int s = 0; s < P.n_sets; ++s)
                    if (P.sets[s].C > kVolNarrowMax && P.sets[s].grad)
                        backward_row<F16>(P.sets[s], wave_first + src, f, sub, 16, part, BandRows{P.sets[s], slot});
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

int64_t band_workspace_bytes(int64_t n) { return scan_scratch_bytes(n); }

hipError_t launch_band_mark(const float *dist, const uint8_t *cell_valid, int nx, int ny, int nz, float band, uint8_t *cell_band, int32_t *slot,
                            int32_t *voxels, int64_t capacity, int64_t *count, void *workspace, hipStream_t s)
{
    const int64_t n = (int64_t)nx * ny * nz, ncells = (int64_t)(nx - 1) * (ny - 1) * (nz - 1);
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(band_cell_kernel, dim3((unsigned)((ncells + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, dist, cell_valid, cell_band, nx, ny, nz,
                       ncells, band);
    hipLaunchKernelGGL(band_flag_kernel, dim3(blocks), dim3(kBlock), 0, s, cell_band, reinterpret_cast<uint32_t *>(slot), nx, ny, nz, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // in place, as the mesh extraction scans: each lane of the scan reads its own elements before it writes them and touches no other lane's
    e = launch_exclusive_scan_u32(reinterpret_cast<uint32_t *>(slot), reinterpret_cast<uint32_t *>(slot), n, workspace, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(band_slot_kernel, dim3(blocks), dim3(kBlock), 0, s, cell_band, slot, voxels, capacity, count, nx, ny, nz, n);
    return hipGetLastError();
}

hipError_t launch_band_sample(const BandParams &B, hipStream_t s)
{
    const int64_t blocks = (B.V.n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool wide = any_wide(B.V, false), f16 = any_f16(B.V, false);
    auto kernel = wide ? (f16 ? band_sample_kernel<true, true> : band_sample_kernel<true, false>)
                       : (f16 ? band_sample_kernel<false, true> : band_sample_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, B);
    return hipGetLastError();
}

hipError_t launch_band_backward(const BandParams &B, hipStream_t s)
{
    const int64_t blocks = (B.V.n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool wide = any_wide(B.V, true), f16 = any_f16(B.V, true);
    auto kernel = wide ? (f16 ? band_backward_kernel<true, true> : band_backward_kernel<true, false>)
                       : (f16 ? band_backward_kernel<false, true> : band_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, B);
    return hipGetLastError();
}

}  // namespace d3f
