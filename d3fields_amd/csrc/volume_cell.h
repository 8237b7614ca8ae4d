// volume_cell.h -- the trilinear chain of a baked volume's cell (DESIGN.md sections 13 and 14), shared by the lookups
// (volume_kernels.hip) and the ray march (raycast_kernels.hip): ONE definition, so a marched sample and a looked-up point round alike.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace d3f {

__device__ __forceinline__ void corner_weights(float tx, float ty, float tz, float (&w)[8])
{
    const float ax[2] = {1.0f - tx, tx}, ay[2] = {1.0f - ty, ty}, az[2] = {1.0f - tz, tz};
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = ax[c >> 2] * ay[(c >> 1) & 1] * az[c & 1];
}

// voxel offset of corner c = dx*4 + dy*2 + dz from the cell's base
__device__ __forceinline__ int64_t corner_offset(int c, int64_t sx, int64_t sy) { return (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1); }

__device__ __forceinline__ float blend(const float (&w)[8], const float (&v)[8])
{
    float acc = w[0] * v[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) acc = fmaf(w[c], v[c], acc);
    return acc;
}

}  // namespace d3f
