// raycast_kernels.hip -- the first surface a ray meets in a BAKED field: a fixed-step march through the truncated signed distance
// volume with one linear interpolation at the sign change (the KinectFusion ray cast).
//
// The contract (include/d3fields_hip.h, ABI 12), all in fp32, per ray p(t) = o + t d:
//   go = (o - origin) / h, gd = d / h;  clip [t0, t1] = the box [0, n-1]^3 in lattice units and [t_near, t_far];
//   dt = march / |d|, K = floor((t1 - t0) / dt), t_k = fma(k, dt, t0) (never accumulated), g_k = clamp(fma(t_k, gd, go), 0, n-1);
//   cell / weights / validity as the lookup (volume_cell.h): the cell byte first, the eight dist corners only where it is set;
//   prev > 0 and s_k <= 0: hit at t* = fma(dt, prev / (prev - s_k), t_{k-1}); an invalid sample empties prev; - to + is no hit.
//
// One lane per ray.  Rays come from the caller's arrays in caller order, or from a pinhole camera: a wave then takes an 8 x 8
// pixel tile, so that its 64 rays walk neighbouring cells and share cache lines.  Everything per launch (extents, strides, K, R,
// the camera centre) is a kernel argument and lives in SGPRs.  The loop is the lane's own; the wave leaves it when its last lane has
// finished (the exec mask runs empty), lanes that hit early idle until then.  No atomics, no LDS, no scratch; every output row is written
// by one lane, so two runs agree bit for bit.
#include "d3f_internal.h"
#include "volume_cell.h"

namespace d3f {

namespace {

__device__ __forceinline__ bool finite(float x) { return fabsf(x) < INFINITY; }      // false for NaN

// one axis of the clip; false: the ray runs beside the slab
__device__ __forceinline__ bool clip_axis(float go, float gd, float nm1, float &lo, float &hi)
{
    if (gd != 0.0f) {
        const float ta = (0.0f - go) / gd, tb = (nm1 - go) / gd;
        lo = fmaxf(lo, fminf(ta, tb));
        hi = fminf(hi, fmaxf(ta, tb));
        return true;
    }
    return go >= 0.0f && go <= nm1;
}

template <bool CAMERA>
__global__ __launch_bounds__(kBlock) void volume_raycast_kernel(RayParams P)
{
    int64_t ray;
    float o[3], d[3];
    if (CAMERA) {
        const int lane = threadIdx.x & 63;
        const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // = the 8 x 8 tile
        const int tiles_x = (P.W + 7) >> 3;
        const int ty = (int)(wave / tiles_x), tx = (int)(wave - (int64_t)ty * tiles_x);
        const int u = tx * 8 + (lane & 7), v = ty * 8 + (lane >> 3);
        if (u >= P.W || v >= P.H) return;
        ray = (int64_t)v * P.W + u;
        const float dcx = ((float)u - P.cx) / P.fx, dcy = ((float)v - P.cy) / P.fy;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                   // d = R^T (dcx, dcy, 1)
            d[a] = fmaf(P.R[3 + a], dcy, P.R[a] * dcx) + P.R[6 + a];
            o[a] = P.co[a];
        }
    } else {
        ray = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (ray >= P.n) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[a] = P.origins[3 * ray + a];
            d[a] = P.dirs[3 * ray + a];
        }
    }
    const float gox = (o[0] - P.ox) / P.h, goy = (o[1] - P.oy) / P.h, goz = (o[2] - P.oz) / P.h;
    const float gdx = d[0] / P.h, gdy = d[1] / P.h, gdz = d[2] / P.h;
    const float fx1 = (float)(P.nx - 1), fy1 = (float)(P.ny - 1), fz1 = (float)(P.nz - 1);
    const float len = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
    bool live = finite(gox) && finite(goy) && finite(goz) && finite(gdx) && finite(gdy) && finite(gdz) && len > 0.0f && finite(len);
    float lo = -INFINITY, hi = INFINITY, t0 = 0.0f, dt = 0.0f;
    int K = -1;
    if (live) {                                          // (no NaN below: finite numerators, finite non-zero divisors)
        live = clip_axis(gox, gdx, fx1, lo, hi) & clip_axis(goy, gdy, fy1, lo, hi) & clip_axis(goz, gdz, fz1, lo, hi);
        t0 = fmaxf(lo, P.t_near);
        const float t1 = fminf(hi, P.t_far);
        dt = P.march / len;
        const float Kf = floorf((t1 - t0) / dt);
        live = live && t0 <= t1 && Kf <= kRayMaxSamples;      // (Kf is NaN or inf where dt or t1 - t0 overflowed)
        if (live) K = (int)Kf;
    }
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    const int cy_n = P.ny - 1, cz_n = P.nz - 1;
    float prev = 0.0f;                                   // <= 0 is as good as empty: only prev > 0 can open a hit
    float t_hit = 0.0f;
    bool hit = false;
    int k = 0;
    for (; k <= K; ++k) {
        const float tk = fmaf((float)k, dt, t0);
        // the clamp is what keeps every index below inside the volume, whatever the ray
        const float gx = fminf(fmaxf(fmaf(tk, gdx, gox), 0.0f), fx1), gy = fminf(fmaxf(fmaf(tk, gdy, goy), 0.0f), fy1),
                    gz = fminf(fmaxf(fmaf(tk, gdz, goz), 0.0f), fz1);
        const int ix = min((int)floorf(gx), P.nx - 2), iy = min((int)floorf(gy), P.ny - 2), iz = min((int)floorf(gz), P.nz - 2);
        if (P.cell[((int64_t)ix * cy_n + iy) * cz_n + iz] == 0) {
            prev = 0.0f;                                 // a hole is never bridged
            continue;
        }
        const int64_t base = ((int64_t)ix * P.ny + iy) * P.nz + iz;
        float w[8], v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = P.dist[base + corner_offset(c, sx, sy)];
        corner_weights(gx - (float)ix, gy - (float)iy, gz - (float)iz, w);
        const float s = blend(w, v);
        if (prev > 0.0f && s <= 0.0f) {
            hit = true;
            t_hit = fmaf(dt, prev / (prev - s), fmaf((float)(k - 1), dt, t0));
            ++k;                                         // this sample counts
            break;
        }
        prev = s;
    }
    P.out_t[ray] = t_hit;
    P.out_hit[ray] = hit ? 1 : 0;
    float *p = P.out_pts + 3 * ray;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = hit ? fmaf(t_hit, d[a], o[a]) : __builtin_nanf("");
    if (P.out_samples) P.out_samples[ray] = k;           // samples taken: K + 1 for a miss that crossed the box, 0 for one that did not
}

}  // namespace

hipError_t launch_volume_raycast(const RayParams &P, bool camera, hipStream_t s)
{
    if (camera) {
        const int64_t tiles = (int64_t)((P.W + 7) / 8) * ((P.H + 7) / 8);      // one wave each
        const int64_t blocks = (tiles + kBlock / 64 - 1) / (kBlock / 64);
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(volume_raycast_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    } else {
        const int64_t blocks = (P.n + kBlock - 1) / kBlock;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(volume_raycast_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    }
    return hipGetLastError();
}

}  // namespace d3f
