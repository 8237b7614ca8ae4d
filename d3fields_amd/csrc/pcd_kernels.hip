// pcd_kernels.hip -- the point-cloud steps on the mask side of the path, fp64 like numpy.
//
//   backproject_*   depth2fgpcd (utils/my_utils.py:522-537) fused with the camera->world transform and the
//                   boundary crop of aggr_point_cloud_from_data (utils/draw_utils.py:325-413): one lane per
//                   pixel, ORDER-PRESERVING compaction (numpy's boolean-mask order = ascending pixel index)
//                   in two passes: per-workgroup survivor counts, then prefix (sum of the counts before the
//                   workgroup) + in-workgroup rank.
//   nearest_kernel  the two directed nearest-neighbour searches of Fusion.pcd_iou (fusion.py:724-741), which
//                   the reference does through an [N,M] distance matrix: one lane per query point, the other
//                   cloud staged through LDS in 256-point tiles; the first minimum of the ROOTED distances wins and the
//                   first NaN beats every number (np.min / np.argmin; the rule is stated at the kernel).
#include "d3f_internal.h"

namespace d3f {

struct BackprojectParams {
    const double *depth;      // [H*W]
    const uint8_t *mask;      // [H*W] or nullptr
    int64_t npix;
    int32_t W;
    double fx, fy, cx, cy;
    double T[12];             // first three rows of inv(pose), row-major
    double lo[3], hi[3];
    int32_t crop;
};

__device__ __forceinline__ bool backproject_pixel(const BackprojectParams &P, int64_t i, double &wx, double &wy, double &wz)
{
    const double d = P.depth[i];
    // aggr_point_cloud_from_data: masks is None -> (depth > 0) & (depth < 1.5); else masks & (depth > 0)
    const bool fg = P.mask ? (P.mask[i] != 0 && d > 0.0) : (d > 0.0 && d < 1.5);
    if (!fg) return false;
    const double px = (double)(i % P.W), py = (double)(i / P.W);
    const double x = (px - P.cx) * d / P.fx;            // depth2fgpcd: (pos_x - cx) * depth / fx
    const double y = (py - P.cy) * d / P.fy;
    wx = ((P.T[0] * x + P.T[1] * y) + P.T[2] * d) + P.T[3];
    wy = ((P.T[4] * x + P.T[5] * y) + P.T[6] * d) + P.T[7];
    wz = ((P.T[8] * x + P.T[9] * y) + P.T[10] * d) + P.T[11];
    if (P.crop)
        return wx > P.lo[0] && wx < P.hi[0] && wy > P.lo[1] && wy < P.hi[1] && wz > P.lo[2] && wz < P.hi[2];
    return true;
}

__global__ __launch_bounds__(kBlock) void backproject_count_kernel(const BackprojectParams P, int64_t *__restrict__ counts)
{
    __shared__ int wave_cnt[kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double x, y, z;
    const bool keep = i < P.npix && backproject_pixel(P, i, x, y, z);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ __launch_bounds__(kBlock) void backproject_write_kernel(const BackprojectParams P, const int64_t *__restrict__ counts,
                                                                  int64_t capacity, double *__restrict__ out_pts,
                                                                  int32_t *__restrict__ out_pixel, int64_t *__restrict__ total)
{
    __shared__ long long part[kBlock];
    __shared__ int wave_cnt[kBlock / 64];
    // exclusive prefix of this workgroup = sum of the counts of all earlier workgroups
    long long acc = 0;
    for (int64_t b = threadIdx.x; b < (int64_t)blockIdx.x; b += kBlock) acc += counts[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    const long long prefix = part[0];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double x = 0, y = 0, z = 0;
    const bool keep = i < P.npix && backproject_pixel(P, i, x, y, z);
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_cnt[w];
    if (keep) {
        const long long slot = prefix + before + __popcll(b & ((1ull << lane) - 1ull));
        if (slot < capacity) {
            out_pts[slot * 3 + 0] = x; out_pts[slot * 3 + 1] = y; out_pts[slot * 3 + 2] = z;
            if (out_pixel) out_pixel[slot] = (int32_t)i;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        *total = prefix + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one count per workgroup of 256 pixels, and one word more that nothing reads
PixelCountsLayout pixel_counts_layout(int64_t npix)
{
    PixelCountsLayout L;
    Carve c;
    L.blocks = (npix + kBlock - 1) / kBlock;
    L.counts = c.take((L.blocks + 1) * 8, 8);
    L.total = c.at;
    return L;
}

hipError_t launch_backproject(const double *depth, const uint8_t *mask, int H, int W, const double *cam, const double *T,
                              const double *bounds, int64_t capacity, double *out_pts, int32_t *out_pixel, int64_t *count,
                              void *workspace, hipStream_t s)
{
    BackprojectParams P;
    P.depth = depth; P.mask = mask; P.npix = (int64_t)H * W; P.W = W;
    P.fx = cam[0]; P.fy = cam[1]; P.cx = cam[2]; P.cy = cam[3];
    for (int k = 0; k < 12; ++k) P.T[k] = T[k];
    P.crop = bounds ? 1 : 0;
    for (int k = 0; k < 3; ++k) { P.lo[k] = bounds ? bounds[2 * k] : 0.0; P.hi[k] = bounds ? bounds[2 * k + 1] : 0.0; }
    const PixelCountsLayout L = pixel_counts_layout(P.npix);
    int64_t *block_counts = static_cast<int64_t *>(ws_at(workspace, L.counts));
    const unsigned nb = (unsigned)L.blocks;
    hipLaunchKernelGGL(backproject_count_kernel, dim3(nb), dim3(kBlock), 0, s, P, block_counts);
    hipLaunchKernelGGL(backproject_write_kernel, dim3(nb), dim3(kBlock), 0, s, P, block_counts, capacity, out_pts, out_pixel, count);
    return hipGetLastError();
}

// ---- directed nearest neighbour (fusion.py:731-735): min / first argmin of sqrt((dx*dx + dy*dy) + dz*dz) ----
// The order is that of the ROOTS, as np.argmin over np.linalg.norm sees them: sqrt is monotone but not injective in floating
// point (two squares one ulp apart often share a root), so among rows with equal roots the FIRST wins, also when a later
// one has the smaller square.  The root stays off the per-pair path: only a square below the smallest one seen so far can
// have a smaller root, so only such a pair takes a root, and it replaces the winner only if that root is strictly smaller.
// Invariant while no NaN was met: best2 = the smallest square seen, best = sqrt(best2), arg = the first row whose root is best.
// NaN as in numpy's min / argmin: the first row with a NaN distance wins and nothing replaces it (best2 = -inf closes the
// gate for every later square, best != best for every later NaN).
constexpr int kNearestGroup = 8;       // rows of b whose squares are formed together before one test whether any of them matters

__device__ __forceinline__ double nearest_square(double ax, double ay, double az, const double *__restrict__ p)
{
    const double dx = ax - p[0], dy = ay - p[1], dz = az - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ void nearest_visit(double d2, int64_t row, double &best2, double &best, int64_t &arg)
{
    if (d2 >= best2) return;                                 // what passes is a smaller square, or a NaN
    const double r = sqrt(d2);
    if (r != r) {
        if (best == best) { best = r; arg = row; }
        best2 = -INFINITY;
    } else {
        if (r < best) { best = r; arg = row; }
        best2 = d2;
    }
}

__global__ __launch_bounds__(kBlock) void nearest_kernel(const double *__restrict__ a, int64_t na, const double *__restrict__ b,
                                                        int64_t nb, double *__restrict__ min_dist, int64_t *__restrict__ argmin)
{
    __shared__ double tile[kBlock * 3];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < na;
    const double ax = live ? a[i * 3 + 0] : 0.0, ay = live ? a[i * 3 + 1] : 0.0, az = live ? a[i * 3 + 2] : 0.0;
    double best2 = INFINITY, best = INFINITY;
    int64_t arg = 0;
    for (int64_t j0 = 0; j0 < nb; j0 += kBlock) {
        const int cnt = (int)min((int64_t)kBlock, nb - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * 3; t += kBlock) tile[t] = b[j0 * 3 + t];
        __syncthreads();
        // rows are visited in order, one by one; a group whose squares all fail the gate as it stands before the group is
        // skipped whole (the gate only tightens, so none of them would pass it later either)
        int t = 0;
        for (; t + kNearestGroup <= cnt; t += kNearestGroup) {
            double d2[kNearestGroup];
            bool any = false;
#pragma unroll
            for (int u = 0; u < kNearestGroup; ++u) {
                d2[u] = nearest_square(ax, ay, az, tile + (t + u) * 3);
                any |= !(d2[u] >= best2);
            }
            if (any) {
#pragma unroll
                for (int u = 0; u < kNearestGroup; ++u) nearest_visit(d2[u], j0 + t + u, best2, best, arg);
            }
        }
        for (; t < cnt; ++t) nearest_visit(nearest_square(ax, ay, az, tile + t * 3), j0 + t, best2, best, arg);
    }
    if (live) { min_dist[i] = best; argmin[i] = arg; }
}

hipError_t launch_nearest(const double *a, int64_t na, const double *b, int64_t nb, double *min_dist, int64_t *argmin, hipStream_t s)
{
    if (na == 0) return hipSuccess;
    hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)((na + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, na, b, nb, min_dist, argmin);
    return hipGetLastError();
}

}  // namespace d3f
