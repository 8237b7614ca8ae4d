// motion_kernels.hip -- how did each part move?  One rigid motion per part from dense correspondences (include/d3fields_hip.h, d3f_part_motion;
// DESIGN.md section 26).
//
// The contract (restated in tests/motion_cases.py).  label, target: int32 [nx, ny, nz], z fastest.  Voxel v is a PAIR of part k when
// label[v] == k with 1 <= k <= K, keep is NULL or keep[v] != 0, 0 <= target[v] < n and, with offset given, its three components at v are
// finite.  In voxel units relative to the part's integer reference corner ref_k (NULL: zeros):
//   a = (x, y, z)(v) - ref_k                      exact integers held as float64
//   b = ((x, y, z)(target[v]) - ref_k) + offset[v]  the integer difference first, then one float64 add per axis (none with offset NULL)
// A member's row is {1, a0, a1, a2, b0, b1, b2, a_i * b_j (i major)}: 16 float64; a member that is no inlier of the current fit gives +0.0.
// The rows of a part are folded in ascending flat index in chunks of 256 consecutive members of that part (a ragged last chunk), the next
// level folds the part's partial rows in chunk order, 256 at a time (the chunk and level structure of d3f_volume_pool).  Inside a chunk:
// pad to 256 rows with +0.0; lane l of 64 holds (((0.0 + m_l) + m_{l+64}) + m_{l+128}) + m_{l+192}; then for s = 32, 16, 8, 4, 2, 1:
// v[l] = v[l] + v[l+s] for l < s.  IEEE float64 adds, the columns independent, nothing fused.
// Fit (one lane per part): n, A, B, M the sums; pm = A / n, cm = B / n, S_ij = M_ij - (A_i * B_j) / n, R by horn_rotation (d3f_horn.h).
// Pose row: R row-major, ref + pm, ref + cm.  Residual of a pair: u = a - pm, w = b - cm, e_i = ((R_i0 u0 + R_i1 u1) + R_i2 u2) - w_i,
// r2 = (e0 e0 + e1 e1) + e2 e2; inlier iff r2 <= tau2 (a NaN compares false).  Fit 0 takes every pair, fit f the inliers under fit f-1.
//
//   motion_mask_kernel    lab[v] = label[v] where v is a pair, else 0
//   (pool_kernels.hip)    launch_pool_members on lab: counts (out_pairs), out_members, the label-sorted list, the plan of chunks per level
//   motion_level_kernel   one wave folds one chunk: level 0 forms the rows (and, from fit 1 on, the residual under the pose of the fit
//                         before), level l > 0 reads the part's partial rows of level l-1.  The chunk that finishes a part's fold writes its
//                         row of sums.  A part whose loop has ended takes no part.
//   motion_fit_kernel     one lane per part: the status, the pose.  The 4 x 4 work matrices live in LDS, 64 lanes interleaved.
//   motion_fill_kernel    NaN / 0 into the residual and inlier volumes
//   motion_level_kernel   again with rows {inlier, r2 of an inlier}: it writes the residual and inlier volumes at level 0
//   motion_finish_kernel  the inlier count and the rmse
// As many levels are launched as the capacity allows.  Every float is added in an order fixed by the input alone, the rest is integer; no
// float atomic, nothing waits for another workgroup, nothing is read back.  Over capacity every kernel after the compaction leaves at once.
// Collinear or coincident pairs leave the rotation about their axis undetermined: the result is then still a function of the input alone.
#include "d3f_horn.h"
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int kChunk = D3F_POOL_CHUNK;
constexpr int kSumRow = D3F_MOTION_SUM_DOUBLES;      // a row of moments
constexpr int kFinalRow = 2;                         // {inlier, r2 of an inlier}
constexpr int kPoseRow = D3F_MOTION_POSE_DOUBLES;
static_assert(kChunk == 256 && kSumRow == 16 && kPoseRow == 15, "four turns of a wave; 1 + 3 + 3 + 9 sums; R, src, dst");

__global__ __launch_bounds__(kBlock) void motion_mask_kernel(const int32_t *__restrict__ label, const uint8_t *__restrict__ keep, const int32_t *__restrict__ target,
                                                             const double *__restrict__ offset, int32_t *__restrict__ lab, int K, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    const int k = label[v];
    bool pair = k >= 1 && k <= K && (!keep || keep[v] != 0);
    if (pair) {
        const int t = target[v];
        pair = t >= 0 && (int64_t)t < n;
    }
    if (pair && offset) {
        const double inf = __builtin_huge_val();
#pragma unroll
        for (int a = 0; a < 3; ++a) pair = pair && fabs(offset[3 * v + a]) < inf;      // a NaN compares false
    }
    lab[v] = pair ? k : 0;
}

__global__ __launch_bounds__(kBlock) void motion_fill_kernel(double *__restrict__ res2, uint8_t *__restrict__ inl, const int64_t *__restrict__ members, int64_t cap,
                                                             int64_t n)
{
    if (*members > cap) return;
    const double nan = __builtin_nan("");
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        if (res2) res2[v] = nan;
        if (inl) inl[v] = 0;
    }
}

struct MotionLevel {
    const int32_t *count;
    const int64_t *members;
    int64_t cap;
    const uint32_t *vals;        // level 0: the sorted member list
    const uint32_t *first;
    const uint32_t *work;        // this level's chunk offsets [K + 1]
    const uint32_t *part_in;     // level l > 0: where each part's partial rows of level l-1 start
    const uint32_t *part_out;    // where it writes this level's (nullptr at the last level the capacity allows)
    const double *rows_in;
    double *rows_out;
    double *out;                 // [K, NC]: the row of a part whose fold is finished
    const int32_t *status;
    const int32_t *target;
    const double *offset;        // or nullptr
    const int32_t *ref;          // or nullptr
    const double *pose;          // [K, 15]
    const double *centre;        // [K, 6]: pm, cm
    double *res2;                // the last pass: the volumes (or nullptr)
    uint8_t *inl;
    double tau2;
    int32_t K, level, fit, ny, nz;
};

// One wave per chunk; NC = 16: the moments of fit P.fit, NC = 2: the last pass.  SCORED (level 0): the rows depend on the residual under the
// pose of the fit before -- every fit but the first, and the last pass.  Waves leave independently: no workgroup barrier.
// The row of a member is written as one select per entry: with the entries assigned inside `if (inlier)` and a run-time `scored` the
// compiler (hipcc -O3) dropped the b0 entry on the scored path.
template <int NC, bool L0, bool SCORED>
__global__ __launch_bounds__(kBlock) void motion_level_kernel(const MotionLevel P)
{
    constexpr bool kFinal = NC == kFinalRow;
    const int lane = threadIdx.x & 63;
    if (*P.members > P.cap) return;
    const int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)P.work[P.K]) return;
    int lo = 0, hi = P.K;                                       // work[lo] <= g < work[hi]: the last part that starts at or below chunk g
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)P.work[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const int k = __builtin_amdgcn_readfirstlane(lo);           // part k + 1; the same in every lane
    if (kFinal ? P.status[k] == D3F_MOTION_TOO_FEW : (P.fit > 0 && P.status[k] != D3F_MOTION_OK)) return;      // no pose / its loop has ended
    const int64_t i = g - (int64_t)P.work[k];                  // its chunk i at this level
    const int64_t c = P.count[k];
    const int sh = 8 * P.level;
    const int64_t n_in = (c + ((1ll << sh) - 1)) >> sh;
    const int64_t n_out = (c + ((1ll << (sh + 8)) - 1)) >> (sh + 8);
    const int rows = (int)min((int64_t)kChunk, n_in - i * kChunk);
    if (rows <= 0) return;                                      // (cannot happen: the offsets come from the same counts)
    const bool last = n_out == 1;                               // this chunk finishes the part's fold
    if (!last && !P.part_out) return;                           // (cannot happen: count <= capacity <= 256^levels)

    double acc[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) acc[e] = 0.0;
    if (L0) {
        constexpr bool scored = SCORED;
        static_assert(SCORED || !kFinal || !L0, "the last pass scores");
        long long r[3] = {0, 0, 0};
        if (P.ref) {
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = P.ref[3 * k + a];
        }
        double R[9], pm[3], cm[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = scored ? P.pose[(int64_t)k * kPoseRow + e] : 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pm[a] = scored ? P.centre[(int64_t)k * 6 + a] : 0.0;
            cm[a] = scored ? P.centre[(int64_t)k * 6 + 3 + a] : 0.0;
        }
        const int64_t m0 = (int64_t)P.first[k] + i * kChunk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double row[NC];
#pragma unroll
            for (int e = 0; e < NC; ++e) row[e] = 0.0;
            if (lane + 64 * j < rows) {
                const uint32_t v = P.vals[m0 + lane + 64 * j];
                const uint32_t t = (uint32_t)P.target[v];       // a pair: 0 <= target < n
                double a[3], b[3];
                {
                    const uint32_t l = v / (uint32_t)P.nz, x = l / (uint32_t)P.ny;
                    a[0] = (double)((long long)x - r[0]);
                    a[1] = (double)((long long)(l - x * (uint32_t)P.ny) - r[1]);
                    a[2] = (double)((long long)(v - l * (uint32_t)P.nz) - r[2]);
                }
                {
                    const uint32_t l = t / (uint32_t)P.nz, x = l / (uint32_t)P.ny;
                    b[0] = (double)((long long)x - r[0]);
                    b[1] = (double)((long long)(l - x * (uint32_t)P.ny) - r[1]);
                    b[2] = (double)((long long)(t - l * (uint32_t)P.nz) - r[2]);
                }
                if (P.offset) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) b[q] = b[q] + P.offset[3 * (int64_t)v + q];
                }
                bool in = true;
                double r2 = 0.0;
                if (scored) {
                    const double u0 = a[0] - pm[0], u1 = a[1] - pm[1], u2 = a[2] - pm[2];
                    const double e0 = ((R[0] * u0 + R[1] * u1) + R[2] * u2) - (b[0] - cm[0]);
                    const double e1 = ((R[3] * u0 + R[4] * u1) + R[5] * u2) - (b[1] - cm[1]);
                    const double e2 = ((R[6] * u0 + R[7] * u1) + R[8] * u2) - (b[2] - cm[2]);
                    r2 = (e0 * e0 + e1 * e1) + e2 * e2;
                    in = r2 <= P.tau2;
                }
                if (kFinal) {
                    if (P.res2) P.res2[v] = r2;
                    if (P.inl) P.inl[v] = in ? 1 : 0;
                    row[0] = in ? 1.0 : 0.0;
                    row[1] = in ? r2 : 0.0;
                } else {
                    row[0] = in ? 1.0 : 0.0;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        row[1 + q] = in ? a[q] : 0.0;
                        row[4 + q] = in ? b[q] : 0.0;
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            const double ab = a[q] * b[p];
                            row[7 + 3 * q + p] = in ? ab : 0.0;
                        }
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < NC; ++e) acc[e] = acc[e] + row[e];
        }
    } else {
        const double *in_row = P.rows_in + ((int64_t)P.part_in[k] + i * kChunk) * NC;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < NC; ++e) {
                const double x = lane + 64 * j < rows ? in_row[(int64_t)(lane + 64 * j) * NC + e] : 0.0;
                acc[e] = acc[e] + x;
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {                          // v[l] = v[l] + v[l+s] for l < s; what the lanes above hold is never read again
#pragma unroll
        for (int e = 0; e < NC; ++e) acc[e] = acc[e] + __shfl_down(acc[e], s);
    }
    if (lane == 0) {
        double *dst = last ? P.out + (int64_t)k * NC : P.rows_out + ((int64_t)P.part_out[k] + i) * NC;
#pragma unroll
        for (int e = 0; e < NC; ++e) dst[e] = acc[e];
    }
}

struct MotionFit {
    const int32_t *count;
    const int64_t *members;
    int64_t cap;
    const int32_t *ref;          // or nullptr
    double *sums;                // [K, 16]
    double *pose;                // [K, 15]
    double *centre;              // [K, 6]
    int32_t *status, *fits;
    int32_t K, fit, min_pairs;
};

// one lane per part; the work matrices of the 64 lanes interleaved in LDS (entry e of lane l at [e * 64 + l]: no bank conflict)
__global__ __launch_bounds__(64) void motion_fit_kernel(const MotionFit F)
{
    __shared__ double sA[16 * 64], sV[16 * 64];
    if (*F.members > F.cap) return;
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    if (k >= F.K) return;
    double *sums = F.sums + k * kSumRow;
    if (F.fit == 0) {
        if (F.count[k] == 0) {                                  // no chunk wrote this row
#pragma unroll
            for (int e = 0; e < kSumRow; ++e) sums[e] = 0.0;
        }
    } else if (F.status[k] != D3F_MOTION_OK) {
        return;
    }
    const double n = sums[0];
    if (!(n >= (double)F.min_pairs)) {
        if (F.fit == 0) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int e = 0; e < kPoseRow; ++e) F.pose[k * kPoseRow + e] = nan;
#pragma unroll
            for (int e = 0; e < 6; ++e) F.centre[k * 6 + e] = nan;
            F.status[k] = D3F_MOTION_TOO_FEW;
            F.fits[k] = 0;
        } else {
            F.status[k] = D3F_MOTION_THINNED;                   // the pose of the fit before stays
            F.fits[k] = F.fit;
        }
        return;
    }
    double A[3], B[3], pm[3], cm[3], S[3][3], R[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        A[a] = sums[1 + a];
        B[a] = sums[4 + a];
        pm[a] = A[a] / n;
        cm[a] = B[a] / n;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) S[a][b] = sums[7 + 3 * a + b] - (A[a] * B[b]) / n;
    horn_rotation<64>(S, sA + lane, sV + lane, R);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r = F.ref ? (double)F.ref[3 * k + a] : 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) F.pose[k * kPoseRow + 3 * a + b] = R[a][b];
        F.pose[k * kPoseRow + 9 + a] = r + pm[a];
        F.pose[k * kPoseRow + 12 + a] = r + cm[a];
        F.centre[k * 6 + a] = pm[a];
        F.centre[k * 6 + 3 + a] = cm[a];
    }
    F.status[k] = D3F_MOTION_OK;
    F.fits[k] = F.fit + 1;
}

__global__ __launch_bounds__(kBlock) void motion_finish_kernel(const double *__restrict__ fsum, const int32_t *__restrict__ status, const int64_t *__restrict__ members,
                                                               int64_t cap, int K, int32_t *__restrict__ inliers, double *__restrict__ rmse)
{
    if (*members > cap) return;
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    double s0 = 0.0, s1 = 0.0;
    if (status[k] != D3F_MOTION_TOO_FEW) {                      // it has pairs, so its row was written
        s0 = fsum[k * kFinalRow];
        s1 = fsum[k * kFinalRow + 1];
    }
    inliers[k] = (int32_t)s0;
    rmse[k] = s0 > 0.0 ? sqrt(s1 / s0) : __builtin_nan("");
}

}  // namespace

// the masked labels, the member list's pieces (pool_layout; a partial row is 16 float64), the sums, the sums of the last pass, (pm, cm) per part
MotionLayout motion_layout(int64_t n, int64_t K, int64_t cap)
{
    MotionLayout L;
    L.P = pool_layout(n, K, cap, 2 * kSumRow);
    Carve c;
    L.lab = c.take(4 * n);
    L.pool = c.take(L.P.total);
    L.sums = c.take(8 * kSumRow * K);
    L.fsum = c.take(8 * kFinalRow * K);
    L.centre = c.take(8 * 6 * K);
    L.total = c.at;
    return L;
}

int64_t motion_workspace_bytes(int64_t n, int64_t K, int64_t cap) { return motion_layout(n, K, std::min(cap, n)).total; }

hipError_t launch_part_motion(const MotionArgs &A, hipStream_t s)
{
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    const int64_t cap = std::min(A.member_capacity, n);
    const int K = A.K;
    const dim3 block(kBlock);
    const MotionLayout L = motion_layout(n, K, cap);
    unsigned char *ws = static_cast<unsigned char *>(A.workspace);
    int32_t *lab = reinterpret_cast<int32_t *>(ws + L.lab);
    double *sums = A.out_sums ? A.out_sums : reinterpret_cast<double *>(ws + L.sums);
    double *fsum = reinterpret_cast<double *>(ws + L.fsum);
    double *centre = reinterpret_cast<double *>(ws + L.centre);
    double *rows[2] = {reinterpret_cast<double *>(ws + L.pool + L.P.rows[0]), reinterpret_cast<double *>(ws + L.pool + L.P.rows[1])};

    // the member list of "label where pair, else 0"
    hipLaunchKernelGGL(motion_mask_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), block, 0, s, A.label, A.keep, A.target, A.offset, lab, K, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    PoolList list;
    e = launch_pool_members(lab, nullptr, nullptr, n, K, cap, A.out_members, A.out_pairs, ws + L.pool, L.P, &list, s);
    if (e != hipSuccess) return e;

    MotionLevel P;
    P.count = A.out_pairs;
    P.members = A.out_members;
    P.cap = cap;
    P.vals = list.vals;
    P.first = list.plan.first;
    P.status = A.out_status;
    P.target = A.target;
    P.offset = A.offset;
    P.ref = A.ref;
    P.pose = A.out_pose;
    P.centre = centre;
    P.res2 = nullptr;
    P.inl = nullptr;
    P.tau2 = A.tau2;
    P.K = K;
    P.ny = A.ny;
    P.nz = A.nz;
    auto fold = [&](bool final_pass) {
        for (int l = 0; l < list.levels; ++l) {
            P.level = l;
            P.work = list.plan.work[l];
            P.part_in = l > 0 ? list.plan.part[l - 1] : nullptr;
            P.part_out = l + 1 < list.levels ? list.plan.part[l] : nullptr;
            P.rows_in = l > 0 ? rows[(l - 1) & 1] : nullptr;
            P.rows_out = rows[l & 1];
            const dim3 grid((unsigned)((pool_level_chunks(cap, K, l) + 3) / 4));
            if (final_pass) {
                if (l == 0)
                    hipLaunchKernelGGL((motion_level_kernel<kFinalRow, true, true>), grid, block, 0, s, P);
                else
                    hipLaunchKernelGGL((motion_level_kernel<kFinalRow, false, false>), grid, block, 0, s, P);
            } else if (l > 0) {
                hipLaunchKernelGGL((motion_level_kernel<kSumRow, false, false>), grid, block, 0, s, P);
            } else if (P.fit > 0) {
                hipLaunchKernelGGL((motion_level_kernel<kSumRow, true, true>), grid, block, 0, s, P);
            } else {
                hipLaunchKernelGGL((motion_level_kernel<kSumRow, true, false>), grid, block, 0, s, P);
            }
        }
    };

    // the loop: fold the moments of the current inliers, fit
    MotionFit F;
    F.count = A.out_pairs;
    F.members = A.out_members;
    F.cap = cap;
    F.ref = A.ref;
    F.sums = sums;
    F.pose = A.out_pose;
    F.centre = centre;
    F.status = A.out_status;
    F.fits = A.out_fits;
    F.K = K;
    F.min_pairs = A.min_pairs;
    P.out = sums;
    for (int f = 0; f < A.fits; ++f) {
        P.fit = F.fit = f;
        fold(false);
        hipLaunchKernelGGL(motion_fit_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, s, F);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }

    // under the final poses: residuals, inliers, rmse
    if (A.out_residual2 || A.out_inlier) {
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 1 << 16));
        hipLaunchKernelGGL(motion_fill_kernel, dim3(grid), block, 0, s, A.out_residual2, A.out_inlier, A.out_members, cap, n);
    }
    P.out = fsum;
    P.res2 = A.out_residual2;
    P.inl = A.out_inlier;
    P.fit = A.fits;
    fold(true);
    hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)((K + kBlock - 1) / kBlock)), block, 0, s, fsum, A.out_status, A.out_members, cap, K, A.out_inliers, A.out_rmse);
    return hipGetLastError();
}

}  // namespace d3f
