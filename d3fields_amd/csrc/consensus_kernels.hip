// consensus_kernels.hip -- which pose explains these matches?  Consensus poses from (model point, candidate) triples (include/d3fields_hip.h,
// d3f_pose_consensus_* / d3f_pose_refit).
//
// The contract.  Model points p [M, 3], candidates c [M, k, 3] (a NaN coordinate: padding), triplets (i < j < l) [n_trip, 3], all float32 / int32.
// A hypothesis is h = (trip * k + a) * k * k + b * k + c: triplet (i, j, l) with the candidate digits (a, b, c).  Only IEEE + - * / sqrt in the
// stated order, no fma anywhere (the build passes -ffp-contract=off), so NumPy restates every number bit for bit (tests/consensus_cases.py).
//   gate (float64 from the float32 inputs):  u = p_j - p_i, v = p_l - p_i, w = v - u;  U = c_jb - c_ia, V = c_lc - c_ia, W = V - U;
//     |x|^2 = (x0 x0 + x1 x1) + x2 x2;  a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  The hypothesis is REJECTED when the triplet is not
//     0 <= i < j < l < M, when one of the nine candidate coordinates is NaN, when not (|u|, |v|, |w| >= min_side), when not
//     (||U| - |u||, ||V| - |v||, ||W| - |w|| <= side_tol), when not (|u x v|^2 >= (min_sin^2 |u|^2) |v|^2) or not the same of (U, V).  Every
//     test is written so that a NaN rejects.  A rejected hypothesis has count 0 and takes no further part.
//   pose (float64):  e1 = u / |u|, e3 = (u x v) / |u x v|, e2 = e3 x e1;  f1, f3, f2 the same of (U, V);
//     R_ab = (f1_a e1_b + f2_a e2_b) + f3_a e3_b;   ps = ((p_i + p_j) + p_l) / 3, cs = ((c_ia + c_jb) + c_lc) / 3;
//     t_a = cs_a - ((R_a0 ps_0 + R_a1 ps_1) + R_a2 ps_2);   every entry rounded ONCE to float32.
//   score (float32), per model point q and candidate s:  x_a = ((R_a0 p_x + R_a1 p_y) + R_a2 p_z) + t_a,  d = x - c_qs,
//     d2 = (dx dx + dy dy) + dz dz;  q is assigned the s with the smallest d2 <= tau2, ties to the lower s, else none (-1); a NaN compares
//     false.  count = the number of assigned points.
//   selection:  survivors = hypotheses with count >= min_inliers, ordered by (count descending, h ascending); the best max_survivors of
//     them are kept.  Then n_poses rounds: take the best live survivor, kill every survivor that shares at least `shared` identical
//     (point, candidate) assignments with it (and the winner itself).  Integer-exact and independent of any order of execution.
//   refit:  Horn's closed form in float64 over the assigned pairs (p_q, c_{q, s_q}) in ascending q: centroids pm, cm (sum / n),
//     S_ab = sum (p - pm)_a (c - cm)_b, the symmetric 4 x 4 N, its largest eigenvector by kRefitSweeps cyclic Jacobi sweeps (a zero
//     off-diagonal entry is skipped), R = the quaternion's matrix divided by |quat|^2, t = cm - R pm, both rounded to float32;
//     rmse = sqrt(sum |R32 p + t32 - c|^2 / n) in float64; the count of the score at the refit pose.
//
// consensus_score_kernel: a workgroup takes kConsPasses * 256 consecutive hypotheses.  p and c are staged in LDS (every lane of a load reads one
// address: a broadcast).  Phase 1, one lane per hypothesis: gate and pose.  Most die there, so the live ones are compacted -- ballot, popcount
// below the lane, four wave totals through LDS -- into a ring of 512 poses in LDS; whenever 256 are queued, phase 2 runs one lane per queued
// pose over the M x k distances with the pose in registers.  Results are keyed by h, so the queue order is invisible.
// Survivors: the histogram of counts (integer atomics), the cut, then per 256 hypotheses the number of flags, scanned by scan_kernels.hip,
// and an order-preserving compaction; the survivors are scored again with their assignments kept (64 bytes each).
// consensus_select_kernel: ONE workgroup runs the rounds over the list: an arg-best over unique keys, then a compare pass.
// pose_refit_kernel: one wave per pose; lane q re-scores point q, lane 0 runs Horn.
// No float atomic, no scratch, nothing waits for another workgroup or polls memory.
#include "d3f_horn.h"
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int kConsPasses = 8;
constexpr int kConsTile = kConsPasses * kBlock;       // hypotheses per workgroup of the score kernel
constexpr int kConsQueue = 2 * kBlock;                // the ring: fewer than 256 left over + at most 256 new
constexpr int kSelectBlock = 1024;
constexpr int kRefitSweeps = kHornSweeps;
static_assert(kRefitSweeps == 12, "the sweeps of the contract (tests/consensus_cases.py)");

__device__ __forceinline__ double norm2(const double (&x)[3]) { return (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]; }

__device__ __forceinline__ void cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// the gate and the pose of hypothesis h (p, c: LDS or global).  -> live; pose = R row-major, then t
__device__ __forceinline__ bool gate_pose(const ConsensusParams &C, const float *p, const float *c, int64_t h, float (&pose)[12])
{
    const int k = C.k, k2 = k * k, k3 = k2 * k;
    const int64_t tr = h / k3;
    const int rem = (int)(h - tr * k3);
    const int da = rem / k2, db = (rem / k) % k, dc = rem % k;
    const int i = C.trip[3 * tr], j = C.trip[3 * tr + 1], l = C.trip[3 * tr + 2];
    if (!(0 <= i && i < j && j < l && l < C.M)) return false;      // (the host has checked the table; this keeps a wrong device copy in bounds)
    const float *ci = c + 3 * (i * k + da), *cj = c + 3 * (j * k + db), *cl = c + 3 * (l * k + dc);
    const float *pi = p + 3 * i, *pj = p + 3 * j, *pl = p + 3 * l;
    double u[3], v[3], w[3], U[3], V[3], W[3];
    bool nan = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nan = nan || ci[a] != ci[a] || cj[a] != cj[a] || cl[a] != cl[a];
        u[a] = (double)pj[a] - (double)pi[a];
        v[a] = (double)pl[a] - (double)pi[a];
        w[a] = v[a] - u[a];
        U[a] = (double)cj[a] - (double)ci[a];
        V[a] = (double)cl[a] - (double)ci[a];
        W[a] = V[a] - U[a];
    }
    if (nan) return false;
    const double u2 = norm2(u), v2 = norm2(v), mu = sqrt(u2), mv = sqrt(v2), mw = sqrt(norm2(w));
    if (!(mu >= C.min_side) || !(mv >= C.min_side) || !(mw >= C.min_side)) return false;
    const double U2 = norm2(U), V2 = norm2(V), oU = sqrt(U2), oV = sqrt(V2), oW = sqrt(norm2(W));
    if (!(fabs(oU - mu) <= C.side_tol) || !(fabs(oV - mv) <= C.side_tol) || !(fabs(oW - mw) <= C.side_tol)) return false;
    double n[3], N[3];
    cross(u, v, n);
    cross(U, V, N);
    const double n2 = norm2(n), N2 = norm2(N);
    if (!(n2 >= (C.min_sin2 * u2) * v2) || !(N2 >= (C.min_sin2 * U2) * V2)) return false;
    const double mn = sqrt(n2), mN = sqrt(N2);
    double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3], ps[3], cs[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = u[a] / mu;
        e3[a] = n[a] / mn;
        f1[a] = U[a] / oU;
        f3[a] = N[a] / mN;
        ps[a] = (((double)pi[a] + (double)pj[a]) + (double)pl[a]) / 3.0;
        cs[a] = (((double)ci[a] + (double)cj[a]) + (double)cl[a]) / 3.0;
    }
    cross(e3, e1, e2);
    cross(f3, f1, f2);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double R[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            R[b] = (f1[a] * e1[b] + f2[a] * e2[b]) + f3[a] * e3[b];
            pose[3 * a + b] = (float)R[b];
        }
        pose[9 + a] = (float)(cs[a] - ((R[0] * ps[0] + R[1] * ps[1]) + R[2] * ps[2]));
    }
    return true;
}

// the assignment of one model point at a pose: the s with the smallest d2 <= tau2, ties to the lower s, else -1
__device__ __forceinline__ int assign_point(const float (&P)[12], const float *pq, const float *cq, int k, float tau2)
{
    const float px = pq[0], py = pq[1], pz = pq[2];
    const float x0 = ((P[0] * px + P[1] * py) + P[2] * pz) + P[9];
    const float x1 = ((P[3] * px + P[4] * py) + P[5] * pz) + P[10];
    const float x2 = ((P[6] * px + P[7] * py) + P[8] * pz) + P[11];
    int bs = -1;
    float bd = 0.0f;
    for (int s = 0; s < k; ++s) {
        const float dx = x0 - cq[3 * s], dy = x1 - cq[3 * s + 1], dz = x2 - cq[3 * s + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= tau2 && (bs < 0 || d2 < bd)) {      // (a NaN compares false)
            bs = s;
            bd = d2;
        }
    }
    return bs;
}

template <class Put>
__device__ __forceinline__ int score_pose(const float (&P)[12], const float *p, const float *c, int M, int k, float tau2, Put put)
{
    int count = 0;
    for (int q = 0; q < M; ++q) {
        const int bs = assign_point(P, p + 3 * q, c + 3 * q * k, k, tau2);
        put(q, bs);
        count += bs >= 0 ? 1 : 0;
    }
    return count;
}

// the rank of a flagged lane among the flagged lanes of its workgroup (in thread order) and their number; `tot` is 4 words of LDS
__device__ __forceinline__ uint32_t block_rank(bool f, uint32_t *tot, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    if (lane == 0) tot[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
    for (int w = 0; w < kBlock / 64; ++w) {
        const uint32_t n = tot[w];
        before += w < wave ? n : 0u;
        total += n;
    }
    return before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void consensus_score_kernel(ConsensusParams C)
{
    __shared__ float sp[3 * kConsMaxM];
    __shared__ float sc[3 * kConsMaxM * kConsMaxK];
    __shared__ float qpose[kConsQueue][13];               // (13: an odd stride, so the lanes of a wave fall on distinct banks)
    __shared__ uint32_t qidx[kConsQueue];
    __shared__ uint32_t tot[kBlock / 64];
    __shared__ uint32_t hist[kConsMaxM + 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < 3 * C.M; e += kBlock) sp[e] = C.model[e];
    for (int e = tid; e < 3 * C.M * C.k; e += kBlock) sc[e] = C.cand[e];
    if (tid <= kConsMaxM) hist[tid] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kConsTile;
    uint32_t head = 0u, tail = 0u;                        // uniform over the workgroup

    // phase 2 on the first n queued poses: the pose to registers, then the M x k distances
    auto drain = [&](uint32_t n) {
        float P[12];
        uint32_t at = 0u;
        const bool mine = (uint32_t)tid < n;
        if (mine) {
            const uint32_t slot = (head + (uint32_t)tid) & (kConsQueue - 1);
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = qpose[slot][e];
            at = qidx[slot];
        }
        // (no barrier here: the next pass writes the ring only after block_rank's barrier, which every lane reaches after these reads)
        if (mine) {
            const int64_t h = base + at;
            int8_t *row = C.assign_dbg != nullptr ? C.assign_dbg + h * C.M : nullptr;
            const int count = score_pose(P, sp, sc, C.M, C.k, C.tau2, [&](int q, int s) {
                if (row != nullptr) row[q] = (int8_t)s;
            });
            C.count[h] = (uint8_t)count;
            atomicAdd(&hist[count], 1u);
        }
        head += n;
    };

#pragma unroll 1
    for (int pass = 0; pass < kConsPasses; ++pass) {
        if (base + (int64_t)pass * kBlock >= C.T) break;  // uniform
        const uint32_t at = (uint32_t)(pass * kBlock + tid);
        const int64_t h = base + at;
        float P[12];
        bool live = false;
        if (h < C.T) {
            live = gate_pose(C, sp, sc, h, P);
            if (!live) {
                C.count[h] = 0;
#pragma unroll
                for (int e = 0; e < 12; ++e) P[e] = 0.0f;
                if (C.assign_dbg != nullptr)
                    for (int q = 0; q < C.M; ++q) C.assign_dbg[h * C.M + q] = (int8_t)-1;
            }
            if (C.pose_dbg != nullptr) {
#pragma unroll
                for (int e = 0; e < 12; ++e) C.pose_dbg[h * 12 + e] = P[e];
            }
        }
        uint32_t total;
        const uint32_t rank = block_rank(live, tot, total);
        if (live) {
            const uint32_t slot = (tail + rank) & (kConsQueue - 1);
#pragma unroll
            for (int e = 0; e < 12; ++e) qpose[slot][e] = P[e];
            qidx[slot] = at;
        }
        tail += total;
        __syncthreads();
        if (tail - head >= (uint32_t)kBlock) drain(kBlock);
    }
    if (tail != head) drain(tail - head);
    __syncthreads();
    if (tid <= kConsMaxM && hist[tid] != 0u) atomicAdd(&C.head[tid], hist[tid]);
    if (tid == 0 && tail != 0u) atomicAdd(&C.head[kConsGated], tail);
}

// the cut: walking the histogram down from 64, the count at which max_survivors is reached and how many hypotheses of that count are kept
__global__ void consensus_cut_kernel(uint32_t *head, int min_inliers, uint32_t max_survivors)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t acc = 0u, cut = (uint32_t)min_inliers, take = 0xffffffffu;
    for (int c = kConsMaxM; c >= min_inliers; --c) {
        const uint32_t n = head[c];
        if (n != 0u && acc + n >= max_survivors) {       // (acc < max_survivors <= 2^16: no wrap)
            cut = (uint32_t)c;
            take = max_survivors - acc;
            break;
        }
        acc += n;
    }
    head[kConsCut] = cut;
    head[kConsTake] = take;
}

// is hypothesis h a survivor?  S.eq_block[blockIdx.x] holds the hypotheses of the cut count before this workgroup's 256 (the scanned totals)
__device__ __forceinline__ bool survivor_flag(const ConsensusSelect &S, int64_t h, uint32_t *tot)
{
    const uint32_t cut = S.C.head[kConsCut], take = S.C.head[kConsTake];
    const uint32_t cnt = h < S.C.T ? S.C.count[h] : 0u;
    const bool eq = cnt == cut;
    uint32_t total;
    const uint32_t rank = block_rank(eq, tot, total);
    return cnt > cut || (eq && (uint64_t)S.eq_block[blockIdx.x] + rank < (uint64_t)take);
}

__global__ __launch_bounds__(kBlock) void consensus_eq_kernel(ConsensusSelect S)
{
    __shared__ uint32_t tot[kBlock / 64];
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool eq = h < S.C.T && S.C.count[h] == S.C.head[kConsCut];
    uint32_t total;
    block_rank(eq, tot, total);
    if (threadIdx.x == 0) S.eq_block[blockIdx.x] = total;
}

// compact == 0: the number of survivors of the workgroup's 256 hypotheses; compact == 1: their h to the list, in ascending order
__global__ __launch_bounds__(kBlock) void consensus_flag_kernel(ConsensusSelect S, int compact)
{
    __shared__ uint32_t tot[kBlock / 64], tot2[kBlock / 64];
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool f = survivor_flag(S, h, tot);
    uint32_t total;
    const uint32_t rank = block_rank(f, tot2, total);
    if (compact == 0) {
        if (threadIdx.x == 0) S.fl_block[blockIdx.x] = total;
        return;
    }
    const uint32_t before = S.fl_block[blockIdx.x];
    if (f && before + rank < S.max_survivors) S.surv_h[before + rank] = (int32_t)h;      // (the cut keeps the total at max_survivors: the test only guards the list)
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) S.C.head[kConsSurvivors] = min(before + total, S.max_survivors);
}

// the survivors scored again, their assignments kept: 64 bytes each, -1 beyond M
__global__ __launch_bounds__(kBlock) void consensus_rescore_kernel(ConsensusSelect S)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S.C.head[kConsSurvivors]) return;
    const ConsensusParams &C = S.C;
    float P[12];
    int8_t *row = S.surv_assign + (int64_t)i * kConsMaxM;
    int count = 0;
    if (gate_pose(C, C.model, C.cand, S.surv_h[i], P))
        count = score_pose(P, C.model, C.cand, C.M, C.k, C.tau2, [&](int q, int s) { row[q] = (int8_t)s; });
    else
        for (int q = 0; q < C.M; ++q) row[q] = (int8_t)-1;
    for (int q = C.M; q < kConsMaxM; ++q) row[q] = (int8_t)-1;
    S.surv_count[i] = (uint8_t)count;
    S.alive[i] = 1;
}

// the greedy rounds, one workgroup.  The list is in ascending h, so (count, 2^32 - 1 - index) is a unique key whose maximum is the best
// survivor under (count descending, h ascending); 0 is "none" (a survivor's count is at least 3).
__global__ __launch_bounds__(kSelectBlock) void consensus_select_kernel(ConsensusSelect S)
{
    __shared__ unsigned long long wave_best[kSelectBlock / 64];
    __shared__ unsigned long long best_s;
    __shared__ uint32_t win[kConsMaxM / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = S.C.head[kConsSurvivors];
    int found = 0;
#pragma unroll 1
    for (int r = 0; r < S.n_poses; ++r) {
        unsigned long long best = 0ull;
        for (uint32_t i = tid; i < n; i += kSelectBlock)
            if (S.alive[i]) best = max(best, ((unsigned long long)S.surv_count[i] << 32) | (unsigned long long)(0xffffffffu - i));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, off, 64));
        if (lane == 0) wave_best[wave] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long b = 0ull;
            for (int w = 0; w < kSelectBlock / 64; ++w) b = max(b, wave_best[w]);
            best_s = b;
        }
        __syncthreads();
        const unsigned long long key = best_s;
        if (key == 0ull) break;                           // uniform: no live survivor is left
        const uint32_t wi = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
        const uint32_t *wrow = reinterpret_cast<const uint32_t *>(S.surv_assign + (int64_t)wi * kConsMaxM);
        if (tid < kConsMaxM / 4) {
            win[tid] = wrow[tid];
            reinterpret_cast<uint32_t *>(S.assign_out + (int64_t)r * kConsMaxM)[tid] = wrow[tid];
        }
        if (tid == 0) {
            S.hyp_out[r] = S.surv_h[wi];
            S.count_out[r] = (int32_t)(key >> 32);
        }
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kSelectBlock) {
            if (!S.alive[i]) continue;
            const uint32_t *row = reinterpret_cast<const uint32_t *>(S.surv_assign + (int64_t)i * kConsMaxM);
            int same = 0;
#pragma unroll
            for (int e = 0; e < kConsMaxM / 4; ++e) {
                const uint32_t a = row[e], x = a ^ win[e];
#pragma unroll
                for (int b = 0; b < 4; ++b) same += ((x >> (8 * b)) & 0xffu) == 0u && ((a >> (8 * b)) & 0x80u) == 0u ? 1 : 0;
            }
            if (same >= S.shared || i == wi) S.alive[i] = 0;
        }
        found = r + 1;
        __syncthreads();                                  // win and best_s are written again in the next round
    }
    // the ranks that were not reached are padding; the poses of the others from their h
    for (int r = found + tid; r < S.n_poses; r += kSelectBlock) {
        S.hyp_out[r] = -1;
        S.count_out[r] = -1;
    }
    for (int e = found * kConsMaxM + tid; e < S.n_poses * kConsMaxM; e += kSelectBlock) S.assign_out[e] = (int8_t)-1;
    if (tid < S.n_poses) {
        float P[12];
        const bool ok = tid < found && gate_pose(S.C, S.C.model, S.C.cand, S.hyp_out[tid], P);      // (hyp_out[tid] was written before a barrier)
#pragma unroll
        for (int e = 0; e < 12; ++e) S.pose_out[12 * tid + e] = ok ? P[e] : __builtin_nanf("");
    }
    if (tid == 0) {
        S.stats_out[0] = found;
        S.stats_out[1] = (int32_t)S.C.head[kConsGated];
        S.stats_out[2] = (int32_t)n;
        S.stats_out[3] = (int32_t)S.C.head[kConsCut];
    }
}

// one wave per pose: Horn's closed form over the assigned pairs on lane 0, the score at the refit pose one point per lane
__global__ __launch_bounds__(64) void pose_refit_kernel(const float *__restrict__ model, const float *__restrict__ cand, int M, int k, const int8_t *__restrict__ assign,
                                                       float tau2, float *__restrict__ pose_out, double *__restrict__ rmse_out, int32_t *__restrict__ count_out)
{
    __shared__ double A[4][4], V[4][4];
    __shared__ float Ps[12];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int8_t *row = assign + (int64_t)r * kConsMaxM;
    if (lane == 0) {
        int n = 0;
        double pm[3] = {0.0, 0.0, 0.0}, cm[3] = {0.0, 0.0, 0.0};
        for (int q = 0; q < M; ++q) {
            const int s = row[q];
            if (s < 0 || s >= k) continue;
            const float *p = model + 3 * q, *c = cand + 3 * (q * k + s);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                pm[a] += (double)p[a];
                cm[a] += (double)c[a];
            }
            ++n;
        }
        const double nan = __builtin_nan("");
        double rmse = nan;
        float P[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = __builtin_nanf("");
        if (n >= 3) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                pm[a] = pm[a] / (double)n;
                cm[a] = cm[a] / (double)n;
            }
            double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
            for (int q = 0; q < M; ++q) {
                const int s = row[q];
                if (s < 0 || s >= k) continue;
                const float *p = model + 3 * q, *c = cand + 3 * (q * k + s);
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[a][b] += ((double)p[a] - pm[a]) * ((double)c[b] - cm[b]);
            }
            double R[3][3];
            horn_rotation<1>(S, &A[0][0], &V[0][0], R);       // d3f_horn.h: the block motion_fit_kernel shares
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) P[3 * a + b] = (float)R[a][b];
                P[9 + a] = (float)(cm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2]));
            }
            double sum = 0.0;
            for (int q = 0; q < M; ++q) {
                const int s = row[q];
                if (s < 0 || s >= k) continue;
                const float *p = model + 3 * q, *c = cand + 3 * (q * k + s);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double d = ((((double)P[3 * a] * (double)p[0] + (double)P[3 * a + 1] * (double)p[1]) + (double)P[3 * a + 2] * (double)p[2]) + (double)P[9 + a]) - (double)c[a];
                    sum += d * d;
                }
            }
            rmse = sqrt(sum / (double)n);
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            Ps[e] = P[e];
            pose_out[12 * r + e] = P[e];
        }
        rmse_out[r] = rmse;
    }
    __syncthreads();
    float P[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = Ps[e];
    const bool real = P[0] == P[0];
    const int bs = (lane < M && real) ? assign_point(P, model + 3 * lane, cand + 3 * lane * k, k, tau2) : -1;
    const int count = __popcll(__ballot(bs >= 0));
    if (lane == 0) count_out[r] = real ? count : -1;
}

}  // namespace

int64_t consensus_blocks(int64_t T) { return (T + kBlock - 1) / kBlock; }

// the head; an eq and a fl word per workgroup of hypotheses and their scan's scratch; per survivor a hypothesis, a count, a flag, an assignment
ConsensusLayout consensus_layout(int64_t T, int64_t max_survivors)
{
    const int64_t nb = consensus_blocks(T);
    ConsensusLayout L;
    Carve c;
    L.head = c.take(kConsHeadWords * 4);
    L.eq = c.take(nb * 4);
    L.fl = c.take(nb * 4);
    L.scan = c.take(scan_scratch_bytes(nb));
    L.surv_h = c.take(max_survivors * 4);
    L.surv_count = c.take(max_survivors);
    L.alive = c.take(max_survivors);
    L.surv_assign = c.take(max_survivors * kConsMaxM);
    L.total = c.at;
    return L;
}

hipError_t launch_consensus_score(const ConsensusParams &C, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(C.head, 0, kConsHeadWords * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const int64_t groups = (C.T + kConsTile - 1) / kConsTile;
    hipLaunchKernelGGL(consensus_score_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, C);
    return hipGetLastError();
}

hipError_t launch_consensus_select(const ConsensusSelect &S, hipStream_t s)
{
    const int64_t nb = consensus_blocks(S.C.T);
    hipLaunchKernelGGL(consensus_cut_kernel, dim3(1), dim3(64), 0, s, S.C.head, S.min_inliers, S.max_survivors);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(consensus_eq_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, S);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_exclusive_scan_u32(S.eq_block, S.eq_block, nb, S.scan_scratch, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(consensus_flag_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, S, 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_exclusive_scan_u32(S.fl_block, S.fl_block, nb, S.scan_scratch, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(consensus_flag_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, S, 1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(consensus_rescore_kernel, dim3((S.max_survivors + kBlock - 1) / kBlock), dim3(kBlock), 0, s, S);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(consensus_select_kernel, dim3(1), dim3(kSelectBlock), 0, s, S);
    return hipGetLastError();
}

hipError_t launch_pose_refit(const float *model, const float *cand, int M, int k, const int8_t *assign, int n_poses, float tau2, float *pose_out, double *rmse_out,
                             int32_t *count_out, hipStream_t s)
{
    hipLaunchKernelGGL(pose_refit_kernel, dim3((unsigned)n_poses), dim3(64), 0, s, model, cand, M, k, assign, tau2, pose_out, rmse_out, count_out);
    return hipGetLastError();
}

}  // namespace d3f
