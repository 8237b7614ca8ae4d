// align_kernels.hip -- rigid alignment of point sets to the baked field (include/d3fields_hip.h, d3f_volume_align_*):
// the 6 x 6 normal equations of a damped Gauss-Newton step, summed per instance on the device, and the step itself.
//
// The contract.  Per instance: model points p_j, weights w_j >= 0, a pose (R, t) in float32.  In fp32
//   x_a = fma(R_a2, p_z, fma(R_a1, p_y, R_a0 * p_x)) + t_a;   c = the same chain on the model's weighted centroid;   xs = x - c (float64).
// x is located exactly as d3f_volume_sample / d3f_band_sample locate a point (volume_rows.h: locate_at).  A valid point with w_j > 0 has
//   the distance residual   r = wd (dist(x) - d_j),      g = (wd / h) d dist / d t      and, with a set and where in_band, per channel k
//   a descriptor residual   r = wf (f_k(x) - s_jk),      g = (wf / h) d f_k / d t,
// values by the eight-corner chain (volume_cell.h: blend), derivatives by the face-weight chain (volume_rows.h: add_derivative).  Per point
//   G = sum g g^T (6),  q = sum g r (3),  e = sum r^2 (1)     in fp32, one fmaf per term, channels first, the distance term last,
// then in float64, with X = [xs]_x:  H = w [[X G X^T, X G], [., G]] (21 upper entries),  b = w [X q; q],  cost = w e.
// A weighted point that is not valid adds w * outside^2 to the cost and nothing else; a point with w_j <= 0 (or NaN) adds nothing at all.
//
// align_accumulate_kernel: 256 points of ONE instance per workgroup.  Phase A, one lane per point: the pose chain, the three divisions, the
// cell byte (and the band byte).  Phase B, as the wide sampler: the wave walks its 64 points four at a time, sixteen lanes per point along the
// channels (16-byte row vectors under that sampler's rule, scalars otherwise); a lane keeps ten sums, the group folds them with __shfl_xor
// (8, 4, 2, 1) and the lane that located the point takes them, adds the distance term and expands to the 28 float64 sums.  The wave folds
// those with __shfl_xor (32 ... 1), the four waves through LDS as (w0 + w1) + (w2 + w3), and lanes 0..31 write ONE row per (instance, chunk).
// align_fold_kernel / align_step_kernel: one wave per instance adds the instance's rows in ascending chunk order -- even chunks in lanes
// 0..31, odd chunks in lanes 32..63, one column per lane, then even + odd -- so both give the same bytes.
// align_step_kernel then runs the Levenberg-Marquardt bookkeeping of DESIGN.md 22 on lane 0 in float64: accept or reject the candidate,
// lambda, the statuses, (H + lambda D) delta = -b by Cholesky, Rodrigues, the candidate pose rounded to the float32 the next accumulate reads.
//
// No atomic, no float atomic, no wait on another workgroup, no polling: every output word is written by exactly one lane and two runs give
// identical bytes.  A solve is a fixed chain of launches on the caller's stream.
#include "d3f_internal.h"
#include "volume_rows.h"

namespace d3f {

namespace {

constexpr int kStRa = 0, kStRc = 12, kStTc = 21, kStModel = 24, kStLambda = 27, kStCost = 28, kStStatus = 29, kStSteps = 30, kStValid = 31,
              kStInBand = 32, kStDelta = 33, kStH = 39, kStB = 60;
constexpr double kLambdaMin = 1e-9, kLambdaMax = 1e6, kDiagFloor = 1e-9;

// x_a = fma(R_a2, p_z, fma(R_a1, p_y, R_a0 * p_x)) + t_a, pose = R row-major then t
__device__ __forceinline__ void pose_chain(const float *pose, float px, float py, float pz, float (&x)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = fmaf(pose[3 * a + 2], pz, fmaf(pose[3 * a + 1], py, pose[3 * a] * px)) + pose[9 + a];
}

// one residual: its value and derivative from the corner values v, added to G (a[0..5]: xx xy xz yy yz zz), q (a[6..8]) and e (a[9])
__device__ __forceinline__ void add_residual(const float (&w)[8], const FaceWeights &f, const float (&v)[8], float target, float wt, float wth, float (&a)[10])
{
    const float val = blend(w, v);
    float d[3] = {0.0f, 0.0f, 0.0f};
    add_derivative(f, v, 1.0f, d);                 // fmaf(1, d, 0): the derivative itself
    const float r = wt * (val - target);
    const float gx = wth * d[0], gy = wth * d[1], gz = wth * d[2];
    a[0] = fmaf(gx, gx, a[0]);
    a[1] = fmaf(gx, gy, a[1]);
    a[2] = fmaf(gx, gz, a[2]);
    a[3] = fmaf(gy, gy, a[3]);
    a[4] = fmaf(gy, gz, a[4]);
    a[5] = fmaf(gz, gz, a[5]);
    a[6] = fmaf(gx, r, a[6]);
    a[7] = fmaf(gy, r, a[7]);
    a[8] = fmaf(gz, r, a[8]);
    a[9] = fmaf(r, r, a[9]);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the 28 sums of one point from its fp32 (G, q, e), its weight and xs = x - c, in float64: put(k, value) takes entry k of the row, the upper
// triangle of the 6 x 6 row by row, then b, then the cost
template <class Put>
__device__ __forceinline__ void expand(const float (&a)[10], double w, double sx, double sy, double sz, Put put)
{
    const double G[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    const double q[3] = {a[6], a[7], a[8]};
    const double X[3][3] = {{0.0, -sz, sy}, {sz, 0.0, -sx}, {-sy, sx, 0.0}};
    constexpr int first[3] = {0, 6, 11};           // where row i of the upper triangle starts
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double M[3];                               // row i of M = X G;  H_rr = M X^T,  H_rt = M
#pragma unroll
        for (int j = 0; j < 3; ++j) M[j] = X[i][0] * G[0][j] + X[i][1] * G[1][j] + X[i][2] * G[2][j];
#pragma unroll
        for (int j = i; j < 3; ++j) put(first[i] + (j - i), w * (M[0] * X[j][0] + M[1] * X[j][1] + M[2] * X[j][2]));
#pragma unroll
        for (int j = 0; j < 3; ++j) put(first[i] + (3 - i) + j, w * M[j]);
        put(21 + i, w * (X[i][0] * q[0] + X[i][1] * q[1] + X[i][2] * q[2]));
    }
    put(15, w * G[0][0]);
    put(16, w * G[0][1]);
    put(17, w * G[0][2]);
    put(18, w * G[1][1]);
    put(19, w * G[1][2]);
    put(20, w * G[2][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) put(24 + i, w * q[i]);
}

__global__ __launch_bounds__(kBlock) void align_accumulate_kernel(AlignParams A)
{
    const VolParams &P = A.V;
    const int64_t inst = (int64_t)blockIdx.x / A.chunks, chunk = (int64_t)blockIdx.x - inst * A.chunks;
    if (A.skip != nullptr && A.skip[inst] != 0) return;      // uniform over the workgroup: a final instance costs one load
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = chunk * kBlock + threadIdx.x;          // the point within its instance
    const int64_t sx = (int64_t)P.ny * P.nz, sy = P.nz;
    const float *pose = A.pose + 12 * inst;
    const float *model = A.centroid + 3 * inst;
    const float wdh = A.wd * P.rh, wfh = A.wf * P.rh;

    Cell me;
    me.base = kNoPoint;
    me.tx = me.ty = me.tz = 0.0f;
    int32_t band_base = kNoPoint;      // what phase B sees of a point: its base where it has descriptor residuals, kNotValid elsewhere
    float x[3] = {0.0f, 0.0f, 0.0f};
    float wt = 0.0f;
    bool in_band = false;
    if (j < P.n) {
        const int64_t at = inst * P.n + j;
        wt = A.weights != nullptr ? A.weights[at] : 1.0f;
        me.base = kNotValid;
        band_base = kNotValid;
        if (wt > 0.0f) {                                     // (a NaN weight is no weight)
            const float *p = P.pts + 3 * at;
            pose_chain(pose, p[0], p[1], p[2], x);
            int64_t cell = 0;
            me = locate_at(P, x[0], x[1], x[2], cell);
            in_band = me.base >= 0 && (A.banded == 0 || (A.cell_band != nullptr && A.cell_band[cell] != 0));
            if (in_band && P.n_sets > 0) band_base = me.base;
        }
    }

    float acc[10] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (P.n_sets > 0) {
        const VolSet &S = P.sets[0];
        const int group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = j - lane;
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            if (wave_first + 4 * r >= P.n) break;                  // wave-uniform: no point left
            const int src = 4 * r + group;
            const int32_t base = __shfl(band_base, src, 64);
            const float tx = __shfl(me.tx, src, 64), ty = __shfl(me.ty, src, 64), tz = __shfl(me.tz, src, 64);
            float part[10] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (base >= 0) {
                float w[8];
                corner_weights(tx, ty, tz, w);
                const FaceWeights f = face_weights(tx, ty, tz);
                const float *row[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int64_t q = (int64_t)base + corner_offset(c, sx, sy);
                    row[c] = S.data + (A.banded != 0 ? (int64_t)A.slot[q] : q) * S.stride;
                }
                const float *tgt = A.targets + (inst * P.n + wave_first + src) * S.C;
                if (S.vec) {
#pragma unroll 1
                    for (int k = 4 * sub; k < S.C; k += 64) {
                        float4 v[8];
#pragma unroll
                        for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(row[c] + k);
                        const float4 sk = *reinterpret_cast<const float4 *>(tgt + k);
                        const float a0[8] = {v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x};
                        const float a1[8] = {v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y};
                        const float a2[8] = {v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z};
                        const float a3[8] = {v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w};
                        add_residual(w, f, a0, sk.x, A.wf, wfh, part);
                        add_residual(w, f, a1, sk.y, A.wf, wfh, part);
                        add_residual(w, f, a2, sk.z, A.wf, wfh, part);
                        add_residual(w, f, a3, sk.w, A.wf, wfh, part);
                    }
                } else {
#pragma unroll 1
                    for (int k = sub; k < S.C; k += 16) {
                        float v[8];
#pragma unroll
                        for (int c = 0; c < 8; ++c) v[c] = row[c][k];
                        add_residual(w, f, v, tgt[k], A.wf, wfh, part);
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < 10; ++a) {
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) part[a] += __shfl_xor(part[a], off, 64);      // every lane of the group holds the sum
                const float mine = __shfl(part[a], (lane & 3) * 16, 64);                            // group (lane & 3) worked on point 4 r + (lane & 3)
                if ((lane >> 2) == r) acc[a] = mine;
            }
        }
    }

    __shared__ double fold[kBlock / 64][kAlignRow];
    const bool valid = me.base >= 0;
    double xs[3] = {0.0, 0.0, 0.0}, cost = 0.0;
    if (valid) {
        float w[8], v[8];
        corner_weights(me.tx, me.ty, me.tz, w);
        const FaceWeights f = face_weights(me.tx, me.ty, me.tz);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = P.dist[(int64_t)me.base + corner_offset(c, sx, sy)];
        add_residual(w, f, v, A.dist_targets != nullptr ? A.dist_targets[inst * P.n + j] : 0.0f, A.wd, wdh, acc);
        float c[3];
        pose_chain(pose, model[0], model[1], model[2], c);
#pragma unroll
        for (int a = 0; a < 3; ++a) xs[a] = (double)x[a] - (double)c[a];
        cost = (double)wt * (double)acc[9];
    } else if (wt > 0.0f) {
        cost = (double)wt * ((double)A.outside * (double)A.outside);
    }
    // (a lane without a valid point holds zeros in acc and xs: its entries are +-0)
    expand(acc, valid ? (double)wt : 0.0, xs[0], xs[1], xs[2], [&](int k, double value) {
        const double total = wave_sum(value);
        if (lane == 0) fold[wave][k] = total;
    });
    const double wave_cost = wave_sum(cost);
    const int n_valid = __popcll(__ballot(valid)), n_band = __popcll(__ballot(in_band));
    if (lane == 0) {
        fold[wave][27] = wave_cost;
        fold[wave][28] = (double)n_valid;
        fold[wave][29] = (double)n_band;
        fold[wave][30] = 0.0;
        fold[wave][31] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < kAlignRow) {
        const int k = threadIdx.x;
        A.partial[((int64_t)blockIdx.x) * kAlignRow + k] = (fold[0][k] + fold[1][k]) + (fold[2][k] + fold[3][k]);
    }
}

// the rows of one instance added in ascending chunk order: every lane returns the sum of column (lane & 31)
__device__ __forceinline__ double fold_rows(const double *partial, int64_t chunks, int lane)
{
    double s = 0.0;
    for (int64_t ch = lane >> 5; ch < chunks; ch += 2) s += partial[ch * kAlignRow + (lane & 31)];
    return s + __shfl_xor(s, 32, 64);
}

__global__ __launch_bounds__(64) void align_fold_kernel(const double *__restrict__ partial, int64_t chunks, const int32_t *__restrict__ skip, double *__restrict__ out)
{
    const int64_t inst = blockIdx.x;
    if (skip != nullptr && skip[inst] != 0) return;
    const int lane = threadIdx.x;
    const double s = fold_rows(partial + inst * chunks * kAlignRow, chunks, lane);
    if (lane < kAlignRow) out[inst * kAlignRow + lane] = s;
}

// the model's weighted centroid over the points with finite coordinates in float64, one wave per instance: lane l adds points l, l + 64, ... in order, the wave folds 32 ... 1
__global__ __launch_bounds__(64) void align_centroid_kernel(const float *__restrict__ pts, const float *__restrict__ weights, int64_t n, float *__restrict__ out)
{
    const int64_t inst = blockIdx.x;
    const int lane = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = lane; j < n; j += 64) {
        const float w = weights != nullptr ? weights[inst * n + j] : 1.0f;
        const float *p = pts + 3 * (inst * n + j);
        if (w > 0.0f && fabsf(p[0]) <= 3.402823466e38f && fabsf(p[1]) <= 3.402823466e38f && fabsf(p[2]) <= 3.402823466e38f) {      // (NaN compares false)
            s[0] += (double)w * (double)p[0];
            s[1] += (double)w * (double)p[1];
            s[2] += (double)w * (double)p[2];
            s[3] += (double)w;
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[a] += __shfl_xor(s[a], off, 64);
    }
    if (lane < 3) {
        const double v = lane == 0 ? s[0] : (lane == 1 ? s[1] : s[2]);
        out[3 * inst + lane] = s[3] > 0.0 ? (float)(v / s[3]) : 0.0f;
    }
}

__device__ __forceinline__ bool small_step(const double *d, double rot_tol, double trans_tol)
{
    return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < rot_tol && sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) < trans_tol;
}

__device__ __forceinline__ int tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }      // i <= j: the upper triangle, row by row

__global__ __launch_bounds__(64) void align_step_kernel(AlignStep S)
{
    const int64_t inst = blockIdx.x;
    const int lane = threadIdx.x;
    double *st = S.state + inst * kAlignState;
    double *hist = S.history + inst * (S.iters + 1) + S.it;
    __shared__ double row[kAlignRow];
    __shared__ double L[6][6];
    __shared__ double y[6];
    if ((int)st[kStStatus] != D3F_ALIGN_RUNNING) {       // final: nothing of the instance changes any more
        if (lane == 0) *hist = st[kStCost];
        return;
    }
    const double sum = fold_rows(S.partial + inst * S.chunks * kAlignRow, S.chunks, lane);
    if (lane < kAlignRow) {
        row[lane] = sum;
        S.out[inst * kAlignRow + lane] = sum;
    }
    __syncthreads();
    if (lane != 0) return;

    // ---- accept or reject the candidate the rows were summed at ----
    double lambda = st[kStLambda];
    int status = D3F_ALIGN_RUNNING;
    const bool accept = S.it == 0 || row[27] < st[kStCost];        // (a NaN cost is rejected)
    if (accept) {
        for (int k = 0; k < 12; ++k) st[kStRa + k] = st[kStRc + k];
        for (int k = 0; k < 21; ++k) st[kStH + k] = row[k];
        for (int k = 0; k < 6; ++k) st[kStB + k] = row[21 + k];
        st[kStCost] = row[27];
        st[kStValid] = row[28];
        st[kStInBand] = row[29];
        if (S.it > 0) {
            lambda = fmax(lambda / 10.0, kLambdaMin);
            st[kStSteps] += 1.0;
            if (small_step(st + kStDelta, S.rot_tol, S.trans_tol)) status = D3F_ALIGN_CONVERGED;
        }
    } else {
        lambda = fmin(lambda * 10.0, kLambdaMax);
        if (lambda >= kLambdaMax) status = D3F_ALIGN_STALLED;
    }
    st[kStLambda] = lambda;
    *hist = st[kStCost];

    // ---- the next candidate: (H + lambda D) delta = -b at the accepted pose ----
    double delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    if (status == D3F_ALIGN_RUNNING && S.it < S.iters) {
        const double *H = st + kStH, *b = st + kStB;
        double hmax = 0.0;
        for (int i = 0; i < 6; ++i) hmax = fmax(hmax, H[tri(i, i)]);      // (fmax drops a NaN)
        if (!(hmax > 0.0)) {
            status = D3F_ALIGN_NO_GRADIENT;
        } else {
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j <= i; ++j) L[i][j] = H[tri(j, i)] + (i == j ? lambda * fmax(H[tri(i, i)], kDiagFloor * hmax) : 0.0);
            bool ok = true;
            for (int j = 0; j < 6 && ok; ++j) {
                double p = L[j][j];
                for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
                if (!(p > 0.0) || !(p <= 1.7976931348623157e308)) {
                    ok = false;
                    break;
                }
                const double d = sqrt(p);
                L[j][j] = d;
                for (int i = j + 1; i < 6; ++i) {
                    double s = L[i][j];
                    for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
                    L[i][j] = s / d;
                }
            }
            if (!ok) {
                status = D3F_ALIGN_FAILED;
            } else {
                for (int i = 0; i < 6; ++i) {
                    double s = -b[i];
                    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
                    y[i] = s / L[i][i];
                }
                for (int i = 5; i >= 0; --i) {
                    double s = y[i];
                    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * y[k];
                    y[i] = s / L[i][i];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) delta[i] = y[i];
                solved = true;
                // the step proposed at a pose that was just accepted is already below both tolerances: the pose is the optimum to within them.
                // (The step itself would lower the cost by less than the fp32 sums resolve, so it could never be accepted and seen to be small.)
                if (accept && small_step(delta, S.rot_tol, S.trans_tol)) {
                    status = D3F_ALIGN_CONVERGED;
                    solved = false;
                }
            }
        }
    }
    st[kStStatus] = (double)status;
    float *po = S.pose_out + 12 * inst;
    if (!solved) {                                   // final, or the iterations ran out: the pose is the accepted one
        for (int k = 0; k < 12; ++k) {
            st[kStRc + k] = st[kStRa + k];
            po[k] = (float)st[kStRa + k];
        }
        if (status != D3F_ALIGN_RUNNING) S.skip_out[inst] = 1;
        return;
    }

    // ---- R <- Exp(w) R, t <- c + Exp(w) (t - c) + v about the pivot the rows were expanded about ----
    float pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = (float)st[kStRa + k];      // (exact: the state holds float32 values)
    float cf[3];
    pose_chain(pose, (float)st[kStModel], (float)st[kStModel + 1], (float)st[kStModel + 2], cf);
    const double wx = delta[0], wy = delta[1], wz = delta[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double ca, cb;                                   // sin(th) / th and (1 - cos(th)) / th^2
    if (th < 1e-4) {
        ca = 1.0 - th2 / 6.0;
        cb = 0.5 - th2 / 24.0;
    } else {
        const double sh = sin(0.5 * th);
        ca = sin(th) / th;
        cb = 2.0 * sh * sh / th2;
    }
    const double E[3][3] = {{1.0 + cb * (wx * wx - th2), -ca * wz + cb * wx * wy, ca * wy + cb * wx * wz},
                            {ca * wz + cb * wx * wy, 1.0 + cb * (wy * wy - th2), -ca * wx + cb * wy * wz},
                            {-ca * wy + cb * wx * wz, ca * wx + cb * wy * wz, 1.0 + cb * (wz * wz - th2)}};
    const double tc[3] = {(double)pose[9] - (double)cf[0], (double)pose[10] - (double)cf[1], (double)pose[11] - (double)cf[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float r = (float)(E[i][0] * (double)pose[j] + E[i][1] * (double)pose[3 + j] + E[i][2] * (double)pose[6 + j]);
            st[kStRc + 3 * i + j] = (double)r;
            po[3 * i + j] = r;
        }
        const float t = (float)((double)cf[i] + (E[i][0] * tc[0] + E[i][1] * tc[1] + E[i][2] * tc[2]) + delta[3 + i]);
        st[kStTc + i] = (double)t;
        po[9 + i] = t;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) st[kStDelta + i] = delta[i];
}

}  // namespace

int64_t align_chunks(int64_t n) { return (n + kBlock - 1) / kBlock; }

// one row of sums per instance and workgroup
AlignLayout align_layout(int64_t I, int64_t n)
{
    AlignLayout L;
    Carve c;
    L.chunks = align_chunks(n);
    L.partial = c.take(I * L.chunks * kAlignRow * (int64_t)sizeof(double), 8);
    L.total = c.at;
    return L;
}

hipError_t launch_align_centroid(const float *pts, const float *weights, int64_t I, int64_t n, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(align_centroid_kernel, dim3((unsigned)I), dim3(64), 0, s, pts, weights, n, out);
    return hipGetLastError();
}

hipError_t launch_align_accumulate(const AlignParams &A, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(align_accumulate_kernel, dim3((unsigned)(A.I * A.chunks)), dim3(kBlock), 0, s, A);
    if (out != nullptr) hipLaunchKernelGGL(align_fold_kernel, dim3((unsigned)A.I), dim3(64), 0, s, A.partial, A.chunks, A.skip, out);
    return hipGetLastError();
}

hipError_t launch_align_step(const AlignStep &S, int64_t I, hipStream_t s)
{
    hipLaunchKernelGGL(align_step_kernel, dim3((unsigned)I), dim3(64), 0, s, S);
    return hipGetLastError();
}

}  // namespace d3f
