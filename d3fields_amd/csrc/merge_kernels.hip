// merge_kernels.hip -- what have I seen so far?  Two baked fields on one grid merged into one (include/d3fields_hip_ext.h, d3f_volume_merge_select
// and d3f_volume_merge_rows).
//
// The contract (restated in tests/merge_cases.py).  a is the older field, b the newer; the flat index is (x*ny + y)*nz + z.  A side is USABLE at q
// iff valid[q], dist[q] is not NaN and 0 < w[q] < inf, with w the side's weight volume or, without one, its scalar.  dist and weight of a voxel
// that is not valid are never read.  Per voxel, float32, one rounding per operation, nothing contracted (the build has -ffp-contract=off and this
// file names no contracted operation):
//   kind 0  neither usable                        dist 1e3, weight 0, beta 0, not valid
//   kind 1  only a                                da, wa, beta 0
//   kind 2  only b                                db, wb, beta 1
//   kind 3  both, not |da - db| > gap             s = wa + wb;  beta = wb / s;  dist = da + beta*(db - da);  weight = min(s, w_max)
//   kind 4  both, |da - db| > gap                 db, wb, beta 1
// Rows of a listed voxel q: a has a row iff kind is 1 or 3 and (a is dense or slot_a[q] >= 0); b iff kind is 2, 3 or 4 and (b is dense or
// slot_b[q] >= 0).  Both: a_c + beta*(b_c - a_c) per channel.  One: that row, bit for bit (a half widened exactly).  None: a's fill row, known = 0.
//
//   merge_select_kernel   one lane per voxel, z along the lanes; every output volume written whole
//   merge_rows_kernel     the two phases of volume_kernels.hip / warp_kernels.hip: one lane per listed voxel decides, writes out_known and the sets
//                         of up to 16 channels; for the wider sets sixteen lanes take one voxel along the channels.  They get the voxel and its kind
//                         by shuffles and read the two slots and beta themselves (sixteen lanes, one word each: DESIGN.md section 15 on why the
//                         group loads what it can address).  WIDE: the launch has a set wider than 16 channels.  HALF_A / HALF_B: that side has a
//                         set stored as IEEE half; the float32-only instance carries no conversion.
// No LDS, no atomics, no workspace, nothing waits for another workgroup: two runs give identical bytes.  Every output is written completely; the
// caller's buffers may hold anything.
#include "d3f_internal.h"
#include "d3fields_hip_ext.h"      // D3F_MERGE_*

namespace d3f {

namespace {

constexpr int kNoVoxel = -2, kOutside = -1;                      // the kind a lane holds: past the list / a listed entry outside the volume
constexpr int kFill = 0, kRowA = 1, kRowB = 2, kBoth = 3;         // which rows a listed voxel has
constexpr float kSentinel = 1e3f;

__global__ __launch_bounds__(kBlock) void merge_select_kernel(const MergeSelectArgs P)
{
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= P.n) return;
    const float inf = __builtin_huge_valf();
    float da = 0.0f, db = 0.0f, wa = 0.0f, wb = 0.0f;
    bool ua = false, ub = false;
    if (P.valid_a[q] != 0) {
        da = P.dist_a[q];
        wa = P.weight_a ? P.weight_a[q] : P.wa;
        ua = da == da && wa > 0.0f && wa < inf;                  // (a NaN weight fails both comparisons)
    }
    if (P.valid_b[q] != 0) {
        db = P.dist_b[q];
        wb = P.weight_b ? P.weight_b[q] : P.wb;
        ub = db == db && wb > 0.0f && wb < inf;
    }
    int kind = D3F_MERGE_NONE;
    float d = kSentinel, w = 0.0f, beta = 0.0f;
    if (ua && ub) {
        if (fabsf(da - db) > P.gap) {
            kind = D3F_MERGE_RESET;
            d = db; w = wb; beta = 1.0f;
        } else {
            kind = D3F_MERGE_BLEND;
            const float s = wa + wb;
            beta = wb / s;
            const float diff = db - da;
            const float step = beta * diff;
            d = da + step;
            w = s < P.w_max ? s : P.w_max;
        }
    } else if (ua) {
        kind = D3F_MERGE_KEEP;
        d = da; w = wa;
    } else if (ub) {
        kind = D3F_MERGE_NEW;
        d = db; w = wb; beta = 1.0f;
    }
    P.out_dist[q] = d;
    P.out_weight[q] = w;
    P.out_beta[q] = beta;
    P.out_valid[q] = kind != D3F_MERGE_NONE ? 1 : 0;
    P.out_kind[q] = (uint8_t)kind;
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------
struct MergeRows {
    const uint8_t *kind;
    const float *beta;
    const int32_t *voxels;
    const int32_t *slot_a, *slot_b;
    uint8_t *out_known;
    int64_t m, n;
    int32_t n_sets, banded_a, banded_b;
    MergeSet sets[D3F_MAX_MAPS];
};

struct Rows {
    int mode;              // kFill, kRowA, kRowB, kBoth
    int64_t ra, rb;        // the row of either side (a voxel or a slot)
    float beta;
};

// kind: of voxel q (0..4), or kOutside
__device__ __forceinline__ Rows rows_of(const MergeRows &P, int kind, int64_t q)
{
    Rows r;
    r.mode = kFill;
    r.ra = r.rb = 0;
    r.beta = 0.0f;
    bool ha = kind == D3F_MERGE_KEEP || kind == D3F_MERGE_BLEND, hb = kind == D3F_MERGE_NEW || kind == D3F_MERGE_BLEND || kind == D3F_MERGE_RESET;
    if (ha) {
        r.ra = !P.banded_a ? q : P.slot_a ? (int64_t)P.slot_a[q] : -1;
        ha = r.ra >= 0;
    }
    if (hb) {
        r.rb = !P.banded_b ? q : P.slot_b ? (int64_t)P.slot_b[q] : -1;
        hb = r.rb >= 0;
    }
    if (ha && hb) {
        r.mode = kBoth;
        r.beta = P.beta[q];
    } else if (ha) {
        r.mode = kRowA;
    } else if (hb) {
        r.mode = kRowB;
    }
    return r;
}

// a stored half widened exactly (one v_cvt_f32_f16: subnormals, signed zeros, Inf and NaN keep their value)
__device__ __forceinline__ float widen(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }

template <bool HALF>
__device__ __forceinline__ const void *row_at(const void *data, int64_t row, int64_t stride)
{
    return static_cast<const char *>(data) + row * stride * (HALF ? 2 : 4);
}

template <bool HALF>
__device__ __forceinline__ float load_one(const void *row, int k)
{
    if constexpr (HALF)
        return (float)static_cast<const _Float16 *>(row)[k];
    else
        return static_cast<const float *>(row)[k];
}

// channels k .. k + 4*N - 1 of a row: N float4; a half row has N == 2, one 16-byte load of eight channels
template <bool HALF, int N>
__device__ __forceinline__ void load_vectors(const void *row, int k, float4 (&v)[N])
{
    if constexpr (HALF) {
        static_assert(N == 2, "eight halves to a 16-byte load");
        const uint4 r = *reinterpret_cast<const uint4 *>(static_cast<const _Float16 *>(row) + k);
        v[0] = make_float4(widen(r.x & 0xffffu), widen(r.x >> 16), widen(r.y & 0xffffu), widen(r.y >> 16));
        v[1] = make_float4(widen(r.z & 0xffffu), widen(r.z >> 16), widen(r.w & 0xffffu), widen(r.w >> 16));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = *reinterpret_cast<const float4 *>(static_cast<const float *>(row) + k + 4 * i);
    }
}

__device__ __forceinline__ float mix(float a, float b, float beta)
{
    const float diff = b - a;
    const float step = beta * diff;
    return a + step;
}

// one stored row to the output row, no arithmetic
template <bool HALF, int N>
__device__ __forceinline__ void copy_row(const MergeSet &S, float *__restrict__ o, const void *row, int first, int lanes)
{
    if (S.vec) {
        for (int k = 4 * N * first; k < S.C; k += 4 * N * lanes) {
            float4 v[N];
            load_vectors<HALF, N>(row, k, v);
#pragma unroll
            for (int i = 0; i < N; ++i) *reinterpret_cast<float4 *>(o + k + 4 * i) = v[i];
        }
    } else {
        for (int k = first; k < S.C; k += lanes) o[k] = load_one<HALF>(row, k);
    }
}

// channels [first, C) in steps of `lanes` vectors / floats of output row `o`; HA / HB: how this pair's rows are stored.  A pair with a half side
// that moves as vectors has C % 8 == 0 and steps by eight channels, a float32 pair by four.
template <bool HA, bool HB>
__device__ __forceinline__ void merge_row(const MergeSet &S, float *__restrict__ o, const Rows &r, int first, int lanes)
{
    constexpr int N = (HA || HB) ? 2 : 1;
    if (r.mode == kFill) {
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes)
                *reinterpret_cast<float4 *>(o + k) = S.fill ? make_float4(S.fill[k], S.fill[k + 1], S.fill[k + 2], S.fill[k + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = S.fill ? S.fill[k] : 0.0f;
        }
    } else if (r.mode == kRowA) {
        copy_row<HA, N>(S, o, row_at<HA>(S.a, r.ra, S.stride_a), first, lanes);
    } else if (r.mode == kRowB) {
        copy_row<HB, N>(S, o, row_at<HB>(S.b, r.rb, S.stride_b), first, lanes);
    } else {
        const void *pa = row_at<HA>(S.a, r.ra, S.stride_a), *pb = row_at<HB>(S.b, r.rb, S.stride_b);
        const float beta = r.beta;
        if (S.vec) {
            for (int k = 4 * N * first; k < S.C; k += 4 * N * lanes) {
                float4 a[N], b[N];
                load_vectors<HA, N>(pa, k, a);
                load_vectors<HB, N>(pb, k, b);
#pragma unroll
                for (int i = 0; i < N; ++i)
                    *reinterpret_cast<float4 *>(o + k + 4 * i) =
                        make_float4(mix(a[i].x, b[i].x, beta), mix(a[i].y, b[i].y, beta), mix(a[i].z, b[i].z, beta), mix(a[i].w, b[i].w, beta));
            }
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = mix(load_one<HA>(pa, k), load_one<HB>(pb, k), beta);
        }
    }
}

// the storage of one pair is the same in every lane: a branch per set, outside the channel loop
template <bool HALF_A, bool HALF_B>
__device__ __forceinline__ void merge_set(const MergeSet &S, float *__restrict__ o, const Rows &r, int first, int lanes)
{
    const bool ha = HALF_A && S.f16_a != 0, hb = HALF_B && S.f16_b != 0;
    if (ha && hb)
        merge_row<true, true>(S, o, r, first, lanes);
    else if (ha)
        merge_row<true, false>(S, o, r, first, lanes);
    else if (hb)
        merge_row<false, true>(S, o, r, first, lanes);
    else
        merge_row<false, false>(S, o, r, first, lanes);
}

template <bool WIDE, bool HALF_A, bool HALF_B>
__global__ __launch_bounds__(kBlock) void merge_rows_kernel(const MergeRows P)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int kind = kNoVoxel;
    int q32 = 0;
    if (j < P.m) {
        const int64_t q = P.voxels ? (int64_t)P.voxels[j] : j;
        const bool inside = q >= 0 && q < P.n;
        kind = inside ? (int)P.kind[q] : kOutside;
        q32 = inside ? (int)q : 0;                               // (n <= 2^31 - 1)
        const Rows r = rows_of(P, kind, q32);
        P.out_known[j] = r.mode != kFill ? 1 : 0;
        for (int s = 0; s < P.n_sets; ++s)
            if (P.sets[s].C <= kVolNarrowMax) merge_set<HALF_A, HALF_B>(P.sets[s], P.sets[s].out + j * P.sets[s].C, r, 0, 1);
    }
    if (WIDE) {
        const int lane = threadIdx.x & 63, group = lane >> 4, sub = lane & 15;
        const int64_t wave_first = j - lane;
        for (int round = 0; round < 16; ++round) {
            if (wave_first + 4 * round >= P.m) break;            // wave-uniform: no voxel left
            const int from = 4 * round + group;
            const int kind_g = __shfl(kind, from, 64);
            const int q_g = __shfl(q32, from, 64);
            if (kind_g == kNoVoxel) continue;
            const Rows r = rows_of(P, kind_g, q_g);
            for (int s = 0; s < P.n_sets; ++s)
                if (P.sets[s].C > kVolNarrowMax) merge_set<HALF_A, HALF_B>(P.sets[s], P.sets[s].out + (wave_first + from) * P.sets[s].C, r, sub, 16);
        }
    }
}

template <bool WIDE, bool HALF_A>
void launch_rows(bool half_b, unsigned blocks, const MergeRows &P, hipStream_t s)
{
    if (half_b)
        hipLaunchKernelGGL((merge_rows_kernel<WIDE, HALF_A, true>), dim3(blocks), dim3(kBlock), 0, s, P);
    else
        hipLaunchKernelGGL((merge_rows_kernel<WIDE, HALF_A, false>), dim3(blocks), dim3(kBlock), 0, s, P);
}

}  // namespace

hipError_t launch_merge_select(const MergeSelectArgs &A, hipStream_t s)
{
    const int64_t blocks = (A.n + kBlock - 1) / kBlock;          // n <= 2^31 - 1: below 2^23
    hipLaunchKernelGGL(merge_select_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_merge_rows(const MergeRowsArgs &A, hipStream_t s)
{
    MergeRows P;
    P.kind = A.kind;
    P.beta = A.beta;
    P.voxels = A.voxels;
    P.slot_a = A.slot_a;
    P.slot_b = A.slot_b;
    P.out_known = A.out_known;
    P.m = A.m;
    P.n = A.n;
    P.n_sets = A.n_sets;
    P.banded_a = A.banded_a ? 1 : 0;
    P.banded_b = A.banded_b ? 1 : 0;
    bool wide = false, half_a = false, half_b = false;
    for (int i = 0; i < A.n_sets; ++i) {
        P.sets[i] = A.sets[i];
        wide = wide || A.sets[i].C > kVolNarrowMax;
        half_a = half_a || A.sets[i].f16_a != 0;
        half_b = half_b || A.sets[i].f16_b != 0;
    }
    const int64_t blocks = (A.m + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (wide) {
        if (half_a)
            launch_rows<true, true>(half_b, (unsigned)blocks, P, s);
        else
            launch_rows<true, false>(half_b, (unsigned)blocks, P, s);
    } else {
        if (half_a)
            launch_rows<false, true>(half_b, (unsigned)blocks, P, s);
        else
            launch_rows<false, false>(half_b, (unsigned)blocks, P, s);
    }
    return hipGetLastError();
}

}  // namespace d3f
