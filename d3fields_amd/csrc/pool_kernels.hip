// pool_kernels.hip -- per-component pooling of a baked field (include/d3fields_hip.h, ABI 16).
//
// Definitions (the contract; restated in tests/pool_cases.py).  label: int32 [nx, ny, nz], z fastest.  A voxel v is a MEMBER of component k
// if label[v] == k with 1 <= k <= K, valid is NULL or valid[v] != 0, and slot is NULL or slot[v] >= 0; any other label indexes nothing.
// A mean row is fold(rows of the members in ascending flat index) / (float)count: fold of up to 256 rows is ((r0 + r1) + r2) + ..., one
// IEEE float32 add per channel starting from r0; a longer list is cut into consecutive chunks of 256 (a ragged last one) and fold is
// applied to the list of the chunks' folds.  A vote goes to the first channel that holds the row's maximum (best = 0; c ascending;
// row[c] > row[best] moves it: a NaN never wins, a NaN at channel 0 stays).  Moments are integer sums of the voxel coordinates.
//
// Store-and-sum, no float atomic anywhere:
//   pool_flag_kernel     flag[v] = member, and count[k] by integer atomic adds: one per distinct label of a wave's turn, the label that holds
//                        most of the wave's voxels kept in registers across the turns (the form of ccl_flatten_kernel).
//   (scan)               launch_exclusive_scan_u32 over the flags: a member's rank in flat order.
//   pool_compact_kernel  (label, flat index) pairs in flat order, below the capacity only; out_members.
//   pool_sort_*          a stable least-significant-digit radix sort of the pairs by label, 8 bits per pass, as many passes as K needs.  A
//                        wave takes 1024 consecutive pairs, 64 at a time; lanes with the same digit find each other by eight ballots, their
//                        rank is the population count of the lower lanes, the wave's running digit offsets live in LDS (one writer per digit
//                        and turn: no atomics).  Counters are laid out [digit][wave], so ONE exclusive scan gives every wave its offsets.
//   pool_prep_kernel     per component: its row count at every level, as inputs of the scans that place its work items and partial rows.
//   pool_level_kernel    one wave folds one chunk of up to 256 rows: lanes along the channels (float4 per lane, 256 channels per pass), the
//                        row index wave-uniform, eight row loads in flight, the adds in order.  Level 0 reads the field's rows through the
//                        sorted member list (and the slot volume); level l > 0 reads the partial rows of level l-1 of ONE component in chunk
//                        order.  A chunk that is its component's last one at its level writes the output row, any other a partial row.  The
//                        host cannot know the largest component without a sync, so it launches the levels the capacity allows (at most 4);
//                        a component whose fold is finished takes no part in the later ones.
//                        Level 0 also casts the votes (wave arg-max per member row) and sums the moments of its chunk: integer atomic adds
//                        into the zeroed outputs, one per chunk and word -- exact in any order.
//   pool_finish_kernel   the division, or the fill row of an empty component.
// Every float is added in an order fixed by the input alone; everything else is integer: two launches give identical bytes.
// Over capacity (out_members > member_capacity) every kernel after the compaction sees no work: only out_members and out_count are defined.
#include "d3f_internal.h"

namespace d3f {

namespace {

constexpr int kPoolChunk = D3F_POOL_CHUNK;
static_assert(kPoolChunk == 256, "a chunk is four turns of a wave; the levels shift by 8 bits");
constexpr int64_t kPoolFlagSpan = 131072;        // pool_flag_kernel: iters = ceil(n / span) turns per workgroup, capped at 64 (as ccl_flatten_kernel)
constexpr int kSortTurns = 16;                   // turns of 64 pairs per wave and pass
constexpr int kSortSpan = 64 * kSortTurns;       // 1024 pairs per wave

__global__ __launch_bounds__(kBlock) void pool_zero_kernel(uint32_t *__restrict__ p, int64_t words)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (int64_t)gridDim.x * kBlock) p[i] = 0u;
}

__device__ __forceinline__ bool pool_member(const int32_t *__restrict__ label, const uint8_t *__restrict__ valid, const int32_t *__restrict__ slot,
                                            int64_t v, int K, int &k)
{
    k = label[v];
    return k >= 1 && k <= K && (!valid || valid[v] != 0) && (!slot || slot[v] >= 0);
}

__global__ __launch_bounds__(kBlock) void pool_flag_kernel(const int32_t *__restrict__ label, const uint8_t *__restrict__ valid, const int32_t *__restrict__ slot,
                                                           uint32_t *__restrict__ flag, int32_t *__restrict__ count, int K, int iters, int64_t n)
{
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kBlock * iters + threadIdx.x;
    int held = 0, held_count = 0;                               // the same in every lane of the wave
    for (int i = 0; i < iters; ++i) {
        const int64_t v = base + (int64_t)i * kBlock;
        int k = 0;
        if (v < n) {
            const bool m = pool_member(label, valid, slot, v, K, k);
            if (!m) k = 0;
            flag[v] = m ? 1u : 0u;
        }
        unsigned long long todo = __ballot(k > 0);
        while (todo) {                                          // one turn per distinct label of the 64 voxels
            const int kl = __shfl(k, (int)__builtin_ctzll(todo));
            const unsigned long long same = __ballot(k == kl);
            const int c = (int)__builtin_popcountll(same);
            if (kl == held) {
                held_count += c;
            } else if (c > held_count) {
                if (held_count > 0 && lane == 0) atomicAdd(count + (held - 1), held_count);
                held = kl;
                held_count = c;
            } else if (lane == 0) {
                atomicAdd(count + (kl - 1), c);
            }
            todo &= ~same;
        }
    }
    if (held_count > 0 && lane == 0) atomicAdd(count + (held - 1), held_count);
}

__global__ __launch_bounds__(kBlock) void pool_compact_kernel(const int32_t *__restrict__ label, const uint8_t *__restrict__ valid, const int32_t *__restrict__ slot,
                                                              const uint32_t *__restrict__ rank, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                              int64_t *__restrict__ out_members, int K, int64_t cap, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    int k;
    const bool m = pool_member(label, valid, slot, v, K, k);
    const int64_t pos = rank[v];
    if (m && pos < cap) {
        keys[pos] = (uint32_t)k;
        vals[pos] = (uint32_t)v;
    }
    if (v == n - 1) *out_members = pos + (m ? 1 : 0);
}

// the members a later kernel works on: none when the list did not fit
__device__ __forceinline__ int64_t pool_listed(const int64_t *__restrict__ members, int64_t cap)
{
    const int64_t m = *members;
    return m <= cap ? m : 0;
}

// the lanes of the wave that hold the same digit as this one (all lanes take part; a lane that is not `on` gets 0)
__device__ __forceinline__ unsigned long long pool_match(bool on, uint32_t d)
{
    unsigned long long mask = __ballot(on);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long has = __ballot(on && bit);
        mask &= bit ? has : ~has;
    }
    return on ? mask : 0ull;
}

// counters[d * waves_total + w] = the pairs of wave w (1024 consecutive ones) whose key has digit d
__global__ __launch_bounds__(kBlock) void pool_sort_count_kernel(const uint32_t *__restrict__ keys, uint32_t *__restrict__ counters, const int64_t *__restrict__ members,
                                                                 int64_t cap, int shift, int64_t waves_total)
{
    __shared__ uint32_t s_hist[kBlock / 64][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t M = pool_listed(members, cap);
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s_hist[w][threadIdx.x] = 0u;
    __syncthreads();
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    for (int t = 0; t < kSortTurns; ++t) {
        const int64_t i = gw * kSortSpan + t * 64 + lane;
        if (gw * kSortSpan + t * 64 >= M) break;                // uniform over the wave
        const bool on = i < M;
        const uint32_t d = on ? (keys[i] >> shift) & 255u : 0u;
        const unsigned long long same = pool_match(on, d);
        if (on && (int)__builtin_ctzll(same) == lane) s_hist[wave][d] += (uint32_t)__builtin_popcountll(same);      // one writer per digit
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) counters[(int64_t)threadIdx.x * waves_total + (int64_t)blockIdx.x * (kBlock / 64) + w] = s_hist[w][threadIdx.x];
}

// offsets: the exclusive scan of the counters.  Stable: a wave's pairs of one digit keep their order, waves are placed in order.
__global__ __launch_bounds__(kBlock) void pool_sort_scatter_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t *__restrict__ keys_out,
                                                                   uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ offsets,
                                                                   const int64_t *__restrict__ members, int64_t cap, int shift, int64_t waves_total)
{
    __shared__ uint32_t s_base[kBlock / 64][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t M = pool_listed(members, cap);
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s_base[w][threadIdx.x] = offsets[(int64_t)threadIdx.x * waves_total + (int64_t)blockIdx.x * (kBlock / 64) + w];
    __syncthreads();
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    for (int t = 0; t < kSortTurns; ++t) {
        const int64_t i = gw * kSortSpan + t * 64 + lane;
        if (gw * kSortSpan + t * 64 >= M) break;
        const bool on = i < M;
        uint32_t key = 0u, val = 0u;
        if (on) {
            key = keys[i];
            val = vals[i];
        }
        const uint32_t d = (key >> shift) & 255u;
        const unsigned long long same = pool_match(on, d);
        const uint32_t below = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
        uint32_t pos = 0u;
        if (on) pos = s_base[wave][d] + below;
        __builtin_amdgcn_wave_barrier();
        if (on && below == 0u) s_base[wave][d] = pos + (uint32_t)__builtin_popcountll(same);
        __builtin_amdgcn_wave_barrier();
        if (on && (int64_t)pos < M) {
            keys_out[pos] = key;
            vals_out[pos] = val;
        }
    }
}

__global__ __launch_bounds__(kBlock) void pool_prep_kernel(const int32_t *__restrict__ count, const int64_t *__restrict__ members, int64_t cap, int K, int levels, PoolPlan A)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k > K) return;
    const bool listed = *members <= cap;
    const int64_t c = (k < K && listed) ? count[k] : 0;
    A.first[k] = (uint32_t)c;
    int64_t rows = c;                                           // rows at level l
    for (int l = 0; l < levels; ++l) {
        const int64_t next = (rows + kPoolChunk - 1) >> 8;
        const bool takes_part = l == 0 ? rows > 0 : rows > 1;
        A.work[l][k] = takes_part ? (uint32_t)next : 0u;
        if (l < 3 && l + 1 < levels) A.part[l][k] = next > 1 ? (uint32_t)next : 0u;
        rows = next;
    }
}

struct PoolSet {
    const float *data;       // row of voxel (or slot) q: data + q * stride
    const float *fill;
    void *out;               // float [K, C] (mean) or int32 [K, C] (votes)
    int64_t stride;
    int32_t C;
    int32_t mode;
    int32_t vec_data;        // rows of the field move as 16-byte vectors
    int32_t vec_out;         // rows of the output do
    int32_t part_offset;     // where the set's channels start in a partial row (a multiple of 4 floats)
};

struct PoolLevel {
    const int32_t *count;
    const int64_t *members;
    int64_t cap;
    const uint32_t *vals;        // level 0: the sorted member list
    const int32_t *slot;
    const uint32_t *first;
    const uint32_t *work;        // this level's chunk offsets [K + 1]
    const uint32_t *part_in;     // level l > 0: where each component's partial rows of level l-1 start
    const uint32_t *part_out;    // where it writes this level's (nullptr at the last level the capacity allows)
    const float *rows_in;        // partial rows of level l-1
    float *rows_out;
    int64_t *moments;            // level 0; may be nullptr
    int32_t pitch;               // floats per partial row
    int32_t K, level, n_sets;
    int32_t ny, nz;
    PoolSet sets[D3F_MAX_MAPS];
};

__device__ __forceinline__ float4 pool_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float pool_add(float a, float b) { return a + b; }

// fold of `rows` rows (1..256), the channels T of this lane at src + row * stride; L0: row t is ridx[t / 64] of lane t % 64, else row t is t.
// Whole waves call it (the row index travels by a cross-lane read); a lane that is not `on` loads nothing and returns rubbish.
template <typename T, bool L0>
__device__ __forceinline__ T pool_fold(const float *__restrict__ src, int64_t stride, const uint32_t (&ridx)[4], int rows, bool on)
{
    T acc = T();
    if (!L0) {                                                  // consecutive rows: one plain loop
#pragma nounroll
        for (int tb = 0; tb < rows; tb += 8) {
            T r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                r[u] = T();
                if (on && tb + u < rows) r[u] = *reinterpret_cast<const T *>(src + (int64_t)(tb + u) * stride);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (tb + u < rows) acc = tb + u == 0 ? r[u] : pool_add(acc, r[u]);
        }
        return acc;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma nounroll
        for (int t0 = 0; t0 < 64; t0 += 8) {
            const int tb = j * 64 + t0;
            if (tb >= rows) break;
            T r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {                      // eight loads in flight
                const uint32_t q = L0 ? (uint32_t)__shfl((int)ridx[j], t0 + u) : (uint32_t)(tb + u);
                r[u] = T();
                if (on && tb + u < rows) r[u] = *reinterpret_cast<const T *>(src + (int64_t)q * stride);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)                        // the adds in order, starting from row 0 itself
                if (tb + u < rows) acc = tb + u == 0 ? r[u] : pool_add(acc, r[u]);
        }
    }
    return acc;
}

template <typename T, bool L0>
__device__ __forceinline__ void pool_fold_set(const float *__restrict__ src, int64_t stride, float *__restrict__ dst, int C, const uint32_t (&ridx)[4], int rows, int lane)
{
    constexpr int W = (int)(sizeof(T) / sizeof(float));
    for (int cb = 0; cb < C; cb += 64 * W) {                    // uniform over the wave
        const int c0 = cb + lane * W;
        const bool on = c0 < C;
        const T acc = pool_fold<T, L0>(src + c0, stride, ridx, rows, on);
        if (on) *reinterpret_cast<T *>(dst + c0) = acc;
    }
}

// the first channel that holds the maximum of each member row; lane L counts the votes of channels L, L + 64, L + 128, L + 192
__device__ __forceinline__ void pool_votes(const PoolSet &S, const uint32_t (&ridx)[4], int rows, int lane, int32_t *__restrict__ out_row)
{
    const float ninf = -__builtin_huge_valf();
    int votes[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        for (int t = 0; t < 64; ++t) {
            if (j * 64 + t >= rows) break;
            const uint32_t q = (uint32_t)__shfl((int)ridx[j], t);
            const float *row = S.data + (int64_t)q * S.stride;
            float best = ninf;
            int at = 0x7fffffff;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = lane + 64 * u;
                if (c < S.C) {
                    float x = row[c];
                    if (x != x) x = c == 0 ? __builtin_huge_valf() : ninf;      // a NaN never wins; at channel 0 it is never beaten
                    if (x > best || at == 0x7fffffff) {
                        best = x;
                        at = c;
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float xo = __shfl_xor(best, o);
                const int ao = __shfl_xor(at, o);
                if (xo > best || (xo == best && ao < at)) {
                    best = xo;
                    at = ao;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) votes[u] += at == lane + 64 * u ? 1 : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < S.C && votes[u] != 0) atomicAdd(out_row + lane + 64 * u, votes[u]);
}

__device__ __forceinline__ long long pool_wave_sum(long long a)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

__device__ __forceinline__ void pool_moments(const uint32_t (&vox)[4], int rows, int lane, int ny, int nz, int64_t *__restrict__ out_row)
{
    long long s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (lane + 64 * j < rows) {
            const uint32_t l = vox[j] / (uint32_t)nz;
            const long long z = (long long)(vox[j] - l * (uint32_t)nz);
            const long long x = (long long)(l / (uint32_t)ny);
            const long long y = (long long)(l - (uint32_t)x * (uint32_t)ny);
            s[0] += x, s[1] += y, s[2] += z;
            s[3] += x * x, s[4] += x * y, s[5] += x * z;
            s[6] += y * y, s[7] += y * z, s[8] += z * z;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const long long total = pool_wave_sum(s[i]);
        if (lane == 0 && total != 0) atomicAdd(reinterpret_cast<unsigned long long *>(out_row + i), (unsigned long long)total);
    }
}

// One wave per chunk.  Waves leave independently: no workgroup barrier in this kernel.
template <bool L0>
__global__ __launch_bounds__(kBlock) void pool_level_kernel(const PoolLevel P)
{
    const int lane = threadIdx.x & 63;
    if (*P.members > P.cap) return;
    const int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (g >= (int64_t)P.work[P.K]) return;
    int lo = 0, hi = P.K;                                       // work[lo] <= g < work[hi]: the last component that starts at or below chunk g
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)P.work[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const int k = lo;                                           // component k + 1
    const int64_t i = g - (int64_t)P.work[k];                  // its chunk i at this level
    const int64_t c = P.count[k];
    const int sh = 8 * P.level;
    const int64_t n_in = (c + ((1ll << sh) - 1)) >> sh;
    const int64_t n_out = (c + ((1ll << (sh + 8)) - 1)) >> (sh + 8);
    const int rows = (int)min((int64_t)kPoolChunk, n_in - i * kPoolChunk);
    if (rows <= 0) return;                                      // (cannot happen: the offsets come from the same counts)
    const bool last = n_out == 1;                               // this chunk finishes the component's fold: it writes the output row
    if (!last && !P.part_out) return;                           // (cannot happen: count <= capacity <= 256^levels)
    float *const part_row = last ? nullptr : P.rows_out + ((int64_t)P.part_out[k] + i) * P.pitch;
    const float *const in_row = L0 ? nullptr : P.rows_in + ((int64_t)P.part_in[k] + i * kPoolChunk) * P.pitch;

    uint32_t vox[4] = {0u, 0u, 0u, 0u}, ridx[4] = {0u, 0u, 0u, 0u};
    if (L0) {
        const int64_t m0 = (int64_t)P.first[k] + i * kPoolChunk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (lane + 64 * j < rows) {
                vox[j] = P.vals[m0 + lane + 64 * j];
                ridx[j] = P.slot ? (uint32_t)P.slot[vox[j]] : vox[j];
            }
        }
        if (P.moments) pool_moments(vox, rows, lane, P.ny, P.nz, P.moments + (int64_t)k * 9);
    }
    for (int s = 0; s < P.n_sets; ++s) {
        const PoolSet &S = P.sets[s];
        if (S.mode == D3F_POOL_VOTES) {
            if (L0) pool_votes(S, ridx, rows, lane, static_cast<int32_t *>(S.out) + (int64_t)k * S.C);
            continue;
        }
        const float *src = L0 ? S.data : in_row + S.part_offset;
        const int64_t stride = L0 ? S.stride : (int64_t)P.pitch;
        float *dst = last ? static_cast<float *>(S.out) + (int64_t)k * S.C : part_row + S.part_offset;
        const bool vec = S.C % 4 == 0 && (!L0 || S.vec_data) && (!last || S.vec_out);
        if (vec)
            pool_fold_set<float4, L0>(src, stride, dst, S.C, ridx, rows, lane);
        else
            pool_fold_set<float, L0>(src, stride, dst, S.C, ridx, rows, lane);
    }
}

__global__ __launch_bounds__(kBlock) void pool_finish_kernel(float *__restrict__ out, const float *__restrict__ fill, const int32_t *__restrict__ count,
                                                             const int64_t *__restrict__ members, int64_t cap, int C, int64_t total)
{
    if (*members > cap) return;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t k = e / C;
        const int c = (int)(e - k * C);
        const int n = count[k];
        out[e] = n > 0 ? out[e] / (float)n : (fill ? fill[c] : 0.0f);
    }
}

unsigned pool_grid(int64_t items)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, 1 << 20));
}

}  // namespace

int pool_levels(int64_t cap)
{
    int levels = 1;
    while (levels < 4 && (1ll << (8 * levels)) < cap) ++levels;
    return levels;
}

PoolLayout pool_layout(int64_t n, int64_t K, int64_t cap, int64_t pitch)
{
    PoolLayout L;
    Carve c;
    L.flag = c.take(4 * n);
    L.flag_scan = c.take(scan_scratch_bytes(n));
    for (int b = 0; b < 2; ++b) L.keys[b] = c.take(4 * cap), L.vals[b] = c.take(4 * cap);
    L.waves_total = (cap + kSortSpan - 1) / kSortSpan;
    L.waves_total = (L.waves_total + 3) / 4 * 4;
    L.counters = c.take(4 * 256 * L.waves_total);
    L.counters_scan = c.take(scan_scratch_bytes(256 * L.waves_total));
    L.first = c.take(4 * (K + 1));
    for (int l = 0; l < 4; ++l) L.work[l] = c.take(4 * (K + 1));
    for (int l = 0; l < 3; ++l) L.part[l] = c.take(4 * (K + 1));
    L.plan_scan = c.take(scan_scratch_bytes(K + 1));
    // partial rows: a component writes ceil(count / 256^(l+1)) of them at level l where that is more than one, so at most
    // capacity / 256^(l+1) + (the components with more than 256^(l+1) members) <= 2 * capacity / 256^(l+1); levels 0 and 2 share buffer a
    L.rows_a = cap > kPoolChunk ? 2 * (cap >> 8) + 2 : 0;
    L.rows_b = cap > 65536 ? 2 * (cap >> 16) + 2 : 0;
    L.rows[0] = c.take(4 * pitch * L.rows_a);
    L.rows[1] = c.take(4 * pitch * L.rows_b);
    L.total = c.at;
    return L;
}

// mean_channels: the sum of C over the mean sets; a partial row pads every set to a multiple of 4 floats
int64_t pool_workspace_bytes(int64_t n, int64_t K, int64_t cap, int64_t mean_channels)
{
    cap = std::min(cap, n);
    return pool_layout(n, K, cap, mean_channels > 0 ? mean_channels + 3 * D3F_MAX_MAPS : 0).total;
}

// Everything before the folds: the zeroed counts, flags and counts, ranks, the list in flat order, the stable sort by label, the plan and its scans.
hipError_t launch_pool_members(const int32_t *label, const uint8_t *valid, const int32_t *slot, int64_t n, int K, int64_t cap, int64_t *out_members,
                               int32_t *out_count, void *workspace, const PoolLayout &L, PoolList *list, hipStream_t s)
{
    const dim3 block(kBlock);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint32_t *flag = reinterpret_cast<uint32_t *>(ws + L.flag);
    uint32_t *keys[2] = {reinterpret_cast<uint32_t *>(ws + L.keys[0]), reinterpret_cast<uint32_t *>(ws + L.keys[1])};
    uint32_t *vals[2] = {reinterpret_cast<uint32_t *>(ws + L.vals[0]), reinterpret_cast<uint32_t *>(ws + L.vals[1])};
    uint32_t *counters = reinterpret_cast<uint32_t *>(ws + L.counters);

    hipLaunchKernelGGL(pool_zero_kernel, dim3(pool_grid(K)), block, 0, s, reinterpret_cast<uint32_t *>(out_count), (int64_t)K);

    // members: flags and counts, ranks, the list in flat order
    const int iters = (int)std::min<int64_t>(64, (n + kPoolFlagSpan - 1) / kPoolFlagSpan);
    const int64_t span = (int64_t)kBlock * iters;
    const dim3 grid_n((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(pool_flag_kernel, dim3((unsigned)((n + span - 1) / span)), block, 0, s, label, valid, slot, flag, out_count, K, iters, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_exclusive_scan_u32(flag, flag, n, ws + L.flag_scan, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pool_compact_kernel, grid_n, block, 0, s, label, valid, slot, flag, keys[0], vals[0], out_members, K, cap, n);

    // the list grouped by label: a stable sort, least significant digit first
    int sorted = 0;
    if (cap > 0) {
        const int passes = K < 256 ? 1 : K < 65536 ? 2 : K < (1 << 24) ? 3 : 4;
        const dim3 grid_sort((unsigned)(L.waves_total / 4));
        for (int p = 0; p < passes; ++p) {
            hipLaunchKernelGGL(pool_sort_count_kernel, grid_sort, block, 0, s, keys[sorted], counters, out_members, cap, 8 * p, L.waves_total);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            e = launch_exclusive_scan_u32(counters, counters, 256 * L.waves_total, ws + L.counters_scan, s);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(pool_sort_scatter_kernel, grid_sort, block, 0, s, keys[sorted], vals[sorted], keys[sorted ^ 1], vals[sorted ^ 1], counters, out_members,
                               cap, 8 * p, L.waves_total);
            sorted ^= 1;
        }
    }

    // where every component's members, chunks and partial rows start
    const int levels = cap > 0 ? pool_levels(cap) : 0;
    PoolPlan plan;
    plan.first = reinterpret_cast<uint32_t *>(ws + L.first);
    for (int l = 0; l < 4; ++l) plan.work[l] = reinterpret_cast<uint32_t *>(ws + L.work[l]);
    for (int l = 0; l < 3; ++l) plan.part[l] = reinterpret_cast<uint32_t *>(ws + L.part[l]);
    hipLaunchKernelGGL(pool_prep_kernel, dim3((unsigned)(((int64_t)K + 1 + kBlock - 1) / kBlock)), block, 0, s, out_count, out_members, cap, K, levels, plan);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (levels > 0) {
        e = launch_exclusive_scan_u32(plan.first, plan.first, (int64_t)K + 1, ws + L.plan_scan, s);
        for (int l = 0; l < levels && e == hipSuccess; ++l) {
            e = launch_exclusive_scan_u32(plan.work[l], plan.work[l], (int64_t)K + 1, ws + L.plan_scan, s);
            if (e == hipSuccess && l + 1 < levels) e = launch_exclusive_scan_u32(plan.part[l], plan.part[l], (int64_t)K + 1, ws + L.plan_scan, s);
        }
        if (e != hipSuccess) return e;
    }

    list->vals = vals[sorted];
    list->plan = plan;
    list->levels = levels;
    return hipGetLastError();
}

hipError_t launch_volume_pool(const PoolArgs &A, hipStream_t s)
{
    const int64_t n = (int64_t)A.nx * A.ny * A.nz;
    const int64_t cap = std::min(A.member_capacity, n);
    const int K = A.K;
    const dim3 block(kBlock);
    int32_t pitch = 0;
    PoolLevel P;
    for (int i = 0; i < A.n_sets; ++i) {
        PoolSet &S = P.sets[i];
        S.data = A.sets[i].data;
        S.fill = A.sets[i].fill;
        S.out = A.out_rows[i];
        S.stride = A.sets[i].stride_voxel;
        S.C = A.sets[i].C;
        S.mode = A.modes[i];
        S.vec_data = S.C % 4 == 0 && S.stride % 4 == 0 && ((uintptr_t)S.data & 15) == 0;
        S.vec_out = S.C % 4 == 0 && ((uintptr_t)S.out & 15) == 0;
        S.part_offset = pitch;
        if (S.mode == D3F_POOL_MEAN) pitch += (S.C + 3) / 4 * 4;
    }
    const PoolLayout L = pool_layout(n, K, cap, pitch);
    unsigned char *ws = static_cast<unsigned char *>(A.workspace);

    // the zeroed integer outputs (out_count: launch_pool_members)
    if (A.out_moments) hipLaunchKernelGGL(pool_zero_kernel, dim3(pool_grid((int64_t)K * 18)), block, 0, s, reinterpret_cast<uint32_t *>(A.out_moments), (int64_t)K * 18);
    for (int i = 0; i < A.n_sets; ++i)
        if (P.sets[i].mode == D3F_POOL_VOTES)
            hipLaunchKernelGGL(pool_zero_kernel, dim3(pool_grid((int64_t)K * P.sets[i].C)), block, 0, s, static_cast<uint32_t *>(P.sets[i].out), (int64_t)K * P.sets[i].C);

    PoolList list;
    hipError_t e = launch_pool_members(A.label, A.valid, A.slot, n, K, cap, A.out_members, A.out_count, A.workspace, L, &list, s);
    if (e != hipSuccess) return e;
    const int levels = list.levels;
    const PoolPlan &plan = list.plan;

    // the folds
    P.count = A.out_count;
    P.members = A.out_members;
    P.cap = cap;
    P.vals = list.vals;
    P.slot = A.slot;
    P.first = plan.first;
    P.moments = A.out_moments;
    P.pitch = pitch;
    P.K = K;
    P.n_sets = A.n_sets;
    P.ny = A.ny;
    P.nz = A.nz;
    float *rows[2] = {reinterpret_cast<float *>(ws + L.rows[0]), reinterpret_cast<float *>(ws + L.rows[1])};
    for (int l = 0; l < levels; ++l) {
        if (l > 0 && pitch == 0) break;                          // votes and moments are done at level 0
        P.level = l;
        P.work = plan.work[l];
        P.part_in = l > 0 ? plan.part[l - 1] : nullptr;
        P.part_out = l + 1 < levels ? plan.part[l] : nullptr;
        P.rows_in = l > 0 ? rows[(l - 1) & 1] : nullptr;
        P.rows_out = rows[l & 1];
        const int64_t chunks = pool_level_chunks(cap, K, l);
        const dim3 grid((unsigned)((chunks + 3) / 4));
        if (l == 0)
            hipLaunchKernelGGL(pool_level_kernel<true>, grid, block, 0, s, P);
        else
            hipLaunchKernelGGL(pool_level_kernel<false>, grid, block, 0, s, P);
    }

    // the division, the fill rows
    for (int i = 0; i < A.n_sets; ++i) {
        const PoolSet &S = P.sets[i];
        if (S.mode != D3F_POOL_MEAN) continue;
        const int64_t total = (int64_t)K * S.C;
        hipLaunchKernelGGL(pool_finish_kernel, dim3(pool_grid(total)), block, 0, s, static_cast<float *>(S.out), S.fill, A.out_count, A.out_members, cap, S.C, total);
    }
    return hipGetLastError();
}

hipError_t launch_pool_nothing(int64_t *out_members, hipStream_t s)
{
    hipLaunchKernelGGL(pool_zero_kernel, dim3(1), dim3(kBlock), 0, s, reinterpret_cast<uint32_t *>(out_members), (int64_t)2);
    return hipGetLastError();
}

}  // namespace d3f
