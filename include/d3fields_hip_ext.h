/*
 * d3fields_hip_ext.h -- entry points of libd3fields_hip.so added after the main table of ABI 16 (include/d3fields_hip.h).
 *
 * The main header is closed: two host tests pin the number of functions it declares and match its text, so it gets no further
 * declaration.  Every entry point added since lives here.  They are exported by the same libd3fields_hip.so, follow the conventions
 * at the top of d3fields_hip.h (device pointers, no allocation, nothing retained, work enqueued on `stream` and not synchronised,
 * outputs and poisoned inputs may hold anything, D3F_OK or a negative D3F_ERR_* code with d3f_last_error()), and D3F_ABI_VERSION
 * stays 16: a library that has the main table and lacks a symbol of this header is an older build of the same ABI.
 */
#ifndef D3FIELDS_HIP_EXT_H
#define D3FIELDS_HIP_EXT_H

#include "d3fields_hip.h" /* d3f_volume_set, d3f_band, D3F_MAX_MAPS, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* What have I seen so far?  Two baked fields on ONE grid merged into one (csrc/merge_kernels.hip): `a` is the older
 * one (the memory), `b` the newer.  The running weighted average of a truncated distance volume, extended to the channel rows: what only one
 * field knows is kept, what both know is averaged by their weights, and where they disagree by more than `gap` the newer one wins.
 * The flat index is q = (x*ny + y)*nz + z.  Everything is float32, no operation is fused, and every output equals the NumPy restatement
 * (tests/merge_cases.py) byte for byte.
 *
 * d3f_volume_merge_select -- one elementwise pass over whole volumes.
 *   per side      dist float32 [nx,ny,nz], valid uint8 [nx,ny,nz], weight float32 [nx,ny,nz] or NULL: then the side's scalar weight
 *                 (weight_a_all / weight_b_all) applies to every voxel.  With a weight volume the scalar is not read.
 *   scalars       w_max in (0, +inf] (+inf: no cap);  gap in [0, +inf] (+inf: never reset), a length in dist's units.
 *   usable        a side is usable at q iff valid[q] != 0, dist[q] is not NaN and 0 < w[q] < +inf (a NaN weight is not usable).
 *                 dist and weight of a voxel with valid == 0 are NEVER read: they may hold NaN or 0xA5.
 *   out_kind      one byte per voxel, with da / db the distances, wa / wb the weights:
 *                   0 D3F_MERGE_NONE   neither side usable             out_dist 1e3 (the library's sentinel), out_weight 0, out_beta 0, out_valid 0
 *                   1 D3F_MERGE_KEEP   only a usable                   out_dist da, out_weight wa, out_beta 0, out_valid 1
 *                   2 D3F_MERGE_NEW    only b usable                   out_dist db, out_weight wb, out_beta 1, out_valid 1
 *                   3 D3F_MERGE_BLEND  both, not fabsf(da - db) > gap  s = wa + wb;  beta = wb / s (one IEEE division);
 *                                                                      out_dist da + beta*(db - da) (three roundings, exact where da == db);
 *                                                                      out_weight min(s, w_max);  out_beta beta;  out_valid 1
 *                   4 D3F_MERGE_RESET  both, fabsf(da - db) > gap      out_dist db, out_weight wb, out_beta 1, out_valid 1
 *                 Where s overflows to +inf, beta = 0 and out_weight = w_max.  Kinds 1, 2 and 4 copy bits.  A NaN the arithmetic of kind 3
 *                 itself produces (infinite distances of equal sign) has no specified payload.
 *   Every output volume is written whole.  One launch, one lane per voxel; no atomics, no workspace.
 *
 * d3f_volume_merge_rows -- the rows of m listed destination voxels, from `kind` and `beta` as select wrote them.
 *   voxels        int32 [m], any order, duplicates allowed; NULL: every voxel in flat order, m must be nx*ny*nz.  An entry outside the
 *                 volume gets fill rows and out_known = 0 (the conventions of d3f_volume_warp_rows).
 *   sets          n_sets in 0..D3F_MAX_MAPS pairs (sets_a[s], sets_b[s]) with equal C.  Each side is dense (band NULL: the row of q at
 *                 q*stride_voxel) or banded (the row at slot[q]*stride_voxel, none where slot[q] < 0; cell_band is not read).  Each set is
 *                 stored as D3F_DTYPE_F32 or D3F_DTYPE_F16 (the storage word of d3f_volume_set, stride_voxel in elements); a half is
 *                 widened exactly and the outputs are always float32.  These are new row loops with a half form of their own: the rule of
 *                 d3fields_hip.h that the entry points outside the lookups need float32 rows does not bind this one.
 *   rows used     a has a row at q iff kind[q] is 1 or 3 and (a is dense or slot_a[q] >= 0);
 *                 b has a row at q iff kind[q] is 2, 3 or 4 and (b is dense or slot_b[q] >= 0).
 *   result        both rows (kind 3 only): out_c = a_c + beta[q]*(b_c - a_c) per channel, three roundings;
 *                 exactly one row: that row, bit for bit as the widening gives it (-0 and NaN payloads stay);
 *                 no row: sets_a[s].fill (NULL: zeros) and out_known = 0; otherwise out_known = 1.  sets_b[s].fill is not read.
 *   out_sets[s]   float32 [m, C], C-contiguous; out_known one byte per listed voxel.
 *   A banded side with n_rows == 0: its slot, cell_band and every data of that side may be NULL, nothing of it is read.
 *   m == 0: D3F_OK, nothing is read.  The 16-byte vector / scalar rule (a pair moves as vectors when both sets and the output row do), the
 *   boundary between <= 16 and wider channel counts (one lane / sixteen lanes per voxel) and stride_voxel >= C are as in
 *   d3f_volume_sample.  One launch; no LDS, no atomics, no workspace; two runs give identical bytes.
 *
 * Status errors, nothing launched, in this order of precedence -- struct, shape, scalars, NULL pointers, layout:
 *   D3F_ERR_INVALID_ARG  a NULL struct; a NULL required pointer; m < 0; voxels NULL with m != nx*ny*nz; a scalar weight that is not finite
 *                        and > 0 where that side's weight volume is NULL; w_max NaN or <= 0; gap NaN or < 0; a `reserved` word != 0;
 *   D3F_ERR_BAD_SHAPE    an extent below 2, more than 2^31 - 1 voxels; n_sets or a C out of range; sets_a[s].C != sets_b[s].C; a band's
 *                        n_rows outside [0, 2^31 - 1];
 *   D3F_ERR_BAD_DTYPE    a storage word other than 0 / 1;
 *   D3F_ERR_BAD_LAYOUT   stride_voxel < C; a pointer not aligned to its element. */
#define D3F_MERGE_NONE 0
#define D3F_MERGE_KEEP 1
#define D3F_MERGE_NEW 2
#define D3F_MERGE_BLEND 3
#define D3F_MERGE_RESET 4
typedef struct d3f_merge_select {
    int32_t nx, ny, nz;
    int32_t reserved;          /* 0 */
    const float *dist_a;
    const uint8_t *valid_a;
    const float *weight_a;     /* NULL: weight_a_all everywhere */
    const float *dist_b;
    const uint8_t *valid_b;
    const float *weight_b;     /* NULL: weight_b_all everywhere */
    float weight_a_all, weight_b_all;
    float w_max, gap;
    float *out_dist;
    float *out_weight;
    float *out_beta;
    uint8_t *out_valid;
    uint8_t *out_kind;
} d3f_merge_select;
typedef struct d3f_merge_rows {
    int32_t nx, ny, nz;
    int32_t n_sets;
    const d3f_band *band_a;    /* NULL: a is dense */
    const d3f_band *band_b;    /* NULL: b is dense */
    const d3f_volume_set *sets_a;
    const d3f_volume_set *sets_b;
    const uint8_t *kind;
    const float *beta;
    const int32_t *voxels;
    int64_t m;
    void *const *out_sets;
    uint8_t *out_known;
    int64_t reserved;          /* 0 */
} d3f_merge_rows;
int d3f_volume_merge_select(const d3f_merge_select *args, void *stream);
int d3f_volume_merge_rows(const d3f_merge_rows *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D3FIELDS_HIP_EXT_H */
