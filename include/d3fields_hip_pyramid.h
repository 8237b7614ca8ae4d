/*
 * d3fields_hip_pyramid.h -- the pyramid of a baked field and the seeded flow: entry points of libd3fields_hip.so added after the main table
 * of ABI 16 (include/d3fields_hip.h) and after the extension header (include/d3fields_hip_ext.h).
 *
 * Both older headers are closed: host tests pin the functions they declare, so neither gets a further declaration.  A feature added since
 * brings a header of its own, and this is the first.  Its entry points are exported by the same libd3fields_hip.so, follow the conventions
 * at the top of d3fields_hip.h (device pointers, no allocation, nothing retained, work enqueued on `stream` and not synchronised,
 * outputs and poisoned inputs may hold anything, D3F_OK or a negative D3F_ERR_* code with d3f_last_error()), and D3F_ABI_VERSION
 * stays 16: a library that has the main table and lacks a symbol of this header is an older build of the same ABI.
 */
#ifndef D3FIELDS_HIP_PYRAMID_H
#define D3FIELDS_HIP_PYRAMID_H

#include "d3fields_hip.h" /* d3f_volume_set, d3f_band, D3F_MAX_MAPS, D3F_FLOW_MAX_RADIUS, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* How far did it move?  A baked field at half the resolution (csrc/pyramid_kernels.hip).  Everything is float32, one
 * rounding per operation, nothing is contracted, and every output equals the NumPy restatement (tests/pyramid_cases.py) byte for byte.
 *
 * GRID.  The fine grid is nx x ny x nz, z fastest, flat index q = (x*ny + y)*nz + z, every extent in [1, D3F_EDT_MAX_EXTENT], at most
 * 2^31 - 1 voxels.  The coarse grid has cx = (nx + 1)/2, cy = (ny + 1)/2, cz = (nz + 1)/2 voxels, flat index Q = (X*cy + Y)*cz + Z.  The
 * CHILDREN of coarse voxel (X, Y, Z) are the fine voxels (2X + i, 2Y + j, 2Z + k), i, j, k in {0, 1}, that lie inside the fine volume,
 * numbered c = 4i + 2j + k: ascending c is ascending fine flat index.  (With voxel 0 centred at `origin`, the coarse field has step 2*step
 * and origin + step/2; the C level knows no origin.)
 *
 * d3f_volume_coarsen_select -- one pass; every coarse output is written whole.
 *   inputs        dist float32 [nx,ny,nz], valid uint8 [nx,ny,nz] of the fine field; min_children in 1..8.
 *   usable        a child is usable iff valid != 0 and dist is not NaN.  dist of a child that is not valid is NEVER read: it may hold NaN
 *                 or 0xA5.
 *   out_children  uint8 [cx,cy,cz]: bit c is set iff child c lies inside the fine volume and is usable;  count = popcount(out_children).
 *   out_valid     uint8 [cx,cy,cz]: count >= min_children.
 *   out_dist      float32 [cx,cy,cz]: where out_valid, fl(sum * inv) with sum ONE float32 accumulator that starts at +0 and adds the usable
 *                 children's dist in ascending c, and inv = fl(1.0f / (float)count), one IEEE division per voxel; elsewhere 1e3, the
 *                 library's sentinel.  A NaN the arithmetic itself produces (infinite distances of both signs) has no specified payload.
 *   One launch, one lane per coarse voxel; no LDS, no atomics, no workspace.
 *
 * d3f_volume_coarsen_rows -- the rows of m listed COARSE voxels, from `children` as select wrote it, with the conventions of
 * d3f_volume_merge_rows.
 *   voxels        int32 [m] coarse flat indices, any order, duplicates allowed; NULL: every coarse voxel in flat order, m must be
 *                 cx*cy*cz.  An entry outside the coarse volume gets fill rows and out_known = 0.
 *   sets          n_sets in 0..D3F_MAX_MAPS sets of the FINE field, dense (band NULL: the row of q at q*stride_voxel) or banded (the row at
 *                 slot[q]*stride_voxel, none where slot[q] < 0; cell_band is not read).  Each set is stored as D3F_DTYPE_F32 or
 *                 D3F_DTYPE_F16 (the storage word of d3f_volume_set, stride_voxel in elements); a half is widened exactly and the outputs
 *                 are always float32.  These are new row loops with a half form of their own: the rule of d3fields_hip.h that the entry
 *                 points outside the lookups need float32 rows does not bind this one.
 *   contributes   child c of Q contributes iff bit c of children[Q] is set, the child lies inside the fine volume (a bit of a child outside
 *                 is ignored) and the source is dense or slot[child] >= 0.  n_r is the number of contributors.
 *   result        n_r > 0: per channel fl(acc * fl(1.0f / (float)n_r)), acc ONE float32 accumulator that starts at +0 and adds the
 *                 contributors' channel in ascending c (a child that does not contribute adds +0, which changes no bit); out_known = 1.
 *                 n_r == 0: sets[s].fill (NULL: zeros) and out_known = 0.  A NaN the arithmetic produces has no specified payload.
 *   out_sets[s]   float32 [m, C], C-contiguous; out_known one byte per listed voxel.
 *   A banded source with n_rows == 0: its slot, cell_band and every data may be NULL, nothing of it is read.
 *   m == 0: D3F_OK, nothing is read.  The 16-byte vector / scalar rule (a set moves as vectors when its rows and the output row do: a half
 *   source steps by eight channels, a float32 source by four), the boundary between <= 16 and wider channel counts (one lane / sixteen
 *   lanes per voxel) and stride_voxel >= C are as in d3f_volume_sample.  One launch; no LDS, no atomics, no workspace; two runs give
 *   identical bytes.
 *
 * Status errors of both, nothing launched, in this order of precedence -- struct, shape, scalars, NULL pointers, layout:
 *   D3F_ERR_INVALID_ARG  a NULL struct; a NULL required pointer; min_children outside 1..8; m < 0; voxels NULL with m != cx*cy*cz; a
 *                        `reserved` word != 0;
 *   D3F_ERR_BAD_SHAPE    an extent outside [1, D3F_EDT_MAX_EXTENT], more than 2^31 - 1 voxels; n_sets or a C out of range; the band's
 *                        n_rows outside [0, 2^31 - 1];
 *   D3F_ERR_BAD_DTYPE    a storage word other than 0 / 1;
 *   D3F_ERR_BAD_LAYOUT   stride_voxel < C; a pointer not aligned to its element. */
typedef struct d3f_coarsen_select {
    int32_t nx, ny, nz;        /* the FINE grid */
    int32_t min_children;      /* 1..8 */
    const float *dist;
    const uint8_t *valid;
    float *out_dist;           /* the three outputs: [cx,cy,cz] */
    uint8_t *out_valid;
    uint8_t *out_children;
    int64_t reserved;          /* 0 */
} d3f_coarsen_select;
typedef struct d3f_coarsen_rows {
    int32_t nx, ny, nz;        /* the FINE grid */
    int32_t n_sets;
    const d3f_band *band;      /* NULL: the source is dense */
    const d3f_volume_set *sets;
    const uint8_t *children;   /* [cx,cy,cz] */
    const int32_t *voxels;     /* coarse flat indices, or NULL */
    int64_t m;
    void *const *out_sets;
    uint8_t *out_known;
    int64_t reserved;          /* 0 */
} d3f_coarsen_rows;
int d3f_volume_coarsen_select(const d3f_coarsen_select *args, void *stream);
int d3f_volume_coarsen_rows(const d3f_coarsen_rows *args, void *stream);

/* The seeded flow (csrc/flow_seeded_kernels.hip): d3f_volume_flow's contract word for word -- volume, site, slot,
 * set, member, cost chain, takes part, outputs, axis cost: see d3fields_hip.h -- with ONE change: the window of every member is centred on
 * a per-voxel predicted offset.
 *   seed         int32 [n, 3] in voxels, (sx, sy, sz) of voxel v at seed + 3v; NULL: zeros.  The seed of a voxel that is no member of A is
 *                NEVER read: it may hold 0xA5.
 *   candidates   of member v: u = v + seed[v] + (dx, dy, dz) with |dx|, |dy|, |dz| <= radius, u inside the volume (spatially: nothing wraps)
 *                and a member of B.  A candidate outside the volume takes no part.
 *   key          (s, d2, j) with d2 = dx^2 + dy^2 + dz^2 and j = ((dx + r)*(2r + 1) + (dy + r))*(2r + 1) + (dz + r) taken from (dx, dy, dz),
 *                the offset from the SEEDED centre: ties go to the candidate nearest the prediction, then to the lower flat index.  The
 *                packed 64-bit key is d3f_volume_flow's.
 *   range        a member whose seed has a component outside [-D3F_FLOW_SEED_MAX, D3F_FLOW_SEED_MAX] has no candidate: target -1, cost
 *                +Inf.  The kernel tests this before any address arithmetic.
 *   out_axis_cost  d3f_volume_flow's rule, which depends on the target alone (the same kernel).
 * With seed NULL or all zero the three outputs equal d3f_volume_flow's byte for byte.
 * One lane per candidate: each lane runs its candidate's chain over the channels, every lane of a voxel reads the same A row, and the
 * voxel's winner is the minimum of the packed keys across its lanes.  A wave takes 64 consecutive voxels and its members in turn (two at a
 * time at radius 1).  No LDS, no atomics, no workspace; two runs give identical bytes.
 * Status errors, nothing launched: a NULL struct, then d3f_volume_flow's checks and codes in its order -- NULL site_a / site_b / set_a /
 * set_b / a set's data / out_target / out_cost, radius outside 1..D3F_FLOW_MAX_RADIUS, a NaN max_cost2, reserved != 0
 * (D3F_ERR_INVALID_ARG); an extent outside [1, 16384], more than 2^31 - 1 voxels, C out of range or different in the two sets
 * (D3F_ERR_BAD_SHAPE); a set stored as half, as for d3f_volume_flow, or any other storage word than 0 (D3F_ERR_BAD_DTYPE); a stride_voxel
 * < C, a slot, seed, data or output not 4-byte aligned (D3F_ERR_BAD_LAYOUT). */
#define D3F_FLOW_SEED_MAX 16384
typedef struct d3f_flow_seeded {
    const uint8_t *site_a;
    const int32_t *slot_a;     /* NULL: A is dense */
    const d3f_volume_set *set_a;
    const uint8_t *site_b;
    const int32_t *slot_b;     /* NULL: B is dense */
    const d3f_volume_set *set_b;
    const int32_t *seed;       /* [n, 3], or NULL: zeros */
    int32_t nx, ny, nz;
    int32_t radius;
    float max_cost2;
    int32_t reserved;          /* 0 */
    int32_t *out_target;
    float *out_cost;
    float *out_axis_cost;      /* NULL to skip */
} d3f_flow_seeded;
int d3f_volume_flow_seeded(const d3f_flow_seeded *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D3FIELDS_HIP_PYRAMID_H */
