/*
 * d3fields_hip.h -- C ABI of libd3fields_hip.so (MI355X / gfx950).
 *
 * The reference (WangYixuan12/d3fields) has no native/FFI layer: its hot path is the Python
 * method surface of `class Fusion` (fusion.py:202) plus utils/corr_utils.py, executed as
 * torch ops.  This header is the boundary a maintainer binds instead of those torch ops;
 * each entry point names the reference lines it replaces.  INTEGRATION.md shows the ctypes
 * stub that goes into fusion.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the device the stream belongs to, unless noted;
 *   - the library never allocates, frees or retains caller memory, reads no environment variable and keeps no
 *     state between calls (re-entrant), with two documented thread-local exceptions: the text behind
 *     d3f_last_error() and the one-shot event pair armed by d3f_profile_next_eval() (a measurement
 *     hook, consumed by the same thread's next query); work is enqueued on `stream` (a
 *     hipStream_t, NULL = default stream) and NOT synchronised;
 *   - a workspace or an output may hold ANYTHING when it is handed over (a fresh hipMalloc, the leftovers of another
 *     call): every call clears or writes what it reads, on `stream`.  The exceptions are stated where they apply and are
 *     these: the point order and gate words under D3F_FLAG_REUSE_POINT_ORDER, the words of D3F_CHECK_WORDS_ARE_ZERO,
 *     out_dims[3] of d3f_lattice_probe, the state block and skip words of d3f_volume_align_step, the workspace
 *     d3f_pose_consensus_select and d3f_volume_geodesic_relax take over from the call before them, the Adam state of
 *     d3f_rigid_update and the scratch of d3f_track_step (tests/test_gpu_dirty_buffers.py);
 *   - all tensors fp32, C-contiguous unless strides are part of the signature;
 *   - return value: D3F_OK or a negative D3F_ERR_* code; d3f_last_error() gives the text of
 *     the calling thread's last failure.  Nothing aborts.
 */
#ifndef D3FIELDS_HIP_H
#define D3FIELDS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3F_ABI_VERSION 16

#define D3F_OK 0
#define D3F_ERR_INVALID_ARG (-1)  /* null pointer, negative count, bad enum               */
#define D3F_ERR_BAD_SHAPE (-2)    /* V/H/W/C/fh/fw outside the supported range             */
#define D3F_ERR_BAD_DTYPE (-3)    /* channel map dtype not supported by this entry point   */
#define D3F_ERR_BAD_LAYOUT (-4)   /* stride/alignment the kernels cannot address           */
#define D3F_ERR_HIP (-5)          /* a HIP runtime call or kernel launch failed            */
#define D3F_ERR_WORKSPACE (-6)    /* workspace missing or too small                        */

#define D3F_MAX_VIEWS 64
#define D3F_MAX_MAPS 8

#define D3F_DTYPE_F32 0
#define D3F_DTYPE_F16 1 /* IEEE half STORAGE of a channel map (a data format of the producer side: DINOv2 run in   \
                           fp16, fusion.py:203,227,616).  Texels are widened to fp32 on load and every operation of \
                           the query stays fp32, so the result equals the fp32 query on the widened map bit for bit  \
                           at half the texel traffic.  Strides stay in ELEMENTS.                                    */

/* d3f_eval flags */
#define D3F_FLAG_FINITE_MAPS 1u /* caller has verified that depth and every channel map hold   \
                                   only finite values: views that are invalid for a point are \
                                   then skipped instead of multiplied by 0 (identical results; \
                                   without the flag 0*NaN / 0*Inf propagate as in the          \
                                   reference, fusion.py:385).  Device-side alternative without \
                                   a host sync: d3f_map_check + the `nonfinite` words below.   */
#define D3F_FLAG_REFERENCE_ROUNDING 4u /* every operation in the reference's own order, also for wide maps.  By default a   \
                                          wide map (more than 256 bytes per texel) takes, for finite operands, the FOLDED  \
                                          form: the view weight and the reciprocal of the view count are multiplied into   \
                                          the four bilinear weights once per (point, view) and the channels run four fma   \
                                          per view -- within a few ulp of the reference's order      \
                                          (1e-5 relative is the contract, ~2e-7 measured).  'dist', 'valid_mask', thin     \
                                          maps (instance masks, colours) and '<k>_inter' are in the reference's order and  \
                                          bit-exact either way.  Slower: the direct gather, no view skipping.              */
/* The planner's thresholds that the two point-order flags below refer to (csrc/d3f_plan.h defines its constants from them; a caller
 * that sets the flags only where they are honoured compares against the same numbers).  Points, and bytes of all requested maps together. */
#define D3F_PLAN_SMALL_BATCH 65536                /* fewer points: caller order, neither flag is looked at                      */
#define D3F_PLAN_WINDOW_CLOUD_MIN 262144          /* a cloud of at least this many points is always walked in Hilbert order    */
#define D3F_PLAN_CACHE_RESIDENT_BYTES 67108864    /* 64 MiB: maps up to this size are "small" (caller order by default)        */
#define D3F_PLAN_INFINITY_CACHE_BYTES 268435456   /* 256 MiB: maps up to this size fit the Infinity Cache                      */
#define D3F_FLAG_UNORDERED_POINTS 2u /* the caller's point order has no spatial locality (shuffled or \
                                        uniformly random cloud; see d3f_point_order_locality): walk the \
                                        points in Hilbert order even when the maps are small (at most   \
                                        D3F_PLAN_CACHE_RESIDENT_BYTES; of at least D3F_PLAN_SMALL_BATCH \
                                        points).  Performance only -- results never depend on it.       */
#define D3F_FLAG_LOCAL_POINTS 128u /* (ABI 6) the caller's point order HAS spatial locality (d3f_points_probe: the mean step between \
                                      consecutive points is a small fraction of the cloud's extent -- a mesh, a scan, the surface    \
                                      points of a lattice in flat-index order): a cloud too small for the window kernel (fewer than  \
                                      D3F_PLAN_WINDOW_CLOUD_MIN points) on maps that fit the Infinity Cache (at most                 \
                                      D3F_PLAN_INFINITY_CACHE_BYTES) keeps the caller's order -- the Hilbert sort (five launches)    \
                                      costs more than it saves there.  Performance only.                                            */
#define D3F_FLAG_REUSE_POINT_ORDER 8u /* `workspace` still holds the point order that an earlier d3f_eval call wrote  \
                                         for the SAME pts / n (a static grid queried every frame): do not rebuild it   \
                                         (~0.12 ms per 1 M points).  Any permutation of 0..n-1 gives the same results; \
                                         a buffer that holds anything else is the caller's error.                      */

/* Tuning bits of `flags` (performance experiments; results never depend on them):
 *   bits 8..11  log2 of the points per workgroup (2..8), 0 = automatic
 *   bit  12     invert the default XCD mapping (default: XCD-contiguous tile ranges on the Hilbert walk,
 *               round-robin otherwise)
 *   bit  13     never reorder points, even when a workspace is supplied
 *   bit  14     always reorder points when a workspace is supplied
 *   bit   4     D3F_TUNE_DIRECT_GATHER: the plain direct gather in the chosen point order -- no LDS texel windows, no cell
 *               runs, no channel slices, thin maps view by view.  Every fast path is bit-identical to it (tests/).
 *   bit   5     D3F_TUNE_NO_WINDOW_GATE: a cloud never gets the gated pair of launches (LDS texel windows / cell runs chosen by a
 *               device-side probe, ABI 5): cell runs only.  bit 6  D3F_TUNE_WINDOW_SIDE: the gate always opens the window side.
 *   bits 24..25 ignored (round 1: the cell size of the point order; the ordering sizes its cells itself);  bit 26 / 27 force batched / load-use corner loads;
 *               bit 28 do not precompute corner set-ups in phase A;  bits 29..31 XCD-mapping chunk = 1024 << (k-1) tiles
 *   bits 16..23 extra dynamic LDS per workgroup in KiB (throttles workgroups per CU); 255 = none      */
#define D3F_TUNE_TILE_LOG2(k) (((uint32_t)(k) & 0xFu) << 8)
#define D3F_TUNE_XCD_REMAP (1u << 12)
#define D3F_TUNE_NO_REORDER (1u << 13)
#define D3F_TUNE_FORCE_REORDER (1u << 14)
#define D3F_TUNE_DIRECT_GATHER (1u << 4)
#define D3F_TUNE_NO_WINDOW_GATE (1u << 5)
#define D3F_TUNE_WINDOW_SIDE (1u << 6)
#define D3F_TUNE_LDS_PAD_KIB(k) (((uint32_t)(k) & 0xFFu) << 16)

/* Calibrated views: the part of Fusion.curr_obs_torch read by every query
 * (fusion.py:210-215, 707-712): 'depth' (V,H,W), 'K' (V,3,3), 'pose' (V,3,4) world->camera. */
typedef struct d3f_views {
    int32_t V, H, W;
    const float *depth; /* [V,H,W]                                                     */
    const float *K;     /* [V,3,3]                                                     */
    const float *pose;  /* [V,3,4]                                                     */
    const uint32_t *depth_nonfinite; /* NULL, or the device word d3f_map_check wrote for `depth` (ABI 4, see below) */
} d3f_views;

/* One channels-last per-view map: curr_obs_torch['dino_feats'|'mask'|'color_tensor'|...]
 * (fusion.py:373 passes these as .permute(0,3,1,2) views; here the channels-last storage is
 * addressed directly).  Element (v,y,x,c) lives at data[v*stride_v + y*stride_y + x*stride_x + c]
 * (strides in ELEMENTS; the channel stride must be 1). */
typedef struct d3f_channel_map {
    const void *data;
    int32_t fh, fw, C;
    int32_t dtype; /* D3F_DTYPE_F32 or D3F_DTYPE_F16 */
    int64_t stride_v, stride_y, stride_x;
    const uint32_t *nonfinite; /* NULL, or the device word d3f_map_check wrote for this map (ABI 4, see below) */
} d3f_channel_map;

/* Device-side replacement of the caller's `torch.isfinite(map).all()` (the precondition of D3F_FLAG_FINITE_MAPS):
 * one streaming pass over the V x fh x fw x C elements of `map` (16-byte loads, no temporaries) that leaves
 * *word_out != 0 iff the map holds a NaN or an Inf.  Enqueued on `stream`, NO host synchronisation: hand the word to the
 * queries through d3f_channel_map::nonfinite (for the depth images: describe them as a one-channel map {depth, H, W, 1,
 * F32, H*W, W, 1} and pass the word as d3f_views::depth_nonfinite).  A query whose depth and maps ALL carry a word reads
 * the words on the device and takes the exact invalid-view skip iff all are zero -- the same results as with / without
 * D3F_FLAG_FINITE_MAPS set by a host that looked, but capturable in a HIP graph and without the ~2 ms of ATen kernels +
 * host sync per new 1.9 GB map.  A caller that rewrites a map in place re-runs the check (on the same stream order).
 * word_out: one device uint32, 4-byte aligned; the call overwrites it. */
int d3f_map_check(const d3f_channel_map *map, int32_t V, uint32_t *word_out, void *stream);

/* ABI 5.  The same for n <= D3F_MAX_MAPS + 1 tensors in ONE launch (the per-frame refresh of a tracking loop checks depth +
 * features + mask: one launch instead of six): maps[k] with views[k] views leaves its verdict in *words_out[k].
 * D3F_CHECK_WORDS_ARE_ZERO: the caller hands over words that are zero already (fresh slots of a zeroed buffer), which saves
 * the clearing launch; without it the call zeroes them first.  A tensor that is not one contiguous 16-byte aligned block is
 * checked by its own d3f_map_check launch inside the call. */
#define D3F_CHECK_WORDS_ARE_ZERO 1u
int d3f_map_check_many(const d3f_channel_map *maps, const int32_t *views, int32_t n, uint32_t *const *words_out, uint32_t flags,
                       void *stream);

/* ABI 9.  A channel map through a linear head: dst[v,y,x,j] = sum_c src[v,y,x,c] * W[j,c], so that a query of k projected
 * channels (a PCA of the descriptors, a policy's 16..64-d head) reads a k-channel map instead of writing C-wide rows: fusion
 * is linear in the channel vector, (sum_v s_v bilinear(map_v) - mean) W^T = sum_v s_v bilinear(map_v W^T) - mean W^T.
 * src is read as stored (fp32, or fp16 widened exactly, explicit strides, texel stride >= C); W is [k,C] row-major fp32 on
 * the device, dst a contiguous [V,fh,fw,k] fp32 buffer, 1 <= k <= D3F_MAX_PROJECTION, any C >= 1.  Dense
 * multiply-accumulate over all C channels in a fixed order: fp32 products in short fp32 fmaf chains (4 or 16 channels), whose
 * sums are added in float64 and rounded to fp32 once.  No term is skipped for a zero weight (a NaN texel makes its k outputs
 * NaN), no atomics: two runs are bit-identical.  A source whose base pointer is not 16-byte aligned (8 for fp16) or whose
 * strides are not multiples of 4 elements is read by scalar loads: correct, but well below the streaming rate.  Enqueued on
 * `stream`, no host synchronisation. */
#define D3F_MAX_PROJECTION 64
int d3f_project_maps(const d3f_channel_map *src, int32_t V, const float *W, int32_t k, float *dst, void *stream);

/* ABI 10.  Weighted moments of M rows of C channels, the device half of a PCA fit: with weights
 * w_m >= 0 (NULL = all ones; [M] fp32 on the device),
 *     wsum = sum_m w_m,   mean_c = sum_m w_m x_mc / wsum,   scatter_ij = sum_m w_m (x_mi - mean_i)(x_mj - mean_j),
 * written as float64 on the device: wsum_out one double, mean_out [C], scatter_out [C,C] row-major with BOTH triangles.
 * rows is fp32, or fp16 widened exactly; element (m,c) lives at rows[m*row_stride + c], row_stride >= C in ELEMENTS, so a
 * contiguous channels-last map [V,fh,fw,C] is M = V*fh*fw rows and so are the [N,C] rows a query wrote.  1 <= C <=
 * D3F_MAX_MOMENT_CHANNELS, M >= 1.  Arithmetic: column sums in fp32 fmaf chains of 32 rows folded in float64; the rows
 * centred at fp32(mean) in fp32, products and chains of 64 rows on v_mfma_f32_16x16x4_f32 (exact fp32), chain sums folded in
 * float64 in a fixed order, the shift from fp32(mean) to mean corrected exactly.  Dense: a row with w == 0 still takes part
 * (0 * NaN = NaN, as in d3f_project_maps), a NaN or Inf in a row makes the affected outputs non-finite, wsum == 0 gives NaN
 * means.  No atomics: two runs are bit-identical, and scatter is bitwise symmetric.  A base pointer that is not 16-byte
 * aligned (8 for fp16) or a row_stride that is not a multiple of 4 elements is read by scalar loads: correct, but slow.
 * workspace: d3f_row_moments_workspace_bytes(M, C) bytes on the device, 16-byte aligned (0 for arguments out of range);
 * its contents need not be preserved.  Enqueued on `stream`, no host synchronisation. */
#define D3F_MAX_MOMENT_CHANNELS 2048
int64_t d3f_row_moments_workspace_bytes(int64_t M, int32_t C);
int d3f_row_moments(const void *rows, int32_t dtype, int64_t M, int32_t C, int64_t row_stride,
                    const float *weights /* NULL = all ones; [M], >= 0 */,
                    double *wsum_out /* 1 */, double *mean_out /* [C] */, double *scatter_out /* [C,C] */,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ---- library ---------------------------------------------------------------------- */
int d3f_abi_version(void);
const char *d3f_version(void);    /* "d3fields-hip <semver> gfx950" (host memory)          */
const char *d3f_last_error(void); /* host memory, valid until the thread's next failure    */
/* 1 when the library was compiled with -DD3F_EXPERIMENTS (tuning sessions: D3F_EXP_* environment variables select
 * kernel variants); 0 for the product build, which reads no environment variable at all. */
int d3f_build_has_experiments(void);

/* ---- fused field query --------------------------------------------------------------
 * Replaces Fusion.eval (fusion.py:305-394) together with project_points_coords
 * (fusion.py:32-55) and interpolate_feats (fusion.py:57-77); one launch covers any N, so it
 * also replaces the 60 000-point chunk loop + torch.cat of Fusion.batch_eval (fusion.py:526-545).
 *   pts        [n,3]
 *   maps       n_maps descriptors (host array), one per entry of `return_names`
 *   out_dist   [n]      'dist'        out_valid [n] (0/1 bytes) 'valid_mask'
 *   out_fused  host array of n_maps device pointers, [n,C_k] each
 *   out_inter  NULL, or host array of n_maps device pointers (entries may be NULL),
 *              [V,n,C_k] each: the reference's '<k>_inter' (return_inter=True, fusion.py:389)
 * The [n,C_k] rows are written once with non-temporal stores (they do not stay in the GPU's caches); like any kernel output
 * they are visible to whatever follows the call in `stream` order.
 */
int d3f_eval(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps,
             int32_t n_maps, float mu, uint32_t flags, float *out_dist, uint8_t *out_valid,
             float *const *out_fused, float *const *out_inter, void *workspace,
             int64_t workspace_bytes, void *stream);

/* Optional device scratch for d3f_eval (NULL/0 is always accepted).  With at least
 * d3f_eval_workspace_bytes(n) bytes the library may walk the points in a cache-friendlier
 * (Hilbert) order when the maps are much larger than the caches or the caller declares the points
 * unordered; outputs are unaffected. */
int64_t d3f_eval_workspace_bytes(int64_t n);
/* (ABI 6) Scratch for the DISTANCE-ONLY query (n_maps == 0; reference: batch_eval(pts, return_names=[]), vis_repr.py:93): with at
 * least this many bytes of workspace d3f_eval first copies the depth maps into tiles of 4 x 8 pixels (one cache line each) and looks
 * the nearest pixels up there -- consecutive query points of a grid column are neighbours along an image column, four cache lines per
 * four lanes in a row-major map.  0: the batch is too small for that to pay (< 2^22 points) or has more than 8 views.  Outputs are
 * unaffected; the workspace may be reused as soon as the call's work in `stream` is done. */
int64_t d3f_eval_dist_workspace_bytes(const d3f_views *views, int64_t n);

/* ABI 5.  For a CLOUD of >= 262 144 points in the Hilbert order on a patch-resolution wide map d3f_eval enqueues TWO fused
 * launches -- the LDS texel-window kernel and the cell-run kernel -- behind one device word: a probe kernel counts, over
 * D3F_GATE_SAMPLES evenly spaced 64-point tiles of the order, those whose touched texels fit the window kernel's pool, and the
 * workgroups of the side that lost return at once (no host sync; which kernel suits a cloud depends on its density against the
 * texel grid, which only the device knows).  The word lives in the workspace: uint32 at byte offset d3f_eval_gate_offset(n);
 * after the call has completed, a value >= D3F_GATE_MIN_FIT means the window kernel ran.  Diagnostics only. */
#define D3F_GATE_SAMPLES 128
#define D3F_GATE_MIN_FIT 96
int64_t d3f_eval_gate_offset(int64_t n);

/* Measurement hook: the calling thread's NEXT d3f_eval / d3f_eval_dist records these two hipEvent_t
 * (NULL = none) on its stream immediately before and after the fused kernel launch, i.e. around the
 * dominant kernel only (not the optional point-ordering kernels).  One-shot. */
void d3f_profile_next_eval(void *start_event, void *stop_event);

/* What d3f_eval would launch for these shapes (no device work; usable without a GPU): the launch
 * geometry and the per-map lane mapping the host logic picked.  For tests and tuning. */
#define D3F_KERNEL_NAME_MAX 80
typedef struct d3f_eval_plan {
    int32_t tile_points;                    /* query points per 256-thread workgroup                  */
    int32_t reorder;                        /* 1: points are walked in Hilbert order (sorted keys); 2: closed-form brick
                                               walk of a lattice (d3f_eval_grid / d3f_eval_lattice)    */
    int32_t lds_bytes;                      /* dynamic LDS per workgroup                              */
    int32_t reserved;                       /* legacy code of the instance `kernel` names (read `kernel` instead).  Cell-run
                                               gather: waves per SIMD the instance is built for; channel-sliced launch:
                                               100 + 10*log2(lanes per point) + views in flight; LDS texel-window kernel:
                                               2000 + 100*U + 10*VC + workgroups per CU (16 lanes per point: the number the
                                               pool is sized for); else 0.  The digits are the INSTANCE's
                                               template arguments: an experiments build whose knob asks for views in flight that no
                                               built instance has (D3F_EXP_WINDOW_VC=2 with 4 / 8 views, D3F_EXP_SLICED_VC=1 with 32 or
                                               8 lanes) reports the instance launched, where ABI 7 echoed the knob */
    int64_t workgroups;
    int32_t vector_floats[D3F_MAX_MAPS];    /* 4 / 2 / 1 floats per load                              */
    int32_t lanes_per_point[D3F_MAX_MAPS];
    int32_t vectors_per_lane[D3F_MAX_MAPS];
    int32_t staged[D3F_MAX_MAPS];           /* 0: direct gather; 3: LDS texel windows per brick (patch-resolution wide
                                               map on a lattice); 16 + K: cell-run gather with runs of K points
                                               (patch-resolution wide maps); 5: the fused rows of a 32-point brick in
                                               registers (1024-channel patch maps, round 6)            */
    int32_t gated_window;                   /* ABI 5.  1: a cloud that gets the gated pair of launches; the fields above describe
                                               the cell-run side, the window side is the lattice's window plan on 64-point tiles */
    int32_t reserved2;                      /* gated_window: the window side's `reserved` code (2000 + 100*U + 10*VC + W)       */
    int32_t family;                         /* ABI 5.  row of the planner's family table that took the query: 0 dist-only, 1 lds-window,
                                               2 cell-runs, 3 channel-sliced, 4 direct, 5 register-rows (d3f_plan_family_name;
                                               csrc/d3f_plan.h)                                                                    */
    int32_t reserved3;
    char kernel[D3F_KERNEL_NAME_MAX];       /* ABI 8.  the kernel instance the launch takes, as its symbol prints: entry point and
                                               template arguments, e.g. "fused_eval_sliced_kernel<5, 2, 7>" (written by the row of the
                                               family's variant list that also launches it, csrc/fuse_<family>.hip); "" when no
                                               built instance takes these parameters (d3f_eval would return D3F_ERR_HIP)          */
    char window_kernel[D3F_KERNEL_NAME_MAX];/* ABI 8.  gated_window: the instance on the window side of the gate; else ""          */
} d3f_eval_plan;
int d3f_eval_plan_query(const d3f_views *views, int64_t n, const d3f_channel_map *maps, int32_t n_maps,
                        uint32_t flags, int32_t have_workspace, int32_t want_inter, d3f_eval_plan *plan);
/* name of a family id ("lds-window", ...; NULL for an id outside the table), and what the row takes, as one line of text */
const char *d3f_plan_family_name(int32_t family);
const char *d3f_plan_family_takes(int32_t family);

/* ---- regular grids and keypoint selection (reference fusion.py:79-88, 1418-1475) ---------------------
 * A grid is given by its three axis coordinate arrays, exactly the `arange(lower, upper, step) + step/2`
 * tensors of create_init_grid (fusion.py:82-84) -- they are tiny, and reading them keeps the points
 * bit-identical to the reference's on any host.  Point (ix,iy,iz) has flat index (ix*ny + iy)*nz + iz
 * ('ij' meshgrid, z fastest), which is also the layout of every per-point output. */
typedef struct d3f_grid {
    const float *x, *y, *z;   /* device arrays of nx, ny, nz floats */
    int32_t nx, ny, nz;
    int32_t reserved;
} d3f_grid;

/* d3f_eval over all nx*ny*nz grid points without materialising them (replaces
 * batch_eval(create_init_grid(...)[0].to(device), ...), vis_repr.py:88-93): saves the 12 B/point read that
 * dominates a distance-only pass.  Outputs as d3f_eval, in flat grid order. */
int d3f_eval_grid(const d3f_views *views, const d3f_grid *grid, const d3f_channel_map *maps, int32_t n_maps,
                  float mu, uint32_t flags, float *out_dist, uint8_t *out_valid, float *const *out_fused,
                  void *stream);

/* d3f_eval for points that the caller has ARRANGED as a regular lattice -- pts[(ix*ny + iy)*nz + iz], e.g. the
 * materialised output of create_init_grid (fusion.py:79-88) handed to batch_eval (vis_repr.py:88-93) -- with n =
 * nx*ny*nz.  Coordinates are read from `pts` exactly as in d3f_eval and the outputs are identical; the dims only let
 * the library walk the index space brick by brick in closed form when the maps are large (no curve keys, no sort, no
 * index array, no workspace).  Any dims whose product is n are correct -- a wrong guess can only cost speed. */
int d3f_eval_lattice(const d3f_views *views, const float *pts, int32_t nx, int32_t ny, int32_t nz,
                     const d3f_channel_map *maps, int32_t n_maps, float mu, uint32_t flags, float *out_dist,
                     uint8_t *out_valid, float *const *out_fused, float *const *out_inter, void *stream);

/* d3f_eval_plan_query for d3f_eval_lattice / d3f_eval_grid launches. */
int d3f_eval_plan_query_lattice(const d3f_views *views, int32_t nx, int32_t ny, int32_t nz, const d3f_channel_map *maps,
                                int32_t n_maps, uint32_t flags, int32_t want_inter, d3f_eval_plan *plan);

/* Is pts[n,3] a z-fastest lattice (every point = (x[ix], y[iy], z[iz]) with strictly increasing axes, flat index
 * (ix*ny + iy)*nz + iz: the layout of create_init_grid, fusion.py:79-88)?  Sixteen workgroups find where the z and y
 * axes restart and 4096 evenly spaced points are compared with the implied axis values.  out_dims: FOUR device int32,
 * the caller zeroes out_dims[3] before the call; afterwards (nx, ny, nz) = out_dims[0..2] is a lattice iff out_dims[0] > 0
 * and out_dims[3] == 0 (axes longer than 65536 are not recognised).  The shim feeds the answer to d3f_eval_lattice,
 * where it only selects the walk order. */
int d3f_lattice_probe(const float *pts, int64_t n, int32_t *out_dims, void *stream);

/* Pre-filter of select_features_* (fusion.py:1430,1444): flat indices of the grid points with
 * valid_mask && |dist| < dist_thr, compacted into idx_out[0..min(count,capacity)) in ASCENDING order (the order
 * of the reference's boolean-mask indexing).  count_out: ONE device int64, the number of survivors (may exceed
 * capacity: then only the first `capacity` indices were stored).  workspace: d3f_grid_shell_workspace_bytes -- rounded up to a multiple of
 * 256 and followed by d3f_eval_dist_workspace_bytes(views, nx*ny*nz) further bytes the depth lookups of a big grid go to a tiled copy
 * (same survivors; optional). */
int64_t d3f_grid_shell_workspace_bytes(const d3f_grid *grid);
int d3f_grid_shell(const d3f_views *views, const d3f_grid *grid, float mu, float dist_thr, int64_t capacity,
                   int64_t *idx_out, int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 7) Iso-surface extraction: what fusion.py:1313-1330 does on the host with mcubes.marching_cubes, on the device.
 * volume: float32 [nx, ny, nz], z fastest (the `dist` of a grid query, flat index (ix*ny + iy)*nz + iz); valid: NULL, or one
 * byte per point (the `valid_mask` of the same query).  A corner is INSIDE when value < iso.  A cell emits when all eight corners
 * are finite and (with `valid`) valid; an edge whose endpoint is non-finite or invalid carries no vertex.
 *   vertices   exactly one per grid edge whose endpoints straddle iso and that belongs to at least one emitting cell:
 *              keys_out[i] = 3*flat(lower endpoint) + axis (0 x, 1 y, 2 z), t_out[i] = (iso - va) / (vb - va) in fp32 with the IEEE
 *              division (va = the value at the lower endpoint), a finite number in [0, 1]; stored in ASCENDING key order;
 *   triangles  int32 [M, 3] indices into the vertex array, ordered by cell (flat index of its lowest corner), inside a cell in
 *              the order of the case table (csrc/mc_table.h, generated by scripts/gen_mc_table.py: ambiguous faces cut inside
 *              corners off separately, so the mesh is closed wherever cells emit on both sides of a face); a triangle's normal
 *              points to the side where value > iso.  Degenerate triangles (a value equal to iso gives t = 0 on several edges)
 *              are emitted as the table says, NOT filtered.
 * Two runs on the same input give byte-identical arrays (no floating-point atomics, no order that depends on the dispatcher).
 * counts_out: TWO device int64, the true numbers of vertices and triangles -- also when they exceed the capacities: then
 * nothing is written beyond the capacities, what was written is unspecified, and the caller re-runs with the counts.
 * Vertex and triangle counts are 32-bit inside: nx*ny*nz <= 715827882 ((2^31 - 1) / 3 points, so neither 3 vertices per point
 * nor 5 triangles per cell can wrap), every extent >= 2, else D3F_ERR_BAD_SHAPE.  workspace: d3f_mesh_workspace_bytes, 8 bytes
 * per 1024 points plus the scan's scratch -- nothing per cell; 256-byte aligned like a hipMalloc'ed pointer (>= 4 needed). */
int64_t d3f_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_mesh_count(const float *volume, const uint8_t *valid, int32_t nx, int32_t ny, int32_t nz, float iso, int64_t *counts_out,
                   void *workspace, int64_t workspace_bytes, void *stream);
int d3f_mesh_extract(const float *volume, const uint8_t *valid, int32_t nx, int32_t ny, int32_t nz, float iso,
                     int64_t vertex_capacity, int64_t triangle_capacity, int64_t *keys_out, float *t_out, int32_t *triangles_out,
                     int64_t *counts_out, void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 7) scipy.ndimage.gaussian_filter(src, sigma, mode='reflect', truncate=truncate) of a float32 volume [nx, ny, nz] in fp32:
 * three axis passes (x, y, z), weights exp(-k^2 / (2 sigma^2)) normalised to sum 1 (formed in double on the host), radius
 * int(truncate*sigma + 0.5), boundary by reflection (d c b a | a b c d | d c b a), as often as the radius needs.  src != dst;
 * sigma > 0, truncate > 0; radius <= D3F_GAUSSIAN_MAX_RADIUS, every extent >= 1 and nx*ny*nz < 2^31, else D3F_ERR_BAD_SHAPE.
 * workspace: one more volume (d3f_volume_gaussian_workspace_bytes = 4*nx*ny*nz), 4-byte aligned. */
#define D3F_GAUSSIAN_MAX_RADIUS 64
int64_t d3f_volume_gaussian_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_volume_gaussian(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, float sigma, float truncate,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 11) A BAKED field: the regular volume d3f_eval_grid wrote (dist, valid and any channel set, flat index (ix*ny + iy)*nz + iz,
 * z fastest), read back at arbitrary points by trilinear interpolation -- eight corner rows of one array per point and no camera
 * arithmetic -- with the closed-form gradient w.r.t. the point.  It interpolates the FUSED field; it does
 * not re-fuse, so off the lattice it is not d3f_eval.
 *   origin  centre of voxel (0,0,0); step h > 0; every extent in [2, 2^24] (lattice coordinates are exact in fp32) and
 *           nx*ny*nz <= 2^31 - 1, else D3F_ERR_BAD_SHAPE;
 *   dist    float32 [nx,ny,nz]; valid: one byte per voxel (read by d3f_volume_cell_valid only);
 *   cell_valid  one byte per CELL, [nx-1,ny-1,nz-1]: the AND of the cell's eight valid bytes, written once per volume by
 *           d3f_volume_cell_valid (the samplers read this array and never `valid`).
 * Per point p, everything in fp32:
 *   g_a = (p_a - origin_a) / h (IEEE division);  inside = 0 <= g_a <= n_a - 1 for x, y, z (a NaN coordinate is not inside);
 *   i_a = min(floor(g_a), n_a - 2), t_a = g_a - i_a in [0,1] (the far face belongs to the last cell, t = 1);
 *   valid = inside && cell_valid[i_x,i_y,i_z] -- a cell with ONE invalid corner is rejected as a whole, also at t = 0;
 *   w(dx,dy,dz) = (dx ? t_x : 1-t_x) * (dy ? t_y : 1-t_y) * (dz ? t_z : 1-t_z), products left to right;
 *   out = w0*v0, then out = fma(w_c, v_c, out) over the corners (dx,dy,dz) = (0,0,1), (0,1,0), (0,1,1), (1,0,0) ... (1,1,1);
 * the same chain for dist and for every channel of every set.  Where valid is false NO corner is read (invalid voxels may hold
 * NaN): dist = 1e3 (d3f_eval's sentinel) and a set's row is its `fill` row (NULL: zeros).  At a lattice point of a valid cell the
 * weights are exactly 1 and 0 and the result equals the stored value.
 * A set: rows of C floats (1 <= C <= D3F_VOLUME_MAX_CHANNELS), voxel q at data + q*stride_voxel (stride_voxel >= C, in floats).
 * Rows move as 16-byte vectors where C % 4 == 0, stride_voxel % 4 == 0 and data / the output are 16-byte aligned, as scalars
 * otherwise; a set of up to 16 channels is sampled one lane per point, a wider one sixteen lanes per point. */
#define D3F_VOLUME_MAX_CHANNELS 4096
typedef struct d3f_volume {
    int32_t nx, ny, nz;
    float origin[3];
    float step;
    int32_t reserved;          /* 0 */
    const float *dist;
    const uint8_t *valid;
    const uint8_t *cell_valid;
} d3f_volume;
/* STORAGE of a set's rows: the word `reserved` of d3f_volume_set (the name is kept; every caller that passes 0 gets float32 rows, as before).
 *   D3F_DTYPE_F32 (0)  rows of C floats.
 *   D3F_DTYPE_F16 (1)  rows of C IEEE halves.  `data` then points at 2-byte elements (its declared type stays const float *),
 *                      stride_voxel and C stay in ELEMENTS (as the strides of d3f_channel_map do), data must be 2-byte aligned
 *                      (D3F_ERR_BAD_LAYOUT otherwise).  fill, every output row and every gradient row stay float32.
 *   any other value    D3F_ERR_BAD_DTYPE, in every entry point that takes a set.
 * Half rows are read by d3f_volume_sample, d3f_volume_sample_backward, d3f_band_sample and d3f_band_sample_backward only; every other
 * entry point that takes a set (d3f_volume_pool, d3f_volume_links, d3f_volume_flow, d3f_volume_align_accumulate, d3f_volume_warp_rows)
 * answers D3F_ERR_BAD_DTYPE for a half set and launches nothing.  Storage is per set: one call may mix float32 and half sets.
 * Numerics of a half set: each stored half is widened to float32 exactly (subnormals, +-0, +-Inf and NaN included) and then runs
 * through the unchanged chain -- out = w0*v0 (a plain multiply: a product of -0 stays -0), then fma(w_c, v_c, out) in the corner order
 * of d3f_volume_sample, and the face-weight chain of the backward -- so a lookup returns the bits the float32 lookup returns on the
 * widened rows.  The backward of a set of up to 16 channels equals the float32 backward on the widened rows bit for bit; a wider set's
 * per-lane partial sums cover other channels than the float32 form's (eight per vector, not four), so its last bits may differ from
 * it, but not between two runs.
 * Vector rule of a half set: rows move as 16-byte vectors (EIGHT channels) where C % 8 == 0, stride_voxel % 8 == 0, data is 16-byte
 * aligned and the output / gradient rows are 16-byte aligned, as scalar halves otherwise; the boundary between one lane per point
 * and sixteen lanes per point stays 16 channels. */
typedef struct d3f_volume_set {
    const float *data;
    int32_t C;
    int32_t reserved;          /* the storage word: D3F_DTYPE_F32 (0) or D3F_DTYPE_F16 (1), see above */
    int64_t stride_voxel;
    const float *fill;         /* C floats on the device, or NULL = zeros */
} d3f_volume_set;
/* cell_valid_out[(cx*(ny-1) + cy)*(nz-1) + cz] = AND of vol->valid over the cell's eight corners (vol->dist / cell_valid unused) */
int d3f_volume_cell_valid(const d3f_volume *vol, uint8_t *cell_valid_out, void *stream);
/* pts [n,3]; out_dist [n], out_valid [n] bytes, out_sets[s] = float32 [n, sets[s].C] (C-contiguous).  n_sets in [0, D3F_MAX_MAPS].
 * n == 0: D3F_OK, nothing is read (buffers may be NULL).  One launch (narrow sets only) or one launch that also walks the wide
 * sets; no allocation, no synchronisation. */
int d3f_volume_sample(const d3f_volume *vol, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets, float *out_dist,
                      uint8_t *out_valid, void *const *out_sets, void *stream);
/* grad_pts[n,a] = (1/h) * sum over dist and the sets of grad * sum_c (dw_c/dt_a) v_c: the analytic derivative of the chain
 * above for the cell the point lies in (no term for the choice of the cell); a zero row where valid is false.  grad_dist: [n] or
 * NULL; grad_sets: NULL, or n_sets pointers to float32 [n, C] (entries may be NULL).  Every row of grad_pts is written by one
 * lane: no atomics, two runs agree bit for bit. */
int d3f_volume_sample_backward(const d3f_volume *vol, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                               const float *grad_dist, const void *const *grad_sets, float *grad_pts, void *stream);

/* (ABI 13) A baked field whose channel rows exist only in a BAND around the surface.  dist, valid and
 * cell_valid of the d3f_volume stay dense; a set's rows are compacted.  For a world length band > 0 (finite), in fp32:
 *   seed     a voxel with valid && fabsf(dist) < band (strict; a NaN dist is no seed);
 *   kept     a cell with cell_valid set and at least one seed among its eight corners: cell_band, one byte per cell [nx-1,ny-1,nz-1];
 *   stored   a voxel that is a corner of at least one kept cell (so every stored voxel is valid and a kept cell has eight rows);
 *   slot[q]  the rank of voxel q among the stored voxels in ascending flat index (ix*ny + iy)*nz + iz, -1 if q is not stored: an int32
 *            volume; M = the number of stored voxels, voxels[M] the inverse list; rows are [M, C] in slot order.
 * d3f_band_mark writes cell_band_out, slot_out (both complete), voxels_out[0 .. min(M, capacity)) and *count_out = M (ONE device
 * int64, the true count also when M > capacity: then nothing is written beyond the capacity and the caller re-runs with a
 * voxels_out of M entries; capacity 0 with voxels_out NULL only counts).  vol->dist and vol->cell_valid are read (vol->valid is not:
 * a valid cell has eight valid corners; dist of an invalid cell is never read).  Four kernels and the recursive exclusive scan on
 * `stream`: order-preserving, no atomics, no spinning, two runs give byte-identical output.  workspace: d3f_band_workspace_bytes (the scan's
 * scratch, about 2 bytes per 1024 voxels; the flags are scanned inside slot_out), 4-byte aligned.  Status errors: the volume checks of
 * d3f_volume_sample, band not finite or <= 0, capacity < 0, NULL outputs, a short workspace. */
typedef struct d3f_band {
    const int32_t *slot;       /* [nx,ny,nz] */
    const uint8_t *cell_band;  /* [nx-1,ny-1,nz-1] */
    int64_t n_rows;            /* M, in [0, 2^31 - 1] */
} d3f_band;
int64_t d3f_band_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_band_mark(const d3f_volume *vol, float band, uint8_t *cell_band_out, int32_t *slot_out, int32_t *voxels_out, int64_t capacity,
                  int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream);
/* d3f_volume_sample on a banded field: g, the cell, t, the weights, out_dist and out_valid exactly as there, read from the dense
 * dist; out_in_band[i] = valid && cell_band[cell] (one byte).  sets[s].data holds the COMPACTED rows [n_rows, C], stride_voxel the
 * row stride: for an in_band point the eight corner rows are data + slot[corner]*stride_voxel (64-bit offsets), run through the same
 * chain in the same corner order -- the same bits as the dense field gives.  Any other point gets the set's fill row, and no slot or
 * row is read for it.  n_rows == 0 is legal: slot, cell_band and every data may be NULL, every point gets fill rows and nothing of the
 * band is dereferenced.  n == 0: D3F_OK, nothing is read.  Same vector / scalar row rule and the same 16-channel boundary between one
 * lane and sixteen lanes per point as d3f_volume_sample.  slot values are trusted to be < n_rows (d3f_band_mark wrote them). */
int d3f_band_sample(const d3f_volume *vol, const d3f_band *band, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                    float *out_dist, uint8_t *out_valid, uint8_t *out_in_band, void *const *out_sets, void *stream);
/* d3f_volume_sample_backward on a banded field: the dist term applies to every valid point, a set's term only to in_band points;
 * no term for the choice of the cell or for the band edge.  No atomics; two runs agree bit for bit. */
int d3f_band_sample_backward(const d3f_volume *vol, const d3f_band *band, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                             const float *grad_dist, const void *const *grad_sets, float *grad_pts, void *stream);

/* (ABI 14) The exact Euclidean distance transform of a volume of SITES.  site: one byte per voxel, [nx,ny,nz]
 * with z fastest, non-zero = site.  With v, s integer voxel coordinates:
 *   true_d2(v)   = min over the sites s of |v - s|^2; INT32_MAX when the volume has no site;
 *   cap          = max_d2 if max_d2 > 0, else INT32_MAX (no cap);
 *   out_d2[v]    = min(true_d2(v), cap);
 *   out_nearest[v] = the flat index (x*ny + y)*nz + z of A site with |v - s|^2 == true_d2(v); -1 where true_d2(v) > cap or no site
 *                  exists.  Among equidistant sites the choice is fixed by the kernels' candidate order (the z line's lower site, then
 *                  the lower y, then the lower x, each at equal distance) -- never by the order in which anything lands: there are
 *                  no atomics and two runs give identical bytes;
 *   out_dist[v]  = sqrtf((float)out_d2[v]) * step, each operation correctly rounded; +inf where out_d2[v] == INT32_MAX.
 * A positive max_d2 also bounds the search: no site farther than floor(sqrt(max_d2)) voxels along an axis is looked at.
 * Each output may be NULL (not all three).  Extents are in [1, D3F_EDT_MAX_EXTENT] (|v - s|^2 <= 3 * 16383^2 stays inside int32; an
 * extent of 1 is legal: a 2-D image is a volume with nz = 1) and the volume holds at most 2^31 - 1 voxels.
 * Three launches on `stream` (z, y, x; separable, the winning site carried through the passes); no allocation, no synchronisation.
 * workspace: d3f_volume_edt_workspace_bytes (6 bytes per voxel: one int32 and one int16 volume), 4-byte aligned; the function
 * returns 0 exactly for a shape d3f_volume_edt rejects.
 * Status errors, nothing launched: site NULL or all outputs NULL, max_d2 < 0, out_dist with a step that is not finite and > 0
 * (D3F_ERR_INVALID_ARG); a bad shape (D3F_ERR_BAD_SHAPE); an int32 / float pointer or the workspace not 4-byte aligned
 * (D3F_ERR_BAD_LAYOUT); workspace NULL or too short (D3F_ERR_WORKSPACE). */
#define D3F_EDT_MAX_EXTENT 16384
int64_t d3f_volume_edt_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_volume_edt(const uint8_t *site, int32_t nx, int32_t ny, int32_t nz, float step, int32_t max_d2, int32_t *out_d2, int32_t *out_nearest,
                   float *out_dist, void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 15) Connected components of a volume of SITES.  site: as d3f_volume_edt, one byte per voxel, [nx,ny,nz]
 * with z fastest, non-zero = site.
 *   neighbours   two sites whose integer coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1 for
 *                connectivity 6 / 18 / 26.  Neighbourhood is spatial: (x, y, nz-1) and (x, y+1, 0) are adjacent in memory and are NOT
 *                neighbours, nor are (x, ny-1, z) and (x+1, 0, z);
 *   component    a class of the transitive closure; its ROOT is its smallest flat index (x*ny + y)*nz + z, its SIZE its voxel count, its
 *                BOX the inclusive min and max of x, y and z;
 *   found        the number of components; the KEPT ones are those with size >= min_voxels, numbered 1..K in ascending order of root;
 *   out_label[v] the number of the voxel's component; 0 for a non-site or a component that is not kept;
 *   out_count    {K, found}, two int32;
 *   out_stats    row k-1 = {root, size, x0, y0, z0, x1, y1, z1} (int32) of component k, for k <= stats_capacity.  Rows beyond the capacity
 *                are not written and out_count still reports K: count, then run again with room (as d3f_band_mark).  May be NULL
 *                with stats_capacity 0.
 * Every output is a function of the input alone -- integer min, max and add only -- and two runs give identical bytes.
 * Union-find on the caller's stream (parents start at the z run, are merged lock-free with agent-scope atomic min, then flattened,
 * counted and numbered by a prefix sum); no allocation, no synchronisation.  Shapes as d3f_volume_edt: extents in
 * [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels.  workspace: d3f_volume_components_workspace_bytes (three int32 volumes and the
 * prefix sum's scratch), 4-byte aligned, contents irrelevant; the function returns 0 exactly for a shape d3f_volume_components rejects.
 * Status errors, nothing launched: site, out_label or out_count NULL, connectivity not 6 / 18 / 26, min_voxels < 1, stats_capacity < 0,
 * out_stats NULL with stats_capacity > 0 (D3F_ERR_INVALID_ARG); a bad shape (D3F_ERR_BAD_SHAPE); an int32 pointer or the workspace not
 * 4-byte aligned (D3F_ERR_BAD_LAYOUT); workspace NULL or too short (D3F_ERR_WORKSPACE). */
int64_t d3f_volume_components_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_volume_components(const uint8_t *site, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, int32_t min_voxels, int32_t *out_label,
                          int32_t *out_count, int32_t *out_stats, int32_t stats_capacity, void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 16) Pool the baked field per component: mean rows, votes and coordinate moments.
 *   label        int32 [nx,ny,nz], z fastest, as d3f_volume_components writes it; K >= 0 the number of components;
 *   valid        NULL, or one byte per voxel, non-zero = valid;  slot: NULL, or the int32 volume of a band (d3f_band_mark), -1 = no row;
 *   sets         n_sets sets as d3f_volume_sample takes them: the row of voxel v is data + v*stride_voxel, with `slot` it is
 *                data + slot[v]*stride_voxel (slot values are trusted to address a row);  modes[s]: D3F_POOL_MEAN or D3F_POOL_VOTES.
 * MEMBER: voxel v is a member of component k if label[v] == k with 1 <= k <= K, valid is NULL or valid[v] != 0, and slot is NULL or
 * slot[v] >= 0.  A label outside 1..K (negative, K+1, INT32_MIN) is no member and never indexes anything.
 * Always written:
 *   out_members  ONE device int64: the total member count;
 *   out_count    int32 [K]: the members of each component.
 * Written when out_members <= member_capacity:
 *   out_moments  (may be NULL) int64 [K,9] = {Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz} over the members' integer voxel coordinates, exact
 *                (extents <= 16384 and fewer than 2^31 voxels: nothing overflows);
 *   out_rows[s]  D3F_POOL_MEAN: float32 [K,C], mean_k = fold(the rows of the members of k in ascending flat index) / (float)count_k.
 *                fold is a radix-256 left-to-right tree: for a list of at most D3F_POOL_CHUNK = 256 rows it is ((r0 + r1) + r2) + ...,
 *                every + one IEEE float32 add per channel, starting from r0 and not from zero (fold of one row is that row; -0.0 rows
 *                pool to -0.0); a longer list is cut into consecutive chunks of 256 with a ragged last chunk, and fold is applied to
 *                the list of the chunks' folds.  The division is IEEE, (float)count rounds to nearest.  Channels are independent: the
 *                vector and the scalar row path (the alignment rule of d3f_volume_sample) give the same bits.
 *                D3F_POOL_VOTES (C <= D3F_POOL_MAX_VOTE_CHANNELS): int32 [K,C], entry [k-1][c] = the members of k whose row has its
 *                maximum at channel c by `best = 0; for c in 1..C-1: if row[c] > row[best]: best = c` -- ties go to the lowest
 *                channel, a NaN never wins, a NaN at channel 0 stays.
 * A component without members: count 0, zero moments, zero votes, the set's fill row (NULL: zeros) as its mean.
 * Over capacity (out_members > member_capacity): only out_members and out_count are defined, the status is D3F_OK, and the caller runs
 * again with room (the protocol of d3f_band_mark).  K == 0: D3F_OK, only out_members = 0 is written.
 * No allocation, no synchronisation, the caller's stream; no float atomic anywhere (counts, votes and moments use integer adds): every
 * output is a function of the input alone and two runs give identical bytes.  The member list is built by a prefix sum and a stable
 * radix sort by label; one wave folds one chunk of 256 rows, the levels above fold the partial rows per component in chunk order; as
 * many levels are launched as member_capacity allows (ceil(log256), at most 4).
 * workspace: d3f_volume_pool_workspace_bytes(nx, ny, nz, K, member_capacity, mean_channels) with mean_channels the sum of C over the
 * mean sets; 8-byte aligned, contents irrelevant; the function returns 0 exactly for arguments d3f_volume_pool rejects.
 * Status errors, nothing launched: NULL label / out_members / out_count, K < 0, n_sets outside 0..D3F_MAX_MAPS, n_sets > 0 with NULL sets /
 * modes / out_rows or a NULL data / out_rows entry, an unknown mode, member_capacity < 0 (D3F_ERR_INVALID_ARG); extents outside
 * [1, D3F_EDT_MAX_EXTENT], more than 2^31 - 1 voxels, K above the voxel count, C outside 1..D3F_VOLUME_MAX_CHANNELS, a votes set with
 * C > 256 (D3F_ERR_BAD_SHAPE); a pointer not aligned to its element, stride_voxel < C (D3F_ERR_BAD_LAYOUT); workspace NULL or too short
 * (D3F_ERR_WORKSPACE). */
#define D3F_POOL_MEAN 0
#define D3F_POOL_VOTES 1
#define D3F_POOL_CHUNK 256
#define D3F_POOL_MAX_VOTE_CHANNELS 256
int64_t d3f_volume_pool_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t K, int64_t member_capacity, int64_t mean_channels);
int d3f_volume_pool(const int32_t *label, int32_t nx, int32_t ny, int32_t nz, int32_t K, const uint8_t *valid, const int32_t *slot,
                    const d3f_volume_set *sets, int32_t n_sets, const int32_t *modes, int64_t member_capacity, int64_t *out_members,
                    int32_t *out_count, int64_t *out_moments, void *const *out_rows, void *workspace, int64_t workspace_bytes, void *stream);

/* (still ABI 16: these symbols are ADDED, no struct or earlier entry point changes, and D3F_ABI_VERSION stays 16 -- a client detects the
 * feature by the symbols.)  Cost-to-go through free space: exact shortest paths on the voxel lattice.
 *   free         uint8 [nx,ny,nz], z fastest, non-zero = traversable: the site-volume convention of d3f_volume_edt and
 *                d3f_volume_components;
 *   neighbours   the spatial rule of d3f_volume_components: coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1
 *                for connectivity 6 / 18 / 26.  Nothing wraps through memory;
 *   moves        a move between neighbours u, v exists when both are free.  It costs w[|u - v|_1 - 1] + penalty[v].  w = (w1, w2, w3)
 *                (HOST int32[3]) are integers with 1 <= w1 <= w2 <= w3 <= 255, for face / edge / corner moves; only the first one or two
 *                are used under 6 / 18 (all three are validated).  penalty is an optional int32 volume of values >= 0, charged for
 *                entering v.  NULL means zero.  A negative entry is read as 0;
 *   cost[v]      (int32) the minimum over all move sequences from any seed to v of the summed move costs.  A seed has cost 0; its own
 *                penalty is not charged.  Seeds are int32 flat indices (x*ny + y)*nz + z; a seed that is out of range or on a non-free
 *                voxel is ignored; duplicates are harmless.  A candidate is formed in unsigned arithmetic, so it never wraps; a candidate
 *                above max_cost is discarded.  max_cost lies in 1..INT32_MAX - 1 (the top of that range = no cap).  The cap is
 *                consistent because a prefix of a cheapest path is never dearer than the path.  An unreached voxel holds INT32_MAX;
 *   next[v]      (int32) among the neighbours u with cost[u] + w(u, v) + penalty[v] == cost[v], the one with the smallest flat index.
 *                For a seed it is v itself.  Unreached: -1.  It is computed from the final costs in a pass of its own and is therefore
 *                a function of the input alone.  Because w1 >= 1, following it strictly lowers the cost, so it cannot cycle;
 *   dist[v]      (float32) = (float)cost[v] * (step / (float)w1), each operation correctly rounded, and +inf where unreached.
 * With integer weights the result is the unique fixed point of a min-plus relaxation: exact, independent of the order in which anything
 * happens on the device, the same bytes on every run.  With w = (3, 4, 5) under connectivity 26 in open space, cost / (3 * Euclidean
 * voxel distance) lies in [2 sqrt(2) / 3, sqrt(11) / 3] = [0.9428, 1.1055] (the chamfer distance 3a + b + c of an offset a >= b >= c >= 0:
 * lowest along (1, 1, 0), highest along (3, 1, 1)).
 *
 * The solve is tile-local relaxation with an active-tile list; the caller drives it:
 *   d3f_volume_geodesic_init    cost = INT32_MAX everywhere and 0 at the accepted seeds; the tiles that hold a seed or a neighbour of one are listed; every
 *                               workspace word is initialised (its contents before the call are irrelevant);
 *   d3f_volume_geodesic_relax   enqueues `rounds` rounds with no synchronisation and leaves in out_pending (ONE device int32) the number
 *                               of tiles listed for the round after the last.  The caller reads that word and calls again until it is 0;
 *                               then `cost` is final.  State lives in `cost` and the workspace only: the library keeps none.  free,
 *                               penalty, the shape, connectivity, w and max_cost must be the same in every call of one solve.  A round
 *                               with an empty list costs two empty launches.  After k rounds every voxel whose cheapest path has at most
 *                               k moves is final, so nx*ny*nz rounds always suffice;
 *   d3f_volume_geodesic_finish  next and dist from the final costs (each output may be NULL, not both);
 *   d3f_volume_follow           one lane per start voxel walks `next` (int32 [n_voxels]) for at most max_steps steps: out_voxels int32
 *                               [n, max_steps] = the visited flat indices, starting with the start voxel, padded with -1; out_length
 *                               int32 [n] = the number written; out_reached uint8 [n] = 1 if a seed (next[v] == v) was reached.  A start
 *                               of -1 (or any index outside 0..n_voxels-1), or one whose next is -1, writes length 0.  A path cut by
 *                               max_steps has out_reached 0 and a full row.  n == 0: D3F_OK, nothing launched.
 * No allocation, no synchronisation, the caller's stream; no atomic on a cost word, no float atomic.  Shapes as d3f_volume_edt: extents in
 * [1, D3F_EDT_MAX_EXTENT] (an extent of 1 is legal: a 2-D image is nz = 1), at most 2^31 - 1 voxels.  workspace:
 * d3f_volume_geodesic_workspace_bytes (a small header, one flag word and one list word per tile), 4-byte aligned; the function returns 0
 * exactly for a rejected shape.
 * Status errors, nothing launched: NULL free / out_cost / cost / out_pending, NULL next / starts / outputs of follow with n > 0, both
 * outputs of finish NULL, connectivity not 6 / 18 / 26, w NULL or outside the rule above, max_cost outside 1..INT32_MAX - 1, rounds < 1,
 * n_seeds < 0, NULL seeds with n_seeds > 0, n < 0, max_steps < 1, out_dist with a step that is not finite and > 0
 * (D3F_ERR_INVALID_ARG); an extent outside [1, 16384], more than 2^31 - 1 voxels, n_voxels outside 1..2^31 - 1 (D3F_ERR_BAD_SHAPE); an
 * int32 / float pointer or the workspace not 4-byte aligned (D3F_ERR_BAD_LAYOUT); workspace NULL or too short (D3F_ERR_WORKSPACE). */
int64_t d3f_volume_geodesic_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int d3f_volume_geodesic_init(const uint8_t *free, int32_t nx, int32_t ny, int32_t nz, const int32_t *seeds, int64_t n_seeds, int32_t *out_cost,
                             void *workspace, int64_t workspace_bytes, void *stream);
int d3f_volume_geodesic_relax(const uint8_t *free, const int32_t *penalty, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, const int32_t *w,
                              int32_t max_cost, int32_t rounds, int32_t *cost, int32_t *out_pending, void *workspace, int64_t workspace_bytes, void *stream);
int d3f_volume_geodesic_finish(const uint8_t *free, const int32_t *penalty, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, const int32_t *w,
                               float step, const int32_t *cost, int32_t *out_next, float *out_dist, void *stream);
int d3f_volume_follow(const int32_t *next, int64_t n_voxels, const int32_t *starts, int64_t n, int32_t max_steps, int32_t *out_voxels, int32_t *out_length,
                      uint8_t *out_reached, void *stream);

/* (still ABI 16: these symbols are ADDED, no struct or earlier entry point changes, and D3F_ABI_VERSION stays 16 -- a client detects the
 * feature by the symbols.)  Can I go straight?  Exact grid segments through a free volume, and shortcuts of voxel rows.
 *   free         uint8 [nx,ny,nz], z fastest, non-zero = traversable: the volume of d3f_volume_geodesic_*;
 *   segment      voxel centres sit at the integer coordinates of index space; for two voxels a, b (int32 flat indices (x*ny + y)*nz + z)
 *                the segment is {a + t (b - a), 0 <= t <= 1};
 *   touched      strict (default): the closed cube [v - 1/2, v + 1/2]^3 meets the segment -- the supercover: where the segment passes
 *                exactly through an edge or a corner of the lattice, every cube round that point counts.  D3F_SEGMENT_CUT_CORNERS: the
 *                open cube meets it.  The ends are integers, so a segment never runs inside a face plane and the two rules differ only at
 *                isolated edge and corner crossings.  Under the open rule every move of a d3f_volume_follow path touches its two ends only;
 *                under the strict rule an edge move also touches its 2 side voxels and a corner move its 6.  Every touched voxel lies in the
 *                box spanned by a and b: nothing outside the volume is ever read;
 *   the walk     all in int32 ((2k + 1) * n < 2^29 for extents up to 16384).  n_i = |b_i - a_i|, s_i = sign(b_i - a_i), k_i = 0, cur = a.
 *                Axis i crosses its next plane at t_i = (2 k_i + 1) / (2 n_i); two such values are compared by cross-multiplication.
 *                Event 0 touches {a}.  Every further event takes the set E of the axes with k_i < n_i that share the smallest t_i; under the
 *                strict rule with |E| >= 2 it touches cur + sum of s_i e_i over every non-empty proper subset of E (2 side voxels for
 *                |E| = 2, 6 for |E| = 3); then cur and k advance on all of E and the event touches the new cur.  There are at most
 *                n_x + n_y + n_z + 1 events, their union is the touched set of the rule, and they come in non-decreasing t.
 * d3f_volume_segments, per segment i of n (every output may be NULL, not all of them):
 *   out_clear      uint8: 1 when every touched voxel is free;
 *   out_last       int32: cur of the last event before the first event that touches a non-free voxel; b if the segment is clear, -1 if
 *                  event 0 is already blocked;
 *   out_blocked    int32: the smallest flat index among the non-free voxels of that first blocking event, -1 if clear;
 *   out_min_value, out_min_voxel   (only with `value`, an int32 [nx,ny,nz] volume such as the clearance field's d2) the minimum of value over
 *                  all voxels touched by the events before the first blocking event (all events if clear) and where it is taken: among equal
 *                  minima the earliest event wins, then the smallest flat index within that event.  INT32_MAX and -1 if event 0 is blocked;
 *   an a or b outside 0 .. nx*ny*nz - 1 gives clear = 0, last = blocked = min_voxel = -1, min_value = INT32_MAX.
 * d3f_path_shorten, per row r of n: voxels int32 [n, row_len] holds p_0 .. p_{L-1}, L = length[r] clamped into 0 .. row_len (what follows is
 *   not read).  Anchors: i_0 = 0; from anchor i the next anchor is the LARGEST j in i + 1 .. min(L - 1, i + max_span) whose segment
 *   (p_i, p_j) is clear, and j = i + 1 if there is none (an original move is always kept, clear or not); until L - 1.  Visibility along a
 *   row is not monotone: a nearer j may be blocked while a farther one is clear.  out_index int32 [n, row_len] = the positions
 *   i_0 < i_1 < ..., padded with -1; out_voxels int32 [n, row_len] = the p at those positions, padded with -1 (one of the two may be NULL);
 *   out_count int32 [n].  L = 0 gives count 0, L = 1 count 1.  A row need not be a lattice path: any sequence of indices is legal, and an
 *   entry outside the volume is never the end of a clear segment.
 * One lane per segment; one wave per row, the candidates of an anchor in chunks of 64 from the far end inwards.  No allocation, no
 * synchronisation, no workspace, no atomics, the caller's stream; every loop is bounded by nx + ny + nz, ceil(max_span / 64) and L.
 * Integer-exact: the same bytes on every run.
 * Status errors, nothing launched: NULL free / a / b / voxels / length with n > 0, every output of d3f_volume_segments NULL, out_min_value
 * or out_min_voxel without value, NULL out_count, out_voxels and out_index both NULL, unknown flag bits, n < 0, row_len < 1, max_span < 1
 * (D3F_ERR_INVALID_ARG); an extent outside [1, 16384], more than 2^31 - 1 voxels, more segments or rows than one launch holds
 * (D3F_ERR_BAD_SHAPE); an int32 pointer not 4-byte aligned (D3F_ERR_BAD_LAYOUT).  n == 0: D3F_OK, nothing launched. */
#define D3F_SEGMENT_CUT_CORNERS 1u
int d3f_volume_segments(const uint8_t *free, const int32_t *value, int32_t nx, int32_t ny, int32_t nz, const int32_t *a, const int32_t *b, int64_t n,
                        uint32_t flags, uint8_t *out_clear, int32_t *out_last, int32_t *out_blocked, int32_t *out_min_value, int32_t *out_min_voxel, void *stream);
int d3f_path_shorten(const uint8_t *free, int32_t nx, int32_t ny, int32_t nz, const int32_t *voxels, const int32_t *length, int64_t n, int32_t row_len,
                     int32_t max_span, uint32_t flags, int32_t *out_index, int32_t *out_voxels, int32_t *out_count, void *stream);

/* (still ABI 16: one symbol and one constant are ADDED, no struct or earlier entry point changes, and D3F_ABI_VERSION stays 16 -- a client
 * detects the feature by the symbol.)  Where is this descriptor?  Exact, order-independent non-maximum suppression of K score columns through
 * the band's slot volume.
 *   volume       nx x ny x nz, z fastest, flat index (x*ny + y)*nz + z, extents in [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels;
 *   slot         NULL, or an int32 volume exactly as d3f_band_mark writes it (-1 = no row).  With NULL, row m is voxel m and M must equal
 *                nx*ny*nz.  Slot values are trusted to be < M, as in d3f_band_sample;
 *   mask         NULL, or one byte per voxel (non-zero = takes part);
 *   score        float32: row m, column q at score[m*stride_row + q], 0 <= q < K, stride_row >= K;
 *   radius       r in [1, D3F_PEAKS_MAX_RADIUS];   threshold   a float that is not NaN; +Inf means no threshold.
 *   takes part   for a column q, voxel v with row m = slot[v] takes part when m >= 0, mask[v] != 0 (when a mask is given) and
 *                score[m, q] < +Inf -- a comparison that is false for NaN and for +Inf; -Inf takes part;
 *   peak         v is a peak of column q when it takes part, score[m, q] <= threshold, and for every OTHER voxel u that takes part and has
 *                |u_a - v_a| <= r on all three axes the pair (score_u, flat_u) is lexicographically greater than (score_v, flat_v).  The
 *                neighbourhood is spatial and clipped to the volume: (x, y, nz-1) and (x, y+1, 0) are no neighbours.  Scores compare as
 *                IEEE floats, so -0.0 == +0.0.  The threshold filters peaks; it does not stop a voxel above it from suppressing others.
 *   Consequences: two peaks of one column differ by more than r on some axis; a constant volume has exactly one peak, voxel 0; the result
 *   does not depend on any order of execution.  Minima only: a caller who wants maxima negates, which is exact.
 *   out          out[m*out_stride + q] = score[m, q] (its very bits) where the voxel of row m is a peak of column q, +Inf otherwise.  Every
 *                row 0 .. M-1 and column 0 .. K-1 is written; the padding between K and the stride is not touched.  out must not overlap
 *                score (checked on the host);
 *   out_count    int32 [K], may be NULL: the number of peaks of column q (zeroed by the call, then integer adds).
 * One workgroup per tile of voxels and chunk of columns: (ordered float, flat index) keys of the tile and a halo of r in LDS, the box minimum as
 * three 1-D window minima of 64-bit keys (associative, so exactly separable), a voxel is a peak when the box minimum is its own key.  A tile
 * without a stored voxel leaves before any score load.  No float atomics, nothing waits for another workgroup, every loop bound is known at
 * launch, the caller's stream, no allocation, no synchronisation.  The call needs NO workspace: `workspace` / `workspace_bytes` are
 * reserved, may be NULL / 0 and are never read, so D3F_ERR_WORKSPACE is never returned and there is no _workspace_bytes companion.
 * Status errors, checked on the host before any HIP call, nothing launched: K < 0, M < 0, a radius outside [1, 8], a NaN threshold, a stride
 * below K, NULL score / out with M*K > 0, out overlapping score, M != nx*ny*nz without slot, M > nx*ny*nz with it (D3F_ERR_INVALID_ARG); an
 * extent outside [1, 16384], more than 2^31 - 1 voxels, more column chunks than one launch holds (65535 chunks of 1 to 8 columns), M times a
 * stride above 2^60 (D3F_ERR_BAD_SHAPE); slot, score, out or out_count not 4-byte aligned (D3F_ERR_BAD_LAYOUT).  M == 0 or K == 0: D3F_OK, no kernel
 * launched; a given out_count is still zeroed when K > 0. */
#define D3F_PEAKS_MAX_RADIUS 8
int d3f_volume_peaks(const int32_t *slot, const uint8_t *mask, int32_t nx, int32_t ny, int32_t nz, const float *score, int64_t M, int32_t K,
                     int64_t stride_row, int32_t radius, float threshold, float *out, int64_t out_stride, int32_t *out_count, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* (ABI 16, additive) Rigid alignment of point sets to a baked field: the 6 x 6 normal equations of a damped Gauss-Newton
 * (Levenberg-Marquardt) step, summed per instance on the device without atomics, and the step itself.
 * Per instance i: model points p_j (points [I, n, 3]), weights w_j >= 0 (weights [I, n] or NULL = ones; w_j <= 0 or NaN: the point is
 * padding and adds nothing), a pose (R, t) = pose[i, 0..8] row-major and pose[i, 9..11], the model's weighted centroid m = centroids[i].
 *   x_a = fma(R_a2, p_z, fma(R_a1, p_y, R_a0 * p_x)) + t_a in fp32; the pivot c = the same chain on m; xs = x - c in float64;
 *   x is located as d3f_volume_sample locates a point (g, cell, t, valid); in_band = valid on a dense field (band NULL), valid &&
 *   cell_band[cell] with a band (n_rows == 0: never);
 *   a valid point has the residual r = wd (dist(x) - d_j) with g = (wd / h) d dist / d t (dist_targets [I, n] or NULL = zeros) and, with a
 *   set and where in_band, per channel k the residual r = wf (f_k(x) - s_jk) with g = (wf / h) d f_k / d t (targets [I, n, C]); values by
 *   the chain of d3f_volume_sample, derivatives by the chain of d3f_volume_sample_backward, wd / h and wf / h as wd * (1 / h);
 *   per point in fp32, one fma per term, channels in the sixteen-lane order of the wide sampler, the distance term last:
 *     G = sum g g^T,  q = sum g r,  e = sum r^2;   then in float64 with X = [xs]_x:  J^T J = [[X G X^T, X G], [G X^T, G]],  J^T r = [X q; q];
 *   the parameters are delta = (w_x, w_y, w_z, v_x, v_y, v_z): x <- c + Exp(w)(x - c) + v, so J = [(xs x g)^T, g^T] per residual.
 * A row of D3F_ALIGN_ROW_DOUBLES float64: [0, 21) the upper triangle of H = sum w_j J^T J row by row, [21, 27) b = sum w_j J^T r, [27] cost =
 * sum w_j r^2 + sum over the weighted points that are NOT valid of w_j outside^2, [28] the weighted points that are valid, [29] those in_band,
 * [30, 32) zero.  Sums across points are float64 in a fixed order: two runs give the same bytes.
 *
 * d3f_volume_align_centroid: centroids_out[i] = sum w_j p_j / sum w_j over the weighted points with finite coordinates, in float64, rounded to
 * float32 (zeros when there is none).
 * d3f_volume_align_accumulate: one launch writes one row per (instance, 256 points) to the workspace (d3f_volume_align_workspace_bytes, 8-byte
 * aligned); with `out` [I, D3F_ALIGN_ROW_DOUBLES] not NULL a second launch adds them per instance in ascending order.  skip: NULL, or [I]
 * int32 -- a non-zero entry makes the instance's workgroups leave at once and leaves its rows as they are.  set: NULL (the distance term
 * alone) or ONE set as d3f_volume_sample takes it (with a band: the compacted rows); 16-byte vectors where C % 4 == 0, stride_voxel % 4 == 0
 * and data / targets are 16-byte aligned.
 *
 * The state block of d3f_volume_align_step, D3F_ALIGN_STATE_DOUBLES float64 per instance (the caller fills [0, 28) and zeros the rest):
 *   [0, 9) R and [9, 12) t of the ACCEPTED pose;  [12, 21) R and [21, 24) t of the CANDIDATE (initially the same), all float32 values;
 *   [24, 27) the model centroid m;  [27] lambda (initially 1e-3);  [28] the accepted cost;  [29] status (D3F_ALIGN_*);  [30] accepted steps;
 *   [31] valid and [32] in_band of the accepted pose;  [33, 39) the delta that led to the candidate;  [39, 60) H and [60, 66) b of the
 *   accepted pose;  the rest reserved.
 * d3f_volume_align_step(it): one wave per instance, float64.  A final instance only copies its cost to history[i, it].  Otherwise the
 * rows of the accumulate at the candidate are added (and written to out[i]) and
 *   it == 0 or cost < accepted cost: the candidate is accepted; for it > 0 lambda = max(lambda / 10, 1e-9), steps += 1 and, with
 *           |w| < rot_tol and |v| < trans_tol of the delta that led to it, status = CONVERGED;
 *   otherwise (equal or NaN included): rejected, lambda = min(10 lambda, 1e6), and STALLED once lambda has reached 1e6;
 *   history[i, it] = the accepted cost.  Still RUNNING and it < iters: hmax = max_j H_jj, not > 0: NO_GRADIENT; D_jj = max(H_jj, 1e-9 hmax);
 *   Cholesky of H + lambda D, a pivot that is not in (0, inf): FAILED; delta = -(H + lambda D)^-1 b.  A delta below both tolerances that was
 *   solved at a pose accepted in this very call also ends the instance as CONVERGED, without being taken: it would lower the cost by less
 *   than the fp32 sums resolve, so it could never be accepted.  Otherwise the candidate R = Exp(w) R, t = c + Exp(w)(t - c) + v with
 *   Rodrigues in float64, rounded to float32, goes to the state and to pose_out[i].
 *   An instance that ends in this call, and every instance at it == iters, gets pose_out[i] = its accepted pose; one that ends also skip_out[i] = 1.
 *   skip_out (the `skip` of the accumulate) must be ZERO before step 0: the step only ever stores 1 there.  pose_out, out and history may hold anything
 *   before step 0, which writes out[i] and pose_out[i] of every instance; an instance that was final at entry keeps what an earlier step wrote there.
 * A solve is accumulate(pose, skip), step(0), accumulate, step(1), ... step(iters) on one stream: 2 iters + 2 launches, no allocation, no
 * synchronisation, no atomics, and no kernel waits for another workgroup.
 * Status errors, on the host before any HIP call: NULL vol / points / pose / centroids / workspace / state / outputs, negative I or n, a weight
 * of a term (or outside, or a tolerance) that is negative or not finite, it outside [0, iters] (D3F_ERR_INVALID_ARG); the volume checks, C outside
 * [1, D3F_VOLUME_MAX_CHANNELS], more than 2^31 - 1 workgroups (D3F_ERR_BAD_SHAPE); a float / int32 pointer off 4 bytes or a double pointer off 8,
 * stride_voxel < C (D3F_ERR_BAD_LAYOUT); a short workspace (D3F_ERR_WORKSPACE).  I == 0 or n == 0: D3F_OK, nothing launched. */
#define D3F_ALIGN_ROW_DOUBLES 32
#define D3F_ALIGN_STATE_DOUBLES 96
#define D3F_ALIGN_RUNNING 0
#define D3F_ALIGN_CONVERGED 1
#define D3F_ALIGN_STALLED 2
#define D3F_ALIGN_NO_GRADIENT 3
#define D3F_ALIGN_FAILED 4
int64_t d3f_volume_align_workspace_bytes(int64_t I, int64_t n);
int d3f_volume_align_centroid(const float *points, const float *weights, int64_t I, int64_t n, float *centroids_out, void *stream);
int d3f_volume_align_accumulate(const d3f_volume *vol, const d3f_band *band, const d3f_volume_set *set, const float *points, const float *weights,
                                const float *targets, const float *dist_targets, const float *pose, const float *centroids, const int32_t *skip,
                                int64_t I, int64_t n, float dist_weight, float feat_weight, float outside, double *out, void *workspace,
                                int64_t workspace_bytes, void *stream);
int d3f_volume_align_step(double *state, const void *workspace, int64_t workspace_bytes, int64_t I, int64_t n, double *out, int32_t it, int32_t iters,
                          double rot_tol, double trans_tol, float *pose_out, int32_t *skip_out, double *history, void *stream);

/* (ABI 16, additive: four symbols and three constants; a client detects the feature by the symbol.)  Which pose explains these matches?
 * Consensus poses from M model points with k candidate places each (csrc/consensus_kernels.hip).
 *   model      float32 [M, 3], 3 <= M <= D3F_CONSENSUS_MAX_POINTS;
 *   cand       float32 [M, k, 3], 1 <= k <= D3F_CONSENSUS_MAX_CANDIDATES; a row with a NaN coordinate is padding;
 *   triplets   int32 [n_trip, 3] on the DEVICE, triplets_host the same table in HOST memory (it is what the call validates: 0 <= i < j < l < M;
 *              a device entry that fails this test rejects its hypotheses, so a wrong copy cannot read out of bounds);
 *   a hypothesis is h = (trip * k + a) * k * k + b * k + c: triplet (i, j, l) with the candidate digits (a, b, c); T = n_trip k^3 <= 2^31 - 1.
 * The arithmetic contract.  Only IEEE + - * / sqrt in the stated order and NO fma, so that a NumPy restatement gives the same bits.
 *   gate, in float64 from the float32 inputs:  u = p_j - p_i, v = p_l - p_i, w = v - u;  U = c_jb - c_ia, V = c_lc - c_ia, W = V - U;
 *     |x|^2 = (x0 x0 + x1 x1) + x2 x2;  a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  Rejected: a NaN among the nine candidate
 *     coordinates; not (|u|, |v|, |w| >= min_side); not (||U| - |u||, ||V| - |v||, ||W| - |w|| <= side_tol); not (|u x v|^2 >= (min_sin^2
 *     |u|^2) |v|^2), or not the same of (U, V).  A NaN rejects.  A rejected hypothesis has count 0 and takes no further part;
 *   pose, in float64:  e1 = u / |u|, e3 = (u x v) / |u x v|, e2 = e3 x e1;  f1, f3, f2 the same of (U, V);  R_ab = (f1_a e1_b + f2_a e2_b)
 *     + f3_a e3_b;  ps = ((p_i + p_j) + p_l) / 3, cs = ((c_ia + c_jb) + c_lc) / 3;  t_a = cs_a - ((R_a0 ps_0 + R_a1 ps_1) + R_a2 ps_2); every
 *     entry is rounded once to float32.  A pose is 12 floats: R row-major, then t (x = R p + t);
 *   score, in float32, per model point q and candidate s:  x_a = ((R_a0 p_x + R_a1 p_y) + R_a2 p_z) + t_a, d = x - c_qs,
 *     d2 = (dx dx + dy dy) + dz dz; the assignment of q is the s with the smallest d2 <= tau2, ties to the lower s, else none (-1); a NaN
 *     compares false; tau2 is the caller's float32; count = the number of assigned points;
 *   selection:  the survivors are the hypotheses with count >= min_inliers, ordered by (count descending, h ascending); only the best
 *     max_survivors are kept.  Then n_poses rounds: take the best live survivor and kill every survivor that shares at least `shared`
 *     identical (point, candidate) assignments with it (the winner included).  Integer-exact and independent of any order of execution;
 *   refit:  Horn's closed form in float64 over the assigned pairs (p_q, c_{q, s_q}), ascending q: centroids pm, cm (sum / n), S_ab = sum
 *     (p - pm)_a (c - cm)_b, the symmetric 4 x 4 matrix N of S, its largest eigenvector by 12 cyclic Jacobi sweeps (zero entries are
 *     skipped), R = the quaternion's matrix / |quat|^2, t = cm - R pm, rounded to float32;  rmse = sqrt(sum |R32 p + t32 - c|^2 / n) in float64.
 * d3f_pose_consensus_score: count_out uint8 [T]; pose_out float32 [T, 12] and assign_out int8 [T, M] may be NULL (they exist for tests; a
 *   rejected hypothesis has a pose of zeros and assignments of -1).  Zeroes the head of the workspace and leaves there the histogram of counts
 *   and the number of hypotheses that passed the gate, which d3f_pose_consensus_select reads: the two are called in this order with the same
 *   arguments and the same workspace (d3f_pose_consensus_workspace_bytes, 16-byte aligned).
 * d3f_pose_consensus_select: hyp_out int32 [n_poses] (-1: no such rank), inliers_out int32 [n_poses] (-1), assign_out int8 [n_poses, 64]
 *   (-1: none, and beyond M), pose_out float32 [n_poses, 12] (NaN), stats_out int32 [4]: poses found, hypotheses that passed the gate,
 *   survivors, the count at the cut.  max_survivors is at most D3F_CONSENSUS_MAX_SURVIVORS = 65536: the rounds run in ONE workgroup, which reads every
 *   live survivor's 64-byte row once per round (at 65536 survivors and 64 rounds 256 MB through one compute unit); a longer list is not built.
 * d3f_pose_refit: assign int8 [n_poses, 64] as select writes it; a row with fewer than 3 assigned points gives a NaN pose, a NaN rmse and
 *   count -1.  pose_out float32 [n_poses, 12], rmse_out float64 [n_poses], inliers_out int32 [n_poses]: the count of the score at the refit pose.
 * Caller's stream, no allocation, no synchronisation, no float atomic; no kernel waits for another workgroup.  Status errors, on the host
 * before any HIP call: a NULL pointer, tau2 / side_tol / min_side / min_sin not finite or out of range (tau2 > 0, the others >= 0),
 * min_inliers outside [3, 64], shared outside [1, 64], max_survivors outside [1, D3F_CONSENSUS_MAX_SURVIVORS], n_trip < 0
 * (D3F_ERR_INVALID_ARG); M, k or n_poses (1..64) out of range, a triplet that is not 0 <= i < j < l < M, T above 2^31 - 1 (D3F_ERR_BAD_SHAPE);
 * a pointer not aligned to its element, the workspace not to 16 bytes (D3F_ERR_BAD_LAYOUT); a short workspace (D3F_ERR_WORKSPACE).
 * n_trip == 0 (and n_poses == 0 for the refit): D3F_OK, nothing launched, no output is written: there are zero poses, and the caller's
 * outputs keep the padding it put there. */
#define D3F_CONSENSUS_MAX_POINTS 64
#define D3F_CONSENSUS_MAX_CANDIDATES 8
#define D3F_CONSENSUS_MAX_SURVIVORS (1 << 16)
int64_t d3f_pose_consensus_workspace_bytes(int32_t M, int32_t k, int64_t n_trip, int64_t max_survivors);
int d3f_pose_consensus_score(const float *model, const float *cand, int32_t M, int32_t k, const int32_t *triplets, const int32_t *triplets_host,
                             int64_t n_trip, float tau2, double side_tol, double min_side, double min_sin, uint8_t *count_out, float *pose_out,
                             int8_t *assign_out, void *workspace, int64_t workspace_bytes, void *stream);
int d3f_pose_consensus_select(const float *model, const float *cand, int32_t M, int32_t k, const int32_t *triplets, int64_t n_trip, float tau2,
                              double side_tol, double min_side, double min_sin, const uint8_t *count, int32_t min_inliers, int32_t shared,
                              int64_t max_survivors, int32_t n_poses, int32_t *hyp_out, int32_t *inliers_out, int8_t *assign_out, float *pose_out,
                              int32_t *stats_out, void *workspace, int64_t workspace_bytes, void *stream);
int d3f_pose_refit(const float *model, const float *cand, int32_t M, int32_t k, const int8_t *assign, int32_t n_poses, float tau2, float *pose_out,
                   double *rmse_out, int32_t *inliers_out, void *stream);

/* (still ABI 16: symbols added -- two entry points and six constants; no struct or earlier entry point changes and D3F_ABI_VERSION stays 16; a
 * client detects the feature by the symbols.)  Which part is this?  Descriptor-gated links between neighbouring voxels, and the connected
 * components over such a link volume (csrc/parts_kernels.hip, csrc/ccl_kernels.hip).
 *   volume       nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, extents in [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels;
 *   site         uint8 [nx,ny,nz], non-zero = site;  valid: NULL or one byte per voxel;  slot: NULL or the int32 volume of a band, -1 = no row;
 *   set          ONE set (HOST struct) as d3f_volume_pool takes it: the row of voxel v is data + v*stride_voxel, with `slot` it is
 *                data + slot[v]*stride_voxel (slot values are trusted to address a row); `fill` is not read;
 *   member       site[v] != 0, valid[v] != 0 (when given) and slot[v] >= 0 (when given);
 *   offsets      (dx, dy, dz) over {-1,0,1}^3 in lexicographic order, the 13 that precede (0,0,0): j = 9*(dx+1) + 3*(dy+1) + (dz+1).  Bits 0..8 are
 *                dx = -1, bits 9..11 are (0,-1,*), bit 12 is (0,0,-1): each names a neighbour of LOWER flat index.
 * d3f_volume_links writes out_links uint16 [nx,ny,nz], every voxel: bit j of voxel v is set iff v is a member, u = v + offset j lies inside the
 * volume (the rule is spatial: (x, y, 0) and (x, y-1, nz-1) are adjacent in memory and are no neighbours), |dx|+|dy|+|dz| <= 1 / 2 / 3 for
 * connectivity 6 / 18 / 26, u is a member, and the rule accepts the rows a (of v) and b (of u).  Bits 13..15 are 0.  Every pair is evaluated
 * once, by its higher voxel, so links are symmetric by construction.
 *   D3F_LINK_L2      s <= threshold; the caller passes the SQUARED radius.  The comparison is false for a NaN s: a row with a NaN, or two rows
 *                    with the same infinity in one channel, link to nothing, and a row with an infinity links to nothing under a finite
 *                    threshold.  threshold = +Inf accepts every s that is not NaN, so every pair of finite rows;
 *   D3F_LINK_COSINE  na > 0 && nb > 0 && dot >= 0 && (double)dot*dot >= ((double)t*t) * ((double)na*nb) with t = threshold in [0, 1]: float64
 *                    products of the float32 sums, each rounded once; no square root, no division.  A zero row and a row with a NaN link to
 *                    nothing; sums that overflow to infinity compare as IEEE has it (Inf >= Inf holds, 0 * Inf is NaN and does not);
 *   D3F_LINK_ARGMAX  best(a) == best(b) with `best = 0; for c in 1..C-1: if row[c] > row[best]: best = c`: the vote rule of d3f_volume_pool
 *                    (ties go to the lowest channel, a NaN never wins, a NaN at channel 0 stays).  Exact; meant for an instance-mask set.
 *                    threshold is not used (it still must not be NaN).
 * THE SUMMATION ORDER.  Every sum has one float32 accumulator that starts at +0.0f and takes the channels in ascending order c = 0 .. C-1:
 *   s = fl(s + fl(d*d)) with d = fl(a_c - b_c);   dot = fl(dot + fl(a_c*b_c));   na = fl(na + fl(a_c*a_c));   nb = fl(nb + fl(b_c*b_c));
 * each operation one IEEE float32 operation, nothing fused.  The vector and the scalar row path (the alignment rule of d3f_volume_sample) give
 * the same bits; tests/parts_cases.py reproduces every sum bit for bit.
 * One workgroup per tile of D3F_LINK_TILE_X x D3F_LINK_TILE_Y x D3F_LINK_TILE_Z voxels stages the rows of the tile and of its halo (x-1, y-1 .. y+1,
 * z-1 .. z+1) through LDS in chunks of channels, so a row is loaded once per tile; a tile without a member writes zeros and loads no row.  No
 * atomics, no workspace, nothing waits for another workgroup, the caller's stream, no allocation, no synchronisation; two runs give identical bytes.
 * Status errors, nothing launched: NULL site / set / set->data / out_links, an unknown rule, connectivity not 6 / 18 / 26, a NaN threshold, a
 * cosine threshold outside [0, 1] (D3F_ERR_INVALID_ARG); an extent outside [1, 16384], more than 2^31 - 1 voxels, C outside
 * 1..D3F_VOLUME_MAX_CHANNELS (D3F_ERR_BAD_SHAPE); stride_voxel < C, slot or data not 4-byte aligned, out_links not 2-byte aligned
 * (D3F_ERR_BAD_LAYOUT).
 *
 * d3f_volume_components_linked is d3f_volume_components with `links` after `site`: the same outputs, stats rows, numbering, workspace
 * (d3f_volume_components_workspace_bytes) and status codes (links NULL: D3F_ERR_INVALID_ARG; not 2-byte aligned: D3F_ERR_BAD_LAYOUT).  Two sites are
 * united iff the higher one's bit for that offset is set, the connectivity allows the offset, and the neighbour lies inside the volume and is
 * a site; components are the classes of the transitive closure.  A bit that points outside the volume or at a non-site, and bits 13..15, are
 * ignored and never followed: a caller may AND or OR criteria of its own into a link volume, and no bit pattern causes a read out of range.  An
 * all-ones link volume gives exactly the labelling of d3f_volume_components. */
#define D3F_LINK_L2 0
#define D3F_LINK_COSINE 1
#define D3F_LINK_ARGMAX 2
#define D3F_LINK_TILE_X 4
#define D3F_LINK_TILE_Y 4
#define D3F_LINK_TILE_Z 16
int d3f_volume_links(const uint8_t *site, const uint8_t *valid, const int32_t *slot, int32_t nx, int32_t ny, int32_t nz, const d3f_volume_set *set, int32_t rule,
                     float threshold, int32_t connectivity, uint16_t *out_links, void *stream);
int d3f_volume_components_linked(const uint8_t *site, const uint16_t *links, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, int32_t min_voxels,
                                 int32_t *out_label, int32_t *out_count, int32_t *out_stats, int32_t stats_capacity, void *workspace, int64_t workspace_bytes,
                                 void *stream);

/* (still ABI 16: symbols added -- one entry point and one constant; no struct or earlier entry point changes and D3F_ABI_VERSION stays 16; a
 * client detects the feature by the symbol.)  How did it move?  Dense descriptor flow between two baked fields on the SAME grid (DESIGN.md
 * section 25; csrc/flow_kernels.hip): for every member voxel of field A the voxel of field B within Chebyshev distance `radius` whose stored
 * row is closest in L2.
 *   volume       nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, extents in [1, D3F_EDT_MAX_EXTENT], at most 2^31 - 1 voxels;
 *   site_a/_b    uint8 [nx,ny,nz], non-zero = site;  slot_a/_b: NULL (dense) or the int32 volume of a band, -1 = no row; either field may be
 *                dense or banded, independently of the other;
 *   set_a/_b     ONE set each (HOST structs) as d3f_volume_links takes it, both with the same C in 1..D3F_VOLUME_MAX_CHANNELS; `fill` is not read;
 *   member       of A: site_a[v] != 0 and slot_a[v] >= 0 (when given); of B likewise (a caller folds `valid` into the site byte);
 *   candidates   of v: u = v + (dx, dy, dz) with |dx|, |dy|, |dz| <= radius, radius in 1..D3F_FLOW_MAX_RADIUS, u inside the volume (spatially:
 *                nothing wraps through memory) and a member of B;
 *   cost         s(v, u): one float32 accumulator that starts at +0.0f and takes the channels in ascending order, s = fl(s + fl(d*d)) with
 *                d = fl(a_c - b_c), each operation one IEEE float32 operation, nothing fused: the L2 chain of d3f_volume_links word for word;
 *   takes part   iff s is finite (not NaN, not +Inf) and s <= max_cost2; the caller passes the SQUARED radius, +Inf means no threshold;
 *   winner       the candidate with the lexicographically smallest key (s, d2, j), d2 = dx^2 + dy^2 + dz^2,
 *                j = ((dx + r)*(2r + 1) + (dy + r))*(2r + 1) + (dz + r); for a fixed v ascending j is ascending flat index of u.  With s >= +0,
 *                d2 <= 48 and j < 729 the key packs exactly into 64 bits: bits(s) << 16 | d2 << 10 | j.
 * Outputs, every voxel of the volume written: out_target int32 [nx,ny,nz] the flat index of the winner or -1; out_cost float32 [nx,ny,nz] the
 * winner's s or +Inf.  -1 and +Inf go together: a non-member of A, or a member with no candidate that takes part.  out_axis_cost (NULL to
 * skip) float32 [n, 6]: for a voxel with target t the costs s(v, t -+ e) in the order x-, x+, y-, y+, z-, z+, +Inf where the neighbour lies
 * outside the volume, is no member of B or has a non-finite s (neither the window nor max_cost2 applies here); six +Inf for a voxel without
 * a target.  The same chain.
 * One workgroup per tile of D3F_LINK_TILE_X x _Y x _Z voxels of A; the window is cut into sub-windows of at most 5 x 5 x 5 offsets, one pass
 * each over the B rows of a shifted box staged through LDS, and the running best 64-bit key makes the merge exact.  No atomics, no workspace,
 * nothing waits for another workgroup, the caller's stream, no allocation, no synchronisation; two runs give identical bytes.
 * Status errors, nothing launched: NULL site_a / site_b / set_a / set_b / a set's data / out_target / out_cost, radius outside
 * 1..D3F_FLOW_MAX_RADIUS, a NaN max_cost2 (D3F_ERR_INVALID_ARG); an extent outside [1, 16384], more than 2^31 - 1 voxels, C outside
 * 1..D3F_VOLUME_MAX_CHANNELS or different in the two sets (D3F_ERR_BAD_SHAPE); a stride_voxel < C, a slot, data or output not 4-byte aligned
 * (D3F_ERR_BAD_LAYOUT). */
#define D3F_FLOW_MAX_RADIUS 4
int d3f_volume_flow(const uint8_t *site_a, const int32_t *slot_a, const d3f_volume_set *set_a, const uint8_t *site_b, const int32_t *slot_b,
                    const d3f_volume_set *set_b, int32_t nx, int32_t ny, int32_t nz, int32_t radius, float max_cost2, int32_t *out_target, float *out_cost,
                    float *out_axis_cost, void *stream);

/* (still ABI 16: symbols added -- two entry points and their constants; no struct or earlier entry point changes and D3F_ABI_VERSION stays 16; a
 * client detects the feature by the symbols.)  How did each part move?  One rigid motion per part from the dense correspondences of a flow, with
 * a trim-and-refit loop and the verdict per voxel (csrc/motion_kernels.hip).
 *   volume       nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, n voxels; extents in [1, D3F_EDT_MAX_EXTENT], n <= 2^31 - 1;
 *   label        int32 [nx,ny,nz] as d3f_volume_components writes it, K >= 0 parts;  keep: NULL (every voxel) or one byte per voxel;
 *   target       int32 [nx,ny,nz] as d3f_volume_flow writes it;  offset: NULL (zeros) or float64 [n,3], the sub-voxel correction in voxels;
 *   ref          NULL (zeros) or int32 [K,3]: an integer reference corner per part (the lower corner of its box), which keeps the moments small.
 * PAIR: voxel v is a pair of part k when label[v] == k with 1 <= k <= K, keep is NULL or keep[v] != 0, 0 <= target[v] < n and, with offset
 * given, its three components at v are finite.  Any other label or target indexes nothing.  In voxel units relative to ref_k:
 *   a = (x,y,z)(v) - ref_k (exact integers held as float64);  b = ((x,y,z)(target[v]) - ref_k) + offset[v]: the integer difference first, then
 *   one float64 add per axis (none with offset NULL).
 * MOMENTS: a member's row is the D3F_MOTION_SUM_DOUBLES = 16 float64 {1, a0,a1,a2, b0,b1,b2, a_i*b_j (i major, 9)}; a member that is no inlier
 * of the current fit contributes a row of +0.0.  The rows of a part are folded in ascending flat index in chunks of D3F_POOL_CHUNK = 256
 * consecutive members of that part with a ragged last chunk, and the next level folds the part's partial rows in chunk order, 256 at a time
 * (the chunk and level structure of d3f_volume_pool).  Inside a chunk: pad to 256 rows with +0.0; lane l of 64 holds
 * (((0.0 + m_l) + m_{l+64}) + m_{l+128}) + m_{l+192}; then for s = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l+s] for l < s; v[0] is the fold.  Every +
 * is one IEEE float64 add, the 16 columns are independent, nothing is fused.  A part without pairs has a row of +0.0.
 * FIT (float64): with n and the sums A, B, M of the row: pm = A / n, cm = B / n, S_ij = M_ij - (A_i * B_j) / n; then Horn's closed form exactly as
 * d3f_pose_refit does it: the symmetric 4 x 4 matrix of S, 12 cyclic Jacobi sweeps that skip zero entries, the first largest diagonal entry,
 * R = the quaternion's matrix / |q|^2.  The pose row is D3F_MOTION_POSE_DOUBLES = 15 float64: R row-major, src = ref + pm, dst = ref + cm, and
 * means q = R (p - src) + dst in voxel index units.
 * RESIDUAL of a pair: u = a - pm, w = b - cm, e_i = ((R_i0 u0 + R_i1 u1) + R_i2 u2) - w_i, r2 = (e0 e0 + e1 e1) + e2 e2.  It is an inlier when
 * r2 <= tau2 (a NaN compares false).
 * LOOP, fits in 1..D3F_MOTION_MAX_FITS: fit 0 uses every pair, fit f >= 1 the inliers under the pose of fit f-1.  A part with fewer than min_pairs
 * (>= 3) pairs at fit 0: a NaN pose row, D3F_MOTION_TOO_FEW, out_fits 0.  A part whose inliers fall below min_pairs at a later fit keeps the pose of
 * its last fit: D3F_MOTION_THINNED, out_fits the number of fits done.  Else D3F_MOTION_OK, out_fits = fits.
 * Always written: out_members ONE device int64, the total pair count; out_pairs int32 [K].  Written when out_members <= member_capacity:
 *   out_pose [K,15], out_status, out_fits [K];  under the final pose: out_residual2 float64 [n] (may be NULL; NaN where v is no pair or its part
 *   has no pose), out_inlier uint8 [n] (may be NULL), out_inliers int32 [K], out_rmse float64 [K] = sqrt(fold(r2 of the final inliers, +0.0 for
 *   the others) / inliers) by the same tree, NaN without inliers;  out_sums (may be NULL; for tests) float64 [K,16]: the sums of the LAST fold a
 *   part took part in (the fold that thinned it, for a thinned part).
 * Over capacity (out_members > member_capacity): only out_members and out_pairs are defined, the status is D3F_OK, the caller runs again with
 * room (the protocol of d3f_volume_pool).  K == 0: D3F_OK, only out_members = 0 is written.
 * Collinear or coincident pairs leave the rotation about their axis undetermined; the pose is then still a deterministic function of the input
 * (whatever the Jacobi sweeps leave).  It is not detected.
 * The member list is built once by d3f_volume_pool's flag, scan, compaction and stable label sort on "label where pair, else 0"; one wave folds one
 * chunk; the whole loop is enqueued on the caller's stream, as many fold levels per fit as member_capacity allows; a part whose loop has ended
 * takes no further part.  No allocation, no synchronisation, no float atomic, nothing waits for another workgroup; two runs give identical bytes.
 * workspace: d3f_part_motion_workspace_bytes(nx, ny, nz, K, member_capacity), 8-byte aligned, contents irrelevant; the function returns 0 exactly
 * for arguments d3f_part_motion rejects.
 * Status errors, nothing launched: NULL label / target / out_members / out_pairs / out_pose / out_inliers / out_rmse / out_status / out_fits, K < 0,
 * fits outside 1..8, tau2 not finite or <= 0, min_pairs < 3, member_capacity < 0 (D3F_ERR_INVALID_ARG); an extent outside
 * [1, D3F_EDT_MAX_EXTENT], more than 2^31 - 1 voxels, K above the voxel count (D3F_ERR_BAD_SHAPE); a pointer not aligned to its element
 * (D3F_ERR_BAD_LAYOUT); the workspace NULL or short (D3F_ERR_WORKSPACE). */
#define D3F_MOTION_OK 0
#define D3F_MOTION_THINNED 1
#define D3F_MOTION_TOO_FEW 2
#define D3F_MOTION_MAX_FITS 8
#define D3F_MOTION_SUM_DOUBLES 16
#define D3F_MOTION_POSE_DOUBLES 15
int64_t d3f_part_motion_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t K, int64_t member_capacity);
int d3f_part_motion(const int32_t *label, int32_t K, int32_t nx, int32_t ny, int32_t nz, const uint8_t *keep, const int32_t *target, const double *offset,
                    const int32_t *ref, int32_t fits, double tau2, int32_t min_pairs, int64_t member_capacity, int64_t *out_members, int32_t *out_pairs,
                    double *out_pose, int32_t *out_inliers, double *out_rmse, int32_t *out_status, int32_t *out_fits, double *out_residual2,
                    uint8_t *out_inlier, double *out_sums, void *workspace, int64_t workspace_bytes, void *stream);

/* (still ABI 16: symbols added -- two entry points, two HOST argument structs and one constant; no earlier struct or entry point changes and
 * D3F_ABI_VERSION stays 16; a client detects the feature by the symbols.)  Where is it now?  A baked field moved by the rigid motions of its parts
 * (csrc/warp_kernels.hip): per destination voxel who wins, then each stored row gathered once.
 * Coordinates are voxel index units, the flat index is v = (x*ny + y)*nz + z.  No operation below is fused; every float equals the NumPy
 * restatement (tests/warp_cases.py) byte for byte.
 *   source field  vol: nx, ny, nz, dist, valid, cell_valid as d3f_volume_sample takes them (origin and step are not read);
 *   owner         int32 [nx,ny,nz];  K in 0..D3F_WARP_MAX_PARTS;  pose float64 [K,15] ON THE DEVICE, a row as d3f_part_motion writes it: R row-major,
 *                 src, dst with q = R (p - src) + dst.  R is trusted to be a rotation: its transpose is used as its inverse.  For any other matrix
 *                 the result is unspecified, but every access stays in bounds.
 *   moving        part k (1..K) moves iff all 15 entries of row k-1 are finite; a voxel is moving when its owner is a moving part.  Owner values
 *                 outside 1..K and the voxels of parts that do not move are BACKGROUND: they stay where they are.
 *   inverse map   of destination voxel q under part k, float64, one rounding per operation:  u = q - dst;
 *                 p_i = ((R_0i*u_0 + R_1i*u_1) + R_2i*u_2) + src_i;  inside: 0 <= p_a <= n_a - 1 on the three axes (NaN is not inside);
 *                 i_a = min(floor(p_a), n_a - 2);  t_a = float32(p_a - i_a);  the nearest corner is i_a + (t_a > 0.5f).
 *   candidate k   exists when p is inside, cell_valid[i] is set, owner[nearest corner] == k and the interpolated distance is not NaN.
 *   interpolation the weights w(dx,dy,dz) of d3f_volume_sample (products left to right); acc = w0*v0, then acc = acc + w_c*v_c for c = 1..7 in that
 *                 sampler's corner order, each product and each sum rounded to float32 (NOT the fused chain of d3f_volume_sample).
 *   candidate 0   the background: the voxel itself with dist[q], when valid[q], q is not moving and dist[q] is not NaN.  A voxel a moving part has
 *                 left has no background: what was behind the part was never observed.
 *   winner        candidates in the order 0, 1, ..., K; a later one replaces the best only if its distance is strictly smaller: the union of the
 *                 moved solids (the minimum of signed distances), ties to the lower index.
 * d3f_volume_warp_select writes, completely: out_source int32 [nx,ny,nz] (0 background, k part k, -1 none); out_dist float32 (1e3 where the source
 * is -1); out_valid uint8 (source >= 0); out_boxes int32 [K,12], per part {lo xyz, hi xyz} of its owner == k voxels, then {lo xyz, hi xyz} of the
 * destination voxels it won, inclusive; an empty box is lo = INT32_MAX, hi = INT32_MIN.  K == 0: pose and out_boxes may be NULL.
 * Three launches on `stream` (the boxes' init, the owner boxes, one workgroup per tile of 4 x 8 x 8 destination voxels that culls the parts 64 per
 * wave step against the owner boxes -- exactly: the map is affine -- and walks the survivors in ascending order).  Integer atomic min / max for the
 * boxes only; no float atomic, no workspace, no allocation, no synchronisation; two runs give identical bytes.
 * d3f_volume_warp_rows produces the rows of m listed destination voxels (voxels int32 [m], any order, duplicates allowed; NULL: every voxel in flat
 * order, m must be nx*ny*nz; an entry outside the volume gets fill rows) from `source` as select wrote it, for n_sets in 0..D3F_MAX_MAPS sets:
 *   source -1     the set's fill row (NULL: zeros); out_known = 0;
 *   source 0      the stored row of q, copied.  Banded (band != NULL): the row slot[q]; slot[q] < 0: fill, out_known = 0;
 *   source k      p, i, t recomputed by the same expressions, then the same unfused chain over the eight corner rows per channel.  Banded: only when
 *                 cell_band[i] is set, rows through slot; otherwise fill, out_known = 0.  (A source value outside -1..K, or an image that is not
 *                 inside, is answered with fill rows.)
 * out_sets[s]: float32 [m, sets[s].C], C-contiguous; out_known one byte per listed voxel.  vol gives the extents only (no array of it is read).
 * Banded with n_rows == 0: slot, cell_band and every data may be NULL, nothing of the band is read.  m == 0: D3F_OK, nothing is read.  The 16-byte
 * vector / scalar rule, the boundary between <= 16 and wider channel counts (one lane / sixteen lanes per voxel) and stride_voxel >= C are as in
 * d3f_volume_sample.  One launch; no atomics.
 * Status errors, nothing launched: a NULL struct, NULL owner / out_source / out_dist / out_valid / source / out_known, NULL pose or out_boxes with
 * K > 0, K < 0, m < 0, voxels NULL with m != nx*ny*nz, NULL sets / out_sets / an out_sets entry / a set's data (D3F_ERR_INVALID_ARG); an extent below
 * 2, more than 2^31 - 1 voxels, K > D3F_WARP_MAX_PARTS, n_sets or a C out of range (D3F_ERR_BAD_SHAPE); stride_voxel < C, a pointer not aligned to
 * its element (D3F_ERR_BAD_LAYOUT). */
#define D3F_WARP_MAX_PARTS 4096
typedef struct d3f_warp_select {
    d3f_volume vol;
    const int32_t *owner;
    const double *pose;
    int32_t K;
    int32_t reserved;          /* 0 */
    int32_t *out_source;
    float *out_dist;
    uint8_t *out_valid;
    int32_t *out_boxes;
} d3f_warp_select;
typedef struct d3f_warp_rows {
    d3f_volume vol;
    const d3f_band *band;      /* NULL: a dense source */
    const d3f_volume_set *sets;
    int32_t n_sets;
    int32_t K;
    const int32_t *source;
    const double *pose;
    const int32_t *voxels;
    int64_t m;
    void *const *out_sets;
    uint8_t *out_known;
} d3f_warp_rows;
int d3f_volume_warp_select(const d3f_warp_select *args, void *stream);
int d3f_volume_warp_rows(const d3f_warp_rows *args, void *stream);

/* (ABI 12) The first surface a ray meets in a baked volume: a fixed-step march through `dist` with one linear interpolation at the
 * sign change.  Everything in fp32.  Ray i is p(t) = o + t*d; d need not be unit.
 *   once per ray: go_a = (o_a - origin_a) / h, gd_a = d_a / h (IEEE divisions), len = sqrtf(fma(d_z, d_z, fma(d_y, d_y, d_x*d_x)));
 *   the ray MISSES if a go_a or gd_a is not finite (NaN or infinite input) or len is not in (0, inf) (d = 0);
 *   clip: per axis with gd_a != 0, ta = (0 - go_a) / gd_a, tb = ((n_a - 1) - go_a) / gd_a, lo = max(lo, min(ta, tb)), hi = min(hi, max(ta, tb))
 *         from lo = -inf, hi = +inf; an axis with gd_a == 0 constrains nothing if 0 <= go_a <= n_a - 1, else the ray misses;
 *         t0 = max(lo, t_near), t1 = min(hi, t_far); the ray misses if !(t0 <= t1);
 *   samples: dt = march_step / len (march_step is a world length), K = floor((t1 - t0) / dt) (a ray with K > 2^17 misses: overflow only, see
 *         the guard below), t_k = fma(k, dt, t0) for k = 0..K -- never accumulated --, g_k,a = min(max(fma(t_k, gd_a, go_a), 0), n_a - 1):
 *         the clip already put the sample into the box, the clamp takes the box faces away as a knife edge;
 *   cell i_a = min(floor(g_a), n_a - 2), t_a = g_a - i_a, validity cell_valid[i] and s_k = the eight-corner chain on `dist` exactly as
 *         d3f_volume_sample forms them; no corner of an invalid cell is read;
 *   decision, `prev` empty at first: an invalid sample empties prev (a hole is never bridged); a valid sample with prev > 0 and s_k <= 0
 *         is the HIT, t* = fma(dt, prev / (prev - s_k), t_{k-1}), and the march stops; any other valid sample becomes prev.  A crossing
 *         from - to + (a back face) is no hit, nor is a first valid sample <= 0.  No refinement beyond this interpolation.
 * Outputs per ray: out_t = t* (0 for a miss, the reference's "no depth"), out_hit one byte, out_points = fma(t*, d_a, o_a) (a NaN row
 * for a miss, which d3f_volume_sample answers with "not valid" and the fill rows), out_samples (may be NULL) the samples taken.
 * Rays: `camera` NULL: origins / dirs [n,3] on the device, one lane per ray in caller order.  `camera` non-NULL (HOST memory;
 * origins / dirs must be NULL and n == H*W): pixel (u, v), u the column, is ray v*W + u with dc = ((u - cx)/fx, (v - cy)/fy, 1),
 * d_a = fma(R[1][a], dc_y, R[0][a]*dc_x) + R[2][a] (= R^T dc) and o = -R^T tc, formed once per launch on the host in double and rounded;
 * pose = [R | tc] world -> camera, 3 x 4 row-major; of K only fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read.  d_cam,z = 1, so t is
 * the camera depth.  A wave takes an 8 x 8 pixel tile.
 * Status errors, never device-side checks: march_step not finite or <= 0; ceil(box diagonal / march_step) > 65536 (a bad argument must
 * not become a long kernel); t_near not finite or < 0; t_far NaN; n or H*W > 2^31 - 1; fx or fy zero or not finite; the volume checks
 * of d3f_volume_sample.  n == 0: D3F_OK, nothing is read.  One launch on `stream`; no atomics, no allocation, no synchronisation;
 * two runs agree bit for bit. */
#define D3F_RAYCAST_MAX_STEPS 65536
typedef struct d3f_pinhole {
    float K[9];                /* row-major 3 x 3 */
    float pose[12];            /* row-major 3 x 4, world -> camera */
    int32_t H, W;
} d3f_pinhole;
int d3f_volume_raycast(const d3f_volume *vol, const float *origins, const float *dirs, int64_t n, const d3f_pinhole *camera,
                       float march_step, float t_near, float t_far, float *out_t, uint8_t *out_hit, float *out_points,
                       int32_t *out_samples, void *stream);

/* fps_np (utils/my_utils.py:478-497): k samples of pts[n,3] starting from init_idx, float32 Euclidean distances,
 * first maximum wins -> out_idx[k] (int64, device), out_maxdist (device float, may be NULL).  k may exceed n: like
 * fps_np the selection then continues with index 0 (every distance is 0).  k + 1 small dependent launches on `stream`
 * (one per round over up to 256 workgroups, maxima merged by the next round); workspace: d3f_fps_workspace_bytes(n)
 * bytes of device scratch, 16-byte aligned. */
int64_t d3f_fps_workspace_bytes(int64_t n);
int d3f_farthest_point_sampling(const float *pts, int64_t n, int32_t k, int64_t init_idx, int64_t *out_idx,
                                float *out_maxdist, void *workspace, void *stream);

/* ---- point clouds on the mask side of the path (fp64, like the reference's numpy) ----------------------
 * depth2fgpcd (utils/my_utils.py:522-537) + camera->world transform + boundary crop of
 * aggr_point_cloud_from_data (utils/draw_utils.py:325-413) for one view.  depth [H,W] fp64 (device);
 * mask [H,W] bytes or NULL (NULL: foreground = 0 < depth < 1.5, as in the reference); cam_params = {fx, fy, cx,
 * cy}, cam_to_world = inv(pose) as 16 row-major doubles, bounds = {x_lower, x_upper, y_lower, y_upper,
 * z_lower, z_upper} or NULL -- these three are HOST arrays.  Survivors are written in ascending pixel order
 * (numpy's boolean-mask order): out_pts [capacity,3] fp64, out_pixel [capacity] int32 (row*W + col) or NULL,
 * count_out: one device int64 (may exceed capacity).  workspace: d3f_backproject_workspace_bytes(H,W). */
int64_t d3f_backproject_workspace_bytes(int32_t H, int32_t W);
int d3f_backproject_view(const double *depth, const uint8_t *mask, int32_t H, int32_t W, const double *cam_params,
                         const double *cam_to_world, const double *bounds, int64_t capacity, double *out_pts,
                         int32_t *out_pixel, int64_t *count_out, void *workspace, void *stream);

/* One direction of Fusion.pcd_iou's nearest-neighbour search (fusion.py:731-735): for every point of a[na,3]
 * the Euclidean distance to, and index of, its nearest point in b[nb,3], fp64, with np.min / np.argmin's rules: the first
 * minimum of the ROOTED distances wins (rows whose squares differ but whose roots are equal tie), and a NaN distance beats
 * every number (min_dist NaN, argmin the first such row). */
int d3f_pcd_nearest(const double *a, int64_t na, const double *b, int64_t nb, double *min_dist, int64_t *argmin,
                    void *stream);

/* ---- multi-view instance association: the integer steps (fusion.py:118-180, 794-849, 1279-1297, 1539-1606) ----
 * d3f_pcd_to_index = pcd_to_voxel + voxel_to_index of _init_low_level_memory (fusion.py:118-180):
 *   voxel = floor((p - lower) / voxel_size) as int32 (fp64 arithmetic, numpy's cast), index = v0*num[1]*num[2] +
 *   v1*num[2] + v2 in wrapping int32.  pts [n,3] fp64 (device); lower[3], voxel_num[3] are HOST arrays;
 *   out_index [n] int32; out_voxel NULL or [n,3] int32 (pcd_to_voxel's result). */
int d3f_pcd_to_index(const double *pts, int64_t n, const double *lower, double voxel_size, const int32_t *voxel_num,
                     int32_t *out_index, int32_t *out_voxel, void *stream);

/* Fusion.vox_idx_iou (fusion.py:794-799) on two int32 index arrays (duplicates allowed, any values):
 * out_counts[0] = |set(a) & set(b)|, out_counts[1] = |set(a) | set(b)| (two device int64); the reference's
 * triple is (counts[0]/counts[1], n1/counts[1], n2/counts[1]).  workspace: d3f_vox_iou_workspace_bytes(n1, n2)
 * bytes of device scratch (one hash set), only used inside the call. */
int64_t d3f_vox_iou_workspace_bytes(int64_t n1, int64_t n2);
int d3f_vox_idx_iou(const int32_t *idx1, int64_t n1, const int32_t *idx2, int64_t n2, int64_t *out_counts,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* cv2.erode(src, np.ones([kh, kw], np.uint8), iterations=1) on an [H,W] uint8 image (fusion.py:1293: 2x2 on a
 * 0/255 mask; fusion.py:1561: 15x15): minimum over the window anchored at (kw/2, kh/2), out-of-image samples
 * ignored (cv2's default border for erosion).  src != dst. */
int d3f_erode(const uint8_t *src, int32_t H, int32_t W, int32_t kh, int32_t kw, uint8_t *dst, void *stream);

/* Fusion.swap_instance_mask (fusion.py:1052-1063) for ONE view: dets [n_dets, n_pix] uint8 (non-zero = the pixel belongs to the
 * detection; the rows of curr_obs_torch['mask_gs'][view]), label_of_det[n_dets] int32 device = the consensus instance index
 * the detection was assigned to (instances_info[k]['idx'][view] == d  =>  label_of_det[d] = k), < 0 = none.  out[n_pix] uint8 =
 * what painting the detections in instance order leaves: the largest instance index covering the pixel (as uint8), 0 where
 * no assigned detection does. */
int d3f_compose_labels(const uint8_t *dets, int32_t n_dets, int64_t n_pix, const int32_t *label_of_det, uint8_t *out, void *stream);

/* open3d's PointCloud.voxel_down_sample as the reference uses it (utils/draw_utils.py:318-323 voxel_downsample, :396-400
 * inside aggr_point_cloud_from_data; radius 0.01): voxels of side voxel_size anchored at min_bound - voxel_size/2, one
 * output point (and colour) per occupied voxel = the mean of its points.  pts / colors [n,3] float64 (colors may be NULL),
 * out_pts / out_colors [n,3] capacity; *count_out (device int64) = the number of voxels.  Output order: ASCENDING voxel
 * index (x, then y, then z) -- open3d's order is that of its hash map, so the SETS agree (means to ~1e-14 m: the sums are
 * exact 64-bit fixed point, hence deterministic), the order does not.  Axis extent < 2^21 voxels. */
int64_t d3f_voxel_downsample_workspace_bytes(int64_t n);
int d3f_voxel_downsample(const double *pts, const double *colors, int64_t n, double voxel_size, double *out_pts,
                         double *out_colors, int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream);

/* The pixel side of select_features_rand_v2 (fusion.py:1554-1565), on the device:
 *   d3f_mask_gate       out(y,x) = 255 where mask(y,x) != 0 and depth_lo < depth(y,x) < depth_hi, else 0 -- the reference's
 *                       `mask.astype(bool) & (depth > 0.0) & (depth < 1.5)` as the uint8 image cv2.erode takes.  The mask
 *                       channel is read in place from the channels-last one-hot tensor: element (y,x) at
 *                       mask_channel[y*stride_y + x*stride_x] (ELEMENT strides); depth, out: [H,W] contiguous.
 *   d3f_nonzero_pixels  np.array(image.nonzero()).T: the (row, col) int32 pairs of the nonzero pixels in ascending row-major
 *                       order (order-preserving compaction).  out_row_col [capacity,2]; *count_out (device int64) = the
 *                       number found, also when it exceeds capacity; workspace: d3f_backproject_workspace_bytes(H, W). */
int d3f_mask_gate(const float *mask_channel, int64_t stride_y, int64_t stride_x, const float *depth, int32_t H, int32_t W,
                  float depth_lo, float depth_hi, uint8_t *out, void *stream);
int d3f_nonzero_pixels(const uint8_t *image, int32_t H, int32_t W, int64_t capacity, int32_t *out_row_col, int64_t *count_out,
                       void *workspace, void *stream);

/* fps_np (utils/my_utils.py:478-497) on integer 2-D points, as select_features_rand_v2 calls it on the (row, col)
 * indices of a mask (fusion.py:1565-1566): pts [n,2] int32, exact squared distances (numpy's float64 norms of
 * integer differences order identically), first maximum wins.  out_idx [k] int64, out_maxdist one device double
 * or NULL; workspace: d3f_fps_pixels_workspace_bytes(n) bytes, 16-byte aligned; k + 1 launches like d3f_farthest_point_sampling. */
int64_t d3f_fps_pixels_workspace_bytes(int64_t n);
int d3f_fps_pixels(const int32_t *pts, int64_t n, int32_t k, int64_t init_idx, int64_t *out_idx, double *out_maxdist,
                   void *workspace, void *stream);

/* Gradient of d3f_eval's outputs w.r.t. the query points: what autograd through Fusion.eval gives
 * the reference's rigid_tracking (fusion.py:1643-1665).  grad_dist: [n] or NULL; grad_fused: host
 * array of n_maps device pointers ([n,C_k], entries may be NULL); grad_pts [n,3] is overwritten.
 * Differentiable paths: projection -> bilinear coordinates, exp weight, clamped distance;
 * nearest-depth lookup, validity and the view count carry no gradient (as in torch).
 * Non-finite inputs: like d3f_eval, the call reads views->depth_nonfinite and every maps[k].nonfinite when ALL are
 * set; a point takes the strict form (every view, multiplied by its validity: 0 * NaN reaches grad_pts as in the
 * reference's autograd) where those words say non-finite, where they are absent, or where its projection is non-finite.
 * With all words zero the other points skip their invalid views (exact for finite operands).  Same signature and structs
 * as before (the words are the ABI 4 fields d3f_eval reads). */
int d3f_eval_backward(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps,
                      int32_t n_maps, float mu, const float *grad_dist, const float *const *grad_fused,
                      float *grad_pts, void *stream);

/* Locality of the caller's point order, decided on the device without a sort: out[0] = mean L1 step between
 * consecutive points, out[1] = mean L1 distance between points n/2 apart (<= 4096 evenly spaced samples,
 * non-finite pairs skipped).  out: 2 floats of DEVICE memory, written asynchronously on `stream`.
 * A grid / mesh / scan-ordered cloud gives out[0] << out[1]; the shim passes D3F_FLAG_UNORDERED_POINTS when
 * out[0] > 0.25 * out[1] (random clouds on patch-resolution maps: 1.93 -> 0.88 ms per 985 600 points). */
int d3f_point_order_locality(const float *pts, int64_t n, float *out, void *stream);

/* (ABI 6) d3f_lattice_probe AND d3f_point_order_locality in ONE launch, with nothing to clear beforehand: every one of the
 * D3F_PROBE_WORDS device words of `out` is written by the call.  out[0..2] = (nx, ny, nz) of the lattice or zeros; out[8 + b],
 * b < 16: non-zero when sample block b contradicts those dims (a lattice iff out[0] > 0 and all sixteen are zero);
 * out[24 + 3q .. 24 + 3q + 2], q < 4, as FLOATS: sum of the steps between consecutive points, sum of the distances between
 * points n/2 apart, number of finite samples of locality block q (mean step = sum of the first / sum of the third). */
#define D3F_PROBE_WORDS 40
int d3f_points_probe(const float *pts, int64_t n, int32_t *out, void *stream);

/* The same for Fusion.eval_dist: d(dist)/d(pts) = -mean over the valid views of row 2 of K@pose. */
int d3f_eval_dist_backward(const d3f_views *views, const float *pts, int64_t n, const float *grad_dist,
                           float *grad_pts, void *stream);

/* Replaces Fusion.eval_dist (fusion.py:396-436): no -mu gate, no clamp, no 1e3 sentinel. */
int d3f_eval_dist(const d3f_views *views, const float *pts, int64_t n, float *out_dist,
                  uint8_t *out_valid, void *stream);

/* ---- instance-mask helpers ----------------------------------------------------------
 * onehot2instance (fusion.py:109-116): argmax over the last dim -> uint8 (first max wins,
 * NaN counts as maximum, like torch.argmax).  instance2onehot (fusion.py:90-107). */
int d3f_onehot2instance(const float *onehot, int64_t n, int32_t NI, uint8_t *out, void *stream);
int d3f_instance2onehot(const uint8_t *instance, int64_t n, int32_t NI, uint8_t *out_bool,
                        void *stream);

/* ---- descriptor similarity (utils/corr_utils.py) --------------------------------------- */
#define D3F_DIST_L2 0     /* dist_type='l2'     : sqrt(sum (a-b)^2)                        */
#define D3F_DIST_SQUARE 1 /* dist_type='square' : sum (a-b)^2                              */

#define D3F_SIM_DIST 0         /* raw distance            compute_dist_tensor  corr_utils.py:44-61 */
#define D3F_SIM_EXP 1          /* exp(-d*scale)           compute_similarity   corr_utils.py:4-19  */
#define D3F_SIM_SOFTMAX_DIM0 2 /* softmax(-d*scale,dim=0) compute_similarity_tensor :21-42,
                                                          compute_similarity_tensor_multi :63-106 */

/* Device scratch needed by the D3F_SIM_SOFTMAX_DIM0 mode (and by argmax_out) for a
 * [rows, cols] result: per-column running max / sum-exp / argmax of each 64-row chunk. */
int64_t d3f_softmax_workspace_bytes(int64_t rows, int64_t cols);

/* Feature map vs ONE target descriptor.  src holds B*inner descriptors of C channels:
 * descriptor (b,j) channel c at src[b*stride_b + j*stride_i + c*stride_c] (elements), which
 * covers both [B,H,W,C] (compute_similarity) and [B,C,*dim] (compute_*_tensor).
 * out [B*inner].  D3F_SIM_SOFTMAX_DIM0 normalises over b for every j and needs
 * workspace >= d3f_softmax_workspace_bytes(B, inner); other modes accept NULL/0. */
int d3f_similarity_to_target(const float *src, int64_t B, int64_t inner, int32_t C,
                             int64_t stride_b, int64_t stride_i, int64_t stride_c,
                             const float *tgt, float scale, int32_t dist_type, int32_t mode,
                             float *out, void *workspace, int64_t workspace_bytes, void *stream);

/* compute_similarity_tensor_multi (corr_utils.py:63-106): src [B1,C], tgt [B2,C] ->
 * out [B1,B2]; the [B1,B2,C] difference tensor of the reference (and its OOM retry,
 * corr_utils.py:84-94) never exists.  `scale` is ignored by D3F_SIM_DIST.
 * argmax_out: NULL or [B2] int64, the row index of the best match of each target, always in [0, B1).  In
 *   D3F_SIM_DIST / D3F_SIM_EXP mode the smallest distance (scale unused); in D3F_SIM_SOFTMAX_DIM0 mode
 *   the largest logit -scale*d in float32, first (lowest) row wins; a row whose logit is NaN never wins, and a column
 *   where every logit is NaN gives row 0 (the reference's argmax of an all-NaN softmax column).  For scale > 0 that is
 *   the smallest distance (+Inf before NaN, ties to the lower row) -- k-NN's first neighbour -- up to the rounding of
 *   d*scale (distances whose logits round equal tie).  For scale < 0 it is the largest distance; for scale == 0 the
 *   first row whose distance is finite.  Distances come from a guarded contraction when B1 >= 512 and C % 32 == 0
 *   (INTEGRATION.md): within 2e-6 relative of float64, so near-equal distances may rank either way.
 * workspace: >= d3f_softmax_workspace_bytes(B1, B2) bytes when mode is D3F_SIM_SOFTMAX_DIM0 or
 * argmax_out is given; only read/written inside the call. */
int d3f_pairwise_similarity(const float *src, const float *tgt, int64_t B1, int64_t B2, int32_t C,
                            float scale, int32_t dist_type, int32_t mode, float *out,
                            int64_t *argmax_out, void *workspace, int64_t workspace_bytes,
                            void *stream);

/* k-nearest-descriptor lookup (k <= 8): d3f_pairwise_similarity plus, per target column, the rows of the k SMALLEST
 * distances -- the k-NN generalisation of the reference's best match, compute_similarity_tensor_multi(...).argmax(0)
 * (the reference has no KNN of its own; this is what the north star's "KNN correspondence lookup" maps
 * to).  Neighbours are chosen on the raw distances (ties -> lower row index, NaN last: after +Inf, NaN rows by index), before exp / softmax can round
 * close values into ties.  topk_idx [k,B2] int64 (row j = the j-th nearest; -1 where B1 < k), topk_val [k,B2] or NULL:
 * the entries of `out` (in `mode`) at those rows.  workspace >= d3f_pairwise_topk_workspace_bytes(B1, B2), 16-B aligned. */
int64_t d3f_pairwise_topk_workspace_bytes(int64_t B1, int64_t B2);
int d3f_pairwise_similarity_topk(const float *src, const float *tgt, int64_t B1, int64_t B2, int32_t C, float scale,
                                 int32_t dist_type, int32_t mode, int32_t k, float *out, int64_t *topk_idx,
                                 float *topk_val, void *workspace, int64_t workspace_bytes, void *stream);

/* The two halves of the k-NN lookup for ROW-SHARDED sources (d3fields_amd/sharding.py: sharded_knn_descriptors):
 *   d3f_topk_smallest  per column of a [rows, cols] matrix (a rank's raw distances) the rows of the k smallest entries (ties ->
 *                      lower row, NaN last: after +Inf): idx_out [k,cols] int64 (-1 where rows < k), val_out [k,cols] or NULL;
 *                      workspace >= d3f_pairwise_topk_workspace_bytes(rows, cols), 16-byte aligned.
 *   d3f_topk_merge     n_parts such lists (indices already GLOBAL rows) -> the k best per column by (value, index), NaN after +Inf;
 *                      parts_idx / parts_val [n_parts, k, cols]; entries with index < 0 are padding. */
int d3f_topk_smallest(const float *x, int64_t rows, int64_t cols, int32_t k, int64_t *idx_out, float *val_out,
                      void *workspace, int64_t workspace_bytes, void *stream);
int d3f_topk_merge(const int64_t *parts_idx, const float *parts_val, int64_t n_parts, int32_t k, int64_t cols,
                   int64_t *out_idx, float *out_val, void *stream);

/* ---- the same softmax with B1 sharded over GPUs -------------------------------
 * softmax(dim=0) of compute_similarity_tensor_multi (corr_utils.py:102) couples all B1 rows.  With the
 * rows split over ranks each rank runs
 *   1. d3f_pairwise_softmax_local : raw distances of ITS rows into out [B1_local,B2] and, per target
 *      column, the running statistics of -d*scale over its rows -> stats [B2]
 *      (argmax = row_offset + local row of the first maximum; B1_local == 0, or a column whose every logit is NaN,
 *      gives (-inf, *, INT64_MAX), which loses every merge);
 *   2. an all-gather of the 16-B records (the only exchange step; host side, RCCL);
 *   3. d3f_softmax_merge : [n_parts,B2] records in rank order -> merged [B2] (+ global argmax, first wins; a column
 *      without a winner gets 0, as d3f_pairwise_similarity's argmax_out);
 *   4. d3f_softmax_apply : out = exp(-out*scale - max) / sum in place.
 * workspace of step 1: >= d3f_softmax_workspace_bytes(B1_local, B2). */
typedef struct d3f_col_stat {
    float max_logit; /* max over rows of -d*scale               */
    float sum_exp;   /* sum over rows of exp(-d*scale - max)    */
    int64_t argmax;  /* global row index of the first maximum   */
} d3f_col_stat;

int d3f_pairwise_softmax_local(const float *src, const float *tgt, int64_t B1_local, int64_t B2, int32_t C,
                               float scale, int32_t dist_type, int64_t row_offset, float *out,
                               d3f_col_stat *stats, void *workspace, int64_t workspace_bytes, void *stream);
int d3f_softmax_merge(const d3f_col_stat *parts, int64_t n_parts, int64_t cols, d3f_col_stat *merged,
                      int64_t *argmax_out, void *stream);
int d3f_softmax_apply(float *x, int64_t rows, int64_t cols, float scale, const d3f_col_stat *merged,
                      void *stream);

/* ---- the optimiser step of Fusion.rigid_tracking (fusion.py:1608-1685) ---------------------------------
 * One step of the reference is  so3_exp_map -> rigid transform -> Fusion.eval -> loss -> autograd -> Adam
 * (pytorch3d + ~90 torch launches).  Around d3f_eval / d3f_eval_backward the rest is closed-form:
 *   1. d3f_rigid_transform : per instance i, R_i = so3_exp_map(w_i) (pytorch3d 0.7.5: Rodrigues, angle clamped
 *      at sqrt(1e-4)), out_pts[i,p] = last[i,p] @ R_i + t_i (row-vector convention); norms[0..1] = |t|_F, |w|_F.
 *   2. d3f_eval on out_pts (one channel map: the descriptors).
 *   3. d3f_track_loss_grad : loss[0] = mean(|f - src| * valid), loss[1] = dist_w * mean(max(dist*valid, 0))
 *      (fusion.py:1654-1657) and their gradients w.r.t. f and dist.
 *   4. d3f_eval_backward -> grad_pts.
 *   5. d3f_rigid_update : chain rule through the transform and the exponential map, + reg_w * d(|t|_F + |w|_F)
 *      (fusion.py:1658), then torch.optim.Adam's update of (t_i, w_i); adam_m / adam_v [n_inst,6] and
 *      step [n_inst] (float counters) are the optimiser state, zero at the start of a frame.
 * All arrays are device memory; last [n_inst,n,3], t / w [n_inst,3], valid = the uint8 mask of d3f_eval. */
int d3f_rigid_transform(const float *last, int32_t n_inst, int32_t n, const float *t, const float *w,
                        float *out_pts, float *norms, void *stream);
int d3f_track_loss_grad(const float *feats, const float *src, const float *dist, const uint8_t *valid,
                        int64_t N, int32_t C, float dist_w, float *grad_feats, float *grad_dist,
                        float *loss, void *stream);
int d3f_rigid_update(const float *last, int32_t n_inst, int32_t n, const float *grad_pts, float *t, float *w,
                     float *adam_m, float *adam_v, float *step, const float *norms, float reg_w, float lr,
                     float beta1, float beta2, float eps, void *stream);

/* The same optimiser step as ONE launch: a wave per keypoint transforms it, queries the descriptor field, forms the
 * loss gradient and back-propagates it to the keypoint with the corner texels held in registers; the last wave to
 * finish reduces per instance and steps Adam.  One descriptor map: fp32, C % 4 == 0, C <= 512, 16-byte aligned texels,
 * at most 8 views (otherwise D3F_ERR_BAD_SHAPE / D3F_ERR_BAD_LAYOUT: use the five launches above).  `state` holds device
 * pointers owned by the caller: t / w [n_inst,3] (updated in place), adam_m / adam_v [n_inst,6], step [n_inst] (float
 * counters), out_pts [n_inst*n,3] (the keypoints as evaluated in this step -- what rigid_tracking returns after its last
 * step), loss [3] (feature term, distance term, regulariser of this step) and scratch of
 * d3f_track_step_scratch_bytes(n_inst, n) bytes that must be ZERO before the first step of a frame (every step leaves
 * it zero again).  src [n_inst*n, C]: the instances' source descriptors. */
typedef struct d3f_track_state {
    float *t, *w;
    float *adam_m, *adam_v;
    float *step;
    float *out_pts;
    float *loss;
    void *scratch;
} d3f_track_state;
int64_t d3f_track_step_scratch_bytes(int32_t n_inst, int32_t n);
int d3f_track_step(const d3f_views *views, const d3f_channel_map *descriptors, const float *last, int32_t n_inst, int32_t n,
                   const float *src, float mu, float dist_w, float reg_w, float lr, float beta1, float beta2, float eps,
                   const d3f_track_state *state, void *stream);

/* `iters` optimiser steps (the whole loop of fusion.py:1650-1665 for one frame) in ONE launch: the waves of step k+1 wait
 * inside the kernel for the Adam update of step k (a device-wide arrival counter and step-tagged parameter words in `scratch`),
 * so K / pose / the source descriptors are read once per frame and no launch boundary separates the steps.  Same
 * arithmetic per step as d3f_track_step (same t / w / out_pts / loss as `iters` calls of it).  Every workgroup must be
 * resident while the others wait: n_inst*n <= d3f_track_run_max_keypoints() and n_inst <= 16, else D3F_ERR_BAD_SHAPE -- call
 * d3f_track_step per iteration then.  d3f_track_run_max_keypoints() is derived at run time for the CURRENT device: the
 * occupancy of the kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor) x its compute units, half of that (the other half is
 * left to whatever else runs), at most 512.  The wait is bounded: should a wave never see the next step's parameters (the
 * device held by other kernels for seconds), loss[0..2] become NaN, the launch ends, and t / w / the optimiser state are
 * UNDEFINED.  The kernel also leaves D3F_TRACK_STALL_SENTINEL in the uint32 at word d3f_track_stall_word(n_inst, n) of `scratch`
 * (ABI 5): a NaN loss WITHOUT the sentinel came out of the data, not out of a stall.  A caller that shares the device reads that
 * word, restores its state and repeats the frame with d3f_track_step (d3fields_amd/rigid.py: RigidTracker.run does exactly
 * that).  scratch is cleared at the start of every
 * d3f_track_run (a one-workgroup launch ahead of the step kernel); d3f_track_step expects the scratch its predecessor left. */
#define D3F_TRACK_STALL_SENTINEL 0x57A11EDu
int64_t d3f_track_stall_word(int32_t n_inst, int32_t n);      /* index (in 4-byte words) of the sentinel inside `scratch` */
int d3f_track_run(const d3f_views *views, const d3f_channel_map *descriptors, const float *last, int32_t n_inst, int32_t n,
                  const float *src, float mu, float dist_w, float reg_w, float lr, float beta1, float beta2, float eps,
                  int32_t iters, const d3f_track_state *state, void *stream);
int32_t d3f_track_run_max_keypoints(void);

#ifdef __cplusplus
}
#endif
#endif /* D3FIELDS_HIP_H */
