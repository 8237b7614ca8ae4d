// d3f_internal.h -- declarations shared by the kernels and the C-ABI layer (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/d3fields_hip.h"
#include "d3f_workspace.h"

// the planner's kernel families (d3f_plan.h: kFamilies; the value of d3f_eval_plan.family)
enum FamilyId { kFamDistOnly = 0, kFamWindow, kFamRuns, kFamSliced, kFamDirect, kFamRows };

namespace d3f {

constexpr int kBlock = 256;                 // 4 waves of 64 lanes
#ifndef D3F_ROWS_PTS
#define D3F_ROWS_PTS 32                     // points per workgroup of the register-rows kernel (fuse_rows.hip; 16: a build-time experiment)
#endif
constexpr uint32_t kFlagFiniteMaps = D3F_FLAG_FINITE_MAPS;
constexpr uint32_t kFlagXcdRemap = D3F_TUNE_XCD_REMAP;

// One channel map as the kernel sees it (strides in elements, channel stride 1).
struct MapDesc {
    const float *data;
    float *out;      // [n, C]
    float *inter;    // [V, n, C] or nullptr
    int64_t sv, sy, sx;
    int32_t fh, fw, C;
    int32_t vw;        // channel-vector width in floats: 4, 2 or 1
    int32_t lpp_log2;  // log2(lanes per point) in phase B
    int32_t unroll;    // channel vectors per lane per pass: +1..+3 batched loads, -1..-4 load-use per vector
    int32_t pre_slot;  // >= 0: bilinear corner set-up of this map is precomputed per (point, view) in LDS slot pre_slot
    int32_t esize;     // bytes per stored channel: 4 (fp32) or 2 (fp16 storage, widened on load)
    int32_t runs;      // > 0: cell-run gather (gather_map_runs): a lane group walks `runs` consecutive points view by view
    int32_t fold;      // 1: wide map -- on the fast path the view weight and the reciprocal of the view count are folded into
                       //    the four bilinear weights once per (point, view): 4 fma per channel vector
};

struct EvalParams {
    const float *depth, *K, *pose, *pts;
    const uint32_t *order;  // nullptr, or n point indices: the kernel processes points in this order
    const float *grid_x, *grid_y, *grid_z;   // regular-grid mode (pts == nullptr): axis coordinate arrays
    int32_t grid_ny, grid_nz;
    float *out_dist;
    uint8_t *out_valid;
    int64_t n;
    int32_t V, H, W;
    int32_t n_maps;
    int32_t tile_pts;  // points per workgroup
    int32_t lds_pad;   // extra dynamic LDS bytes (occupancy throttle, tuning only)
    int32_t crec_offset;   // byte offset of the precomputed corner records, 16-B aligned
    int32_t n_pre;         // number of maps with precomputed corner records
    int32_t xcd_chunk;     // tiles per XCD-mapping chunk (multiple of 8), 0 = the whole launch
    // lattice walk: the n = walk_nx*walk_ny*walk_nz points form a regular lattice in index space (flat index
    // (ix*ny + iy)*nz + iz); workgroups take bricks of walk_tx x walk_ty x walk_tz points in a blocked order computed
    // from blockIdx alone (no keys, no sort, no index array).  walk_nx == 0: off.
    int32_t walk_nx, walk_ny, walk_nz;
    int32_t walk_tx, walk_ty, walk_tz;
    // channel-sliced launch (fused_eval_sliced_kernel): sl_slices > 0 selects it
    int32_t sl_unit;                   // workgroups (of 32 points) per unit
    int32_t sl_ilv;                    // units an XCD works on at the same time (1: one after the other)
    int32_t sl_slices, sl_lg, sl_vc;   // slices per texel of map 0, log2(lanes per point), views with loads in flight
    int64_t sl_tiles, sl_groups, sl_chunks;   // walk tiles, groups of 4 tiles, chunks of 128 groups
    // LDS texel windows (fused_eval_window_kernel): win_slices > 0 selects it
    int32_t win_slices;        // channel slices of 128 * win_u channels per texel of map 0 (looped inside the workgroup)
    int32_t win_u, win_vc;     // 16-byte vectors per lane (1..4), views with corner reads in flight
    int32_t win_pipe;          // 1 (default): software-pipelined point loop when the view count is 4 or 8
    int32_t win_pool_offset;   // byte offset of the two all-zero slices; the pool follows them
    int32_t win_pool_texels;   // pool capacity in texel slices of 512 * win_u bytes
    int32_t win_occ;           // workgroups per CU the kernel variant is built for (2 / 3 / 4)
    int32_t win_lpp;           // lanes per point in phase B: 32, or 16 (two vectors per lane inside a 512-byte slice)
    int32_t win_sparse;        // 1: the pool holds only the texels the tile's pairs touch (bitmap + ranks), 0: the views' whole rectangles
    int32_t rows;              // 1: the register-rows kernel (fuse_rows.hip): 32 points per workgroup, their fused rows in registers
    int32_t thin_max_views;    // 8 (default): thin maps with 2..8 views are gathered with the views in parallel across lanes
                               // (gather_map_thin); 0 switches that off (D3F_EXP_THIN=-1, tests)
    int32_t runs_occ;      // experiment: waves per SIMD of the (1,8) cell-run kernel variant (4 / 5 / 6)
    // the distance-only pass on a big batch (fuse_direct.hip): a copy of the depth maps in tiles of 4 x 8 pixels (one 128-byte line
    // each), [V][depth_th][depth_tw][8][4]; nullptr: the caller's row-major maps
    const float *depth_tiled;
    int32_t depth_tw, depth_th;
    int32_t dist_variant;  // the distance-only pass: 0 = fused_eval_dist_kernel, 8 = held to eight waves per SIMD with three and more views too, + 16 = the compiler's divisions, + 32 = no tiled depth copy, -1 = the branch of fused_eval_kernel (rounds 1-5)
    int32_t store_policy;  // 2 (default) = fused rows leave as non-temporal stores (nt), 3 = sc1 nt (the window kernel's own form), 1 = sc1, 0 = plain
    uint32_t flags;
    float mu;
    // device-side "this tensor holds a non-finite value" words written by d3f_map_check (depth first, then one per map);
    // n_words == 0: the host's D3F_FLAG_FINITE_MAPS alone decides.  All words zero <=> the exact invalid-view skip is allowed.
    int32_t n_words;
    int32_t walk_snake;    // lattice walk: 1 = the 16-tile macro-bricks are walked as a serpentine (fuse_common.h: walk_tile; set by
                           // the channel-sliced family for fp32 maps).  Here it takes the four bytes that were padding.
    const uint32_t *words[D3F_MAX_MAPS + 1];
    // device-side choice between the window kernel and the cell-run kernel for a cloud (fuse_common.h: gated_out)
    const uint32_t *gate;  // nullptr: this launch is not gated
    uint32_t gate_min;     // the window side runs iff *gate >= gate_min, the cell-run side iff *gate < gate_min
    int32_t gate_want;     // 1: the window side, 0: the cell-run side
    unsigned long long *exp_stamps;   // experiments builds (D3F_EXP_STAMPS=1): s_memtime stamps of every 64th workgroup's phases; else nullptr
    MapDesc maps[D3F_MAX_MAPS];
};

// LDS bytes in front of the stage buffers: records, cnt/flag/idx, KRt, per-view windows
inline int fused_lds_base(int tile_pts, int V) { return ((tile_pts * V * 24 + tile_pts * 12 + V * 48 + V * 16) + 15) / 16 * 16; }

// ---- which kernel instance a plan launches ----------------------------------------------------------------------------------------
// The planner (d3f_plan.h) decides the family; inside a family ONE list next to its launcher (fuse_<family>.hip) holds the built
// instances, one row each: D3F_VARIANT(condition on EvalParams, legacy code, instance), walked top down.  The first row whose
// condition holds launches its instance -- or, for a plan query, only reports it: the printed name is the row's own text, so what
// d3f_eval_plan.kernel names is what runs, and d3f_eval_plan.reserved is the row's code.
struct Launch {
    int64_t workgroups;        // plan_workgroups (d3f_plan.h)
    hipStream_t stream;
    d3f_eval_plan *describe;   // a plan query: the row fills kernel / reserved here and nothing is launched; nullptr: launch
};
template <typename K>
inline hipError_t take_variant(const Launch &L, K kernel, const char *name, int code, size_t lds, const EvalParams &P, bool opt_in_lds)
{
    if (L.describe) {
        snprintf(L.describe->kernel, sizeof(L.describe->kernel), "%s", name);
        L.describe->reserved = code;
        return hipSuccess;
    }
    if (opt_in_lds && lds > 64 * 1024) {
        hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)L.workgroups), dim3(kBlock), lds, L.stream, P);
    return hipGetLastError();
}
// (expects `L`, `lds` and `P` in scope; returns from the launcher when the row is taken.  A row is a bare `if`, and the families'
//  own row macros expand to several: statement position only, never under an unbraced if / else)
#define D3F_VARIANT_LDS(OPT_IN, COND, CODE, ...) if (COND) return take_variant(L, __VA_ARGS__, #__VA_ARGS__, CODE, lds, P, OPT_IN)
#define D3F_VARIANT(COND, CODE, ...) D3F_VARIANT_LDS(false, COND, CODE, __VA_ARGS__)

hipError_t launch_fused_eval(const EvalParams &P, FamilyId family, int mode, const Launch &L);      // fuse_launch.hip: the family's launcher
hipError_t launch_direct(const EvalParams &P, const Launch &L);                       // fuse_direct.hip
hipError_t launch_dist(const EvalParams &P, int mode, const Launch &L);               // fuse_direct.hip: the distance-only pass
hipError_t launch_depth_tiles(const EvalParams &P, float *tiled, hipStream_t stream);  // fuse_direct.hip: fills EvalParams::depth_tiled's buffer
inline int64_t depth_tiled_bytes(int V, int H, int W) { return (int64_t)V * ((H + 7) / 8) * ((W + 3) / 4) * 128; }
constexpr int64_t kDistTiledMin = 1LL << 22;      // the distance-only pass tiles the depth maps first from this many points on
hipError_t launch_runs(const EvalParams &P, const Launch &L);                         // fuse_runs.hip
hipError_t launch_sliced(const EvalParams &P, const Launch &L);                       // fuse_sliced.hip
hipError_t launch_window(const EvalParams &P, const Launch &L);                       // fuse_window.hip
hipError_t launch_rows(const EvalParams &P, const Launch &L);                         // fuse_rows.hip
constexpr int kGateSamples = D3F_GATE_SAMPLES;            // tiles the probe looks at (evenly spaced over the order)
hipError_t launch_window_gate_probe(const EvalParams &P, uint32_t *gate, int nsamples, hipStream_t stream);

// fuse_backward.hip
struct BackwardParams {
    const float *depth, *K, *pose, *pts;
    const float *grad_dist;                    // [n] or nullptr
    const float *grad_fused[D3F_MAX_MAPS];     // [n, C_k] or nullptr
    float *grad_pts;                           // [n, 3]
    int64_t n;
    int32_t V, H, W;
    int32_t n_maps;
    int32_t tile_pts;
    float mu;
    // d3f_map_check words of depth + every map (n_words = 0: unknown, every point takes the strict form)
    const uint32_t *words[D3F_MAX_MAPS + 1];
    int32_t n_words;
    MapDesc maps[D3F_MAX_MAPS];                // out / inter unused
};
hipError_t launch_fused_backward(const BackwardParams &P, int mode, hipStream_t stream);

// scan_kernels.hip: exclusive prefix sum of uint32 counters (in == out allowed); scratch laid out by scan_layout(n)
struct ScanLayout { int64_t sums[6], spare, total; int64_t blocks[6]; int levels; };
ScanLayout scan_layout(int64_t n);
int64_t scan_scratch_bytes(int64_t n);      // scan_layout(n).total
hipError_t launch_exclusive_scan_u32(const uint32_t *in, uint32_t *out, int64_t n, void *scratch, hipStream_t s);
int64_t scan_status_words(int64_t n);      // single-launch form (decoupled look-back): zeroed status words, total < 2^30
hipError_t launch_exclusive_scan_lookback_u32(const uint32_t *in, uint32_t *out, int64_t n, uint32_t *status, hipStream_t s);

// order_kernels.hip; gate: the word of the gated pair of launches (4 words are cleared), public as d3f_eval_gate_offset
struct OrderLayout { int64_t keys, ranks, order, slots, table, scan, gate, parts, total; };
OrderLayout order_layout(int64_t n);
int64_t order_workspace_bytes(int64_t n);   // 0 for n <= 0, else order_layout(n).total
hipError_t build_point_order(const float *pts, int64_t n, void *workspace, int64_t workspace_bytes,
                             const uint32_t **order_out, hipStream_t stream, int fine = 0);
// is pts a z-fastest lattice?  out: 3 device int32 (nx, ny, nz), zeros when not
hipError_t launch_lattice_probe(const float *pts, int64_t n, int32_t *out_dims, hipStream_t stream);
// mean L1 step between consecutive points vs between points n/2 apart (out: 2 device floats)
hipError_t launch_point_locality(const float *pts, int64_t n, float *out, hipStream_t stream);
// both probes in one launch; out: D3F_PROBE_WORDS device words, every one written (no clearing needed)
hipError_t launch_points_probe(const float *pts, int64_t n, int32_t *out, hipStream_t stream);

// grid_kernels.hip
hipError_t launch_grid_shell(const float *depth, const float *K, const float *pose, int V, int H, int W, const float *gx,
                             const float *gy, const float *gz, int nx, int ny, int nz, float mu, float dist_thr,
                             int64_t capacity, int64_t *idx_out, unsigned long long *count, void *workspace, hipStream_t s,
                             float *tiled_scratch);
struct ShellLayout { int64_t ballots, counts, offsets, scan, total; int64_t blocks; };
ShellLayout grid_shell_layout(int64_t n);
struct ShellTiledLayout { int64_t shell, tiles, total; };
ShellTiledLayout grid_shell_tiled_layout(int64_t n, int64_t tiled_bytes);
hipError_t launch_fps(const float *pts, int64_t n, int k, int64_t init_idx, int64_t *out_idx, float *out_maxdist,
                      void *workspace, hipStream_t s);
struct FpsLayout { int64_t dist, maxima, total; };
FpsLayout fps_layout(int64_t n, int dist_bytes);            // dist_bytes: 4 (d3f_farthest_point_sampling) or 8 (d3f_fps_pixels)
constexpr int kFpsMaxBlocks = 256;                          // entries per round parity of fps_layout's `maxima`: one per workgroup of a round
int64_t fps_blocks(int64_t n);                              // workgroups of one round, 1..kFpsMaxBlocks (tests/layout_check.cpp holds it to the table)

// mesh_kernels.hip
struct MeshLayout { int64_t voff, toff, scan, total; int64_t blocks; };
MeshLayout mesh_layout(int64_t n);
hipError_t launch_mesh(const float *vol, const uint8_t *valid, int nx, int ny, int nz, float iso, int64_t vertex_capacity,
                       int64_t triangle_capacity, int64_t *keys, float *ts, int32_t *tris, int64_t *counts_out, void *workspace,
                       bool extract, hipStream_t s);
constexpr int kGaussMaxRadius = D3F_GAUSSIAN_MAX_RADIUS;
hipError_t launch_volume_gaussian(const float *src, float *dst, int nx, int ny, int nz, const float *weights, int radius, float *tmp,
                                  hipStream_t s);

// volume_kernels.hip: trilinear lookups in a baked volume
constexpr int kVolNarrowMax = 16;           // channels of a set sampled one lane per point; a wider set takes sixteen lanes per point
struct VolSet {
    const float *data;       // row of voxel q: data + q * stride (f16: in halves, from the same address)
    const float *fill;       // C floats or nullptr (zeros): the row of a point that is not valid
    float *out;              // forward: [n, C]
    const float *grad;       // backward: [n, C] or nullptr
    int64_t stride;
    int32_t C;
    int32_t vec;             // 1: rows (and out / grad rows) move as 16-byte vectors
    int32_t f16;             // 1: the rows are IEEE half (D3F_DTYPE_F16): d3f_volume_sample / d3f_band_sample and their backwards only
};
struct VolParams {
    const float *dist;
    const uint8_t *cell;     // [nx-1, ny-1, nz-1]
    const float *pts;
    float *out_dist;         // forward
    uint8_t *out_valid;
    const float *grad_dist;  // backward: [n] or nullptr
    float *grad_pts;         // backward: [n, 3]
    int64_t n;
    int32_t nx, ny, nz;
    float ox, oy, oz, h, rh; // rh = 1 / h
    int32_t n_sets;
    VolSet sets[D3F_MAX_MAPS];
};
hipError_t launch_volume_cell_valid(const uint8_t *valid, uint8_t *cell, int nx, int ny, int nz, hipStream_t s);
hipError_t launch_volume_sample(const VolParams &P, hipStream_t s);
hipError_t launch_volume_backward(const VolParams &P, hipStream_t s);

// band_kernels.hip: a baked volume whose channel rows exist only near the surface
struct BandParams {
    VolParams V;               // sets[s].data / stride: the COMPACTED rows [n_rows, C] and their row stride
    const int32_t *slot;       // [nx, ny, nz]: the row of a stored voxel, -1 elsewhere
    const uint8_t *cell_band;  // [nx-1, ny-1, nz-1], or nullptr (n_rows == 0): no point is in the band, nothing of the band is read
    uint8_t *out_in_band;      // forward: [n]
};
int64_t band_workspace_bytes(int64_t n);
hipError_t launch_band_mark(const float *dist, const uint8_t *cell_valid, int nx, int ny, int nz, float band, uint8_t *cell_band, int32_t *slot,
                            int32_t *voxels, int64_t capacity, int64_t *count, void *workspace, hipStream_t s);
hipError_t launch_band_sample(const BandParams &B, hipStream_t s);
hipError_t launch_band_backward(const BandParams &B, hipStream_t s);

// edt_kernels.hip: the exact Euclidean distance transform of a site volume; cap: max_d2, or INT32_MAX for none
struct EdtLayout { int64_t B, A, total; };
EdtLayout edt_layout(int64_t n);
hipError_t launch_volume_edt(const uint8_t *site, int nx, int ny, int nz, float step, int32_t cap, int32_t *out_d2, int32_t *out_nearest, float *out_dist,
                             void *workspace, hipStream_t s);

// ccl_kernels.hip: connected components of a site volume
struct CclLayout { int64_t parent, size, rank, scan, total; };
CclLayout ccl_layout(int64_t n);
hipError_t launch_volume_components(const uint8_t *site, int nx, int ny, int nz, int connectivity, int min_voxels, int32_t *out_label, int32_t *out_count,
                                    int32_t *out_stats, int capacity, void *workspace, hipStream_t s);
hipError_t launch_volume_components_linked(const uint8_t *site, const uint16_t *links, int nx, int ny, int nz, int connectivity, int min_voxels,
                                           int32_t *out_label, int32_t *out_count, int32_t *out_stats, int capacity, void *workspace, hipStream_t s);

// parts_kernels.hip: descriptor-gated links between neighbouring voxels; vec: rows may move as 16-byte vectors
hipError_t launch_volume_links(const uint8_t *site, const uint8_t *valid, const int32_t *slot, int nx, int ny, int nz, const float *data, int C, int64_t stride,
                               bool vec, int rule, float threshold, int connectivity, uint16_t *out, hipStream_t s);

// flow_kernels.hip: dense descriptor flow between two fields on one grid; vec: the rows of BOTH sets may move as 16-byte vectors
hipError_t launch_volume_flow(const uint8_t *site_a, const int32_t *slot_a, const float *data_a, int64_t stride_a, const uint8_t *site_b, const int32_t *slot_b,
                              const float *data_b, int64_t stride_b, int C, bool vec, int nx, int ny, int nz, int radius, float max_cost2, int32_t *out_target,
                              float *out_cost, float *out_axis_cost, hipStream_t s);
// ... its axis-cost pass alone (flow_axis_kernel), from targets already written: shared with the seeded flow, whose rule is the same
hipError_t launch_flow_axis(const int32_t *slot_a, const float *data_a, int64_t stride_a, const uint8_t *site_b, const int32_t *slot_b, const float *data_b,
                            int64_t stride_b, int C, int nx, int ny, int nz, const int32_t *target, float *out_axis_cost, hipStream_t s);

// flow_seeded_kernels.hip: the flow with every member's window centred on a per-voxel seed (include/d3fields_hip_pyramid.h)
struct FlowSeededArgs {
    const uint8_t *site_a, *site_b;
    const int32_t *slot_a, *slot_b;
    const float *data_a, *data_b;
    int64_t stride_a, stride_b;
    const int32_t *seed;         // [n, 3] or nullptr: zeros
    int32_t *target;
    float *cost;
    int32_t nx, ny, nz, C, r;
    int32_t vec;                 // 1: the rows of both sets move as 16-byte vectors
    float max_cost2;
};
hipError_t launch_flow_seeded(const FlowSeededArgs &A, hipStream_t s);

// pyramid_kernels.hip: a baked field at half the resolution (include/d3fields_hip_pyramid.h)
struct CoarsenSelectArgs {
    const float *dist;
    const uint8_t *valid;
    int32_t nx, ny, nz, cy, cz, min_children;
    int64_t nc;                  // coarse voxels
    float *out_dist;
    uint8_t *out_valid, *out_children;
};
struct CoarsenSet {
    const void *data;            // the fine rows: floats or halves (f16)
    const float *fill;           // or nullptr (zeros)
    float *out;                  // [m, C]
    int64_t stride;              // in elements
    int32_t C;
    int32_t vec;                 // 1: the rows and the output row move as 16-byte vectors
    int32_t f16;
};
struct CoarsenRowsArgs {
    const uint8_t *children;
    const int32_t *voxels;       // or nullptr: every coarse voxel in flat order
    const int32_t *slot;         // a banded source: nullptr with no stored voxel
    bool banded;
    int64_t m, nc;
    int32_t nx, ny, nz, cy, cz;
    int32_t n_sets;
    CoarsenSet sets[D3F_MAX_MAPS];
    uint8_t *out_known;
};
hipError_t launch_coarsen_select(const CoarsenSelectArgs &A, hipStream_t s);
hipError_t launch_coarsen_rows(const CoarsenRowsArgs &A, hipStream_t s);

// pool_kernels.hip: mean rows, votes and moments of the baked field per component
struct PoolArgs {
    const int32_t *label;
    int32_t nx, ny, nz, K;
    const uint8_t *valid;        // or nullptr
    const int32_t *slot;         // or nullptr
    const d3f_volume_set *sets;  // host memory
    int32_t n_sets;
    const int32_t *modes;        // host memory
    int64_t member_capacity;
    int64_t *out_members;
    int32_t *out_count;
    int64_t *out_moments;        // or nullptr
    void *const *out_rows;       // host memory
    void *workspace;
};
int64_t pool_workspace_bytes(int64_t n, int64_t K, int64_t cap, int64_t mean_channels);      // cap clamped to n, then pool_layout(...).total
int pool_levels(int64_t cap);                                       // fold levels a member capacity needs: 1..4
hipError_t launch_volume_pool(const PoolArgs &A, hipStream_t s);
hipError_t launch_pool_nothing(int64_t *out_members, hipStream_t s);   // K == 0: out_members = 0
// The label-sorted member list on its own (motion_kernels.hip folds float64 rows over it).
// The arrays the scans turn into offsets, K + 1 entries each (the last one 0, so that entry K of a scan is the total):
//   first[k]      count_k: where the component's members start in the sorted list
//   work[l][k]    the chunks component k folds at level l: ceil(count / 256^(l+1)) while it still has more than one row there (any at l = 0)
//   part[l][k]    the partial rows it writes at level l: the same number where that is more than one
struct PoolPlan {
    uint32_t *first;
    uint32_t *work[4];
    uint32_t *part[3];
};
// pitch: the 4-byte words of a partial row; first / work / part: the arrays of PoolPlan
struct PoolLayout {
    int64_t flag, flag_scan, keys[2], vals[2], counters, counters_scan, first, work[4], part[3], plan_scan, rows[2], total;
    int64_t waves_total, rows_a, rows_b;
};
PoolLayout pool_layout(int64_t n, int64_t K, int64_t cap, int64_t pitch);
struct PoolList {
    const uint32_t *vals;        // the members' flat indices grouped by label, ascending inside a label; valid where *out_members <= cap
    PoolPlan plan;               // scanned
    int levels;                  // 0 with cap == 0
};
// out_count is zeroed and counted, out_members written, the list sorted and the plan scanned: everything of launch_volume_pool before its folds.
// cap = min(member_capacity, n); workspace laid out by L = pool_layout(n, K, cap, pitch).
hipError_t launch_pool_members(const int32_t *label, const uint8_t *valid, const int32_t *slot, int64_t n, int K, int64_t cap, int64_t *out_members,
                               int32_t *out_count, void *workspace, const PoolLayout &L, PoolList *list, hipStream_t s);
inline int64_t pool_level_chunks(int64_t cap, int K, int l)   // an upper bound of the chunks folded at level l
{
    // capacity / 256^(l+1) plus one ragged chunk per component that takes part (every non-empty one at level 0, those with more than 256^l members later)
    return l == 0 ? (cap >> 8) + (K < cap ? K : cap) : (cap >> (8 * l + 8)) + (cap >> (8 * l)) + 1;
}

// motion_kernels.hip: one rigid motion per part from dense correspondences
struct MotionArgs {
    const int32_t *label;
    int32_t K, nx, ny, nz;
    const uint8_t *keep;         // or nullptr
    const int32_t *target;
    const double *offset;        // or nullptr
    const int32_t *ref;          // or nullptr
    int32_t fits, min_pairs;
    double tau2;
    int64_t member_capacity;
    int64_t *out_members;
    int32_t *out_pairs;
    double *out_pose;
    int32_t *out_inliers;
    double *out_rmse;
    int32_t *out_status, *out_fits;
    double *out_residual2;       // or nullptr
    uint8_t *out_inlier;         // or nullptr
    double *out_sums;            // or nullptr
    void *workspace;
};
struct MotionLayout {
    int64_t lab, pool, sums, fsum, centre, total;
    PoolLayout P;                // of the pool region, offsets from its start
};
MotionLayout motion_layout(int64_t n, int64_t K, int64_t cap);
int64_t motion_workspace_bytes(int64_t n, int64_t K, int64_t cap);          // cap clamped to n, then motion_layout(n, K, cap).total
hipError_t launch_part_motion(const MotionArgs &A, hipStream_t s);

// warp_kernels.hip: a baked field moved by the rigid motions of its parts
struct WarpSelectArgs {
    const float *dist;
    const uint8_t *valid, *cell_valid;
    const int32_t *owner;
    const double *pose;          // [K, 15] on the device
    int32_t nx, ny, nz, K;
    int32_t *out_source;
    float *out_dist;
    uint8_t *out_valid;
    int32_t *out_boxes;          // [K, 12]
};
struct WarpRowsArgs {
    const int32_t *source;
    const double *pose;
    const int32_t *voxels;       // or nullptr: every voxel in flat order (m = the voxel count)
    int64_t m;
    int32_t nx, ny, nz, K;
    bool banded;
    const int32_t *slot;         // banded: nullptr with no stored voxel
    const uint8_t *cell_band;
    int32_t n_sets;
    VolSet sets[D3F_MAX_MAPS];   // data, fill, out, stride, C, vec
    uint8_t *out_known;
};
hipError_t launch_warp_select(const WarpSelectArgs &A, hipStream_t s);
hipError_t launch_warp_rows(const WarpRowsArgs &A, hipStream_t s);

// merge_kernels.hip: two baked fields on one grid merged into one (include/d3fields_hip_ext.h)
struct MergeSelectArgs {
    const float *dist_a, *weight_a, *dist_b, *weight_b;      // a weight volume or nullptr: the scalar
    const uint8_t *valid_a, *valid_b;
    float wa, wb, w_max, gap;
    int64_t n;
    float *out_dist, *out_weight, *out_beta;
    uint8_t *out_valid, *out_kind;
};
struct MergeSet {
    const void *a, *b;           // the rows of either side: floats or halves (f16_a / f16_b)
    const float *fill;           // a's fill row or nullptr (zeros)
    float *out;                  // [m, C]
    int64_t stride_a, stride_b;  // in elements
    int32_t C;
    int32_t vec;                 // 1: both rows and the output row move as 16-byte vectors
    int32_t f16_a, f16_b;
};
struct MergeRowsArgs {
    const uint8_t *kind;
    const float *beta;
    const int32_t *voxels;       // or nullptr: every voxel in flat order (m = the voxel count)
    const int32_t *slot_a, *slot_b;      // a banded side: nullptr with no stored voxel
    bool banded_a, banded_b;
    int64_t m, n;
    int32_t n_sets;
    MergeSet sets[D3F_MAX_MAPS];
    uint8_t *out_known;
};
hipError_t launch_merge_select(const MergeSelectArgs &A, hipStream_t s);
hipError_t launch_merge_rows(const MergeRowsArgs &A, hipStream_t s);

// geodesic_kernels.hip: cost-to-go through free space, exact shortest paths on the lattice; w: host int32[3]
struct GeoLayout { int64_t header, flags, list, total; int64_t tiles; };
GeoLayout geodesic_layout(int nx, int ny, int nz);
hipError_t launch_geodesic_init(const uint8_t *free, int nx, int ny, int nz, const int32_t *seeds, int64_t n_seeds, int32_t *out_cost, void *workspace,
                                hipStream_t s);
hipError_t launch_geodesic_relax(const uint8_t *free, const int32_t *penalty, int nx, int ny, int nz, int connectivity, const int32_t *w, int32_t max_cost,
                                 int rounds, int32_t *cost, int32_t *out_pending, void *workspace, hipStream_t s);
hipError_t launch_geodesic_finish(const uint8_t *free, const int32_t *penalty, int nx, int ny, int nz, int connectivity, const int32_t *w, float step,
                                  const int32_t *cost, int32_t *out_next, float *out_dist, hipStream_t s);
hipError_t launch_volume_follow(const int32_t *next, int64_t n_voxels, const int32_t *starts, int64_t n, int max_steps, int32_t *out_voxels, int32_t *out_length,
                                uint8_t *out_reached, hipStream_t s);

// segment_kernels.hip: exact grid segments through a free volume and shortcuts of voxel rows
hipError_t launch_volume_segments(const uint8_t *free, const int32_t *value, int nx, int ny, int nz, const int32_t *a, const int32_t *b, int64_t n, bool strict,
                                  uint8_t *out_clear, int32_t *out_last, int32_t *out_blocked, int32_t *out_min_value, int32_t *out_min_voxel, hipStream_t s);
hipError_t launch_path_shorten(const uint8_t *free, int nx, int ny, int nz, const int32_t *voxels, const int32_t *length, int64_t n, int row_len, int max_span,
                               bool strict, int32_t *out_index, int32_t *out_voxels, int32_t *out_count, hipStream_t s);

// peaks_kernels.hip: exact non-maximum suppression through the slot volume
struct PeaksPlan {
    int tile, log_ck, hzp, tiles_y, tiles_z;     // tile edge, log2 of the column chunk, padded z line of the staged box
    int64_t tiles, chunks, lds_bytes;            // grid.x, grid.y, dynamic LDS of one workgroup
};
PeaksPlan peaks_plan(int nx, int ny, int nz, int K, int radius);
hipError_t launch_volume_peaks(const int32_t *slot, const uint8_t *mask, int nx, int ny, int nz, const float *score, int K, int64_t stride_row, int radius,
                               float threshold, float *out, int64_t out_stride, int32_t *out_count, hipStream_t s);

// align_kernels.hip: the normal equations of a rigid alignment to the baked field and the damped Gauss-Newton step
constexpr int kAlignRow = D3F_ALIGN_ROW_DOUBLES;        // one row of sums: 21 + 6 + 1 + 2 counts + 2 zeros
constexpr int kAlignState = D3F_ALIGN_STATE_DOUBLES;
struct AlignParams {
    VolParams V;               // dist, cell, the lattice; pts = the MODEL points [I, n, 3], n = points per instance; sets[0] (n_sets 0 or 1) the descriptor set
    const int32_t *slot;       // banded: [nx, ny, nz]; nullptr with banded: no row is stored, no point is in the band
    const uint8_t *cell_band;
    int32_t banded;
    int32_t I;
    const float *weights;      // [I, n] or nullptr (ones)
    const float *targets;      // [I, n, C] with a set
    const float *dist_targets; // [I, n] or nullptr (zeros)
    const float *pose;         // [I, 12]: R row-major, then t
    const float *centroid;     // [I, 3]: the model's weighted centroid
    const int32_t *skip;       // [I] or nullptr: non-zero = the instance is final, its workgroups leave at once
    float wd, wf, outside;
    int64_t chunks;            // workgroups per instance
    double *partial;           // [I, chunks, kAlignRow]
};
struct AlignStep {
    double *state;             // [I, kAlignState]
    const double *partial;     // [I, chunks, kAlignRow]
    int64_t chunks;
    double *out;               // [I, kAlignRow]
    int32_t it, iters;
    double rot_tol, trans_tol;
    float *pose_out;           // [I, 12]
    int32_t *skip_out;         // [I]
    double *history;           // [I, iters + 1]
};
int64_t align_chunks(int64_t n);
struct AlignLayout {
    int64_t partial, total;
    int64_t chunks;            // workgroups per instance
};
AlignLayout align_layout(int64_t I, int64_t n);
hipError_t launch_align_centroid(const float *pts, const float *weights, int64_t I, int64_t n, float *out, hipStream_t s);
hipError_t launch_align_accumulate(const AlignParams &A, double *out, hipStream_t s);
hipError_t launch_align_step(const AlignStep &S, int64_t I, hipStream_t s);

// consensus_kernels.hip: consensus poses from (model point, candidate) triples
constexpr int kConsMaxM = D3F_CONSENSUS_MAX_POINTS, kConsMaxK = D3F_CONSENSUS_MAX_CANDIDATES;
constexpr int kConsHeadWords = 128;      // the head of the workspace: [0, 65) the histogram of counts, then the words below
constexpr int kConsGated = 65, kConsCut = 66, kConsTake = 67, kConsSurvivors = 68;
struct ConsensusParams {
    const float *model;        // [M, 3]
    const float *cand;         // [M, k, 3]
    const int32_t *trip;       // [n_trip, 3]
    int32_t M, k;
    int64_t T;                 // n_trip * k^3
    float tau2;
    double side_tol, min_side, min_sin2;
    uint8_t *count;            // [T]
    float *pose_dbg;           // [T, 12] or nullptr
    int8_t *assign_dbg;        // [T, M] or nullptr
    uint32_t *head;            // [kConsHeadWords]
};
struct ConsensusSelect {
    ConsensusParams C;         // count is read here; pose_dbg / assign_dbg unused
    int32_t min_inliers, shared, n_poses;
    uint32_t max_survivors;
    uint32_t *eq_block, *fl_block;      // [ceil(T / 256)] each
    void *scan_scratch;
    int32_t *surv_h;           // [max_survivors]
    uint8_t *surv_count, *alive;
    int8_t *surv_assign;       // [max_survivors, 64]
    int32_t *hyp_out, *count_out, *stats_out;
    int8_t *assign_out;        // [n_poses, 64]
    float *pose_out;           // [n_poses, 12]
};
int64_t consensus_blocks(int64_t T);
struct ConsensusLayout {       // the scoring pass uses the head alone: the bytes in front of eq
    int64_t head, eq, fl, scan, surv_h, surv_count, alive, surv_assign, total;
};
ConsensusLayout consensus_layout(int64_t T, int64_t max_survivors);
hipError_t launch_consensus_score(const ConsensusParams &C, hipStream_t s);
hipError_t launch_consensus_select(const ConsensusSelect &S, hipStream_t s);
hipError_t launch_pose_refit(const float *model, const float *cand, int M, int k, const int8_t *assign, int n_poses, float tau2, float *pose_out, double *rmse_out,
                             int32_t *count_out, hipStream_t s);

// raycast_kernels.hip: the first surface a ray meets in a baked volume
constexpr float kRayMaxSamples = 131072.0f;  // a ray whose K exceeds this misses: unreachable under the entry point's 65536-step guard but for overflow
struct RayParams {
    const float *dist;
    const uint8_t *cell;     // [nx-1, ny-1, nz-1]
    const float *origins;    // explicit rays: [n, 3] each
    const float *dirs;
    float *out_t;            // [n]
    uint8_t *out_hit;        // [n]
    float *out_pts;          // [n, 3]
    int32_t *out_samples;    // [n] or nullptr
    int64_t n;
    int32_t nx, ny, nz;
    float ox, oy, oz, h;
    float march, t_near, t_far;
    int32_t H, W;            // camera rays: pixel (u, v) is ray v * W + u
    float fx, fy, cx, cy;
    float R[9];              // world -> camera rotation, row-major
    float co[3];             // the camera centre -R^T tc
};
hipError_t launch_volume_raycast(const RayParams &P, bool camera, hipStream_t s);

// pcd_kernels.hip
hipError_t launch_backproject(const double *depth, const uint8_t *mask, int H, int W, const double *cam, const double *T,
                              const double *bounds, int64_t capacity, double *out_pts, int32_t *out_pixel, int64_t *count,
                              void *workspace, hipStream_t s);
struct PixelCountsLayout {     // d3f_backproject_view and d3f_nonzero_pixels
    int64_t counts, total;
    int64_t blocks;
};
PixelCountsLayout pixel_counts_layout(int64_t npix);
hipError_t launch_nearest(const double *a, int64_t na, const double *b, int64_t nb, double *min_dist, int64_t *argmin, hipStream_t s);

// assoc_kernels.hip
hipError_t launch_pcd_to_index(const double *pts, int64_t n, const double *lower, double voxel_size, const int32_t *voxel_num,
                               int32_t *out_index, int32_t *out_voxel, hipStream_t s);
struct VoxsetLayout {
    int64_t table, total;
    int64_t cap;               // slots, a power of two
};
VoxsetLayout voxset_layout(int64_t n1, int64_t n2);
hipError_t launch_voxset_iou(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int64_t *counts, void *workspace,
                             hipStream_t s);
struct VoxmeanLayout {
    int64_t minb, table, counts, list, total;
    int64_t cap, blocks;       // slots, workgroups over them
};
VoxmeanLayout voxmean_layout(int64_t n);
hipError_t launch_voxel_mean(const double *pts, const double *col, int64_t n, double vs, double *out_pts, double *out_col, int64_t *count,
                             void *workspace, hipStream_t s);
hipError_t launch_erode(const uint8_t *src, int H, int W, int kh, int kw, uint8_t *dst, hipStream_t s);
hipError_t launch_compose_labels(const uint8_t *dets, int n_dets, int64_t n_pix, const int32_t *label_of_det, uint8_t *out, hipStream_t s);
hipError_t launch_mask_gate(const float *mask, int64_t sy, int64_t sx, const float *depth, int H, int W, float lo, float hi,
                            uint8_t *out, hipStream_t s);
hipError_t launch_nonzero_pixels(const uint8_t *img, int H, int W, int64_t capacity, int32_t *out_rc, int64_t *count,
                                 void *workspace, hipStream_t s);
hipError_t launch_fps_pixels(const int32_t *pts, int64_t n, int k, int64_t init_idx, int64_t *out_idx, double *out_maxdist,
                             void *workspace, hipStream_t s);

// misc_kernels.hip
hipError_t launch_map_check(const void *data, int V, int fh, int fw, int C, int64_t sv, int64_t sy, int64_t sx, int esize,
                            uint32_t *word, hipStream_t s);
bool map_is_flat(const void *data, int V, int fh, int fw, int C, int64_t sv, int64_t sy, int64_t sx);
hipError_t launch_map_check_many(const void *const *data, const int64_t *nbytes, const int *esize, uint32_t *const *words, int n,
                                 bool words_are_zero, hipStream_t s);
hipError_t launch_onehot2instance(const float *onehot, int64_t n, int NI, uint8_t *out, hipStream_t s);
hipError_t launch_instance2onehot(const uint8_t *inst, int64_t n, int NI, uint8_t *out, hipStream_t s);

// proj_kernels.hip
hipError_t launch_project_maps(const void *data, int V, int fh, int fw, int C, int64_t sv, int64_t sy, int64_t sx, bool half, const float *W,
                               int k, float *dst, hipStream_t s);

// moment_kernels.hip
struct MomentPlan {
    int panels, pairs, cpad;
    int64_t sum_slabs, sum_rows;                 // pass 1: slabs and rows per slab
    int64_t slabs, slab_rows;                    // pass 2
    int64_t off_wsum_part, off_sum_part, off_wsum, off_m32, off_col_part, off_tiles, bytes;
};
MomentPlan moment_plan(int64_t M, int C);
int64_t row_moments_workspace_bytes(int64_t M, int C);      // moment_plan(M, C).bytes
hipError_t launch_row_moments(const void *rows, bool half, int64_t M, int C, int64_t row_stride, const float *weights, double *wsum_out,
                              double *mean_out, double *scatter_out, void *workspace, hipStream_t s);

// corr_kernels.hip
struct ColStat {   // running softmax statistics of one column (16 B)
    float m;       // max of -d*scale
    float s;       // sum exp(x - m)
    int64_t arg;   // row index of the first maximum
};
constexpr int kSoftmaxRowsPerBlock = 64;     // = the row tile of pairwise_dist_kernel, whose epilogue emits the statistics
hipError_t launch_dist_to_target(const float *src, int64_t B, int64_t inner, int C, int64_t sb, int64_t si,
                                 int64_t sc, const float *tgt, int dist_type, float *out, hipStream_t s);
hipError_t launch_pairwise_dist(const float *src, const float *tgt, int64_t B1, int64_t B2, int C,
                                int dist_type, float *out, hipStream_t s, ColStat *ws = nullptr, float stat_scale = 1.0f,
                                bool direct_only = false);
hipError_t launch_exp_neg_scale(float *x, int64_t n, float scale, hipStream_t s);
// softmax(-x*scale, dim=0) of a row-major [rows, cols] matrix in place (+ optional argmax)
hipError_t launch_softmax_dim0(float *x, int64_t rows, int64_t cols, float scale, int64_t *argmax_out,
                               ColStat *ws, bool have_stats, hipStream_t s);
// row-sharded softmax: local column statistics, cross-rank merge, normalisation with merged statistics
hipError_t launch_softmax_local_stats(const float *x, int64_t rows, int64_t cols, float scale, int64_t row_offset,
                                      ColStat *ws, ColStat *stats_out, bool have_stats, hipStream_t s);
hipError_t launch_softmax_merge(const ColStat *parts, int64_t nparts, int64_t cols, ColStat *merged, int64_t *argmax_out,
                                hipStream_t s);
hipError_t launch_softmax_apply(float *x, int64_t rows, int64_t cols, float scale, const ColStat *merged, hipStream_t s);
// argmin over dim 0 of raw distances (used for D3F_SIM_DIST + argmax_out)
hipError_t launch_argmin_dim0(const float *x, int64_t rows, int64_t cols, int64_t *arg_out, ColStat *ws,
                              bool have_stats, hipStream_t s);

// k smallest entries per column of a [rows, cols] distance matrix (k <= 8), ties -> lower row, NaN last
struct SoftmaxLayout { int64_t stats, total; };
SoftmaxLayout softmax_layout(int64_t rows, int64_t cols);
struct TopkLayout {
    int64_t list[16], total;       // 2^31 - 1 rows (the entry points' limit): 7 levels; any int64: 13
    int64_t items[16], chunks[16];
    int levels;
};
TopkLayout topk_layout(int64_t rows, int64_t cols);
int64_t topk_workspace_bytes(int64_t rows, int64_t cols);   // 0 without rows or columns, else topk_layout(rows, cols).total
struct PairTopkLayout { int64_t stats, topk, slack, total; };
PairTopkLayout pair_topk_layout(int64_t rows, int64_t cols);
hipError_t launch_topk_select(const float *dist, int64_t rows, int64_t cols, void *workspace, const void **final_list, hipStream_t s);
hipError_t launch_topk_write(const void *final_list, const float *x, int64_t rows, int64_t cols, int k, int64_t *idx_out,
                             float *val_out, hipStream_t s);

hipError_t launch_topk_merge_parts(const int64_t *pidx, const float *pval, int64_t n_parts, int k, int64_t cols, int64_t *out_idx,
                                   float *out_val, hipStream_t s);

// track_kernels.hip: the closed-form parts of the rigid-tracking optimiser step
hipError_t launch_rigid_transform(const float *last, int I, int n, const float *t, const float *w, float eps, float *out_pts,
                                  float *norms, hipStream_t s);
hipError_t launch_track_loss_grad(const float *feats, const float *src, const float *dist, const uint8_t *valid, int N, int C,
                                  float dist_w, float *grad_feats, float *grad_dist, float *loss, hipStream_t s);
hipError_t launch_rigid_update(const float *last, int I, int n, const float *grad_pts, float *t, float *w, float *adam_m, float *adam_v,
                               float *step, const float *norms, float eps_rot, float reg_w, float lr, float beta1, float beta2,
                               float eps_adam, hipStream_t s);

struct TrackStepParams {
    const float *depth, *K, *pose;      // views
    int32_t V, H, W;
    MapDesc map;                        // the descriptor map (fp32, C % 4 == 0)
    const float *last;                  // [I, n, 3]
    const float *src;                   // [I*n, C]
    int32_t I, n;
    float mu, dist_w, reg_w, lr, beta1, beta2, eps_adam, eps_rot;
    double ln_beta1, ln_beta2;          // ln of the decimal numbers beta1 / beta2 stand for (log_of_decimal): Adam's bias corrections in double
    float *t, *w, *adam_m, *adam_v, *step;     // [I,3] [I,3] [I,6] [I,6] [I]
    float *out_pts;                     // [I*n, 3] the keypoints as evaluated in this step
    float *grad_pts;                    // [I*n, 3] scratch
    float *loss_acc;                    // [4] two slots of two accumulators (steps alternate), zero between launches
    unsigned long long *par;            // [I*6] (value, step tag) words: the parameters a multi-step launch publishes
    float *loss_out;                    // [3] feature loss, distance loss, regulariser of this step
    unsigned int *counter;              // [2] arrivals (the second word is spare); zero between launches
    int32_t iters;                      // optimiser steps in this launch (> 1: all I*n waves resident, <= kTrackMaxResident)
};
constexpr int kTrackMaxResident = 512;       // one wave per SIMD at this kernel's register count = 1024 on the chip; half of it

hipError_t launch_track_step(const TrackStepParams &P, hipStream_t s);
double log_of_decimal(float beta);
int track_run_capacity();          // keypoints one d3f_track_run launch may hold on the current device

}  // namespace d3f
