// d3f_api.hip -- the extern "C" boundary of libd3fields_hip.so (see include/d3fields_hip.h).
// Validates arguments, picks the lane mapping of every channel map and enqueues the kernels on
// the caller's stream.  No allocation, no synchronisation, no state besides the thread-local
// error text.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "d3f_internal.h"
#include "d3fields_hip_ext.h"      // the entry points added after the main table of ABI 16
#include "d3fields_hip_pyramid.h"  // ... and the pyramid's, a header per feature from here on

namespace {

thread_local char g_err[512] = "";
thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;   // one-shot, see d3f_profile_next_eval

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(D3F_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

int check_views(const d3f_views *v)
{
    if (!v) return fail(D3F_ERR_INVALID_ARG, "views is NULL");
    if (!v->depth || !v->K || !v->pose) return fail(D3F_ERR_INVALID_ARG, "views: depth/K/pose must be non-NULL");
    if (v->V < 1 || v->V > D3F_MAX_VIEWS) return fail(D3F_ERR_BAD_SHAPE, "views: V=%d outside [1,%d]", v->V, D3F_MAX_VIEWS);
    if (v->H < 2 || v->W < 2) return fail(D3F_ERR_BAD_SHAPE, "views: H=%d W=%d must be >= 2", v->H, v->W);
    return D3F_OK;
}

// ---- the argument rules the kernels rely on, each stated once: an entry point calls these and restates none of them (which status wins when
// two arguments are bad is pinned row by row, tests/test_api_status_host.py).  who: the entry point's short name, the first word of every message ----
bool finite_nonneg(double v) { return v >= 0.0 && v * 0.0 == 0.0; }
bool positive_finite(float x) { return x > 0.0f && x * 0.0f == 0.0f; }

// a site volume: 32-bit voxel indices, and the extents the distance transform's rows can take.  The predicate of the *_workspace_bytes functions.
bool edt_shape_ok(int32_t nx, int32_t ny, int32_t nz)
{
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= D3F_EDT_MAX_EXTENT && ny <= D3F_EDT_MAX_EXTENT && nz <= D3F_EDT_MAX_EXTENT &&
           (int64_t)nx * ny * nz <= 0x7fffffffLL;
}

int check_extents(const char *who, int32_t nx, int32_t ny, int32_t nz)
{
    if (edt_shape_ok(nx, ny, nz)) return D3F_OK;
    return fail(D3F_ERR_BAD_SHAPE, "%s: nx=%d ny=%d nz=%d, every extent must be in [1, %d] and the volume at most 2^31 - 1 voxels", who, nx, ny, nz,
                D3F_EDT_MAX_EXTENT);
}

int check_connectivity(const char *who, int32_t c)
{
    if (c == 6 || c == 18 || c == 26) return D3F_OK;
    return fail(D3F_ERR_INVALID_ARG, "%s: connectivity=%d, must be 6, 18 or 26", who, c);
}

// the workspace protocol: absent or short is D3F_ERR_WORKSPACE (with the size to bring), only then misaligned is D3F_ERR_BAD_LAYOUT
int check_workspace(const char *who, const void *workspace, int64_t bytes, int64_t need, int alignment)
{
    if (!workspace || bytes < need) return fail(D3F_ERR_WORKSPACE, "%s: needs %lld workspace bytes", who, (long long)need);
    if (!aligned(workspace, alignment)) return fail(D3F_ERR_BAD_LAYOUT, "%s: workspace must be %d-byte aligned", who, alignment);
    return D3F_OK;
}

// a stored set, by status: its width (the kernels' row loops), then its rows (stride_voxel and the 4-byte loads).  fill is read by the lookups and
// the pooling only, and checked there.
int check_set_shape(const char *who, int s, const d3f_volume_set &set)
{
    if (set.C >= 1 && set.C <= D3F_VOLUME_MAX_CHANNELS) return D3F_OK;
    return fail(D3F_ERR_BAD_SHAPE, "%s: set %d: C=%d outside [1,%d]", who, s, set.C, D3F_VOLUME_MAX_CHANNELS);
}

// the set's storage word (`reserved`): float32 everywhere; IEEE half only where the entry point's row loops have a half form (half_ok: the
// four lookups).  Called by EVERY entry point that takes a set, right after check_set_shape: a loop that knows float32 only would read
// halves as floats and run past the rows.
int check_set_storage(const char *who, int s, const d3f_volume_set &set, bool half_ok)
{
    if (set.reserved == D3F_DTYPE_F32 || (half_ok && set.reserved == D3F_DTYPE_F16)) return D3F_OK;
    if (set.reserved == D3F_DTYPE_F16)
        return fail(D3F_ERR_BAD_DTYPE, "%s: set %d: rows stored as half (D3F_DTYPE_F16) are read by the lookups only; this entry point needs float32 rows", who, s);
    return fail(D3F_ERR_BAD_DTYPE, "%s: set %d: storage word %d is neither D3F_DTYPE_F32 nor D3F_DTYPE_F16", who, s, set.reserved);
}

bool set_is_half(const d3f_volume_set &set) { return set.reserved == D3F_DTYPE_F16; }

int check_set_layout(const char *who, int s, const d3f_volume_set &set)
{
    if (set.stride_voxel < set.C) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: stride_voxel=%lld < C=%d", who, s, (long long)set.stride_voxel, set.C);
    if (set_is_half(set)) {
        if (!aligned(set.data, 2)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: data must be 2-byte aligned", who, s);
        return D3F_OK;
    }
    if (!aligned(set.data, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: data must be 4-byte aligned", who, s);
    return D3F_OK;
}

// may the rows of a set move as 16-byte vectors?  (and-ed with the alignment of what is written or read beside them by the caller)
// float32: four channels to a vector; half: eight
bool set_reads_vectors(const d3f_volume_set &set)
{
    const int per = set_is_half(set) ? 8 : 4;
    return set.C % per == 0 && set.stride_voxel % per == 0 && aligned(set.data, 16);
}

// one thread per item, per_block items to a workgroup: the grid's x has 31 bits
int check_launch_blocks(const char *who, int64_t n, int64_t per_block)
{
    if ((n + per_block - 1) / per_block > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "%s: n=%lld too large for one launch", who, (long long)n);
    return D3F_OK;
}

// the per-set outputs of a lookup / the per-set gradients of its backward; a set keeps its vectors only if these are 16-byte aligned too
int attach_outputs(const char *who, d3f::VolParams &P, int32_t n_sets, void *const *out_sets)
{
    for (int s = 0; s < n_sets; ++s) {
        if (!out_sets[s]) return fail(D3F_ERR_INVALID_ARG, "%s: out_sets[%d] is NULL", who, s);
        if (!aligned(out_sets[s], 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: out_sets[%d] must be 4-byte aligned", who, s);
        P.sets[s].out = static_cast<float *>(out_sets[s]);
        if (!aligned(out_sets[s], 16)) P.sets[s].vec = 0;
    }
    return D3F_OK;
}

int attach_grads(const char *who, d3f::VolParams &P, int32_t n_sets, const void *const *grad_sets)
{
    for (int s = 0; s < n_sets && grad_sets; ++s) {
        if (!aligned(grad_sets[s], 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: grad_sets[%d] must be 4-byte aligned", who, s);
        P.sets[s].grad = static_cast<const float *>(grad_sets[s]);
        if (!aligned(grad_sets[s], 16)) P.sets[s].vec = 0;
    }
    return D3F_OK;
}

#ifdef D3F_EXPERIMENTS
// phase stamps of the window kernel (Tune::stamps): 32 x uint64 per sampled workgroup, read back with d3f_exp_read_stamps
constexpr int64_t kStampBytes = 8LL * 32 * 65536;
unsigned long long *exp_stamp_buffer(bool clear)
{
    static unsigned long long *buf = nullptr;
    if (!buf && hipMalloc(reinterpret_cast<void **>(&buf), kStampBytes) != hipSuccess) buf = nullptr;
    if (buf && clear) (void)hipMemset(buf, 0, kStampBytes);
    return buf;
}
#endif

// the launch planner: thresholds, the family table, one function per kernel family (host logic only)
#include "d3f_plan.h"

// Validates one channel map and fills the kernel-side descriptor (out/inter may be NULL for backward).
int fill_map(const d3f_channel_map &c, int s, int V, float *out, float *inter, const float *extra_aligned,
             d3f::MapDesc &m, int64_t &map_bytes, uint32_t flags = 0)
{
    if (!c.data) return fail(D3F_ERR_INVALID_ARG, "map %d: data pointer is NULL", s);
    if (c.dtype != D3F_DTYPE_F32 && c.dtype != D3F_DTYPE_F16)
        return fail(D3F_ERR_BAD_DTYPE, "map %d: dtype %d unsupported (D3F_DTYPE_F32 or D3F_DTYPE_F16)", s, c.dtype);
    const int es = c.dtype == D3F_DTYPE_F16 ? 2 : 4;          // bytes per stored channel
    if (c.fh < 1 || c.fw < 1 || c.C < 1) return fail(D3F_ERR_BAD_SHAPE, "map %d: fh=%d fw=%d C=%d", s, c.fh, c.fw, c.C);
    if (c.stride_x < c.C || c.stride_y < 0 || c.stride_v < 0)
        return fail(D3F_ERR_BAD_LAYOUT, "map %d: strides (%lld,%lld,%lld) do not describe a channels-last map", s,
                    (long long)c.stride_v, (long long)c.stride_y, (long long)c.stride_x);
    if (((int64_t)(c.fh - 1) * c.stride_y + (int64_t)(c.fw - 1) * c.stride_x + c.C) * es >= (1LL << 32))
        return fail(D3F_ERR_BAD_SHAPE, "map %d: one view spans 4 GiB or more (32-bit texel offsets)", s);
    m.data = static_cast<const float *>(c.data);
    m.out = out;
    m.inter = inter;
    m.runs = 0;
    m.pre_slot = -1;
    m.esize = es;
    m.fold = ((int64_t)c.C * es > 256) ? 1 : 0;        // wide map: folded weights on the fast path (fuse_common.h)
    m.sv = c.stride_v; m.sy = c.stride_y; m.sx = c.stride_x;
    m.fh = c.fh; m.fw = c.fw; m.C = c.C;
    if (!aligned(m.data, es) || !aligned(out, 4) || !aligned(extra_aligned, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "map %d: pointers must be aligned to their element size", s);
    // 4-channel vectors: 16 B of fp32 / 8 B of fp16 per load; outputs are fp32 either way
    const bool str4 = (c.stride_v % 4 == 0) && (c.stride_y % 4 == 0) && (c.stride_x % 4 == 0);
    const bool str2 = (c.stride_v % 2 == 0) && (c.stride_y % 2 == 0) && (c.stride_x % 2 == 0);
    const bool can16 = str4 && aligned(m.data, 4 * es) && aligned(out, 16) && aligned(inter, 16) && aligned(extra_aligned, 16);
    const bool can8 = str2 && aligned(m.data, 2 * es) && aligned(out, 8) && aligned(inter, 8) && aligned(extra_aligned, 8);
    const int64_t this_bytes = (int64_t)V * c.fh * c.fw * c.C * es;
    map_bytes += this_bytes;
    if (es == 2) {
        // fp16 storage: 8 channels per 16-B load (fp32 accumulators / 32-B stores), else scalar lanes; batched loads only
        const bool str8 = (c.stride_v % 8 == 0) && (c.stride_y % 8 == 0) && (c.stride_x % 8 == 0);
        const bool vec8 = (c.C % 8 == 0) && str8 && aligned(m.data, 16) && aligned(out, 16) && aligned(inter, 16) &&
                          aligned(extra_aligned, 16);      // backward: grad_fused is read as 32-byte f32x8 pieces of 16-B aligned rows
        const int max_u = m.fold ? 4 : 1;               // thin maps: one vector per lane (see below)
        pick_mapping(m, false, false, true, max_u);     // scalar lanes ...
        if (vec8) {                                     // ... or the same search over 8-channel vectors
            d3f::MapDesc t = m;
            t.C = c.C / 2;                               // cvec = C/8 = (C/2)/4: reuse the 4-wide search
            pick_mapping(t, true, true, true, max_u);
            m.vw = 8; m.lpp_log2 = t.lpp_log2; m.unroll = t.unroll;
        }
        return D3F_OK;
    }
    bool batch = this_bytes <= kBatchedLoadBytes;
    if (flags & (1u << 26)) batch = true;
    if (flags & (1u << 27)) batch = false;
    // thin maps (<= 256 bytes per texel: masks, colours) keep the reference's operation order and get ONE kernel form -- one
    // batched vector per lane; the wide ones have the whole family (and the folded weights).  Keeping the two families apart
    // halves the instantiations of gather_map a kernel carries (with both full families the generic kernels spilled 1 KiB).
    if (!m.fold) batch = true;
    pick_mapping(m, can16, can8, batch, m.fold ? 4 : 1);
    return D3F_OK;
}

constexpr int kGatedSecondPass = 1;          // eval_common's internal "now enqueue the other side" status (never returned to callers)

// Validates, fills the kernel parameters, PLANS (d3f_plan.h), builds / reuses the point order, launches.
// cloud_side (d3f_eval): 0 = plan queries and the callers that never gate; 1 = first pass of a query -- if the points are a cloud the
// window kernel may take (kWindowCloudMin points, a patch-resolution wide map, the Hilbert order), this pass enqueues order +
// probe + the GATED window launch and returns kGatedSecondPass; 2 = the second pass: the gated cell-run launch.
int eval_common(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps, int32_t n_maps,
                float mu, uint32_t flags, float *out_dist, uint8_t *out_valid, float *const *out_fused,
                float *const *out_inter, void *workspace, int64_t workspace_bytes, void *stream, int mode,
                d3f_eval_plan *plan_out = nullptr, const d3f_grid *grid = nullptr, const int32_t *lattice = nullptr, int cloud_side = 0)
{
    const bool plan_only = plan_out != nullptr;
    int rc = check_views(views);
    if (rc != D3F_OK) return rc;
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "n=%lld is negative", (long long)n);
    if (n == 0 && !plan_only) return D3F_OK;
    if (!plan_only && ((!pts && !grid) || !out_dist || !out_valid)) return fail(D3F_ERR_INVALID_ARG, "pts/out_dist/out_valid must be non-NULL");
    if (n_maps < 0 || n_maps > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "n_maps=%d outside [0,%d]", n_maps, D3F_MAX_MAPS);
    if (n_maps > 0 && (!maps || (!out_fused && !plan_only))) return fail(D3F_ERR_INVALID_ARG, "maps/out_fused must be non-NULL when n_maps > 0");
    if (!(mu > 0.0f)) return fail(D3F_ERR_INVALID_ARG, "mu must be > 0");

    // D3F_FLAG_REFERENCE_ROUNDING: no fast path at all -- every point takes the strict form (the reference's operation order)
    if (flags & D3F_FLAG_REFERENCE_ROUNDING) flags = (flags & ~D3F_FLAG_FINITE_MAPS) | D3F_TUNE_DIRECT_GATHER;
    d3f::EvalParams P;
    const Tune tune = load_tune();          // every knob 0 in the product build (d3f_plan.h)
    // device-side finiteness words (d3f_map_check): used when the host did not vouch for the maps and EVERY tensor of the
    // query carries one; the kernels then decide on the device, and the launch is planned for finite maps
    P.n_words = 0;
    if (!(flags & (D3F_FLAG_FINITE_MAPS | D3F_FLAG_REFERENCE_ROUNDING)) && views->depth_nonfinite && mode == 0) {
        bool all = true;
        for (int s = 0; s < n_maps; ++s) all = all && maps && maps[s].nonfinite;
        if (all) {
            P.words[P.n_words++] = views->depth_nonfinite;
            for (int s = 0; s < n_maps; ++s) P.words[P.n_words++] = maps[s].nonfinite;
        }
    }
    for (int k = 0; k < P.n_words; ++k)
        if (!aligned(P.words[k], 4)) return fail(D3F_ERR_BAD_LAYOUT, "nonfinite word %d: device pointer must be 4-byte aligned", k);
    P.exp_stamps = nullptr;
#ifdef D3F_EXPERIMENTS
    if (tune.stamps > 0 && !plan_out) P.exp_stamps = exp_stamp_buffer(true);
#endif
    P.depth = views->depth; P.K = views->K; P.pose = views->pose; P.pts = pts;
    P.order = nullptr; P.lds_pad = 0;
    P.grid_x = grid ? grid->x : nullptr; P.grid_y = grid ? grid->y : nullptr; P.grid_z = grid ? grid->z : nullptr;
    P.grid_ny = grid ? grid->ny : 0; P.grid_nz = grid ? grid->nz : 0;
    P.walk_nx = P.walk_ny = P.walk_nz = 0; P.walk_tx = P.walk_ty = P.walk_tz = 1; P.walk_snake = 0;
    P.sl_unit = 128; P.sl_ilv = 1; P.sl_slices = 0; P.sl_lg = 3; P.sl_vc = 4; P.sl_tiles = P.sl_groups = P.sl_chunks = 0;
    P.runs_occ = tune.runs_occ;
    P.dist_variant = tune.dist;
    P.depth_tiled = nullptr; P.depth_tw = P.depth_th = 0;
    P.thin_max_views = (tune.thin < 0 || (flags & D3F_TUNE_DIRECT_GATHER)) ? 0 : 8;
    P.win_lpp = tune.window_lpp == 32 ? 32 : 16;     // 16 lanes x 2 vectors per point (C2 patch 0.565 -> 0.54 ms); U > 1: 32
    P.win_slices = 0; P.win_u = 1; P.win_vc = 1; P.win_pool_offset = 0; P.win_pool_texels = 0; P.win_occ = 4;
    P.win_pipe = tune.window_pipe < 0 ? 0 : 1;
    P.win_sparse = 0;
    P.rows = 0;
    P.gate = nullptr; P.gate_min = 0u; P.gate_want = 0;
    P.store_policy = tune.store < 0 ? 0 : (tune.store == 1 ? 1 : (tune.store == 3 ? 3 : 2));     // non-temporal rows (fuse_common.h: store_out)
    P.out_dist = out_dist; P.out_valid = out_valid;
    P.n = n; P.V = views->V; P.H = views->H; P.W = views->W;
    P.n_maps = n_maps; P.tile_pts = tile_points_for(views->V);
    P.flags = flags; P.mu = mu;

    Query q;
    q.views = views; q.n = n; q.n_maps = n_maps; q.flags = flags; q.mode = mode; q.lattice = lattice; q.grid = grid != nullptr;
    q.plan_only = plan_only; q.cloud_side = cloud_side; q.tune = tune;
    q.finite_expected = (flags & D3F_FLAG_FINITE_MAPS) || P.n_words > 0;
    q.direct = (flags & D3F_TUNE_DIRECT_GATHER) != 0;     // the plain direct gather in the chosen point order: the reference of the bit-identity tests
    q.tl = (int)((flags >> 8) & 0xF);
    q.map_bytes = 0;
    for (int s = 0; s < n_maps; ++s) {
        if (!plan_only && !out_fused[s]) return fail(D3F_ERR_INVALID_ARG, "map %d: output pointer is NULL", s);
        rc = fill_map(maps[s], s, views->V, out_fused ? out_fused[s] : nullptr, out_inter ? out_inter[s] : nullptr, nullptr,
                      P.maps[s], q.map_bytes, flags);
        if (rc != D3F_OK) return rc;
    }
    // The channel-sliced and the LDS-window kernels want THE wide map first (the thin ones ride along).  A map descriptor
    // carries its own output pointers, so the launch may take the maps in any order: return_names=['mask', 'dino_feats']
    // gets the same kernels as the reference's default ['dino_feats', 'mask'].  caller_map[k] = caller's index of P.maps[k].
    int caller_map[D3F_MAX_MAPS];
    for (int s = 0; s < D3F_MAX_MAPS; ++s) { caller_map[s] = s; q.want_inter[s] = false; }
    {
        int wide = -1, nwide = 0;
        for (int s = 0; s < n_maps; ++s)
            if ((int64_t)P.maps[s].C * P.maps[s].esize > 256) { if (wide < 0) wide = s; ++nwide; }
        if (nwide == 1 && wide > 0) {
            const d3f::MapDesc t = P.maps[0]; P.maps[0] = P.maps[wide]; P.maps[wide] = t;
            caller_map[0] = wide; caller_map[wide] = 0;
        }
        for (int s = 0; s < n_maps; ++s) q.want_inter[s] = out_inter && out_inter[caller_map[s]];
    }
    // Hilbert point order (performance only) when scratch is supplied
    hipStream_t hs = static_cast<hipStream_t>(stream);
    q.may_reorder = (workspace || plan_only) && !grid && n_maps > 0 && n <= 0x7fffffffLL && !(flags & D3F_TUNE_NO_REORDER) &&
                    workspace_bytes >= d3f::order_workspace_bytes(n);

    // ---- the plan: family + point order, then (device work) the order itself, then the geometry ----
    Plan pl;
    plan_family_and_order(q, P, pl);
    if (!pl.walk && pl.reorder && !plan_only) {
        if (flags & D3F_FLAG_REUSE_POINT_ORDER) {
            P.order = static_cast<const uint32_t *>(d3f::ws_at(workspace, d3f::order_layout(n).order));       // written by an earlier call for the same points
        } else {
            // Hilbert order of the cells of a 512^3 grid over the cloud's box, exact (order_kernels.hip); experiments builds: D3F_EXP_ORDER_MORTON=1 = the Z curve of rounds 1-4
            hipError_t eo = d3f::build_point_order(pts, n, workspace, workspace_bytes, &P.order, hs,
                                                   (tune.order_morton > 0 ? 1 : 0) | (tune.scan3 > 0 ? 2 : 0) | (tune.order_fixed_grid > 0 ? 4 : 0) | (tune.order_bits > 0 ? tune.order_bits << 8 : 0));
            if (eo != hipSuccess) return hip_fail(eo, "point ordering");
        }
    }
    plan_geometry(q, P, pl);
    const int64_t ntiles = plan_workgroups(P, pl, n);
    if (ntiles > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "n=%lld needs more than 2^31 workgroups", (long long)n);
    // the window and the channel-sliced kernels keep a point's global index in 32 bits of LDS (their rows already require
    // n < 2^31; this is the guard that says so)
    if ((pl.family == kFamWindow || pl.family == kFamRows || pl.family == kFamSliced) && n > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "n=%lld: 32-bit point indices", (long long)n);
    // the distance-only pass over a big batch in caller order, with scratch: the depth maps are tiled first (a plan query: would be)
    const bool tile_depth = n_maps == 0 && n >= d3f::kDistTiledMin && !P.order && P.walk_nx <= 0 && !P.grid_x && views->V <= 8 && tune.dist >= 0 &&
                            !(tune.dist & 32) && (workspace || plan_only) && workspace_bytes >= d3f::depth_tiled_bytes(views->V, views->H, views->W) &&
                            d3f::depth_tiled_bytes(views->V, views->H, views->W) < (1LL << 32);         // (32-bit pixel indices in the tiled copy)
    // (depth_tw > 0 is what selects the TILED instances, launch_dist; P.depth_tiled itself is set below, once the copy is enqueued)
    if (tile_depth) { P.depth_tw = (views->W + 3) / 4; P.depth_th = (views->H + 7) / 8; }
    if (plan_only) {
        plan_out->gated_window = 0; plan_out->reserved2 = 0; plan_out->window_kernel[0] = 0;
        if (cloud_side == 0 && !lattice && !grid) {       // would d3f_eval's first pass take the window side?  (its plan: the lattice's)
            d3f_eval_plan side;
            if (eval_common(views, pts, n, maps, n_maps, mu, flags, out_dist, out_valid, out_fused, out_inter, workspace, workspace_bytes,
                            stream, mode, &side, grid, lattice, 1) == D3F_OK)
                for (int s = 0; s < n_maps; ++s)
                    if (side.staged[s] == 3 && side.reorder == 1) {
                        plan_out->gated_window = 1; plan_out->reserved2 = side.reserved;
                        snprintf(plan_out->window_kernel, sizeof(plan_out->window_kernel), "%s", side.kernel);
                    }
        }
        report_plan(P, pl, caller_map, n_maps, ntiles, plan_out);
        (void)d3f::launch_fused_eval(P, pl.family, mode, d3f::Launch{ntiles, nullptr, plan_out});      // names the instance, launches nothing
        return D3F_OK;
    }
    // a cloud on the gated pair of launches: the window side (this pass) and the cell-run side (the next) read one device word
    const bool gated_window = cloud_side == 1 && pl.family == kFamWindow && !pl.walk && P.order != nullptr;
    const bool gated_runs = cloud_side == 2;
    uint32_t *gate = (gated_window || gated_runs) ? static_cast<uint32_t *>(d3f::ws_at(workspace, d3f::order_layout(n).gate)) : nullptr;
    if (gate) {
        P.gate = gate;
        P.gate_min = (uint32_t)D3F_GATE_MIN_FIT;                   // three quarters of the sampled tiles fit their pool
        if ((flags & D3F_TUNE_WINDOW_SIDE) || tune.gate > 0) P.gate_min = 0u;          // always the window side
        if (tune.gate < 0) P.gate_min = 0xffffffffu;                                    // experiments: always the cell runs
        P.gate_want = gated_window ? 1 : 0;
    }
    hipEvent_t ev0 = g_prof_start, ev1 = gated_window ? nullptr : g_prof_stop;
    g_prof_start = nullptr;
    if (!gated_window) g_prof_stop = nullptr;
    if (ev0) (void)hipEventRecord(ev0, hs);
    if (gated_window) {
        hipError_t ep = d3f::launch_window_gate_probe(P, gate, d3f::kGateSamples, hs);
        if (ep != hipSuccess) return hip_fail(ep, "window gate probe");
    }
    if (tile_depth) {                                  // (inside the timed pair)
        hipError_t et = d3f::launch_depth_tiles(P, static_cast<float *>(workspace), hs);
        if (et != hipSuccess) return hip_fail(et, "depth tiling");
        P.depth_tiled = static_cast<const float *>(workspace);
    }
    hipError_t e = d3f::launch_fused_eval(P, pl.family, mode, d3f::Launch{ntiles, hs, nullptr});
    if (ev1) (void)hipEventRecord(ev1, hs);
    if (e != hipSuccess) return hip_fail(e, "fused_eval launch");
    return gated_window ? kGatedSecondPass : D3F_OK;
}

}  // namespace

extern "C" {

int d3f_abi_version(void) { return D3F_ABI_VERSION; }
const char *d3f_version(void) { return "d3fields-hip 0.3.0 gfx950"; }
int d3f_build_has_experiments(void)
{
#ifdef D3F_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}
const char *d3f_last_error(void) { return g_err; }

int d3f_eval(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps, int32_t n_maps,
             float mu, uint32_t flags, float *out_dist, uint8_t *out_valid, float *const *out_fused,
             float *const *out_inter, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = eval_common(views, pts, n, maps, n_maps, mu, flags, out_dist, out_valid, out_fused, out_inter, workspace,
                         workspace_bytes, stream, 0, nullptr, nullptr, nullptr, 1);
    if (rc == kGatedSecondPass)         // a cloud: the window launch is enqueued behind its gate; now the cell-run launch behind the same word
        rc = eval_common(views, pts, n, maps, n_maps, mu, flags | D3F_FLAG_REUSE_POINT_ORDER, out_dist, out_valid, out_fused, out_inter,
                         workspace, workspace_bytes, stream, 0, nullptr, nullptr, nullptr, 2);
    return rc;
}

int64_t d3f_eval_workspace_bytes(int64_t n) { return d3f::order_workspace_bytes(n); }
int64_t d3f_eval_dist_workspace_bytes(const d3f_views *views, int64_t n)
{
    if (!views || n < d3f::kDistTiledMin || views->V < 1 || views->V > 8 || views->H < 1 || views->W < 1) return 0;
    const int64_t bytes = d3f::depth_tiled_bytes(views->V, views->H, views->W);
    return bytes < (1LL << 32) ? bytes : 0;
}

const char *d3f_plan_family_name(int32_t family) { return (family >= 0 && family < (int32_t)(sizeof(kFamilies) / sizeof(kFamilies[0]))) ? kFamilies[family].name : nullptr; }
const char *d3f_plan_family_takes(int32_t family) { return (family >= 0 && family < (int32_t)(sizeof(kFamilies) / sizeof(kFamilies[0]))) ? kFamilies[family].takes : nullptr; }

int64_t d3f_eval_gate_offset(int64_t n)
{
    return n <= 0 ? 0 : d3f::order_layout(n).gate;
}

void d3f_profile_next_eval(void *start_event, void *stop_event)
{
    g_prof_start = static_cast<hipEvent_t>(start_event);
    g_prof_stop = static_cast<hipEvent_t>(stop_event);
}

int d3f_eval_plan_query(const d3f_views *views, int64_t n, const d3f_channel_map *maps, int32_t n_maps, uint32_t flags,
                        int32_t have_workspace, int32_t want_inter, d3f_eval_plan *plan)
{
    if (!plan) return fail(D3F_ERR_INVALID_ARG, "plan is NULL");
    float *inter[D3F_MAX_MAPS];
    for (int s = 0; s < D3F_MAX_MAPS; ++s) inter[s] = want_inter ? reinterpret_cast<float *>(16) : nullptr;
    return eval_common(views, nullptr, n, maps, n_maps, 0.02f, flags, nullptr, nullptr, nullptr, want_inter ? inter : nullptr,
                       nullptr, have_workspace ? d3f::order_workspace_bytes(n) : 0, nullptr, 0, plan);
}

int d3f_eval_plan_query_lattice(const d3f_views *views, int32_t nx, int32_t ny, int32_t nz, const d3f_channel_map *maps,
                                int32_t n_maps, uint32_t flags, int32_t want_inter, d3f_eval_plan *plan)
{
    if (!plan) return fail(D3F_ERR_INVALID_ARG, "plan is NULL");
    if (nx < 0 || ny < 0 || nz < 0) return fail(D3F_ERR_BAD_SHAPE, "plan_query_lattice: negative size");
    float *inter[D3F_MAX_MAPS];
    for (int s = 0; s < D3F_MAX_MAPS; ++s) inter[s] = want_inter ? reinterpret_cast<float *>(16) : nullptr;
    const int32_t dims[3] = {nx, ny, nz};
    return eval_common(views, nullptr, (int64_t)nx * ny * nz, maps, n_maps, 0.02f, flags, nullptr, nullptr, nullptr,
                       want_inter ? inter : nullptr, nullptr, 0, nullptr, 0, plan, nullptr, dims);
}

int64_t d3f_backproject_workspace_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return d3f::pixel_counts_layout((int64_t)H * W).total;
}

int d3f_backproject_view(const double *depth, const uint8_t *mask, int32_t H, int32_t W, const double *cam_params,
                         const double *cam_to_world, const double *bounds, int64_t capacity, double *out_pts, int32_t *out_pixel,
                         int64_t *count_out, void *workspace, void *stream)
{
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "backproject: H=%d W=%d", H, W);
    if (!depth || !cam_params || !cam_to_world || !count_out || !workspace || capacity < 0 || (capacity > 0 && !out_pts))
        return fail(D3F_ERR_INVALID_ARG, "backproject: NULL pointer or negative capacity");
    if (!(cam_params[0] != 0.0) || !(cam_params[1] != 0.0)) return fail(D3F_ERR_INVALID_ARG, "backproject: fx/fy must be non-zero");
    hipError_t e = d3f::launch_backproject(depth, mask, H, W, cam_params, cam_to_world, bounds, capacity, out_pts, out_pixel,
                                           count_out, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "backproject launch");
}

int d3f_pcd_nearest(const double *a, int64_t na, const double *b, int64_t nb, double *min_dist, int64_t *argmin, void *stream)
{
    if (na < 0 || nb < 1) return fail(D3F_ERR_BAD_SHAPE, "pcd_nearest: na=%lld nb=%lld (nb must be >= 1)", (long long)na, (long long)nb);
    if (na == 0) return D3F_OK;
    if (!a || !b || !min_dist || !argmin) return fail(D3F_ERR_INVALID_ARG, "pcd_nearest: NULL pointer");
    hipError_t e = d3f::launch_nearest(a, na, b, nb, min_dist, argmin, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "pcd_nearest launch");
}

int d3f_pcd_to_index(const double *pts, int64_t n, const double *lower, double voxel_size, const int32_t *voxel_num,
                     int32_t *out_index, int32_t *out_voxel, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "pcd_to_index: n=%lld is negative", (long long)n);
    if (!lower || !voxel_num) return fail(D3F_ERR_INVALID_ARG, "pcd_to_index: lower / voxel_num (host arrays) are NULL");
    if (!(voxel_size != 0.0)) return fail(D3F_ERR_INVALID_ARG, "pcd_to_index: voxel_size must be non-zero");
    if (n == 0) return D3F_OK;
    if (!pts || !out_index) return fail(D3F_ERR_INVALID_ARG, "pcd_to_index: NULL pointer");
    if (const int rc = check_launch_blocks("pcd_to_index", n, d3f::kBlock)) return rc;
    hipError_t e = d3f::launch_pcd_to_index(pts, n, lower, voxel_size, voxel_num, out_index, out_voxel, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "pcd_to_index launch");
}

int64_t d3f_vox_iou_workspace_bytes(int64_t n1, int64_t n2)
{
    if (n1 < 0 || n2 < 0) return 0;
    return d3f::voxset_layout(n1, n2).total;
}

int d3f_vox_idx_iou(const int32_t *idx1, int64_t n1, const int32_t *idx2, int64_t n2, int64_t *out_counts, void *workspace,
                    int64_t workspace_bytes, void *stream)
{
    if (n1 < 0 || n2 < 0 || n1 + n2 > 0x3fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "vox_idx_iou: n1=%lld n2=%lld", (long long)n1, (long long)n2);
    if (!out_counts || (n1 > 0 && !idx1) || (n2 > 0 && !idx2)) return fail(D3F_ERR_INVALID_ARG, "vox_idx_iou: NULL pointer");
    if (const int rc = check_workspace("vox_idx_iou", workspace, workspace_bytes, d3f_vox_iou_workspace_bytes(n1, n2), 8)) return rc;
    if (!aligned(out_counts, 8)) return fail(D3F_ERR_BAD_LAYOUT, "vox_idx_iou: out_counts must be 8-byte aligned");
    hipError_t e = d3f::launch_voxset_iou(idx1, n1, idx2, n2, out_counts, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "vox_idx_iou launch");
}

int d3f_erode(const uint8_t *src, int32_t H, int32_t W, int32_t kh, int32_t kw, uint8_t *dst, void *stream)
{
    if (H < 0 || W < 0 || kh < 1 || kw < 1 || kh > 255 || kw > 255) return fail(D3F_ERR_BAD_SHAPE, "erode: H=%d W=%d kernel %dx%d", H, W, kh, kw);
    if ((int64_t)H * W == 0) return D3F_OK;
    if (!src || !dst || src == dst) return fail(D3F_ERR_INVALID_ARG, "erode: src/dst must be distinct non-NULL images");
    if (((int64_t)H * W + d3f::kBlock - 1) / d3f::kBlock > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "erode: image too large for one launch");
    hipError_t e = d3f::launch_erode(src, H, W, kh, kw, dst, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "erode launch");
}

int d3f_compose_labels(const uint8_t *dets, int32_t n_dets, int64_t n_pix, const int32_t *label_of_det, uint8_t *out, void *stream)
{
    if (n_dets < 0 || n_pix < 0 || n_pix > 0x3fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "compose_labels: n_dets=%d n_pix=%lld", n_dets, (long long)n_pix);
    if (n_pix == 0) return D3F_OK;
    if (!out || (n_dets > 0 && (!dets || !label_of_det))) return fail(D3F_ERR_INVALID_ARG, "compose_labels: NULL pointer");
    if (!aligned(label_of_det, 4)) return fail(D3F_ERR_BAD_LAYOUT, "compose_labels: label_of_det must be 4-byte aligned");
    hipError_t e = d3f::launch_compose_labels(dets, n_dets, n_pix, label_of_det, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "compose_labels launch");
}

int64_t d3f_voxel_downsample_workspace_bytes(int64_t n) { return n > 0 ? d3f::voxmean_layout(n).total : 0; }

int d3f_voxel_downsample(const double *pts, const double *colors, int64_t n, double voxel_size, double *out_pts, double *out_colors,
                         int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (n < 0 || n > 0x3fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "voxel_downsample: n=%lld", (long long)n);
    if (!(voxel_size > 0.0)) return fail(D3F_ERR_INVALID_ARG, "voxel_downsample: voxel_size must be > 0 (open3d raises too)");
    if (!count_out) return fail(D3F_ERR_INVALID_ARG, "voxel_downsample: count_out is NULL");
    if (n == 0) return hipMemsetAsync(count_out, 0, sizeof(int64_t), static_cast<hipStream_t>(stream)) == hipSuccess ? D3F_OK : D3F_ERR_HIP;
    if (!pts || !out_pts || (colors && !out_colors)) return fail(D3F_ERR_INVALID_ARG, "voxel_downsample: NULL pointer");
    if (const int rc = check_workspace("voxel_downsample", workspace, workspace_bytes, d3f_voxel_downsample_workspace_bytes(n), 16)) return rc;
    hipError_t e = d3f::launch_voxel_mean(pts, colors, n, voxel_size, out_pts, colors ? out_colors : nullptr, count_out, workspace,
                                          static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "voxel_downsample launch");
}

int d3f_mask_gate(const float *mask_channel, int64_t stride_y, int64_t stride_x, const float *depth, int32_t H, int32_t W,
                  float depth_lo, float depth_hi, uint8_t *out, void *stream)
{
    if (H < 0 || W < 0 || (int64_t)H * W > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "mask_gate: H=%d W=%d", H, W);
    if ((int64_t)H * W == 0) return D3F_OK;
    if (!mask_channel || !depth || !out) return fail(D3F_ERR_INVALID_ARG, "mask_gate: NULL pointer");
    hipError_t e = d3f::launch_mask_gate(mask_channel, stride_y, stride_x, depth, H, W, depth_lo, depth_hi, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "mask_gate launch");
}

int d3f_nonzero_pixels(const uint8_t *image, int32_t H, int32_t W, int64_t capacity, int32_t *out_row_col, int64_t *count_out,
                       void *workspace, void *stream)
{
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "nonzero_pixels: H=%d W=%d", H, W);
    if (!image || !count_out || !workspace || capacity < 0 || (capacity > 0 && !out_row_col))
        return fail(D3F_ERR_INVALID_ARG, "nonzero_pixels: NULL pointer or negative capacity");
    hipError_t e = d3f::launch_nonzero_pixels(image, H, W, capacity, out_row_col, count_out, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "nonzero_pixels launch");
}

int d3f_fps_pixels(const int32_t *pts, int64_t n, int32_t k, int64_t init_idx, int64_t *out_idx, double *out_maxdist,
                   void *workspace, void *stream)
{
    if (n < 1 || k < 0) return fail(D3F_ERR_BAD_SHAPE, "fps_pixels: n=%lld must be >= 1 (fps_np asserts a non-empty set), k=%d", (long long)n, k);
    if (k == 0) return D3F_OK;
    if (!pts || !out_idx || !workspace) return fail(D3F_ERR_INVALID_ARG, "fps_pixels: NULL pointer");
    if (!aligned(workspace, 16)) return fail(D3F_ERR_BAD_LAYOUT, "fps_pixels: workspace must be 16-byte aligned");
    if (init_idx < 0 || init_idx >= n) return fail(D3F_ERR_INVALID_ARG, "fps_pixels: init_idx=%lld outside [0,%lld)", (long long)init_idx, (long long)n);
    hipError_t e = d3f::launch_fps_pixels(pts, n, k, init_idx, out_idx, out_maxdist, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "fps_pixels launch");
}

static int check_grid(const d3f_grid *g)
{
    if (!g) return fail(D3F_ERR_INVALID_ARG, "grid is NULL");
    if (g->nx < 0 || g->ny < 0 || g->nz < 0) return fail(D3F_ERR_BAD_SHAPE, "grid: negative size");
    if ((int64_t)g->nx * g->ny * g->nz > 0 && (!g->x || !g->y || !g->z)) return fail(D3F_ERR_INVALID_ARG, "grid: axis arrays must be non-NULL");
    return D3F_OK;
}

int d3f_eval_grid(const d3f_views *views, const d3f_grid *grid, const d3f_channel_map *maps, int32_t n_maps, float mu,
                  uint32_t flags, float *out_dist, uint8_t *out_valid, float *const *out_fused, void *stream)
{
    int rc = check_grid(grid);
    if (rc != D3F_OK) return rc;
    const int32_t dims[3] = {grid->nx, grid->ny, grid->nz};
    return eval_common(views, nullptr, (int64_t)grid->nx * grid->ny * grid->nz, maps, n_maps, mu, flags, out_dist, out_valid,
                       out_fused, nullptr, nullptr, 0, stream, 0, nullptr, grid, dims);
}

int d3f_eval_lattice(const d3f_views *views, const float *pts, int32_t nx, int32_t ny, int32_t nz, const d3f_channel_map *maps,
                     int32_t n_maps, float mu, uint32_t flags, float *out_dist, uint8_t *out_valid, float *const *out_fused,
                     float *const *out_inter, void *stream)
{
    if (nx < 0 || ny < 0 || nz < 0) return fail(D3F_ERR_BAD_SHAPE, "eval_lattice: negative size");
    const int32_t dims[3] = {nx, ny, nz};
    return eval_common(views, pts, (int64_t)nx * ny * nz, maps, n_maps, mu, flags, out_dist, out_valid, out_fused, out_inter,
                       nullptr, 0, stream, 0, nullptr, nullptr, dims);
}

int64_t d3f_grid_shell_workspace_bytes(const d3f_grid *grid)
{
    if (!grid || grid->nx <= 0 || grid->ny <= 0 || grid->nz <= 0) return 0;
    return d3f::grid_shell_layout((int64_t)grid->nx * grid->ny * grid->nz).total;
}

int d3f_grid_shell(const d3f_views *views, const d3f_grid *grid, float mu, float dist_thr, int64_t capacity, int64_t *idx_out,
                   int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_views(views);
    if (rc != D3F_OK) return rc;
    rc = check_grid(grid);
    if (rc != D3F_OK) return rc;
    if (!count_out || capacity < 0 || (capacity > 0 && !idx_out)) return fail(D3F_ERR_INVALID_ARG, "grid_shell: idx_out/count_out/capacity");
    if ((int64_t)grid->nx * grid->ny * grid->nz > 0 && (!workspace || workspace_bytes < d3f_grid_shell_workspace_bytes(grid)))
        return fail(D3F_ERR_WORKSPACE, "grid_shell: needs %lld workspace bytes", (long long)d3f_grid_shell_workspace_bytes(grid));
    if (!(mu > 0.0f)) return fail(D3F_ERR_INVALID_ARG, "mu must be > 0");
    if (((int64_t)grid->nx * grid->ny * grid->nz + d3f::kBlock - 1) / d3f::kBlock > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "grid too large for one launch");
    // a workspace with d3f_eval_dist_workspace_bytes(views, n) bytes MORE than the shell needs: the depth lookups go to a tiled copy there
    const int64_t n_grid = (int64_t)grid->nx * grid->ny * grid->nz, tiled_bytes = d3f_eval_dist_workspace_bytes(views, n_grid);
    const d3f::ShellTiledLayout L = d3f::grid_shell_tiled_layout(n_grid, tiled_bytes);
    float *tiled = (tiled_bytes > 0 && workspace_bytes >= L.total) ? static_cast<float *>(d3f::ws_at(workspace, L.tiles)) : nullptr;
    hipError_t e = d3f::launch_grid_shell(views->depth, views->K, views->pose, views->V, views->H, views->W, grid->x, grid->y,
                                          grid->z, grid->nx, grid->ny, grid->nz, mu, dist_thr, capacity, idx_out,
                                          reinterpret_cast<unsigned long long *>(count_out), workspace, static_cast<hipStream_t>(stream),
                                          tiled);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "grid_shell launch");
}

// ---- iso-surface extraction and volume smoothing (mesh_kernels.hip) ----
static int check_mesh(const char *who, const float *volume, int32_t nx, int32_t ny, int32_t nz, const int64_t *counts_out, const void *workspace,
                      int64_t workspace_bytes)
{
    if (nx < 2 || ny < 2 || nz < 2) return fail(D3F_ERR_BAD_SHAPE, "%s: nx=%d ny=%d nz=%d, every extent must be >= 2", who, nx, ny, nz);
    if ((int64_t)nx * ny * nz > 0x7fffffffLL / 3)
        return fail(D3F_ERR_BAD_SHAPE, "%s: %lld points exceed (2^31 - 1) / 3 (32-bit vertex and triangle indices)", who, (long long)nx * ny * nz);
    if (!volume || !counts_out) return fail(D3F_ERR_INVALID_ARG, "%s: volume / counts_out must be non-NULL", who);
    if (!aligned(volume, 4) || !aligned(counts_out, 8)) return fail(D3F_ERR_BAD_LAYOUT, "%s: volume / counts_out must be aligned to their element size", who);
    return check_workspace(who, workspace, workspace_bytes, d3f_mesh_workspace_bytes(nx, ny, nz), 4);
}

int64_t d3f_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    return d3f::mesh_layout((int64_t)nx * ny * nz).total;
}

int d3f_mesh_count(const float *volume, const uint8_t *valid, int32_t nx, int32_t ny, int32_t nz, float iso, int64_t *counts_out,
                   void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = check_mesh("mesh_count", volume, nx, ny, nz, counts_out, workspace, workspace_bytes);
    if (rc != D3F_OK) return rc;
    if (iso != iso) return fail(D3F_ERR_INVALID_ARG, "mesh_count: iso is NaN");
    hipError_t e = d3f::launch_mesh(volume, valid, nx, ny, nz, iso, 0, 0, nullptr, nullptr, nullptr, counts_out, workspace, false,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "mesh_count launch");
}

int d3f_mesh_extract(const float *volume, const uint8_t *valid, int32_t nx, int32_t ny, int32_t nz, float iso,
                     int64_t vertex_capacity, int64_t triangle_capacity, int64_t *keys_out, float *t_out, int32_t *triangles_out,
                     int64_t *counts_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = check_mesh("mesh_extract", volume, nx, ny, nz, counts_out, workspace, workspace_bytes);
    if (rc != D3F_OK) return rc;
    if (iso != iso) return fail(D3F_ERR_INVALID_ARG, "mesh_extract: iso is NaN");
    if (vertex_capacity < 0 || triangle_capacity < 0) return fail(D3F_ERR_INVALID_ARG, "mesh_extract: negative capacity");
    if ((vertex_capacity > 0 && (!keys_out || !t_out)) || (triangle_capacity > 0 && !triangles_out))
        return fail(D3F_ERR_INVALID_ARG, "mesh_extract: keys_out / t_out / triangles_out must be non-NULL for a positive capacity");
    if (!aligned(keys_out, 8) || !aligned(t_out, 4) || !aligned(triangles_out, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "mesh_extract: outputs must be aligned to their element size");
    hipError_t e = d3f::launch_mesh(volume, valid, nx, ny, nz, iso, vertex_capacity, triangle_capacity, keys_out, t_out, triangles_out,
                                    counts_out, workspace, true, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "mesh_extract launch");
}

int64_t d3f_volume_gaussian_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return (int64_t)nx * ny * nz * 4;
}

int d3f_volume_gaussian(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, float sigma, float truncate,
                        void *workspace, int64_t workspace_bytes, void *stream)
{
    if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz > 0x7fffffffLL)
        return fail(D3F_ERR_BAD_SHAPE, "volume_gaussian: nx=%d ny=%d nz=%d", nx, ny, nz);
    if (!(sigma > 0.0f) || !(truncate > 0.0f) || sigma * truncate > 1e6f) return fail(D3F_ERR_INVALID_ARG, "volume_gaussian: sigma and truncate must be > 0 and finite");
    // scipy: lw = int(truncate * sd + 0.5), in double on the double values of the arguments
    const int radius = (int)((double)truncate * (double)sigma + 0.5);
    if (radius > D3F_GAUSSIAN_MAX_RADIUS)
        return fail(D3F_ERR_BAD_SHAPE, "volume_gaussian: radius %d exceeds D3F_GAUSSIAN_MAX_RADIUS = %d", radius, D3F_GAUSSIAN_MAX_RADIUS);
    if (!src || !dst || src == dst) return fail(D3F_ERR_INVALID_ARG, "volume_gaussian: src / dst must be distinct non-NULL volumes");
    if (const int rc = check_workspace("volume_gaussian", workspace, workspace_bytes, d3f_volume_gaussian_workspace_bytes(nx, ny, nz), 4)) return rc;
    if (!aligned(src, 4) || !aligned(dst, 4)) return fail(D3F_ERR_BAD_LAYOUT, "volume_gaussian: src / dst must be 4-byte aligned");
    // scipy _gaussian_kernel1d: phi = exp(-0.5 / sigma^2 * x^2), phi / phi.sum(), float64
    double w[D3F_GAUSSIAN_MAX_RADIUS + 1], sum = 0.0;
    const double sd = (double)sigma;
    for (int k = 0; k <= radius; ++k) {
        w[k] = exp(-0.5 / (sd * sd) * (double)k * (double)k);
        sum += k == 0 ? w[k] : 2.0 * w[k];
    }
    float wf[D3F_GAUSSIAN_MAX_RADIUS + 1];
    for (int k = 0; k <= radius; ++k) wf[k] = (float)(w[k] / sum);
    hipError_t e = d3f::launch_volume_gaussian(src, dst, nx, ny, nz, wf, radius, static_cast<float *>(workspace), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_gaussian launch");
}

// ---- trilinear lookups in a baked volume (volume_kernels.hip) ----
static int check_volume(const char *who, const d3f_volume *vol)
{
    if (!vol) return fail(D3F_ERR_INVALID_ARG, "%s: vol is NULL", who);
    if (vol->nx < 2 || vol->ny < 2 || vol->nz < 2 || vol->nx > (1 << 24) || vol->ny > (1 << 24) || vol->nz > (1 << 24))
        return fail(D3F_ERR_BAD_SHAPE, "%s: vol nx=%d ny=%d nz=%d, every extent must be in [2, 2^24]", who, vol->nx, vol->ny, vol->nz);
    if ((int64_t)vol->nx * vol->ny * vol->nz > 0x7fffffffLL)
        return fail(D3F_ERR_BAD_SHAPE, "%s: vol holds %lld voxels, more than 2^31 - 1", who, (long long)vol->nx * vol->ny * vol->nz);
    return D3F_OK;
}

int d3f_volume_cell_valid(const d3f_volume *vol, uint8_t *cell_valid_out, void *stream)
{
    const int rc = check_volume("volume_cell_valid", vol);
    if (rc != D3F_OK) return rc;
    if (!vol->valid || !cell_valid_out) return fail(D3F_ERR_INVALID_ARG, "volume_cell_valid: vol->valid / cell_valid_out must be non-NULL");
    hipError_t e = d3f::launch_volume_cell_valid(vol->valid, cell_valid_out, vol->nx, vol->ny, vol->nz, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_cell_valid launch");
}

// the checks the forward and the backward lookup share; fills P but for the outputs / gradients.  Returns 1 for "nothing to do".
static int volume_common(const char *who, const d3f_volume *vol, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                         d3f::VolParams &P, bool null_data_ok = false, bool half_ok = true)
{
    const int rc = check_volume(who, vol);
    if (rc != D3F_OK) return rc;
    if (!positive_finite(vol->step)) return fail(D3F_ERR_INVALID_ARG, "%s: vol->step must be > 0 and finite", who);
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "%s: n=%lld is negative", who, (long long)n);
    if (n_sets < 0 || n_sets > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_sets=%d outside [0,%d]", who, n_sets, D3F_MAX_MAPS);
    if (n_sets > 0 && !sets) return fail(D3F_ERR_INVALID_ARG, "%s: sets is NULL with n_sets=%d", who, n_sets);
    for (int s = 0; s < n_sets; ++s) {
        if (const int rc = check_set_shape(who, s, sets[s])) return rc;
        if (const int rc = check_set_storage(who, s, sets[s], half_ok)) return rc;
    }
    if (n == 0) return 1;
    if (!vol->dist || !vol->cell_valid || !pts) return fail(D3F_ERR_INVALID_ARG, "%s: vol->dist / vol->cell_valid / pts must be non-NULL", who);
    if (!aligned(vol->dist, 4) || !aligned(pts, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: vol->dist / pts must be 4-byte aligned", who);
    for (int s = 0; s < n_sets; ++s) {
        if (!sets[s].data && !null_data_ok) return fail(D3F_ERR_INVALID_ARG, "%s: set %d: data is NULL", who, s);
        if (const int rc = check_set_layout(who, s, sets[s])) return rc;
        if (!aligned(sets[s].fill, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: fill must be 4-byte aligned", who, s);
        d3f::VolSet &S = P.sets[s];
        S.data = sets[s].data;
        S.fill = sets[s].fill;
        S.out = nullptr;
        S.grad = nullptr;
        S.stride = sets[s].stride_voxel;
        S.C = sets[s].C;
        S.vec = set_reads_vectors(sets[s]) ? 1 : 0;      // and-ed with the alignment of out / grad by the caller
        S.f16 = set_is_half(sets[s]) ? 1 : 0;
    }
    P.dist = vol->dist;
    P.cell = vol->cell_valid;
    P.pts = pts;
    P.out_dist = nullptr;
    P.out_valid = nullptr;
    P.grad_dist = nullptr;
    P.grad_pts = nullptr;
    P.n = n;
    P.nx = vol->nx; P.ny = vol->ny; P.nz = vol->nz;
    P.ox = vol->origin[0]; P.oy = vol->origin[1]; P.oz = vol->origin[2];
    P.h = vol->step;
    P.rh = 1.0f / vol->step;
    P.n_sets = n_sets;
    return D3F_OK;
}

int d3f_volume_sample(const d3f_volume *vol, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets, float *out_dist,
                      uint8_t *out_valid, void *const *out_sets, void *stream)
{
    d3f::VolParams P;
    const int rc = volume_common("volume_sample", vol, pts, n, sets, n_sets, P);
    if (rc != D3F_OK) return rc == 1 ? D3F_OK : rc;
    if (!out_dist || !out_valid || (n_sets > 0 && !out_sets)) return fail(D3F_ERR_INVALID_ARG, "volume_sample: out_dist / out_valid / out_sets must be non-NULL");
    if (!aligned(out_dist, 4)) return fail(D3F_ERR_BAD_LAYOUT, "volume_sample: out_dist must be 4-byte aligned");
    if (const int rc = attach_outputs("volume_sample", P, n_sets, out_sets)) return rc;
    P.out_dist = out_dist;
    P.out_valid = out_valid;
    hipError_t e = d3f::launch_volume_sample(P, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_sample launch");
}

int d3f_volume_sample_backward(const d3f_volume *vol, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                               const float *grad_dist, const void *const *grad_sets, float *grad_pts, void *stream)
{
    d3f::VolParams P;
    const int rc = volume_common("volume_sample_backward", vol, pts, n, sets, n_sets, P);
    if (rc != D3F_OK) return rc == 1 ? D3F_OK : rc;
    if (!grad_pts) return fail(D3F_ERR_INVALID_ARG, "volume_sample_backward: grad_pts is NULL");
    if (!aligned(grad_pts, 4) || !aligned(grad_dist, 4)) return fail(D3F_ERR_BAD_LAYOUT, "volume_sample_backward: grad_pts / grad_dist must be 4-byte aligned");
    if (const int rc = attach_grads("volume_sample_backward", P, n_sets, grad_sets)) return rc;
    P.grad_dist = grad_dist;
    P.grad_pts = grad_pts;
    hipError_t e = d3f::launch_volume_backward(P, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_sample_backward launch");
}

// ---- a baked volume with rows only near the surface (band_kernels.hip) ----
int64_t d3f_band_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz > 0x7fffffffLL) return 0;
    return d3f::band_workspace_bytes((int64_t)nx * ny * nz);
}

int d3f_band_mark(const d3f_volume *vol, float band, uint8_t *cell_band_out, int32_t *slot_out, int32_t *voxels_out, int64_t capacity,
                  int64_t *count_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = check_volume("band_mark", vol);
    if (rc != D3F_OK) return rc;
    if (!positive_finite(band)) return fail(D3F_ERR_INVALID_ARG, "band_mark: band must be > 0 and finite");
    if (capacity < 0) return fail(D3F_ERR_INVALID_ARG, "band_mark: capacity=%lld is negative", (long long)capacity);
    if (!vol->dist || !vol->cell_valid) return fail(D3F_ERR_INVALID_ARG, "band_mark: vol->dist / vol->cell_valid must be non-NULL");
    if (!cell_band_out || !slot_out || !count_out || (capacity > 0 && !voxels_out))
        return fail(D3F_ERR_INVALID_ARG, "band_mark: cell_band_out / slot_out / count_out (and voxels_out for a positive capacity) must be non-NULL");
    if (!aligned(vol->dist, 4) || !aligned(slot_out, 4) || !aligned(voxels_out, 4) || !aligned(count_out, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "band_mark: vol->dist / slot_out / voxels_out / count_out must be aligned to their element size");
    if (const int rc = check_workspace("band_mark", workspace, workspace_bytes, d3f_band_workspace_bytes(vol->nx, vol->ny, vol->nz), 4)) return rc;
    hipError_t e = d3f::launch_band_mark(vol->dist, vol->cell_valid, vol->nx, vol->ny, vol->nz, band, cell_band_out, slot_out, voxels_out, capacity,
                                         count_out, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "band_mark launch");
}

// the checks of the band on top of volume_common's; fills B but for the outputs / gradients.  Returns 1 for "nothing to do".
static int band_common(const char *who, const d3f_volume *vol, const d3f_band *band, const float *pts, int64_t n, const d3f_volume_set *sets,
                       int32_t n_sets, d3f::BandParams &B)
{
    if (!band) return fail(D3F_ERR_INVALID_ARG, "%s: band is NULL", who);
    if (band->n_rows < 0 || band->n_rows > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "%s: band->n_rows=%lld outside [0, 2^31 - 1]", who, (long long)band->n_rows);
    const bool empty = band->n_rows == 0;
    const int rc = volume_common(who, vol, pts, n, sets, n_sets, B.V, empty);
    if (rc != D3F_OK) return rc;
    if (!empty && (!band->slot || !band->cell_band)) return fail(D3F_ERR_INVALID_ARG, "%s: band->slot / band->cell_band must be non-NULL with n_rows > 0", who);
    if (!empty && !aligned(band->slot, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: band->slot must be 4-byte aligned", who);
    B.slot = empty ? nullptr : band->slot;
    B.cell_band = empty ? nullptr : band->cell_band;      // nullptr: the kernels read nothing of the band and no row
    B.out_in_band = nullptr;
    return D3F_OK;
}

int d3f_band_sample(const d3f_volume *vol, const d3f_band *band, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                    float *out_dist, uint8_t *out_valid, uint8_t *out_in_band, void *const *out_sets, void *stream)
{
    d3f::BandParams B;
    const int rc = band_common("band_sample", vol, band, pts, n, sets, n_sets, B);
    if (rc != D3F_OK) return rc == 1 ? D3F_OK : rc;
    if (!out_dist || !out_valid || !out_in_band || (n_sets > 0 && !out_sets))
        return fail(D3F_ERR_INVALID_ARG, "band_sample: out_dist / out_valid / out_in_band / out_sets must be non-NULL");
    if (!aligned(out_dist, 4)) return fail(D3F_ERR_BAD_LAYOUT, "band_sample: out_dist must be 4-byte aligned");
    if (const int rc = attach_outputs("band_sample", B.V, n_sets, out_sets)) return rc;
    B.V.out_dist = out_dist;
    B.V.out_valid = out_valid;
    B.out_in_band = out_in_band;
    hipError_t e = d3f::launch_band_sample(B, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "band_sample launch");
}

int d3f_band_sample_backward(const d3f_volume *vol, const d3f_band *band, const float *pts, int64_t n, const d3f_volume_set *sets, int32_t n_sets,
                             const float *grad_dist, const void *const *grad_sets, float *grad_pts, void *stream)
{
    d3f::BandParams B;
    const int rc = band_common("band_sample_backward", vol, band, pts, n, sets, n_sets, B);
    if (rc != D3F_OK) return rc == 1 ? D3F_OK : rc;
    if (!grad_pts) return fail(D3F_ERR_INVALID_ARG, "band_sample_backward: grad_pts is NULL");
    if (!aligned(grad_pts, 4) || !aligned(grad_dist, 4)) return fail(D3F_ERR_BAD_LAYOUT, "band_sample_backward: grad_pts / grad_dist must be 4-byte aligned");
    if (const int rc = attach_grads("band_sample_backward", B.V, n_sets, grad_sets)) return rc;
    B.V.grad_dist = grad_dist;
    B.V.grad_pts = grad_pts;
    hipError_t e = d3f::launch_band_backward(B, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "band_sample_backward launch");
}

// ---- the exact Euclidean distance transform of a site volume (edt_kernels.hip) ----
int64_t d3f_volume_edt_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    return edt_shape_ok(nx, ny, nz) ? d3f::edt_layout((int64_t)nx * ny * nz).total : 0;
}

int d3f_volume_edt(const uint8_t *site, int32_t nx, int32_t ny, int32_t nz, float step, int32_t max_d2, int32_t *out_d2, int32_t *out_nearest,
                   float *out_dist, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!site) return fail(D3F_ERR_INVALID_ARG, "volume_edt: site is NULL");
    if (!out_d2 && !out_nearest && !out_dist) return fail(D3F_ERR_INVALID_ARG, "volume_edt: out_d2, out_nearest and out_dist are all NULL");
    if (const int rc = check_extents("volume_edt", nx, ny, nz)) return rc;
    if (max_d2 < 0) return fail(D3F_ERR_INVALID_ARG, "volume_edt: max_d2=%d is negative (0: no cap)", max_d2);
    if (out_dist && !positive_finite(step)) return fail(D3F_ERR_INVALID_ARG, "volume_edt: step must be > 0 and finite with out_dist");
    if (!aligned(out_d2, 4) || !aligned(out_nearest, 4) || !aligned(out_dist, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_edt: out_d2 / out_nearest / out_dist must be 4-byte aligned");
    if (const int rc = check_workspace("volume_edt", workspace, workspace_bytes, d3f_volume_edt_workspace_bytes(nx, ny, nz), 4)) return rc;
    hipError_t e = d3f::launch_volume_edt(site, nx, ny, nz, step, max_d2 > 0 ? max_d2 : 0x7fffffff, out_d2, out_nearest, out_dist, workspace,
                                          static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_edt launch");
}

// ---- connected components of a site volume (ccl_kernels.hip) ----
int64_t d3f_volume_components_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    return edt_shape_ok(nx, ny, nz) ? d3f::ccl_layout((int64_t)nx * ny * nz).total : 0;
}

// both forms: every pair of neighbouring sites is joined, or (linked) only the pairs whose bit of links is set (d3f_volume_links)
static int components_impl(const char *who, bool linked, const uint8_t *site, const uint16_t *links, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity,
                           int32_t min_voxels, int32_t *out_label, int32_t *out_count, int32_t *out_stats, int32_t stats_capacity, void *workspace,
                           int64_t workspace_bytes, void *stream)
{
    if (!site) return fail(D3F_ERR_INVALID_ARG, "%s: site is NULL", who);
    if (linked && !links) return fail(D3F_ERR_INVALID_ARG, "%s: links is NULL", who);
    if (!out_label || !out_count) return fail(D3F_ERR_INVALID_ARG, "%s: out_label or out_count is NULL", who);
    if (const int rc = check_connectivity(who, connectivity)) return rc;
    if (min_voxels < 1) return fail(D3F_ERR_INVALID_ARG, "%s: min_voxels=%d, must be >= 1", who, min_voxels);
    if (stats_capacity < 0) return fail(D3F_ERR_INVALID_ARG, "%s: stats_capacity=%d is negative", who, stats_capacity);
    if (stats_capacity > 0 && !out_stats) return fail(D3F_ERR_INVALID_ARG, "%s: out_stats is NULL with stats_capacity=%d", who, stats_capacity);
    if (const int rc = check_extents(who, nx, ny, nz)) return rc;
    if (!aligned(links, 2)) return fail(D3F_ERR_BAD_LAYOUT, "%s: links must be 2-byte aligned", who);
    if (!aligned(out_label, 4) || !aligned(out_count, 4) || !aligned(out_stats, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: out_label / out_count / out_stats must be 4-byte aligned", who);
    if (const int rc = check_workspace(who, workspace, workspace_bytes, d3f_volume_components_workspace_bytes(nx, ny, nz), 4)) return rc;
    int32_t *stats = stats_capacity > 0 ? out_stats : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = linked ? d3f::launch_volume_components_linked(site, links, nx, ny, nz, connectivity, min_voxels, out_label, out_count, stats, stats_capacity, workspace, s)
                          : d3f::launch_volume_components(site, nx, ny, nz, connectivity, min_voxels, out_label, out_count, stats, stats_capacity, workspace, s);
    return e == hipSuccess ? D3F_OK : fail(D3F_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
}

int d3f_volume_components(const uint8_t *site, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, int32_t min_voxels, int32_t *out_label,
                          int32_t *out_count, int32_t *out_stats, int32_t stats_capacity, void *workspace, int64_t workspace_bytes, void *stream)
{
    return components_impl("volume_components", false, site, nullptr, nx, ny, nz, connectivity, min_voxels, out_label, out_count, out_stats, stats_capacity,
                           workspace, workspace_bytes, stream);
}

int d3f_volume_components_linked(const uint8_t *site, const uint16_t *links, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, int32_t min_voxels,
                                 int32_t *out_label, int32_t *out_count, int32_t *out_stats, int32_t stats_capacity, void *workspace, int64_t workspace_bytes,
                                 void *stream)
{
    return components_impl("volume_components_linked", true, site, links, nx, ny, nz, connectivity, min_voxels, out_label, out_count, out_stats, stats_capacity,
                           workspace, workspace_bytes, stream);
}

// ---- descriptor-gated links between neighbouring voxels (parts_kernels.hip) ----
int d3f_volume_links(const uint8_t *site, const uint8_t *valid, const int32_t *slot, int32_t nx, int32_t ny, int32_t nz, const d3f_volume_set *set, int32_t rule,
                     float threshold, int32_t connectivity, uint16_t *out_links, void *stream)
{
    if (!site || !set || !out_links) return fail(D3F_ERR_INVALID_ARG, "volume_links: site, set or out_links is NULL");
    if (!set->data) return fail(D3F_ERR_INVALID_ARG, "volume_links: set->data is NULL");
    if (rule != D3F_LINK_L2 && rule != D3F_LINK_COSINE && rule != D3F_LINK_ARGMAX) return fail(D3F_ERR_INVALID_ARG, "volume_links: unknown rule %d", rule);
    if (const int rc = check_connectivity("volume_links", connectivity)) return rc;
    if (threshold != threshold) return fail(D3F_ERR_INVALID_ARG, "volume_links: threshold is NaN (+Inf accepts every pair of finite rows under D3F_LINK_L2)");
    if (rule == D3F_LINK_COSINE && !(threshold >= 0.0f && threshold <= 1.0f))
        return fail(D3F_ERR_INVALID_ARG, "volume_links: threshold=%g, the cosine bound must lie in [0, 1]", (double)threshold);
    if (const int rc = check_extents("volume_links", nx, ny, nz)) return rc;
    if (const int rc = check_set_shape("volume_links", 0, *set)) return rc;
    if (const int rc = check_set_storage("volume_links", 0, *set, false)) return rc;
    if (const int rc = check_set_layout("volume_links", 0, *set)) return rc;
    if (!aligned(slot, 4) || !aligned(out_links, 2)) return fail(D3F_ERR_BAD_LAYOUT, "volume_links: slot must be 4-byte aligned, out_links 2-byte aligned");
    hipError_t e = d3f::launch_volume_links(site, valid, slot, nx, ny, nz, set->data, set->C, set->stride_voxel, set_reads_vectors(*set), rule, threshold,
                                            connectivity, out_links, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_links launch");
}

// ---- dense descriptor flow between two fields on one grid (flow_kernels.hip) ----
int d3f_volume_flow(const uint8_t *site_a, const int32_t *slot_a, const d3f_volume_set *set_a, const uint8_t *site_b, const int32_t *slot_b,
                    const d3f_volume_set *set_b, int32_t nx, int32_t ny, int32_t nz, int32_t radius, float max_cost2, int32_t *out_target, float *out_cost,
                    float *out_axis_cost, void *stream)
{
    if (!site_a || !site_b || !set_a || !set_b) return fail(D3F_ERR_INVALID_ARG, "volume_flow: site_a, site_b, set_a or set_b is NULL");
    if (!set_a->data || !set_b->data) return fail(D3F_ERR_INVALID_ARG, "volume_flow: set_a->data or set_b->data is NULL");
    if (!out_target || !out_cost) return fail(D3F_ERR_INVALID_ARG, "volume_flow: out_target or out_cost is NULL");
    if (radius < 1 || radius > D3F_FLOW_MAX_RADIUS) return fail(D3F_ERR_INVALID_ARG, "volume_flow: radius=%d outside [1,%d]", radius, D3F_FLOW_MAX_RADIUS);
    if (max_cost2 != max_cost2) return fail(D3F_ERR_INVALID_ARG, "volume_flow: max_cost2 is NaN (+Inf means no threshold)");
    if (const int rc = check_extents("volume_flow", nx, ny, nz)) return rc;
    if (const int rc = check_set_shape("volume_flow", 0, *set_a)) return rc;             // set 0: set_a, set 1: set_b
    if (set_b->C != set_a->C) return fail(D3F_ERR_BAD_SHAPE, "volume_flow: C=%d of set_a, C=%d of set_b: the sets must have the same width", set_a->C, set_b->C);
    if (const int rc = check_set_storage("volume_flow", 0, *set_a, false)) return rc;
    if (const int rc = check_set_storage("volume_flow", 1, *set_b, false)) return rc;
    if (const int rc = check_set_layout("volume_flow", 0, *set_a)) return rc;
    if (const int rc = check_set_layout("volume_flow", 1, *set_b)) return rc;
    if (!aligned(slot_a, 4) || !aligned(slot_b, 4) || !aligned(out_target, 4) || !aligned(out_cost, 4) || !aligned(out_axis_cost, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_flow: slots and outputs must be 4-byte aligned");
    const bool vec = set_reads_vectors(*set_a) && set_reads_vectors(*set_b);                // (one width: checked above)
    hipError_t e = d3f::launch_volume_flow(site_a, slot_a, set_a->data, set_a->stride_voxel, site_b, slot_b, set_b->data, set_b->stride_voxel, set_a->C, vec, nx,
                                           ny, nz, radius, max_cost2, out_target, out_cost, out_axis_cost, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_flow launch");
}

// ---- mean rows, votes and moments per component (pool_kernels.hip) ----
static bool pool_shape_ok(int32_t nx, int32_t ny, int32_t nz, int32_t K)
{
    return edt_shape_ok(nx, ny, nz) && (int64_t)K <= (int64_t)nx * ny * nz;
}

int64_t d3f_volume_pool_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t K, int64_t member_capacity, int64_t mean_channels)
{
    if (K < 0 || member_capacity < 0 || mean_channels < 0 || mean_channels > (int64_t)D3F_MAX_MAPS * D3F_VOLUME_MAX_CHANNELS) return 0;
    if (!pool_shape_ok(nx, ny, nz, K)) return 0;
    return d3f::pool_workspace_bytes((int64_t)nx * ny * nz, K, member_capacity, mean_channels);
}

int d3f_volume_pool(const int32_t *label, int32_t nx, int32_t ny, int32_t nz, int32_t K, const uint8_t *valid, const int32_t *slot,
                    const d3f_volume_set *sets, int32_t n_sets, const int32_t *modes, int64_t member_capacity, int64_t *out_members,
                    int32_t *out_count, int64_t *out_moments, void *const *out_rows, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!label || !out_members || !out_count) return fail(D3F_ERR_INVALID_ARG, "volume_pool: label, out_members or out_count is NULL");
    if (K < 0) return fail(D3F_ERR_INVALID_ARG, "volume_pool: K=%d is negative", K);
    if (n_sets < 0 || n_sets > D3F_MAX_MAPS) return fail(D3F_ERR_INVALID_ARG, "volume_pool: n_sets=%d outside [0,%d]", n_sets, D3F_MAX_MAPS);
    if (n_sets > 0 && (!sets || !modes || !out_rows)) return fail(D3F_ERR_INVALID_ARG, "volume_pool: sets, modes or out_rows is NULL with n_sets=%d", n_sets);
    for (int s = 0; s < n_sets; ++s) {
        if (!sets[s].data || !out_rows[s]) return fail(D3F_ERR_INVALID_ARG, "volume_pool: set %d: data or out_rows[%d] is NULL", s, s);
        if (modes[s] != D3F_POOL_MEAN && modes[s] != D3F_POOL_VOTES) return fail(D3F_ERR_INVALID_ARG, "volume_pool: set %d: unknown mode %d", s, modes[s]);
    }
    if (member_capacity < 0) return fail(D3F_ERR_INVALID_ARG, "volume_pool: member_capacity=%lld is negative", (long long)member_capacity);
    if (const int rc = check_extents("volume_pool", nx, ny, nz)) return rc;
    if (!pool_shape_ok(nx, ny, nz, K)) return fail(D3F_ERR_BAD_SHAPE, "volume_pool: K=%d exceeds the %lld voxels", K, (long long)nx * ny * nz);
    int64_t mean_channels = 0;
    for (int s = 0; s < n_sets; ++s) {
        if (const int rc = check_set_shape("volume_pool", s, sets[s])) return rc;
        if (const int rc = check_set_storage("volume_pool", s, sets[s], false)) return rc;
        if (modes[s] == D3F_POOL_VOTES && sets[s].C > D3F_POOL_MAX_VOTE_CHANNELS)
            return fail(D3F_ERR_BAD_SHAPE, "volume_pool: set %d: votes over C=%d channels, more than %d", s, sets[s].C, D3F_POOL_MAX_VOTE_CHANNELS);
        if (modes[s] == D3F_POOL_MEAN) mean_channels += sets[s].C;
    }
    if (!aligned(label, 4) || !aligned(slot, 4) || !aligned(out_members, 8) || !aligned(out_count, 4) || !aligned(out_moments, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_pool: label / slot / out_members / out_count / out_moments must be aligned to their element size");
    for (int s = 0; s < n_sets; ++s) {
        if (const int rc = check_set_layout("volume_pool", s, sets[s])) return rc;
        if (!aligned(sets[s].fill, 4) || !aligned(out_rows[s], 4))
            return fail(D3F_ERR_BAD_LAYOUT, "volume_pool: set %d: fill / out_rows must be 4-byte aligned", s);
    }
    if (const int rc = check_workspace("volume_pool", workspace, workspace_bytes, d3f_volume_pool_workspace_bytes(nx, ny, nz, K, member_capacity, mean_channels), 8)) return rc;
    hipError_t e;
    if (K == 0) {
        e = d3f::launch_pool_nothing(out_members, static_cast<hipStream_t>(stream));
    } else {
        d3f::PoolArgs A;
        A.label = label;
        A.nx = nx; A.ny = ny; A.nz = nz; A.K = K;
        A.valid = valid;
        A.slot = slot;
        A.sets = sets;
        A.n_sets = n_sets;
        A.modes = modes;
        A.member_capacity = member_capacity;
        A.out_members = out_members;
        A.out_count = out_count;
        A.out_moments = out_moments;
        A.out_rows = out_rows;
        A.workspace = workspace;
        e = d3f::launch_volume_pool(A, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_pool launch");
}

// ---- one rigid motion per part from dense correspondences (motion_kernels.hip) ----
int64_t d3f_part_motion_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t K, int64_t member_capacity)
{
    if (K < 0 || member_capacity < 0 || !pool_shape_ok(nx, ny, nz, K)) return 0;
    return d3f::motion_workspace_bytes((int64_t)nx * ny * nz, K, member_capacity);
}

int d3f_part_motion(const int32_t *label, int32_t K, int32_t nx, int32_t ny, int32_t nz, const uint8_t *keep, const int32_t *target, const double *offset,
                    const int32_t *ref, int32_t fits, double tau2, int32_t min_pairs, int64_t member_capacity, int64_t *out_members, int32_t *out_pairs,
                    double *out_pose, int32_t *out_inliers, double *out_rmse, int32_t *out_status, int32_t *out_fits, double *out_residual2, uint8_t *out_inlier,
                    double *out_sums, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!label || !target) return fail(D3F_ERR_INVALID_ARG, "part_motion: label or target is NULL");
    if (!out_members || !out_pairs || !out_pose || !out_inliers || !out_rmse || !out_status || !out_fits)
        return fail(D3F_ERR_INVALID_ARG, "part_motion: out_members, out_pairs, out_pose, out_inliers, out_rmse, out_status or out_fits is NULL");
    if (K < 0) return fail(D3F_ERR_INVALID_ARG, "part_motion: K=%d is negative", K);
    if (fits < 1 || fits > D3F_MOTION_MAX_FITS) return fail(D3F_ERR_INVALID_ARG, "part_motion: fits=%d outside [1,%d]", fits, D3F_MOTION_MAX_FITS);
    if (!(tau2 > 0.0 && tau2 < __builtin_huge_val())) return fail(D3F_ERR_INVALID_ARG, "part_motion: tau2=%g, the squared inlier radius must be finite and > 0", tau2);
    if (min_pairs < 3) return fail(D3F_ERR_INVALID_ARG, "part_motion: min_pairs=%d, a rigid motion needs at least 3 pairs", min_pairs);
    if (member_capacity < 0) return fail(D3F_ERR_INVALID_ARG, "part_motion: member_capacity=%lld is negative", (long long)member_capacity);
    if (const int rc = check_extents("part_motion", nx, ny, nz)) return rc;
    if (!pool_shape_ok(nx, ny, nz, K)) return fail(D3F_ERR_BAD_SHAPE, "part_motion: K=%d exceeds the %lld voxels", K, (long long)nx * ny * nz);
    if (!aligned(label, 4) || !aligned(target, 4) || !aligned(offset, 8) || !aligned(ref, 4) || !aligned(out_members, 8) || !aligned(out_pairs, 4) ||
        !aligned(out_pose, 8) || !aligned(out_inliers, 4) || !aligned(out_rmse, 8) || !aligned(out_status, 4) || !aligned(out_fits, 4) ||
        !aligned(out_residual2, 8) || !aligned(out_sums, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "part_motion: every pointer must be aligned to its element size");
    if (const int rc = check_workspace("part_motion", workspace, workspace_bytes, d3f_part_motion_workspace_bytes(nx, ny, nz, K, member_capacity), 8)) return rc;
    hipError_t e;
    if (K == 0) {
        e = d3f::launch_pool_nothing(out_members, static_cast<hipStream_t>(stream));
    } else {
        d3f::MotionArgs A;
        A.label = label;
        A.K = K; A.nx = nx; A.ny = ny; A.nz = nz;
        A.keep = keep;
        A.target = target;
        A.offset = offset;
        A.ref = ref;
        A.fits = fits;
        A.min_pairs = min_pairs;
        A.tau2 = tau2;
        A.member_capacity = member_capacity;
        A.out_members = out_members;
        A.out_pairs = out_pairs;
        A.out_pose = out_pose;
        A.out_inliers = out_inliers;
        A.out_rmse = out_rmse;
        A.out_status = out_status;
        A.out_fits = out_fits;
        A.out_residual2 = out_residual2;
        A.out_inlier = out_inlier;
        A.out_sums = out_sums;
        A.workspace = workspace;
        e = d3f::launch_part_motion(A, static_cast<hipStream_t>(stream));
    }
    return e == hipSuccess ? D3F_OK : hip_fail(e, "part_motion launch");
}

// ---- a baked field moved by the rigid motions of its parts (warp_kernels.hip) ----
// the parts of both calls: K, then the pose rows
static int check_warp_parts(const char *who, int32_t K)
{
    if (K < 0) return fail(D3F_ERR_INVALID_ARG, "%s: K=%d is negative", who, K);
    if (K > D3F_WARP_MAX_PARTS) return fail(D3F_ERR_BAD_SHAPE, "%s: K=%d exceeds D3F_WARP_MAX_PARTS=%d", who, K, D3F_WARP_MAX_PARTS);
    return D3F_OK;
}

int d3f_volume_warp_select(const d3f_warp_select *args, void *stream)
{
    const char *who = "volume_warp_select";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    const d3f_volume *vol = &args->vol;
    if (const int rc = check_volume(who, vol)) return rc;
    if (const int rc = check_warp_parts(who, args->K)) return rc;
    if (!vol->dist || !vol->valid || !vol->cell_valid || !args->owner) return fail(D3F_ERR_INVALID_ARG, "%s: vol.dist / vol.valid / vol.cell_valid / owner must be non-NULL", who);
    if (args->K > 0 && (!args->pose || !args->out_boxes)) return fail(D3F_ERR_INVALID_ARG, "%s: pose / out_boxes must be non-NULL with K=%d", who, args->K);
    if (!args->out_source || !args->out_dist || !args->out_valid) return fail(D3F_ERR_INVALID_ARG, "%s: out_source / out_dist / out_valid must be non-NULL", who);
    if (!aligned(vol->dist, 4) || !aligned(args->owner, 4) || !aligned(args->pose, 8) || !aligned(args->out_source, 4) || !aligned(args->out_dist, 4) ||
        !aligned(args->out_boxes, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: vol.dist / owner / pose / out_source / out_dist / out_boxes must be aligned to their element size", who);
    d3f::WarpSelectArgs A;
    A.dist = vol->dist;
    A.valid = vol->valid;
    A.cell_valid = vol->cell_valid;
    A.owner = args->owner;
    A.pose = args->pose;
    A.nx = vol->nx; A.ny = vol->ny; A.nz = vol->nz; A.K = args->K;
    A.out_source = args->out_source;
    A.out_dist = args->out_dist;
    A.out_valid = args->out_valid;
    A.out_boxes = args->out_boxes;
    hipError_t e = d3f::launch_warp_select(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_warp_select launch");
}

int d3f_volume_warp_rows(const d3f_warp_rows *args, void *stream)
{
    const char *who = "volume_warp_rows";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    const d3f_volume *vol = &args->vol;
    const d3f_band *band = args->band;
    if (const int rc = check_volume(who, vol)) return rc;
    if (band && (band->n_rows < 0 || band->n_rows > 0x7fffffffLL))
        return fail(D3F_ERR_BAD_SHAPE, "%s: band->n_rows=%lld outside [0, 2^31 - 1]", who, (long long)band->n_rows);
    if (const int rc = check_warp_parts(who, args->K)) return rc;
    const int64_t n = (int64_t)vol->nx * vol->ny * vol->nz;
    if (args->m < 0) return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld is negative", who, (long long)args->m);
    if (!args->voxels && args->m != n) return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld with voxels NULL, must be the voxel count %lld", who, (long long)args->m, (long long)n);
    const int32_t n_sets = args->n_sets;
    if (n_sets < 0 || n_sets > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_sets=%d outside [0,%d]", who, n_sets, D3F_MAX_MAPS);
    if (n_sets > 0 && !args->sets) return fail(D3F_ERR_INVALID_ARG, "%s: sets is NULL with n_sets=%d", who, n_sets);
    for (int s = 0; s < n_sets; ++s) {
        if (const int rc = check_set_shape(who, s, args->sets[s])) return rc;
        if (const int rc = check_set_storage(who, s, args->sets[s], false)) return rc;
    }
    if (args->m == 0) return D3F_OK;
    const bool empty = band && band->n_rows == 0;
    if (!args->source || !args->out_known || (args->K > 0 && !args->pose) || (n_sets > 0 && !args->out_sets))
        return fail(D3F_ERR_INVALID_ARG, "%s: source / out_known / pose (with K > 0) / out_sets must be non-NULL", who);
    if (band && !empty && (!band->slot || !band->cell_band)) return fail(D3F_ERR_INVALID_ARG, "%s: band->slot / band->cell_band must be non-NULL with n_rows > 0", who);
    if (!aligned(args->source, 4) || !aligned(args->pose, 8) || !aligned(args->voxels, 4) || (band && !empty && !aligned(band->slot, 4)))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: source / pose / voxels / band->slot must be aligned to their element size", who);
    d3f::WarpRowsArgs A;
    for (int s = 0; s < n_sets; ++s) {
        const d3f_volume_set &set = args->sets[s];
        if (!set.data && !empty) return fail(D3F_ERR_INVALID_ARG, "%s: set %d: data is NULL", who, s);
        if (const int rc = check_set_layout(who, s, set)) return rc;
        if (!aligned(set.fill, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: fill must be 4-byte aligned", who, s);
        if (!args->out_sets[s]) return fail(D3F_ERR_INVALID_ARG, "%s: out_sets[%d] is NULL", who, s);
        if (!aligned(args->out_sets[s], 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: out_sets[%d] must be 4-byte aligned", who, s);
        d3f::VolSet &S = A.sets[s];
        S.data = set.data;
        S.fill = set.fill;
        S.out = static_cast<float *>(args->out_sets[s]);
        S.grad = nullptr;
        S.stride = set.stride_voxel;
        S.C = set.C;
        S.vec = set_reads_vectors(set) && aligned(args->out_sets[s], 16) ? 1 : 0;
        S.f16 = 0;
    }
    A.source = args->source;
    A.pose = args->pose;
    A.voxels = args->voxels;
    A.m = args->m;
    A.nx = vol->nx; A.ny = vol->ny; A.nz = vol->nz; A.K = args->K;
    A.banded = band != nullptr;
    A.slot = band && !empty ? band->slot : nullptr;
    A.cell_band = band && !empty ? band->cell_band : nullptr;
    A.n_sets = n_sets;
    A.out_known = args->out_known;
    hipError_t e = d3f::launch_warp_rows(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_warp_rows launch");
}

// ---- two baked fields on one grid merged into one (merge_kernels.hip; declared by include/d3fields_hip_ext.h) ----
// the grid of both calls: the extents of a d3f_volume
static int check_merge_grid(const char *who, int32_t nx, int32_t ny, int32_t nz)
{
    d3f_volume vol = {};
    vol.nx = nx; vol.ny = ny; vol.nz = nz;
    return check_volume(who, &vol);
}

// in (0, +inf]
static bool positive_or_inf(float x) { return x > 0.0f; }

int d3f_volume_merge_select(const d3f_merge_select *args, void *stream)
{
    const char *who = "volume_merge_select";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    if (const int rc = check_merge_grid(who, args->nx, args->ny, args->nz)) return rc;
    if (args->reserved != 0) return fail(D3F_ERR_INVALID_ARG, "%s: reserved=%d, must be 0", who, args->reserved);
    if (!args->weight_a && !positive_finite(args->weight_a_all))
        return fail(D3F_ERR_INVALID_ARG, "%s: weight_a_all=%g must be > 0 and finite where weight_a is NULL", who, (double)args->weight_a_all);
    if (!args->weight_b && !positive_finite(args->weight_b_all))
        return fail(D3F_ERR_INVALID_ARG, "%s: weight_b_all=%g must be > 0 and finite where weight_b is NULL", who, (double)args->weight_b_all);
    if (!positive_or_inf(args->w_max)) return fail(D3F_ERR_INVALID_ARG, "%s: w_max=%g must be in (0, +inf]", who, (double)args->w_max);
    if (!(args->gap >= 0.0f)) return fail(D3F_ERR_INVALID_ARG, "%s: gap=%g must be in [0, +inf]", who, (double)args->gap);
    if (!args->dist_a || !args->valid_a || !args->dist_b || !args->valid_b)
        return fail(D3F_ERR_INVALID_ARG, "%s: dist_a / valid_a / dist_b / valid_b must be non-NULL", who);
    if (!args->out_dist || !args->out_weight || !args->out_beta || !args->out_valid || !args->out_kind)
        return fail(D3F_ERR_INVALID_ARG, "%s: out_dist / out_weight / out_beta / out_valid / out_kind must be non-NULL", who);
    if (!aligned(args->dist_a, 4) || !aligned(args->weight_a, 4) || !aligned(args->dist_b, 4) || !aligned(args->weight_b, 4) || !aligned(args->out_dist, 4) ||
        !aligned(args->out_weight, 4) || !aligned(args->out_beta, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: dist_a / weight_a / dist_b / weight_b / out_dist / out_weight / out_beta must be aligned to their element size", who);
    d3f::MergeSelectArgs A;
    A.dist_a = args->dist_a; A.weight_a = args->weight_a; A.valid_a = args->valid_a;
    A.dist_b = args->dist_b; A.weight_b = args->weight_b; A.valid_b = args->valid_b;
    A.wa = args->weight_a_all; A.wb = args->weight_b_all;
    A.w_max = args->w_max; A.gap = args->gap;
    A.n = (int64_t)args->nx * args->ny * args->nz;
    A.out_dist = args->out_dist; A.out_weight = args->out_weight; A.out_beta = args->out_beta;
    A.out_valid = args->out_valid; A.out_kind = args->out_kind;
    hipError_t e = d3f::launch_merge_select(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_merge_select launch");
}

int d3f_volume_merge_rows(const d3f_merge_rows *args, void *stream)
{
    const char *who = "volume_merge_rows";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    if (const int rc = check_merge_grid(who, args->nx, args->ny, args->nz)) return rc;
    const d3f_band *bands[2] = {args->band_a, args->band_b};
    for (int side = 0; side < 2; ++side)
        if (bands[side] && (bands[side]->n_rows < 0 || bands[side]->n_rows > 0x7fffffffLL))
            return fail(D3F_ERR_BAD_SHAPE, "%s: band_%c->n_rows=%lld outside [0, 2^31 - 1]", who, 'a' + side, (long long)bands[side]->n_rows);
    const int32_t n_sets = args->n_sets;
    if (n_sets < 0 || n_sets > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_sets=%d outside [0,%d]", who, n_sets, D3F_MAX_MAPS);
    if (n_sets > 0 && (!args->sets_a || !args->sets_b)) return fail(D3F_ERR_INVALID_ARG, "%s: sets_a / sets_b is NULL with n_sets=%d", who, n_sets);
    for (int s = 0; s < n_sets; ++s) {                           // (the messages count a's sets 0 .., b's n_sets ..)
        if (const int rc = check_set_shape(who, s, args->sets_a[s])) return rc;
        if (const int rc = check_set_shape(who, n_sets + s, args->sets_b[s])) return rc;
        if (args->sets_a[s].C != args->sets_b[s].C)
            return fail(D3F_ERR_BAD_SHAPE, "%s: pair %d: sets_a C=%d != sets_b C=%d", who, s, args->sets_a[s].C, args->sets_b[s].C);
        if (const int rc = check_set_storage(who, s, args->sets_a[s], true)) return rc;
        if (const int rc = check_set_storage(who, n_sets + s, args->sets_b[s], true)) return rc;
    }
    const int64_t n = (int64_t)args->nx * args->ny * args->nz;
    if (args->reserved != 0) return fail(D3F_ERR_INVALID_ARG, "%s: reserved=%lld, must be 0", who, (long long)args->reserved);
    if (args->m < 0) return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld is negative", who, (long long)args->m);
    if (!args->voxels && args->m != n) return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld with voxels NULL, must be the voxel count %lld", who, (long long)args->m, (long long)n);
    if (args->m == 0) return D3F_OK;
    const bool empty[2] = {bands[0] && bands[0]->n_rows == 0, bands[1] && bands[1]->n_rows == 0};
    if (!args->kind || !args->beta || !args->out_known || (n_sets > 0 && !args->out_sets))
        return fail(D3F_ERR_INVALID_ARG, "%s: kind / beta / out_known / out_sets must be non-NULL", who);
    for (int side = 0; side < 2; ++side)
        if (bands[side] && !empty[side] && !bands[side]->slot)
            return fail(D3F_ERR_INVALID_ARG, "%s: band_%c->slot must be non-NULL with n_rows > 0", who, 'a' + side);
    if (!aligned(args->beta, 4) || !aligned(args->voxels, 4) || (bands[0] && !empty[0] && !aligned(bands[0]->slot, 4)) ||
        (bands[1] && !empty[1] && !aligned(bands[1]->slot, 4)))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: beta / voxels / band_a->slot / band_b->slot must be aligned to their element size", who);
    d3f::MergeRowsArgs A;
    for (int s = 0; s < n_sets; ++s) {
        const d3f_volume_set &sa = args->sets_a[s], &sb = args->sets_b[s];
        if (!sa.data && !empty[0]) return fail(D3F_ERR_INVALID_ARG, "%s: set %d: data is NULL", who, s);
        if (!sb.data && !empty[1]) return fail(D3F_ERR_INVALID_ARG, "%s: set %d: data is NULL", who, n_sets + s);
        if (const int rc = check_set_layout(who, s, sa)) return rc;
        if (const int rc = check_set_layout(who, n_sets + s, sb)) return rc;
        if (!aligned(sa.fill, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: fill must be 4-byte aligned", who, s);
        if (!args->out_sets[s]) return fail(D3F_ERR_INVALID_ARG, "%s: out_sets[%d] is NULL", who, s);
        if (!aligned(args->out_sets[s], 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: out_sets[%d] must be 4-byte aligned", who, s);
        d3f::MergeSet &S = A.sets[s];
        S.a = sa.data;
        S.b = sb.data;
        S.fill = sa.fill;
        S.out = static_cast<float *>(args->out_sets[s]);
        S.stride_a = sa.stride_voxel;
        S.stride_b = sb.stride_voxel;
        S.C = sa.C;
        S.vec = set_reads_vectors(sa) && set_reads_vectors(sb) && aligned(args->out_sets[s], 16) ? 1 : 0;
        S.f16_a = set_is_half(sa) ? 1 : 0;
        S.f16_b = set_is_half(sb) ? 1 : 0;
    }
    A.kind = args->kind;
    A.beta = args->beta;
    A.voxels = args->voxels;
    A.m = args->m;
    A.n = n;
    A.banded_a = bands[0] != nullptr;
    A.banded_b = bands[1] != nullptr;
    A.slot_a = bands[0] && !empty[0] ? bands[0]->slot : nullptr;
    A.slot_b = bands[1] && !empty[1] ? bands[1]->slot : nullptr;
    A.n_sets = n_sets;
    A.out_known = args->out_known;
    hipError_t e = d3f::launch_merge_rows(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_merge_rows launch");
}

// ---- a baked field at half the resolution (pyramid_kernels.hip; declared by include/d3fields_hip_pyramid.h) ----
int d3f_volume_coarsen_select(const d3f_coarsen_select *args, void *stream)
{
    const char *who = "volume_coarsen_select";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    if (const int rc = check_extents(who, args->nx, args->ny, args->nz)) return rc;
    if (args->min_children < 1 || args->min_children > 8) return fail(D3F_ERR_INVALID_ARG, "%s: min_children=%d outside [1,8]", who, args->min_children);
    if (args->reserved != 0) return fail(D3F_ERR_INVALID_ARG, "%s: reserved=%lld, must be 0", who, (long long)args->reserved);
    if (!args->dist || !args->valid) return fail(D3F_ERR_INVALID_ARG, "%s: dist / valid must be non-NULL", who);
    if (!args->out_dist || !args->out_valid || !args->out_children) return fail(D3F_ERR_INVALID_ARG, "%s: out_dist / out_valid / out_children must be non-NULL", who);
    if (!aligned(args->dist, 4) || !aligned(args->out_dist, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: dist / out_dist must be aligned to their element size", who);
    d3f::CoarsenSelectArgs A;
    A.dist = args->dist;
    A.valid = args->valid;
    A.nx = args->nx; A.ny = args->ny; A.nz = args->nz;
    A.cy = (args->ny + 1) / 2;
    A.cz = (args->nz + 1) / 2;
    A.min_children = args->min_children;
    A.nc = (int64_t)((args->nx + 1) / 2) * A.cy * A.cz;
    A.out_dist = args->out_dist;
    A.out_valid = args->out_valid;
    A.out_children = args->out_children;
    hipError_t e = d3f::launch_coarsen_select(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_coarsen_select launch");
}

int d3f_volume_coarsen_rows(const d3f_coarsen_rows *args, void *stream)
{
    const char *who = "volume_coarsen_rows";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    if (const int rc = check_extents(who, args->nx, args->ny, args->nz)) return rc;
    const d3f_band *band = args->band;
    if (band && (band->n_rows < 0 || band->n_rows > 0x7fffffffLL))
        return fail(D3F_ERR_BAD_SHAPE, "%s: band->n_rows=%lld outside [0, 2^31 - 1]", who, (long long)band->n_rows);
    const int32_t n_sets = args->n_sets;
    if (n_sets < 0 || n_sets > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_sets=%d outside [0,%d]", who, n_sets, D3F_MAX_MAPS);
    if (n_sets > 0 && !args->sets) return fail(D3F_ERR_INVALID_ARG, "%s: sets is NULL with n_sets=%d", who, n_sets);
    for (int s = 0; s < n_sets; ++s) {
        if (const int rc = check_set_shape(who, s, args->sets[s])) return rc;
        if (const int rc = check_set_storage(who, s, args->sets[s], true)) return rc;
    }
    const int32_t cy = (args->ny + 1) / 2, cz = (args->nz + 1) / 2;
    const int64_t nc = (int64_t)((args->nx + 1) / 2) * cy * cz;
    if (args->reserved != 0) return fail(D3F_ERR_INVALID_ARG, "%s: reserved=%lld, must be 0", who, (long long)args->reserved);
    if (args->m < 0) return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld is negative", who, (long long)args->m);
    if (!args->voxels && args->m != nc)
        return fail(D3F_ERR_INVALID_ARG, "%s: m=%lld with voxels NULL, must be the coarse voxel count %lld", who, (long long)args->m, (long long)nc);
    if (args->m == 0) return D3F_OK;
    const bool empty = band && band->n_rows == 0;
    if (!args->children || !args->out_known || (n_sets > 0 && !args->out_sets)) return fail(D3F_ERR_INVALID_ARG, "%s: children / out_known / out_sets must be non-NULL", who);
    if (band && !empty && !band->slot) return fail(D3F_ERR_INVALID_ARG, "%s: band->slot must be non-NULL with n_rows > 0", who);
    if (!aligned(args->voxels, 4) || (band && !empty && !aligned(band->slot, 4)))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: voxels / band->slot must be aligned to their element size", who);
    d3f::CoarsenRowsArgs A;
    for (int s = 0; s < n_sets; ++s) {
        const d3f_volume_set &set = args->sets[s];
        if (!set.data && !empty) return fail(D3F_ERR_INVALID_ARG, "%s: set %d: data is NULL", who, s);
        if (const int rc = check_set_layout(who, s, set)) return rc;
        if (!aligned(set.fill, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: set %d: fill must be 4-byte aligned", who, s);
        if (!args->out_sets[s]) return fail(D3F_ERR_INVALID_ARG, "%s: out_sets[%d] is NULL", who, s);
        if (!aligned(args->out_sets[s], 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: out_sets[%d] must be 4-byte aligned", who, s);
        d3f::CoarsenSet &S = A.sets[s];
        S.data = set.data;
        S.fill = set.fill;
        S.out = static_cast<float *>(args->out_sets[s]);
        S.stride = set.stride_voxel;
        S.C = set.C;
        S.vec = set_reads_vectors(set) && aligned(args->out_sets[s], 16) ? 1 : 0;
        S.f16 = set_is_half(set) ? 1 : 0;
    }
    A.children = args->children;
    A.voxels = args->voxels;
    A.slot = band && !empty ? band->slot : nullptr;
    A.banded = band != nullptr;
    A.m = args->m;
    A.nc = nc;
    A.nx = args->nx; A.ny = args->ny; A.nz = args->nz; A.cy = cy; A.cz = cz;
    A.n_sets = n_sets;
    A.out_known = args->out_known;
    hipError_t e = d3f::launch_coarsen_rows(A, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_coarsen_rows launch");
}

// ---- the flow with a per-voxel seed (flow_seeded_kernels.hip; declared by include/d3fields_hip_pyramid.h): d3f_volume_flow's checks in its order ----
int d3f_volume_flow_seeded(const d3f_flow_seeded *args, void *stream)
{
    const char *who = "volume_flow_seeded";
    if (!args) return fail(D3F_ERR_INVALID_ARG, "%s: args is NULL", who);
    const d3f_volume_set *set_a = args->set_a, *set_b = args->set_b;
    if (!args->site_a || !args->site_b || !set_a || !set_b) return fail(D3F_ERR_INVALID_ARG, "%s: site_a, site_b, set_a or set_b is NULL", who);
    if (!set_a->data || !set_b->data) return fail(D3F_ERR_INVALID_ARG, "%s: set_a->data or set_b->data is NULL", who);
    if (!args->out_target || !args->out_cost) return fail(D3F_ERR_INVALID_ARG, "%s: out_target or out_cost is NULL", who);
    if (args->radius < 1 || args->radius > D3F_FLOW_MAX_RADIUS) return fail(D3F_ERR_INVALID_ARG, "%s: radius=%d outside [1,%d]", who, args->radius, D3F_FLOW_MAX_RADIUS);
    if (args->max_cost2 != args->max_cost2) return fail(D3F_ERR_INVALID_ARG, "%s: max_cost2 is NaN (+Inf means no threshold)", who);
    if (args->reserved != 0) return fail(D3F_ERR_INVALID_ARG, "%s: reserved=%d, must be 0", who, args->reserved);
    if (const int rc = check_extents(who, args->nx, args->ny, args->nz)) return rc;
    if (const int rc = check_set_shape(who, 0, *set_a)) return rc;             // set 0: set_a, set 1: set_b
    if (set_b->C != set_a->C) return fail(D3F_ERR_BAD_SHAPE, "%s: C=%d of set_a, C=%d of set_b: the sets must have the same width", who, set_a->C, set_b->C);
    if (const int rc = check_set_storage(who, 0, *set_a, false)) return rc;
    if (const int rc = check_set_storage(who, 1, *set_b, false)) return rc;
    if (const int rc = check_set_layout(who, 0, *set_a)) return rc;
    if (const int rc = check_set_layout(who, 1, *set_b)) return rc;
    if (!aligned(args->slot_a, 4) || !aligned(args->slot_b, 4) || !aligned(args->seed, 4) || !aligned(args->out_target, 4) || !aligned(args->out_cost, 4) ||
        !aligned(args->out_axis_cost, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: slots, seed and outputs must be 4-byte aligned", who);
    d3f::FlowSeededArgs A;
    A.site_a = args->site_a; A.site_b = args->site_b;
    A.slot_a = args->slot_a; A.slot_b = args->slot_b;
    A.data_a = static_cast<const float *>(set_a->data); A.data_b = static_cast<const float *>(set_b->data);
    A.stride_a = set_a->stride_voxel; A.stride_b = set_b->stride_voxel;
    A.seed = args->seed;
    A.target = args->out_target;
    A.cost = args->out_cost;
    A.nx = args->nx; A.ny = args->ny; A.nz = args->nz;
    A.C = set_a->C;
    A.r = args->radius;
    A.vec = set_reads_vectors(*set_a) && set_reads_vectors(*set_b) ? 1 : 0;
    A.max_cost2 = args->max_cost2;
    hipError_t e = d3f::launch_flow_seeded(A, static_cast<hipStream_t>(stream));
    if (e == hipSuccess && args->out_axis_cost)
        e = d3f::launch_flow_axis(A.slot_a, A.data_a, A.stride_a, A.site_b, A.slot_b, A.data_b, A.stride_b, A.C, A.nx, A.ny, A.nz, A.target, args->out_axis_cost,
                                  static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_flow_seeded launch");
}

// ---- cost-to-go through free space (geodesic_kernels.hip) ----
static int check_geo_weights(const char *who, int32_t connectivity, const int32_t *w)
{
    if (const int rc = check_connectivity(who, connectivity)) return rc;
    if (!w) return fail(D3F_ERR_INVALID_ARG, "%s: w is NULL", who);
    if (!(1 <= w[0] && w[0] <= w[1] && w[1] <= w[2] && w[2] <= 255)) return fail(D3F_ERR_INVALID_ARG, "%s: weights must satisfy 1 <= w1 <= w2 <= w3 <= 255", who);
    return D3F_OK;
}

int64_t d3f_volume_geodesic_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    return edt_shape_ok(nx, ny, nz) ? d3f::geodesic_layout(nx, ny, nz).total : 0;
}

int d3f_volume_geodesic_init(const uint8_t *free, int32_t nx, int32_t ny, int32_t nz, const int32_t *seeds, int64_t n_seeds, int32_t *out_cost,
                             void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!free || !out_cost) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_init: free or out_cost is NULL");
    if (n_seeds < 0) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_init: n_seeds=%lld is negative", (long long)n_seeds);
    if (n_seeds > 0 && !seeds) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_init: seeds is NULL with n_seeds=%lld", (long long)n_seeds);
    if (const int rc = check_extents("volume_geodesic_init", nx, ny, nz)) return rc;
    if (!aligned(seeds, 4) || !aligned(out_cost, 4)) return fail(D3F_ERR_BAD_LAYOUT, "volume_geodesic_init: seeds / out_cost must be 4-byte aligned");
    if (const int rc = check_workspace("volume_geodesic_init", workspace, workspace_bytes, d3f_volume_geodesic_workspace_bytes(nx, ny, nz), 4)) return rc;
    hipError_t e = d3f::launch_geodesic_init(free, nx, ny, nz, seeds, n_seeds, out_cost, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_geodesic_init launch");
}

int d3f_volume_geodesic_relax(const uint8_t *free, const int32_t *penalty, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, const int32_t *w,
                              int32_t max_cost, int32_t rounds, int32_t *cost, int32_t *out_pending, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!free || !cost || !out_pending) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_relax: free, cost or out_pending is NULL");
    if (const int rc = check_geo_weights("volume_geodesic_relax", connectivity, w)) return rc;
    if (max_cost < 1 || max_cost > 0x7ffffffe) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_relax: max_cost=%d outside [1, INT32_MAX - 1]", max_cost);
    if (rounds < 1) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_relax: rounds=%d, must be >= 1", rounds);
    if (const int rc = check_extents("volume_geodesic_relax", nx, ny, nz)) return rc;
    if (!aligned(penalty, 4) || !aligned(cost, 4) || !aligned(out_pending, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_geodesic_relax: penalty / cost / out_pending must be 4-byte aligned");
    if (const int rc = check_workspace("volume_geodesic_relax", workspace, workspace_bytes, d3f_volume_geodesic_workspace_bytes(nx, ny, nz), 4)) return rc;
    hipError_t e = d3f::launch_geodesic_relax(free, penalty, nx, ny, nz, connectivity, w, max_cost, rounds, cost, out_pending, workspace,
                                              static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_geodesic_relax launch");
}

int d3f_volume_geodesic_finish(const uint8_t *free, const int32_t *penalty, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, const int32_t *w,
                               float step, const int32_t *cost, int32_t *out_next, float *out_dist, void *stream)
{
    if (!free || !cost) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_finish: free or cost is NULL");
    if (!out_next && !out_dist) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_finish: out_next and out_dist are both NULL");
    if (const int rc = check_geo_weights("volume_geodesic_finish", connectivity, w)) return rc;
    if (out_dist && !positive_finite(step)) return fail(D3F_ERR_INVALID_ARG, "volume_geodesic_finish: step must be > 0 and finite with out_dist");
    if (const int rc = check_extents("volume_geodesic_finish", nx, ny, nz)) return rc;
    if (!aligned(penalty, 4) || !aligned(cost, 4) || !aligned(out_next, 4) || !aligned(out_dist, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_geodesic_finish: penalty / cost / out_next / out_dist must be 4-byte aligned");
    hipError_t e = d3f::launch_geodesic_finish(free, penalty, nx, ny, nz, connectivity, w, step, cost, out_next, out_dist, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_geodesic_finish launch");
}

int d3f_volume_follow(const int32_t *next, int64_t n_voxels, const int32_t *starts, int64_t n, int32_t max_steps, int32_t *out_voxels, int32_t *out_length,
                      uint8_t *out_reached, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "volume_follow: n=%lld is negative", (long long)n);
    if (max_steps < 1) return fail(D3F_ERR_INVALID_ARG, "volume_follow: max_steps=%d, must be >= 1", max_steps);
    if (n > 0 && (!next || !starts || !out_voxels || !out_length || !out_reached))
        return fail(D3F_ERR_INVALID_ARG, "volume_follow: next, starts, out_voxels, out_length or out_reached is NULL with n=%lld", (long long)n);
    if (n_voxels < 1 || n_voxels > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "volume_follow: n_voxels=%lld outside [1, 2^31 - 1]", (long long)n_voxels);
    if (const int rc = check_launch_blocks("volume_follow", n, d3f::kBlock)) return rc;
    if (!aligned(next, 4) || !aligned(starts, 4) || !aligned(out_voxels, 4) || !aligned(out_length, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_follow: next / starts / out_voxels / out_length must be 4-byte aligned");
    if (n == 0) return D3F_OK;
    hipError_t e = d3f::launch_volume_follow(next, n_voxels, starts, n, max_steps, out_voxels, out_length, out_reached, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_follow launch");
}

// ---- exact grid segments and shortcuts of voxel rows (segment_kernels.hip) ----
int d3f_volume_segments(const uint8_t *free, const int32_t *value, int32_t nx, int32_t ny, int32_t nz, const int32_t *a, const int32_t *b, int64_t n,
                        uint32_t flags, uint8_t *out_clear, int32_t *out_last, int32_t *out_blocked, int32_t *out_min_value, int32_t *out_min_voxel, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "volume_segments: n=%lld is negative", (long long)n);
    if (flags & ~D3F_SEGMENT_CUT_CORNERS) return fail(D3F_ERR_INVALID_ARG, "volume_segments: unknown flag bits 0x%x", flags & ~D3F_SEGMENT_CUT_CORNERS);
    if (n > 0 && (!free || !a || !b)) return fail(D3F_ERR_INVALID_ARG, "volume_segments: free, a or b is NULL with n=%lld", (long long)n);
    if (!out_clear && !out_last && !out_blocked && !out_min_value && !out_min_voxel)
        return fail(D3F_ERR_INVALID_ARG, "volume_segments: every output is NULL");
    if (!value && (out_min_value || out_min_voxel)) return fail(D3F_ERR_INVALID_ARG, "volume_segments: out_min_value / out_min_voxel need value");
    if (const int rc = check_extents("volume_segments", nx, ny, nz)) return rc;
    if (const int rc = check_launch_blocks("volume_segments", n, d3f::kBlock)) return rc;
    if (!aligned(value, 4) || !aligned(a, 4) || !aligned(b, 4) || !aligned(out_last, 4) || !aligned(out_blocked, 4) || !aligned(out_min_value, 4) ||
        !aligned(out_min_voxel, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_segments: value / a / b / out_last / out_blocked / out_min_value / out_min_voxel must be 4-byte aligned");
    if (n == 0) return D3F_OK;
    hipError_t e = d3f::launch_volume_segments(free, value, nx, ny, nz, a, b, n, !(flags & D3F_SEGMENT_CUT_CORNERS), out_clear, out_last, out_blocked,
                                               out_min_value, out_min_voxel, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_segments launch");
}

int d3f_path_shorten(const uint8_t *free, int32_t nx, int32_t ny, int32_t nz, const int32_t *voxels, const int32_t *length, int64_t n, int32_t row_len,
                     int32_t max_span, uint32_t flags, int32_t *out_index, int32_t *out_voxels, int32_t *out_count, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "path_shorten: n=%lld is negative", (long long)n);
    if (row_len < 1) return fail(D3F_ERR_INVALID_ARG, "path_shorten: row_len=%d, must be >= 1", row_len);
    if (max_span < 1) return fail(D3F_ERR_INVALID_ARG, "path_shorten: max_span=%d, must be >= 1", max_span);
    if (flags & ~D3F_SEGMENT_CUT_CORNERS) return fail(D3F_ERR_INVALID_ARG, "path_shorten: unknown flag bits 0x%x", flags & ~D3F_SEGMENT_CUT_CORNERS);
    if (n > 0 && (!free || !voxels || !length)) return fail(D3F_ERR_INVALID_ARG, "path_shorten: free, voxels or length is NULL with n=%lld", (long long)n);
    if (!out_count) return fail(D3F_ERR_INVALID_ARG, "path_shorten: out_count is NULL");
    if (!out_index && !out_voxels) return fail(D3F_ERR_INVALID_ARG, "path_shorten: out_index and out_voxels are both NULL");
    if (const int rc = check_extents("path_shorten", nx, ny, nz)) return rc;
    if (const int rc = check_launch_blocks("path_shorten", n, 4)) return rc;            // four rows to a workgroup (segment_kernels.hip)
    if (!aligned(voxels, 4) || !aligned(length, 4) || !aligned(out_index, 4) || !aligned(out_voxels, 4) || !aligned(out_count, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "path_shorten: voxels / length / out_index / out_voxels / out_count must be 4-byte aligned");
    if (n == 0) return D3F_OK;
    hipError_t e = d3f::launch_path_shorten(free, nx, ny, nz, voxels, length, n, row_len, max_span, !(flags & D3F_SEGMENT_CUT_CORNERS), out_index, out_voxels,
                                            out_count, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "path_shorten launch");
}

// ---- exact non-maximum suppression through the slot volume (peaks_kernels.hip) ----
int d3f_volume_peaks(const int32_t *slot, const uint8_t *mask, int32_t nx, int32_t ny, int32_t nz, const float *score, int64_t M, int32_t K,
                     int64_t stride_row, int32_t radius, float threshold, float *out, int64_t out_stride, int32_t *out_count, void *workspace,
                     int64_t workspace_bytes, void *stream)
{
    (void)workspace;
    (void)workspace_bytes;
    if (K < 0 || M < 0) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: M=%lld K=%d, neither may be negative", (long long)M, K);
    if (radius < 1 || radius > D3F_PEAKS_MAX_RADIUS) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: radius=%d outside [1, %d]", radius, D3F_PEAKS_MAX_RADIUS);
    if (threshold != threshold) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: threshold is NaN (+Inf means none)");
    if (stride_row < K || out_stride < K)
        return fail(D3F_ERR_INVALID_ARG, "volume_peaks: stride_row=%lld out_stride=%lld, both must be >= K=%d", (long long)stride_row, (long long)out_stride, K);
    if (M > 0 && K > 0 && (!score || !out)) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: score or out is NULL with M=%lld K=%d", (long long)M, K);
    if (const int rc = check_extents("volume_peaks", nx, ny, nz)) return rc;
    const int64_t n_voxels = (int64_t)nx * ny * nz;
    if (!slot && M != n_voxels) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: M=%lld without slot, must equal nx*ny*nz=%lld", (long long)M, (long long)n_voxels);
    if (slot && M > n_voxels) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: M=%lld rows for %lld voxels", (long long)M, (long long)n_voxels);
    if (!aligned(slot, 4) || !aligned(score, 4) || !aligned(out, 4) || !aligned(out_count, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_peaks: slot / score / out / out_count must be 4-byte aligned");
    if (M > 0 && K > 0) {
        if (stride_row > ((int64_t)1 << 60) / M || out_stride > ((int64_t)1 << 60) / M)      // (the byte spans below stay inside 64 bits)
            return fail(D3F_ERR_BAD_SHAPE, "volume_peaks: stride_row=%lld out_stride=%lld too large for M=%lld rows", (long long)stride_row, (long long)out_stride,
                        (long long)M);
        const uintptr_t s0 = (uintptr_t)score, s1 = s0 + (uintptr_t)((M - 1) * stride_row + K) * 4;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((M - 1) * out_stride + K) * 4;
        if (s0 < o1 && o0 < s1) return fail(D3F_ERR_INVALID_ARG, "volume_peaks: out overlaps score");
    }
    const d3f::PeaksPlan plan = d3f::peaks_plan(nx, ny, nz, K, radius);
    if (plan.chunks > 65535 || plan.tiles > 0x7fffffffLL)
        return fail(D3F_ERR_BAD_SHAPE, "volume_peaks: K=%d columns are %lld chunks, too large for one launch (65535)", K, (long long)plan.chunks);
    if (K == 0) return D3F_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (out_count) {
        hipError_t e = hipMemsetAsync(out_count, 0, (size_t)K * sizeof(int32_t), s);
        if (e != hipSuccess) return hip_fail(e, "volume_peaks memset");
    }
    if (M == 0) return D3F_OK;
    hipError_t e = d3f::launch_volume_peaks(slot, mask, nx, ny, nz, score, K, stride_row, radius, threshold, out, out_stride, out_count, s);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_peaks launch");
}

// ---- rigid alignment of point sets to the baked field (align_kernels.hip) ----
static bool align_counts_ok(int64_t I, int64_t n) { return I >= 0 && n >= 0; }

int64_t d3f_volume_align_workspace_bytes(int64_t I, int64_t n)
{
    if (I <= 0 || n <= 0) return 0;
    const int64_t chunks = d3f::align_chunks(n);
    if (chunks > 0x7fffffffLL / I) return 0;
    return d3f::align_layout(I, n).total;
}

int d3f_volume_align_centroid(const float *points, const float *weights, int64_t I, int64_t n, float *centroids_out, void *stream)
{
    if (!align_counts_ok(I, n)) return fail(D3F_ERR_INVALID_ARG, "volume_align_centroid: I=%lld n=%lld, a count is negative", (long long)I, (long long)n);
    if (I > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "volume_align_centroid: I=%lld is too large for one launch", (long long)I);
    if (I == 0) return D3F_OK;
    if (!centroids_out || (n > 0 && !points)) return fail(D3F_ERR_INVALID_ARG, "volume_align_centroid: points / centroids_out is NULL");
    if (!aligned(points, 4) || !aligned(weights, 4) || !aligned(centroids_out, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_align_centroid: points / weights / centroids_out must be 4-byte aligned");
    hipError_t e = d3f::launch_align_centroid(points, weights, I, n, centroids_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_align_centroid launch");
}

int d3f_volume_align_accumulate(const d3f_volume *vol, const d3f_band *band, const d3f_volume_set *set, const float *points, const float *weights,
                                const float *targets, const float *dist_targets, const float *pose, const float *centroids, const int32_t *skip,
                                int64_t I, int64_t n, float dist_weight, float feat_weight, float outside, double *out, void *workspace,
                                int64_t workspace_bytes, void *stream)
{
    const char *who = "volume_align_accumulate";
    if (!align_counts_ok(I, n)) return fail(D3F_ERR_INVALID_ARG, "%s: I=%lld n=%lld, a count is negative", who, (long long)I, (long long)n);
    if (!finite_nonneg(dist_weight) || !finite_nonneg(feat_weight) || !finite_nonneg(outside))
        return fail(D3F_ERR_INVALID_ARG, "%s: dist_weight / feat_weight / outside must be finite and not negative", who);
    if (band && (band->n_rows < 0 || band->n_rows > 0x7fffffffLL))
        return fail(D3F_ERR_BAD_SHAPE, "%s: band->n_rows=%lld outside [0, 2^31 - 1]", who, (long long)band->n_rows);
    const bool empty_band = band && band->n_rows == 0;
    d3f::AlignParams A;
    // (volume_common answers n == 0 with "nothing to do": the instances only scale the count)
    const int rc = volume_common(who, vol, points, I == 0 ? 0 : n, set, set ? 1 : 0, A.V, empty_band, false);      // (float32 rows only)
    if (rc != D3F_OK) return rc == 1 ? D3F_OK : rc;
    const int64_t chunks = d3f::align_chunks(n);
    if (chunks > 0x7fffffffLL / I) return fail(D3F_ERR_BAD_SHAPE, "%s: I=%lld instances of %lld workgroups are too many for one launch", who, (long long)I, (long long)chunks);
    if (!pose || !centroids || !workspace || (set && !targets)) return fail(D3F_ERR_INVALID_ARG, "%s: pose / centroids / workspace (and targets with a set) must be non-NULL", who);
    if (band && !empty_band && (!band->slot || !band->cell_band)) return fail(D3F_ERR_INVALID_ARG, "%s: band->slot / band->cell_band must be non-NULL with n_rows > 0", who);
    if (!aligned(weights, 4) || !aligned(targets, 4) || !aligned(dist_targets, 4) || !aligned(pose, 4) || !aligned(centroids, 4) || !aligned(skip, 4) ||
        (band && !aligned(band->slot, 4)))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: float and int32 arrays must be 4-byte aligned", who);
    if (!aligned(out, 8) || !aligned(workspace, 8)) return fail(D3F_ERR_BAD_LAYOUT, "%s: out / workspace must be 8-byte aligned", who);
    if (workspace_bytes < d3f_volume_align_workspace_bytes(I, n))
        return fail(D3F_ERR_WORKSPACE, "%s: needs %lld workspace bytes", who, (long long)d3f_volume_align_workspace_bytes(I, n));
    if (set && !aligned(targets, 16)) A.V.sets[0].vec = 0;
    A.slot = (band && !empty_band) ? band->slot : nullptr;
    A.cell_band = (band && !empty_band) ? band->cell_band : nullptr;
    A.banded = band ? 1 : 0;
    A.I = (int32_t)I;
    A.weights = weights;
    A.targets = targets;
    A.dist_targets = dist_targets;
    A.pose = pose;
    A.centroid = centroids;
    A.skip = skip;
    A.wd = dist_weight;
    A.wf = feat_weight;
    A.outside = outside;
    A.chunks = chunks;
    A.partial = static_cast<double *>(d3f::ws_at(workspace, d3f::align_layout(I, n).partial));
    hipError_t e = d3f::launch_align_accumulate(A, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_align_accumulate launch");
}

int d3f_volume_align_step(double *state, const void *workspace, int64_t workspace_bytes, int64_t I, int64_t n, double *out, int32_t it, int32_t iters,
                          double rot_tol, double trans_tol, float *pose_out, int32_t *skip_out, double *history, void *stream)
{
    const char *who = "volume_align_step";
    if (!align_counts_ok(I, n)) return fail(D3F_ERR_INVALID_ARG, "%s: I=%lld n=%lld, a count is negative", who, (long long)I, (long long)n);
    if (iters < 0 || it < 0 || it > iters) return fail(D3F_ERR_INVALID_ARG, "%s: it=%d outside [0, iters=%d]", who, it, iters);
    if (!finite_nonneg(rot_tol) || !finite_nonneg(trans_tol)) return fail(D3F_ERR_INVALID_ARG, "%s: rot_tol / trans_tol must be finite and not negative", who);
    if (I == 0 || n == 0) return D3F_OK;
    const int64_t chunks = d3f::align_chunks(n);
    if (chunks > 0x7fffffffLL / I) return fail(D3F_ERR_BAD_SHAPE, "%s: I=%lld instances of %lld workgroups are too many for one launch", who, (long long)I, (long long)chunks);
    if (!state || !workspace || !out || !pose_out || !skip_out || !history)
        return fail(D3F_ERR_INVALID_ARG, "%s: state / workspace / out / pose_out / skip_out / history must be non-NULL", who);
    if (!aligned(state, 8) || !aligned(workspace, 8) || !aligned(out, 8) || !aligned(history, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: state / workspace / out / history must be 8-byte aligned", who);
    if (!aligned(pose_out, 4) || !aligned(skip_out, 4)) return fail(D3F_ERR_BAD_LAYOUT, "%s: pose_out / skip_out must be 4-byte aligned", who);
    if (workspace_bytes < d3f_volume_align_workspace_bytes(I, n))
        return fail(D3F_ERR_WORKSPACE, "%s: needs %lld workspace bytes", who, (long long)d3f_volume_align_workspace_bytes(I, n));
    d3f::AlignStep S;
    S.state = state;
    S.partial = static_cast<const double *>(d3f::ws_at(const_cast<void *>(workspace), d3f::align_layout(I, n).partial));
    S.chunks = chunks;
    S.out = out;
    S.it = it;
    S.iters = iters;
    S.rot_tol = rot_tol;
    S.trans_tol = trans_tol;
    S.pose_out = pose_out;
    S.skip_out = skip_out;
    S.history = history;
    hipError_t e = d3f::launch_align_step(S, I, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_align_step launch");
}

// ---- consensus poses from (model point, candidate) triples (consensus_kernels.hip) ----
namespace {

// M, k, n_trip -> T, or a status
int consensus_shape(const char *who, int32_t M, int32_t k, int64_t n_trip, int64_t &T)
{
    if (n_trip < 0) return fail(D3F_ERR_INVALID_ARG, "%s: n_trip=%lld is negative", who, (long long)n_trip);
    if (M < 3 || M > D3F_CONSENSUS_MAX_POINTS || k < 1 || k > D3F_CONSENSUS_MAX_CANDIDATES)
        return fail(D3F_ERR_BAD_SHAPE, "%s: M=%d outside [3, %d] or k=%d outside [1, %d]", who, M, D3F_CONSENSUS_MAX_POINTS, k, D3F_CONSENSUS_MAX_CANDIDATES);
    const int64_t k3 = (int64_t)k * k * k;
    if (n_trip > 0x7fffffffLL / k3) return fail(D3F_ERR_BAD_SHAPE, "%s: n_trip=%lld times k^3=%lld is above 2^31 - 1 hypotheses", who, (long long)n_trip, (long long)k3);
    T = n_trip * k3;
    return D3F_OK;
}

int consensus_terms(const char *who, float tau2, double side_tol, double min_side, double min_sin)
{
    if (!(tau2 > 0.0f) || !finite_nonneg(tau2)) return fail(D3F_ERR_INVALID_ARG, "%s: tau2 must be finite and positive", who);
    if (!finite_nonneg(side_tol) || !finite_nonneg(min_side) || !finite_nonneg(min_sin) || min_sin > 1.0)
        return fail(D3F_ERR_INVALID_ARG, "%s: side_tol / min_side must be finite and not negative, min_sin in [0, 1]", who);
    return D3F_OK;
}

}  // namespace

int64_t d3f_pose_consensus_workspace_bytes(int32_t M, int32_t k, int64_t n_trip, int64_t max_survivors)
{
    int64_t T = 0;
    if (consensus_shape("pose_consensus_workspace_bytes", M, k, n_trip, T) != D3F_OK) return 0;
    if (max_survivors < 1 || max_survivors > D3F_CONSENSUS_MAX_SURVIVORS) return 0;
    return d3f::consensus_layout(T, max_survivors).total;
}

int d3f_pose_consensus_score(const float *model, const float *cand, int32_t M, int32_t k, const int32_t *triplets, const int32_t *triplets_host,
                             int64_t n_trip, float tau2, double side_tol, double min_side, double min_sin, uint8_t *count_out, float *pose_out,
                             int8_t *assign_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "pose_consensus_score";
    int64_t T = 0;
    int rc = consensus_terms(who, tau2, side_tol, min_side, min_sin);
    if (rc != D3F_OK) return rc;
    rc = consensus_shape(who, M, k, n_trip, T);
    if (rc != D3F_OK) return rc;
    if (n_trip == 0) return D3F_OK;
    if (!model || !cand || !triplets || !triplets_host || !count_out || !workspace)
        return fail(D3F_ERR_INVALID_ARG, "%s: model / cand / triplets / triplets_host / count_out / workspace must be non-NULL", who);
    for (int64_t t = 0; t < n_trip; ++t) {
        const int32_t i = triplets_host[3 * t], j = triplets_host[3 * t + 1], l = triplets_host[3 * t + 2];
        if (!(0 <= i && i < j && j < l && l < M)) return fail(D3F_ERR_BAD_SHAPE, "%s: triplet %lld = (%d, %d, %d) is not 0 <= i < j < l < M=%d", who, (long long)t, i, j, l, M);
    }
    if (!aligned(model, 4) || !aligned(cand, 4) || !aligned(triplets, 4) || !aligned(pose_out, 4) || !aligned(workspace, 16))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: model / cand / triplets / pose_out must be 4-byte aligned, the workspace 16-byte aligned", who);
    const d3f::ConsensusLayout L = d3f::consensus_layout(T, 1);
    if (workspace_bytes < L.eq) return fail(D3F_ERR_WORKSPACE, "%s: needs %lld workspace bytes", who, (long long)L.eq);
    d3f::ConsensusParams C;
    C.model = model;
    C.cand = cand;
    C.trip = triplets;
    C.M = M;
    C.k = k;
    C.T = T;
    C.tau2 = tau2;
    C.side_tol = side_tol;
    C.min_side = min_side;
    C.min_sin2 = min_sin * min_sin;
    C.count = count_out;
    C.pose_dbg = pose_out;
    C.assign_dbg = assign_out;
    C.head = static_cast<uint32_t *>(d3f::ws_at(workspace, L.head));
    hipError_t e = d3f::launch_consensus_score(C, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "pose_consensus_score launch");
}

int d3f_pose_consensus_select(const float *model, const float *cand, int32_t M, int32_t k, const int32_t *triplets, int64_t n_trip, float tau2,
                              double side_tol, double min_side, double min_sin, const uint8_t *count, int32_t min_inliers, int32_t shared,
                              int64_t max_survivors, int32_t n_poses, int32_t *hyp_out, int32_t *inliers_out, int8_t *assign_out, float *pose_out,
                              int32_t *stats_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "pose_consensus_select";
    int64_t T = 0;
    int rc = consensus_terms(who, tau2, side_tol, min_side, min_sin);
    if (rc != D3F_OK) return rc;
    if (min_inliers < 3 || min_inliers > D3F_CONSENSUS_MAX_POINTS || shared < 1 || shared > D3F_CONSENSUS_MAX_POINTS)
        return fail(D3F_ERR_INVALID_ARG, "%s: min_inliers=%d outside [3, 64] or shared=%d outside [1, 64]", who, min_inliers, shared);
    if (max_survivors < 1 || max_survivors > D3F_CONSENSUS_MAX_SURVIVORS)
        return fail(D3F_ERR_INVALID_ARG, "%s: max_survivors=%lld outside [1, %d]", who, (long long)max_survivors, D3F_CONSENSUS_MAX_SURVIVORS);
    rc = consensus_shape(who, M, k, n_trip, T);
    if (rc != D3F_OK) return rc;
    if (n_poses < 1 || n_poses > D3F_CONSENSUS_MAX_POINTS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_poses=%d outside [1, 64]", who, n_poses);
    if (n_trip == 0) return D3F_OK;
    if (!model || !cand || !triplets || !count || !hyp_out || !inliers_out || !assign_out || !pose_out || !stats_out || !workspace)
        return fail(D3F_ERR_INVALID_ARG, "%s: model / cand / triplets / count / the outputs / workspace must be non-NULL", who);
    if (!aligned(model, 4) || !aligned(cand, 4) || !aligned(triplets, 4) || !aligned(hyp_out, 4) || !aligned(inliers_out, 4) || !aligned(assign_out, 4) ||
        !aligned(pose_out, 4) || !aligned(stats_out, 4) || !aligned(workspace, 16))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: float / int32 arrays and assign_out must be 4-byte aligned, the workspace 16-byte aligned", who);
    const d3f::ConsensusLayout L = d3f::consensus_layout(T, max_survivors);
    if (workspace_bytes < L.total) return fail(D3F_ERR_WORKSPACE, "%s: needs %lld workspace bytes", who, (long long)L.total);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    d3f::ConsensusSelect S;
    S.C.model = model;
    S.C.cand = cand;
    S.C.trip = triplets;
    S.C.M = M;
    S.C.k = k;
    S.C.T = T;
    S.C.tau2 = tau2;
    S.C.side_tol = side_tol;
    S.C.min_side = min_side;
    S.C.min_sin2 = min_sin * min_sin;
    S.C.count = const_cast<uint8_t *>(count);
    S.C.pose_dbg = nullptr;
    S.C.assign_dbg = nullptr;
    S.C.head = reinterpret_cast<uint32_t *>(ws + L.head);
    S.min_inliers = min_inliers;
    S.shared = shared;
    S.n_poses = n_poses;
    S.max_survivors = (uint32_t)max_survivors;
    S.eq_block = reinterpret_cast<uint32_t *>(ws + L.eq);
    S.fl_block = reinterpret_cast<uint32_t *>(ws + L.fl);
    S.scan_scratch = ws + L.scan;
    S.surv_h = reinterpret_cast<int32_t *>(ws + L.surv_h);
    S.surv_count = ws + L.surv_count;
    S.alive = ws + L.alive;
    S.surv_assign = reinterpret_cast<int8_t *>(ws + L.surv_assign);
    S.hyp_out = hyp_out;
    S.count_out = inliers_out;
    S.stats_out = stats_out;
    S.assign_out = assign_out;
    S.pose_out = pose_out;
    hipError_t e = d3f::launch_consensus_select(S, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "pose_consensus_select launch");
}

int d3f_pose_refit(const float *model, const float *cand, int32_t M, int32_t k, const int8_t *assign, int32_t n_poses, float tau2, float *pose_out,
                   double *rmse_out, int32_t *inliers_out, void *stream)
{
    const char *who = "pose_refit";
    int64_t T = 0;
    if (!(tau2 > 0.0f) || !finite_nonneg(tau2)) return fail(D3F_ERR_INVALID_ARG, "%s: tau2 must be finite and positive", who);
    int rc = consensus_shape(who, M, k, 0, T);
    if (rc != D3F_OK) return rc;
    if (n_poses < 0 || n_poses > D3F_CONSENSUS_MAX_POINTS) return fail(D3F_ERR_BAD_SHAPE, "%s: n_poses=%d outside [0, 64]", who, n_poses);
    if (n_poses == 0) return D3F_OK;
    if (!model || !cand || !assign || !pose_out || !rmse_out || !inliers_out) return fail(D3F_ERR_INVALID_ARG, "%s: model / cand / assign / the outputs must be non-NULL", who);
    if (!aligned(model, 4) || !aligned(cand, 4) || !aligned(pose_out, 4) || !aligned(inliers_out, 4) || !aligned(rmse_out, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "%s: float / int32 arrays must be 4-byte aligned, rmse_out 8-byte aligned", who);
    hipError_t e = d3f::launch_pose_refit(model, cand, M, k, assign, n_poses, tau2, pose_out, rmse_out, inliers_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "pose_refit launch");
}

// ---- the first surface a ray meets in a baked volume (raycast_kernels.hip) ----
int d3f_volume_raycast(const d3f_volume *vol, const float *origins, const float *dirs, int64_t n, const d3f_pinhole *camera,
                       float march_step, float t_near, float t_far, float *out_t, uint8_t *out_hit, float *out_points,
                       int32_t *out_samples, void *stream)
{
    const int rc = check_volume("volume_raycast", vol);
    if (rc != D3F_OK) return rc;
    if (!positive_finite(vol->step)) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: vol->step must be > 0 and finite");
    if (!positive_finite(march_step)) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: march_step must be > 0 and finite");
    const double ex = vol->nx - 1, ey = vol->ny - 1, ez = vol->nz - 1;
    const double steps = ceil((double)vol->step * sqrt(ex * ex + ey * ey + ez * ez) / (double)march_step);
    if (!(steps <= (double)D3F_RAYCAST_MAX_STEPS))
        return fail(D3F_ERR_INVALID_ARG, "volume_raycast: march_step=%g takes %.0f steps across the box diagonal, more than %d", (double)march_step, steps,
                    D3F_RAYCAST_MAX_STEPS);
    if (!(t_near >= 0.0f) || t_near * 0.0f != 0.0f) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: t_near must be >= 0 and finite");
    if (t_far != t_far) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: t_far is NaN");
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: n=%lld is negative", (long long)n);
    if (n > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "volume_raycast: n=%lld rays, more than 2^31 - 1", (long long)n);
    d3f::RayParams P = {};
    if (camera) {
        if (camera->H < 0 || camera->W < 0) return fail(D3F_ERR_BAD_SHAPE, "volume_raycast: camera H=%d W=%d", camera->H, camera->W);
        if ((int64_t)camera->H * camera->W > 0x7fffffffLL)
            return fail(D3F_ERR_BAD_SHAPE, "volume_raycast: camera H*W=%lld pixels, more than 2^31 - 1", (long long)camera->H * camera->W);
        if (n != (int64_t)camera->H * camera->W) return fail(D3F_ERR_BAD_SHAPE, "volume_raycast: n=%lld but camera H*W=%lld", (long long)n, (long long)camera->H * camera->W);
        if (origins || dirs) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: origins / dirs must be NULL with a camera");
        const float fx = camera->K[0], fy = camera->K[4];
        if (fx == 0.0f || fy == 0.0f || fx * 0.0f != 0.0f || fy * 0.0f != 0.0f) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: camera fx / fy must be non-zero and finite");
        P.H = camera->H; P.W = camera->W;
        P.fx = fx; P.fy = fy; P.cx = camera->K[2]; P.cy = camera->K[5];
        for (int r = 0; r < 3; ++r)
            for (int a = 0; a < 3; ++a) P.R[3 * r + a] = camera->pose[4 * r + a];
        for (int a = 0; a < 3; ++a) {                      // o = -R^T tc in double, rounded once
            double acc = 0.0;
            for (int r = 0; r < 3; ++r) acc += (double)camera->pose[4 * r + a] * (double)camera->pose[4 * r + 3];
            P.co[a] = (float)(-acc);
        }
    }
    if (n == 0) return D3F_OK;
    if (!vol->dist || !vol->cell_valid) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: vol->dist / vol->cell_valid must be non-NULL");
    if (!camera && (!origins || !dirs)) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: origins / dirs must be non-NULL without a camera");
    if (!out_t || !out_hit || !out_points) return fail(D3F_ERR_INVALID_ARG, "volume_raycast: out_t / out_hit / out_points must be non-NULL");
    if (!aligned(vol->dist, 4) || !aligned(origins, 4) || !aligned(dirs, 4) || !aligned(out_t, 4) || !aligned(out_points, 4) || !aligned(out_samples, 4))
        return fail(D3F_ERR_BAD_LAYOUT, "volume_raycast: vol->dist / origins / dirs / out_t / out_points / out_samples must be 4-byte aligned");
    P.dist = vol->dist;
    P.cell = vol->cell_valid;
    P.origins = origins;
    P.dirs = dirs;
    P.out_t = out_t;
    P.out_hit = out_hit;
    P.out_pts = out_points;
    P.out_samples = out_samples;
    P.n = n;
    P.nx = vol->nx; P.ny = vol->ny; P.nz = vol->nz;
    P.ox = vol->origin[0]; P.oy = vol->origin[1]; P.oz = vol->origin[2];
    P.h = vol->step;
    P.march = march_step;
    P.t_near = t_near;
    P.t_far = t_far;
    hipError_t e = d3f::launch_volume_raycast(P, camera != nullptr, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "volume_raycast launch");
}

int64_t d3f_fps_workspace_bytes(int64_t n) { return n > 0 ? d3f::fps_layout(n, 4).total : 0; }
int64_t d3f_fps_pixels_workspace_bytes(int64_t n) { return n > 0 ? d3f::fps_layout(n, 8).total : 0; }

int d3f_farthest_point_sampling(const float *pts, int64_t n, int32_t k, int64_t init_idx, int64_t *out_idx, float *out_maxdist,
                                void *workspace, void *stream)
{
    if (n < 1 || k < 0) return fail(D3F_ERR_BAD_SHAPE, "fps: n=%lld must be >= 1 (fps_np asserts a non-empty cloud), k=%d", (long long)n, k);
    if (k == 0) return D3F_OK;
    if (!pts || !out_idx || !workspace) return fail(D3F_ERR_INVALID_ARG, "fps: NULL pointer");
    if (!aligned(workspace, 16)) return fail(D3F_ERR_BAD_LAYOUT, "fps: workspace must be 16-byte aligned");
    if (init_idx < 0 || init_idx >= n) return fail(D3F_ERR_INVALID_ARG, "fps: init_idx=%lld outside [0,%lld)", (long long)init_idx, (long long)n);
    hipError_t e = d3f::launch_fps(pts, n, k, init_idx, out_idx, out_maxdist, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "fps launch");
}

static int backward_common(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps, int32_t n_maps,
                           float mu, const float *grad_dist, const float *const *grad_fused, float *grad_pts, void *stream,
                           int mode)
{
    int rc = check_views(views);
    if (rc != D3F_OK) return rc;
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "n=%lld is negative", (long long)n);
    if (n == 0) return D3F_OK;
    if (!pts || !grad_pts) return fail(D3F_ERR_INVALID_ARG, "pts/grad_pts must be non-NULL");
    if (n_maps < 0 || n_maps > D3F_MAX_MAPS) return fail(D3F_ERR_BAD_SHAPE, "n_maps=%d outside [0,%d]", n_maps, D3F_MAX_MAPS);
    if (n_maps > 0 && (!maps || !grad_fused)) return fail(D3F_ERR_INVALID_ARG, "maps/grad_fused must be non-NULL when n_maps > 0");
    if (!(mu > 0.0f)) return fail(D3F_ERR_INVALID_ARG, "mu must be > 0");
    d3f::BackwardParams P;
    P.depth = views->depth; P.K = views->K; P.pose = views->pose; P.pts = pts;
    P.grad_dist = grad_dist; P.grad_pts = grad_pts;
    P.n = n; P.V = views->V; P.H = views->H; P.W = views->W; P.n_maps = n_maps; P.mu = mu;
    // the forward's rule (eval_common): the words are read when depth and every map carry one; eval_dist needs none (a
    // non-finite depth texel passes no NaN there) and decides per point on its projection alone
    P.n_words = 0;
    if (mode == 0 && views->depth_nonfinite) {
        bool all = true;
        for (int s = 0; s < n_maps; ++s) all = all && maps[s].nonfinite;
        if (all) {
            P.words[P.n_words++] = views->depth_nonfinite;
            for (int s = 0; s < n_maps; ++s) P.words[P.n_words++] = maps[s].nonfinite;
        }
    }
    for (int k = 0; k < P.n_words; ++k)
        if (!aligned(P.words[k], 4)) return fail(D3F_ERR_BAD_LAYOUT, "nonfinite word %d: device pointer must be 4-byte aligned", k);
    int64_t map_bytes = 0;
    for (int s = 0; s < n_maps; ++s) {
        P.grad_fused[s] = grad_fused[s];
        rc = fill_map(maps[s], s, views->V, nullptr, nullptr, grad_fused[s], P.maps[s], map_bytes);
        if (rc != D3F_OK) return rc;
    }
    int t = 128;                       // LDS: 44 B per (point, view) + 8 B per point
    while (t > 16 && (long)t * views->V * 44 > 60 * 1024) t >>= 1;
    while (t > 8 && n / t < 1024) t >>= 1;     // small batches: spread over many workgroups (latency, not throughput)
    P.tile_pts = t;
    if ((n + t - 1) / t > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "n=%lld needs more than 2^31 workgroups", (long long)n);
    hipError_t e = d3f::launch_fused_backward(P, mode, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "fused_eval_backward launch");
}

int d3f_eval_backward(const d3f_views *views, const float *pts, int64_t n, const d3f_channel_map *maps, int32_t n_maps,
                      float mu, const float *grad_dist, const float *const *grad_fused, float *grad_pts, void *stream)
{
    return backward_common(views, pts, n, maps, n_maps, mu, grad_dist, grad_fused, grad_pts, stream, 0);
}

int d3f_eval_dist_backward(const d3f_views *views, const float *pts, int64_t n, const float *grad_dist, float *grad_pts,
                           void *stream)
{
    return backward_common(views, pts, n, nullptr, 0, 1.0f, grad_dist, nullptr, grad_pts, stream, 1);
}

int d3f_point_order_locality(const float *pts, int64_t n, float *out, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "n=%lld is negative", (long long)n);
    if (!out || (n > 0 && !pts)) return fail(D3F_ERR_INVALID_ARG, "point_order_locality: NULL pointer");
    hipError_t e = d3f::launch_point_locality(pts, n, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "point locality launch");
}

int d3f_points_probe(const float *pts, int64_t n, int32_t *out, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "n=%lld is negative", (long long)n);
    if (!out || (n > 0 && !pts)) return fail(D3F_ERR_INVALID_ARG, "points_probe: NULL pointer");
    hipError_t e = d3f::launch_points_probe(pts, n, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "points probe launch");
}

int d3f_lattice_probe(const float *pts, int64_t n, int32_t *out_dims, void *stream)
{
    if (n < 0) return fail(D3F_ERR_INVALID_ARG, "n=%lld is negative", (long long)n);
    if (!out_dims || (n > 0 && !pts)) return fail(D3F_ERR_INVALID_ARG, "lattice_probe: NULL pointer");
    hipError_t e = d3f::launch_lattice_probe(pts, n, out_dims, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "lattice probe launch");
}

int d3f_eval_dist(const d3f_views *views, const float *pts, int64_t n, float *out_dist, uint8_t *out_valid,
                  void *stream)
{
    return eval_common(views, pts, n, nullptr, 0, 1.0f, 0u, out_dist, out_valid, nullptr, nullptr, nullptr, 0, stream, 1);
}

#ifdef D3F_EXPERIMENTS
// experiments builds only (not in the header): the phase stamps of the last stamped launch, 32 x uint64 per sampled workgroup
int d3f_exp_read_stamps(unsigned long long *host_out, int64_t n_words)
{
    unsigned long long *dev = exp_stamp_buffer(false);
    if (!dev || !host_out || n_words < 0 || n_words * 8 > kStampBytes) return D3F_ERR_INVALID_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return D3F_ERR_HIP;
    return hipMemcpy(host_out, dev, (size_t)n_words * 8, hipMemcpyDeviceToHost) == hipSuccess ? D3F_OK : D3F_ERR_HIP;
}
#endif

int d3f_map_check(const d3f_channel_map *map, int32_t V, uint32_t *word_out, void *stream)
{
    if (!map || !word_out) return fail(D3F_ERR_INVALID_ARG, "map_check: NULL pointer");
    if (!aligned(word_out, 4)) return fail(D3F_ERR_BAD_LAYOUT, "map_check: word_out must be 4-byte aligned");
    if (V < 1 || map->fh < 1 || map->fw < 1 || map->C < 1) return fail(D3F_ERR_BAD_SHAPE, "map_check: V=%d fh=%d fw=%d C=%d", V, map->fh, map->fw, map->C);
    if (!map->data) return fail(D3F_ERR_INVALID_ARG, "map_check: data pointer is NULL");
    if (map->dtype != D3F_DTYPE_F32 && map->dtype != D3F_DTYPE_F16) return fail(D3F_ERR_BAD_DTYPE, "map_check: dtype %d unsupported", map->dtype);
    const int es = map->dtype == D3F_DTYPE_F16 ? 2 : 4;
    if (!aligned(map->data, es)) return fail(D3F_ERR_BAD_LAYOUT, "map_check: data must be aligned to its element size");
    if (map->stride_x < map->C || map->stride_y < 0 || map->stride_v < 0) return fail(D3F_ERR_BAD_LAYOUT, "map_check: strides do not describe a channels-last map");
    hipError_t e = d3f::launch_map_check(map->data, V, map->fh, map->fw, map->C, map->stride_v, map->stride_y, map->stride_x, es,
                                         word_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "map_check launch");
}

int d3f_map_check_many(const d3f_channel_map *maps, const int32_t *views, int32_t n, uint32_t *const *words_out, uint32_t flags, void *stream)
{
    if (n < 0 || n > D3F_MAX_MAPS + 1) return fail(D3F_ERR_BAD_SHAPE, "map_check_many: n=%d outside [0,%d]", n, D3F_MAX_MAPS + 1);
    if (n == 0) return D3F_OK;
    if (!maps || !views || !words_out) return fail(D3F_ERR_INVALID_ARG, "map_check_many: NULL pointer");
    const void *data[D3F_MAX_MAPS + 1];
    int64_t nbytes[D3F_MAX_MAPS + 1];
    int esize[D3F_MAX_MAPS + 1];
    uint32_t *words[D3F_MAX_MAPS + 1];
    int nf = 0;
    const bool zero = (flags & D3F_CHECK_WORDS_ARE_ZERO) != 0;
    for (int k = 0; k < n; ++k) {
        const d3f_channel_map &m = maps[k];
        // the same validation as d3f_map_check; a tensor that is not one flat 16-byte aligned block takes the single-tensor call
        if (!words_out[k] || !aligned(words_out[k], 4)) return fail(D3F_ERR_BAD_LAYOUT, "map_check_many: word %d must be a 4-byte aligned device pointer", k);
        if (views[k] < 1 || m.fh < 1 || m.fw < 1 || m.C < 1) return fail(D3F_ERR_BAD_SHAPE, "map_check_many: tensor %d: V=%d fh=%d fw=%d C=%d", k, views[k], m.fh, m.fw, m.C);
        if (!m.data) return fail(D3F_ERR_INVALID_ARG, "map_check_many: tensor %d: data pointer is NULL", k);
        if (m.dtype != D3F_DTYPE_F32 && m.dtype != D3F_DTYPE_F16) return fail(D3F_ERR_BAD_DTYPE, "map_check_many: tensor %d: dtype %d unsupported", k, m.dtype);
        const int es = m.dtype == D3F_DTYPE_F16 ? 2 : 4;
        if (!aligned(m.data, es)) return fail(D3F_ERR_BAD_LAYOUT, "map_check_many: tensor %d: data must be aligned to its element size", k);
        if (m.stride_x < m.C || m.stride_y < 0 || m.stride_v < 0) return fail(D3F_ERR_BAD_LAYOUT, "map_check_many: tensor %d: strides do not describe a channels-last map", k);
        if (d3f::map_is_flat(m.data, views[k], m.fh, m.fw, m.C, m.stride_v, m.stride_y, m.stride_x)) {
            data[nf] = m.data; nbytes[nf] = (int64_t)views[k] * m.fh * m.fw * m.C * es; esize[nf] = es; words[nf] = words_out[k];
            ++nf;
        } else {
            hipError_t e = d3f::launch_map_check(m.data, views[k], m.fh, m.fw, m.C, m.stride_v, m.stride_y, m.stride_x, es, words_out[k],
                                                 static_cast<hipStream_t>(stream));
            if (e != hipSuccess) return hip_fail(e, "map_check launch");
        }
    }
    hipError_t e = d3f::launch_map_check_many(data, nbytes, esize, words, nf, zero, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "map_check_many launch");
}

int d3f_project_maps(const d3f_channel_map *src, int32_t V, const float *W, int32_t k, float *dst, void *stream)
{
    if (!src || !W || !dst) return fail(D3F_ERR_INVALID_ARG, "project_maps: NULL pointer");
    if (!src->data) return fail(D3F_ERR_INVALID_ARG, "project_maps: data pointer is NULL");
    if (k < 1 || k > D3F_MAX_PROJECTION) return fail(D3F_ERR_BAD_SHAPE, "project_maps: k=%d outside [1,%d]", k, D3F_MAX_PROJECTION);
    if (V < 1 || src->fh < 1 || src->fw < 1 || src->C < 1) return fail(D3F_ERR_BAD_SHAPE, "project_maps: V=%d fh=%d fw=%d C=%d", V, src->fh, src->fw, src->C);
    if (src->dtype != D3F_DTYPE_F32 && src->dtype != D3F_DTYPE_F16) return fail(D3F_ERR_BAD_DTYPE, "project_maps: dtype %d unsupported", src->dtype);
    const int es = src->dtype == D3F_DTYPE_F16 ? 2 : 4;
    if (!aligned(src->data, es) || !aligned(W, 4) || !aligned(dst, 4)) return fail(D3F_ERR_BAD_LAYOUT, "project_maps: pointers must be aligned to their element size");
    if (src->stride_x < src->C || src->stride_y < 0 || src->stride_v < 0) return fail(D3F_ERR_BAD_LAYOUT, "project_maps: strides do not describe a channels-last map");
    hipError_t e = d3f::launch_project_maps(src->data, V, src->fh, src->fw, src->C, src->stride_v, src->stride_y, src->stride_x, es == 2, W, k, dst,
                                            static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "project_maps launch");
}

int64_t d3f_row_moments_workspace_bytes(int64_t M, int32_t C)
{
    if (M < 1 || C < 1 || C > D3F_MAX_MOMENT_CHANNELS) return 0;
    return d3f::row_moments_workspace_bytes(M, C);
}

int d3f_row_moments(const void *rows, int32_t dtype, int64_t M, int32_t C, int64_t row_stride, const float *weights, double *wsum_out,
                    double *mean_out, double *scatter_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (C < 1 || C > D3F_MAX_MOMENT_CHANNELS) return fail(D3F_ERR_BAD_SHAPE, "row_moments: C=%d outside [1,%d]", C, D3F_MAX_MOMENT_CHANNELS);
    if (M < 1) return fail(D3F_ERR_BAD_SHAPE, "row_moments: M=%lld (at least one row)", (long long)M);
    if (dtype != D3F_DTYPE_F32 && dtype != D3F_DTYPE_F16) return fail(D3F_ERR_BAD_DTYPE, "row_moments: dtype %d unsupported", dtype);
    if (row_stride < C) return fail(D3F_ERR_BAD_LAYOUT, "row_moments: row_stride=%lld below C=%d", (long long)row_stride, C);
    if (!rows || !wsum_out || !mean_out || !scatter_out) return fail(D3F_ERR_INVALID_ARG, "row_moments: NULL pointer");
    if (!aligned(rows, dtype == D3F_DTYPE_F16 ? 2 : 4) || !aligned(weights, 4) || !aligned(wsum_out, 8) || !aligned(mean_out, 8) || !aligned(scatter_out, 8))
        return fail(D3F_ERR_BAD_LAYOUT, "row_moments: pointers must be aligned to their element size");
    const int64_t need = d3f::row_moments_workspace_bytes(M, C);
    if (!workspace || workspace_bytes < need) return fail(D3F_ERR_WORKSPACE, "row_moments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    if (!aligned(workspace, 16)) return fail(D3F_ERR_BAD_LAYOUT, "row_moments: workspace must be 16-byte aligned");
    hipError_t e = d3f::launch_row_moments(rows, dtype == D3F_DTYPE_F16, M, C, row_stride, weights, wsum_out, mean_out, scatter_out, workspace,
                                           static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "row_moments launch");
}

int d3f_onehot2instance(const float *onehot, int64_t n, int32_t NI, uint8_t *out, void *stream)
{
    if (n < 0 || NI < 1 || NI > 256) return fail(D3F_ERR_BAD_SHAPE, "onehot2instance: n=%lld NI=%d (NI must be in [1,256])", (long long)n, NI);
    if (n == 0) return D3F_OK;
    if (!onehot || !out) return fail(D3F_ERR_INVALID_ARG, "onehot2instance: NULL pointer");
    hipError_t e = d3f::launch_onehot2instance(onehot, n, NI, out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "onehot2instance launch");
}

int d3f_instance2onehot(const uint8_t *instance, int64_t n, int32_t NI, uint8_t *out_bool, void *stream)
{
    if (n < 0 || NI < 1 || NI > 256) return fail(D3F_ERR_BAD_SHAPE, "instance2onehot: n=%lld NI=%d (NI must be in [1,256])", (long long)n, NI);
    if (n == 0) return D3F_OK;
    if (!instance || !out_bool) return fail(D3F_ERR_INVALID_ARG, "instance2onehot: NULL pointer");
    hipError_t e = d3f::launch_instance2onehot(instance, n, NI, out_bool, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "instance2onehot launch");
}

int64_t d3f_softmax_workspace_bytes(int64_t rows, int64_t cols)
{
    if (rows <= 0 || cols <= 0) return 0;
    return d3f::softmax_layout(rows, cols).total;
}

// the column statistics inside a workspace of d3f_softmax_workspace_bytes(rows, cols) (or of a layout that begins with them); NULL stays NULL
static d3f::ColStat *softmax_stats(void *workspace, int64_t rows, int64_t cols)
{
    return workspace ? static_cast<d3f::ColStat *>(d3f::ws_at(workspace, d3f::softmax_layout(rows, cols).stats)) : nullptr;
}

static int check_sim_enums(int32_t dist_type, int32_t mode)
{
    if (dist_type != D3F_DIST_L2 && dist_type != D3F_DIST_SQUARE) return fail(D3F_ERR_INVALID_ARG, "dist_type=%d (expected D3F_DIST_L2 or D3F_DIST_SQUARE)", dist_type);
    if (mode < D3F_SIM_DIST || mode > D3F_SIM_SOFTMAX_DIM0) return fail(D3F_ERR_INVALID_ARG, "mode=%d is not a D3F_SIM_* value", mode);
    return D3F_OK;
}

int d3f_similarity_to_target(const float *src, int64_t B, int64_t inner, int32_t C, int64_t stride_b,
                             int64_t stride_i, int64_t stride_c, const float *tgt, float scale, int32_t dist_type,
                             int32_t mode, float *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_sim_enums(dist_type, mode);
    if (rc != D3F_OK) return rc;
    if (B < 0 || inner < 0 || C < 1) return fail(D3F_ERR_BAD_SHAPE, "similarity_to_target: B=%lld inner=%lld C=%d", (long long)B, (long long)inner, C);
    if (B == 0 || inner == 0) return D3F_OK;
    if (!src || !tgt || !out) return fail(D3F_ERR_INVALID_ARG, "similarity_to_target: NULL pointer");
    if (mode == D3F_SIM_SOFTMAX_DIM0 && (!workspace || workspace_bytes < d3f_softmax_workspace_bytes(B, inner)))
        return fail(D3F_ERR_WORKSPACE, "similarity_to_target: softmax needs %lld workspace bytes", (long long)d3f_softmax_workspace_bytes(B, inner));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = d3f::launch_dist_to_target(src, B, inner, C, stride_b, stride_i, stride_c, tgt, dist_type, out, s);
    if (e != hipSuccess) return hip_fail(e, "dist_to_target launch");
    if (mode == D3F_SIM_EXP) {
        e = d3f::launch_exp_neg_scale(out, B * inner, scale, s);
        if (e != hipSuccess) return hip_fail(e, "exp launch");
    } else if (mode == D3F_SIM_SOFTMAX_DIM0) {
        e = d3f::launch_softmax_dim0(out, B, inner, scale, nullptr, softmax_stats(workspace, B, inner), false, s);
        if (e != hipSuccess) return hip_fail(e, "softmax launch");
    }
    return D3F_OK;
}

int d3f_pairwise_similarity(const float *src, const float *tgt, int64_t B1, int64_t B2, int32_t C, float scale,
                            int32_t dist_type, int32_t mode, float *out, int64_t *argmax_out, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    int rc = check_sim_enums(dist_type, mode);
    if (rc != D3F_OK) return rc;
    if (B1 < 0 || B2 < 0 || C < 1) return fail(D3F_ERR_BAD_SHAPE, "pairwise: B1=%lld B2=%lld C=%d", (long long)B1, (long long)B2, C);
    if (B1 == 0 || B2 == 0) return D3F_OK;
    if (!src || !tgt || !out) return fail(D3F_ERR_INVALID_ARG, "pairwise: NULL pointer");
    if ((B2 + 63) / 64 > 0x7fffffffLL || (B1 + 63) / 64 > 65535) return fail(D3F_ERR_BAD_SHAPE, "pairwise: B1=%lld exceeds 64*65535 rows per call", (long long)B1);
    const bool need_ws = (mode == D3F_SIM_SOFTMAX_DIM0) || (argmax_out != nullptr);
    if (need_ws && (!workspace || workspace_bytes < d3f_softmax_workspace_bytes(B1, B2)))
        return fail(D3F_ERR_WORKSPACE, "pairwise: needs %lld workspace bytes", (long long)d3f_softmax_workspace_bytes(B1, B2));
    hipStream_t s = static_cast<hipStream_t>(stream);
    d3f::ColStat *ws = softmax_stats(workspace, B1, B2);
    // the column statistics (softmax / best match) come out of the distance kernel's epilogue, per 64-row tile
    hipError_t e = d3f::launch_pairwise_dist(src, tgt, B1, B2, C, dist_type, out, s, need_ws ? ws : nullptr,
                                             mode == D3F_SIM_SOFTMAX_DIM0 ? scale : 1.0f);
    if (e != hipSuccess) return hip_fail(e, "pairwise_dist launch");
    if (mode == D3F_SIM_SOFTMAX_DIM0) {
        e = d3f::launch_softmax_dim0(out, B1, B2, scale, argmax_out, ws, true, s);
        if (e != hipSuccess) return hip_fail(e, "softmax launch");
    } else {
        if (argmax_out) {   // best match = smallest distance, decided before exp() can tie values
            e = d3f::launch_argmin_dim0(out, B1, B2, argmax_out, ws, true, s);
            if (e != hipSuccess) return hip_fail(e, "argmin launch");
        }
        if (mode == D3F_SIM_EXP) {
            e = d3f::launch_exp_neg_scale(out, B1 * B2, scale, s);
            if (e != hipSuccess) return hip_fail(e, "exp launch");
        }
    }
    return D3F_OK;
}

int64_t d3f_pairwise_topk_workspace_bytes(int64_t B1, int64_t B2)
{
    if (B1 <= 0 || B2 <= 0) return 0;
    return d3f::pair_topk_layout(B1, B2).total;
}

int d3f_pairwise_similarity_topk(const float *src, const float *tgt, int64_t B1, int64_t B2, int32_t C, float scale,
                                 int32_t dist_type, int32_t mode, int32_t k, float *out, int64_t *topk_idx, float *topk_val,
                                 void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_sim_enums(dist_type, mode);
    if (rc != D3F_OK) return rc;
    if (k < 1 || k > 8) return fail(D3F_ERR_INVALID_ARG, "pairwise_topk: k=%d outside [1,8]", k);
    if (B1 < 0 || B2 < 0 || C < 1) return fail(D3F_ERR_BAD_SHAPE, "pairwise_topk: B1=%lld B2=%lld C=%d", (long long)B1, (long long)B2, C);
    if (B2 == 0) return D3F_OK;
    if (!topk_idx) return fail(D3F_ERR_INVALID_ARG, "pairwise_topk: topk_idx is NULL");
    if (B1 > 0 && (!src || !tgt || !out)) return fail(D3F_ERR_INVALID_ARG, "pairwise_topk: NULL pointer");
    if (B1 > 0x7fffffffLL || (B2 + 63) / 64 > 0x7fffffffLL || (B1 + 63) / 64 > 65535)
        return fail(D3F_ERR_BAD_SHAPE, "pairwise_topk: B1=%lld exceeds 64*65535 rows per call", (long long)B1);
    if (B1 > 0 && (!workspace || workspace_bytes < d3f_pairwise_topk_workspace_bytes(B1, B2) || !aligned(workspace, 16)))
        return fail(D3F_ERR_WORKSPACE, "pairwise_topk: needs %lld bytes of 16-byte aligned workspace", (long long)d3f_pairwise_topk_workspace_bytes(B1, B2));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const void *final_list = nullptr;
    if (B1 > 0) {
        const d3f::PairTopkLayout L = d3f::pair_topk_layout(B1, B2);
        d3f::ColStat *ws = static_cast<d3f::ColStat *>(d3f::ws_at(workspace, L.stats));
        void *tk = d3f::ws_at(workspace, L.topk);
        const bool stats = mode == D3F_SIM_SOFTMAX_DIM0;
        e = d3f::launch_pairwise_dist(src, tgt, B1, B2, C, dist_type, out, s, stats ? ws : nullptr, stats ? scale : 1.0f);
        if (e != hipSuccess) return hip_fail(e, "pairwise_dist launch");
        // neighbours are chosen on the raw distances, before exp() / softmax can round close values into ties
        e = d3f::launch_topk_select(out, B1, B2, tk, &final_list, s);
        if (e != hipSuccess) return hip_fail(e, "topk launch");
        if (mode == D3F_SIM_SOFTMAX_DIM0) e = d3f::launch_softmax_dim0(out, B1, B2, scale, nullptr, ws, true, s);
        else if (mode == D3F_SIM_EXP) e = d3f::launch_exp_neg_scale(out, B1 * B2, scale, s);
        if (e != hipSuccess) return hip_fail(e, "similarity launch");
    }
    e = d3f::launch_topk_write(final_list, out, B1, B2, k, topk_idx, topk_val, s);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "topk write launch");
}

static_assert(sizeof(d3f_col_stat) == sizeof(d3f::ColStat) && sizeof(d3f_col_stat) == 16, "d3f_col_stat layout");

int d3f_topk_smallest(const float *x, int64_t rows, int64_t cols, int32_t k, int64_t *idx_out, float *val_out, void *workspace,
                      int64_t workspace_bytes, void *stream)
{
    if (k < 1 || k > 8) return fail(D3F_ERR_INVALID_ARG, "topk_smallest: k=%d outside [1,8]", k);
    if (rows < 0 || cols < 0 || rows > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "topk_smallest: rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (cols == 0) return D3F_OK;
    if (!idx_out || (rows > 0 && !x)) return fail(D3F_ERR_INVALID_ARG, "topk_smallest: NULL pointer");
    if (rows > 0 && (!workspace || workspace_bytes < d3f::topk_workspace_bytes(rows, cols) || !aligned(workspace, 16)))
        return fail(D3F_ERR_WORKSPACE, "topk_smallest: needs %lld bytes of 16-byte aligned workspace", (long long)d3f::topk_workspace_bytes(rows, cols));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const void *final_list = nullptr;
    if (rows > 0) {
        hipError_t e = d3f::launch_topk_select(x, rows, cols, workspace, &final_list, s);
        if (e != hipSuccess) return hip_fail(e, "topk launch");
    }
    hipError_t e = d3f::launch_topk_write(final_list, x, rows, cols, k, idx_out, val_out, s);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "topk write launch");
}

int d3f_topk_merge(const int64_t *parts_idx, const float *parts_val, int64_t n_parts, int32_t k, int64_t cols, int64_t *out_idx,
                   float *out_val, void *stream)
{
    if (k < 1 || k > 8) return fail(D3F_ERR_INVALID_ARG, "topk_merge: k=%d outside [1,8]", k);
    if (n_parts < 0 || cols < 0) return fail(D3F_ERR_BAD_SHAPE, "topk_merge: n_parts=%lld cols=%lld", (long long)n_parts, (long long)cols);
    if (cols == 0) return D3F_OK;
    if (!out_idx || (n_parts > 0 && (!parts_idx || !parts_val))) return fail(D3F_ERR_INVALID_ARG, "topk_merge: NULL pointer");
    hipError_t e = d3f::launch_topk_merge_parts(parts_idx, parts_val, n_parts, k, cols, out_idx, out_val, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "topk merge launch");
}

int d3f_pairwise_softmax_local(const float *src, const float *tgt, int64_t B1, int64_t B2, int32_t C, float scale,
                               int32_t dist_type, int64_t row_offset, float *out, d3f_col_stat *stats, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    int rc = check_sim_enums(dist_type, D3F_SIM_SOFTMAX_DIM0);
    if (rc != D3F_OK) return rc;
    if (B1 < 0 || B2 < 0 || C < 1 || row_offset < 0) return fail(D3F_ERR_BAD_SHAPE, "pairwise_softmax_local: B1=%lld B2=%lld C=%d row_offset=%lld", (long long)B1, (long long)B2, C, (long long)row_offset);
    if (B2 == 0) return D3F_OK;
    if (!stats || !tgt) return fail(D3F_ERR_INVALID_ARG, "pairwise_softmax_local: NULL pointer");
    if (B1 > 0 && (!src || !out)) return fail(D3F_ERR_INVALID_ARG, "pairwise_softmax_local: NULL pointer");
    if ((B2 + 63) / 64 > 0x7fffffffLL || (B1 + 63) / 64 > 65535) return fail(D3F_ERR_BAD_SHAPE, "pairwise_softmax_local: B1=%lld exceeds 64*65535 rows per call", (long long)B1);
    if (B1 > 0 && (!workspace || workspace_bytes < d3f_softmax_workspace_bytes(B1, B2)))
        return fail(D3F_ERR_WORKSPACE, "pairwise_softmax_local: needs %lld workspace bytes", (long long)d3f_softmax_workspace_bytes(B1, B2));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    if (B1 > 0) {
        e = d3f::launch_pairwise_dist(src, tgt, B1, B2, C, dist_type, out, s, softmax_stats(workspace, B1, B2), scale);
        if (e != hipSuccess) return hip_fail(e, "pairwise_dist launch");
    }
    e = d3f::launch_softmax_local_stats(out, B1, B2, scale, row_offset, softmax_stats(workspace, B1, B2),
                                        reinterpret_cast<d3f::ColStat *>(stats), true, s);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "softmax statistics launch");
}

int d3f_softmax_merge(const d3f_col_stat *parts, int64_t n_parts, int64_t cols, d3f_col_stat *merged, int64_t *argmax_out,
                      void *stream)
{
    if (n_parts < 0 || cols < 0) return fail(D3F_ERR_BAD_SHAPE, "softmax_merge: n_parts=%lld cols=%lld", (long long)n_parts, (long long)cols);
    if (cols == 0) return D3F_OK;
    if (!merged || (n_parts > 0 && !parts)) return fail(D3F_ERR_INVALID_ARG, "softmax_merge: NULL pointer");
    hipError_t e = d3f::launch_softmax_merge(reinterpret_cast<const d3f::ColStat *>(parts), n_parts, cols,
                                             reinterpret_cast<d3f::ColStat *>(merged), argmax_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "softmax merge launch");
}

int d3f_softmax_apply(float *x, int64_t rows, int64_t cols, float scale, const d3f_col_stat *merged, void *stream)
{
    if (rows < 0 || cols < 0) return fail(D3F_ERR_BAD_SHAPE, "softmax_apply: rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return D3F_OK;
    if (!x || !merged) return fail(D3F_ERR_INVALID_ARG, "softmax_apply: NULL pointer");
    hipError_t e = d3f::launch_softmax_apply(x, rows, cols, scale, reinterpret_cast<const d3f::ColStat *>(merged),
                                             static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "softmax apply launch");
}

// ---- rigid tracking step (fusion.py:1643-1665) -----------------------------------------------------------------------
int d3f_rigid_transform(const float *last, int32_t n_inst, int32_t n, const float *t, const float *w, float *out_pts,
                        float *norms, void *stream)
{
    if (n_inst < 0 || n < 0 || (int64_t)n_inst * n > 0x7fffffffLL) return fail(D3F_ERR_BAD_SHAPE, "rigid_transform: n_inst=%d n=%d", n_inst, n);
    if (!norms || (n_inst > 0 && (!t || !w)) || ((int64_t)n_inst * n > 0 && (!last || !out_pts)))
        return fail(D3F_ERR_INVALID_ARG, "rigid_transform: NULL pointer");
    hipError_t e = d3f::launch_rigid_transform(last, n_inst, n, t, w, 1e-4f, out_pts, norms, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "rigid_transform launch");
}

int d3f_track_loss_grad(const float *feats, const float *src, const float *dist, const uint8_t *valid, int64_t N, int32_t C,
                        float dist_w, float *grad_feats, float *grad_dist, float *loss, void *stream)
{
    if (N < 0 || N > 0x7fffffffLL || C < 1) return fail(D3F_ERR_BAD_SHAPE, "track_loss_grad: N=%lld C=%d", (long long)N, C);
    if (!loss || (N > 0 && (!feats || !src || !dist || !valid || !grad_feats || !grad_dist)))
        return fail(D3F_ERR_INVALID_ARG, "track_loss_grad: NULL pointer");
    hipError_t e = d3f::launch_track_loss_grad(feats, src, dist, valid, (int)N, C, dist_w, grad_feats, grad_dist, loss,
                                               static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "track_loss_grad launch");
}

int d3f_rigid_update(const float *last, int32_t n_inst, int32_t n, const float *grad_pts, float *t, float *w, float *adam_m,
                     float *adam_v, float *step, const float *norms, float reg_w, float lr, float beta1, float beta2, float eps,
                     void *stream)
{
    if (n_inst < 0 || n < 0) return fail(D3F_ERR_BAD_SHAPE, "rigid_update: n_inst=%d n=%d", n_inst, n);
    if (n_inst == 0) return D3F_OK;
    if (!t || !w || !adam_m || !adam_v || !step || !norms || (n > 0 && (!last || !grad_pts)))
        return fail(D3F_ERR_INVALID_ARG, "rigid_update: NULL pointer");
    if (!(lr > 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f))
        return fail(D3F_ERR_INVALID_ARG, "rigid_update: lr=%g beta=(%g,%g) eps=%g", lr, beta1, beta2, eps);
    hipError_t e = d3f::launch_rigid_update(last, n_inst, n, grad_pts, t, w, adam_m, adam_v, step, norms, 1e-4f, reg_w, lr, beta1,
                                            beta2, eps, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? D3F_OK : hip_fail(e, "rigid_update launch");
}

int64_t d3f_track_step_scratch_bytes(int32_t n_inst, int32_t n)
{
    if (n_inst < 0 || n < 0) return 0;
    // gradients [n_inst*n*3], loss slots [4], arrival counter [2] (floats / words), then the tagged parameter words [n_inst*6] (8 bytes each)
    return (((int64_t)n_inst * n * 3 + 6) * (int64_t)sizeof(float) + 7) / 8 * 8 + (int64_t)n_inst * 6 * 8;
}

int64_t d3f_track_stall_word(int32_t n_inst, int32_t n) { return (n_inst < 0 || n < 0) ? 0 : (int64_t)n_inst * n * 3 + 5; }      // counter[1]

static int track_impl(const d3f_views *views, const d3f_channel_map *descriptors, const float *last, int32_t n_inst, int32_t n,
                      const float *src, float mu, float dist_w, float reg_w, float lr, float beta1, float beta2, float eps,
                      int32_t iters, const d3f_track_state *state, void *stream)
{
    int rc = check_views(views);
    if (rc != D3F_OK) return rc;
    if (n_inst < 0 || n < 0) return fail(D3F_ERR_BAD_SHAPE, "track_step: n_inst=%d n=%d", n_inst, n);
    if (iters < 0) return fail(D3F_ERR_INVALID_ARG, "track_run: iters=%d", iters);
    if ((int64_t)n_inst * n == 0 || iters == 0) return D3F_OK;
    if ((int64_t)n_inst * n > 0x7fffffLL) return fail(D3F_ERR_BAD_SHAPE, "track_step: %lld keypoints (one workgroup each) are too many", (long long)n_inst * n);
    if (iters > 1 && ((int64_t)n_inst * n > d3f::track_run_capacity() || n_inst > 16))
        return fail(D3F_ERR_BAD_SHAPE, "track_run: %lld keypoints of %d instances; the steps of one launch wait for one another, so every "
                                       "workgroup must be resident (<= %d keypoints on this device, <= 16 instances); call d3f_track_step per iteration",
                    (long long)n_inst * n, n_inst, d3f::track_run_capacity());
    if (!descriptors || !last || !src || !state) return fail(D3F_ERR_INVALID_ARG, "track_step: NULL pointer");
    if (!state->t || !state->w || !state->adam_m || !state->adam_v || !state->step || !state->out_pts || !state->loss || !state->scratch)
        return fail(D3F_ERR_INVALID_ARG, "track_step: NULL pointer in d3f_track_state");
    if (!(mu > 0.0f)) return fail(D3F_ERR_INVALID_ARG, "mu must be > 0");
    if (!(lr > 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f))
        return fail(D3F_ERR_INVALID_ARG, "track_step: lr=%g beta=(%g,%g) eps=%g", lr, beta1, beta2, eps);
    if (views->V > 8) return fail(D3F_ERR_BAD_SHAPE, "track_step: at most 8 views (V=%d); use the five-launch step", views->V);
    d3f::TrackStepParams P;
    int64_t map_bytes = 0;
    rc = fill_map(*descriptors, 0, views->V, nullptr, nullptr, nullptr, P.map, map_bytes);
    if (rc != D3F_OK) return rc;
    if (P.map.esize != 4 || P.map.C % 4 != 0 || P.map.C > 512 || (P.map.sx % 4) || (P.map.sy % 4) || (P.map.sv % 4) ||
        !aligned(descriptors->data, 16) || !aligned(src, 16))
        return fail(D3F_ERR_BAD_LAYOUT, "track_step: the descriptor map must be fp32 with C %% 4 == 0, C <= 512 and 16-byte aligned texels "
                                        "(C=%d); use the five-launch step", P.map.C);
    P.depth = views->depth; P.K = views->K; P.pose = views->pose; P.V = views->V; P.H = views->H; P.W = views->W;
    P.last = last; P.src = src; P.I = n_inst; P.n = n; P.iters = iters;
    P.mu = mu; P.dist_w = dist_w; P.reg_w = reg_w; P.lr = lr; P.beta1 = beta1; P.beta2 = beta2; P.eps_adam = eps; P.eps_rot = 1e-4f;
    P.ln_beta1 = d3f::log_of_decimal(beta1); P.ln_beta2 = d3f::log_of_decimal(beta2);
    P.t = state->t; P.w = state->w; P.adam_m = state->adam_m; P.adam_v = state->adam_v; P.step = state->step;
    P.out_pts = state->out_pts; P.loss_out = state->loss;
    float *scr = static_cast<float *>(state->scratch);
    P.grad_pts = scr; P.loss_acc = scr + (int64_t)n_inst * n * 3; P.counter = reinterpret_cast<unsigned int *>(P.loss_acc + 4);
    P.par = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(state->scratch) + (((int64_t)n_inst * n * 3 + 6) * 4 + 7) / 8 * 8);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    hipError_t e = d3f::launch_track_step(P, hs);
    return e == hipSuccess ? D3F_OK : hip_fail(e, "track_step launch");
}

int d3f_track_step(const d3f_views *views, const d3f_channel_map *descriptors, const float *last, int32_t n_inst, int32_t n,
                   const float *src, float mu, float dist_w, float reg_w, float lr, float beta1, float beta2, float eps,
                   const d3f_track_state *state, void *stream)
{
    return track_impl(views, descriptors, last, n_inst, n, src, mu, dist_w, reg_w, lr, beta1, beta2, eps, 1, state, stream);
}

int d3f_track_run(const d3f_views *views, const d3f_channel_map *descriptors, const float *last, int32_t n_inst, int32_t n,
                  const float *src, float mu, float dist_w, float reg_w, float lr, float beta1, float beta2, float eps,
                  int32_t iters, const d3f_track_state *state, void *stream)
{
    return track_impl(views, descriptors, last, n_inst, n, src, mu, dist_w, reg_w, lr, beta1, beta2, eps, iters, state, stream);
}

int32_t d3f_track_run_max_keypoints(void) { return d3f::track_run_capacity(); }

}  // extern "C"
