// layout_check.cpp -- a stand-alone host program: every workspace layout function of csrc/ over the argument table of tests/workspace_args.py.
// For every row the public size function accepts, the layout's regions must start at 0, follow each other in the order of the struct, end at or
// before `total`, and `total` must be what the size function returns; a round of farthest point sampling must not launch more workgroups
// (fps_blocks) than its table of maxima has entries per round parity.  Meant to be built with the host side under AddressSanitizer and
// UndefinedBehaviorSanitizer (the level arrays of scan_layout / topk_layout, the int64 products); it launches nothing and needs no device.
//
//   python tests/workspace_args.py --rows > rows.txt
//   for f in d3fields_amd/csrc/*.hip; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//           -I include -I d3fields_amd/csrc -c $f -o obj/$(basename $f .hip).o; done
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include -I d3fields_amd/csrc -x hip tests/layout_check.cpp -c -o obj/layout_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined obj/*.o -o layout_check && ./layout_check rows.txt
#include <algorithm>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "d3f_internal.h"

using namespace d3f;
typedef std::vector<int64_t> Row;

static int g_bad = 0, g_checked = 0, g_rejected = 0;

// offs: the regions in the order the layout takes them
static void check(const std::string &fn, const Row &a, const char *layout, const std::vector<int64_t> &offs, int64_t total, int64_t want_total)
{
    bool ok = !offs.empty() && offs[0] == 0 && total == want_total && offs.back() <= total;
    for (size_t i = 1; i < offs.size(); ++i) ok = ok && offs[i - 1] <= offs[i];
    ++g_checked;
    if (ok) return;
    ++g_bad;
    std::cout << "BAD " << fn << "(";
    for (int64_t v : a) std::cout << " " << v;
    std::cout << " ) " << layout << ": total " << total << ", the size function " << want_total << ", offsets";
    for (int64_t v : offs) std::cout << " " << v;
    std::cout << "\n";
}

static std::vector<int64_t> scan_fields(const ScanLayout &L, int64_t base)
{
    std::vector<int64_t> o;
    for (int l = 0; l < L.levels; ++l) o.push_back(base + L.sums[l]);
    o.push_back(base + L.spare);
    return o;
}

static std::vector<int64_t> pool_fields(const PoolLayout &L, int64_t base)
{
    std::vector<int64_t> o = {L.flag, L.flag_scan, L.keys[0], L.vals[0], L.keys[1], L.vals[1], L.counters, L.counters_scan, L.first, L.work[0], L.work[1],
                              L.work[2], L.work[3], L.part[0], L.part[1], L.part[2], L.plan_scan, L.rows[0], L.rows[1]};
    for (int64_t &v : o) v += base;
    return o;
}

static void one(const std::string &fn, const Row &a)
{
    auto vol = [&]() { return a[0] * a[1] * a[2]; };
    int64_t want = 0;
    d3f_views views = {};
    d3f_grid grid = {};
    if (fn == "d3f_eval_workspace_bytes") want = d3f_eval_workspace_bytes(a[0]);
    else if (fn == "d3f_eval_gate_offset") want = d3f_eval_gate_offset(a[0]);
    else if (fn == "d3f_eval_dist_workspace_bytes") {
        views.V = (int32_t)a[0]; views.H = (int32_t)a[1]; views.W = (int32_t)a[2];
        want = d3f_eval_dist_workspace_bytes(a[0] == -1 && a[1] == -1 ? nullptr : &views, a[3]);
    } else if (fn == "d3f_grid_shell_workspace_bytes") {
        grid.nx = (int32_t)a[0]; grid.ny = (int32_t)a[1]; grid.nz = (int32_t)a[2];
        want = d3f_grid_shell_workspace_bytes(a[0] == -1 && a[1] == -1 ? nullptr : &grid);
    } else if (fn == "d3f_mesh_workspace_bytes") want = d3f_mesh_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_volume_gaussian_workspace_bytes") want = d3f_volume_gaussian_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_band_workspace_bytes") want = d3f_band_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_volume_edt_workspace_bytes") want = d3f_volume_edt_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_volume_components_workspace_bytes") want = d3f_volume_components_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_volume_geodesic_workspace_bytes") want = d3f_volume_geodesic_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2]);
    else if (fn == "d3f_volume_pool_workspace_bytes") want = d3f_volume_pool_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2], (int32_t)a[3], a[4], a[5]);
    else if (fn == "d3f_part_motion_workspace_bytes") want = d3f_part_motion_workspace_bytes((int32_t)a[0], (int32_t)a[1], (int32_t)a[2], (int32_t)a[3], a[4]);
    else if (fn == "d3f_volume_align_workspace_bytes") want = d3f_volume_align_workspace_bytes(a[0], a[1]);
    else if (fn == "d3f_pose_consensus_workspace_bytes") want = d3f_pose_consensus_workspace_bytes((int32_t)a[0], (int32_t)a[1], a[2], a[3]);
    else if (fn == "d3f_fps_workspace_bytes") want = d3f_fps_workspace_bytes(a[0]);
    else if (fn == "d3f_fps_pixels_workspace_bytes") want = d3f_fps_pixels_workspace_bytes(a[0]);
    else if (fn == "d3f_backproject_workspace_bytes") want = d3f_backproject_workspace_bytes((int32_t)a[0], (int32_t)a[1]);
    else if (fn == "d3f_vox_iou_workspace_bytes") want = d3f_vox_iou_workspace_bytes(a[0], a[1]);
    else if (fn == "d3f_voxel_downsample_workspace_bytes") want = d3f_voxel_downsample_workspace_bytes(a[0]);
    else if (fn == "d3f_softmax_workspace_bytes") want = d3f_softmax_workspace_bytes(a[0], a[1]);
    else if (fn == "d3f_pairwise_topk_workspace_bytes") want = d3f_pairwise_topk_workspace_bytes(a[0], a[1]);
    else if (fn == "d3f_row_moments_workspace_bytes") want = d3f_row_moments_workspace_bytes(a[0], (int32_t)a[1]);
    else { std::cout << "BAD unknown function " << fn << "\n"; ++g_bad; return; }
    if (want == 0) { ++g_rejected; return; }        // a rejected row: the guards in front of the layout answered

    if (fn == "d3f_eval_workspace_bytes" || fn == "d3f_eval_gate_offset") {
        const OrderLayout L = order_layout(a[0]);
        if (fn == "d3f_eval_gate_offset") check(fn, a, "order_layout.gate", {L.keys, L.gate}, L.gate, want);
        else check(fn, a, "order_layout", {L.keys, L.ranks, L.order, L.slots, L.table, L.scan, L.gate, L.parts}, L.total, want);
        check(fn, a, "order_layout.scan", scan_fields(scan_layout(1 << 21), 0), L.gate - L.scan, scan_scratch_bytes(1 << 21));
    } else if (fn == "d3f_grid_shell_workspace_bytes") {
        const ShellLayout L = grid_shell_layout(vol());
        check(fn, a, "grid_shell_layout", {L.ballots, L.counts, L.offsets, L.scan}, L.total, want);
        check(fn, a, "grid_shell_layout.scan", scan_fields(scan_layout(L.blocks), 0), L.total - L.scan, scan_scratch_bytes(L.blocks));
        const ShellTiledLayout T = grid_shell_tiled_layout(vol(), 4915200);
        check(fn, a, "grid_shell_tiled_layout", {T.shell, T.tiles}, T.total, pad256(want) + 4915200);
        if (T.tiles != pad256(want)) check(fn, a, "grid_shell_tiled_layout.tiles", {T.tiles}, 0, 0);      // the header's rule
    } else if (fn == "d3f_mesh_workspace_bytes") {
        const MeshLayout L = mesh_layout(vol());
        check(fn, a, "mesh_layout", {L.voff, L.toff, L.scan}, L.total, want);
    } else if (fn == "d3f_band_workspace_bytes") {
        const ScanLayout L = scan_layout(vol());
        check(fn, a, "scan_layout", scan_fields(L, 0), L.total, want);
    } else if (fn == "d3f_volume_edt_workspace_bytes") {
        const EdtLayout L = edt_layout(vol());
        check(fn, a, "edt_layout", {L.B, L.A}, L.total, want);
    } else if (fn == "d3f_volume_components_workspace_bytes") {
        const CclLayout L = ccl_layout(vol());
        check(fn, a, "ccl_layout", {L.parent, L.size, L.rank, L.scan}, L.total, want);
    } else if (fn == "d3f_volume_geodesic_workspace_bytes") {
        const GeoLayout L = geodesic_layout((int)a[0], (int)a[1], (int)a[2]);
        check(fn, a, "geodesic_layout", {L.header, L.flags, L.list}, L.total, want);
    } else if (fn == "d3f_volume_pool_workspace_bytes") {
        const PoolLayout L = pool_layout(vol(), a[3], std::min(a[4], vol()), a[5] > 0 ? a[5] + 3 * D3F_MAX_MAPS : 0);
        check(fn, a, "pool_layout", pool_fields(L, 0), L.total, want);
    } else if (fn == "d3f_part_motion_workspace_bytes") {
        const MotionLayout L = motion_layout(vol(), a[3], std::min(a[4], vol()));
        check(fn, a, "motion_layout", {L.lab, L.pool, L.sums, L.fsum, L.centre}, L.total, want);
        check(fn, a, "motion_layout.P", pool_fields(L.P, 0), L.P.total, L.P.total);
        if (L.pool + L.P.total > L.sums) check(fn, a, "motion_layout.pool", {L.pool}, L.P.total, L.sums - L.pool);
    } else if (fn == "d3f_volume_align_workspace_bytes") {
        const AlignLayout L = align_layout(a[0], a[1]);
        check(fn, a, "align_layout", {L.partial}, L.total, want);
    } else if (fn == "d3f_pose_consensus_workspace_bytes") {
        const ConsensusLayout L = consensus_layout(a[2] * a[1] * a[1] * a[1], a[3]);
        check(fn, a, "consensus_layout", {L.head, L.eq, L.fl, L.scan, L.surv_h, L.surv_count, L.alive, L.surv_assign}, L.total, want);
    } else if (fn == "d3f_fps_workspace_bytes" || fn == "d3f_fps_pixels_workspace_bytes") {
        const FpsLayout L = fps_layout(a[0], fn == "d3f_fps_workspace_bytes" ? 4 : 8);
        check(fn, a, "fps_layout", {L.dist, L.maxima}, L.total, want);
        // a round's workgroups each own one 16-byte entry of their parity's half of `maxima`: never more workgroups than entries
        const int64_t entries = (L.total - L.maxima) / (2 * 16);
        ++g_checked;
        if (entries != kFpsMaxBlocks || fps_blocks(a[0]) < 1 || fps_blocks(a[0]) > entries) {
            ++g_bad;
            std::cout << "BAD " << fn << "( " << a[0] << " ) fps_blocks: " << fps_blocks(a[0]) << " workgroups a round, fps_layout.maxima holds " << entries
                      << " entries per parity (kFpsMaxBlocks " << kFpsMaxBlocks << ")\n";
        }
    } else if (fn == "d3f_backproject_workspace_bytes") {
        const PixelCountsLayout L = pixel_counts_layout(a[0] * a[1]);
        check(fn, a, "pixel_counts_layout", {L.counts}, L.total, want);
    } else if (fn == "d3f_vox_iou_workspace_bytes") {
        const VoxsetLayout L = voxset_layout(a[0], a[1]);
        check(fn, a, "voxset_layout", {L.table}, L.total, want);
    } else if (fn == "d3f_voxel_downsample_workspace_bytes") {
        const VoxmeanLayout L = voxmean_layout(a[0]);
        check(fn, a, "voxmean_layout", {L.minb, L.table, L.counts, L.list}, L.total, want);
    } else if (fn == "d3f_softmax_workspace_bytes") {
        const SoftmaxLayout L = softmax_layout(a[0], a[1]);
        check(fn, a, "softmax_layout", {L.stats}, L.total, want);
    } else if (fn == "d3f_pairwise_topk_workspace_bytes") {
        const PairTopkLayout L = pair_topk_layout(a[0], a[1]);
        check(fn, a, "pair_topk_layout", {L.stats, L.topk, L.slack}, L.total, want);
        const TopkLayout T = topk_layout(a[0], a[1]);
        check(fn, a, "topk_layout", std::vector<int64_t>(T.list, T.list + T.levels), T.total, L.slack - L.topk);
        if (T.chunks[T.levels - 1] != 1 || T.items[0] != a[0]) check(fn, a, "topk_layout.levels", {1}, 0, 0);
        if (L.topk < softmax_layout(a[0], a[1]).total || L.slack == L.total || L.total - L.slack > 256) check(fn, a, "pair_topk_layout.slack", {1}, 0, 0);
    } else if (fn == "d3f_row_moments_workspace_bytes") {
        const MomentPlan p = moment_plan(a[0], (int)a[1]);
        check(fn, a, "moment_plan", {p.off_wsum, p.off_wsum_part, p.off_sum_part, p.off_col_part, p.off_tiles, p.off_m32}, p.bytes, want);
        if (p.off_m32 % 16 || p.bytes % 256 || p.off_m32 + (int64_t)p.cpad * 4 > p.bytes) check(fn, a, "moment_plan.m32", {1}, 0, 0);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::cerr << "usage: layout_check ROWS   (python tests/workspace_args.py --rows)\n"; return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int rows = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fn;
        Row a;
        int64_t v;
        ls >> fn;
        while (ls >> v) a.push_back(v);
        one(fn, a);
        ++rows;
    }
    std::cout << rows << " rows: " << g_rejected << " rejected by the size function, " << g_checked << " layouts checked, " << g_bad << " bad\n";
    return rows > 0 && g_bad == 0 ? 0 : 1;
}
