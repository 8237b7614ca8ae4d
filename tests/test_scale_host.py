"""CPU: the workload-sized cases of tests/scale_cases.py before they meet a kernel.

  1. The shapes cross the thresholds the launch code has, and the *_workspace_bytes entry points agree with the restated scratch layout.
  2. Every fast reference equals the slow one the project already trusts (ccl_cases, pool_cases, edt_cases, volume_cases) on that module's own
     small cases -- exactly.  The band marks, the cost-to-go and the mesh use band_cases.mark, geodesic_cases.travel_ref / next_ref / dist_ref
     and mesh_ref.reference_mesh themselves: they are vectorised and affordable at 4 M voxels.
  3. Each comparison of tests/test_gpu_scale.py rejects the NumPy emulation of the mistake its branch invites, on the committed shapes.  The
     emulations never run on the device: a wrong offset there is a stray write.
"""
import time

import numpy as np
import pytest

import band_cases as BC
import ccl_cases as CC
import edt_cases as EC
import geodesic_cases as GC
import pool_cases as PC
import scale_cases as SC
import volume_cases as VC
from d3fields_amd import _lib

NA, NB = SC.voxels(SC.A), SC.voxels(SC.B)


# ---- 1. thresholds --------------------------------------------------------------------------------------------------------------------
def test_the_shapes_cross_the_thresholds():
    assert NA == 4251366 > SC.SCAN_BLOCK ** 2 == SC.SPLIT and SC.scan_levels(NA) == [NA, 2076, 2]
    assert NA % SC.SCAN_BLOCK == 1766 and 2076 % SC.SCAN_BLOCK == 28                      # ragged last workgroups at levels 1 and 2
    assert 158 * SC.A[1] * SC.A[2] <= SC.SCAN_BLOCK ** 2                                  # three x planes fewer would stay at two levels
    assert SC.tiles(SC.A) == (21, 21, 21) and 21 ** 3 > 2 * SC.GEO_MAX_GRID               # a third turn for some workgroups
    nb = (NA + SC.MESH_BLOCK - 1) // SC.MESH_BLOCK
    assert nb == 4152 and SC.scan_levels(nb + 1) == [4153, 3] and 4153 % SC.SCAN_BLOCK == 57
    assert all(64 < s <= 256 and s % 8 and s % 64 for s in SC.A)                           # long z kernel, LDS line pass with 64 lines, ragged everywhere
    assert SC.turns(NA) == (33, 504) and SC.turns(NB) == (64, 519) and NB > 64 * SC.SPAN >= SC.voxels((204, 204, 201))
    assert NB - 518 * 64 * 256 == 2548                                                     # the last workgroup of B is ragged
    assert NA * SC.ROW_CHANNELS > 2 ** 31 > (NA * SC.ROW_CHANNELS) // 2 and 2 ** 31 // SC.ROW_CHANNELS == 2 ** 22 < NA
    assert SC.sort_passes(65535) == 2 and SC.sort_passes(65536) == 3


def test_workspace_bytes_follow_the_restated_layout():
    lib = _lib.load()
    assert SC.scan_scratch_bytes(NA) == (2076 * 4 + 255) // 256 * 256 + 256 + 256 == 8960   # two levels of totals: 2076 words, then 2
    assert lib.d3f_band_workspace_bytes(*SC.A) == SC.scan_scratch_bytes(NA)
    assert lib.d3f_band_workspace_bytes(158, 162, 163) == SC.scan_scratch_bytes(158 * 162 * 163) < SC.scan_scratch_bytes(NA)      # one level of totals fewer
    for shape in (SC.A, SC.B):
        n = SC.voxels(shape)
        assert lib.d3f_volume_components_workspace_bytes(*shape) == 12 * n + SC.scan_scratch_bytes(n)
        assert lib.d3f_volume_edt_workspace_bytes(*shape) == 4 * n + 2 * ((n + 1) // 2 * 2)
        t = SC.tiles(shape)
        assert lib.d3f_volume_geodesic_workspace_bytes(*shape) == 4 * (16 + 2 * t[0] * t[1] * t[2])
    nb = (NA + SC.MESH_BLOCK - 1) // SC.MESH_BLOCK
    assert lib.d3f_mesh_workspace_bytes(*SC.A) == 2 * (((nb + 1) * 4 + 255) // 256 * 256) + SC.scan_scratch_bytes(nb + 1)
    for K, cap, ch in ((232205, 1300000, 7), (65536, NA, 0), (2047, 5000, 512), (2048, 70000, 3)):
        assert lib.d3f_volume_pool_workspace_bytes(*SC.A, K, cap, ch) == SC.pool_layout_bytes(NA, K, cap, ch), (K, cap, ch)
    assert SC.scan_levels(2047 + 1) == [2048] and SC.scan_levels(2048 + 1) == [2049, 2]


# ---- 2. the fast references equal the slow ones ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 70000, SC.SPLIT, SC.SPLIT + 1, NA])
def test_scan_model_is_the_cumulative_sum(n):
    x = np.random.default_rng(n).integers(0, 3, n)
    want = np.cumsum(x) - x
    assert np.array_equal(SC.scan_model(x), want)
    assert np.array_equal(SC.scan_model(x, "last total dropped"), want), "an exclusive scan never reads the last workgroup's total"
    rank, lst, count = SC.compact_model(x > 0)
    assert count == int((x > 0).sum()) and np.array_equal(lst, np.flatnonzero(x))


def same_components(a, b):
    return np.array_equal(a["label"], b["label"]) and (a["K"], a["found"]) == (b["K"], b["found"]) and np.array_equal(a["stats"], b["stats"]) \
        and np.array_equal(a["sizes_all"], b["sizes_all"])


@pytest.mark.parametrize("name", CC.CASES)
def test_scipy_label_equals_the_restatement(name):
    for conn in CC.CONNECTIVITIES:
        assert same_components(SC.components_fast(CC.site_volume(name), conn), CC.reference(name, conn)), (name, conn)


@pytest.mark.parametrize("case", CC.MIN_VOXELS, ids=lambda c: "%s conn %d m %d" % c)
def test_scipy_label_with_min_voxels(case):
    name, conn, m = case
    assert same_components(SC.components_fast(CC.site_volume(name), conn, m), CC.reference(name, conn, m))


@pytest.mark.parametrize("name", list(PC.VOLUMES))
def test_fast_pooling_equals_the_restatement(name):
    label, K = PC.volume(name)
    n = label.size
    valid = (np.random.default_rng(3).random(label.shape) < 0.8).astype(np.uint8)
    for v in (None, valid):
        assert np.array_equal(SC.members_fast(label, K, v)[3], PC.counts_ref(label, K, v))
        assert np.array_equal(SC.moments_fast(label, K, v), PC.moments_ref(label, K, v))
        for C in (1, 4, 5):
            rows = PC.field_rows(n, C, 40 + C)
            fill = PC.field_rows(1, C, 7)[0]
            got, want = SC.pool_fast(label, K, rows, v, fill), PC.pool_ref(label, K, rows, v, None, fill)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, C)
            mean64, abs64 = SC.pool_mean64(label, K, rows, v)
            counts = PC.counts_ref(label, K, v)
            live = counts > 0
            assert np.all(np.abs(want[live] - mean64[live]) <= SC.fold_bound(counts[live])[:, None] * abs64[live]), (name, C, "the fold against float64")
        votes = PC.vote_rows(n, 6, 44)
        assert np.array_equal(SC.votes_fast(label, K, votes, v), PC.votes_ref(label, K, votes, v))


def test_fast_fold_with_negative_zero_and_many_levels():
    rows = np.full((70000, 2), -0.0, np.float32)
    got = SC.fold_fast(rows, [65537, 0, 1, 4462])
    assert np.signbit(got[[0, 2, 3]]).all() and not got.any() and not np.signbit(got[1]).any()
    rows = PC.field_rows(70000, 3, 5)
    got = SC.fold_fast(rows, [65537, 0, 1, 4462])
    for k, a, b in ((0, 0, 65537), (2, 65537, 65538), (3, 65538, 70000)):
        assert np.array_equal(got[k].view(np.int32), PC.fold(rows[a:b]).view(np.int32)), k
    assert not got[1].any()


@pytest.mark.parametrize("name", EC.CASES)
def test_scipy_feature_transform_equals_the_restatement(name):
    site = EC.site_volume(name)
    d2 = SC.edt_fast(site)
    assert d2.dtype == np.int32 and np.array_equal(d2, EC.true_d2(name)), name


@pytest.mark.parametrize("channels", [(3,), (20,), (3, 68)])
def test_corner_chain_equals_volume_cases(channels):
    """blend64 / blend32 / grad64 / grad32 on gathered corner rows are volume_cases' functions on whole volumes, bit for bit"""
    vol, pts, ref = VC.case("5x4x6", channels, 1003, 2)
    assert ref["valid"].all()
    port = VC.trilinear32(vol, pts)
    shape = vol["shape"]
    i, t = SC.locate_cells(shape, vol["origin"], vol["step"], pts)
    i32, t32 = SC.locate_cells(shape, vol["origin"], vol["step"], pts, np.float32)
    assert np.array_equal(i, VC.locate64(vol, pts)[1]) and np.array_equal(t, VC.locate64(vol, pts)[2]) and np.array_equal(t32, VC.locate32(vol, pts)[2])
    vox = SC.corner_voxels(shape, i)
    rng = np.random.default_rng(1)
    for k, arr in vol["sets"].items():
        v = arr.reshape(-1, arr.shape[3])[vox]
        val, Aq, S = SC.blend64(v, t)
        assert np.array_equal(val, ref[k][0]) and np.array_equal(Aq, ref[k][1]) and np.array_equal(S, ref[k][2])
        assert np.array_equal(SC.blend32(v, t32).view(np.int32), port[k].view(np.int32))
        g = rng.standard_normal((len(pts), arr.shape[3])).astype(np.float32)
        want = VC.trilinear_grad64(vol, pts, None, {k: g})
        got = SC.grad64(v, t, g, float(vol["step"]))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(SC.grad32(v, t32, g, vol["step"]).view(np.int32), VC.trilinear_grad32(vol, pts, None, {k: g}).view(np.int32))


# ---- the cases hold what the GPU tests say of them, within the time budget ------------------------------------------------------------------
def test_case_conditions_and_reference_times():
    """Every reference of a GPU test is built and timed here (printed with -s; 0.1 to 9 s each where this was written), and the properties the
    GPU tests rely on are asserted on it."""
    times = {}

    def timed(name, f):
        t0 = time.perf_counter()
        out = f()
        times[name] = time.perf_counter() - t0
        return out

    a = timed("components A (scipy label, 6)", lambda: SC.ccl_reference("A"))
    b = timed("components B (scipy label, 26)", lambda: SC.ccl_reference("B"))
    assert a["K"] >= 65536 and a["sizes_all"].max() > 10000
    big = b["stats"][np.argmax(b["stats"][:, 1])]
    assert big[2:5].tolist() == [0, 0, 0] and big[5:8].tolist() == [s - 1 for s in SC.B] and (b["sizes_all"] == 1).sum() > 10000
    m3 = SC.ccl_reference("A", 3)
    assert 0 < m3["K"] < a["K"] and m3["found"] == a["found"] and {2, 3, 4} <= set(a["sizes_all"].tolist())
    case = SC.pool_case("A")
    timed("pool A (fold, 2 sets)", lambda: [SC.pool_fast(case["label"], case["K"], r, case["valid"]) for r in case["rows"]])
    timed("pool A (moments, votes)", lambda: (SC.moments_fast(case["label"], case["K"], case["valid"]), SC.votes_fast(case["label"], case["K"], case["votes"], case["valid"])))
    d2 = timed("distance transform A (scipy)", SC.edt_reference)
    assert int(d2.max()) > 35 ** 2
    free, seeds = SC.travel_case()
    assert len(seeds) == 9261 and len(GC.accepted_seeds(free, seeds)) == 9261 - 441 and len(SC.listed_after_init(free, seeds)) > SC.GEO_MAX_GRID
    for conn, w in SC.GEO_CONFIGS:
        cost, _, sweeps = timed("cost-to-go A (%d, %s)" % (conn, w), lambda: SC.travel_reference(conn, w))
        reached = cost != SC.INT32_MAX
        assert sweeps <= 24 and reached[free != 0].mean() > 0.9999 and not reached[free == 0].any()
    vol = timed("band volume A", lambda: SC.band_volume(True))
    m = timed("band mark A (cumsum)", lambda: BC.mark(vol, SC.band_length(vol)))
    assert 0.05 < BC.kept_share(m) < 0.10 and (m["voxels"] >= SC.SPLIT).sum() > 1000
    pts = SC.band_points(vol, m["cell_band"])
    timed("band sample A (float64 + port)", lambda: (VC.trilinear64(vol, pts), VC.trilinear32(vol, pts)))
    for kind in ("sphere", "clipped"):
        k, _, tri = timed("mesh A %s (mesh_ref)" % kind, lambda: SC.mesh_reference(kind))
        assert k.size > 50000 and (k // 3 >= 2048 * SC.MESH_BLOCK).any() and (k // 3 < 2048 * SC.MESH_BLOCK).any()      # vertices on both sides of the second scan workgroup
    print()
    for name, t in times.items():
        print("  %-36s %6.2f s" % (name, t))


# ---- 3. the emulated mistakes are rejected ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", SC.SCAN_MUTANTS)
def test_a_wrong_scan_is_rejected_by_every_scan_dependent_comparison(mutant):
    # band: slot, voxels, count
    vol = SC.band_volume()
    m = BC.mark(vol, SC.band_length(vol))
    stored = m["stored"].reshape(-1)
    rank, lst, count = SC.compact_model(stored, mutant)
    slot = np.where(stored, rank, -1).astype(np.int32).reshape(vol["shape"])
    assert not np.array_equal(slot, m["slot"]), "slot"
    assert count != m["M"] or not np.array_equal(lst, m["voxels"]), "voxels"
    # components: the rank of every kept root numbers the labels
    ref = SC.ccl_reference("A")
    flags = np.zeros(NA, np.int64)
    flags[ref["stats"][:, 0]] = 1
    rank = SC.scan_model(flags, mutant)
    lab = ref["label"].reshape(-1)
    mut = np.where(lab > 0, rank[ref["stats"][np.maximum(lab, 1) - 1, 0]] + 1, 0)
    assert not np.array_equal(mut, lab), "labels"
    # pooling: the member list in flat order
    case = SC.pool_case("A")
    ok, idx, keys, counts = SC.members_fast(case["label"], case["K"], case["valid"])
    _, lst, count = SC.compact_model(ok, mutant)
    assert count != int(ok.sum()) or not np.array_equal(lst, np.flatnonzero(ok)), "members"
    # mesh: where a vertex lands
    keys = SC.mesh_reference("sphere")[0]
    pos, total = SC.mesh_offsets_model(keys, NA, mutant)
    good, good_total = SC.mesh_offsets_model(keys, NA)
    assert np.array_equal(good, np.arange(keys.size)) and good_total == keys.size
    if mutant == "ragged last workgroup dropped":                     # (the mesh scan has two levels: no third to forget)
        assert not np.array_equal(pos, good) or total != good_total, "vertex keys"


def test_a_truncated_tile_loop_is_rejected_behind_the_solid_layer():
    free, seeds = SC.travel_case()
    cost = SC.travel_reference(6, (1, 1, 1))[0]
    assert SC.tile_loop_model(free, seeds).all(), "the whole list every round: every tile runs"
    ran = SC.tile_loop_model(free, seeds, SC.GEO_MAX_GRID)
    t = SC.tiles(SC.A)
    assert not ran.reshape(t)[SC.GEO_SLAB[1] // SC.TILE:].any() and ran.reshape(t)[:SC.GEO_SLAB[0] // SC.TILE].all()
    mut = SC.unrun_tiles_cost(cost, free, seeds, ran)
    assert int((mut != cost).sum()) > 1000000
    # without the solid layer the truncated loop heals itself: a neighbour that lowers a voxel beside a dropped tile lists it again.  That is
    # why the case has the layer -- on connected free space no output can show this mistake.
    joined = np.array(free)
    joined[SC.GEO_SLAB[0]:SC.GEO_SLAB[1]] = 1
    assert SC.tile_loop_model(joined, seeds, SC.GEO_MAX_GRID).all()


def test_a_sort_that_stops_after_two_passes_is_rejected():
    case = SC.pool_case("A")
    K = case["K"]
    ok, idx, keys, counts = SC.members_fast(case["label"], K, case["valid"])
    flat_order = np.flatnonzero(ok)                                   # the list before the sort
    k0 = case["label"].reshape(-1)[flat_order].astype(np.int64)
    full = SC.sort_model(k0, SC.sort_passes(K))
    assert SC.sort_passes(K) == 3 and np.array_equal(flat_order[full], idx) and np.array_equal(k0[full], keys)
    two = SC.sort_model(k0, 2)
    assert not np.array_equal(k0[two], keys)
    # what the fold would read: component k's members are list[first[k] : first[k] + count[k]]
    x = np.unravel_index(flat_order[two], case["label"].shape)[0].astype(np.int64)
    first = np.cumsum(counts) - counts
    live = counts > 0
    sx = np.add.reduceat(x, first[live])
    assert not np.array_equal(sx, SC.moments_fast(case["label"], K, case["valid"])[live, 0]), "moments"
    r = case["rows"][0][flat_order[two]]
    mut = SC.fold_fast(r, counts)
    want = SC.fold_fast(case["rows"][0][idx], counts)
    assert int((mut.view(np.int32) != want.view(np.int32)).any(axis=1).sum()) > 1000, "means"


def test_a_32_bit_row_offset_is_rejected():
    pts, cells = SC.row_points()
    vol = {"origin": np.asarray(VC.ORIGIN, np.float32), "step": np.float32(VC.STEP), "shape": SC.A}
    i, t = SC.locate_cells(SC.A, VC.ORIGIN, VC.STEP, pts)
    assert np.array_equal(i, cells)
    vox = SC.corner_voxels(SC.A, i)
    past = (vox >= 2 ** 22).any(axis=0)
    assert past.sum() > 1500 and (~past).sum() > 1500
    wrapped = SC.wrapped_voxel(vox, SC.ROW_CHANNELS, NA)
    assert np.array_equal(wrapped[:, ~past], vox[:, ~past]) and (wrapped[vox >= 2 ** 22] != vox[vox >= 2 ** 22]).all()
    C = 8
    val, Aq, S = SC.blend64(SC.virtual_rows(vox, C), t)
    mut = SC.blend64(SC.virtual_rows(wrapped, C), t)[0]
    bound = 16.0 * VC.U                                               # the cap of volume_cases.tolerance
    per_point = np.max((np.abs(mut - val) - VC.coord_term(vol, S)) / Aq, axis=1)
    assert (per_point[past] > 1000 * bound).mean() > 0.99 and per_point[~past].max() <= 0
    g = SC.virtual_rows(np.arange(len(pts)), C, salt=7)
    want, Bq, T = SC.grad64(SC.virtual_rows(vox, C), t, g, float(VC.STEP))
    mutg = SC.grad64(SC.virtual_rows(wrapped, C), t, g, float(VC.STEP))[0]
    assert VC.worst_ratio(mutg[past], want[past], Bq[past], VC.grad_coord_term(vol, T[past])[:, None]) > 1000 * bound
    # the pooled means: both components have members beyond voxel 2^22
    for m in SC.row_pool_members():
        assert (m >= 2 ** 22).sum() >= 1000 and np.all(np.diff(m) > 0)
        a, b = PC.fold(SC.virtual_rows(m, C)), PC.fold(SC.virtual_rows(SC.wrapped_voxel(m, SC.ROW_CHANNELS, NA), C))
        assert not np.array_equal(a.view(np.int32), b.view(np.int32))
