"""The baked-volume kernels at the sizes the product bakes: the smallest volumes that cross every size-dependent branch of their launch
code (tests/scale_cases.py has the arithmetic), against references that share nothing with the kernels -- numpy.cumsum / nonzero,
scipy.ndimage.label and distance_transform_edt, bincount, the float64 chain of tests/volume_cases.py, tests/mesh_ref.py, the Jacobi sweeps
of tests/geodesic_cases.py.  tests/test_scale_host.py pins every fast reference to the slow one of the matching *_cases.py on its small
cases, and shows that each comparison below rejects the emulated mistake it is there for.  No tolerance is new: integers are exact, floats
keep the bounds of test_gpu_volume.py (tol * A + the coordinate term, tol from the float32 port) and test_gpu_pool.py (the bits of the fold).

The branches, where they are first reached, and what ran them before this file (A = 161x162x163 = 4 251 366 voxels, B = 205x204x203 = 8 489 460):

  where                                        what changes with size                                first reached at            largest before   here
  scan_kernels.hip launch_exclusive_scan_u32   a recursion level per factor 2048                     3rd level: n > 4 194 304    262 144 (2)      A: 2076 / 2 / 1 workgroups
    band mark, components, pool flags          one word per voxel                                    volume > 4 194 304 voxels   2 workgroups     A
    pool plan.* scans                          K + 1 words, up to eight scans, one scratch           K + 1 > 2048                K = 300          A: K = 232 205 (2 levels)
    mesh_kernels.hip launch_mesh               n / 1024 + 1 workgroup totals                         n > 2 097 152 (2 levels)    1 level          A: 4153 totals, 3 workgroups
  pool_kernels.hip label sort                  1 / 2 / 3 passes for K < 256 / < 65 536 / >= 65 536   K >= 65 536                 K = 300 (2)      A: 3 passes
  pool_kernels.hip pool_level_kernel           a fold level per factor 256 of the largest component  > 256, > 65 536 members     65 537 (3)       A: 35 309 (2), rows: 66 000 (3)
  ccl_flatten / ccl_box / pool_flag kernels    min(64, ceil(n / 131 072)) turns, then a wider grid   n > 8 388 608               2 turns          A: 33 turns, B: 64 turns, 519 workgroups
  geodesic_kernels.hip geo_tile_kernel         ceil(listed / 4096) tiles per workgroup, LDS reused   > 4096 tiles listed         343 tiles        A: 8964 listed, 3 turns
  edt_kernels.hip z pass                       nz <= 64: one wave per line(s); longer: ballot words  nz > 64                     12 lines of 300  A: 26 082 lines of 163
  edt_kernels.hip line passes                  64 lines of <= 256 entries in LDS per workgroup       more than 64 lines          650 lines        A: 26 243 / 26 406 lines, ragged last workgroup
  volume_kernels.hip / pool_kernels.hip rows   voxel * stride                                        voxels * C > 2^31 floats    far below        A x 512 channels = 2.18 G floats

What catches what (each emulated in NumPy and rejected in tests/test_scale_host.py):
  a scan whose third-level offsets are not added back     slot / voxels (test_band_mark...), labels and stats (test_components[A]), members and moments (test_pool[A])
  a scan whose ragged last workgroup is dropped           the same three, and the vertex keys (test_mesh...: 4153 totals end in a ragged workgroup)
  a tile loop that runs only the first 4096 listed tiles  cost / next / dist behind the solid tile layer (test_cost_to_go...); the listed count is asserted > 4096
  a label sort that stops after two passes                moments, votes and means of test_pool[A] (K = 232 205 needs the third digit)
  a 32-bit voxel * stride                                 rows, gradients and means of test_rows_past_two_to_the_31 at voxels >= 2^22
  a held label flushed wrongly at the 64-turn cap         sizes and boxes of test_components[B] (one component spans the box), counts of test_pool_flags_at_the_turn_cap
"""
import ctypes

import numpy as np
import pytest
import torch

import band_cases as BC
import ccl_cases as CC
import edt_cases as EC
import geodesic_cases as GC
import pool_cases as PC
import scale_cases as SC
import volume_cases as VC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

MEAN, VOTES = _lib.POOL_MEAN, _lib.POOL_VOTES
STEP = 0.0125
GUARD = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(nbytes, dev):
    return torch.full((max(int(nbytes), 16),), 0xA5, dtype=torch.uint8, device=dev)


def field_of(vol, dev, with_sets=True):
    from d3fields_amd import BakedField
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()} if with_sets else {}
    fills = {k: torch.from_numpy(f).to(dev) for k, f in vol["fills"].items() if f is not None} if with_sets else {}
    return BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev),
                                  valid=torch.from_numpy(vol["valid"]).to(dev), fills=fills, **sets)


# ---- band -------------------------------------------------------------------------------------------------------------------------------
def run_mark(field, band):
    """one d3f_band_mark launch on poisoned outputs and workspace -> (cell_band, slot, voxels, count) as NumPy"""
    dev = field.device
    lib = _lib.load()
    nx, ny, nz = field.grid_shape
    n = nx * ny * nz
    cell_band = torch.full((nx - 1, ny - 1, nz - 1), 7, dtype=torch.uint8, device=dev)
    slot = torch.full((nx, ny, nz), -7, dtype=torch.int32, device=dev)
    voxels = torch.full((n + 5,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws_bytes = lib.d3f_band_workspace_bytes(nx, ny, nz)
    ws = poisoned(ws_bytes, dev)
    vol = field._volume()
    _lib.check(lib.d3f_band_mark(ctypes.byref(vol), float(band), _lib.ptr(cell_band), _lib.ptr(slot), _lib.ptr(voxels), n, _lib.ptr(count), _lib.ptr(ws), ws_bytes,
                                 _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return cell_band.cpu().numpy(), slot.cpu().numpy(), voxels.cpu().numpy(), int(count.item())


def test_band_mark_takes_the_third_scan_level(dev):
    vol = SC.band_volume()
    band = SC.band_length(vol)
    m = BC.mark(vol, band)
    assert SC.scan_levels(vol["dist"].size) == [4251366, 2076, 2] and int((m["voxels"] >= SC.SPLIT).sum()) > 1000
    f = field_of(vol, dev)
    cb, slot, vox, count = run_mark(f, band)
    assert count == m["M"], (count, m["M"])
    assert np.array_equal(cb.astype(bool), m["cell_band"]) and set(np.unique(cb)) <= {0, 1}
    assert np.array_equal(slot, m["slot"]), int((slot != m["slot"]).sum())
    assert np.array_equal(vox[:count], m["voxels"]) and np.all(vox[count:] == -7)
    again = run_mark(f, band)
    assert all(np.array_equal(a, b) for a, b in zip((cb, slot, vox), again[:3])) and again[3] == count, "two runs must agree byte for byte"
    b = f.to_band(float(band))                                          # the Python layer holds the same arrays
    assert np.array_equal(b.band_voxels.cpu().numpy(), m["voxels"]) and np.array_equal(b.slot.cpu().numpy(), m["slot"])


def test_band_sample_and_backward_either_side_of_the_split(dev):
    """4099 points in kept cells at the first voxels, the last voxels and either side of flat index 2048^2, and 99 outside the band: the float64
    reference and bound of test_gpu_volume.py on the rows the slot volume names; the dense field's bits where in the band"""
    vol = SC.band_volume(True)
    band = SC.band_length(vol)
    m = BC.mark(vol, band)
    pts = SC.band_points(vol, m["cell_band"])
    names = list(vol["sets"])
    ok_ref, ib_ref = BC.in_band(vol, m, pts)
    assert int(ib_ref.sum()) == 4000 and int((ok_ref & ~ib_ref).sum()) > 50
    dense = field_of(vol, dev)
    banded = dense.to_band(float(band))
    dpts = torch.from_numpy(pts).to(dev)
    out, want = banded.eval(dpts), dense.eval(dpts)
    torch.cuda.synchronize()
    assert np.array_equal(out["valid_mask"].cpu().numpy(), ok_ref) and np.array_equal(out["in_band"].cpu().numpy(), ib_ref)
    ref, port = VC.trilinear64(vol, pts), VC.trilinear32(vol, pts)
    has = {"dist": ok_ref, **{k: ib_ref for k in names}}
    port_worst = max(VC.worst_ratio(port[k][has[k]], ref[k][0][has[k]], ref[k][1][has[k]], VC.coord_term(vol, ref[k][2][has[k]])) for k in ["dist"] + names)
    tol = VC.tolerance(port_worst)
    got_worst = 0.0
    for k in ["dist"] + names:
        got = out[k].cpu().numpy()
        val, Aq, S = ref[k]
        assert not np.isnan(got).any(), k
        got_worst = max(got_worst, VC.worst_ratio(got[has[k]], val[has[k]], Aq[has[k]], VC.coord_term(vol, S[has[k]])))
        if k == "dist":
            assert np.all(got[~ok_ref] == VC.SENTINEL)
        else:
            fill = np.zeros(got.shape[1], np.float32) if vol["fills"][k] is None else vol["fills"][k]
            assert np.array_equal(got[~ib_ref], np.broadcast_to(fill, got[~ib_ref].shape)), (k, "fill row outside the band")
            assert torch.equal(out[k][out["in_band"]], want[k][out["in_band"]]), (k, "the dense field's bits where in the band")
    print("\n  band sample   N=%d  port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (len(pts), port_worst, tol, got_worst))
    assert got_worst <= tol, (got_worst, tol)
    # backward: the dist term at every valid point, a set's term only where in the band
    rng = np.random.default_rng(11)
    gd = rng.standard_normal(len(pts)).astype(np.float32)
    gs = {k: rng.standard_normal((len(pts), vol["sets"][k].shape[3])).astype(np.float32) for k in names}
    got = banded.backward(dpts, torch.from_numpy(gd).to(dev), {k: torch.from_numpy(g).to(dev) for k, g in gs.items()})
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    masked = {k: g * ib_ref[:, None] for k, g in gs.items()}
    want64, Bq, T = VC.trilinear_grad64(vol, pts, gd, masked)
    port = VC.trilinear_grad32(vol, pts, gd, masked)
    slack = VC.grad_coord_term(vol, T)[:, None]
    port_worst = VC.worst_ratio(port, want64, Bq, slack)
    tol = VC.tolerance(port_worst)
    got_worst = VC.worst_ratio(got, want64, Bq, slack)
    print("  band backward N=%d  port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (len(pts), port_worst, tol, got_worst))
    assert not np.isnan(got).any() and np.all(got[~ok_ref] == 0) and np.abs(got[ib_ref]).max() > 0
    assert got_worst <= tol, (got_worst, tol)


# ---- components -------------------------------------------------------------------------------------------------------------------------
def run_ccl(site, dev, connectivity, min_voxels, capacity):
    lib = _lib.load()
    nx, ny, nz = site.shape
    s = torch.from_numpy(np.array(site)).to(dev)
    poison = int(CC.POISON)
    label = torch.full((nx, ny, nz), poison, dtype=torch.int32, device=dev)
    count = torch.full((2,), poison, dtype=torch.int32, device=dev)
    stats = torch.full((capacity, 8), poison, dtype=torch.int32, device=dev)
    ws_bytes = lib.d3f_volume_components_workspace_bytes(nx, ny, nz)
    ws = poisoned(ws_bytes, dev)
    _lib.check(lib.d3f_volume_components(_lib.ptr(s), nx, ny, nz, connectivity, min_voxels, _lib.ptr(label), _lib.ptr(count), _lib.ptr(stats), capacity,
                                         _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return label.cpu().numpy(), count.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("which,min_voxels", [("A", 1), ("A", 3), ("B", 1)])
def test_components(dev, which, min_voxels):
    """A at the percolation density of connectivity 6: three scan levels over the rank volume, K >= 65 536.  B under connectivity 26: 64 turns per
    workgroup in the flatten and box kernels, one component that spans the box (its label is held across all 64 turns) among thousands of specks."""
    site, conn = SC.ccl_case(which)
    ref = SC.ccl_reference(which, min_voxels)
    print("\n  components %s: connectivity %d, K = %d of %d found, largest %d voxels, turns x workgroups %s" % (
        which, conn, ref["K"], ref["found"], int(ref["sizes_all"].max()), SC.turns(site.size)))
    if which == "A":
        assert ref["found"] >= 65536 and (min_voxels > 1 or ref["K"] >= 65536) and SC.scan_levels(site.size) == [4251366, 2076, 2]
    else:
        big = ref["stats"][np.argmax(ref["stats"][:, 1])]
        assert SC.turns(site.size) == (64, 519) and big[2:5].tolist() == [0, 0, 0] and big[5:8].tolist() == [s - 1 for s in SC.B]
        assert 2 * big[1] > int((site != 0).sum()) and int((ref["sizes_all"] == 1).sum()) > 10000
    capacity = ref["K"] + 3
    label, count, stats = run_ccl(site, dev, conn, min_voxels, capacity)
    assert np.array_equal(label, ref["label"]), int((label != ref["label"]).sum())
    assert count.tolist() == [ref["K"], ref["found"]], count.tolist()
    bad = np.flatnonzero((stats[:ref["K"]] != ref["stats"]).any(axis=1))
    assert bad.size == 0, (bad.size, stats[bad[:3]].tolist(), ref["stats"][bad[:3]].tolist())
    assert (stats[ref["K"]:] == CC.POISON).all()
    again = run_ccl(site, dev, conn, min_voxels, capacity)
    assert all(np.array_equal(a, b) for a, b in zip((label, count, stats), again)), "two launches differ"


# ---- pooling ----------------------------------------------------------------------------------------------------------------------------
def run_pool(dev, label, K, valid, sets):
    """one d3f_volume_pool launch on poisoned outputs and workspace.  sets: (rows float32 [n, C], mode) -> (members, count, moments, [rows])"""
    lib = _lib.load()
    nx, ny, nz = label.shape
    lab = torch.from_numpy(np.array(label)).to(dev)
    val = torch.from_numpy(np.array(valid, dtype=np.uint8)).to(dev)
    cap = int(((label >= 1) & (label <= K) & (valid != 0)).sum())
    arr = (_lib.VolumeSet * max(len(sets), 1))()
    modes = (ctypes.c_int32 * max(len(sets), 1))()
    outs = (ctypes.c_void_p * max(len(sets), 1))()
    hold, bufs, mean_channels = [], [], 0
    for s, (rows, mode) in enumerate(sets):
        t = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        C = rows.shape[1]
        arr[s] = _lib.VolumeSet(t.data_ptr(), C, 0, C, None)
        modes[s] = mode
        ob = poisoned(4 * K * C, dev)
        outs[s] = ob.data_ptr()
        hold.append(t)
        bufs.append((ob, C, mode))
        mean_channels += C if mode == MEAN else 0
    members = poisoned(8, dev)
    count = poisoned(4 * K, dev)
    moments = poisoned(72 * K, dev)
    ws_bytes = lib.d3f_volume_pool_workspace_bytes(nx, ny, nz, K, cap, mean_channels)
    assert ws_bytes > 0
    ws = poisoned(ws_bytes, dev)
    _lib.check(lib.d3f_volume_pool(_lib.ptr(lab), nx, ny, nz, K, _lib.ptr(val), None, arr, len(sets), modes, cap, _lib.ptr(members), _lib.ptr(count),
                                   _lib.ptr(moments), outs, _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    rows = [ob[:4 * K * C].cpu().numpy().view(np.float32 if mode == MEAN else np.int32).reshape(K, C) for ob, C, mode in bufs]
    return int(members[:8].view(torch.int64).item()), count[:4 * K].view(torch.int32).cpu().numpy(), moments[:72 * K].view(torch.int64).view(K, 9).cpu().numpy(), rows


def test_pool_with_a_third_sort_pass_and_three_scan_levels(dev):
    """the components of A (K >= 65 536: three digits of the label sort, K + 1 > 2048: multi-workgroup plan scans), two narrow mean sets and votes"""
    case = SC.pool_case("A")
    label, K, valid = case["label"], case["K"], case["valid"]
    assert K >= 65536 and SC.sort_passes(K) == 3 and len(SC.scan_levels(K + 1)) == 2
    _, _, _, counts = SC.members_fast(label, K, valid)
    print("\n  pool A: K = %d components, %d members, largest %d, %d empty" % (K, int(counts.sum()), int(counts.max()), int((counts == 0).sum())))
    assert counts.max() > 256 and (counts == 0).any()
    sets = [(r, MEAN) for r in case["rows"]] + [(case["votes"], VOTES)]
    members, count, moments, rows = run_pool(dev, label, K, valid, sets)
    assert members == int(counts.sum()) and np.array_equal(count, counts.astype(np.int32))
    assert np.array_equal(moments, SC.moments_fast(label, K, valid))
    assert np.array_equal(rows[-1], SC.votes_fast(label, K, case["votes"], valid)) and np.array_equal(rows[-1].sum(axis=1), count)
    for s, r in enumerate(case["rows"]):
        want = SC.pool_fast(label, K, r, valid)
        bad = np.argwhere(rows[s].view(np.int32) != want.view(np.int32))
        assert bad.size == 0, (s, len(bad), bad[:4].tolist())                                    # the bound of test_gpu_pool.py: the bits of the fold
        mean64, abs64 = SC.pool_mean64(label, K, r, valid)
        live = counts > 0
        ratio = np.abs(rows[s][live] - mean64[live]) / (SC.fold_bound(counts[live])[:, None] * abs64[live])
        print("  pool A set %d (C = %d): bits equal the fold; worst |mean - float64| / ((255 levels + 1) 2^-24 mean|row|) = %.3g" % (s, r.shape[1], float(ratio.max())))
        assert ratio.max() <= 1.0
    again = run_pool(dev, label, K, valid, sets)
    assert again[0] == members and all(np.array_equal(a, b) for a, b in zip([count, moments] + rows, [again[1], again[2]] + again[3])), "two launches differ"


def test_pool_flags_at_the_turn_cap(dev):
    """B: pool_flag_kernel takes 64 turns per workgroup on 519 workgroups; the spanning component's count is held in registers across all of them"""
    case = SC.pool_case("B")
    label, K, valid = case["label"], case["K"], case["valid"]
    assert SC.turns(label.size) == (64, 519)
    _, _, _, counts = SC.members_fast(label, K, valid)
    members, count, moments, _ = run_pool(dev, label, K, valid, [])
    print("\n  pool B: K = %d components, %d members, largest %d" % (K, members, int(counts.max())))
    assert members == int(counts.sum()) and np.array_equal(count, counts.astype(np.int32))
    assert np.array_equal(moments, SC.moments_fast(label, K, valid))


# ---- distance transform -------------------------------------------------------------------------------------------------------------------
def test_distance_transform_with_long_lines(dev):
    site = SC.edt_case()
    true = SC.edt_reference()
    assert site.shape[2] > 64 and int(true[:, :, (SC.EDT_SLAB[0] + SC.EDT_SLAB[1]) // 2].min()) > 32 ** 2
    lib = _lib.load()
    nx, ny, nz = site.shape
    s = torch.from_numpy(np.array(site)).to(dev)
    d2 = torch.full((nx, ny, nz), -77, dtype=torch.int32, device=dev)
    nearest = torch.full((nx, ny, nz), -77, dtype=torch.int32, device=dev)
    dist = torch.full((nx, ny, nz), float("nan"), dtype=torch.float32, device=dev)
    ws_bytes = lib.d3f_volume_edt_workspace_bytes(nx, ny, nz)
    ws = poisoned(ws_bytes, dev)
    _lib.check(lib.d3f_volume_edt(_lib.ptr(s), nx, ny, nz, STEP, 0, _lib.ptr(d2), _lib.ptr(nearest), _lib.ptr(dist), _lib.ptr(ws), ws_bytes,
                                  _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    got = d2.cpu().numpy()
    print("\n  edt A: %d sites, largest d2 %d" % (int((site != 0).sum()), int(true.max())))
    assert np.array_equal(got, true), int((got != true).sum())
    EC.check_nearest(site, true, nearest.cpu().numpy())
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), EC.dist_ref(true, STEP).view(np.uint32))


# ---- cost-to-go ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn,w", SC.GEO_CONFIGS, ids=lambda v: str(v).replace(" ", ""))
def test_cost_to_go_with_more_listed_tiles_than_workgroups(dev, conn, w):
    """a goal in every tile of A: the first round lists more than kGeoMaxGrid = 4096 tiles, so a workgroup takes up to three in turn and reuses its
    LDS.  The count is read, not assumed: word 0 of the workspace header is the length of the list the next round runs -- the number relax
    copies to out_pending after its last round (the entry point rejects rounds = 0, so it cannot be asked for it before the first)."""
    free, seeds = SC.travel_case()
    want_cost, want_next, sweeps = SC.travel_reference(conn, w)
    lib = _lib.load()
    nx, ny, nz = free.shape
    f = torch.from_numpy(np.array(free)).to(dev)
    s = torch.from_numpy(np.array(seeds)).to(dev)
    cost = poisoned(4 * free.size, dev).view(torch.int32)
    nxt = poisoned(4 * free.size, dev).view(torch.int32)
    dist = poisoned(4 * free.size, dev).view(torch.float32)
    pending = poisoned(16, dev).view(torch.int32)
    ws_bytes = lib.d3f_volume_geodesic_workspace_bytes(nx, ny, nz)
    ws = poisoned(ws_bytes, dev)
    warr = (ctypes.c_int32 * 3)(*w)
    stream = _lib.current_stream_handle(dev)
    _lib.check(lib.d3f_volume_geodesic_init(_lib.ptr(f), nx, ny, nz, _lib.ptr(s), len(seeds), _lib.ptr(cost), _lib.ptr(ws), ws_bytes, stream))
    listed = int(ws[:4].view(torch.int32).item())
    print("\n  cost-to-go A, connectivity %d: %d tiles, %d listed for the first round (%d workgroups), reference sweeps %d" % (
        conn, int(np.prod(SC.tiles(free.shape))), listed, SC.GEO_MAX_GRID, sweeps))
    assert listed > SC.GEO_MAX_GRID and listed == len(SC.listed_after_init(free, seeds))
    rounds, total = 16, 0
    while True:                                                           # the loop of BakedField.travel
        _lib.check(lib.d3f_volume_geodesic_relax(_lib.ptr(f), None, nx, ny, nz, conn, warr, GC.NO_CAP, rounds, _lib.ptr(cost), _lib.ptr(pending), _lib.ptr(ws),
                                                 ws_bytes, stream))
        total += rounds
        left = int(pending[0].item())
        if left == 0:
            break
        assert total <= free.size
        rounds = min(2 * rounds, 256)
    assert left == 0
    _lib.check(lib.d3f_volume_geodesic_finish(_lib.ptr(f), None, nx, ny, nz, conn, warr, STEP, _lib.ptr(cost), _lib.ptr(nxt), _lib.ptr(dist), stream))
    torch.cuda.synchronize()
    got_cost = cost.cpu().numpy().reshape(free.shape)
    assert np.array_equal(got_cost, want_cost), int((got_cost != want_cost).sum())
    assert np.array_equal(nxt.cpu().numpy().reshape(free.shape), want_next)
    assert np.array_equal(dist.cpu().numpy().reshape(free.shape).view(np.int32), GC.dist_ref(want_cost, STEP, w[0]).view(np.int32))
    behind = want_cost[SC.GEO_SLAB[1]:]
    assert (behind != SC.INT32_MAX).mean() > 0.8 and (want_cost[SC.GEO_SLAB[0]:SC.GEO_SLAB[1]] == SC.INT32_MAX).all()


# ---- mesh ---------------------------------------------------------------------------------------------------------------------------------
def raw_extract(dev, vol, valid, cap_v, cap_t, count_only=False):
    lib = _lib.load()
    nx, ny, nz = vol.shape
    v = torch.from_numpy(np.ascontiguousarray(vol)).to(dev).view(-1)
    va = torch.from_numpy(np.ascontiguousarray(valid)).to(dev).view(-1) if valid is not None else None
    ws_bytes = int(lib.d3f_mesh_workspace_bytes(nx, ny, nz))
    ws = poisoned(ws_bytes, dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    stream = _lib.current_stream_handle(dev)
    if count_only:
        _lib.check(lib.d3f_mesh_count(_lib.ptr(v), _lib.ptr(va), nx, ny, nz, 0.0, _lib.ptr(counts), _lib.ptr(ws), ws_bytes, stream))
        return tuple(int(c) for c in counts.tolist())
    pad = 64
    keys = torch.full((cap_v * 8 + pad,), GUARD, dtype=torch.uint8, device=dev)
    t = torch.full((cap_v * 4 + pad,), GUARD, dtype=torch.uint8, device=dev)
    tris = torch.full((cap_t * 12 + pad,), GUARD, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_mesh_extract(_lib.ptr(v), _lib.ptr(va), nx, ny, nz, 0.0, cap_v, cap_t, _lib.ptr(keys), _lib.ptr(t), _lib.ptr(tris), _lib.ptr(counts),
                                    _lib.ptr(ws), ws_bytes, stream))
    torch.cuda.synchronize()
    for buf, used in ((keys, cap_v * 8), (t, cap_v * 4), (tris, cap_t * 12)):
        assert bool((buf[used:] == GUARD).all()), "written past a capacity"
    assert tuple(int(c) for c in counts.tolist()) == (cap_v, cap_t)
    return keys[:cap_v * 8].view(torch.int64).cpu().numpy(), t[:cap_v * 4].view(torch.float32).cpu().numpy(), tris[:cap_t * 12].view(torch.int32).view(-1, 3).cpu().numpy()


@pytest.mark.parametrize("kind", ["sphere", "clipped"])
def test_mesh_with_two_scan_levels(dev, kind):
    """4153 workgroup totals: two scan levels with a ragged third workgroup.  Compared with tests/mesh_ref.py itself (it takes two to three seconds
    at this size): keys and triangles exactly, t within the 2^-22 of test_gpu_mesh.py; the hole-free sphere is a closed surface with V - E + F = 2."""
    import mesh_ref
    vol, valid = SC.mesh_volume(kind)
    rk, rt, rtri = SC.mesh_reference(kind)
    assert len(SC.scan_levels(vol.size // SC.MESH_BLOCK + 2)) == 2 and rk.size > 50000
    nv, nt = raw_extract(dev, vol, valid, 0, 0, count_only=True)
    assert (nv, nt) == (rk.size, rtri.shape[0])
    k, t, tri = raw_extract(dev, vol, valid, nv, nt)
    assert np.array_equal(k, rk), int((k != rk).sum())
    flat = vol.reshape(-1).astype(np.float64)
    a = rk // 3
    b = a + np.asarray([vol.shape[1] * vol.shape[2], vol.shape[2], 1])[rk % 3]
    err = float(np.max(np.abs(t.astype(np.float64) - (0.0 - flat[a]) / (flat[b] - flat[a]))))
    print("\n  mesh %s: %d vertices, %d triangles, max |dt| = %.3g (bound 2^-22 = %.3g)" % (kind, nv, nt, err, 2.0 ** -22))
    assert np.all((t >= 0) & (t <= 1)) and err <= 2.0 ** -22
    assert np.array_equal(tri.astype(np.int64), rtri)
    if kind == "sphere":
        assert mesh_ref.is_closed_manifold(tri) and mesh_ref.euler_characteristic(k.size, tri) == 2
    else:
        assert valid is not None and not valid.all()


# ---- rows past 2^31 -----------------------------------------------------------------------------------------------------------------------
def test_rows_past_two_to_the_31(dev):
    """A with 512 dense float32 channels, made on the device (8.7 GB, 2.18 G floats): voxel * stride passes 2^31 from voxel 2^22 on.  The dense
    sample, its backward and a pool mean over two components, against the eight corner rows gathered with torch indexing (int64) on the device and
    the float64 chain and bounds of volume_cases on them; the means against the fold of the gathered member rows, bit for bit."""
    from d3fields_amd import BakedField
    nx, ny, nz = SC.A
    n, C = nx * ny * nz, SC.ROW_CHANNELS
    assert n * C > 2 ** 31
    gen = torch.Generator(device=dev).manual_seed(5)
    big = torch.randn((nx, ny, nz, C), device=dev, generator=gen)
    dist = torch.zeros((nx, ny, nz), device=dev)
    f = BakedField.from_arrays(list(VC.ORIGIN), VC.STEP, dist, big=big)
    assert f._sets["big"].data_ptr() == big.data_ptr()
    pts, cells = SC.row_points()
    vol = {"origin": np.asarray(VC.ORIGIN, np.float32), "step": np.float32(VC.STEP), "shape": SC.A}
    i, t = SC.locate_cells(SC.A, VC.ORIGIN, VC.STEP, pts)
    i32, t32 = SC.locate_cells(SC.A, VC.ORIGIN, VC.STEP, pts, np.float32)
    assert np.array_equal(i, cells) and np.array_equal(i32, cells)
    vox = SC.corner_voxels(SC.A, i)
    assert int((vox >= 2 ** 22).any(axis=0).sum()) > 1500 and int(vox.max()) == n - 1
    flat = big.view(n, C)
    v = flat[torch.from_numpy(vox.reshape(-1)).to(dev)].view(8, len(pts), C).cpu().numpy()
    dpts = torch.from_numpy(pts).to(dev)
    out = f.eval(dpts)
    torch.cuda.synchronize()
    assert bool(out["valid_mask"].all())
    val, Aq, S = SC.blend64(v, t)
    port = SC.blend32(v, t32)
    port_worst = VC.worst_ratio(port, val, Aq, VC.coord_term(vol, S))
    tol = VC.tolerance(port_worst)
    got_worst = VC.worst_ratio(out["big"].cpu().numpy(), val, Aq, VC.coord_term(vol, S))
    print("\n  rows past 2^31: sample   port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (port_worst, tol, got_worst))
    assert got_worst <= tol, (got_worst, tol)
    g = torch.randn((len(pts), C), device=dev, generator=gen)
    got = f.backward(dpts, None, {"big": g}).cpu().numpy()
    gn = g.cpu().numpy()
    want, Bq, T = SC.grad64(v, t, gn, float(VC.STEP))
    port = SC.grad32(v, t32, gn, VC.STEP)
    slack = VC.grad_coord_term(vol, T)[:, None]
    port_worst = VC.worst_ratio(port, want, Bq, slack)
    tol = VC.tolerance(port_worst)
    got_worst = VC.worst_ratio(got, want, Bq, slack)
    print("  rows past 2^31: backward port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (port_worst, tol, got_worst))
    assert got_worst <= tol, (got_worst, tol)
    del out, g
    # a pool mean over two components: the last 1000 voxels, and 66 000 scattered ones (three fold levels)
    m1, m2 = SC.row_pool_members()
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    labels[torch.from_numpy(m1).to(dev)] = 1
    labels[torch.from_numpy(m2).to(dev)] = 2
    pooled = f.pool(labels.view(nx, ny, nz), count=2)
    torch.cuda.synchronize()
    assert pooled["count"].tolist() == [len(m1), len(m2)] and PC.fold_levels(len(m2)) == 3
    got = pooled["big"].cpu().numpy()
    for k, m in enumerate((m1, m2)):
        rows = flat[torch.from_numpy(m).to(dev)].cpu().numpy()
        want = PC.fold(rows) / np.float32(len(m))
        assert np.array_equal(got[k].view(np.int32), want.view(np.int32)), (k, int((got[k] != want).sum()))
    del f, big, flat, labels, pooled
    torch.cuda.empty_cache()
