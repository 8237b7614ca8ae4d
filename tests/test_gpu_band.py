"""The surface band of a baked field on the device (d3f_band_mark / d3f_band_sample / d3f_band_sample_backward, csrc/band_kernels.hip;
BakedField.to_band, Fusion.bake(band=)) against the NumPy restatement of tests/band_cases.py and against the DENSE field of the same
volume: marking equals the restatement exactly; wherever the band covers a point the banded lookup, gradient and ray rows are the
dense field's bit for bit; elsewhere they are the fill row, the dist-only gradient and in_band = False.

Mutants of the kernels and the assert that catches each:
  `<=` for the strict seed test, or |dist| of invalid voxels used    test_mark_equals_the_restatement (cell_band on every volume)
  stored flag not clipped at a face / one neighbour cell forgotten   test_mark_equals_the_restatement (slot, voxels, count)
  slot read as a voxel index, or the row stride of the dense array   test_lookup_is_the_dense_fields_where_in_band (rows bitwise)
  rows read for a point outside the band                             the same test with NaN-poisoned invalid voxels, and M == 0 (NULL rows)
  a set's gradient added outside the band / dist's dropped there     test_gradient
"""
import ctypes

import numpy as np
import pytest
import torch

import band_cases as BC
import raycast_cases as RC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 257, 1003)
CHANNELS = [(1,), (3,), (4,), (16,), (17,), (20,), (64,), (68,), (384,), (3, 68), (16, 384, 17, 4)]
LOOKUP_CASES = ["large plane holes band 1h", "large sphere band 0.5h", "9x8x10 sphere holes band 1.5h"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def field_of(vol, dev):
    from d3fields_amd import BakedField
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()}
    fills = {k: torch.from_numpy(f).to(dev) for k, f in vol["fills"].items() if f is not None}
    return BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev),
                                  valid=torch.from_numpy(vol["valid"]).to(dev), fills=fills, **sets)


def run_mark(field, band, capacity, voxels=None):
    """one d3f_band_mark launch on freshly poisoned outputs -> (cell_band, slot, voxels, count) as NumPy"""
    dev = field.device
    lib = _lib.load()
    nx, ny, nz = field.grid_shape
    cell_band = torch.full((nx - 1, ny - 1, nz - 1), 7, dtype=torch.uint8, device=dev)
    slot = torch.full((nx, ny, nz), -7, dtype=torch.int32, device=dev)
    voxels = torch.full((capacity + 5,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws_bytes = lib.d3f_band_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vol = field._volume()
    _lib.check(lib.d3f_band_mark(ctypes.byref(vol), float(band), _lib.ptr(cell_band), _lib.ptr(slot), _lib.ptr(voxels), capacity, _lib.ptr(count),
                                 _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return cell_band.cpu().numpy(), slot.cpu().numpy(), voxels.cpu().numpy(), int(count.item())


# ---- marking ----------------------------------------------------------------------------------------------------------------------
MARK_BANDS = [(name, None) for name in BC.CASES] + [("large sphere holes band 1h", BC.ABOVE_MU), ("9x8x10 plane holes band 1.5h", BC.ABOVE_MU),
                                                    ("large plane holes band 1h", BC.BELOW_ALL), ("5x4x6 sphere band 1.5h", BC.BELOW_ALL)]


@pytest.mark.parametrize("name,steps", MARK_BANDS)
def test_mark_equals_the_restatement(dev, name, steps):
    vol = BC.volume(name)
    band = BC.band_of(name, steps)
    m = BC.mark(vol, band)
    f = field_of(vol, dev)
    n = vol["dist"].size
    cb, slot, vox, count = run_mark(f, band, n)
    assert count == m["M"], (name, count, m["M"])
    assert np.array_equal(cb.astype(bool), m["cell_band"]) and set(np.unique(cb)) <= {0, 1}
    assert np.array_equal(slot, m["slot"])
    assert np.array_equal(vox[:count], m["voxels"]) and np.all(vox[count:] == -7)
    again = run_mark(f, band, n)
    assert all(np.array_equal(a, b) for a, b in zip((cb, slot, vox), again[:3])) and again[3] == count, "two runs must agree byte for byte"
    if steps == BC.ABOVE_MU:
        assert np.array_equal(cb.astype(bool), m["cell_valid"]) and count > 0
    if steps == BC.BELOW_ALL:
        assert count == 0 and np.all(slot == -1) and not cb.any()
    # the Python layer: to_band holds the same arrays
    b = f.to_band(float(band))
    assert b.band_voxels.dtype == torch.int32 and np.array_equal(b.band_voxels.cpu().numpy(), m["voxels"])
    assert np.array_equal(b.slot.cpu().numpy(), m["slot"]) and np.array_equal(b.cell_band.cpu().numpy().astype(bool), m["cell_band"])
    assert b.stored_fraction == m["M"] / n and b.dist is f.dist and b.valid is f.valid and b.cell_valid is f.cell_valid and b.band == float(band)


@pytest.mark.parametrize("name", ["large plane holes band 1h", "2x2x2 plane band 1.5h"])
def test_mark_with_a_short_capacity(dev, name):
    """the true count is reported, nothing is written past the capacity, and a re-run with the count is complete"""
    vol = BC.volume(name)
    band = BC.band_of(name)
    m = BC.mark(vol, band)
    f = field_of(vol, dev)
    for cap in (0, 3, m["M"] - 1):
        cb, slot, vox, count = run_mark(f, band, cap)
        assert count == m["M"] > cap
        assert np.array_equal(vox[:cap], m["voxels"][:cap]) and np.all(vox[cap:] == -7), (name, cap)
        assert np.array_equal(slot, m["slot"]) and np.array_equal(cb.astype(bool), m["cell_band"])
    cb, slot, vox, count = run_mark(f, band, m["M"])
    assert count == m["M"] and np.array_equal(vox[:count], m["voxels"]) and np.all(vox[count:] == -7)


# ---- lookups ----------------------------------------------------------------------------------------------------------------------
def points_of(vol, n, seed):
    """n inside points; from 63 on the specials (outside, NaN, faces) lead and lattice points follow -- -> (points, rows with a float64 verdict)"""
    pts = BC.inside_points(vol, n, seed)
    exact = np.ones(n, bool)
    if n >= 63:
        sp, lat = BC.special_points(vol), BC.lattice_points(vol)
        lat = lat[:: max(1, len(lat) // 20)][:20]
        pts[:len(sp)] = sp
        pts[len(sp):len(sp) + len(lat)] = lat
        exact[:len(sp) + len(lat)] = False
    return pts, exact


def check_lookup(vol, m, dense_out, band_out, pts, exact, label):
    ok_ref, ib_ref = BC.in_band(vol, m, pts)
    ok = band_out["valid_mask"].cpu().numpy()
    ib = band_out["in_band"].cpu().numpy()
    assert band_out["in_band"].dtype == torch.bool and list(band_out)[:3] == ["dist", "valid_mask", "in_band"]
    assert torch.equal(band_out["dist"], dense_out["dist"]) and torch.equal(band_out["valid_mask"], dense_out["valid_mask"]), label
    assert np.array_equal(ok[exact], ok_ref[exact]) and np.array_equal(ib[exact], ib_ref[exact]), (label, "in_band differs from the float64 reference")
    assert not (ib & ~ok).any(), label
    for k in vol["sets"]:
        got, want = band_out[k].cpu().numpy(), dense_out[k].cpu().numpy()
        fill = np.zeros(got.shape[1], np.float32) if vol["fills"][k] is None else vol["fills"][k]
        assert np.array_equal(got[ib].view(np.uint32), want[ib].view(np.uint32)), (label, k, "rows differ from the dense field's where in_band")
        assert np.array_equal(got[~ib].view(np.uint32), np.broadcast_to(fill, got[~ib].shape).view(np.uint32)), (label, k, "fill row")
        assert not np.isnan(got).any(), (label, k)
    return ok, ib


@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "C" + "_".join(map(str, c)))
@pytest.mark.parametrize("name", LOOKUP_CASES)
def test_lookup_is_the_dense_fields_where_in_band(dev, name, channels):
    fills = (0,) if len(channels) != 2 else (1,)
    vol = BC.volume(name, channels, fills)
    band = BC.band_of(name)
    m = BC.mark(vol, band)
    dense = field_of(vol, dev)
    banded = dense.to_band(float(band))
    assert banded.names() == dense.names() and all(tuple(banded._sets[k].shape) == (m["M"], C) for k, C in zip(banded.names(), channels))
    seen = np.zeros(2, int)
    for n in COUNTS:
        pts, exact = points_of(vol, n, n % 5)
        dpts = torch.from_numpy(pts).to(dev)
        ok, ib = check_lookup(vol, m, dense.eval(dpts), banded.eval(dpts), pts, exact, "%s C=%s N=%d" % (name, channels, n))
        seen += (int(ib.sum()), int((ok & ~ib).sum()))
    assert seen[0] > 0 and (seen[1] > 0 or not BC.CASES[name][2]), "points inside and outside the band must both occur"
    # a subset of the names in another order, and the distance-only lookup
    names = list(reversed(banded.names()))[:2]
    some = banded.eval(dpts, return_names=names)
    full = banded.batch_eval(dpts)
    assert list(some) == ["dist", "valid_mask", "in_band"] + names and all(torch.equal(some[k], full[k]) for k in some)
    d = banded.eval_dist(dpts)
    assert list(d) == ["dist", "valid_mask", "in_band"] and torch.equal(d["in_band"], full["in_band"])


def test_output_rows_off_16_bytes_equal_the_aligned_call(dev):
    """out_sets[s] 4-byte but not 16-byte aligned while the compacted rows are (C = 8 on a 3x4x5 volume, 64 points; the entry point called
    directly): the set drops to scalar stores and gives the aligned call's rows bit for bit, and nothing beside them is written"""
    import volume_cases as VC
    shape, n, C = (3, 4, 5), 64, 8
    vol = VC.make_volume(shape, (C,), 2, 0.1, True, (0,))
    banded = field_of(vol, dev).to_band(float(np.abs(vol["dist"][vol["valid"]]).max()) * 0.75)
    lib = _lib.load()
    pts = torch.from_numpy(np.concatenate([VC.special_points(shape)[:8], VC.inside_points(shape, n - 8, 2)])).to(dev)
    assert banded._sets["s0"].data_ptr() % 16 == 0 and banded._sets["s0"].stride(-2) == C and 0 < banded.band_voxels.numel()

    def run(offset):
        buf = torch.full((n * C + 8,), float("nan"), dtype=torch.float32, device=dev)
        rows = buf[offset:offset + n * C].view(n, C)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        valid, in_band = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        v, b = banded._volume(), banded._band_struct()
        _lib.check(lib.d3f_band_sample(ctypes.byref(v), ctypes.byref(b), _lib.ptr(pts), n, banded._set_array(["s0"]), 1, _lib.ptr(dist), _lib.ptr(valid),
                                       _lib.ptr(in_band), (ctypes.c_void_p * 1)(rows.data_ptr()), _lib.current_stream_handle(dev)))
        torch.cuda.synchronize()
        assert rows.data_ptr() % 16 == 4 * offset and bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n * C:]).all())
        return rows.view(torch.int32), dist.view(torch.int32), valid, in_band

    aligned, shifted = run(0), run(1)
    assert all(torch.equal(a, b) for a, b in zip(aligned, shifted))
    assert 0 < int(aligned[3].sum()) < n and not bool(torch.isnan(aligned[0].view(torch.float32)).any())
    assert torch.equal(aligned[0].view(torch.float32), banded.eval(pts)["s0"])


@pytest.mark.parametrize("name", ["large sphere holes band 1h", "9x8x10 plane holes band 1.5h"])
def test_everything_kept_and_nothing_kept(dev, name):
    vol = BC.volume(name, (3, 68), (0,))
    dense = field_of(vol, dev)
    pts, _ = points_of(vol, 1003, 2)
    dpts = torch.from_numpy(pts).to(dev)
    want = dense.eval(dpts)
    every = dense.to_band(float(BC.band_of(name, BC.ABOVE_MU)))
    got = every.eval(dpts)
    assert torch.equal(got["in_band"], want["valid_mask"])
    assert all(torch.equal(got[k], want[k]) for k in want), "with every valid cell kept the whole dict is the dense field's"
    if name in BC.EMPTY_CASES:
        none = dense.to_band(float(BC.band_of(name, BC.BELOW_ALL)))
        assert none.band_voxels.numel() == 0 and none.stored_fraction == 0.0 and tuple(none._sets["s1"].shape) == (0, 68)
        got = none.eval(dpts)
        torch.cuda.synchronize()
        assert not bool(got["in_band"].any()) and torch.equal(got["dist"], want["dist"]) and torch.equal(got["valid_mask"], want["valid_mask"])
        for k in ("s0", "s1"):
            assert torch.equal(got[k], none.fill_row(k).expand(len(pts), -1)), k
        g = none.backward(dpts, torch.ones(len(pts), device=dev), {"s1": torch.ones(len(pts), 68, device=dev)})
        assert torch.equal(g, dense.backward(dpts, torch.ones(len(pts), device=dev)))


# ---- gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [(3,), (68,), (16, 384, 17)], ids=lambda c: "C" + "_".join(map(str, c)))
@pytest.mark.parametrize("name", ["large plane holes band 1h", "large sphere band 0.5h"])
def test_gradient(dev, name, channels):
    vol = BC.volume(name, channels, (0,))
    m = BC.mark(vol, BC.band_of(name))
    dense = field_of(vol, dev)
    banded = dense.to_band(float(BC.band_of(name)))
    for n in (65, 1003):
        pts, exact = points_of(vol, n, n % 5)
        dpts = torch.from_numpy(pts).to(dev)
        gen = torch.Generator().manual_seed(n)
        gd = torch.randn(n, generator=gen).to(dev)
        gs = {k: torch.randn(n, C, generator=gen).to(dev) for k, C in zip(banded.names(), channels)}
        out = banded.eval(dpts)
        ok, ib = out["valid_mask"], out["in_band"]
        got = banded.backward(dpts, gd, gs)
        full, dist_only = dense.backward(dpts, gd, gs), dense.backward(dpts, gd)
        assert torch.equal(got[ib], full[ib]), "the dense field's gradient where in_band"
        assert torch.equal(got[ok & ~ib], dist_only[ok & ~ib]), "the dist term alone where valid but outside the band"
        assert bool((got[~ok] == 0).all()) and not bool(torch.isnan(got).any())
        assert int(ib.sum()) > 0 and int((~ok).sum()) > 0 and (n < 1003 or int((ok & ~ib).sum()) > 0)
        assert torch.equal(banded.backward(dpts, gd, gs), got), "two runs must agree bit for bit"
        assert torch.equal(banded.backward(dpts, None, gs)[ok & ~ib], torch.zeros_like(got[ok & ~ib]))
        # autograd through eval
        p = dpts.clone().requires_grad_(True)
        res = banded.eval(p)
        assert list(res) == list(out) and not res["in_band"].requires_grad and torch.equal(res["in_band"], ib)
        loss = (res["dist"] * gd).sum() + sum((res[k] * gs[k]).sum() for k in gs)
        loss.backward()
        assert torch.equal(p.grad, got)
        assert all(torch.equal(res[k].detach(), out[k]) for k in out)


# ---- rays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x8x10 plane holes band 1.5h", "9x8x10 sphere band 1.5h", "large plane holes band 1h", "large sphere holes band 1h"])
def test_rays(dev, name):
    vol = BC.volume(name, (3, 68), (1,))
    m = BC.mark(vol, BC.band_of(name))
    dense = field_of(vol, dev)
    banded = dense.to_band(float(BC.band_of(name)))
    o, d = BC.rays(vol)
    ref = RC.march(vol, o, d)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    want = dense.raycast(do, dd, return_names=["s0", "s1"], normals=True)
    got = banded.raycast(do, dd, return_names=["s0", "s1"], normals=True)
    torch.cuda.synchronize()
    assert list(got) == ["t", "hit_mask", "points", "normal", "in_band", "s0", "s1"]
    for k in ("t", "hit_mask"):
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(got["points"].cpu().numpy(), want["points"].cpu().numpy(), equal_nan=True)
    ib = got["in_band"]
    assert ib.dtype == torch.bool and not bool((ib & ~got["hit_mask"]).any()) and int(ib.sum()) >= 17
    assert torch.equal(got["normal"], want["normal"])                 # grad dist: every valid point, whatever the band
    for k in ("s0", "s1"):
        assert torch.equal(got[k][ib], want[k][ib]), k
        assert torch.equal(got[k][~ib], banded.fill_row(k).expand(int((~ib).sum()), -1)), k
    # in_band at the hit points against the float64 reference, on the rays that sit on no knife edge and where the device's hit
    # point lies in the cell of the reference's (the march itself is compared in test_gpu_raycast.py)
    keep = ref["hit"] & ~ref["fragile"] & got["hit_mask"].cpu().numpy()
    ok64, ib64 = BC.in_band(vol, m, ref["points"].astype(np.float32))
    ok_dev, ib_dev = BC.in_band(vol, m, got["points"].cpu().numpy())
    same_cell = ok64 == ok_dev
    assert np.array_equal(ib.cpu().numpy()[keep & same_cell], ib64[keep & same_cell]) and (keep & same_cell).sum() >= 17
    assert np.array_equal(ib64[keep], ok64[keep]), "every hit in a valid cell lies in a kept cell"
    # a camera
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1]], np.float32)
    ext = (np.asarray(vol["shape"]) - 1) * float(vol["step"])
    pose = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)         # looks along world -z from the free side of the plane
    pose[:3, 3] = -(pose[:3, :3] @ (vol["centre"] + np.array([0.0, 0.0, 2.5 * ext.max()]))).astype(np.float32)
    w2, g2 = dense.render(K, pose, 24, 32, return_names=["s1"], normals=True), banded.render(K, pose, 24, 32, return_names=["s1"], normals=True)
    assert tuple(g2["in_band"].shape) == (24, 32) and g2["in_band"].dtype == torch.bool
    assert torch.equal(g2["depth"], w2["depth"]) and torch.equal(g2["hit_mask"], w2["hit_mask"]) and torch.equal(g2["normal"], w2["normal"])
    ib2 = g2["in_band"]
    assert int(ib2.sum()) > 0 and not bool((ib2 & ~g2["hit_mask"]).any())
    assert torch.equal(g2["s1"][ib2], w2["s1"][ib2]) and torch.equal(g2["s1"][~ib2], banded.fill_row("s1").expand(int((~ib2).sum()), -1))
    only = banded.raycast(do, dd)
    assert list(only) == ["t", "hit_mask", "points", "in_band"] and torch.equal(only["in_band"], ib)


# ---- Fusion.bake(band=) -----------------------------------------------------------------------------------------------------------
def test_fusion_bake_band(dev):
    """Four 48 x 64 views of the smooth synthetic scene, a 128-channel map, a mask-like 1-channel map and a 3-component head; a
    24 x 20 x 16 grid (7680 voxels) whose step is a power of two.  Memory: the banded bake may hold dist-sized arrays and the M x C
    rows, never n_voxels x C: peak - before <= 12 dist-sized arrays (dist, slot and the voxel list are one each, valid / cell_valid /
    cell_band a quarter each, the rest is slack for the query's own [M] arrays and the allocator's 512-byte rounding) + 1.25 x the row
    bytes (the rows, the [M, 3] points, dist / valid of the row query) + 64 KiB; the dense rows alone exceed that."""
    from d3fields_amd import Fusion, synth
    V, H, W = 4, 48, 64
    sc = synth.make_scene(V, H, W, "smooth")
    feats = synth.random_map(V, 12, 16, 128, seed=4)
    mask = (synth.random_map(V, 12, 16, 1, seed=6) > 0).to(torch.float32)
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {"depth": sc["depth"].to(dev), "K": sc["K"].to(dev), "pose": sc["pose"].to(dev), "dino_feats": feats.to(dev), "mask": mask.to(dev)}
    f.H, f.W = H, W
    f.add_projection("pca3", components=torch.randn(3, 128, generator=torch.Generator().manual_seed(8)), mean=torch.randn(128, generator=torch.Generator().manual_seed(9)))
    box = dict(x_lower=-0.1875, x_upper=0.1875, y_lower=-0.1875, y_upper=0.125, z_lower=-0.21875, z_upper=0.03125)
    step, band = 2.0 ** -6, 0.012                                     # under the truncation mu = 0.02, where |dist| saturates
    names = ["pca3", "dino_feats", "mask"]
    n_vox, C_all = 24 * 20 * 16, 3 + 128 + 1
    with torch.no_grad():
        f.batch_eval(torch.zeros(8, 3, device=dev), return_names=names)      # the head's projected maps exist before memory is measured
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    banded = f.bake(box, step, return_names=names, band=band)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    M = banded.band_voxels.numel()
    bound = 12 * 4 * n_vox + int(1.25 * 4 * M * C_all) + (64 << 10)
    print("\n  banded bake: M = %d of %d voxels (%.1f %%), peak %d bytes, bound %d, dense rows %d" % (M, n_vox, 100.0 * M / n_vox, peak, bound, 4 * n_vox * C_all))
    assert banded.grid_shape == torch.Size([24, 20, 16]) and 0 < M < n_vox
    assert 4 * n_vox * C_all > bound, "the dense size must be the failing side"
    assert peak <= bound, (peak, bound)
    dense = f.bake(box, step, return_names=names)
    assert torch.equal(banded.dist.view(torch.int32), dense.dist.view(torch.int32)) and torch.equal(banded.valid, dense.valid) and torch.equal(banded.cell_valid, dense.cell_valid)
    vol = {"shape": (24, 20, 16), "dist": dense.dist.cpu().numpy(), "valid": dense.valid.cpu().numpy()}
    m = BC.mark(vol, np.float32(band))
    # (no margin is needed here: the restatement compares the very float32 values the kernel compared)
    assert M == m["M"] and np.array_equal(banded.slot.cpu().numpy(), m["slot"]) and np.array_equal(banded.band_voxels.cpu().numpy(), m["voxels"])
    pts = banded.band_points()
    assert tuple(pts.shape) == (M, 3)
    with torch.no_grad():
        rows = f.batch_eval(pts, return_names=names)
    stored = banded.band_voxels.long()
    for k in names:
        got = banded._sets[k]
        assert tuple(got.shape) == (M, dense._sets[k].shape[3])
        assert torch.equal(got, rows[k]), (k, "slot <-> row plumbing")
        want = dense._sets[k].view(n_vox, -1)[stored]
        if k == "dino_feats":                                          # the grid pass and the point query may order their sums differently: 1e-5 of the largest magnitude
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), k
        else:                                                          # a mask and a projected head: bit identity, as the dense bake states
            assert torch.equal(got, want), k
        assert torch.equal(banded.fill_row(k), dense.fill_row(k)), k
    # at the lattice points of kept cells the lookup returns the stored row.  A stored voxel's centre is looked up in the cell whose
    # low corner it is (the last cell at a far face), which need be neither valid nor kept: the voxel may be stored as the high
    # corner of another cell.  So valid_mask / in_band are the cell bytes of that cell, and the rows are compared where in_band.
    out = banded.eval(pts)
    ib, ok = out["in_band"], out["valid_mask"]
    q = stored
    iz, iy, ix = q % 16, (q // 16) % 20, q // (16 * 20)
    cell = (ix.clamp(max=22) * 19 + iy.clamp(max=18)) * 15 + iz.clamp(max=14)
    assert torch.equal(ok, dense.cell_valid.view(-1)[cell] != 0) and torch.equal(ib, banded.cell_band.view(-1)[cell] != 0)
    assert int(ib.sum()) > 0 and not bool((ib & ~ok).any())
    for k in names:
        assert torch.equal(out[k][ib], banded._sets[k][ib]), k
        assert torch.equal(out[k][~ib], banded.fill_row(k).expand(int((~ib).sum()), -1)), k
    assert torch.equal(out["dist"][ok], dense.dist.view(-1)[stored][ok])
    assert torch.equal(out["dist"], dense.eval(pts, return_names=[])["dist"])
    # and to_band of the dense bake is the same band
    tb = dense.to_band(band)
    assert torch.equal(tb.slot, banded.slot) and torch.equal(tb.band_points(), pts)
    for k in ("pca3", "mask"):
        assert torch.equal(tb._sets[k], banded._sets[k]), k


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_error_paths(dev):
    from d3fields_amd import BakedField
    vol = BC.volume("5x4x6 sphere band 1.5h", (3,))
    f = field_of(vol, dev)
    for bad in (0.0, -0.004, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="band"):
            f.to_band(bad)
    with pytest.raises(TypeError, match="band"):
        f.to_band(None)
    with pytest.raises(AttributeError, match="dense"):
        f.band_points()
    assert f.band is None and "in_band" not in f.eval(torch.zeros(2, 3, device=dev))
    b = f.to_band(0.006)
    with pytest.raises(ValueError, match="already banded"):
        b.to_band(0.006)
    named = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), in_band=torch.zeros(5, 4, 6, 2, device=dev),
                                   t=torch.zeros(5, 4, 6, 2, device=dev))
    with pytest.raises(ValueError, match="in_band"):
        named.to_band(0.006)
    rays = torch.zeros(2, 3, device=dev)
    with pytest.raises(ValueError, match="output key"):
        BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), t=torch.zeros(5, 4, 6, 2, device=dev)).to_band(0.006).raycast(
            rays, rays + 1, return_names=["t"])
    with pytest.raises(KeyError):
        b.eval(rays, return_names=["nope"])
    # a volume of more than 2^31 - 1 voxels is a status code before anything is launched or allocated
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    big = _lib.Volume(2048, 1024, 1024, (ctypes.c_float * 3)(0, 0, 0), 0.5, 0, p, p, p)
    assert lib.d3f_band_mark(ctypes.byref(big), 0.1, p, p, p, 8, p, p, 1 << 20, None) == _lib.ERR_BAD_SHAPE
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(lib.d3f_band_mark(ctypes.byref(f._volume()), float("nan"), p, p, p, 8, p, p, 1 << 20, None))
    assert e.value.code == _lib.ERR_INVALID_ARG
