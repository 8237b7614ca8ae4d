"""Channel sets stored as IEEE half (BakedField.half / from_arrays(rows_dtype=) / Fusion.bake(rows_dtype=); d3f_volume_set's storage word,
csrc/volume_rows.h) on the device.  A half is widened exactly and takes the float32 chain, so every comparison here
is torch.equal / byte equality against the SAME lookup on the widened rows (half().float()), except where said: the forward also passes
test_gpu_volume.py's comparison with the float64 reference, and the backward of a WIDE set (eight channels per lane where float32 has
four: other partial sums) is held to volume_cases.trilinear_grad64 with volume_cases.tolerance, as the float32 path is there.

Mutants of the kernel and the assert that catches each:
  first term as fma(w0, v0, +0)        test_forward: the lattice point (0, 0, 0) of channel 0 must give -0 (volume_f16_cases), as float() does
  stride / C counted in bytes or floats test_forward at every C, test_layouts (stride C + 8, C + 1)
  vectors kept on a misaligned set      test_layouts: data off by 2 and 8 bytes, output rows off by 4 bytes equal the contiguous result
  C % 4 rule instead of C % 8           test_forward C = 20 (scalar where float32 takes vectors), C = 24
  storage word of the wrong set         test_mixed_call"""
import ctypes

import numpy as np
import pytest
import torch

import band_cases as BC
import test_gpu_volume as TGV
import volume_cases as VC
import volume_f16_cases as HC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

CHANNELS = [1, 7, 8, 16, 20, 24, 128, 136, 264]      # narrow | wide at 16 | 20; 20: C % 4 == 0 only; 24: lanes 3..15 idle; 128: one step; 136: + one lane
NS = [1, 63, 64, 65, 257]                            # wave tails, the `wave_first + 4 r >= n` exit, a second workgroup
SHAPE_NAMES = ["5x4x6", "2x2x2"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def half_field(vol, dev, names=None, wide_names=()):
    """the field of a volume_f16_cases volume with its sets stored as half (wide_names: those as the widened float32 instead)"""
    from d3fields_amd import BakedField
    names = list(vol["sets"]) if names is None else names
    sets = {k: torch.from_numpy(vol["sets"][k] if k in wide_names else vol["bits"][k].view(np.float16)).to(dev) for k in names}
    fills = {k: torch.from_numpy(vol["fills"][k]).to(dev) for k in names if vol["fills"][k] is not None}
    f = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                               fills=fills, rows_dtype={k: torch.float16 for k in names if k not in wide_names}, **sets)
    for k in names:
        assert f.rows_dtype(k) == (torch.float32 if k in wide_names else torch.float16)
    return f


def same(a, b, label):
    assert list(a) == list(b), label
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (label, k)
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (label, k)


def banded(f, vol):
    return f.to_band(float(HC.band_of(vol)))


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_forward(dev, shape_name, C):
    """dense and banded: half.eval == half.float().eval on every key (valid_mask, in_band and the non-zero fill rows included), for every n;
    the dense result also passes the float32 path's own comparison with the float64 reference on the widened arrays"""
    vol = HC.case(shape_name, (C,), C % 5, 0.2 if shape_name == "5x4x6" else 0.0, True, (0,))
    assert np.abs(vol["fills"]["s0"]).min() > 0
    h = half_field(vol, dev)
    w = h.float()
    assert w.rows_dtype("s0") == torch.float32 and h.rows_bytes * 2 == w.rows_bytes
    assert torch.equal(w._sets["s0"].view(torch.int32)[h.valid], torch.from_numpy(vol["sets"]["s0"]).to(dev).view(torch.int32)[h.valid])
    hb, wb = banded(h, vol), banded(w, vol)
    for n in NS:
        pts = HC.points(vol["shape"], n, C % 5)
        d = torch.from_numpy(pts).to(dev)
        got = h.eval(d)
        same(got, w.eval(d), ("dense", shape_name, C, n))
        assert tuple(got["s0"].shape) == (n, C) and got["s0"].dtype == torch.float32
        TGV.check_forward(vol, pts, VC.trilinear64(vol, pts), got, "half %s C=%d N=%d" % (shape_name, C, n))
        gb = hb.eval(d)
        same(gb, wb.eval(d), ("banded", shape_name, C, n))
        assert list(gb) == ["dist", "valid_mask", "in_band", "s0"]
        ib = gb["in_band"]
        assert torch.equal(gb["s0"][ib].view(torch.int32), got["s0"][ib].view(torch.int32))           # the dense field's bits where in the band
        assert torch.equal(gb["s0"][~ib], hb.fill_row("s0").expand(int((~ib).sum()), -1))
    # the chain's first term is a plain multiply: -0 at the lattice point (0, 0, 0), channel 0
    first = h.eval(torch.from_numpy(HC.lattice_points(vol["shape"])[:1]).to(dev))
    assert bool(first["valid_mask"][0]) and int(first["s0"][0, 0].view(torch.int32)) == -2 ** 31


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 24, 136])
def test_layouts(dev, C):
    """from_arrays on views: a voxel stride of C + 8 (vectors kept) and C + 1 (scalars), data off by 2 and by 8 bytes (scalars); the entry
    point called directly with output rows off by 4 bytes (vectors dropped).  All equal the contiguous field's rows."""
    from d3fields_amd import BakedField
    vol = HC.case("5x4x6", (C,), 1, 0.2, True, (0,))
    nx, ny, nz = vol["shape"]
    nv = nx * ny * nz
    rows = torch.from_numpy(vol["bits"]["s0"].view(np.float16)).to(dev)
    ref_field = half_field(vol, dev)
    assert ref_field._sets["s0"].data_ptr() % 16 == 0 and ref_field._sets["s0"].stride(-2) == C
    pts = torch.from_numpy(HC.points(vol["shape"], 257, 1)).to(dev)
    want = ref_field.eval(pts)

    def field(view):
        return BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                                      fills={"s0": torch.from_numpy(vol["fills"]["s0"]).to(dev)}, rows_dtype=torch.float16, s0=view)

    for pad in (8, 1):
        buf = torch.full((nv, C + pad), float("nan"), dtype=torch.float16, device=dev)
        buf[:, :C] = rows.view(nv, C)
        f = field(buf[:, :C].view(nx, ny, nz, C))
        assert f._sets["s0"].data_ptr() == buf.data_ptr() and f._set_array(["s0"])[0].stride_voxel == C + pad      # used in place
        same(f.eval(pts), want, ("stride", C + pad))
        if pad == 8 or C <= 16:                                           # (scalar rows of a WIDE set put other channels on a lane: other partial sums)
            same({"g": f.backward(pts, None, {"s0": torch.ones(257, C, device=dev)})}, {"g": ref_field.backward(pts, None, {"s0": torch.ones(257, C, device=dev)})},
                 ("stride backward", C + pad))
    for off in (1, 4):                                                     # elements: 2 and 8 bytes
        buf = torch.full((nv * C + 8,), float("nan"), dtype=torch.float16, device=dev)
        buf[off:off + nv * C] = rows.view(-1)
        f = field(buf[off:off + nv * C].view(nx, ny, nz, C))
        assert f._sets["s0"].data_ptr() == buf.data_ptr() + 2 * off and f._sets["s0"].data_ptr() % 16 == 2 * off
        same(f.eval(pts), want, ("data offset", 2 * off))
    # output rows 4-byte but not 16-byte aligned
    lib, n = _lib.load(), 257
    out = torch.full((n * C + 8,), float("nan"), dtype=torch.float32, device=dev)
    got = out[1:1 + n * C].view(n, C)
    dist, valid = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    v = ref_field._volume()
    _lib.check(lib.d3f_volume_sample(ctypes.byref(v), _lib.ptr(pts), n, ref_field._set_array(["s0"]), 1, _lib.ptr(dist), _lib.ptr(valid),
                                     (ctypes.c_void_p * 1)(got.data_ptr()), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    assert got.data_ptr() % 16 == 4 and bool(torch.isnan(out[:1]).all()) and bool(torch.isnan(out[1 + n * C:]).all())
    assert torch.equal(got.view(torch.int32), want["s0"].view(torch.int32))


# ---- one call, both storages ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half_names", [("s0",), ("s1",)])
def test_mixed_call(dev, half_names):
    """a narrow set and a wide set, one half and one float32, in one launch = the two sets looked up separately (dense and banded,
    forward and backward)"""
    vol = HC.case("5x4x6", (8, 136), 2, 0.2, True, (0, 1))
    wide_names = tuple(k for k in ("s0", "s1") if k not in half_names)
    mixed = half_field(vol, dev, wide_names=wide_names)
    assert {mixed.rows_dtype(k) for k in ("s0", "s1")} == {torch.float16, torch.float32}
    pts = torch.from_numpy(HC.points(vol["shape"], 257, 2)).to(dev)
    g = {k: torch.randn(257, C, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) for k, C in (("s0", 8), ("s1", 136))}
    for f in (mixed, banded(mixed, vol)):
        both = f.eval(pts)
        for k in ("s0", "s1"):
            alone = f.eval(pts, return_names=[k])
            assert torch.equal(both[k].view(torch.int32), alone[k].view(torch.int32)) and torch.equal(both["dist"], alone["dist"]), k
        swapped = f.eval(pts, return_names=["s1", "s0"])
        same({k: swapped[k] for k in both}, both, "the names in another order")
        # the same bits as the all-float32 field
        same(both, f.float().eval(pts), ("mixed", half_names))
        # backward: a gradient through one set alone equals the call that holds both sets with the other's gradient None
        for k in ("s0", "s1"):
            other = "s1" if k == "s0" else "s0"
            assert torch.equal(f.backward(pts, None, {k: g[k]}), f.backward(pts, None, {k: g[k], other: None}))
        assert torch.equal(f.backward(pts, None, g), f.backward(pts, None, g))


# ---- backward and autograd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_backward(dev, shape_name, C):
    vol = HC.case(shape_name, (C, 3), C % 5, 0.1 if shape_name == "5x4x6" else 0.0, True, (0,))
    h = half_field(vol, dev)
    w = h.float()
    hb, wb = banded(h, vol), banded(w, vol)
    rng = np.random.default_rng(100 + C)
    for n in (1, 65, 257):
        pts = HC.points(vol["shape"], n, C % 5)
        d = torch.from_numpy(pts).to(dev)
        gd = rng.standard_normal(n).astype(np.float32)
        gs = {"s0": rng.standard_normal((n, C)).astype(np.float32), "s1": rng.standard_normal((n, 3)).astype(np.float32)}
        tgd, tgs = torch.from_numpy(gd).to(dev), {k: torch.from_numpy(v).to(dev) for k, v in gs.items()}
        for f, wf, kind in ((h, w, "dense"), (hb, wb, "banded")):
            got = f.backward(d, tgd, tgs)
            assert got.shape == (n, 3) and got.dtype == torch.float32 and not bool(torch.isnan(got).any())
            assert torch.equal(got.view(torch.int32), f.backward(d, tgd, tgs).view(torch.int32)), (kind, "two runs")
            # entries that are None are skipped: the narrow s1 alone, and the call that names s0 as None, are one result
            assert torch.equal(f.backward(d, tgd, {"s1": tgs["s1"]}), f.backward(d, tgd, {"s0": None, "s1": tgs["s1"]}))
            assert torch.equal(f.backward(d, tgd, {"s1": tgs["s1"]}).view(torch.int32), wf.backward(d, tgd, {"s1": tgs["s1"]}).view(torch.int32))
            if C <= 16:                                                     # one lane, channels in order: the float32 backward's bytes
                assert torch.equal(got.view(torch.int32), wf.backward(d, tgd, tgs).view(torch.int32)), (kind, C, n)
        # every width, dense: the float64 reference with the float32 path's tolerance
        got = h.backward(d, tgd, tgs).cpu().numpy()
        want, B, T = VC.trilinear_grad64(vol, pts, gd, gs)
        port = VC.trilinear_grad32(vol, pts, gd, gs)
        slack = VC.grad_coord_term(vol, T)[:, None]
        port_worst = VC.worst_ratio(port, want, B, slack)
        tol = VC.tolerance(port_worst)
        got_worst = VC.worst_ratio(got, want, B, slack)
        print("\n  %s C=%-4d N=%-4d port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (shape_name, C, n, port_worst, tol, got_worst))
        ok = VC.trilinear64(vol, pts, names=[])["valid"]
        assert np.all(got[~ok] == 0) and got_worst <= tol, (C, n, got_worst, tol)
        # banded: the dense field's bytes where the point is in the band (the same lanes sum the same channels)
        ib = hb.eval(d, return_names=[])["in_band"]
        assert torch.equal(hb.backward(d, None, tgs)[ib].view(torch.int32), h.backward(d, None, tgs)[ib].view(torch.int32))
    # autograd through eval: the entry point's numbers
    for f in (h, hb):
        p = d.clone().requires_grad_(True)
        out = f.eval(p)
        loss = (out["dist"] * tgd).sum() + (out["s0"] * tgs["s0"]).sum() + (out["s1"] * tgs["s1"]).sum()
        loss.backward()
        assert torch.equal(p.grad, f.backward(d, tgd, tgs))
        with torch.no_grad():
            plain = f.eval(d)
        assert all(torch.equal(plain[k], out[k].detach()) for k in plain)


# ---- the band ---------------------------------------------------------------------------------------------------------------------
def test_band_commutes_with_half_and_may_be_empty(dev):
    vol = HC.case("5x4x6", (8, 136), 4, 0.2, True, (0,))
    h = half_field(vol, dev)
    w = h.float()
    band = float(HC.band_of(vol))
    a, b = h.to_band(band), w.to_band(band).half()
    m = HC.mark(vol, band)
    assert a.band_voxels.numel() == m["M"] > 0 and np.array_equal(a.slot.cpu().numpy(), m["slot"])
    pts = torch.from_numpy(HC.points(vol["shape"], 257, 4)).to(dev)
    for k in ("s0", "s1"):
        assert a.rows_dtype(k) == b.rows_dtype(k) == torch.float16 and tuple(a._sets[k].shape) == (m["M"], vol["sets"][k].shape[3])
        assert torch.equal(a._sets[k].view(torch.int16), b._sets[k].view(torch.int16)), k
    assert a.rows_bytes == b.rows_bytes == 2 * m["M"] * (8 + 136)
    same(a.eval(pts), b.eval(pts), "to_band and half commute")
    same(a.eval(pts), a.float().eval(pts), "banded half against its float()")
    # a band below every |dist|: no rows, every point gets fill rows
    tiny = float(np.float32(np.abs(vol["dist"][vol["valid"]]).min() / 4))
    e = h.to_band(tiny)
    assert e.band_voxels.numel() == 0 and e.rows_dtype("s0") == torch.float16 and e.rows_bytes == 0
    out = e.eval(pts)
    assert not bool(out["in_band"].any()) and torch.equal(out["dist"], h.eval(pts)["dist"])
    assert torch.equal(out["s0"], e.fill_row("s0").expand(257, -1)) and torch.equal(out["s1"], torch.zeros(257, 136, device=dev))
    assert torch.equal(e.backward(pts, None, {"s0": torch.ones(257, 8, device=dev)}), torch.zeros(257, 3, device=dev))


# ---- Fusion.bake(rows_dtype=torch.float16) ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    """the scene of test_gpu_band.py's bake test: four 48 x 64 views, a 128-channel map, a 1-channel mask and a 3-component head"""
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
    return f, box, 2.0 ** -6, ["pca3", "dino_feats", "mask"]


@pytest.mark.parametrize("band", [None, 0.012])
def test_bake_in_chunks_equals_bake_then_half(dev, scene, band):
    f, box, step, names = scene
    whole = f.bake(box, step, return_names=names, band=band)
    want = whole.half()
    rows = want._sets["pca3"].numel() // 3
    budget = 4 * (3 + 128 + 1) * (rows // 5)                                # five or six chunks
    assert rows > 100 and -(-rows // (budget // (4 * 132))) >= 3
    got = f.bake(box, step, return_names=names, band=band, rows_dtype=torch.float16, max_rows_bytes=budget)
    assert got.names() == want.names() and (got.band is None) == (band is None) and got.rows_bytes == want.rows_bytes == 2 * rows * 132
    assert torch.equal(got.dist.view(torch.int32), want.dist.view(torch.int32)) and torch.equal(got.valid, want.valid) and torch.equal(got.cell_valid, want.cell_valid)
    if band is not None:
        assert torch.equal(got.slot, want.slot) and torch.equal(got.band_voxels, want.band_voxels)
    for k in names:
        assert got.rows_dtype(k) == torch.float16 and got._sets[k].shape == want._sets[k].shape, k
        a, b = got._sets[k].view(torch.int16), want._sets[k].view(torch.int16)
        if band is None:                                                    # (invalid voxels hold whatever the query wrote: compared too)
            a, b = a.view(-1, a.shape[-1]), b.view(-1, b.shape[-1])
        differ = int((a != b).sum())
        print("\n  bake %s %-10s %d of %d halves differ" % ("dense" if band is None else "banded", k, differ, a.numel()))
        assert differ == 0, (k, differ)
        assert torch.equal(got.fill_row(k), want.fill_row(k)), k
    pts = torch.from_numpy(np.random.default_rng(3).uniform([-0.18, -0.18, -0.21], [0.18, 0.12, 0.03], size=(257, 3)).astype(np.float32)).to(dev)
    same(got.eval(pts), want.eval(pts), "lookups of the two bakes")
    same(got.eval(pts), want.float().eval(pts), "and of the widened one")


# ---- rays -------------------------------------------------------------------------------------------------------------------------
def test_raycast_rows_come_through_the_half_lookup(dev):
    vol = BC.volume("large sphere holes band 1h", channels=(8, 136), fills=(0,))
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()}
    from d3fields_amd import BakedField
    f = BakedField.from_arrays(np.asarray(vol["origin"]).tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                               fills={"s0": torch.from_numpy(vol["fills"]["s0"]).to(dev)}, **sets)
    origins, dirs = (torch.from_numpy(a).to(dev) for a in BC.rays(vol))
    for field in (f, f.to_band(float(BC.band_of("large sphere holes band 1h")))):
        h = field.half()
        got = h.raycast(origins, dirs, return_names=["s0", "s1"], normals=True)
        want = h.float().raycast(origins, dirs, return_names=["s0", "s1"], normals=True)
        assert int(got["hit_mask"].sum()) >= 17 and list(got) == list(want)
        same(got, want, "raycast")
        K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1]], np.float32)
        ext = (np.asarray(vol["shape"]) - 1) * float(vol["step"])
        pose = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
        pose[:3, 3] = -(pose[:3, :3] @ (vol["centre"] + np.array([0.0, 0.0, 2.5 * ext.max()]))).astype(np.float32)
        same(h.render(K, pose, 24, 32, return_names=["s1"]), h.float().render(K, pose, 24, 32, return_names=["s1"]), "render")


# ---- what needs float32 rows ---------------------------------------------------------------------------------------------------------
def test_methods_with_row_loops_of_their_own(dev):
    """pool / links / flow / warp / align raise TypeError on a half field; after float() they give what the widened field gives; the methods
    that touch no rows work on the half field as they are"""
    vol = HC.case("5x4x6", (8, 136), 4, 0.0, False, (0,))
    h = half_field(vol, dev)
    wide = half_field(vol, dev, wide_names=("s0", "s1"))                  # the widened arrays, given as float32
    back = h.float()
    comps = wide.components(iso=float(np.median(vol["dist"])))
    pose = torch.empty((0, _lib.MOTION_POSE_DOUBLES), dtype=torch.float64, device=dev)
    owner = torch.zeros(vol["shape"], dtype=torch.int32, device=dev)
    pts = torch.from_numpy(HC.inside_points(vol["shape"], 64, 4)).to(dev)[None]
    tg = wide.eval(pts[0])["s0"][None].contiguous()
    calls = {
        "pool": lambda f: f.pool(comps.labels, count=comps.count),
        "links": lambda f: {"links": f.links("s1", tau=40.0, iso=float(np.median(vol["dist"]))).view(torch.int16)},
        "flow": lambda f: (lambda fl: {"target": fl.target, "cost": fl.cost})(f.flow(f, "s0", radius_voxels=1, iso=float(np.median(vol["dist"])))),
        "warp": lambda f: (lambda m: {"dist": m.dist, "s0": m._sets["s0"], "known": m.rows_known})(f.warp(pose, owner)),
        "align": lambda f: f.align(pts, name="s0", targets=tg, iters=2),
    }
    for who, call in calls.items():
        with pytest.raises(TypeError, match=r"float\("):
            call(h)
        got, want = call(back), call(wide)
        for k in want:
            if isinstance(want[k], torch.Tensor):
                x, y = got[k], want[k]
                if x.dtype in (torch.float32, torch.float64):
                    x, y = x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)
                assert torch.equal(x, y), (who, k)
    # no rows touched: the half field answers as the float32 one
    assert torch.equal(h.components(iso=float(np.median(vol["dist"]))).labels, comps.labels)
    assert torch.equal(h.clearance(iso=float(np.median(vol["dist"]))).dist, wide.clearance(iso=float(np.median(vol["dist"]))).dist)
