"""The baked-volume lookup (BakedField / d3f_volume_sample / d3f_volume_sample_backward, csrc/volume_kernels.hip) against the
float64 reference of tests/volume_cases.py, entry by entry.

Per entry, with G = max extent:  |got - ref64| <= tol * A + 4 G 2^-24 S   (A = sum_c w_c |v_c|, S = corner spread; the second
term is the rounding of the coordinates, volume_cases.coord_term).  tol = 3 x the worst ratio of the float32 NumPy port of the
chain, measured in the same test on the host, capped at 16 x 2^-24.  valid_mask equals the reference exactly.  The gradient:
the same with B = sum |grad| sum_c |dw_c/dt| |v_c| / h for A and T = sum |grad| S / h for S (volume_cases.grad_coord_term).

Mutants of the kernel and the assert that catches each:
  corner order swapped along one axis   test_sample_against_float64 (values) and test_lattice_points_are_bit_identical: a point on
                                        a far face (t = 1) must return the stored value of the corner at +1, the swap returns -1's
  n - 1 instead of n - 2 in the clamp   test_lattice_points_are_bit_identical / test_points_that_are_not_valid: a far-face point
                                        would take cell n - 1, whose byte does not exist, with t = 0 -- valid_mask / the value differ
  the sentinel blended, not rejected    test_sample_against_float64 on the volume with holes: valid_mask must equal the reference
                                        exactly and every row of such a point the fill row; the poisoned corners would give NaN
  fill row not applied (projected name) test_points_that_are_not_valid (non-zero fill rows) and test_end_to_end_bake (the -b row)
"""
import ctypes

import numpy as np
import pytest
import torch

import volume_cases as VC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

CHANNELS = [1, 3, 8, 16, 18, 20, 67, 68, 384, 1024]      # both instances, 16 | 18 / 20 across their boundary, vector and scalar rows, tails
VOLUMES = {"5x4x6 holes": ("5x4x6", 0.2, True), "5x4x6 solid": ("5x4x6", 0.0, False), "2x2x2": ("2x2x2", 0.0, False)}


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


def check_forward(vol, pts, ref, out, label):
    """valid_mask exactly; every entry within tol * A + coord_term; the sentinel and the fill rows exactly; no NaN anywhere"""
    port = VC.trilinear32(vol, pts)
    ok = ref["valid"]
    assert out["valid_mask"].dtype == torch.bool and np.array_equal(out["valid_mask"].cpu().numpy(), ok), label
    assert np.array_equal(port["valid"], ok), label
    names = ["dist"] + list(vol["sets"])
    port_worst = max(VC.worst_ratio(port[k], ref[k][0], ref[k][1], VC.coord_term(vol, ref[k][2])) for k in names)
    tol = VC.tolerance(port_worst)
    got_worst = 0.0
    for k in names:
        got = out[k].cpu().numpy()
        val, A, S = ref[k]
        assert got.dtype == np.float32 and got.shape == val.shape, (label, k)
        assert not np.isnan(got).any(), (label, k, "NaN in the output")
        got_worst = max(got_worst, VC.worst_ratio(got, val, A, VC.coord_term(vol, S)))
        assert np.array_equal(got[~ok], val[~ok].astype(np.float32)), (label, k, "sentinel / fill row")
    print("\n  %-40s port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (label, port_worst, tol, got_worst))
    assert got_worst <= tol, (label, got_worst, tol)


@pytest.mark.parametrize("n", [1, 63, 1003])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("volume", list(VOLUMES))
def test_sample_against_float64(dev, volume, C, n):
    shape_name, frac, poison = VOLUMES[volume]
    vol, pts, ref = VC.case(shape_name, (C,), n, C % len(VC.SEEDS), frac, poison)
    f = field_of(vol, dev)
    out = f.eval(torch.from_numpy(pts).to(dev))
    torch.cuda.synchronize()
    assert tuple(out["s0"].shape) == (n, C)
    check_forward(vol, pts, ref, out, "%s C=%d N=%d" % (volume, C, n))
    if n == 1003 and frac > 0:
        assert 0 < ref["valid"].sum() < n                      # both kinds of point are there


@pytest.mark.parametrize("channels", [(3, 384), (1, 3, 8, 16, 20, 68, 18, 67), (1024, 16, 4, 384, 20, 2, 1, 68)])
def test_several_sets_in_one_launch(dev, channels):
    """two sets and D3F_MAX_MAPS sets, narrow and wide mixed, some with a fill row; a subset of the names in another order"""
    assert len(channels) in (2, _lib.MAX_MAPS)
    vol, pts, ref = VC.case("5x4x6", channels, 1003, 3, 0.1, True, (0, len(channels) - 1))
    f = field_of(vol, dev)
    dpts = torch.from_numpy(pts).to(dev)
    out = f.batch_eval(dpts)
    torch.cuda.synchronize()
    assert list(out) == ["dist", "valid_mask"] + ["s%d" % s for s in range(len(channels))]
    check_forward(vol, pts, ref, out, "sets %s" % (channels,))
    some = f.eval(dpts, return_names=["s1", "s0"])
    assert list(some) == ["dist", "valid_mask", "s1", "s0"]
    assert all(torch.equal(some[k], out[k]) for k in some)
    d = f.eval_dist(dpts)
    assert list(d) == ["dist", "valid_mask"] and torch.equal(d["dist"], out["dist"]) and torch.equal(d["valid_mask"], out["valid_mask"])


@pytest.mark.parametrize("volume", list(VOLUMES))
def test_lattice_points_are_bit_identical(dev, volume):
    """At a lattice point (far faces included: last cell, t = 1) whose cell is fully valid the lookup returns the stored values
    bit for bit; elsewhere the sentinel and the fill row."""
    shape_name, frac, poison = VOLUMES[volume]
    shape = VC.SHAPES[shape_name]
    vol = VC.make_volume(shape, (3, 68, 67), 5, frac / 4, poison, (1,))
    lat = VC.lattice_points(shape)
    ok, i, t = VC.locate64(vol, lat)
    assert np.all((t == 0) | (t == 1)) and ok.any()
    f = field_of(vol, dev)
    out = f.eval(torch.from_numpy(lat).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(out["valid_mask"].cpu().numpy(), ok)
    assert np.array_equal(f.cell_valid.cpu().numpy().astype(bool), np.all([vol["valid"][dx:shape[0] - 1 + dx, dy:shape[1] - 1 + dy, dz:shape[2] - 1 + dz]
                                                                           for dx, dy, dz in VC.CORNERS], axis=0))
    got = out["dist"].cpu().numpy()
    assert np.array_equal(got[ok], vol["dist"].reshape(-1)[ok]) and np.all(got[~ok] == VC.SENTINEL)
    for k, arr in vol["sets"].items():
        got = out[k].cpu().numpy()
        assert np.array_equal(got[ok], arr.reshape(len(lat), -1)[ok]), k
        fill = np.zeros(arr.shape[3], np.float32) if vol["fills"][k] is None else vol["fills"][k]
        assert np.array_equal(got[~ok], np.broadcast_to(fill, got[~ok].shape)), k


def test_points_that_are_not_valid(dev):
    """Outside on every side, on each far face, NaN / infinite coordinates, a volume with 20 % invalid voxels scattered and NaN
    stored in them: valid_mask as the reference, exactly 1e3 and the (non-zero) fill rows, no NaN in any output."""
    shape = VC.SHAPES["5x4x6"]
    for frac in (0.0, 0.2):
        vol = VC.make_volume(shape, (3, 68), 6, frac, True, (0, 1))
        pts = np.concatenate([VC.special_points(shape), VC.inside_points(shape, 200, 6)])
        ref = VC.trilinear64(vol, pts)
        f = field_of(vol, dev)
        out = f.eval(torch.from_numpy(pts).to(dev))
        torch.cuda.synchronize()
        check_forward(vol, pts, ref, out, "special points, %.0f %% invalid voxels" % (100 * frac))
        ok = ref["valid"]
        assert 0 < ok.sum() < ok.size
        assert np.all(out["dist"].cpu().numpy()[~ok] == np.float32(1e3))
        for k in ("s0", "s1"):
            assert np.abs(vol["fills"][k]).min() > 0
            assert np.array_equal(out[k].cpu().numpy()[~ok], np.broadcast_to(vol["fills"][k], (int((~ok).sum()), vol["fills"][k].size)))
        if frac == 0.0:                                      # far-face points are valid here, with t = 1
            far = (np.asarray(VC.ORIGIN) + (np.asarray(shape) - 1) * VC.STEP).astype(np.float32)
            on_far = np.any(pts == far, axis=1) & np.all(np.isfinite(pts), axis=1)
            assert on_far.sum() >= 4 and ok[on_far & np.all(pts <= far, axis=1)].all()


def test_output_rows_off_16_bytes_equal_the_aligned_call(dev):
    """out_sets[s] 4-byte but not 16-byte aligned while the stored rows are (C = 8 on a 3x4x5 volume, 64 points; the entry point called
    directly): the set drops to scalar stores and gives the aligned call's rows bit for bit, and nothing beside them is written"""
    shape, n, C = (3, 4, 5), 64, 8
    vol = VC.make_volume(shape, (C,), 2, 0.1, True, (0,))
    f = field_of(vol, dev)
    lib = _lib.load()
    pts = torch.from_numpy(np.concatenate([VC.special_points(shape)[:8], VC.inside_points(shape, n - 8, 2)])).to(dev)
    assert f._sets["s0"].data_ptr() % 16 == 0 and f._sets["s0"].stride(-2) == C

    def run(offset):
        buf = torch.full((n * C + 8,), float("nan"), dtype=torch.float32, device=dev)
        rows = buf[offset:offset + n * C].view(n, C)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
        v = f._volume()
        _lib.check(lib.d3f_volume_sample(ctypes.byref(v), _lib.ptr(pts), n, f._set_array(["s0"]), 1, _lib.ptr(dist), _lib.ptr(valid),
                                         (ctypes.c_void_p * 1)(rows.data_ptr()), _lib.current_stream_handle(dev)))
        torch.cuda.synchronize()
        assert rows.data_ptr() % 16 == 4 * offset and bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n * C:]).all())
        return rows.view(torch.int32), dist.view(torch.int32), valid

    aligned, shifted = run(0), run(1)
    assert all(torch.equal(a, b) for a, b in zip(aligned, shifted))
    assert 0 < int(aligned[2].sum()) < n and not bool(torch.isnan(aligned[0].view(torch.float32)).any())
    assert torch.equal(aligned[0].view(torch.float32), f.eval(pts)["s0"])


BACKWARD = [((), 1003), ((3,), 1003), ((16,), 63), ((18,), 1003), ((20,), 1), ((68,), 1003), ((67,), 63), ((384,), 1003), ((1024,), 63),
            ((3, 384, 18), 1003), ((1, 3, 8, 16, 20, 68, 18, 67), 63)]


@pytest.mark.parametrize("channels,n", BACKWARD)
@pytest.mark.parametrize("volume", ["5x4x6 holes", "2x2x2"])
def test_backward_against_float64(dev, volume, channels, n):
    """grad_dist only, sets only (one of them without a gradient), both; zero rows where not valid; torch.autograd through
    BakedField.eval gives the entry point's numbers."""
    shape_name, frac, poison = VOLUMES[volume]
    vol, pts, ref = VC.case(shape_name, channels, n, 7, frac / 2, poison)
    rng = np.random.default_rng(11)
    names = list(vol["sets"])
    gd = rng.standard_normal(n).astype(np.float32)
    gs = {k: rng.standard_normal((n, vol["sets"][k].shape[3])).astype(np.float32) for k in names}
    f = field_of(vol, dev)
    dpts = torch.from_numpy(pts).to(dev)
    ok = ref["valid"]
    modes = [("dist", gd, {})] + ([("sets", None, dict(gs, **({names[0]: None} if len(names) > 1 else {}))), ("both", gd, gs)] if names else [])
    for mode, d, s in modes:
        got = f.backward(dpts, None if d is None else torch.from_numpy(d).to(dev), {k: (None if g is None else torch.from_numpy(g).to(dev)) for k, g in s.items()})
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        want, B, T = VC.trilinear_grad64(vol, pts, d, s)
        port = VC.trilinear_grad32(vol, pts, d, s)
        slack = VC.grad_coord_term(vol, T)[:, None]
        port_worst = VC.worst_ratio(port, want, B, slack)
        tol = VC.tolerance(port_worst)
        got_worst = VC.worst_ratio(got, want, B, slack)
        print("\n  %-14s %-34s N=%-5d %-5s port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g" % (volume, channels, n, mode, port_worst, tol, got_worst))
        assert got.shape == (n, 3) and not np.isnan(got).any()
        assert np.all(got[~ok] == 0)
        assert got_worst <= tol, (mode, got_worst, tol)
        if ok.any():
            assert np.abs(got[ok]).max() > 0
    # autograd: the same numbers as the entry point
    p = dpts.clone().requires_grad_(True)
    out = f.eval(p)
    assert not out["valid_mask"].requires_grad
    loss = (out["dist"] * torch.from_numpy(gd).to(dev)).sum()
    for k in names:
        loss = loss + (out[k] * torch.from_numpy(gs[k]).to(dev)).sum()
    loss.backward()
    direct = f.backward(dpts, torch.from_numpy(gd).to(dev), {k: torch.from_numpy(g).to(dev) for k, g in gs.items()})
    assert torch.equal(p.grad, direct)
    with torch.no_grad():
        plain = f.eval(dpts)
    assert all(torch.equal(plain[k], out[k].detach()) for k in plain)


def test_input_checks(dev):
    vol = VC.make_volume((2, 2, 2), (3,), 0)
    f = field_of(vol, dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f.eval(torch.zeros(4, 3))
    with pytest.raises(TypeError):
        f.eval(torch.zeros(4, 3, dtype=torch.float64, device=dev))
    with pytest.raises(AssertionError):
        f.eval(torch.zeros(4, 2, device=dev))
    with pytest.raises(KeyError):
        f.eval(torch.zeros(4, 3, device=dev), return_names=["nope"])
    empty = f.eval(torch.zeros(0, 3, device=dev))
    assert tuple(empty["dist"].shape) == (0,) and tuple(empty["s0"].shape) == (0, 3)
    assert f.grid_shape == torch.Size([2, 2, 2]) and f.step == VC.STEP and set(f.boundaries) == {"x_lower", "x_upper", "y_lower", "y_upper", "z_lower", "z_upper"}
    assert abs(f.boundaries["x_lower"] - (VC.ORIGIN[0] - VC.STEP / 2)) < 1e-12


def test_end_to_end_bake(dev):
    """Fusion.bake on the synthetic smooth scene (two views of 48 x 64, a 12 x 16 x 20 feature map, a 3-component head, a
    12 x 10 x 8 grid whose step is a power of two, so the lattice is exact in float32): at the lattice points the lookup equals
    eval_grid's tensors bit for bit where the cell is fully valid and the sentinel / fill row elsewhere; the projected name's
    fill row is what Fusion.eval gives an all-invalid point; the field answers the same after update() with another observation."""
    from d3fields_amd import BakedField, Fusion, create_init_grid, synth
    V, H, W = 2, 48, 64
    sc = synth.make_scene(V, H, W, "smooth")
    feats = synth.random_map(V, 12, 16, 20, seed=4)
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {"depth": sc["depth"].to(dev), "K": sc["K"].to(dev), "pose": sc["pose"].to(dev), "dino_feats": feats.to(dev)}
    f.H, f.W = H, W
    head = torch.randn(3, 20, generator=torch.Generator().manual_seed(8))
    f.add_projection("pca3", components=head, mean=torch.randn(20, generator=torch.Generator().manual_seed(9)))
    box = dict(x_lower=-0.1875, x_upper=0.1875, y_lower=-0.1875, y_upper=0.125, z_lower=-0.21875, z_upper=0.03125)
    step = 2.0 ** -5
    names = ["pca3", "dino_feats"]
    baked = f.bake(box, step, return_names=names)
    assert isinstance(baked, BakedField) and baked.grid_shape == torch.Size([12, 10, 8]) and baked.names() == names
    assert baked.boundaries == box and baked.step == step
    with torch.no_grad():
        grid = f.eval_grid(box, step, return_names=names)
    lat = create_init_grid(box, step)[0].to(dev)
    out = baked.eval(lat)
    torch.cuda.synchronize()
    # the cell of a lattice point: its own, or the last one on a far face
    valid = grid["valid_mask"].view(12, 10, 8).cpu().numpy()
    cell = np.all([valid[dx:11 + dx, dy:9 + dy, dz:7 + dz] for dx, dy, dz in VC.CORNERS], axis=0)
    ix, iy, iz = np.meshgrid(np.minimum(np.arange(12), 10), np.minimum(np.arange(10), 8), np.minimum(np.arange(8), 6), indexing="ij")
    ok = torch.from_numpy(cell[ix, iy, iz].reshape(-1)).to(dev)
    assert 0 < int(ok.sum()) < ok.numel(), "the grid must hold fully valid cells and others"
    assert torch.equal(out["valid_mask"], ok)
    assert torch.equal(out["dist"][ok], grid["dist"][ok]) and bool((out["dist"][~ok] == 1e3).all())
    far = torch.full((1, 3), 50.0, device=dev)
    with torch.no_grad():
        dead = f.eval(far, return_names=names)
    assert not bool(dead["valid_mask"][0]) and bool(dead["pca3"].abs().sum() > 0)
    for k in names:
        assert torch.equal(out[k][ok], grid[k][ok]), k
        assert torch.equal(out[k][~ok], dead[k].expand(int((~ok).sum()), -1)), k
        assert torch.equal(baked.fill_row(k), dead[k][0]), k
    # off the lattice, and after another observation
    pts = (torch.rand(500, 3, generator=torch.Generator().manual_seed(10)) * torch.tensor([0.34, 0.28, 0.21]) + torch.tensor([-0.17, -0.17, -0.2])).to(dev)
    before = baked.eval(pts)
    f.update({"color": np.zeros((V, H, W, 3), np.uint8), "depth": sc["depth"].numpy() * 1.07, "pose": sc["pose"].numpy(), "K": sc["K"].numpy(),
              "dino_feats": synth.random_map(V, 12, 16, 20, seed=5)})
    with torch.no_grad():
        assert not torch.equal(f.eval_grid(box, step, return_names=names)["dist"], grid["dist"])
    after = baked.eval(pts)
    assert all(torch.equal(before[k], after[k]) for k in before) and bool(before["valid_mask"].any())
