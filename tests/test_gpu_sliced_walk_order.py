"""The channel-sliced kernel at small shapes: the lattice walk on the device (csrc/fuse_common.h: walk_tile, the macro-bricks as a
serpentine on fp32 maps) and the dead (point, view) pairs of the fp32 instance, which ask for no texel (range-checked buffer
loads, csrc/fuse_sliced.hip).  The sliced family is forced with D3F_TUNE_FORCE_REORDER (through Fusion.eval_grid, so that
lattices below 65 536 points take the walk too) and compared with the caller-order direct gather of the materialised grid
(D3F_TUNE_DIRECT_GATHER): every output element written (the outputs are pre-filled with a sentinel), and `valid_mask`, `dist`
and every row torch.equal.  Lattices, in points, walked in tiles of 2x2x1 (a wide map alone) or 2x2x2 (a thin mask riding
along): several macro-bricks with clipped blocks at every level, a lattice inside one sub-brick, a single tile, a dimension of
1; C = 384 (three slices) and 128 (one), four views and three (a last view alone behind the pairs in flight).  Scenes with
one view dead, with a whole pair of views in flight dead, and with a box that overhangs the images (whole workgroups dead).
The same cases run once on fp16-stored maps, whose kernel instance and row-major order are as they were.
tests/test_walk_order_host.py holds the NumPy restatement of the walk's closed form."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

F32_SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
U8_SENTINEL = 0xA5                 # valid_mask bytes are 0 or 1
H, W = 96, 128

LATTICES = {"66x34x35": (66, 34, 35), "35x19x9": (35, 19, 9), "2x2x1": (2, 2, 1), "40x1x37": (40, 1, 37)}
# scene name: (depth kind, views with all-zero depth, step, shift of the box)
SCENES = {
    "plain": ("smooth", (), 0.004, (0.0, 0.0, 0.0)),
    "view1-dead": ("smooth", (1,), 0.004, (0.0, 0.0, 0.0)),
    "views23-dead": ("stress", (2, 3), 0.004, (0.0, 0.0, 0.0)),           # a whole group of views in flight
    "overhang": ("smooth", (), 0.012, (0.9, 0.0, 0.0)),                  # all-dead points and whole dead workgroups
}
CASES = [(lat, "plain", C, V, mask) for lat in LATTICES for C in (384, 128) for V in (4, 3) for mask in (False, True)]
CASES += [("66x34x35", scene, C, 4, mask) for scene in ("view1-dead", "views23-dead", "overhang") for C, mask in ((384, False), (128, True))]
CASES += [("35x19x9", "overhang", 384, 4, False)]


def lattice_box(nx, ny, nz, step, shift):
    """boundaries whose create_init_grid has exactly (nx, ny, nz) points, around the scene centre + shift"""
    return dict(x_lower=shift[0] - nx * step / 2, x_upper=shift[0] + nx * step / 2 - step / 4,
                y_lower=shift[1] - ny * step / 2, y_upper=shift[1] + ny * step / 2 - step / 4,
                z_lower=shift[2] - 0.2, z_upper=shift[2] - 0.2 + nz * step - step / 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shared(dev):
    """maps, scenes and the direct-gather references, computed once and left unchanged"""
    return {}


def sentinel_empty(real_empty):
    """torch.empty whose float32 / bool results start out as sentinels (what torch.empty returns is unspecified anyway)"""
    def empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.is_cuda and t.dtype == torch.float32:
            t.view(torch.int32).fill_(F32_SENTINEL)
        elif t.is_cuda and t.dtype == torch.bool:
            t.view(torch.uint8).fill_(U8_SENTINEL)
        return t
    return empty


def fusion_for(shared, dev, scene, C, V, mask, half):
    from d3fields_amd import Fusion, synth
    kind, zero_views, _, _ = SCENES[scene]
    key = ("fusion", scene, C, V, mask, half)
    if key not in shared:
        if ("feats", C, V) not in shared:
            shared[("feats", C, V)] = synth.random_map(V, H, W, C, seed=1, device=dev)
        if ("mask", V) not in shared:
            shared[("mask", V)] = synth.random_onehot_mask(V, H, W, 8, seed=2, device=dev)
        feats = shared[("feats", C, V)]
        if half:
            if ("feats16", C, V) not in shared:
                shared[("feats16", C, V)] = (feats * 2.0).half()
            feats = shared[("feats16", C, V)]
        sc = synth.make_scene(V, H, W, kind)
        depth = sc["depth"].clone()
        for v in zero_views:
            depth[v] = 0.0
        maps = {"dino_feats": feats}
        if mask:
            maps["mask"] = shared[("mask", V)]
        f = Fusion(num_cam=V, device=str(dev))
        f.curr_obs_torch = dict(maps, depth=depth.to(dev), K=sc["K"].to(dev), pose=sc["pose"].to(dev))
        f.H, f.W = H, W
        shared[key] = f
    return shared[key]


def planned_kernel(dims, C, V, mask, half, flags):
    """what d3f_eval_plan_query_lattice names for these shapes and flags (no device work)"""
    from d3fields_amd import Fusion, _lib
    stub = types.SimpleNamespace(_lib=_lib.load(), _last_plan=None)
    shapes = [(H, W, C)] + ([(H, W, 8)] if mask else [])
    arr = (_lib.ChannelMap * len(shapes))()
    for i, (fh, fw, c) in enumerate(shapes):
        arr[i] = _lib.ChannelMap(16, fh, fw, c, _lib.DTYPE_F16 if (half and i == 0) else _lib.DTYPE_F32, fh * fw * c, fw * c, c)
    Fusion._record_plan(stub, _lib.Views(V, H, W, 16, 16, 16), dims[0] * dims[1] * dims[2], arr, len(shapes), flags, False, False, dims)
    assert stub._last_plan is not None
    return stub._last_plan


def same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float()))


def run_case(shared, dev, monkeypatch, lat, scene, C, V, mask, half):
    from d3fields_amd import create_init_grid, _lib
    dims = LATTICES[lat]
    _, _, step, shift = SCENES[scene]
    box = lattice_box(*dims, step, shift)
    names = ["dino_feats"] + (["mask"] if mask else [])
    f = fusion_for(shared, dev, scene, C, V, mask, half)
    with torch.no_grad():
        key = ("base", lat, scene, C, V, mask, half)
        if key not in shared:
            pts, shape = create_init_grid(box, step)
            assert tuple(shape) == dims and pts.shape[0] == dims[0] * dims[1] * dims[2]
            f.tuning_flags = _lib.TUNE_NO_REORDER | _lib.TUNE_DIRECT_GATHER
            f.record_plans = True
            shared[key] = f.batch_eval(pts.to(dev), return_names=names)
            assert "sliced" not in f.last_plan()["kernel"], f.last_plan()
        base = shared[key]
        f.tuning_flags = _lib.TUNE_FORCE_REORDER
        monkeypatch.setattr(torch, "empty", sentinel_empty(torch.empty))
        out = f.eval_grid(box, step, return_names=names)
        monkeypatch.undo()
    assert tuple(out["grid_shape"]) == dims
    plan = planned_kernel(dims, C, V, mask, half, _lib.TUNE_FORCE_REORDER)
    if not half:
        assert plan["kernel"].startswith("fused_eval_sliced_kernel<5, 2, 7>") and "brick walk" in plan["point_order"], plan
    elif C == 384:
        assert plan["kernel"].startswith("fused_eval_sliced_kernel<4, 2, 7, true>") and "brick walk" in plan["point_order"], plan
    dead_points = float((~base["valid_mask"]).float().mean())
    print("%s %s C=%d V=%d mask=%s half=%s: %.1f %% of the points without a valid view, kernel %s"
          % (lat, scene, C, V, mask, half, 100.0 * dead_points, plan["kernel"]))
    if scene == "overhang":
        assert 0.2 <= dead_points < 1.0, dead_points
    # every element written by the launch: no sentinel left
    assert int((out["valid_mask"].view(torch.uint8) > 1).sum()) == 0
    for k in ["dist"] + names:
        assert int((out[k].view(torch.int32) == F32_SENTINEL).sum()) == 0, k
    for k in ["dist", "valid_mask"] + names:
        assert same(out[k], base[k]), k


def case_id(c):
    return "%s-%s-C%d-V%d%s" % (c[0], c[1], c[2], c[3], "-mask" if c[4] else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sliced_walk_equals_the_direct_gather(shared, dev, monkeypatch, case):
    run_case(shared, dev, monkeypatch, *case, half=False)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp16_stored_maps_take_the_walk_they_took(shared, dev, monkeypatch, case):
    run_case(shared, dev, monkeypatch, *case, half=True)
