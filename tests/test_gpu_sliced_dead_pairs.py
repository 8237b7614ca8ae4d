"""Dead (point, view) pairs in the channel-sliced kernel, and the serpentine walk of its lattices.  A pair that failed the
depth test carries an all-zero corner record: its four loads go to texel 0 of the view and its term is +-0.
Every case compares the reordered launch (lattice brick walk or Hilbert-ordered cloud, `fused_eval_sliced_kernel`) with the
caller-order direct gather, NaN-aware torch.equal on `dist`, `valid_mask` and every map, and checks that the launch wrote
every output element (the outputs are pre-filled with a sentinel) -- which is also the device-side coverage of the
serpentine order of the macro-bricks (tests/test_walk_snake.py has the closed form's CPU mirror): the lattices have odd and
even macro-brick counts along y and z and a dimension of more than 32 tiles.  The cases are chosen for where a change to
how dead pairs are handled can go wrong: dead and live pairs mixed inside a wave and inside a point's views, views that
are dead in every wave, all-dead points and workgroups with clipped tiles and a ragged last group, a poisoned texel 0
(where the dead loads go: any dependence on its value or sign shows), a strict point among them, 1 / 3 / 8 slices, a
fp16-stored map, thin maps riding along."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32_SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces
U8_SENTINEL = 0xA5                 # valid_mask bytes are 0 or 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def lattice_box(nx, ny, nz, step, shift=(0.0, 0.0, 0.0)):
    """boundaries whose create_init_grid has exactly (nx, ny, nz) points, around the scene centre + shift"""
    return dict(x_lower=shift[0] - nx * step / 2, x_upper=shift[0] + nx * step / 2 - step / 4,
                y_lower=shift[1] - ny * step / 2, y_upper=shift[1] + ny * step / 2 - step / 4,
                z_lower=shift[2] - 0.2, z_upper=shift[2] - 0.2 + nz * step - step / 4)


# name: (points, depth kind, views with all-zero depth, C, (H, W), fp16 map, thin mask, poisoned texel 0)
#   points: ("lattice", dims, step, shift) or ("cloud", n, scale)
CASES = {
    # scattered holes: dead and live pairs mixed inside one wave and inside one point's views
    "holes-lattice-384": (("lattice", (70, 70, 17), 0.004, (0, 0, 0)), "stress", (), 384, (96, 128), False, False, False),
    "holes-cloud-384-mask": (("cloud", 70001, 1.0), "stress", (), 384, (96, 128), False, True, False),
    # one view without depth; two views of ONE group of views in flight without depth: that group is dead in every wave
    "view1-zero-lattice-128": (("lattice", (33, 35, 61), 0.004, (0, 0, 0)), "smooth", (1,), 128, (192, 256), False, False, False),
    "views23-zero-lattice-384": (("lattice", (64, 33, 37), 0.004, (0, 0, 0)), "smooth", (2, 3), 384, (96, 128), False, True, False),
    "views01-zero-cloud-1024": (("cloud", 66000, 1.0), "smooth", (0, 1), 1024, (96, 128), False, False, False),
    # the box overhangs every image on one side: all-dead points and 16-point workgroups, clipped tiles, a ragged last group
    "overhang-lattice-384": (("lattice", (71, 69, 19), 0.012, (0.9, 0, 0)), "smooth", (), 384, (96, 128), False, False, False),
    "overhang-cloud-384": (("cloud", 65537, 3.0), "smooth", (), 384, (96, 128), False, False, False),
    # texel 0 of every view at -3e38 (fp16: -60000): a dead pair's load that reaches it with a weight, or a dependence on its sign, shows
    "texel0-lattice-384": (("lattice", (70, 70, 17), 0.004, (0, 0, 0)), "stress", (), 384, (96, 128), False, False, True),
    "texel0-lattice-1024": (("lattice", (33, 35, 61), 0.004, (0, 0, 0)), "stress", (3,), 1024, (96, 128), False, False, True),
    "texel0-f16-lattice-384": (("lattice", (47, 53, 29), 0.004, (0, 0, 0)), "stress", (), 384, (192, 256), True, True, True),
    "texel0-f16-cloud-384": (("cloud", 131072, 1.5), "stress", (0,), 384, (192, 256), True, False, True),
}


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


@pytest.mark.parametrize("case", sorted(CASES))
def test_sliced_launch_with_dead_pairs_is_bit_identical(dev, case, monkeypatch):
    from d3fields_amd import Fusion, create_init_grid, synth, _lib
    points, kind, zero_views, C, (H, W), half, mask, poison = CASES[case]
    V = 4
    sc = synth.make_scene(V, H, W, kind)
    depth = sc["depth"].clone()
    for v in zero_views:
        depth[v] = 0.0
    feats = synth.random_map(V, H, W, C, seed=1, device=dev)
    if half:
        feats = (feats * 2.0).half()
    if poison:
        feats[:, 0, 0, :] = -60000.0 if half else -3e38
    maps = {"dino_feats": feats}
    names = ["dino_feats"]
    if mask:
        maps["mask"] = synth.random_onehot_mask(V, H, W, 8, seed=2, device=dev)
        names.append("mask")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = dict(maps, depth=depth.to(dev), K=sc["K"].to(dev), pose=sc["pose"].to(dev))
    f.H, f.W = H, W
    if points[0] == "lattice":
        _, dims, step, shift = points
        pts = create_init_grid(lattice_box(*dims, step, shift), step)[0]
        assert pts.shape[0] == dims[0] * dims[1] * dims[2]
    else:
        pts = synth.random_cloud(points[1], seed=5) * points[2]
    assert 65536 <= pts.shape[0] <= 131072
    pts[4322, 1] = float("nan")                                                        # a strict point among the dead pairs
    pts = pts.to(dev)
    with torch.no_grad():
        f.tuning_flags = _lib.TUNE_NO_REORDER | _lib.TUNE_DIRECT_GATHER
        f.record_plans = True
        base = f.batch_eval(pts, return_names=names)
        assert "sliced" not in f.last_plan()["kernel"], f.last_plan()
        f.tuning_flags = _lib.TUNE_FORCE_REORDER
        monkeypatch.setattr(torch, "empty", sentinel_empty(torch.empty))
        out = f.batch_eval(pts, return_names=names)
        monkeypatch.undo()
        plan = f.last_plan()
        assert plan["kernel"].startswith("fused_eval_sliced_kernel"), plan
        assert ("brick walk" if points[0] == "lattice" else "Hilbert") in plan["point_order"], plan
    # what the case is there for must be in it (the validity rule is dist / valid_mask's own)
    dead_points = float((~base["valid_mask"]).float().mean())
    print("%s: %d points, %.1f %% without a valid view, kernel %s" % (case, pts.shape[0], 100.0 * dead_points, plan["kernel"]))
    if case.startswith("overhang"):
        assert 0.2 <= dead_points <= 0.9, dead_points
    else:
        assert dead_points <= 0.9, dead_points
    # every element written exactly by the launch: no sentinel left
    assert int((out["valid_mask"].view(torch.uint8) > 1).sum()) == 0
    for k in ["dist"] + names:
        assert int((out[k].view(torch.int32) == F32_SENTINEL).sum()) == 0, k
    for k in ["dist", "valid_mask"] + names:
        a, b = out[k], base[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(b.float())), k
