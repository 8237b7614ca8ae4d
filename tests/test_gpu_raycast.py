"""The ray march through a baked volume (BakedField.raycast / render, d3f_volume_raycast, csrc/raycast_kernels.hip) against the float64
reference of tests/raycast_cases.py, ray by ray.

hit_mask (and the number of samples taken) equals the reference exactly on every ray the reference does not call fragile; at a hit
    |t - t64| <= tol scale_t + slack_t,   |point - point64| <= tol scale_p + slack_p   (raycast_cases.bound_terms)
with tol = 3 x the worst ratio of the float32 NumPy port measured in the same test, capped at 32 x 2^-24, and slack the coordinate term
4 G 2^-24 S of section 13 propagated through prev / (prev - s).  A miss is exactly t = 0 and a NaN row; t never holds a NaN.
On top of the bound, t and the points equal that port BIT FOR BIT on non-fragile rays (raycast_cases.assert_equals_port): every
operation of the contract is correctly rounded on both sides, so the kernel has no room to differ.

Mutants of the kernel and the assert that catches each:
  a + -> - test that also accepts - -> +   test_rays_against_float64, hit_mask: every case of 63 rays or more holds rays that meet the
                                           surface from behind -- every eighth random ray and the 'back face' special -- and would hit
                                           (shown on the host: test_raycast_host.py::test_a_back_face_hit_fails_the_hit_assert)
  prev kept across an invalid sample       test_rays_against_float64 on the volumes with holes: a ray whose + sample and - sample lie on
                                           either side of a hole would hit across it -- hit_mask and the sample counts differ
  an accumulated t_k                       test_rays_against_float64, raycast_cases.assert_equals_port: t and the points equal the float32 port
                                           bit for bit on non-fragile rays.  The error bound does NOT catch this mutant (the marches are short
                                           and t0 dominates k dt); the bitwise assert does, on every 1003-ray half-step case
                                           (shown on the host: test_raycast_host.py::test_an_accumulated_t_k_fails_the_bitwise_assert)
  K + 1 versus K samples                   test_rays_against_float64: `samples` of every miss that crossed the box is K + 1 exactly
  the clamp of g missing                   test_rays_against_float64: the first and last sample of a ray sit ON a face; unclamped, rounding
                                           puts some outside, the cell index leaves the volume (on 2x2x2 at once) -- hit_mask / samples differ
  u and v swapped                          test_render_against_float64 at 16 x 12 and 17 x 9 (not square, cx != cy) and test_render_equals_raycast
  R used instead of R^T                    the same two tests: the pose is no symmetric rotation, and o = -R^T tc moves with it
"""
import numpy as np
import pytest
import torch

import raycast_cases as RC
import volume_cases as VC

pytestmark = pytest.mark.gpu

CASES = RC.case_list()


def case_id(c):
    (shape, kind, family, holes), n, variant = c
    return "%s-%s-%s-%s-N%d-%s" % (shape, kind, family, "holes" if holes else "solid", n, variant.replace(" ", "_"))


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


def check_march(vol, o, d, kw, ref, t, hit, pts, samples, label):
    port = RC.march(vol, o, d, f=np.float32, **kw)
    keep = ~ref["fragile"]
    assert t.dtype == np.float32 and pts.dtype == np.float32 and hit.dtype == np.bool_ and t.shape == ref["t"].shape and pts.shape == ref["points"].shape, label
    assert not np.isnan(t).any(), label
    assert np.array_equal(hit[keep], ref["hit"][keep]), (label, "hit_mask")
    if samples is not None:
        assert np.array_equal(samples[keep], ref["samples"][keep]), (label, "samples")
    assert np.all(t[~hit] == 0) and np.isnan(pts[~hit]).all() and np.all(t[hit] > 0) and np.isfinite(pts[hit]).all(), (label, "misses are 0 and NaN")
    port_worst = RC.worst_ratios(port["t"], port["points"], ref, keep)
    tol = RC.tolerance(port_worst)
    got_worst = RC.worst_ratios(t, pts, ref, keep)
    differ = int((t[keep] != port["t"][keep]).sum())
    print("\n  %-52s fragile %4.1f %%  hits %4d  port worst ratio %.3g  tol %.3g  kernel worst ratio %.3g  t differs from the port on %d rays"
          % (label, 100 * ref["fragile"].mean(), int(ref["hit"].sum()), port_worst, tol, got_worst, differ))
    assert got_worst <= tol, (label, got_worst, tol)
    RC.assert_equals_port(t, hit, pts, samples, port, keep, label)


def march_on_device(f, o, d, kw, dev):
    t, hit, pts, cnt = f._march(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), None, o.shape[0], kw["march_step"], kw["t_near"], kw["t_far"], samples=True)
    torch.cuda.synchronize()
    return t.cpu().numpy(), hit.cpu().numpy(), pts.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_rays_against_float64(dev, c):
    vol, o, d, kw, ref = RC.case(*c)
    f = field_of(vol, dev)
    t, hit, pts, cnt = march_on_device(f, o, d, kw, dev)
    check_march(vol, o, d, kw, ref, t, hit, pts, cnt, case_id(c))
    out = f.raycast(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), **kw)          # the public method: the same launch
    assert list(out) == ["t", "hit_mask", "points"] and out["hit_mask"].dtype == torch.bool
    assert np.array_equal(out["t"].cpu().numpy(), t) and np.array_equal(out["hit_mask"].cpu().numpy(), hit)
    assert np.array_equal(out["points"].cpu().numpy(), pts, equal_nan=True)


# ---- the camera source ------------------------------------------------------------------------------------------------------------
def camera_for(vol, H, W):
    """a camera on the free side that sees the whole box and more (so some pixels miss), rotated about all three axes"""
    c, nrm = vol["centre"], vol["normal"]
    ext = (np.asarray(vol["shape"]) - 1) * float(vol["step"])
    eye = c + 1.6 * ext.max() * nrm + np.array([0.21, -0.13, 0.05]) * ext.max()
    z = (c - eye) / np.linalg.norm(c - eye)
    x = np.cross(z, [0.1, 0.2, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                                  # world -> camera
    pose = np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32)
    fx = 0.9 * W
    K = np.array([[fx, 0, 0.5 * W - 0.3], [0, 1.1 * fx, 0.5 * H + 0.4], [0, 0, 1]], np.float32)
    return K, pose


@pytest.mark.parametrize("HW", [(12, 16), (9, 17)], ids=["16x12", "17x9 ragged tiles"])
@pytest.mark.parametrize("key", [("9x8x10", "plane", "pow2", True), ("9x8x10", "sphere", "4mm", False), ("5x4x6", "sphere", "pow2", False)],
                         ids=lambda k: "-".join(map(str, k)))
def test_render_against_float64(dev, key, HW):
    H, W = HW
    vol = RC.make_volume(*key)
    K, pose = camera_for(vol, H, W)
    o1, d = RC.camera_rays(K, pose, H, W)
    o = np.broadcast_to(o1, d.shape).copy()
    kw = {"march_step": np.float32(vol["step"]), "t_near": 0.0, "t_far": np.inf}
    ref = RC.march(vol, o, d, **kw)
    assert ref["fragile"].mean() <= 0.03 and 0 < ref["hit"].sum() < H * W, (ref["fragile"].mean(), ref["hit"].sum())
    f = field_of(vol, dev)
    out = f.render(torch.from_numpy(K), torch.from_numpy(pose).to(dev), H, W, normals=True)
    torch.cuda.synchronize()
    assert list(out) == ["depth", "hit_mask", "points", "normal"]
    assert tuple(out["depth"].shape) == (H, W) and tuple(out["hit_mask"].shape) == (H, W) and tuple(out["points"].shape) == (H, W, 3) and tuple(out["normal"].shape) == (H, W, 3)
    t, hit, pts = out["depth"].cpu().numpy().reshape(-1), out["hit_mask"].cpu().numpy().reshape(-1), out["points"].cpu().numpy().reshape(-1, 3)
    check_march(vol, o, d, kw, ref, t, hit, pts, None, "render %dx%d %s" % (W, H, "-".join(map(str, key))))
    assert np.array_equal(hit, t > 0)
    # the camera depth: a hit's point has z = depth in camera coordinates (to float32 rounding of the point)
    zc = pts[hit].astype(np.float64) @ pose[2, :3].astype(np.float64) + float(pose[2, 3])
    assert np.all(np.abs(zc - t[hit]) <= 1e-5 * np.abs(pts[hit]).sum(1) + 1e-5 * t[hit])


@pytest.mark.parametrize("HW", [(12, 16), (9, 17)], ids=["16x12", "17x9 ragged tiles"])
def test_render_equals_raycast_on_host_built_rays(dev, HW):
    """depth[v, u] of render == t of raycast on the rays the host builds by the same formulas (pixel (u, v) = ray v W + u): bit for
    bit, which is inside any bound -- the two sources feed one march"""
    H, W = HW
    vol = RC.make_volume("9x8x10", "sphere", "pow2", True)
    K, pose = camera_for(vol, H, W)
    o1, d = RC.camera_rays(K, pose, H, W)
    f = field_of(vol, dev)
    img = f.render(K, pose, H, W)
    ray = f.raycast(torch.from_numpy(np.broadcast_to(o1, d.shape).copy()).to(dev), torch.from_numpy(d).to(dev))
    torch.cuda.synchronize()
    assert 0 < int(ray["hit_mask"].sum()) < H * W
    assert torch.equal(img["hit_mask"].view(-1), ray["hit_mask"])
    assert torch.equal(img["depth"].view(-1), ray["t"])
    assert np.array_equal(img["points"].view(-1, 3).cpu().numpy(), ray["points"].cpu().numpy(), equal_nan=True)
    assert not torch.equal(img["depth"], img["depth"].flip(1)) and tuple(img["depth"].shape) == (H, W)


# ---- rows and normals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 20, 384])
def test_rows_are_the_lookup_at_the_hit_points(dev, C):
    vol = RC.make_volume("9x8x10", "sphere", "pow2", True, (C, 5), (0, 1))
    o, d = RC.random_rays(vol, 1003, 2)
    so, sd = RC.special_rays(vol)
    o[:len(so)], d[:len(sd)] = so, sd
    f = field_of(vol, dev)
    out = f.raycast(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), return_names=["s1", "s0"], normals=True)
    torch.cuda.synchronize()
    assert list(out) == ["t", "hit_mask", "points", "normal", "s1", "s0"] and tuple(out["s0"].shape) == (1003, C) and tuple(out["s1"].shape) == (1003, 5)
    hit = out["hit_mask"]
    assert 200 < int(hit.sum()) < 800
    look = f.eval(out["points"])
    for k in ("s0", "s1"):
        assert torch.equal(out[k], look[k]), k                               # bit for bit, hits and misses
        fill = torch.from_numpy(vol["fills"][k]).to(dev)
        assert float(fill.abs().min()) > 0
        assert torch.equal(out[k][~hit], fill.expand(int((~hit).sum()), -1)), k
        assert not torch.isnan(out[k]).any(), k
    assert not bool(look["valid_mask"][~hit].any())
    with pytest.raises(KeyError):
        f.raycast(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), return_names=["nope"])


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_normals_on_the_plane(dev, family):
    """normal = grad dist / |grad dist| at the hit point.  The gradient itself is within section 13's bound of the float64 gradient at
    the kernel's own points; near the plane no corner of the point's cell is clamped, so that gradient is the plane's normal but for the
    float32 storage of the corners (2 x 2^-24 mu / h = 6 x 2^-24 per component); normalising a vector of length ~1 doubles an
    absolute error at most and adds the roundings of the norm and the division (4 x 2^-24)."""
    vol = RC.make_volume("9x8x10", "plane", family, False)
    o, d = RC.random_rays(vol, 1003, 3)
    f = field_of(vol, dev)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    out = f.raycast(do, dd, normals=True)
    torch.cuda.synchronize()
    hit = out["hit_mask"].cpu().numpy()
    nrm, pts = out["normal"].cpu().numpy(), out["points"].cpu().numpy()
    assert hit.sum() > 250 and (~hit).sum() > 100
    assert np.all(nrm[~hit] == 0)
    assert np.all(np.abs(np.linalg.norm(nrm[hit].astype(np.float64), axis=1) - 1) <= 4 * RC.U)
    grad = f.backward(out["points"], torch.ones(1003, device=dev)).cpu().numpy()
    want, B, T = VC.trilinear_grad64(vol, pts[hit], np.ones(int(hit.sum())))
    port = VC.trilinear_grad32(vol, pts[hit], np.ones(int(hit.sum()), np.float32))
    slack = VC.grad_coord_term(vol, T)[:, None]
    tol = VC.tolerance(VC.worst_ratio(port, want, B, slack))
    assert VC.worst_ratio(grad[hit], want, B, slack) <= tol
    assert np.all(np.abs(want - vol["normal"]) <= 6 * RC.U + 1e-12)
    bound = 2 * (tol * B + slack + 6 * RC.U) / np.linalg.norm(want, axis=1, keepdims=True) + 4 * RC.U
    err = np.abs(nrm[hit] - vol["normal"])
    print("\n  normals, %s: worst |normal - n| %.3g, bound there %.3g" % (family, err.max(), bound.reshape(err.shape)[np.unravel_index(err.argmax(), err.shape)]))
    assert np.all(err <= bound)
    assert np.all(nrm[hit] @ vol["normal"] > 0.999)                              # it points into free space


def test_two_runs_give_identical_bytes(dev):
    vol = RC.make_volume("9x8x10", "sphere", "4mm", True, (20,), (0,))
    o, d = RC.random_rays(vol, 1003, 5)
    f = field_of(vol, dev)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    K, pose = camera_for(vol, 9, 17)
    runs = []
    for _ in range(2):
        a = f.raycast(do, dd, return_names=["s0"], normals=True)
        b = f.render(K, pose, 9, 17, return_names=["s0"], normals=True)
        torch.cuda.synchronize()
        runs.append([v.cpu().numpy().tobytes() for v in list(a.values()) + list(b.values())])
    assert runs[0] == runs[1]


def test_input_checks(dev):
    vol = RC.make_volume("2x2x2", "plane", "pow2", False)
    f = field_of(vol, dev)
    z = torch.zeros(4, 3, device=dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f.raycast(torch.zeros(4, 3), z)
    with pytest.raises(TypeError):
        f.raycast(z, z.double())
    with pytest.raises(AssertionError):
        f.raycast(torch.zeros(4, 2, device=dev), z)
    with pytest.raises(ValueError, match="origins"):
        f.raycast(torch.zeros(5, 3, device=dev), z)
    with pytest.raises(ValueError, match="K must"):
        f.render(torch.eye(4), torch.eye(4), 4, 4)
    with pytest.raises(ValueError, match="pose must"):
        f.render(torch.eye(3), torch.eye(3), 4, 4)
    from d3fields_amd import _lib
    with pytest.raises(_lib.D3FError, match="march_step"):
        f.raycast(z, z, march_step=0.0)
    with pytest.raises(_lib.D3FError, match="steps"):
        f.raycast(z, z, march_step=1e-9)
    with pytest.raises(_lib.D3FError, match="t_near"):
        f.raycast(z, z, t_near=-1.0)
    # a set may carry the name of a ray output (from_arrays accepts it as before); only asking for it here is refused
    from d3fields_amd import BakedField
    g = BakedField.from_arrays((0, 0, 0), 0.5, torch.ones(2, 2, 2, device=dev), points=torch.zeros(2, 2, 2, 3, device=dev))
    assert tuple(g.eval(z)["points"].shape) == (4, 3)
    with pytest.raises(ValueError, match="output key"):
        g.raycast(z, z, return_names=["points"])
    empty = f.raycast(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), normals=True)
    assert tuple(empty["t"].shape) == (0,) and tuple(empty["points"].shape) == (0, 3) and tuple(empty["normal"].shape) == (0, 3)
    p = torch.zeros(4, 3, device=dev, requires_grad=True)
    out = f.raycast(p, z + 1.0, normals=True)
    assert not any(v.requires_grad for v in out.values())                      # no autograd through the march


def test_end_to_end_render_of_a_bake(dev):
    """Fusion.bake of the synthetic smooth scene at a coarse step, rendered from view 0's own K and pose at quarter resolution
    (K / 4: pixel (u, v) of the render looks along the ray of pixel (4u, 4v) of the observation)."""
    from d3fields_amd import Fusion, synth
    V, H, W = 4, 96, 128
    sc = synth.make_scene(V, H, W, "smooth")
    fu = Fusion(num_cam=V, device=str(dev))
    fu.curr_obs_torch = {"depth": sc["depth"].to(dev), "K": sc["K"].to(dev), "pose": sc["pose"].to(dev), "dino_feats": synth.random_map(V, 12, 16, 20, seed=4).to(dev)}
    fu.H, fu.W = H, W
    fu.add_projection("pca3", components=torch.randn(3, 20, generator=torch.Generator().manual_seed(8)))
    baked = fu.bake(synth.WORK_BOX, 0.01, return_names=["pca3"])
    K4 = sc["K"][0].clone()
    K4[:2] /= 4
    h, w = H // 4, W // 4
    out = baked.render(K4, sc["pose"][0], h, w, return_names=["pca3"], normals=True)
    torch.cuda.synchronize()
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == {
        "depth": ((h, w), torch.float32), "hit_mask": ((h, w), torch.bool), "points": ((h, w, 3), torch.float32), "normal": ((h, w, 3), torch.float32),
        "pca3": ((h, w, 3), torch.float32)}
    hit = out["hit_mask"]
    assert int(hit.sum()) > 0
    assert torch.equal(hit, out["depth"] > 0)
    at = baked.eval_dist(out["points"][hit])
    assert bool(at["valid_mask"].all()) and float(at["dist"].abs().max()) <= fu.mu
    seen = sc["depth"][0][::4, ::4].to(dev)
    both = hit & (seen > 0)
    diff = (out["depth"] - seen).abs()[both]
    print("\n  end to end: %d of %d pixels hit, %d in common with the observation; |depth - observed| median %.4g m, 99th percentile %.4g m (step 0.01 m)"
          % (int(hit.sum()), h * w, int(both.sum()), float(diff.median()), float(diff.quantile(0.99))))
