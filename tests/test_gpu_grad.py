"""Point gradients of the HIP backward kernels against the float64 reference (oracle/grad_ref.py), point by point.

fused_eval_backward_kernel<0> (Fusion.eval), <1> (Fusion.eval_dist) and the gradient inside track_step_kernel
(d3f_track_step) and the five-launch step, at the tile sizes, map layouts, branch edges and non-finite inputs where a
kernel goes wrong.  Every entry must meet |g - g64| <= grad_ref.TOL * scale (scale: the sum of |contributions| of the
entry), and the non-finite entries must be the reference's exactly.  Upstream gradients are random normals.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import grad_ref as R
from oracle.grad_cases import (EH, EW, MU_EDGE, TILE_CASES, backward_tile, edge_maps, edge_points, edge_scene,  # noqa: F401
                                layout_maps, normals, poison, scene)

pytestmark = pytest.mark.gpu
SAMPLE = 20000            # rows checked of a large batch (a point's gradient depends on its own row only)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def fusion(dev, obs, maps, H, W, mu=0.02):
    from d3fields_amd import Fusion
    f = Fusion(num_cam=obs["depth"].shape[0], device=str(dev))
    f.mu = mu
    f.curr_obs_torch = {k: obs[k].to(dev, torch.float32).contiguous() for k in ("depth", "K", "pose")}
    for k, m in maps.items():
        f.curr_obs_torch[k] = m.to(dev) if m.device != dev else m
    f.H, f.W = int(H), int(W)
    return f


def kernel_grad(f, pts, names, gd, gks, mode="eval"):
    """grad_pts of the HIP backward for loss = <gd, dist> + sum <gks[k], fused_k> (gks[k] None: no upstream gradient)."""
    dev = torch.device(f.device)
    p = pts.to(dev)
    if mode == "eval_dist":
        p = p.clone().requires_grad_(True)
        out = f.eval_dist(p)
        (out["dist"] * gd.to(dev)).sum().backward()
        return p.grad.cpu()
    out, saved = f._launch(p.contiguous(), names, False, "eval")
    g = f._backward(saved, gd.to(dev) if gd is not None else None, [None if x is None else x.to(dev) for x in gks])
    torch.cuda.synchronize()
    return g.cpu()


def compare(g, obs, pts, H, W, mu, maps, gd, gks, mode="eval", rows=None):
    sub = (lambda t: t) if rows is None else (lambda t: None if t is None else t[rows])
    g64, sc, dec = R.field_grad(obs, pts, H, W, mu, maps, gd, gks, mode=mode, rows=rows)
    ok, worst, msg = R.check(sub(g), g64, sc)
    assert ok, msg
    return g64, dec


# ---- tile sizes and LDS paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,V,N,C,tile", TILE_CASES)
def test_backward_tiles_against_float64(dev, mode, V, N, C, tile):
    from d3fields_amd import synth
    assert backward_tile(V, N) == tile, "the case no longer runs the tile it is meant for"
    H, W = 48, 64
    obs = scene(V, H, W, "stress" if V in (4, 30) else "smooth")
    pts = synth.random_cloud(N, seed=V + N)
    gd = normals(1, N)
    maps, gks, names = [], [], []
    if mode == "eval":
        maps = [synth.random_map(V, 12, 16, C, seed=2)]
        gks = [normals(3, N, C)]
        names = ["dino_feats"]
    f = fusion(dev, obs, dict(zip(names, maps)), H, W)
    g = kernel_grad(f, pts, names, gd, gks, mode)
    rows = None if N <= SAMPLE else torch.randperm(N, generator=torch.Generator().manual_seed(5))[:SAMPLE]
    g64, dec = compare(g, obs, pts, H, W, 0.02, maps, gd, gks, mode, rows)
    assert dec["valid"].any(), "no valid view: the case tests nothing"


# ---- map layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,none_mask", [
    ("fp16_vec8", ()), ("fp16_scalar", ()), ("slice_unaligned", ()), ("slice_aligned", ()), ("row_1xW", ()), ("col_Hx1", ()),
    ("full_res", ()), ("three_maps", (1,)), ("three_maps", (0, 2)),
])
def test_backward_map_layouts_against_float64(dev, kind, none_mask):
    from d3fields_amd import synth
    V, H, W, N = 4, 48, 64, 3000
    obs = scene(V, H, W)
    maps = layout_maps(kind, V, H, W)
    pts = synth.random_cloud(N, seed=21)
    gd = normals(22, N)
    gks = [None if k in none_mask else normals(23 + k, N, m.shape[3]) for k, m in enumerate(maps)]
    names = ["m%d" % k for k in range(len(maps))]
    f = fusion(dev, obs, dict(zip(names, maps)), H, W)
    g = kernel_grad(f, pts, names, gd, gks)
    compare(g, obs, pts, H, W, 0.02, maps, gd, gks)


def test_backward_unbatched_map_above_128mib(dev):
    """A fp32 map above kBatchedLoadBytes takes the unbatched backward_map instantiations (fill_map); with 1024 channels
    (256 four-channel vectors, 64 lanes per point) pick_mapping gives it four vectors per lane, backward_map<4, 4>."""
    from d3fields_amd import synth
    V, H, W, N = 4, 96, 128, 3000
    obs = scene(V, H, W)
    m = synth.random_map(V, 96, 96, 1024, seed=31)
    assert m.numel() * m.element_size() > 128 << 20
    pts = synth.random_cloud(N, seed=32)
    gd, gk = normals(33, N), normals(34, N, 1024)
    f = fusion(dev, obs, {"dino_feats": m}, H, W)
    g = kernel_grad(f, pts, ["dino_feats"], gd, [gk])
    compare(g, obs, pts, H, W, 0.02, [m], gd, [gk])


# ---- branch edges, built on purpose ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eval", "eval_dist"])
def test_backward_branch_edges_against_float64(dev, mode):
    obs = edge_scene()
    pts = edge_points()
    N = pts.shape[0]
    maps = edge_maps(4) if mode == "eval" else []
    gks = [normals(44 + k, N, m.shape[3]) for k, m in enumerate(maps)]
    gd = normals(43, N)
    names = ["a", "b"][:len(maps)]
    f = fusion(dev, obs, dict(zip(names, maps)), EH, EW, MU_EDGE)
    g = kernel_grad(f, pts, names, gd, gks, mode)
    g64, dec = compare(g, obs, pts, EH, EW, MU_EDGE, maps, gd, gks, mode)
    v = dec["valid"]
    dist = dec["dist"]
    # every edge is present (eval_dist has no -mu gate, no clamp and no weight)
    assert (~dec["ok"]).any() and (v[2] & (dec["zc"][2] < 0)).any()
    if mode == "eval":
        assert ((dist == -MU_EDGE) & ~v).any() and ((dist == MU_EDGE) & v).any()
        assert ((dist > -MU_EDGE) & (dist < -MU_EDGE + 1e-6) & v).any()
        assert ((dist.abs() > MU_EDGE) & v).any()
        c = dec["cells"][0]
        fx = ((dec["gx"] + 1) / 2) * 16
        assert (((fx > -1) & (fx < 0)) | ((fx > 16) & (fx < 17))).any() and ((fx == c["x0"]) & v).any()
    empty = ~v.any(0)
    part = v.any(0) & ~v.all(0)
    assert empty.any() and part.any()
    assert (g[empty] == 0).all(), "all-invalid points must get exactly 0"


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,where", [("eval", "maps"), ("eval", "depth"), ("eval", "points"), ("eval_dist", "points"),
                                        ("eval_dist", "depth")])
def test_backward_nonfinite_inputs_match_reference(dev, mode, where):
    """The non-finite entries of the gradient are the reference's (autograd through torch: 0 * NaN of invalid views,
    NaN weights, non-finite projections), the finite ones meet the bound."""
    obs = edge_scene()
    pts = edge_points(6000)
    N = pts.shape[0]
    maps = edge_maps(4) if mode == "eval" else []
    maps, obs["depth"] = poison(maps, obs["depth"], where)
    if where == "points":
        for j, val in enumerate([float("nan"), float("inf"), float("-inf")]):
            pts[j::97, j % 3] = val
    gks = [normals(54 + k, N, m.shape[3]) for k, m in enumerate(maps)]
    gd = normals(53, N)
    names = ["a", "b"][:len(maps)]
    f = fusion(dev, obs, dict(zip(names, maps)), EH, EW, MU_EDGE)
    g = kernel_grad(f, pts, names, gd, gks, mode)
    g64, dec = compare(g, obs, pts, EH, EW, MU_EDGE, maps, gd, gks, mode)
    nf = ~torch.isfinite(g64).all(1)
    if mode == "eval_dist" and where == "depth":
        assert not nf.any()         # the depth texel only makes its view invalid: eval_dist passes no NaN from it
        assert (~torch.isfinite(dec["d"]) & (dec["d"] != float("-inf"))).any(), "no lookup reads the poisoned texels"
    else:
        assert nf.any(), "the case reaches no non-finite gradient"
    if where == "maps":
        # the poisoned texels sit in the footprints of valid views, of invalid views and of all-invalid points
        bad = [~torch.isfinite(m).all(-1) for m in maps]
        c = dec["cells"][0]
        V = obs["depth"].shape[0]
        vv = torch.arange(V)[:, None].expand_as(c["x0"])
        hit = torch.zeros_like(dec["valid"])
        for q, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            inb = c["inb"][q]
            xs = torch.where(inb, c["x0"] + dx, torch.zeros_like(c["x0"])).long()
            ys = torch.where(inb, c["y0"] + dy, torch.zeros_like(c["y0"])).long()
            hit |= inb & bad[0][vv, ys, xs]
        empty = ~dec["valid"].any(0)
        assert (hit & dec["valid"]).any() and (hit & ~dec["valid"] & ~empty[None]).any() and (hit & empty[None]).any()


# ---- the tracking step's own gradient -------------------------------------------------------------------------------------
def _track_setup(dev, I, V, C, n=24, seed=61):
    from d3fields_amd import synth
    H, W = 96, 128
    obs = scene(V, H, W)
    m = synth.random_map(V, H // 8, W // 8, C, seed=seed)
    f = fusion(dev, obs, {"dino_feats": m}, H, W)
    last = synth.random_cloud(I * n, seed=seed).reshape(I, n, 3).to(dev).contiguous()
    src = normals(seed + 1, I * n, C).to(dev)
    g = torch.Generator().manual_seed(seed + 2)
    t = (torch.rand(I, 3, generator=g) - 0.5) * 0.02
    starts = [torch.zeros(3), torch.tensor([0.0101, 0.0, 0.0]), torch.tensor([0.6, -0.5, 0.6])]
    w = torch.stack([starts[i % 3] for i in range(I)])
    return f, obs, m, last, src, t.to(dev), w.to(dev)


def _adam_zero(I, dev):
    return torch.zeros(I, 6, device=dev), torch.zeros(I, 6, device=dev), torch.zeros(I, device=dev)


TRACK = dict(mu=0.02, dist_w=100.0, reg_w=1.0, lr=0.01, beta2=0.999, eps=1e-8)


def track_step_grad(f, m, last, src, t, w):
    """adam_m after ONE d3f_track_step with beta1 = 0 and zeroed state: d(loss)/d(t, w) [I,6] and the evaluated keypoints."""
    from d3fields_amd import _lib
    lib = _lib.load()
    dev = last.device
    I, n = last.shape[0], last.shape[1]
    t, w = t.clone(), w.clone()
    am, av, st = _adam_zero(I, dev)
    out_pts = torch.empty(I * n, 3, device=dev)
    loss = torch.zeros(3, device=dev)
    scratch = torch.zeros(lib.d3f_track_step_scratch_bytes(I, n) // 4 + 1, device=dev)
    views, keep, _ = f._views(dev)
    cm = _lib.ChannelMap(m.data_ptr(), m.shape[1], m.shape[2], m.shape[3], _lib.DTYPE_F32, m.stride(0), m.stride(1), m.stride(2))
    state = _lib.TrackState(_lib.ptr(t), _lib.ptr(w), _lib.ptr(am), _lib.ptr(av), _lib.ptr(st), _lib.ptr(out_pts), _lib.ptr(loss),
                            _lib.ptr(scratch))
    _lib.check(lib.d3f_track_step(ctypes.byref(views), ctypes.byref(cm), _lib.ptr(last), I, n, _lib.ptr(src), TRACK["mu"],
                                  TRACK["dist_w"], TRACK["reg_w"], TRACK["lr"], 0.0, TRACK["beta2"], TRACK["eps"], ctypes.byref(state),
                                  _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return am.cpu(), out_pts.cpu()


def five_launch_grad(f, m, last, src, t, w):
    """The same through d3f_rigid_transform -> d3f_eval -> d3f_track_loss_grad -> d3f_eval_backward -> d3f_rigid_update."""
    from d3fields_amd import _lib
    lib = _lib.load()
    dev = last.device
    I, n = last.shape[0], last.shape[1]
    N, C = I * n, m.shape[3]
    t, w = t.clone(), w.clone()
    am, av, st = _adam_zero(I, dev)
    pts = torch.empty(N, 3, device=dev)
    norms = torch.zeros(2, device=dev)
    gf, gdist, loss = torch.empty(N, C, device=dev), torch.empty(N, device=dev), torch.zeros(2, device=dev)
    stream = _lib.current_stream_handle(dev)
    _lib.check(lib.d3f_rigid_transform(_lib.ptr(last), I, n, _lib.ptr(t), _lib.ptr(w), _lib.ptr(pts), _lib.ptr(norms), stream))
    out, saved = f._launch(pts, ["dino_feats"], False, "eval")
    _lib.check(lib.d3f_track_loss_grad(_lib.ptr(out["dino_feats"]), _lib.ptr(src), _lib.ptr(out["dist"]), _lib.ptr(out["valid_mask"]), N, C,
                                       TRACK["dist_w"], _lib.ptr(gf), _lib.ptr(gdist), _lib.ptr(loss), stream))
    gp = f._backward(saved, gdist, [gf])
    _lib.check(lib.d3f_rigid_update(_lib.ptr(last), I, n, _lib.ptr(gp), _lib.ptr(t), _lib.ptr(w), _lib.ptr(am), _lib.ptr(av), _lib.ptr(st),
                                    _lib.ptr(norms), TRACK["reg_w"], TRACK["lr"], 0.0, TRACK["beta2"], TRACK["eps"], stream))
    torch.cuda.synchronize()
    return am.cpu(), pts.cpu()


@pytest.mark.parametrize("I,V,C", [(1, 1, 48), (3, 4, 384), (16, 8, 512), (3, 8, 48), (16, 4, 384)])
def test_track_step_gradient_against_float64(dev, I, V, C):
    """adam_m after one step with beta1 = 0 is the loss gradient w.r.t. (t, w) per instance: the single-launch step, the
    five-launch step and the float64 loss gradient agree.  Start angles w = 0 (clamped), |w|^2 just above 1e-4, |w| ~ 1.
    Tracking with non-finite maps is out of scope (the tracker's maps are finite; the step kernel has no strict form)."""
    f, obs, m, last, src, t, w = _track_setup(dev, I, V, C)
    md = f.curr_obs_torch["dino_feats"]
    g1, p1 = track_step_grad(f, md, last, src, t, w)
    g5, p5 = five_launch_grad(f, md, last, src, t, w)
    ref1, sc1 = R.track_grad(obs, f.H, f.W, m, last, src, t, w, p1, TRACK["mu"], TRACK["dist_w"], TRACK["reg_w"])
    ok, worst, msg = R.check(g1, ref1, sc1)
    assert ok, "d3f_track_step: " + msg
    ref5, sc5 = R.track_grad(obs, f.H, f.W, m, last, src, t, w, p5, TRACK["mu"], TRACK["dist_w"], TRACK["reg_w"])
    ok, worst, msg = R.check(g5, ref5, sc5)
    assert ok, "five launches: " + msg
    ok, worst, msg = R.check(g1, g5.to(torch.float64), torch.maximum(sc1, sc5))
    assert ok, "single vs five launches: " + msg
    assert g1.abs().max() > 0


@pytest.mark.parametrize("I,V,C", [(3, 4, 384), (16, 9, 48)])
def test_tracker_five_launch_gradient_against_float64(dev, I, V, C):
    """RigidTracker's own five-launch step (single_launch=False; V = 9 would force it anyway): its private observation,
    the forward without words and the backward reading the words _check_maps leaves (zero for these finite maps).  One
    step from zeroed Adam state with the tracker's beta1 = 0.9 leaves adam_m = (1 - beta1) * d(loss)/d(t, w)."""
    from d3fields_amd import rigid
    f, obs, m, last, src, t, w = _track_setup(dev, I, V, C)
    tr = rigid.RigidTracker(f, I, last.shape[1], single_launch=False)
    assert tr.fused and not tr.single
    with torch.no_grad():
        for k, x in tr.shadow.curr_obs_torch.items():
            x.copy_(f.curr_obs_torch[k])
        tr.last.copy_(last)
        tr.src.copy_(src)
    tr._check_maps()
    tr._rewind()
    with torch.no_grad():
        tr.t_params.copy_(t)
        tr.log_r.copy_(w)
    tr._fused_iteration()
    torch.cuda.synchronize()
    assert int(tr.words.abs().sum()) == 0, "finite maps must read finite (the backward's fast path)"
    g = tr.state[:I * 6].view(I, 6).cpu().to(torch.float64) / float(1.0 - np.float32(0.9))
    ref, sc = R.track_grad(obs, f.H, f.W, m, last, src, t, w, tr.pts.cpu(), TRACK["mu"], TRACK["dist_w"], TRACK["reg_w"])
    ok, worst, msg = R.check(g, ref, sc)
    assert ok, msg
