"""The float64 gradient reference (oracle/grad_ref.py) pinned on the CPU: against the reference's own autograd gradient
(golden grad_500), the float32 torch port's autograd (values and non-finite sets), central finite differences, and the
calibration of grad_ref.TOL on the float32 port over the cases of tests/test_gpu_grad.py (oracle/grad_cases.py)."""
import torch

from conftest import load_golden
from oracle import grad_ref as R
from oracle import torch_port

from oracle import grad_cases as G


def port_grad(obs, pts, H, W, mu, maps, gd, gks, mode="eval"):
    p = pts.clone().requires_grad_(True)
    if mode == "eval_dist":
        (torch_port.dist_query(obs, p, H, W)["dist"] * gd).sum().backward()
        return p.grad
    o = dict(obs)
    names = []
    for k, m in enumerate(maps):
        o["m%d" % k] = m.float()
        names.append("m%d" % k)
    out = torch_port.field_query(o, p, names, H, W, mu)
    loss = (out["dist"] * gd).sum()
    for k, g in enumerate(gks):
        if g is not None:
            loss = loss + (out["m%d" % k] * g).sum()
    loss.backward()
    return p.grad


def test_matches_reference_golden_grad_500():
    """Per point, within the float32 rounding of the golden (the reference's autograd, upstream gradients all 1)."""
    g = load_golden("grad_500")
    obs = {k: torch.from_numpy(g[k]) for k in ("depth", "K", "pose")}
    m, pts = torch.from_numpy(g["in_dino_feats"]), torch.from_numpy(g["pts"])
    N = pts.shape[0]
    g64, sc, dec = R.field_grad(obs, pts, int(g["H"]), int(g["W"]), float(g["mu"]), [m], torch.ones(N), [torch.ones(N, 4)])
    ok, worst, msg = R.check(torch.from_numpy(g["grad_pts"]), g64, sc)
    assert ok, msg
    assert dec["valid"].any() and (~dec["valid"]).any()


def _cases():
    """(name, obs, pts, H, W, mu, maps, gd, gks, mode) of every case of tests/test_gpu_grad.py that the port can run on the
    CPU; large batches on a seeded sample of their rows (a point's gradient depends on its own row only)."""
    from d3fields_amd import synth
    for mode, V, N, C, _ in G.TILE_CASES:
        H, W = 48, 64
        obs = G.scene(V, H, W, "stress" if V in (4, 30) else "smooth")
        pts = synth.random_cloud(N, seed=V + N)
        gd = G.normals(1, N)
        maps, gks = [], []
        if mode == "eval":
            maps, gks = [synth.random_map(V, 12, 16, C, seed=2)], [G.normals(3, N, C)]
        if N > 3000:
            rows = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:3000]
            pts, gd, gks = pts[rows], gd[rows], [g[rows] for g in gks]
        yield "tiles-%s-%d-%d-%d" % (mode, V, N, C), obs, pts, H, W, 0.02, maps, gd, gks, mode
    for kind in ("fp16_vec8", "fp16_scalar", "slice_unaligned", "row_1xW", "col_Hx1", "full_res", "three_maps"):
        V, H, W, N = 4, 48, 64, 3000
        maps = G.layout_maps(kind, V, H, W)
        gks = [None if (kind == "three_maps" and k == 1) else G.normals(23 + k, N, m.shape[3]) for k, m in enumerate(maps)]
        yield kind, G.scene(V, H, W), synth.random_cloud(N, seed=21), H, W, 0.02, maps, G.normals(22, N), gks, "eval"
    for mode in ("eval", "eval_dist"):
        pts = G.edge_points()
        N = pts.shape[0]
        maps = G.edge_maps(4) if mode == "eval" else []
        gks = [G.normals(44 + k, N, m.shape[3]) for k, m in enumerate(maps)]
        yield "edges-" + mode, G.edge_scene(), pts, G.EH, G.EW, G.MU_EDGE, maps, G.normals(43, N), gks, mode


def test_float32_port_within_bound_and_tol_calibrated():
    """The float32 port meets |g - g64| <= TOL * scale on every case; TOL is a few times the port's worst ratio (the
    constant PORT_WORST records the measured value)."""
    worst = 0.0
    for name, obs, pts, H, W, mu, maps, gd, gks, mode in _cases():
        g64, sc, _ = R.field_grad(obs, pts, H, W, mu, maps, gd, gks, mode=mode)
        ok, w, msg = R.check(port_grad(obs, pts, H, W, mu, maps, gd, gks, mode), g64, sc)
        assert ok, "%s: %s" % (name, msg)
        worst = max(worst, w)
    assert worst <= R.PORT_WORST * 1.5, "port worst ratio %.3g: re-measure PORT_WORST" % worst
    assert 2.0 * worst <= R.TOL <= 10.0 * max(worst, R.PORT_WORST), "TOL %.3g vs port worst %.3g" % (R.TOL, worst)


def test_nonfinite_sets_match_port():
    """NaN / Inf texels, depth and query points: the non-finite entries of the float64 reference are those of autograd
    through the float32 port (grid_sample's backward and all); the finite ones meet the bound."""
    for mode, where in (("eval", "maps"), ("eval", "depth"), ("eval", "points"), ("eval_dist", "points"), ("eval_dist", "depth")):
        obs = G.edge_scene()
        pts = G.edge_points(1500)
        N = pts.shape[0]
        maps = G.edge_maps(4) if mode == "eval" else []
        maps, obs["depth"] = G.poison(maps, obs["depth"], where)
        if where == "points":
            for j, val in enumerate([float("nan"), float("inf"), float("-inf")]):
                pts[j::97, j % 3] = val
        gks = [G.normals(54 + k, N, m.shape[3]) for k, m in enumerate(maps)]
        gd = G.normals(53, N)
        g64, sc, _ = R.field_grad(obs, pts, G.EH, G.EW, G.MU_EDGE, maps, gd, gks, mode=mode)
        ok, w, msg = R.check(port_grad(obs, pts, G.EH, G.EW, G.MU_EDGE, maps, gd, gks, mode), g64, sc)
        assert ok, "%s/%s: %s" % (mode, where, msg)


def test_matches_central_differences():
    """d/dp of the float64 loss by central differences (h = 1e-6, the float32 choices held fixed), on the points whose
    float32 choices stay the same within 1e-4 (world units) along the difference: there the piece the derivative is
    taken on is the function itself."""
    from d3fields_amd import synth
    V, H, W, N, C = 3, 48, 64, 400, 5
    obs = G.scene(V, H, W)
    m = synth.random_map(V, 12, 16, C, seed=71).double()
    pts = synth.random_cloud(N, seed=72)
    gd, gk = G.normals(73, N).double(), G.normals(74, N, C).double()
    for mode in ("eval", "eval_dist"):
        maps, gks = ([m], [gk]) if mode == "eval" else ([], [])
        g64, sc, dec = R.field_grad(obs, pts, H, W, 0.02, maps, gd, gks, mode=mode)
        h = 1e-6
        checked = 0
        for j in range(3):
            e = torch.zeros(3)
            e[j] = h
            lp, ln = (R.field_loss64(obs, pts.double() + s * e, H, W, 0.02, maps, gd, gks, mode, dec) for s in (1, -1))
            same = R.same_choices(obs, pts.double() + e, pts.double() - e, H, W, 0.02, maps, mode)
            fd = (lp - ln) / (2 * h)
            keep = same & torch.isfinite(g64[:, j])
            err = (fd - g64[:, j]).abs()[keep]
            assert (err <= 1e-5 * (1 + g64[:, j].abs()[keep])).all(), "coordinate %d: FD err %.3g" % (j, float(err.max()))
            checked += int(keep.sum())
        assert checked >= N, "too few points away from the boundaries"
