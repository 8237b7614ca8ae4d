"""TEST INFRASTRUCTURE ONLY -- the inputs of the fused-feature pins: scenes, points at controlled distances in front of the
surface, maps whose channels span six decades, and which kernel family each case is routed to.  Shared by
tests/test_gpu_field_ref.py (every kernel family against oracle/field_ref.py) and tests/test_field_ref.py (the float32
torch port and the C oracle against the same bound, on the CPU).  Never imported by d3fields_amd.
"""
import torch

from oracle import grad_cases as G


def scaled_map(V, fh, fw, C, seed, cancel=True):
    """[V,fh,fw,C] float32: N(0,1) texels times a per-channel scale 10^U(-4, 2) with a random sign, every fourth channel
    constant in space (per view: the sampling position plays no part there, the bound is at its tightest); with `cancel`,
    every third texel row holds pairs T, -T * (1 + 2^-20) on adjacent texels (x even, x + 1) of every channel."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(V, fh, fw, C, generator=g)
    sc = 10.0 ** (torch.rand(C, generator=g) * 6.0 - 4.0)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    m = m * (sc * sign)
    flat = torch.randn(V, 1, 1, C, generator=g) * (sc * sign)
    m[..., 3::4] = flat[..., 3::4].expand(V, fh, fw, -1)                               # every 4th channel constant in space
    if cancel and fw >= 2:
        e = (fw // 2) * 2
        m[:, ::3, 1:e:2, :] = -m[:, ::3, 0:e:2, :] * (1.0 + 2.0 ** -20)
    return m.contiguous()


def surface_points(obs, H, W, n, mu, seed):
    """[n,3] float32 points placed on pixel rays of random views at distances s in front of the ray-cast surface, so that the
    weight exp(min(mu - s, 0) / mu) runs from 1 through 1e-6 and 1e-30 into float32's subnormal range and to zero."""
    g = torch.Generator().manual_seed(seed)
    depth, K, pose = obs["depth"].double(), obs["K"].double(), obs["pose"].double()
    V = depth.shape[0]
    # s = 0, mu / 2, mu: weight 1; then the weight's exponent (mu - s) / mu = -1, -4, -13.8 (1e-6), -69 (1e-30), -87.5 and
    # -95 (float32 subnormal), -110 (zero in float32)
    s = mu * torch.tensor([0.0, 0.5, 1.0, 2.0, 5.0, 14.8, 70.0, 88.5, 96.0, 111.0], dtype=torch.float64)
    pts = []
    while sum(p.shape[0] for p in pts) < n:
        v = torch.randint(0, V, (4 * n,), generator=g)
        u = torch.rand(4 * n, generator=g) * (W - 1)
        w = torch.rand(4 * n, generator=g) * (H - 1)
        d = depth[v, torch.round(w).long(), torch.round(u).long()]
        dist = s[torch.randint(0, s.numel(), (4 * n,), generator=g)]
        zc = d - dist
        keep = (d > 0) & (zc > 0.05)
        v, u, w, zc = v[keep], u[keep], w[keep], zc[keep]
        Kv, R, t = K[v], pose[v, :, :3], pose[v, :, 3]
        cam = torch.stack(((u - Kv[:, 0, 2]) / Kv[:, 0, 0] * zc, (w - Kv[:, 1, 2]) / Kv[:, 1, 1] * zc, zc), 1)
        pts.append(torch.einsum("nji,nj->ni", R, cam - t))
    return torch.cat(pts)[:n].float().contiguous()


def scene(V, H, W, kind="smooth"):
    return G.scene(V, H, W, kind)


def _mix(obs, H, W, n_cloud, n_surf, mu, seed, scale=1.0):
    from d3fields_amd import synth
    cloud = synth.random_cloud(n_cloud, seed=seed) * scale
    surf = surface_points(obs, H, W, n_surf, mu, seed + 1)
    return torch.cat((cloud, surf)), torch.arange(n_cloud, n_cloud + n_surf)


def _grid():
    from d3fields_amd import create_init_grid, synth
    return create_init_grid(synth.WORK_BOX, 0.0107)[0]                            # 74 x 65 x 20 points, a lattice


# Every case: name -> builder.  A builder returns dict(obs, H, W, mu, maps {name: [V,fh,fw,C] cpu tensor}, names (queried
# maps, wide first), pts [N,3] cpu, edge (rows always compared), and how the GPU test calls it: call ("eval" /
# "batch_eval"), flags (tuning-flag names of d3fields_amd._lib), reorder (Fusion.reorder_points), reference_rounding,
# expect (prefix of last_plan()["kernel"]; for a gated cloud the side that ran), rows (sample size on big batches)).
def _direct(V=4, C=384, cs=(), f16=False, mu=0.005, n=3000, seed=1, **kw):
    H, W = 96, 128
    obs = scene(V, H, W)
    maps = {"wide": scaled_map(V, 12, 16, C, seed)}
    for j, c in enumerate(cs):
        maps["m%d" % j] = scaled_map(V, 12, 16, c, seed + 1 + j)
    if f16:
        maps = {k: (m / m.abs().amax((0, 1, 2)).clamp_min(1e-30) * 100.0).half() for k, m in maps.items()}
    pts, edge = _mix(obs, H, W, n // 2, n - n // 2, mu, seed + 10)
    d = dict(obs=obs, H=H, W=W, mu=mu, maps=maps, names=list(maps), pts=pts, edge=edge, call="eval", flags=(), reorder=True,
             reference_rounding=False, expect="fused_eval_f16_kernel<0>" if f16 else "fused_eval_kernel<0>", rows=None)
    d.update(kw)
    return d


def _edges(mu=G.MU_EDGE):
    """grad_cases' edge scene: dyadic cameras, points on texel lines / centres and on the border, a 9 x 17 patch map, a
    full-resolution one, 1 x W and H x 1 maps."""
    obs = G.edge_scene()
    pts = G.edge_points(3000)
    maps = {"patch": scaled_map(4, 9, 17, 96, 61), "full": scaled_map(4, G.EH, G.EW, 72, 62),
            "row": scaled_map(4, 1, 16, 80, 63, cancel=False), "col": scaled_map(4, 12, 1, 80, 64, cancel=False)}
    return dict(obs=obs, H=G.EH, W=G.EW, mu=mu, maps=maps, names=list(maps), pts=pts, edge=torch.arange(270), call="eval",
                flags=(), reorder=True, reference_rounding=False, expect="fused_eval_kernel<0>", rows=None)


def _slice_view():
    """a channel-range view: channels 1..384 of a 392-channel tensor (4-byte offset, texel stride 392)"""
    d = _direct(C=392, seed=5)
    d["maps"] = {"wide": d["maps"]["wide"][..., 1:385]}
    return d


def _wide():
    V, H, W = 4, 96, 128
    obs = scene(V, H, W)
    maps = {"dense": scaled_map(V, H, W, 1024, 7)}
    pts, edge = _mix(obs, H, W, 2000, 2000, 0.005, 70)
    return dict(obs=obs, H=H, W=W, mu=0.005, maps=maps, names=["dense"], pts=pts, edge=edge, call="eval", flags=(), reorder=True,
                reference_rounding=False, expect="fused_eval_wide_kernel<0>", rows=None)


def _big(V, H, W, fhw, C, points, mu, expect, seed, n=0, flags=(), call="batch_eval", rows=20000, f16=False, kind="smooth"):
    obs = scene(V, H, W, kind)
    m = scaled_map(V, fhw[0], fhw[1], C, seed)
    if f16:
        m = (m / m.abs().amax((0, 1, 2)).clamp_min(1e-30) * 100.0).half()
    if points == "grid":
        pts, edge = _grid(), torch.zeros(0, dtype=torch.long)
    else:
        from d3fields_amd import synth
        pts = synth.random_cloud(n, seed=seed + 1) * (0.6 if points == "dense cloud" else 1.0)
        if points == "sorted cloud":
            pts = pts[torch.argsort(pts[:, 0])].contiguous()
        surf = surface_points(obs, H, W, 3000, mu, seed + 2)
        pts = torch.cat((pts[:n - 3000], surf))                 # the controlled-distance rows at the end
        edge = torch.arange(n - 3000, n)
    return dict(obs=obs, H=H, W=W, mu=mu, maps={"feats": m}, names=["feats"], pts=pts.contiguous(), edge=edge, call=call,
                flags=tuple(flags), reorder=True, reference_rounding=False, expect=expect, rows=rows)


CASES = {
    # the direct kernels (small batches: every row compared)
    "direct V4 C384": lambda: _direct(),
    "direct V1 C1000": lambda: _direct(V=1, C=1000, seed=2),
    "direct V9 C65 + C64": lambda: _direct(V=9, C=65, cs=(64,), seed=3, mu=0.02),
    "direct V2 C384 C1024": lambda: _direct(V=2, C=384, cs=(1024,), seed=4, n=2000),
    "direct channel-range view": _slice_view,
    "direct f16 C129 + C128": lambda: _direct(C=129, cs=(128,), f16=True, seed=6),
    "direct edges": _edges,
    "wide dense C1024": _wide,
    "strict: reference rounding": lambda: _direct(V=5, seed=8, reference_rounding=True),
    "batch_eval, reorder off": lambda: _direct(V=3, C=256, seed=9, n=4000, call="batch_eval", reorder=False),
    # the big-batch families (a seeded sample of rows plus the controlled-distance rows)
    "window lattice": lambda: _big(4, 480, 640, (48, 64), 384, "grid", 0.005, "fused_eval_window_kernel", 21),
    "window cloud, window side": lambda: _big(4, 480, 640, (48, 64), 384, "dense cloud", 0.005, "fused_eval_window_kernel", 22,
                                              n=300001, flags=("TUNE_WINDOW_SIDE",)),
    "window cloud, cell-run side": lambda: _big(4, 480, 640, (48, 64), 384, "dense cloud", 0.005, "fused_eval_runs_kernel", 23,
                                                n=300001, flags=("TUNE_NO_WINDOW_GATE",)),
    "cell runs V8 C512": lambda: _big(8, 480, 640, (24, 32), 512, "cloud", 0.02, "fused_eval_runs_kernel", 24, n=150001),
    "sliced lattice": lambda: _big(4, 192, 256, (192, 256), 384, "grid", 0.005, "fused_eval_sliced_kernel", 25),
    "sliced cloud, eval, reorder off": lambda: dict(_big(4, 96, 128, (96, 128), 384, "cloud", 0.005, "fused_eval_kernel<0>", 26,
                                                         n=70001, call="eval"), reorder=False),
    "sliced cloud": lambda: _big(4, 96, 128, (96, 128), 384, "cloud", 0.005, "fused_eval_sliced_kernel", 26, n=70001),
    "sliced lattice f16": lambda: _big(4, 192, 256, (192, 256), 384, "grid", 0.005, "fused_eval_sliced_kernel", 27, f16=True),
    "window lattice f16": lambda: _big(3, 480, 640, (24, 32), 256, "grid", 0.005, "fused_eval_window_kernel", 28, f16=True),
    "rows V8 lattice": lambda: _big(8, 480, 640, (36, 64), 1024, "grid", 0.005, "fused_eval_rows_kernel", 31, rows=5000),
    "rows V8 cloud": lambda: _big(8, 480, 640, (36, 64), 1024, "cloud", 0.02, "fused_eval_rows_kernel", 32, n=150001, rows=5000),
    "rows V4 sorted cloud": lambda: _big(4, 480, 640, (24, 32), 1024, "sorted cloud", 0.005, "fused_eval_rows_kernel", 33, n=100000),
    "rows V5 lattice": lambda: _big(5, 480, 640, (24, 32), 1024, "grid", 0.005, "fused_eval_rows_kernel", 34, rows=10000),
    "rows V1 sorted cloud eval": lambda: _big(1, 480, 640, (48, 64), 1024, "sorted cloud", 0.005, "fused_eval_rows_kernel", 35,
                                             n=66000, call="eval"),
}

# what every query with a wide map can be routed to (fusion.py: Fusion._record_plan)
FAMILIES = ("fused_eval_kernel<0>", "fused_eval_wide_kernel<0>", "fused_eval_f16_kernel<0>", "fused_eval_window_kernel",
            "fused_eval_runs_kernel", "fused_eval_sliced_kernel", "fused_eval_rows_kernel")


def sample_rows(case, n=None):
    """The rows compared: every row of a small batch; on a big one a seeded sample of case['rows'] (or n) plus the edge rows."""
    N = case["pts"].shape[0]
    k = n if n is not None else case["rows"]
    if k is None or k >= N:
        return torch.arange(N)
    pick = torch.randperm(N, generator=torch.Generator().manual_seed(N))[:k]
    return torch.unique(torch.cat((pick, case["edge"])))


def poison(case, points=True):
    """Non-finite inputs for the strict path: a NaN and an Inf texel in the first map and (points) NaN / Inf query points."""
    m = case["maps"][case["names"][0]].clone()
    m[0, 1, 1, 0] = float("nan")
    m[-1, m.shape[1] // 2, m.shape[2] // 2, m.shape[3] - 1] = float("inf")
    case["maps"][case["names"][0]] = m
    if not points:
        return case
    p = case["pts"].clone()
    for j, val in enumerate([float("nan"), float("inf"), float("-inf")]):
        p[j::101, j % 3] = val
    case["pts"] = p
    return case
