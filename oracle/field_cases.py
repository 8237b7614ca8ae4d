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


def onehot_map(V, fh, fw, NI, seed, block=16):
    """[V,fh,fw,NI] float32 one-hot instance mask, constant over block x block texels: an instance covers a region, so away
    from the region borders the four corners of a sample agree (the fused value is then the normalised weight sum or 0);
    half the regions belong to instance 0, so that the views of a point often agree as well."""
    g = torch.Generator().manual_seed(seed)
    shape = (V, (fh + block - 1) // block, (fw + block - 1) // block)
    idx = torch.randint(0, NI, shape, generator=g)
    idx = torch.where(torch.rand(shape, generator=g) < 0.5, torch.zeros_like(idx), idx)      # instance 0 is large: views often agree
    idx = idx.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :fh, :fw]
    return torch.nn.functional.one_hot(idx, NI).float().contiguous()


def companions(V, H, W, thin, seed):
    """The thin maps that ride along with a wide one, at full resolution (what the product queries: features + mask):
    'mask' = 8-channel one-hot, 'color' = 3 channels of scaled_map."""
    made = {"mask": lambda: onehot_map(V, H, W, 8, seed + 50), "color": lambda: scaled_map(V, H, W, 3, seed + 51)}
    return {k: made[k]() for k in thin}


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
    return create_init_grid(synth.WORK_BOX, 0.0107)[0]                            # 75 x 66 x 21 points, a lattice


# Every case: name -> builder.  A builder returns dict(obs, H, W, mu, maps {name: [V,fh,fw,C] cpu tensor}, names (queried
# maps, wide first), pts [N,3] cpu, edge (rows always compared), and how the GPU test calls it: call ("eval" /
# "batch_eval"), flags (tuning-flag names of d3fields_amd._lib), reorder (Fusion.reorder_points), reference_rounding,
# expect (prefix of last_plan()["kernel"]; for a gated cloud the side that ran), rows (sample size on big batches)).
# The thin cases (THIN_CASES) add: thin_form ("parallel": every thin map of the case meets thin_map()'s condition of
# csrc/fuse_common.h and is gathered with the views across lanes; "outside": none does), base (the earlier case it was derived
# from: its share of rows left out / non-finite bounds the new case's).
def _direct(V=4, C=384, cs=(), f16=False, mu=0.005, n=3000, seed=1, thin=(), **kw):
    H, W = 96, 128
    obs = scene(V, H, W)
    maps = {"wide": scaled_map(V, 12, 16, C, seed)}
    for j, c in enumerate(cs):
        maps["m%d" % j] = scaled_map(V, 12, 16, c, seed + 1 + j)
    if f16:
        maps = {k: (m / m.abs().amax((0, 1, 2)).clamp_min(1e-30) * 100.0).half() for k, m in maps.items()}
    maps.update(companions(V, H, W, thin, seed))
    pts, edge = _mix(obs, H, W, n // 2, n - n // 2, mu, seed + 10)
    d = dict(obs=obs, H=H, W=W, mu=mu, maps=maps, names=list(maps), pts=pts, edge=edge, call="eval", flags=(), reorder=True,
             reference_rounding=False, expect="fused_eval_f16_kernel<0>" if f16 else "fused_eval_kernel<0>", rows=None)
    d.update(kw)
    return d


def _edges(mu=G.MU_EDGE, thin=False):
    """grad_cases' edge scene: dyadic cameras, points on texel lines / centres and on the border, a 9 x 17 patch map, a
    full-resolution one, 1 x W and H x 1 maps (thin: the same four shapes with 3, 8, 2 and 1 channels)."""
    obs = G.edge_scene()
    pts = G.edge_points(3000)
    C = (3, 8, 2, 1) if thin else (96, 72, 80, 80)
    maps = {"patch": scaled_map(4, 9, 17, C[0], 61), "full": scaled_map(4, G.EH, G.EW, C[1], 62),
            "row": scaled_map(4, 1, 16, C[2], 63, cancel=False), "col": scaled_map(4, 12, 1, C[3], 64, cancel=False)}
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


def _thin(V, C, n, seed, call="eval", f16=False, onehot=False, view=None, mu=0.005, **kw):
    """A thin map (<= 256 bytes per texel) queried alone: full resolution, points on the surface and far off it.  view =
    (first channel, channels of the tensor): the map is that channel range of a wider tensor (texel stride > C; a first
    channel that is no multiple of 4 leaves the pointer off the 16-byte boundary: scalar lanes)."""
    H, W = 96, 128
    obs = scene(V, H, W)
    lo, total = view if view else (0, C)
    m = onehot_map(V, H, W, total, seed, block=8) if onehot else scaled_map(V, H, W, total, seed)
    if f16:
        m = (m / m.abs().amax((0, 1, 2)).clamp_min(1e-30) * 100.0).half()
    m = m[..., lo:lo + C]
    pts, edge = _mix(obs, H, W, n // 2, n - n // 2, mu, seed + 10)
    d = dict(obs=obs, H=H, W=W, mu=mu, maps={"thin": m}, names=["thin"], pts=pts, edge=edge, call=call, flags=(), reorder=True,
             reference_rounding=False, expect="fused_eval_f16_kernel<0>" if f16 else "fused_eval_kernel<0>", rows=None,
             base="direct V4 C384")
    d.update(kw)
    return d


def _big(V, H, W, fhw, C, points, mu, expect, seed, n=0, flags=(), call="batch_eval", rows=20000, f16=False, kind="smooth", thin=()):
    obs = scene(V, H, W, kind)
    m = scaled_map(V, fhw[0], fhw[1], C, seed)
    if f16:
        m = (m / m.abs().amax((0, 1, 2)).clamp_min(1e-30) * 100.0).half()
    maps = {"feats": m}
    maps.update(companions(V, H, W, thin, seed))
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
    return dict(obs=obs, H=H, W=W, mu=mu, maps=maps, names=list(maps), pts=pts.contiguous(), edge=edge, call=call,
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
    "window lattice": lambda thin=(): _big(4, 480, 640, (48, 64), 384, "grid", 0.005, "fused_eval_window_kernel", 21, thin=thin),
    "window cloud, window side": lambda thin=(): _big(4, 480, 640, (48, 64), 384, "dense cloud", 0.005, "fused_eval_window_kernel", 22,
                                              n=300001, flags=("TUNE_WINDOW_SIDE",), thin=thin),
    "window cloud, cell-run side": lambda thin=(): _big(4, 480, 640, (48, 64), 384, "dense cloud", 0.005, "fused_eval_runs_kernel", 23,
                                                n=300001, flags=("TUNE_NO_WINDOW_GATE",), thin=thin),
    "cell runs V8 C512": lambda thin=(): _big(8, 480, 640, (24, 32), 512, "cloud", 0.02, "fused_eval_runs_kernel", 24, n=150001, thin=thin),
    "sliced lattice": lambda thin=(): _big(4, 192, 256, (192, 256), 384, "grid", 0.005, "fused_eval_sliced_kernel", 25, thin=thin),
    "sliced cloud, eval, reorder off": lambda: dict(_big(4, 96, 128, (96, 128), 384, "cloud", 0.005, "fused_eval_kernel<0>", 26,
                                                         n=70001, call="eval"), reorder=False),
    "sliced cloud": lambda thin=(): _big(4, 96, 128, (96, 128), 384, "cloud", 0.005, "fused_eval_sliced_kernel", 26, n=70001, thin=thin),
    "sliced lattice f16": lambda: _big(4, 192, 256, (192, 256), 384, "grid", 0.005, "fused_eval_sliced_kernel", 27, f16=True),
    "window lattice f16": lambda: _big(3, 480, 640, (24, 32), 256, "grid", 0.005, "fused_eval_window_kernel", 28, f16=True),
    "rows V8 lattice": lambda thin=(): _big(8, 480, 640, (36, 64), 1024, "grid", 0.005, "fused_eval_rows_kernel", 31, rows=5000, thin=thin),
    "rows V8 cloud": lambda thin=(): _big(8, 480, 640, (36, 64), 1024, "cloud", 0.02, "fused_eval_rows_kernel", 32, n=150001, rows=5000, thin=thin),
    "rows V4 sorted cloud": lambda: _big(4, 480, 640, (24, 32), 1024, "sorted cloud", 0.005, "fused_eval_rows_kernel", 33, n=100000),
    "rows V5 lattice": lambda: _big(5, 480, 640, (24, 32), 1024, "grid", 0.005, "fused_eval_rows_kernel", 34, rows=10000),
    "rows V1 sorted cloud eval": lambda: _big(1, 480, 640, (48, 64), 1024, "sorted cloud", 0.005, "fused_eval_rows_kernel", 35,
                                             n=66000, call="eval"),
}


def _beside(base, thin):
    """The earlier case `base` with thin companions beside its wide map (same points, same sample of rows, same kernel)."""
    return lambda: dict(CASES[base](thin=thin), thin_form="parallel", base=base)


# The thin family (<= 256 bytes per texel: the instance mask, colours, fp16 maps of up to 128 channels), which keeps the
# reference's operation order in every kernel.  Also part of CASES.
THIN_CASES = {
    # thin alone, the views in parallel across lanes (gather_map_thin): vector widths 4 / 2 / 1, 1 / 2 / 4 lanes per point, 2..8
    # views (3 and 5 leave view lanes idle), N no multiple of the points per workgroup, N = 1 and 17
    "thin V2 C3": lambda: _thin(2, 3, 3001, 101, thin_form="parallel"),
    # (five scalar vectors get 8 lanes per point from the planner -- one pass --, so this one is view-sequential; V3 C6 is the
    #  nearest shape that keeps three views in the parallel form)
    "thin V3 C5": lambda: _thin(3, 5, 3003, 102, call="batch_eval", thin_form="outside"),
    "thin V3 C6": lambda: _thin(3, 6, 3003, 112, call="batch_eval", thin_form="parallel"),
    "thin V4 C8": lambda: _thin(4, 8, 3999, 103, thin_form="parallel"),
    "thin V4 C8 one-hot, batch_eval": lambda: _thin(4, 8, 3001, 113, call="batch_eval", onehot=True, thin_form="parallel"),
    "thin V5 C1": lambda: _thin(5, 1, 3005, 104, call="batch_eval", thin_form="parallel"),
    "thin V8 C16": lambda: _thin(8, 16, 3007, 105, mu=0.02, thin_form="parallel"),
    "thin V4 C12": lambda: _thin(4, 12, 17, 106, call="batch_eval", thin_form="parallel"),
    "thin V8 C2": lambda: _thin(8, 2, 1, 107, mu=0.02, thin_form="parallel"),
    "thin V8 C2, batch_eval": lambda: _thin(8, 2, 3011, 117, call="batch_eval", mu=0.02, thin_form="parallel"),
    "thin V4 C8 in a 16-channel tensor": lambda: _thin(4, 8, 3001, 108, view=(4, 16), thin_form="parallel"),
    "thin edges": lambda: dict(_edges(thin=True), thin_form="parallel", base="direct edges"),
    # thin alone, outside that form: the view-sequential gather_map
    "thin V1 C8": lambda: _thin(1, 8, 3001, 121, thin_form="outside"),
    "thin V9 C8": lambda: _thin(9, 8, 3001, 122, mu=0.02, call="batch_eval", thin_form="outside"),
    "thin V4 C17": lambda: _thin(4, 17, 3001, 123, thin_form="outside"),
    "thin V4 C33": lambda: _thin(4, 33, 3001, 124, call="batch_eval", thin_form="outside"),
    "thin V4 C64": lambda: _thin(4, 64, 3001, 125, thin_form="outside"),
    "thin f16 V4 C8": lambda: _thin(4, 8, 3001, 126, f16=True, thin_form="outside", base="direct f16 C129 + C128"),
    "thin f16 V4 C24": lambda: _thin(4, 24, 3001, 127, f16=True, call="batch_eval", thin_form="outside", base="direct f16 C129 + C128"),
    "thin f16 V4 C127": lambda: _thin(4, 127, 3001, 128, f16=True, thin_form="outside", base="direct f16 C129 + C128"),
    "thin f16 V4 C128": lambda: _thin(4, 128, 3001, 129, f16=True, thin_form="outside", base="direct f16 C129 + C128"),
    "thin channel-range view C20 of 32": lambda: _thin(4, 20, 3001, 130, view=(4, 32), thin_form="outside", base="direct channel-range view"),
    "thin C8 off by 4 bytes": lambda: _thin(4, 8, 3001, 131, view=(1, 12), thin_form="outside", base="direct channel-range view"),
    # reference_rounding: thin_max_views is 0, every point strict
    "strict: reference rounding, thin alone": lambda: _thin(4, 8, 3001, 132, reference_rounding=True, thin_form="outside",
                                                            base="strict: reference rounding"),
    "strict: reference rounding + mask + color": lambda: dict(_direct(V=5, seed=8, reference_rounding=True, thin=("mask", "color")),
                                                              thin_form="outside", base="strict: reference rounding"),
    # thin beside wide: once per big-batch family, an 8-channel one-hot mask (and once a 3-channel colour map)
    "window lattice + mask + color": _beside("window lattice", ("mask", "color")),
    "window cloud, window side + mask": _beside("window cloud, window side", ("mask",)),
    "window cloud, cell-run side + mask": _beside("window cloud, cell-run side", ("mask",)),
    "cell runs V8 C512 + mask": _beside("cell runs V8 C512", ("mask",)),
    "sliced lattice + mask": _beside("sliced lattice", ("mask",)),
    "sliced cloud + mask": _beside("sliced cloud", ("mask",)),
    "rows V8 lattice + mask": _beside("rows V8 lattice", ("mask",)),
    "rows V8 cloud + mask": _beside("rows V8 cloud", ("mask",)),
}
CASES.update(THIN_CASES)
# the big-batch cases a thin map rides along in (each must be seen with a companion): lattice and cloud of every family
BESIDE_BASES = ("window lattice", "window cloud, window side", "window cloud, cell-run side", "cell runs V8 C512", "sliced lattice",
                "sliced cloud", "rows V8 lattice", "rows V8 cloud")


def ordered_names():
    """The cases, each one with thin companions right behind the case it was derived from (the two share the wide map's
    float64 reference: field_ref.field64_shared)."""
    beside = {}
    for k in CASES:
        if k in THIN_CASES and " + " in k:
            beside.setdefault(k.split(" + ")[0], []).append(k)
    rest = [k for k in CASES if not any(k in v for v in beside.values())]
    return [n for k in rest for n in [k] + beside.get(k, [])]


def thin_names(case):
    """The queried maps of the thin family (<= 256 bytes per texel)."""
    return [k for k in case["names"] if case["maps"][k].shape[3] * case["maps"][k].element_size() <= 256]


def views_in_parallel(case, k, plan):
    """thin_map() of csrc/fuse_common.h for the queried map k, recomputed from the lane mapping the plan recorded
    (Fusion.last_lane_mapping()): one vector per lane, at most 4 lanes per point that hold every vector of a texel, 2..8 views (none
    under reference_rounding: thin_max_views is 0 there); fp16 maps never take that form (fuse_body.h: gather_map_half_u)."""
    i, m = case["names"].index(k), case["maps"][k]
    vw, lanes, per_lane = plan["vector_floats"][i], plan["lanes_per_point"][i], plan["vectors_per_lane"][i]
    max_views = 0 if case["reference_rounding"] or "TUNE_DIRECT_GATHER" in case["flags"] else 8
    return bool(m.dtype == torch.float32 and per_lane == 1 and lanes <= 4 and m.shape[3] // vw <= lanes and 2 <= m.shape[0] <= max_views)


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


def poison(case, points=True, name=None):
    """Non-finite inputs for the strict path: a NaN and an Inf texel in the first map -- or NaN and Inf texels spread over
    the (thin, full-resolution) map `name` -- and (points) NaN / Inf query points."""
    thin = name is not None
    name = case["names"][0] if name is None else name
    m = case["maps"][name].clone()
    m[0, 1, 1, 0] = float("nan")
    m[-1, m.shape[1] // 2, m.shape[2] // 2, m.shape[3] - 1] = float("inf")
    if thin:
        # a full-resolution map: one texel is a pixel, which few points see -- one in every 8 x 8 texels
        m[0, 1::8, 1::8, 0] = float("nan")
        m[-1, 5::8, 5::8, m.shape[3] - 1] = float("inf")
    case["maps"][name] = m
    if not points:
        return case
    p = case["pts"].clone()
    for j, val in enumerate([float("nan"), float("inf"), float("-inf")]):
        p[j::101, j % 3] = val
    case["pts"] = p
    return case
