"""TEST INFRASTRUCTURE ONLY -- the inputs of the gradient tests: scenes, points, maps, upstream gradients and the tile size
the backward launch picks.  Shared by tests/test_gpu_grad.py (the HIP kernels) and tests/test_grad_ref.py (the float64
reference and its calibration on the float32 torch port, on the CPU).  Never imported by d3fields_amd.
"""
import numpy as np
import torch


def backward_tile(V, n):
    """Points per workgroup of d3f_eval_backward / d3f_eval_dist_backward (d3f_api.hip: backward_common): 128, halved
    while a tile's LDS (44 B per point and view) exceeds 60 KiB (not below 16), then while fewer than 1024 tiles (not
    below 8)."""
    t = 128
    while t > 16 and t * V * 44 > 60 * 1024:
        t >>= 1
    while t > 8 and n // t < 1024:
        t >>= 1
    return t


# (mode, V, N, C, tile): every tile of the backward -- 8 (small N), 16 / 32 / 64 (LDS-limited at V = 64 / 30 / 11, N large
# enough to keep them), 128 with a ragged last tile, ~2^21 points.  The tests assert backward_tile(V, N) == tile.
TILE_CASES = [
    ("eval", 1, 1, 3, 8),
    ("eval", 4, 257, 2, 8),
    ("eval", 11, 3000, 384, 8),
    ("eval", 64, 16384 + 5, 10, 16),
    ("eval", 30, 32768 + 7, 7, 32),
    ("eval", 11, 65536 + 9, 384, 64),
    ("eval", 4, 131072 + 37, 1024, 128),
    ("eval", 1, (1 << 21) + 3, 1, 128),
    ("eval_dist", 1, (1 << 21) + 3, 0, 128),
    ("eval_dist", 64, 257, 0, 8),
    ("eval_dist", 64, 16384 + 5, 0, 16),
    ("eval_dist", 30, 32768 + 7, 0, 32),
    ("eval_dist", 11, 131072 + 37, 0, 64),
    ("eval_dist", 4, 3000, 0, 8),
]


def scene(V, H, W, kind="smooth"):
    from d3fields_amd import synth
    sc = synth.make_scene(V, H, W, kind)
    return {"depth": sc["depth"], "K": sc["K"], "pose": sc["pose"]}

def normals(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

def layout_maps(kind, V, H, W):
    from d3fields_amd import synth
    g = torch.Generator().manual_seed(11)
    if kind == "fp16_vec8":
        return [synth.random_map(V, 12, 16, 48, seed=4).half()]
    if kind == "fp16_scalar":
        return [synth.random_map(V, 12, 16, 7, seed=4).half()]
    if kind == "slice_unaligned":           # channels 3..9 of a 16-channel tensor: odd base, vw = 1
        return [torch.randn(V, 12, 16, 16, generator=g)[..., 3:10]]
    if kind == "slice_aligned":             # channels 4..11: 16-B base, stride 16, vw = 4
        return [torch.randn(V, 12, 16, 16, generator=g)[..., 4:12]]
    if kind == "row_1xW":
        return [torch.randn(V, 1, 16, 10, generator=g)]
    if kind == "col_Hx1":
        return [torch.randn(V, 12, 1, 10, generator=g)]
    if kind == "full_res":
        return [torch.rand(V, H, W, 3, generator=g)]
    if kind == "three_maps":                # mask-like (1 ch), fp16 vec8, fp32 wide
        return [torch.rand(V, H, W, 1, generator=g), synth.random_map(V, 12, 16, 48, seed=6).half(),
                synth.random_map(V, 6, 8, 384, seed=7)]
    raise KeyError(kind)

# ---- branch edges, built on purpose ---------------------------------------------------------------------------------------
MU_EDGE = 2.0 ** -6           # dyadic: dist = d - zc lands exactly on +-mu
EH, EW = 33, 65               # W - 1 = 64, H - 1 = 32: integer pixels map to exact grid coordinates
D0 = 0.5


def edge_scene():
    """Four identity-rotation cameras with dyadic translations: zc and dist are exact in fp32.  View 2 sits 1 m in front of
    the points (t_z = -1): points with z < 1 are behind it yet project inside onto positive depth."""
    V = 4
    K = torch.tensor([[32.0, 0, 32.0], [0, 32.0, 16.0], [0, 0, 1.0]]).repeat(V, 1, 1)
    K[2, 0, 2], K[2, 1, 2] = 0.0, 0.0
    pose = torch.zeros(V, 3, 4)
    pose[:, :, :3] = torch.eye(3)
    pose[1, 0, 3] = 0.25
    pose[2, 2, 3] = -1.0
    pose[3, 1, 3], pose[3, 2, 3] = 0.125, 0.25
    depth = torch.full((V, EH, EW), D0)
    depth[2] = 0.75
    return {"depth": depth, "K": K, "pose": pose}


def edge_points(extra=2000):
    zs = [D0 + MU_EDGE, D0 - MU_EDGE, float(np.nextafter(np.float32(D0 + MU_EDGE), np.float32(0))), D0 + 2 * MU_EDGE,
          D0 - 2 * MU_EDGE, D0, 2.0 ** -16, -(2.0 ** -16), 0.3]
    us = [32.0, 16.0, -0.25, 64.25, 13.3, 1000.0]
    ws = [16.0, 8.0, -0.25, 32.25, 5.7]
    pts = []
    for z in zs:
        for u in us:
            for w in ws:
                zz = z if abs(z) >= 1e-4 else 1e-3            # the degenerate views project with zc := 1e-3
                pts.append([(u - 32.0) * zz / 32.0, (w - 16.0) * zz / 32.0, z])
    p = torch.tensor(pts, dtype=torch.float32)
    g = torch.Generator().manual_seed(41)
    rnd = torch.rand(extra, 3, generator=g) * torch.tensor([1.2, 0.8, 0.3]) + torch.tensor([-0.5, -0.4, 0.35])
    return torch.cat((p, rnd))


def edge_maps(V):
    g = torch.Generator().manual_seed(42)
    return [torch.randn(V, 9, 17, 8, generator=g), torch.randn(V, EH, EW, 3, generator=g)]


def poison(maps, depth, where):
    """NaN / +Inf / -Inf texels spread over the maps (or one depth texel) of the edge scene."""
    maps = [m.clone() for m in maps]
    if where == "maps":
        vals = [float("nan"), float("inf"), float("-inf")]
        for k, m in enumerate(maps):
            fh, fw = m.shape[1], m.shape[2]
            for v in range(m.shape[0]):
                for j, val in enumerate(vals):
                    m[v, (3 * j + v + k) % fh, (5 * j + 2 * v + 7 * k) % fw, (j + v) % m.shape[3]] = val
    elif where == "depth":
        depth = depth.clone()
        depth[0, 16, 32] = float("nan")
        depth[1, 10, 20] = float("inf")
        depth[3, 20, 40] = float("-inf")
    return maps, depth
