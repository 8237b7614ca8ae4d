"""Iso-surface extraction of a distance volume on the device, volume smoothing, and the vertex colours of the reference's
mesh builders (fusion.py:1313-1416).

`marching_cubes` / `gaussian_filter` bind d3f_mesh_extract / d3f_volume_gaussian (csrc/mesh_kernels.hip); there is no host
implementation of either.  The colour helpers are a few torch ops on 1e4-1e5 vertices and run wherever their inputs live.
"""
import collections

import numpy as np
import torch

from . import _lib

__all__ = ["Mesh", "marching_cubes", "gaussian_filter", "mesh_vertices", "color_mesh", "descriptor_mesh", "descriptor_colors"]

Mesh = collections.namedtuple("Mesh", ["vertices", "faces", "vertex_colors"])
Mesh.__doc__ = """What trimesh.Trimesh(vertices=, faces=, vertex_colors=) receives in the reference, as arrays (returned where trimesh is not
installed): faces = triangles[..., ::-1], vertex_colors uint8 [Nv, 4]."""


def _volume(vol, shape):
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise RuntimeError("the volume must be a tensor on the ROCm device (no CPU path)")
    nx, ny, nz = (int(s) for s in shape)
    if vol.numel() != nx * ny * nz:
        raise ValueError("volume of %d elements does not match the grid shape %s" % (vol.numel(), (nx, ny, nz)))
    return vol.detach().to(torch.float32).contiguous().view(-1), nx, ny, nz


def gaussian_filter(vol, shape, sigma=1.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter(vol.reshape(shape), sigma, mode='reflect', truncate=truncate) in fp32 on the device
    (d3f_volume_gaussian); returns a new flat tensor."""
    v, nx, ny, nz = _volume(vol, shape)
    out = torch.empty_like(v)
    with _lib.on(v.device) as q:
        ws, ws_bytes = q.workspace("d3f_volume_gaussian_workspace_bytes", nx, ny, nz)
        q.d3f_volume_gaussian(v, out, nx, ny, nz, float(sigma), float(truncate), ws, ws_bytes)
    return out


def marching_cubes(vol, shape, iso=0.0, valid=None, count_first=False, capacities=None):
    """(keys int64 [Nv], t float32 [Nv], triangles int32 [M, 3]) of the iso-surface, on the device (include/d3fields_hip.h,
    d3f_mesh_extract: vertices in ascending key order, key = 3*flat(lower endpoint) + axis).

    The first run uses a guess of the capacities (or d3f_mesh_count's answer with count_first); when the surface is larger
    the call is repeated once with the exact counts, as grid_shell does."""
    v, nx, ny, nz = _volume(vol, shape)
    dev = v.device
    if valid is not None:
        if valid.device != dev or valid.numel() != v.numel() or valid.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("valid must be a bool / uint8 tensor of the volume's size on %s" % dev)
        valid = valid.contiguous().view(-1)
    counts = torch.empty(2, dtype=torch.int64, device=dev)       # (both calls write both counts)
    with _lib.on(dev) as q:
        ws, ws_bytes = q.workspace("d3f_mesh_workspace_bytes", nx, ny, nz)
        if count_first:
            q.d3f_mesh_count(v, valid, nx, ny, nz, float(iso), counts, ws, ws_bytes)
            cap_v, cap_t = (int(c) for c in counts.tolist())
        elif capacities is not None:
            cap_v, cap_t = (int(c) for c in capacities)
        else:                                          # a surface crosses ~ one edge per lattice point of a slice
            cap_v = max(1 << 16, 8 * max(nx * ny, ny * nz, nx * nz))
            cap_t = 2 * cap_v
        while True:
            keys = torch.empty(cap_v, dtype=torch.int64, device=dev)
            t = torch.empty(cap_v, dtype=torch.float32, device=dev)
            tris = torch.empty((cap_t, 3), dtype=torch.int32, device=dev)
            q.d3f_mesh_extract(v, valid, nx, ny, nz, float(iso), cap_v, cap_t, keys, t, tris, counts, ws, ws_bytes)
            nv, nt = (int(c) for c in counts.tolist())
            if nv <= cap_v and nt <= cap_t:
                break
            cap_v, cap_t = nv, nt                      # one exact re-run
    return keys[:nv], t[:nv], tris[:nt]


def mesh_vertices(keys, t, shape, coords, snap=True):
    """Vertex coordinates from edge keys.  coords(flat indices) -> [N, 3] coordinates of lattice points.  snap: the lower
    endpoint of the edge -- what `vertices.astype(np.int32)` + ravel_multi_index selects in the reference -- and the upper
    one where t == 1 exactly; else the interpolated position a + t * (b - a)."""
    nx, ny, nz = (int(s) for s in shape)
    a = keys // 3
    axis = keys - 3 * a
    stride = torch.tensor([ny * nz, nz, 1], dtype=torch.int64, device=keys.device)[axis]
    b = a + stride
    if snap:
        return coords(torch.where(t == 1.0, b, a))
    pa, pb = coords(a), coords(b)
    return pa + t.to(device=pa.device, dtype=pa.dtype)[:, None] * (pb - pa)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _make(vertices, triangles, colors):
    faces = triangles[..., ::-1] if isinstance(triangles, np.ndarray) else torch.flip(triangles, dims=(-1,))
    try:
        import trimesh
    except ImportError:
        return Mesh(vertices, faces, colors)
    return trimesh.Trimesh(vertices=_host(vertices), faces=_host(faces), vertex_colors=_host(colors))


def _alpha(rgb_u8):
    return torch.cat([rgb_u8, torch.full((rgb_u8.shape[0], 1), 255, dtype=torch.uint8, device=rgb_u8.device)], dim=1)


def color_mesh(vertices, triangles, res):
    """Reference create_color_mesh (fusion.py:1411-1416): BGR flip, (x * 255).astype(uint8), alpha 255."""
    colors = torch.as_tensor(res["color_tensor"]).detach()
    colors = torch.flip(colors, dims=(-1,))
    colors = _alpha((colors * 255).to(torch.uint8))
    return _make(vertices, triangles, colors)


def pca_project(pca, features):
    """pca.transform(features) for any object with mean_ and components_ (and sklearn's whiten / explained_variance_), in
    float64 where the features live."""
    x = torch.as_tensor(features).detach().to(torch.float64)
    mean = torch.as_tensor(np.asarray(pca.mean_, dtype=np.float64), device=x.device)
    comp = torch.as_tensor(np.asarray(pca.components_, dtype=np.float64), device=x.device)
    y = (x - mean) @ comp.T
    if getattr(pca, "whiten", False):
        y = y / torch.sqrt(torch.as_tensor(np.asarray(pca.explained_variance_, dtype=np.float64), device=x.device))
    return y


def descriptor_rgb(res, params):
    """float64 [Nv, 3] of create_descriptor_mesh before the uint8 conversion (fusion.py:1387-1404)."""
    from .fusion import onehot2instance
    mask = torch.as_tensor(res["mask"]).detach()
    inst = onehot2instance(mask) if mask.is_cuda else torch.from_numpy(onehot2instance(mask.numpy()))
    bg = inst == 0
    proj = pca_project(params["pca"], res["dino_feats"])
    lo, hi = proj.min(dim=0).values, proj.max(dim=0).values
    rgb = torch.zeros((proj.shape[0], 3), dtype=torch.float64, device=proj.device)
    rgb[:, :proj.shape[1]] = (proj - lo) / (hi - lo)
    rgb[bg.to(rgb.device)] = 0.8
    return torch.flip(rgb, dims=(-1,))


def descriptor_colors(proj, mask, mask_out_bg=False):
    """uint8 [N,4] vertex colours from ALREADY-PROJECTED descriptors (Fusion.add_projection with a 3-component head) and the
    fused mask [N,NI], where the inputs live: the colour rule of create_descriptor_mesh (fusion.py:1394-1407) -- per-component
    min / max normalisation over all rows, background rows (instance 0) 0.8, BGR order, (x * 255) truncated, alpha 255 -- in
    float32, without the wide rows and the float64 pca_project of descriptor_rgb.  mask_out_bg: both branches are the same
    lines in the reference."""
    from .fusion import onehot2instance
    proj = torch.as_tensor(proj).detach().to(torch.float32)
    mask = torch.as_tensor(mask).detach()
    if proj.dim() != 2 or not 1 <= proj.shape[1] <= 3 or mask.dim() != 2 or mask.shape[0] != proj.shape[0]:
        raise ValueError("descriptor_colors: proj must be [N,<=3] and mask [N,NI], got %s and %s" % (tuple(proj.shape), tuple(mask.shape)))
    inst = onehot2instance(mask) if mask.is_cuda else torch.from_numpy(onehot2instance(mask.numpy()))
    bg = (inst == 0).to(proj.device)
    lo, hi = proj.min(dim=0).values, proj.max(dim=0).values
    rgb = torch.zeros((proj.shape[0], 3), dtype=torch.float32, device=proj.device)
    rgb[:, :proj.shape[1]] = (proj - lo) / (hi - lo)
    rgb[bg] = 0.8
    return _alpha((torch.flip(rgb, dims=(-1,)) * 255).to(torch.uint8))


def descriptor_mesh(vertices, triangles, res, params, mask_out_bg):
    """Reference create_descriptor_mesh (fusion.py:1386-1409); both branches of mask_out_bg are the same lines there."""
    rgb = descriptor_rgb(res, params)
    return _make(vertices, triangles, _alpha((rgb * 255).to(torch.uint8)))
