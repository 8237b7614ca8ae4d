"""The iso-surface extraction (d3f_mesh_count / d3f_mesh_extract) and the volume Gaussian (d3f_volume_gaussian) on the MI355X,
against the float64 reference of tests/mesh_ref.py (shown sound in tests/test_mesh_host.py) and scipy, plus
Fusion.extract_mesh / mesh_from_grid / create_color_mesh end to end.

Bounds.  keys and triangles: exact.  t: |dt| <= 2^-22 against the float64 quotient of the same fp32 inputs (two subtractions
and one division, each correctly rounded: below 1.5 ulp of a number <= 1).  Gaussian: 3 (T + 2) 2^-24 max|x| with T taps per
pass (the summation bound for positive weights that sum to one, three passes)."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_ref

pytestmark = pytest.mark.gpu

SHAPE = (37, 29, 53)
GUARD = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cpu(x):
    return x.detach().cpu().numpy()


def _raw_extract(dev, vol, valid, iso, cap_v, cap_t, count_first=False):
    """One d3f_mesh_extract with guard bytes behind every output; returns (keys, t, tris, counts) as the kernels left them."""
    from d3fields_amd import _lib
    lib = _lib.load()
    nx, ny, nz = vol.shape
    v = torch.from_numpy(np.ascontiguousarray(vol)).to(dev).view(-1)
    va = torch.from_numpy(np.ascontiguousarray(valid)).to(dev).view(-1) if valid is not None else None
    ws_bytes = int(lib.d3f_mesh_workspace_bytes(nx, ny, nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    stream = _lib.current_stream_handle(dev)
    if count_first:
        _lib.check(lib.d3f_mesh_count(_lib.ptr(v), _lib.ptr(va), nx, ny, nz, iso, _lib.ptr(counts), _lib.ptr(ws), ws_bytes, stream))
        cap_v, cap_t = (int(c) for c in counts.tolist())
    pad = 64
    keys = torch.full((cap_v * 8 + pad,), GUARD, dtype=torch.uint8, device=dev)
    t = torch.full((cap_v * 4 + pad,), GUARD, dtype=torch.uint8, device=dev)
    tris = torch.full((cap_t * 12 + pad,), GUARD, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_mesh_extract(_lib.ptr(v), _lib.ptr(va), nx, ny, nz, iso, cap_v, cap_t, _lib.ptr(keys), _lib.ptr(t), _lib.ptr(tris),
                                    _lib.ptr(counts), _lib.ptr(ws), ws_bytes, stream))
    torch.cuda.synchronize()
    for buf, used in ((keys, cap_v * 8), (t, cap_v * 4), (tris, cap_t * 12)):
        assert bool((buf[used:] == GUARD).all()), "written past a capacity"
    nv, nt = (int(c) for c in counts.tolist())
    k = keys[:cap_v * 8].view(torch.int64)[:min(nv, cap_v)]
    tt = t[:cap_v * 4].view(torch.float32)[:min(nv, cap_v)]
    tr = tris[:cap_t * 12].view(torch.int32).view(-1, 3)[:min(nt, cap_t)]
    return cpu(k), cpu(tt), cpu(tr), (nv, nt)


def _t_reference(vol, keys, iso):
    flat = vol.reshape(-1).astype(np.float64)
    a = keys // 3
    b = a + np.asarray([vol.shape[1] * vol.shape[2], vol.shape[2], 1])[keys % 3]
    return (np.float64(np.float32(iso)) - flat[a]) / (flat[b] - flat[a])


def _compare(dev, vol, valid=None, iso=0.0):
    rk, rt, rtri = mesh_ref.reference_mesh(vol, iso=iso, valid=valid)
    k, t, tri, (nv, nt) = _raw_extract(dev, vol, valid, iso, 0, 0, count_first=True)
    assert (nv, nt) == (rk.size, rtri.shape[0])
    assert np.array_equal(k, rk)                                             # same set, same order
    assert t.dtype == np.float32 and np.all(np.isfinite(t)) and np.all((t >= 0) & (t <= 1)) and not np.any(np.signbit(t))
    err = float(np.max(np.abs(t.astype(np.float64) - _t_reference(vol, rk, iso)))) if rk.size else 0.0
    print("max |dt| = %.3g (bound 2^-22 = %.3g), %d vertices, %d triangles" % (err, 2.0 ** -22, nv, nt))
    assert err <= 2.0 ** -22
    assert np.array_equal(tri.astype(np.int64), rtri)                        # same table, same order
    assert tri.size == 0 or (tri.min() >= 0 and tri.max() < nv)
    # byte-identical second run; count skipped with capacities that are too small, then the exact re-run
    k2, t2, tri2, _ = _raw_extract(dev, vol, valid, iso, nv, nt)
    assert k2.tobytes() == k.tobytes() and t2.tobytes() == t.tobytes() and tri2.tobytes() == tri.tobytes()
    _, _, _, small = _raw_extract(dev, vol, valid, iso, max(nv // 3, 1), max(nt // 5, 1))
    assert small == (nv, nt)                                                 # the true counts, nothing past the capacities
    _, _, _, small = _raw_extract(dev, vol, valid, iso, nv, max(nt // 2, 1))
    assert small == (nv, nt)
    k3, t3, tri3, _ = _raw_extract(dev, vol, valid, iso, *small)
    assert k3.tobytes() == k.tobytes() and t3.tobytes() == t.tobytes() and tri3.tobytes() == tri.tobytes()
    return k, t, tri


@pytest.mark.parametrize("name,chi,parts", [("sphere", 2, 1), ("torus", 0, 1), ("two_spheres", 4, 2)])
def test_closed_surfaces(dev, name, chi, parts):
    vol = getattr(mesh_ref, name)(SHAPE)
    k, t, tri = _compare(dev, vol)
    assert mesh_ref.is_closed_manifold(tri)
    assert mesh_ref.euler_characteristic(k.size, tri) == chi
    assert mesh_ref.connected_components(k.size, tri) == parts
    assert mesh_ref.signed_volume(mesh_ref.vertex_positions(k, t, SHAPE), tri.astype(np.int64)) > 0


@pytest.mark.parametrize("iso", [0.0, 0.37, -1.25])
def test_other_iso_values(dev, iso):
    k, t, tri = _compare(dev, mesh_ref.sphere(SHAPE), iso=iso)
    assert mesh_ref.is_closed_manifold(tri) and mesh_ref.euler_characteristic(k.size, tri) == 2


def test_plane_through_lattice_points(dev):
    vol = mesh_ref.lattice_plane(SHAPE)
    k, t, tri = _compare(dev, vol)
    assert np.all(t == 1.0) and k.size == SHAPE[1] * SHAPE[2]
    k, t, tri = _compare(dev, -vol)
    assert np.all(t == 0.0) and k.size == SHAPE[1] * SHAPE[2]
    # values equal to iso on whole blocks: degenerate triangles are emitted, not filtered
    blocky = mesh_ref.sphere(SHAPE).copy()
    blocky[np.abs(blocky) < 0.8] = 0.0
    k, t, tri = _compare(dev, blocky)
    assert np.count_nonzero(t == 0.0) + np.count_nonzero(t == 1.0) > 100


def test_smooth_noise(dev):
    for seed in (0, 7):
        vol = mesh_ref.smooth_noise(SHAPE, seed=seed)
        k, t, tri = _compare(dev, vol)
        assert k.size > 3000
        pos = mesh_ref.vertex_positions(k, t, SHAPE)
        for a, b in mesh_ref.boundary_edges(tri.astype(np.int64)):           # open at the volume border only
            assert all(np.any((pos[v] == 0) | (pos[v] == np.asarray(SHAPE) - 1)) for v in (a, b))


def test_nan_invalid_and_sentinel_regions(dev):
    vol, valid = mesh_ref.troubled(SHAPE)
    k0, _, _ = _compare(dev, vol)                                            # NaN / Inf alone
    k, t, tri = _compare(dev, vol, valid=valid)
    assert 0 < k.size < k0.size
    good = np.isfinite(vol) & valid
    cell = np.ones(tuple(n - 1 for n in SHAPE), dtype=bool)
    for c in range(8):
        cell &= mesh_ref._shift(good, c)
    pos = mesh_ref.vertex_positions(k, t, SHAPE)
    lo = np.minimum(np.floor(pos[tri].min(axis=1) + 1e-9).astype(int), np.asarray(SHAPE) - 2)
    assert np.all(cell[lo[:, 0], lo[:, 1], lo[:, 2]])                        # no triangle touches a cell with a bad corner
    for a, b in mesh_ref.boundary_edges(tri.astype(np.int64)):
        m = (pos[a] + pos[b]) / 2.0
        c0 = np.clip(np.floor(m).astype(int) - 1, 0, np.asarray(SHAPE) - 2)
        c1 = np.clip(np.floor(m).astype(int) + 1, 0, np.asarray(SHAPE) - 2)
        assert (~cell)[c0[0]:c1[0] + 1, c0[1]:c1[1] + 1, c0[2]:c1[2] + 1].any() or np.any((m <= 0.5) | (m >= np.asarray(SHAPE) - 1.5))
    # uint8 and bool masks are the same thing
    k_u8, _, _, _ = _raw_extract(dev, vol, valid.astype(np.uint8), 0.0, k.size, tri.shape[0])
    assert np.array_equal(k_u8, k)


@pytest.mark.parametrize("shape", [(2, 29, 53), (37, 2, 53), (37, 29, 2), (2, 2, 2), (5, 3, 1031)])
def test_thin_volumes(dev, shape):
    c = [(n - 1) * 0.45 + 0.1 for n in shape]
    vol = mesh_ref.sphere(shape, c, 0.3 * max(shape[0], shape[1], min(shape[2], 40)) + 0.2)
    k, t, tri = _compare(dev, vol)
    assert k.size > 0
    _compare(dev, mesh_ref.smooth_noise(shape, seed=2))


def test_empty_surface(dev):
    vol = np.full(SHAPE, 1.0, dtype=np.float32)
    k, t, tri = _compare(dev, vol)
    assert k.size == 0 and tri.shape[0] == 0
    _compare(dev, np.full(SHAPE, np.nan, dtype=np.float32))


# ---- Fusion ----------------------------------------------------------------------------------------------------------
def _bare_fusion(dev):
    from d3fields_amd import Fusion
    return Fusion(num_cam=1, device=str(dev))


def _grid_points(shape, step=0.01):
    axes = [torch.arange(n, dtype=torch.float32) * step - 0.2 + 0.003 * k for k, n in enumerate(shape)]
    return torch.cartesian_prod(*axes)


def test_extract_mesh_defaults_snap_to_lattice_points(dev):
    f = _bare_fusion(dev)
    pts = _grid_points(SHAPE)
    for vol in (mesh_ref.torus(SHAPE), mesh_ref.lattice_plane(SHAPE)):
        res = {"dist": torch.from_numpy(vol.reshape(-1)).to(dev), "valid_mask": torch.ones(vol.size, dtype=torch.bool, device=dev)}
        verts, tris = f.extract_mesh(pts, res, SHAPE)
        rk, rt, rtri = mesh_ref.reference_mesh(vol)
        assert isinstance(verts, np.ndarray) and isinstance(tris, np.ndarray) and tris.dtype == np.int32
        assert np.array_equal(tris.astype(np.int64), rtri)
        a = rk // 3
        b = a + np.asarray([SHAPE[1] * SHAPE[2], SHAPE[2], 1])[rk % 3]
        want = pts.numpy()[np.where(rt == 1.0, b, a)]                         # the upper endpoint where t == 1, as astype(int32) does
        assert np.array_equal(verts, want)
        if np.all(rt < 1.0):
            assert np.array_equal(verts, pts.numpy()[rk // 3])
        else:
            assert np.count_nonzero(rt == 1.0) == SHAPE[1] * SHAPE[2]
        # device in, device out
        v_dev, t_dev = f.extract_mesh(pts.to(dev), res, SHAPE, as_numpy=False)
        assert v_dev.is_cuda and t_dev.is_cuda and t_dev.dtype == torch.int32
        assert np.array_equal(cpu(v_dev), want) and np.array_equal(cpu(t_dev), tris)
        # host dist / numpy pts are uploaded once
        v_h, _ = f.extract_mesh(pts.numpy(), {"dist": torch.from_numpy(vol.reshape(-1))}, SHAPE)
        assert np.array_equal(v_h, want)


def test_extract_mesh_interpolated_positions(dev):
    f = _bare_fusion(dev)
    step = 0.01
    pts = _grid_points(SHAPE, step)
    vol = mesh_ref.two_spheres(SHAPE)
    res = {"dist": torch.from_numpy(vol.reshape(-1)).to(dev)}
    verts, _ = f.extract_mesh(pts, res, SHAPE, snap=False)
    rk, rt, _ = mesh_ref.reference_mesh(vol)
    a = rk // 3
    b = a + np.asarray([SHAPE[1] * SHAPE[2], SHAPE[2], 1])[rk % 3]
    p = pts.numpy().astype(np.float64)
    want = p[a] + rt[:, None] * (p[b] - p[a])
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2.0 ** -22 * step
    err = np.abs(verts.astype(np.float64) - want)
    print("max position error / bound = %.3g" % float(np.max(err / bound)))
    assert verts.dtype == np.float32 and np.all(err <= bound)


def _scene_fusion(dev, H=120, W=160):
    from d3fields_amd import Fusion, synth
    sc = synth.make_scene(4, H, W, "smooth")
    f = Fusion(num_cam=4, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    return f, sc


def test_mesh_from_grid_equals_extract_mesh_of_the_materialised_grid(dev):
    from d3fields_amd import create_init_grid, synth
    f, _ = _scene_fusion(dev)
    box, step = dict(synth.WORK_BOX), 0.011
    pts, shape = create_init_grid(box, step)
    assert len({int(s) for s in shape}) == 3
    pts = pts.to(dev)
    with torch.no_grad():
        res = f.batch_eval(pts, return_names=[])
    for kw in (dict(), dict(use_valid_mask=True), dict(use_valid_mask=True, snap=False), dict(smooth="gaussian", sigma=0.8, use_valid_mask=True)):
        v1, t1 = f.extract_mesh(pts, res, shape, as_numpy=False, **kw)
        v2, t2 = f.mesh_from_grid(box, step, as_numpy=False, **kw)
        assert v1.shape[0] > 500 and t1.shape[0] > 500
        assert torch.equal(t1, t2) and cpu(v1).tobytes() == cpu(v2).tobytes(), kw
    # the documented consequence of no mask and no smoothing: a second sheet where dist jumps to the sentinel
    n_plain = f.mesh_from_grid(box, step)[0].shape[0]
    n_masked = f.mesh_from_grid(box, step, use_valid_mask=True)[0].shape[0]
    assert n_plain > n_masked
    # a host callable as the smoother
    v3, t3 = f.extract_mesh(pts, res, shape, smooth=lambda v: v + 0.0, use_valid_mask=True)
    v4, t4 = f.extract_mesh(pts, res, shape, use_valid_mask=True)
    assert np.array_equal(v3, v4) and np.array_equal(t3, t4)
    with pytest.raises(ValueError):
        f.extract_mesh(pts, res, shape, smooth="box")


def test_end_to_end_on_the_synthetic_scene(dev):
    from d3fields_amd import synth
    H, W, C = 120, 160, 32
    f, sc = _scene_fusion(dev, H, W)
    f.curr_obs_torch["dino_feats"] = synth.random_map(4, H // 10, W // 10, C, seed=2, device=str(dev))
    f.curr_obs_torch["mask"] = synth.random_onehot_mask(4, H, W, 5, seed=3, device=str(dev)).to(torch.float32)
    f.curr_obs_torch["color_tensor"] = synth.random_map(4, H, W, 3, seed=4, device=str(dev)).abs().clamp(0, 1)
    box, step = dict(synth.WORK_BOX), 0.009
    with torch.no_grad():
        res = f.eval_grid(box, step, return_names=[])
        shape = res["grid_shape"]
        from d3fields_amd import create_init_grid
        pts = create_init_grid(box, step)[0].to(dev)
        verts, tris = f.extract_mesh(pts, res, shape, use_valid_mask=True, as_numpy=False)
        out = f.batch_eval(verts, return_names=["dino_feats", "mask", "color_tensor"])
    nv = verts.shape[0]
    assert nv > 1000 and tris.shape[0] > 1000 and int(tris.max()) < nv and int(tris.min()) >= 0
    assert out["dino_feats"].shape == (nv, C) and out["mask"].shape == (nv, 5) and out["color_tensor"].shape == (nv, 3)
    m = f.create_color_mesh(verts, tris, out)
    colors = cpu(m.vertex_colors) if isinstance(m.vertex_colors, torch.Tensor) else np.asarray(m.vertex_colors)
    assert colors.shape == (nv, 4) and colors.dtype == np.uint8 and np.all(colors[:, 3] == 255)
    ref = (cpu(out["color_tensor"])[..., ::-1] * 255).astype(np.uint8)
    assert np.array_equal(colors[:, :3], ref)
    faces = cpu(m.faces) if isinstance(m.faces, torch.Tensor) else np.asarray(m.faces)
    assert np.array_equal(faces, cpu(tris)[..., ::-1])
    # every snapped vertex is an endpoint of a sign-changing edge of the volume
    dist = cpu(res["dist"]).reshape(tuple(shape))
    inside = dist < 0
    endpoint = np.zeros(dist.shape, dtype=bool)
    for ax in range(3):
        change = np.diff(inside, axis=ax) != 0
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        endpoint[tuple(lo)] |= change
        endpoint[tuple(hi)] |= change
    allowed = {p.tobytes() for p in cpu(pts)[endpoint.reshape(-1)]}
    assert all(p.tobytes() in allowed for p in cpu(verts))


def test_full_size_volume_once(dev):
    """The 800 x 700 x 220 distance volume of bench.py's dist_only workload with its valid_mask: one run of count + extract,
    then one more extract for the byte comparison.  No loop, no retry."""
    import bench
    from d3fields_amd import mesh
    f, pts, names, w, sc = bench.build_workload("dist_only", dev, 0, 1, "grid")
    shape = (800, 700, 220)
    assert pts.shape[0] == 800 * 700 * 220
    with torch.no_grad():
        res = f.batch_eval(pts, return_names=[])
    del pts
    dist, valid = res["dist"], res["valid_mask"]
    keys, t, tris = mesh.marching_cubes(dist, shape, valid=valid, count_first=True)
    d3 = dist.view(shape)
    inside = d3 < 0
    good = torch.isfinite(d3) & valid.view(shape)
    cell = good[:-1, :-1, :-1].clone()
    for c in range(1, 8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cell &= good[dx:799 + dx, dy:699 + dy, dz:219 + dz]
    n_edges = 0
    for ax in range(3):                                  # three comparisons, restricted by `valid` the way the kernels are
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        straddle = (inside[tuple(lo)] != inside[tuple(hi)]) & good[tuple(lo)] & good[tuple(hi)]
        others = [a for a in range(3) if a != ax]
        padded = [799, 699, 219]
        padded[others[0]] += 2
        padded[others[1]] += 2
        cp = torch.zeros(padded, dtype=torch.bool, device=dev)          # the cells, one empty layer round the other two axes
        inner = [slice(None)] * 3
        inner[others[0]] = inner[others[1]] = slice(1, -1)
        cp[tuple(inner)] = cell
        touch = torch.zeros_like(straddle)
        for du in (0, 1):
            for dw in (0, 1):
                sl = [slice(None)] * 3
                sl[others[0]] = slice(du, du + straddle.shape[others[0]])
                sl[others[1]] = slice(dw, dw + straddle.shape[others[1]])
                touch |= cp[tuple(sl)]
        n_edges += int((straddle & touch).sum())
        del straddle, touch, cp
    print("800 x 700 x 220: %d vertices, %d triangles" % (keys.numel(), tris.shape[0]))
    assert keys.numel() == n_edges and n_edges > 100000
    assert bool((keys[1:] > keys[:-1]).all())
    assert int(tris.min()) >= 0 and int(tris.max()) < keys.numel()
    assert bool(((t >= 0) & (t <= 1)).all())
    k2, t2, tris2 = mesh.marching_cubes(dist, shape, valid=valid, capacities=(keys.numel(), tris.shape[0]))
    assert torch.equal(keys, k2) and torch.equal(tris, tris2) and cpu(t).tobytes() == cpu(t2).tobytes()


# ---- the Gaussian filter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.7, 1.0, 3.0])
@pytest.mark.parametrize("shape", [SHAPE, (5, 70, 131), (3, 2, 9), (130, 9, 7), (1, 1, 40)])
def test_gaussian_against_scipy(dev, sigma, shape):
    from scipy import ndimage
    from d3fields_amd import mesh
    rng = np.random.default_rng(int(sigma * 10) + shape[0])
    vol = (rng.standard_normal(shape) * 3.0 + 1.0).astype(np.float32)
    got = cpu(mesh.gaussian_filter(torch.from_numpy(vol).to(dev), shape, sigma=sigma)).reshape(shape)
    ref = ndimage.gaussian_filter(vol.astype(np.float64), sigma, mode="reflect", truncate=4.0)
    taps = 2 * int(4.0 * sigma + 0.5) + 1
    bound = 3 * (taps + 2) * 2.0 ** -24 * float(np.max(np.abs(vol)))
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print("sigma %.1f shape %s: max |d| = %.3g, bound %.3g" % (sigma, shape, err, bound))
    assert err <= bound
    again = cpu(mesh.gaussian_filter(torch.from_numpy(vol).to(dev), shape, sigma=sigma)).reshape(shape)
    assert again.tobytes() == got.tobytes()
