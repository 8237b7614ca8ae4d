"""CPU: the float64 reference of the iso-surface extraction (tests/mesh_ref.py) is sound on analytic volumes, the mesh entry
points of the C ABI validate their arguments on the host, and the vertex colours of the mesh builders equal numpy / sklearn."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_ref
from d3fields_amd import _lib, mesh

SHAPE = (21, 17, 25)


# ---- the reference itself --------------------------------------------------------------------------------------------
def _check_common(vol, keys, t, tris, valid=None):
    assert np.all(np.diff(keys) > 0)
    assert np.all((t >= 0) & (t <= 1)) and np.all(np.isfinite(t))
    assert tris.size == 0 or (tris.min() >= 0 and tris.max() < keys.size)
    assert np.unique(tris).size == keys.size                       # every vertex belongs to an emitting cell, i.e. to a triangle
    # the vertex set, once more and independently: one lattice edge per key, endpoints straddle
    a = keys // 3
    b = a + np.asarray([vol.shape[1] * vol.shape[2], vol.shape[2], 1])[keys % 3]
    flat = vol.reshape(-1)
    assert np.all((flat[a] < 0) != (flat[b] < 0))
    assert np.all(np.isfinite(flat[a]) & np.isfinite(flat[b]))
    if valid is not None:
        assert np.all(valid.reshape(-1)[a] & valid.reshape(-1)[b])


@pytest.mark.parametrize("name,chi,parts", [("sphere", 2, 1), ("torus", 0, 1), ("two_spheres", 4, 2)])
def test_reference_on_closed_surfaces(name, chi, parts):
    vol = getattr(mesh_ref, name)(SHAPE)
    keys, t, tris = mesh_ref.reference_mesh(vol)
    _check_common(vol, keys, t, tris)
    assert mesh_ref.is_closed_manifold(tris)
    assert mesh_ref.boundary_edges(tris).size == 0
    assert mesh_ref.euler_characteristic(keys.size, tris) == chi
    assert mesh_ref.connected_components(keys.size, tris) == parts
    pos = mesh_ref.vertex_positions(keys, t, SHAPE)
    vol_mesh = mesh_ref.signed_volume(pos, tris)
    assert vol_mesh > 0                                            # negative inside, normals towards value > iso
    if name == "sphere":
        r = 0.36 * (min(SHAPE) - 1)
        assert abs(vol_mesh / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.05
        # vertices lie on the sphere to within the linear interpolation's error
        c = np.asarray([(n - 1) / 2.0 + 0.13 * (k + 1) for k, n in enumerate(SHAPE)])
        assert np.max(np.abs(np.linalg.norm(pos - c, axis=1) - r)) < 0.08


def test_reference_all_vertex_count_equals_straddling_edges_without_masks():
    vol = mesh_ref.smooth_noise(SHAPE, seed=4)
    keys, t, tris = mesh_ref.reference_mesh(vol)
    inside = vol < 0
    n = sum(int(np.count_nonzero(np.diff(inside, axis=ax))) for ax in range(3))
    assert keys.size == n and n > 500
    _check_common(vol, keys, t, tris)
    # open at the volume border only
    pos = mesh_ref.vertex_positions(keys, t, SHAPE)
    for a, b in mesh_ref.boundary_edges(tris):
        on_border = [np.any((pos[v] == 0) | (pos[v] == np.asarray(SHAPE) - 1)) for v in (a, b)]
        assert all(on_border)


def test_reference_plane_through_lattice_points_has_t_zero_and_degenerate_triangles():
    vol = mesh_ref.lattice_plane(SHAPE)
    keys, t, tris = mesh_ref.reference_mesh(vol)
    # value == iso is NOT inside: the crossing edges are the x-edges arriving at the layer from below, with t == 1
    assert np.all(keys % 3 == 0) and np.all(t == 1.0)
    assert keys.size == SHAPE[1] * SHAPE[2]
    assert tris.shape[0] == 2 * (SHAPE[1] - 1) * (SHAPE[2] - 1)
    vol2 = -vol                                                    # now the layer's upward edges cross, with t == 0
    k2, t2, _ = mesh_ref.reference_mesh(vol2)
    assert np.all(t2 == 0.0) and k2.size == keys.size


def test_reference_skips_cells_with_bad_corners():
    vol, valid = mesh_ref.troubled(SHAPE)
    keys, t, tris = mesh_ref.reference_mesh(vol, valid=valid)
    _check_common(vol, keys, t, tris, valid)
    k0, _, tr0 = mesh_ref.reference_mesh(vol)
    assert k0.size > keys.size                                     # the sentinel block adds a spurious sheet without the mask
    good = np.isfinite(vol) & valid
    # no triangle touches a cell with a bad corner: every vertex's edge has good endpoints (checked above) and every
    # triangle's three vertices share a cell whose corners are all good
    cell = np.ones(tuple(n - 1 for n in SHAPE), dtype=bool)
    for c in range(8):
        cell &= mesh_ref._shift(good, c)
    pos = mesh_ref.vertex_positions(keys, t, SHAPE)
    lo = np.floor(pos[tris].min(axis=1) + 1e-9).astype(int)
    lo = np.minimum(lo, np.asarray(SHAPE) - 2)
    assert np.all(cell[lo[:, 0], lo[:, 1], lo[:, 2]])
    # boundary edges occur only next to a bad cell or the border
    bad_near = ~cell
    for a, b in mesh_ref.boundary_edges(tris):
        m = (pos[a] + pos[b]) / 2.0
        c0 = np.clip(np.floor(m).astype(int) - 1, 0, np.asarray(SHAPE) - 2)
        c1 = np.clip(np.floor(m).astype(int) + 1, 0, np.asarray(SHAPE) - 2)
        near_bad = bad_near[c0[0]:c1[0] + 1, c0[1]:c1[1] + 1, c0[2]:c1[2] + 1].any()
        on_border = np.any((m <= 0.5) | (m >= np.asarray(SHAPE) - 1.5))
        assert near_bad or on_border


def test_reference_with_an_extent_of_two():
    vol = mesh_ref.sphere((2, 19, 23), centre=(0.4, 9.2, 11.1), radius=6.3)
    keys, t, tris = mesh_ref.reference_mesh(vol)
    _check_common(vol, keys, t, tris)
    assert tris.shape[0] > 20


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_mesh_symbols_and_version():
    lib = _lib.load()
    for name in ("d3f_mesh_workspace_bytes", "d3f_mesh_count", "d3f_mesh_extract", "d3f_volume_gaussian", "d3f_volume_gaussian_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 7           # the mesh entry points came with ABI 7


def test_mesh_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    q = ctypes.c_void_p(4096)
    big = 1 << 30

    def count(vol=p, valid=None, shape=(8, 8, 8), iso=0.0, counts=p, ws=p, nbytes=big):
        return lib.d3f_mesh_count(vol, valid, shape[0], shape[1], shape[2], iso, counts, ws, nbytes, None)

    def extract(vol=p, shape=(8, 8, 8), iso=0.0, cv=10, ct=10, keys=p, t=p, tris=p, counts=p, ws=p, nbytes=big):
        return lib.d3f_mesh_extract(vol, None, shape[0], shape[1], shape[2], iso, cv, ct, keys, t, tris, counts, ws, nbytes, None)

    for fn in (count, extract):
        assert fn(shape=(1, 8, 8)) == _lib.ERR_BAD_SHAPE and b"extent" in lib.d3f_last_error()
        assert fn(shape=(8, 0, 8)) == _lib.ERR_BAD_SHAPE
        assert fn(shape=(8, 8, -3)) == _lib.ERR_BAD_SHAPE
        assert fn(shape=(1024, 1024, 1024)) == _lib.ERR_BAD_SHAPE            # more than (2^31 - 1) / 3 points
        assert fn(vol=None) == _lib.ERR_INVALID_ARG
        assert fn(counts=None) == _lib.ERR_INVALID_ARG
        assert fn(ws=None) == _lib.ERR_WORKSPACE
        assert fn(nbytes=lib.d3f_mesh_workspace_bytes(8, 8, 8) - 1) == _lib.ERR_WORKSPACE
        assert fn(iso=float("nan")) == _lib.ERR_INVALID_ARG
        assert fn(vol=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT
    assert extract(cv=-1) == _lib.ERR_INVALID_ARG
    assert extract(keys=None) == _lib.ERR_INVALID_ARG
    assert extract(t=None) == _lib.ERR_INVALID_ARG
    assert extract(tris=None) == _lib.ERR_INVALID_ARG
    assert extract(keys=ctypes.c_void_p(260)) == _lib.ERR_BAD_LAYOUT
    with pytest.raises(_lib.D3FError):
        _lib.check(count(shape=(1, 1, 1)))

    def gauss(src=p, dst=q, shape=(8, 8, 8), sigma=1.0, truncate=4.0, ws=p, nbytes=big):
        return lib.d3f_volume_gaussian(src, dst, shape[0], shape[1], shape[2], sigma, truncate, ws, nbytes, None)

    assert gauss(shape=(0, 8, 8)) == _lib.ERR_BAD_SHAPE
    assert gauss(shape=(2048, 2048, 2048)) == _lib.ERR_BAD_SHAPE
    assert gauss(sigma=0.0) == _lib.ERR_INVALID_ARG
    assert gauss(sigma=-1.0) == _lib.ERR_INVALID_ARG
    assert gauss(sigma=float("nan")) == _lib.ERR_INVALID_ARG
    assert gauss(truncate=0.0) == _lib.ERR_INVALID_ARG
    assert gauss(sigma=20.0) == _lib.ERR_BAD_SHAPE and b"radius" in lib.d3f_last_error()      # radius 80 > 64
    assert gauss(src=None) == _lib.ERR_INVALID_ARG
    assert gauss(dst=None) == _lib.ERR_INVALID_ARG
    assert gauss(dst=p) == _lib.ERR_INVALID_ARG                                               # in place is not supported
    assert gauss(ws=None) == _lib.ERR_WORKSPACE
    assert gauss(nbytes=8 * 8 * 8 * 4 - 1) == _lib.ERR_WORKSPACE
    assert lib.d3f_volume_gaussian_workspace_bytes(8, 8, 8) == 8 * 8 * 8 * 4


def test_mesh_workspace_grows_with_workgroups_not_cells():
    lib = _lib.load()
    nbytes = lib.d3f_mesh_workspace_bytes(800, 700, 220)
    assert 0 < nbytes < 800 * 700 * 220 * 4 // 64
    assert lib.d3f_mesh_workspace_bytes(1, 700, 220) == 0
    # two words per 1024 points, the scan's scratch, and alignment padding
    assert lib.d3f_mesh_workspace_bytes(200, 175, 55) <= 2 * 4 * (200 * 175 * 55 // 1024 + 2) + 4096


# ---- vertex colours ----------------------------------------------------------------------------------------------------
def test_color_mesh_equals_the_reference_lines():
    rng = np.random.default_rng(5)
    colors = rng.random((5000, 3), dtype=np.float32)
    colors[:7] = [[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.125], [1 / 255, 2 / 255, 3 / 255], [0.999999, 0.0039, 0.00392157], [0.2, 0.4, 0.6], [0.1, 0.3, 0.7]]
    verts = rng.random((5000, 3))
    tris = rng.integers(0, 5000, (900, 3))
    out = mesh.color_mesh(verts, tris, {"color_tensor": torch.from_numpy(colors)})
    ref = colors[..., ::-1]
    ref = (ref * 255).astype(np.uint8)
    ref = np.concatenate([ref, np.ones((ref.shape[0], 1), dtype=np.uint8) * 255], axis=1)
    got = np.asarray(out.vertex_colors)
    assert got.dtype == np.uint8 and got.shape == (5000, 4)
    assert np.array_equal(got, ref)
    assert np.array_equal(np.asarray(out.faces), tris[..., ::-1])
    assert np.array_equal(np.asarray(out.vertices), verts)


def test_descriptor_mesh_against_sklearn():
    from sklearn.decomposition import PCA
    rng = np.random.default_rng(6)
    n, C = 4000, 48
    feats = (rng.standard_normal((n, 6)) @ rng.standard_normal((6, C)) + 0.1 * rng.standard_normal((n, C))).astype(np.float32)
    mask = rng.random((n, 4)).astype(np.float32)
    pca = PCA(n_components=3).fit(feats[:1500].astype(np.float64))
    res = {"dino_feats": torch.from_numpy(feats), "mask": torch.from_numpy(mask)}
    out = mesh.descriptor_mesh(np.zeros((n, 3)), np.zeros((1, 3), dtype=np.int64), res, {"pca": pca}, True)
    got = np.asarray(out.vertex_colors)
    # the reference's lines (fusion.py:1387-1407) in numpy, the projection by sklearn
    bg = np.argmax(mask, axis=-1).astype(np.uint8) == 0
    proj = pca.transform(feats)
    rgb = np.zeros((n, 3))
    for i in range(3):
        rgb[:, i] = (proj[:, i] - proj[:, i].min()) / (proj[:, i].max() - proj[:, i].min())
    rgb[bg] = np.ones(3) * 0.8
    rgb = rgb[..., ::-1]
    ref = np.concatenate([(rgb * 255).astype(np.uint8), np.ones((n, 1), dtype=np.uint8) * 255], axis=1)
    # the projection, in float64
    mine = mesh.pca_project(pca, torch.from_numpy(feats)).numpy()
    exact = (feats.astype(np.float64) - pca.mean_) @ pca.components_.T
    err = max(float(np.max(np.abs(proj - exact))), float(np.max(np.abs(mine - exact))))
    assert np.max(np.abs(mine - exact)) <= 1e-12 * max(1.0, np.max(np.abs(exact)))
    # uint8 may differ by one only where the float64 value lies within the projection's error of an integer boundary
    span = (exact.max(axis=0) - exact.min(axis=0))[::-1]
    scaled = rgb * 255
    slack = 255.0 * 4.0 * err / span                                 # value, minimum and maximum each carry `err`
    near = np.abs(scaled - np.round(scaled)) <= slack
    diff = got[:, :3].astype(np.int64) - ref[:, :3].astype(np.int64)
    assert np.all(got[:, 3] == 255)
    assert np.all(np.abs(diff) <= 1)
    assert np.all(near[diff != 0])
    # a condition on the reference alone: with this seed fewer than 1 % of the entries sit that close to a boundary
    assert np.count_nonzero(near & ~bg[:, None]) < 0.01 * near.size
    assert np.array_equal(got[bg, :3], np.full((int(bg.sum()), 3), 204, dtype=np.uint8))


def test_mask_meshes_name_trimesh_when_it_is_absent():
    try:
        import trimesh  # noqa: F401
        return                      # trimesh is installed: the colour maps are its own
    except ImportError:
        pass
    from d3fields_amd import Fusion
    f = Fusion.__new__(Fusion)
    for fn in (f.create_mask_mesh, f.create_instance_mask_mesh):
        with pytest.raises(NotImplementedError, match="trimesh"):
            fn(np.zeros((3, 3)), np.zeros((1, 3), dtype=np.int64), {})
