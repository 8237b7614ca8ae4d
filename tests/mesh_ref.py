"""float64 / numpy reference of the iso-surface extraction (include/d3fields_hip.h, d3f_mesh_extract), the analytic test
volumes, and the property checks of a triangle mesh.  A plain module: tests/test_mesh_host.py shows it sound on the CPU,
tests/test_gpu_mesh.py compares the HIP kernels with it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_mc_table  # noqa: E402

sys.path.pop(0)

TABLE = gen_mc_table.build_table()


def _shift(a, c):
    """a at corner c of every cell: shape (nx-1, ny-1, nz-1)."""
    dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
    nx, ny, nz = a.shape
    return a[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]


def reference_mesh(vol, iso=0.0, valid=None):
    """(keys int64 [Nv] ascending, t float64 [Nv], triangles int64 [M, 3]) of a float32 volume [nx, ny, nz].

    Vertices: three array comparisons (one per axis) of straddling edges with good endpoints that touch an emitting cell.
    Triangles: emitting cells in flat order, the generator's table (scripts/gen_mc_table.py) inside a cell."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    iso32 = np.float32(iso)
    nx, ny, nz = vol.shape
    good = np.isfinite(vol)
    if valid is not None:
        good &= np.asarray(valid).reshape(vol.shape).astype(bool)
    with np.errstate(invalid="ignore"):
        inside = vol < iso32
    cell = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    for c in range(8):
        cell &= _shift(good, c)
    flat = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    keys, va, vb = [], [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        straddle = good[lo] & good[hi] & (inside[lo] != inside[hi])
        # an edge along `axis` at (.., u, w) touches the cells (.., u-1..u, w-1..w): pad the cell array by one on both sides
        pad = [(1, 1)] * 3
        pad[axis] = (0, 0)
        cp = np.pad(cell, pad, constant_values=False)
        touch = np.zeros(straddle.shape, dtype=bool)
        for du in (0, 1):
            for dw in (0, 1):
                sl = [slice(None)] * 3
                others = [a for a in range(3) if a != axis]
                sl[others[0]] = slice(du, du + straddle.shape[others[0]])
                sl[others[1]] = slice(dw, dw + straddle.shape[others[1]])
                touch |= cp[tuple(sl)]
        sel = straddle & touch
        keys.append(3 * flat[lo][sel] + axis)
        va.append(vol[lo][sel])
        vb.append(vol[hi][sel])
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    va = np.concatenate(va)[order].astype(np.float64)
    vb = np.concatenate(vb)[order].astype(np.float64)
    t = (np.float64(iso32) - va) / (vb - va)

    case = np.zeros(cell.shape, dtype=np.int64)
    for c in range(8):
        case |= _shift(inside, c).astype(np.int64) << c
    case[~cell] = 0
    strides = (ny * nz, nz, 1)
    tris = []
    for cx, cy, cz in zip(*np.nonzero((case != 0) & (case != 255))):      # C order = ascending flat index of the lowest corner
        p = int(flat[cx, cy, cz])
        for tri in TABLE[int(case[cx, cy, cz])][1]:
            row = []
            for e in tri:
                axis, j = e >> 2, e & 3
                u, w = gen_mc_table.AXES[axis]
                q = p + (j & 1) * strides[u] + (j >> 1) * strides[w]
                k = 3 * q + axis
                pos = int(np.searchsorted(keys, k))
                assert pos < keys.size and keys[pos] == k, "triangle edge without a vertex"
                row.append(pos)
            tris.append(row)
    return keys, t, np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def vertex_positions(keys, t, shape):
    """float64 [Nv, 3] in index space."""
    nx, ny, nz = shape
    a = keys // 3
    axis = keys % 3
    pos = np.stack(np.unravel_index(a, shape), axis=1).astype(np.float64)
    pos[np.arange(keys.size), axis] += np.asarray(t, dtype=np.float64)
    return pos


def directed_edges(tris):
    tris = np.asarray(tris, dtype=np.int64)
    return np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], axis=0)


def boundary_edges(tris):
    """Directed edges whose reverse does not occur exactly as often (empty for a closed, consistently oriented surface)."""
    e = directed_edges(tris)
    if e.size == 0:
        return e
    big = int(e.max()) + 1
    fwd, cf = np.unique(e[:, 0] * big + e[:, 1], return_counts=True)
    count = dict(zip(fwd.tolist(), cf.tolist()))
    out = [(a, b) for a, b in e.tolist() if count.get(b * big + a, 0) != count[a * big + b]]
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def is_closed_manifold(tris):
    """Every directed edge occurs once and its reverse once."""
    e = directed_edges(tris)
    big = int(e.max()) + 1
    code = e[:, 0] * big + e[:, 1]
    if np.unique(code).size != code.size:
        return False
    rev = e[:, 1] * big + e[:, 0]
    return bool(np.array_equal(np.sort(code), np.sort(rev)))


def euler_characteristic(n_vertices, tris):
    e = np.sort(directed_edges(tris), axis=1)
    n_edges = np.unique(e, axis=0).shape[0]
    return n_vertices - n_edges + np.asarray(tris).shape[0]


def connected_components(n_vertices, tris):
    parent = np.arange(n_vertices)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in directed_edges(tris).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(x) for x in np.unique(np.asarray(tris)).tolist()})


def signed_volume(pos, tris):
    p = np.asarray(pos, dtype=np.float64)
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- analytic volumes (float32 [nx, ny, nz]); negative inside ----------------------------------------------------------
def _axes(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def sphere(shape, centre=None, radius=None):
    x, y, z = _axes(shape)
    c = [(n - 1) / 2.0 + 0.13 * (k + 1) for k, n in enumerate(shape)] if centre is None else centre
    r = 0.36 * (min(shape) - 1) if radius is None else radius
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def torus(shape):
    x, y, z = _axes(shape)
    c = [(n - 1) / 2.0 + 0.21 for n in shape]
    big, small = 0.29 * (min(shape[0], shape[1]) - 1), 0.12 * (min(shape) - 1)
    ring = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - big
    return (np.sqrt(ring ** 2 + (z - c[2]) ** 2) - small).astype(np.float32)


def two_spheres(shape):
    r = 0.17 * (min(shape) - 1)
    c1 = [0.3 * (shape[0] - 1) + 0.1, 0.5 * (shape[1] - 1) + 0.2, 0.3 * (shape[2] - 1) + 0.3]
    c2 = [0.7 * (shape[0] - 1) + 0.1, 0.5 * (shape[1] - 1) + 0.2, 0.72 * (shape[2] - 1) + 0.3]
    return np.minimum(sphere(shape, c1, r), sphere(shape, c2, r))


def lattice_plane(shape, at=None):
    """x - at: exactly iso = 0 on the lattice layer ix == at (t = 0 on the edges leaving it upwards, t = 1 on those arriving)."""
    x, _, _ = _axes(shape)
    return (x - (shape[0] // 2 if at is None else at)).astype(np.float32)


def smooth_noise(shape, seed=0):
    """Seeded noise, low-pass filtered (a few box passes with wrap-around): many small closed and open sheets."""
    v = np.random.default_rng(seed).standard_normal(shape)
    for _ in range(3):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + v + np.roll(v, -1, ax)) / 3.0
    return v.astype(np.float32)


def troubled(shape, seed=1):
    """(volume, valid): a sphere with a NaN, an Inf, a block of invalid points and a block at the 1e3 sentinel."""
    v = sphere(shape).copy()
    nx, ny, nz = shape
    v[nx // 2, ny // 2, int(nz * 0.86)] = np.nan
    v[int(nx * 0.15), ny // 2, nz // 2] = np.inf
    v[nx // 2:, : ny // 3, :] = 1e3                      # "behind the surface": a spurious second crossing where it meets dist < 0
    valid = np.ones(shape, dtype=bool)
    valid[: nx // 3, ny // 2:, nz // 3: nz // 2] = False
    valid[nx // 2:, : ny // 3, :] = False
    return v, valid
