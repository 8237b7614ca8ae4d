"""NumPy restatement and case generators of the warp of a baked field by the rigid motions of its parts (d3f_volume_warp_select /
d3f_volume_warp_rows, include/d3fields_hip.h), shared by tests/test_warp_host.py and tests/test_gpu_warp.py.

Coordinates are voxel index units, the flat index is (x*ny + y)*nz + z.  warp_ref / rows_ref state the contract with ONE NumPy operation per
rounded operation (float64 arrays for the inverse map, float32 arrays for the weights and the chain: NumPy rounds every array operation to
the array's type and fuses nothing), so the device must give the same bytes.  warp_loop is a second formulation of the selection that shares
nothing with warp_ref: a plain Python loop per destination voxel and part over Python floats and np.float32 scalars, without any culling.

Generated arrays are read-only."""
import functools
import math

import numpy as np

MAX_PARTS = 4096
POSE = 15
SENTINEL = np.float32(1e3)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
CORNERS = [(c >> 2, (c >> 1) & 1, c & 1) for c in range(8)]      # the samplers' corner order: c = dx*4 + dy*2 + dz


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def pose_row(R=None, src=(0.0, 0.0, 0.0), dst=None):
    """[15]: R row-major, src, dst with q = R (p - src) + dst"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return np.concatenate([R.reshape(9), np.asarray(src, np.float64), np.asarray(src if dst is None else dst, np.float64)])


def shift_row(d):
    return pose_row(dst=d)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


QUARTER_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # 90 degrees about z
HALF_TILTED = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])       # 180 degrees about (1, 1, 0) / sqrt 2
THIRD_DIAGONAL = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])     # 120 degrees about (1, 1, 1) / sqrt 3
NAN_ROW = np.full(POSE, np.nan)


def moving(pose):
    """bool [K]: all 15 entries finite"""
    return np.isfinite(np.asarray(pose, np.float64).reshape(-1, POSE)).all(axis=1)


def cell_valid(valid):
    nx, ny, nz = valid.shape
    v = valid != 0
    return np.all([v[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in CORNERS], axis=0)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def inverse_map(row, X, Y, Z):
    """float64 p[3] of destination coordinates X, Y, Z (float64 arrays) under one pose row; one rounding per operation"""
    R, src, dst = row[:9].reshape(3, 3), row[9:12], row[12:15]
    u0, u1, u2 = X - dst[0], Y - dst[1], Z - dst[2]
    with np.errstate(invalid="ignore", over="ignore"):
        return [((R[0, i] * u0 + R[1, i] * u1) + R[2, i] * u2) + src[i] for i in range(3)]


def locate(p, shape):
    """(inside bool, i int64[3], t float32[3]); i is 0 where not inside"""
    with np.errstate(invalid="ignore"):
        inside = np.ones(np.shape(p[0]), bool)
        for a in range(3):
            inside &= (p[a] >= 0.0) & (p[a] <= float(shape[a] - 1))
    i, t = [], []
    for a in range(3):
        pa = np.where(inside, p[a], 0.0)
        ia = np.minimum(np.floor(pa), float(shape[a] - 2))
        i.append(ia.astype(np.int64))
        t.append((pa - ia).astype(np.float32))
    return inside, i, t


def corner_weights(t):
    one = np.float32(1.0)
    ax, ay, az = (one - t[0], t[0]), (one - t[1], t[1]), (one - t[2], t[2])
    return [(ax[dx] * ay[dy]) * az[dz] for dx, dy, dz in CORNERS]


def chain(w, v):
    """acc = w0*v0, then acc = acc + w_c*v_c: float32 arrays, two roundings per corner"""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = w[0] * v[0]
        for c in range(1, 8):
            acc = acc + w[c] * v[c]
    assert acc.dtype == np.float32
    return acc


def warp_ref(dist, valid, owner, pose):
    """-> dict(source int32, dist float32, valid uint8 (volumes), boxes int32 [K, 12])"""
    shape = dist.shape
    K = len(pose)
    pose = np.asarray(pose, np.float64).reshape(K, POSE)
    mv = moving(pose)
    cv = cell_valid(valid)
    X, Y, Z = [g.astype(np.float64) for g in np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")]
    o = owner.astype(np.int64)
    q_moving = (o >= 1) & (o <= K) & np.concatenate([[False], mv])[np.clip(o, 0, K)]
    bg = (valid != 0) & ~q_moving & ~np.isnan(dist)
    source = np.where(bg, 0, -1).astype(np.int32)
    best = np.where(bg, dist, SENTINEL).astype(np.float32)
    for k in np.flatnonzero(mv):
        inside, i, t = locate(inverse_map(pose[k], X, Y, Z), shape)
        near = [i[a] + (t[a] > np.float32(0.5)) for a in range(3)]
        cand = inside & cv[i[0], i[1], i[2]] & (owner[near[0], near[1], near[2]] == k + 1)
        if not cand.any():
            continue
        d = chain(corner_weights(t), [dist[i[0] + dx, i[1] + dy, i[2] + dz] for dx, dy, dz in CORNERS])
        with np.errstate(invalid="ignore"):
            take = cand & ~np.isnan(d) & ((source < 0) | (d < best))
        source[take] = k + 1
        best[take] = d[take]
    boxes = np.empty((K, 12), np.int32)
    boxes[:, [0, 1, 2, 6, 7, 8]] = INT32_MAX
    boxes[:, [3, 4, 5, 9, 10, 11]] = INT32_MIN
    for at, vol in ((0, owner), (6, source)):
        idx = np.argwhere((vol >= 1) & (vol <= K))
        lab = vol[idx[:, 0], idx[:, 1], idx[:, 2]] - 1
        for a in range(3):
            np.minimum.at(boxes[:, at + a], lab, idx[:, a].astype(np.int32))
            np.maximum.at(boxes[:, at + 3 + a], lab, idx[:, a].astype(np.int32))
    return {"source": source, "dist": np.where(source >= 0, best, SENTINEL).astype(np.float32), "valid": (source >= 0).astype(np.uint8), "boxes": boxes}


def rows_ref(source, pose, data, fill=None, voxels=None, slot=None, cell_band=None):
    """-> (rows float32 [m, C], known uint8 [m]).  data: [nx, ny, nz, C] (dense) or [M, C] behind slot / cell_band (banded; both None with M == 0)"""
    shape = source.shape
    n = source.size
    K = len(pose)
    pose = np.asarray(pose, np.float64).reshape(K, POSE)
    banded = data.ndim == 2
    C = data.shape[-1]
    flat = data.reshape(-1, C)
    fill = np.zeros(C, np.float32) if fill is None else fill
    voxels = np.arange(n) if voxels is None else voxels
    out, known = np.empty((len(voxels), C), np.float32), np.zeros(len(voxels), np.uint8)
    src = source.reshape(-1)
    for j, q in enumerate(voxels):
        out[j] = fill
        s = int(src[q]) if 0 <= q < n else -1
        if s == 0:
            r = int(slot.reshape(-1)[q]) if banded and slot is not None else (-1 if banded else q)
            if r >= 0:
                out[j], known[j] = flat[r], 1
        elif 1 <= s <= K:
            x, y, z = np.unravel_index(q, shape)
            inside, i, t = locate(inverse_map(pose[s - 1], np.float64(x), np.float64(y), np.float64(z)), shape)
            if not inside or (banded and (cell_band is None or not cell_band[i[0], i[1], i[2]])):
                continue
            at = [np.ravel_multi_index((i[0] + dx, i[1] + dy, i[2] + dz), shape) for dx, dy, dz in CORNERS]
            if banded:
                at = [int(slot.reshape(-1)[a]) for a in at]
            w = corner_weights(t)
            out[j], known[j] = chain([np.float32(wc) for wc in w], [flat[a] for a in at]), 1
    return out, known


# ---- the second formulation ---------------------------------------------------------------------------------------------------------
def _image(row, x, y, z, shape):
    """Python floats: (inside, i, t) of one voxel under one pose row"""
    r = [float(v) for v in row]
    u = [float(x) - r[12], float(y) - r[13], float(z) - r[14]]
    p = [((r[0 + a] * u[0] + r[3 + a] * u[1]) + r[6 + a] * u[2]) + r[9 + a] for a in range(3)]
    if not all(0.0 <= p[a] <= shape[a] - 1 for a in range(3)):
        return False, None, None
    i = [min(int(math.floor(p[a])), shape[a] - 2) for a in range(3)]
    return True, i, [np.float32(p[a] - i[a]) for a in range(3)]


def _blend(t, values):
    """np.float32 scalars: the eight weights and the chain over eight values"""
    one = np.float32(1.0)
    acc = None
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(8):
            wx = t[0] if c & 4 else one - t[0]
            wy = t[1] if c & 2 else one - t[1]
            wz = t[2] if c & 1 else one - t[2]
            term = np.float32(np.float32(wx * wy) * wz) * np.float32(values[c])
            acc = term if acc is None else np.float32(acc + term)
    return acc


def warp_loop(dist, valid, owner, pose):
    shape = dist.shape
    nx, ny, nz = shape
    K = len(pose)
    finite = [all(math.isfinite(float(v)) for v in pose[k]) for k in range(K)]
    source, out = np.full(shape, -1, np.int32), np.full(shape, SENTINEL, np.float32)
    boxes = np.tile(np.int32([INT32_MAX] * 3 + [INT32_MIN] * 3), (K, 2))

    def grow(k, at, v):
        for a in range(3):
            boxes[k, at + a] = min(boxes[k, at + a], v[a])
            boxes[k, at + 3 + a] = max(boxes[k, at + 3 + a], v[a])

    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                o = int(owner[x, y, z])
                if 1 <= o <= K:
                    grow(o - 1, 0, (x, y, z))
                best, best_d = -1, None
                if valid[x, y, z] and not (1 <= o <= K and finite[o - 1]) and not math.isnan(dist[x, y, z]):
                    best, best_d = 0, dist[x, y, z]
                for k in range(K):
                    if not finite[k]:
                        continue
                    inside, i, t = _image(pose[k], x, y, z, shape)
                    if not inside:
                        continue
                    if not all(valid[i[0] + dx, i[1] + dy, i[2] + dz] for dx, dy, dz in CORNERS):
                        continue
                    near = [i[a] + (1 if t[a] > np.float32(0.5) else 0) for a in range(3)]
                    if int(owner[near[0], near[1], near[2]]) != k + 1:
                        continue
                    d = _blend(t, [dist[i[0] + dx, i[1] + dy, i[2] + dz] for dx, dy, dz in CORNERS])
                    if math.isnan(d):
                        continue
                    if best < 0 or d < best_d:
                        best, best_d = k + 1, d
                if best >= 0:
                    source[x, y, z], out[x, y, z] = best, best_d
                if best > 0:
                    grow(best - 1, 6, (x, y, z))
    return {"source": source, "dist": out, "valid": (source >= 0).astype(np.uint8), "boxes": boxes}


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _blocks(shape, K, rng):
    """an owner volume of K boxes of 3 to 6 voxels a side (later boxes overwrite earlier ones), 0 elsewhere"""
    owner = np.zeros(shape, np.int32)
    for k in range(K):
        lo = [int(rng.integers(0, max(n - 2, 1))) for n in shape]
        hi = [min(lo[a] + int(rng.integers(3, 7)), shape[a]) for a in range(3)]
        owner[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = k + 1
    return owner


@functools.lru_cache(maxsize=None)
def random_case(shape, seed, K=3, specials=True, motions="mixed"):
    """a seeded volume with K block parts and a pose per part.  specials: 10 % invalid voxels that hold NaN, NaN distances at valid voxels, negative
    zeros, owner values -3 and K + 1, one NaN pose row (K >= 3)"""
    rng = np.random.default_rng(seed)
    dist = rng.normal(size=shape).astype(np.float32)
    valid = np.ones(shape, np.uint8)
    owner = _blocks(shape, K, rng)
    dist[owner > 0] -= np.float32(2.0)              # the parts are solid against the background: where they land they mostly win
    n = dist.size
    if specials:
        valid.reshape(-1)[rng.choice(n, max(1, n // 10), replace=False)] = 0
        dist[valid == 0] = np.nan
        dist.reshape(-1)[rng.choice(n, max(1, n // 25), replace=False)] = np.nan
        dist.reshape(-1)[rng.choice(n, max(1, n // 25), replace=False)] = -0.0
        owner.reshape(-1)[rng.choice(n, max(1, n // 40), replace=False)] = -3
        owner.reshape(-1)[rng.choice(n, max(1, n // 40), replace=False)] = K + 1
    centre = (np.asarray(shape) - 1) / 2.0
    rows = []
    for k in range(K):
        kind = ("shift", "quarter", "half", "small", "third", "identity")[k % 6] if motions == "mixed" else motions
        src = np.argwhere(owner == k + 1).mean(axis=0) if (owner == k + 1).any() else centre
        d = rng.integers(-2, 3, size=3).astype(np.float64)
        if kind == "identity":
            rows.append(pose_row())
        elif kind == "shift":
            rows.append(shift_row(d))
        elif kind == "quarter":
            rows.append(pose_row(QUARTER_Z, np.round(src), np.round(src) + d))
        elif kind == "half":
            rows.append(pose_row(HALF_TILTED, np.round(src), np.round(src) + d))
        elif kind == "third":
            rows.append(pose_row(THIRD_DIAGONAL, np.round(src), np.round(src) + d))
        else:
            rows.append(pose_row(rotation(rng.normal(size=3), math.radians(10.0) * rng.uniform(0.8, 1.2)), src, src + rng.uniform(-1.5, 1.5, size=3)))
    pose = np.array(rows).reshape(K, POSE)
    if specials and K >= 3:
        pose[K - 1] = NAN_ROW
        pose[K - 1, 4] = 1.0            # one finite entry among NaN: still not moving
    return _frozen({"shape": shape, "dist": dist, "valid": valid, "owner": owner, "pose": pose, "K": K})


@functools.lru_cache(maxsize=None)
def planted_case(shape=(9, 10, 17)):
    """Figures known in advance.  Everything valid; the background is free space (dist = +1) and three solid boxes (dist = -1) are parts:
       part 1  [1:4, 1:4, 2:6]   shifted by (3, 2, 5): lands on [4:7, 3:6, 7:11], 36 voxels
       part 2  [5:8, 6:9, 12:15] moved wholly off the grid: wins nothing, its voxels are vacated
       part 3  [1:3, 6:9, 1:3]   a NaN pose: it stays, as background
       part 4  [1:4, 1:4, 2:6]'s duplicate pose (owns nothing): wins nothing
    A part wins exactly where its solid lands (-1 < +1), the vacated voxels have no source."""
    dist = np.ones(shape, np.float32)
    owner = np.zeros(shape, np.int32)
    boxes = {1: ((1, 1, 2), (4, 4, 6)), 2: ((5, 6, 12), (8, 9, 15)), 3: ((1, 6, 1), (3, 9, 3))}
    for k, (lo, hi) in boxes.items():
        owner[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = k
        dist[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = -1.0
    pose = np.array([shift_row((3, 2, 5)), shift_row((40, 0, 0)), NAN_ROW, shift_row((3, 2, 5))])
    won = np.int64([36, 0, 0, 0])
    E = [INT32_MAX] * 3 + [INT32_MIN] * 3
    want = np.int32([[1, 1, 2, 3, 3, 5, 4, 3, 7, 6, 5, 10], [5, 6, 12, 7, 8, 14] + E, [1, 6, 1, 2, 8, 2] + E, E + E])
    return _frozen({"shape": shape, "dist": dist, "valid": np.ones(shape, np.uint8), "owner": owner, "pose": pose, "K": 4, "won": won, "boxes": want,
                    "vacated": 36 + 27})


@functools.lru_cache(maxsize=None)
def collision_case(shape=(9, 10, 17)):
    """Collisions, all by integer shifts on a background of free space at 2.0:
       parts 1, 2  two random solids moved onto one place, [2:5, 4:7, 8:12]: the deeper one wins voxel by voxel
       part 3      its distances equal the background's where it lands, [4:6, 4:6, 7:9]: the background keeps every tie
       parts 4, 5  THE DUPLICATE: part 5's voxels hold a copy of part 4's distances and its pose lands them on the same place,
                   [4:7, 4:7, 9:12]: equal distances everywhere, so part 5 wins nowhere"""
    rng = np.random.default_rng(77)
    dist = np.full(shape, 2.0, np.float32)
    owner = np.zeros(shape, np.int32)
    owner[0:3, 0:3, 0:4], owner[5:8, 0:3, 0:4] = 1, 2
    dist[0:3, 0:3, 0:4] = rng.normal(size=(3, 3, 4)).astype(np.float32)
    dist[5:8, 0:3, 0:4] = rng.normal(size=(3, 3, 4)).astype(np.float32)
    owner[0:2, 7:9, 13:15] = 3
    owner[6:9, 6:9, 0:3], owner[6:9, 0:3, 13:16] = 4, 5
    dist[6:9, 6:9, 0:3] = rng.normal(size=(3, 3, 3)).astype(np.float32) - np.float32(3.0)
    dist[6:9, 0:3, 13:16] = dist[6:9, 6:9, 0:3]
    pose = np.array([shift_row((2, 4, 8)), shift_row((-3, 4, 8)), shift_row((4, -3, -6)), shift_row((-2, -2, 9)), shift_row((-2, 4, -4))])
    return _frozen({"shape": shape, "dist": dist, "valid": np.ones(shape, np.uint8), "owner": owner, "pose": pose, "K": 5,
                    "tie": (slice(4, 6), slice(4, 6), 7), "both": (slice(2, 5), slice(4, 7), 8), "duplicate": (slice(5, 7), slice(5, 7), slice(9, 12))})


@functools.lru_cache(maxsize=None)
def many_parts_case(K, shape):
    """K one-voxel parts, each with its own integer shift (K = 4096 on 17 x 16 x 16: 94 % of the voxels are parts)"""
    rng = np.random.default_rng(4096 + K)
    n = int(np.prod(shape))
    dist = rng.normal(size=shape).astype(np.float32)
    owner = np.zeros(n, np.int32)
    owner[rng.choice(n, K, replace=False)] = rng.permutation(K).astype(np.int32) + 1
    pose = np.array([shift_row(rng.integers(-3, 4, size=3)) for _ in range(K)])
    pose[rng.choice(K, max(K // 16, 1), replace=False)] = NAN_ROW
    pose[K - 1] = pose_row()                       # the last part stays where it is: it wins its own voxel unless a deeper one lands there
    return _frozen({"shape": shape, "dist": dist, "valid": np.ones(shape, np.uint8), "owner": owner.reshape(shape), "pose": pose, "K": K})


def rows_data(shape, C, seed, stride=None):
    """a dense set [nx, ny, nz, C] as a view of a [n, stride] array (stride >= C), finite"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    stride = C if stride is None else stride
    full = rng.normal(size=(n, stride)).astype(np.float32)
    full.setflags(write=False)
    return full, full[:, :C].reshape(shape + (C,))


def voxel_list(n, seed):
    """a shuffled subset with a duplicate"""
    rng = np.random.default_rng(seed)
    v = rng.permutation(n)[:max(n // 3, 2)].astype(np.int32)
    v[-1] = v[0]
    v.setflags(write=False)
    return v


# ---- BakedField.owners ----------------------------------------------------------------------------------------------------------------
def owners_ref(labels, margin_voxels):
    """every voxel within margin_voxels of a part voxel gets the label of its NEAREST part voxel (any nearest one where several tie: the caller
    compares where the nearest label is unique); -> (owner int32, unique bool)"""
    shape = labels.shape
    sites = np.argwhere(labels > 0)
    owner, unique = np.zeros(shape, np.int32), np.ones(shape, bool)
    if len(sites) == 0:
        return owner, unique
    lab = labels[sites[:, 0], sites[:, 1], sites[:, 2]]
    cap = int(math.floor(float(margin_voxels) ** 2))
    for v in np.argwhere(np.ones(shape, bool)):
        d2 = ((sites - v) ** 2).sum(axis=1)
        m = d2.min()
        if m <= cap:
            near = lab[d2 == m]
            owner[tuple(v)] = near[0]
            unique[tuple(v)] = (near == near[0]).all()
    return owner, unique
