"""NumPy restatements and case lists of the pyramid of a baked field and of the seeded flow (d3f_volume_coarsen_select, d3f_volume_coarsen_rows,
d3f_volume_flow_seeded; include/d3fields_hip_pyramid.h), shared by tests/test_pyramid_host.py and
tests/test_gpu_pyramid.py.

The contract, restated:
    grid        fine nx x ny x nz, z fastest, q = (x*ny + y)*nz + z; coarse ceil(n/2) per axis, Q = (X*cy + Y)*cz + Z.  The children of (X, Y, Z)
                are (2X+i, 2Y+j, 2Z+k), i, j, k in {0, 1}, inside the fine volume, numbered c = 4i + 2j + k (ascending fine flat index)
    select      usable = valid != 0 and dist is not NaN (dist of a voxel that is not valid is never read); children = the usable bits;
                count = popcount; valid = count >= min_children; dist = fl(sum * fl(1 / count)), sum one float32 accumulator from +0 over the
                usable children in ascending c; 1e3 where not valid
    rows        child c of a listed Q contributes iff bit c of children[Q] is set, the child lies inside, and the source is dense or
                slot[child] >= 0; n_r contributors: every channel fl(acc * fl(1 / n_r)), acc one float32 accumulator from +0 over the
                contributors in ascending c; n_r == 0: the fill row and known = 0.  An entry outside the coarse volume: fill, known = 0
    seeded flow tests/flow_cases.py's contract with the candidates of member v at u = v + seed[v] + (dx, dy, dz); d2 and j of the key from
                (dx, dy, dz); a member whose seed has a component outside [-SEED_MAX, SEED_MAX] has no candidate; the seed of a non-member
                is never read

coarsen_ref / rows_ref / flow_seeded_ref work on whole arrays, one NumPy ufunc call per rounded operation; coarsen_loop / rows_loop /
flow_seeded_loop are plain Python loops over voxels, children, offsets and channels.  None shares anything with the kernels.
"""
import functools
import itertools

import numpy as np

import flow_cases as FC

POISON = 0xA5
SENTINEL = np.float32(1e3)
SEED_MAX = 16384
INF = np.float32(np.inf)
CHILDREN = [(c >> 2, (c >> 1) & 1, c & 1) for c in range(8)]


def coarse_shape(shape):
    return tuple((n + 1) // 2 for n in shape)


def child_index(shape):
    """(q int64 [cx,cy,cz,8], inside bool [cx,cy,cz,8]): the fine flat index of every child (0 where outside) and whether it lies inside"""
    X, Y, Z = np.indices(coarse_shape(shape))
    q, inside = [], []
    for i, j, k in CHILDREN:
        x, y, z = 2 * X + i, 2 * Y + j, 2 * Z + k
        ok = (x < shape[0]) & (y < shape[1]) & (z < shape[2])
        q.append(np.where(ok, (x * shape[1] + y) * shape[2] + z, 0))
        inside.append(ok)
    return np.stack(q, -1).astype(np.int64), np.stack(inside, -1)


# ---- select -----------------------------------------------------------------------------------------------------------------------
def coarsen_ref(dist, valid, min_children=1):
    """dist float32 [nx,ny,nz] (what lies behind valid == 0 is not looked at), valid -> dict(dist float32, valid uint8, children uint8) [cx,cy,cz]"""
    dist, valid = np.asarray(dist, np.float32), np.asarray(valid) != 0
    q, inside = child_index(dist.shape)
    ok = inside & valid.reshape(-1)[q]
    d = np.where(ok, dist.reshape(-1)[q], np.float32(0)).astype(np.float32)
    usable = ok & ~np.isnan(d)
    children = np.zeros(q.shape[:3], np.uint8)
    total = np.zeros(q.shape[:3], np.float32)
    with np.errstate(all="ignore"):
        for c in range(8):
            children |= (usable[..., c].astype(np.uint8) << np.uint8(c)).astype(np.uint8)
            total = np.where(usable[..., c], total + d[..., c], total)
        count = usable.sum(-1)
        good = count >= min_children
        inv = np.float32(1) / np.maximum(count, 1).astype(np.float32)
        mean = total * inv
    return {"dist": np.where(good, mean, SENTINEL).astype(np.float32), "valid": good.astype(np.uint8), "children": children}


def coarsen_loop(dist, valid, min_children=1):
    dist, valid = np.asarray(dist, np.float32), np.asarray(valid) != 0
    shape, cs = dist.shape, coarse_shape(dist.shape)
    out = {"dist": np.full(cs, SENTINEL, np.float32), "valid": np.zeros(cs, np.uint8), "children": np.zeros(cs, np.uint8)}
    for X, Y, Z in itertools.product(*map(range, cs)):
        total, count, mask = np.float32(0), 0, 0
        for c, (i, j, k) in enumerate(CHILDREN):
            at = (2 * X + i, 2 * Y + j, 2 * Z + k)
            if all(a < n for a, n in zip(at, shape)) and valid[at] and not np.isnan(dist[at]):
                with np.errstate(all="ignore"):
                    total = np.float32(total + dist[at])
                count += 1
                mask |= 1 << c
        out["children"][X, Y, Z] = mask
        if count >= min_children:
            out["valid"][X, Y, Z] = 1
            with np.errstate(all="ignore"):
                out["dist"][X, Y, Z] = np.float32(total * np.float32(np.float32(1) / np.float32(count)))
    return out


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def rows_ref(children, shape, rows, fill=None, voxels=None, slot=None):
    """children uint8 [cx,cy,cz]; shape: the FINE grid; rows: dense [nx,ny,nz,C] or, with slot int32 [nx,ny,nz], the stored rows [M,C];
    float32 or float16 (widened exactly) -> (out float32 [m, C], known uint8 [m])"""
    q, inside = child_index(shape)
    nc = children.size
    C = rows.shape[-1]
    flat = np.asarray(rows).reshape(-1, C)
    listed = np.arange(nc, dtype=np.int64) if voxels is None else np.asarray(voxels, np.int64)
    within = (listed >= 0) & (listed < nc)
    Q = np.where(within, listed, 0)
    mask = np.where(within, children.reshape(-1)[Q].astype(np.int64), 0)
    qc = q.reshape(nc, 8)[Q]
    acc = np.zeros((len(listed), C), np.float32)
    n_r = np.zeros(len(listed), np.int64)
    with np.errstate(all="ignore"):
        for c in range(8):
            has = ((mask >> c) & 1).astype(bool) & inside.reshape(nc, 8)[Q, c]
            row = qc[:, c] if slot is None else np.asarray(slot).reshape(-1)[qc[:, c]].astype(np.int64)
            has &= row >= 0
            if flat.shape[0]:
                v = flat[np.where(has, row, 0)].astype(np.float32)
                acc = np.where(has[:, None], acc + v, acc)
            n_r += has
        inv = np.float32(1) / np.maximum(n_r, 1).astype(np.float32)
        mean = acc * inv[:, None]
    fill_row = np.zeros(C, np.float32) if fill is None else np.asarray(fill, np.float32)
    out = np.where((n_r > 0)[:, None], mean, fill_row[None, :]).astype(np.float32)
    return out, (n_r > 0).astype(np.uint8)


def rows_loop(children, shape, rows, fill=None, voxels=None, slot=None):
    cs = coarse_shape(shape)
    nc = children.size
    C = rows.shape[-1]
    flat = np.asarray(rows).reshape(-1, C)
    listed = range(nc) if voxels is None else [int(v) for v in voxels]
    out = np.zeros((len(listed), C), np.float32)
    known = np.zeros(len(listed), np.uint8)
    fill_row = np.zeros(C, np.float32) if fill is None else np.asarray(fill, np.float32)
    for n, Q in enumerate(listed):
        picked = []
        if 0 <= Q < nc:
            X, Y, Z = np.unravel_index(Q, cs)
            for c, (i, j, k) in enumerate(CHILDREN):
                at = (2 * X + i, 2 * Y + j, 2 * Z + k)
                if not (int(children.reshape(-1)[Q]) >> c) & 1 or not all(a < s for a, s in zip(at, shape)):
                    continue
                row = (at[0] * shape[1] + at[1]) * shape[2] + at[2]
                if slot is not None:
                    row = int(np.asarray(slot).reshape(-1)[row])
                if row >= 0:
                    picked.append(row)
        if not picked:
            out[n] = fill_row
            continue
        known[n] = 1
        inv = np.float32(np.float32(1) / np.float32(len(picked)))
        for ch in range(C):
            acc = np.float32(0)
            with np.errstate(all="ignore"):
                for row in picked:
                    acc = np.float32(acc + np.float32(flat[row, ch]))
                out[n, ch] = np.float32(acc * inv)
    return out, known


def same_rows(got, want):
    """bytes everywhere, NaN-ness where `want` is NaN (a NaN the arithmetic produces has no specified payload)"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and np.where(nan, np.float32(0), got).tobytes() == np.where(nan, np.float32(0), want).tobytes()


# ---- the cases of coarsen ---------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 3, 3), (4, 4, 4), (5, 6, 17), (9, 4, 33), (3, 4, 130)]
CHANNELS = (1, 3, 4, 5, 8, 15, 16, 17, 33, 40)
HALF_CHANNELS = (8, 16, 17, 24, 40)
MIN_CHILDREN = (1, 2, 8)


@functools.lru_cache(maxsize=None)
def coarsen_case(shape, C, seed, half=False):
    """dict, read-only: dist (0xA5 bytes behind valid == 0), valid uint8, rows [shape + (C,)] float32 or float16, fill [C], slot int32 (a band
    that stores a cycling part of the children), banded [M, C] in shuffled slot order, voxels (a list with duplicates and entries outside).
    Coarse voxel Q has Q % 9 valid children (fewer where it has fewer inside); some valid children hold NaN, -0, a subnormal; every seventh
    coarse voxel stores no child at all"""
    rng = np.random.default_rng(seed)
    q, inside = child_index(shape)
    cs, n = coarse_shape(shape), int(np.prod(shape))
    nc = int(np.prod(cs))
    valid = np.zeros(n, np.uint8)
    stored = np.zeros(n, bool)
    for Q in range(nc):
        order = rng.permutation(8)
        for rank, c in enumerate(order):
            if inside.reshape(nc, 8)[Q, c]:
                at = q.reshape(nc, 8)[Q, c]
                valid[at] = 1 if rank < Q % 9 else 0
                stored[at] = (Q + c) % 3 != 0 and Q % 7 != 3
    dist = rng.standard_normal(n).astype(np.float32)
    special = rng.random(n)
    dist[special < 0.08] = np.nan
    dist[(special >= 0.08) & (special < 0.12)] = np.float32(-0.0)
    dist[(special >= 0.12) & (special < 0.16)] = np.float32(1e-41)
    dist.view(np.uint8).reshape(n, 4)[valid == 0] = POISON
    rows = rng.standard_normal((n, C)).astype(np.float32)
    rows[rng.random((n, C)) < 0.03] = np.float32(-0.0)
    rows[rng.random((n, C)) < 0.03] = np.float32(3e-41 if not half else 6e-8)
    if half:
        rows = rows.astype(np.float16)
    idx = np.flatnonzero(stored)
    order = rng.permutation(len(idx))
    slot = np.full(n, -1, np.int32)
    slot[idx[order]] = np.arange(len(idx), dtype=np.int32)
    voxels = np.concatenate([rng.permutation(nc), rng.integers(0, nc, 5), [-1, nc, nc + 7, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)
    out = {"dist": dist.reshape(shape), "valid": valid.reshape(shape), "rows": rows.reshape(shape + (C,)), "fill": rng.standard_normal(C).astype(np.float32),
           "slot": slot.reshape(shape), "banded": np.ascontiguousarray(rows[idx[order]]), "voxels": voxels}
    FC.freeze(*out.values())
    return out


# ---- the seeded flow --------------------------------------------------------------------------------------------------------------
def seed_in_range(seed):
    return (np.abs(np.asarray(seed, np.int64)) <= SEED_MAX).all(-1)


def flow_seeded_ref(member_a, rows_a, member_b, rows_b, seed, r, max_cost2, axis=True):
    """flow_cases.flow_ref with the window of every member of A centred on v + seed[v]; seed int [nx,ny,nz,3] or None (zeros); what lies in
    the seed of a non-member is not looked at"""
    member_a, member_b = np.asarray(member_a, bool), np.asarray(member_b, bool)
    rows_a, rows_b = np.asarray(rows_a, np.float32), np.asarray(rows_b, np.float32)
    shape = member_a.shape
    at = np.argwhere(member_a)
    K = len(at)
    sd = np.zeros((K, 3), np.int64) if seed is None else np.asarray(seed)[member_a].astype(np.int64)
    live = seed_in_range(sd)
    centre = at + np.where(live[:, None], sd, 0)
    a = rows_a[tuple(at.T)]
    has = np.zeros(K, bool)
    bs, bd2, bj, bt = np.full(K, INF, np.float32), np.zeros(K, np.int64), np.zeros(K, np.int64), np.full(K, -1, np.int64)
    for off in FC.offsets(r):
        u = centre + np.array(off)
        inside = live & ((u >= 0) & (u < np.array(shape))).all(1)
        uc = np.where(inside[:, None], u, 0)
        s = FC.chain(a, rows_b[tuple(uc.T)]) if K else np.zeros(0, np.float32)
        part = inside & member_b[tuple(uc.T)] & FC.takes_part(s, max_cost2)
        d2, j = sum(o * o for o in off), FC.j_of(off, r)
        with np.errstate(invalid="ignore"):
            better = part & (~has | (s < bs) | ((s == bs) & ((d2 < bd2) | ((d2 == bd2) & (j < bj)))))
        bs, bd2, bj = np.where(better, s, bs), np.where(better, d2, bd2), np.where(better, j, bj)
        bt = np.where(better, (uc[:, 0] * shape[1] + uc[:, 1]) * shape[2] + uc[:, 2], bt)
        has |= better
    target = np.full(shape, -1, np.int32)
    cost = np.full(shape, INF, np.float32)
    target[member_a] = bt
    cost[member_a] = np.where(has, bs, INF)
    return {"target": target, "cost": cost, "axis_cost": FC.axis_costs(target, member_b, rows_a, rows_b) if axis else None}


def flow_seeded_loop(member_a, rows_a, member_b, rows_b, seed, r, max_cost2):
    """a plain Python loop over voxels, offsets and channels (small volumes only) -> dict(target, cost)"""
    shape = member_a.shape
    target = np.full(shape, -1, np.int32)
    cost = np.full(shape, INF, np.float32)
    for v in itertools.product(*map(range, shape)):
        if not member_a[v]:
            continue
        sd = (0, 0, 0) if seed is None else tuple(int(e) for e in seed[v])
        if any(abs(e) > SEED_MAX for e in sd):
            continue
        best = None
        for off in FC.offsets(r):
            u = tuple(v[k] + sd[k] + off[k] for k in range(3))
            if not all(0 <= u[k] < shape[k] for k in range(3)) or not member_b[u]:
                continue
            s = np.float32(0)
            with np.errstate(all="ignore"):
                for c in range(rows_a.shape[-1]):
                    d = np.float32(rows_a[v][c] - rows_b[u][c])
                    s = np.float32(s + np.float32(d * d))
            if not np.isfinite(s) or not s <= np.float32(max_cost2):
                continue
            key = (float(s), sum(o * o for o in off), FC.j_of(off, r))
            if best is None or key < best[0]:
                best = (key, u, s)
        if best is not None:
            target[v] = (best[1][0] * shape[1] + best[1][1]) * shape[2] + best[1][2]
            cost[v] = best[2]
    return {"target": target, "cost": cost}


def seed_ref(target, cost, axis_cost, fine_shape, refined=True):
    """Flow.seed restated: int32 [fine_shape + (3,)]"""
    matched = target >= 0
    whole = FC.voxel_offsets(target).astype(np.int64)
    if refined and axis_cost is not None:
        with np.errstate(all="ignore"):
            whole = np.where(matched[..., None], np.rint(2.0 * (whole.astype(np.float64) + FC.refine_offsets(cost, axis_cost, matched))), 0.0).astype(np.int64)
    else:
        whole = 2 * whole
    ix, iy, iz = (np.arange(n) >> 1 for n in fine_shape)
    return np.ascontiguousarray(whole[ix[:, None, None], iy[None, :, None], iz[None, None, :]].astype(np.int32))


@functools.lru_cache(maxsize=None)
def random_seed(shape, seed, lo=-6, hi=6):
    s = np.random.default_rng(seed).integers(lo, hi + 1, shape + (3,)).astype(np.int32)
    s.setflags(write=False)
    return s


# ---- the whole chain on a small scene ---------------------------------------------------------------------------------------------------
SCENE_SHAPE, SCENE_C, SCENE_SHIFT = (24, 24, 24), 8, (7, -6, 5)


@functools.lru_cache(maxsize=None)
def scene(shape=SCENE_SHAPE, C=SCENE_C, shift=SCENE_SHIFT, seed=5):
    """a sphere over a static table, before (a) and after the sphere moved by `shift` voxels (b) -> dict, read-only: per side dist (-1 inside
    an object, +1 outside), valid (all ones), rows [shape + (C,)] (zeros outside the objects); sphere bool: the sphere's voxels in a.  The
    rows are a smooth function of the position in the object's own frame plus a little noise that moves with the object, so that a box mean
    of them still tells places apart"""
    rng = np.random.default_rng(seed)
    pos = np.stack(np.indices(shape), -1).astype(np.float64)
    freq = rng.uniform(0.15, 0.6, (C, 3)) * rng.choice([-1.0, 1.0], (C, 3))
    phase = rng.uniform(0, 2 * np.pi, C)

    def describe(local):
        return np.sin(local @ freq.T + phase)

    centre = np.array([8.0, 15.0, 11.0])
    table = pos[..., 2] <= 2
    noise = 0.05 * rng.standard_normal(shape + (C,))
    out = {}
    for side, c in (("a", centre), ("b", centre + np.array(shift))):
        sphere = ((pos - c) ** 2).sum(-1) <= 6.05 ** 2
        moved = np.zeros(shape + (C,))
        if side == "b":
            va, ub = FC.pair_slices(shape, shift)
            moved[ub] = noise[va]
        else:
            moved = noise
        rows = np.where(sphere[..., None], describe(pos - c) + moved, np.where(table[..., None], 0.5 * describe(pos + 40.0) + noise, 0.0))
        occupied = sphere | table
        out["dist_" + side] = np.where(occupied, -1.0, 1.0).astype(np.float32)
        out["valid_" + side] = np.ones(shape, np.uint8)
        out["rows_" + side] = np.where(occupied[..., None], rows, 0.0).astype(np.float32)
        out["sphere_" + side] = sphere
        out["table"] = table
    FC.freeze(*out.values())
    return out


def level_members(dist, valid, slot=None):
    m = (np.asarray(valid) != 0) & (np.asarray(dist) <= 0)
    return m if slot is None else m & (np.asarray(slot) >= 0)


def pyramid_ref(dist, valid, rows, levels, min_children=1):
    """[(dist, valid, rows [shape + (C,)]), ...] finest first, dense"""
    out = [(np.asarray(dist, np.float32), np.asarray(valid), np.asarray(rows, np.float32))]
    for _ in range(levels):
        d, v, r = out[-1]
        sel = coarsen_ref(d, v, min_children)
        coarse, _ = rows_ref(sel["children"], d.shape, r)
        out.append((sel["dist"], sel["valid"], coarse.reshape(sel["dist"].shape + (r.shape[-1],))))
    return out


def chain_ref(levels_a, levels_b, r_top=2, r_fine=1, refine=True, slots_a=None, slots_b=None):
    """the flows of flow_pyramid, coarsest first, from the levels of both pyramids (finest first, rows dense [shape + (C,)]; slots: per level
    None or the slot volume of a banded level, which takes part in the membership only)"""
    n = len(levels_a)
    slots_a, slots_b = slots_a or [None] * n, slots_b or [None] * n
    flows, seed = [], None
    for lv in range(n - 1, -1, -1):
        (da, va, ra), (db, vb, rb) = levels_a[lv], levels_b[lv]
        ma, mb = level_members(da, va, slots_a[lv]), level_members(db, vb, slots_b[lv])
        if seed is None:
            f = FC.flow_ref(ma, ra, mb, rb, r_top, np.inf, axis=refine)
        else:
            f = flow_seeded_ref(ma, ra, mb, rb, seed, r_fine, np.inf, axis=refine)
        flows.append(f)
        if lv > 0:
            seed = seed_ref(f["target"], f["cost"], f["axis_cost"], levels_a[lv - 1][0].shape, refined=refine)
    return flows


@functools.lru_cache(maxsize=None)
def scene_chain(levels=2):
    sc = scene()
    pa = pyramid_ref(sc["dist_a"], sc["valid_a"], sc["rows_a"], levels)
    pb = pyramid_ref(sc["dist_b"], sc["valid_b"], sc["rows_b"], levels)
    return pa, pb, chain_ref(pa, pb)


def on_shift(target, mask, shift):
    """how many voxels of `mask` have their target exactly at voxel + shift"""
    off = FC.voxel_offsets(target)
    return int(((target >= 0) & mask & (off == np.array(shift)).all(-1)).sum())
