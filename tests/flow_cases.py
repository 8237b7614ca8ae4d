"""NumPy restatement and case list of the dense descriptor flow between two baked fields (d3f_volume_flow; include/d3fields_hip.h, the flow
block), shared by tests/test_flow_host.py and tests/test_gpu_flow.py.

The contract, restated:
    grid        two fields A and B on one volume nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z; rows of C floats each, the same C
    member      of A: site_a[v] != 0 and slot_a[v] >= 0 (when given); of B likewise
    candidates  of v: u = v + (dx, dy, dz), |dx|, |dy|, |dz| <= r, r in 1..MAX_RADIUS, u inside the volume (spatially) and a member of B
    cost        s(v, u) = one float32 accumulator from +0, channels ascending: s = fl(s + fl(d*d)), d = fl(a_c - b_c), nothing fused
    takes part  iff s is finite (not NaN, not +Inf) and s <= max_cost2 (a squared radius; +Inf: no threshold)
    winner      the lexicographically smallest (s, d2, j), d2 = dx^2 + dy^2 + dz^2, j = ((dx + r)*(2r + 1) + (dy + r))*(2r + 1) + (dz + r);
                the key packs exactly into 64 bits, bits(s) << 16 | d2 << 10 | j  (s >= +0, d2 <= 48, j < 729)
    outputs     target int32: the winner's flat index or -1; cost float32: its s or +Inf; -1 and +Inf go together (a non-member of A, or a
                member without a candidate that takes part).  Every voxel is written.
    axis_cost   float32 [.., 6]: for a voxel with target t the costs s(v, t -+ e), order x-, x+, y-, y+, z-, z+; +Inf where the neighbour lies
                outside the volume, is no member of B or has a non-finite s; neither the window nor max_cost2 applies; six +Inf without a target

flow_ref walks the offsets, and for each offset the channels one at a time over whole arrays of pairs, so every float32 operation is one NumPy
ufunc call and rounds once; it keeps the best candidate by the plain three-way comparison.  flow_ref_packed keeps the smallest 64-bit key
instead, and flow_loop is a plain Python loop over voxels, offsets and channels.  None shares anything with the kernels.
"""
import functools
import itertools

import numpy as np

MAX_RADIUS = 4                        # D3F_FLOW_MAX_RADIUS
TILE = (4, 4, 16)                     # the workgroup's tile of A voxels (D3F_LINK_TILE_X / _Y / _Z)
POISON = 0xA5
INF = np.float32(np.inf)
AXIS_STEPS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


def offsets(r):
    """the (2r+1)^3 offsets in ascending j"""
    return list(itertools.product(range(-r, r + 1), repeat=3))


def j_of(off, r):
    side = 2 * r + 1
    return ((off[0] + r) * side + (off[1] + r)) * side + (off[2] + r)


def members_of(site, slot=None):
    m = np.asarray(site) != 0
    return m if slot is None else m & (np.asarray(slot) >= 0)


def pair_slices(shape, off):
    """(va, ub): index tuples of the voxels v that have u = v + off inside the volume, and of those u; None when there is none"""
    va, ub = [], []
    for n, d in zip(shape, off):
        if abs(d) >= n:
            return None
        va.append(slice(max(0, -d), n - max(0, d)))
        ub.append(slice(max(0, d), n - max(0, -d)))
    return tuple(va), tuple(ub)


def chain(a, b, dtype=np.float32):
    """s over the last axis: one accumulator from +0, channels ascending, every operation rounded once in `dtype`"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    s = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, dtype)
    with np.errstate(all="ignore"):
        for c in range(a.shape[-1]):
            d = a[..., c] - b[..., c]
            s = s + d * d
    return s


def takes_part(s, max_cost2):
    with np.errstate(invalid="ignore"):
        return np.isfinite(s) & (s <= np.float32(max_cost2))


def pack_key(s, d2, j):
    """uint64: bits(s) << 16 | d2 << 10 | j for s >= +0 finite"""
    bits = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(16)) | np.uint64(d2 << 10) | np.uint64(j)


def axis_costs(target, member_b, rows_a, rows_b):
    """float32 [nx, ny, nz, 6] of the contract, from the targets"""
    shape = target.shape
    out = np.full(shape + (6,), INF, np.float32)
    at = np.argwhere(target >= 0)
    if len(at) == 0:
        return out
    t = np.stack(np.unravel_index(target[target >= 0].astype(np.int64), shape), axis=1)
    a = rows_a[tuple(at.T)]
    for k, e in enumerate(AXIS_STEPS):
        u = t + np.array(e)
        inside = ((u >= 0) & (u < np.array(shape))).all(1)
        uc = np.where(inside[:, None], u, 0)
        s = chain(a, rows_b[tuple(uc.T)])
        ok = inside & member_b[tuple(uc.T)] & np.isfinite(s)
        out[tuple(at.T) + (k,)] = np.where(ok, s, INF)
    return out


def flow_ref(member_a, rows_a, member_b, rows_b, r, max_cost2, axis=True):
    """member bool [nx,ny,nz], rows float32 [nx,ny,nz,C] (only members' rows matter) -> dict(target int32, cost float32, axis_cost or None);
    the three-way comparison of (s, d2, j)"""
    member_a, member_b = np.asarray(member_a, bool), np.asarray(member_b, bool)
    rows_a, rows_b = np.asarray(rows_a, np.float32), np.asarray(rows_b, np.float32)
    shape = member_a.shape
    flat = np.arange(member_a.size, dtype=np.int64).reshape(shape)
    has = np.zeros(shape, bool)
    bs = np.full(shape, INF, np.float32)
    bd2 = np.zeros(shape, np.int64)
    bj = np.zeros(shape, np.int64)
    bt = np.full(shape, -1, np.int64)
    for off in offsets(r):
        sl = pair_slices(shape, off)
        if sl is None:
            continue
        va, ub = sl
        s = chain(rows_a[va], rows_b[ub])
        part = member_a[va] & member_b[ub] & takes_part(s, max_cost2)
        d2, j = sum(o * o for o in off), j_of(off, r)
        cs, cd2, cj = bs[va], bd2[va], bj[va]
        with np.errstate(invalid="ignore"):
            better = part & (~has[va] | (s < cs) | ((s == cs) & ((d2 < cd2) | ((d2 == cd2) & (j < cj)))))
        bs[va] = np.where(better, s, cs)
        bd2[va] = np.where(better, d2, cd2)
        bj[va] = np.where(better, j, cj)
        bt[va] = np.where(better, flat[ub], bt[va])
        has[va] |= better
    target = bt.astype(np.int32)
    cost = np.where(has, bs, INF).astype(np.float32)
    return {"target": target, "cost": cost, "axis_cost": axis_costs(target, member_b, rows_a, rows_b) if axis else None}


def flow_ref_packed(member_a, rows_a, member_b, rows_b, r, max_cost2):
    """flow_ref's target and cost by the smallest packed 64-bit key"""
    member_a, member_b = np.asarray(member_a, bool), np.asarray(member_b, bool)
    rows_a, rows_b = np.asarray(rows_a, np.float32), np.asarray(rows_b, np.float32)
    shape = member_a.shape
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(shape, none, np.uint64)
    for off in offsets(r):
        sl = pair_slices(shape, off)
        if sl is None:
            continue
        va, ub = sl
        s = chain(rows_a[va], rows_b[ub])
        part = member_a[va] & member_b[ub] & takes_part(s, max_cost2)
        key = np.where(part, pack_key(np.where(part, s, 0), sum(o * o for o in off), j_of(off, r)), none)
        best[va] = np.minimum(best[va], key)
    found = best != none
    side = 2 * r + 1
    j = (best & np.uint64(1023)).astype(np.int64)
    o = np.stack((j // (side * side) - r, (j // side) % side - r, j % side - r), axis=-1)
    at = np.stack(np.indices(shape), axis=-1) + o
    target = np.where(found, (at[..., 0] * shape[1] + at[..., 1]) * shape[2] + at[..., 2], -1).astype(np.int32)
    cost = np.where(found, (best >> np.uint64(16)).astype(np.uint32).view(np.float32), INF).astype(np.float32)
    return {"target": target, "cost": cost}


def flow_loop(member_a, rows_a, member_b, rows_b, r, max_cost2, axis=True):
    """flow_ref as a plain Python loop over voxels, offsets and channels in NumPy float32 scalars (small volumes only)"""
    shape = member_a.shape
    nx, ny, nz = shape
    target = np.full(shape, -1, np.int32)
    cost = np.full(shape, INF, np.float32)
    axis_cost = np.full(shape + (6,), INF, np.float32) if axis else None

    def s_of(a, b):
        s = np.float32(0)
        with np.errstate(all="ignore"):
            for c in range(len(a)):
                d = np.float32(a[c] - b[c])
                s = np.float32(s + np.float32(d * d))
        return s

    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):
        if not member_a[x, y, z]:
            continue
        best = None
        for off in offsets(r):
            u = (x + off[0], y + off[1], z + off[2])
            if not all(0 <= u[k] < shape[k] for k in range(3)) or not member_b[u]:
                continue
            s = s_of(rows_a[x, y, z], rows_b[u])
            if not np.isfinite(s) or not s <= np.float32(max_cost2):
                continue
            key = (float(s), sum(o * o for o in off), j_of(off, r))
            if best is None or key < best[0]:
                best = (key, u, s)
        if best is None:
            continue
        (tx, ty, tz), cost[x, y, z] = best[1], best[2]
        target[x, y, z] = (tx * ny + ty) * nz + tz
        if axis:
            for k, e in enumerate(AXIS_STEPS):
                u = (tx + e[0], ty + e[1], tz + e[2])
                if all(0 <= u[q] < shape[q] for q in range(3)) and member_b[u]:
                    s = s_of(rows_a[x, y, z], rows_b[u])
                    if np.isfinite(s):
                        axis_cost[x, y, z, k] = s
    return {"target": target, "cost": cost, "axis_cost": axis_cost}


def refine_offsets(cost, axis_cost, matched):
    """float64 [.., 3]: per axis 0.5 (f- - f+) / (f- - 2 f0 + f+) clamped to [-0.5, 0.5]; 0 where a side is +Inf or the denominator is not > 0;
    NaN where unmatched (the formula of BakedField.peaks' refinement)"""
    f0 = cost.astype(np.float64)
    out = np.zeros(cost.shape + (3,), np.float64)
    with np.errstate(all="ignore"):
        for a in range(3):
            fm, fp = axis_cost[..., 2 * a].astype(np.float64), axis_cost[..., 2 * a + 1].astype(np.float64)
            den = fm - 2.0 * f0 + fp
            off = np.clip(0.5 * (fm - fp) / den, -0.5, 0.5)
            out[..., a] = np.where(np.isfinite(fm) & np.isfinite(fp) & (den > 0), off, 0.0)
    out[~matched] = np.nan
    return out


def voxel_offsets(target):
    """int32 [.., 3]: the target's coordinates minus the voxel's, 0 where unmatched"""
    shape = target.shape
    to = np.stack(np.unravel_index(np.maximum(target, 0).astype(np.int64), shape), axis=-1)
    return np.where((target >= 0)[..., None], to - np.stack(np.indices(shape), axis=-1), 0).astype(np.int32)


def consistent_ref(forward, back, tol):
    """bool: matched, back has a target at the target, and that voxel lies within Chebyshev distance tol of the voxel"""
    shape = forward.shape
    ret = back.reshape(-1)[np.maximum(forward, 0)]
    where = np.stack(np.unravel_index(np.maximum(ret, 0).astype(np.int64), shape), axis=-1)
    near = np.abs(where - np.stack(np.indices(shape), axis=-1)).max(-1) <= tol
    return (forward >= 0) & (ret >= 0) & near


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def random_case(shape, C, seed, density=0.9, kind="gauss"):
    """(member_a, rows_a, member_b, rows_b), read-only.  B is A moved by one voxel along z plus noise, so that winners mean something and
    are spread over the window.  kind "gauss": Gaussian rows, inexact sums -- a different order of summation shows in the cost's bits;
    kind "int": rows in {0, 1, 2}, exact sums with MANY ties in s, which the d2 and j parts of the key decide"""
    rng = np.random.default_rng(seed)
    member_a = rng.random(shape) < density
    member_b = rng.random(shape) < density
    if kind == "gauss":
        rows_a = rng.standard_normal(shape + (C,)).astype(np.float32)
        rows_b = (np.roll(rows_a, 1, axis=2) + 0.5 * rng.standard_normal(shape + (C,))).astype(np.float32)
    else:
        rows_a = rng.integers(0, 3, shape + (C,)).astype(np.float32)
        rows_b = rng.integers(0, 3, shape + (C,)).astype(np.float32)
    return freeze(member_a, rows_a, member_b, rows_b)


@functools.lru_cache(maxsize=None)
def random_reference(shape, C, seed, density, kind, r, max_cost2=float("inf")):
    ref = flow_ref(*random_case(shape, C, seed, density, kind), r, max_cost2)
    freeze(*ref.values())
    return ref


SMALL = [((3, 4, 5), 7, 1, 0.8, "gauss"), ((3, 4, 5), 2, 2, 0.8, "int"), ((2, 2, 6), 1, 3, 0.6, "int"), ((1, 3, 4), 3, 4, 1.0, "gauss")]
CHANNELS = (1, 3, 4, 5, 15, 16, 17, 33, 40)
CHANNEL_SHAPE = (5, 6, 18)
TILE_SHAPES = [(1, 1, 1), (2, 2, 2), (3, 5, 15), (4, 4, 16), (5, 5, 17), (9, 4, 33), (4, 9, 1)]
SHIFT = (1, -2, 1)


@functools.lru_cache(maxsize=None)
def shifted_copy(shape=(6, 7, 9), C=6, seed=21, density=0.85, shift=SHIFT):
    """(member_a, rows_a, member_b, rows_b, moved): B holds at u = v + shift what A holds at v (rows and membership), and has no member where
    u - shift lies outside the volume.  rows i.i.d. Gaussian, so that cost 0 names the copy alone.  moved: the members of A whose copy v +
    shift lies inside the volume"""
    rng = np.random.default_rng(seed)
    member_a = rng.random(shape) < density
    rows_a = rng.standard_normal(shape + (C,)).astype(np.float32)
    member_b = np.zeros(shape, bool)
    rows_b = np.full(shape + (C,), np.nan, np.float32)
    va, ub = pair_slices(shape, shift)
    member_b[ub], rows_b[ub] = member_a[va], rows_a[va]
    moved = np.zeros(shape, bool)
    moved[va] = member_a[va]
    return freeze(member_a, rows_a, member_b, rows_b, moved)


def identical_b(shape=(5, 5, 7), C=3):
    """every row of A and of B is the same row, every voxel a member of both except that B lacks v itself for the voxels of `hole`: every
    candidate ties in s = 0, so d2 and then j decide"""
    member_a = np.ones(shape, bool)
    member_b = np.ones(shape, bool)
    hole = np.zeros(shape, bool)
    hole[2, 2, 3] = hole[0, 0, 0] = hole[4, 4, 6] = True
    member_b[hole] = False
    rows = np.full(shape + (C,), 1.5, np.float32)
    return member_a, rows, member_b, rows.copy(), hole


def planted(shape, r, C, where, cost_levels=(0.0,)):
    """one member of A at the centre voxel, all of B members with rows far away, except the offsets in `where`, whose rows differ from A's
    row by sqrt(level) in channel 0 -> (member_a, rows_a, member_b, rows_b, centre)"""
    centre = tuple(n // 2 for n in shape)
    member_a = np.zeros(shape, bool)
    member_a[centre] = True
    rows_a = np.zeros(shape + (C,), np.float32)
    rows_a[centre] = np.arange(1, C + 1, dtype=np.float32)
    rows_b = np.full(shape + (C,), 100.0, np.float32)
    for off, level in zip(where, itertools.cycle(cost_levels)):
        u = tuple(c + o for c, o in zip(centre, off))
        rows_b[u] = rows_a[centre]
        rows_b[u][0] += np.float32(np.sqrt(level))
    return member_a, rows_a, np.ones(shape, bool), rows_b, centre


def window_marks(r):
    """the corners, the face centres and the centre of the window of radius r"""
    return list(itertools.product((-r, r), repeat=3)) + [tuple(s * r if a == k else 0 for a in range(3)) for k in range(3) for s in (-1, 1)] + [(0, 0, 0)]


def band_of(member, rows, seed, keep=0.7):
    """a slot volume that stores a random part of the voxels in shuffled row order -> (slot int32 [shape], compacted rows [M, C])"""
    rng = np.random.default_rng(seed)
    stored = rng.random(member.shape) < keep
    idx = np.flatnonzero(stored.reshape(-1))
    order = rng.permutation(len(idx))
    slot = np.full(member.size, -1, np.int32)
    slot[idx[order]] = np.arange(len(idx), dtype=np.int32)
    flat = np.asarray(rows, np.float32).reshape(member.size, -1)
    return slot.reshape(member.shape), np.ascontiguousarray(flat[idx[order]])
