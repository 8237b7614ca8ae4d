"""NumPy restatement and case list of descriptor-gated links and of the components over a link volume (d3f_volume_links,
d3f_volume_components_linked; include/d3fields_hip.h, the links block), shared by tests/test_parts_host.py and
tests/test_gpu_parts.py.

The contract, restated:
    member      site[v] != 0, valid[v] != 0 (when given), slot[v] >= 0 (when given)
    offsets     (dx, dy, dz) over {-1,0,1}^3 in lexicographic order, the 13 before (0,0,0): j = 9*(dx+1) + 3*(dy+1) + (dz+1)
    links[v]    uint16; bit j iff v and u = v + offset j are members, u lies inside the volume (spatially), |dx|+|dy|+|dz| <= 1 / 2 / 3 for
                connectivity 6 / 18 / 26 and the rule accepts the rows a (of v) and b (of u); bits 13..15 are 0
    L2          s <= threshold;  s = fl(s + fl(d*d)), d = fl(a_c - b_c), c ascending from s = +0, all float32
    COSINE      na > 0 and nb > 0 and dot >= 0 and f64(dot)*f64(dot) >= (f64(t)*f64(t)) * (f64(na)*f64(nb)); the three sums as above
    ARGMAX      best(a) == best(b), best = 0; for c in 1..C-1: if row[c] > row[best]: best = c
    linked components   two sites are united iff the higher one's bit is set, the connectivity allows the offset and the neighbour is a
                site inside the volume; numbering, found, stats as d3f_volume_components (tests/ccl_cases.py)

links_ref walks the channels one at a time over whole arrays of pairs, so every float32 operation is one NumPy ufunc call and rounds once.
components_linked_ref turns the link volume into an explicit edge list and labels that by minimum-label propagation and pointer jumping; it
shares nothing with the kernels.
"""
import functools
import itertools

import numpy as np

L2, COSINE, ARGMAX = 0, 1, 2
RULES = {"l2": L2, "cosine": COSINE, "argmax": ARGMAX}
OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))[:13]
CONN_MASK = {6: 0x1410, 18: 0x1EBA, 26: 0x1FFF}
CONNECTIVITIES = (6, 18, 26)
TILE = (4, 4, 16)                     # D3F_LINK_TILE_X / _Y / _Z
POISON16 = 0xA5A5


def allowed(j, connectivity):
    return sum(abs(c) for c in OFFSETS[j]) <= {6: 1, 18: 2, 26: 3}[connectivity]


def members_of(site, valid=None, slot=None):
    m = np.asarray(site) != 0
    if valid is not None:
        m = m & (np.asarray(valid) != 0)
    if slot is not None:
        m = m & (np.asarray(slot) >= 0)
    return m


def pair_slices(shape, off):
    """(hi, lo): index tuples of the voxels v that have u = v + off inside the volume, and of those u"""
    hi, lo = [], []
    for n, d in zip(shape, off):
        hi.append(slice(1, n) if d < 0 else slice(0, n - 1) if d > 0 else slice(None))
        lo.append(slice(0, n - 1) if d < 0 else slice(1, n) if d > 0 else slice(None))
    return tuple(hi), tuple(lo)


def pair_sums(rows, off, dtype=np.float32):
    """{s, dot, na, nb} of every pair (v, v + off), arrays over the hi region; one accumulator each, channels ascending, in `dtype`"""
    hi, lo = pair_slices(rows.shape[:3], off)
    a, b = rows[hi].astype(dtype), rows[lo].astype(dtype)
    out = {k: np.zeros(a.shape[:3], dtype) for k in ("s", "dot", "na", "nb")}
    with np.errstate(all="ignore"):
        for c in range(rows.shape[3]):
            ac, bc = a[..., c], b[..., c]
            d = ac - bc
            out["s"] = out["s"] + d * d
            out["dot"] = out["dot"] + ac * bc
            out["na"] = out["na"] + ac * ac
            out["nb"] = out["nb"] + bc * bc
    return out


def first_max(rows):
    """int [..]: the vote rule of d3f_volume_pool along the last axis"""
    best = np.zeros(rows.shape[:-1], np.int64)
    top = rows[..., 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, rows.shape[-1]):
            better = rows[..., c] > top
            top = np.where(better, rows[..., c], top)
            best = np.where(better, c, best)
    return best


def verdict(sums, rule, threshold):
    t = np.float32(threshold)
    with np.errstate(all="ignore"):
        if rule == L2:
            return sums["s"] <= t
        dot, na, nb = (sums[k].astype(np.float64) for k in ("dot", "na", "nb"))
        tt = np.float64(t) * np.float64(t)
        return (sums["na"] > 0) & (sums["nb"] > 0) & (sums["dot"] >= 0) & (dot * dot >= tt * (na * nb))


def links_ref(member, rows, rule, threshold, connectivity):
    """member bool [nx,ny,nz], rows float32 [nx,ny,nz,C] (only members' rows matter) -> uint16 [nx,ny,nz]"""
    member = np.asarray(member, bool)
    rows = np.asarray(rows, np.float32)
    out = np.zeros(member.shape, np.uint16)
    best = first_max(rows) if rule == ARGMAX else None
    for j, off in enumerate(OFFSETS):
        if not allowed(j, connectivity) or any(n < 2 and d for n, d in zip(member.shape, off)):
            continue
        hi, lo = pair_slices(member.shape, off)
        ok = best[hi] == best[lo] if rule == ARGMAX else verdict(pair_sums(rows, off), rule, threshold)
        out[hi] |= ((ok & member[hi] & member[lo]).astype(np.uint16) << np.uint16(j))
    return out


def links_loop(member, rows, rule, threshold, connectivity):
    """links_ref as a plain Python loop over voxels, offsets and channels in NumPy float32 scalars (small volumes only)"""
    nx, ny, nz = member.shape
    out = np.zeros(member.shape, np.uint16)
    t = np.float32(threshold)
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):
        if not member[x, y, z]:
            continue
        for j, (dx, dy, dz) in enumerate(OFFSETS):
            u = (x + dx, y + dy, z + dz)
            if not allowed(j, connectivity) or not all(0 <= u[k] < member.shape[k] for k in range(3)) or not member[u]:
                continue
            a, b = rows[x, y, z], rows[u]
            with np.errstate(all="ignore"):
                if rule == ARGMAX:
                    best = []
                    for r in (a, b):
                        k = 0
                        for c in range(1, len(r)):
                            if r[c] > r[k]:
                                k = c
                        best.append(k)
                    ok = best[0] == best[1]
                else:
                    s = dot = na = nb = np.float32(0)
                    for c in range(len(a)):
                        d = np.float32(a[c] - b[c])
                        s = np.float32(s + np.float32(d * d))
                        dot = np.float32(dot + np.float32(a[c] * b[c]))
                        na = np.float32(na + np.float32(a[c] * a[c]))
                        nb = np.float32(nb + np.float32(b[c] * b[c]))
                    if rule == L2:
                        ok = s <= t
                    else:
                        ok = na > 0 and nb > 0 and dot >= 0 and float(dot) * float(dot) >= (float(t) * float(t)) * (float(na) * float(nb))
            if ok:
                out[x, y, z] |= np.uint16(1 << j)
    return out


# ---- components over a link volume ---------------------------------------------------------------------------------------------------
def edges_of_links(site, links, connectivity):
    """int64 [E, 2]: (v, u) flat indices of every pair the link volume unites -- bit set, offset allowed, u inside the volume, both sites"""
    site = np.asarray(site) != 0
    links = np.asarray(links).view(np.uint16) if np.asarray(links).dtype == np.int16 else np.asarray(links, np.uint16)
    flat = np.arange(site.size, dtype=np.int64).reshape(site.shape)
    edges = [np.zeros((0, 2), np.int64)]
    for j, off in enumerate(OFFSETS):
        if not allowed(j, connectivity) or any(n < 2 and d for n, d in zip(site.shape, off)):
            continue
        hi, lo = pair_slices(site.shape, off)
        on = ((links[hi] >> np.uint16(j)) & 1).astype(bool) & site[hi] & site[lo]
        edges.append(np.stack([flat[hi][on], flat[lo][on]], axis=1))
    return np.concatenate(edges)


def components_of_edges(site, edges, min_voxels=1):
    """the classes of the sites under the edge list -> the dict of ccl_cases.components_ref (label, K, found, stats, sizes_all)"""
    site = np.asarray(site) != 0
    n = site.size
    lab = np.where(site.reshape(-1), np.arange(n, dtype=np.int64), n)
    v, u = edges[:, 0], edges[:, 1]
    while True:
        low = lab.copy()
        np.minimum.at(low, v, lab[u])
        np.minimum.at(low, u, lab[v])
        par = np.arange(n + 1, dtype=np.int64)
        np.minimum.at(par, lab, low)
        while True:
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt
        new = par[lab]
        if np.array_equal(new, lab):
            break
        lab = new
    roots_all = np.unique(lab[lab < n])
    sizes_all = np.bincount(lab[lab < n], minlength=n)[roots_all] if len(roots_all) else np.zeros(0, np.int64)
    keep = sizes_all >= min_voxels
    kept = roots_all[keep]
    number = np.zeros(n + 1, np.int32)
    number[kept] = np.arange(1, len(kept) + 1, dtype=np.int32)
    label = number[lab].reshape(site.shape)
    at = np.argwhere(label > 0)
    k = label[label > 0] - 1
    lo = np.full((len(kept), 3), max(site.shape), np.int64)
    hi = np.full((len(kept), 3), -1, np.int64)
    np.minimum.at(lo, k, at)
    np.maximum.at(hi, k, at)
    stats = np.concatenate([kept[:, None], sizes_all[keep][:, None], lo, hi], axis=1).astype(np.int32)
    return {"label": label, "K": len(kept), "found": len(roots_all), "stats": stats, "sizes_all": sizes_all.astype(np.int64)}


def components_linked_ref(site, links, connectivity, min_voxels=1):
    return components_of_edges(site, edges_of_links(site, links, connectivity), min_voxels)


def flood_fill_edges(site, edges):
    """labels by ascending root from a pure-Python flood fill over the edge list"""
    site = np.asarray(site) != 0
    adj = {}
    for v, u in edges.tolist():
        adj.setdefault(v, []).append(u)
        adj.setdefault(u, []).append(v)
    label = np.zeros(site.size, np.int32)
    k = 0
    for start in np.nonzero(site.reshape(-1))[0].tolist():
        if label[start]:
            continue
        k += 1
        label[start] = k
        stack = [start]
        while stack:
            for q in adj.get(stack.pop(), ()):
                if not label[q]:
                    label[q] = k
                    stack.append(q)
    return label.reshape(site.shape)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def blocky_rows(shape, C, seed, exact=True):
    """rows of three classes laid out in blocks of 2 x 2 x 3 voxels.  exact: prototypes -6 / 0 / +6 plus noise in {0, 1}: integers of
    magnitude <= 8 (with a dot product below 2^24 every float32 sum is exact); else unit-variance prototypes plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    x, y, z = np.indices(shape)
    cls = rng.integers(0, 3, (shape[0] // 2 + 1, shape[1] // 2 + 1, shape[2] // 3 + 1))[x // 2, y // 2, z // 3]
    if exact:
        rows = (np.array([-6, 0, 6])[cls][..., None] + rng.integers(0, 2, shape + (C,))).astype(np.float32)
        assert np.abs(rows).max() <= 8
    else:
        rows = (rng.standard_normal((3, C))[cls] + 0.35 * rng.standard_normal(shape + (C,))).astype(np.float32)
    return rows


def random_case(shape, C, seed, density=0.9):
    """(site uint8, rows float32 [shape, C], L2 threshold, cosine threshold).  Two rows of one class differ by 0 or 1 per channel, so their s
    is binomial over 0..C and the threshold (C + 1) // 2 lies inside that spread: links fail at random inside a class as well as between
    classes (where s >= 25 C), and many pairs sit exactly on the threshold"""
    rng = np.random.default_rng(seed + 1000)
    site = (rng.random(shape) < density) * rng.integers(1, 256, shape)
    return site.astype(np.uint8), blocky_rows(shape, C, seed), float((C + 1) // 2), 0.9


# name -> (shape, C).  nz in {1, 3, 63, 64, 65, 130} at 3 x 5: lines that share a wave, span waves, and a link across a wave boundary.
LINES = {"3x5x%d" % nz: ((3, 5, nz), 5) for nz in (1, 3, 63, 64, 65, 130)}
# extents T-1, T, T+1, 2T+1 of the link kernel's tile on each axis
TILES = {"%dx%dx%d" % s: (s, 4) for s in [(x, 5, 17) for x in (3, 4, 5, 9)] + [(5, y, 17) for y in (3, 4, 5, 9)] + [(5, 5, z) for z in (15, 16, 17, 33)]}
RANDOM = dict(LINES, **TILES)
CHANNELS = (1, 3, 4, 5, 16, 17, 31, 64, 100, 384)
CHANNEL_SHAPE = (5, 6, 18)


@functools.lru_cache(maxsize=None)
def random_volume(name):
    shape, C = RANDOM[name]
    case = random_case(shape, C, 7000 + sorted(RANDOM).index(name))
    for a in case[:2]:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def random_reference(name, rule, connectivity):
    """(links, components) of a random case under the rule, computed once and shared (read-only)"""
    site, rows, t2, tc = random_volume(name)
    links = links_ref(site != 0, rows, rule, 0.0 if rule == ARGMAX else t2 if rule == L2 else tc, connectivity)
    comp = components_linked_ref(site, links, connectivity)
    for a in [links] + [v for v in comp.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return links, comp


STRADDLE_SHAPE = (9, 9, 33)
# (offset, higher voxel): from the first voxel of tile (1, 1, 1) every offset leaves the tile through a face, an edge or a corner; the offsets with
# dy = +1 also from the voxel of that tile whose y + 1 lies in the next one
STRADDLES = [(j, (4, 4, 16)) for j in range(13)] + [(j, (4, 7, 16)) for j in (6, 7, 8)]


def straddle(j, hi):
    """exactly two members with equal rows, hi and hi + offset j -> (site, rows)"""
    site = np.zeros(STRADDLE_SHAPE, np.uint8)
    site[hi] = 1
    site[tuple(h + d for h, d in zip(hi, OFFSETS[j]))] = 1
    return site, np.ones(STRADDLE_SHAPE + (4,), np.float32)


SERPENTINE_SHAPE = (8, 8, 70)


@functools.lru_cache(maxsize=None)
def serpentine():
    """(rows [8,8,70,1], links uint16): one channel that holds the position along a path through EVERY voxel -- up one z line, over to the next
    line at its end, down that one; lines in boustrophedon order over (x, y) -- so that under L2 with tau = 1 and connectivity 6 exactly the
    consecutive voxels of the path link; and that link volume, built by hand"""
    nx, ny, nz = SERPENTINE_SHAPE
    pos = np.zeros(SERPENTINE_SHAPE, np.float32)
    links = np.zeros(SERPENTINE_SHAPE, np.uint16)
    links[:, :, 1:] = 1 << 12
    lines = [(x, y) for x in range(nx) for y in (range(ny) if x % 2 == 0 else range(ny - 1, -1, -1))]
    for i, (x, y) in enumerate(lines):
        zs = np.arange(nz) if i % 2 == 0 else np.arange(nz - 1, -1, -1)
        pos[x, y, zs] = i * nz + np.arange(nz)
        if i > 0:
            px, py = lines[i - 1]
            turn = nz - 1 if i % 2 == 1 else 0
            hi = max((x, y), (px, py))
            links[hi[0], hi[1], turn] |= (1 << 4) if px != x else (1 << 10)
    pos.setflags(write=False)
    links.setflags(write=False)
    return pos[..., None], links


SERPENTINE_CUT = (3, 4, 35)               # clearing bit 12 here cuts the path inside a line


def touching_boxes(seed=11):
    """a scene of two boxes that touch at the plane between x = 11 and x = 12, with different descriptors and instance-mask rows, plus seeded
    noise -> dict(shape, dist, feat [.., 16], mask [.., 3], inside_a, inside_b)"""
    shape = (24, 20, 16)
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, bool)
    b = np.zeros(shape, bool)
    a[4:12, 5:15, 3:11] = True
    b[12:20, 5:15, 3:11] = True
    core = np.zeros(shape, bool)                    # deeper than two voxels inside: beyond a band of two steps, so a banded field stores no row there
    core[6:18, 7:13, 5:9] = True
    near = np.zeros(shape, bool)
    near[2:22, 3:17, 1:13] = True
    dist = np.where(core, -1.0, np.where(a | b, -0.005, np.where(near, 0.005, 1.0))).astype(np.float32)
    proto = np.zeros((3, 16), np.float32)
    proto[1, :8] = 1.0
    proto[2, 8:] = 1.0
    which = np.where(a, 1, np.where(b, 2, 0))
    feat = (proto[which] + 0.02 * rng.standard_normal(shape + (16,))).astype(np.float32)
    mask = (np.eye(3, dtype=np.float32)[which] + 0.05 * rng.random(shape + (3,))).astype(np.float32)
    return {"shape": shape, "dist": dist, "feat": feat, "mask": mask, "inside_a": a, "inside_b": b}


TOUCHING_TAU = 0.5                        # |proto_a - proto_b| = 4; the noise moves a pair of one box by about 0.02 * sqrt(32) = 0.11
