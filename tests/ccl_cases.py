"""NumPy restatement and case list of connected-component labelling (d3f_volume_components, include/d3fields_hip.h ABI 15; DESIGN.md
section 17), shared by tests/test_components_host.py and tests/test_gpu_components.py.

The contract, restated:
    site        uint8 [nx, ny, nz], z fastest; any non-zero byte is a site
    neighbours  two sites whose integer coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1 for connectivity
                6 / 18 / 26.  Spatial: (x, y, nz-1) and (x, y+1, 0) are adjacent in memory and are not neighbours, nor are (x, ny-1, z)
                and (x+1, 0, z)
    component   a class of the transitive closure; root = its smallest flat index, size = its voxel count, box = inclusive min / max of
                x, y, z
    found       the number of components; the kept ones (size >= min_voxels) are numbered 1..K in ascending order of root
    label[v]    the number of v's component, 0 for a non-site or a dropped component
    stats[k-1]  {root, size, x0, y0, z0, x1, y1, z1}

components_ref shares nothing with the kernels: the minimum label over the neighbourhood from padded shifted copies (nothing wraps), the
minimum hooked onto each label, pointer jumping par = par[par], repeated until nothing changes.  test_components_host.py checks it
against a pure-Python flood fill and, where scipy imports, against scipy.ndimage.label.
"""
import functools
import itertools

import numpy as np

CONNECTIVITIES = (6, 18, 26)
POISON = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]      # four 0xA5 bytes as int32


def offsets(connectivity):
    """the neighbour offsets (dx, dy, dz) of a connectivity, without (0, 0, 0)"""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(c) for c in o) <= reach]


def components_ref(site, connectivity, min_voxels=1):
    """-> dict(label int32 [nx,ny,nz], K, found, stats int32 [K, 8], sizes_all int64 [found] (every component, ascending root))"""
    site = np.asarray(site) != 0
    assert site.ndim == 3 and min_voxels >= 1
    nx, ny, nz = site.shape
    n = site.size
    offs = offsets(connectivity)
    lab = np.where(site, np.arange(n, dtype=np.int64).reshape(site.shape), n).reshape(-1)      # n: "no label", above every flat index
    rounds = 0
    while True:
        rounds += 1
        padded = np.pad(lab.reshape(site.shape), 1, constant_values=n)
        low = lab.reshape(site.shape).copy()
        for dx, dy, dz in offs:
            low = np.minimum(low, padded[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny, 1 + dz:1 + dz + nz])
        low = np.where(site, low, n).reshape(-1)
        par = np.arange(n + 1, dtype=np.int64)
        np.minimum.at(par, lab, low)                 # every label learns the smallest label one of its voxels sees
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
    kept = roots_all[sizes_all >= min_voxels]
    number = np.zeros(n + 1, np.int32)
    number[kept] = np.arange(1, len(kept) + 1, dtype=np.int32)
    label = number[lab].reshape(site.shape)
    at = np.argwhere(label > 0)
    k = label[label > 0] - 1
    lo = np.full((len(kept), 3), max(site.shape), np.int64)
    hi = np.full((len(kept), 3), -1, np.int64)
    np.minimum.at(lo, k, at)
    np.maximum.at(hi, k, at)
    stats = np.concatenate([kept[:, None], sizes_all[sizes_all >= min_voxels][:, None], lo, hi], axis=1).astype(np.int32)
    return {"label": label, "K": len(kept), "found": len(roots_all), "stats": stats, "sizes_all": sizes_all.astype(np.int64), "rounds": rounds}


def flood_fill(site, connectivity):
    """label by ascending root from a pure-Python flood fill (small volumes only), min_voxels = 1"""
    site = np.asarray(site) != 0
    label = np.zeros(site.shape, np.int32)
    offs = offsets(connectivity)
    k = 0
    for start in zip(*np.nonzero(site)):             # C order: ascending flat index, so a new component is met at its root
        if label[start]:
            continue
        k += 1
        label[start] = k
        stack = [start]
        while stack:
            x, y, z = stack.pop()
            for dx, dy, dz in offs:
                q = (x + dx, y + dy, z + dz)
                if all(0 <= q[a] < site.shape[a] for a in range(3)) and site[q] and not label[q]:
                    label[q] = k
                    stack.append(q)
    return label


def renumber_by_root(label):
    """any labelling (0 = background) renumbered 1..K by the smallest flat index of each label"""
    flat = np.asarray(label).reshape(-1)
    out = np.zeros(flat.shape, np.int32)
    ids, first = np.unique(flat, return_index=True)
    order = [i for i in np.argsort(first) if ids[i] != 0]
    lut = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.int32)
    for k, i in enumerate(order):
        lut[ids[i]] = k + 1
    out = lut[flat]
    return out.reshape(np.asarray(label).shape)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _random(shape, density, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    k = max(1, int(round(density * n)))
    site = np.zeros(n, np.uint8)
    site[rng.choice(n, k, replace=False)] = rng.integers(1, 256, k)      # any non-zero byte is a site
    return site.reshape(shape)


def _points(shape, *pts):
    site = np.zeros(shape, np.uint8)
    for p in pts:
        site[p] = 1
    return site


# name -> (shape, density).  The kernels put the flat index along the lanes, 64 to a wave, and start a run at a wave boundary as well as
# at a line start: 2x3x33 ... 2x3x130 put wave boundaries inside lines at every phase, nz = 64 puts them on line starts, nz = 1 and 5
# put many lines into one wave, 3x4x300 several waves into one line.  The flatten kernel's workgroup takes ceil(n / 131072) turns of 256 voxels:
# one turn up to 131 072 voxels (130x66x5, the serpentine), two beyond (50x50x53 with a ragged last workgroup, 64x64x64 exactly).
RANDOM = {
    "1x1x90": ((1, 1, 90), 0.5), "1x300x1": ((1, 300, 1), 0.5), "300x1x1": ((300, 1, 1), 0.5), "40x33x1 45%": ((40, 33, 1), 0.45),
    "5x4x6 30%": ((5, 4, 6), 0.30), "9x8x10 30%": ((9, 8, 10), 0.30), "65x3x67 25%": ((65, 3, 67), 0.25), "3x4x300 30%": ((3, 4, 300), 0.30),
    "130x66x5 25%": ((130, 66, 5), 0.25), "2x3x33 50%": ((2, 3, 33), 0.5), "2x3x63 50%": ((2, 3, 63), 0.5), "2x3x64 50%": ((2, 3, 64), 0.5),
    "2x3x65 50%": ((2, 3, 65), 0.5), "2x3x130 50%": ((2, 3, 130), 0.5),
    "ragged 50x50x53 6%": ((50, 50, 53), 0.06), # 132 500 voxels: two turns per workgroup of the flatten kernel, the last workgroup ragged
    "64x64x64 31%": ((64, 64, 64), 0.31),       # beside the site-percolation threshold of connectivity 6 (0.3116): tortuous spanning components
}
CORNERS_345 = list(itertools.product((0, 2), (0, 3), (0, 4)))
SERPENTINE_SHAPE = (21, 20, 130)
SERPENTINE_GATES = [(x, 0, 0) if (x // 2) % 2 == 0 else (x, 19, 129) for x in range(1, 21, 2)]
PLATE_JOINT = (3, 39, 69)

# constructed cases: name -> the number of components under connectivity 6 / 18 / 26
EXPECTED = {
    "no site": (0, 0, 0), "all sites": (1, 1, 1),
    "face pair": (1, 1, 1), "edge pair": (2, 1, 1), "corner pair": (2, 2, 1),
    "wrap z": (2, 2, 2), "wrap y": (2, 2, 2), "wrap yz": (2, 2, 2),
    "checkerboard": (360, 1, 1),
    "serpentine": (1, 1, 1), "serpentine cut": (2, 2, 2),
    "plates": (1, 1, 1), "plates apart": (2, 2, 2),
    "combs": (2, 2, 2), "nested": (2, 2, 2),
}
EXPECTED.update({"one site %d%d%d" % c: (1, 1, 1) for c in CORNERS_345})


@functools.lru_cache(maxsize=None)
def site_volume(name):
    if name in RANDOM:
        shape, density = RANDOM[name]
        site = _random(shape, density, 9000 + sorted(RANDOM).index(name))
    elif name == "no site":
        site = np.zeros((3, 4, 5), np.uint8)
    elif name == "all sites":
        site = np.full((3, 4, 5), 7, np.uint8)
    elif name.startswith("one site "):
        site = _points((3, 4, 5), tuple(int(c) for c in name[-3:]))
    elif name == "face pair":
        site = _points((3, 3, 3), (0, 0, 0), (1, 0, 0))
    elif name == "edge pair":
        site = _points((3, 3, 3), (0, 0, 0), (1, 1, 0))
    elif name == "corner pair":
        site = _points((3, 3, 3), (0, 0, 0), (1, 1, 1))
    elif name == "wrap z":
        site = _points((3, 3, 4), (0, 0, 3), (0, 1, 0))
    elif name == "wrap y":
        site = _points((3, 3, 4), (0, 2, 1), (1, 0, 1))
    elif name == "wrap yz":
        site = _points((3, 3, 4), (0, 2, 3), (1, 0, 0))
    elif name == "checkerboard":
        site = (np.indices((9, 8, 10)).sum(0) % 2 == 0).astype(np.uint8)
    elif name in ("serpentine", "serpentine cut"):      # full x slabs at even x; a single gate voxel at alternating far corners joins two slabs
        site = np.zeros(SERPENTINE_SHAPE, np.uint8)
        site[0::2] = 1
        for g in SERPENTINE_GATES:
            site[g] = 1
        if name == "serpentine cut":
            site[SERPENTINE_GATES[5]] = 0
    elif name in ("plates", "plates apart"):          # the joint is the last place a merge in flat order reaches
        site = np.zeros((7, 40, 70), np.uint8)
        site[2] = 1
        site[4] = 1
        if name == "plates":
            site[PLATE_JOINT] = 1
    elif name == "combs":                               # teeth alternate along x with one empty layer between them on every side
        site = np.zeros((24, 20, 66), np.uint8)
        site[:, 0, :] = 1
        site[0::4, 0:18, :] = 1
        site[:, 19, :] = 2
        site[2::4, 2:20, :] = 2
    elif name == "nested":                              # a hollow cube shell, a 2x2x2 blob in its cavity
        site = np.ones((12, 12, 12), np.uint8)
        site[1:11, 1:11, 1:11] = 0
        site[5:7, 5:7, 5:7] = 3
    else:
        raise KeyError(name)
    site.setflags(write=False)
    return site


CASES = list(EXPECTED) + list(RANDOM)
SMALL = [name for name in CASES if site_volume(name).size <= 1000]      # a flood fill in Python is affordable

# (case, connectivity, m): components of size m-1, m and m+1 all exist (asserted on the host), so a wrong comparison shows
MIN_VOXELS = [("9x8x10 30%", 6, 2), ("9x8x10 30%", 6, 3), ("65x3x67 25%", 6, 2), ("65x3x67 25%", 6, 5), ("65x3x67 25%", 18, 2), ("65x3x67 25%", 26, 2)]
CAPACITY_CASE = ("9x8x10 30%", 6)                        # stats_capacity 0 (NULL), 1, K-1, K, K+3


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, min_voxels=1):
    """components_ref of a case, computed once and shared (read-only)"""
    ref = components_ref(site_volume(name), connectivity, min_voxels)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
