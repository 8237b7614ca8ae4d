"""NumPy restatement and case list of the cost-to-go field (d3f_volume_geodesic_init / _relax / _finish and d3f_volume_follow,
include/d3fields_hip.h), shared by tests/test_geodesic_host.py and tests/test_gpu_geodesic.py.

The contract, restated:
    free        uint8 [nx, ny, nz], z fastest; any non-zero byte is traversable
    neighbours  coordinates differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1 for connectivity 6 / 18 / 26; spatial, nothing
                wraps through memory
    moves       between two free neighbours u, v; entering v costs w[|u - v|_1 - 1] + max(penalty[v], 0), w = (w1, w2, w3) integers with
                1 <= w1 <= w2 <= w3 <= 255
    cost[v]     int32: the cheapest sum of move costs from any seed; 0 at a seed (its own penalty is not charged); seeds out of range or on
                a non-free voxel are ignored; candidates never wrap and are discarded above max_cost; INT32_MAX where unreached
    next[v]     among the neighbours u with cost[u] + w(u, v) + penalty[v] == cost[v] the one with the smallest flat index; v at a seed; -1
                where unreached
    dist[v]     float32(cost[v]) * (float32(step) / float32(w1)), +inf where unreached

travel_ref shares nothing with the kernels' tiles: Jacobi sweeps of the whole volume over padded shifted copies (nothing wraps), in int64,
until nothing changes.  test_geodesic_host.py checks it against scipy.sparse.csgraph.dijkstra on a graph built from the definition.
"""
import functools
import itertools

import numpy as np

import ccl_cases as CC

INT32_MAX = 2 ** 31 - 1
NO_CAP = INT32_MAX - 1
POISON = CC.POISON
CONFIGS = [(6, (1, 1, 1)), (18, (2, 3, 3)), (26, (3, 4, 5))]
_FAR = np.int64(1) << 40      # "unreached" inside travel_ref: above every sum, far from wrapping int64


def offsets(connectivity):
    """the neighbour offsets (dx, dy, dz) in ascending order of the flat index they lead to"""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(c) for c in o) <= reach]


def _shift(padded, o, shape):
    return padded[1 + o[0]:1 + o[0] + shape[0], 1 + o[1]:1 + o[1] + shape[1], 1 + o[2]:1 + o[2] + shape[2]]


def accepted_seeds(free, seeds):
    free = np.asarray(free).reshape(-1) != 0
    return sorted({int(s) for s in np.asarray(seeds, np.int64).reshape(-1) if 0 <= s < free.size and free[s]})


def _penalty(penalty, shape):
    return np.zeros(shape, np.int64) if penalty is None else np.maximum(np.asarray(penalty).astype(np.int64), 0)


def travel_ref(free, seeds, connectivity, w, penalty=None, max_cost=NO_CAP):
    """-> (cost int32 [nx, ny, nz], sweeps)"""
    free = np.asarray(free) != 0
    shape = free.shape
    assert free.ndim == 3 and 1 <= w[0] <= w[1] <= w[2] <= 255 and 1 <= max_cost <= NO_CAP
    pen = _penalty(penalty, shape)
    cost = np.full(free.size, _FAR, np.int64)
    cost[accepted_seeds(free, seeds)] = 0
    cost = cost.reshape(shape)
    sweeps = 0
    while True:
        sweeps += 1
        padded = np.pad(cost, 1, constant_values=_FAR)
        cand = np.full(shape, _FAR, np.int64)
        for o in offsets(connectivity):
            np.minimum(cand, _shift(padded, o, shape) + w[sum(abs(c) for c in o) - 1], out=cand)
        cand += pen
        new = np.where(free & (cand <= max_cost), np.minimum(cost, cand), cost)
        if np.array_equal(new, cost):
            break
        cost = new
    return np.where(cost >= _FAR, INT32_MAX, cost).astype(np.int32), sweeps


def next_ref(cost, connectivity, w, penalty=None):
    """int32 [nx, ny, nz] from final costs: offsets taken in descending order and overwritten, so the smallest flat index stays"""
    cost = np.asarray(cost)
    shape = cost.shape
    c = np.where(cost == INT32_MAX, _FAR, cost.astype(np.int64))
    pen = _penalty(penalty, shape)
    flat = np.arange(cost.size, dtype=np.int64).reshape(shape)
    padded_c = np.pad(c, 1, constant_values=_FAR)
    padded_i = np.pad(flat, 1, constant_values=-1)
    nxt = np.full(shape, -1, np.int64)
    for o in reversed(offsets(connectivity)):
        hit = (c < _FAR) & (_shift(padded_c, o, shape) + w[sum(abs(k) for k in o) - 1] + pen == c)
        nxt = np.where(hit, _shift(padded_i, o, shape), nxt)
    nxt = np.where(c == 0, flat, nxt)
    return nxt.astype(np.int32)


def dist_ref(cost, step, w1):
    cost = np.asarray(cost)
    scale = np.float32(step) / np.float32(w1)
    with np.errstate(over="ignore"):
        return np.where(cost == INT32_MAX, np.float32(np.inf), cost.astype(np.float32) * scale).astype(np.float32)


def follow_ref(nxt, starts, max_steps):
    """-> (voxels int32 [N, max_steps] padded with -1, length int32 [N], reached uint8 [N])"""
    nxt = np.asarray(nxt).reshape(-1)
    starts = np.asarray(starts).reshape(-1)
    voxels = np.full((len(starts), max_steps), -1, np.int32)
    length = np.zeros(len(starts), np.int32)
    reached = np.zeros(len(starts), np.uint8)
    for i, s in enumerate(starts.tolist()):
        if not 0 <= s < nxt.size or nxt[s] < 0:
            continue
        k = 0
        while k < max_steps:
            voxels[i, k] = s
            k += 1
            if nxt[s] == s:
                reached[i] = 1
                break
            s = int(nxt[s])
        length[i] = k
    return voxels, length, reached


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# random volumes: name -> (shape, free fraction).  None has an extent that is a multiple of a plausible tile (4, 8, 16, 32) on all three axes;
# 50x50x53 gives many tiles and a ragged last one, 2x3x130 lines longer than two waves, 17^3 one voxel more than a tile on every axis.
RANDOM = {"13x11x19 70%": ((13, 11, 19), 0.70), "9x20x33 55%": ((9, 20, 33), 0.55), "17x17x17 45%": ((17, 17, 17), 0.45), "2x3x130 60%": ((2, 3, 130), 0.60),
          "50x50x53 45%": ((50, 50, 53), 0.45), "7x9x1 70%": ((7, 9, 1), 0.70), "1x1x130 85%": ((1, 1, 130), 0.85)}
PAIRS = {"face pair": (True, True, True), "edge pair": (False, True, True), "corner pair": (False, False, True),
         "wrap z": (False, False, False), "wrap y": (False, False, False), "wrap yz": (False, False, False)}      # is the second voxel reached under 6 / 18 / 26
SERPENTINE_SHAPE = (12, 12, 12)
# two free voxels on either side of a tile boundary, the seed first: nobody else lowers anything, so the second voxel is reached only if the tile
# that holds it runs because of the SEED.  32 is a boundary of every plausible tile extent (4, 8, 16, 32); the 16-voxel cases are the 8-voxel tile's.
BOUNDARY_SHAPE = (34, 34, 34)
BOUNDARY = {
    "tile face z": ((31, 31, 31), (31, 31, 32)), "tile face y": ((31, 31, 31), (31, 32, 31)), "tile face x": ((31, 31, 31), (32, 31, 31)),
    "tile face z back": ((31, 31, 32), (31, 31, 31)), "tile face y back": ((31, 32, 31), (31, 31, 31)), "tile face x back": ((32, 31, 31), (31, 31, 31)),
    "tile edge yz": ((31, 31, 31), (31, 32, 32)), "tile edge xz": ((31, 31, 31), (32, 31, 32)), "tile edge xy": ((31, 31, 31), (32, 32, 31)),
    "tile edge yz mixed": ((31, 32, 31), (31, 31, 32)), "tile edge xy back": ((32, 32, 31), (31, 31, 31)),
    "tile corner": ((31, 31, 31), (32, 32, 32)), "tile corner back": ((32, 32, 32), (31, 31, 31)), "tile corner mixed": ((32, 31, 32), (31, 32, 31)),
    "tile corner mixed 2": ((31, 32, 32), (32, 31, 31)),
}
SMALL_BOUNDARY = {"line 1x1x16": ((1, 1, 16), (0, 0, 7), (0, 0, 8)), "corner 16x16x16": ((16, 16, 16), (7, 7, 7), (8, 8, 8)),
                  "edge 16x16x1": ((16, 16, 1), (8, 7, 0), (7, 8, 0))}


def boundary_pair(name):
    """-> (shape, seed voxel, other voxel)"""
    return (BOUNDARY_SHAPE,) + BOUNDARY[name] if name in BOUNDARY else SMALL_BOUNDARY[name]


def l1(a, b):
    return sum(abs(p - q) for p, q in zip(a, b))


def serpentine():
    """the 12^3 double serpentine: one corridor one voxel wide.  Slabs at even x; inside a slab the corridor runs along z in the rows of even
    y, joined at alternating z ends; slabs are joined by one gate voxel at alternating ends of the slab's own corridor.  467 free voxels in
    one chain: from the seed at its first voxel the last one is 466 unit moves away under connectivity 6."""
    free = np.zeros(SERPENTINE_SHAPE, np.uint8)
    chain = []
    for xi, x in enumerate(range(0, 12, 2)):
        slab = []
        for yi, y in enumerate(range(0, 12, 2)):
            zs = list(range(12)) if yi % 2 == 0 else list(range(11, -1, -1))
            slab += [(x, y, z) for z in zs]
            if y + 2 < 12:
                slab.append((x, y + 1, zs[-1]))
        if xi % 2 == 1:
            slab.reverse()
        chain += slab
        if x + 2 < 12:
            chain.append((x + 1,) + slab[-1][1:])
    for p in chain:
        free[p] = 1
    return free, chain


def _random_case(name):
    shape, fraction = RANDOM[name]
    rng = np.random.default_rng(7100 + sorted(RANDOM).index(name))
    n = int(np.prod(shape))
    free = np.zeros(n, np.uint8)
    k = max(1, int(round(fraction * n)))
    open_ = rng.choice(n, k, replace=False)
    free[open_] = rng.integers(1, 256, k)                                # any non-zero byte is traversable
    seeds = np.concatenate([rng.choice(open_, min(4, k), replace=False), rng.choice(n, 2)]).astype(np.int32)      # (two may fall on walls)
    penalty = rng.integers(0, 4, n).astype(np.int32).reshape(shape)
    return free.reshape(shape), seeds, penalty


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (free uint8 [nx, ny, nz], seeds int32 [S], penalty int32 [nx, ny, nz] or None), read-only"""
    penalty = None
    if name in RANDOM:
        free, seeds, penalty = _random_case(name)
    elif name == "1x1x1":
        free, seeds = np.ones((1, 1, 1), np.uint8), [0]
    elif name == "all free":
        free, seeds = np.full((5, 4, 6), 9, np.uint8), [0, 77]
    elif name == "none free":
        free, seeds = np.zeros((5, 4, 6), np.uint8), [0, 77]
    elif name == "no seeds":
        free, seeds = np.ones((5, 4, 6), np.uint8), []
    elif name == "bad seeds":                      # every seed on a wall or out of range
        free = np.ones((5, 4, 6), np.uint8)
        free[0, 0, 0] = free[2, 3, 1] = free[4, 3, 5] = 0
        seeds = [0, 2 * 24 + 3 * 6 + 1, 119, -1, 120, 121, -7, INT32_MAX, -INT32_MAX - 1]
    elif name == "duplicate seeds":
        free, seeds = np.ones((5, 4, 6), np.uint8), [31, 31, 31, 90, 31, 90]
    elif name in PAIRS:                            # the pairs of ccl_cases: the seed is the first voxel, the question is the second
        free = np.array(CC.site_volume(name))
        seeds = [int(np.flatnonzero(free.reshape(-1))[0])]
    elif name in BOUNDARY or name in SMALL_BOUNDARY:
        shape, a, b = boundary_pair(name)
        free = np.zeros(shape, np.uint8)
        free[a] = free[b] = 1
        seeds = [int(np.ravel_multi_index(a, shape))]
    elif name == "corridor seed at 31":           # the seed is the last voxel of its tile: the far side hangs on the move that starts at the seed
        free, seeds = np.ones((1, 1, 40), np.uint8), [31]
    elif name == "slab seed at 31":               # the same with a whole tile face behind the seed, and walls that leave only the seed's moves
        free = np.zeros((34, 34, 34), np.uint8)
        free[:32, :32, :32] = 1
        free[32:, 32:, 32:] = 1                      # joined to the block only through the corner move (31,31,31) -> (32,32,32)
        seeds = [int(np.ravel_multi_index((31, 31, 31), free.shape))]
    elif name == "serpentine":
        free, chain = serpentine()
        seeds = [int(np.ravel_multi_index(chain[0], SERPENTINE_SHAPE))]
    elif name == "open 5x5x5":                     # the ties of next: most voxels have several equal predecessors under (26, (1, 1, 1))
        free, seeds = np.ones((5, 5, 5), np.uint8), [62]
    elif name == "corridor":                       # max_cost and saturation: a line of 24 voxels, the seed at its start
        free, seeds = np.ones((1, 1, 24), np.uint8), [0]
    else:
        raise KeyError(name)
    free = np.ascontiguousarray(free, np.uint8)
    seeds = np.asarray(seeds, np.int64).astype(np.int32)      # (int32 wraps nothing here: every listed value fits)
    for a in (free, seeds, penalty):
        if a is not None:
            a.setflags(write=False)
    return free, seeds, penalty


DEGENERATE = ["1x1x1", "7x9x1 70%", "1x1x130 85%", "all free", "none free", "no seeds", "bad seeds", "duplicate seeds"]
VOLUMES = ["13x11x19 70%", "9x20x33 55%", "17x17x17 45%", "2x3x130 60%", "50x50x53 45%"]
SEED_ON_BOUNDARY = list(BOUNDARY) + list(SMALL_BOUNDARY) + ["corridor seed at 31", "slab seed at 31"]
UNCAPPED = DEGENERATE + list(PAIRS) + VOLUMES + SEED_ON_BOUNDARY + ["serpentine", "open 5x5x5"]      # every case that runs without a cap


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, w, max_cost=NO_CAP, with_penalty=True):
    """(cost, next, sweeps) of a case from the restatement, computed once and shared (read-only)"""
    free, seeds, penalty = case(name)
    penalty = penalty if with_penalty else None
    cost, sweeps = travel_ref(free, seeds, connectivity, w, penalty, max_cost)
    nxt = next_ref(cost, connectivity, w, penalty)
    cost.setflags(write=False)
    nxt.setflags(write=False)
    return cost, nxt, sweeps
