"""Workload-sized cases of the baked-volume kernels and the fast references that can follow them there, shared by
tests/test_scale_host.py (CPU: every fast reference pinned to the slow one the project already trusts, every emulated mistake rejected)
and tests/test_gpu_scale.py (the kernels themselves).

The shapes are the smallest that cross the size-dependent branches of the launch code (the table in tests/test_gpu_scale.py):

  A = 161 x 162 x 163 = 4 251 366 voxels
      scan (scan_kernels.hip: 2048 elements per workgroup): 4 251 366 > 2048^2 = 4 194 304, so one word per voxel is three levels:
        2076 workgroups -> 2076 totals in 2 workgroups -> 2 totals in 1.  The last level-1 workgroup holds 4 251 366 - 2075 * 2048 = 1766
        elements, the last level-2 workgroup 2076 - 2048 = 28: both ragged.
      mesh: ceil(4 251 366 / 1024) = 4152 workgroups, 4153 scanned totals = 2 * 2048 + 57: two levels, a ragged third workgroup.
      geodesic: ceil(161 / 8) * ceil(162 / 8) * ceil(163 / 8) = 21^3 = 9261 tiles > kGeoMaxGrid = 4096: up to three turns per workgroup.
      distance transform: nz = 163 > 64 is the long z kernel; 161 and 162 <= 256 is the LDS line pass with 64 lines per workgroup.
      No extent is a multiple of 8 or 64: every tile row, scan workgroup and ballot word has a ragged end.
  B = 205 x 204 x 203 = 8 489 460 voxels > 64 * 131 072 = 8 388 608: ccl_flatten_kernel, ccl_box_kernel and pool_flag_kernel
      (kCclFlattenSpan = kPoolFlagSpan = 131 072) take min(64, ceil(n / 131 072)) = min(64, 65) = 64 turns -- the cap -- and the grid grows
      instead: ceil(8 489 460 / 16 384) = 519 workgroups, the last one ragged (8 489 460 - 518 * 16 384 = 2 548 voxels).
  A with ROW_CHANNELS = 512 dense float32 rows: 4 251 366 * 512 = 2 176 699 392 floats > 2^31 = 2 147 483 648; voxel * 512 passes 2^31
      from voxel 2^22 = 4 194 304 on, which is x >= 158 (the last two and a bit x planes).

Nothing here is read by the kernels' own restatements: the fast references are scipy / cumsum / bincount; the *_model functions emulate
the launch code's arithmetic in NumPy only so that its mistakes can be emulated too (SCAN_MUTANTS, tile_loop_model, sort_model, wrapped_voxel).
"""
import functools

import numpy as np

import ccl_cases as CC
import edt_cases as EC
import geodesic_cases as GC
import pool_cases as PC
import volume_cases as VC

A = (161, 162, 163)
B = (205, 204, 203)
ROW_CHANNELS = 512
INT32_MAX = 2 ** 31 - 1
SCAN_BLOCK = 2048                     # elements per workgroup of scan_kernels.hip
MESH_BLOCK = 1024                     # lattice points per workgroup of mesh_kernels.hip
SPAN = 131072                         # kCclFlattenSpan = kPoolFlagSpan
TILE = 8                              # kGeoTX = kGeoTY = kGeoTZ
GEO_MAX_GRID = 4096                   # kGeoMaxGrid
SPLIT = 2048 * 2048                   # the first flat index whose scan offset comes from the third level


def voxels(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2])


# ---- the scan, as launched -----------------------------------------------------------------------------------------------------------
def scan_levels(n):
    """element counts of the recursion: [n, ceil(n / 2048), ...] down to the first level that fits one workgroup"""
    out = [int(n)]
    while out[-1] > SCAN_BLOCK:
        out.append((out[-1] + SCAN_BLOCK - 1) // SCAN_BLOCK)
    return out


def scan_scratch_bytes(n):
    """scan_scratch_bytes of scan_kernels.hip: every level of totals padded to 256 bytes, plus 256"""
    return sum((m * 4 + 255) // 256 * 256 for m in scan_levels(n)[1:]) + 256


def turns(n):
    """(turns per workgroup, workgroups) of ccl_flatten_kernel, ccl_box_kernel and pool_flag_kernel"""
    iters = min(64, (n + SPAN - 1) // SPAN)
    return iters, (n + 256 * iters - 1) // (256 * iters)


def tiles(shape):
    return tuple((s + TILE - 1) // TILE for s in shape)


SCAN_MUTANTS = ("third level not added back", "ragged last workgroup dropped")


def scan_model(x, mutant=None, _level=1):
    """launch_exclusive_scan_u32 in NumPy (uint32 wrap-around included): per-workgroup exclusive scans, the totals scanned recursively and added back.
      'third level not added back'     the scan of the level-1 totals (level 2) forgets the offsets its own recursion (level 3) produced
      'ragged last workgroup dropped'  at any level with several workgroups the last, partly filled one does nothing: its elements keep their input
                                       values (the scans run in place) and its total counts as 0
    Writing only the TOTAL of the last workgroup wrongly is not a mutant: an exclusive scan never reads it (test_scale_host.py asserts that)."""
    x = np.asarray(x, np.int64)
    n = x.size
    nb = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    v = np.zeros(nb * SCAN_BLOCK, np.int64)
    v[:n] = x
    v = v.reshape(nb, SCAN_BLOCK)
    incl = np.cumsum(v, axis=1)
    out = incl - v
    totals = incl[:, -1].copy()
    ragged = nb > 1 and n % SCAN_BLOCK != 0
    if mutant == "ragged last workgroup dropped" and ragged:
        out[-1] = v[-1]
        totals[-1] = 0
    if mutant == "last total dropped" and ragged:
        totals[-1] = 0
    if nb > 1:
        offs = scan_model(totals & 0xFFFFFFFF, mutant, _level + 1)
        if mutant == "ragged last workgroup dropped" and ragged:
            offs = offs.copy()
            offs[-1] = 0                                      # (its scan_add does nothing either)
        out = out + offs[:, None]
    if mutant == "third level not added back" and _level == 2 and nb > 1:
        out = incl - v
    return (out.reshape(-1)[:n] & 0xFFFFFFFF).astype(np.int64)


def compact_model(flags, mutant=None):
    """an order-preserving compaction as band_slot_kernel / pool_compact_kernel / ccl_label_kernel do it: rank = scan(flags),
    list[rank[q]] = q for every flagged q below the count -> (rank [n], list [count], count); count = rank[n-1] + flags[n-1] as the kernels form it"""
    flags = np.asarray(flags).astype(np.int64)
    rank = scan_model(flags, mutant)
    count = int(rank[-1] + flags[-1])
    out = np.full(max(count, 0), -1, np.int64)
    q = np.flatnonzero(flags)
    ok = rank[q] < count
    out[rank[q][ok]] = q[ok]
    return rank, out, count


# ---- connected components: scipy.ndimage.label -----------------------------------------------------------------------------------------
def components_fast(site, connectivity, min_voxels=1):
    """the dict of ccl_cases.components_ref (without 'rounds') from scipy.ndimage.label, canonicalised by ccl_cases.renumber_by_root"""
    from scipy import ndimage
    site = np.asarray(site) != 0
    n = site.size
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    raw, found = ndimage.label(site, structure=structure)
    lab = CC.renumber_by_root(raw).reshape(-1)                          # 1..found in ascending order of root
    sizes_all = np.bincount(lab, minlength=found + 1)[1:].astype(np.int64)
    keep = sizes_all >= min_voxels
    number = np.zeros(found + 1, np.int32)
    number[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    label = number[lab]
    K = int(keep.sum())
    at = np.flatnonzero(label)
    k = label[at] - 1
    roots = np.full(K, n, np.int64)
    np.minimum.at(roots, k, at)
    xyz = np.stack(np.unravel_index(at, site.shape), axis=1).astype(np.int64)
    lo = np.full((K, 3), max(site.shape), np.int64)
    hi = np.full((K, 3), -1, np.int64)
    np.minimum.at(lo, k, xyz)
    np.maximum.at(hi, k, xyz)
    stats = np.concatenate([roots[:, None], sizes_all[keep][:, None], lo, hi], axis=1).astype(np.int32)
    return {"label": label.reshape(site.shape), "K": K, "found": int(found), "stats": stats, "sizes_all": sizes_all}


def random_sites(shape, density, seed):
    """ccl_cases._random: exactly round(density * n) sites of any non-zero byte"""
    rng = np.random.default_rng(seed)
    n = voxels(shape)
    k = max(1, int(round(density * n)))
    site = np.zeros(n, np.uint8)
    site[rng.choice(n, k, replace=False)] = rng.integers(1, 256, k)
    return site.reshape(shape)


PERCOLATION_DENSITY = CC.RANDOM["64x64x64 31%"][1]      # 0.31, beside the site-percolation threshold of connectivity 6 (0.3116)
SPECK_DENSITY = 0.15                                    # above the threshold of connectivity 26 (0.097): one spanning component, many specks


@functools.lru_cache(maxsize=None)
def ccl_case(which):
    """'A': A at the percolation density (connectivity 6: tortuous spanning components, K >= 65 536);
    'B': B at 15 % (connectivity 26: one component that spans the box and holds most sites, thousands of specks) -> (site, connectivity)"""
    site = random_sites(A, PERCOLATION_DENSITY, 9100) if which == "A" else random_sites(B, SPECK_DENSITY, 9101)
    site.setflags(write=False)
    return site, (6 if which == "A" else 26)


@functools.lru_cache(maxsize=None)
def ccl_reference(which, min_voxels=1):
    site, conn = ccl_case(which)
    ref = components_fast(site, conn, min_voxels)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- pooling: cumsum / bincount for the integers, a vectorised fold for the bits ----------------------------------------------------------
def members_fast(label, K, valid=None):
    """(member flags [n] bool, the members grouped by label in ascending flat index [M], their labels [M], counts int64 [K])"""
    flat = np.asarray(label).reshape(-1)
    ok = (flat >= 1) & (flat <= K)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    idx = np.flatnonzero(ok)
    keys = flat[idx].astype(np.int64)
    order = np.argsort(keys, kind="stable")
    counts = np.bincount(keys, minlength=K + 1)[1:]
    return ok, idx[order], keys[order], counts


def moments_fast(label, K, valid=None):
    """int64 [K, 9] by bincount: the coordinate sums stay below 2^53 (at most 8.5 M members times 205^2), so the float64 weights are exact"""
    shape = np.asarray(label).shape
    _, idx, keys, _ = members_fast(label, K, valid)
    x, y, z = (a.astype(np.float64) for a in np.unravel_index(idx, shape))
    cols = [x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    return np.stack([np.bincount(keys, weights=c, minlength=K + 1)[1:] for c in cols], axis=1).astype(np.int64)


def _fold_segments(rows, starts, lengths):
    """((r0 + r1) + r2) + ... of every segment rows[starts[g] : starts[g] + lengths[g]] (1 <= length <= 256), one float32 add per step"""
    acc = rows[starts].copy()
    for t in range(1, int(lengths.max()) if lengths.size else 0):
        on = np.flatnonzero(lengths > t)
        if on.size == 0:
            break
        acc[on] = acc[on] + rows[starts[on] + t]
    return acc


def fold_fast(rows, counts):
    """pool_cases.fold of every component at once.  rows float32 [M, C]: the member rows grouped by component (ascending flat index inside);
    counts [K] -> float32 [K, C], zeros for an empty component.  Level by level: every component's list is cut into chunks of 256 (a ragged
    last one), every chunk folded, and the chunk folds are the next level's list."""
    rows = np.ascontiguousarray(rows, np.float32)
    counts = np.asarray(counts, np.int64)
    K = counts.size
    out = np.zeros((K, rows.shape[1]), np.float32)
    while True:
        starts = np.cumsum(counts) - counts
        chunks = (counts + PC.CHUNK - 1) // PC.CHUNK
        comp = np.repeat(np.arange(K), chunks)
        within = np.arange(int(chunks.sum())) - np.repeat(np.cumsum(chunks) - chunks, chunks)
        cstart = starts[comp] + within * PC.CHUNK
        clen = np.minimum(PC.CHUNK, counts[comp] - within * PC.CHUNK)
        rows = _fold_segments(rows, cstart, clen)
        done = chunks == 1
        first_chunk = np.cumsum(chunks) - chunks
        out[done] = rows[first_chunk[done]]
        counts = np.where(done, 0, chunks)
        keep = np.repeat(~done, chunks)
        rows = rows[keep]
        if not counts.any():
            return out


def pool_fast(label, K, rows, valid=None, fill=None):
    """pool_cases.pool_ref: float32 [K, C], the same bits"""
    rows = np.asarray(rows)
    _, idx, _, counts = members_fast(label, K, valid)
    out = fold_fast(rows[idx], counts)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (out / counts.astype(np.float32)[:, None]).astype(np.float32)
    out[counts == 0] = 0 if fill is None else fill
    return out


def pool_mean64(label, K, rows, valid=None):
    """(mean float64 [K, C], mean of |row| float64 [K, C]) by bincount: the order-free reference of the means"""
    rows = np.asarray(rows)
    _, idx, keys, counts = members_fast(label, K, valid)
    r = rows[idx].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.stack([np.bincount(keys, weights=r[:, c], minlength=K + 1)[1:] for c in range(r.shape[1])], axis=1) / counts[:, None]
        a = np.stack([np.bincount(keys, weights=np.abs(r[:, c]), minlength=K + 1)[1:] for c in range(r.shape[1])], axis=1) / counts[:, None]
    return s, a


def fold_bound(counts):
    """[K]: the relative rounding of a mean against sum |row| / count.  A row takes part in at most 255 adds per level of the radix-256 tree,
    each correctly rounded (relative error <= 2^-24), and the division rounds once: (255 * levels + 1) * 2^-24, first order; the factor 1.01
    covers the second-order terms (766 * 2^-24 < 5e-5)."""
    levels = np.array([PC.fold_levels(int(c)) if c > 0 else 1 for c in np.asarray(counts)], np.float64)
    return 1.01 * (255.0 * levels + 1.0) * VC.U


def votes_fast(label, K, rows, valid=None):
    rows = np.asarray(rows)
    _, idx, keys, _ = members_fast(label, K, valid)
    best = PC.argmax_rule(rows[idx])
    C = rows.shape[1]
    return np.bincount((keys - 1) * C + best, minlength=K * C).reshape(K, C).astype(np.int32)


def sort_model(keys, passes):
    """the stable LSD radix sort of pool_sort_*: 8 bits per pass -> the permutation after `passes` passes"""
    order = np.arange(keys.size)
    for p in range(passes):
        order = order[np.argsort((keys[order] >> (8 * p)) & 255, kind="stable")]
    return order


def sort_passes(K):
    return 1 if K < 256 else 2 if K < 65536 else 3 if K < (1 << 24) else 4


def pool_layout_bytes(n, K, cap, mean_channels):
    """pool_workspace_bytes of pool_kernels.hip (every piece padded to 256 bytes), restated so that a change of the layout shows"""
    pad = lambda b: (b + 255) // 256 * 256      # noqa: E731
    cap = min(cap, n)
    pitch = mean_channels + 3 * 8 if mean_channels > 0 else 0
    waves = ((cap + 1023) // 1024 + 3) // 4 * 4
    total = pad(4 * n) + pad(scan_scratch_bytes(n)) + 4 * pad(4 * cap) + pad(4 * 256 * waves) + pad(scan_scratch_bytes(256 * waves))
    total += pad(8 * pad(4 * (K + 1))) + pad(scan_scratch_bytes(K + 1))
    rows_a = 2 * (cap >> 8) + 2 if cap > 256 else 0
    rows_b = 2 * (cap >> 16) + 2 if cap > 65536 else 0
    return total + pad(4 * pitch * rows_a) + pad(4 * pitch * rows_b)


POOL_CHANNELS = (3, 4)            # a scalar and a vector row
POOL_VOTE_CHANNELS = 6


@functools.lru_cache(maxsize=None)
def pool_case(which):
    """the label volume of ccl_reference(which), 1 % invalid voxels, two narrow mean sets and one vote set -> dict"""
    ref = ccl_reference(which)
    shape = ref["label"].shape
    n = voxels(shape)
    rng = np.random.default_rng(9200 + (which == "B"))
    valid = np.ones(n, np.uint8)
    valid[rng.choice(n, n // 100, replace=False)] = 0
    rows = [PC.field_rows(n, C, 9210 + C) for C in POOL_CHANNELS] if which == "A" else []
    votes = rng.integers(-2, 3, size=(n, POOL_VOTE_CHANNELS)).astype(np.float32) * np.float32(0.5) if which == "A" else None      # exact ties are common
    return {"label": ref["label"], "K": ref["K"], "valid": valid.reshape(shape), "rows": rows, "votes": votes}


# ---- distance transform: scipy.ndimage.distance_transform_edt -------------------------------------------------------------------------------
def edt_fast(site):
    """edt_cases.edt_true from scipy's feature transform: the squared distance is formed from the integer coordinates of the site scipy names,
    so it is an exact integer whatever scipy's float distance rounds to"""
    from scipy import ndimage
    site = np.asarray(site) != 0
    if not site.any():
        return np.full(site.shape, EC.INT32_MAX, np.int32)
    idx = ndimage.distance_transform_edt(~site, return_distances=False, return_indices=True)
    d2 = np.zeros(site.shape, np.int64)
    for a in range(3):
        own = np.arange(site.shape[a], dtype=np.int64).reshape([-1 if b == a else 1 for b in range(3)])
        d2 += (idx[a].astype(np.int64) - own) ** 2
    return d2.astype(np.int32)


EDT_SLAB = (48, 118)              # z planes without a site: 70 > 64, wider than a wave of the z pass and than one ballot word


@functools.lru_cache(maxsize=None)
def edt_case():
    """A with 0.05 % random sites and none in the slab: distances of some ten voxels everywhere, up to 35 along z in the slab"""
    site = np.array(random_sites(A, 0.0005, 9300))
    site[:, :, EDT_SLAB[0]:EDT_SLAB[1]] = 0
    site.setflags(write=False)
    return site


@functools.lru_cache(maxsize=None)
def edt_reference():
    d2 = edt_fast(edt_case())
    d2.setflags(write=False)
    return d2


# ---- cost-to-go -----------------------------------------------------------------------------------------------------------------------------
GEO_WALLS = 0.15                  # obstacle density: the free space of each half is one component but for single enclosed voxels
GEO_SLAB = (80, 88)               # x planes of the tile layer bx = 10, solid: see tile_loop_model for why the case needs it
GEO_CONFIGS = [(26, (3, 4, 5)), (6, (1, 1, 1))]


@functools.lru_cache(maxsize=None)
def travel_case():
    """-> (free uint8 A, seeds int32 [9261]): 15 % random walls, one solid tile layer, one goal in every tile -- on a free voxel wherever one of
    eight random picks inside the tile is free, which leaves only the goals of the 441 solid tiles on walls (ignored by the contract)"""
    rng = np.random.default_rng(9400)
    free = np.where(rng.random(A) >= GEO_WALLS, rng.integers(1, 256, A), 0).astype(np.uint8)
    free[GEO_SLAB[0]:GEO_SLAB[1]] = 0
    t = tiles(A)
    b = np.stack(np.meshgrid(*[np.arange(m) for m in t], indexing="ij"), axis=-1).reshape(-1, 3)                  # ascending tile index
    ext = np.minimum(TILE, np.asarray(A) - b * TILE)
    pick = b[:, None, :] * TILE + (rng.random((len(b), 8, 3)) * ext[:, None, :]).astype(np.int64)
    flat = np.ravel_multi_index((pick[..., 0], pick[..., 1], pick[..., 2]), A)
    first_free = np.argmax(free.reshape(-1)[flat] != 0, axis=1)
    seeds = flat[np.arange(len(b)), first_free].astype(np.int32)
    free.setflags(write=False)
    seeds.setflags(write=False)
    return free, seeds


@functools.lru_cache(maxsize=None)
def travel_reference(connectivity, w):
    free, seeds = travel_case()
    cost, sweeps = GC.travel_ref(free, seeds, connectivity, w)
    nxt = GC.next_ref(cost, connectivity, w)
    cost.setflags(write=False)
    nxt.setflags(write=False)
    return cost, nxt, sweeps


def listed_after_init(free, seeds):
    """the tiles geo_seed_kernel flags: the tile of every accepted seed and every tile that holds one of its 26 neighbours -> sorted tile indices"""
    t = tiles(free.shape)
    s = np.asarray(GC.accepted_seeds(free, seeds), np.int64)
    xyz = np.stack(np.unravel_index(s, free.shape), axis=1)
    out = set()
    for d in np.stack(np.meshgrid(*[(-1, 0, 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3):
        q = xyz + d
        ok = np.all((q >= 0) & (q < np.asarray(free.shape)), axis=1)
        out.update(np.ravel_multi_index(tuple((q[ok] // TILE).T), t).tolist())
    return np.array(sorted(out), np.int64)


def tile_loop_model(free, seeds, limit=None):
    """Which tiles EVER run when a round processes only the first `limit` entries of its list (None: all of them) -> bool [tiles].
    The model is as kind to the mistake as the kernels could be: the list is in ascending tile order, a tile that runs and holds a free voxel
    flags all 26 neighbours, every time (the kernel flags fewer: only where a voxel on that side fell).  A tile without a free voxel never
    lowers anything and so never flags.  A tile that never runs keeps what init wrote: INT32_MAX, and 0 at its seeds.
    On connected free space the truncated loop heals itself under this model (and in the kernel: a dropped tile is listed again as soon as a
    neighbour lowers a voxel beside it, and then relaxes from its own goal as well), so no output can show it; a solid tile layer stops the
    flags, and the tiles behind it that the first round dropped are never listed again."""
    t = tiles(free.shape)
    has_free = np.zeros(t, bool)
    fx, fy, fz = np.nonzero(np.asarray(free) != 0)
    has_free[fx // TILE, fy // TILE, fz // TILE] = True
    has_free = has_free.reshape(-1)
    ran = np.zeros(has_free.size, bool)
    listed = listed_after_init(free, seeds)
    nb = np.stack(np.meshgrid(*[(-1, 0, 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    for _ in range(4 * sum(t)):
        if listed.size == 0:
            break
        run = listed if limit is None else listed[:limit]
        fresh = run[~ran[run]]                                 # (a tile that ran before has converged as far as this model goes)
        ran[run] = True
        src = fresh[has_free[fresh]]
        b = np.stack(np.unravel_index(src, t), axis=1)
        q = (b[:, None, :] + nb[None, :, :]).reshape(-1, 3)
        ok = np.all((q >= 0) & (q < np.asarray(t)), axis=1)
        flagged = np.unique(np.ravel_multi_index(tuple(q[ok].T), t))
        listed = flagged[~ran[flagged]]
    return ran


def unrun_tiles_cost(cost, free, seeds, ran):
    """the cost volume the model leaves: the true cost in every tile that ran, init's values elsewhere"""
    t = tiles(cost.shape)
    ix, iy, iz = np.indices(cost.shape, sparse=True)
    tile_ran = ran.reshape(t)[ix // TILE, iy // TILE, iz // TILE]
    init = np.full(cost.size, INT32_MAX, np.int32)
    init[GC.accepted_seeds(free, seeds)] = 0
    return np.where(tile_ran, cost, init.reshape(cost.shape))


# ---- volumes for the band and the mesh ------------------------------------------------------------------------------------------------------
BAND_CHANNELS = (3, 20)           # a narrow and a wide set (kVolNarrowMax = 16)
BAND_STEPS = 1.0
N_POINTS = 4099                   # 16 workgroups of 256 and three points


@functools.lru_cache(maxsize=None)
def band_volume(with_sets=False):
    """A on the lattice of volume_cases (origin and step short binary fractions, so g is exact up to one rounding): a sphere of radius 79.2
    around x = 100.13 that the far x face cuts -- its shell crosses the planes x = 158 .. 160 in a ring of radius 53, so more than a thousand
    kept cells lie beyond flat index 2048^2 (x = 158.8) -- signed distance clamped to +- 3 h, 1 % invalid voxels with NaN"""
    h = float(VC.STEP)
    rng = np.random.default_rng(9500)
    ax = [np.arange(n, dtype=np.float64) for n in A]
    centre = [100.13, (A[1] - 1) / 2.0 + 0.26, (A[2] - 1) / 2.0 + 0.39]
    radius = 0.495 * (min(A) - 1)
    r = np.sqrt((ax[0][:, None, None] - centre[0]) ** 2 + (ax[1][None, :, None] - centre[1]) ** 2 + (ax[2][None, None, :] - centre[2]) ** 2)
    vol = {"origin": np.asarray(VC.ORIGIN, np.float32), "step": np.float32(VC.STEP), "shape": A, "sets": {}, "fills": {}, "centre": centre, "radius": radius}
    vol["dist"] = np.clip((r - radius) * h, -3 * h, 3 * h).astype(np.float32)
    valid = np.ones(voxels(A), bool)
    valid[rng.choice(valid.size, valid.size // 100, replace=False)] = False
    vol["valid"] = valid.reshape(A)
    vol["dist"][~vol["valid"]] = np.nan
    if with_sets:
        for s, C in enumerate(BAND_CHANNELS):
            arr = rng.standard_normal(A + (C,), dtype=np.float32) + rng.choice([0.0, 3.0], size=C).astype(np.float32)
            arr[~vol["valid"]] = np.nan
            vol["sets"]["s%d" % s] = arr
            vol["fills"]["s%d" % s] = rng.standard_normal(C).astype(np.float32) if s == 0 else None
    return vol


def band_length(vol):
    return np.float32(float(vol["step"]) * BAND_STEPS)


def points_in_cells(vol, cells, seed):
    """one float32 point inside each cell [N, 3] (g = cell + U(0.01, 0.99)); the 1e-4 margin from the lattice planes is asserted"""
    rng = np.random.default_rng(seed)
    g = np.asarray(cells, np.float64) + rng.uniform(0.01, 0.99, size=(len(cells), 3))
    pts = (np.asarray(vol["origin"], np.float64) + g * float(vol["step"])).astype(np.float32)
    g32 = (pts.astype(np.float64) - np.asarray(vol["origin"], np.float64)) / float(vol["step"])
    assert np.all(np.abs(g32 - np.round(g32)) >= 1e-4) and np.all(np.floor(g32) == np.asarray(cells))
    return pts


def band_points(vol, cell_band):
    """N_POINTS points: the first 1000 kept cells in flat voxel order, the 2000 nearest below flat voxel index 2048^2, the last 1000 -- all of them
    above it: their slots are the ones that depend on the third scan level -- and 99 cells outside the band at the first and last voxels"""
    nx, ny, nz = vol["shape"]
    cx, cy, cz = np.nonzero(cell_band)                                 # C order = ascending flat index of the cell's lowest voxel
    base = (cx * ny + cy) * nz + cz
    cut = int(np.searchsorted(base, SPLIT))
    assert 3000 <= cut <= base.size - 1000, "kept cells on both sides of flat index 2048^2"
    pick = np.concatenate([np.arange(1000), np.arange(cut - 2000, cut), np.arange(base.size - 1000, base.size)])
    kept = np.stack([cx[pick], cy[pick], cz[pick]], axis=1)
    corners = np.array([[i, j, k] for i in (0, nx - 2) for j in (0, ny - 2) for k in range(0, 25)])[:99]
    corners[50:, 2] = nz - 2 - corners[50:, 2]
    cells = np.concatenate([kept, corners])
    assert len(cells) == N_POINTS
    return points_in_cells(vol, cells, 9600)


def row_points(shape=A):
    """N_POINTS points for the rows past 2^31: 2100 in cells with ix >= 157 (corner rows at voxels >= 2^22, where voxel * 512 passes 2^31, and
    just below), 999 in the first two x planes, 1000 anywhere"""
    rng = np.random.default_rng(9700)
    nx, ny, nz = shape

    def cells(n, x_lo, x_hi):
        return np.stack([rng.integers(x_lo, x_hi, n), rng.integers(0, ny - 1, n), rng.integers(0, nz - 1, n)], axis=1)

    c = np.concatenate([cells(2100, nx - 4, nx - 1), cells(999, 0, 2), cells(1000, 0, nx - 1)])
    c[0] = (nx - 2, ny - 2, nz - 2)                                    # the last cell: its far corner is the last voxel
    assert len(c) == N_POINTS
    vol = {"origin": np.asarray(VC.ORIGIN, np.float32), "step": np.float32(VC.STEP), "shape": shape}
    return points_in_cells(vol, c, 9701), c


def row_pool_members(shape=A):
    """the two components pooled on the 512-channel volume: the last 1000 voxels (every one beyond 2^22), and 66 000 scattered ones in ascending
    order (65 536 < 66 000: three fold levels), a third of them beyond 2^22 as well"""
    n = voxels(shape)
    rng = np.random.default_rng(9702)
    m1 = np.arange(n - 1000, n, dtype=np.int64)
    low = rng.choice(2 ** 22, 44000, replace=False)
    high = 2 ** 22 + rng.choice(n - 1000 - 2 ** 22, 22000, replace=False)
    return m1, np.sort(np.concatenate([low, high])).astype(np.int64)


# ---- the eight-corner chain from gathered corner values ------------------------------------------------------------------------------------
# volume_cases works on whole volumes; the 8.7 GB volume exists on the device only, so its test gathers the eight corner rows there and hands
# them to these functions.  They are volume_cases' own formulas on [8, N, C] corner values (test_scale_host.py asserts equality with
# volume_cases.trilinear64 / trilinear32 / trilinear_grad64 / trilinear_grad32 on its small cases).
def locate_cells(shape, origin, step, pts, dtype=np.float64):
    """(i [N, 3] int64, t [N, 3] dtype) of points known to lie inside: g formed in `dtype` as volume_cases.locate64 / locate32 do"""
    n = np.asarray(shape)
    if dtype == np.float64:
        g = (pts.astype(np.float64) - np.asarray(origin, np.float64)) / float(step)
    else:
        g = ((pts.astype(np.float32) - np.asarray(origin, np.float32)) / np.float32(step)).astype(np.float32)
    i = np.minimum(np.floor(g).astype(np.int64), n - 2)
    return i, (g - i.astype(dtype)).astype(dtype)


def corner_voxels(shape, i):
    """int64 [8, N]: the flat voxel index of corner c = dx*4 + dy*2 + dz of cell i"""
    return np.stack([((i[:, 0] + dx) * shape[1] + i[:, 1] + dy) * shape[2] + i[:, 2] + dz for dx, dy, dz in VC.CORNERS])


def blend64(v, t):
    """(value, A, S) [N, C] float64 from corner values v [8, N, C]"""
    w = VC._weights(t)
    v = v.astype(np.float64)
    return np.einsum("cn,cnk->nk", w, v), np.einsum("cn,cnk->nk", w, np.abs(v)), v.max(axis=0) - v.min(axis=0)


def blend32(v, t32):
    w = VC._weights(t32, np.float32).astype(np.float32)
    acc = w[0][:, None] * v[0]
    for c in range(1, 8):
        acc = VC._fma32(np.broadcast_to(w[c][:, None], v[c].shape), v[c], acc)
    return acc.astype(np.float32)


def grad64(v, t, g, h):
    """(grad [N, 3], B [N, 3], T [N]) of sum(g * rows) from corner values v [8, N, C] and g [N, C]"""
    dw = VC._dweights(t)
    v, g = v.astype(np.float64), np.asarray(g, np.float64)
    grad = np.einsum("acn,cnk,nk->na", dw, v, g) / h
    Bq = np.einsum("acn,cnk,nk->na", np.abs(dw), np.abs(v), np.abs(g)) / h
    T = np.einsum("nk,nk->n", v.max(axis=0) - v.min(axis=0), np.abs(g)) / h
    return grad, Bq, T


def grad32(v, t32, g, step):
    f = np.float32
    g = np.asarray(g, f)
    a = [np.stack([f(1) - t32[:, k], t32[:, k]]).astype(f) for k in range(3)]
    yz = [a[1][j >> 1] * a[2][j & 1] for j in range(4)]
    xz = [a[0][j >> 1] * a[2][j & 1] for j in range(4)]
    xy = [a[0][j >> 1] * a[1][j & 1] for j in range(4)]
    pairs = [(yz, [(4, 0), (5, 1), (6, 2), (7, 3)]), (xz, [(2, 0), (3, 1), (6, 4), (7, 5)]), (xy, [(1, 0), (3, 2), (5, 4), (7, 6)])]
    acc = np.zeros((v.shape[1], 3), f)
    for ax, (wts, pr) in enumerate(pairs):
        d = wts[0][:, None] * (v[pr[0][0]] - v[pr[0][1]])
        for j in range(1, 4):
            d = VC._fma32(np.broadcast_to(wts[j][:, None], d.shape), v[pr[j][0]] - v[pr[j][1]], d)
        for ch in range(d.shape[1]):
            acc[:, ax] = VC._fma32(g[:, ch], d[:, ch], acc[:, ax])
    return (f(f(1) / f(step)) * acc).astype(f)


def virtual_rows(voxel, C, salt=0):
    """float32 [..., C] rows of a volume that exists nowhere: a hash of (voxel, channel) in [-1, 1), for the host emulation of the 32-bit offset"""
    v = np.asarray(voxel, np.uint64)[..., None] * np.uint64(C) + np.arange(C, dtype=np.uint64) + np.uint64(salt)
    v = (v ^ (v >> np.uint64(31))) * np.uint64(0x9E3779B97F4A7C15)
    v = (v ^ (v >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(32)
    return ((v >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def wrapped_voxel(voxel, stride, n):
    """the row a 32-bit `voxel * stride` reads: the float offset wrapped to int32 -- negative from voxel 2^31 / stride on, which is memory in
    front of the array; taken modulo the n rows as a stand-in for 'somewhere else'"""
    off = (np.asarray(voxel, np.int64) * stride + 2 ** 31) % 2 ** 32 - 2 ** 31
    return (off // stride) % n


# ---- mesh -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_volume(kind):
    """'sphere': mesh_ref.sphere(A), every voxel valid: a closed surface.  'clipped': the union of that sphere and a tilted half space, cut by
    the box, with 1 % invalid voxels -> (float32 volume, valid uint8 or None)"""
    import mesh_ref
    vol = mesh_ref.sphere(A)
    if kind == "sphere":
        return vol, None
    normal = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    ax = [np.arange(n, dtype=np.float64) for n in A]
    plane = (ax[0][:, None, None] - 50.3) * normal[0] + (ax[1][None, :, None] - 81.1) * normal[1] + (ax[2][None, None, :] - 60.7) * normal[2]
    vol = np.minimum(vol, plane.astype(np.float32))
    valid = np.ones(vol.size, np.uint8)
    valid[np.random.default_rng(9800).choice(vol.size, vol.size // 100, replace=False)] = 0
    return vol, valid.reshape(A)


@functools.lru_cache(maxsize=None)
def mesh_reference(kind):
    import mesh_ref
    vol, valid = mesh_volume(kind)
    return mesh_ref.reference_mesh(vol, valid=valid)


def mesh_offsets_model(keys, n, mutant=None):
    """where mesh_vertices_kernel puts every vertex: the scanned per-workgroup totals (one more element receives the grand total) plus the rank
    inside the workgroup -> (position of every reference vertex [Nv], the grand total)"""
    nb = (n + MESH_BLOCK - 1) // MESH_BLOCK
    block = (np.asarray(keys) // 3) // MESH_BLOCK
    totals = np.bincount(block, minlength=nb + 1)
    offs = scan_model(totals, mutant)
    rank = np.arange(len(keys)) - (np.cumsum(totals) - totals)[block]
    return offs[block] + rank, int(offs[nb])
