"""The restatement of d3f_volume_peaks (include/d3fields_hip.h, the peaks block) in NumPy, its case generator, and the
references of BakedField.peaks (the k best peaks, the sub-voxel refinement).

Definitions (the contract).  A volume nx x ny x nz, z fastest, flat index (x*ny + y)*nz + z.  slot: None, or an int32 volume as d3f_band_mark
writes it (-1 = no row; the rows ascend with the flat index); with None, row m is voxel m.  mask: None, or one byte per voxel (non-zero =
takes part).  score: float32 [M, K].  radius r in 1..8.  threshold: not NaN, +Inf = none.
  takes part   for column q, voxel v with row m = slot[v]: m >= 0, mask[v] != 0 (when given), score[m, q] < +Inf (false for NaN and +Inf;
               -Inf takes part).
  peak         v takes part, score[m, q] <= threshold, and for every OTHER voxel u that takes part with |u_a - v_a| <= r on all three axes
               the pair (score_u, flat_u) is lexicographically greater than (score_v, flat_v).  The box is spatial and clipped to the volume.
               Scores compare as IEEE floats (-0.0 == +0.0).  The threshold filters peaks; a voxel above it still suppresses others.
  out[m, q] = score[m, q] where the voxel of row m is a peak of column q, +Inf otherwise;  count[q] = the number of peaks of column q.
"""
import functools

import numpy as np

INF = np.float32(np.inf)
MAX_RADIUS = 8


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def voxel_rows(shape, slot):
    """int64 [nx, ny, nz]: the row of every voxel (-1: none)"""
    n = int(np.prod(shape))
    return np.arange(n, dtype=np.int64).reshape(shape) if slot is None else np.asarray(slot, np.int64).reshape(shape)


def takes_part(shape, slot, mask, score):
    """-> (S float32 [nx, ny, nz, K] the score of every voxel's row (0 where it has none), P bool [nx, ny, nz, K] takes part)"""
    rows = voxel_rows(shape, slot)
    has = rows >= 0
    if mask is not None:
        has = has & (np.asarray(mask).reshape(shape) != 0)
    S = np.asarray(score, np.float32)[np.maximum(rows, 0)]
    S = np.where((rows >= 0)[..., None], S, np.float32(0))
    with np.errstate(invalid="ignore"):
        P = has[..., None] & (S < INF)
    return S, P


def peaks_ref(shape, slot, mask, score, r, threshold=np.inf):
    """plain loops over the voxels and, for each, its clipped box -- straight from the definition (the K columns at once)
    -> (out float32 [M, K], count int32 [K], loser int64 [K]); loser counts the voxels that take part and equal the smallest score of their
    box but are no peak because a voxel of the same score has the lower index"""
    nx, ny, nz = shape
    score = np.asarray(score, np.float32)
    M, K = score.shape
    rows = voxel_rows(shape, slot)
    S, P = takes_part(shape, slot, mask, score)
    F = np.arange(nx * ny * nz, dtype=np.int64).reshape(shape)
    out = np.full((M, K), INF, np.float32)
    count, loser = np.zeros(K, np.int32), np.zeros(K, np.int64)
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        for x in range(nx):
            for y in range(ny):
                for z in range(nz):
                    m = rows[x, y, z]
                    if m < 0 or not P[x, y, z].any():
                        continue
                    box = (slice(max(0, x - r), min(nx, x + r + 1)), slice(max(0, y - r), min(ny, y + r + 1)), slice(max(0, z - r), min(nz, z + r + 1)))
                    Sb, Pb, Fb = S[box], P[box], F[box][..., None]
                    s, f = S[x, y, z], F[x, y, z]
                    other = Pb & (Fb != f)
                    greater = (Sb > s) | ((Sb == s) & (Fb > f))
                    beaten = (other & ~greater).any(axis=(0, 1, 2))
                    lower = (other & (Sb < s)).any(axis=(0, 1, 2))
                    peak = P[x, y, z] & ~beaten
                    loser += P[x, y, z] & beaten & ~lower
                    peak &= s <= thr
                    out[m, peak] = score[m, peak]
                    count += peak
    return out, count, loser


def ordered_u32(s):
    """the order-preserving uint32 of a float32 array, -0.0 first made +0.0"""
    s = np.asarray(s, np.float32)
    b = np.where(s == 0, np.float32(0), s).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _window_min(a, r):
    """the minimum over i-r .. i+r along axis 0, clipped to the array (all ones outside)"""
    res = a.copy()
    for d in range(1, min(r, a.shape[0] - 1) + 1):
        res[d:] = np.minimum(res[d:], a[:-d])
        res[:-d] = np.minimum(res[:-d], a[d:])
    return res


def peaks_keys_ref(shape, slot, mask, score, r, threshold=np.inf, wrap=False):
    """the second formulation: packed (ordered float, flat index) uint64 keys, all ones where a voxel does not take part, and three 1-D
    window minima; a voxel is a peak when the box minimum is its own key -> (out, count).  wrap=True takes the z and y windows on flat
    indices (v +- d and v +- d*nz), so that they run on past the end of a z or y line into the next one: the wrong answer the wrap case is
    built to expose."""
    score = np.asarray(score, np.float32)
    M, K = score.shape
    rows = voxel_rows(shape, slot)
    S, P = takes_part(shape, slot, mask, score)
    F = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)[..., None]
    key = np.where(P, (ordered_u32(S).astype(np.uint64) << np.uint64(32)) | F, np.uint64(0xFFFFFFFFFFFFFFFF))
    nx, ny, nz = shape
    if wrap:
        box = _window_min(key.reshape(nx * ny * nz, K), r)
        box = _window_min(box.reshape(nx * ny, nz, K), r)
    else:
        box = np.moveaxis(_window_min(np.moveaxis(key, 2, 0), r), 0, 2)
        box = np.moveaxis(_window_min(np.moveaxis(box, 1, 0), r), 0, 1)
    box = _window_min(box.reshape(nx, ny, nz, K), r)
    with np.errstate(invalid="ignore"):
        peak = P & (box == key) & (S <= np.float32(threshold))
    out = np.full((M, K), INF, np.float32)
    sel = rows >= 0
    out[rows[sel]] = np.where(peak[sel], score[rows[sel]], INF)
    return out, peak.sum(axis=(0, 1, 2)).astype(np.int32)


def topk_ref(out, k, row_voxels=None):
    """the k best peaks of every column of peaks_ref's out: ascending value, ties to the lower row
    -> (voxel int32 [K, k] padded with -1, value float32 [K, k] padded with +Inf)"""
    M, K = out.shape
    voxel, value = np.full((K, k), -1, np.int32), np.full((K, k), INF, np.float32)
    for q in range(K):
        order = np.argsort(out[:, q], kind="stable")
        order = [m for m in order[:k] if out[m, q] < INF]
        for j, m in enumerate(order):
            voxel[q, j] = m if row_voxels is None else row_voxels[m]
            value[q, j] = out[m, q]
    return voxel, value


def refine_ref(shape, slot, mask, score, voxel):
    """the sub-voxel offsets of the hits voxel int32 [K, k] (-1: padding), float64 [K, k, 3] in voxel units, NaN rows for the padding: per axis
    0.5 (f- - f+) / (f- - 2 f0 + f+) in float64, clamped to [-0.5, 0.5]; 0 where a neighbour does not take part or lies outside the volume,
    and 0 where the denominator is not > 0"""
    S, P = takes_part(shape, slot, mask, score)
    K, k = voxel.shape
    off = np.full((K, k, 3), np.nan, np.float64)
    for q in range(K):
        for j in range(k):
            if voxel[q, j] < 0:
                continue
            at = list(np.unravel_index(int(voxel[q, j]), shape))
            f0 = float(S[tuple(at)][q])
            for a in range(3):
                off[q, j, a] = 0.0
                lo, hi = list(at), list(at)
                lo[a] -= 1
                hi[a] += 1
                if lo[a] < 0 or hi[a] >= shape[a] or not P[tuple(lo)][q] or not P[tuple(hi)][q]:
                    continue
                fm, fp = float(S[tuple(lo)][q]), float(S[tuple(hi)][q])
                with np.errstate(invalid="ignore", over="ignore"):
                    den = np.float64(fm) - 2.0 * np.float64(f0) + np.float64(fp)
                    if den > 0:
                        off[q, j, a] = min(0.5, max(-0.5, float(0.5 * (np.float64(fm) - np.float64(fp)) / den)))
    return off


def radius_from_separation(separation, step):
    """r = max(1, ceil(separation / step) - 1) in float64: two peaks then lie at least `separation` apart along some axis"""
    return max(1, int(np.ceil(np.float64(separation) / np.float64(step))) - 1)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def band_slot(shape, fraction, seed):
    """a slot volume as d3f_band_mark writes it: `fraction` of the voxels stored, rows ascending with the flat index -> (slot, voxels [M])"""
    n = int(np.prod(shape))
    stored = np.random.default_rng(seed).random(n) < fraction
    slot = np.where(stored, np.cumsum(stored) - 1, -1).astype(np.int32).reshape(shape)
    return slot, np.flatnonzero(stored).astype(np.int32)


# name: shape, K, r, kind ("float" tie-free | ("int", lo, hi) integer-valued | "inf" | "const" | "wrap"), stored fraction or None, mask fraction
# or None, plant specials, threshold ("none" | "mid": in the middle of the peak values), seed
CASES = {
    "1x1x1": ((1, 1, 1), 3, 1, "float", None, None, False, "none", 1),
    "line r1": ((1, 1, 40), 3, 1, "float", None, None, False, "none", 2),
    "line r3": ((1, 1, 40), 64, 3, "float", None, None, False, "mid", 3),
    "line r8": ((1, 1, 40), 65, 8, "float", None, None, False, "none", 4),
    "image 7x9x1": ((7, 9, 1), 130, 1, "float", None, None, False, "none", 5),
    "ints r1": ((9, 10, 11), 1, 1, ("int", 0, 4), None, None, False, "none", 12),
    "ints r2": ((9, 10, 11), 3, 2, ("int", 0, 40), None, None, False, "mid", 12),
    "5x4x19 r8": ((5, 4, 19), 64, 8, "float", None, None, False, "none", 6),
    "20x17x37 dense": ((20, 17, 37), 3, 2, "float", None, None, True, "mid", 7),
    "20x17x37 band": ((20, 17, 37), 65, 1, "float", 0.3, None, False, "none", 8),
    "20x17x37 mask": ((20, 17, 37), 1, 4, "float", None, 0.5, False, "none", 9),
    "20x17x37 band mask ints": ((20, 17, 37), 3, 3, ("int", 0, 60), 0.3, 0.7, True, "mid", 10),
    "13x9x21 r5": ((13, 9, 21), 8, 5, "float", 0.6, None, False, "none", 11),
    "5x6x20 r6": ((5, 6, 20), 20, 6, "float", None, None, False, "none", 14),
    "6x7x23 r7": ((6, 7, 23), 24, 7, "float", None, 0.8, False, "mid", 15),
    "wrap": ((3, 4, 5), 1, 1, "wrap", None, None, False, "none", 0),
    "all inf": ((6, 5, 9), 3, 1, "inf", None, None, False, "none", 0),
    "constant": ((9, 8, 10), 2, 2, "const", None, None, False, "none", 0),
    "constant band": ((9, 8, 10), 2, 2, "const", 0.5, None, False, "none", 13),
}
RANDOM = [k for k, c in CASES.items() if c[3] == "float" or isinstance(c[3], tuple)]
RANDOM = [k for k in RANDOM if k != "1x1x1"]                     # a single voxel has a single peak per column
INTEGER = [k for k, c in CASES.items() if isinstance(c[3], tuple)]
WRAP_PAIRS = (((1, 1, 4), (1, 2, 0)), ((0, 3, 2), (1, 0, 2)))   # flat neighbours across the end of a z line / a y line; no spatial neighbours at r = 1
SPECIALS = (np.float32(np.nan), INF, -INF, np.float32(-0.0), np.float32(0.0))


def _plant(shape, slot, mask, score, r):
    """specials next to the peaks of the clean data: at the peaks of column 0, in turn, the z+1 neighbour of the peak becomes NaN, +Inf, -Inf;
    or the peak itself -0.0 and its z-1 neighbour (the lower index) +0.0, which then wins the tie of equal zeros; or the other way round"""
    out, _, _ = peaks_ref(shape, slot, mask, score, r)
    rows = voxel_rows(shape, slot)
    score = score.copy()
    planted = 0
    for m in np.flatnonzero(out[:, 0] < INF):
        v = int(np.flatnonzero(rows.reshape(-1) == m)[0])
        x, y, z = np.unravel_index(v, shape)
        kind = planted % 5
        if kind < 3 and z + 1 < shape[2] and rows[x, y, z + 1] >= 0:
            score[rows[x, y, z + 1], :] = SPECIALS[kind]
        elif kind >= 3 and z >= 1 and rows[x, y, z - 1] >= 0:
            score[m, :] = SPECIALS[3 if kind == 3 else 4]
            score[rows[x, y, z - 1], :] = SPECIALS[4 if kind == 3 else 3]
        else:
            continue
        planted += 1
    return score, planted


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(shape, slot, voxels, mask, score [M, K] float32, r, threshold, planted)"""
    shape, K, r, kind, stored, masked, plant, thr, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    slot, voxels = (None, np.arange(n, dtype=np.int32)) if stored is None else band_slot(shape, stored, seed + 100)
    M = len(voxels)
    mask = None if masked is None else (np.random.default_rng(seed + 200).random(shape) < masked).astype(np.uint8)
    if kind == "float":
        score = rng.uniform(1.0, 2.0, size=(M, K)).astype(np.float32)
    elif kind == "inf":
        score = np.full((M, K), INF, np.float32)
    elif kind == "const":
        score = np.full((M, K), 1.5, np.float32)
    elif kind == "wrap":
        score = (10.0 + 0.01 * np.arange(n)).astype(np.float32).reshape(M, K)
        for value, at in enumerate(p for pair in WRAP_PAIRS for p in pair):
            score[np.ravel_multi_index(at, shape), 0] = value
    else:
        if K == 1 and stored is None:            # the issue's figures: default_rng(12) on 9 x 10 x 11, integers 0..3
            score = rng.integers(kind[1], kind[2], size=shape).astype(np.float32).reshape(M, K)
        else:
            score = rng.integers(kind[1], kind[2], size=(M, K)).astype(np.float32)
    planted = 0
    if plant:
        score, planted = _plant(shape, slot, mask, score, r)
    threshold = np.inf
    if thr == "mid":                              # the median of the finite peak values: about half of the peaks pass
        free = peaks_ref(shape, slot, mask, score, r)[0]
        threshold = float(np.median(free[np.isfinite(free)]))
    return dict(shape=shape, slot=slot, voxels=voxels, mask=mask, score=score, r=r, threshold=threshold, planted=planted)


@functools.lru_cache(maxsize=None)
def reference(name):
    """peaks_ref of a case, computed once -> (out, count, loser)"""
    c = case(name)
    return peaks_ref(c["shape"], c["slot"], c["mask"], c["score"], c["r"], c["threshold"])
