"""Restatement and case list of the grid segments and row shortcuts (d3f_volume_segments, d3f_path_shorten, include/d3fields_hip.h;
DESIGN.md section 20), shared by tests/test_segment_host.py and tests/test_gpu_segment.py.

The contract, restated:
    free        uint8 [nx, ny, nz], z fastest; any non-zero byte is traversable.  Voxel centres sit at integer coordinates of index space.
    segment     of two voxels a, b: {a + t (b - a), 0 <= t <= 1}
    touched     strict: the closed cube [v - 1/2, v + 1/2]^3 meets the segment; cut corners (open): the open cube meets it
    the walk    n_i = |b_i - a_i|, s_i = sign(b_i - a_i), k_i = 0, cur = a; axis i crosses its next plane at t_i = (2 k_i + 1) / (2 n_i).  Event 0
                touches {a}.  Every further event takes the set E of the axes with k_i < n_i that share the smallest t_i; under the strict rule
                with |E| >= 2 it touches cur + sum of s_i e_i over every non-empty proper subset of E; then cur and k advance on all of E and
                the event touches the new cur.
    clear       1 when every touched voxel is free
    last        cur of the last event before the first event that touches a non-free voxel; b if clear; -1 if event 0 is blocked
    blocked     the smallest flat index among the non-free voxels of that first blocking event; -1 if clear
    min_value, min_voxel   (with an int32 value volume) over all voxels touched by the events before the first blocking event; among equal
                minima the earliest event, then the smallest flat index within it; INT32_MAX, -1 if event 0 is blocked
    a or b outside 0 .. nx*ny*nz - 1: clear = 0, last = blocked = min_voxel = -1, min_value = INT32_MAX
    shortening  anchors i_0 = 0; from anchor i the next is the LARGEST j in i + 1 .. min(L - 1, i + max_span) whose segment (p_i, p_j) is
                clear, j = i + 1 if there is none; until L - 1.  L = length clamped into 0 .. row_len.

touched_ref is the definition: the cube test on every voxel of the box, in fractions.Fraction.  walk_ref follows the events; segment_ref and
shorten_ref are plain loops over it.  Nothing here shares code or structure with the kernels beyond the event rule itself, which
test_segment_host.py checks against touched_ref.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np

import ccl_cases as CC
import geodesic_cases as GC

INT32_MAX = 2 ** 31 - 1
POISON = CC.POISON


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def touched_ref(a, b, strict):
    """the set of voxels (x, y, z) whose closed (strict) or open cube meets the segment a -> b: the slab test per axis in exact rationals"""
    a, b = tuple(int(c) for c in a), tuple(int(c) for c in b)
    out = set()
    for v in itertools.product(*[range(min(p, q), max(p, q) + 1) for p, q in zip(a, b)]):
        if any(p == q and p != c for p, q, c in zip(a, b, v)):      # a constant coordinate at least 1 > 1/2 away: outside under both rules
            continue
        # per moving axis the t interval in which the coordinate lies within 1/2 of c: closed or open as the cube is
        slabs = [sorted((Fraction(2 * (c - p) - 1, 2 * (q - p)), Fraction(2 * (c - p) + 1, 2 * (q - p)))) for p, q, c in zip(a, b, v) if p != q]
        if not slabs:                                               # a == b == v
            out.add(v)
            continue
        lo, hi = max(t0 for t0, _ in slabs), min(t1 for _, t1 in slabs)
        if strict:
            meets = max(lo, Fraction(0)) <= min(hi, Fraction(1))   # closed intervals and the closed [0, 1]
        else:
            meets = lo < hi and lo < 1 and hi > 0                   # the open interval (lo, hi) against the closed [0, 1]
        if meets:
            out.add(v)
    return out


def walk_ref(a, b, strict):
    """-> the events [(t Fraction, [touched voxels], cur after the event)], event 0 first"""
    a, b = tuple(int(c) for c in a), tuple(int(c) for c in b)
    n = [abs(q - p) for p, q in zip(a, b)]
    s = [(q > p) - (q < p) for p, q in zip(a, b)]
    k = [0, 0, 0]
    cur = list(a)
    events = [(Fraction(0), [a], a)]
    while True:
        live = [i for i in range(3) if k[i] < n[i]]
        if not live:
            break
        t = min(Fraction(2 * k[i] + 1, 2 * n[i]) for i in live)
        E = [i for i in live if (2 * k[i] + 1) * t.denominator == t.numerator * 2 * n[i]]
        touched = []
        if strict and len(E) >= 2:
            for r in range(1, len(E)):
                for sub in itertools.combinations(E, r):
                    v = list(cur)
                    for i in sub:
                        v[i] += s[i]
                    touched.append(tuple(v))
        for i in E:
            cur[i] += s[i]
            k[i] += 1
        touched.append(tuple(cur))
        events.append((t, touched, tuple(cur)))
    assert tuple(cur) == b and len(events) <= sum(n) + 1
    return events


def _coords(flat, shape):
    return tuple(int(c) for c in np.unravel_index(int(flat), shape))


def _flat(v, shape):
    return (v[0] * shape[1] + v[1]) * shape[2] + v[2]


def segment_ref(free, value, a, b, strict):
    """one segment of flat indices a, b -> (clear, last, blocked, min_value, min_voxel); the last two are INT32_MAX / -1 without value"""
    shape = free.shape
    ff = free.reshape(-1)
    vv = None if value is None else value.reshape(-1)
    if not (0 <= a < ff.size and 0 <= b < ff.size):
        return 0, -1, -1, INT32_MAX, -1
    last, best, at = -1, INT32_MAX, -1
    for _, touched, cur in walk_ref(_coords(a, shape), _coords(b, shape), strict):
        idx = sorted(_flat(v, shape) for v in touched)
        bad = [i for i in idx if ff[i] == 0]
        if bad:
            return 0, last, bad[0], best, at
        if vv is not None:
            for i in idx:                                      # ascending flat index, strict <: the earliest event, then the smallest index
                if at < 0 or int(vv[i]) < best:
                    best, at = int(vv[i]), i
        last = _flat(cur, shape)
    return 1, last, -1, best, at


def segments_ref(free, value, a, b, strict):
    """arrays as the entry point writes them: (clear uint8, last, blocked, min_value, min_voxel int32)"""
    rows = [segment_ref(free, value, int(p), int(q), strict) for p, q in zip(a, b)]
    cols = list(zip(*rows)) if rows else [[]] * 5
    return tuple(np.array(c, dtype=np.uint8 if k == 0 else np.int32) for k, c in enumerate(cols))


def clear_ref(free, a, b, strict, memo=None):
    """clear of one segment; memo, if given, is a dict of this (free, strict) that keeps the answers"""
    if memo is None:
        return segment_ref(free, None, int(a), int(b), strict)[0]
    key = (int(a), int(b))
    if key not in memo:
        memo[key] = segment_ref(free, None, key[0], key[1], strict)[0]
    return memo[key]


def shorten_ref(free, row, length, max_span, strict, note=None, memo=None):
    """one row -> (index list, voxel list).  note, if given, collects the anchors i whose chosen j lies beyond a blocked nearer j."""
    L = min(max(int(length), 0), len(row))
    if L == 0:
        return [], []
    index = [0]
    i = 0
    while i < L - 1:
        top = min(L - 1, i + max_span)
        nxt = i + 1
        for j in range(top, i, -1):                            # the largest clear j: the first one met from the far end
            if clear_ref(free, row[i], row[j], strict, memo):
                nxt = j
                break
        if note is not None and nxt > i + 1 and any(not clear_ref(free, row[i], row[j], strict, memo) for j in range(i + 1, nxt)):
            note.append(i)
        i = nxt
        index.append(i)
    return index, [int(row[k]) for k in index]


def shorten_rows_ref(free, rows, lengths, max_span, strict, memo=None):
    """arrays as the entry point writes them: (out_index, out_voxels int32 [n, row_len] padded with -1, out_count int32 [n])"""
    rows = np.asarray(rows, np.int32)
    n, row_len = rows.shape
    oi = np.full((n, row_len), -1, np.int32)
    ov = np.full((n, row_len), -1, np.int32)
    oc = np.zeros(n, np.int32)
    for r in range(n):
        index, vox = shorten_ref(free, rows[r].tolist(), lengths[r], max_span, strict, memo=memo)
        oc[r] = len(index)
        oi[r, :len(index)] = index
        ov[r, :len(index)] = vox
    return oi, ov, oc


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# random volumes: name -> (shape, free share).  Dense enough that the clear share of 400 random segments stays inside [0.2, 0.8]
RANDOM = {"7x9x1 90%": ((7, 9, 1), 0.90), "1x1x130 99%": ((1, 1, 130), 0.99), "2x3x130 98%": ((2, 3, 130), 0.98), "24x20x28 97%": ((24, 20, 28), 0.97),
          "50x50x53 99%": ((50, 50, 53), 0.99)}
RANDOM_3D = ["24x20x28 97%", "50x50x53 99%"]
N_PAIRS = 400
SEGMENT_VOLUMES = ["1x1x1"] + list(RANDOM) + ["all free", "none free"]


@functools.lru_cache(maxsize=None)
def _volumes():
    """every segment volume, drawn in the order of SEGMENT_VOLUMES from one default_rng(11)"""
    rng = np.random.default_rng(11)
    out = {}
    for name in SEGMENT_VOLUMES:
        if name in RANDOM:
            shape, share = RANDOM[name]
            n = int(np.prod(shape))
            free = np.zeros(n, np.uint8)
            k = max(1, int(round(share * n)))
            free[rng.choice(n, k, replace=False)] = rng.integers(1, 256, k)          # any non-zero byte is traversable
        elif name == "1x1x1":
            shape, free = (1, 1, 1), np.ones(1, np.uint8)
        elif name == "all free":
            shape, free = (5, 4, 6), np.full(120, 9, np.uint8)
        else:
            assert name == "none free"
            shape, free = (5, 4, 6), np.zeros(120, np.uint8)
        n = int(np.prod(shape))
        value = rng.integers(0, 51, n).astype(np.int32)             # 0..50: ties occur
        a = rng.integers(0, n, N_PAIRS).astype(np.int32)
        b = rng.integers(0, n, N_PAIRS).astype(np.int32)
        out[name] = (free.reshape(shape), value.reshape(shape), a, b)
        for t in out[name]:
            t.setflags(write=False)
    return out


def volume(name):
    """-> (free uint8 [nx, ny, nz], value int32 [nx, ny, nz], a int32 [N], b int32 [N]), read-only"""
    return _volumes()[name]


@functools.lru_cache(maxsize=None)
def volume_reference(name, strict, with_value):
    free, value, a, b = volume(name)
    out = segments_ref(free, value if with_value else None, a, b, strict)
    for t in out:
        t.setflags(write=False)
    return out


# tie cases: (shape, a, b, the side voxels of the segment's edge / corner crossings); each is blocked in turn, strict against open
TIES = {
    "(2,2,0)": ((3, 3, 1), (0, 0, 0), (2, 2, 0), [(1, 0, 0), (0, 1, 0), (2, 1, 0), (1, 2, 0)]),
    "(3,1,0)": ((4, 2, 1), (0, 0, 0), (3, 1, 0), [(1, 1, 0), (2, 0, 0)]),
    "(1,1,1)": ((2, 2, 2), (0, 0, 0), (1, 1, 1), [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]),
}

# ---- rows ----------------------------------------------------------------------------------------------------------------------------
PILLAR_SHAPE, PILLAR_GOAL = (28, 20, 3), (26, 3, 1)
PILLAR_STARTS = [(1, 10, 1), (1, 2, 0), (5, 18, 2), (17, 9, 1)]


def pillar_free():
    free = np.ones(PILLAR_SHAPE, np.uint8)
    free[10:16, 6:14, :] = 0
    free[20:22, 0:9, :] = 0
    return free


@functools.lru_cache(maxsize=None)
def pillar_rows():
    """-> (free, rows int32 [4, L], length int32 [4]): the travel paths of the pillar scene under connectivity 26, weights (3, 4, 5)"""
    free = pillar_free()
    cost, _ = GC.travel_ref(free, [_flat(PILLAR_GOAL, PILLAR_SHAPE)], 26, (3, 4, 5))
    nxt = GC.next_ref(cost, 26, (3, 4, 5))
    rows, length, reached = GC.follow_ref(nxt, [_flat(s, PILLAR_SHAPE) for s in PILLAR_STARTS], sum(PILLAR_SHAPE))
    assert reached.all()
    for t in (free, rows, length):
        t.setflags(write=False)
    return free, rows, length


@functools.lru_cache(maxsize=None)
def serpentine_rows(connectivity):
    """-> (free, rows int32 [1, L], length int32 [1]): the path from the far end of the 12^3 serpentine of geodesic_cases to its seed.
    Not three independent cases: connectivity 18 and 26 give the SAME row (397 voxels; test_segment_host.py asserts it), and on it
    the strict and the open rule keep the same anchors at every max_span.  Only the row of connectivity 6 (467 voxels) tells the rules apart, at
    max_span 2 (252 anchors strict, 234 open); the pillar scene and the random rows are what separates the rules for rows."""
    free, seeds, _ = GC.case("serpentine")
    w = dict(GC.CONFIGS)[connectivity]
    cost, nxt, _ = GC.reference("serpentine", connectivity, w)
    c = cost.reshape(-1)
    far = int(np.argmax(np.where(c == GC.INT32_MAX, -1, c)))
    rows, length, reached = GC.follow_ref(nxt, [far], free.size)
    L = int(length[0])
    assert reached.all()
    rows = np.ascontiguousarray(rows[:, :L])
    for t in (rows, length):
        t.setflags(write=False)
    return free, rows, length


RANDOM_ROW_LENGTHS = [0, 1, 2, 64, 65, 200]
RANDOM_ROW_LEN = 208                                            # padded: every row is shorter than the row length


@functools.lru_cache(maxsize=None)
def random_rows():
    """-> (free of '24x20x28 97%', rows int32 [6, 208], length int32 [6]): arbitrary voxel sequences (not paths), rows padded with junk beyond
    their length, an entry of -1 inside the row of 65 and one past the volume inside the row of 200"""
    free = volume("24x20x28 97%")[0]
    rng = np.random.default_rng(12)
    open_ = np.flatnonzero(free.reshape(-1))
    rows = rng.choice(open_, (len(RANDOM_ROW_LENGTHS), RANDOM_ROW_LEN)).astype(np.int32)
    # neighbouring entries a few voxels apart, so that a share of the segments is clear: a random walk of short jumps, clipped to the volume
    for r in range(rows.shape[0]):
        p = np.array(np.unravel_index(int(rows[r, 0]), free.shape))
        for k in range(1, RANDOM_ROW_LEN):
            p = np.clip(p + rng.integers(-7, 8, 3), 0, np.array(free.shape) - 1)
            rows[r, k] = _flat(p.tolist(), free.shape)
    rows[4, 30] = -1
    rows[5, 100] = free.size
    length = np.array(RANDOM_ROW_LENGTHS, np.int32)
    for t in (rows, length):
        t.setflags(write=False)
    return free, rows, length


ROW_SETS = {"pillar": pillar_rows, "random": random_rows, "serpentine 6": lambda: serpentine_rows(6), "serpentine 18": lambda: serpentine_rows(18),
            "serpentine 26": lambda: serpentine_rows(26)}
_CLEAR_MEMO = {}                                                # (row set, rule) -> {(a, b): clear}: every max_span asks for the same segments


@functools.lru_cache(maxsize=None)
def shorten_reference(which, max_span, strict):
    free, rows, length = ROW_SETS[which]()
    out = shorten_rows_ref(free, rows, length, max_span, strict, _CLEAR_MEMO.setdefault((which, strict), {}))
    for t in out:
        t.setflags(write=False)
    return out
