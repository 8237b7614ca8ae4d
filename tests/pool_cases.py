"""The contract of d3f_volume_pool (include/d3fields_hip.h, ABI 16) restated in NumPy, and the label volumes the tests pool.

MEMBER      voxel v belongs to component k if label[v] == k with 1 <= k <= K, valid is None or valid[v] != 0, slot is None or slot[v] >= 0.
fold        a radix-256 left-to-right tree of float32 adds: a list of at most 256 rows is ((r0 + r1) + r2) + ..., starting from r0; a longer
            list is cut into consecutive chunks of 256 (a ragged last one) and fold is applied to the list of the chunks' folds.
pool_ref    mean_k = fold(rows of the members of k in ascending flat index) / float32(count_k); the fill row (zeros) for an empty component.
votes_ref   best = 0; for c in 1..C-1: if row[c] > row[best]: best = c -- one vote per member.
moments_ref {Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz} of the members' integer voxel coordinates, int64.
Every float32 operation below is one NumPy float32 operation: IEEE single, round to nearest even."""
import numpy as np

CHUNK = 256
INT32_MIN = -2 ** 31


def fold_levels(n):
    """the number of times a list of n rows is cut before one row is left (1 for n <= 256)"""
    levels = 1
    while n > CHUNK:
        n = (n + CHUNK - 1) // CHUNK
        levels += 1
    return levels


def _fold_chunks(rows):
    """[G, L, C] -> [G, C]: every group's ((r0 + r1) + r2) + ..., L <= 256"""
    acc = rows[:, 0].copy()
    for t in range(1, rows.shape[1]):
        acc = acc + rows[:, t]
    return acc


def fold(rows):
    """[L, C] float32, L >= 1 -> [C]"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.ndim == 2 and rows.shape[0] >= 1
    while rows.shape[0] > CHUNK:
        full = rows.shape[0] // CHUNK
        parts = [_fold_chunks(rows[:full * CHUNK].reshape(full, CHUNK, -1))]
        if rows.shape[0] > full * CHUNK:
            parts.append(_fold_chunks(rows[None, full * CHUNK:]))
        rows = np.concatenate(parts, axis=0)
    return _fold_chunks(rows[None])[0]


def member_lists(label, K, valid=None, slot=None):
    """[K] arrays of ascending flat indices"""
    flat = np.asarray(label).reshape(-1).astype(np.int64)
    ok = (flat >= 1) & (flat <= K)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1) != 0
    if slot is not None:
        ok &= np.asarray(slot).reshape(-1) >= 0
    idx = np.flatnonzero(ok)
    order = np.argsort(flat[idx], kind="stable")
    idx, keys = idx[order], flat[idx][order]
    cuts = np.searchsorted(keys, np.arange(1, K + 2))
    return [idx[cuts[k]:cuts[k + 1]] for k in range(K)]


def counts_ref(label, K, valid=None, slot=None):
    return np.array([len(m) for m in member_lists(label, K, valid, slot)], dtype=np.int32).reshape(K)


def _rows_of(rows, members, slot):
    """rows: [n or M, C] (any strides); the rows of these voxels, through the slot volume where there is one"""
    at = members if slot is None else np.asarray(slot).reshape(-1)[members].astype(np.int64)
    return rows[at]


def pool_ref(label, K, rows, valid=None, slot=None, fill=None):
    rows = np.asarray(rows)
    out = np.zeros((K, rows.shape[1]), dtype=np.float32)
    for k, members in enumerate(member_lists(label, K, valid, slot)):
        if len(members) == 0:
            if fill is not None:
                out[k] = fill
            continue
        out[k] = fold(_rows_of(rows, members, slot)) / np.float32(len(members))
    return out


def argmax_rule(rows):
    """[L, C] -> [L] int: the channel of each row by the rule of the contract, vectorised over the rows"""
    rows = np.asarray(rows, dtype=np.float32)
    best = np.zeros(rows.shape[0], dtype=np.int64)
    at = np.arange(rows.shape[0])
    with np.errstate(invalid="ignore"):
        for c in range(1, rows.shape[1]):
            best[rows[:, c] > rows[at, best]] = c
    return best


def votes_ref(label, K, rows, valid=None, slot=None):
    rows = np.asarray(rows)
    out = np.zeros((K, rows.shape[1]), dtype=np.int32)
    for k, members in enumerate(member_lists(label, K, valid, slot)):
        if len(members):
            out[k] = np.bincount(argmax_rule(_rows_of(rows, members, slot)), minlength=rows.shape[1])
    return out


def moments_ref(label, K, valid=None, slot=None):
    shape = np.asarray(label).shape
    out = np.zeros((K, 9), dtype=np.int64)
    for k, members in enumerate(member_lists(label, K, valid, slot)):
        x, y, z = (a.astype(np.int64) for a in np.unravel_index(members, shape))
        out[k] = [x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(), (z * z).sum()]
    return out


# ---- label volumes --------------------------------------------------------------------------------------------------------------------
def _random_labels(shape, K, seed):
    return np.random.default_rng(seed).integers(0, K + 1, size=shape).astype(np.int32)


def _three_levels():
    """41x40x41: the first 65537 voxels are component 1 (65537 -> 257 -> 2 -> 1: three levels, a ragged chunk at each), the next 255
    component 2, the rest component 3"""
    lab = np.full(41 * 40 * 41, 3, dtype=np.int32)
    lab[:65537] = 1
    lab[65537:65537 + 255] = 2
    return lab.reshape(41, 40, 41)


def _exact_chunks():
    """a component of exactly 256 members and one of exactly 257, interleaved with the background and with each other"""
    rng = np.random.default_rng(7)
    lab = np.zeros(9 * 8 * 10, dtype=np.int32)
    at = rng.permutation(lab.size)
    lab[at[:256]] = 1
    lab[at[256:513]] = 2
    return lab.reshape(9, 8, 10)


def _gaps():
    """K = 9 with components 2, 5, 6 and 9 empty"""
    lab = _random_labels((6, 7, 11), 9, 11)
    lab[np.isin(lab, (2, 5, 6, 9))] = 0
    return lab


def _foreign(shape, K, seed):
    """labels outside 1..K scattered in: -1, K + 1, INT32_MIN"""
    lab = _random_labels(shape, K, seed)
    rng = np.random.default_rng(seed + 1)
    pick = rng.integers(0, 12, size=shape)
    lab[pick == 0] = -1
    lab[pick == 1] = K + 1
    lab[pick == 2] = INT32_MIN
    return lab


# name -> (label volume builder, K)
VOLUMES = {
    "2x3x33": (lambda: _random_labels((2, 3, 33), 3, 1), 3),
    "9x8x10": (lambda: _random_labels((9, 8, 10), 7, 2), 7),
    "65x3x67": (lambda: _random_labels((65, 3, 67), 40, 3), 40),
    "three levels": (_three_levels, 3),
    "256 and 257": (_exact_chunks, 2),
    "gaps": (_gaps, 9),
    "foreign": (lambda: _foreign((9, 8, 10), 7, 5), 7),
    "K 300": (lambda: _random_labels((17, 9, 31), 300, 9), 300),              # two digits of the sort
}
SMALL = ("2x3x33", "9x8x10", "256 and 257", "gaps", "foreign")
CHANNELS = (1, 3, 4, 5, 64, 65, 255, 256, 257, 384, 1024, 4096)
VOTE_CHANNELS = (1, 2, 8, 256)
_cache = {}


def volume(name):
    if name not in _cache:
        build, K = VOLUMES[name]
        lab = build()
        lab.setflags(write=False)
        _cache[name] = (lab, K)
    return _cache[name]


def field_rows(n, C, seed, stride=None):
    """[n, C] float32 rows away from denormals (magnitudes in [0.25, 4), both signs), as a view of a [n, stride] array"""
    rng = np.random.default_rng(seed)
    stride = C if stride is None else stride
    full = (rng.uniform(0.25, 4.0, size=(n, stride)) * rng.choice([-1.0, 1.0], size=(n, stride))).astype(np.float32)
    return full[:, :C]


def vote_rows(n, C, seed):
    """rows on a grid of few values, so that exact ties are common; some rows all equal, some NaN entries (also at channel 0)"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, size=(n, C)).astype(np.float32) * np.float32(0.5)
    rows[rng.random(n) < 0.1] = 1.0
    nan = rng.random((n, C)) < 0.08
    rows[nan] = np.nan
    rows[rng.random(n) < 0.05, 0] = np.nan
    zero = rows == 0
    rows[zero & (rng.random((n, C)) < 0.5)] = -0.0
    return rows
