"""NumPy restatement and case generator of the merge of two baked fields (d3f_volume_merge_select / d3f_volume_merge_rows,
include/d3fields_hip_ext.h), shared by tests/test_merge_host.py and tests/test_gpu_merge.py.

The contract, one NumPy operation per rounded operation, everything float32.  a is the older field, b the newer; the flat index is
(x*ny + y)*nz + z.  A side is usable at q iff valid[q], dist[q] is not NaN and 0 < w[q] < inf (w: the side's weight volume or, for a
scalar, that scalar everywhere).  dist / weight of a voxel that is not valid are never looked at: the generator poisons them with NaN.
    kind 0 NONE   neither usable                  dist 1e3, weight 0, beta 0, valid 0
    kind 1 KEEP   only a                          da, wa, beta 0
    kind 2 NEW    only b                          db, wb, beta 1
    kind 3 BLEND  both, not |da - db| > gap       s = wa + wb;  beta = wb / s;  dist = da + beta*(db - da);  weight = min(s, w_max)
    kind 4 RESET  both, |da - db| > gap           db, wb, beta 1
Rows of a listed voxel: a has a row iff kind in {1, 3} and (a dense or slot_a[q] >= 0), b iff kind in {2, 3, 4} and (b dense or
slot_b[q] >= 0); both -> a_c + beta*(b_c - a_c); one -> that row's bits (a half widened exactly); none -> the fill row, known 0.
"""
import numpy as np

NONE, KEEP, NEW, BLEND, RESET = 0, 1, 2, 3, 4
KINDS = (NONE, KEEP, NEW, BLEND, RESET)
SENTINEL = np.float32(1e3)
F = np.float32
INF = F(np.inf)


def _weights(w, shape):
    """a weight volume as it is, a scalar as a volume of that scalar"""
    if isinstance(w, np.ndarray):
        assert w.dtype == np.float32 and w.shape == tuple(shape)
        return w
    return np.full(shape, F(w), np.float32)


def usable(dist, valid, w):
    v = valid != 0
    d = np.where(v, dist, F(0))                      # (what lies behind an invalid voxel is not looked at)
    ww = np.where(v, _weights(w, dist.shape), F(0))
    with np.errstate(invalid="ignore"):
        return v & ~np.isnan(d) & (ww > 0) & (ww < INF)


def select_ref(da, va, wa, db, vb, wb, w_max=np.inf, gap=np.inf):
    """-> dict(dist float32, weight float32, beta float32, valid uint8, kind uint8), volumes of da's shape"""
    assert da.dtype == np.float32 and db.dtype == np.float32 and da.shape == db.shape
    w_max, gap = F(w_max), F(gap)
    assert w_max > 0 and gap >= 0
    ua, ub = usable(da, va, wa), usable(db, vb, wb)
    one = F(1)
    a, b = np.where(ua, da, F(0)), np.where(ub, db, F(0))
    pa, pb = np.where(ua, _weights(wa, da.shape), one), np.where(ub, _weights(wb, da.shape), one)
    with np.errstate(over="ignore", invalid="ignore"):
        both = ua & ub
        reset = both & (np.abs(a - b) > gap)
        blend = both & ~reset
        s = pa + pb                                  # one rounding
        beta = pb / s                                # one IEEE division (s = inf: 0)
        diff = b - a
        step = beta * diff
        mixed = a + step                             # three roundings in all
        capped = np.minimum(s, w_max)
    kind = np.zeros(da.shape, np.uint8)
    kind[ua & ~ub], kind[ub & ~ua], kind[blend], kind[reset] = KEEP, NEW, BLEND, RESET
    from_b = (kind == NEW) | (kind == RESET)
    dist = np.where(kind == KEEP, a, np.where(from_b, b, np.where(blend, mixed, SENTINEL))).astype(np.float32)
    weight = np.where(kind == KEEP, pa, np.where(from_b, pb, np.where(blend, capped, F(0)))).astype(np.float32)
    out_beta = np.where(from_b, one, np.where(blend, beta, F(0))).astype(np.float32)
    return {"dist": dist, "weight": weight, "beta": out_beta, "valid": (kind != NONE).astype(np.uint8), "kind": kind}


def select_loop(da, va, wa, db, vb, wb, w_max=np.inf, gap=np.inf):
    """the same contract, one voxel at a time with float32 scalars"""
    shape = da.shape
    wa, wb = _weights(wa, shape).reshape(-1), _weights(wb, shape).reshape(-1)
    da, db, va, vb = da.reshape(-1), db.reshape(-1), va.reshape(-1), vb.reshape(-1)
    w_max, gap = F(w_max), F(gap)
    n = da.size
    out = {"dist": np.empty(n, np.float32), "weight": np.empty(n, np.float32), "beta": np.empty(n, np.float32), "valid": np.empty(n, np.uint8),
           "kind": np.empty(n, np.uint8)}
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(n):
            ua = ub = False
            if va[q]:
                ua = bool(not np.isnan(da[q]) and wa[q] > 0 and wa[q] < INF)
            if vb[q]:
                ub = bool(not np.isnan(db[q]) and wb[q] > 0 and wb[q] < INF)
            if ua and ub:
                if np.abs(F(da[q] - db[q])) > gap:
                    res = (RESET, db[q], wb[q], F(1))
                else:
                    s = F(wa[q] + wb[q])
                    beta = F(wb[q] / s)
                    res = (BLEND, F(da[q] + F(beta * F(db[q] - da[q]))), s if s < w_max else w_max, beta)
            elif ua:
                res = (KEEP, da[q], wa[q], F(0))
            elif ub:
                res = (NEW, db[q], wb[q], F(1))
            else:
                res = (NONE, SENTINEL, F(0), F(0))
            out["kind"][q], out["dist"][q], out["weight"][q], out["beta"][q] = res
            out["valid"][q] = res[0] != NONE
    return {k: v.reshape(shape) for k, v in out.items()}


def _side(data, slot, n):
    """(float32 [rows, C] widened exactly, row index per voxel [n] with -1 for none) of a dense [nx,ny,nz,C] or banded [M,C] set"""
    if slot is None:
        assert data.ndim == 4 and int(np.prod(data.shape[:3])) == n
        return data.reshape(n, data.shape[3]).astype(np.float32), np.arange(n, dtype=np.int64)
    assert data.ndim == 2 and slot.size == n
    return data.astype(np.float32), slot.reshape(-1).astype(np.int64)


def rows_ref(kind, beta, data_a, data_b, fill=None, voxels=None, slot_a=None, slot_b=None):
    """-> (float32 [m, C], known uint8 [m]).  data: float32 or float16; dense [nx,ny,nz,C] with slot None, banded [M,C] with slot int32
    [nx,ny,nz] (an empty band: data [0, C] and a slot volume of -1)"""
    n = kind.size
    ra, ia = _side(data_a, slot_a, n)
    rb, ib = _side(data_b, slot_b, n)
    C = ra.shape[1]
    assert rb.shape[1] == C
    q = np.arange(n, dtype=np.int64) if voxels is None else np.asarray(voxels, np.int64)
    inside = (q >= 0) & (q < n)
    qq = np.where(inside, q, 0)
    k = np.where(inside, kind.reshape(-1)[qq].astype(np.int64), -1)
    has_a = ((k == KEEP) | (k == BLEND)) & (ia[qq] >= 0)
    has_b = ((k == NEW) | (k == BLEND) | (k == RESET)) & (ib[qq] >= 0)
    a = ra[np.where(has_a, ia[qq], 0)] if ra.shape[0] else np.zeros((q.size, C), np.float32)
    b = rb[np.where(has_b, ib[qq], 0)] if rb.shape[0] else np.zeros((q.size, C), np.float32)
    out = np.empty((q.size, C), np.float32)
    out[...] = np.zeros(C, np.float32) if fill is None else np.asarray(fill, np.float32)
    only_a, only_b, both = has_a & ~has_b, has_b & ~has_a, has_a & has_b
    out.view(np.uint32)[only_a] = a.view(np.uint32)[only_a]          # bit copies
    out.view(np.uint32)[only_b] = b.view(np.uint32)[only_b]
    bt = beta.reshape(-1)[qq][both][:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        diff = b[both] - a[both]
        step = bt * diff
        out[both] = a[both] + step
    return out, (has_a | has_b).astype(np.uint8)


def rows_loop(kind, beta, data_a, data_b, fill=None, voxels=None, slot_a=None, slot_b=None):
    """the same, one voxel and one channel at a time"""
    n = kind.size
    ra, ia = _side(data_a, slot_a, n)
    rb, ib = _side(data_b, slot_b, n)
    C = ra.shape[1]
    q = list(range(n)) if voxels is None else [int(v) for v in voxels]
    out, known = np.empty((len(q), C), np.float32), np.zeros(len(q), np.uint8)
    kind, beta = kind.reshape(-1), beta.reshape(-1)
    fill = np.zeros(C, np.float32) if fill is None else np.asarray(fill, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j, v in enumerate(q):
            k = int(kind[v]) if 0 <= v < n else -1
            has_a = k in (KEEP, BLEND) and ia[v] >= 0
            has_b = k in (NEW, BLEND, RESET) and ib[v] >= 0
            known[j] = has_a or has_b
            for c in range(C):
                if has_a and has_b:
                    out[j, c] = F(ra[ia[v], c] + F(beta[v] * F(rb[ib[v], c] - ra[ia[v], c])))
                elif has_a or has_b:
                    out[j:j + 1, c:c + 1].view(np.uint32)[...] = (ra[ia[v], c:c + 1] if has_a else rb[ib[v], c:c + 1]).view(np.uint32)
                else:
                    out[j, c] = fill[c]
    return out, known


# ---- cases ------------------------------------------------------------------------------------------------------------------------
GAP = F(0.5)            # of every random case; planted ties differ by exactly this
W_MAX = F(5.0)          # of every random case: weights lie in [0.5, 4), so some sums are capped and some are not
HUGE = F(3e38)          # two of these overflow


def _freeze(cs):
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def _rows(rng, n, C, half):
    """[n, C] rows with -0, subnormals and (float32 only) non-dyadic fractions; a half set holds values a half holds exactly"""
    r = rng.uniform(-2, 2, size=(n, C)).astype(np.float16 if half else np.float32)
    flat = r.reshape(-1)
    idx = rng.permutation(flat.size)
    third = max(flat.size // 8, 1)
    flat[idx[:third]] = -0.0
    tiny = np.float16(6e-8) if half else np.float32(1e-41)             # subnormal in either format
    flat[idx[third:2 * third]] = tiny * (1 + (np.arange(min(third, flat.size - third)) % 5)).astype(flat.dtype)
    return r


def random_case(shape, C, seed, banded_a=False, banded_b=False, half_a=False, half_b=False):
    """Two fields on `shape` with every kind planted on a fifth of the voxels each (test_merge_host.py asserts at least 5 %), and:
    NaN dist in valid voxels; NaN, 0, negative and inf weights; NaN dist / weights / rows at invalid voxels; -0 and subnormal row
    entries; ties |da - db| == GAP exactly; a pair with wa + wb overflowing; quiet NaN payloads in rows that are copied, not blended.
    A banded side stores about half the voxels; over the kind-3 voxels the stored patterns (a, b) cycle so that a quarter or more
    have exactly one banded row and a quarter or more none."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    want = np.empty(n, np.int64)
    want[rng.permutation(n)] = np.arange(n) % 5
    da = rng.uniform(-1, 1, n).astype(np.float32)
    db = np.empty(n, np.float32)
    wa = rng.uniform(0.5, 4, n).astype(np.float32)
    wb = rng.uniform(0.5, 4, n).astype(np.float32)
    va, vb = np.ones(n, np.uint8), np.ones(n, np.uint8)
    near = rng.uniform(-0.4, 0.4, n).astype(np.float32)
    far = (rng.uniform(0.6, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    db[...] = da + np.where(want == RESET, far, near)
    nan = F(np.nan)
    tie = overflow = equal = -1
    for rank, q in enumerate(np.flatnonzero(want == BLEND)):
        if rank % 7 == 0:                            # an exact tie: multiples of 1/64, |da - db| == GAP, not > GAP
            da[q] = F(int(rng.integers(-32, 32)) / 64.0)
            db[q] = da[q] + (GAP if rank % 2 else -GAP)
            tie = q
        elif rank % 7 == 1:
            wa[q] = wb[q] = HUGE                     # s = inf: beta 0, weight w_max
            overflow = q
        elif rank % 7 == 2:
            db[q] = da[q]                            # exact where da == db
            equal = q
    bad_w = (nan, F(0), F(-1.5), INF)
    for rank, q in enumerate(np.flatnonzero(want == NONE)):
        r = rank % 4
        if r == 0:
            va[q] = vb[q] = 0
        elif r == 1:
            da[q], vb[q] = nan, 0
        elif r == 2:
            wa[q], wb[q] = bad_w[(rank // 4) % 4], bad_w[(rank // 4 + 1) % 4]
        else:
            va[q], db[q] = 0, nan
    for kind_, (d_other, v_other, w_other) in ((KEEP, (db, vb, wb)), (NEW, (da, va, wa))):
        for rank, q in enumerate(np.flatnonzero(want == kind_)):
            r = rank % 3
            if r == 0:
                v_other[q] = 0
            elif r == 1:
                d_other[q] = nan
            else:
                w_other[q] = bad_w[(rank // 3) % 4]
    for d, v, w in ((da, va, wa), (db, vb, wb)):     # what is not valid is poison
        d[v == 0] = nan
        w[v == 0] = nan
    shape = tuple(shape)
    cs = {"shape": shape, "C": C, "da": da.reshape(shape), "va": va.reshape(shape), "wa": wa.reshape(shape), "db": db.reshape(shape), "vb": vb.reshape(shape),
          "wb": wb.reshape(shape), "w_max": W_MAX, "gap": GAP, "tie": int(tie), "overflow": int(overflow), "equal": int(equal),
          "fill": (np.arange(C) + 0.25).astype(np.float32)}
    ref = select_ref(cs["da"], cs["va"], cs["wa"], cs["db"], cs["vb"], cs["wb"], W_MAX, GAP)
    kind = ref["kind"].reshape(-1)
    blended = np.flatnonzero(kind == BLEND)
    for side, banded, half, valid in (("a", banded_a, half_a, va), ("b", banded_b, half_b, vb)):
        rows = _rows(rng, n, C, half)
        rows[valid == 0] = np.nan                    # poison
        copied = np.flatnonzero((valid != 0) & (kind != BLEND))
        payload = np.uint16(0x7e01) if half else np.uint32(0x7fc00123)       # a quiet NaN with a payload, where rows are only ever copied
        if copied.size:
            rows.view(payload.dtype)[copied[::3], 0] = payload
        if banded:
            stored = rng.permutation(n) % 2 == 0
            pattern = (1, 1, 0, 0) if side == "a" else (1, 0, 1, 0)
            if not (banded_a and banded_b):
                pattern = (1, 0, 1, 0)
            stored[blended] = [pattern[r % 4] for r in range(blended.size)]
            voxels = np.flatnonzero(stored).astype(np.int32)
            slot = np.where(stored, np.cumsum(stored) - 1, -1).astype(np.int32).reshape(shape)
            cs["rows_" + side], cs["slot_" + side], cs["voxels_" + side] = np.ascontiguousarray(rows[stored]), slot, voxels
        else:
            cs["rows_" + side], cs["slot_" + side], cs["voxels_" + side] = rows.reshape(shape + (C,)), None, None
    return _freeze(cs)


# (shape, C, seed, banded_a, banded_b, half_a, half_b): the random cases of both test files.  Every kind covers a fifth of the voxels by
# construction; the seeds are the ones the host test has checked the conditions for through the restatement.
RANDOM = [((2, 2, 2), 3, 1, False, False, False, False), ((5, 4, 6), 1, 2, False, False, False, False), ((9, 8, 10), 16, 3, False, False, True, False),
          ((17, 12, 11), 20, 4, False, False, False, True), ((5, 4, 6), 18, 5, True, False, False, False), ((9, 8, 10), 3, 6, False, True, True, True),
          ((9, 8, 10), 64, 7, True, True, False, False), ((17, 12, 11), 16, 8, True, True, True, False)]


def case_id(spec):
    shape, C, seed, ba, bb, ha, hb = spec
    return "%dx%dx%d C=%d %s%s+%s%s" % (shape + (C, "band" if ba else "dense", " f16" if ha else "", "band" if bb else "dense", " f16" if hb else ""))


def voxel_list(n, seed):
    """a shuffled list with duplicates and entries outside the volume"""
    rng = np.random.default_rng(seed)
    lst = np.concatenate([rng.permutation(n)[: max(n * 2 // 3, 1)], rng.integers(0, n, size=max(n // 4, 2)), [-1, n, n + 7, -2 ** 31, 2 ** 31 - 1]])
    lst = lst[rng.permutation(lst.size)]
    return np.concatenate([lst, lst[:1]]).astype(np.int32)


def field_pair(shape=(24, 20, 16), C=20, seed=11, step=0.004):
    """Two observations of one tilted plane for BakedField.merge: dist in world units clamped to +-3 steps; a sees it everywhere but for 2 %
    holes, b sees it shifted by a quarter step with a box of voxels invalidated (an occluder) and a patch where its surface has moved by
    two steps (for reset_gap).  -> dict(shape, step, da, va, db, vb, rows_a, rows_b [nx,ny,nz,C] float32, box, moved (slices))"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    X, Y, Z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    h = np.float32(step)
    plane = (Z - (nz / 2 - 0.37) + 0.11 * (X - nx / 2) - 0.07 * (Y - ny / 2)) / np.sqrt(1 + 0.11 ** 2 + 0.07 ** 2)
    da = (np.clip(plane, -3, 3) * h).astype(np.float32)
    db = (np.clip(plane - 0.25, -3, 3) * h).astype(np.float32)
    moved = (slice(2, 8), slice(3, 9), slice(0, nz))
    db[moved] = (np.clip(plane[moved] - 2.0, -3, 3) * h).astype(np.float32)
    va = rng.uniform(size=shape) > 0.02
    vb = rng.uniform(size=shape) > 0.02
    box = (slice(12, 20), slice(6, 15), slice(3, 13))
    vb[box] = False
    da[~va], db[~vb] = np.nan, np.nan
    rows_a = rng.normal(size=shape + (C,)).astype(np.float32)
    rows_b = (rows_a + 0.1 * rng.normal(size=shape + (C,))).astype(np.float32)
    rows_a[~va], rows_b[~vb] = np.nan, np.nan
    return _freeze({"shape": shape, "step": step, "C": C, "da": da, "va": va, "db": db, "vb": vb, "rows_a": rows_a, "rows_b": rows_b, "box": box, "moved": moved})
