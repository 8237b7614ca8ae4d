"""Grid segments and row shortcuts on the device (d3f_volume_segments, d3f_path_shorten, csrc/segment_kernels.hip; BakedField.straight /
shortcut) against the restatement of tests/segment_cases.py: integer data, equality of every output byte, no tolerance, from poisoned
buffers, and identical bytes from a second run.

What each assert is there to catch:
  a tie of two or three axes resolved as one axis after the other, side voxels missed or counted under the wrong rule      the tie cases, the 3-D volumes
  a sign or an axis mixed up in the walk                                                                                    the eight octants
  a read outside the box of a and b (and so outside the volume)                                                             1x1x1, the image, the line
  an output the kernel does not write, or writes where it should not                                                        poison, each output NULL in turn
  the tie rule of the minimum (earliest event, then smallest index)                                                         value in 0..50
  a scan that stops at the first blocked candidate, a chunk boundary off by one, an anchor beyond max_span                 pillar, serpentine, max_span 64 / 65
  a wave that reads past its row's length, a partial workgroup                                                              padded rows, 1 / 3 / 5 rows
"""
import numpy as np
import pytest
import torch

import segment_cases as SC
from d3fields_amd import _lib
from d3fields_amd.baked import BakedField

pytestmark = pytest.mark.gpu

INT32_MAX = SC.INT32_MAX
NAMES = ("clear", "last", "blocked", "min_value", "min_voxel")
POISON32 = np.frombuffer(b"\xa5" * 4, np.int32)[0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(shape, dtype, dev):
    t = torch.full(tuple(shape), 0xA5, dtype=torch.uint8, device=dev)
    return t if dtype == torch.uint8 else torch.full(tuple(shape) + (4,), 0xA5, dtype=torch.uint8, device=dev).view(dtype).reshape(tuple(shape))


def run_segments(free, value, a, b, strict, dev, skip=()):
    """-> {name: numpy array} of the outputs asked for (all but `skip`, and the minima only with value), from freshly poisoned buffers"""
    lib = _lib.load()
    nx, ny, nz = free.shape
    n = len(a)
    f = torch.from_numpy(np.array(free)).to(dev)
    v = None if value is None else torch.from_numpy(np.array(value)).to(dev)
    ta, tb = (torch.from_numpy(np.array(t, dtype=np.int32)).to(dev) for t in (a, b))
    wanted = [k for k in NAMES if k not in skip and (value is not None or not k.startswith("min_"))]
    out = {k: poisoned((n + 1,), torch.uint8 if k == "clear" else torch.int32, dev) for k in wanted}      # one entry more: it must stay as it is
    _lib.check(lib.d3f_volume_segments(_lib.ptr(f), _lib.ptr(v), nx, ny, nz, _lib.ptr(ta) if n else None, _lib.ptr(tb) if n else None, n,
                                       0 if strict else _lib.SEGMENT_CUT_CORNERS, *[_lib.ptr(out[k]) if k in out else None for k in NAMES],
                                       _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in out.items()}
    assert all(t[n] == (0xA5 if k == "clear" else POISON32) for k, t in out.items()), "a write past the last segment"
    return {k: t[:n] for k, t in out.items()}


def check_segments(free, value, a, b, strict, dev, want=None, skip=()):
    if want is None:
        want = SC.segments_ref(free, value, a, b, strict)
    got = run_segments(free, value, a, b, strict, dev, skip)
    for k, w in zip(NAMES, want):
        if k in got:
            assert got[k].dtype == w.dtype and got[k].tobytes() == w.tobytes(), (k, strict, value is not None, np.flatnonzero(got[k] != w)[:5])
    again = run_segments(free, value, a, b, strict, dev, skip)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), "two runs differ"
    return got


@pytest.mark.parametrize("name", SC.SEGMENT_VOLUMES)
def test_segments_equal_the_restatement(dev, name):
    free, value, a, b = SC.volume(name)
    for strict in (True, False):
        for with_value in (True, False):
            got = check_segments(free, value if with_value else None, a, b, strict, dev, SC.volume_reference(name, strict, with_value))
            if name in ("1x1x1", "all free"):
                assert got["clear"].all() and np.array_equal(got["last"], b) and (got["blocked"] == -1).all()
            if name == "none free":
                assert not got["clear"].any() and (got["last"] == -1).all() and np.array_equal(got["blocked"], a)
                assert not with_value or ((got["min_value"] == INT32_MAX).all() and (got["min_voxel"] == -1).all())


@pytest.mark.parametrize("name", list(SC.TIES))
def test_ties_strict_against_open(dev, name):
    """each side voxel of an edge or corner crossing blocked in turn: the strict rule stops there, the open rule passes"""
    shape, a, b, sides = SC.TIES[name]
    fa, fb = SC._flat(a, shape), SC._flat(b, shape)
    value = (np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape) * 7) % 5
    for side in sides + [None]:
        free = np.ones(shape, np.uint8)
        if side is not None:
            free[side] = 0
        for strict in (True, False):
            got = check_segments(free, value, [fa, fb], [fb, fa], strict, dev)
            blocked = strict and side is not None
            assert got["clear"].tolist() == [0 if blocked else 1] * 2
            assert got["blocked"].tolist() == ([SC._flat(side, shape)] * 2 if blocked else [-1, -1])


def test_segments_through_all_eight_octants(dev):
    free = np.ones((9, 9, 9), np.uint8)
    free[6, 5, 3] = 0
    value = np.random.default_rng(4).integers(0, 51, free.shape).astype(np.int32)
    centre = (4, 4, 4)
    octants = [tuple(1 - 2 * q for q in bits) for bits in np.ndindex(2, 2, 2)]
    ends = [tuple(c + s * d for c, s, d in zip(centre, signs, delta)) for signs in octants for delta in ((4, 4, 4), (4, 2, 1), (2, 1, 3), (1, 4, 2))]
    assert len(set(ends)) == 32
    a = [SC._flat(centre, free.shape)] * len(ends) + [SC._flat(e, free.shape) for e in ends] + [SC._flat(e, free.shape) for e in ends]
    b = [SC._flat(e, free.shape) for e in ends] + [SC._flat(centre, free.shape)] * len(ends) + [SC._flat(tuple(8 - c for c in e), free.shape) for e in ends]
    for strict in (True, False):
        got = check_segments(free, value, a, b, strict, dev)
        assert 0 < got["clear"].sum() < len(a) and (got["blocked"][got["clear"] == 0] == SC._flat((6, 5, 3), free.shape)).all()


def test_ends_outside_the_volume_and_counts(dev):
    free, value, a, b = SC.volume("24x20x28 97%")
    n = free.size
    ends_a = np.array([-1, 5, n, 7, -1, n, -INT32_MAX - 1, INT32_MAX, 0, n - 1], np.int32)
    ends_b = np.array([5, -1, 7, n, n, -1, 3, 3, n - 1, 0], np.int32)
    for strict in (True, False):
        got = check_segments(free, value, ends_a, ends_b, strict, dev)
        assert not got["clear"][:8].any() and (got["last"][:8] == -1).all() and (got["blocked"][:8] == -1).all()
        assert (got["min_value"][:8] == INT32_MAX).all() and (got["min_voxel"][:8] == -1).all()
    for count in (0, 1, 63, 65, 1000):
        aa, bb = np.resize(a, count), np.resize(b[::-1], count)
        got = check_segments(free, value, aa, bb, True, dev)
        assert all(len(t) == count for t in got.values())


def test_each_output_null_in_turn(dev):
    free, value, a, b = SC.volume("24x20x28 97%")
    for strict in (True, False):
        want = SC.volume_reference("24x20x28 97%", strict, True)
        for skip in NAMES:
            assert skip not in check_segments(free, value, a, b, strict, dev, want, skip=(skip,))
        check_segments(free, value, a, b, strict, dev, want, skip=NAMES[1:])                 # clear alone
        check_segments(free, None, a, b, strict, dev, SC.volume_reference("24x20x28 97%", strict, False), skip=("clear", "last"))


# ---- d3f_path_shorten ---------------------------------------------------------------------------------------------------------------
def run_shorten(free, rows, length, max_span, strict, dev, skip=()):
    lib = _lib.load()
    nx, ny, nz = free.shape
    rows = np.array(rows, dtype=np.int32, order="C")                 # (a copy: the references are read-only)
    n, row_len = rows.shape
    f = torch.from_numpy(np.array(free)).to(dev)
    r = torch.from_numpy(rows).to(dev)
    ln = torch.from_numpy(np.array(length, dtype=np.int32)).to(dev)
    oi = None if "index" in skip else poisoned((n + 1, row_len), torch.int32, dev)                       # one row more: it must stay as it is
    ov = None if "voxels" in skip else poisoned((n + 1, row_len), torch.int32, dev)
    oc = poisoned((n + 1,), torch.int32, dev)
    _lib.check(lib.d3f_path_shorten(_lib.ptr(f), nx, ny, nz, _lib.ptr(r), _lib.ptr(ln), n, row_len, max_span, 0 if strict else _lib.SEGMENT_CUT_CORNERS,
                                    _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(oc), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    got = tuple(None if t is None else t.cpu().numpy() for t in (oi, ov, oc))
    assert all(t is None or (t[n:] == POISON32).all() for t in got), "a write past the last row"
    return tuple(None if t is None else np.ascontiguousarray(t[:n]) for t in got)


def check_shorten(free, rows, length, max_span, strict, dev, want, skip=()):
    got = run_shorten(free, rows, length, max_span, strict, dev, skip)
    for k, g, w in zip(("index", "voxels", "count"), got, want):
        if g is not None:
            assert g.dtype == np.int32 and g.tobytes() == w.tobytes(), (k, max_span, strict, np.argwhere(g != w)[:5].tolist())
    again = run_shorten(free, rows, length, max_span, strict, dev, skip)
    assert all(g is None or g.tobytes() == h.tobytes() for g, h in zip(got, again)), "two runs differ"
    return got


def spans(row_len):
    return (1, 2, 64, 65, row_len)


@pytest.mark.parametrize("which,strict", [(w, r) for w in ("serpentine 6", "serpentine 18", "serpentine 26") for r in (True, False)])
def test_shorten_the_serpentine(dev, which, strict):
    """several chunks of candidates per anchor; under 18 / 26 with the strict rule 70 kept moves are not clear.  The rows of 18 and 26 are the same
    path, and on them the two rules keep the same anchors; under 6 the rules differ at max_span 2 (252 anchors strict, 234 open)"""
    free, rows, length = SC.ROW_SETS[which]()
    assert rows.shape[1] == (467 if which == "serpentine 6" else 397)
    for span in spans(rows.shape[1]):
        oi, ov, oc = check_shorten(free, rows, length, span, strict, dev, SC.shorten_reference(which, span, strict))
        k = int(oc[0])
        assert oi[0, 0] == 0 and oi[0, k - 1] == rows.shape[1] - 1 and (np.diff(oi[0, :k]) >= 1).all() and (np.diff(oi[0, :k]) <= span).all()
        assert k == rows.shape[1] if span == 1 else 64 < k < rows.shape[1]


def test_shorten_the_pillar_scene(dev):
    free, rows, length = SC.pillar_rows()
    note = []
    for r in range(len(SC.PILLAR_STARTS)):
        SC.shorten_ref(free, rows[r].tolist(), length[r], rows.shape[1], True, note)
    assert note, "the case set must hold an anchor whose chosen j lies beyond a blocked nearer j: a first-blocked scan cannot pass"
    for strict in (True, False):
        for span in spans(rows.shape[1]):
            oi, ov, oc = check_shorten(free, rows, length, span, strict, dev, SC.shorten_reference("pillar", span, strict))
            for r in range(4):
                k = int(oc[r])
                assert oi[r, 0] == 0 and oi[r, k - 1] == length[r] - 1 and ov[r, k - 1] == SC._flat(SC.PILLAR_GOAL, SC.PILLAR_SHAPE)


def test_shorten_random_rows(dev):
    """arbitrary voxel sequences of lengths 0, 1, 2, 64, 65, 200 in rows of 208, an entry outside the volume inside two of them; 1, 3, 4, 5 and 6
    rows per launch; lengths outside 0 .. row_len; each of out_index / out_voxels NULL"""
    free, rows, length = SC.random_rows()
    for strict in (True, False):
        for span in spans(rows.shape[1]):
            want = SC.shorten_reference("random", span, strict)
            check_shorten(free, rows, length, span, strict, dev, want)
            for k in (1, 3, 4, 5):                                   # the last k rows: a partial workgroup, one full one, one and a quarter
                check_shorten(free, rows[-k:], length[-k:], span, strict, dev, tuple(w[-k:] for w in want))
        want = SC.shorten_reference("random", 64, strict)
        check_shorten(free, rows, length, 64, strict, dev, want, skip=("index",))
        check_shorten(free, rows, length, 64, strict, dev, want, skip=("voxels",))
        check_shorten(free, rows, length, 2 ** 31 - 1, strict, dev, SC.shorten_reference("random", rows.shape[1], strict))
    wild = np.array([-5, 10 ** 6, INT32_MAX, -INT32_MAX - 1, 208, 209], np.int32)
    clamped = np.clip(wild, 0, rows.shape[1])
    check_shorten(free, rows, wild, 3, True, dev, SC.shorten_rows_ref(free, rows, clamped, 3, True))
    # row_len = 1
    got = check_shorten(free, rows[:, :1], np.array([0, 1, 1, 2, 1, 1], np.int32), 1, True, dev,
                        SC.shorten_rows_ref(free, rows[:, :1], [0, 1, 1, 1, 1, 1], 1, True))
    assert got[2].tolist() == [0, 1, 1, 1, 1, 1]


# ---- BakedField.straight / shortcut -------------------------------------------------------------------------------------------------
ROOMS_SHAPE, ROOMS_STEP, ROOMS_R = (31, 14, 5), 0.05, 0.12


def rooms(dev):
    """the three rooms of test_gpu_geodesic.py, rebuilt: A | B | C along x; the wall at x = 9 has a door 8 voxels wide (y = 3..10), the wall at
    x = 20 one 2 voxels wide (y = 6..7); r = 2.4 voxels: a body fits through the first and not the second"""
    dist = np.full(ROOMS_SHAPE, 1.0, np.float32)
    dist[9, :, :] = -1.0
    dist[9, 3:11, :] = 1.0
    dist[20, :, :] = -1.0
    dist[20, 6:8, :] = 1.0
    return BakedField.from_arrays((0.0, 0.0, 0.0), ROOMS_STEP, torch.from_numpy(dist).to(dev)).clearance()


def flat(p):
    return int(np.ravel_multi_index(p, ROOMS_SHAPE))


def world(voxels, dev):
    return torch.tensor([[c * ROOMS_STEP for c in v] for v in voxels], dtype=torch.float32, device=dev)


def row_length(voxels):
    """float64: the summed Euclidean voxel distances between consecutive entries"""
    xyz = np.array(np.unravel_index(np.asarray(voxels, np.int64), ROOMS_SHAPE), dtype=np.int64).T
    return float(np.sqrt((np.diff(xyz, axis=0) ** 2).sum(axis=1).astype(np.float64)).sum())


@pytest.fixture(scope="module")
def scene(dev):
    c = rooms(dev)
    goal = (15, 7, 2)
    t = c.travel(torch.tensor([flat(goal)], device=dev), radius=ROOMS_R)
    free = (c.valid & (c.dist >= ROOMS_R)).cpu().numpy().astype(np.uint8)
    assert np.array_equal(t.free.cpu().numpy(), free != 0)
    return c, t, free, c.d2.cpu().numpy()


def test_straight_equals_the_numpy_composition(dev, scene):
    c, t, free, d2 = scene
    rng = np.random.default_rng(6)
    a = rng.integers(0, free.size, 300).astype(np.int32)
    b = rng.integers(0, free.size, 300).astype(np.int32)
    a[:3], b[:3] = [flat((2, 2, 1)), flat((2, 2, 1)), flat((12, 7, 2))], [flat((8, 5, 1)), flat((15, 7, 2)), flat((27, 7, 2))]
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for cut in (False, True):
        want = SC.segments_ref(free, d2, a, b, not cut)
        assert want[0][0] == 1 and (cut or want[0][1] == 0) and want[0][2] == 0 and 0.1 < want[0].mean() < 0.9
        got = c.straight(ta, tb, radius=ROOMS_R, cut_corners=cut)
        assert sorted(got) == ["blocked_voxel", "clear", "clearance", "last_voxel", "min_d2", "min_voxel", "points"]
        assert got["clear"].dtype == torch.bool and got["points"].dtype == torch.float32 and got["clearance"].dtype == torch.float32
        for k, w in zip(("clear", "last_voxel", "blocked_voxel", "min_d2", "min_voxel"), want):
            assert got[k].dtype == (torch.bool if k == "clear" else torch.int32) and np.array_equal(got[k].cpu().numpy().astype(w.dtype), w), (k, cut)
        # clearance = float32(step * sqrt(float64(min_d2))), inf where no voxel was touched before the blocked one
        with np.errstate(invalid="ignore"):
            narrow = np.where(want[3] == INT32_MAX, np.inf, c.step * np.sqrt(want[3].astype(np.float64))).astype(np.float32)
        assert np.array_equal(got["clearance"].cpu().numpy().view(np.int32), narrow.view(np.int32)) and np.isinf(narrow).any()
        assert (narrow[want[0] == 1] >= np.float32(ROOMS_R)).all()                    # a clear segment stays at clearance >= radius at every touched voxel
        last = got["last_voxel"]
        centres = c._voxel_centres(torch.clamp(last, min=0))
        assert torch.equal(got["points"][last >= 0], centres[last >= 0]) and bool(torch.isnan(got["points"][last < 0]).all()) and bool((last < 0).any())
        assert not any(v.requires_grad for v in got.values())
        # the travel field: its own free volume by default, no d2 -> no minima; an explicit free= (bool or uint8) anywhere; float32 points
        want = SC.segments_ref(free, None, a, b, not cut)
        pa = c._voxel_centres(ta)
        for other in (t.straight(ta, tb, cut_corners=cut), t.straight(ta.long(), tb, free=t.free, cut_corners=cut), t.straight(pa, tb, cut_corners=cut),
                      c.straight(ta, tb, free=t.free.to(torch.uint8) * 3, cut_corners=cut)):
            for k, w in zip(("clear", "last_voxel", "blocked_voxel"), want):
                assert np.array_equal(other[k].cpu().numpy().astype(w.dtype), w), (k, cut)
        assert sorted(t.straight(ta, tb)) == ["blocked_voxel", "clear", "last_voxel", "points"]
    # a single a is broadcast (and a single b); points with a NaN or outside the volume are not clear
    one = t.straight(ta[:1], tb)
    assert np.array_equal(one["clear"].cpu().numpy(), SC.segments_ref(free, None, np.repeat(a[:1], 300), b, True)[0] != 0)
    back = t.straight(ta, tb[:1])
    assert np.array_equal(back["last_voxel"].cpu().numpy(), SC.segments_ref(free, None, a, np.repeat(b[:1], 300), True)[1])
    messy = torch.tensor([[float("nan"), 0.1, 0.1], [99.0, 0.1, 0.1], [0.1, 0.1, 0.1]], dtype=torch.float32, device=dev)
    got = t.straight(messy, world([(3, 3, 1)], dev))
    assert got["clear"].tolist() == [False, False, True] and got["last_voxel"].tolist()[:2] == [-1, -1] and bool(torch.isnan(got["points"][:2]).all())
    got = t.straight(world([(3, 3, 1)], dev), messy)
    assert got["clear"].tolist() == [False, False, True] and got["blocked_voxel"].tolist() == [-1, -1, -1]
    empty = t.straight(ta[:0], tb[:0])
    assert tuple(empty["clear"].shape) == (0,) and tuple(empty["points"].shape) == (0, 3)


def test_shortcut_equals_the_numpy_composition(dev, scene):
    c, t, free, _ = scene
    starts = [(2, 2, 1), (5, 12, 3), (12, 2, 0), (27, 10, 3)]                          # the last one lies behind the narrow door: an empty path
    paths = t.path(torch.tensor([flat(s) for s in starts], device=dev))
    rows, length = paths["voxels"].cpu().numpy(), paths["length"].cpu().numpy()
    L = rows.shape[1]
    assert length[0] == 14 and length[3] == 0 and paths["reached"].tolist() == [True, True, True, False]
    for cut in (False, True):
        for span in (None, 1, 3):
            want = SC.shorten_rows_ref(free, rows, length, L if span is None else span, not cut)
            out = t.shortcut(paths, cut_corners=cut, max_span=span)
            assert sorted(out) == ["distance", "distance_before", "index", "length", "points", "reached", "voxels"]
            for k, w in zip(("index", "voxels", "length"), want):
                assert out[k].dtype == torch.int32 and np.array_equal(out[k].cpu().numpy(), w), (k, cut, span)
            assert out["reached"] is paths["reached"] and out["distance"].dtype == torch.float64 and out["distance_before"].dtype == torch.float64
            assert not any(v.requires_grad for v in out.values())
            idx, vox, cnt = want
            pts = out["points"]
            assert tuple(pts.shape) == (4, L, 3) and pts.dtype == torch.float32
            for r in range(4):
                k = int(cnt[r])
                assert torch.equal(pts[r, :k], t._voxel_centres(out["voxels"][r, :k])) and bool(torch.isnan(pts[r, k:]).all())
                if k:
                    # the first and last anchors are the row's ends; index rises strictly
                    assert idx[r, 0] == 0 and idx[r, k - 1] == length[r] - 1 and vox[r, 0] == rows[r, 0] and vox[r, k - 1] == rows[r, length[r] - 1]
                    assert (np.diff(idx[r, :k]) >= 1).all()
                after, before = c.step * row_length(vox[r, :k]), c.step * row_length(rows[r, :length[r]])
                got_after, got_before = float(out["distance"][r]), float(out["distance_before"][r])
                # float64 sums of at most 500 non-negative terms err below 500 * 2^-53 relative, whatever the order: 1e-12 is far above it
                assert abs(got_after - after) <= 1e-12 * max(after, 1e-300) and abs(got_before - before) <= 1e-12 * max(before, 1e-300)
                assert got_after <= got_before * (1 + 1e-12)
                if span == 1:
                    assert k == length[r] and got_after == got_before
    # the figures of the route from (2, 2, 1): 14 voxels become 3 anchors, 15.389 voxels of path become 14.057
    out = t.shortcut(paths)
    assert out["voxels"][0, :3].tolist() == [flat((2, 2, 1)), flat((8, 5, 1)), flat((15, 7, 2))] and int(out["length"][0]) == 3
    assert abs(float(out["distance_before"][0]) / c.step - 15.389) < 5e-4 and abs(float(out["distance"][0]) / c.step - 14.057) < 5e-4
    # max_span of any integer type
    for span in (np.int64(3), torch.tensor(3)):
        other = t.shortcut(paths, max_span=span)
        assert torch.equal(other["index"], t.shortcut(paths, max_span=3)["index"])
    # anything path() takes as starts
    direct = t.shortcut(world(starts, dev))
    assert torch.equal(direct["voxels"], out["voxels"]) and torch.equal(direct["length"], out["length"]) and torch.equal(direct["distance"], out["distance"])
    empty = t.shortcut(torch.zeros((0,), dtype=torch.int64, device=dev))
    assert tuple(empty["voxels"].shape) == (0, L) and tuple(empty["points"].shape) == (0, L, 3) and tuple(empty["distance"].shape) == (0,)


def test_straight_and_shortcut_errors(dev, scene):
    c, t, free, _ = scene
    plain = BakedField.from_arrays((0.0, 0.0, 0.0), ROOMS_STEP, torch.ones(ROOMS_SHAPE, dtype=torch.float32, device=dev))
    idx = torch.tensor([flat((2, 2, 1)), flat((8, 5, 1))], device=dev)
    mask = torch.ones(ROOMS_SHAPE, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError):
        c.straight(idx, idx)                                     # neither radius nor free on a field without a free volume of its own
    with pytest.raises(ValueError):
        plain.straight(idx, idx)
    with pytest.raises(ValueError):
        c.straight(idx, idx, radius=0.1, free=mask)              # both
    with pytest.raises(ValueError):
        t.straight(idx, idx, radius=0.1)                         # radius on a field that is no clearance field
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            c.straight(idx, idx, radius=bad)
    for bad in (mask[:-1], mask.float(), mask.int(), "free"):
        with pytest.raises(ValueError):
            t.straight(idx, idx, free=bad)
    for bad in (torch.zeros((2, 2), dtype=torch.float32, device=dev), torch.zeros((2, 3), dtype=torch.float64, device=dev), idx.float(), [5]):
        with pytest.raises(ValueError):
            t.straight(bad, idx)
        with pytest.raises(ValueError):
            t.straight(idx, bad)
    with pytest.raises(ValueError):
        t.straight(idx, torch.cat([idx, idx[:1]]))               # 2 rows against 3
    for kw in (dict(a=idx.cpu(), b=idx), dict(a=idx, b=idx.cpu()), dict(a=idx, b=idx, free=mask.cpu())):
        with pytest.raises(RuntimeError):
            t.straight(**kw)
    assert plain.straight(idx, idx[:1], free=mask)["clear"].tolist() == [True, True]      # free= works on any field
    paths = t.path(idx)
    with pytest.raises(ValueError):
        c.shortcut(paths)                                        # not a travel field
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            t.shortcut(paths, max_span=bad)
    for bad in ({"voxels": paths["voxels"]}, dict(paths, voxels=paths["voxels"].long()), dict(paths, voxels=paths["voxels"][0]),
                dict(paths, length=paths["length"].long()), dict(paths, length=paths["length"][:1]), dict(paths, voxels="rows")):
        with pytest.raises(ValueError):
            t.shortcut(bad)
    with pytest.raises(ValueError):
        t.shortcut(idx.float())                                  # what path() rejects
    for bad in (dict(paths, voxels=paths["voxels"].cpu()), dict(paths, length=paths["length"].cpu()), idx.cpu()):
        with pytest.raises(RuntimeError):
            t.shortcut(bad)
