"""The merge of two baked fields on the device (d3f_volume_merge_select / d3f_volume_merge_rows, csrc/merge_kernels.hip; BakedField.merge) against
the NumPy restatement of tests/merge_cases.py: distances, weights, betas, validity, kinds, rows and known flags are compared byte for byte, no
tolerance anywhere.  EVERY launch runs twice on outputs poisoned with 0xA5 and the two runs must give the bytes of the restatement: the entry
points take their arguments in a struct, so tests/dirty_cases.py does not list them, and this file carries the dirty-buffer guarantee instead.
On the parent commit there is no symbol and no method: every test here fails there.

What each assert is there to catch:
  a ragged last wave, a kind decided from poison, a strict / non-strict gap, a fused or reordered blend, the cap      test_select (shapes x weights x w_max x gap)
  the lane mappings at 16 / 18 channels, vectors against scalars, strides, a misaligned base, half rows               test_rows_widths
  slots of either side, rows kept / blended / filled per band, voxel lists, NaN payloads, -0, subnormals              test_rows_random
  a set count of 0, mixed storage in one launch, an empty band behind NULL pointers, an empty list                    test_rows_sets_*, test_rows_empty_*
  a wiring error between BakedField.merge and the kernels, the band of the result, the weights of a chain             test_api_*
  a merge that loses what an occluder hides, or that builds a dense row array on the banded path                      test_occlusion"""
import ctypes

import numpy as np
import pytest
import torch

import band_cases as BC
import merge_cases as MC
import warp_cases as WC
from d3fields_amd import BakedField, _lib

pytestmark = pytest.mark.gpu
POISON = 0xA5
SELECT_KEYS = ("dist", "weight", "beta", "valid", "kind")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(dev, shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(n, 16),), POISON, dtype=torch.uint8, device=dev)[:n].view(dtype).view(shape)


def up(dev, a, dt=None):
    return torch.from_numpy(np.array(a, dt)).to(dev)               # (a copy: the case arrays are read-only)


def same_bytes(have, want, what):
    assert have.dtype == want.dtype and have.shape == want.shape, (what, have.dtype, want.dtype, have.shape, want.shape)
    if have.tobytes() != want.tobytes():
        word = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.itemsize]
        bad = np.flatnonzero(np.ascontiguousarray(have).view(word).reshape(-1) != np.ascontiguousarray(want).view(word).reshape(-1))
        raise AssertionError((what, len(bad), bad[:4].tolist(), have.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist()))


def call(dev, name, args):
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(args), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()


# ---- select -----------------------------------------------------------------------------------------------------------------------
def select_once(dev, da, va, wa, db, vb, wb, w_max, gap):
    shape = da.shape
    hold = [up(dev, da, np.float32), up(dev, va, np.uint8), up(dev, db, np.float32), up(dev, vb, np.uint8)]
    wva = up(dev, wa, np.float32) if isinstance(wa, np.ndarray) else None
    wvb = up(dev, wb, np.float32) if isinstance(wb, np.ndarray) else None
    out = {"dist": poisoned(dev, shape, torch.float32), "weight": poisoned(dev, shape, torch.float32), "beta": poisoned(dev, shape, torch.float32),
           "valid": poisoned(dev, shape, torch.uint8), "kind": poisoned(dev, shape, torch.uint8)}
    a = _lib.MergeSelect(shape[0], shape[1], shape[2], 0, _lib.ptr(hold[0]), _lib.ptr(hold[1]), _lib.ptr(wva), _lib.ptr(hold[2]), _lib.ptr(hold[3]), _lib.ptr(wvb),
                         1.0 if wva is not None else float(wa), 1.0 if wvb is not None else float(wb), float(w_max), float(gap),
                         *[_lib.ptr(out[k]) for k in SELECT_KEYS])
    call(dev, "d3f_volume_merge_select", a)
    return {k: t.cpu().numpy() for k, t in out.items()}


def run_select(dev, what, da, va, wa, db, vb, wb, w_max, gap):
    ref = MC.select_ref(da, va, wa, db, vb, wb, w_max, gap)
    got, again = select_once(dev, da, va, wa, db, vb, wb, w_max, gap), select_once(dev, da, va, wa, db, vb, wb, w_max, gap)
    for k in SELECT_KEYS:
        same_bytes(got[k], again[k], (what, k, "two runs differ"))
        same_bytes(got[k], ref[k], (what, k))
    return ref


_CASES = {}


def case(spec):
    """a random case and the restatement of its select, made once and shared"""
    if spec not in _CASES:
        cs = MC.random_case(*spec)
        _CASES[spec] = (cs, MC.select_ref(cs["da"], cs["va"], cs["wa"], cs["db"], cs["vb"], cs["wb"], cs["w_max"], cs["gap"]))
    return _CASES[spec]


SELECT_SHAPES = [((2, 2, 2), 1, 21), ((5, 4, 6), 1, 22), ((9, 8, 10), 1, 23), ((17, 12, 11), 1, 24)]      # (the last is no multiple of the wave)


@pytest.mark.parametrize("spec", SELECT_SHAPES, ids=["%dx%dx%d" % s[0] for s in SELECT_SHAPES])
@pytest.mark.parametrize("volumes", ["neither", "a", "b", "both"])
def test_select(dev, spec, volumes):
    cs = MC.random_case(*spec)
    wa = cs["wa"] if volumes in ("a", "both") else 1.5
    wb = cs["wb"] if volumes in ("b", "both") else 0.75
    seen = set()
    for w_max, gap in ((cs["w_max"], cs["gap"]), (np.inf, 0.0), (2.0, np.inf), (np.inf, np.nextafter(cs["gap"], np.float32(0)))):
        ref = run_select(dev, (spec[0], volumes, w_max, gap), cs["da"], cs["va"], wa, cs["db"], cs["vb"], wb, w_max, gap)
        seen |= set(np.unique(ref["kind"]).tolist())
    assert seen == set(MC.KINDS)


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def up_rows(dev, full, misalign):
    """the rows on the device, their base `misalign` elements past an allocation (whose first elements are poison)"""
    if full is None:
        return None, None
    t = poisoned(dev, (full.size + misalign,), torch.float16 if full.dtype == np.float16 else torch.float32)
    t[misalign:] = torch.from_numpy(np.array(full).reshape(-1)).to(dev)
    return t, t[misalign:]


def rows_once(dev, shape, kind, beta, sets, voxels, slot_a, slot_b, misalign=0, misalign_out=0):
    """sets: [(full_a, full_b, C, fill)], full: [rows, stride] float32 / float16, or None behind an empty band; slot: None (dense), an int32 volume,
    or "empty" (a band with n_rows == 0 and NULL pointers)"""
    n = int(np.prod(shape))
    m = n if voxels is None else len(voxels)
    vox = None if voxels is None else up(dev, np.concatenate([voxels, [0]]), np.int32)      # (one entry more: an empty list still has an address)
    hold, res = [], []
    arr_a, arr_b, outs = (_lib.VolumeSet * max(len(sets), 1))(), (_lib.VolumeSet * max(len(sets), 1))(), (ctypes.c_void_p * max(len(sets), 1))()
    for s, (full_a, full_b, C, fill) in enumerate(sets):
        f = None if fill is None else up(dev, fill, np.float32)
        out = poisoned(dev, (m * C + misalign_out,), torch.float32)[misalign_out:].view(m, C)
        hold += [f]
        for arr, full, fl in ((arr_a, full_a, f), (arr_b, full_b, None)):
            base, view = up_rows(dev, full, misalign)
            hold.append(base)
            word = _lib.DTYPE_F16 if full is not None and full.dtype == np.float16 else _lib.DTYPE_F32
            arr[s] = _lib.VolumeSet(None if view is None else view.data_ptr(), C, word, C if full is None else full.shape[1], _lib.ptr(fl))
        outs[s] = out.data_ptr()
        res.append(out)
    known = poisoned(dev, (m,), torch.uint8)
    bands = []
    for slot in (slot_a, slot_b):
        if slot is None:
            bands.append(None)
        elif isinstance(slot, str):
            bands.append(ctypes.pointer(_lib.Band(None, None, 0)))
        else:
            t = up(dev, slot, np.int32)
            hold.append(t)
            bands.append(ctypes.pointer(_lib.Band(_lib.ptr(t), None, int(slot.max()) + 1)))        # (cell_band is not read)
    k, b = up(dev, kind, np.uint8), up(dev, beta, np.float32)
    a = _lib.MergeRows(shape[0], shape[1], shape[2], len(sets), bands[0], bands[1], arr_a, arr_b, _lib.ptr(k), _lib.ptr(b), _lib.ptr(vox), m, outs, _lib.ptr(known), 0)
    call(dev, "d3f_volume_merge_rows", a)
    return [r.cpu().numpy() for r in res], known.cpu().numpy()


def ref_side(shape, full, C, slot):
    """(data, slot) as rows_ref takes them"""
    if isinstance(slot, str):
        return np.zeros((0, C), np.float32), np.full(shape, -1, np.int32)
    data = full[:, :C]
    return (data.reshape(tuple(shape) + (C,)), None) if slot is None else (data, slot)


def run_rows(dev, what, shape, kind, beta, sets, voxels=None, slot_a=None, slot_b=None, **kw):
    got, again = rows_once(dev, shape, kind, beta, sets, voxels, slot_a, slot_b, **kw), rows_once(dev, shape, kind, beta, sets, voxels, slot_a, slot_b, **kw)
    want_known = None
    for s, (full_a, full_b, C, fill) in enumerate(sets):
        same_bytes(got[0][s], again[0][s], (what, s, "two runs differ"))
        (data_a, sa), (data_b, sb) = ref_side(shape, full_a, C, slot_a), ref_side(shape, full_b, C, slot_b)
        want, want_known = MC.rows_ref(kind, beta, data_a, data_b, fill=fill, voxels=voxels, slot_a=sa, slot_b=sb)
        same_bytes(got[0][s], want, (what, "set", s, C))
    same_bytes(got[1], again[1], (what, "known: two runs differ"))
    if want_known is None:                           # no set: the known flags of a one-channel stand-in
        def stand_in(slot):
            rows = int(np.prod(shape)) if slot is None else 0 if isinstance(slot, str) else int(slot.max()) + 1
            return ref_side(shape, np.zeros((rows, 1), np.float32), 1, slot)
        (data_a, sa), (data_b, sb) = stand_in(slot_a), stand_in(slot_b)
        _, want_known = MC.rows_ref(kind, beta, data_a, data_b, voxels=voxels, slot_a=sa, slot_b=sb)
    same_bytes(got[1], want_known, (what, "known"))
    return got


def flat_rows(rows, stride=None):
    """a case's rows as [rows, stride]: the pad beyond C is poison"""
    C = rows.shape[-1]
    r = np.array(rows).reshape(-1, C)
    if stride is None or stride == C:
        return r
    full = np.full((r.shape[0], stride), np.nan, r.dtype)
    full[:, :C] = r
    return full


@pytest.mark.parametrize("spec", MC.RANDOM, ids=MC.case_id)
@pytest.mark.parametrize("listed", [False, True], ids=["every voxel", "list"])
def test_rows_random(dev, spec, listed):
    """all four dense / banded combinations and all four float32 / half combinations are among MC.RANDOM"""
    cs, ref = case(spec)
    voxels = MC.voxel_list(ref["kind"].size, 9) if listed else None
    run_rows(dev, (MC.case_id(spec), listed), cs["shape"], ref["kind"], ref["beta"], [(flat_rows(cs["rows_a"]), flat_rows(cs["rows_b"]), cs["C"], cs["fill"])],
             voxels=voxels, slot_a=cs["slot_a"], slot_b=cs["slot_b"])


def test_random_cases_cover_the_storage_and_band_combinations():
    combos = {(s[3], s[4]) for s in MC.RANDOM}, {(s[5], s[6]) for s in MC.RANDOM}
    assert all(len(c) == 4 for c in combos)


@pytest.mark.parametrize("C", [1, 3, 16, 18, 20, 64])
@pytest.mark.parametrize("half", [(False, False), (True, True), (False, True)], ids=["f32+f32", "f16+f16", "f32+f16"])
def test_rows_widths(dev, C, half):
    """one lane and sixteen lanes per voxel, the vector and the scalar rule: stride_voxel == C, larger and vector-friendly, larger and odd; a base
    pointer one element past 16-byte alignment; an output row base off 16 bytes"""
    spec = ((5, 4, 6), C, 30 + C, False, False, half[0], half[1])
    cs, ref = case(spec)
    voxels = MC.voxel_list(ref["kind"].size, C)
    for stride, misalign, misalign_out in ((C, 0, 0), (C + 8, 0, 0), (C + 1, 0, 0), (C, 1, 0), (C + 8, 1, 0), (C, 0, 1)):
        sets = [(flat_rows(cs["rows_a"], stride), flat_rows(cs["rows_b"], stride), C, None if stride > C else cs["fill"])]
        run_rows(dev, (C, half, stride, misalign, misalign_out), cs["shape"], ref["kind"], ref["beta"], sets, voxels=voxels if misalign else None, misalign=misalign,
                 misalign_out=misalign_out)


def split_sets(cs, widths, halves, stride_pad=0):
    """the channels of a case as several set pairs: [(full_a, full_b, C, fill)], halves[s] = (a is half, b is half)"""
    out, c0 = [], 0
    for C, (ha, hb) in zip(widths, halves):
        a = flat_rows(cs["rows_a"])[:, c0:c0 + C].astype(np.float16 if ha else np.float32)
        b = flat_rows(cs["rows_b"])[:, c0:c0 + C].astype(np.float16 if hb else np.float32)
        out.append((flat_rows(a, C + stride_pad), flat_rows(b, C + stride_pad), C, cs["fill"][c0:c0 + C]))
        c0 += C
    return out


@pytest.mark.parametrize("spec", [((9, 8, 10), 40, 41, False, False, False, False), ((9, 8, 10), 40, 42, True, False, False, False), ((5, 4, 6), 40, 43, True, True, False, False)],
                         ids=["dense+dense", "band+dense", "band+band"])
def test_rows_sets_mixed_storage(dev, spec):
    cs, ref = case(spec)
    args = (cs["shape"], ref["kind"], ref["beta"])
    three = split_sets(cs, (3, 16, 21), ((False, True), (True, False), (False, False)))
    run_rows(dev, "three sets", *args, three, slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    run_rows(dev, "three sets, list", *args, three, voxels=MC.voxel_list(ref["kind"].size, 2), slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    run_rows(dev, "one set", *args, three[1:2], slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    eight = split_sets(cs, (5,) * 8, ((False, False), (True, True)) * 4)
    run_rows(dev, "eight sets", *args, eight, slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    got = run_rows(dev, "no set", *args, [], voxels=MC.voxel_list(ref["kind"].size, 4), slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    assert got[0] == []


def test_rows_empty_band_and_empty_list(dev):
    cs, ref = case(((9, 8, 10), 20, 44, True, True, False, True))
    args = (cs["shape"], ref["kind"], ref["beta"])
    a, b = flat_rows(cs["rows_a"]), flat_rows(cs["rows_b"])
    got = run_rows(dev, "a empty", *args, [(None, b, 20, cs["fill"])], slot_a="empty", slot_b=cs["slot_b"])
    assert got[1].any() and not got[1].all()
    run_rows(dev, "b empty", *args, [(a, None, 20, None)], voxels=MC.voxel_list(ref["kind"].size, 5), slot_a=cs["slot_a"], slot_b="empty")
    got = run_rows(dev, "both empty", *args, [(None, None, 20, cs["fill"]), (None, None, 3, None)], slot_a="empty", slot_b="empty")
    assert not got[1].any() and (got[0][0] == cs["fill"]).all() and (got[0][1] == 0).all()
    none = run_rows(dev, "m == 0", *args, [(a, b, 20, cs["fill"])], voxels=np.zeros(0, np.int32), slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    assert none[0][0].shape == (0, 20) and none[1].shape == (0,)


# ---- BakedField.merge -----------------------------------------------------------------------------------------------------------------
STEP = 0.25                                          # a power of two: the lattice points are exact in float32


@pytest.fixture(scope="module")
def pair(dev):
    cs = MC.field_pair(step=STEP)
    a = BakedField.from_arrays((0.0, 0.0, 0.0), STEP, up(dev, cs["da"]), valid=up(dev, cs["va"]), fills={"feat": up(dev, np.arange(cs["C"], dtype=np.float32))},
                               feat=up(dev, cs["rows_a"]), only_a=up(dev, cs["rows_a"][..., :2]))
    b = BakedField.from_arrays((0.0, 0.0, 0.0), STEP, up(dev, cs["db"]), valid=up(dev, cs["vb"]), feat=up(dev, cs["rows_b"]), only_b=up(dev, cs["rows_b"][..., :2]))
    return cs, a, b


def vol_of(shape, dist, valid):
    return {"shape": tuple(shape), "dist": dist, "valid": valid != 0}


def check_field(m, ref, want_rows, want_known, name="feat", mark=None):
    """every array of a merged field against the restatement; want_rows / want_known in the result's own row order"""
    same_bytes(m.dist.cpu().numpy(), ref["dist"], "dist")
    same_bytes(m.valid.view(torch.uint8).cpu().numpy(), ref["valid"], "valid")
    same_bytes(m.weight.cpu().numpy(), ref["weight"], "weight")
    same_bytes(m.merged_from.cpu().numpy(), ref["kind"], "merged_from")
    assert m.valid.dtype == torch.bool and m.rows_known.dtype == torch.bool and m.merged_from.dtype == torch.uint8
    C = want_rows.shape[1]
    same_bytes(m._sets[name].reshape(-1, C).cpu().numpy(), want_rows, "rows")
    same_bytes(m.rows_known.view(torch.uint8).reshape(-1).cpu().numpy(), want_known, "rows_known")
    if mark is None:
        assert m.band is None and m.slot is None and tuple(m.rows_known.shape) == tuple(m.grid_shape)
    else:
        same_bytes(m.slot.cpu().numpy(), mark["slot"], "slot")
        same_bytes(m.band_voxels.cpu().numpy(), mark["voxels"], "band_voxels")
        same_bytes(m.cell_band.cpu().numpy(), mark["cell_band"].astype(np.uint8), "cell_band")


def lattice(f):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in f.grid_shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return torch.from_numpy((np.float32(f.origin) + idx.astype(np.float32) * np.float32(f.step)).astype(np.float32)).to(f.device)


def test_api_dense(dev, pair):
    cs, a, b = pair
    m = a.merge(b)
    assert isinstance(m, BakedField) and m.grid_shape == a.grid_shape and m.origin == a.origin and m.step == a.step and m.names() == ["feat"]
    ref = MC.select_ref(cs["da"], cs["va"], 1.0, cs["db"], cs["vb"], 1.0)
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=np.arange(cs["C"], dtype=np.float32))
    check_field(m, ref, rows, known)
    assert a.weight is None and a.merged_from is None and (ref["kind"] == MC.NONE).any() and (ref["kind"] == MC.KEEP).any() and (ref["kind"] == MC.NEW).any()
    assert BakedField.MERGE_BLEND == 3 and int((m.merged_from == BakedField.MERGE_BLEND).sum()) == int((ref["kind"] == MC.BLEND).sum()) > 0
    # weights: a scalar per side, a volume for the newer side, a cap
    views = np.random.default_rng(3).integers(0, 4, cs["shape"]).astype(np.float32)
    m2 = a.merge(b, weight=2.0, other_weight=up(dev, views), max_weight=3.5, return_names=["feat"])
    ref2 = MC.select_ref(cs["da"], cs["va"], 2.0, cs["db"], cs["vb"], views, 3.5)
    check_field(m2, ref2, *MC.rows_ref(ref2["kind"], ref2["beta"], cs["rows_a"], cs["rows_b"], fill=np.arange(cs["C"], dtype=np.float32)))
    assert (ref2["kind"] != ref["kind"]).any()       # a view count of 0 is not usable
    # half rows on either side: widened exactly, the result is float32
    mh = a.half().merge(b.half(["feat"]))
    ha, hb = cs["rows_a"].astype(np.float16), cs["rows_b"].astype(np.float16)
    check_field(mh, ref, *MC.rows_ref(ref["kind"], ref["beta"], ha, hb, fill=np.arange(cs["C"], dtype=np.float32)))
    assert mh.rows_dtype("feat") == torch.float32
    # the result is an ordinary field: its lookup at the lattice points of valid cells returns the stored merged values
    out = m.eval(lattice(m))
    ok = out["valid_mask"].cpu().numpy()
    assert 100 < ok.sum() < ok.size
    assert np.array_equal(out["dist"].cpu().numpy()[ok], ref["dist"].reshape(-1)[ok]) and np.array_equal(out["feat"].cpu().numpy()[ok], rows[ok])


def test_api_reset_gap(dev, pair):
    cs, a, b = pair
    gap = 1.0 * STEP
    m = a.merge(b, reset_gap=gap)
    ref = MC.select_ref(cs["da"], cs["va"], 1.0, cs["db"], cs["vb"], 1.0, gap=gap)
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=np.arange(cs["C"], dtype=np.float32))
    check_field(m, ref, rows, known)
    moved = np.zeros(cs["shape"], bool)
    moved[cs["moved"]] = True
    reset = ref["kind"] == MC.RESET
    assert reset.sum() > 50 and (reset & moved).sum() == reset.sum()                        # the planted moved surface, and nowhere else
    got = m._sets["feat"].cpu().numpy()
    assert got[reset].tobytes() == cs["rows_b"][reset].tobytes() and m.dist.cpu().numpy()[reset].tobytes() == cs["db"][reset].tobytes()
    assert (a.merge(b).merged_from.cpu().numpy()[reset] == MC.BLEND).all()                   # without the rule they are averaged


def band_rows(cs_rows, mark):
    return np.ascontiguousarray(cs_rows.reshape(-1, cs_rows.shape[-1])[mark["voxels"]])


def test_api_banded(dev, pair):
    cs, a, b = pair
    shape, fill = cs["shape"], np.arange(cs["C"], dtype=np.float32)
    band_a, band_b = 1.5 * STEP, 2.25 * STEP
    ab, bb = a.to_band(band_a), b.to_band(band_b)
    mark_a, mark_b = BC.mark(vol_of(shape, cs["da"], cs["va"]), band_a), BC.mark(vol_of(shape, cs["db"], cs["vb"]), band_b)
    same_bytes(ab.slot.cpu().numpy(), mark_a["slot"], "a's slots")
    ref = MC.select_ref(cs["da"], cs["va"], 1.0, cs["db"], cs["vb"], 1.0)
    vol = vol_of(shape, ref["dist"], ref["valid"])
    # banded + dense: banded with a's band
    m = ab.merge(b)
    mark = BC.mark(vol, band_a)
    assert m.band == band_a and 0 < mark["M"] < ref["kind"].size
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], band_rows(cs["rows_a"], mark_a), cs["rows_b"], fill=fill, voxels=mark["voxels"], slot_a=mark_a["slot"])
    check_field(m, ref, rows, known, mark=mark)
    # dense + banded: b's band
    m = a.merge(bb)
    mark = BC.mark(vol, band_b)
    assert m.band == band_b
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], band_rows(cs["rows_b"], mark_b), fill=fill, voxels=mark["voxels"], slot_b=mark_b["slot"])
    check_field(m, ref, rows, known, mark=mark)
    # banded + banded with different bands, the result with a's; then with a band of its own; rows missing on both sides are fill rows
    for band in (None, 3.0 * STEP):
        m = ab.merge(bb, band=band)
        mark = BC.mark(vol, band_a if band is None else band)
        assert m.band == (band_a if band is None else band)
        rows, known = MC.rows_ref(ref["kind"], ref["beta"], band_rows(cs["rows_a"], mark_a), band_rows(cs["rows_b"], mark_b), fill=fill, voxels=mark["voxels"],
                                  slot_a=mark_a["slot"], slot_b=mark_b["slot"])
        check_field(m, ref, rows, known, mark=mark)
    assert not known.all() and (rows[known == 0] == fill).all()
    # dense + dense with band=: a banded result from two dense fields
    m = a.merge(b, band=band_a)
    mark = BC.mark(vol, band_a)
    check_field(m, ref, *MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=fill, voxels=mark["voxels"]), mark=mark)


def test_api_chain_picks_up_the_weights(dev, pair):
    cs, a, b = pair
    rng = np.random.default_rng(17)
    dc = (cs["da"] + np.float32(0.125 * STEP)).astype(np.float32)
    vc = cs["va"] & (rng.uniform(size=cs["shape"]) > 0.1)
    dc[~vc] = np.nan
    rows_c = rng.normal(size=cs["rows_a"].shape).astype(np.float32)
    c = BakedField.from_arrays((0.0, 0.0, 0.0), STEP, up(dev, dc), valid=up(dev, vc), feat=up(dev, rows_c))
    fill = np.arange(cs["C"], dtype=np.float32)
    m1 = a.merge(b)
    m2 = m1.merge(c, weight=100.0, max_weight=2.5)                  # `weight` is not used: m1 has a weight volume
    r1 = MC.select_ref(cs["da"], cs["va"], 1.0, cs["db"], cs["vb"], 1.0)
    rows1, _ = MC.rows_ref(r1["kind"], r1["beta"], cs["rows_a"], cs["rows_b"], fill=fill)
    r2 = MC.select_ref(r1["dist"], r1["valid"], r1["weight"], dc, vc.astype(np.uint8), 1.0, 2.5)
    rows2, known2 = MC.rows_ref(r2["kind"], r2["beta"], rows1.reshape(cs["rows_a"].shape), rows_c, fill=fill)
    check_field(m2, r2, rows2, known2)
    third = np.float32(1) / np.float32(3)
    assert (r2["beta"] == third).any() and (r2["beta"] == 0.5).any() and (r2["weight"] == 2.5).any() and (r2["weight"] == 2).any()
    # ... and the other way round: a merged field as the NEWER side brings its weights when other_weight is left alone
    m3 = c.merge(m1)
    r3 = MC.select_ref(dc, vc.astype(np.uint8), 1.0, r1["dist"], r1["valid"], r1["weight"])
    check_field(m3, r3, *MC.rows_ref(r3["kind"], r3["beta"], rows_c, rows1.reshape(cs["rows_a"].shape)))
    assert (r3["beta"] == np.float32(2) / np.float32(3)).any()


def test_api_argument_errors_on_the_device(dev, pair):
    cs, a, b = pair
    with pytest.raises(ValueError):
        a.merge(b, other_weight=torch.ones(cs["shape"]))             # on the host
    with pytest.raises(KeyError):
        a.merge(b, return_names=["only_a"])
    assert a.merge(b, return_names=[]).names() == []


def test_api_warp_then_merge(dev):
    """the recipe: predicted = a.warp(...); predicted.merge(b) on the small warp fixture.  Where b is invalid and predicted is valid the result is
    predicted's"""
    cs = WC.random_case((9, 10, 17), 12, K=6)
    _, rows = WC.rows_data(cs["shape"], 20, 42)
    f = BakedField.from_arrays((1.0, -2.0, 0.5), 0.25, up(dev, cs["dist"], np.float32), valid=up(dev, cs["valid"], np.uint8), b=up(dev, rows, np.float32))
    predicted = f.warp(up(dev, cs["pose"], np.float64), up(dev, cs["owner"], np.int32))
    rng = np.random.default_rng(2)
    vb = rng.uniform(size=cs["shape"]) > 0.4
    db = rng.normal(size=cs["shape"]).astype(np.float32)
    rows_b = rng.normal(size=rows.shape).astype(np.float32)
    b = BakedField.from_arrays((1.0, -2.0, 0.5), 0.25, up(dev, db), valid=up(dev, vb), b=up(dev, rows_b))
    m = predicted.merge(b)
    pd, pv, pr = predicted.dist.cpu().numpy(), predicted.valid.cpu().numpy(), predicted._sets["b"].cpu().numpy()
    ref = MC.select_ref(pd, pv.astype(np.uint8), 1.0, db, vb.astype(np.uint8), 1.0)
    check_field(m, ref, *MC.rows_ref(ref["kind"], ref["beta"], pr, rows_b), name="b")
    keep = pv & ~vb & ~np.isnan(pd)
    assert keep.sum() > 20 and (ref["kind"][keep] == MC.KEEP).all()
    assert m.dist.cpu().numpy()[keep].tobytes() == pd[keep].tobytes() and m._sets["b"].cpu().numpy()[keep].tobytes() == pr[keep].tobytes()


def test_occlusion(dev):
    """b has a box of voxels invalidated (an occluder in front of the cameras): the merged valid is the union, the rows inside the box are a's bit
    for bit, and the banded path allocates dist-sized arrays and the M x C rows, never a dense row array"""
    C = 128
    cs = MC.field_pair(C=C, seed=12, step=STEP)
    shape = cs["shape"]
    n_vox = int(np.prod(shape))
    assert shape == (24, 20, 16)
    a = BakedField.from_arrays((0.0, 0.0, 0.0), STEP, up(dev, cs["da"]), valid=up(dev, cs["va"]), feat=up(dev, cs["rows_a"]))
    b = BakedField.from_arrays((0.0, 0.0, 0.0), STEP, up(dev, cs["db"]), valid=up(dev, cs["vb"]), feat=up(dev, cs["rows_b"]))
    m = a.merge(b)
    valid = m.valid.cpu().numpy()
    assert np.array_equal(valid, cs["va"] | cs["vb"]) and not cs["vb"][cs["box"]].any() and cs["va"][cs["box"]].sum() > 500
    inside = np.zeros(shape, bool)
    inside[cs["box"]] = True
    inside &= cs["va"]
    assert (m.merged_from.cpu().numpy()[inside] == MC.KEEP).all() and m._sets["feat"].cpu().numpy()[inside].tobytes() == cs["rows_a"][inside].tobytes()
    assert m.dist.cpu().numpy()[inside].tobytes() == cs["da"][inside].tobytes() and m.rows_known.cpu().numpy()[inside].all()
    band = 1.5 * STEP
    ab, bb = a.to_band(band), b.to_band(band)
    del m
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    mb = ab.merge(bb)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    M = mb.band_voxels.numel()
    bound = 12 * 4 * n_vox + int(1.25 * 4 * M * C) + (64 << 10)       # the bound of tests/test_gpu_band.py
    print("\n  banded merge: M = %d of %d voxels (%.1f %%), peak %d bytes, bound %d, dense rows %d" % (M, n_vox, 100.0 * M / n_vox, peak, bound, 4 * n_vox * C))
    assert 0 < M < n_vox and 4 * n_vox * C > bound, "the dense size must be the failing side"
    assert peak <= bound, (peak, bound)
    ref = MC.select_ref(cs["da"], cs["va"], 1.0, cs["db"], cs["vb"], 1.0)
    mark = BC.mark(vol_of(shape, ref["dist"], ref["valid"]), band)
    mark_a, mark_b = BC.mark(vol_of(shape, cs["da"], cs["va"]), band), BC.mark(vol_of(shape, cs["db"], cs["vb"]), band)
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], band_rows(cs["rows_a"], mark_a), band_rows(cs["rows_b"], mark_b), voxels=mark["voxels"], slot_a=mark_a["slot"],
                              slot_b=mark_b["slot"])
    check_field(mb, ref, rows, known, mark=mark)
    stored_in_box = inside.reshape(-1)[mark["voxels"]] & (mark_a["slot"].reshape(-1)[mark["voxels"]] >= 0)
    assert stored_in_box.sum() > 50 and known[stored_in_box].all()
