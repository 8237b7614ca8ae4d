"""The warp of a baked field on the device (d3f_volume_warp_select / d3f_volume_warp_rows, csrc/warp_kernels.hip; BakedField.warp, .owners)
against the NumPy restatement of tests/warp_cases.py: sources, distances, validity, boxes, rows and known flags are compared byte for byte, no
tolerance anywhere -- winners depend on float comparisons.  EVERY launch runs twice on outputs poisoned with 0xA5 and the two runs must give
the bytes of the restatement: the entry points take their arguments in a struct, so tests/dirty_cases.py does not list them, and this file
carries the dirty-buffer guarantee instead.

What each assert is there to catch:
  a tile edge, a ragged volume, a wrong corner or weight, a fused chain, a candidate order                 test_select (shapes x motions)
  NaN / invalid voxels, signed zeros, owner values outside 1..K, NaN pose rows, K = 0                         test_select (specials)
  a tie that goes the wrong way, a culled part that had a candidate                                         test_select (collisions, planted)
  the second ballot word, the LDS list at its capacity, per-lane box atomics                                test_many_parts
  the lane mappings at 16 / 17 channels, vectors against scalars, strides, fills, voxel lists               test_rows
  slots, known flags and fill rows of a banded source, an empty band                                        test_band
  a wiring error between BakedField.warp / .owners and the kernels                                          test_api_*
  a warp that does not put the observation where the object is now                                          test_scene"""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import band_cases as BC
import warp_cases as WC
from conftest import ROOT
from d3fields_amd import BakedField, _lib

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(dev, shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(n, 16),), POISON, dtype=torch.uint8, device=dev)[:n].view(dtype).view(shape)


def up(dev, a, dt):
    return torch.from_numpy(np.array(a, dt)).to(dev)               # (a copy: the case arrays are read-only)


def volume_struct(shape, dist=None, valid=None, cell=None):
    return _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0.0, 0.0, 0.0), 1.0, 0, _lib.ptr(dist), _lib.ptr(valid), _lib.ptr(cell))


def select_once(dev, dist, valid, owner, pose):
    shape, K = dist.shape, len(pose)
    d, v, c = up(dev, dist, np.float32), up(dev, valid, np.uint8), up(dev, WC.cell_valid(valid), np.uint8)
    o, p = up(dev, owner, np.int32), up(dev, np.asarray(pose, np.float64).reshape(K, WC.POSE), np.float64)
    out = {"source": poisoned(dev, shape, torch.int32), "dist": poisoned(dev, shape, torch.float32), "valid": poisoned(dev, shape, torch.uint8),
           "boxes": poisoned(dev, (K, 12), torch.int32)}
    a = _lib.WarpSelect(volume_struct(shape, d, v, c), _lib.ptr(o), _lib.ptr(p) if K else None, K, 0, _lib.ptr(out["source"]), _lib.ptr(out["dist"]),
                        _lib.ptr(out["valid"]), _lib.ptr(out["boxes"]) if K else None)
    _lib.check(_lib.load().d3f_volume_warp_select(ctypes.byref(a), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def same_bytes(have, want, what):
    assert have.dtype == want.dtype and have.shape == want.shape, (what, have.dtype, want.dtype, have.shape, want.shape)
    if have.tobytes() != want.tobytes():
        word = {1: np.uint8, 4: np.uint32, 8: np.uint64}[want.itemsize]
        bad = np.flatnonzero(np.ascontiguousarray(have).view(word).reshape(-1) != np.ascontiguousarray(want).view(word).reshape(-1))
        raise AssertionError((what, len(bad), bad[:4].tolist(), have.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist()))


_REF = {}


def select_ref(key, cs):
    """the restatement of a case, computed once and shared"""
    if key not in _REF:
        _REF[key] = WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    return _REF[key]


def run_select(dev, key, cs):
    """two launches on poisoned outputs: equal to each other and to the restatement, byte for byte"""
    ref = select_ref(key, cs)
    got, again = select_once(dev, cs["dist"], cs["valid"], cs["owner"], cs["pose"]), select_once(dev, cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    for k in ("source", "dist", "valid", "boxes"):
        same_bytes(got[k], again[k], (key, k, "two runs differ"))
        same_bytes(got[k], ref[k], (key, k))
    return ref


def rows_once(dev, shape, source, pose, sets, voxels, band):
    """sets: [(full [rows, stride] float32, C, fill or None)]; band: None or (slot, cell_band, M) with slot / cell_band None for M == 0"""
    K = len(pose)
    n = int(np.prod(shape))
    m = n if voxels is None else len(voxels)
    src, p = up(dev, source, np.int32), up(dev, np.asarray(pose, np.float64).reshape(K, WC.POSE), np.float64)
    vox = None if voxels is None else up(dev, voxels, np.int32)
    hold, arr, outs = [], (_lib.VolumeSet * max(len(sets), 1))(), (ctypes.c_void_p * max(len(sets), 1))()
    res = []
    for s, (full, C, fill) in enumerate(sets):
        data = None if full is None else up(dev, full, np.float32)
        f = None if fill is None else up(dev, fill, np.float32)
        out = poisoned(dev, (m, C), torch.float32)
        hold += [data, f]
        arr[s] = _lib.VolumeSet(_lib.ptr(data), C, 0, C if full is None else full.shape[1], _lib.ptr(f))
        outs[s] = out.data_ptr()
        res.append(out)
    known = poisoned(dev, (m,), torch.uint8)
    b = None
    if band is not None:
        slot, cb = (None, None) if band[0] is None else (up(dev, band[0], np.int32), up(dev, band[1], np.uint8))
        hold += [slot, cb]
        b = ctypes.pointer(_lib.Band(_lib.ptr(slot), _lib.ptr(cb), band[2]))
    a = _lib.WarpRows(volume_struct(shape), b, arr, len(sets), K, _lib.ptr(src), _lib.ptr(p) if K else None, _lib.ptr(vox), m, outs, _lib.ptr(known))
    _lib.check(_lib.load().d3f_volume_warp_rows(ctypes.byref(a), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res], known.cpu().numpy()


def run_rows(dev, what, shape, source, pose, sets, voxels=None, band=None):
    got, again = rows_once(dev, shape, source, pose, sets, voxels, band), rows_once(dev, shape, source, pose, sets, voxels, band)
    want_known = None
    for s, (full, C, fill) in enumerate(sets):
        same_bytes(got[0][s], again[0][s], (what, s, "two runs differ"))
        if band is None:
            data = full[:, :C].reshape(tuple(shape) + (C,))
            want, want_known = WC.rows_ref(source, pose, data, fill=fill, voxels=voxels)
        else:
            data = np.zeros((0, C), np.float32) if full is None else full[:, :C]
            want, want_known = WC.rows_ref(source, pose, data, fill=fill, voxels=voxels, slot=band[0], cell_band=band[1])
        same_bytes(got[0][s], want, (what, "set", s, C))
    same_bytes(got[1], again[1], (what, "known: two runs differ"))
    if want_known is not None:
        same_bytes(got[1], want_known, (what, "known"))
    return got


# ---- select -------------------------------------------------------------------------------------------------------------------------
BIG, WIDE, SMALL = (9, 10, 17), (16, 8, 8), (2, 2, 2)
SELECT = {
    "2x2x2 shift": lambda: WC.random_case(SMALL, 2, K=2, specials=False, motions="shift"),
    "2x2x2 specials": lambda: WC.random_case(SMALL, 3, K=2),
    "9x10x17 identity": lambda: WC.random_case(BIG, 20, K=3, specials=False, motions="identity"),
    "9x10x17 shifts": lambda: WC.random_case(BIG, 21, K=4, specials=False, motions="shift"),
    "9x10x17 quarter turns": lambda: WC.random_case(BIG, 22, K=3, specials=False, motions="quarter"),
    "9x10x17 half turns": lambda: WC.random_case(BIG, 23, K=3, specials=False, motions="half"),
    "9x10x17 about 10 degrees": lambda: WC.random_case(BIG, 24, K=4, specials=False, motions="small"),
    "9x10x17 mixed specials": lambda: WC.random_case(BIG, 12, K=6),
    "16x8x8 mixed": lambda: WC.random_case(WIDE, 25, K=6, specials=False),
    "16x8x8 mixed specials": lambda: WC.random_case(WIDE, 13, K=6),
    "16x8x8 about 10 degrees specials": lambda: WC.random_case(WIDE, 26, K=5, motions="small"),
    "planted": WC.planted_case,
    "collisions": WC.collision_case,
}


@pytest.mark.parametrize("name", list(SELECT))
def test_select(dev, name):
    cs = SELECT[name]()
    ref = run_select(dev, name, cs)
    if "specials" not in name and name != "2x2x2 shift":
        assert (ref["source"] > 0).sum() >= 10, (name, "the case moves nothing: it would test nothing")
    if name == "planted":
        assert np.array_equal(ref["boxes"], cs["boxes"]) and int((ref["source"] == -1).sum()) == cs["vacated"]
        assert ref["boxes"][1, 6:].tolist() == [WC.INT32_MAX] * 3 + [WC.INT32_MIN] * 3      # moved wholly off the grid: an empty landing box
    if name == "collisions":
        assert (ref["source"][cs["tie"]] == 0).all() and (ref["source"] != 5).all() and set(ref["source"][cs["both"]].reshape(-1).tolist()) == {1, 2}


def test_select_without_parts(dev):
    cs = dict(WC.random_case(BIG, 12, K=6))
    cs["pose"], cs["K"] = np.zeros((0, WC.POSE)), 0
    ref = run_select(dev, "K = 0", cs)
    assert set(np.unique(ref["source"]).tolist()) == {-1, 0} and ref["boxes"].shape == (0, 12)
    still = dict(WC.random_case(BIG, 12, K=6))
    still["pose"] = np.full((6, WC.POSE), np.nan)                   # no part has a pose: the same field
    same_bytes(run_select(dev, "all NaN", still)["dist"], ref["dist"], "NaN poses against K = 0")


@pytest.mark.parametrize("K,shape", [(65, BIG), (4096, (17, 16, 16))], ids=["K=65", "K=4096"])
def test_many_parts(dev, K, shape):
    cs = WC.many_parts_case(K, shape)
    ref = run_select(dev, ("many", K), cs)
    won = np.bincount(ref["source"][ref["source"] > 0], minlength=K + 1)[1:]
    assert (won[64:] > 0).any() and (won <= 1).all() and won.sum() >= K // 4
    if K == 65:
        mixed = WC.random_case(BIG, 14, K=65, specials=False)
        ref = run_select(dev, "65 blocks", mixed)
        assert (ref["source"] > 64).any(), "no part of the second ballot word wins"


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_case():
    cs = WC.random_case(BIG, 12, K=6)
    return cs, select_ref("9x10x17 mixed specials", cs)["source"]


@pytest.mark.parametrize("widths", [((1, None), (3, 5), (16, None), (17, 19)), ((16, 20), (20, None), (20, 21), (17, None)), ((384, None),), ((384, 388), (3, None))],
                         ids=["1 3 16 17", "16 20 20 17 strided", "384", "384 strided 3"])
@pytest.mark.parametrize("listed", [False, True], ids=["every voxel", "list"])
def test_rows(dev, rows_case, widths, listed):
    cs, source = rows_case
    rng = np.random.default_rng(len(widths))
    sets = []
    for s, (C, stride) in enumerate(widths):
        full, _ = WC.rows_data(cs["shape"], C, 100 + C, stride=stride)
        sets.append((full, C, rng.normal(size=C).astype(np.float32) if s % 2 == 0 else None))      # fills given and NULL
    voxels = WC.voxel_list(source.size, 7) if listed else None
    got = run_rows(dev, (widths, listed), cs["shape"], source, cs["pose"], sets, voxels=voxels)
    src = source.reshape(-1) if voxels is None else source.reshape(-1)[voxels]
    assert {-1, 0} < set(src.tolist()) and (src > 0).sum() >= 5
    assert np.array_equal(got[1], (src >= 0).astype(np.uint8))


def test_rows_without_sets_and_outside_entries(dev, rows_case):
    cs, source = rows_case
    voxels = np.int32([0, source.size - 1, -1, source.size, 5, 5])
    full, _ = WC.rows_data(cs["shape"], 3, 9)
    got = run_rows(dev, "outside", cs["shape"], source, cs["pose"], [(full, 3, np.float32([1, 2, 3]))], voxels=voxels)
    assert got[1][2] == 0 and got[1][3] == 0 and (got[0][0][2:4] == np.float32([1, 2, 3])).all()
    run_rows(dev, "no set", cs["shape"], source, cs["pose"], [], voxels=voxels)


# ---- band ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def band_case():
    """a banded source from band_cases: the 16 x 12 x 14 sphere with holes at band = h, two sets; three block parts shifted and turned"""
    name = "large sphere holes band 1h"
    vol = BC.volume(name, channels=(3, 20), fills=(1,))
    m = BC.mark(vol, BC.band_of(name))
    shape = vol["shape"]
    rng = np.random.default_rng(31)
    owner = np.zeros(shape, np.int32)
    owner[2:8, 2:7, 3:9], owner[9:14, 5:11, 6:12], owner[3:7, 8:11, 2:6] = 1, 2, 3
    centre = np.float64([5, 4, 6])
    pose = np.array([WC.shift_row((2, 1, -1)), WC.pose_row(WC.rotation(rng.normal(size=3), math.radians(10)), (11, 8, 9), (10.4, 7.2, 8.7)),
                     WC.pose_row(WC.QUARTER_Z, centre, centre + [0, 4, 0])])
    valid = vol["valid"].astype(np.uint8)
    return vol, m, owner, pose, WC.warp_ref(vol["dist"], valid, owner, pose)


def test_band(dev, band_case):
    vol, m, owner, pose, ref = band_case
    shape = vol["shape"]
    got = select_once(dev, vol["dist"], vol["valid"].astype(np.uint8), owner, pose)
    for k in ("source", "dist", "valid", "boxes"):
        same_bytes(got[k], ref[k], ("band select", k))
    assert (ref["source"] > 0).sum() >= 30
    sets = [(np.ascontiguousarray(vol["sets"][k].reshape(-1, vol["sets"][k].shape[-1])[m["voxels"]]), vol["sets"][k].shape[-1], vol["fills"][k]) for k in ("s0", "s1")]
    band = (m["slot"], m["cell_band"].astype(np.uint8), m["M"])
    rows, known = run_rows(dev, "band", shape, ref["source"], pose, sets, band=band)
    src = ref["source"].reshape(-1)
    assert 0 < known.sum() < (src >= 0).sum(), "the band keeps some rows and not all"
    assert not known[src < 0].any() and not known[(src == 0) & (m["slot"].reshape(-1) < 0)].any() and known[(src == 0) & (m["slot"].reshape(-1) >= 0)].all()
    assert (known[src > 0] == 0).any() and (known[src > 0] == 1).any(), "moved voxels inside and outside the band"
    assert (rows[1][known == 0] == vol["fills"]["s1"]).all() and (rows[0][known == 0] == 0).all()
    dense = [(np.ascontiguousarray(vol["sets"][k].reshape(-1, vol["sets"][k].shape[-1])), vol["sets"][k].shape[-1], vol["fills"][k]) for k in ("s0", "s1")]
    full, _ = run_rows(dev, "band's dense twin", shape, ref["source"], pose, dense)
    for s in range(2):
        same_bytes(rows[s][known == 1], full[s][known == 1], ("a known row equals the dense field's", s))
    lst = WC.voxel_list(src.size, 5)
    run_rows(dev, "band list", shape, ref["source"], pose, sets, voxels=lst, band=band)
    # an empty band: NULL slot, cell_band and data; every row is the fill row
    rows, known = run_rows(dev, "empty band", shape, ref["source"], pose, [(None, 3, None), (None, 20, vol["fills"]["s1"])], band=(None, None, 0))
    assert not known.any() and (rows[0] == 0).all() and (rows[1] == vol["fills"]["s1"]).all()


# ---- BakedField.owners / .warp ------------------------------------------------------------------------------------------------------
def test_api_owners(dev):
    labels = np.zeros((9, 10, 11), np.int32)
    labels[1:4, 1:4, 1:5], labels[5:8, 5:9, 6:9], labels[8, 0, 10] = 1, 2, 3
    f = BakedField.from_arrays((0.0, 0.0, 0.0), 0.02, torch.ones(labels.shape, device=dev))
    lab = up(dev, labels, np.int32)
    assert f.owners(lab, margin_voxels=0).data_ptr() == lab.data_ptr()
    for margin in (1, 2, 2.5, 30):
        want, unique = WC.owners_ref(labels, margin)
        got = f.owners(lab, margin_voxels=margin).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got[unique], want[unique]) and np.array_equal(got > 0, want > 0), margin
        assert np.array_equal(got[labels > 0], labels[labels > 0])
    assert (f.owners(lab, margin_voxels=30).cpu().numpy() > 0).all()
    parts = f.components(sites=lab > 0, connectivity=6)
    assert torch.equal(f.owners(parts, margin_voxels=2) > 0, f.owners(lab, margin_voxels=2) > 0)


@pytest.fixture(scope="module")
def api_case(dev):
    cs = WC.random_case(BIG, 12, K=6)
    origin, step = (1.0, -2.0, 0.5), 0.25                            # a power of two: the lattice points are exact in float32
    full3, d3 = WC.rows_data(cs["shape"], 3, 41)
    full20, d20 = WC.rows_data(cs["shape"], 20, 42)
    fill = np.float32(np.arange(20))
    f = BakedField.from_arrays(origin, step, up(dev, cs["dist"], np.float32), valid=up(dev, cs["valid"], np.uint8), fills={"b": up(dev, fill, np.float32)},
                               a=up(dev, d3, np.float32), b=up(dev, d20, np.float32))
    return cs, f, {"a": (full3, 3, None), "b": (full20, 20, fill)}


def lattice(f):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in f.grid_shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return torch.from_numpy((np.float32(f.origin) + idx.astype(np.float32) * np.float32(f.step)).astype(np.float32)).to(f.device)


def test_api_warp_dense(dev, api_case):
    cs, f, sets = api_case
    ref = select_ref("9x10x17 mixed specials", cs)
    raw = select_once(dev, cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    w = f.warp(up(dev, cs["pose"], np.float64), up(dev, cs["owner"], np.int32))
    assert isinstance(w, BakedField) and w.band is None and w.grid_shape == f.grid_shape and w.origin == f.origin and w.step == f.step and w.names() == ["a", "b"]
    for have, key in ((w.source, "source"), (w.dist, "dist"), (w.valid.view(torch.uint8), "valid")):
        same_bytes(have.cpu().numpy(), raw[key], ("warp", key))
        same_bytes(raw[key], ref[key], ("raw", key))
    same_bytes(torch.cat((w.part_box_from.reshape(-1, 6), w.part_box_to.reshape(-1, 6)), dim=1).cpu().numpy(), raw["boxes"], "boxes")
    assert w.valid.dtype == torch.bool and w.rows_known.dtype == torch.bool and tuple(w.part_box_to.shape) == (6, 2, 3)
    rows, known = rows_once(dev, cs["shape"], ref["source"], cs["pose"], [sets["a"], sets["b"]], None, None)
    same_bytes(w._sets["a"].reshape(-1, 3).cpu().numpy(), rows[0], "set a")
    same_bytes(w._sets["b"].reshape(-1, 20).cpu().numpy(), rows[1], "set b")
    same_bytes(w.rows_known.view(torch.uint8).reshape(-1).cpu().numpy(), known, "known")
    only_b = f.warp(up(dev, cs["pose"], np.float64), up(dev, cs["owner"], np.int32), return_names=["b"])
    assert only_b.names() == ["b"] and torch.equal(only_b._sets["b"], w._sets["b"])
    # the result is an ordinary field: its lookup at the lattice points of valid cells gives its arrays back
    out = w.eval(lattice(w))
    ok = out["valid_mask"].cpu().numpy()
    assert 10 < ok.sum() < ok.size
    assert np.array_equal(out["dist"].cpu().numpy()[ok], w.dist.reshape(-1).cpu().numpy()[ok])
    for k, C in (("a", 3), ("b", 20)):
        assert np.array_equal(out[k].cpu().numpy()[ok], w._sets[k].reshape(-1, C).cpu().numpy()[ok]), k
    assert w.components().count >= 1 and w.clearance().dist.shape == w.dist.shape


def test_api_which_leaves_unselected_parts_alone(dev, api_case):
    cs, f, sets = api_case
    pose, owner = up(dev, cs["pose"], np.float64), up(dev, cs["owner"], np.int32)
    none = f.warp(pose, owner, which=torch.zeros(6, dtype=torch.bool, device=dev))
    keep = (cs["valid"] != 0) & ~np.isnan(cs["dist"])
    assert np.array_equal(none.source.cpu().numpy(), np.where(keep, 0, -1))
    same_bytes(none.dist.cpu().numpy()[keep], cs["dist"][keep], "nothing selected: dist")
    for k in ("a", "b"):
        same_bytes(none._sets[k].cpu().numpy()[keep], f._sets[k].cpu().numpy()[keep], ("nothing selected", k))
    assert np.array_equal(none.rows_known.cpu().numpy(), keep)
    which = torch.zeros(6, dtype=torch.bool, device=dev)
    which[1] = True
    one = f.warp(pose, owner, which=which)
    want = WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], np.where(which.cpu().numpy()[:, None], cs["pose"], np.nan))
    same_bytes(one.source.cpu().numpy(), want["source"], "which: source")
    src = one.source.cpu().numpy()
    assert set(np.unique(src).tolist()) <= {-1, 0, 2} and (src == 2).any()
    others = keep & (cs["owner"] != 2) & (src == 0)                  # the unselected parts and the background: bit-identical to the source field
    assert (others & (cs["owner"] > 0)).any()
    same_bytes(one.dist.cpu().numpy()[others], cs["dist"][others], "which: dist of the others")
    same_bytes(one._sets["b"].cpu().numpy()[others], f._sets["b"].cpu().numpy()[others], "which: rows of the others")


def test_api_warp_banded(dev, band_case):
    vol, m, owner, pose, ref = band_case
    shape = vol["shape"]
    t = lambda a, dt: up(dev, a, dt)
    dense = BakedField.from_arrays(tuple(float(o) for o in vol["origin"]), float(vol["step"]), t(vol["dist"], np.float32), valid=t(vol["valid"], np.uint8),
                                   fills={"s1": t(vol["fills"]["s1"], np.float32)}, s0=t(vol["sets"]["s0"], np.float32), s1=t(vol["sets"]["s1"], np.float32))
    band = float(BC.band_of("large sphere holes band 1h"))
    src = dense.to_band(band)
    assert np.array_equal(src.slot.cpu().numpy(), m["slot"])
    w = src.warp(t(pose, np.float64), t(owner, np.int32))
    assert w.band == src.band and w.names() == ["s0", "s1"]
    same_bytes(w.source.cpu().numpy(), ref["source"], "banded warp: source")
    same_bytes(w.dist.cpu().numpy(), ref["dist"], "banded warp: dist")
    new = BC.mark({"shape": shape, "dist": ref["dist"], "valid": ref["valid"].astype(bool)}, np.float32(band))
    assert np.array_equal(w.slot.cpu().numpy(), new["slot"]) and np.array_equal(w.band_voxels.cpu().numpy(), new["voxels"]) and new["M"] > 0
    assert tuple(w.rows_known.shape) == (new["M"],)
    for k in ("s0", "s1"):
        C = vol["sets"][k].shape[-1]
        rows = np.ascontiguousarray(vol["sets"][k].reshape(-1, C)[m["voxels"]])
        want, known = WC.rows_ref(ref["source"], pose, rows, fill=vol["fills"][k], voxels=new["voxels"], slot=m["slot"], cell_band=m["cell_band"])
        assert tuple(w._sets[k].shape) == (new["M"], C)
        same_bytes(w._sets[k].cpu().numpy(), want, ("banded warp", k))
        same_bytes(w.rows_known.view(torch.uint8).cpu().numpy(), known, ("banded warp: known", k))
    out = w.eval(lattice(w))
    assert out["in_band"].any() and "s1" in out
    # the dense twin: the same selection, and the same rows wherever the banded result knows them
    wd = dense.warp(t(pose, np.float64), t(owner, np.int32))
    assert torch.equal(wd.source, w.source) and torch.equal(wd.dist, w.dist)
    at = w.band_voxels.long()[w.rows_known]
    assert torch.equal(wd._sets["s1"].reshape(-1, 20)[at], w._sets["s1"][w.rows_known])


def test_api_argument_errors_on_the_device(dev, api_case):
    cs, f, _ = api_case
    pose, owner = up(dev, cs["pose"], np.float64), up(dev, cs["owner"], np.int32)
    for bad in (lambda: f.warp(pose.cpu(), owner), lambda: f.warp(pose, owner.cpu()), lambda: f.warp(pose, owner, which=torch.ones(6, dtype=torch.bool)),
                lambda: f.owners(owner.cpu())):
        with pytest.raises(ValueError):
            bad()


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
def test_scene(dev):
    """Two observations of the synthetic scene of examples/flow_synthetic.py (one sphere moved by (2, -1, 0) voxels) at an 8 mm step:
    parts -> flow both ways -> consistent -> motions -> owners -> warp.  Relations only: the warped first observation overlaps the second
    better than the first itself does, and what is left for the flow from the second to find on the moved sphere is smaller."""
    spec = importlib.util.spec_from_file_location("flow_synthetic", os.path.join(ROOT, "examples", "flow_synthetic.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    from d3fields_amd import synth
    step, move = 0.008, (2, -1, 0)
    V, H, W = 4, 120, 160
    K, Rt = synth.ring_cameras(V, H, W)
    proto = np.random.default_rng(3).standard_normal((len(fs.NAMES), fs.C - 24)).astype(np.float32)
    before = list(synth._SPHERES)
    after = list(before)
    after[1] = tuple(c + m * step for c, m in zip(before[1][:3], move)) + (before[1][3],)
    a = fs.observe(before, K, Rt, H, W, proto, str(dev)).bake(synth.WORK_BOX, step, return_names=["mask", "feat"])
    b = fs.observe(after, K, Rt, H, W, proto, str(dev)).bake(synth.WORK_BOX, step, return_names=["mask", "feat"])
    iso = step
    fwd, back = a.flow(b, "feat", radius_voxels=3, iso=iso), b.flow(a, "feat", radius_voxels=3, iso=iso)
    parts = a.parts("mask", rule="argmax", iso=iso, min_voxels=30)
    pm = fwd.motions(parts, keep=fwd.consistent(back))
    which = pm.moved(min_shift=0.5 * step)
    assert 1 <= int(which.sum()) < pm.count, "the moved sphere, and not everything"
    w = a.warp(pm, a.owners(parts, margin_voxels=2), which=which)
    occupied = lambda f: f.valid & (f.dist <= iso)

    def iou(x, y):
        return float((x & y).sum()) / float((x | y).sum())

    # the overlap is measured where the moved sphere was or is: elsewhere the two observations agree and a warp changes nothing
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev) for n in a.grid_shape], indexing="ij"), dim=-1).double()
    world = torch.tensor(a.origin, dtype=torch.float64, device=dev) + grid * a.step
    near = lambda s: (world - torch.tensor(s[:3], dtype=torch.float64, device=dev)).norm(dim=-1) <= s[3] + 2 * step
    region = near(before[1]) | near(after[1])
    iou_before, iou_after = iou(occupied(a) & region, occupied(b) & region), iou(occupied(w) & region, occupied(b) & region)
    on_sphere = near(after[1]) & occupied(b)

    def residual(first):
        fl = b.flow(first, "feat", radius_voxels=3, iso=iso)
        sel = on_sphere & fl.matched
        assert int(sel.sum()) >= 20
        return float(fl.displacement(refined=False)[sel].norm(dim=-1).median()) / step

    res_before, res_after = residual(a), residual(w)
    print("scene: IoU with the second bake %.3f -> %.3f; median residual flow on the moved sphere %.2f -> %.2f voxels; %d of %d parts moved"
          % (iou_before, iou_after, res_before, res_after, int(which.sum()), pm.count))
    assert iou_after > iou_before
    assert res_after < res_before
