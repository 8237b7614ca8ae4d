"""CPU: the merge entry points (d3f_volume_merge_select, d3f_volume_merge_rows) live in the EXTENSION header include/d3fields_hip_ext.h and the
extension tables of _lib (the main header and its tables are closed by their count pins): tests/test_abi.py's checks applied to that pair; the
host structs have the header's layout; every documented status code comes back with a text that names the entry point; the NumPy restatement
(tests/merge_cases.py) equals a per-voxel loop byte for byte and has the properties a merge must have; the generator plants what it says it
plants, so that no GPU case is vacuous; merge_kernels.hip uses no scratch and names no fused operation and no atomic; the argument errors of
BakedField.merge need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import merge_cases as MC
import test_abi
from conftest import ROOT
from d3fields_amd import _lib, build

MAIN = os.path.join(ROOT, "include", "d3fields_hip.h")
EXT = os.path.join(ROOT, "include", "d3fields_hip_ext.h")
SOURCE = os.path.join(ROOT, "d3fields_amd", "csrc", "merge_kernels.hip")
SYMBOLS = ("d3f_volume_merge_select", "d3f_volume_merge_rows")


# ---- C ABI: the extension header and the extension tables ---------------------------------------------------------------------------
def test_extension_header_is_exported_and_bound(monkeypatch):
    """test_abi.py's two checks with the extension header in the main header's place and EXT_* in the place of SIGNATURES / STREAMED"""
    lib = _lib.load()
    main_names = test_abi.declared_functions()
    monkeypatch.setattr(test_abi, "HEADER", EXT)
    names = test_abi.declared_functions()
    assert names == sorted(SYMBOLS) == sorted(_lib.EXT_SIGNATURES)
    for n in names:
        assert hasattr(lib, n), "libd3fields_hip.so lacks %s" % n
    declared = test_abi.declared_signatures()
    assert sorted(declared) == names
    for name, (res, args) in _lib.EXT_SIGNATURES.items():
        ret, params, streamed = declared[name]
        assert test_abi._ctypes_kind(res) == ret == "int32_t", name
        assert [test_abi._ctypes_kind(a) for a in args] == params, name
        assert (name in _lib.EXT_STREAMED) == streamed, name
    assert _lib.EXT_STREAMED <= set(_lib.EXT_SIGNATURES)
    # the tables of the two headers are disjoint, and the main header declares neither new name (nor does its text mention them)
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES) and not _lib.EXT_STREAMED & _lib.STREAMED and not set(names) & set(main_names)
    assert "d3f_volume_merge" not in open(MAIN).read() and "d3f_merge_" not in open(MAIN).read()
    ext = open(EXT).read()
    assert '#include "d3fields_hip.h"' in ext and "added after the main table of ABI 16" in ext and "same libd3fields_hip.so" in ext
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16 and "D3F_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    for k, name in enumerate(("NONE", "KEEP", "NEW", "BLEND", "RESET")):
        assert int(re.search(r"#define D3F_MERGE_%s (\d+)" % name, ext).group(1)) == getattr(_lib, "MERGE_" + name) == getattr(MC, name) == k
    assert "merge_kernels.hip" in build.SOURCES and os.path.exists(SOURCE) and "d3fields_hip_ext.h" in build.PUBLIC_HEADERS
    assert not [fn for fn in _lib.EXT_SIGNATURES if fn.endswith("_workspace_bytes")], "the merge needs no workspace"
    import d3fields_amd
    assert hasattr(d3fields_amd.BakedField, "merge")
    assert [getattr(d3fields_amd.BakedField, "MERGE_" + n) for n in ("NONE", "KEEP", "NEW", "BLEND", "RESET")] == [0, 1, 2, 3, 4]


def test_on_accepts_both_tables_and_nothing_else():
    q = _lib.on("cpu", lib=_lib.load())
    for name in SYMBOLS + ("d3f_volume_warp_rows",):
        assert callable(getattr(q, name))
    with pytest.raises(AttributeError):
        q.d3f_volume_merge
    with pytest.raises(AttributeError):
        q.d3f_no_such_entry_point
    # a status other than OK raises, and the stream is appended: one struct, no further argument
    q.stream = None
    with pytest.raises(_lib.D3FError) as e:
        q.d3f_volume_merge_select(_lib.MergeSelect())
    assert e.value.code == _lib.ERR_BAD_SHAPE and "volume_merge_select" in str(e.value)
    with pytest.raises(_lib.D3FError) as e:
        q.d3f_volume_merge_rows(_lib.MergeRows())
    assert e.value.code == _lib.ERR_BAD_SHAPE and "volume_merge_rows" in str(e.value)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}


def header_struct(hdr, name):
    """a ctypes Structure built from the header's own text of `typedef struct name { ... } name;` (pointers and scalars)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        if "*" in decl:
            fields += [(re.findall(r"\w+", n)[-1], ctypes.c_void_p) for n in decl[decl.index("*"):].split(",")]
            continue
        ctype, rest = decl.replace("const ", "").split(None, 1)
        fields += [(n.strip(), C_TYPES[ctype]) for n in rest.split(",")]
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def test_struct_layouts_match_the_extension_header():
    hdr = open(EXT).read()
    for cname, bound in (("d3f_merge_select", _lib.MergeSelect), ("d3f_merge_rows", _lib.MergeRows)):
        want = header_struct(hdr, cname)
        assert ctypes.sizeof(bound) == ctypes.sizeof(want), cname
        assert [f[0] for f in bound._fields_] == [f[0] for f in want._fields_], cname
        for f in want._fields_:
            assert getattr(bound, f[0]).offset == getattr(want, f[0]).offset and getattr(bound, f[0]).size == getattr(want, f[0]).size, (cname, f[0])
    assert ctypes.sizeof(_lib.MergeSelect) == 120 and _lib.MergeSelect.dist_a.offset == 16 and _lib.MergeSelect.weight_a_all.offset == 64
    assert _lib.MergeSelect.gap.offset == 76 and _lib.MergeSelect.out_kind.offset == 112
    assert ctypes.sizeof(_lib.MergeRows) == 104 and _lib.MergeRows.band_a.offset == 16 and _lib.MergeRows.m.offset == 72 and _lib.MergeRows.reserved.offset == 96


def test_validation_status_codes():
    lib = _lib.load()
    p, odd4 = 256, 258
    v = ctypes.c_void_p
    inf, nan = float("inf"), float("nan")

    def select(shape=(4, 5, 6), reserved=0, da=p, va=p, wa=None, db=p, vb=p, wb=None, wa_all=1.0, wb_all=1.0, w_max=inf, gap=inf, dist=p, weight=p, beta=p, valid=p,
               kind=p, null=False):
        a = _lib.MergeSelect(shape[0], shape[1], shape[2], reserved, v(da), v(va), v(wa), v(db), v(vb), v(wb), wa_all, wb_all, w_max, gap, v(dist), v(weight), v(beta),
                             v(valid), v(kind))
        rc = lib.d3f_volume_merge_select(None if null else ctypes.byref(a), None)
        assert b"volume_merge_select" in lib.d3f_last_error()
        return rc

    assert select(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for name in ("da", "va", "db", "vb", "dist", "weight", "beta", "valid", "kind"):
        assert select(**{name: None}) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), name
    for shape in ((1, 5, 6), (4, 0, 6), (4, 5, -1), (2048, 1024, 1024)):
        assert select(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert b"2^31" in lib.d3f_last_error()
    assert select(reserved=1) == _lib.ERR_INVALID_ARG and b"reserved" in lib.d3f_last_error()
    for bad in (0.0, -1.0, inf, nan):
        assert select(wa_all=bad) == _lib.ERR_INVALID_ARG and b"weight_a_all" in lib.d3f_last_error(), bad
        assert select(wb_all=bad) == _lib.ERR_INVALID_ARG and b"weight_b_all" in lib.d3f_last_error(), bad
        assert select(wa_all=bad, wa=p, wb_all=bad, wb=p, dist=None) == _lib.ERR_INVALID_ARG and b"out_dist" in lib.d3f_last_error()      # with a volume the scalar is not read
    for bad in (0.0, -2.0, nan, -inf):
        assert select(w_max=bad) == _lib.ERR_INVALID_ARG and b"w_max" in lib.d3f_last_error(), bad
    for bad in (-1e-9, nan, -inf):
        assert select(gap=bad) == _lib.ERR_INVALID_ARG and b"gap" in lib.d3f_last_error(), bad
    assert select(gap=0.0, w_max=1e-30, dist=None) == _lib.ERR_INVALID_ARG and b"out_dist" in lib.d3f_last_error()     # the ends of both ranges pass
    for kw in ({"da": odd4}, {"wa": odd4}, {"db": odd4}, {"wb": odd4}, {"dist": odd4}, {"weight": odd4}, {"beta": odd4}):
        assert select(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    # precedence: struct, shape, scalars, NULL pointers, layout
    assert select(shape=(1, 5, 6), gap=nan, da=None, db=odd4) == _lib.ERR_BAD_SHAPE
    assert select(gap=nan, da=None, db=odd4) == _lib.ERR_INVALID_ARG and b"gap" in lib.d3f_last_error()
    assert select(da=None, db=odd4) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()

    def rows(shape=(4, 5, 6), band_a=None, band_b=None, data_a=p, data_b=p, C=8, C_b=None, word_a=0, word_b=0, stride_a=8, stride_b=8, fill=None, n_sets=1,
             kind=p, beta=p, voxels=p, m=10, out=p, known=p, reserved=0, null=False, no_sets=False, no_outs=False):
        sa = (_lib.VolumeSet * 1)(_lib.VolumeSet(data_a, C, word_a, stride_a, fill))
        sb = (_lib.VolumeSet * 1)(_lib.VolumeSet(data_b, C if C_b is None else C_b, word_b, stride_b, None))
        outs = (ctypes.c_void_p * 1)(out)
        ba = None if band_a is None else ctypes.pointer(_lib.Band(v(band_a[0]), v(band_a[1]), band_a[2]))
        bb = None if band_b is None else ctypes.pointer(_lib.Band(v(band_b[0]), v(band_b[1]), band_b[2]))
        a = _lib.MergeRows(shape[0], shape[1], shape[2], n_sets, ba, bb, None if no_sets else sa, None if no_sets else sb, v(kind), v(beta), v(voxels), m,
                           None if no_outs else outs, v(known), reserved)
        rc = lib.d3f_volume_merge_rows(None if null else ctypes.byref(a), None)
        assert b"volume_merge_rows" in lib.d3f_last_error()
        return rc

    assert rows(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for kw in ({"kind": None}, {"beta": None}, {"known": None}, {"no_sets": True}, {"no_outs": True}, {"out": None}, {"data_a": None}, {"data_b": None},
               {"band_a": (None, None, 5)}, {"band_b": (None, p, 5)}):
        assert rows(**kw) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), kw
    for shape in ((1, 5, 6), (4, 5, 1), (2048, 1024, 1024)):
        assert rows(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert rows(m=-1) == _lib.ERR_INVALID_ARG and b"m=" in lib.d3f_last_error()
    assert rows(voxels=None, m=10) == _lib.ERR_INVALID_ARG and b"voxel count" in lib.d3f_last_error()
    assert rows(reserved=3) == _lib.ERR_INVALID_ARG and b"reserved" in lib.d3f_last_error()
    for bad in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert rows(C=bad, stride_a=1 << 20, stride_b=1 << 20) == _lib.ERR_BAD_SHAPE and b"C=" in lib.d3f_last_error(), bad
    assert rows(C=8, C_b=4) == _lib.ERR_BAD_SHAPE and b"sets_a C=8 != sets_b C=4" in lib.d3f_last_error()
    assert rows(n_sets=-1) == _lib.ERR_BAD_SHAPE and rows(n_sets=_lib.MAX_MAPS + 1) == _lib.ERR_BAD_SHAPE
    for side in ("band_a", "band_b"):
        assert rows(**{side: (p, p, -1)}) == _lib.ERR_BAD_SHAPE and rows(**{side: (p, p, 2 ** 31)}) == _lib.ERR_BAD_SHAPE and b"n_rows" in lib.d3f_last_error()
    # the storage word: a half set is ACCEPTED on either side (these row loops have a half form), anything but 0 / 1 is a dtype error
    for kw in ({"word_a": 1}, {"word_b": 1}, {"word_a": 1, "word_b": 1}):
        assert rows(out=None, **kw) == _lib.ERR_INVALID_ARG and b"out_sets[0] is NULL" in lib.d3f_last_error(), kw      # past every check of the sets
    assert rows(word_a=1, data_a=258, m=0) == _lib.OK
    for kw in ({"word_a": 7}, {"word_b": 7}, {"word_a": -1}):
        assert rows(**kw) == _lib.ERR_BAD_DTYPE and b"storage word" in lib.d3f_last_error(), kw
    assert rows(stride_a=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    assert rows(stride_b=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    for kw in ({"beta": odd4}, {"voxels": odd4}, {"data_a": odd4}, {"data_b": odd4}, {"data_a": 257, "word_a": 1}, {"fill": odd4}, {"out": odd4}, {"band_a": (odd4, p, 5)},
               {"band_b": (odd4, p, 5)}):
        assert rows(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    assert rows(data_a=258, word_a=1, out=None) == _lib.ERR_INVALID_ARG                       # a half row needs 2-byte alignment only
    assert rows(m=0, kind=None, beta=None, known=None, out=None) == _lib.OK                   # nothing to do: nothing is read
    assert rows(band_a=(None, None, 0), data_a=None, band_b=(None, None, 0), data_b=None, out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0]" in lib.d3f_last_error()
    assert rows(band_a=(p, None, 5), out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0]" in lib.d3f_last_error()      # cell_band is not read
    # precedence: shape, dtype and scalars before NULL pointers before layout
    assert rows(shape=(1, 5, 6), m=-1, kind=None) == _lib.ERR_BAD_SHAPE
    assert rows(word_a=7, m=-1, kind=None, stride_a=7) == _lib.ERR_BAD_DTYPE
    assert rows(m=-1, kind=None, stride_a=7) == _lib.ERR_INVALID_ARG and b"m=" in lib.d3f_last_error()
    assert rows(kind=None, stride_a=7) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(rows(m=-1))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def select_of(cs, **kw):
    args = {"w_max": cs["w_max"], "gap": cs["gap"]}
    args.update(kw)
    return MC.select_ref(cs["da"], cs["va"], cs["wa"], cs["db"], cs["vb"], cs["wb"], **args)


@pytest.fixture(scope="module")
def cases():
    return {spec: MC.random_case(*spec) for spec in MC.RANDOM}


@pytest.mark.parametrize("spec", MC.RANDOM[:6], ids=MC.case_id)
def test_restatement_equals_the_loop_formulation(cases, spec):
    cs = cases[spec]
    for kw in ({}, {"gap": 0.0}, {"gap": np.inf, "w_max": np.inf}):
        ref = select_of(cs, **kw)
        args = {"w_max": cs["w_max"], "gap": cs["gap"]}
        args.update(kw)
        loop = MC.select_loop(cs["da"], cs["va"], cs["wa"], cs["db"], cs["vb"], cs["wb"], **args)
        for k in ("dist", "weight", "beta", "valid", "kind"):
            same(ref[k], loop[k], (spec, kw, k))
    scalar = MC.select_ref(cs["da"], cs["va"], 2.0, cs["db"], cs["vb"], cs["wb"], 3.0, cs["gap"])
    loop = MC.select_loop(cs["da"], cs["va"], 2.0, cs["db"], cs["vb"], cs["wb"], 3.0, cs["gap"])
    for k in ("dist", "weight", "beta", "valid", "kind"):
        same(scalar[k], loop[k], (spec, "scalar weight", k))
    ref = select_of(cs)
    n = ref["kind"].size
    for voxels in (None, MC.voxel_list(n, 1)[:40]):
        a = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=cs["fill"], voxels=voxels, slot_a=cs["slot_a"], slot_b=cs["slot_b"])
        b = MC.rows_loop(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=cs["fill"], voxels=voxels, slot_a=cs["slot_a"], slot_b=cs["slot_b"])
        same(a[0], b[0], (spec, "rows"))
        same(a[1], b[1], (spec, "known"))


def test_generated_arrays_are_read_only(cases):
    cs = cases[MC.RANDOM[1]]
    for k in ("da", "va", "wa", "db", "vb", "wb", "rows_a", "rows_b"):
        with pytest.raises(ValueError):
            cs[k][...] = 0


@pytest.mark.parametrize("spec", MC.RANDOM, ids=MC.case_id)
def test_generator_conditions(cases, spec):
    """no case is vacuous: every kind on at least 5 % of the voxels; a band stores 20-80 % of them; over the kind-3 voxels of a banded case
    at least 5 % have exactly one row stored in a band and at least 5 % none (counting the banded sides: a dense side always has its row)"""
    cs = cases[spec]
    ref = select_of(cs)
    kind = ref["kind"].reshape(-1)
    n = kind.size
    for k in MC.KINDS:
        assert (kind == k).sum() >= 0.05 * n and (kind == k).sum() >= 1, (spec, k)
    banded = [cs[s] for s in ("slot_a", "slot_b") if cs[s] is not None]
    for slot in banded:
        assert 0.2 * n <= (slot >= 0).sum() <= 0.8 * n, spec
    if banded:
        stored = sum((slot.reshape(-1) >= 0).astype(int) for slot in banded)[kind == MC.BLEND]
        assert (stored == 1).sum() >= 0.05 * stored.size and (stored == 1).sum() >= 1 and (stored == 0).sum() >= 0.05 * stored.size and (stored == 0).sum() >= 1, spec
    # what the docstring of random_case promises (the eight voxels of 2x2x2 hold one or two of each kind and cannot hold every special)
    va, vb = cs["va"].reshape(-1) != 0, cs["vb"].reshape(-1) != 0
    for d, wv, valid in ((cs["da"], cs["wa"], va), (cs["db"], cs["wb"], vb)):
        assert np.isnan(d.reshape(-1)[~valid]).all() and np.isnan(wv.reshape(-1)[~valid]).all() and (~valid).any()
    t = cs["tie"]
    assert t >= 0 and np.abs(cs["da"].reshape(-1)[t] - cs["db"].reshape(-1)[t]) == cs["gap"] and kind[t] == MC.BLEND
    if n == 8:
        return
    assert np.isnan(cs["da"].reshape(-1)[va]).any() and np.isnan(cs["db"].reshape(-1)[vb]).any()
    w = np.concatenate([cs["wa"].reshape(-1)[va], cs["wb"].reshape(-1)[vb]])
    assert np.isnan(w).any() and (w == 0).any() and (w < 0).any() and np.isinf(w).any(), spec
    for side in ("a", "b"):
        rows = cs["rows_" + side].reshape(-1)
        assert (np.signbit(rows) & (rows == 0)).any() and ((rows != 0) & (np.abs(rows) < np.finfo(rows.dtype).tiny)).any(), (spec, side)
        assert np.isnan(rows).any()
    o = cs["overflow"]
    assert o >= 0 and float(cs["wa"].reshape(-1)[o]) + float(cs["wb"].reshape(-1)[o]) > float(np.finfo(np.float32).max) and kind[o] == MC.BLEND
    assert cs["equal"] >= 0 and kind[cs["equal"]] == MC.BLEND


def test_merging_a_field_with_itself_gives_the_field(cases):
    for spec in MC.RANDOM[:6]:
        cs = cases[spec]
        ref = MC.select_ref(cs["da"], cs["va"], cs["wa"], cs["da"], cs["va"], cs["wa"], np.inf, np.inf)
        ok = MC.usable(cs["da"], cs["va"], cs["wa"])
        assert ((ref["kind"] == MC.BLEND) == ok).all() and ((ref["kind"] == MC.NONE) == ~ok).all()
        same(ref["dist"][ok], cs["da"][ok], (spec, "dist"))
        rows, known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_a"], slot_a=cs["slot_a"], slot_b=cs["slot_a"])
        full = cs["rows_a"].astype(np.float32)
        if cs["slot_a"] is None:
            have = ok.reshape(-1)
            want = full.reshape(-1, cs["C"])[have]
        else:
            have = ok.reshape(-1) & (cs["slot_a"].reshape(-1) >= 0)
            want = full[cs["slot_a"].reshape(-1)[have]]
        assert np.array_equal(known != 0, have)
        # a + beta*(a - a) = a + 0 = a bit for bit -- but for a = -0, where -0 + +0 is +0, and for a NaN entry, which stays a NaN
        got = rows[have]
        num = ~np.isnan(want)
        assert np.isnan(got[~num]).all() and np.array_equal(got[num], want[num])
        assert (got.view(np.uint32) == want.view(np.uint32))[num & (want != 0)].all() and (num & (want != 0)).sum() > want.size // 2


def test_kinds_1_2_4_are_bit_copies_and_the_gap_rule_is_strict(cases):
    cs = cases[MC.RANDOM[3]]
    ref = select_of(cs)
    kind = ref["kind"]
    for k, d, w, beta in ((MC.KEEP, cs["da"], cs["wa"], 0.0), (MC.NEW, cs["db"], cs["wb"], 1.0), (MC.RESET, cs["db"], cs["wb"], 1.0)):
        sel = kind == k
        same(ref["dist"][sel], d[sel], k)
        same(ref["weight"][sel], w[sel], k)
        assert (ref["beta"][sel] == beta).all() and ref["valid"][sel].all()
    none = kind == MC.NONE
    assert (ref["dist"][none] == MC.SENTINEL).all() and (ref["weight"][none] == 0).all() and not ref["valid"][none].any()
    rows, known = MC.rows_ref(kind, ref["beta"], cs["rows_a"], cs["rows_b"], fill=cs["fill"])
    a, b = cs["rows_a"].astype(np.float32).reshape(-1, cs["C"]), cs["rows_b"].astype(np.float32).reshape(-1, cs["C"])
    flat = kind.reshape(-1)
    assert rows[flat == MC.KEEP].tobytes() == a[flat == MC.KEEP].tobytes() and np.isnan(rows[flat == MC.KEEP]).any()       # NaN payloads included
    for k in (MC.NEW, MC.RESET):
        assert rows[flat == k].tobytes() == b[flat == k].tobytes()
    assert (rows[flat == MC.NONE] == cs["fill"]).all() and np.array_equal(known, (flat != MC.NONE).astype(np.uint8))
    # the tie |da - db| == gap blends; one ulp less gap resets it
    t = np.unravel_index(cs["tie"], cs["shape"])
    assert kind[t] == MC.BLEND and select_of(cs, gap=np.nextafter(cs["gap"], np.float32(0)))["kind"][t] == MC.RESET
    assert (select_of(cs, gap=np.inf)["kind"] != MC.RESET).all()
    zero = select_of(cs, gap=0.0)
    both = MC.usable(cs["da"], cs["va"], cs["wa"]) & MC.usable(cs["db"], cs["vb"], cs["wb"])
    assert np.array_equal(zero["kind"] == MC.BLEND, both & (cs["da"] == cs["db"])) and (zero["kind"] == MC.BLEND).any()


def test_weight_cap_and_overflow(cases):
    cs = cases[MC.RANDOM[2]]
    ref, free = select_of(cs), select_of(cs, w_max=np.inf)
    blend = ref["kind"] == MC.BLEND
    with np.errstate(over="ignore"):
        s = cs["wa"][blend] + cs["wb"][blend]
    assert np.array_equal(ref["weight"][blend], np.minimum(s, cs["w_max"])) and (s > cs["w_max"]).any() and (s < cs["w_max"]).any()
    assert np.array_equal(free["weight"][blend], s)
    same(ref["dist"], free["dist"], "the cap does not touch the distances")
    o = np.unravel_index(cs["overflow"], cs["shape"])
    assert ref["beta"][o] == 0 and ref["weight"][o] == cs["w_max"] and ref["dist"][o].tobytes() == cs["da"][o].tobytes() and np.isinf(free["weight"][o])


def test_three_equal_merges_weight_the_frames_a_third_each():
    """x1, x2, x3 merged in a row with weight 1 each.  First merge: s = 2, beta = 1/2 exactly; d12 = x1 + (x2 - x1)/2 carries the rounding
    of the difference (|x2 - x1| <= 2M, half of u*2M after the exact halving) and of the sum (u*M'): |d12 - (x1 + x2)/2| <= 2uM(1 + u),
    with u = 2^-24 and M = max |x|.  Second merge: the weights are 2 and 1, s = 3, beta = fl(1/3) = (1 + e)/3 with |e| <= u;
    d = d12 + fl(beta * fl(x3 - d12)): the error of d12 enters with the factor 1 - 1/3 (4uM/3), the difference rounds by u*2M and enters
    with 1/3 (2uM/3), beta's own error (2uM/3), the product's rounding (2uM/3), the sum's rounding (uM): 13uM/3 to first order.  The
    bound asserted is 5uM, which also covers the second-order terms."""
    rng = np.random.default_rng(5)
    shape = (6, 5, 7)
    x = [rng.uniform(-1, 1, shape).astype(np.float32) for _ in range(3)]
    ones = np.ones(shape, np.uint8)
    m12 = MC.select_ref(x[0], ones, 1.0, x[1], ones, 1.0)
    assert (m12["beta"] == 0.5).all() and (m12["weight"] == 2).all()
    m123 = MC.select_ref(m12["dist"], m12["valid"], m12["weight"], x[2], ones, 1.0)
    assert (m123["weight"] == 3).all() and (m123["beta"] == np.float32(1) / np.float32(3)).all() and (m123["kind"] == MC.BLEND).all()
    mean = (x[0].astype(np.float64) + x[1] + x[2]) / 3
    M = max(float(np.abs(v).max()) for v in x)
    assert np.abs(m123["dist"].astype(np.float64) - mean).max() <= 5 * 2.0 ** -24 * M
    rows = [v[..., None] for v in x]                 # the same chain on a one-channel set
    r12, _ = MC.rows_ref(m12["kind"], m12["beta"], rows[0], rows[1])
    r123, known = MC.rows_ref(m123["kind"], m123["beta"], r12.reshape(shape + (1,)), rows[2])
    same(r123.reshape(shape), m123["dist"], "rows take the distances' chain")
    assert known.all()


def test_rows_of_the_restatement(cases):
    cs = cases[MC.RANDOM[6]]                          # both banded
    ref = select_of(cs)
    n = ref["kind"].size
    rows, known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=cs["fill"], slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    flat, sa, sb = ref["kind"].reshape(-1), cs["slot_a"].reshape(-1), cs["slot_b"].reshape(-1)
    blend = flat == MC.BLEND
    only_a = blend & (sa >= 0) & (sb < 0)
    assert only_a.any() and rows[only_a].tobytes() == cs["rows_a"][sa[only_a]].tobytes()
    only_b = blend & (sa < 0) & (sb >= 0)
    assert only_b.any() and rows[only_b].tobytes() == cs["rows_b"][sb[only_b]].tobytes()
    neither = blend & (sa < 0) & (sb < 0)
    assert neither.any() and (rows[neither] == cs["fill"]).all() and not known[neither].any() and known[only_a].all() and known[only_b].all()
    lst = MC.voxel_list(n, 3)
    sub, sub_known = MC.rows_ref(ref["kind"], ref["beta"], cs["rows_a"], cs["rows_b"], fill=cs["fill"], voxels=lst, slot_a=cs["slot_a"], slot_b=cs["slot_b"])
    inside = (lst >= 0) & (lst < n)
    assert sub[inside].tobytes() == rows[lst[inside]].tobytes() and np.array_equal(sub_known[inside], known[lst[inside]]) and lst[-1] == lst[0]
    assert (~inside).sum() >= 5 and (sub[~inside] == cs["fill"]).all() and not sub_known[~inside].any()
    empty = np.full(cs["shape"], -1, np.int32)
    rows0, known0 = MC.rows_ref(ref["kind"], ref["beta"], np.zeros((0, cs["C"]), np.float32), cs["rows_b"], slot_a=empty, slot_b=cs["slot_b"])
    has_b = np.isin(flat, (MC.NEW, MC.BLEND, MC.RESET)) & (sb >= 0)
    assert np.array_equal(known0 != 0, has_b) and rows0[has_b].tobytes() == cs["rows_b"][sb[has_b]].tobytes() and (rows0[~has_b] == 0).all()


# ---- BakedField.merge: argument errors ----------------------------------------------------------------------------------------------
def host_field(shape=(4, 5, 6), C=3, origin=(0.0, 0.0, 0.0)):
    import torch
    from d3fields_amd import BakedField
    f = object.__new__(BakedField)
    f.origin, f.step, f.grid_shape, f.device = origin, 0.1, torch.Size(shape), torch.device("cpu")
    f.dist, f.valid = torch.zeros(shape), torch.ones(shape, dtype=torch.bool)
    f._sets, f._fills, f.band = {"a": torch.zeros(shape + (C,))}, {"a": None}, None
    return f


def test_merge_argument_errors_need_no_device():
    import torch
    f, g = host_field(), host_field()
    shape = tuple(f.grid_shape)
    w = torch.ones(shape)
    nan, inf = float("nan"), float("inf")
    for bad in (lambda: f.merge(host_field(origin=(1.0, 0.0, 0.0))), lambda: f.merge(host_field(shape=(4, 5, 7))), lambda: f.merge(host_field(C=4)),
                lambda: f.merge(g, weight=0.0), lambda: f.merge(g, weight=-1.0), lambda: f.merge(g, weight=nan), lambda: f.merge(g, weight=inf),
                lambda: f.merge(g, other_weight=0.0), lambda: f.merge(g, other_weight=inf), lambda: f.merge(g, other_weight=w.double()),
                lambda: f.merge(g, other_weight=w[:-1]), lambda: f.merge(g, max_weight=0.0), lambda: f.merge(g, max_weight=-3), lambda: f.merge(g, max_weight=nan),
                lambda: f.merge(g, reset_gap=-1e-3), lambda: f.merge(g, reset_gap=nan), lambda: f.merge(g, band=0.0), lambda: f.merge(g, band=inf),
                lambda: f.merge(g, return_names=["a"] * (_lib.MAX_MAPS + 1))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: f.merge("field"), lambda: f.merge(None), lambda: f.merge(g, weight="1"), lambda: f.merge(g, weight=True), lambda: f.merge(g, other_weight=[1.0]),
                lambda: f.merge(g, max_weight="inf"), lambda: f.merge(g, reset_gap="0"), lambda: f.merge(g, band="thin")):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(KeyError):
        f.merge(g, return_names=["b"])
    g._sets["in_band"] = f._sets["in_band"] = torch.zeros(shape + (1,))
    with pytest.raises(ValueError):
        f.merge(g, band=0.01)
    del g._sets["in_band"], f._sets["in_band"]
    for ok in (lambda: f.merge(g), lambda: f.merge(g, other_weight=w, max_weight=inf, reset_gap=0.0), lambda: f.merge(g, weight=2, max_weight=8, reset_gap=inf, band=0.01)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ok()                                     # every argument is fine: there is no CPU path


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "merge_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    want = ["merge_select_kernel"] + ["merge_rows_kernelILb%dELb%dELb%dE" % (w, a, b) for w in (0, 1) for a in (0, 1) for b in (0, 1)]
    for kernel in want:
        assert kernel in names, (kernel, out[-800:])
    assert len(rows) == len(want)
    for name, scratch, occ in rows:
        assert scratch == 0 and occ >= 4, (name, scratch, occ)


def test_source_names_no_fused_operation_no_atomic_and_no_lds():
    src = open(SOURCE).read().lower()
    assert "fma" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.findall(r"\batomic\w*", code) and "__shared__" not in code and "__syncthreads" not in code
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
