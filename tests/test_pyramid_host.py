"""CPU: the pyramid's entry points (d3f_volume_coarsen_select, d3f_volume_coarsen_rows, d3f_volume_flow_seeded) live in a header of their own,
include/d3fields_hip_pyramid.h, bound through _lib.FEATURE_TABLES: tests/test_abi.py's checks applied to EVERY entry of that table, each
header against its own signatures, so that the next feature adds a header and an entry and no test breaks; the host structs have the header's
layout; every documented status code comes back from calls that launch nothing; the NumPy restatements (tests/pyramid_cases.py) equal their
loop formulations byte for byte, the means lie within gamma_9 of float64, and the case set holds what it must; the seeded restatement with a
zero seed is flow_cases.flow_ref; Flow.seed on hand-made numbers; the whole coarse-to-fine chain restated on a small scene; the two new
sources use no scratch and name no fused operation; the argument errors of the Python entry points need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_cases as FC
import pyramid_cases as PC
import test_abi
from conftest import ROOT
from d3fields_amd import _lib, build

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "d3fields_hip_pyramid.h")
SOURCES = ("pyramid_kernels.hip", "flow_seeded_kernels.hip")
SYMBOLS = ("d3f_volume_coarsen_rows", "d3f_volume_coarsen_select", "d3f_volume_flow_seeded")


# ---- C ABI: every feature header against its own table -----------------------------------------------------------------------------
def test_every_feature_header_is_exported_and_bound(monkeypatch):
    lib = _lib.load()
    assert "d3fields_hip_pyramid.h" in _lib.FEATURE_TABLES
    seen = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES)
    for header, (signatures, streamed) in _lib.FEATURE_TABLES.items():
        path = os.path.join(INCLUDE, header)
        assert os.path.exists(path) and header in build.PUBLIC_HEADERS, header
        monkeypatch.setattr(test_abi, "HEADER", path)
        names = test_abi.declared_functions()
        assert names == sorted(signatures), header
        declared = test_abi.declared_signatures()
        assert sorted(declared) == names, header
        for name, (res, args) in signatures.items():
            assert hasattr(lib, name), "libd3fields_hip.so lacks %s" % name
            ret, params, has_stream = declared[name]
            assert test_abi._ctypes_kind(res) == ret, name
            assert [test_abi._ctypes_kind(a) for a in args] == params, name
            assert (name in streamed) == has_stream, name
        assert set(streamed) <= set(signatures), header
        assert not set(signatures) & seen, "%s declares a name another table holds" % header
        seen |= set(signatures)
        text = open(path).read()
        assert '#include "d3fields_hip.h"' in text and "same libd3fields_hip.so" in text, header
        assert "D3F_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S), header
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    # this feature
    assert sorted(_lib.FEATURE_TABLES["d3fields_hip_pyramid.h"][0]) == list(SYMBOLS)
    for other in ("d3fields_hip.h", "d3fields_hip_ext.h"):
        text = open(os.path.join(INCLUDE, other)).read()
        assert "coarsen" not in text and "flow_seeded" not in text, other
    for src in SOURCES:
        assert src in build.SOURCES and os.path.exists(os.path.join(ROOT, "d3fields_amd", "csrc", src))
    assert int(re.search(r"#define D3F_FLOW_SEED_MAX (\d+)", open(HEADER).read()).group(1)) == _lib.FLOW_SEED_MAX == PC.SEED_MAX
    import d3fields_amd
    for method in ("coarsen", "pyramid", "flow_pyramid"):
        assert hasattr(d3fields_amd.BakedField, method)
    assert hasattr(d3fields_amd.Flow, "seed")


def test_on_accepts_the_feature_tables():
    q = _lib.on("cpu", lib=_lib.load())
    for name in SYMBOLS + ("d3f_volume_merge_rows", "d3f_volume_flow"):
        assert callable(getattr(q, name))
    for name in ("d3f_volume_coarsen", "d3f_volume_flow_seed"):
        with pytest.raises(AttributeError):
            getattr(q, name)
    q.stream = None      # a status other than OK raises, and the stream is appended: one struct, no further argument
    for name, struct in (("d3f_volume_coarsen_select", _lib.CoarsenSelect), ("d3f_volume_coarsen_rows", _lib.CoarsenRows)):
        with pytest.raises(_lib.D3FError) as e:
            getattr(q, name)(struct())
        assert e.value.code == _lib.ERR_BAD_SHAPE and name[4:] in str(e.value)
    with pytest.raises(_lib.D3FError) as e:
        q.d3f_volume_flow_seeded(_lib.FlowSeeded())
    assert e.value.code == _lib.ERR_INVALID_ARG and "volume_flow_seeded" in str(e.value)


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


def test_struct_layouts_match_the_header():
    hdr = open(HEADER).read()
    for cname, bound in (("d3f_coarsen_select", _lib.CoarsenSelect), ("d3f_coarsen_rows", _lib.CoarsenRows), ("d3f_flow_seeded", _lib.FlowSeeded)):
        want = header_struct(hdr, cname)
        assert ctypes.sizeof(bound) == ctypes.sizeof(want), cname
        assert [f[0] for f in bound._fields_] == [f[0] for f in want._fields_], cname
        for f in want._fields_:
            assert getattr(bound, f[0]).offset == getattr(want, f[0]).offset and getattr(bound, f[0]).size == getattr(want, f[0]).size, (cname, f[0])
    assert ctypes.sizeof(_lib.CoarsenSelect) == 64 and _lib.CoarsenSelect.dist.offset == 16 and _lib.CoarsenSelect.reserved.offset == 56
    assert ctypes.sizeof(_lib.CoarsenRows) == 80 and _lib.CoarsenRows.band.offset == 16 and _lib.CoarsenRows.m.offset == 48 and _lib.CoarsenRows.reserved.offset == 72
    assert ctypes.sizeof(_lib.FlowSeeded) == 104 and _lib.FlowSeeded.nx.offset == 56 and _lib.FlowSeeded.max_cost2.offset == 72 and _lib.FlowSeeded.out_target.offset == 80


def test_validation_status_codes():
    lib = _lib.load()
    p, odd4 = 256, 258
    v = ctypes.c_void_p
    nan = float("nan")

    def select(shape=(4, 5, 6), mc=1, dist=p, valid=p, od=p, ov=p, oc=p, reserved=0, null=False):
        a = _lib.CoarsenSelect(shape[0], shape[1], shape[2], mc, v(dist), v(valid), v(od), v(ov), v(oc), reserved)
        rc = lib.d3f_volume_coarsen_select(None if null else ctypes.byref(a), None)
        assert b"volume_coarsen_select" in lib.d3f_last_error()
        return rc

    assert select(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for name in ("dist", "valid", "od", "ov", "oc"):
        assert select(**{name: None}) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), name
    for shape in ((0, 5, 6), (4, -1, 6), (4, 5, 16385), (2048, 1024, 1024)):
        assert select(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert select(shape=(1, 1, 1), od=None) == _lib.ERR_INVALID_ARG       # the C level takes extents from 1
    for bad in (0, 9, -1):
        assert select(mc=bad) == _lib.ERR_INVALID_ARG and b"min_children" in lib.d3f_last_error(), bad
    assert select(mc=8, od=None) == _lib.ERR_INVALID_ARG and b"out_dist" in lib.d3f_last_error()
    assert select(reserved=1) == _lib.ERR_INVALID_ARG and b"reserved" in lib.d3f_last_error()
    for kw in ({"dist": odd4}, {"od": odd4}):
        assert select(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    # precedence: struct, shape, scalars, NULL pointers, layout
    assert select(shape=(0, 5, 6), mc=0, dist=None, od=odd4) == _lib.ERR_BAD_SHAPE
    assert select(mc=0, dist=None, od=odd4) == _lib.ERR_INVALID_ARG and b"min_children" in lib.d3f_last_error()
    assert select(dist=None, od=odd4) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()

    def rows(shape=(4, 5, 6), band=None, data=p, C=8, word=0, stride=8, fill=None, n_sets=1, children=p, voxels=p, m=10, out=p, known=p, reserved=0, null=False,
             no_sets=False, no_outs=False):
        sets = (_lib.VolumeSet * 1)(_lib.VolumeSet(data, C, word, stride, fill))
        outs = (ctypes.c_void_p * 1)(out)
        b = None if band is None else ctypes.pointer(_lib.Band(v(band[0]), v(band[1]), band[2]))
        a = _lib.CoarsenRows(shape[0], shape[1], shape[2], n_sets, b, None if no_sets else sets, v(children), v(voxels), m, None if no_outs else outs, v(known), reserved)
        rc = lib.d3f_volume_coarsen_rows(None if null else ctypes.byref(a), None)
        assert b"volume_coarsen_rows" in lib.d3f_last_error()
        return rc

    assert rows(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for kw in ({"children": None}, {"known": None}, {"no_sets": True}, {"no_outs": True}, {"out": None}, {"data": None}, {"band": (None, None, 5)}):
        assert rows(**kw) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), kw
    for shape in ((0, 5, 6), (4, 5, -2), (2048, 1024, 1024)):
        assert rows(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert rows(m=-1) == _lib.ERR_INVALID_ARG and b"m=" in lib.d3f_last_error()
    assert rows(voxels=None, m=10) == _lib.ERR_INVALID_ARG and b"coarse voxel count 18" in lib.d3f_last_error()
    assert rows(voxels=None, m=18, out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0]" in lib.d3f_last_error()
    assert rows(reserved=3) == _lib.ERR_INVALID_ARG and b"reserved" in lib.d3f_last_error()
    for bad in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert rows(C=bad, stride=1 << 20) == _lib.ERR_BAD_SHAPE and b"C=" in lib.d3f_last_error(), bad
    assert rows(n_sets=-1) == _lib.ERR_BAD_SHAPE and rows(n_sets=_lib.MAX_MAPS + 1) == _lib.ERR_BAD_SHAPE
    assert rows(band=(p, p, -1)) == _lib.ERR_BAD_SHAPE and rows(band=(p, p, 2 ** 31)) == _lib.ERR_BAD_SHAPE and b"n_rows" in lib.d3f_last_error()
    # the storage word: a half set is ACCEPTED (these row loops have a half form), anything but 0 / 1 is a dtype error
    assert rows(word=1, out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0] is NULL" in lib.d3f_last_error()
    for bad in (7, -1, 2):
        assert rows(word=bad) == _lib.ERR_BAD_DTYPE and b"storage word" in lib.d3f_last_error(), bad
    assert rows(stride=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    for kw in ({"voxels": odd4}, {"data": odd4}, {"data": 257, "word": 1}, {"fill": odd4}, {"out": odd4}, {"band": (odd4, p, 5)}):
        assert rows(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    assert rows(data=258, word=1, out=None) == _lib.ERR_INVALID_ARG                           # a half row needs 2-byte alignment only
    assert rows(m=0, children=None, known=None, out=None, data=None) == _lib.OK               # nothing to do: nothing is read
    assert rows(band=(None, None, 0), data=None, out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0]" in lib.d3f_last_error()
    assert rows(band=(p, None, 5), out=None) == _lib.ERR_INVALID_ARG and b"out_sets[0]" in lib.d3f_last_error()      # cell_band is not read
    # precedence
    assert rows(shape=(0, 5, 6), m=-1, children=None) == _lib.ERR_BAD_SHAPE
    assert rows(word=7, m=-1, children=None, stride=7) == _lib.ERR_BAD_DTYPE
    assert rows(m=-1, children=None, stride=7) == _lib.ERR_INVALID_ARG and b"m=" in lib.d3f_last_error()
    assert rows(children=None, stride=7) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()

    def seeded(shape=(4, 5, 6), site_a=p, slot_a=None, data_a=p, site_b=p, slot_b=None, data_b=p, C=8, C_b=None, word_a=0, word_b=0, stride_a=8, stride_b=8, seed=p,
               radius=1, max_cost2=1.0, reserved=0, target=p, cost=p, axis=None, null=False, no_set=False):
        sa = (_lib.VolumeSet * 1)(_lib.VolumeSet(data_a, C, word_a, stride_a, None))
        sb = (_lib.VolumeSet * 1)(_lib.VolumeSet(data_b, C if C_b is None else C_b, word_b, stride_b, None))
        a = _lib.FlowSeeded(v(site_a), v(slot_a), None if no_set else sa, v(site_b), v(slot_b), sb, v(seed), shape[0], shape[1], shape[2], radius, max_cost2, reserved,
                            v(target), v(cost), v(axis))
        rc = lib.d3f_volume_flow_seeded(None if null else ctypes.byref(a), None)
        assert b"volume_flow_seeded" in lib.d3f_last_error()
        return rc

    assert seeded(null=True) == _lib.ERR_INVALID_ARG
    for kw in ({"site_a": None}, {"site_b": None}, {"no_set": True}, {"data_a": None}, {"data_b": None}, {"target": None}, {"cost": None}):
        assert seeded(**kw) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), kw
    for bad in (0, 5, -1):
        assert seeded(radius=bad) == _lib.ERR_INVALID_ARG and b"radius" in lib.d3f_last_error()
    assert seeded(max_cost2=nan) == _lib.ERR_INVALID_ARG and b"NaN" in lib.d3f_last_error()
    assert seeded(reserved=2) == _lib.ERR_INVALID_ARG and b"reserved" in lib.d3f_last_error()
    for shape in ((0, 5, 6), (4, 5, 16385), (2048, 1024, 1024)):
        assert seeded(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert seeded(C=0) == _lib.ERR_BAD_SHAPE and seeded(C=8, C_b=4, stride_b=8) == _lib.ERR_BAD_SHAPE and b"same width" in lib.d3f_last_error()
    for kw in ({"word_a": 1}, {"word_b": 1}, {"word_a": 7}):                                    # a half set: the rule of d3f_volume_flow
        assert seeded(**kw) == _lib.ERR_BAD_DTYPE, kw
    assert seeded(stride_a=7) == _lib.ERR_BAD_LAYOUT and seeded(stride_b=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    for kw in ({"slot_a": odd4}, {"slot_b": odd4}, {"seed": odd4}, {"target": odd4}, {"cost": odd4}, {"axis": odd4}, {"data_a": odd4}):
        assert seeded(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("shape", PC.SHAPES[:4], ids=str)
def test_coarsen_restatement_equals_the_loop_formulation(shape):
    for C, half in ((5, False), (8, True)):
        cs = PC.coarsen_case(shape, C, 11, half)
        for mc in PC.MIN_CHILDREN:
            ref, loop = PC.coarsen_ref(cs["dist"], cs["valid"], mc), PC.coarsen_loop(cs["dist"], cs["valid"], mc)
            for k in ("dist", "valid", "children"):
                same(ref[k], loop[k], (shape, mc, k))
        children = PC.coarsen_ref(cs["dist"], cs["valid"])["children"]
        for kw in ({"rows": cs["rows"]}, {"rows": cs["rows"], "voxels": cs["voxels"], "fill": cs["fill"]},
                   {"rows": cs["banded"], "slot": cs["slot"], "voxels": cs["voxels"], "fill": cs["fill"]}):
            a, b = PC.rows_ref(children, shape, **kw), PC.rows_loop(children, shape, **kw)
            assert PC.same_rows(a[0], b[0]), (shape, C, sorted(kw))
            same(a[1], b[1], (shape, C, "known"))


def test_coarsen_means_lie_within_gamma_9_of_float64():
    """eight additions and one multiplication by a rounded reciprocal: |fl - exact| <= gamma_9 * mean(|d|) with gamma_k = k u / (1 - k u), u = 2^-24
    (the division's rounding is one of the nine)"""
    u = 2.0 ** -24
    gamma = 9 * u / (1 - 9 * u)
    rng = np.random.default_rng(3)
    shape = (8, 8, 8)
    dist = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)
    valid = (rng.random(shape) < 0.8).astype(np.uint8)
    ref = PC.coarsen_ref(dist, valid)
    q, inside = PC.child_index(shape)
    ok = inside & (valid.reshape(-1)[q] != 0)
    d = np.where(ok, dist.reshape(-1)[q].astype(np.float64), 0.0)
    count = ok.sum(-1)
    live = count > 0
    exact = d.sum(-1)[live] / count[live]
    bound = gamma * np.abs(d).sum(-1)[live] / count[live]
    assert live.sum() > 50 and (np.abs(ref["dist"][live].astype(np.float64) - exact) <= bound).all()
    assert (ref["valid"] != 0).tobytes() == live.tobytes()
    rows = rng.standard_normal(shape + (3,)).astype(np.float32)
    out, known = PC.rows_ref(ref["children"], shape, rows)
    r = np.where(ok[..., None], rows.reshape(-1, 3)[q].astype(np.float64), 0.0)
    exact = r.sum(-2)[live] / count[live][:, None]
    assert (np.abs(out.reshape(q.shape[:3] + (3,))[live].astype(np.float64) - exact) <= gamma * np.abs(r).sum(-2)[live] / count[live][:, None]).all()
    assert known.reshape(live.shape).astype(bool).tobytes() == live.tobytes()


def test_the_case_set_holds_what_it_must():
    """every count 0..8; a coarse voxel with fewer stored contributors than usable children; one with none stored of some usable; NaN, -0 and a
    subnormal among the valid distances; poison behind every invalid one"""
    counts, fewer, none_of_some, specials = set(), 0, 0, np.zeros(3, int)
    for shape in PC.SHAPES:
        cs = PC.coarsen_case(shape, 5, 11)
        ref = PC.coarsen_ref(cs["dist"], cs["valid"])
        q, inside = PC.child_index(shape)
        bits = ((ref["children"][..., None] >> np.arange(8)) & 1).astype(bool)
        count = bits.sum(-1)
        counts |= set(count.reshape(-1).tolist())
        n_r = (bits & inside & (cs["slot"].reshape(-1)[q] >= 0)).sum(-1)
        fewer += int(((n_r < count) & (n_r > 0)).sum())
        none_of_some += int(((n_r == 0) & (count > 0)).sum())
        live = cs["dist"][cs["valid"] != 0]
        specials += [np.isnan(live).sum(), (np.signbit(live) & (live == 0)).sum(), ((live != 0) & (np.abs(live) < 1e-38)).sum()]
        assert (cs["dist"].view(np.uint8).reshape(-1, 4)[cs["valid"].reshape(-1) == 0] == PC.POISON).all()
        known = PC.rows_ref(ref["children"], shape, cs["banded"], slot=cs["slot"])[1]
        assert known.tobytes() == (n_r > 0).astype(np.uint8).tobytes()
    assert counts == set(range(9)) and fewer >= 10 and none_of_some >= 5 and (specials >= 5).all(), (counts, fewer, none_of_some, specials)


@pytest.mark.parametrize("spec", FC.SMALL, ids=str)
def test_seeded_restatement_with_a_zero_seed_is_the_flow_restatement(spec):
    case = FC.random_case(*spec)
    shape = spec[0]
    poisoned = np.where(case[0][..., None], 0, np.int32(-1515870811)).astype(np.int32)      # 0xA5A5A5A5 behind the non-members of A
    for r in range(1, FC.MAX_RADIUS + 1):
        want = FC.flow_ref(*case, r, np.inf)
        for seed in (None, np.zeros(shape + (3,), np.int32), poisoned):
            got = PC.flow_seeded_ref(*case, seed, r, np.inf)
            for k in ("target", "cost", "axis_cost"):
                same(got[k], want[k], (spec, r, k))
        sd = PC.random_seed(shape, 3, -2, 2)
        got, loop = PC.flow_seeded_ref(*case, sd, r, 30.0, axis=False), PC.flow_seeded_loop(*case, sd, r, 30.0)
        for k in ("target", "cost"):
            same(got[k], loop[k], (spec, r, k, "loop"))


def test_seeded_restatement_finds_a_planted_shift_and_refuses_a_seed_out_of_range():
    shift = (5, -6, 7)
    ma, ra, mb, rb, moved = FC.shifted_copy((8, 9, 10), 6, 21, 0.85, shift)
    seed = np.broadcast_to(np.array(shift, np.int32), ma.shape + (3,)).copy()
    got = PC.flow_seeded_ref(ma, ra, mb, rb, seed, 1, np.inf)
    assert moved.sum() > 5 and (FC.voxel_offsets(got["target"])[moved] == np.array(shift)).all() and (got["cost"][moved] == 0).all()
    at = tuple(np.argwhere(moved)[0])
    seed[at] = (0, PC.SEED_MAX + 1, 0)
    again = PC.flow_seeded_ref(ma, ra, mb, rb, seed, 1, np.inf)
    assert again["target"][at] == -1 and again["cost"][at] == np.inf
    keep = np.ones(ma.shape, bool)
    keep[at] = False
    assert (again["target"][keep] == got["target"][keep]).all()


def test_flow_seed_on_hand_made_numbers():
    import torch
    from d3fields_amd import Flow
    shape = (2, 2, 3)
    target = torch.full(shape, -1, dtype=torch.int32)
    cost = torch.full(shape, float("inf"))
    axis = torch.full(shape + (6,), float("inf"))
    target[0, 0, 0], cost[0, 0, 0] = (1 * 2 + 1) * 3 + 2, 1.0                 # offset (1, 1, 2)
    axis[0, 0, 0] = torch.tensor([2.0, 2.0, 3.0, 1.5, 1.2, 3.0])            # sub-voxel: 0, +0.3, -0.45 -> 2 * (1, 1.3, 1.55) = (2, 2.6, 3.1) -> (2, 3, 3)
    target[1, 1, 2], cost[1, 1, 2] = (1 * 2 + 0) * 3 + 0, 0.5                 # offset (0, -1, -2), no finite neighbour: sub-voxel 0
    flow = Flow((0.0, 0.0, 0.0), 0.1, target, cost, axis)
    assert flow.coarse is None
    for fine in ((4, 4, 6), (3, 4, 5), (4, 3, 6)):
        s = flow.seed(fine)
        assert s.dtype == torch.int32 and tuple(s.shape) == fine + (3,) and s.is_contiguous()
        assert s[0, 0, 0].tolist() == s[1, 1, 1].tolist() == s[1, 0, 1].tolist() == [2, 3, 3]
        assert s[2, 2, 4].tolist() == [0, -2, -4] and s[fine[0] - 1, fine[1] - 1, fine[2] - 1].tolist() == [0, -2, -4]
        assert s[0, 2, 0].tolist() == [0, 0, 0] and s[2, 0, 2].tolist() == [0, 0, 0]          # unmatched: zero
        plain = flow.seed(fine, refined=False)
        assert plain[1, 1, 0].tolist() == [2, 2, 4] and plain[2, 2, 5 if fine[2] > 5 else 4].tolist() == [0, -2, -4]
        want = PC.seed_ref(target.numpy(), cost.numpy(), axis.numpy(), fine)
        assert s.numpy().tobytes() == want.tobytes()
        assert plain.numpy().tobytes() == PC.seed_ref(target.numpy(), cost.numpy(), None, fine).tobytes()
    assert Flow((0.0, 0.0, 0.0), 0.1, target, cost).seed((4, 4, 6)).numpy().tobytes() == flow.seed((4, 4, 6), refined=False).numpy().tobytes()
    for bad in ((4, 4, 7), (2, 2, 3), (5, 4, 6), (4, 4), (0, 4, 6)):
        with pytest.raises(ValueError):
            flow.seed(bad)
    with pytest.raises(TypeError):
        flow.seed(None)


def test_the_chain_reaches_a_shift_the_window_cannot():
    """a sphere of 925 voxels moved by (7, -6, 5) voxels over a static table on 24^3 with 8 channels: direct flow at r = 4 puts NONE of the
    sphere on the planted shift; two box-mean levels, r = 2 at the top and seeded r = 1 below, put 405 of the 925 exactly on it (measured
    here on the CPU; recorded in DESIGN.md 31) and every table voxel at zero"""
    sc = PC.scene()
    ma, mb = PC.level_members(sc["dist_a"], sc["valid_a"]), PC.level_members(sc["dist_b"], sc["valid_b"])
    assert int(sc["sphere_a"].sum()) == 925 and max(abs(s) for s in PC.SCENE_SHIFT) > FC.MAX_RADIUS and any(s % 2 for s in PC.SCENE_SHIFT)
    direct = FC.flow_ref(ma, sc["rows_a"], mb, sc["rows_b"], FC.MAX_RADIUS, np.inf, axis=False)
    assert PC.on_shift(direct["target"], sc["sphere_a"], PC.SCENE_SHIFT) == 0
    pa, pb, flows = PC.scene_chain()
    assert [f["target"].shape for f in flows] == [(6, 6, 6), (12, 12, 12), (24, 24, 24)]
    fine = flows[-1]
    assert PC.on_shift(fine["target"], sc["sphere_a"], PC.SCENE_SHIFT) == 405
    assert PC.on_shift(fine["target"], sc["table"], (0, 0, 0)) == int(sc["table"].sum()) == 1728


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh")] + list(SOURCES), capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    want = ["coarsen_select_kernel"] + ["coarsen_rows_kernelILb%dELb%dEE" % (w, h) for w in (0, 1) for h in (0, 1)] + ["flow_seeded_kernelILb%dEE" % v for v in (0, 1)]
    for kernel in want:
        assert kernel in names, (kernel, out[-800:])
    assert len(rows) == len(want)
    for name, scratch, occ in rows:
        assert scratch == 0 and occ >= 4, (name, scratch, occ)


@pytest.mark.parametrize("source", SOURCES)
def test_source_names_no_fused_operation_no_atomic_and_no_lds(source):
    src = open(os.path.join(ROOT, "d3fields_amd", "csrc", source)).read().lower()
    assert "fma" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.findall(r"\batomic\w*", code) and "__shared__" not in code and "__syncthreads" not in code
    assert "-ffp-contract=off" in build.HIPCC_FLAGS


# ---- Python: argument errors need no device -------------------------------------------------------------------------------------------
def host_field(shape=(4, 5, 6), origin=(0.0, 0.0, 0.0), C=8, dtype=None):
    import torch
    from d3fields_amd import BakedField
    f = object.__new__(BakedField)
    f.origin, f.step, f.grid_shape, f.device = origin, 0.1, torch.Size(shape), torch.device("cpu")
    f.dist, f.valid = torch.zeros(shape), torch.ones(shape, dtype=torch.bool)
    f._sets, f._fills, f.band, f.slot = {"a": torch.zeros(shape + (C,), dtype=dtype or torch.float32)}, {"a": None}, None, None
    return f


def test_argument_errors_need_no_device():
    import torch
    f, g = host_field(), host_field()
    for bad in (lambda: f.coarsen(min_children=0), lambda: f.coarsen(min_children=9), lambda: f.coarsen(band=0.0), lambda: f.coarsen(band=float("inf")),
                lambda: f.coarsen(return_names=["a"] * (_lib.MAX_MAPS + 1)), lambda: host_field(shape=(2, 5, 6)).coarsen(),
                lambda: f.pyramid(-1), lambda: f.pyramid(2), lambda: host_field(shape=(9, 9, 9)).pyramid(4),
                lambda: f.flow(g, "a", seed=torch.zeros((4, 5, 6, 3))), lambda: f.flow(g, "a", seed=torch.zeros((4, 5, 6), dtype=torch.int32)),
                lambda: f.flow(g, "a", seed=torch.zeros((4, 5, 7, 3), dtype=torch.int32)),
                lambda: f.flow_pyramid("field", "a"), lambda: f.flow_pyramid(g, "b"), lambda: f.flow_pyramid(host_field(shape=(4, 5, 7)), "a"),
                lambda: f.flow_pyramid(g, "a", radius_voxels=0), lambda: f.flow_pyramid(g, "a", radius_voxels=5), lambda: f.flow_pyramid(g, "a", fine_radius_voxels=0),
                lambda: f.flow_pyramid(g, "a", fine_radius_voxels=True), lambda: f.flow_pyramid(g, "a", levels=2), lambda: f.flow_pyramid(g, "a", levels=-1)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: f.coarsen(min_children=1.0), lambda: f.coarsen(min_children=True), lambda: f.coarsen(band="thin"), lambda: f.pyramid(1.5), lambda: f.pyramid(True),
                lambda: f.flow(g, "a", seed=[0, 0, 0]), lambda: f.flow(g, "a", seed=np.zeros((4, 5, 6, 3), np.int32)), lambda: f.flow_pyramid(g, "a", levels="2"),
                lambda: f.flow_pyramid(g, "a", levels=1, sites=f.valid), lambda: f.flow_pyramid(g, "a", levels=1, seed=None),
                lambda: f.flow_pyramid(host_field(dtype=torch.float16), "a", levels=1)):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(KeyError):
        f.coarsen(return_names=["b"])
    with pytest.raises(ValueError, match=r"0\.\.1\b"):
        f.pyramid(3)                                 # the message names the largest possible levels
    with pytest.raises(ValueError, match=r"0\.\.3\b"):
        host_field(shape=(9, 17, 33)).pyramid(4)
    f._sets["in_band"] = torch.zeros((4, 5, 6, 1))
    with pytest.raises(ValueError):
        f.coarsen(band=0.01)
    del f._sets["in_band"]
    assert f.pyramid(0) == [f]
    for ok in (lambda: f.coarsen(), lambda: f.coarsen(min_children=8, band=0.01, return_names=["a"]), lambda: f.pyramid(1), lambda: host_field(dtype=torch.float16).coarsen(),
               lambda: f.flow_pyramid(g, "a", levels=1, max_cost=1.0, iso=0.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ok()                                     # every argument is fine: there is no CPU path
