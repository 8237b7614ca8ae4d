"""CPU: the warp entry points (d3f_volume_warp_select, d3f_volume_warp_rows) are declared by the header, bound and exported with D3F_ABI_VERSION
still 16, their host structs have the header's layout, and they validate their arguments on the host with the documented status codes; the NumPy
restatement (tests/warp_cases.py) equals a plain loop formulation byte for byte on every tiny case and has the properties a warp must have
(identity, integer shifts, ties, the planted figures); the ValueErrors of BakedField.warp and .owners need no device; no kernel of
warp_kernels.hip uses scratch and the file names no fused operation and no float atomic."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import warp_cases as WC
from conftest import ROOT
from d3fields_amd import _lib, build

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SOURCE = os.path.join(ROOT, "d3fields_amd", "csrc", "warp_kernels.hip")
SYMBOLS = ("d3f_volume_warp_select", "d3f_volume_warp_rows")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_version_and_sources():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(const d3f_\w+ \*args, void \*stream\);" % name, hdr), name
    assert int(re.search(r"#define D3F_WARP_MAX_PARTS (\d+)", hdr).group(1)) == _lib.WARP_MAX_PARTS == WC.MAX_PARTS == 4096
    assert _lib.MOTION_POSE_DOUBLES == WC.POSE
    assert not [fn for fn in _lib.SIGNATURES if "warp" in fn and fn.endswith("_workspace_bytes")], "the warp needs no workspace"
    assert "warp_kernels.hip" in build.SOURCES and os.path.exists(SOURCE)
    import d3fields_amd
    assert hasattr(d3fields_amd.BakedField, "warp") and hasattr(d3fields_amd.BakedField, "owners")


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}


def header_struct(hdr, name, known):
    """a ctypes Structure built from the header's own text of `typedef struct name { ... } name;` (pointers, scalars, arrays, known structs)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        if "*" in decl:
            fields += [(re.findall(r"\w+", n)[-1], ctypes.c_void_p) for n in decl[decl.index("*"):].split(",")]      # (`void *const *out_sets`: the last word)
            continue
        ctype, rest = decl.replace("const ", "").split(None, 1)
        base = known[ctype] if ctype in known else C_TYPES[ctype]
        for n in rest.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def test_struct_layouts_match_the_header():
    hdr = open(HEADER).read()
    known = {}
    for cname, bound in (("d3f_volume", _lib.Volume), ("d3f_volume_set", _lib.VolumeSet), ("d3f_band", _lib.Band), ("d3f_warp_select", _lib.WarpSelect),
                         ("d3f_warp_rows", _lib.WarpRows)):
        want = header_struct(hdr, cname, known)
        known[cname] = want
        assert ctypes.sizeof(bound) == ctypes.sizeof(want), cname
        assert [f[0] for f in bound._fields_] == [f[0] for f in want._fields_], cname
        for f in want._fields_:
            assert getattr(bound, f[0]).offset == getattr(want, f[0]).offset and getattr(bound, f[0]).size == getattr(want, f[0]).size, (cname, f[0])
    assert ctypes.sizeof(_lib.WarpSelect) == 112 and _lib.WarpSelect.owner.offset == 56 and _lib.WarpSelect.out_boxes.offset == 104
    assert ctypes.sizeof(_lib.WarpRows) == 128 and _lib.WarpRows.m.offset == 104


def test_validation_status_codes():
    lib = _lib.load()
    p, odd4, odd8 = 256, 258, 260
    v = ctypes.c_void_p

    def select(shape=(4, 5, 6), dist=p, valid=p, cell=p, owner=p, pose=p, K=3, source=p, out_dist=p, out_valid=p, boxes=p, null=False):
        vol = _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), 1.0, 0, v(dist), v(valid), v(cell))
        a = _lib.WarpSelect(vol, v(owner), v(pose), K, 0, v(source), v(out_dist), v(out_valid), v(boxes))
        return lib.d3f_volume_warp_select(None if null else ctypes.byref(a), None)

    assert select(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for name in ("dist", "valid", "cell", "owner", "pose", "source", "out_dist", "out_valid", "boxes"):
        assert select(**{name: None}) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), name
    for shape in ((1, 5, 6), (4, 0, 6), (4, 5, -1), (2048, 1024, 1024)):
        assert select(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert b"2^31" in lib.d3f_last_error()
    assert select(K=-1) == _lib.ERR_INVALID_ARG and b"K=" in lib.d3f_last_error()
    assert select(K=_lib.WARP_MAX_PARTS + 1) == _lib.ERR_BAD_SHAPE and b"D3F_WARP_MAX_PARTS" in lib.d3f_last_error()
    for kw in ({"dist": odd4}, {"owner": odd4}, {"pose": odd8}, {"source": odd4}, {"out_dist": odd4}, {"boxes": odd4}):
        assert select(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw

    def rows(shape=(4, 5, 6), band=None, data=p, C=8, stride=8, fill=None, n_sets=1, K=3, source=p, pose=p, voxels=p, m=10, out=p, known=p, null=False, no_sets=False,
             no_outs=False):
        vol = _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), 1.0, 0, None, None, None)
        sets = (_lib.VolumeSet * 1)(_lib.VolumeSet(data, C, 0, stride, fill))
        outs = (ctypes.c_void_p * 1)(out)
        b = None if band is None else ctypes.pointer(_lib.Band(v(band[0]), v(band[1]), band[2]))
        a = _lib.WarpRows(vol, b, None if no_sets else sets, n_sets, K, v(source), v(pose), v(voxels), m, None if no_outs else outs, v(known))
        return lib.d3f_volume_warp_rows(None if null else ctypes.byref(a), None)

    assert rows(null=True) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error()
    for kw in ({"source": None}, {"known": None}, {"pose": None}, {"no_sets": True}, {"no_outs": True}, {"out": None}, {"data": None}, {"band": (None, p, 5)},
               {"band": (p, None, 5)}):
        assert rows(**kw) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), kw
    for shape in ((1, 5, 6), (4, 5, 1), (2048, 1024, 1024)):
        assert rows(shape=shape) == _lib.ERR_BAD_SHAPE, shape
    assert rows(K=-1) == _lib.ERR_INVALID_ARG and rows(K=_lib.WARP_MAX_PARTS + 1) == _lib.ERR_BAD_SHAPE
    assert rows(m=-1) == _lib.ERR_INVALID_ARG and b"m=" in lib.d3f_last_error()
    assert rows(voxels=None, m=10) == _lib.ERR_INVALID_ARG and b"voxel count" in lib.d3f_last_error()
    for bad in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert rows(C=bad, stride=1 << 20) == _lib.ERR_BAD_SHAPE and b"C=" in lib.d3f_last_error(), bad
    assert rows(n_sets=-1) == _lib.ERR_BAD_SHAPE and rows(n_sets=_lib.MAX_MAPS + 1) == _lib.ERR_BAD_SHAPE
    assert rows(band=(p, p, -1)) == _lib.ERR_BAD_SHAPE and rows(band=(p, p, 2 ** 31)) == _lib.ERR_BAD_SHAPE
    assert rows(C=8, stride=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    for kw in ({"source": odd4}, {"pose": odd8}, {"voxels": odd4}, {"data": odd4}, {"fill": odd4}, {"out": odd4}, {"band": (odd4, p, 5)}):
        assert rows(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    assert rows(m=0, source=None, known=None, out=None) == _lib.OK                 # nothing to do: nothing is read
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(rows(m=-1))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    for k in ("source", "dist", "valid", "boxes"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


TINY = [("random 2x2x2", lambda: WC.random_case((2, 2, 2), 2, K=2)), ("random 5x4x6", lambda: WC.random_case((5, 4, 6), 1)),
        ("random 4x6x5 K=6", lambda: WC.random_case((4, 6, 5), 3, K=6)), ("plain 5x5x5 small angles", lambda: WC.random_case((5, 5, 5), 4, K=2, specials=False, motions="small")),
        ("planted", lambda: WC.planted_case((8, 9, 16))), ("collisions", WC.collision_case), ("64 + 1 parts", lambda: WC.many_parts_case(65, (5, 5, 6)))]


@pytest.mark.parametrize("name,make", TINY, ids=[t[0] for t in TINY])
def test_restatement_equals_the_loop_formulation(name, make):
    cs = make()
    same(WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], cs["pose"]), WC.warp_loop(cs["dist"], cs["valid"], cs["owner"], cs["pose"]), name)


def test_generated_arrays_are_read_only():
    cs = WC.random_case((5, 4, 6), 1)
    for k in ("dist", "valid", "owner", "pose"):
        with pytest.raises(ValueError):
            cs[k][...] = 0


def test_identity_and_integer_shifts():
    rng = np.random.default_rng(9)
    shape = (6, 5, 7)
    dist = rng.normal(size=shape).astype(np.float32)
    valid, owner = np.ones(shape, np.uint8), np.ones(shape, np.int32)
    out = WC.warp_ref(dist, valid, owner, WC.pose_row()[None])
    assert np.array_equal(out["dist"], dist) and (out["source"] == 1).all() and out["valid"].all()
    assert out["boxes"].tolist() == [[0, 0, 0, 5, 4, 6] * 2]
    rows, known = WC.rows_ref(out["source"], WC.pose_row()[None], dist[..., None])
    assert np.array_equal(rows[:, 0], dist.reshape(-1)) and known.all()
    for d in ((1, 0, 0), (0, -2, 3), (-1, 1, -1), (6, 0, 0)):
        out = WC.warp_ref(dist, valid, owner, WC.shift_row(d)[None])
        want_src = np.full(shape, -1, np.int32)
        want = np.full(shape, WC.SENTINEL, np.float32)
        dst = tuple(slice(max(d[a], 0), shape[a] + min(d[a], 0)) for a in range(3))
        src = tuple(slice(max(-d[a], 0), shape[a] + min(-d[a], 0)) for a in range(3))
        want[dst], want_src[dst] = dist[src], 1
        assert np.array_equal(out["source"], want_src) and np.array_equal(out["dist"], want) and np.array_equal(out["valid"], want_src >= 0), d
    assert not out["valid"].any() and out["boxes"][0, 6:].tolist() == [WC.INT32_MAX] * 3 + [WC.INT32_MIN] * 3       # shifted off the grid as a whole


def test_ties_go_to_the_background_then_to_the_lower_index():
    cs = WC.collision_case()
    out = WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    assert (out["source"][cs["tie"]] == 0).all() and (out["source"] != 3).all()             # equal distances: the background keeps them
    assert (out["source"] != 5).all() and (out["source"][cs["duplicate"]] == 4).all()        # the duplicate: the lower index everywhere
    both = out["source"][cs["both"]]
    assert set(both.reshape(-1).tolist()) == {1, 2}                                          # two parts on one place: each wins somewhere
    d1, d2 = cs["dist"][0:3, 0:3, 0], cs["dist"][5:8, 0:3, 0]
    assert np.array_equal(both, np.where(d2 < d1, 2, 1)) and np.array_equal(out["dist"][cs["both"]], np.minimum(d1, d2))
    twice = np.concatenate([cs["pose"][:1], cs["pose"][:1]])                                # one part listed twice, its voxels split between the two labels
    owner = np.where(cs["owner"] == 1, 1 + (np.arange(cs["owner"].size).reshape(cs["shape"]) % 2), 0).astype(np.int32)
    split = WC.warp_ref(cs["dist"], cs["valid"], owner, twice)
    whole = WC.warp_ref(cs["dist"], cs["valid"], (owner > 0).astype(np.int32), twice)
    assert np.array_equal(split["dist"], whole["dist"]) and (whole["source"] != 2).all() and (split["source"] == 2).any()


def test_planted_figures_come_out_as_planted():
    cs = WC.planted_case()
    out = WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    assert np.array_equal(np.bincount(out["source"][out["source"] > 0], minlength=cs["K"] + 1)[1:], cs["won"])
    assert np.array_equal(out["boxes"], cs["boxes"]) and int((out["source"] == -1).sum()) == cs["vacated"]
    assert (out["source"][cs["owner"] == 3] == 0).all()                                      # a part without a pose stays, as background
    assert (out["dist"][out["source"] == 1] == -1).all() and (out["dist"][out["source"] == -1] == WC.SENTINEL).all()


def test_rows_of_the_restatement():
    cs = WC.random_case((7, 6, 9), 12, K=4)
    out = WC.warp_ref(cs["dist"], cs["valid"], cs["owner"], cs["pose"])
    _, data = WC.rows_data(cs["shape"], 3, 5)
    fill = np.float32([7, 8, 9])
    rows, known = WC.rows_ref(out["source"], cs["pose"], data, fill=fill)
    src = out["source"].reshape(-1)
    assert np.array_equal(known, (src >= 0).astype(np.uint8)) and (rows[src < 0] == fill).all()
    assert np.array_equal(rows[src == 0], data.reshape(-1, 3)[src == 0])
    one, _ = WC.rows_ref(out["source"], cs["pose"], cs["dist"][..., None])                   # the dist volume as a one-channel set: the select's own chain
    moved = (src > 0)
    assert moved.any() and one[moved, 0].tobytes() == out["dist"].reshape(-1)[moved].tobytes()
    lst = WC.voxel_list(src.size, 3)
    sub, sub_known = WC.rows_ref(out["source"], cs["pose"], data, fill=fill, voxels=lst)
    assert np.array_equal(sub, rows[lst]) and np.array_equal(sub_known, known[lst]) and lst[-1] == lst[0]


def test_owners_restatement():
    labels = np.zeros((6, 7, 5), np.int32)
    labels[1:3, 1:3, 1:3], labels[4, 5, 3] = 1, 2
    owner, unique = WC.owners_ref(labels, 0)
    assert np.array_equal(owner, labels)
    owner, unique = WC.owners_ref(labels, 1.5)
    assert (owner[labels > 0] == labels[labels > 0]).all() and owner[0, 0, 0] == 0 and owner[0, 1, 1] == 1 and owner[4, 4, 4] == 2 and owner[3, 2, 2] == 1 and owner[3, 3, 3] == 0
    assert (owner > 0).sum() == 8 + 24 + 24 + 1 + 18


# ---- BakedField.warp / .owners: argument errors --------------------------------------------------------------------------------------
def host_field(shape=(4, 5, 6)):
    import torch
    from d3fields_amd import BakedField
    f = object.__new__(BakedField)
    f.origin, f.step, f.grid_shape, f.device = (0.0, 0.0, 0.0), 0.1, torch.Size(shape), torch.device("cpu")
    f.dist, f.valid = torch.zeros(shape), torch.ones(shape, dtype=torch.bool)
    f._sets, f._fills, f.band = {"a": torch.zeros(shape + (3,))}, {"a": None}, None
    return f


def test_warp_and_owners_argument_errors_need_no_device():
    import torch
    from d3fields_amd import Components, PartMotions
    f = host_field()
    shape = tuple(f.grid_shape)
    owner = torch.zeros(shape, dtype=torch.int32)
    pose = torch.from_numpy(np.stack([WC.pose_row()] * 3))
    stats = torch.zeros((2, 8), dtype=torch.int32)
    two = Components(f.origin, f.step, owner, 2, 2, stats, owner > 0, 26, 1)
    elsewhere = Components((1.0, 0.0, 0.0), f.step, owner, 3, 3, torch.zeros((3, 8), dtype=torch.int32), owner > 0, 26, 1)
    vol64, volb = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.bool)
    other_grid = PartMotions((0.0, 0.0, 0.0), 0.2, pose, *[torch.zeros(3, dtype=torch.int32)] * 3, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), vol64, volb)
    many = torch.zeros((_lib.WARP_MAX_PARTS + 1, 15), dtype=torch.float64)
    for bad in (lambda: f.warp("pose", owner), lambda: f.warp(pose.float(), owner), lambda: f.warp(pose[:, :12], owner), lambda: f.warp(pose[0], owner),
                lambda: f.warp(many, owner), lambda: f.warp(other_grid, owner), lambda: f.warp(pose, owner.long()), lambda: f.warp(pose, owner[:-1]),
                lambda: f.warp(pose, "owner"), lambda: f.warp(pose, two), lambda: f.warp(pose, elsewhere), lambda: f.warp(pose, owner, which=torch.ones(2, dtype=torch.bool)),
                lambda: f.warp(pose, owner, which=torch.ones(3, dtype=torch.int32)), lambda: f.warp(pose, owner, which=[True] * 3),
                lambda: f.owners(owner.long()), lambda: f.owners(owner[:, :-1]), lambda: f.owners("labels"), lambda: f.owners(elsewhere),
                lambda: f.owners(owner, margin_voxels=-1), lambda: f.owners(owner, margin_voxels=float("nan")), lambda: f.owners(owner, margin_voxels=float("inf")),
                lambda: f.owners(owner, margin_voxels="2"), lambda: f.owners(owner, margin_voxels=True)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(KeyError):
        f.warp(pose, owner, return_names=["b"])
    with pytest.raises(RuntimeError):
        f.warp(pose, owner)                                                 # there is no CPU path
    assert f.owners(owner, margin_voxels=0).data_ptr() == owner.data_ptr() == f.owners(two, margin_voxels=0.5).data_ptr()      # the labels themselves


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "warp_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("warp_box_init_kernel", "warp_owner_box_kernel", "warp_select_kernel", "warp_rows_kernelILb0E", "warp_rows_kernelILb1E"):
        assert kernel in names, (kernel, out[-800:])
    for name, scratch, occ in rows:
        assert scratch == 0 and occ >= 2, (name, scratch, occ)


def test_source_names_no_fused_operation_and_no_float_atomic():
    src = open(SOURCE).read().lower()
    assert "fma" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    atomics = set(re.findall(r"\batomic\w*", code))
    assert atomics == {"atomicmin", "atomicmax"}, atomics                   # integer min / max, on the int32 boxes only
    for call in re.findall(r"atomic(?:min|max)\(([^,]+),", code):
        assert call.strip() == "box", call
    assert "void box_min(int32_t *box, int v)" in open(SOURCE).read() and "void box_max(int32_t *box, int v)" in open(SOURCE).read()
