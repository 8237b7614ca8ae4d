"""CPU: the link entry points (d3f_volume_links, d3f_volume_components_linked) are declared by the header, bound and exported with
D3F_ABI_VERSION still 16 and validate their arguments on the host with the documented status codes; the NumPy restatement
(tests/parts_cases.py) equals a plain Python loop over pairs and stays within the float32 chain's bound of the float64 sums; the labelling
over an edge list equals a flood fill and, on an all-ones link volume, tests/ccl_cases.py and scipy; every case has the planted figures that
make it a case; no kernel of parts_kernels.hip or ccl_kernels.hip uses scratch, and parts_kernels.hip names no fused operation."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ccl_cases as CC
import parts_cases as PC
from conftest import ROOT
from d3fields_amd import _lib, build

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SOURCE = os.path.join(ROOT, "d3fields_amd", "csrc", "parts_kernels.hip")
SYMBOLS = ("d3f_volume_links", "d3f_volume_components_linked")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_version_and_sources():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    assert "still ABI 16: symbols added" in hdr
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    for name, value in (("L2", _lib.LINK_L2), ("COSINE", _lib.LINK_COSINE), ("ARGMAX", _lib.LINK_ARGMAX)):
        assert int(re.search(r"#define D3F_LINK_%s (\d+)" % name, hdr).group(1)) == value == PC.RULES[name.lower()]
    tile = tuple(int(re.search(r"#define D3F_LINK_TILE_%s (\d+)" % a, hdr).group(1)) for a in "XYZ")
    assert tile == _lib.LINK_TILE == PC.TILE and tile[0] * tile[1] * tile[2] == 256
    assert "parts_kernels.hip" in build.SOURCES and os.path.exists(SOURCE)


def test_links_validation_status_codes():
    lib = _lib.load()
    p, odd, odd2 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(257)

    def links(site=p, valid=None, slot=None, shape=(4, 5, 6), data=256, C=8, stride=8, rule=_lib.LINK_L2, thr=1.0, conn=26, out=p, null_set=False):
        st = _lib.VolumeSet(data, C, 0, stride, None)
        return lib.d3f_volume_links(site, valid, slot, shape[0], shape[1], shape[2], None if null_set else ctypes.byref(st), rule, thr, conn, out, None)

    assert links(site=None) == _lib.ERR_INVALID_ARG and b"site" in lib.d3f_last_error()
    assert links(out=None) == _lib.ERR_INVALID_ARG and links(null_set=True) == _lib.ERR_INVALID_ARG
    assert links(data=None) == _lib.ERR_INVALID_ARG and b"data" in lib.d3f_last_error()
    for bad in (-1, 3, 99):
        assert links(rule=bad) == _lib.ERR_INVALID_ARG and b"rule" in lib.d3f_last_error(), bad
    for bad in (0, 4, 8, 27, -6):
        assert links(conn=bad) == _lib.ERR_INVALID_ARG and b"connectivity" in lib.d3f_last_error(), bad
    for rule in PC.RULES.values():
        assert links(rule=rule, thr=float("nan")) == _lib.ERR_INVALID_ARG and b"NaN" in lib.d3f_last_error(), rule
    for bad in (-0.25, 1.0000001, float("inf"), -float("inf")):
        assert links(rule=_lib.LINK_COSINE, thr=bad) == _lib.ERR_INVALID_ARG and b"cosine" in lib.d3f_last_error(), bad
    for shape in ((0, 5, 6), (4, 16385, 6), (4, 5, -1), (2048, 1024, 1024)):
        assert links(shape=shape) == _lib.ERR_BAD_SHAPE and b"extent" in lib.d3f_last_error(), shape
    for bad in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert links(C=bad, stride=1 << 20) == _lib.ERR_BAD_SHAPE and b"C=" in lib.d3f_last_error(), bad
    assert links(stride=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    assert links(data=258) == _lib.ERR_BAD_LAYOUT and links(slot=odd) == _lib.ERR_BAD_LAYOUT and links(out=odd2) == _lib.ERR_BAD_LAYOUT
    assert b"aligned" in lib.d3f_last_error()
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(links(conn=7))
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_components_linked_validation_status_codes():
    lib = _lib.load()
    p, odd, odd1 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(257)
    ws_bytes = lib.d3f_volume_components_workspace_bytes(4, 5, 6)

    def ccl(site=p, links=p, shape=(4, 5, 6), conn=26, min_voxels=1, label=p, count=p, stats=p, capacity=3, ws=p, wsb=ws_bytes):
        return lib.d3f_volume_components_linked(site, links, shape[0], shape[1], shape[2], conn, min_voxels, label, count, stats, capacity, ws, wsb, None)

    assert ccl(site=None) == _lib.ERR_INVALID_ARG and ccl(links=None) == _lib.ERR_INVALID_ARG and b"links" in lib.d3f_last_error()
    assert ccl(label=None) == _lib.ERR_INVALID_ARG and ccl(count=None) == _lib.ERR_INVALID_ARG
    for bad in (0, 4, 27):
        assert ccl(conn=bad) == _lib.ERR_INVALID_ARG and b"connectivity" in lib.d3f_last_error(), bad
    assert ccl(min_voxels=0) == _lib.ERR_INVALID_ARG and ccl(capacity=-1) == _lib.ERR_INVALID_ARG
    assert ccl(stats=None, capacity=1) == _lib.ERR_INVALID_ARG and b"out_stats" in lib.d3f_last_error()
    assert ccl(shape=(0, 5, 6)) == _lib.ERR_BAD_SHAPE and ccl(shape=(2048, 1024, 1024)) == _lib.ERR_BAD_SHAPE
    assert ccl(links=odd1) == _lib.ERR_BAD_LAYOUT and b"links" in lib.d3f_last_error()
    assert ccl(label=odd) == _lib.ERR_BAD_LAYOUT and ccl(count=odd) == _lib.ERR_BAD_LAYOUT and ccl(stats=odd) == _lib.ERR_BAD_LAYOUT
    assert ccl(ws=odd) == _lib.ERR_BAD_LAYOUT and b"workspace" in lib.d3f_last_error()
    assert ccl(ws=None) == _lib.ERR_WORKSPACE and ccl(wsb=ws_bytes - 1) == _lib.ERR_WORKSPACE
    for conn in PC.CONNECTIVITIES:                                   # the legal forms pass every check before the workspace
        assert ccl(conn=conn, ws=None) == _lib.ERR_WORKSPACE and ccl(conn=conn, links=odd, ws=None) == _lib.ERR_WORKSPACE


# ---- the restatement of the links ---------------------------------------------------------------------------------------------------
def test_offsets_and_masks():
    assert len(PC.OFFSETS) == 13 and PC.OFFSETS[12] == (0, 0, -1) and PC.OFFSETS[9:12] == [(0, -1, -1), (0, -1, 0), (0, -1, 1)]
    assert all(o[0] == -1 for o in PC.OFFSETS[:9])
    for j, (dx, dy, dz) in enumerate(PC.OFFSETS):
        assert j == 9 * (dx + 1) + 3 * (dy + 1) + (dz + 1) and (dx * 100 + dy * 10 + dz) < 0
    for conn, want in zip(PC.CONNECTIVITIES, (3, 9, 13)):
        assert PC.CONN_MASK[conn] == sum(1 << j for j in range(13) if PC.allowed(j, conn)) and bin(PC.CONN_MASK[conn]).count("1") == want
        assert sorted(PC.OFFSETS[j] for j in range(13) if PC.allowed(j, conn)) == sorted(o for o in CC.offsets(conn) if o < (0, 0, 0))


@pytest.mark.parametrize("rule", sorted(PC.RULES))
def test_links_ref_equals_the_python_loop(rule):
    rng = np.random.default_rng(5)
    shape, C = (3, 4, 5), 7
    member = rng.random(shape) < 0.8
    rows = PC.blocky_rows(shape, C, 3, exact=False)
    rows[1, 1, 1] = np.nan
    rows[2, 2, 2, 3] = np.inf
    rows[0, 1, 2] = 0.0
    s = np.concatenate([PC.pair_sums(rows, off)["s"].reshape(-1) for off in PC.OFFSETS])
    thr = {"l2": float(np.nanmedian(s[np.isfinite(s)])), "cosine": 0.8, "argmax": 0.0}[rule]
    for conn in PC.CONNECTIVITIES:
        ref = PC.links_ref(member, rows, PC.RULES[rule], thr, conn)
        assert ref.dtype == np.uint16 and np.array_equal(ref, PC.links_loop(member, rows, PC.RULES[rule], thr, conn)), (rule, conn)
        assert not (ref & ~np.uint16(PC.CONN_MASK[conn])).any() and not ref[~member].any()
        assert 0 < int(np.unpackbits(ref.view(np.uint8)).sum()) < 13 * int(member.sum())
    assert not PC.links_ref(member, rows, PC.RULES[rule], thr, 26)[1, 1, 1] or rule == "argmax"      # a NaN row links to nothing


def test_float32_sums_stay_within_the_chain_bound_of_float64():
    u = 2.0 ** -24
    for C in (5, 100, 384):
        rows = PC.blocky_rows((3, 4, 5), C, C, exact=False)
        gamma = (C + 2) * u / (1 - (C + 2) * u)                      # C - 1 additions and up to three roundings inside a term
        for off in PC.OFFSETS:
            f32, f64 = PC.pair_sums(rows, off), PC.pair_sums(rows, off, np.float64)
            hi, lo = PC.pair_slices(rows.shape[:3], off)
            a, b = rows[hi].astype(np.float64), rows[lo].astype(np.float64)
            mag = {"s": f64["s"], "dot": np.abs(a * b).sum(-1), "na": f64["na"], "nb": f64["nb"]}
            for k in f32:
                assert f32[k].dtype == np.float32 and (np.abs(f32[k].astype(np.float64) - f64[k]) <= gamma * mag[k]).all(), (C, off, k)
    exact = PC.blocky_rows((3, 4, 5), 384, 1)                         # small integers: the float32 sums are the float64 sums
    for off in PC.OFFSETS:
        f32, f64 = PC.pair_sums(exact, off), PC.pair_sums(exact, off, np.float64)
        assert all(np.array_equal(f32[k].astype(np.float64), f64[k]) for k in f32)


# ---- the restatement of the labelling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x5x3", "3x5x63", "3x5x17", "5x5x15"])
def test_components_of_edges_equal_a_flood_fill(name):
    site, rows, t2, tc = PC.random_volume(name)
    for conn in PC.CONNECTIVITIES:
        links, ref = PC.random_reference(name, PC.L2, conn)
        edges = PC.edges_of_links(site, links, conn)
        fill = PC.flood_fill_edges(site, edges)
        assert np.array_equal(ref["label"], fill) and ref["K"] == ref["found"] == int(fill.max()), (name, conn)
        for k in range(ref["K"]):
            at = np.argwhere(fill == k + 1)
            assert ref["stats"][k].tolist() == [np.ravel_multi_index(tuple(at[0]), site.shape), len(at), *at.min(0), *at.max(0)], (name, conn, k)
        m = 2
        kept = PC.components_linked_ref(site, links, conn, m)
        assert kept["found"] == ref["found"] and np.array_equal(kept["stats"], ref["stats"][ref["stats"][:, 1] >= m])


@pytest.mark.parametrize("name", ["5x4x6 30%", "9x8x10 30%", "2x3x65 50%", "checkerboard", "wrap yz", "nested"])
def test_all_ones_links_equal_plain_components(name):
    site = CC.site_volume(name)
    junk = np.full(site.shape, 0xFFFF, np.uint16)
    for rank, conn in enumerate(CC.CONNECTIVITIES):
        ref = CC.reference(name, conn)
        got = PC.components_linked_ref(site, junk, conn)
        assert got["found"] == ref["found"] and np.array_equal(got["label"], ref["label"]) and np.array_equal(got["stats"], ref["stats"]), (name, conn)
        try:
            import scipy.ndimage as ndi
        except ImportError:
            continue
        lab, found = ndi.label(site != 0, structure=ndi.generate_binary_structure(3, rank + 1))
        assert found == got["found"] and np.array_equal(CC.renumber_by_root(lab), got["label"])


# ---- case conditions: no case passes vacuously --------------------------------------------------------------------------------------
def bits(links):
    return int(np.unpackbits(np.ascontiguousarray(links).view(np.uint8)).sum())


def test_case_conditions():
    assert {PC.RANDOM[n][0][2] for n in PC.LINES} == {1, 3, 63, 64, 65, 130}
    T = PC.TILE
    for axis in range(3):
        assert {T[axis] - 1, T[axis], T[axis] + 1, 2 * T[axis] + 1} <= {PC.RANDOM[n][0][axis] for n in PC.TILES}
    for name in PC.RANDOM:
        site, rows, t2, tc = PC.random_volume(name)
        members = int((site != 0).sum())
        assert np.abs(rows).max() <= 8 and np.array_equal(rows, np.round(rows)) and site.max() > 1, name
        for rule, conn in ((PC.L2, 26), (PC.L2, 6), (PC.COSINE, 18), (PC.ARGMAX, 26)):
            links, comp = PC.random_reference(name, rule, conn)
            assert 0 < bits(links) and 2 <= comp["found"] <= members // 2, (name, rule, conn, comp["found"], members)
        plain = CC.components_ref(site, 26)["found"]
        assert PC.random_reference(name, PC.L2, 26)[1]["found"] > plain, name          # the links cut what adjacency joins
    # the straddling pairs: one bit, at the higher voxel, or none when the connectivity forbids the offset
    assert {j for j, _ in PC.STRADDLES} == set(range(13))
    for j, hi in PC.STRADDLES:
        site, rows = PC.straddle(j, hi)
        lo = tuple(h + d for h, d in zip(hi, PC.OFFSETS[j]))
        assert int(site.sum()) == 2 and any(h // t != l // t for h, l, t in zip(hi, lo, T)), (j, hi)
        for conn in PC.CONNECTIVITIES:
            links = PC.links_ref(site != 0, rows, PC.L2, 0.0, conn)
            want = 1 if PC.allowed(j, conn) else 0
            assert bits(links) == want and int(links[hi]) == (want << j), (j, hi, conn)
            assert PC.components_linked_ref(site, links, conn)["found"] == 2 - want
    assert {tuple(h // t != (h + d) // t for h, d, t in zip(hi, PC.OFFSETS[j], T)) for j, hi in PC.STRADDLES} >= {
        (True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True), (True, True, True)}
    # the serpentine: the rule gives exactly the hand-built path, one component of every voxel; one cleared bit makes two
    pos, path = PC.serpentine()
    n = int(np.prod(PC.SERPENTINE_SHAPE))
    site = np.ones(PC.SERPENTINE_SHAPE, np.uint8)
    assert np.array_equal(PC.links_ref(site != 0, pos, PC.L2, 1.0, 6), path) and bits(path) == n - 1
    whole = PC.components_linked_ref(site, path, 6)
    assert whole["found"] == 1 and whole["stats"][0].tolist() == [0, n, 0, 0, 0, 7, 7, 69]
    cut = path.copy()
    assert cut[PC.SERPENTINE_CUT] == 1 << 12
    cut[PC.SERPENTINE_CUT] = 0
    halves = PC.components_linked_ref(site, cut, 6)
    assert halves["found"] == 2 and halves["stats"][:, 1].sum() == n and halves["stats"][:, 1].min() > 1000
    # the touching boxes: adjacency sees one object, the descriptors two; the instance-mask rows agree with the boxes
    sc = PC.touching_boxes()
    occupied = sc["dist"] <= 0
    assert CC.components_ref(occupied, 26)["found"] == 1
    t2 = np.float32(PC.TOUCHING_TAU) * np.float32(PC.TOUCHING_TAU)
    two = PC.components_linked_ref(occupied, PC.links_ref(occupied, sc["feat"], PC.L2, t2, 26), 26)
    assert two["found"] == 2 and np.array_equal(two["label"] == 1, sc["inside_a"]) and np.array_equal(two["label"] == 2, sc["inside_b"])
    by_mask = PC.components_linked_ref(occupied, PC.links_ref(occupied, sc["mask"], PC.ARGMAX, 0.0, 26), 26)
    assert np.array_equal(by_mask["label"], two["label"])


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "parts_kernels.hip", "ccl_kernels.hip"], capture_output=True, text=True,
                         timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("links_kernelILi0ELb1", "links_kernelILi0ELb0", "links_kernelILi1ELb1", "links_kernelILi1ELb0", "links_argmax_kernel", "ccl_linked_init_kernel",
                   "ccl_linked_merge_kernel", "ccl_init_kernel", "ccl_flatten_kernel", "ccl_box_kernel"):
        assert kernel in names, (kernel, out[-800:])
    for name, scratch in rows:
        assert scratch == 0, (name, scratch)


def test_source_names_no_fused_operation():
    assert "fma" not in open(SOURCE).read().lower()
