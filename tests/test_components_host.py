"""CPU: ABI 15 (connected components of a site volume, d3f_volume_components) is declared by the header, the binding and the library; the
entry point validates its arguments on the host with the documented status codes and launches nothing; the NumPy restatement
(tests/ccl_cases.py) equals a pure-Python flood fill and, where scipy imports, scipy.ndimage.label; every constructed case has the
component counts that make it a case; no kernel of ccl_kernels.hip uses scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ccl_cases as CC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_volume_components_workspace_bytes", "d3f_volume_components")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_components_symbols_and_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 15
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name


REJECTED_SHAPES = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2048, 1024, 1024), (16384, 16384, 8)]
ACCEPTED_SHAPES = [(1, 1, 1), (4, 4, 4), (16384, 1, 1), (1, 16384, 1), (1, 1, 16384), (16384, 16384, 1), (2047, 1024, 1024)]


def test_components_workspace_bytes_is_zero_exactly_for_rejected_shapes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    for shape in REJECTED_SHAPES:
        assert lib.d3f_volume_components_workspace_bytes(*shape) == 0, shape
        assert lib.d3f_volume_components(p, *shape, 26, 1, p, p, p, 4, p, 1 << 62, None) == _lib.ERR_BAD_SHAPE, shape
        assert b"extent" in lib.d3f_last_error()
    for shape in ACCEPTED_SHAPES:
        n = shape[0] * shape[1] * shape[2]
        got = lib.d3f_volume_components_workspace_bytes(*shape)
        assert got >= 12 * n and got % 4 == 0, shape              # three int32 volumes and the scratch of the prefix sum
        assert lib.d3f_volume_components(p, *shape, 26, 1, p, p, p, 4, p, got - 1, None) == _lib.ERR_WORKSPACE, shape      # one byte short
        assert b"workspace" in lib.d3f_last_error()


def test_components_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    ws_bytes = lib.d3f_volume_components_workspace_bytes(4, 5, 6)

    def ccl(site=p, shape=(4, 5, 6), conn=26, min_voxels=1, label=p, count=p, stats=p, capacity=3, ws=p, wsb=ws_bytes):
        return lib.d3f_volume_components(site, shape[0], shape[1], shape[2], conn, min_voxels, label, count, stats, capacity, ws, wsb, None)

    assert ccl(site=None) == _lib.ERR_INVALID_ARG and b"site" in lib.d3f_last_error()
    assert ccl(label=None) == _lib.ERR_INVALID_ARG and b"out_label" in lib.d3f_last_error()
    assert ccl(count=None) == _lib.ERR_INVALID_ARG and b"out_count" in lib.d3f_last_error()
    for bad in (0, 4, 8, 27, -6):
        assert ccl(conn=bad) == _lib.ERR_INVALID_ARG and b"connectivity" in lib.d3f_last_error(), bad
    for bad in (0, -1):
        assert ccl(min_voxels=bad) == _lib.ERR_INVALID_ARG and b"min_voxels" in lib.d3f_last_error(), bad
    assert ccl(capacity=-1) == _lib.ERR_INVALID_ARG and b"stats_capacity" in lib.d3f_last_error()
    assert ccl(stats=None, capacity=1) == _lib.ERR_INVALID_ARG and b"out_stats" in lib.d3f_last_error()
    assert ccl(shape=(0, 5, 6)) == _lib.ERR_BAD_SHAPE and ccl(shape=(4, 16385, 6)) == _lib.ERR_BAD_SHAPE
    assert ccl(shape=(2048, 1024, 1024)) == _lib.ERR_BAD_SHAPE and b"voxels" in lib.d3f_last_error()
    assert ccl(label=odd) == _lib.ERR_BAD_LAYOUT and ccl(count=odd) == _lib.ERR_BAD_LAYOUT and ccl(stats=odd) == _lib.ERR_BAD_LAYOUT
    assert b"aligned" in lib.d3f_last_error()
    assert ccl(ws=odd) == _lib.ERR_BAD_LAYOUT and b"workspace" in lib.d3f_last_error()
    assert ccl(ws=None) == _lib.ERR_WORKSPACE and ccl(wsb=ws_bytes - 1) == _lib.ERR_WORKSPACE and ccl(wsb=0) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.d3f_last_error()
    # the legal forms pass every check before the workspace (and stop there: nothing is launched without a GPU)
    for conn in CC.CONNECTIVITIES:
        assert ccl(conn=conn, ws=None) == _lib.ERR_WORKSPACE
    assert ccl(stats=None, capacity=0, ws=None) == _lib.ERR_WORKSPACE and ccl(min_voxels=2 ** 31 - 1, ws=None) == _lib.ERR_WORKSPACE
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(ccl(conn=7))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_offsets_are_the_three_neighbourhoods():
    assert [len(CC.offsets(c)) for c in CC.CONNECTIVITIES] == [6, 18, 26]
    for c, reach in zip(CC.CONNECTIVITIES, (1, 2, 3)):
        assert all(max(abs(a) for a in o) == 1 and sum(abs(a) for a in o) <= reach for o in CC.offsets(c))


@pytest.mark.parametrize("name", CC.SMALL)
def test_ref_equals_flood_fill(name):
    site = CC.site_volume(name)
    for conn in CC.CONNECTIVITIES:
        ref = CC.reference(name, conn)
        fill = CC.flood_fill(site, conn)
        assert np.array_equal(ref["label"], fill), (name, conn)
        assert ref["K"] == ref["found"] == int(fill.max())
        for k in range(ref["K"]):                                    # the stats rows, from the flood fill's own labels
            at = np.argwhere(fill == k + 1)
            assert ref["stats"][k].tolist() == [np.ravel_multi_index(tuple(at[0]), site.shape), len(at), *at.min(0), *at.max(0)], (name, conn, k)


@pytest.mark.parametrize("name", CC.CASES)
def test_ref_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    site = CC.site_volume(name) != 0
    for rank, conn in enumerate(CC.CONNECTIVITIES):
        lab, found = ndi.label(site, structure=ndi.generate_binary_structure(3, rank + 1))
        ref = CC.reference(name, conn)
        assert found == ref["found"] and np.array_equal(CC.renumber_by_root(lab), ref["label"]), (name, conn)
        assert np.array_equal(np.bincount(ref["label"].reshape(-1), minlength=found + 1)[1:], ref["stats"][:, 1])


def test_ref_with_min_voxels_keeps_root_order():
    for name, conn, m in CC.MIN_VOXELS:
        full, ref = CC.reference(name, conn), CC.reference(name, conn, m)
        keep = full["stats"][:, 1] >= m
        assert ref["found"] == full["found"] and ref["K"] == int(keep.sum()) and np.array_equal(ref["stats"], full["stats"][keep])
        lut = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)]).astype(np.int32)
        assert np.array_equal(ref["label"], lut[full["label"]])


# ---- case conditions: no case passes vacuously --------------------------------------------------------------------------------------
def test_case_conditions():
    assert len(set(CC.CASES)) == len(CC.CASES)
    for name, counts in CC.EXPECTED.items():
        assert tuple(CC.reference(name, c)["found"] for c in CC.CONNECTIVITIES) == counts, name
    for name in CC.RANDOM:
        site = CC.site_volume(name)
        assert site.shape == CC.RANDOM[name][0] and (site != 0).any() and not (site != 0).all() and site.max() > 1, name
    box = CC.reference("all sites", 6)["stats"][0]
    assert box.tolist() == [0, 60, 0, 0, 0, 2, 3, 4]                # one component whose box is the volume
    board = CC.reference("checkerboard", 6)
    assert board["found"] == int((CC.site_volume("checkerboard") != 0).sum()) == 360 and (board["stats"][:, 1] == 1).all()
    # the serpentine's one component visits every slab; a missing gate leaves exactly two pieces, each of several slabs
    assert CC.reference("serpentine", 6)["stats"][0, 1] == 11 * 20 * 130 + 10
    cut = CC.reference("serpentine cut", 6)["stats"]
    assert cut[:, 1].tolist() == [6 * 2600 + 5, 5 * 2600 + 4]
    assert CC.reference("plates", 6)["stats"][0, 1] == 2 * 2800 + 1 and CC.PLATE_JOINT == (3, 39, 69)
    outer, inner = CC.reference("nested", 26)["stats"]
    assert (outer[2:5] <= inner[2:5]).all() and (inner[5:8] <= outer[5:8]).all() and inner[1] == 8
    combs = CC.site_volume("combs")
    for conn in CC.CONNECTIVITIES:                                   # the two combs are the two components, whatever the connectivity
        lab = CC.reference("combs", conn)["label"]
        assert np.array_equal(lab[combs == 1], np.ones((combs == 1).sum())) and np.array_equal(lab[combs == 2], np.full((combs == 2).sum(), 2))
    # a component of size m-1, m and m+1 around every threshold
    for name, conn, m in CC.MIN_VOXELS:
        sizes = set(CC.reference(name, conn)["sizes_all"].tolist())
        assert {m - 1, m, m + 1} <= sizes, (name, conn, m)
    assert {name for name, _, _ in CC.MIN_VOXELS} == {"9x8x10 30%", "65x3x67 25%"}
    assert CC.reference(*CC.CAPACITY_CASE)["K"] > 4
    # the tiling of the kernels: 64 consecutive flat indices to a wave.  Lines inside one wave, lines across a wave boundary at every
    # phase, wave boundaries on line starts, more than one workgroup of 256
    nz = {CC.site_volume(n).shape[2] for n in CC.CASES}
    assert {1, 5, 33, 63, 64, 65, 130, 300} <= nz
    assert any(CC.site_volume(n).size < 64 for n in CC.CASES) and any(CC.site_volume(n).size > 256 for n in CC.CASES)
    assert max(CC.site_volume(n).size for n in CC.CASES) == 262144
    sizes = sorted(CC.site_volume(n).size for n in CC.CASES)                  # the flatten kernel: one turn per workgroup up to 131072 voxels, two beyond
    assert any(n <= 131072 and n > 256 for n in sizes) and any(131072 < n < 262144 and n % 512 for n in sizes) and 262144 in sizes
    big = CC.reference("64x64x64 31%", 6)
    assert big["stats"][:, 1].max() > 2000 and big["found"] > 10000           # tortuous large components among thousands of small ones


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "ccl_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("ccl_init_kernel", "ccl_merge_kernelILi6E", "ccl_merge_kernelILi18E", "ccl_merge_kernelILi26E", "ccl_flatten_kernel", "ccl_flag_kernel",
                   "ccl_label_kernel", "ccl_box_kernel"):
        assert kernel in names, (kernel, out[-800:])
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0 and vgpr <= 64 and occ == 8, (name, vgpr, scratch, occ)
