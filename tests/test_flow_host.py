"""CPU: the flow entry point (d3f_volume_flow) is declared by the header, bound and exported with D3F_ABI_VERSION still 16 and validates its
arguments on the host with the documented status codes; the NumPy restatement (tests/flow_cases.py) equals a plain Python loop and its
packed-key variant and stays within the float32 chain's bound of the float64 sums; the planted figures (self-flow, a shifted copy, ties)
come out as planted; Flow's consistent rule and refinement are restated; no kernel of flow_kernels.hip uses scratch and the file names no
fused operation."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_cases as FC
from conftest import ROOT
from d3fields_amd import _lib, build

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SOURCE = os.path.join(ROOT, "d3fields_amd", "csrc", "flow_kernels.hip")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbol_version_and_sources():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    assert hasattr(lib, "d3f_volume_flow") and "d3f_volume_flow" in _lib.SIGNATURES and re.search(r"\bint d3f_volume_flow\(", hdr)
    assert int(re.search(r"#define D3F_FLOW_MAX_RADIUS (\d+)", hdr).group(1)) == _lib.FLOW_MAX_RADIUS == FC.MAX_RADIUS == 4
    assert _lib.LINK_TILE == FC.TILE
    assert "flow_kernels.hip" in build.SOURCES and os.path.exists(SOURCE)
    import d3fields_amd
    assert d3fields_amd.Flow is d3fields_amd.baked.Flow and hasattr(d3fields_amd.BakedField, "flow")


def test_validation_status_codes():
    lib = _lib.load()
    p, odd = 256, 258

    def flow(site_a=p, slot_a=None, data_a=p, Ca=8, stride_a=8, site_b=p, slot_b=None, data_b=p, Cb=8, stride_b=8, shape=(4, 5, 6), r=2, mc=float("inf"),
             target=p, cost=p, axis=None, null_a=False, null_b=False):
        sa, sb = _lib.VolumeSet(data_a, Ca, 0, stride_a, None), _lib.VolumeSet(data_b, Cb, 0, stride_b, None)
        v = ctypes.c_void_p
        return lib.d3f_volume_flow(v(site_a), v(slot_a), None if null_a else ctypes.byref(sa), v(site_b), v(slot_b), None if null_b else ctypes.byref(sb),
                                   shape[0], shape[1], shape[2], r, mc, v(target), v(cost), v(axis), None)

    for kw in ({"site_a": None}, {"site_b": None}, {"null_a": True}, {"null_b": True}, {"data_a": None}, {"data_b": None}, {"target": None}, {"cost": None}):
        assert flow(**kw) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), kw
    for bad in (0, -1, 5, 99):
        assert flow(r=bad) == _lib.ERR_INVALID_ARG and b"radius" in lib.d3f_last_error(), bad
    assert flow(mc=float("nan")) == _lib.ERR_INVALID_ARG and b"NaN" in lib.d3f_last_error()
    for shape in ((0, 5, 6), (4, 16385, 6), (4, 5, -1), (2048, 1024, 1024)):
        assert flow(shape=shape) == _lib.ERR_BAD_SHAPE and b"extent" in lib.d3f_last_error(), shape
    for bad in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert flow(Ca=bad, Cb=bad, stride_a=1 << 20, stride_b=1 << 20) == _lib.ERR_BAD_SHAPE and b"C=" in lib.d3f_last_error(), bad
    assert flow(Ca=8, Cb=4) == _lib.ERR_BAD_SHAPE and b"same width" in lib.d3f_last_error()
    assert flow(stride_a=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    assert flow(stride_b=7) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    for kw in ({"data_a": odd}, {"data_b": odd}, {"slot_a": odd}, {"slot_b": odd}, {"target": odd}, {"cost": odd}, {"axis": odd}):
        assert flow(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(flow(r=7))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    for k in b:
        if b[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def test_offsets_and_keys():
    for r in range(1, FC.MAX_RADIUS + 1):
        offs = FC.offsets(r)
        assert len(offs) == (2 * r + 1) ** 3 and [FC.j_of(o, r) for o in offs] == list(range(len(offs)))
        assert max(sum(c * c for c in o) for o in offs) <= 48 and len(offs) <= 729
        for shape, v in (((3, 4, 5), (1, 2, 2)), ((9, 2, 11), (0, 1, 10))):      # among the candidates inside the volume, ascending j is ascending flat index
            us = [tuple(a + b for a, b in zip(v, o)) for o in offs]
            flat = [int(np.ravel_multi_index(u, shape)) for u in us if all(0 <= u[k] < shape[k] for k in range(3))]
            assert len(flat) > 1 and all(a < b for a, b in zip(flat, flat[1:]))
    # the packed key orders exactly as the tuple does, across the binades of s and at s = +0
    rng = np.random.default_rng(0)
    s = np.concatenate([np.float32([0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38]), rng.random(40).astype(np.float32) * 1e3])
    keys = [(float(x), int(d2), int(j)) for x in s[:12] for d2 in (0, 1, 48) for j in (0, 1, 728)]
    packed = [int(FC.pack_key(np.float32(k[0]), k[1], k[2])) for k in keys]
    for (ka, pa), (kb, pb) in itertools.combinations(zip(keys, packed), 2):
        assert (ka < kb) == (pa < pb) and (ka == kb) == (pa == pb), (ka, kb)
    assert max(packed) < 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("case", FC.SMALL)
def test_flow_ref_equals_the_loop_and_the_packed_key(case):
    shape, C, seed, density, kind = case
    ma, ra, mb, rb = FC.random_case(shape, C, seed, density, kind)
    ra, rb = ra.copy(), rb.copy()
    if C > 1:
        ra[0, 1, 1, 0] = np.nan
        rb[0, 2, 2, 1] = np.inf
    s_all = FC.chain(ra.reshape(-1, 1, C), rb.reshape(1, -1, C))
    finite = np.sort(s_all[np.isfinite(s_all)])
    for r in (1, 2, 3, 4):
        for mc in (float("inf"), float(finite[len(finite) // 4]), 0.0):
            ref = FC.flow_ref(ma, ra, mb, rb, r, mc)
            same(ref, FC.flow_loop(ma, ra, mb, rb, r, mc), (case, r, mc, "loop"))
            same(ref, FC.flow_ref_packed(ma, ra, mb, rb, r, mc), (case, r, mc, "packed"))
            assert ((ref["target"] < 0) == np.isinf(ref["cost"])).all() and (ref["target"][~ma] == -1).all()
            assert np.isinf(ref["axis_cost"][ref["target"] < 0]).all()
    full = FC.flow_ref(ma, ra, mb, rb, 4, float("inf"))
    assert (full["target"] >= 0).sum() > 0 and ((full["target"] >= 0) <= ma).all()
    if kind == "int":                                                # ties in s do occur: the d2 and j parts of the key decide somewhere
        tied = 0
        for v in np.argwhere(full["target"] >= 0):
            v = tuple(v)
            ss = [FC.chain(ra[v], rb[tuple(np.add(v, o))]) for o in FC.offsets(4)
                  if all(0 <= v[k] + o[k] < shape[k] for k in range(3)) and mb[tuple(np.add(v, o))]]
            tied += int(sum(1 for x in ss if x == full["cost"][v]) > 1)
        assert tied > 0


def test_float32_cost_stays_within_the_chain_bound_of_float64():
    u = 2.0 ** -24
    for C in (5, 40, 384):
        ma, ra, mb, rb = FC.random_case((3, 4, 5), C, 50 + C, 1.0, "gauss")
        gamma = (C + 2) * u / (1 - (C + 2) * u)                      # C - 1 additions and up to three roundings inside a term
        for off in FC.offsets(1):
            va, ub = FC.pair_slices(ma.shape, off)
            f32, f64 = FC.chain(ra[va], rb[ub]), FC.chain(ra[va], rb[ub], np.float64)
            assert f32.dtype == np.float32 and (np.abs(f32.astype(np.float64) - f64) <= gamma * f64).all(), (C, off)
    ma, ra, mb, rb = FC.random_case((3, 4, 5), 384, 9, 1.0, "int")    # small integers: the float32 sums are the float64 sums
    for off in FC.offsets(1):
        va, ub = FC.pair_slices(ma.shape, off)
        assert np.array_equal(FC.chain(ra[va], rb[ub]).astype(np.float64), FC.chain(ra[va], rb[ub], np.float64))


# ---- planted figures ------------------------------------------------------------------------------------------------------------------
def test_self_flow_is_the_identity():
    ma, ra, mb, rb = FC.random_case((4, 5, 6), 6, 77, 0.8, "gauss")
    for r in (1, 2, 4):
        ref = FC.flow_ref(ma, ra, ma, ra, r, float("inf"))
        flat = np.arange(ma.size).reshape(ma.shape)
        assert np.array_equal(ref["target"][ma], flat[ma]) and (ref["cost"][ma] == 0).all() and (ref["target"][~ma] == -1).all()
        off = FC.refine_offsets(ref["cost"], ref["axis_cost"], ref["target"] >= 0)
        assert np.isnan(off[~ma]).all() and (np.abs(off[ma]) <= 0.5).all()


def test_shifted_copy_gives_the_shift():
    ma, ra, mb, rb, moved = FC.shifted_copy()
    assert 0 < moved.sum() < ma.sum()
    for r in (2, 3):
        ref = FC.flow_ref(ma, ra, mb, rb, r, float("inf"))
        assert (FC.voxel_offsets(ref["target"])[moved] == np.array(FC.SHIFT)).all() and (ref["cost"][moved] == 0).all()
        rest = ma & ~moved
        assert ((ref["cost"][rest] > 0) | (ref["target"][rest] == -1)).all()
        back = FC.flow_ref(mb, rb, ma, ra, r, float("inf"))
        assert np.array_equal(FC.consistent_ref(ref["target"], back["target"], 0), moved)
        assert (FC.consistent_ref(ref["target"], back["target"], 1) >= moved).all()
    assert not (FC.flow_ref(ma, ra, mb, rb, 1, float("inf"))["cost"][ma] == 0).any()      # the shift lies outside a window of radius 1


def test_ties_go_to_the_nearest_then_the_lowest_index():
    ma, ra, mb, rb, hole = FC.identical_b()
    ny, nz = ma.shape[1:]
    for r in (1, 2, 4):
        ref = FC.flow_ref(ma, ra, mb, rb, r, float("inf"))
        flat = np.arange(ma.size).reshape(ma.shape)
        assert np.array_equal(ref["target"][~hole], flat[~hole]) and (ref["cost"] == 0).all()
        # B lacks the voxel itself: d2 = 1, and among the six the lowest j that lies inside: x-, else y-, else z-, else z+ ...
        assert ref["target"][2, 2, 3] == flat[1, 2, 3] and ref["target"][0, 0, 0] == flat[0, 0, 1] and ref["target"][4, 4, 6] == flat[3, 4, 6]
    assert FC.j_of((-1, 0, 0), 2) < FC.j_of((0, -1, 0), 2) < FC.j_of((0, 0, -1), 2) < FC.j_of((0, 0, 1), 2)


def test_planted_best_across_the_window():
    for r in (3, 4):
        shape = (2 * r + 1, 2 * r + 1, 2 * r + 3)
        for off in FC.window_marks(r):
            ma, ra, mb, rb, centre = FC.planted(shape, r, 3, [off])
            ref = FC.flow_ref(ma, ra, mb, rb, r, float("inf"), axis=False)
            assert tuple(FC.voxel_offsets(ref["target"])[centre]) == off and ref["cost"][centre] == 0


# ---- the Python side, restated ------------------------------------------------------------------------------------------------------
def test_refine_formula_and_consistent_rule():
    cost = np.float32([[[1.0, 1.0, 2.0, 1.0]]])
    axis = np.full((1, 1, 4, 6), np.inf, np.float32)
    axis[0, 0, 0] = [2, 4, 3, 3, 1.5, 9]          # x: 0.5 * (2 - 4) / (2 - 2 + 4) = -0.25; y: 0; z: 0.5 * (1.5 - 9) / (1.5 - 2 + 9) = -0.44
    axis[0, 0, 1] = [np.inf, 4, 1, 1, 0.5, 0.5]   # x: a side is +Inf -> 0; y: denominator 0 -> 0; z: denominator < 0 -> 0
    axis[0, 0, 2] = [3, 3, 3, 3, 3, 3]
    matched = np.array([[[True, True, True, False]]])
    off = FC.refine_offsets(cost, axis, matched)
    assert np.allclose(off[0, 0, 0], [-0.25, 0.0, 0.5 * (1.5 - 9) / (1.5 - 2 + 9)]) and (off[0, 0, 1] == 0).all() and (off[0, 0, 2] == 0).all()
    assert np.isnan(off[0, 0, 3]).all()
    axis[0, 0, 2] = [1.0, 10, 2.5, 2.5, 2.5, 2.5]                    # 0.5 * (1 - 10) / (1 - 4 + 10) = -0.64 clamps to -0.5
    assert FC.refine_offsets(cost, axis, matched)[0, 0, 2, 0] == -0.5
    # consistent: matched, the way back has a target, and it lands within tol
    forward = np.int32([[[1, 2, -1, 0]]])
    back = np.int32([[[-1, 0, 0, 3]]])
    assert FC.consistent_ref(forward, back, 0).tolist() == [[[True, False, False, False]]]      # 0 -> 1 -> 0;  1 -> 2 -> 0, one voxel off
    assert FC.consistent_ref(forward, back, 1).tolist() == [[[True, True, False, False]]]
    assert FC.consistent_ref(forward, back, 3).tolist() == [[[True, True, False, False]]]       # 3 -> 0, which has no way back


def test_flow_object_on_host_tensors():
    """Flow holds tensors only and its arithmetic is plain torch: on host tensors made from the restatement's outputs every derived field
    equals the restated formula"""
    import torch
    from d3fields_amd import Flow
    ma, ra, mb, rb, moved = FC.shifted_copy()
    ref, back = FC.flow_ref(ma, ra, mb, rb, 2, float("inf")), FC.flow_ref(mb, rb, ma, ra, 2, float("inf"))
    t = lambda a: torch.from_numpy(np.array(a))
    step = 0.02
    f = Flow((0.5, -0.25, 1.0), step, t(ref["target"]), t(ref["cost"]), t(ref["axis_cost"]))
    b = Flow((0.5, -0.25, 1.0), step, t(back["target"]), t(back["cost"]))
    matched, vo = ref["target"] >= 0, FC.voxel_offsets(ref["target"])
    off = FC.refine_offsets(ref["cost"], ref["axis_cost"], matched)
    assert np.array_equal(f.matched.numpy(), matched) and f.voxel_offset.dtype == torch.int32 and np.array_equal(f.voxel_offset.numpy(), vo)
    assert f.offset.dtype == torch.float64 and np.array_equal(f.offset.numpy(), off, equal_nan=True) and (np.abs(off[matched]) > 0).any()
    assert np.array_equal(f.displacement().numpy(), (vo.astype(np.float64) + off) * step, equal_nan=True)
    assert np.array_equal(f.displacement(refined=False).numpy(), np.where(matched[..., None], vo.astype(np.float64) * step, np.nan), equal_nan=True)
    for tol in (0, 1, 2):
        assert np.array_equal(f.consistent(b, tol_voxels=tol).numpy(), FC.consistent_ref(ref["target"], back["target"], tol)), tol
    assert np.array_equal(f.consistent(b, tol_voxels=0).numpy(), moved)
    assert b.offset is None and b.axis_cost is None
    for bad in (lambda: b.displacement(), lambda: f.consistent(back["target"]), lambda: f.consistent(b, tol_voxels=-1), lambda: f.consistent(b, tol_voxels=1.0)):
        with pytest.raises(ValueError):
            bad()


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "flow_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ["flow_kernelILi%dELb%dE" % (w, vec) for w in (3, 4, 5) for vec in (0, 1)] + ["flow_axis_kernel"]:
        assert kernel in names, (kernel, out[-800:])
    for name, scratch, occ in rows:
        assert scratch == 0 and occ >= 2, (name, scratch, occ)


def test_source_names_no_fused_operation():
    assert "fma" not in open(SOURCE).read().lower()
