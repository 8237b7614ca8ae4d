"""CPU: the float64 reference of the baked-volume lookup (tests/volume_cases.py) agrees with torch's grid_sample and with
central differences of itself, the case generator keeps its margin for every seed, the ABI 11 entry points exist with the
documented struct layouts and validate their arguments on the host, and BakedField.from_arrays rejects mismatched shapes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import volume_cases as VC
from conftest import ROOT
from d3fields_amd import BakedField, _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")


# ---- the reference itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_name", list(VC.SHAPES))
def test_reference_against_grid_sample(shape_name):
    """trilinear64 == F.grid_sample(mode='bilinear', align_corners=True, padding_mode='zeros') in float64 on an all-valid volume
    at inside points, to 1e-12 relative (of A)."""
    vol, pts, ref = VC.case(shape_name, (5,), 400, 0)
    assert ref["valid"].all()
    n = np.asarray(vol["shape"], np.float64)
    g = (pts.astype(np.float64) - vol["origin"].astype(np.float64)) / float(vol["step"])
    norm = 2.0 * g / (n - 1) - 1.0                                    # align_corners: lattice index 0 -> -1, n - 1 -> +1
    grid = torch.from_numpy(norm[:, [2, 1, 0]].copy()).view(1, -1, 1, 1, 3)      # grid_sample's (x, y, z) = (W, H, D) = (z, y, x) here
    for k, arr in (("dist", vol["dist"][..., None]), ("s0", vol["sets"]["s0"])):
        inp = torch.from_numpy(arr.astype(np.float64)).permute(3, 0, 1, 2)[None]      # [1, C, D = nx, H = ny, W = nz]
        got = F.grid_sample(inp, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, :, 0, 0].T.numpy()
        val, A, _ = ref[k]
        val, A = (val[:, None], A[:, None]) if k == "dist" else (val, A)
        assert np.all(np.abs(got - val) <= 1e-12 * np.maximum(A, 1e-300)), k


def test_reference_gradient_against_central_differences():
    vol, pts, _ = VC.case("5x4x6", (5,), 400, 1)
    rng = np.random.default_rng(7)
    gd, gs = rng.standard_normal(pts.shape[0]), rng.standard_normal((pts.shape[0], 5))
    grad, B, _ = VC.trilinear_grad64(vol, pts, gd, {"s0": gs})
    # float64 points a float32 volume dict accepts: the reference casts pts to float64 itself
    eps = 2.0 ** -20                                                  # in world units: 2^-15 of a cell, far inside the 1e-2 margin
    num = np.zeros_like(grad)
    for a in range(3):
        d = np.zeros(3)
        d[a] = eps
        hi, lo = VC.trilinear64(vol, pts.astype(np.float64) + d), VC.trilinear64(vol, pts.astype(np.float64) - d)
        num[:, a] = ((hi["dist"][0] - lo["dist"][0]) * gd + ((hi["s0"][0] - lo["s0"][0]) * gs).sum(1)) / (2 * eps)
    # trilinear: the central difference along one axis is exact up to rounding, ~ 2^-53 * values / eps
    assert np.all(np.abs(num - grad) <= 1e-8 * np.maximum(B, 1e-300))
    assert np.abs(grad).min() > 0


def test_reference_rejects_whole_cells_and_takes_the_far_face():
    vol = VC.make_volume((3, 3, 3), (2,), 0)
    vol["valid"][1, 1, 1] = False                                     # the centre voxel: a corner of all eight cells
    lat = VC.lattice_points((3, 3, 3))
    ref = VC.trilinear64(vol, lat)
    assert not ref["valid"].any() and np.all(ref["dist"][0] == VC.SENTINEL)      # also at t = 0, weight 0 on the bad corner
    vol["valid"][1, 1, 1] = True
    ref = VC.trilinear64(vol, lat)
    assert ref["valid"].all()
    assert np.array_equal(ref["dist"][0], vol["dist"].reshape(-1).astype(np.float64))          # far faces: last cell, t = 1
    assert np.array_equal(ref["s0"][0], vol["sets"]["s0"].reshape(-1, 2).astype(np.float64))
    p32 = VC.trilinear32(vol, lat)
    assert np.array_equal(p32["dist"], vol["dist"].reshape(-1)) and np.array_equal(p32["s0"], vol["sets"]["s0"].reshape(-1, 2))


def test_generator_margin_holds_for_every_seed():
    """inside_points asserts in float64 that no float32 point's g is within 1e-4 of an integer; nothing is filtered."""
    for shape_name, shape in VC.SHAPES.items():
        for seed in VC.SEEDS:
            for n in (1, 63, 1003):
                pts = VC.inside_points(shape, n, seed)
                assert pts.shape == (n, 3) and pts.dtype == np.float32
    sp = VC.special_points((5, 4, 6))
    ok, _, _ = VC.locate64(VC.make_volume((5, 4, 6), (), 0), sp)
    ok32, _, _ = VC.locate32(VC.make_volume((5, 4, 6), (), 0), sp)
    assert np.array_equal(ok, ok32) and 0 < ok.sum() < ok.size


def test_port_ratio_is_a_few_ulp():
    vol, pts, ref = VC.case("5x4x6", (20,), 1003, 2)
    port = VC.trilinear32(vol, pts)
    assert np.array_equal(port["valid"], ref["valid"])
    worst = max(VC.worst_ratio(port[k], ref[k][0], ref[k][1], VC.coord_term(vol, ref[k][2])) for k in ("dist", "s0"))
    assert 0 < worst <= 8 * VC.U, worst


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
def test_volume_symbols_version_and_layouts():
    lib = _lib.load()
    hdr = open(HEADER).read()
    for name in ("d3f_volume_cell_valid", "d3f_volume_sample", "d3f_volume_sample_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr)
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 11
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define D3F_VOLUME_MAX_CHANNELS (\d+)", hdr).group(1)) == _lib.VOLUME_MAX_CHANNELS == 4096
    # d3f_volume: 3 x int32, 3 + 1 floats, a reserved word, three pointers; d3f_volume_set: ptr, 2 x int32, int64, ptr
    V, S = _lib.Volume, _lib.VolumeSet
    assert ctypes.sizeof(V) == 56 and (V.nx.offset, V.origin.offset, V.step.offset, V.dist.offset, V.valid.offset, V.cell_valid.offset) == (0, 12, 24, 32, 40, 48)
    assert ctypes.sizeof(S) == 32 and (S.data.offset, S.C.offset, S.stride_voxel.offset, S.fill.offset) == (0, 8, 16, 24)
    assert re.search(r"typedef struct d3f_volume \{\s*int32_t nx, ny, nz;\s*float origin\[3\];\s*float step;\s*int32_t reserved;[^}]*const float \*dist;\s*"
                     r"const uint8_t \*valid;\s*const uint8_t \*cell_valid;\s*\} d3f_volume;", hdr)
    assert re.search(r"typedef struct d3f_volume_set \{\s*const float \*data;\s*int32_t C;\s*int32_t reserved;[^}]*int64_t stride_voxel;\s*"
                     r"const float \*fill;[^}]*\} d3f_volume_set;", hdr)


def test_volume_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)

    def vol(shape=(4, 4, 4), step=0.5, dist=p, valid=p, cell=p):
        return _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), step, 0, dist, valid, cell)

    def sets(*Cs, stride=None, data=256):
        arr = (_lib.VolumeSet * max(len(Cs), 1))()
        for s, C in enumerate(Cs):
            arr[s] = _lib.VolumeSet(data, C, 0, C if stride is None else stride, None)
        return arr

    outs = (ctypes.c_void_p * _lib.MAX_MAPS)(*([256] * _lib.MAX_MAPS))

    def fwd(v=None, pts=p, n=5, s=None, ns=0, od=p, ov=p, o=outs, null_vol=False):
        return lib.d3f_volume_sample(None if null_vol else ctypes.byref(v or vol()), pts, n, s, ns, od, ov, o, None)

    def bwd(v=None, pts=p, n=5, s=None, ns=0, gd=None, gs=None, gp=p, null_vol=False):
        return lib.d3f_volume_sample_backward(None if null_vol else ctypes.byref(v or vol()), pts, n, s, ns, gd, gs, gp, None)

    for fn in (fwd, bwd):
        assert fn(null_vol=True) == _lib.ERR_INVALID_ARG and b"vol" in lib.d3f_last_error()
        assert fn(v=vol(shape=(1, 4, 4))) == _lib.ERR_BAD_SHAPE and b"nx=1" in lib.d3f_last_error()
        assert fn(v=vol(shape=(4, 0, 4))) == _lib.ERR_BAD_SHAPE
        assert fn(v=vol(shape=(4, 4, -2))) == _lib.ERR_BAD_SHAPE
        assert fn(v=vol(shape=(2048, 1024, 1024))) == _lib.ERR_BAD_SHAPE and b"voxels" in lib.d3f_last_error()      # 2^31 > 2^31 - 1
        assert fn(v=vol(shape=((1 << 24) + 1, 2, 2))) == _lib.ERR_BAD_SHAPE
        assert fn(v=vol(step=0.0)) == _lib.ERR_INVALID_ARG and b"step" in lib.d3f_last_error()
        assert fn(v=vol(step=-1.0)) == _lib.ERR_INVALID_ARG
        assert fn(v=vol(step=float("nan"))) == _lib.ERR_INVALID_ARG
        assert fn(v=vol(step=float("inf"))) == _lib.ERR_INVALID_ARG
        assert fn(n=-1) == _lib.ERR_INVALID_ARG and b"n=-1" in lib.d3f_last_error()
        assert fn(s=sets(*([4] * 8)), ns=_lib.MAX_MAPS + 1) == _lib.ERR_BAD_SHAPE and b"n_sets" in lib.d3f_last_error()
        assert fn(ns=-1) == _lib.ERR_BAD_SHAPE
        assert fn(s=None, ns=1) == _lib.ERR_INVALID_ARG
        assert fn(s=sets(0), ns=1) == _lib.ERR_BAD_SHAPE and b"C=0" in lib.d3f_last_error()
        assert fn(s=sets(4, 4097), ns=2) == _lib.ERR_BAD_SHAPE and b"set 1" in lib.d3f_last_error()
        assert fn(s=sets(4096), ns=1, n=0) == 0
        # n == 0: a no-op success with NULL buffers
        assert fn(v=vol(dist=None, valid=None, cell=None), pts=None, n=0) == 0
        assert fn(v=vol(dist=None)) == _lib.ERR_INVALID_ARG
        assert fn(v=vol(cell=None)) == _lib.ERR_INVALID_ARG
        assert fn(pts=None) == _lib.ERR_INVALID_ARG
        assert fn(pts=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT
        assert fn(s=sets(4, data=None), ns=1) == _lib.ERR_INVALID_ARG
        assert fn(s=sets(4, stride=3), ns=1) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in lib.d3f_last_error()
    assert fwd(od=None) == _lib.ERR_INVALID_ARG
    assert fwd(ov=None) == _lib.ERR_INVALID_ARG
    assert fwd(s=sets(4), ns=1, o=None) == _lib.ERR_INVALID_ARG
    assert bwd(gp=None) == _lib.ERR_INVALID_ARG and b"grad_pts" in lib.d3f_last_error()
    assert fwd(n=0, od=None, ov=None, o=None) == 0 and bwd(n=0, gp=None) == 0
    # the cell bytes
    assert lib.d3f_volume_cell_valid(None, p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3f_volume_cell_valid(ctypes.byref(vol(shape=(4, 1, 4))), p, None) == _lib.ERR_BAD_SHAPE
    assert lib.d3f_volume_cell_valid(ctypes.byref(vol(valid=None)), p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3f_volume_cell_valid(ctypes.byref(vol()), None, None) == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(fwd(null_vol=True))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- Python surface -------------------------------------------------------------------------------------------------------
def test_from_arrays_rejects_mismatched_shapes():
    d = torch.zeros(4, 3, 5)
    with pytest.raises(ValueError, match="valid"):
        BakedField.from_arrays((0, 0, 0), 0.5, d, valid=torch.ones(4, 3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="feat"):
        BakedField.from_arrays((0, 0, 0), 0.5, d, feat=torch.zeros(4, 3, 6, 8))
    with pytest.raises(ValueError, match="feat"):
        BakedField.from_arrays((0, 0, 0), 0.5, d, feat=torch.zeros(4, 3, 5))
    with pytest.raises(ValueError, match="fill"):
        BakedField.from_arrays((0, 0, 0), 0.5, d, feat=torch.zeros(4, 3, 5, 8), fills={"feat": torch.zeros(7)})
    with pytest.raises(ValueError, match="extent"):
        BakedField.from_arrays((0, 0, 0), 0.5, torch.zeros(4, 1, 5))
    with pytest.raises(ValueError, match="extent"):
        BakedField.from_arrays((0, 0, 0), 0.5, torch.zeros(4 * 3 * 5))
    with pytest.raises(ValueError, match="step"):
        BakedField.from_arrays((0, 0, 0), 0.0, d)
    with pytest.raises(ValueError, match="origin"):
        BakedField.from_arrays((0, 0), 0.5, d)
    with pytest.raises(ValueError, match="output key"):
        BakedField.from_arrays((0, 0, 0), 0.5, d, valid_mask=torch.zeros(4, 3, 5, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):            # well-formed, but not on the device
        BakedField.from_arrays((0, 0, 0), 0.5, d, feat=torch.zeros(4, 3, 5, 8))
    from d3fields_amd import Fusion
    assert callable(Fusion.bake)
