"""CPU: ABI 13 (the surface band of a baked volume) is declared by the header, the binding and the library with the documented
struct layout; the NumPy restatement of mark / slot (tests/band_cases.py) holds its invariants on every case volume; every
committed case keeps its generator conditions; the entry points validate their arguments on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

import band_cases as BC
import raycast_cases as RC
import volume_cases as VC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_band_workspace_bytes", "d3f_band_mark", "d3f_band_sample", "d3f_band_sample_backward")
ALL_BANDS = [(name, steps) for name in BC.CASES for steps in (None, BC.ABOVE_MU)] + [(name, BC.BELOW_ALL) for name in BC.EMPTY_CASES]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_band_symbols_version_and_layout():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 13
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
    B = _lib.Band
    assert ctypes.sizeof(B) == 24 and (B.slot.offset, B.cell_band.offset, B.n_rows.offset) == (0, 8, 16)
    assert re.search(r"typedef struct d3f_band \{\s*const int32_t \*slot;[^}]*const uint8_t \*cell_band;[^}]*int64_t n_rows;[^}]*\} d3f_band;", hdr)
    # the structs of ABI 11 are untouched
    assert ctypes.sizeof(_lib.Volume) == 56 and ctypes.sizeof(_lib.VolumeSet) == 32


def test_band_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)

    def vol(shape=(4, 4, 4), step=0.5, dist=p, cell=p):
        return _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), step, 0, dist, p, cell)

    ws_bytes = lib.d3f_band_workspace_bytes(4, 4, 4)
    assert ws_bytes > 0 and lib.d3f_band_workspace_bytes(1, 4, 4) == 0 and lib.d3f_band_workspace_bytes(2048, 1024, 1024) == 0
    assert lib.d3f_band_workspace_bytes(1024, 1024, 1024) < (1 << 22)          # the scan's scratch only: nothing per voxel

    def mark(v=None, band=0.1, cb=p, slot=p, vox=p, cap=8, cnt=p, ws=p, wsb=ws_bytes, null_vol=False):
        return lib.d3f_band_mark(None if null_vol else ctypes.byref(v or vol()), band, cb, slot, vox, cap, cnt, ws, wsb, None)

    assert mark(null_vol=True) == _lib.ERR_INVALID_ARG
    assert mark(v=vol(shape=(1, 4, 4))) == _lib.ERR_BAD_SHAPE
    assert mark(v=vol(shape=(2048, 1024, 1024))) == _lib.ERR_BAD_SHAPE and b"voxels" in lib.d3f_last_error()      # 2^31 > 2^31 - 1, nothing allocated
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert mark(band=bad) == _lib.ERR_INVALID_ARG and b"band" in lib.d3f_last_error()
    assert mark(cap=-1) == _lib.ERR_INVALID_ARG
    assert mark(v=vol(dist=None)) == _lib.ERR_INVALID_ARG and mark(v=vol(cell=None)) == _lib.ERR_INVALID_ARG
    assert mark(cb=None) == _lib.ERR_INVALID_ARG and mark(slot=None) == _lib.ERR_INVALID_ARG and mark(cnt=None) == _lib.ERR_INVALID_ARG
    assert mark(vox=None) == _lib.ERR_INVALID_ARG                         # a positive capacity needs the array
    assert mark(slot=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT and mark(cnt=ctypes.c_void_p(260)) == _lib.ERR_BAD_LAYOUT
    assert mark(ws=None) == _lib.ERR_WORKSPACE and mark(wsb=ws_bytes - 1) == _lib.ERR_WORKSPACE

    def band(n_rows=5, slot=p, cb=p):
        return _lib.Band(slot, cb, n_rows)

    def sets(*Cs, data=256):
        arr = (_lib.VolumeSet * max(len(Cs), 1))()
        for s, C in enumerate(Cs):
            arr[s] = _lib.VolumeSet(data, C, 0, C, None)
        return arr

    outs = (ctypes.c_void_p * _lib.MAX_MAPS)(*([256] * _lib.MAX_MAPS))

    def fwd(v=None, b=None, pts=p, n=5, s=None, ns=0, od=p, ov=p, ob=p, o=outs, null_band=False):
        return lib.d3f_band_sample(ctypes.byref(v or vol()), None if null_band else ctypes.byref(b or band()), pts, n, s, ns, od, ov, ob, o, None)

    def bwd(v=None, b=None, pts=p, n=5, s=None, ns=0, gp=p, null_band=False):
        return lib.d3f_band_sample_backward(ctypes.byref(v or vol()), None if null_band else ctypes.byref(b or band()), pts, n, s, ns, None, None, gp, None)

    for fn in (fwd, bwd):
        assert fn(null_band=True) == _lib.ERR_INVALID_ARG and b"band" in lib.d3f_last_error()
        assert fn(b=band(n_rows=-1)) == _lib.ERR_BAD_SHAPE and b"n_rows" in lib.d3f_last_error()
        assert fn(b=band(n_rows=2 ** 31)) == _lib.ERR_BAD_SHAPE
        assert fn(b=band(slot=None)) == _lib.ERR_INVALID_ARG and fn(b=band(cb=None)) == _lib.ERR_INVALID_ARG
        assert fn(b=band(slot=ctypes.c_void_p(258))) == _lib.ERR_BAD_LAYOUT
        # the volume checks of ABI 11
        assert fn(v=vol(shape=(4, 0, 4))) == _lib.ERR_BAD_SHAPE and fn(v=vol(step=0.0)) == _lib.ERR_INVALID_ARG
        assert fn(n=-1) == _lib.ERR_INVALID_ARG and fn(ns=_lib.MAX_MAPS + 1, s=sets(*([4] * 8))) == _lib.ERR_BAD_SHAPE
        assert fn(s=sets(4, data=None), ns=1) == _lib.ERR_INVALID_ARG          # rows may be NULL only with n_rows == 0
        # n == 0: a no-op, also with an empty band and NULL everything
        assert fn(n=0, pts=None) == 0 and fn(n=0, pts=None, b=band(0, None, None), s=sets(4, data=None), ns=1) == 0
    assert fwd(ob=None) == _lib.ERR_INVALID_ARG and b"out_in_band" in lib.d3f_last_error()
    assert fwd(od=None) == _lib.ERR_INVALID_ARG and bwd(gp=None) == _lib.ERR_INVALID_ARG


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps", ALL_BANDS)
def test_mark_invariants(name, steps):
    vol = BC.volume(name)
    m = BC.mark(vol, BC.band_of(name, steps))
    nx, ny, nz = vol["shape"]
    stored, slot, vox = m["stored"], m["slot"], m["voxels"]
    assert not (stored & ~vol["valid"]).any(), "stored must be a subset of valid"
    assert not (m["seed"] & np.isnan(vol["dist"])).any()
    closure = np.zeros(vol["shape"], bool)
    for dx, dy, dz in BC.CORNERS:
        corner = stored[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
        assert corner[m["cell_band"]].all(), "a kept cell has eight stored corners"
        closure[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] |= m["cell_band"]
    assert np.array_equal(closure, stored), "the stored set is exactly the corner closure of the kept cells"
    assert not (m["cell_band"] & ~m["cell_valid"]).any()
    flat = slot.reshape(-1)
    assert slot.dtype == np.int32 and np.array_equal(flat >= 0, stored.reshape(-1)) and np.all(flat[~stored.reshape(-1)] == -1)
    assert np.array_equal(flat[flat >= 0], np.arange(m["M"])), "slot is the ascending bijection onto 0..M-1"
    assert vox.dtype == np.int32 and vox.size == m["M"] and np.all(np.diff(vox) > 0) and np.array_equal(flat[vox], np.arange(m["M"]))


def test_every_case_keeps_its_conditions():
    for name, (key, steps, selective) in BC.CASES.items():
        vol = BC.volume(name)
        assert vol["mu"] == RC.MU_STEPS * float(vol["step"]) and np.isnan(vol["dist"][~vol["valid"]]).all()
        for st in (None, BC.ABOVE_MU) + ((BC.BELOW_ALL,) if name in BC.EMPTY_CASES else ()):
            band = BC.band_of(name, st)
            assert BC.seed_margin(vol, band) >= BC.SEED_MARGIN, (name, st)
        share = BC.kept_share(BC.mark(vol, BC.band_of(name)))
        if selective:
            assert BC.SELECTIVE[0] <= share <= BC.SELECTIVE[1], (name, share)
            assert min(vol["shape"]) >= 11
        else:
            assert share > 0.5, (name, share)                      # the small fixtures: most cells lie within 1.5 h of the surface
        everything = BC.mark(vol, BC.band_of(name, BC.ABOVE_MU))
        assert np.array_equal(everything["cell_band"], everything["cell_valid"]) and everything["M"] > 0, name
        if name in BC.EMPTY_CASES:
            assert BC.mark(vol, BC.band_of(name, BC.BELOW_ALL))["M"] == 0, name
    holes = [k for k in BC.CASES if "holes" in k]
    assert holes and all((~BC.volume(k)["valid"]).sum() >= 1 for k in holes)
    # the generator's margin (asserted inside) for every point count and seed the GPU tests use
    for name in BC.CASES:
        vol = BC.volume(name)
        if min(vol["shape"]) < 3:
            continue
        for n in (1, 63, 65, 257, 1003):
            assert BC.inside_points(vol, n, n % 5).shape == (n, 3)


def test_in_band_reference_and_selective_points():
    """both kinds of valid point occur in the selective cases, and in_band implies valid"""
    for name, (key, steps, selective) in BC.CASES.items():
        if not selective:
            continue
        vol = BC.volume(name)
        ok, ib = BC.in_band(vol, BC.mark(vol, BC.band_of(name)), BC.inside_points(vol, 1003, 3))
        assert not (ib & ~ok).any() and 0 < ib.sum() < ok.sum(), name


RAY_CASES = [k for k in BC.CASES if k.startswith(("9x8x10", "large")) and "band 0.5h" not in k]


@pytest.mark.parametrize("name", RAY_CASES)
def test_hits_in_valid_cells_lie_in_kept_cells(name):
    """the float64 march puts every hit that lies in a valid cell into a kept cell at band >= h: a banded render loses no row there"""
    vol = BC.volume(name)
    assert BC.CASES[name][1] >= 1.0
    o, d = BC.rays(vol)
    ref = RC.march(vol, o, d)
    keep = ref["hit"] & ~ref["fragile"]
    ok, ib = BC.in_band(vol, BC.mark(vol, BC.band_of(name)), ref["points"].astype(np.float32))
    assert (ok & keep).sum() >= 17 and np.array_equal(ok[keep], ib[keep]), (name, int(ok[keep].sum()), int(ib[keep].sum()))


# ---- Python surface ---------------------------------------------------------------------------------------------------------------
def test_band_argument_checks():
    import inspect
    from d3fields_amd import BakedField, Fusion
    from d3fields_amd.baked import _check_band, _check_band_names
    for bad in (0.0, -0.005, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="band"):
            _check_band(bad, "to_band")
    with pytest.raises(TypeError, match="band"):
        _check_band("thick", "to_band")
    assert _check_band(0.005, "bake") == 0.005
    with pytest.raises(ValueError, match="in_band"):
        _check_band_names(["feat", "in_band"])
    assert inspect.signature(Fusion.bake).parameters["band"].default is None
    assert callable(BakedField.to_band) and callable(BakedField.band_points) and isinstance(BakedField.stored_fraction, property)
    assert VC.CORNERS == BC.CORNERS
