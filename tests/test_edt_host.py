"""CPU: ABI 14 (the exact Euclidean distance transform, d3f_volume_edt) is declared by the header, the binding and the library; the
entry point validates its arguments on the host with the documented status codes and launches nothing; the NumPy restatement
(tests/edt_cases.py) equals the brute-force minimum over all sites and, where scipy imports, scipy's transform; every case keeps the
conditions that make it a case."""
import ctypes
import os
import re

import numpy as np
import pytest

import edt_cases as EC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_volume_edt_workspace_bytes", "d3f_volume_edt")
SMALL = [name for name in EC.CASES if EC.site_volume(name).size <= 1000]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_edt_symbols_and_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 14
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
    assert int(re.search(r"#define D3F_EDT_MAX_EXTENT (\d+)", hdr).group(1)) == _lib.EDT_MAX_EXTENT == 16384


REJECTED_SHAPES = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2048, 1024, 1024), (16384, 16384, 8)]
ACCEPTED_SHAPES = [(1, 1, 1), (4, 4, 4), (16384, 1, 1), (1, 16384, 1), (1, 1, 16384), (16384, 16384, 1), (2047, 1024, 1024)]


def test_edt_workspace_bytes_is_zero_exactly_for_rejected_shapes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    for shape in REJECTED_SHAPES:
        assert lib.d3f_volume_edt_workspace_bytes(*shape) == 0, shape
        assert lib.d3f_volume_edt(p, *shape, 0.5, 0, p, p, p, p, 1 << 62, None) == _lib.ERR_BAD_SHAPE, shape
    for shape in ACCEPTED_SHAPES:
        n = shape[0] * shape[1] * shape[2]
        got = lib.d3f_volume_edt_workspace_bytes(*shape)
        assert 6 * n <= got <= 6 * n + 8, shape                 # one int32 and one int16 volume
        assert lib.d3f_volume_edt(p, *shape, 0.5, 0, p, p, p, p, got - 1, None) == _lib.ERR_WORKSPACE, shape      # the shape itself passes


def test_edt_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    ws_bytes = lib.d3f_volume_edt_workspace_bytes(4, 5, 6)

    def edt(site=p, shape=(4, 5, 6), step=0.5, max_d2=0, d2=p, nearest=p, dist=p, ws=p, wsb=ws_bytes):
        return lib.d3f_volume_edt(site, shape[0], shape[1], shape[2], step, max_d2, d2, nearest, dist, ws, wsb, None)

    assert edt(site=None) == _lib.ERR_INVALID_ARG and b"site" in lib.d3f_last_error()
    assert edt(d2=None, nearest=None, dist=None) == _lib.ERR_INVALID_ARG
    assert edt(shape=(0, 5, 6)) == _lib.ERR_BAD_SHAPE and edt(shape=(4, 16385, 6)) == _lib.ERR_BAD_SHAPE
    assert edt(shape=(2048, 1024, 1024)) == _lib.ERR_BAD_SHAPE and b"voxels" in lib.d3f_last_error()
    assert edt(max_d2=-1) == _lib.ERR_INVALID_ARG and b"max_d2" in lib.d3f_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert edt(step=bad) == _lib.ERR_INVALID_ARG and b"step" in lib.d3f_last_error(), bad
        assert edt(step=bad, dist=None, ws=None) == _lib.ERR_WORKSPACE          # without out_dist the step is not looked at
    assert edt(d2=odd) == _lib.ERR_BAD_LAYOUT and edt(nearest=odd) == _lib.ERR_BAD_LAYOUT and edt(dist=odd) == _lib.ERR_BAD_LAYOUT
    assert edt(ws=odd) == _lib.ERR_BAD_LAYOUT
    assert edt(ws=None) == _lib.ERR_WORKSPACE and edt(wsb=ws_bytes - 1) == _lib.ERR_WORKSPACE and edt(wsb=0) == _lib.ERR_WORKSPACE
    # every single output alone passes the NULL check (and stops at the workspace here: nothing is launched without a GPU)
    assert edt(nearest=None, dist=None, ws=None) == edt(d2=None, dist=None, ws=None) == edt(d2=None, nearest=None, ws=None) == _lib.ERR_WORKSPACE
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(edt(max_d2=-5))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_edt_ref_equals_brute_force(name):
    site = EC.site_volume(name)
    assert np.array_equal(EC.true_d2(name), EC.brute_force(site))
    for cap in EC.CAPS:
        assert np.array_equal(EC.edt_ref(site, cap), np.minimum(EC.brute_force(site), cap))


@pytest.mark.parametrize("name", [n for n in EC.CASES if n != "no site"])      # scipy's transform needs a background voxel
def test_edt_ref_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    site = EC.site_volume(name) != 0
    idx = ndi.distance_transform_edt(~site, return_distances=False, return_indices=True)
    v = np.indices(site.shape)
    assert np.array_equal(((v - idx).astype(np.int64) ** 2).sum(0), EC.true_d2(name).astype(np.int64))
    assert site[tuple(idx)].all()


def test_check_nearest_catches_a_wrong_index():
    site = EC.site_volume("9x8x10 2%")
    d2 = EC.true_d2("9x8x10 2%")
    s = np.argwhere(site != 0).astype(np.int64)
    v = np.argwhere(np.ones(site.shape, bool)).astype(np.int64)
    d = ((v[:, None, :] - s[None, :, :]) ** 2).sum(-1)
    flat = np.ravel_multi_index(tuple(s.T), site.shape)
    good = flat[d.argmin(1)].reshape(site.shape)
    EC.check_nearest(site, d2, good)
    EC.check_nearest(site, d2, np.where(d2 > 5, -1, good), cap=5)
    with pytest.raises(AssertionError):
        EC.check_nearest(site, d2, good, cap=5)                      # -1 is missing beyond the cap
    with pytest.raises(AssertionError):
        EC.check_nearest(site, d2, flat[d.argmax(1)].reshape(site.shape))      # a site, but not the nearest
    bad = good.copy()
    bad[0, 0, 0] = int(np.flatnonzero(site.reshape(-1) == 0)[0])
    with pytest.raises(AssertionError):
        EC.check_nearest(site, d2, bad)                              # no site at all


# ---- case conditions: no case passes vacuously --------------------------------------------------------------------------------------
def test_case_conditions():
    assert len(set(EC.CASES)) == len(EC.CASES)
    for name in EC.RANDOM:
        site = EC.site_volume(name)
        assert site.shape == EC.RANDOM[name][0] and (site != 0).any() and not (site != 0).all(), name
        assert site.max() > 1, name                                  # any non-zero byte is a site, not only 1
    for name in EC.TIE_CASES:
        assert (EC.nearest_count(EC.site_volume(name)) > 1).any(), name
    assert (EC.nearest_count(EC.site_volume("checkerboard")) > 1).mean() > 0.4      # mostly ties (the plane's ties are those of the z and y passes: a whole row of f = 0)
    assert (EC.true_d2("plane")[:, 3] == 0).all() and EC.true_d2("plane").max() == 16
    for name in EC.CAP_CASES:
        d2 = EC.true_d2(name)
        for cap in EC.CAPS:
            assert (d2 < cap).any() and (d2 == cap).any() and (d2 > cap).any(), (name, cap)
    for name, corner in EC.CORNER_CASES.items():
        site = EC.site_volume(name)
        far = tuple(n - 1 - c for n, c in zip(site.shape, corner))
        assert EC.true_d2(name)[far] == sum((n - 1) ** 2 for n in site.shape), name
    assert (EC.true_d2("no site") == EC.INT32_MAX).all() and (EC.true_d2("all sites") == 0).all()
    assert np.isposinf(EC.dist_ref(EC.true_d2("no site"), 0.5)).all()
    # a line of every pass on either side of every boundary between two kernel forms
    z_extents = {EC.site_volume(n).shape[2] for n in EC.CASES}
    assert any(n <= 32 for n in z_extents) and any(32 < n <= 64 for n in z_extents) and any(n > 64 for n in z_extents) and 1 in z_extents
    for axis in (0, 1):
        ext = {EC.site_volume(n).shape[axis] for n in EC.CASES}
        assert any(n <= 256 for n in ext) and any(256 < n <= 512 for n in ext) and any(512 < n <= 1280 for n in ext) and any(n > 1280 for n in ext), axis
