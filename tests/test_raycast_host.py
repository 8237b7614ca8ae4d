"""CPU: the float64 reference of the ray march (tests/raycast_cases.py) against the analytic ray-plane intersection, the conditions
every committed case must keep (fragile share, hits and misses), the float32 port against the reference, and the ABI 12 entry point:
symbol, binding, header prototype and every guard as a status code."""
import ctypes
import os
import re

import numpy as np
import pytest

import raycast_cases as RC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
CASES = RC.case_list()


def case_id(c):
    (shape, kind, family, holes), n, variant = c
    return "%s-%s-%s-%s-N%d-%s" % (shape, kind, family, "holes" if holes else "solid", n, variant.replace(" ", "_"))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_case_keeps_its_conditions(c):
    """At most 3 % of a case's rays are fragile; from 63 rays on at least a quarter of the others hit and a quarter miss.  Nothing is
    filtered: a case that fails this fails the suite."""
    key, n, variant = c
    vol, o, d, kw, ref = RC.case(*c)
    assert o.shape == d.shape == (n, 3) and o.dtype == d.dtype == np.float32
    assert (~vol["valid"]).mean() <= 0.03 and bool(key[3]) == bool((~vol["valid"]).any())
    assert np.isnan(vol["dist"][~vol["valid"]]).all() and np.isfinite(vol["dist"][vol["valid"]]).all()
    assert np.abs(vol["origin"]).min() > 0
    fragile = ref["fragile"]
    assert fragile.mean() <= 0.03, fragile.mean()
    if n >= 63:
        keep = ~fragile
        assert (ref["hit"] & keep).sum() >= keep.sum() / 4 and (~ref["hit"] & keep).sum() >= keep.sum() / 4, (ref["hit"][keep].sum(), keep.sum())
    assert np.all(ref["t"][~ref["hit"]] == 0) and np.isnan(ref["points"][~ref["hit"]]).all()
    assert np.all(ref["t"][ref["hit"]] > 0) and np.isfinite(ref["points"][ref["hit"]]).all()


def test_special_rays_do_what_their_names_say():
    for key in RC.VOLUMES:
        if key[0] == "2x2x2" or key[3]:
            continue
        vol, o, d, kw, ref = RC.case(key, 63, "default")
        got = dict(zip(RC.SPECIALS, zip(ref["hit"], ref["samples"])))
        for name in ("misses the box", "axis-parallel outside the slab", "d = 0", "NaN origin", "NaN direction", "infinite origin", "d = 0 inside the box"):
            assert not got[name][0] and got[name][1] == 0, (key, name)
        assert not got["back face"][0] and got["back face"][1] > 2, key          # it crosses the surface from - to +, inside the box
        assert got["starts inside"][0], key
        if key[1] == "plane":                       # straight down from under the +z face onto a plane whose normal points up
            assert got["axis-parallel inside the slab"][0] and got["two zero components"][0], key
    # the window cuts hits off, the double step loses some
    key = ("9x8x10", "plane", "pow2", False)
    base, win = RC.case(key, 1003, "default")[4], RC.case(key, 1003, "window")[4]
    assert 0 < (base["hit"] & ~win["hit"]).sum() and not (win["hit"] & ~base["hit"]).any()
    half = RC.case(key, 1003, "half step")[4]
    assert half["samples"].sum() > 1.5 * base["samples"].sum()


@pytest.mark.parametrize("key", [k for k in RC.VOLUMES if k[1] == "plane" and not k[3]], ids=lambda k: "%s-%s" % (k[0], k[2]))
@pytest.mark.parametrize("variant", ["default", "half step"])
def test_reference_meets_the_analytic_plane(key, variant):
    """On a solid plane volume t* is the ray-plane intersection.  With a step of at most h, prev <= h and |s| <= h, every corner of the
    two bracketing cells lies within h + sqrt(3) h < mu of the plane, so none is clamped and the interpolant is the plane itself but
    for the float32 storage of the corners, 2^-24 mu each: both samples move by at most that (convex weights), t* by
    dt (|s| + prev) 2^-24 mu / (prev - s)^2 = 2^-24 mu / |d . n|; float64 rounding adds 1e-12 |t|."""
    shape = key[0]
    n = 1003
    if variant == "default":
        vol, o, d, kw, ref = RC.case(key, n, "default")
    else:
        vol = RC.make_volume(*key)
        o, d = RC.random_rays(vol, n, 0)
        kw = {"march_step": np.float32(vol["step"]) * np.float32(0.5)}
        ref = RC.march(vol, o, d, **kw)
    m = ref["hit"] & ~ref["fragile"]
    assert m.sum() >= n / 5, shape
    o64, d64 = o.astype(np.float64)[m], d.astype(np.float64)[m]
    dn = d64 @ vol["normal"]
    want = -((o64 - vol["centre"]) @ vol["normal"]) / dn
    bound = RC.U * vol["mu"] / np.abs(dn) + 1e-12 * np.abs(want)
    err = np.abs(ref["t"][m] - want)
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_port_agrees_with_the_reference(c):
    vol, o, d, kw, ref = RC.case(*c)
    port = RC.march(vol, o, d, f=np.float32, **kw)
    keep = ~ref["fragile"]
    assert port["t"].dtype == np.float32
    assert np.array_equal(port["hit"][keep], ref["hit"][keep])
    assert np.array_equal(port["samples"][keep], ref["samples"][keep])
    worst = RC.worst_ratios(port["t"], port["points"], ref, keep)
    assert worst <= 4 * RC.U, worst / RC.U                    # a few ulp of the bound's terms (and far under the cap)
    assert RC.tolerance(worst) <= RC.CAP


@pytest.mark.parametrize("c", [c for c in CASES if c[1] == 1003 and c[2] == "half step"], ids=case_id)
def test_an_accumulated_t_k_fails_the_bitwise_assert(c):
    """The mutant 't_k = t_{k-1} + dt' of the float32 port stays inside the error bound (the marches are short and t0 dominates k dt),
    so the bound cannot catch it; raycast_cases.assert_equals_port, which the GPU tests apply to the kernel, does."""
    vol, o, d, kw, ref = RC.case(*c)
    keep = ~ref["fragile"]
    port = RC.march(vol, o, d, f=np.float32, **kw)
    bad = RC.march(vol, o, d, f=np.float32, mutant="accumulated t_k", **kw)
    RC.assert_equals_port(port["t"], port["hit"], port["points"], port["samples"], port, keep)
    assert RC.worst_ratios(bad["t"], bad["points"], ref, keep) <= RC.tolerance(RC.worst_ratios(port["t"], port["points"], ref, keep))      # the bound is blind to it
    with pytest.raises(AssertionError, match="bit for bit"):
        RC.assert_equals_port(bad["t"], bad["hit"], bad["points"], bad["samples"], port, keep)


@pytest.mark.parametrize("c", [c for c in CASES if c[1] >= 63], ids=case_id)
def test_a_back_face_hit_fails_the_hit_assert(c):
    """every case of 63 rays or more holds rays that meet the surface from behind (every eighth random ray and the 'back face'
    special): a kernel that takes - to + for a hit differs in hit_mask on non-fragile rays"""
    vol, o, d, kw, ref = RC.case(*c)
    keep = ~ref["fragile"]
    port = RC.march(vol, o, d, f=np.float32, **kw)
    bad = RC.march(vol, o, d, f=np.float32, mutant="back faces hit", **kw)
    assert (bad["hit"] & ~port["hit"] & keep).sum() >= 2
    with pytest.raises(AssertionError, match="hit_mask"):
        RC.assert_equals_port(bad["t"], bad["hit"], bad["points"], bad["samples"], port, keep)


def test_port_ratio_is_not_vacuous():
    vol, o, d, kw, ref = RC.case(("9x8x10", "sphere", "4mm", True), 1003, "default")
    port = RC.march(vol, o, d, f=np.float32, **kw)
    assert 0 < RC.worst_ratios(port["t"], port["points"], ref, ~ref["fragile"])


def test_camera_rays_are_the_pinhole_model():
    K = np.array([[50.0, 0, 7.5], [0, 40.0, 5.5], [0, 0, 1]], np.float32)
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])
    pose = np.concatenate([R, [[0.1], [-0.2], [0.7]]], 1).astype(np.float32)
    o, d = RC.camera_rays(K, pose, 12, 16)
    R64, tc = pose[:, :3].astype(np.float64), pose[:, 3].astype(np.float64)
    assert np.allclose(R64 @ o + tc, 0, atol=1e-6)                              # the camera centre maps to the camera's origin
    v, u = 7, 11                                                              # pixel (u, v) is ray v * W + u; d in camera coordinates has z = 1
    dc = R64 @ d[v * 16 + u].astype(np.float64)
    assert np.allclose(dc, [(u - 7.5) / 50.0, (v - 5.5) / 40.0, 1.0], atol=1e-6)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_raycast_symbol_signature_and_prototype():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert hasattr(lib, "d3f_volume_raycast") and "d3f_volume_raycast" in _lib.SIGNATURES
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 12
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define D3F_RAYCAST_MAX_STEPS (\d+)", hdr).group(1)) == _lib.RAYCAST_MAX_STEPS == 65536
    proto = re.search(r"\bint d3f_volume_raycast\(([^)]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    assert params == ["const d3f_volume *vol", "const float *origins", "const float *dirs", "int64_t n", "const d3f_pinhole *camera", "float march_step",
                      "float t_near", "float t_far", "float *out_t", "uint8_t *out_hit", "float *out_points", "int32_t *out_samples", "void *stream"]
    res, args = _lib.SIGNATURES["d3f_volume_raycast"]
    vp, f32 = ctypes.c_void_p, ctypes.c_float
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.Volume), vp, vp, ctypes.c_int64, ctypes.POINTER(_lib.Pinhole), f32, f32, f32, vp, vp, vp, vp, vp]
    P = _lib.Pinhole
    assert ctypes.sizeof(P) == 92 and (P.K.offset, P.pose.offset, P.H.offset, P.W.offset) == (0, 36, 84, 88)
    assert re.search(r"typedef struct d3f_pinhole \{\s*float K\[9\];[^}]*float pose\[12\];[^}]*int32_t H, W;\s*\} d3f_pinhole;", hdr)


def test_raycast_guards_return_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    inf, nan = float("inf"), float("nan")

    def vol(shape=(4, 4, 4), step=0.5, dist=p, cell=p):
        return _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), step, 0, dist, p, cell)

    def cam(H=4, W=6, fx=50.0, fy=50.0):
        return _lib.Pinhole((ctypes.c_float * 9)(fx, 0, 3, 0, fy, 2, 0, 0, 1), (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), H, W)

    def go(v=None, o=p, d=p, n=5, c=None, march=0.5, near=0.0, far=inf, ot=p, oh=p, op=p, os_=None, null_vol=False):
        return lib.d3f_volume_raycast(None if null_vol else ctypes.byref(v or vol()), o, d, n, None if c is None else ctypes.byref(c), march, near, far,
                                      ot, oh, op, os_, None)

    def err():
        return lib.d3f_last_error()

    assert go(null_vol=True) == _lib.ERR_INVALID_ARG and b"vol" in err()
    assert go(v=vol(shape=(1, 4, 4))) == _lib.ERR_BAD_SHAPE and b"nx=1" in err()
    assert go(v=vol(shape=(2048, 1024, 1024))) == _lib.ERR_BAD_SHAPE and b"voxels" in err()
    assert go(v=vol(step=0.0)) == _lib.ERR_INVALID_ARG and b"step" in err()
    for bad in (0.0, -1.0, nan, inf):
        assert go(march=bad) == _lib.ERR_INVALID_ARG and b"march_step" in err(), bad
    # the box diagonal of 4 x 4 x 4 at h = 0.5 is 2.59808: 65535 steps across it pass, 65540 do not
    assert go(march=2.5981 / 65535, n=0) == 0
    assert go(march=2.5980 / 65540) == _lib.ERR_INVALID_ARG and b"steps" in err()
    assert go(march=1e-30) == _lib.ERR_INVALID_ARG and b"steps" in err()
    for bad in (-1e-6, nan, inf):
        assert go(near=bad) == _lib.ERR_INVALID_ARG and b"t_near" in err(), bad
    assert go(far=nan) == _lib.ERR_INVALID_ARG and b"t_far" in err()
    assert go(far=-inf, n=0) == 0 and go(far=-1.0, n=0) == 0                      # an empty window is no error: every ray misses
    assert go(n=-1) == _lib.ERR_INVALID_ARG and b"n=-1" in err()
    assert go(n=2 ** 31) == _lib.ERR_BAD_SHAPE and b"2^31" in err()
    assert go(n=2 ** 31, c=cam(H=32768, W=65536), o=None, d=None) == _lib.ERR_BAD_SHAPE and b"2^31" in err()
    assert go(c=cam(H=46341, W=46341), o=None, d=None, n=5) == _lib.ERR_BAD_SHAPE and b"H*W" in err()
    assert go(c=cam(H=-1), o=None, d=None, n=0) == _lib.ERR_BAD_SHAPE
    assert go(c=cam(), o=None, d=None, n=23) == _lib.ERR_BAD_SHAPE and b"H*W" in err()
    assert go(c=cam(), d=None, n=24) == _lib.ERR_INVALID_ARG and b"camera" in err()
    for bad in (0.0, nan, inf):
        assert go(c=cam(fx=bad), o=None, d=None, n=24) == _lib.ERR_INVALID_ARG and b"fx" in err()
        assert go(c=cam(fy=bad), o=None, d=None, n=24) == _lib.ERR_INVALID_ARG
    # n == 0 is a no-op with NULL buffers, explicit and camera (H or W zero)
    assert go(v=vol(dist=None, cell=None), o=None, d=None, n=0, ot=None, oh=None, op=None) == 0
    assert go(v=vol(dist=None, cell=None), o=None, d=None, n=0, c=cam(H=0), ot=None, oh=None, op=None) == 0
    assert go(v=vol(dist=None)) == _lib.ERR_INVALID_ARG and b"dist" in err()
    assert go(v=vol(cell=None)) == _lib.ERR_INVALID_ARG
    assert go(o=None) == _lib.ERR_INVALID_ARG and b"origins" in err()
    assert go(d=None) == _lib.ERR_INVALID_ARG
    for k in ("ot", "oh", "op"):
        assert go(**{k: None}) == _lib.ERR_INVALID_ARG and b"out_" in err()
    assert go(o=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT
    assert go(ot=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT
    assert go(os_=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT and b"aligned" in err()
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(go(march=-1.0))
    assert e.value.code == _lib.ERR_INVALID_ARG and "march_step" in str(e.value)
