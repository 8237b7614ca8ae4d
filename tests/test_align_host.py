"""CPU: the d3f_volume_align_* entry points are declared by the header, bound and exported with D3F_ABI_VERSION still 16, and validate their
arguments on the host with the documented status codes before any HIP call; the restatement of tests/align_cases.py has the Jacobian its
central differences give, exact zeros where the contract has them, a pose update that does not depend on the pivot to first order, and a
Levenberg-Marquardt loop that ends CONVERGED on the two-sphere scene from every start, with each status planted once; the float32 port stays
under the cap of the tolerance; align_kernels.hip uses no scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_cases as AC
import band_cases as BC
import volume_cases as VC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
F = np.float32
NAMES = ("d3f_volume_align_workspace_bytes", "d3f_volume_align_centroid", "d3f_volume_align_accumulate", "d3f_volume_align_step")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def _declared(hdr, name):
    decl = re.search(r"\b(?:int|int64_t) %s\(([^;]*)\);" % name, hdr).group(1)
    return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]


def test_align_symbols_and_unchanged_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
    for macro, value in (("ROW_DOUBLES", AC.ROW), ("STATE_DOUBLES", AC.STATE), ("RUNNING", AC.RUNNING), ("CONVERGED", AC.CONVERGED), ("STALLED", AC.STALLED),
                         ("NO_GRADIENT", AC.NO_GRADIENT), ("FAILED", AC.FAILED)):
        assert int(re.search(r"#define D3F_ALIGN_%s (\d+)" % macro, hdr).group(1)) == value == getattr(_lib, "ALIGN_" + macro), macro
    assert _lib.ALIGN_CHUNK == AC.CHUNK
    vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    assert _lib.SIGNATURES[NAMES[0]] == (i64, [i64, i64])
    assert _lib.SIGNATURES[NAMES[1]] == (ctypes.c_int, [vp, vp, i64, i64, vp, vp])
    res, args = _lib.SIGNATURES[NAMES[2]]
    assert res is ctypes.c_int and args[3:] == [vp] * 7 + [i64, i64, f32, f32, f32, vp, vp, i64, vp]
    assert args[:3] == [ctypes.POINTER(_lib.Volume), ctypes.POINTER(_lib.Band), ctypes.POINTER(_lib.VolumeSet)]
    assert _lib.SIGNATURES[NAMES[3]] == (ctypes.c_int, [vp, vp, i64, i64, i64, vp, i32, i32, f64, f64, vp, vp, vp, vp])
    # the declarations have as many parameters, in this order
    assert _declared(hdr, NAMES[0]) == ["I", "n"]
    assert _declared(hdr, NAMES[1]) == ["points", "weights", "I", "n", "centroids_out", "stream"]
    assert _declared(hdr, NAMES[2]) == ["vol", "band", "set", "points", "weights", "targets", "dist_targets", "pose", "centroids", "skip", "I", "n", "dist_weight",
                                        "feat_weight", "outside", "out", "workspace", "workspace_bytes", "stream"]
    assert _declared(hdr, NAMES[3]) == ["state", "workspace", "workspace_bytes", "I", "n", "out", "it", "iters", "rot_tol", "trans_tol", "pose_out", "skip_out",
                                        "history", "stream"]
    for name in NAMES:
        assert len(_declared(hdr, name)) == len(_lib.SIGNATURES[name][1]), name
    # one row of 32 doubles per (instance, 256 points)
    ws = lib.d3f_volume_align_workspace_bytes
    assert ws(1, 1) == ws(1, 256) == 256 and ws(1, 257) == 512 and ws(3, 513) == 3 * 3 * 256 and ws(0, 5) == ws(5, 0) == ws(-1, 5) == 0


def test_align_validation_status_codes():
    lib = _lib.load()
    err = lib.d3f_last_error
    p, q, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p((1 << 20) + 2)
    odd8 = ctypes.c_void_p((1 << 20) + 4)
    vol = _lib.Volume(5, 4, 6, (ctypes.c_float * 3)(0, 0, 0), 0.5, 0, p, p, p)
    good = _lib.VolumeSet(p, 4, 0, 4, None)

    def acc(vol=vol, band=None, st=good, points=p, weights=None, targets=p, dist_targets=None, pose=p, centroids=p, skip=None, I=2, n=300, wd=1.0, wf=1.0,
            outside=0.1, out=q, ws=q, ws_bytes=1 << 20):
        return lib.d3f_volume_align_accumulate(None if vol is None else ctypes.byref(vol), None if band is None else ctypes.byref(band),
                                               None if st is None else ctypes.byref(st), points, weights, targets, dist_targets, pose, centroids, skip, I, n, wd, wf,
                                               outside, out, ws, ws_bytes, None)

    def step(state=p, ws=q, ws_bytes=1 << 20, I=2, n=300, out=q, it=0, iters=3, rot_tol=1e-5, trans_tol=1e-4, pose=p, skip=p, history=q):
        return lib.d3f_volume_align_step(state, ws, ws_bytes, I, n, out, it, iters, rot_tol, trans_tol, pose, skip, history, None)

    # D3F_ERR_INVALID_ARG: NULL pointers, negative counts, weights of the terms that are negative or not finite
    assert acc(vol=None) == _lib.ERR_INVALID_ARG and b"NULL" in err()
    for kw in ("points", "pose", "centroids", "ws", "targets"):
        assert acc(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    assert acc(I=-1) == _lib.ERR_INVALID_ARG and acc(n=-1) == _lib.ERR_INVALID_ARG and b"negative" in err()
    for kw in ("wd", "wf", "outside"):
        for bad in (-1.0, float("nan"), float("inf")):
            assert acc(**{kw: bad}) == _lib.ERR_INVALID_ARG and b"finite" in err(), (kw, bad)
    assert acc(band=_lib.Band(None, None, 5)) == _lib.ERR_INVALID_ARG and b"band" in err()
    assert step(state=None) == _lib.ERR_INVALID_ARG and step(out=None) == _lib.ERR_INVALID_ARG and step(history=None) == _lib.ERR_INVALID_ARG and b"NULL" in err()
    assert step(pose=None) == _lib.ERR_INVALID_ARG and step(skip=None) == _lib.ERR_INVALID_ARG and step(ws=None) == _lib.ERR_INVALID_ARG
    assert step(I=-1) == _lib.ERR_INVALID_ARG and step(n=-2) == _lib.ERR_INVALID_ARG and b"negative" in err()
    assert step(it=4) == _lib.ERR_INVALID_ARG and step(it=-1) == _lib.ERR_INVALID_ARG and step(iters=-1) == _lib.ERR_INVALID_ARG and b"iters" in err()
    for kw in ("rot_tol", "trans_tol"):
        for bad in (-1.0, float("nan"), float("inf")):
            assert step(**{kw: bad}) == _lib.ERR_INVALID_ARG and b"finite" in err(), (kw, bad)
    # D3F_ERR_BAD_SHAPE: C out of range, the volume checks, more workgroups than one launch holds
    for C in (0, -3, _lib.VOLUME_MAX_CHANNELS + 1):
        assert acc(st=_lib.VolumeSet(p, C, 0, 8192, None)) == _lib.ERR_BAD_SHAPE and b"outside" in err(), C
    assert acc(vol=_lib.Volume(1, 4, 6, (ctypes.c_float * 3)(0, 0, 0), 0.5, 0, p, p, p)) == _lib.ERR_BAD_SHAPE
    assert acc(I=1 << 40, n=1 << 20, ws_bytes=1 << 62) == _lib.ERR_BAD_SHAPE and step(I=1 << 40, n=1 << 20, ws_bytes=1 << 62) == _lib.ERR_BAD_SHAPE
    assert acc(band=_lib.Band(p, p, -1)) == _lib.ERR_BAD_SHAPE
    # D3F_ERR_BAD_LAYOUT: misaligned float / double pointers, a stride below C
    for kw in ("points", "weights", "targets", "dist_targets", "pose", "centroids", "skip"):
        assert acc(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    for kw in ("out", "ws"):
        assert acc(**{kw: odd8}) == _lib.ERR_BAD_LAYOUT and b"8-byte" in err(), kw
    assert acc(st=_lib.VolumeSet(p, 4, 0, 3, None)) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in err()
    assert acc(st=_lib.VolumeSet(odd, 4, 0, 4, None)) == _lib.ERR_BAD_LAYOUT
    for kw in ("state", "ws", "out", "history"):
        assert step(**{kw: odd8}) == _lib.ERR_BAD_LAYOUT and b"8-byte" in err(), kw
    for kw in ("pose", "skip"):
        assert step(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"4-byte" in err(), kw
    # D3F_ERR_WORKSPACE: 2 instances x 2 chunks x 256 bytes
    assert acc(ws_bytes=1023) == _lib.ERR_WORKSPACE and step(ws_bytes=1023) == _lib.ERR_WORKSPACE and b"1024" in err()
    # I == 0 or n == 0: D3F_OK and nothing launched, buffers may be NULL; validation still comes first
    for kw in ({"I": 0}, {"n": 0}):
        assert acc(points=None, pose=None, centroids=None, ws=None, out=None, targets=None, ws_bytes=0, **kw) == _lib.OK
        assert step(state=None, ws=None, out=None, pose=None, skip=None, history=None, ws_bytes=0, **kw) == _lib.OK
        assert acc(wd=-1.0, **kw) == _lib.ERR_INVALID_ARG and step(rot_tol=-1.0, **kw) == _lib.ERR_INVALID_ARG
        assert acc(st=_lib.VolumeSet(p, 0, 0, 4, None), **kw) == _lib.ERR_BAD_SHAPE
    cen = lib.d3f_volume_align_centroid
    assert cen(p, None, -1, 4, p, None) == _lib.ERR_INVALID_ARG and cen(None, None, 2, 4, p, None) == _lib.ERR_INVALID_ARG and cen(p, None, 2, 4, None, None) == _lib.ERR_INVALID_ARG
    assert cen(odd, None, 2, 4, p, None) == _lib.ERR_BAD_LAYOUT and cen(p, odd, 2, 4, p, None) == _lib.ERR_BAD_LAYOUT and cen(None, None, 0, 4, None, None) == _lib.OK
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(acc(wd=-1.0))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement against central differences ----------------------------------------------------------------------------------------
def _interior_problem(C=3, n=40, seed=1, margin=0.05):
    """points whose images lie at least `margin` cells from every cell face of the 5x4x6 volume"""
    vol = VC.make_volume(VC.SHAPES["5x4x6"], (C,), seed)
    rng = np.random.default_rng(300 + seed)
    cells = np.asarray(VC.SHAPES["5x4x6"]) - 1
    g = rng.integers(0, cells, size=(n, 3)) + rng.uniform(margin * 2, 1 - margin * 2, size=(n, 3))
    x = np.asarray(VC.ORIGIN, np.float64) + g * VC.STEP
    R = AC.rotation(rng.standard_normal(3), 0.3).astype(F)
    t = (0.02 * rng.standard_normal(3)).astype(F)
    p = ((x - t.astype(np.float64)) @ R.astype(np.float64)).astype(F)
    image = AC.transform32(R, t, p).astype(np.float64)
    gi = (image - np.asarray(VC.ORIGIN, np.float64)) / VC.STEP
    assert np.all(np.abs(gi - np.round(gi)) >= margin), "an image lies closer than the margin to a cell face"
    w = rng.uniform(0.5, 2.0, n).astype(F)
    targets = rng.standard_normal((n, C)).astype(F)
    dist_targets = (0.1 * rng.standard_normal(n)).astype(F)
    return vol, p, R, t, w, targets, dist_targets


def test_jacobian_equals_central_differences():
    """Along an axis the interpolant is exactly linear, so the translation columns agree to rounding: (r(+e) - r(-e)) / 2e carries 2 u |r|-scale / e
    of rounding (the scale: sum |w_c v_c| + |target|, a few operations each: x 8).  A rotation column moves the point along x(e) = c + Exp(e a)(x - c):
    the central difference is off by e^2 / 6 |d^3 r / d e^3|, and with the trilinear bounds |d_a f| <= S / h, |d_ab f| <= 2 S / h^2, |d_xyz f| <= 4 S / h^3
    (S the corner spread) and |x'|, |x''|, |x'''| <= |xs| = rho h that third derivative is at most S (5 rho^3 + 18 rho^2 + 2 rho)."""
    vol, p, R, t, w, targets, dist_targets = _interior_problem()
    model = AC.centroid(p, w)
    ref = AC.accumulate64(vol, None, "s0", p, R, t, model, w, targets, dist_targets, wd=0.7, wf=1.3)
    x, c = ref["x"].astype(np.float64), ref["pivot"]
    base = AC.residuals64(vol, None, "s0", x, w, targets, dist_targets, 0.7, 1.3)
    assert base["valid"].all()
    h = VC.STEP
    rho = np.linalg.norm(x - c, axis=1) / h
    u64 = 2.0 ** -53

    def residuals_at(delta):
        moved = c + (x - c) @ AC.rodrigues(delta[:3]).T + delta[3:]
        res = AC.residuals64(vol, None, "s0", moved, w, targets, dist_targets, 0.7, 1.3)
        assert res["valid"].all()
        return res["r"]

    worst = {"translation": 0.0, "rotation": 0.0}
    for col in range(6):
        rotation = col < 3
        eps = 1e-4 if rotation else 1e-3 * h                     # both keep every point inside its cell: 1e-4 x 6 voxels, 1e-3 of a voxel
        d = np.zeros(6)
        d[col] = eps
        diff = (residuals_at(d) - residuals_at(-d)) / (2 * eps)
        rounding = 8 * 2 * u64 * base["rabs"] / eps
        trunc = eps ** 2 / 6 * base["spread"] * (5 * rho ** 3 + 18 * rho ** 2 + 2 * rho)[:, None] if rotation else 0.0
        gap = np.abs(diff - ref["J"][:, :, col])
        assert np.all(gap <= rounding + trunc), (col, float((gap - rounding - trunc).max()))
        scale = np.abs(ref["J"][:, :, col]).max()
        worst["rotation" if rotation else "translation"] = max(worst["rotation" if rotation else "translation"], float(gap.max() / scale))
    print("central differences: worst gap / largest entry", worst)
    assert worst["translation"] < 1e-9 and worst["rotation"] < 1e-4              # (the bounds above are what is asserted; these say they are not vacuous)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("banded", [False, True])
def test_H_is_symmetric_psd_and_zero_residuals_give_exact_zeros(banded):
    vol, p, R, t, w, _, _ = _interior_problem(C=5, n=60, seed=2)
    mark = BC.mark(vol, AC.band_of(vol)) if banded else None
    model = AC.centroid(p, w)
    image = AC.transform32(R, t, p)
    sampled = VC.trilinear64(vol, image, ["s0"])["s0"][0]                       # float64: the field at the pose under test
    ref = AC.accumulate64(vol, mark, "s0", p, R, t, model, w, sampled, None, wd=0.0, wf=1.0)
    assert ref["cost"] == 0.0 and not ref["b"].any()
    assert np.array_equal(ref["H"], ref["H"].T)
    assert np.linalg.eigvalsh(ref["H"]).min() >= -1e-12 * np.abs(ref["H"]).max()
    if mark is not None:
        assert 0 < ref["in_band"] < ref["valid"] == len(p), (ref["in_band"], ref["valid"])
    full = AC.accumulate64(vol, mark, "s0", p, R, t, model, w, sampled + 0.25, 0.1 * np.ones(len(p)), wd=0.5, wf=1.0)
    assert np.array_equal(full["H"], full["H"].T) and np.linalg.eigvalsh(full["H"]).min() >= -1e-12 * np.abs(full["H"]).max()
    assert full["cost"] > 0 and full["b"].any()
    H, b, cost, valid, in_band = AC.unpack_row(AC.row_of(full))
    assert np.array_equal(H, full["H"]) and np.array_equal(b, full["b"]) and (cost, valid, in_band) == (full["cost"], full["valid"], full["in_band"])


# ---- invariances ------------------------------------------------------------------------------------------------------------------------
def test_the_pivot_changes_delta_but_not_the_updated_pose():
    """With pivots c1, c2 the linearised motions w x (x - c) + v agree for the same w and v1 = v2 + w x (c1 - c2), so the undamped steps map onto
    each other exactly; the finite motions differ by (I - Exp(w) + [w]x)(c1 - c2), of size <= |w|^2 |c1 - c2| / 2 -- asserted as such."""
    vol, p, R, t, w, targets, dist_targets = _interior_problem(C=3, n=50, seed=3)
    image = AC.transform32(R, t, p)
    targets = (VC.trilinear64(vol, image, ["s0"])["s0"][0] + 1e-4 * np.random.default_rng(5).standard_normal(targets.shape)).astype(F)     # a small step
    m1 = AC.centroid(p, w)
    m2 = (m1 + np.array([0.3, -0.2, 0.25], F)).astype(F)
    out = []
    for m in (m1, m2):
        ref = AC.accumulate64(vol, None, "s0", p, R, t, m, w, targets, dist_targets * 0, wd=0.5)
        status, delta = AC.solve_ref(ref["H"][AC.TRIU], ref["b"], 0.0)
        assert status == AC.RUNNING
        assert np.allclose(delta, np.linalg.solve(ref["H"], -ref["b"]), rtol=100 * np.linalg.cond(ref["H"]) * 2.0 ** -53, atol=0)
        E = AC.rodrigues(delta[:3])
        x = ref["x"].astype(np.float64)
        out.append((delta, ref["pivot"], ref["pivot"] + (x - ref["pivot"]) @ E.T + delta[3:]))
    (d1, c1, x1), (d2, c2, x2) = out
    cond = np.linalg.cond(ref["H"])
    assert np.linalg.norm(d1[3:] - d2[3:]) > 1e3 * np.linalg.norm(d1[:3] - d2[:3])                          # delta does change: the translation part
    assert np.allclose(d1[:3], d2[:3], rtol=0, atol=100 * cond * 2.0 ** -53 * np.linalg.norm(d1[:3]))
    assert np.allclose(d1[3:], d2[3:] + np.cross(d1[:3], c1 - c2), rtol=0, atol=100 * cond * 2.0 ** -53 * np.linalg.norm(d1))
    second_order = 0.5 * np.dot(d1[:3], d1[:3]) * np.linalg.norm(c1 - c2)
    assert np.abs(x1 - x2).max() <= second_order + 100 * cond * 2.0 ** -53 * np.linalg.norm(d1)
    assert second_order < 1e-3 * np.abs(x1 - AC.transform32(R, t, p)).max()                                # ... which is far below the step itself


def test_a_point_of_weight_zero_and_a_missing_point_give_identical_sums():
    vol, p, R, t, w, targets, dist_targets = _interior_problem(C=4, n=33, seed=4)
    model = AC.centroid(p[:-1], w[:-1])
    short = AC.accumulate64(vol, None, "s0", p[:-1], R, t, model, w[:-1], targets[:-1], dist_targets[:-1])
    w0 = w.copy()
    w0[-1] = 0
    assert np.array_equal(AC.centroid(p, w0), model)
    padded = AC.accumulate64(vol, None, "s0", p, R, t, model, w0, targets, dist_targets)
    for k in ("H", "b", "cost"):
        assert np.allclose(padded[k], short[k], rtol=0, atol=1e-14 * np.max(short["A_" + k])), k
    assert (padded["valid"], padded["in_band"]) == (short["valid"], short["in_band"]) == (32, 32)
    nan = p.copy()
    nan[-1] = np.nan                                                    # ... also when the padding holds no coordinates at all
    again = AC.accumulate64(vol, None, "s0", nan, R, t, model, w0, targets, dist_targets)
    assert np.isfinite(again["H"]).all() and np.allclose(again["H"], short["H"], rtol=0, atol=1e-14 * np.max(short["A_H"])) and again["cost"] == padded["cost"]
    # a weighted point outside adds its weight times outside^2 to the cost and nothing else
    far = p.copy()
    far[-1] = 100.0
    out = AC.accumulate64(vol, None, "s0", far, R, t, model, w, targets, dist_targets, outside=0.5)
    assert np.isclose(out["cost"], short["cost"] + float(w[-1]) * 0.25, rtol=1e-14) and np.allclose(out["H"], short["H"], rtol=0, atol=1e-14 * np.max(short["A_H"]))
    assert out["valid"] == 32


# ---- the float32 port ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,vec", [(1, False), (3, False), (4, True), (20, True), (20, False), (68, True)])
def test_the_float32_port_stays_under_the_cap(C, vec):
    """on a case whose coordinates do not round (no slack) the port's error shows against A alone; on a general case the slack is added"""
    worst = 0.0
    for c, slack in ((AC.exact_case("5x4x6", C, 65, 2, 0.1), False), (AC.entry_case("5x4x6", C, 65, 2, 0.1, True), True)):
        mark = BC.mark(c["vol"], AC.band_of(c["vol"]))
        model = AC.centroid(c["p"], c["w"])
        args = (c["vol"], mark, "s0", c["p"], c["R"], c["t"], model, c["w"], c["targets"], c["dist_targets"], 0.75, 1.25)
        ref, port = AC.accumulate64(*args), AC.accumulate32(*args, vec=vec)
        assert (port["valid"], port["in_band"]) == (ref["valid"], ref["in_band"]) and 0 < ref["in_band"] < ref["valid"] < 65
        got = AC.ratios(port, ref, slack)
        print("C = %d vec = %s slack = %s: port worst ratios (H, b, cost) %s x 2^-24, cap %.3g x 2^-24" % (C, vec, slack, np.round(np.array(got) / AC.U, 4), AC.cap(C) / AC.U))
        worst = max(worst, *got)
    assert 0 < 3 * worst <= AC.cap(C)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def test_the_scene_is_not_rotationally_symmetric():
    s = AC.scene()
    feat = s["vol"]["sets"]["feat"].astype(np.float64)
    assert feat.shape[3] == AC.SCENE_CHANNELS and len(s["p"]) == 225
    # no axis is left alone by all four channel gradients: the descriptors pin every rotation
    grads = np.stack([np.stack(np.gradient(feat[..., k]), -1).reshape(-1, 3) for k in range(4)], 1)      # [voxels, 4, 3]
    assert np.linalg.svd(grads.reshape(-1, 3), compute_uv=False).min() > 1.0
    ref = AC.accumulate64(s["vol"], None, "feat", s["p"], s["R"], s["t"], AC.centroid(s["p"]), targets=s["targets"])
    assert np.linalg.cond(ref["H"]) < 1e6 and ref["valid"] == 225
    assert max(a for a, _, _ in AC.STARTS) == 10.0 and max(v for _, v, _ in AC.STARTS) == 2.5


@pytest.mark.parametrize("start", AC.STARTS)
@pytest.mark.parametrize("banded", [False, True])
def test_the_restatement_converges_on_the_scene(start, banded):
    s = AC.scene()
    mark = BC.mark(s["vol"], AC.SCENE_BAND_STEPS * VC.STEP) if banded else None
    R, t = AC.scene_start(*start)
    before = AC.point_error_voxels(AC.transform32(R, t, s["p"]))
    fit = AC.align_ref(s["vol"], mark, "feat", s["p"], R, t, targets=s["targets"], iters=20)
    after = AC.point_error_voxels(fit["points"])
    print(start, "banded" if banded else "dense", "error %.3f -> %.5f voxels, %d steps, cost %.4g -> %.4g" % (before, after, fit["steps"], fit["history"][0], fit["cost"]))
    assert before > start[1]
    assert fit["status"] == AC.CONVERGED and fit["valid"] == 225
    assert after < 0.05
    assert np.all(np.diff(fit["history"]) <= 0) and fit["history"][-1] == fit["cost"] < 1e-3 * fit["history"][0]
    assert 1 <= fit["steps"] <= 20


def test_planted_statuses():
    s = AC.scene()
    vol = s["vol"]
    R, t = AC.scene_start(10.0, 2.5, 1)
    # RUNNING: one iteration is not enough
    fit = AC.align_ref(vol, None, "feat", s["p"], R, t, targets=s["targets"], iters=1)
    assert fit["status"] == AC.RUNNING and fit["steps"] == 1 and fit["history"][1] < fit["history"][0]
    fit0 = AC.align_ref(vol, None, "feat", s["p"], R, t, targets=s["targets"], iters=0)
    assert fit0["status"] == AC.RUNNING and fit0["steps"] == 0 and np.array_equal(fit0["R"], R) and fit0["history"].tolist() == [fit["history"][0]]
    # NO_GRADIENT: every point outside the volume; the pose is unchanged and the cost is the penalty
    away = (t + F(10.0)).astype(F)
    fit = AC.align_ref(vol, None, "feat", s["p"], R, away, targets=s["targets"], outside=0.5)
    assert fit["status"] == AC.NO_GRADIENT and fit["valid"] == 0 and fit["steps"] == 0 and np.array_equal(fit["R"], R) and np.array_equal(fit["t"], away)
    assert fit["cost"] == 225 * 0.25 and (fit["history"] == fit["cost"]).all()
    # STALLED: one point in the crease of dist = |x - x0| with a target below it -- the gradient is that of the cell on the right, every step to the
    # left raises the cost, and lambda climbs to its maximum
    crease = {"origin": np.zeros(3, F), "step": F(VC.STEP), "shape": (6, 3, 3), "valid": np.ones((6, 3, 3), bool), "sets": {}, "fills": {}}
    crease["dist"] = np.broadcast_to((np.abs(np.arange(6) - 3) * VC.STEP)[:, None, None], (6, 3, 3)).astype(F).copy()
    point = np.array([[3 * VC.STEP, 1.25 * VC.STEP, 0.75 * VC.STEP]], F)
    fit = AC.align_ref(crease, None, None, point, np.eye(3, dtype=F), np.zeros(3, F), dist_targets=np.array([-VC.STEP], F))
    assert fit["status"] == AC.STALLED and fit["steps"] == 0 and fit["state"][AC.S_LAMBDA] == AC.LAMBDA_MAX
    assert (fit["history"] == fit["history"][0]).all() and fit["history"][0] == VC.STEP ** 2
    # FAILED: a system that is not finite
    st = AC.new_state(np.eye(3), np.zeros(3), np.zeros(3))
    row = np.zeros(AC.ROW)
    row[:21] = np.eye(6)[AC.TRIU]
    row[1] = np.inf
    _, _, skip = AC.step_ref(st, row, 0, 5, 1e-5, 1e-5)
    assert int(st[AC.S_STATUS]) == AC.FAILED and skip == 1


def test_step_transitions_on_a_planted_sequence():
    """equal costs reject, lambda clamps at both ends, every final state stays what it is"""
    H = np.diag([4.0, 3.0, 2.0, 5.0, 6.0, 7.0])
    row = np.zeros(AC.ROW)
    row[:21], row[21:27] = H[AC.TRIU], 1e-3 * np.arange(1, 7)
    st = AC.new_state(np.eye(3), np.zeros(3), np.zeros(3))
    costs = [5.0, 4.0, 3.0, 2.5, 2.0, 1.5, 1.0, 0.9, 0.8, 0.8]                 # eight accepted steps, then an equal cost
    lambdas = []
    for it, cost in enumerate(costs):
        row[27] = cost
        AC.step_ref(st, row, it, 40, 0.0, 0.0)
        lambdas.append(st[AC.S_LAMBDA])
    assert lambdas[0] == 1e-3 and abs(lambdas[6] - 1e-9) < 1e-23 and lambdas[7] == lambdas[8] == 1e-9 and np.all(np.diff(lambdas[:7]) < 0)      # the clamp below
    assert lambdas[9] == 1e-8 and st[AC.S_STEPS] == 8 and st[AC.S_COST] == 0.8                                          # the equal cost was rejected
    it = len(costs)
    while int(st[AC.S_STATUS]) == AC.RUNNING:
        row[27] = float("nan") if it % 2 else 0.8                                # NaN and equal costs: rejected
        AC.step_ref(st, row, it, 40, 0.0, 0.0)
        it += 1
    assert int(st[AC.S_STATUS]) == AC.STALLED and st[AC.S_LAMBDA] == 1e6 and 13 <= it - len(costs) <= 15 and st[AC.S_STEPS] == 8
    frozen = st.copy()
    row[27] = 0.0
    hist, pose, skip = AC.step_ref(st, row, it, 40, 0.0, 0.0)
    assert np.array_equal(st, frozen) and skip == 1 and hist == 0.8
    # CONVERGED: a step below both tolerances that was ACCEPTED, or one proposed at a pose that was just accepted; one proposed after a
    # rejection has to be accepted first.  Here |w| = 1.66e-3 and |v| = 1.44e-3 at lambda = 1e-3, and half of that at lambda = 1.
    st = AC.new_state(np.eye(3), np.zeros(3), np.zeros(3))
    for it, cost in enumerate([1.0, 1.0, 2.0, 1.0]):
        row[27] = cost
        AC.step_ref(st, row, it, 40, 1e-3, 1e-3)
        assert int(st[AC.S_STATUS]) == AC.RUNNING, it                             # too large at first, then small but proposed after a rejection
    d = st[AC.S_DELTA:AC.S_DELTA + 6]
    assert st[AC.S_LAMBDA] == 1.0 and np.linalg.norm(d[:3]) < 1e-3 and np.linalg.norm(d[3:]) < 1e-3
    row[27] = 0.5
    AC.step_ref(st, row, 4, 40, 1e-3, 1e-3)
    assert int(st[AC.S_STATUS]) == AC.CONVERGED and st[AC.S_STEPS] == 1 and st[AC.S_COST] == 0.5
    st = AC.new_state(np.eye(3), np.zeros(3), np.zeros(3))
    row[27] = 1.0
    _, pose, skip = AC.step_ref(st, row, 0, 40, 1e-2, 1e-2)                         # proposed at the pose iteration 0 accepted: not taken
    assert int(st[AC.S_STATUS]) == AC.CONVERGED and st[AC.S_STEPS] == 0 and skip == 1 and np.array_equal(pose, st[0:12].astype(F)) and np.array_equal(st[0:12], st[12:24])


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "align_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    for kernel in ("align_accumulate_kernel", "align_step_kernel", "align_fold_kernel", "align_centroid_kernel"):
        assert any(kernel in r[0] for r in rows), (kernel, out[-800:])
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0, (name, vgpr, scratch, occ)
