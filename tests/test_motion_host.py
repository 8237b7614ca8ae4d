"""CPU: the motion entry points (d3f_part_motion, d3f_part_motion_workspace_bytes) are declared by the header, bound and exported with
D3F_ABI_VERSION still 16 and validate their arguments on the host with the documented status codes; the NumPy restatement
(tests/motion_cases.py) folds as a plain recursion does and within the float64 chain bound of math.fsum, its Horn block agrees with
SVD-Kabsch, and the whole loop agrees with a second formulation within 1e-9 voxels -- a wiring catch, not a precision claim: a wiring error
is of order 1 -- with identical inlier sets; the planted cases come out as planted; PartMotions' arithmetic on host tensors; no kernel of
motion_kernels.hip uses scratch and the file names no fused operation."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import motion_cases as MC
from conftest import ROOT
from d3fields_amd import _lib, build

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SOURCE = os.path.join(ROOT, "d3fields_amd", "csrc", "motion_kernels.hip")
SYMBOLS = ("d3f_part_motion_workspace_bytes", "d3f_part_motion")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_version_and_sources():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr), name
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert (define("D3F_MOTION_OK"), define("D3F_MOTION_THINNED"), define("D3F_MOTION_TOO_FEW")) == (_lib.MOTION_OK, _lib.MOTION_THINNED, _lib.MOTION_TOO_FEW)
    assert (_lib.MOTION_OK, _lib.MOTION_THINNED, _lib.MOTION_TOO_FEW) == (MC.OK, MC.THINNED, MC.TOO_FEW) and len({MC.OK, MC.THINNED, MC.TOO_FEW}) == 3
    assert define("D3F_MOTION_MAX_FITS") == _lib.MOTION_MAX_FITS == MC.MAX_FITS == 8
    assert define("D3F_MOTION_SUM_DOUBLES") == _lib.MOTION_SUM_DOUBLES == MC.SUMS and define("D3F_MOTION_POSE_DOUBLES") == _lib.MOTION_POSE_DOUBLES == MC.POSE
    assert define("D3F_POOL_CHUNK") == MC.CHUNK
    assert "motion_kernels.hip" in build.SOURCES and os.path.exists(SOURCE)
    import d3fields_amd
    assert d3fields_amd.PartMotions is d3fields_amd.baked.PartMotions and hasattr(d3fields_amd.Flow, "motions")


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.d3f_part_motion_workspace_bytes
    for args in ((0, 5, 6, 1, 10), (4, 16385, 6, 1, 10), (4, 5, -1, 1, 10), (2048, 1024, 1024, 1, 10), (4, 5, 6, -1, 10), (4, 5, 6, 121, 10), (4, 5, 6, 3, -1)):
        assert ws(*args) == 0, args
    for args in ((4, 5, 6, 0, 0), (4, 5, 6, 3, 0), (4, 5, 6, 120, 120), (41, 40, 41, 12, 70000), (16384, 2, 2, 5, 1 << 40)):
        assert ws(*args) > 0 and ws(*args) % 256 == 0, args
    assert ws(64, 64, 64, 10, 1000) < ws(64, 64, 64, 10, 100000)
    assert ws(4, 5, 6, 3, 120) == ws(4, 5, 6, 3, 10 ** 12)                   # the capacity is cut at the voxel count


def test_validation_status_codes():
    lib = _lib.load()
    p, odd4, odd8 = 256, 258, 260
    names = ("label", "target", "members", "pairs", "pose", "inliers", "rmse", "status", "fits_out")

    def motion(label=p, K=3, shape=(4, 5, 6), keep=None, target=p, offset=None, ref=None, fits=3, tau2=1.0, min_pairs=8, cap=50, members=p, pairs=p, pose=p,
               inliers=p, rmse=p, status=p, fits_out=p, res2=None, inlier=None, sums=None, ws=p, ws_bytes=None):
        v = ctypes.c_void_p
        if ws_bytes is None:
            ws_bytes = max(lib.d3f_part_motion_workspace_bytes(shape[0], shape[1], shape[2], K, cap), 0)
        return lib.d3f_part_motion(v(label), K, shape[0], shape[1], shape[2], v(keep), v(target), v(offset), v(ref), fits, tau2, min_pairs, cap, v(members), v(pairs),
                                   v(pose), v(inliers), v(rmse), v(status), v(fits_out), v(res2), v(inlier), v(sums), v(ws), ws_bytes, None)

    for name in names:
        assert motion(**{name: None}) == _lib.ERR_INVALID_ARG and b"NULL" in lib.d3f_last_error(), name
    assert motion(K=-1) == _lib.ERR_INVALID_ARG and b"K=" in lib.d3f_last_error()
    for bad in (0, -1, 9, 100):
        assert motion(fits=bad) == _lib.ERR_INVALID_ARG and b"fits" in lib.d3f_last_error(), bad
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert motion(tau2=bad) == _lib.ERR_INVALID_ARG and b"tau2" in lib.d3f_last_error(), bad
    for bad in (2, 0, -5):
        assert motion(min_pairs=bad) == _lib.ERR_INVALID_ARG and b"min_pairs" in lib.d3f_last_error(), bad
    assert motion(cap=-1) == _lib.ERR_INVALID_ARG and b"member_capacity" in lib.d3f_last_error()
    for shape in ((0, 5, 6), (4, 16385, 6), (4, 5, -1), (2048, 1024, 1024)):
        assert motion(shape=shape) == _lib.ERR_BAD_SHAPE and b"extent" in lib.d3f_last_error(), shape
    assert motion(K=121) == _lib.ERR_BAD_SHAPE and b"exceeds" in lib.d3f_last_error()
    for kw in ({"label": odd4}, {"target": odd4}, {"ref": odd4}, {"pairs": odd4}, {"inliers": odd4}, {"status": odd4}, {"fits_out": odd4}, {"offset": odd8},
               {"members": odd8}, {"pose": odd8}, {"rmse": odd8}, {"res2": odd8}, {"sums": odd8}, {"ws": odd8}):
        assert motion(**kw) == _lib.ERR_BAD_LAYOUT and b"aligned" in lib.d3f_last_error(), kw
    need = lib.d3f_part_motion_workspace_bytes(4, 5, 6, 3, 50)
    assert motion(ws=None) == _lib.ERR_WORKSPACE and motion(ws_bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.d3f_last_error()
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(motion(fits=0))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement: the tree ------------------------------------------------------------------------------------------------------
def test_fold_is_the_recursion_and_stays_within_the_chain_bound():
    rng = np.random.default_rng(3)
    u = 2.0 ** -53
    for m in (1, 2, 63, 64, 65, 255, 256, 257, 513, 700, 65537):
        rows = rng.normal(size=(m, 3)) * 10.0 ** rng.integers(-3, 4, size=(m, 1))
        got = MC.fold(rows)
        assert got.dtype == np.float64 and got.shape == (3,)
        if m <= 700:
            assert got.tobytes() == MC.fold_recursive(rows).tobytes(), m
        depth = 10 * (1 if m <= 256 else 2 if m <= 65536 else 3)          # adds on the longest path: 4 per lane and 6 steps per level
        gamma = depth * u / (1 - depth * u)
        for e in range(3):
            exact, mass = math.fsum(rows[:, e]), math.fsum(np.abs(rows[:, e]))
            assert abs(got[e] - exact) <= gamma * mass, (m, e)
    assert MC.fold(np.zeros((0, 16))).tobytes() == np.zeros(16).tobytes()
    neg = MC.fold(np.full((5, 2), -0.0))
    assert (neg == 0).all() and not np.signbit(neg).any()                   # the fold starts from +0.0
    ints = rng.integers(-1000, 1000, size=(3000, 16)).astype(np.float64)   # small integers: any order gives the exact sums
    assert np.array_equal(MC.fold(ints), ints.sum(axis=0))


def test_moment_rows_and_members():
    a, b = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 2.0]]), np.array([[4.0, 5.0, 6.0], [-0.5, 0.25, 7.0]])
    rows = MC.moment_rows(a, b)
    assert rows[0].tolist() == [1, 1, 2, 3, 4, 5, 6, 4, 5, 6, 8, 10, 12, 12, 15, 18]
    assert np.signbit(rows[1, 7]) and rows[1, 7] == 0 and not np.signbit(MC.fold(rows[1:])[7])      # 0 * -0.5 = -0.0; 0.0 + -0.0 = +0.0
    assert not MC.moment_rows(a, b, np.array([True, False]))[1].any() and not np.signbit(MC.moment_rows(a, b, np.array([True, False]))[1]).any()
    label = np.int32([[[0, 2, 1, 2, 3, -1, MC.INT32_MIN, 2]]])
    target = np.int32([[[0, 1, 2, -1, 3, 3, 3, 8]]])
    pair = MC.pair_mask(label, 2, target)
    assert pair.tolist() == [False, True, True, False, False, False, False, False]
    lists, counts = MC.members_by_part(label, 2, pair)
    assert [l.tolist() for l in lists] == [[2], [1]] and counts.tolist() == [1, 1]
    off = np.zeros((1, 1, 8, 3))
    off[0, 0, 1, 2], off[0, 0, 2, 0] = np.nan, np.inf
    assert not MC.pair_mask(label, 2, target, offset=off).any()
    assert MC.pair_mask(label, 2, target, keep=np.uint8([[[1, 0, 9, 1, 1, 1, 1, 1]]])).tolist() == [False, False, True, False, False, False, False, False]


# ---- the restatement: Horn against SVD ----------------------------------------------------------------------------------------------
def test_horn_against_svd_kabsch():
    rng = np.random.default_rng(11)
    for trial in range(40):
        m = int(rng.integers(4, 60))
        a = rng.normal(size=(m, 3)) * 5
        R = MC.rotation(rng.normal(size=3), rng.uniform(0, math.pi * 0.99))
        b = a @ R.T + rng.normal(size=3) + rng.normal(size=(m, 3)) * (0.0 if trial % 2 else 0.05)
        pm, cm, Rk = MC.kabsch(a, b)
        Rh = MC.horn((a - pm).T @ (b - cm))
        assert np.abs(Rh - Rk).max() < 1e-9 and np.abs(Rh @ Rh.T - np.eye(3)).max() < 1e-13 and np.linalg.det(Rh) > 0.999
        if trial % 2:
            assert np.abs(Rh - R).max() < 1e-12
    assert np.array_equal(MC.horn(np.zeros((3, 3))), np.eye(3))             # coincident points: nothing to rotate, the identity by construction
    line = np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])                         # collinear: undetermined about the axis, but deterministic and a rotation
    Rl = MC.horn(line)
    assert np.array_equal(Rl, MC.horn(line)) and np.abs(Rl @ Rl.T - np.eye(3)).max() < 1e-13


# ---- the restatement: the whole loop --------------------------------------------------------------------------------------------------
def agree(ref, loop, what):
    for k in ("pairs", "inliers", "status", "fits", "inlier"):
        assert np.array_equal(ref[k], loop[k]), (what, k)
    assert ref["members"] == loop["members"]
    for k in ("pose", "residual2", "rmse"):
        assert np.array_equal(np.isnan(ref[k]), np.isnan(loop[k])), (what, k)
        assert np.nanmax(np.abs(ref[k] - loop[k]), initial=0.0) <= 1e-9, (what, k, np.nanmax(np.abs(ref[k] - loop[k])))


@pytest.mark.parametrize("seed", MC.PLANTED_SEEDS)
def test_planted_cases_come_out_as_planted(seed):
    cs = MC.planted(seed)
    for ref_k in (cs["ref"], None):
        ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=ref_k, fits=3, tau2=1.0, min_pairs=8)
        assert (ref["status"] == MC.OK).all() and (ref["fits"] == 3).all()
        assert np.array_equal(ref["inlier"].reshape(cs["truth"].shape).astype(bool), cs["truth"])
        assert 40 <= ref["pairs"].min() and ref["pairs"].max() <= 400 and ref["members"] == ref["pairs"].sum() == (cs["label"] > 0).sum()
        assert np.array_equal(ref["inliers"], np.bincount(cs["label"][cs["truth"]], minlength=cs["K"] + 1)[1:])
        R = ref["pose"][:, :9].reshape(-1, 3, 3)
        assert np.abs(R - cs["R"]).max() < 1e-12
        moved = np.einsum("kij,kj->ki", R, cs["src"] - ref["pose"][:, 9:12]) + ref["pose"][:, 12:15]        # the planted centroid under the pose found
        assert np.abs(moved - cs["dst"]).max() < 1e-11 and np.nanmax(ref["rmse"]) < 1e-12
        agree(ref, MC.motion_loop(cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=ref_k, fits=3, tau2=1.0, min_pairs=8), (seed, ref_k is None))
    one = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=cs["ref"], fits=1, tau2=1.0, min_pairs=8)
    assert (one["fits"] == 1).all() and np.abs(one["pose"][:, :9].reshape(-1, 3, 3) - cs["R"]).max() > 1e-6     # fit 0 alone is pulled by the outliers
    coarse = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=None, ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)       # the rounded targets alone
    agree(coarse, MC.motion_loop(cs["label"], cs["K"], cs["target"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8), (seed, "no offset"))


def test_statuses_and_the_interleaved_case():
    cs = MC.status_case()
    ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8)
    assert ref["pairs"].tolist() == [2, 12, 0, 30, 0] and ref["members"] == 44
    assert ref["status"].tolist() == [MC.TOO_FEW, MC.THINNED, MC.TOO_FEW, MC.OK, MC.TOO_FEW] and ref["fits"].tolist() == [0, 1, 0, 3, 0]
    assert np.isnan(ref["pose"][[0, 2, 4]]).all() and np.isfinite(ref["pose"][[1, 3]]).all()
    first = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=1, tau2=1.0, min_pairs=8)
    assert first["status"][1] == MC.OK and first["pose"][1].tobytes() == ref["pose"][1].tobytes()          # thinned: the pose of fit 0 stays
    assert ref["inliers"][1] < 8 and ref["sums"][1, 0] == ref["inliers"][1] and first["sums"][1, 0] == 12
    assert ref["inliers"][3] == 30 and ref["rmse"][3] < 1e-12 and np.abs(ref["pose"][3, 12:15] - ref["pose"][3, 9:12] - [1, -1, 2]).max() < 1e-12
    assert np.isnan(ref["residual2"][(cs["label"] == 1).reshape(-1)]).all() and np.isnan(ref["rmse"][[0, 2, 4]]).all()
    agree(ref, MC.motion_loop(cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8), "statuses")
    none = MC.motion_ref(cs["label"], cs["K"], cs["target"], keep=np.zeros(cs["label"].shape, np.uint8), fits=3, tau2=1.0, min_pairs=8)
    assert none["members"] == 0 and (none["status"] == MC.TOO_FEW).all() and not none["sums"].any()
    over = MC.motion_ref(cs["label"], cs["K"], cs["target"], capacity=43)
    assert over["members"] == 44 and over["pairs"].tolist() == [2, 12, 0, 30, 0] and over["pose"] is None
    iv = MC.interleaved_case()
    seen = set()
    for fits, tau2, mp in ((3, 2.0, 8), (2, 0.5, 8)):                        # (8 scattered pairs are never collinear: the two formulations must agree)
        ref = MC.motion_ref(iv["label"], iv["K"], iv["target"], keep=iv["keep"], offset=iv["offset"], fits=fits, tau2=tau2, min_pairs=mp)
        seen |= set(ref["status"].tolist())
        agree(ref, MC.motion_loop(iv["label"], iv["K"], iv["target"], keep=iv["keep"], offset=iv["offset"], fits=fits, tau2=tau2, min_pairs=mp), ("interleaved", fits))
    assert seen == {MC.OK, MC.THINNED, MC.TOO_FEW}, "every status occurs"


# ---- PartMotions on host tensors ------------------------------------------------------------------------------------------------------
def test_part_motions_arithmetic_on_host_tensors():
    import torch
    from d3fields_amd import PartMotions
    cs = MC.planted(1)
    ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    t = lambda a: torch.from_numpy(np.array(a))
    origin, step, shape = (0.5, -0.25, 1.0), 0.02, cs["label"].shape
    pose = ref["pose"].copy()
    pose[2] = np.nan
    status = ref["status"].copy()
    status[2] = MC.TOO_FEW
    pm = PartMotions(origin, step, t(pose), t(ref["pairs"]), t(ref["inliers"]), t(ref["fits"]), t(ref["rmse"]), t(status), t(ref["residual2"].reshape(shape)),
                     t(ref["inlier"].reshape(shape).astype(bool)))
    rot, trans, angle, shift = MC.load_world(pose, origin, step)
    assert pm.count == cs["K"] and tuple(pm.grid_shape) == shape and pm.rot.dtype == pm.trans.dtype == pm.angle.dtype == torch.float64
    for got, want in ((pm.rot, rot), (pm.shift, shift)):
        assert np.array_equal(got.numpy(), want, equal_nan=True)
    # (a matrix product and an arc tangent: torch and NumPy may round the last bit differently; the values are of order 1)
    assert np.allclose(pm.trans.numpy(), trans, rtol=0, atol=1e-14, equal_nan=True) and np.allclose(pm.angle.numpy(), angle, rtol=0, atol=1e-14, equal_nan=True)
    assert np.array_equal(pm.rmse.numpy(), ref["rmse"] * step, equal_nan=True)
    assert np.allclose(pm.residual.numpy(), np.sqrt(ref["residual2"].reshape(shape)) * step, rtol=1e-14, atol=0, equal_nan=True)
    o = np.array(origin)
    keep = [k for k in range(cs["K"]) if k != 2]
    # the planted motion in world coordinates: x' = R (x - c) + c + s with c = origin + step src, s = step (dst - src)
    planted_angle = np.arccos(np.clip((np.trace(cs["R"], axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert np.abs(pm.angle.numpy()[keep] - planted_angle[keep]).max() < 1e-9
    for k in keep:
        x = o + step * np.argwhere(cs["label"] == k + 1).astype(np.float64)
        c, s = o + step * cs["src"][k], step * (cs["dst"][k] - cs["src"][k])
        want = (x - c) @ cs["R"][k].T + c + s
        assert np.abs(pm.apply(t(x), k + 1).numpy() - want).max() < 1e-12
        ids = torch.full((len(x),), k + 1, dtype=torch.int32)
        assert torch.equal(pm.apply(t(x), ids), pm.apply(t(x), k + 1))
    x = t(o + step * np.argwhere(cs["label"] > 0).astype(np.float64))
    ids = t(cs["label"][cs["label"] > 0])
    mixed = pm.apply(x, ids).numpy()
    assert np.isnan(mixed[ids.numpy() == 3]).all() and np.isfinite(mixed[ids.numpy() != 3]).all()
    # moved: a part without a pose never moved; the bounds are "or"
    far = pm.moved(min_shift=0.0).numpy()
    assert far.tolist() == [k != 2 for k in range(cs["K"])]
    sh, an = np.linalg.norm(shift, axis=1), angle
    assert pm.moved(min_shift=float(np.nanmedian(sh))).numpy().tolist() == [bool(v) for v in (sh >= np.nanmedian(sh))]
    assert pm.moved(min_angle=float(np.nanmedian(an))).numpy().tolist() == [bool(v) for v in (an >= np.nanmedian(an))]
    assert pm.moved(min_shift=1e9, min_angle=0.0).numpy().tolist() == far.tolist()
    for bad in (lambda: pm.moved(), lambda: pm.apply(x.float(), 1), lambda: pm.apply(x, 0), lambda: pm.apply(x, cs["K"] + 1), lambda: pm.apply(x, ids[:-1]),
                lambda: pm.apply(x, 1.5)):
        with pytest.raises(ValueError):
            bad()


def test_motions_argument_errors_need_no_device():
    import torch
    from d3fields_amd import Flow
    shape = (4, 5, 6)
    target = torch.full(shape, -1, dtype=torch.int32)
    cost = torch.full(shape, float("inf"))
    f = Flow((0.0, 0.0, 0.0), 0.1, target, cost)
    lab = torch.zeros(shape, dtype=torch.int32)
    for bad in (lambda: f.motions(lab), lambda: f.motions(lab, count=-1), lambda: f.motions(lab.long(), count=1), lambda: f.motions(lab[:-1], count=1),
                lambda: f.motions("lab", count=1), lambda: f.motions(lab, count=121, refined=False), lambda: f.motions(lab, count=1),      # refine=False flow
                lambda: f.motions(lab, count=1, refined=False, tau_voxels=0.0), lambda: f.motions(lab, count=1, refined=False, tau_voxels=float("inf")),
                lambda: f.motions(lab, count=1, refined=False, tau_voxels=float("nan")), lambda: f.motions(lab, count=1, refined=False, fits=0),
                lambda: f.motions(lab, count=1, refined=False, fits=9), lambda: f.motions(lab, count=1, refined=False, fits=2.0),
                lambda: f.motions(lab, count=1, refined=False, min_pairs=2), lambda: f.motions(lab, count=1, refined=False, keep=lab),
                lambda: f.motions(lab, count=1, refined=False, keep=torch.ones(shape[:2], dtype=torch.bool))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        f.motions(lab, count=1, refined=False)                              # there is no CPU path


# ---- the kernels' resources and source ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "motion_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ["motion_level_kernelILi%dELb%dE" % (nc, l0) for nc in (16, 2) for l0 in (0, 1)] + ["motion_mask_kernel", "motion_fit_kernel", "motion_fill_kernel",
                                                                                                         "motion_finish_kernel"]:
        assert kernel in names, (kernel, out[-800:])
    for name, scratch, occ in rows:
        assert scratch == 0 and occ >= 2, (name, scratch, occ)


def test_source_names_no_fused_operation_and_no_float_atomic():
    src = open(SOURCE).read().lower()
    assert "fma" not in src and "atomic" not in "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "fma" not in open(os.path.join(ROOT, "d3fields_amd", "csrc", "d3f_horn.h")).read().lower()
