"""Rigid motion per part on the device (d3f_part_motion, csrc/motion_kernels.hip; Flow.motions, PartMotions) against the NumPy restatement of
tests/motion_cases.py: sums, poses, residuals, the inlier volume, counts, rmse, status and fits are compared byte for byte, no tolerance
anywhere; every launch runs twice on outputs (and a workspace) poisoned with 0xA5 and must give equal bytes.

What each assert is there to catch:
  a ragged chunk, a level boundary, a reduction order that differs from the contract                  test_tree
  a member list that is not in ascending flat index per part, an index out of range                     test_parts_interleaved
  a loop that does not end with the planted inliers                                                      test_planted
  a status, a pose kept or dropped at the wrong fit, a part without pairs                                test_statuses
  NaN / Inf offsets, NULL offset and ref, signed zeros                                                   test_specials
  anything written over capacity; K = 0                                                                  test_capacity
  a wiring error between Flow.motions and the kernel                                                     test_api
test_tree: the member counts 1 .. 513 sit together in one 41 x 40 x 41 volume, 65 537 in a second launch on the same volume (with parts of 1
and 257 beside it): all twelve together are 67 527 members, 287 more than the volume has voxels."""
import math

import numpy as np
import pytest
import torch

import motion_cases as MC
from d3fields_amd import BakedField, Components, PartMotions, _lib

pytestmark = pytest.mark.gpu
KEYS = ("members", "pairs", "pose", "inliers", "rmse", "status", "fits", "residual2", "inlier", "sums")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(dev, nbytes):
    return torch.full((max(nbytes, 8),), MC.POISON, dtype=torch.uint8, device=dev)


def launch(dev, label, K, target, keep=None, offset=None, ref=None, fits=3, tau2=1.0, min_pairs=8, capacity=None, volumes=True, sums=True):
    lib = _lib.load()
    nx, ny, nz = label.shape
    n = nx * ny * nz
    up = lambda a, dt: None if a is None else torch.from_numpy(np.array(a, dt)).to(dev)      # (a copy: the case arrays are read-only)
    lab, tgt, kp, off, rf = up(label, np.int32), up(target, np.int32), up(keep, np.uint8), up(offset, np.float64), up(ref, np.int32)
    cap = int(MC.pair_mask(label, K, target, keep, offset).sum()) if capacity is None else capacity
    sizes = {"members": 8, "pairs": 4 * K, "pose": 8 * MC.POSE * K, "inliers": 4 * K, "rmse": 8 * K, "status": 4 * K, "fits": 4 * K, "residual2": 8 * n, "inlier": n,
             "sums": 8 * MC.SUMS * K}
    buf = {k: poisoned(dev, b) for k, b in sizes.items()}
    ws_bytes = int(lib.d3f_part_motion_workspace_bytes(nx, ny, nz, K, cap))
    assert ws_bytes > 0
    ws = poisoned(dev, ws_bytes)
    opt = lambda k, on: _lib.ptr(buf[k]) if on else None
    _lib.check(lib.d3f_part_motion(_lib.ptr(lab), K, nx, ny, nz, _lib.ptr(kp), _lib.ptr(tgt), _lib.ptr(off), _lib.ptr(rf), fits, float(tau2), min_pairs, cap,
                                   _lib.ptr(buf["members"]), _lib.ptr(buf["pairs"]), _lib.ptr(buf["pose"]), _lib.ptr(buf["inliers"]), _lib.ptr(buf["rmse"]),
                                   _lib.ptr(buf["status"]), _lib.ptr(buf["fits"]), opt("residual2", volumes), opt("inlier", volumes), opt("sums", sums),
                                   _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return {k: buf[k].cpu().numpy()[:sizes[k]] for k in KEYS}


def run_motion(dev, *args, **kw):
    """two launches on poisoned outputs, which must agree byte for byte -> the raw bytes of every output"""
    got, again = launch(dev, *args, **kw), launch(dev, *args, **kw)
    for k in KEYS:
        assert got[k].tobytes() == again[k].tobytes(), (k, "two runs differ")
    return got


DTYPES = {"members": np.int64, "pairs": np.int32, "pose": np.float64, "inliers": np.int32, "rmse": np.float64, "status": np.int32, "fits": np.int32,
          "residual2": np.float64, "inlier": np.uint8, "sums": np.float64}


def same(got, ref, what, skip=()):
    """byte equality of every output with the restatement; an output the restatement leaves None must still hold the poison"""
    for k in KEYS:
        if k in skip:
            continue
        if ref[k] is None:
            assert (got[k] == MC.POISON).all(), (what, k, "written over capacity")
            continue
        want = np.ascontiguousarray(np.asarray(ref[k], DTYPES[k]).reshape(-1))
        have = got[k].view(DTYPES[k])
        assert have.shape == want.shape, (what, k, have.shape, want.shape)
        if have.tobytes() != want.tobytes():
            word = np.uint8 if DTYPES[k] == np.uint8 else np.uint32 if want.itemsize == 4 else np.uint64
            bad = np.flatnonzero(have.view(word) != want.view(word))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), have[bad[:4]].tolist(), want[bad[:4]].tolist()))


@pytest.mark.parametrize("counts", [MC.TREE_SMALL, MC.TREE_LARGE], ids=["1..513", "65537"])
def test_tree(dev, counts):
    cs = MC.tree_case(counts, 5)
    assert np.array_equal(np.bincount(cs["label"].reshape(-1), minlength=len(counts) + 1)[1:], counts)
    for fits, mp in ((3, 3), (1, 8)):
        ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=cs["offset"], fits=fits, tau2=MC.TREE_TAU2, min_pairs=mp)
        assert ref["pairs"].tolist() == list(counts)
        if fits == 3:                                                # the later fits fold chunks in which inliers and +0.0 rows mix
            big = np.argmax(counts)
            assert ref["status"][big] == MC.OK and 0.1 * counts[big] < ref["inliers"][big] < 0.9 * counts[big]
        same(run_motion(dev, cs["label"], cs["K"], cs["target"], offset=cs["offset"], fits=fits, tau2=MC.TREE_TAU2, min_pairs=mp), ref, (counts, fits))


def test_parts_interleaved(dev):
    cs = MC.interleaved_case()
    lab = cs["label"].reshape(-1)
    for k in (3, 4):                                                 # the 40-voxel parts: not contiguous in flat order
        assert np.diff(np.flatnonzero(lab == k)).max() > 1
    assert {0, -1, cs["K"] + 1, MC.INT32_MIN} <= set(lab.tolist()) and {-1, lab.size, MC.INT32_MAX} <= set(cs["target"].reshape(-1).tolist())
    for kw in ({"fits": 3, "tau2": 2.0, "min_pairs": 3}, {"fits": 2, "tau2": 0.5, "min_pairs": 8}):
        ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], keep=cs["keep"], offset=cs["offset"], **kw)
        same(run_motion(dev, cs["label"], cs["K"], cs["target"], keep=cs["keep"], offset=cs["offset"], **kw), ref, kw)
    ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=2, tau2=1.0, min_pairs=4)          # no keep, no offset
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=2, tau2=1.0, min_pairs=4), ref, "bare")


@pytest.mark.parametrize("seed", MC.PLANTED_SEEDS)
def test_planted(dev, seed):
    cs = MC.planted(seed)
    ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    got = run_motion(dev, cs["label"], cs["K"], cs["target"], offset=cs["offset"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    same(got, ref, seed)
    assert np.array_equal(got["inlier"].reshape(cs["truth"].shape).astype(bool), cs["truth"])
    assert (got["status"].view(np.int32) == MC.OK).all() and (got["fits"].view(np.int32) == 3).all()


def test_statuses(dev):
    cs = MC.status_case()
    ref = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8)
    assert ref["status"].tolist() == [MC.TOO_FEW, MC.THINNED, MC.TOO_FEW, MC.OK, MC.TOO_FEW] and ref["fits"].tolist() == [0, 1, 0, 3, 0]
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8), ref, "statuses")
    one = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=1, tau2=1.0, min_pairs=8)
    assert one["status"].tolist() == [MC.TOO_FEW, MC.OK, MC.TOO_FEW, MC.OK, MC.TOO_FEW]
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=1, tau2=1.0, min_pairs=8), one, "fits = 1")
    nothing = np.zeros(cs["label"].shape, np.uint8)
    none = MC.motion_ref(cs["label"], cs["K"], cs["target"], keep=nothing, fits=3, tau2=1.0, min_pairs=8)
    assert none["members"] == 0
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], keep=nothing, fits=3, tau2=1.0, min_pairs=8), none, "keep all zero")
    # without the optional outputs the others are the same
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, volumes=False, sums=False), ref, "no optional outputs",
         skip=("residual2", "inlier", "sums"))


def test_specials(dev):
    cs = MC.planted(2)
    label, K, target = cs["label"], cs["K"], cs["target"]
    off = cs["offset"].copy()
    part1 = np.argwhere(label == 1)
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        off[tuple(part1[i])][i] = bad
    ref = MC.motion_ref(label, K, target, offset=off, ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    clean = MC.motion_ref(label, K, target, offset=cs["offset"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    assert ref["pairs"][0] == clean["pairs"][0] - 3 and ref["members"] == clean["members"] - 3
    got = run_motion(dev, label, K, target, offset=off, ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    same(got, ref, "non-finite offsets")
    assert np.isnan(got["residual2"].view(np.float64).reshape(label.shape)[tuple(part1[:3].T)]).all()
    # offset = NULL is an offset of zeros
    zeros = run_motion(dev, label, K, target, offset=np.zeros(label.shape + (3,)), ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    null = run_motion(dev, label, K, target, ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    same(null, MC.motion_ref(label, K, target, ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8), "offset NULL")
    for k in KEYS:
        assert null[k].tobytes() == zeros[k].tobytes(), k
    # ref = NULL: other sums, the same inlier set
    bare = run_motion(dev, label, K, target, offset=cs["offset"], fits=3, tau2=1.0, min_pairs=8)
    same(bare, MC.motion_ref(label, K, target, offset=cs["offset"], fits=3, tau2=1.0, min_pairs=8), "ref NULL")
    with_ref = run_motion(dev, label, K, target, offset=cs["offset"], ref=cs["ref"], fits=3, tau2=1.0, min_pairs=8)
    assert bare["inlier"].tobytes() == with_ref["inlier"].tobytes() and bare["sums"].tobytes() != with_ref["sums"].tobytes()
    # -0.0 products: a part in the plane x = 0 (a0 = 0) whose matches have negative coordinates b: 0 * b = -0.0, and the fold starts from +0.0
    shape = (3, 6, 6)
    lab = np.zeros(shape, np.int32)
    lab[0, 1:5, 1:5] = 1
    tgt = np.where(lab > 0, np.arange(lab.size).reshape(shape), -1).astype(np.int32)
    neg = np.full(shape + (3,), -0.25)
    neg[0, :, :, 1:] = -6.5
    ref = MC.motion_ref(lab, 1, tgt, offset=neg, fits=2, tau2=1.0, min_pairs=3)
    zero = ref["sums"][0] == 0
    assert ref["pairs"][0] == 16 and zero[7:10].all() and not np.signbit(ref["sums"][0][zero]).any() and (ref["sums"][0, 4:7] < 0).all()
    assert np.signbit(MC.moment_rows(*MC.points(np.flatnonzero(lab.reshape(-1)), shape, tgt, neg, None))[:, 7:10]).all()      # the rows do hold -0.0
    same(run_motion(dev, lab, 1, tgt, offset=neg, fits=2, tau2=1.0, min_pairs=3), ref, "-0.0")


def test_capacity(dev):
    cs = MC.status_case()
    full = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8)
    members = int(full["members"])
    over = MC.motion_ref(cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=members - 1)
    assert over["pose"] is None and over["members"] == members
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=members - 1), over, "one below")
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=0), over, "capacity 0")
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=members), full, "exactly enough")
    same(run_motion(dev, cs["label"], cs["K"], cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=10 ** 12), full, "more than the volume")
    # K = 0: only out_members = 0 is written
    got = run_motion(dev, cs["label"], 0, cs["target"], fits=3, tau2=1.0, min_pairs=8, capacity=5)
    assert got["members"].view(np.int64)[0] == 0
    for k in ("residual2", "inlier"):
        assert (got[k] == MC.POISON).all(), k


def test_api(dev):
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    shape, origin, step, C = (12, 12, 12), (0.5, -0.25, 1.0), 0.02, 6
    rng = np.random.default_rng(9)
    blob_a = np.zeros(shape, bool)
    blob_a[1:5, 1:5, 1:5] = True                                     # stays
    blob_b = np.zeros(shape, bool)
    blob_b[6:10, 6:10, 5:9] = True                                   # moves by (1, 0, -1)
    # rows that are linear in the position (small integers: exact in float32): the cost around a match is the same on both sides of every
    # axis, so the sub-voxel offset is exactly 0 and the recovered shift is the planted one
    W = rng.integers(-3, 4, size=(C, 3))
    assert np.linalg.matrix_rank(W) == 3
    rows = (np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1) @ W.T).astype(np.float32)
    ma = blob_a | blob_b
    mb = blob_a | np.roll(blob_b, (1, 0, -1), axis=(0, 1, 2))
    rows_b = np.where(blob_a[..., None], rows, np.roll(rows, (1, 0, -1), axis=(0, 1, 2)))
    dist = lambda m: np.where(m, -0.001, 1.0).astype(np.float32)
    A = BakedField.from_arrays(origin, step, t(dist(ma)), feat=t(rows))
    B = BakedField.from_arrays(origin, step, t(dist(mb)), feat=t(rows_b))

    def chain(fa, fb):
        parts = fa.parts("feat", tau=math.inf, connectivity=6)
        fwd, back = fa.flow(fb, "feat", radius_voxels=2), fb.flow(fa, "feat", radius_voxels=2)
        ok = fwd.consistent(back, tol_voxels=0)
        return parts, fwd, ok, fwd.motions(parts, keep=ok, min_pairs=8)

    parts, fwd, ok, pm = chain(A, B)
    assert isinstance(parts, Components) and parts.count == 2 and isinstance(pm, PartMotions) and pm.count == 2
    ref = MC.motion_ref(parts.labels.cpu().numpy(), 2, fwd.target.cpu().numpy(), keep=ok.cpu().numpy(), offset=fwd.offset.cpu().numpy(),
                        ref=parts.box_lo.cpu().numpy(), fits=3, tau2=1.0, min_pairs=8)
    assert ref["pairs"].tolist() == [64, 64] and ref["status"].tolist() == [MC.OK, MC.OK]
    for key, have in (("pose", pm.pose), ("pairs", pm.pairs), ("inliers", pm.inliers), ("fits", pm.fits), ("status", pm.status)):
        assert have.cpu().numpy().tobytes() == np.asarray(ref[key], DTYPES[key]).tobytes(), key
    assert pm.inlier.dtype == torch.bool and np.array_equal(pm.inlier.cpu().numpy(), ref["inlier"].reshape(shape).astype(bool))
    # the world quantities: the restatement pushed through the same torch formulas
    want = PartMotions(origin, step, t(ref["pose"]), t(ref["pairs"]), t(ref["inliers"]), t(ref["fits"]), t(ref["rmse"]), t(ref["status"]),
                       t(ref["residual2"].reshape(shape)), t(ref["inlier"].reshape(shape).astype(bool)))
    for name in ("rot", "trans", "shift", "angle", "rmse", "residual"):
        a, b = getattr(pm, name), getattr(want, name)
        assert a.dtype == torch.float64 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
    moved = int(parts.labels[7, 7, 6]) - 1
    assert np.abs(pm.shift[moved].cpu().numpy() - np.array([1, 0, -1]) * step).max() < 1e-9 and np.abs(pm.shift[1 - moved].cpu().numpy()).max() < 1e-9
    assert pm.moved(min_shift=0.5 * step).cpu().numpy().tolist() == [k == moved for k in range(2)]
    x = t(np.array(origin) + step * np.argwhere(blob_b).astype(np.float64))
    assert np.abs((pm.apply(x, moved + 1) - x).cpu().numpy() - np.array([1, 0, -1]) * step).max() < 1e-9
    # a label volume with count= gives the same poses (the moments are then taken about voxel (0, 0, 0): other sums, so not the same bytes)
    by_volume = fwd.motions(parts.labels, keep=ok, count=2)
    assert torch.equal(by_volume.inlier, pm.inlier) and torch.equal(by_volume.status, pm.status)
    assert float((by_volume.rot - pm.rot).abs().max()) < 1e-12 and float((by_volume.trans - pm.trans).abs().max()) < 1e-12
    # the same call on banded bakes gives the same bytes
    _, _, _, pm_band = chain(A.to_band(0.5 * step), B.to_band(0.5 * step))
    for name in ("pose", "pairs", "inliers", "fits", "status", "rmse", "residual", "inlier", "rot", "trans"):
        assert getattr(pm_band, name).cpu().numpy().tobytes() == getattr(pm, name).cpu().numpy().tobytes(), name
    # unrefined, and the argument errors that need the device
    coarse = fwd.motions(parts, keep=ok, refined=False)
    assert torch.equal(coarse.status, pm.status)
    other = BakedField.from_arrays((0.0, 0.0, 0.0), step, t(dist(ma)), feat=t(rows)).components(connectivity=6)
    for bad in (lambda: fwd.motions(other), lambda: fwd.motions(parts, count=2), lambda: fwd.motions(parts.labels.cpu(), count=2),
                lambda: fwd.motions(parts, keep=ok.cpu())):
        with pytest.raises(ValueError):
            bad()
