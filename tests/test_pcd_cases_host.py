"""CPU: every case of tests/pcd_cases.py has the property it is named for, and the expected results (oracle/np_pcd.py) alone meet every
condition tests/test_gpu_pcd_edges.py puts on the kernels -- so a pass on the device means the kernel met the edge, not that the case
missed it."""
import numpy as np
import pytest

import pcd_cases as PC
from oracle import np_pcd


# ---- nearest neighbour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.tie_cases(), ids=lambda c: c["name"])
def test_near_ties_are_near_ties(case):
    """on every property row: d2[later] < d2[earlier] in float64, the two roots are equal, and np.argmin returns the earlier row"""
    a, b, rows, earlier, later = case["a"], case["b"], case["rows"], case["earlier"], case["later"]
    d2 = PC.d2_of(a[rows], b)
    r = np.arange(len(rows))
    ok = (d2[r, later] < d2[r, earlier]) & (np.sqrt(d2[r, later]) == np.sqrt(d2[r, earlier])) & (earlier < later) & (case["argmin"][rows] == earlier)
    print("%s: %d of %d query rows see a later row with the smaller square and the same root" % (case["name"], int(ok.sum()), len(a)))
    assert ok.all() and ok.sum() >= 8
    # the rule the kernel had (first minimum of the SQUARES) answers these rows differently, so the case can tell the two apart
    assert np.array_equal(d2.argmin(axis=1), later)
    assert np.array_equal(case["min_dist"][rows], np.sqrt(d2[r, earlier]))
    # the expected result is np_pcd.nearest's, for every chunking
    md, am = np_pcd.nearest(a, b, chunk=5)
    assert PC.same_bits(md, case["min_dist"]) and np.array_equal(am, case["argmin"])


def test_tie_positions():
    K = PC.KBLOCK
    e, l = PC.TIE_POSITIONS["same tile"]
    assert e // K == l // K
    assert PC.TIE_POSITIONS["tile boundary"] == (K - 1, K) == (255, 256)
    assert PC.TIE_POSITIONS["different tiles"] == (3, 700) and PC.TIE_NB > 700 and PC.TIE_NB % K == 1
    c = PC.cluster_case()
    x = np.sort(c["b"][np.isin(c["b"][:, 1], PC.ANCHOR[1]), 0])
    assert x.size == PC.CLUSTER and np.array_equal(np.diff(x), np.full(PC.CLUSTER - 1, np.spacing(PC.ANCHOR[0])))      # consecutive doubles
    assert len(set(c["earlier"] // K) | set(c["later"] // K)) == 2                  # the ties lie on both sides of the tile boundary


def test_duplicate_rows_first_wins():
    c = PC.duplicate_case()
    b = c["b"]
    assert np.array_equal(b[5], b[300]) and np.array_equal(b[5], b[511]) and np.array_equal(b[17], b[18])
    for first, rows in c["first"].items():
        assert np.all(c["argmin"][rows] == first)
    assert c["min_dist"][80] == 0.0 and c["min_dist"][81] == 0.0


def test_sized_cases():
    assert PC.NEAREST_NB == (1, 255, 256, 257, 513) and PC.NEAREST_NA == (1, 255, 257)
    ties = 0
    for na in PC.NEAREST_NA:
        for nb in PC.NEAREST_NB:
            c = PC.sized_case(na, nb)
            assert c["a"].shape == (na, 3) and c["b"].shape == (nb, 3) and c["argmin"].shape == (na,)
            d = np.sqrt(PC.d2_of(c["a"], c["b"]))
            ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties >= 100                          # the lattice half makes exact ties common: "first" is exercised, not only "minimum"


def test_nan_and_overflow_cases():
    c = PC.nan_b_case()
    assert np.isnan(c["b"][PC.NAN_ROWS[0]]).sum() == 1 and np.isnan(c["b"][PC.NAN_ROWS[1]]).all() and np.isnan(c["b"]).any(axis=1).sum() == 2
    assert np.isnan(c["min_dist"]).all() and np.all(c["argmin"] == PC.NAN_ROWS[0]) and len(c["a"]) > PC.KBLOCK
    c = PC.nan_query_case()
    nanq = np.zeros(len(c["a"]), bool)
    nanq[list(PC.NAN_QUERIES)] = True
    assert np.array_equal(np.isnan(c["a"]).any(axis=1), nanq) and not np.isnan(c["b"]).any()
    assert np.array_equal(np.isnan(c["min_dist"]), nanq) and np.all(c["argmin"][nanq] == 0) and np.any(c["argmin"][~nanq] != 0)
    c = PC.overflow_case()
    assert np.isfinite(c["a"]).all() and np.isfinite(c["b"]).all() and np.isinf(PC.d2_of(c["a"], c["b"])).all()
    assert np.all(c["min_dist"] == np.inf) and np.all(c["argmin"] == 0)


def test_same_bits():
    z = np.array([0.0, np.nan, 1.0])
    assert PC.same_bits(z, z.copy()) and PC.same_bits(z, np.array([0.0, -np.nan, 1.0]))
    assert not PC.same_bits(z, np.array([-0.0, np.nan, 1.0])) and not PC.same_bits(z, np.array([0.0, 2.0, 1.0]))
    assert not PC.same_bits(z, np.array([0.0, np.nan, np.nextafter(1.0, 2.0)])) and not PC.same_bits(z, z[:2])


# ---- back-projection ---------------------------------------------------------------------------------------------------------------
def test_view_cases_cover_their_edges():
    cases = PC.view_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert all(W % 64 for _, W in PC.SHAPES) and {H * W for H, W in PC.SHAPES} >= {1, 255, 256, 257, 259, 513}
    for c in cases:
        H, W = c["depth"].shape
        n = len(c["pix"])
        assert c["pts"].shape == (n, 3) and np.all(np.diff(c["pix"]) > 0) and (n == 0 or (0 <= c["pix"][0] and c["pix"][-1] < H * W))
        if "which" in c:
            if c["which"] == "none":
                assert n == 0
            elif c["which"] == "all":
                assert n == H * W
            else:
                assert n == H * W - c["last"] >= 1 and c["pix"][0] == c["last"] and c["last"] % PC.KBLOCK == 0 and H * W - c["last"] <= PC.KBLOCK
    for c in cases:
        if c["name"].startswith("random"):      # every random case keeps some pixels and drops some, for each of its reasons
            assert 0 < len(c["pix"]) < c["depth"].size or c["depth"].size == 1, c["name"]
            if c["bounds"] is not None and c["depth"].size > 1:
                assert len(c["pix"]) < len(PC.uncropped_points(c)[1]), c["name"]
    assert {tuple(np.unique(c["mask"])) for c in cases if c["name"].startswith("random") and c["mask"] is not None and c["mask"].size > 4} == {PC.MASK_BYTES}


def test_special_depths_gate_differently_with_and_without_a_mask():
    plain, masked = PC.special_depth_case(False), PC.special_depth_case(True)
    depth = plain["depth"].reshape(-1)
    assert np.array_equal(depth, masked["depth"].reshape(-1), equal_nan=True)
    for v in PC.SPECIAL_DEPTHS:
        assert np.any((depth == v) | (np.isnan(depth) & np.isnan(v)))
    assert {0.0, 1.5, -0.25, np.inf} <= set(PC.SPECIAL_DEPTHS) and any(np.isnan(v) for v in PC.SPECIAL_DEPTHS)
    kept = set(depth[plain["pix"]].tolist())
    assert kept == {np.nextafter(1.5, 0.0), 5e-324, 0.75}                           # 0 < d < 1.5, both strict
    byte = masked["mask"].reshape(-1)
    assert set(byte.tolist()) == set(PC.MASK_BYTES)
    assert np.array_equal(masked["pix"], np.flatnonzero((byte != 0) & (depth > 0)))
    kept_m = set(depth[masked["pix"]].tolist())
    assert kept_m == kept | {1.5, np.nextafter(1.5, 2.0), 3.0, np.inf}              # byte != 0 and d > 0: no upper gate
    for v in kept_m:                            # every kept depth is kept under each of the bytes 1, 2 and 255
        assert set(byte[masked["pix"]][depth[masked["pix"]] == v].tolist()) == {1, 2, 255}
    assert np.isinf(masked["pts"]).any() or np.isnan(masked["pts"]).any()           # an infinite depth passes the mask gate uncropped


@pytest.mark.parametrize("masked", [False, True])
def test_points_land_exactly_on_the_crop_bounds(masked):
    c = PC.on_bound_case(masked)
    pts, pix = PC.uncropped_points(c)
    lo, hi = np.array(c["bounds"][0::2]), np.array(c["bounds"][1::2])
    on = (pts == lo) | (pts == hi)
    faces = [(pts[:, k] == lo[k]).any() for k in range(3)] + [(pts[:, k] == hi[k]).any() for k in range(3)]
    want = [True, True, True, True, True, masked]                                  # without a mask, depth 2 never passes the gate
    assert faces == want, faces
    inside = np.all((pts > lo) & (pts < hi), axis=1)
    assert on.any(axis=1).sum() >= 20 and not (on.any(axis=1) & inside).any()
    assert np.array_equal(c["pix"], pix[inside]) and 0 < len(c["pix"]) < len(pix)
    # a kernel with <= or >= on one face keeps another set
    for k in range(3):
        for face in ((pts[:, k] == lo[k]), (pts[:, k] == hi[k])):
            others = np.all(((pts > lo) & (pts < hi)) | (np.arange(3) == k), axis=1)
            assert (face & others).any() or (k == 2 and not masked and not face.any()), (k, masked)


# ---- voxel-grid mean ---------------------------------------------------------------------------------------------------------------
def _per_voxel(points, voxel_size):
    _, counts = np.unique(PC.voxel_index(points, voxel_size), axis=0, return_counts=True)
    return counts


def test_voxel_cases():
    assert PC.VOXEL_SIZES == (1e-4, 0.01, 0.25, 10.0) and PC.VOX_FIX == 2.0 ** -40
    for c in PC.tolerance_voxel_cases():
        counts = _per_voxel(c["points"], c["voxel_size"])
        assert counts.max() <= PC.MAX_PER_VOXEL, (c["name"], int(counts.max()))   # point_tol's bound on the reference's sums holds
        assert c["want_points"].shape == (len(counts), 3), c["name"]
        if c["colours"] is not None:
            assert c["want_colours"].shape == (len(counts), 3)
        assert PC.point_tol(c["points"], c["voxel_size"]) < 1e-3 * c["voxel_size"], c["name"]      # the tolerance cannot hide a wrong voxel
    for v in PC.VOXEL_SIZES:
        c = PC.cloud_case(v)
        counts = _per_voxel(c["points"], v)
        assert len(counts) > 2 * PC.KBLOCK and counts.max() >= 3 and np.abs(c["points"]).min() > 1000 * v
    assert np.abs(PC.cloud_case(0.01, "negative")["colours"]).max() > 1 and PC.cloud_case(0.01, "negative")["colours"].min() < -1
    byt = PC.cloud_case(0.01, "bytes")["colours"]
    assert byt.max() == 255 and byt.min() == 0 and np.array_equal(byt, np.round(byt))


def test_voxel_face_case_is_exact_and_on_faces():
    c = PC.face_case()
    pts, vs = c["points"], c["voxel_size"]
    assert vs == 0.25 and np.array_equal(pts, np.round(pts * 8) / 8) and pts.min() < 0 < pts.max()
    ref = (pts - (pts.min(axis=0) - vs * 0.5)) / vs
    on_face = ref == np.floor(ref)
    assert 0.3 < on_face.mean() < 0.7 and (on_face & (pts < 0)).any()
    # a point on a face belongs to the voxel above it: moving it down by an ulp changes its voxel
    assert np.array_equal(np.floor(ref)[on_face], np.floor(np.nextafter(ref, -np.inf))[on_face] + 1)


def test_identical_points_case_is_exact():
    c = PC.identical_case()
    assert c["points"].shape == (PC.IDENTICAL, 3) == (4097, 3)
    assert c["want_points"].shape == (1, 3) and PC.same_bits(c["want_points"][0], c["points"][0]) and PC.same_bits(c["want_colours"][0], c["colours"][0])
    one = PC.one_point_case()
    assert PC.same_bits(one["want_points"], one["points"]) and PC.same_bits(one["want_colours"], one["colours"])


def test_voxel_count_and_extent_cases():
    assert PC.VOXEL_COUNTS[:3] == (255, 256, 257) and 19000 < PC.VOXEL_COUNTS[3] < 21000
    for v in PC.VOXEL_COUNTS:
        c = PC.count_case(v)
        assert len(c["want_points"]) == v and len(c["points"]) > 1.5 * v
    big = PC.count_case(PC.VOXEL_COUNTS[3])
    assert 20000 < len(big["points"]) < 60000
    assert max(len(c["points"]) for c in PC.tolerance_voxel_cases() if c is not big) <= 4000
    for axis in (0, 2):
        c = PC.extent_case(axis)
        idx = PC.voxel_index(c["points"], c["voxel_size"])
        assert (idx[1] - idx[0]).tolist() == [PC.AXIS_EXTENT if k == axis else 0 for k in range(3)]
        assert idx.max() == PC.AXIS_EXTENT == 2 ** 21 - 2 and len(c["want_points"]) == 2


# ---- voxel-index sets --------------------------------------------------------------------------------------------------------------
def test_iou_cases():
    cases = {c["name"]: c for c in PC.iou_cases()}
    for c in cases.values():
        a, b = c["a"], c["b"]
        assert a.dtype == np.int32 and b.dtype == np.int32
        assert len(set(a.tolist()) | set(b.tolist())) == c["distinct"], c["name"]
        assert c["want"] == np_pcd.vox_idx_iou(a, b)
    assert {PC.INT32_MIN, -1, 0, PC.INT32_MAX} <= set(cases["extreme keys"]["a"].tolist()) & set(cases["extreme keys"]["b"].tolist())
    assert len(cases["first empty"]["a"]) == 0 and len(cases["second empty"]["b"]) == 0
    assert cases["one repeated key"]["want"][0] == 1.0 and cases["two repeated keys"]["want"][0] == 0.0
    for total in (512, 513):
        c = cases["%d distinct keys, disjoint" % total]
        assert len(c["a"]) + len(c["b"]) == total == c["length"] and c["want"][0] == 0.0
        c = cases["%d distinct keys, overlapping" % total]
        assert c["want"][0] == 256 / total
    run = cases["dense run"]
    keys = np.union1d(run["a"], run["b"])
    assert np.array_equal(np.diff(keys), np.ones(2999, np.int32)) and keys[0] < 0 < keys[-1] and run["want"] == (1000 / 3000, 2000 / 3000, 2000 / 3000)
