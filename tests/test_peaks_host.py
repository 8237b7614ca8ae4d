"""CPU: d3f_volume_peaks is declared by the header, bound and exported with D3F_ABI_VERSION still 16; it validates its arguments on the host
with the documented status codes before any HIP call; the restatement of tests/peaks_cases.py (plain loops over the clipped box) equals
scipy's minimum filter on tie-free data and a second formulation through packed (ordered float, index) uint64 keys and three 1-D minima on
every case, the tie-heavy ones included; its peaks are separated, a constant volume has one, signed zeros, NaN and the infinities follow the
definition, the threshold suppresses nothing; the case set holds what the device tests rely on; peaks_kernel uses no scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import peaks_cases as PC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
INF = PC.INF


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_peaks_symbol_and_unchanged_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    assert hasattr(lib, "d3f_volume_peaks") and re.search(r"\bint d3f_volume_peaks\(", hdr)
    assert int(re.search(r"#define D3F_PEAKS_MAX_RADIUS (\d+)", hdr).group(1)) == _lib.PEAKS_MAX_RADIUS == PC.MAX_RADIUS == 8
    res, args = _lib.SIGNATURES["d3f_volume_peaks"]
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert res is ctypes.c_int
    assert args == [vp, vp, i32, i32, i32, vp, i64, i32, i64, i32, ctypes.c_float, vp, i64, vp, vp, i64, vp]
    # the declaration has as many parameters, in this order
    decl = re.search(r"\bint d3f_volume_peaks\(([^;]*)\);", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["slot", "mask", "nx", "ny", "nz", "score", "M", "K", "stride_row", "radius", "threshold", "out", "out_stride", "out_count",
                     "workspace", "workspace_bytes", "stream"]


def test_peaks_validation_status_codes():
    lib = _lib.load()
    err = lib.d3f_last_error
    p, q, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p((1 << 20) + 2)

    def peaks(slot=None, mask=None, shape=(4, 5, 6), score=p, M=120, K=3, stride_row=3, radius=1, threshold=float("inf"), out=q, out_stride=3, count=None,
              ws=None, ws_bytes=0):
        return lib.d3f_volume_peaks(slot, mask, shape[0], shape[1], shape[2], score, M, K, stride_row, radius, threshold, out, out_stride, count, ws, ws_bytes,
                                    None)

    # D3F_ERR_INVALID_ARG
    assert peaks(score=None) == _lib.ERR_INVALID_ARG and b"NULL" in err()
    assert peaks(out=None) == _lib.ERR_INVALID_ARG and b"NULL" in err()
    assert peaks(threshold=float("nan")) == _lib.ERR_INVALID_ARG and b"NaN" in err()
    for radius in (0, -1, 9, 1 << 20):
        assert peaks(radius=radius) == _lib.ERR_INVALID_ARG and b"radius" in err(), radius
    assert peaks(K=-1) == _lib.ERR_INVALID_ARG and peaks(M=-1) == _lib.ERR_INVALID_ARG and b"negative" in err()
    assert peaks(stride_row=2) == _lib.ERR_INVALID_ARG and peaks(out_stride=2) == _lib.ERR_INVALID_ARG and b"stride" in err()
    assert peaks(out=p) == _lib.ERR_INVALID_ARG and b"overlaps" in err()
    last = (119 * 3 + 3) * 4                         # the bytes score spans: out may begin right behind them, not one float earlier
    assert peaks(out=ctypes.c_void_p((1 << 20) + last - 4)) == _lib.ERR_INVALID_ARG and b"overlaps" in err()
    assert peaks(out=ctypes.c_void_p((1 << 20) - last + 4)) == _lib.ERR_INVALID_ARG and b"overlaps" in err()
    assert peaks(M=119) == _lib.ERR_INVALID_ARG and peaks(M=121) == _lib.ERR_INVALID_ARG and b"without slot" in err()
    assert peaks(slot=p, score=q, out=ctypes.c_void_p(1 << 28), M=121) == _lib.ERR_INVALID_ARG and b"rows" in err()
    # D3F_ERR_BAD_SHAPE: extents, voxel count, more column chunks than one launch holds (65535 chunks of 8 columns at r = 1)
    for bad in ((0, 5, 6), (4, 16385, 6), (4, 5, -2), (2048, 1024, 1024)):
        assert peaks(shape=bad) == _lib.ERR_BAD_SHAPE and b"extent" in err(), bad
    big = 65535 * 8 + 1
    assert peaks(shape=(1, 1, 1), M=1, K=big, stride_row=big, out_stride=big, out=ctypes.c_void_p(1 << 30)) == _lib.ERR_BAD_SHAPE and b"too large" in err()
    assert peaks(stride_row=1 << 62) == _lib.ERR_BAD_SHAPE and peaks(out_stride=1 << 58) == _lib.ERR_BAD_SHAPE and b"too large" in err()
    # D3F_ERR_BAD_LAYOUT: every int32 and float pointer; the mask is bytes
    for kw in ("slot", "score", "out", "count"):
        assert peaks(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    # M == 0 or K == 0: D3F_OK and nothing launched (without out_count no HIP call at all); validation still comes first
    assert peaks(K=0, stride_row=0, out_stride=0) == _lib.OK and peaks(K=0, stride_row=0, out_stride=0, score=None, out=None) == _lib.OK
    assert peaks(slot=p, M=0) == _lib.OK and peaks(slot=p, M=0, score=None, out=None) == _lib.OK and peaks(slot=p, M=0, mask=odd) == _lib.OK
    assert peaks(K=0, stride_row=0, out_stride=0, radius=0) == _lib.ERR_INVALID_ARG and peaks(slot=p, M=0, shape=(0, 1, 1)) == _lib.ERR_BAD_SHAPE
    assert peaks(slot=p, M=0, score=odd) == _lib.ERR_BAD_LAYOUT and peaks(M=0) == _lib.ERR_INVALID_ARG       # (without slot M must be the voxel count)
    for radius in range(1, 9):
        assert peaks(slot=p, M=0, radius=radius, threshold=-float("inf")) == _lib.OK
    # the call needs no workspace: NULL / 0 is legal and whatever is passed is never looked at
    assert peaks(slot=p, M=0, ws=odd, ws_bytes=-5) == _lib.OK
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(peaks(radius=9))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_ordered_keys_follow_float_order():
    vals = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4e38], np.float32)
    keys = PC.ordered_u32(vals).astype(np.int64)
    assert keys[4] == keys[5] and (np.diff(np.delete(keys, 4)) > 0).all()                     # -0.0 and +0.0 share a key; all else ascends strictly
    assert keys.max() < 0xFFFFFFFF                                                            # all ones stays free for "does not take part"


@pytest.mark.parametrize("shape,r", [((9, 10, 11), 1), ((9, 10, 11), 2), ((5, 4, 19), 8), ((1, 1, 40), 3), ((7, 9, 1), 1), ((12, 6, 7), 4)])
def test_restatement_equals_scipy_minimum_filter_on_tie_free_data(shape, r):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(21)
    vol = rng.permutation(int(np.prod(shape))).astype(np.float32).reshape(shape)             # tie-free
    out, count, loser = PC.peaks_ref(shape, None, None, vol.reshape(-1, 1), r)
    want = vol == ndimage.minimum_filter(vol, size=2 * r + 1, mode="constant", cval=np.inf)
    assert np.array_equal(out[:, 0] < INF, want.reshape(-1)) and count[0] == want.sum() and loser[0] == 0
    assert np.array_equal(out[want.reshape(-1), 0], vol[want])


@pytest.mark.parametrize("name", list(PC.CASES))
def test_restatement_equals_the_packed_key_formulation(name):
    c = PC.case(name)
    out, count, _ = PC.reference(name)
    out2, count2 = PC.peaks_keys_ref(c["shape"], c["slot"], c["mask"], c["score"], c["r"], c["threshold"])
    assert out.tobytes() == out2.tobytes() and np.array_equal(count, count2)
    assert np.array_equal(count, (out < INF).sum(axis=0))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_two_peaks_differ_by_more_than_r_on_some_axis(name):
    c = PC.case(name)
    out, _, _ = PC.reference(name)
    for q in range(out.shape[1]):
        at = np.stack(np.unravel_index(c["voxels"][out[:, q] < INF], c["shape"]), axis=1)
        if len(at) > 1:
            gap = np.abs(at[:, None, :] - at[None, :, :]).max(axis=2)
            assert (gap[~np.eye(len(at), dtype=bool)] > c["r"]).all(), (name, q)


def test_constant_volume_has_exactly_one_peak():
    out, count, loser = PC.reference("constant")
    assert count.tolist() == [1, 1] and (out[0] == 1.5).all() and (out[1:] == INF).all() and loser.tolist() == [719, 719]
    c = PC.case("constant band")                     # through a slot volume: the first STORED voxel, row 0
    out, count, _ = PC.reference("constant band")
    # a stored voxel is a peak only where no stored voxel of a lower index lies in its box: row 0 always is one
    assert (out[0] == 1.5).all() and count.min() >= 1
    out, count, _ = PC.reference("all inf")
    assert count.tolist() == [0, 0, 0] and (out == INF).all()


def test_signed_zeros_nan_and_infinities():
    shape = (1, 1, 5)

    def run(vals, r=1, threshold=np.inf):
        out, count, _ = PC.peaks_ref(shape, None, None, np.array(vals, np.float32).reshape(5, 1), r, threshold)
        return out[:, 0], int(count[0])

    out, n = run([1, -0.0, 0.0, 1, 1])                # equal zeros: the lower index wins, and the output keeps the sign bit
    assert n == 1 and np.signbit(out[1]) and out[1] == 0 and out[2] == INF
    out, n = run([1, 0.0, -0.0, 1, 1])
    assert n == 1 and not np.signbit(out[1]) and out[1] == 0 and out[2] == INF
    out, n = run([np.nan, 2, np.nan, 3, np.nan], r=2) # NaN takes no part: it neither wins nor suppresses
    assert n == 1 and out[1] == 2 and np.isinf(out[[0, 2, 3, 4]]).all()
    out, n = run([np.nan, 2, np.nan, np.nan, 3], r=1)
    assert n == 2 and out[1] == 2 and out[4] == 3
    out, n = run([np.inf, 5, np.inf, np.inf, np.inf]) # +Inf takes no part
    assert n == 1 and out[1] == 5
    out, n = run([3, -np.inf, -np.inf, 3, 3])         # -Inf takes part; ties among them go to the lower index
    assert n == 1 and out[1] == -np.inf and out[2] == INF
    out, n = run([-np.inf] * 5, r=2)                  # not greedy: voxel 3 loses to voxel 1, which is no peak itself
    assert n == 1 and out[0] == -np.inf
    out, n = run([3, 1, 2, 5, 4], threshold=-np.inf)
    assert n == 0


def test_the_threshold_suppresses_nothing():
    # 1 at z = 1 is above the threshold: no peak itself, it still suppresses the 2 next to it, which is below no threshold either
    out, count, _ = PC.peaks_ref((1, 1, 6), None, None, np.array([5, 1, 2, 6, 0.5, 7], np.float32).reshape(6, 1), 1, 0.75)
    assert count[0] == 1 and out[4, 0] == 0.5 and np.isinf(out[[0, 1, 2, 3, 5], 0]).all()
    for name in ("line r3", "ints r2", "20x17x37 dense", "6x7x23 r7"):
        c = PC.case(name)
        out, count, _ = PC.reference(name)
        free, free_count, _ = PC.peaks_ref(c["shape"], c["slot"], c["mask"], c["score"], c["r"])
        with np.errstate(invalid="ignore"):
            keep = free <= np.float32(c["threshold"])
        assert out.tobytes() == np.where(keep, free, INF).tobytes(), name               # the thresholded result is a filter of the free one
        assert 0 < count.sum() < free_count.sum(), (name, count.sum(), free_count.sum())


def test_wrap_case_tells_a_flat_neighbourhood_from_a_spatial_one():
    c = PC.case("wrap")
    out, count, _ = PC.reference("wrap")
    for pair in PC.WRAP_PAIRS:
        for at in pair:
            assert out[np.ravel_multi_index(at, c["shape"]), 0] < INF, at
        assert abs(np.ravel_multi_index(pair[0], c["shape"]) - np.ravel_multi_index(pair[1], c["shape"])) in (1, c["shape"][2])
    wrapped, _ = PC.peaks_keys_ref(c["shape"], None, None, c["score"], c["r"], wrap=True)
    for pair in PC.WRAP_PAIRS:                        # a window that runs round the end of its line loses the second voxel of each pair
        assert wrapped[np.ravel_multi_index(pair[1], c["shape"]), 0] == INF


def test_radius_from_separation():
    assert PC.radius_from_separation(0.004, 0.004) == 1 and PC.radius_from_separation(0.001, 0.004) == 1
    assert PC.radius_from_separation(0.008, 0.004) == 1 and PC.radius_from_separation(0.0081, 0.004) == 2
    assert PC.radius_from_separation(0.012, 0.004) == 2 and PC.radius_from_separation(0.036, 0.004) == 8 and PC.radius_from_separation(0.0361, 0.004) == 9
    # two peaks differ by more than r voxels, so by at least r + 1 >= separation / step, on some axis
    for sep, step in ((0.03, 0.004), (1.0, 0.25), (0.7, 0.1)):
        assert (PC.radius_from_separation(sep, step) + 1) * np.float64(step) >= sep


def test_topk_and_refine_references():
    out = np.array([[3, INF], [1, INF], [INF, INF], [1, 2], [0.5, INF]], np.float32)
    voxel, value = PC.topk_ref(out, 3, np.array([10, 11, 12, 13, 14]))
    assert voxel.tolist() == [[14, 11, 13], [13, -1, -1]] and value[0].tolist() == [0.5, 1, 1] and value[1, 0] == 2 and np.isinf(value[1, 1:]).all()
    # a parabola f = (z - 2.3)^2 sampled on a line: the vertex is recovered exactly
    z = np.arange(6, dtype=np.float64)
    f = ((z - 2.3) ** 2).astype(np.float32).reshape(6, 1)
    off = PC.refine_ref((1, 1, 6), None, None, f, np.array([[2, 0, -1]], np.int32))
    assert abs(off[0, 0, 2] - 0.3) < 1e-6 and off[0, 0, :2].tolist() == [0, 0]           # x, y: no neighbours inside the volume
    assert off[0, 1].tolist() == [0, 0, 0] and np.isnan(off[0, 2]).all()                   # z = 0 has no lower neighbour; padding is NaN
    flat = PC.refine_ref((1, 1, 3), None, None, np.ones((3, 1), np.float32), np.array([[1]], np.int32))
    assert flat[0, 0].tolist() == [0, 0, 0]                                                 # denominator 0


# ---- conditions of the case set -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.RANDOM)
def test_case_set_conditions(name):
    c = PC.case(name)
    _, count, loser = PC.reference(name)
    assert count.sum() >= 20, (name, count.sum())
    if name in PC.INTEGER:
        assert loser.sum() >= 20, (name, loser.sum())
    if CASE_PLANTS.get(name):
        assert c["planted"] >= CASE_PLANTS[name] and np.isnan(c["score"]).any() and (c["score"] == -np.inf).any() and np.signbit(c["score"][c["score"] == 0]).any()


CASE_PLANTS = {"20x17x37 dense": 20, "20x17x37 band mask ints": 10}


def test_the_issue_figures_of_the_integer_case():
    c = PC.case("ints r1")
    want = np.random.default_rng(12).integers(0, 4, size=(9, 10, 11)).astype(np.float32)
    assert np.array_equal(c["score"].reshape(9, 10, 11), want)
    _, count, loser = PC.reference("ints r1")
    assert (int(count[0]), int(loser[0])) == (24, 222)
    # the same data at r = 2 has few peaks (5: the plain loops, the packed keys and a per-pair loop agree), hence the wider range of "ints r2"
    assert int(PC.peaks_ref((9, 10, 11), None, None, c["score"], 2)[1][0]) == 5


def test_cases_cover_the_plans_of_the_kernel():
    radii = set(c[2] for c in PC.CASES.values())
    assert radii == set(range(1, 9))
    assert set(c[1] for c in PC.CASES.values()) >= {1, 3, 64, 65, 130}
    shape = PC.CASES["20x17x37 dense"][0]
    assert all(n > 2 * 8 for n in shape)                                                  # more than two tiles of 8 voxels on every axis


# ---- the kernel's resources ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "peaks_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    assert any("peaks_kernel" in r[0] for r in rows), out[-800:]
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0 and vgpr <= 64 and occ >= 8, (name, vgpr, scratch, occ)
