"""The fp64 point-cloud kernels on the mask side (csrc/pcd_kernels.hip: d3f_pcd_nearest, d3f_backproject_view; csrc/assoc_kernels.hip:
d3f_voxel_downsample, d3f_vox_idx_iou) against oracle/np_pcd.py on the cases of tests/pcd_cases.py: ties, near ties, NaN, overflow,
ragged sizes, strict bounds, capacity, extreme keys.  tests/test_pcd_cases_host.py shows on the CPU that every case has its property.
Every entry point is called through the C ABI on poisoned outputs, so a row the kernel leaves unwritten, or writes past the end, shows.

Mutants of the kernels and the assert that catches each:
  first minimum of the SQUARES instead of the roots (the rule before this file)     test_nearest_near_ties (argmin, 12 rows per case)
  `<=` for `<` when a root replaces the winner                                      test_nearest_duplicate_rows, test_nearest_sizes (lattice ties)
  NaN skipped (`NaN < best` is false), or a later NaN replacing the first           test_nearest_nan
  a tile's tail rows read from the previous tile (cnt ignored)                      test_nearest_sizes (nb 1, 255, 257, 513)
  `>=` / `<=` on a crop face                                                        test_backproject (on the crop bound)
  `d <= 1.5`, `d >= 0`, the upper gate applied under a mask, mask byte & 1          test_backproject (special depths)
  a slot written at or past capacity, or count clipped to capacity                  test_backproject_capacity
  an fma contracted into the transform, or x * (d / fx)                             test_backproject (points bit for bit)
  rank tile tail compared as a key, slot list past V                                test_voxel_mean (255 / 256 / 257 / 19683 voxels)
  20-bit axis keys                                                                  test_voxel_mean (extent)
  key -1 taken for the empty slot, table not doubled at 513                         test_vox_idx_iou
"""
import ctypes

import numpy as np
import pytest
import torch

import pcd_cases as PC
from d3fields_amd import _lib, pcd_utils

pytestmark = pytest.mark.gpu

POISON = -7.0
PAD = 5                             # poisoned rows behind every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _to(dev, arr, dtype=None):
    return torch.from_numpy(np.array(arr, dtype=dtype, order="C")).to(dev)         # a copy: the cases are read-only


# ---- d3f_pcd_nearest -----------------------------------------------------------------------------------------------------------------
def run_nearest(dev, a, b):
    lib = _lib.load()
    na = len(a)
    ta, tb = _to(dev, a, np.float64), _to(dev, b, np.float64)
    md = torch.full((na + PAD,), POISON, dtype=torch.float64, device=dev)
    am = torch.full((na + PAD,), int(POISON), dtype=torch.int64, device=dev)
    _lib.check(lib.d3f_pcd_nearest(_lib.ptr(ta), na, _lib.ptr(tb), len(b), _lib.ptr(md), _lib.ptr(am), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    md, am = md.cpu().numpy(), am.cpu().numpy()
    assert np.all(md[na:] == POISON) and np.all(am[na:] == int(POISON)), "written past the last query"
    return md[:na], am[:na]


def check_nearest(dev, case):
    md, am = run_nearest(dev, case["a"], case["b"])
    bad = np.flatnonzero(am != case["argmin"])
    print("%s: %d of %d argmin differ%s" % (case["name"], bad.size, len(am), "" if not bad.size else " (first: row %d got %d want %d)" % (bad[0], am[bad[0]], case["argmin"][bad[0]])))
    assert np.array_equal(am, case["argmin"]), case["name"]
    assert PC.same_bits(md, case["min_dist"]), case["name"]


@pytest.mark.parametrize("case", PC.tie_cases(), ids=lambda c: c["name"])
def test_nearest_near_ties(dev, case):
    """two rows of b whose squares differ and whose roots are equal: the earlier row wins, as with np.argmin over np.linalg.norm"""
    check_nearest(dev, case)


def test_nearest_duplicate_rows(dev):
    check_nearest(dev, PC.duplicate_case())


@pytest.mark.parametrize("nb", PC.NEAREST_NB)
def test_nearest_sizes(dev, nb):
    for na in PC.NEAREST_NA:
        check_nearest(dev, PC.sized_case(na, nb))


def test_nearest_nan(dev):
    """numpy's min / argmin: a NaN distance beats every number and the first NaN row wins; a NaN query sees NaN everywhere, row 0"""
    check_nearest(dev, PC.nan_b_case())
    check_nearest(dev, PC.nan_query_case())


def test_nearest_overflow(dev):
    """every square is inf: min_dist inf, argmin 0"""
    check_nearest(dev, PC.overflow_case())


def test_nearest_empty_b_is_bad_shape(dev):
    lib = _lib.load()
    t = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    md, am = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    assert lib.d3f_pcd_nearest(_lib.ptr(t), 4, _lib.ptr(t), 0, _lib.ptr(md), _lib.ptr(am), _lib.current_stream_handle(dev)) == _lib.ERR_BAD_SHAPE
    assert lib.d3f_pcd_nearest(_lib.ptr(t), 4, None, 0, _lib.ptr(md), _lib.ptr(am), _lib.current_stream_handle(dev)) == _lib.ERR_BAD_SHAPE


def test_pcd_iou_returns_numpys_rows_on_near_ties(dev):
    """the caller's view: min_idx_from_1_to_2 of pcd_iou is np.argmin's row"""
    case = PC.tie_case("tile boundary")
    out = pcd_utils.pcd_iou(np.array(case["a"]), np.array(case["b"]), 0.5)
    assert np.array_equal(out[5], case["argmin"]) and np.array_equal(out[3], np.flatnonzero(case["min_dist"] < 0.5))


# ---- d3f_backproject_view ------------------------------------------------------------------------------------------------------------
def run_backproject(dev, case, capacity=None):
    """-> (points [capacity + PAD, 3], pixels [capacity + PAD], count) as NumPy, outputs poisoned before the launch"""
    lib = _lib.load()
    H, W = case["depth"].shape
    cap = H * W if capacity is None else capacity
    d = _to(dev, case["depth"], np.float64)
    m = None if case["mask"] is None else _to(dev, case["mask"], np.uint8)
    pts = torch.full((cap + PAD, 3), POISON, dtype=torch.float64, device=dev)
    pix = torch.full((cap + PAD,), int(POISON), dtype=torch.int32, device=dev)
    cnt = torch.full((1,), int(POISON), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.d3f_backproject_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    dbl = lambda v: (ctypes.c_double * len(v))(*[float(x) for x in v])
    _lib.check(lib.d3f_backproject_view(_lib.ptr(d), _lib.ptr(m), H, W, dbl(case["cam"]), dbl(case["T"].reshape(-1)),
                                        dbl(case["bounds"]) if case["bounds"] is not None else None, cap, _lib.ptr(pts), _lib.ptr(pix), _lib.ptr(cnt),
                                        _lib.ptr(ws), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return pts.cpu().numpy(), pix.cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("case", PC.view_cases(), ids=lambda c: c["name"])
def test_backproject(dev, case):
    """count and pixel indices exactly, points bit for bit: the build contracts nothing, divides as IEEE does, and the kernel states numpy's
    operation order, so equality is the contract"""
    pts, pix, count = run_backproject(dev, case)
    n = len(case["pix"])
    assert count == n, case["name"]
    assert np.array_equal(pix[:n], case["pix"]) and np.all(pix[n:] == int(POISON)), case["name"]
    assert np.all(pts[n:] == POISON), "written past the last survivor"
    same = PC.same_bits(pts[:n], case["pts"])
    if not same:
        err = np.abs(pts[:n] - case["pts"])
        print("%s: %d of %d coordinates differ, max |diff| %.3g" % (case["name"], int((pts[:n] != case["pts"]).sum()), 3 * n, float(np.nanmax(err))))
    assert same, case["name"]


@pytest.mark.parametrize("capacity", [0, 1, 100, 255, 256, 257])
def test_backproject_capacity(dev, capacity):
    """capacity below the survivor count: count_out is the full count, exactly the first `capacity` rows are written, the rest untouched"""
    case = PC.survivors_case((9, 57), "all", False)
    n = len(case["pix"])
    assert capacity < n == 513
    pts, pix, count = run_backproject(dev, case, capacity)
    assert count == n
    assert np.array_equal(pix[:capacity], case["pix"][:capacity]) and PC.same_bits(pts[:capacity], case["pts"][:capacity])
    assert np.all(pix[capacity:] == int(POISON)) and np.all(pts[capacity:] == POISON)


def test_backproject_through_pcd_utils(dev):
    """the Python path sizes its outputs by H * W and cuts them at the count"""
    case = PC.random_view_case((7, 37), True, True)
    pts, pix = pcd_utils._backproject(case["depth"], case["mask"], case["cam"], case["T"], case["bounds"], dev)
    assert np.array_equal(pix.cpu().numpy(), case["pix"]) and PC.same_bits(pts.cpu().numpy(), case["pts"])


# ---- d3f_voxel_downsample ------------------------------------------------------------------------------------------------------------
def run_voxel_mean(dev, case):
    """-> (points [V,3], colours [V,3] or None), after checking that nothing behind row V was written"""
    lib = _lib.load()
    n = len(case["points"])
    p = _to(dev, case["points"], np.float64)
    c = None if case["colours"] is None else _to(dev, case["colours"], np.float64)
    out_p = torch.full((n + PAD, 3), POISON, dtype=torch.float64, device=dev)
    out_c = None if c is None else torch.full((n + PAD, 3), POISON, dtype=torch.float64, device=dev)
    cnt = torch.full((1,), int(POISON), dtype=torch.int64, device=dev)
    ws_bytes = lib.d3f_voxel_downsample_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_voxel_downsample(_lib.ptr(p), _lib.ptr(c), n, case["voxel_size"], _lib.ptr(out_p), _lib.ptr(out_c), _lib.ptr(cnt), _lib.ptr(ws),
                                        ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    v = int(cnt.item())
    assert 0 <= v <= n
    out_p = out_p.cpu().numpy()
    assert np.all(out_p[v:] == POISON), "a point written behind the last voxel"
    if out_c is None:
        return out_p[:v], None
    out_c = out_c.cpu().numpy()
    assert np.all(out_c[v:] == POISON), "a colour written behind the last voxel"
    return out_p[:v], out_c[:v]


@pytest.mark.parametrize("case", PC.tolerance_voxel_cases(), ids=lambda c: c["name"])
def test_voxel_mean(dev, case):
    """The voxel count equals np_pcd.voxel_mean's and the means agree in ascending voxel order to a tolerance derived from the code:
    the kernel truncates each point's offset inside its voxel to 2^-40 of a voxel side before its exact integer sum, so its mean lies
    within 2^-40 * voxel_size of the exact mean; the reference adds at most 8 points per voxel in float64 (asserted on the host), at
    most 7 roundings of an ulp of the mean each, and the kernel's corner + offset rounds once more: 8 ulp of max|p|.  Colours are stored
    at the same fixed point unscaled: 2^-40 absolute + 8 ulp of max|c|.  (pcd_cases.point_tol / colour_tol.)"""
    got_p, got_c = run_voxel_mean(dev, case)
    assert len(got_p) == len(case["want_points"]), case["name"]
    err = float(np.abs(got_p - case["want_points"]).max())
    tol = PC.point_tol(case["points"], case["voxel_size"])
    print("%s: %d voxels, points off by %.3g (tolerance %.3g)" % (case["name"], len(got_p), err, tol))
    assert err <= tol, case["name"]
    if case["colours"] is not None:
        err_c, tol_c = float(np.abs(got_c - case["want_colours"]).max()), PC.colour_tol(case["colours"])
        print("%s: colours off by %.3g (tolerance %.3g)" % (case["name"], err_c, tol_c))
        assert err_c <= tol_c, case["name"]


def test_voxel_mean_of_identical_points_is_the_point(dev):
    case = PC.identical_case()
    got_p, got_c = run_voxel_mean(dev, case)
    assert got_p.shape == (1, 3) and PC.same_bits(got_p[0], case["points"][0]) and PC.same_bits(got_c[0], case["colours"][0])


def test_voxel_mean_twice_gives_the_same_bits(dev):
    case = PC.count_case(PC.VOXEL_COUNTS[-1])
    first, again = run_voxel_mean(dev, case), run_voxel_mean(dev, case)
    assert PC.same_bits(first[0], again[0]) and PC.same_bits(first[1], again[1])


def test_voxel_downsample_through_pcd_utils(dev):
    case = PC.face_case()
    got_p, got_c = pcd_utils.voxel_downsample(case["points"], case["voxel_size"], case["colours"])
    assert got_p.shape == case["want_points"].shape and np.abs(got_p - case["want_points"]).max() <= PC.point_tol(case["points"], case["voxel_size"])
    assert np.abs(got_c - case["want_colours"]).max() <= PC.colour_tol(case["colours"])


# ---- d3f_vox_idx_iou -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.iou_cases(), ids=lambda c: c["name"])
def test_vox_idx_iou(dev, case):
    """|A & B| and |A | B| exactly, and the reference's triple of ratios"""
    lib = _lib.load()
    a, b = _to(dev, case["a"], np.int32), _to(dev, case["b"], np.int32)
    ws_bytes = lib.d3f_vox_iou_workspace_bytes(a.numel(), b.numel())
    assert ws_bytes == 8 * (1024 if a.numel() + b.numel() <= 512 else 1 << int(np.ceil(np.log2(2 * (a.numel() + b.numel())))))
    ws = torch.full((ws_bytes + 8 * PAD,), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((2 + PAD,), int(POISON), dtype=torch.int64, device=dev)
    _lib.check(lib.d3f_vox_idx_iou(_lib.ptr(a), a.numel(), _lib.ptr(b), b.numel(), _lib.ptr(counts), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    sa, sb = set(case["a"].tolist()), set(case["b"].tolist())
    assert counts[:2].tolist() == [len(sa & sb), len(sa | sb)], case["name"]
    assert np.all(counts[2:] == int(POISON)) and np.all(ws[ws_bytes:].cpu().numpy() == 0x5A), "written past the counts or the workspace"
    assert pcd_utils.vox_idx_iou(case["a"], case["b"]) == case["want"], case["name"]
