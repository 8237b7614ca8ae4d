"""Dense descriptor flow on the device (d3f_volume_flow, csrc/flow_kernels.hip; BakedField.flow, Flow) against the NumPy restatement of
tests/flow_cases.py: targets, costs and axis costs are compared byte for byte, no tolerance anywhere; every launch runs twice for equal bytes.

What each assert is there to catch:
  a sum that rounds differently from the contract (order, a fused operation, the vector against the scalar path)   test_channels
  a halo row that is missing or taken from the wrong voxel, a window that wraps through memory                     test_tiles
  a merge across sub-window passes that is not exact                                                               test_subwindows
  <= against < at the threshold                                                                                    test_ties_and_threshold
  NaN, Inf, signed zeros, a NaN row of A, axis costs that must be +Inf                                             test_specials
  a row read through a slot of -1                                                                                  test_band
  a tile without a member of A that does not leave early, a B without members                                      test_empty
  a wiring error between BakedField.flow and the kernel                                                            test_api
  an output word read before it is written, or not written                                                         everything is poisoned with 0xA5
"""
import numpy as np
import pytest
import torch

import flow_cases as FC
from d3fields_amd import BakedField, Flow, _lib

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def upload_rows(dev, rows, stride, shift):
    """rows [.., C] -> (buffer, data pointer): rows `stride` floats apart, `shift` floats into a 16-byte aligned buffer, NaN between and behind"""
    C = rows.shape[-1]
    flat = np.array(rows, np.float32).reshape(-1, C)                 # (a copy: the case arrays are read-only)
    buf = torch.full((shift + max(len(flat), 1) * stride + 4,), float("nan"), dtype=torch.float32, device=dev)
    if len(flat):
        buf[shift:shift + len(flat) * stride].view(len(flat), stride)[:, :C] = torch.from_numpy(flat).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * shift


def launch(dev, member_a, rows_a, member_b, rows_b, r, max_cost2, slot_a=None, slot_b=None, stride=None, shift=0, axis=True):
    lib = _lib.load()
    nx, ny, nz = member_a.shape
    n, C = nx * ny * nz, rows_a.shape[-1]
    stride = C if stride is None else stride
    buf_a, ptr_a = upload_rows(dev, rows_a, stride, shift)
    buf_b, ptr_b = upload_rows(dev, rows_b, stride, shift)
    site_a = torch.from_numpy(np.asarray(member_a, np.uint8) * 3).to(dev)
    site_b = torch.from_numpy(np.asarray(member_b, np.uint8) * 255).to(dev)
    sl_a = None if slot_a is None else torch.from_numpy(np.ascontiguousarray(slot_a, np.int32)).to(dev)
    sl_b = None if slot_b is None else torch.from_numpy(np.ascontiguousarray(slot_b, np.int32)).to(dev)
    target = torch.full((n * 4,), FC.POISON, dtype=torch.uint8, device=dev)
    cost = torch.full((n * 4,), FC.POISON, dtype=torch.uint8, device=dev)
    ax = torch.full((n * 24,), FC.POISON, dtype=torch.uint8, device=dev) if axis else None
    sa, sb = _lib.VolumeSet(ptr_a, C, 0, stride, None), _lib.VolumeSet(ptr_b, C, 0, stride, None)
    _lib.check(lib.d3f_volume_flow(_lib.ptr(site_a), _lib.ptr(sl_a), sa, _lib.ptr(site_b), _lib.ptr(sl_b), sb, nx, ny, nz, r, float(max_cost2), _lib.ptr(target),
                                   _lib.ptr(cost), _lib.ptr(ax), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return {"target": target.cpu().numpy().view(np.int32).reshape(nx, ny, nz), "cost": cost.cpu().numpy().view(np.float32).reshape(nx, ny, nz),
            "axis_cost": ax.cpu().numpy().view(np.float32).reshape(nx, ny, nz, 6) if axis else None}


def run_flow(dev, *args, **kw):
    """two launches on poisoned outputs, which must agree byte for byte"""
    got, again = launch(dev, *args, **kw), launch(dev, *args, **kw)
    for k, a in got.items():
        assert a is None or a.tobytes() == again[k].tobytes(), (k, "two runs differ")
    return got


def same(got, ref, what):
    for k in ("target", "cost", "axis_cost"):
        if ref.get(k) is None or got.get(k) is None:
            continue
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


@pytest.mark.parametrize("C", FC.CHANNELS)
def test_channels(dev, C):
    """Gaussian rows: the sums are inexact, so another order of summation shows in the cost's bits"""
    shape = FC.CHANNEL_SHAPE
    case = FC.random_case(shape, C, 300 + C, 0.9, "gauss")
    ref = FC.random_reference(shape, C, 300 + C, 0.9, "gauss", 2)
    assert (ref["target"] >= 0).sum() > 300
    for stride, shift in ((C, 0), (C + 4, 0), (C + 3, 1)):           # plain and padded rows (vector where C % 4 == 0); odd stride off 16 bytes: scalar
        same(run_flow(dev, *case, 2, INF, stride=stride, shift=shift), ref, (C, stride, shift))


@pytest.mark.parametrize("shape", FC.TILE_SHAPES)
def test_tiles(dev, shape):
    for r in (1, 2, 3, 4):
        for density, kind, C in ((0.9, "gauss", 4), (0.3, "int", 3)):
            case = FC.random_case(shape, C, 400 + r, density, kind)
            ref = FC.random_reference(shape, C, 400 + r, density, kind, r)
            same(run_flow(dev, *case, r, INF), ref, (shape, r, density))


@pytest.mark.parametrize("r", [3, 4])
def test_subwindows(dev, r):
    shape = (2 * r + 1, 2 * r + 1, 2 * r + 3)
    for off in FC.window_marks(r):                                   # the unique best at each corner, each face centre and the centre
        ma, ra, mb, rb, centre = FC.planted(shape, r, 3, [off])
        got = run_flow(dev, ma, ra, mb, rb, r, INF)
        same(got, FC.flow_ref(ma, ra, mb, rb, r, INF), (r, off))
        assert tuple(FC.voxel_offsets(got["target"])[centre]) == off and got["cost"][centre] == 0
    # two candidates tie in s and sit in different passes (the sub-windows split every axis between 0 and 1)
    for pair, winner in ((((-2, 0, 0), (1, 0, 0)), (1, 0, 0)),       # d2 decides, against the order of j and of the passes
                         (((-1, 0, 0), (1, 0, 0)), (-1, 0, 0)),      # only j decides
                         (((0, 1, -1), (0, -1, 1)), (0, -1, 1)),
                         (((1, 1, 1), (-1, -1, -1)), (-1, -1, -1)),
                         (((0, 0, 2), (0, -1, 0)), (0, -1, 0))):
        ma, ra, mb, rb, centre = FC.planted(shape, r, 3, list(pair), cost_levels=(4.0,))
        got = run_flow(dev, ma, ra, mb, rb, r, INF)
        same(got, FC.flow_ref(ma, ra, mb, rb, r, INF), (r, pair))
        assert tuple(FC.voxel_offsets(got["target"])[centre]) == winner and got["cost"][centre] == 4.0


def test_ties_and_threshold(dev):
    shape, C, r = (5, 5, 17), 5, 2
    case = FC.random_case(shape, C, 500, 0.9, "gauss")
    free = FC.random_reference(shape, C, 500, 0.9, "gauss", r)
    costs = np.sort(free["cost"][free["target"] >= 0])
    s = costs[len(costs) // 2]                                       # the winning cost of one voxel, exactly
    below = np.nextafter(s, np.float32(0))
    got = {}
    for mc in (s, below, np.float32(np.inf)):
        got[float(mc)] = run_flow(dev, *case, r, float(mc))
        same(got[float(mc)], FC.flow_ref(*case, r, float(mc)), ("threshold", float(mc)))
    at = free["cost"] == s
    assert (got[float(s)]["cost"][at] == s).all() and not (got[float(below)]["cost"][at] == s).any()
    assert (got[float(s)]["target"] >= 0).sum() > (got[float(below)]["target"] >= 0).sum() > 0
    # exact sums: many candidates sit ON the threshold, and many tie
    case = FC.random_case(shape, 3, 501, 0.9, "int")
    for mc in (0.0, 1.0, 2.0):
        same(run_flow(dev, *case, r, mc), FC.flow_ref(*case, r, mc), ("int threshold", mc))
    ma, ra, mb, rb, hole = FC.identical_b()
    same(run_flow(dev, ma, ra, mb, rb, 4, INF), FC.flow_ref(ma, ra, mb, rb, 4, INF), "identical rows")


def test_specials(dev):
    shape, C = (4, 5, 17), 4
    ma, ra, mb, rb = (a.copy() for a in FC.random_case(shape, C, 600, 1.0, "gauss"))
    rb[1, 1, 3, 2] = np.nan                      # a candidate with a NaN takes no part
    rb[1, 2, 5, 0] = np.inf                      # s = +Inf: takes no part
    rb[2, 2, 7, 1] = -np.inf
    rb[2, 3, 9] = 3e38                           # d*d overflows: s = +Inf
    ra[3, 3, 12] = np.nan                        # an A row of NaN: every candidate is NaN, -1 / +Inf
    ra[0, 0, 15, 1] = np.inf                     # Inf - finite: +Inf everywhere; no candidate
    ra[1, 1, 1], rb[1, 1, 1] = -0.0, 0.0         # signed zeros: s = +0
    rb[0, 0, 0], rb[0, 0, 1] = [0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, -0.0, 0.0]
    ra[0, 0, 0] = 0.0
    rb[2:4, 0:3, 14:17] = np.nan                 # every candidate of (3, 1, 15) at r = 1 is NaN
    for r in (1, 2):
        ref = FC.flow_ref(ma, ra, mb, rb, r, INF)
        got = run_flow(dev, ma, ra, mb, rb, r, INF)
        same(got, ref, ("specials", r))
        assert got["target"][3, 3, 12] == -1 and got["target"][0, 0, 15] == -1 and np.isinf(got["axis_cost"][3, 3, 12]).all()
        assert got["target"][1, 1, 1] == np.ravel_multi_index((1, 1, 1), shape) and got["cost"][1, 1, 1].tobytes() == np.float32(0).tobytes()
        assert got["cost"][0, 0, 0].tobytes() == np.float32(0).tobytes()
    assert got["target"][3, 1, 15] >= 0 and FC.flow_ref(ma, ra, mb, rb, 1, INF)["target"][3, 1, 15] == -1
    matched = ref["target"] >= 0
    assert np.isinf(ref["axis_cost"][matched]).any() and np.isfinite(ref["axis_cost"][matched]).any()


def test_band(dev):
    shape, C, r = (5, 6, 18), 8, 2
    ma, ra, mb, rb = FC.random_case(shape, C, 700, 0.9, "gauss")
    slot_a, band_a = FC.band_of(ma, ra, 701)
    slot_b, band_b = FC.band_of(mb, rb, 702)
    assert (slot_a[ma] < 0).any() and (slot_b[mb] < 0).any()
    for use_a, use_b in ((True, False), (False, True), (True, True)):
        ref = FC.flow_ref(FC.members_of(ma, slot_a if use_a else None), ra, FC.members_of(mb, slot_b if use_b else None), rb, r, INF)
        got = run_flow(dev, ma, band_a if use_a else ra, mb, band_b if use_b else rb, r, INF, slot_a=slot_a if use_a else None,
                       slot_b=slot_b if use_b else None)
        same(got, ref, ("band", use_a, use_b))


def test_empty(dev):
    shape, C = (9, 9, 33), 4
    ma, ra, mb, rb = FC.random_case(shape, C, 800, 0.9, "gauss")
    none = np.zeros(shape, bool)
    for r in (1, 4):
        got = run_flow(dev, ma, ra, none, rb, r, INF)                # B without any member
        assert (got["target"] == -1).all() and np.isinf(got["cost"]).all() and (got["cost"] > 0).all() and np.isinf(got["axis_cost"]).all()
        got = run_flow(dev, none, ra, mb, rb, r, INF)                # A without any member: every tile leaves early
        assert (got["target"] == -1).all() and np.isinf(got["cost"]).all() and np.isinf(got["axis_cost"]).all()
        corner = none.copy()
        corner[:2, :2, :3] = ma[:2, :2, :3]                          # one tile with members among tiles without
        same(run_flow(dev, corner, ra, mb, rb, r, INF), FC.flow_ref(corner, ra, mb, rb, r, INF), ("corner", r))
    # an empty band through the Python API: nothing is launched
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    far = BakedField.from_arrays((0, 0, 0), 0.01, t(np.ones(shape, np.float32)), feat=t(ra)).to_band(0.005)
    near = BakedField.from_arrays((0, 0, 0), 0.01, t(np.where(ma, -0.001, 1.0).astype(np.float32)), feat=t(ra))
    assert far.band_voxels.shape[0] == 0
    for a, b in ((far, near), (near, far)):
        f = a.flow(b, "feat", radius_voxels=2, sites=t(ma), other_sites=t(mb))
        assert bool((f.target == -1).all()) and bool(torch.isinf(f.cost).all()) and not bool(f.matched.any()) and bool(torch.isinf(f.axis_cost).all())
        assert bool(torch.isnan(f.offset).all()) and bool((f.voxel_offset == 0).all())


def test_api(dev):
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    ma, ra, mb, rb, moved = FC.shifted_copy()
    shape, origin, step = ma.shape, (0.5, -0.25, 1.0), 0.02
    rb0 = np.nan_to_num(rb, nan=7.0)                                  # (finite rows where B has no member: a dense field stores every voxel)
    rng = np.random.default_rng(5)
    valid_a, valid_b = rng.random(shape) < 0.95, rng.random(shape) < 0.95
    dist = lambda m: np.where(m, -0.001, 1.0).astype(np.float32)
    A = BakedField.from_arrays(origin, step, t(dist(ma)), valid=t(valid_a), feat=t(ra), other=t(ra[..., :3]))
    B = BakedField.from_arrays(origin, step, t(dist(mb)), valid=t(valid_b), feat=t(rb0), other=t(rb0[..., :4]))
    Ab, Bb = A.to_band(0.5 * step), B.to_band(0.5 * step)
    assert 0 < Ab.stored_fraction < 1 and 0 < Bb.stored_fraction < 1
    for fa, fb in ((A, B), (Ab, B), (A, Bb), (Ab, Bb)):
        mem_a = ma & valid_a & (True if fa.band is None else fa.slot.cpu().numpy() >= 0)
        mem_b = mb & valid_b & (True if fb.band is None else fb.slot.cpu().numpy() >= 0)
        for r, max_cost in ((2, None), (3, 2.5)):
            mc2 = INF if max_cost is None else float(np.float32(max_cost) * np.float32(max_cost))
            ref = FC.flow_ref(mem_a, ra, mem_b, rb0, r, mc2)
            f = fa.flow(fb, "feat", radius_voxels=r, max_cost=max_cost)
            assert isinstance(f, Flow) and f.target.dtype == torch.int32 and f.cost.dtype == torch.float32 and f.axis_cost.dtype == torch.float32
            same({"target": f.target.cpu().numpy(), "cost": f.cost.cpu().numpy(), "axis_cost": f.axis_cost.cpu().numpy()}, ref, ("api", r, max_cost))
            matched = ref["target"] >= 0
            assert matched.sum() > 50 and np.array_equal(f.matched.cpu().numpy(), matched)
            vo = FC.voxel_offsets(ref["target"])
            assert f.voxel_offset.dtype == torch.int32 and np.array_equal(f.voxel_offset.cpu().numpy(), vo)
            off = FC.refine_offsets(ref["cost"], ref["axis_cost"], matched)
            assert f.offset.dtype == torch.float64 and np.array_equal(f.offset.cpu().numpy(), off, equal_nan=True)
            assert np.array_equal(f.displacement().cpu().numpy(), (vo.astype(np.float64) + off) * step, equal_nan=True)
            plain = np.where(matched[..., None], vo.astype(np.float64) * step, np.nan)
            assert np.array_equal(f.displacement(refined=False).cpu().numpy(), plain, equal_nan=True)
        coarse = fa.flow(fb, "feat", radius_voxels=2, refine=False)
        assert coarse.axis_cost is None and coarse.offset is None and torch.equal(coarse.target, fa.flow(fb, "feat").target)
        with pytest.raises(ValueError):
            coarse.displacement()
    # the shifted copy with explicit sites: forward and backward agree (tol 0: exactly) on the members whose copy lies inside the volume
    ones = np.ones(shape, np.float32)
    A1 = BakedField.from_arrays(origin, step, t(ones), feat=t(ra))
    B1 = BakedField.from_arrays(origin, step, t(ones), feat=t(rb0))
    fwd = A1.flow(B1, "feat", radius_voxels=2, sites=t(ma), other_sites=t(mb))
    back = B1.flow(A1, "feat", radius_voxels=2, sites=t(mb), other_sites=t(ma))
    same({"target": fwd.target.cpu().numpy(), "cost": fwd.cost.cpu().numpy()}, FC.flow_ref(ma, ra, mb, rb0, 2, INF, axis=False), "sites")
    assert np.array_equal(fwd.consistent(back, tol_voxels=0).cpu().numpy(), moved)
    assert np.array_equal(fwd.consistent(back).cpu().numpy(), FC.consistent_ref(fwd.target.cpu().numpy(), back.target.cpu().numpy(), 1))
    assert (fwd.voxel_offset.cpu().numpy()[moved] == np.array(FC.SHIFT)).all() and bool((fwd.cost[t(moved)] == 0).all())
    # the argument errors
    bare = BakedField.from_arrays(origin, step, t(ones))
    for bad in (lambda: bare.flow(B, "feat"), lambda: A.flow(bare, "feat"), lambda: A.flow(B, "nope"), lambda: A.flow("B", "feat"),
                lambda: A.flow(BakedField.from_arrays(origin, step, t(ones), other=t(rb0)), "feat"),      # the name is missing in the other field
                lambda: A.flow(B, "other"),                                                                 # 3 channels against 4
                lambda: A.flow(BakedField.from_arrays(origin, step, t(ones[:-1]), feat=t(rb0[:-1])), "feat"),
                lambda: A.flow(BakedField.from_arrays((0.5, -0.25, 1.5), step, t(ones), feat=t(rb0)), "feat"),
                lambda: A.flow(BakedField.from_arrays(origin, 0.03, t(ones), feat=t(rb0)), "feat"),
                lambda: A.flow(B, "feat", radius_voxels=0), lambda: A.flow(B, "feat", radius_voxels=5), lambda: A.flow(B, "feat", radius_voxels=True),
                lambda: A.flow(B, "feat", radius_voxels=2.0), lambda: A.flow(B, "feat", max_cost=-1.0), lambda: A.flow(B, "feat", max_cost=float("nan")),
                lambda: fwd.consistent(back, tol_voxels=-1), lambda: fwd.consistent(fwd.target)):
        with pytest.raises(ValueError):
            bad()
