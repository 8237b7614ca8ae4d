"""Non-maximum suppression on the device (d3f_volume_peaks, csrc/peaks_kernels.hip; BakedField.peaks / locate) against the restatement of
tests/peaks_cases.py: equality of every output byte, no tolerance, from poisoned buffers one row longer than needed, and identical bytes
from a second run.

What each assert is there to catch:
  a window that runs on past the end of a z or y line, a halo read outside the volume                      wrap, 1x1x1, the line, the image
  a tie resolved by anything but the lower flat index, an order-dependent (greedy) suppression             integer scores, constant volumes
  -0.0 ordered below +0.0, NaN or +Inf taking part, -Inf left out                                          specials planted next to peaks
  a threshold that stops a voxel from suppressing                                                          the "mid" thresholds
  a tile, halo, column chunk or padded line off by one: every radius 1..8, K = 1, 3, 64, 65, 130           the case table
  a row found through the wrong slot, a masked voxel that still suppresses                                  band, mask, band + mask
  an output the kernel does not write, or writes where it should not (stride padding, the row past M)      poison
"""

import numpy as np
import pytest
import torch

import peaks_cases as PC
from d3fields_amd import _lib, corr_utils
from d3fields_amd.baked import BakedField

pytestmark = pytest.mark.gpu

INF = PC.INF
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run_kernel(c, dev, stride_row, out_stride, want_count=True):
    """one d3f_volume_peaks of a case from freshly poisoned buffers -> (out bytes of [M, K], count or None); the stride padding of out, its
    extra row and the entry past the last count must keep their poison; the padding of score holds -Inf, which would win wherever it were read"""
    lib = _lib.load()
    nx, ny, nz = c["shape"]
    score = c["score"]
    M, K = score.shape
    padded = np.full((M, stride_row), -np.inf, np.float32)
    padded[:, :K] = score
    t_score = torch.from_numpy(padded).to(dev)
    t_slot = None if c["slot"] is None else torch.from_numpy(c["slot"]).to(dev)
    t_mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(dev)
    out = torch.full(((M + 1) * out_stride * 4,), POISON, dtype=torch.uint8, device=dev)
    count = torch.full(((K + 1) * 4,), POISON, dtype=torch.uint8, device=dev) if want_count else None
    _lib.check(lib.d3f_volume_peaks(_lib.ptr(t_slot), _lib.ptr(t_mask), nx, ny, nz, _lib.ptr(t_score), M, K, stride_row, c["r"], c["threshold"], _lib.ptr(out),
                                    out_stride, _lib.ptr(count), None, 0, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    raw = out.cpu().numpy().reshape(M + 1, out_stride * 4)
    assert (raw[M] == POISON).all(), "a write past the last row"
    assert (raw[:M, K * 4:] == POISON).all(), "a write into the stride padding"
    got_count = None
    if want_count:
        words = count.cpu().numpy().view(np.int32)
        assert words[K] == np.frombuffer(bytes([POISON] * 4), np.int32)[0], "a write past the last count"
        got_count = words[:K].copy()
    return np.ascontiguousarray(raw[:M, :K * 4]).view(np.float32), got_count


def assert_same_bytes(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d entries differ, first at row %d column %d: got %r, want %r"
                             % (what, len(bad), got.size, bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_kernel_equals_the_restatement(name, dev):
    c = PC.case(name)
    want, want_count, _ = PC.reference(name)
    K = want.shape[1]
    got, count = run_kernel(c, dev, K + 3, K + 1)                    # stride_row > K, out_stride != stride_row
    assert_same_bytes(got, want, name)
    assert np.array_equal(count, want_count), (name, count.tolist()[:8], want_count.tolist()[:8])
    again, count2 = run_kernel(c, dev, K + 3, K + 1)                 # a second run gives identical bytes
    assert again.tobytes() == got.tobytes() and np.array_equal(count, count2)


@pytest.mark.parametrize("name", ["1x1x1", "line r8", "ints r1", "20x17x37 band", "20x17x37 band mask ints", "6x7x23 r7", "all inf", "constant"])
def test_kernel_contiguous_rows_and_no_count(name, dev):
    c = PC.case(name)
    want, _, _ = PC.reference(name)
    K = want.shape[1]
    got, _ = run_kernel(c, dev, K, K, want_count=False)
    assert_same_bytes(got, want, name)


def test_kernel_specials_are_planted_and_decided_as_defined(dev):
    """the planted case once more, entry by entry at the planted voxels: a NaN or +Inf neighbour leaves the peak alone and is none itself, a
    -Inf neighbour takes it over, of two equal zeros the lower index wins whatever the sign bits, and the output keeps the sign bit"""
    c = PC.case("20x17x37 dense")
    got, _ = run_kernel(c, dev, 3, 3)
    score = c["score"]
    with np.errstate(invalid="ignore"):
        assert not (got[np.isnan(score) | (score == INF)] < INF).any()
        peak = got < INF
    assert (got[peak].view(np.uint32) == score[peak].view(np.uint32)).all()
    zeros = peak & (score == 0)
    assert zeros.any() and np.signbit(score[zeros]).any() and (~np.signbit(score[zeros])).any()
    assert (peak & (score == -np.inf)).any()


# ---- BakedField.peaks -------------------------------------------------------------------------------------------------------------------
def make_field(shape, dev, step=0.25, origin=(-1.0, 0.5, 2.0), plane=None, **sets):
    """from_arrays on a plane distance (x - plane) * step, so that to_band keeps the slab round it"""
    x = torch.arange(shape[0], dtype=torch.float32, device=dev)[:, None, None].expand(shape)
    dist = ((x - (shape[0] // 2 if plane is None else plane)) * step).contiguous()
    return BakedField.from_arrays(origin, step, dist, **sets)


def check_peaks(field, c, got, want_out, k, largest, voxels_of_rows, slot, mask, work):
    voxel, value = PC.topk_ref(want_out, k, voxels_of_rows)
    assert np.array_equal(got["voxel"].cpu().numpy(), voxel)
    sign = -1.0 if largest else 1.0
    assert got["value"].cpu().numpy().tobytes() == (np.float32(sign) * value).tobytes()
    assert got["voxel"].dtype == torch.int32 and got["value"].dtype == torch.float32 and got["count"].dtype == torch.int32
    assert np.array_equal(got["count"].cpu().numpy(), (want_out < INF).sum(axis=0))
    centres = field._voxel_centres(torch.from_numpy(np.maximum(voxel, 0).reshape(-1)).to(field.device)).cpu().numpy().reshape(voxel.shape + (3,))
    centres = np.where((voxel >= 0)[..., None], centres, np.float32(np.nan))
    assert np.array_equal(got["points"].cpu().numpy(), centres, equal_nan=True)
    off = PC.refine_ref(c["shape"], slot, mask, work, voxel)
    want_refined = centres.astype(np.float64) + off * field.step
    refined = got["refined"].cpu().numpy()
    assert got["refined"].dtype == torch.float64 and np.array_equal(np.isnan(refined), np.isnan(want_refined))
    assert np.nanmax(np.abs(refined - want_refined), initial=0.0) <= 1e-12
    assert (np.abs(off[~np.isnan(off)]) <= 0.5).all()
    return off


@pytest.mark.parametrize("name,k,largest", [("ints r1", 8, False), ("ints r2", 3, True), ("20x17x37 dense", 8, False), ("20x17x37 mask", 5, True),
                                            ("5x4x19 r8", 1, False)])
def test_peaks_equals_topk_of_the_restatement(name, k, largest, dev):
    c = PC.case(name)
    want, _, _ = PC.reference(name)
    shape = c["shape"]
    K = want.shape[1]
    field = make_field(shape, dev)
    work = c["score"]
    values = torch.from_numpy(-work if largest else work).to(dev).view(shape + (K,))
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(dev)
    thr = None if c["threshold"] == np.inf else (-c["threshold"] if largest else c["threshold"])
    got = field.peaks(values, radius_voxels=c["r"], k=k, threshold=thr, largest=largest, mask=mask)
    off = check_peaks(field, c, got, want, k, largest, None, None, c["mask"], work)
    if name == "5x4x19 r8":                                              # 64 minima of tie-free floats, most with both z neighbours
        assert (np.abs(off[~np.isnan(off)]) > 1e-3).sum() >= 20          # the refinement does move points
    if K == 1:                                                           # one column may come without its axis
        one = field.peaks(values.view(shape), radius_voxels=c["r"], k=k, threshold=thr, largest=largest, mask=mask, refine=False)
        assert torch.equal(one["voxel"], got["voxel"]) and torch.equal(one["value"], got["value"]) and "refined" not in one
    sep = field.peaks(values, separation=(c["r"] + 1) * field.step, k=k, threshold=thr, largest=largest, mask=mask)
    assert torch.equal(sep["voxel"], got["voxel"])                       # r = max(1, ceil(separation / step) - 1)


def test_peaks_on_band_rows_equals_the_scattered_dense_volume(dev):
    shape, K, r, k = (20, 17, 37), 3, 2, 8
    field = make_field(shape, dev).to_band(0.6)                          # the slab |x - 10| <= 3 or so
    M = field.band_voxels.shape[0]
    assert 0 < M < 20 * 17 * 37 // 2
    rng = np.random.default_rng(31)
    rows = rng.integers(0, 30, size=(M, K)).astype(np.float32)
    rows[rng.random((M, K)) < 0.02] = np.nan
    got = field.peaks(torch.from_numpy(rows).to(dev), radius_voxels=r, k=k)
    slot, voxels = field.slot.cpu().numpy(), field.band_voxels.cpu().numpy()
    assert np.array_equal(slot.reshape(-1)[voxels], np.arange(M))
    want, _, loser = PC.peaks_ref(shape, slot, None, rows, r)
    assert (want < INF).sum() >= 20 and loser.sum() >= 20
    c = dict(shape=shape)
    check_peaks(field, c, got, want, k, False, voxels, slot, None, rows)
    dense = np.full((20 * 17 * 37, K), -1.0, np.float32)                # below every stored value: it would win if the mask let it
    dense[voxels] = rows
    stored = torch.from_numpy((slot >= 0)).to(dev)
    same = field.peaks(torch.from_numpy(dense).to(dev).view(shape + (K,)), radius_voxels=r, k=k, mask=stored)
    for key in ("voxel", "value", "count"):
        assert torch.equal(same[key], got[key]), key
    assert torch.equal(torch.nan_to_num(same["refined"], nan=7.0), torch.nan_to_num(got["refined"], nan=7.0))
    one = field.peaks(torch.from_numpy(rows[:, 1].copy()).to(dev), radius_voxels=r, k=k)          # [M]: one column
    assert torch.equal(one["voxel"][0], got["voxel"][1])


def test_peaks_argument_checks(dev):
    field = make_field((6, 5, 7), dev)
    v = torch.zeros((6, 5, 7), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="exactly one"):
        field.peaks(v)
    with pytest.raises(ValueError, match="exactly one"):
        field.peaks(v, radius_voxels=1, separation=0.5)
    with pytest.raises(ValueError, match="not built"):
        field.peaks(v, radius_voxels=9)
    with pytest.raises(ValueError, match="not built"):
        field.peaks(v, separation=10 * field.step + 1e-6)
    with pytest.raises(ValueError, match="k must"):
        field.peaks(v, radius_voxels=1, k=9)
    with pytest.raises(RuntimeError, match="CPU"):
        field.peaks(v.cpu(), radius_voxels=1)
    with pytest.raises(ValueError, match="values must be"):
        field.peaks(v.view(-1), radius_voxels=1)                         # rows need a banded field
    with pytest.raises(ValueError, match="mask"):
        field.peaks(v, radius_voxels=1, mask=torch.ones((6, 5), dtype=torch.bool, device=dev))
    got = field.peaks(v, separation=9 * field.step)                      # r = 8 is built; a constant volume has one peak, voxel 0
    assert got["voxel"][0].tolist() == [0] + [-1] * 7 and got["count"].tolist() == [1] and got["value"][0, 0] == 0 and torch.isinf(got["value"][0, 1:]).all()
    assert torch.isnan(got["points"][0, 1:]).all() and torch.isnan(got["refined"][0, 1:]).all() and not got["refined"].requires_grad
    none = field.peaks(torch.zeros((6, 5, 7, 0), dtype=torch.float32, device=dev), radius_voxels=1, k=4)      # an empty K launches nothing
    assert tuple(none["voxel"].shape) == (0, 4) and tuple(none["points"].shape) == (0, 4, 3) and tuple(none["count"].shape) == (0,)
    top = field.peaks(-v, radius_voxels=1, largest=True, k=2)
    assert top["voxel"][0].tolist() == [0, -1] and top["value"][0, 1] == -np.inf


# ---- BakedField.locate ------------------------------------------------------------------------------------------------------------------
PLANT_SHAPE, PLANT_C, PLANT_R = (24, 20, 28), 32, 2
PLANT_AT = (((12, 3, 4), (12, 10, 20), (11, 16, 8), (13, 5, 25)),       # per query four voxels near the plane x = 12, pairwise more than r apart
            ((12, 6, 12), (11, 2, 22), (13, 17, 17), (12, 13, 2)),
            ((13, 9, 9), (12, 17, 25), (11, 8, 16), (12, 1, 14)))


@pytest.fixture(scope="module")
def planted(dev):
    """a set whose background rows lie at L2 distance >= 0.5 from every query (they are about 10.4 away), with, for each of 3 queries d_q, the
    4 copies d_q + 0.05 j e at PLANT_AT[q][j]: their distances 0, 0.05, 0.10, 0.15 fix the order whatever the contraction rounds (its error
    is 2e-6 relative, against gaps of 0.05)"""
    rng = np.random.default_rng(41)
    n = int(np.prod(PLANT_SHAPE))
    feats = (0.1 / np.sqrt(PLANT_C)) * rng.uniform(-1, 1, size=(n, PLANT_C)).astype(np.float32)
    feats[:, 5] += 10.0
    queries = np.zeros((3, PLANT_C), np.float32)
    e = np.zeros(PLANT_C, np.float32)
    e[7] = 1.0
    want = np.zeros((3, 4), np.int32)
    for q in range(3):
        queries[q, q] = 3.0
        for j, at in enumerate(PLANT_AT[q]):
            want[q, j] = np.ravel_multi_index(at, PLANT_SHAPE)
            feats[want[q, j]] = queries[q] + np.float32(0.05 * j) * e
    flat = want.reshape(-1)
    at = np.stack(np.unravel_index(flat, PLANT_SHAPE), axis=1)
    gap = np.abs(at[:, None] - at[None]).max(axis=2)
    assert (gap[~np.eye(12, dtype=bool)] > PLANT_R).all()
    d = np.linalg.norm(feats[:, None, :].astype(np.float64) - queries[None].astype(np.float64), axis=2)
    background = np.ones(n, bool)
    background[flat] = False
    assert d[background].min() >= 0.5
    t = torch.from_numpy(feats).to(dev).view(PLANT_SHAPE + (PLANT_C,))
    field = make_field(PLANT_SHAPE, dev, plane=12, desc=t)
    return field, field.to_band(0.5), torch.from_numpy(queries).to(dev), want


@pytest.mark.parametrize("banded", [False, True])
def test_locate_finds_the_planted_copies_in_order(planted, banded):
    dense, band, queries, want = planted
    field = band if banded else dense
    if banded:
        assert set(want.reshape(-1).tolist()) <= set(field.band_voxels.cpu().tolist()) and field.stored_fraction < 0.5
    got = field.locate(queries, "desc", k=5, radius_voxels=PLANT_R, max_distance=0.4)
    assert np.array_equal(got["voxel"].cpu().numpy()[:, :4], want) and (got["voxel"][:, 4] == -1).all()       # the fifth slot is padding
    dist = got["distance"].cpu().numpy()
    assert np.abs(dist[:, :4] - 0.05 * np.arange(4)).max() < 1e-4 and np.isinf(dist[:, 4]).all()
    assert got["count"].tolist() == [4, 4, 4] and torch.isnan(got["points"][:, 4]).all() and "value" not in got
    assert torch.allclose(got["points"][:, :4], field._voxel_centres(torch.from_numpy(want.reshape(-1)).to(field.device)).view(3, 4, 3))
    sep = field.locate(queries, "desc", k=5, separation=(PLANT_R + 1) * field.step, max_distance=0.4)
    assert torch.equal(sep["voxel"], got["voxel"])
    # column chunking: two chunks (2 + 1 columns) give the same result
    M = field.band_voxels.shape[0] if banded else int(np.prod(PLANT_SHAPE))
    two = field.locate(queries, "desc", k=5, radius_voxels=PLANT_R, max_distance=0.4, max_bytes=8 * M * 2)
    assert torch.equal(two["voxel"], got["voxel"]) and torch.equal(two["count"], got["count"])
    assert np.abs(two["distance"].cpu().numpy()[:, :4] - dist[:, :4]).max() < 1e-5
    assert tuple(two["refined"].shape) == (3, 5, 3)


@pytest.mark.parametrize("banded", [False, True])
def test_locate_equals_peaks_on_the_distance_matrix(planted, banded):
    dense, band, queries, _ = planted
    field = band if banded else dense
    rows = field._sets["desc"].reshape(-1, PLANT_C)
    matrix, _ = corr_utils._pairwise(rows, queries, 1.0, "l2", _lib.SIM_DIST, False)
    got = field.locate(queries, "desc", k=8, radius_voxels=1)             # no max_distance: the background's own minima fill the list
    if banded:
        want = field.peaks(matrix, radius_voxels=1, k=8)
    else:
        want = field.peaks(matrix.view(PLANT_SHAPE + (3,)), radius_voxels=1, k=8, mask=field.valid)
    assert (got["voxel"] >= 0).all() and (got["count"] > 8).all()
    for key, other in (("voxel", "voxel"), ("distance", "value"), ("count", "count"), ("points", "points"), ("refined", "refined")):
        assert torch.equal(got[key], want[other]), key


def test_locate_argument_checks(planted, dev):
    dense, band, queries, _ = planted
    with pytest.raises(KeyError):
        dense.locate(queries, "colour", radius_voxels=1)
    with pytest.raises(ValueError, match="channels"):
        dense.locate(queries[:, :16], "desc", radius_voxels=1)
    with pytest.raises(RuntimeError, match="CPU"):
        dense.locate(queries.cpu(), "desc", radius_voxels=1)
    with pytest.raises(NotImplementedError):
        dense.locate(queries, "desc", radius_voxels=1, dist_type="cosine")
    with pytest.raises(ValueError, match="not built"):
        band.locate(queries, "desc", radius_voxels=9)
    none = band.locate(queries[:0], "desc", k=3, radius_voxels=1)
    assert tuple(none["voxel"].shape) == (0, 3) and tuple(none["distance"].shape) == (0, 3) and tuple(none["refined"].shape) == (0, 3, 3)
