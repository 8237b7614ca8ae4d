"""The pyramid of a baked field and the seeded flow on the device (d3f_volume_coarsen_select / d3f_volume_coarsen_rows, csrc/pyramid_kernels.hip;
d3f_volume_flow_seeded, csrc/flow_seeded_kernels.hip; BakedField.coarsen / pyramid / flow(seed=) / flow_pyramid, Flow.seed) against the NumPy
restatements of tests/pyramid_cases.py: every output is compared byte for byte, no tolerance anywhere, except NaN-ness where a NaN the mean
itself produces has no specified payload.  EVERY launch runs twice on outputs poisoned with 0xA5 and both runs must give the bytes of the
restatement: the entry points take their arguments in a struct, so tests/dirty_cases.py does not list them, and this file carries the
dirty-buffer guarantee instead.  On the parent commit there is no symbol and no method: every test here fails there.

What each assert is there to catch:
  a child outside the volume read, a ragged last wave, dist read behind valid == 0, a NaN counted, another order of the sum     test_select
  the lane mappings at 16 / 17 channels, vectors against scalars, strides, a misaligned base, half rows                         test_rows_widths, test_rows_half
  a slot of -1 read, a bit of a child that is not stored, fill rows, voxel lists with duplicates and entries outside            test_rows_band_and_lists
  an empty list, an empty band behind NULL pointers, no set at all                                                              test_rows_empty
  a wiring error between BakedField.coarsen / pyramid and the kernels, the band of the result                                   test_api_coarsen
  a seeded kernel that differs from d3f_volume_flow at a zero seed (the pin against existing code)                              test_zero_seed_*
  a window centred elsewhere than v + seed, a candidate that wraps, a seed read behind a non-member, the range test             test_seeded_*
  ties about the seeded centre, <= against < at the threshold                                                                   test_seeded_ties_and_threshold
  a wiring error between flow(seed=), Flow.seed, flow_pyramid and the kernels                                                   test_api_chain"""
import ctypes

import numpy as np
import pytest
import torch

import flow_cases as FC
import pyramid_cases as PC
from d3fields_amd import BakedField, Flow, _lib

pytestmark = pytest.mark.gpu
POISON = 0xA5
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(dev, shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(n, 16),), POISON, dtype=torch.uint8, device=dev)[:n].view(dtype).view(shape)


def up(dev, a, dt=None):
    return torch.from_numpy(np.array(a, dt)).to(dev)               # (a copy: the case arrays are read-only)


def same_bytes(have, want, what):
    assert have.dtype == want.dtype and have.shape == want.shape, (what, have.dtype, want.dtype, have.shape, want.shape)
    if have.tobytes() != want.tobytes():
        word = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.itemsize]
        bad = np.flatnonzero(np.ascontiguousarray(have).view(word).reshape(-1) != np.ascontiguousarray(want).view(word).reshape(-1))
        raise AssertionError((what, len(bad), bad[:4].tolist(), have.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist()))


def call(dev, name, args):
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(args), _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()


# ---- select -----------------------------------------------------------------------------------------------------------------------
def select_once(dev, dist, valid, mc):
    shape, cs = dist.shape, PC.coarse_shape(dist.shape)
    d, v = up(dev, dist, np.float32), up(dev, valid, np.uint8)
    out = {"dist": poisoned(dev, cs, torch.float32), "valid": poisoned(dev, cs, torch.uint8), "children": poisoned(dev, cs, torch.uint8)}
    call(dev, "d3f_volume_coarsen_select", _lib.CoarsenSelect(shape[0], shape[1], shape[2], mc, _lib.ptr(d), _lib.ptr(v), _lib.ptr(out["dist"]), _lib.ptr(out["valid"]),
                                                               _lib.ptr(out["children"]), 0))
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("shape", PC.SHAPES + [(1, 1, 1), (1, 2, 67)], ids=str)
def test_select(dev, shape):
    cs = PC.coarsen_case(shape, 4, 31)
    for mc in PC.MIN_CHILDREN:
        ref = PC.coarsen_ref(cs["dist"], cs["valid"], mc)
        got, again = select_once(dev, cs["dist"], cs["valid"], mc), select_once(dev, cs["dist"], cs["valid"], mc)
        for k in ("children", "valid", "dist"):
            same_bytes(got[k], again[k], (shape, mc, k, "two runs differ"))
            same_bytes(got[k], ref[k], (shape, mc, k))


def test_select_signs_and_infinities(dev):
    """-0 alone stays out of the sum's sign (+0 + -0 = +0); infinities of one sign give that infinity, of both a NaN (NaN-ness only)"""
    shape = (4, 2, 2)
    dist = np.zeros(shape, np.float32)
    dist[:2] = np.float32(-0.0)
    dist[2:] = np.inf
    dist[3, 1, 1] = -np.inf
    valid = np.ones(shape, np.uint8)
    ref = PC.coarsen_ref(dist, valid)
    got = select_once(dev, dist, valid, 1)
    assert ref["dist"].tobytes()[:4] == np.float32(0).tobytes() and np.isnan(ref["dist"][1, 0, 0])
    assert PC.same_rows(got["dist"], ref["dist"])
    same_bytes(got["children"], ref["children"], "children")


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def up_rows(dev, rows, C, stride, misalign):
    """[R, C] rows -> (buffer, view): rows `stride` elements apart, the base `misalign` elements into a 16-byte aligned buffer, NaN between"""
    dt = torch.float16 if rows.dtype == np.float16 else torch.float32
    R = rows.shape[0]
    buf = torch.full((misalign + max(R, 1) * stride + 8,), float("nan"), dtype=dt, device=dev)
    if R:
        buf[misalign:misalign + R * stride].view(R, stride)[:, :C] = torch.from_numpy(np.array(rows)).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[misalign:]


def rows_once(dev, shape, children, sets, voxels=None, slot=None, stride_extra=0, misalign=0):
    """sets: [(rows [R, C] float32 / float16 or None behind an empty band, fill)]; slot: None (dense), an int32 volume, or "empty" """
    nc = int(np.prod(PC.coarse_shape(shape)))
    m = nc if voxels is None else len(voxels)
    vox = None if voxels is None else up(dev, np.concatenate([voxels, [0]]), np.int32)      # (one entry more: an empty list still has an address)
    hold, res = [], []
    arr, outs = (_lib.VolumeSet * max(len(sets), 1))(), (ctypes.c_void_p * max(len(sets), 1))()
    for s, (rows, fill, C) in enumerate(sets):
        f = None if fill is None else up(dev, fill, np.float32)
        out = poisoned(dev, (max(m, 1) * C,), torch.float32)[:m * C].view(m, C)
        stride = C + stride_extra
        if rows is None:
            arr[s] = _lib.VolumeSet(None, C, _lib.DTYPE_F32, stride, _lib.ptr(f))
        else:
            buf, view = up_rows(dev, rows, C, stride, misalign)
            hold.append(buf)
            arr[s] = _lib.VolumeSet(view.data_ptr(), C, _lib.DTYPE_F16 if rows.dtype == np.float16 else _lib.DTYPE_F32, stride, _lib.ptr(f))
        hold.append(f)
        outs[s] = out.data_ptr()
        res.append(out)
    known = poisoned(dev, (max(m, 1),), torch.uint8)[:m]
    band = None
    if isinstance(slot, str):
        band = ctypes.pointer(_lib.Band(None, None, 0))
    elif slot is not None:
        t = up(dev, slot, np.int32)
        hold.append(t)
        band = ctypes.pointer(_lib.Band(_lib.ptr(t), None, int(slot.max()) + 1))              # (cell_band is not read)
    ch = up(dev, children, np.uint8)
    call(dev, "d3f_volume_coarsen_rows", _lib.CoarsenRows(shape[0], shape[1], shape[2], len(sets), band, arr, _lib.ptr(ch), _lib.ptr(vox), m, outs, _lib.ptr(known), 0))
    return [r.cpu().numpy() for r in res], known.cpu().numpy()


def run_rows(dev, what, shape, children, sets, voxels=None, slot=None, **kw):
    got, again = rows_once(dev, shape, children, sets, voxels, slot, **kw), rows_once(dev, shape, children, sets, voxels, slot, **kw)
    same_bytes(got[1], again[1], (what, "known: two runs differ"))
    for s, (rows, fill, C) in enumerate(sets):
        same_bytes(got[0][s], again[0][s], (what, s, "two runs differ"))
        if isinstance(slot, str):
            data, sl = np.zeros((0, C), np.float32), np.full(shape, -1, np.int32)
        else:
            data, sl = (rows.reshape(tuple(shape) + (C,)), None) if slot is None else (rows, slot)
        want, want_known = PC.rows_ref(children, shape, data, fill=fill, voxels=voxels, slot=sl)
        assert PC.same_rows(got[0][s], want), (what, "set", s, C, np.flatnonzero((got[0][s] != want).any(1))[:4])
        same_bytes(got[1], want_known, (what, "known"))
    return got


def flat_rows(cs):
    C = cs["rows"].shape[-1]
    return np.ascontiguousarray(cs["rows"]).reshape(-1, C)


@pytest.mark.parametrize("C", PC.CHANNELS)
def test_rows_widths(dev, C):
    shape = (5, 6, 17)
    cs = PC.coarsen_case(shape, C, 40 + C)
    children = PC.coarsen_ref(cs["dist"], cs["valid"])["children"]
    for extra, misalign in ((0, 0), (4, 0), (3, 1)):              # plain and padded rows (vectors where C % 4 == 0); odd stride off 16 bytes: scalar
        run_rows(dev, (C, extra, misalign), shape, children, [(flat_rows(cs), cs["fill"], C)], stride_extra=extra, misalign=misalign)
    run_rows(dev, (C, "band"), shape, children, [(cs["banded"], cs["fill"], C)], slot=cs["slot"], voxels=cs["voxels"])


@pytest.mark.parametrize("C", PC.HALF_CHANNELS)
def test_rows_half(dev, C):
    shape = (5, 6, 17)
    cs = PC.coarsen_case(shape, C, 60 + C, True)
    assert cs["rows"].dtype == np.float16
    children = PC.coarsen_ref(cs["dist"], cs["valid"])["children"]
    for extra, misalign in ((0, 0), (8, 0), (3, 1)):
        run_rows(dev, (C, extra, misalign), shape, children, [(flat_rows(cs), cs["fill"], C)], stride_extra=extra, misalign=misalign)
    run_rows(dev, (C, "band"), shape, children, [(cs["banded"], None, C)], slot=cs["slot"])
    # both storages and both widths in one launch
    other = PC.coarsen_case(shape, 20, 77)
    run_rows(dev, (C, "mixed"), shape, children, [(flat_rows(cs), cs["fill"], C), (flat_rows(other), other["fill"], 20), (flat_rows(other)[:, :3].copy(), None, 3)])


@pytest.mark.parametrize("shape", PC.SHAPES, ids=str)
def test_rows_band_and_lists(dev, shape):
    cs = PC.coarsen_case(shape, 17, 90)
    narrow = PC.coarsen_case(shape, 4, 91)
    for mc in (1, 8):
        children = PC.coarsen_ref(cs["dist"], cs["valid"], mc)["children"]
        sets = [(flat_rows(cs), cs["fill"], 17), (flat_rows(narrow), None, 4)]
        run_rows(dev, (shape, "dense"), shape, children, sets)
        run_rows(dev, (shape, "dense list"), shape, children, sets, voxels=cs["voxels"])
    children = PC.coarsen_ref(cs["dist"], cs["valid"])["children"]
    got = run_rows(dev, (shape, "band list"), shape, children, [(cs["banded"], cs["fill"], 17)], slot=cs["slot"], voxels=cs["voxels"])
    assert (got[1][-5:] == 0).all() and same_bytes(got[0][0][-1], cs["fill"], "an entry outside: the fill row") is None
    # every bit set, whatever select would say: the bits of children outside the volume are ignored, nothing is read out of bounds
    full = np.full(PC.coarse_shape(shape), 255, np.uint8)
    run_rows(dev, (shape, "all bits"), shape, full, [(flat_rows(cs), None, 17)])
    run_rows(dev, (shape, "all bits band"), shape, full, [(cs["banded"], None, 17)], slot=cs["slot"])


def test_rows_empty(dev):
    shape = (4, 5, 6)
    cs = PC.coarsen_case(shape, 8, 95)
    children = PC.coarsen_ref(cs["dist"], cs["valid"])["children"]
    got = rows_once(dev, shape, children, [(flat_rows(cs), cs["fill"], 8)], voxels=np.zeros(0, np.int32))
    assert got[0][0].shape == (0, 8) and got[1].shape == (0,)
    got = run_rows(dev, "empty band", shape, children, [(None, cs["fill"], 8)], slot="empty")
    assert (got[1] == 0).all() and (got[0][0] == cs["fill"]).all()
    got, again = rows_once(dev, shape, children, []), rows_once(dev, shape, children, [])
    want = PC.rows_ref(children, shape, np.zeros(shape + (1,), np.float32))[1]
    same_bytes(got[1], want, "no set: known")
    same_bytes(again[1], want, "no set: known, second run")


# ---- BakedField.coarsen / pyramid ---------------------------------------------------------------------------------------------------
def field_of(dev, dist, valid, rows, step=0.01, origin=(0.1, -0.2, 0.3)):
    return BakedField.from_arrays(origin, step, up(dev, dist, np.float32), up(dev, np.asarray(valid) != 0), feats=up(dev, rows, np.float32))


def check_coarse(fine, coarse, mc, what):
    """a coarsened field against the restatement fed with the fine field's own arrays (and slots: the band of either is the library's)"""
    shape = tuple(fine.grid_shape)
    ref = PC.coarsen_ref(fine.dist.cpu().numpy(), fine.valid.cpu().numpy(), mc)
    same_bytes(coarse.dist.cpu().numpy(), ref["dist"], (what, "dist"))
    same_bytes(coarse.valid.cpu().numpy(), ref["valid"] != 0, (what, "valid"))
    same_bytes(coarse.children.cpu().numpy(), ref["children"], (what, "children"))
    assert tuple(coarse.grid_shape) == PC.coarse_shape(shape) and coarse.step == 2 * fine.step
    assert coarse.origin == tuple(o + fine.step / 2 for o in fine.origin)
    rows = fine._sets["feats"].cpu().numpy()
    slot = None if fine.band is None else fine.slot.cpu().numpy()
    voxels = None if coarse.band is None else coarse.band_voxels.cpu().numpy()
    want, known = PC.rows_ref(ref["children"], shape, rows, voxels=voxels, slot=slot)
    have = coarse._sets["feats"].cpu().numpy()
    assert coarse._sets["feats"].dtype == torch.float32 and PC.same_rows(have.reshape(want.shape), want), what
    same_bytes(coarse.rows_known.cpu().numpy().reshape(-1), known != 0, (what, "rows_known"))


def smooth_field(dev, shape=(24, 20, 28), C=8, seed=7):
    rng = np.random.default_rng(seed)
    pos = np.stack(np.indices(shape), -1).astype(np.float64)
    dist = (0.01 * (np.linalg.norm(pos - np.array(shape) / 2.0, axis=-1) - 5.0)).astype(np.float32)
    valid = rng.random(shape) < 0.9
    return field_of(dev, dist, valid, rng.standard_normal(shape + (C,)).astype(np.float32))


def test_api_coarsen(dev):
    f = smooth_field(dev)
    assert f.children is None
    dense = f.coarsen()
    assert dense.band is None
    check_coarse(f, dense, 1, "dense -> dense")
    check_coarse(f, f.coarsen(min_children=8), 8, "min_children 8")
    banded = f.coarsen(band=0.012)
    assert banded.band == 0.012 and 0 < banded.band_voxels.shape[0] < dense.dist.numel()
    check_coarse(f, banded, 1, "dense -> band")
    fb = f.to_band(0.02)
    bb = fb.coarsen(min_children=2)
    assert bb.band == fb.band and bb.band_voxels.shape[0] > 0
    check_coarse(fb, bb, 2, "band -> band")
    check_coarse(fb, fb.coarsen(band=0.05), 1, "band -> another band")
    half = f.half()
    check_coarse(half, half.coarsen(), 1, "half -> float32")
    check_coarse(fb.half(), fb.half().coarsen(), 1, "banded half -> float32")
    # the result is an ordinary field
    pts = torch.tensor([[0.16, -0.15, 0.37], [0.155, -0.14, 0.36]], dtype=torch.float32, device=dev)
    for field in (dense, banded, bb):
        out = field.eval(pts, return_names=["feats"])
        assert out["feats"].shape == (2, 8) and out["dist"].shape == (2,)
    levels = f.pyramid(2)
    assert levels[0] is f and [tuple(l.grid_shape) for l in levels] == [(24, 20, 28), (12, 10, 14), (6, 5, 7)]
    check_coarse(levels[0], levels[1], 1, "pyramid 1")
    check_coarse(levels[1], levels[2], 1, "pyramid 2")
    with pytest.raises(ValueError, match=r"0\.\.4\b"):
        f.pyramid(5)


# ---- the seeded flow --------------------------------------------------------------------------------------------------------------
def upload_rows(dev, rows, stride, shift):
    """rows [.., C] -> (buffer, data pointer): rows `stride` floats apart, `shift` floats into a 16-byte aligned buffer, NaN between and behind"""
    C = rows.shape[-1]
    flat = np.array(rows, np.float32).reshape(-1, C)
    buf = torch.full((shift + max(len(flat), 1) * stride + 4,), float("nan"), dtype=torch.float32, device=dev)
    if len(flat):
        buf[shift:shift + len(flat) * stride].view(len(flat), stride)[:, :C] = torch.from_numpy(flat).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * shift


def launch(dev, member_a, rows_a, member_b, rows_b, r, max_cost2, seed="none", slot_a=None, slot_b=None, stride=None, shift=0, axis=True, entry="seeded"):
    """entry "seeded": d3f_volume_flow_seeded with seed None (NULL) or an int32 [.., 3] array; entry "flow": the device's own d3f_volume_flow"""
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
    target, cost = poisoned(dev, (nx, ny, nz), torch.int32), poisoned(dev, (nx, ny, nz), torch.float32)
    ax = poisoned(dev, (nx, ny, nz, 6), torch.float32) if axis else None
    sa, sb = (_lib.VolumeSet * 1)(_lib.VolumeSet(ptr_a, C, 0, stride, None)), (_lib.VolumeSet * 1)(_lib.VolumeSet(ptr_b, C, 0, stride, None))
    if entry == "flow":
        _lib.check(lib.d3f_volume_flow(_lib.ptr(site_a), _lib.ptr(sl_a), sa, _lib.ptr(site_b), _lib.ptr(sl_b), sb, nx, ny, nz, r, float(max_cost2), _lib.ptr(target),
                                       _lib.ptr(cost), _lib.ptr(ax), _lib.current_stream_handle(dev)))
        torch.cuda.synchronize()
    else:
        sd = None if seed is None else up(dev, seed, np.int32)
        call(dev, "d3f_volume_flow_seeded", _lib.FlowSeeded(_lib.ptr(site_a), _lib.ptr(sl_a), sa, _lib.ptr(site_b), _lib.ptr(sl_b), sb, _lib.ptr(sd), nx, ny, nz, r,
                                                            float(max_cost2), 0, _lib.ptr(target), _lib.ptr(cost), _lib.ptr(ax)))
    return {"target": target.cpu().numpy(), "cost": cost.cpu().numpy(), "axis_cost": ax.cpu().numpy() if axis else None}


def run_seeded(dev, *args, **kw):
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


def poison_behind(member_a, seed):
    """`seed` with 0xA5 bytes behind every non-member of A"""
    out = np.array(seed, np.int32, order="C")        # (a copy: a broadcast seed has strides of zero)
    out.view(np.uint8).reshape(member_a.shape + (12,))[~np.asarray(member_a, bool)] = POISON
    return out


@pytest.mark.parametrize("shape", FC.TILE_SHAPES + [(3, 4, 130)], ids=str)
def test_zero_seed_is_the_flow(dev, shape):
    """seed NULL and seed all zero == the device's own d3f_volume_flow == the restatement, r = 1..4"""
    for r in (1, 2, 3, 4):
        for density, kind, C in ((0.9, "gauss", 4), (0.3, "int", 3)):
            case = FC.random_case(shape, C, 400 + r, density, kind)
            ref = FC.random_reference(shape, C, 400 + r, density, kind, r)
            own = launch(dev, *case, r, INF, entry="flow")
            same(own, ref, (shape, r, density, "d3f_volume_flow"))
            same(run_seeded(dev, *case, r, INF, seed=None), own, (shape, r, density, "seed NULL"))
            same(run_seeded(dev, *case, r, INF, seed=poison_behind(case[0], np.zeros(shape + (3,), np.int32))), own, (shape, r, density, "seed zero"))


@pytest.mark.parametrize("C", FC.CHANNELS)
def test_zero_seed_channels(dev, C):
    """Gaussian rows on both load paths: the chain of one lane per candidate has the bits of the LDS-staged one"""
    shape = FC.CHANNEL_SHAPE
    case = FC.random_case(shape, C, 300 + C, 0.9, "gauss")
    ref = FC.random_reference(shape, C, 300 + C, 0.9, "gauss", 2)
    sd = PC.random_seed(shape, 500 + C)
    want = PC.flow_seeded_ref(*case, sd, 1, INF)
    assert (want["target"] >= 0).sum() > 50
    for stride, shift in ((C, 0), (C + 4, 0), (C + 3, 1)):           # plain and padded rows (vector where C % 4 == 0); odd stride off 16 bytes: scalar
        same(run_seeded(dev, *case, 2, INF, seed=None, stride=stride, shift=shift), ref, (C, stride, shift))
        same(run_seeded(dev, *case, 1, INF, seed=poison_behind(case[0], sd), stride=stride, shift=shift), want, (C, stride, shift, "seeded"))


def test_seeded_finds_a_planted_shift(dev):
    shift = (5, -6, 7)
    ma, ra, mb, rb, moved = FC.shifted_copy((8, 9, 10), 6, 21, 0.85, shift)
    seed = np.broadcast_to(np.array(shift, np.int32), ma.shape + (3,))
    for r in (1, 2):
        got = run_seeded(dev, ma, ra, mb, rb, r, INF, seed=poison_behind(ma, seed))
        same(got, PC.flow_seeded_ref(ma, ra, mb, rb, seed, r, INF), ("shifted copy", r))
        assert moved.sum() > 5 and (FC.voxel_offsets(got["target"])[moved] == np.array(shift)).all() and (got["cost"][moved] == 0).all()


@pytest.mark.parametrize("shape", [(5, 5, 17), (9, 4, 33), (3, 4, 130), (1, 1, 1)], ids=str)
def test_seeded_random_seeds(dev, shape):
    """per-voxel seeds in [-6, 6]: windows partly and wholly outside the volume; a seed out of range on members; 0xA5 behind non-members"""
    sd = PC.random_seed(shape, 600)
    for r in (1, 2, 3, 4):
        for density, kind, C in ((0.9, "gauss", 4), (0.4, "int", 3)):
            case = FC.random_case(shape, C, 700 + r, density, kind)
            want = PC.flow_seeded_ref(*case, sd, r, INF)
            same(run_seeded(dev, *case, r, INF, seed=poison_behind(case[0], sd)), want, (shape, r, density))
    case = FC.random_case(shape, 4, 701, 0.9, "gauss")
    far = np.array(sd)
    members = np.argwhere(case[0])
    for k, at in enumerate(members[::3]):
        far[tuple(at)] = [(PC.SEED_MAX + 1, 0, 0), (0, -PC.SEED_MAX - 1, 0), (0, 0, 2 ** 31 - 1), (-2 ** 31, -2 ** 31, -2 ** 31), (PC.SEED_MAX, 0, 0), (0, -40, 0)][k % 6]
    want = PC.flow_seeded_ref(*case, far, 2, INF)
    same(run_seeded(dev, *case, 2, INF, seed=poison_behind(case[0], far)), want, (shape, "out of range"))
    if len(members):
        assert want["target"][tuple(members[0])] == -1 and want["cost"][tuple(members[0])] == np.inf


def test_seeded_ties_and_threshold(dev):
    """every candidate ties in s = 0: d2, then j, about the SEEDED centre decide; max_cost2 at a winner's s, one ulp below, +Inf"""
    ma, ra, mb, rb, hole = FC.identical_b()
    shape = ma.shape
    sd = PC.random_seed(shape, 800, -2, 2)
    for r in (1, 2, 3):
        want = PC.flow_seeded_ref(ma, ra, mb, rb, sd, r, INF)
        got = run_seeded(dev, ma, ra, mb, rb, r, INF, seed=sd)
        same(got, want, ("ties", r))
        centre = np.stack(np.indices(shape), -1) + sd
        inside = ((centre >= 0) & (centre < np.array(shape))).all(-1)
        at = inside & mb[tuple(np.where(inside[..., None], centre, 0).transpose(3, 0, 1, 2))]
        assert at.sum() > 20 and (FC.voxel_offsets(got["target"])[at] == sd[at]).all()             # the seeded centre itself wins where it is a member of B
    case = FC.random_case((5, 6, 18), 5, 810, 0.9, "gauss")
    sd = PC.random_seed((5, 6, 18), 811, -1, 1)
    free = PC.flow_seeded_ref(*case, sd, 2, INF)
    s = np.sort(free["cost"][free["target"] >= 0])[len(free["cost"][free["target"] >= 0]) // 2]
    for bound in (s, np.nextafter(s, np.float32(0)), np.float32(np.inf), np.float32(0)):
        want = PC.flow_seeded_ref(*case, sd, 2, bound)
        same(run_seeded(dev, *case, 2, bound, seed=sd), want, ("threshold", float(bound)))
    at_s, below = PC.flow_seeded_ref(*case, sd, 2, s), PC.flow_seeded_ref(*case, sd, 2, np.nextafter(s, np.float32(0)))
    assert (at_s["cost"] == s).any() and not (below["cost"] == s).any()


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_seeded_band(dev, which):
    shape = (5, 6, 18)
    ma, ra, mb, rb = FC.random_case(shape, 8, 820, 0.9, "gauss")
    sd = PC.random_seed(shape, 821, -3, 3)
    slot_a, comp_a = FC.band_of(ma, ra, 822) if which in ("a", "both") else (None, ra)
    slot_b, comp_b = FC.band_of(mb, rb, 823) if which in ("b", "both") else (None, rb)
    mem_a, mem_b = FC.members_of(ma, slot_a), FC.members_of(mb, slot_b)
    for axis in (True, False):
        want = PC.flow_seeded_ref(mem_a, ra, mem_b, rb, sd, 2, INF, axis=axis)
        got = run_seeded(dev, ma, comp_a, mb, comp_b, 2, INF, seed=poison_behind(mem_a, sd), slot_a=slot_a, slot_b=slot_b, axis=axis)
        same(got, want, (which, axis))
        assert (got["axis_cost"] is None) == (not axis)


def test_seeded_empty(dev):
    shape = (5, 6, 18)
    ma, ra, mb, rb = FC.random_case(shape, 4, 830, 0.9, "gauss")
    sd = PC.random_seed(shape, 831)
    none = np.zeros(shape, bool)
    for a, b in ((none, mb), (ma, none), (none, none)):
        got = run_seeded(dev, a, ra, b, rb, 1, INF, seed=poison_behind(a, sd))
        same(got, PC.flow_seeded_ref(a, ra, b, rb, sd, 1, INF), "empty")
        assert (got["target"] == -1).all() and np.isinf(got["cost"]).all() and np.isinf(got["axis_cost"]).all()


# ---- BakedField.flow(seed=), Flow.seed, flow_pyramid ----------------------------------------------------------------------------------
def level_arrays(field):
    rows = field._sets["feats"].cpu().numpy()
    slot = None
    if field.band is not None:
        slot = field.slot.cpu().numpy()
        dense = np.zeros(tuple(field.grid_shape) + (rows.shape[-1],), np.float32)
        dense.reshape(-1, rows.shape[-1])[field.band_voxels.cpu().numpy()] = rows
        rows = dense
    return (field.dist.cpu().numpy(), field.valid.cpu().numpy(), rows), slot


def check_flow(flow, ref, what):
    same({"target": flow.target.cpu().numpy(), "cost": flow.cost.cpu().numpy(), "axis_cost": None if flow.axis_cost is None else flow.axis_cost.cpu().numpy()}, ref, what)


@pytest.mark.parametrize("banded", [False, True], ids=["dense", "banded"])
def test_api_chain(dev, banded):
    sc = PC.scene()
    unit = np.float32(0.01 if banded else 1.0)       # banded: distances of one voxel (the step), so that a band of 1.5 voxels holds the objects' surfaces
    a, b = field_of(dev, sc["dist_a"] * unit, sc["valid_a"], sc["rows_a"]), field_of(dev, sc["dist_b"] * unit, sc["valid_b"], sc["rows_b"])
    if banded:
        a, b = a.to_band(0.015), b.to_band(0.015)
        assert a.band_voxels.shape[0] > 0 and b.band_voxels.shape[0] > 0
    out = a.flow_pyramid(b, "feats")
    assert isinstance(out, Flow) and len(out.coarse) == 2 and [tuple(f.grid_shape) for f in out.coarse] == [(6, 6, 6), (12, 12, 12)]
    if banded:
        pa, pb = a.pyramid(2, return_names=["feats"]), b.pyramid(2, return_names=["feats"])
        la, lb = [level_arrays(f) for f in pa], [level_arrays(f) for f in pb]
        flows = PC.chain_ref([l[0] for l in la], [l[0] for l in lb], slots_a=[l[1] for l in la], slots_b=[l[1] for l in lb])
    else:
        flows = PC.scene_chain()[2]
        assert PC.on_shift(out.target.cpu().numpy(), sc["sphere_a"], PC.SCENE_SHIFT) == 405
    for lv, (have, want) in enumerate(zip(out.coarse + [out], flows)):
        check_flow(have, want, ("flow_pyramid", banded, lv))
    # the pieces by hand: Flow.seed against its restatement, flow(seed=) against the seeded restatement, seed=None the same call as ever
    top = out.coarse[0]
    seed = top.seed((12, 12, 12))
    assert seed.dtype == torch.int32 and seed.device == a.device
    same_bytes(seed.cpu().numpy(), PC.seed_ref(flows[0]["target"], flows[0]["cost"], flows[0]["axis_cost"], (12, 12, 12)), "Flow.seed")
    same_bytes(top.seed((12, 12, 12), refined=False).cpu().numpy(), PC.seed_ref(flows[0]["target"], flows[0]["cost"], None, (12, 12, 12)), "Flow.seed unrefined")
    zero = torch.zeros(tuple(a.grid_shape) + (3,), dtype=torch.int32, device=dev)
    plain, seeded = a.flow(b, "feats", radius_voxels=1), a.flow(b, "feats", radius_voxels=1, seed=zero)
    for k in ("target", "cost", "axis_cost", "offset"):
        same_bytes(getattr(seeded, k).cpu().numpy(), getattr(plain, k).cpu().numpy(), ("flow(seed=0)", k))
    back = b.flow_pyramid(a, "feats", refine=False, fine_radius_voxels=2)
    assert back.axis_cost is None and out.consistent(back).any() and out.displacement().shape == (24, 24, 24, 3)
