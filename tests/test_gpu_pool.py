"""Per-component pooling on the device (d3f_volume_pool, csrc/pool_kernels.hip; BakedField.pool) against the NumPy restatement of
tests/pool_cases.py: mean rows bit for bit (the summation order is part of the contract), counts, votes and moments exactly.

What each assert is there to catch:
  a member list that is not in ascending flat index per component, a chunk that straddles components     the bits of the means
  a level that re-adds a finished row, a ragged chunk dropped, a partial row misplaced                    "three levels", "256 and 257"
  a sum that starts from +0.0 instead of from the first row                                               all -0.0 rows pool to -0.0
  a result that depends on the order in which anything lands                                              two launches give identical bytes
  a workspace word or an output the kernels do not write before reading                                   everything is poisoned with 0xA5
  a label outside 1..K used as an index                                                                   "foreign": -1, K + 1, INT32_MIN
  a vector path that differs from the scalar one                                                          stride > C, a base off by one float
  a sort pass too few                                                                                     "K 300" (two digits)
"""
import ctypes

import numpy as np
import pytest
import torch

import band_cases as BC
import pool_cases as PC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

MEAN, VOTES = _lib.POOL_MEAN, _lib.POOL_VOTES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(nbytes, dev):
    return torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)


def upload_rows(rows, dev, shift=0):
    """a [R, C] view of a [R, stride] array -> (device buffer, address of row 0, stride); shift: floats the base is moved off its alignment"""
    base = rows if rows.base is None else rows.base
    assert base.ndim == 2 and base.flags["C_CONTIGUOUS"] and rows.strides[1] == 4
    buf = torch.empty(base.size + shift + 4, dtype=torch.float32, device=dev)
    buf[shift:shift + base.size] = torch.from_numpy(np.array(base)).reshape(-1).to(dev)
    return buf, buf.data_ptr() + 4 * shift, base.shape[1]


def run_pool(dev, label, K, sets=(), valid=None, slot=None, cap=None, want_moments=True, shift_out=0):
    """one d3f_volume_pool launch on freshly poisoned outputs and workspace.  sets: (rows [R, C] view, mode, fill or None, shift) tuples
    -> {'members', 'count', 'moments', 'rows': [...], 'bytes': every output as one byte string}"""
    lib = _lib.load()
    nx, ny, nz = label.shape
    lab = torch.from_numpy(np.array(label)).to(dev)
    val = None if valid is None else torch.from_numpy(np.array(valid, dtype=np.uint8)).to(dev)
    slt = None if slot is None else torch.from_numpy(np.array(slot, dtype=np.int32)).to(dev)
    if cap is None:
        cap = int(PC.counts_ref(label, K, valid, slot).sum())
    hold, arr = [], (_lib.VolumeSet * max(len(sets), 1))()
    modes = (ctypes.c_int32 * max(len(sets), 1))()
    outs = (ctypes.c_void_p * max(len(sets), 1))()
    out_bufs, mean_channels = [], 0
    for s, (rows, mode, fill, shift) in enumerate(sets):
        buf, addr, stride = upload_rows(rows, dev, shift)
        f = None if fill is None else torch.from_numpy(np.asarray(fill, np.float32)).to(dev)
        hold += [buf, f]
        C = rows.shape[1]
        arr[s] = _lib.VolumeSet(addr, C, 0, stride, _lib.ptr(f))
        modes[s] = mode
        ob = poisoned(4 * K * C + 4 * shift_out + 16, dev)
        out_bufs.append((ob, C, mode))
        outs[s] = ob.data_ptr() + 4 * shift_out
        mean_channels += C if mode == MEAN else 0
    members = poisoned(8, dev)
    count = poisoned(4 * K, dev)
    moments = poisoned(72 * K, dev) if want_moments else None
    ws_bytes = lib.d3f_volume_pool_workspace_bytes(nx, ny, nz, K, cap, mean_channels)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws = poisoned(ws_bytes, dev)
    _lib.check(lib.d3f_volume_pool(_lib.ptr(lab), nx, ny, nz, K, _lib.ptr(val), _lib.ptr(slt), arr, len(sets), modes, cap, _lib.ptr(members), _lib.ptr(count),
                                   _lib.ptr(moments), outs, _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    got = {"members": int(members[:8].view(torch.int64).item()), "count": count[:4 * K].view(torch.int32).cpu().numpy(),
           "moments": None if moments is None else moments[:72 * K].view(torch.int64).view(K, 9).cpu().numpy(), "rows": [], "poison_count": count.cpu().numpy()}
    for ob, C, mode in out_bufs:
        body = ob[4 * shift_out:4 * shift_out + 4 * K * C].cpu().numpy()
        got["rows"].append(body.view(np.float32 if mode == MEAN else np.int32).reshape(K, C))
        assert (ob[4 * shift_out + 4 * K * C:].cpu().numpy() == 0xA5).all(), "an output row beyond K was written"
    got["bytes"] = b"".join(np.ascontiguousarray(a).tobytes() for a in [got["count"]] + ([] if moments is None else [got["moments"]]) + got["rows"])
    return got


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check(got, label, K, sets, valid=None, slot=None, what=None):
    counts = PC.counts_ref(label, K, valid, slot)
    assert got["members"] == int(counts.sum()), (what, got["members"])
    assert np.array_equal(got["count"], counts), what
    if got["moments"] is not None:
        assert np.array_equal(got["moments"], PC.moments_ref(label, K, valid, slot)), what
    for s, (rows, mode, fill, _) in enumerate(sets):
        if mode == MEAN:
            want = PC.pool_ref(label, K, rows, valid, slot, fill)
            bad = np.argwhere(got["rows"][s].view(np.int32) != want.view(np.int32))
            assert same_bits(got["rows"][s], want), (what, s, len(bad), bad[:4].tolist())
        else:
            assert np.array_equal(got["rows"][s], PC.votes_ref(label, K, rows, valid, slot)), (what, s)


# ---- bits, on every label volume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.VOLUMES))
def test_means_counts_votes_and_moments_equal_the_restatement(dev, name):
    label, K = PC.volume(name)
    n = label.size
    sets = [(PC.field_rows(n, 8, 31), MEAN, None, 0), (PC.field_rows(n, 5, 32), MEAN, None, 0), (PC.vote_rows(n, 6, 33), VOTES, None, 0)]
    got = run_pool(dev, label, K, sets)
    check(got, label, K, sets, what=name)
    again = run_pool(dev, label, K, sets)
    assert got["bytes"] == again["bytes"], (name, "two launches differ")


def test_three_levels_with_room_to_spare(dev):
    """65537 members -> 257 partial rows -> 2 -> 1; a capacity above the voxel count changes nothing"""
    label, K = PC.volume("three levels")
    sets = [(PC.field_rows(label.size, 4, 34), MEAN, None, 0)]
    assert PC.fold_levels(65537) == 3
    a = run_pool(dev, label, K, sets)
    check(a, label, K, sets, what="exact capacity")
    for cap in (label.size, (1 << 24) + 5):
        assert a["bytes"] == run_pool(dev, label, K, sets, cap=cap)["bytes"], cap
    # levels the capacity allows and no component needs: 630 members allow two, no component of this volume has more than 256
    small, Ks = PC.volume("9x8x10")
    sets = [(PC.field_rows(small.size, 4, 36), MEAN, None, 0)]
    assert PC.counts_ref(small, Ks).max() <= 256 < PC.counts_ref(small, Ks).sum()
    check(run_pool(dev, small, Ks, sets), small, Ks, sets, what="a spare level")


def test_no_components(dev):
    label, _ = PC.volume("9x8x10")
    got = run_pool(dev, label, 0, [(PC.field_rows(label.size, 4, 35), MEAN, None, 0)])
    assert got["members"] == 0 and got["count"].size == 0 and got["rows"][0].shape == (0, 4)
    assert (got["poison_count"] == 0xA5).all()
    got = run_pool(dev, label, 0, [], want_moments=False, cap=0)
    assert got["members"] == 0


# ---- channels and layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", PC.CHANNELS)
def test_channel_counts(dev, C):
    for name in ("9x8x10", "256 and 257"):
        label, K = PC.volume(name)
        sets = [(PC.field_rows(label.size, C, 100 + C), MEAN, PC.field_rows(1, C, 7)[0], 0)]
        check(run_pool(dev, label, K, sets), label, K, sets, what=(name, C))


@pytest.mark.parametrize("name", ["2x3x33", "65x3x67", "256 and 257"])
def test_strides_offsets_and_several_sets(dev, name):
    label, K = PC.volume(name)
    n = label.size
    wide = PC.field_rows(n, 64, 41, stride=72)                   # stride > C, still a multiple of 4: the vector path
    odd = PC.field_rows(n, 64, 42, stride=67)                    # a stride that is no multiple of 4: the scalar path
    assert wide.strides[0] == 288 and odd.strides[0] == 268
    plain = PC.field_rows(n, 64, 43)
    votes = PC.vote_rows(n, 8, 44)
    sets = [(wide, MEAN, None, 0), (votes, VOTES, None, 0), (odd, MEAN, None, 0)]
    check(run_pool(dev, label, K, sets), label, K, sets, what="strides")
    # the same rows from a base moved by one float (scalar path) give the bits of the aligned base (vector path); so does an output off by one float
    aligned = run_pool(dev, label, K, [(plain, MEAN, None, 0), (votes, VOTES, None, 0)])
    shifted = run_pool(dev, label, K, [(plain, MEAN, None, 1), (votes, VOTES, None, 1)])
    out_shifted = run_pool(dev, label, K, [(plain, MEAN, None, 0), (votes, VOTES, None, 0)], shift_out=1)
    check(aligned, label, K, [(plain, MEAN, None, 0), (votes, VOTES, None, 0)], what="aligned")
    assert aligned["bytes"] == shifted["bytes"] == out_shifted["bytes"]


# ---- membership -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["foreign", "65x3x67"])
def test_valid_and_slot_volumes(dev, name):
    label, K = PC.volume(name)
    n = label.size
    rng = np.random.default_rng(50)
    valid = (rng.random(label.shape) < 0.8) * rng.integers(1, 256, label.shape)      # any non-zero byte is valid
    keep = rng.random(n) < 0.6
    M = int(keep.sum())
    ascending = np.full(n, -1, dtype=np.int32)
    ascending[keep] = np.arange(M, dtype=np.int32)
    permuted = np.full(n, -1, dtype=np.int32)
    permuted[keep] = rng.permutation(M).astype(np.int32)
    dense = [(PC.field_rows(n, 12, 51), MEAN, None, 0), (PC.vote_rows(n, 5, 52), VOTES, None, 0)]
    dense[0][0][valid.reshape(-1) == 0] = np.nan                                 # an invalid voxel's row is never read
    check(run_pool(dev, label, K, dense, valid=valid), label, K, dense, valid=valid, what="valid")
    rows = [(PC.field_rows(M, 12, 53), MEAN, None, 0), (PC.vote_rows(M, 5, 54), VOTES, None, 0)]
    for slot in (ascending, permuted):
        slot = slot.reshape(label.shape)
        check(run_pool(dev, label, K, rows, slot=slot), label, K, rows, slot=slot, what="slot")
        check(run_pool(dev, label, K, rows, valid=valid, slot=slot), label, K, rows, valid=valid, slot=slot, what="valid and slot")


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def test_negative_zero_rows_pool_to_negative_zero(dev):
    for name in ("9x8x10", "256 and 257", "three levels"):
        label, K = PC.volume(name)
        rows = np.full((label.size, 4), -0.0, dtype=np.float32)
        got = run_pool(dev, label, K, [(rows, MEAN, None, 0)])["rows"][0]
        assert np.signbit(got).all() and (got == 0).all(), name


def test_empty_components_get_the_fill_row_or_zeros(dev):
    label, K = PC.volume("gaps")
    n = label.size
    fill = np.array([1.5, -2.0, 3.25, -0.0, 7.0], dtype=np.float32)
    sets = [(PC.field_rows(n, 5, 61), MEAN, fill, 0), (PC.field_rows(n, 8, 62), MEAN, None, 0), (PC.vote_rows(n, 4, 63), VOTES, None, 0)]
    got = run_pool(dev, label, K, sets)
    check(got, label, K, sets, what="gaps")
    empty = [1, 4, 5, 8]
    assert (got["count"][empty] == 0).all() and (got["moments"][empty] == 0).all() and (got["rows"][2][empty] == 0).all()
    assert all(same_bits(got["rows"][0][k], fill) for k in empty) and (got["rows"][1][empty].view(np.int32) == 0).all()
    # all components empty: a valid volume of zeros
    got = run_pool(dev, label, K, sets, valid=np.zeros(label.shape, np.uint8))
    assert got["members"] == 0 and (got["count"] == 0).all() and all(same_bits(r, fill) for r in got["rows"][0]) and (got["moments"] == 0).all()


@pytest.mark.parametrize("C", PC.VOTE_CHANNELS)
def test_votes_with_exact_ties_and_nans(dev, C):
    for name in ("9x8x10", "256 and 257"):
        label, K = PC.volume(name)
        rows = PC.vote_rows(label.size, C, 70 + C)
        sets = [(rows, VOTES, None, 0), (rows, VOTES, None, 1)]
        got = run_pool(dev, label, K, sets)
        check(got, label, K, sets, what=(name, C))
        assert got["rows"][0].sum(axis=1).tolist() == got["count"].tolist()


def test_moments_on_the_longest_axis(dev):
    rng = np.random.default_rng(80)
    label = rng.integers(0, 4, size=(16384, 1, 2)).astype(np.int32)
    label[16000:] = 2                                                # the far end, where x * x is largest
    got = run_pool(dev, label, 3, [])
    check(got, label, 3, [], what="16384x1x2")
    assert got["moments"][1, 3] > 2 ** 36
    swapped = np.ascontiguousarray(label.reshape(2, 1, 16384))
    check(run_pool(dev, swapped, 3, []), swapped, 3, [], what="2x1x16384")


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def test_member_capacity(dev):
    label, K = PC.volume("65x3x67")
    sets = [(PC.field_rows(label.size, 8, 90), MEAN, None, 0), (PC.vote_rows(label.size, 3, 91), VOTES, None, 0)]
    counts = PC.counts_ref(label, K)
    members = int(counts.sum())
    for cap in (0, members - 1, members, members + 3):
        got = run_pool(dev, label, K, sets, cap=cap)
        assert got["members"] == members and np.array_equal(got["count"], counts), cap
        if cap >= members:
            check(got, label, K, sets, what=cap)


# ---- BakedField.pool ----------------------------------------------------------------------------------------------------------------------
def geometry_ref(moments, counts, origin, step):
    """centroid and covariance by the float64 formulas"""
    with np.errstate(invalid="ignore", divide="ignore"):
        m, n = moments.astype(np.float64), counts.astype(np.float64)[:, None]
        mean = m[:, :3] / n
        second = m[:, [3, 4, 5, 4, 6, 7, 5, 7, 8]].reshape(-1, 3, 3) / n[:, :, None]
        centroid = np.asarray(origin, np.float64) + float(step) * mean
        cov = (second - mean[:, :, None] * mean[:, None, :]) * (float(step) * float(step))
    return centroid.astype(np.float32), cov.astype(np.float32)


def check_field_pool(out, field, label, K, names, votes):
    """BakedField.pool against the NumPy composition on the field's own tensors"""
    valid = field.valid.cpu().numpy()
    slot = None if field.band is None else field.slot.cpu().numpy()
    counts = PC.counts_ref(label, K, valid, slot)
    moments = PC.moments_ref(label, K, valid, slot)
    assert out["count"].dtype == torch.int32 and np.array_equal(out["count"].cpu().numpy(), counts)
    assert out["moments"].dtype == torch.int64 and np.array_equal(out["moments"].cpu().numpy(), moments)
    centroid, cov = geometry_ref(moments, counts, field.origin, field.step)
    assert out["centroid"].dtype == out["covariance"].dtype == torch.float32
    assert tuple(out["centroid"].shape) == (K, 3) and tuple(out["covariance"].shape) == (K, 3, 3)
    np.testing.assert_allclose(out["centroid"].cpu().numpy(), centroid, rtol=1e-6, atol=0, equal_nan=True)
    np.testing.assert_allclose(out["covariance"].cpu().numpy(), cov, rtol=1e-6, atol=1e-12, equal_nan=True)
    assert np.isnan(out["centroid"].cpu().numpy()[counts == 0]).all() and np.isnan(out["covariance"].cpu().numpy()[counts == 0]).all()
    assert not np.isnan(out["centroid"].cpu().numpy()[counts > 0]).any()
    for k in names:
        rows = field._sets[k].reshape(-1, field._sets[k].shape[-1]).cpu().numpy()
        want = PC.pool_ref(label, K, rows, valid, slot, field.fill_row(k).cpu().numpy())
        assert not out[k].requires_grad and same_bits(out[k].cpu().numpy(), want), k
    for k in votes:
        rows = field._sets[k].reshape(-1, field._sets[k].shape[-1]).cpu().numpy()
        assert out[k + "_votes"].dtype == torch.int32 and np.array_equal(out[k + "_votes"].cpu().numpy(), PC.votes_ref(label, K, rows, valid, slot)), k
    assert set(out) == {"count", "moments", "centroid", "covariance"} | set(names) | {k + "_votes" for k in votes}


@pytest.mark.parametrize("name", ["large sphere holes band 1h", "large plane holes band 0.5h"])
def test_field_pool_equals_the_composition(dev, name):
    from d3fields_amd import BakedField
    vol = BC.volume(name, channels=(16, 3), fills=(0,))
    assert not vol["valid"].all()
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()}
    fills = {k: torch.from_numpy(v).to(dev) for k, v in vol["fills"].items() if v is not None}
    f = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                               fills=fills, **sets)
    mask = np.random.default_rng(5).random(vol["shape"]) < 0.2                   # many small components ...
    for x, y, z in np.argwhere(~vol["valid"])[:5]:                               # ... some of them a single invalid voxel: no member
        mask[max(x - 1, 0):x + 2, max(y - 1, 0):y + 2, max(z - 1, 0):z + 2] = False
        mask[x, y, z] = True
    comp = f.components(sites=torch.from_numpy(mask).to(dev), connectivity=6)
    label, K = comp.labels.cpu().numpy(), comp.count
    assert K > 10
    out = f.pool(comp, votes=["s1"])
    check_field_pool(out, f, label, K, ["s0", "s1"], ["s1"])
    assert (out["count"].cpu().numpy() == 0).any(), "a component without a valid voxel is part of the case"
    check_field_pool(f.pool(comp.labels, return_names=["s1"], count=K), f, label, K, ["s1"], [])
    check_field_pool(f.pool(comp, return_names=[]), f, label, K, [], [])
    surface = f.components()                                                     # the field's own shell
    check_field_pool(f.pool(surface), f, surface.labels.cpu().numpy(), surface.count, ["s0", "s1"], [])
    b = f.to_band(float(BC.band_of(name)))
    assert 0 < b.band_voxels.numel() < mask.size
    check_field_pool(b.pool(comp, votes=["s0"]), b, label, K, ["s0", "s1"], ["s0"])
    empty = f.to_band(1e-9)                                                      # a band that stores nothing: fill rows, no members
    if empty.band_voxels.numel() == 0:
        check_field_pool(empty.pool(comp, votes=["s1"]), empty, label, K, ["s0", "s1"], ["s1"])
    c = f.clearance()                                                            # no sets: the count and the geometry
    check_field_pool(c.pool(comp), c, label, K, [], [])
    check_field_pool(f.pool(comp.labels, count=0), f, label, 0, ["s0", "s1"], [])


def test_field_pool_on_a_fused_bake(dev):
    """Four 48 x 64 views of the smooth synthetic scene, a 128-channel map and a mask-like map, baked dense and banded on a 24 x 20 x 16 grid"""
    from d3fields_amd import Fusion, synth
    V, H, W = 4, 48, 64
    sc = synth.make_scene(V, H, W, "smooth")
    feats = synth.random_map(V, 12, 16, 128, seed=4)
    mask = (synth.random_map(V, 12, 16, 1, seed=6) > 0).to(torch.float32)
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {"depth": sc["depth"].to(dev), "K": sc["K"].to(dev), "pose": sc["pose"].to(dev), "dino_feats": feats.to(dev), "mask": mask.to(dev)}
    f.H, f.W = H, W
    box = dict(x_lower=-0.1875, x_upper=0.1875, y_lower=-0.1875, y_upper=0.125, z_lower=-0.21875, z_upper=0.03125)
    names = ["dino_feats", "mask"]
    for band in (None, 0.012):
        field = f.bake(box, 2.0 ** -6, return_names=names, band=band)
        comp = field.components(connectivity=6)
        assert comp.count >= 1
        out = field.pool(comp, votes=["mask"])
        check_field_pool(out, field, comp.labels.cpu().numpy(), comp.count, names, ["mask"])
        assert int(out["count"].sum()) > 0


def test_field_pool_errors(dev):
    from d3fields_amd import BakedField
    vol = BC.volume("5x4x6 sphere band 1.5h")
    shape = tuple(vol["shape"])
    wide = torch.zeros(shape + (257,), device=dev)
    f = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                               wide=wide, thin=torch.ones(shape + (2,), device=dev))
    labels = torch.zeros(shape, dtype=torch.int32, device=dev)
    assert f.pool(labels, count=2)["count"].tolist() == [0, 0]
    other = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.zeros((6, 4, 6), device=dev))
    for args, kw in (((labels,), {}), ((labels,), {"count": -1}), ((labels,), {"count": 1.0}), ((labels,), {"count": True}), ((labels.long(),), {"count": 1}),
                     ((labels[:-1],), {"count": 1}), ((labels.cpu().numpy(),), {"count": 1}), ((None,), {}), ((other.components(),), {}),
                     ((f.components(),), {"count": 1}), ((labels,), {"count": labels.numel() + 1}), ((labels,), {"count": 1, "votes": ["wide"]})):
        with pytest.raises(ValueError):
            f.pool(*args, **kw)
    with pytest.raises(RuntimeError):
        f.pool(labels.cpu(), count=1)
    with pytest.raises(KeyError):
        f.pool(labels, count=1, return_names=["nope"])
    with pytest.raises(KeyError):
        f.pool(labels, count=1, votes=["nope"])
    clash = BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), count=torch.ones(shape + (2,), device=dev),
                                   thin=torch.ones(shape + (2,), device=dev), thin_votes=torch.ones(shape + (2,), device=dev))
    with pytest.raises(ValueError):
        clash.pool(labels, count=1)
    with pytest.raises(ValueError):
        clash.pool(labels, count=1, return_names=["thin", "thin_votes"], votes=["thin"])
    assert set(clash.pool(labels, count=1, return_names=["thin", "thin_votes"])) == {"count", "moments", "centroid", "covariance", "thin", "thin_votes"}
    pts = torch.zeros((4, 3), device=dev, requires_grad=True)
    out = f.pool(labels + 1, count=1, return_names=["thin"], votes=["thin"])
    assert not any(t.requires_grad for t in out.values()) and pts.grad is None
    assert out["thin_votes"].tolist() == [[int(vol["valid"].sum()), 0]] and out["count"].tolist() == [int(vol["valid"].sum())]
