"""Connected components on the device (d3f_volume_components, csrc/ccl_kernels.hip; BakedField.components / Components /
clearance(min_voxels=, sites=)) against the NumPy restatement of tests/ccl_cases.py: integer data, equality everywhere, no tolerance.

The contract, restated: two sites (non-zero bytes) are neighbours if their coordinates differ by at most 1 on every axis and by at most
1 / 2 / 3 in L1 for connectivity 6 / 18 / 26 -- spatially, never across the end of a line or a plane; a component's root is its smallest
flat index; the components with size >= min_voxels are numbered 1..K in ascending order of root; out_count = {K, found}; stats row k-1 =
{root, size, x0, y0, z0, x1, y1, z1} for k <= stats_capacity.

What each assert is there to catch:
  a union dropped or made across a wrap, a wrong skip of the "voxel below did it" rule     test_labels_counts_and_stats_equal_the_restatement
  a run that crosses a wave boundary or a line start                                        the 2x3x33 ... 2x3x130, nz = 1 / 5 / 64 / 300 cases
  a result that depends on the order in which atomics land                                  two launches give identical bytes
  a workspace word or an output the kernels do not write before reading                     everything is poisoned with 0xA5 before every launch
  >= against >, numbering that is not by root, found that follows min_voxels                test_min_voxels
  a stats row written beyond the capacity, a count that follows the capacity                test_stats_capacity
"""
import numpy as np
import pytest
import torch

import band_cases as BC
import ccl_cases as CC
import edt_cases as EC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

INT32_MAX = int(EC.INT32_MAX)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run_ccl(site, dev, connectivity, min_voxels=1, capacity=0):
    """one d3f_volume_components launch on freshly poisoned outputs and workspace -> (label, count [2], stats [capacity, 8] or None)"""
    lib = _lib.load()
    nx, ny, nz = site.shape
    s = torch.from_numpy(np.array(site)).to(dev)      # (a copy: the case arrays are read-only)
    poison = int(CC.POISON)
    label = torch.full((nx, ny, nz), poison, dtype=torch.int32, device=dev)
    count = torch.full((2,), poison, dtype=torch.int32, device=dev)
    stats = torch.full((capacity, 8), poison, dtype=torch.int32, device=dev) if capacity > 0 else None
    ws_bytes = lib.d3f_volume_components_workspace_bytes(nx, ny, nz)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_volume_components(_lib.ptr(s), nx, ny, nz, connectivity, min_voxels, _lib.ptr(label), _lib.ptr(count), _lib.ptr(stats), capacity,
                                         _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return label.cpu().numpy(), count.cpu().numpy(), None if stats is None else stats.cpu().numpy()


def check_against(ref, got, capacity, what):
    label, count, stats = got
    assert label.dtype == np.int32 and np.array_equal(label, ref["label"]), (what, int((label != ref["label"]).sum()))
    assert count.tolist() == [ref["K"], ref["found"]], (what, count.tolist())
    if capacity > 0:
        rows = min(capacity, ref["K"])
        assert np.array_equal(stats[:rows], ref["stats"][:rows]), what
        assert (stats[rows:] == CC.POISON).all(), (what, "a row at or beyond the capacity or K was written")


@pytest.mark.parametrize("name", CC.CASES)
def test_labels_counts_and_stats_equal_the_restatement(dev, name):
    site = CC.site_volume(name)
    for rank, conn in enumerate(CC.CONNECTIVITIES):
        ref = CC.reference(name, conn)
        if name in CC.EXPECTED:
            assert ref["found"] == CC.EXPECTED[name][rank]
        capacity = ref["K"] + 3
        got = run_ccl(site, dev, conn, capacity=capacity)
        check_against(ref, got, capacity, (name, conn))
        again = run_ccl(site, dev, conn, capacity=capacity)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), (name, conn, "two launches differ")


def test_any_non_zero_byte_is_a_site(dev):
    site = CC.site_volume("9x8x10 30%")
    assert len(np.unique(site)) > 3
    ref = CC.reference("9x8x10 30%", 18)
    for value in (1, 2, 128, 255):
        check_against(ref, run_ccl(((site != 0) * value).astype(np.uint8), dev, 18, capacity=ref["K"]), ref["K"], value)


@pytest.mark.parametrize("case", CC.MIN_VOXELS, ids=lambda c: "%s conn %d m %d" % c)
def test_min_voxels(dev, case):
    name, conn, m = case
    site = CC.site_volume(name)
    full = CC.reference(name, conn)
    assert {m - 1, m, m + 1} <= set(full["sizes_all"].tolist())
    ref = CC.reference(name, conn, m)
    assert 0 < ref["K"] < full["K"] and ref["found"] == full["found"]
    got = run_ccl(site, dev, conn, min_voxels=m, capacity=ref["K"] + 3)
    check_against(ref, got, ref["K"] + 3, case)
    kept = np.unique(got[0][got[0] > 0])
    assert kept.tolist() == list(range(1, ref["K"] + 1))                     # consecutive
    assert (np.diff(got[2][:ref["K"], 0]) > 0).all()                         # in root order
    # above the largest size: nothing is kept, found does not change
    above = int(full["sizes_all"].max()) + 1
    label, count, stats = run_ccl(site, dev, conn, min_voxels=above, capacity=2)
    assert (label == 0).all() and count.tolist() == [0, full["found"]] and (stats == CC.POISON).all()
    label, count, _ = run_ccl(site, dev, conn, min_voxels=2 ** 31 - 1)
    assert (label == 0).all() and count.tolist() == [0, full["found"]]


def test_stats_capacity(dev):
    name, conn = CC.CAPACITY_CASE
    site = CC.site_volume(name)
    ref = CC.reference(name, conn)
    K = ref["K"]
    for capacity in (0, 1, K - 1, K, K + 3):                                 # 0: out_stats is NULL
        check_against(ref, run_ccl(site, dev, conn, capacity=capacity), capacity, capacity)
    ref = CC.reference(name, conn, 3)                                        # ... and with dropped components between the kept ones
    for capacity in (0, 1, ref["K"] - 1, ref["K"], ref["K"] + 3):
        check_against(ref, run_ccl(site, dev, conn, min_voxels=3, capacity=capacity), capacity, ("m = 3", capacity))


# ---- BakedField.components ----------------------------------------------------------------------------------------------------------
def field_of(vol, dev):
    from d3fields_amd import BakedField
    return BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev),
                                  valid=torch.from_numpy(vol["valid"]).to(dev))


def sites_of(dist, valid, iso=0.0, unknown="free"):
    """the site mask of clearance() and components(), in NumPy"""
    with np.errstate(invalid="ignore"):
        s = valid & (dist <= np.float32(iso))
    return s | ~valid if unknown == "occupied" else s


def check_components(comp, sites, conn, min_voxels=1):
    ref = CC.components_ref(sites, conn, min_voxels)
    assert comp.labels.dtype == torch.int32 and comp.sites.dtype == torch.bool
    assert np.array_equal(comp.sites.cpu().numpy(), sites)
    assert np.array_equal(comp.labels.cpu().numpy(), ref["label"])
    assert (comp.count, comp.found, comp.connectivity, comp.min_voxels) == (ref["K"], ref["found"], conn, min_voxels)
    for t, cols in ((comp.roots, slice(0, 1)), (comp.sizes, slice(1, 2)), (comp.box_lo, slice(2, 5)), (comp.box_hi, slice(5, 8))):
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy().reshape(ref["stats"][:, cols].shape), ref["stats"][:, cols])
    assert tuple(comp.roots.shape) == tuple(comp.sizes.shape) == (ref["K"],) and tuple(comp.box_lo.shape) == tuple(comp.box_hi.shape) == (ref["K"], 3)
    return ref


HOLE_CASES = [k for k in BC.CASES if "holes" in k and not k.endswith("band 0.5h")]      # every hole-carrying volume of tests/band_cases.py once


@pytest.mark.parametrize("name", HOLE_CASES)
def test_field_components_equal_the_composition(dev, name):
    vol = BC.volume(name)
    assert not vol["valid"].all()
    f = field_of(vol, dev)
    h = float(vol["step"])
    dist, valid = vol["dist"], vol["valid"]
    ref = check_components(f.components(), sites_of(dist, valid), 26)
    assert ref["found"] >= 1
    for conn in (6, 18):
        check_components(f.components(connectivity=conn), sites_of(dist, valid), conn)
    check_components(f.components(unknown="occupied", connectivity=6), sites_of(dist, valid, unknown="occupied"), 6)
    check_components(f.components(iso=-1.5 * h, connectivity=6, min_voxels=2), sites_of(dist, valid, iso=-1.5 * h), 6, 2)
    check_components(f.components(iso=0.5 * h, unknown="occupied", connectivity=18), sites_of(dist, valid, iso=0.5 * h, unknown="occupied"), 18)
    none = f.components(iso=-1e3)
    assert none.count == none.found == 0 and not none.labels.any() and tuple(none.roots.shape) == (0,) and tuple(none.box_lo.shape) == (0, 3)
    # explicit sites, bool and uint8 (any non-zero byte)
    rng = np.random.default_rng(3)
    mask = rng.random(vol["shape"]) < 0.3
    check_components(f.components(sites=torch.from_numpy(mask).to(dev), connectivity=6, min_voxels=3), mask, 6, 3)
    check_components(f.components(sites=torch.from_numpy(mask * rng.integers(1, 256, mask.shape)).to(torch.uint8).to(dev)), mask, 26)
    # a banded source labels like its dense source; a clearance field labels its own dist (here: everything within 1.5 h of a site)
    b = f.to_band(float(BC.band_of(name)))
    cb, cd = b.components(connectivity=18), f.components(connectivity=18)
    assert torch.equal(cb.labels, cd.labels) and torch.equal(cb.roots, cd.roots) and torch.equal(cb.box_hi, cd.box_hi) and cb.count == cd.count
    c = f.clearance()
    check_components(c.components(iso=1.5 * h, connectivity=6), sites_of(c.dist.cpu().numpy(), c.valid.cpu().numpy(), iso=1.5 * h), 6)


def test_components_errors(dev):
    vol = BC.volume("5x4x6 sphere band 1.5h")
    f = field_of(vol, dev)
    ok = torch.zeros(tuple(vol["shape"]), dtype=torch.bool, device=dev)
    for kw in ({"connectivity": 4}, {"connectivity": None}, {"min_voxels": 0}, {"min_voxels": 1.5}, {"min_voxels": True}, {"unknown": "Free"},
               {"iso": float("nan")}, {"sites": ok, "iso": 0.1}, {"sites": ok, "unknown": "occupied"}, {"sites": ok[:-1]}, {"sites": ok.float()},
               {"sites": np.zeros(vol["shape"], bool)}):
        with pytest.raises(ValueError):
            f.components(**kw)
        with pytest.raises(ValueError):
            f.clearance(**kw)
    with pytest.raises(RuntimeError):
        f.components(sites=ok.cpu())
    assert f.components(sites=ok).count == 0


def test_mask_largest_boxes_world(dev):
    name = "large sphere holes band 1h"
    vol = BC.volume(name)
    f = field_of(vol, dev)
    rng = np.random.default_rng(5)
    mask = rng.random(vol["shape"]) < 0.12
    comp = f.components(sites=torch.from_numpy(mask).to(dev), connectivity=6)
    ref = check_components(comp, mask, 6)
    K, sizes = ref["K"], ref["stats"][:, 1]
    assert K > 10 and len(set(sizes.tolist())) < K                           # there are ties in size
    label = ref["label"]
    assert np.array_equal(comp.mask().cpu().numpy(), label > 0)
    assert np.array_equal(comp.mask(3).cpu().numpy(), label == 3)
    assert np.array_equal(comp.mask([2, K, 5]).cpu().numpy(), np.isin(label, [2, K, 5]))
    assert np.array_equal(comp.mask(torch.tensor([1, 4], device=dev)).cpu().numpy(), np.isin(label, [1, 4]))
    assert comp.mask().dtype == torch.bool and not comp.mask([]).any()
    for bad in (0, K + 1, [1, -1]):
        with pytest.raises(ValueError):
            comp.mask(bad)
    order = sorted(range(1, K + 1), key=lambda k: (-int(sizes[k - 1]), k))  # descending size, the smaller id first at a tie
    assert comp.largest().tolist() == order[:1] and comp.largest(5).tolist() == order[:5] and comp.largest(K + 7).tolist() == order
    assert comp.largest(0).tolist() == []
    # the outer faces of the voxels' cubes, in the float32 arithmetic origin + (i -+ 0.5) * step
    o, h = vol["origin"].astype(np.float32), np.float32(vol["step"])
    lo = o + (ref["stats"][:, 2:5].astype(np.float32) - np.float32(0.5)) * h
    hi = o + (ref["stats"][:, 5:8].astype(np.float32) + np.float32(0.5)) * h
    boxes = comp.boxes_world()
    assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (K, 2, 3)
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), np.stack((lo, hi), axis=1).astype(np.float32).view(np.uint32))
    centres = BC.lattice_points(vol).reshape(tuple(vol["shape"]) + (3,))
    for k in (1, K):
        own = centres[label == k]
        assert (own >= boxes[k - 1, 0].cpu().numpy()).all() and (own <= boxes[k - 1, 1].cpu().numpy()).all()


def test_more_components_than_the_first_launch_has_rows_for(dev, monkeypatch):
    from d3fields_amd import BakedField
    vol = BC.volume("large sphere holes band 1h")
    f = field_of(vol, dev)
    mask = np.random.default_rng(5).random(vol["shape"]) < 0.12
    sites = torch.from_numpy(mask).to(dev)
    K = CC.components_ref(mask, 6)["K"]
    for rows in (1, K - 1, K, K + 1):                                        # a re-run with the count on one side, none on the other
        monkeypatch.setattr(BakedField, "_STATS_ROWS", rows)
        check_components(f.components(sites=sites, connectivity=6), mask, 6)
    monkeypatch.setattr(BakedField, "_STATS_ROWS", 2)
    check_components(f.components(sites=sites, connectivity=6, min_voxels=4), mask, 6, 4)


def test_label_at(dev):
    vol = BC.volume("large sphere holes band 1h")
    f = field_of(vol, dev)
    shape = np.asarray(vol["shape"])
    h, o = float(f.step), np.asarray(f.origin, np.float64)
    rng = np.random.default_rng(12)
    mask = rng.random(vol["shape"]) < 0.4
    comp = f.components(sites=torch.from_numpy(mask).to(dev), connectivity=6, min_voxels=2)
    ref = check_components(comp, mask, 6, 2)
    assert ref["K"] < ref["found"]                                           # some sites belong to a dropped component
    centres = BC.lattice_points(vol)
    g = rng.uniform(-1.5, shape + 0.5, size=(997, 3))
    g[:40] = np.round(g[:40])                                                # lattice points, some of them outside
    g[40:60] = np.floor(g[40:60]) + 0.5                                      # the faces between two cubes
    g[60:70, 0] = -0.5                                                       # the outer faces of the lattice's box ...
    g[70:80, 2] = shape[2] - 0.5
    pts = np.concatenate([centres, (o + g * h).astype(np.float32)])
    pts[-6:-2] = np.nan
    pts[-2, 1] = np.inf
    pts[-1] = [np.nan, pts[-1, 1], pts[-1, 2]]
    got = comp.label_at(torch.from_numpy(pts).to(dev))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(pts),)
    # float64, half away from zero, inside the box of the voxels' own cubes: the rule of BakedField.nearest_site
    gg = (pts.astype(np.float64) - o) / h
    with np.errstate(invalid="ignore"):
        inside = np.all((gg >= -0.5) & (gg <= shape - 0.5), axis=1)
        i = np.clip(np.nan_to_num(np.sign(gg) * np.floor(np.abs(gg) + 0.5), nan=0.0, posinf=0.0, neginf=0.0), 0, shape - 1).astype(np.int64)
    want = np.where(inside, ref["label"][i[:, 0], i[:, 1], i[:, 2]], 0)
    assert inside.any() and (~inside).any() and not inside[-6:].any()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy()[:len(centres)].reshape(vol["shape"]), ref["label"])      # every voxel centre reads its own label
    assert (want[:len(centres)][(mask & (ref["label"] == 0)).reshape(-1)] == 0).all()
    with pytest.raises(TypeError):
        comp.label_at(torch.from_numpy(pts).to(dev).double())


# ---- clearance(min_voxels=, sites=) -------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_clearance(c, sites, step, signed=False):
    """the NumPy composition of tests/test_gpu_edt.py: the transform of `sites`, with signed the one of the complement inside"""
    step = np.float32(step)
    d2, nearest, dist = c.d2.cpu().numpy(), c.nearest_voxel.cpu().numpy(), c.dist.cpu().numpy()
    assert np.array_equal(c.sites.cpu().numpy(), sites)
    true_out = EC.edt_true(sites)
    ref_d2, ref_dist = true_out, EC.dist_ref(true_out, step)
    own = np.arange(sites.size).reshape(sites.shape)
    if signed:
        true_in = EC.edt_true(~sites)
        ref_d2 = np.where(sites, true_in, true_out)
        ref_dist = np.where(sites, -EC.dist_ref(true_in, step), ref_dist).astype(np.float32)
        EC.check_nearest(~sites, true_in, np.where(sites, nearest, own))
        EC.check_nearest(sites, true_out, np.where(sites, own, nearest))
    else:
        EC.check_nearest(sites, true_out, nearest)
    assert d2.dtype == np.int32 and np.array_equal(d2, ref_d2)
    assert same_bits(dist, ref_dist)
    assert np.array_equal(c.valid.cpu().numpy(), ref_d2 != INT32_MAX)


def test_clearance_without_floaters(dev):
    clean = BC.volume("large sphere holes band 1h")
    h = float(clean["step"])
    base = sites_of(clean["dist"], clean["valid"])
    sizes = CC.components_ref(base, 26)["sizes_all"]
    assert sizes.min() >= 2                                                  # nothing of the clean volume is a floater
    far = EC.edt_true(base) >= 9                                             # three voxels away from every site
    spots = np.argwhere(far & clean["valid"])
    spots = [tuple(spots[0]), tuple(spots[len(spots) // 2]), tuple(spots[-1])]
    assert all(max(abs(a - b) for a, b in zip(p, q)) >= 2 for i, p in enumerate(spots) for q in spots[:i])
    vol = dict(clean, dist=clean["dist"].copy())
    for p in spots:
        vol["dist"][p] = np.float32(-0.5 * h)                                # three single-voxel floaters
    dirty = sites_of(vol["dist"], vol["valid"])
    assert int(dirty.sum()) == int(base.sum()) + 3
    assert sorted(CC.components_ref(dirty, 26)["sizes_all"].tolist()) == [1, 1, 1, int(base.sum())]
    f, f_clean = field_of(vol, dev), field_of(clean, dev)
    for signed in (False, True):
        # the new defaults: the composition the parent commit's clearance() is pinned to
        plain = f.clearance(signed=signed)
        check_clearance(plain, dirty, f.step, signed)
        filtered = f.clearance(signed=signed, min_voxels=2)
        check_clearance(filtered, base, f.step, signed)
        ref = f_clean.clearance(signed=signed)
        assert not torch.equal(plain.d2, ref.d2)                             # the floaters cast phantom obstacles ...
        for k in ("d2", "nearest_voxel", "sites", "valid"):                  # ... and none with min_voxels = 2
            assert torch.equal(getattr(filtered, k), getattr(ref, k)), (signed, k)
        assert same_bits(filtered.dist.cpu().numpy(), ref.dist.cpu().numpy())
    # the threshold, the connectivity and `unknown` reach the labelling: with the holes occupied there are components of many sizes
    occupied = sites_of(vol["dist"], vol["valid"], unknown="occupied")
    kept = set()
    for conn, m in ((6, 2), (26, 2)):
        keep = CC.components_ref(occupied, conn, m)["label"] > 0
        kept.add(int(keep.sum()))
        assert keep.any() and (occupied & ~keep).sum() > 3
        check_clearance(f.clearance(unknown="occupied", min_voxels=m, connectivity=conn), keep, f.step)
    assert len(kept) == 2
    # explicit sites, alone and filtered
    rng = np.random.default_rng(21)
    mask = rng.random(vol["shape"]) < 0.05
    check_clearance(f.clearance(sites=torch.from_numpy(mask).to(dev)), mask, f.step)
    check_clearance(f.clearance(sites=torch.from_numpy(mask.astype(np.uint8) * 9).to(dev), signed=True), mask, f.step, signed=True)
    keep = CC.components_ref(mask, 26, 2)["label"] > 0
    assert keep.any() and (mask & ~keep).any()
    check_clearance(f.clearance(sites=torch.from_numpy(mask).to(dev), min_voxels=2), keep, f.step)


def test_reachability_through_a_gap(dev):
    """a sphere of radius r gets from start to goal exactly when both lie in one 6-connected component of the free
    space with clearance >= r.  A wall with a gap three voxels wide: the gap's middle line is two steps from the wall's nearest voxel."""
    from d3fields_amd import BakedField
    h, shape = 0.01, (24, 16, 12)
    dist = np.ones(shape, np.float32)
    dist[12] = -1.0
    dist[12, 6:9, :] = 1.0
    field = BakedField.from_arrays((0.0, 0.0, 0.0), h, torch.from_numpy(dist).to(dev))
    c = field.clearance()
    assert int(c.d2[12, 7, 5]) == 4 and int(c.d2[12, 6, 5]) == 1
    start = torch.tensor([[4 * h, 7 * h, 5 * h]], dtype=torch.float32, device=dev)
    goal = torch.tensor([[20 * h, 8 * h, 6 * h]], dtype=torch.float32, device=dev)
    labels = {}
    for r in (0.025, 0.015):                                                 # the gap is narrower than 2 * 0.025 and wider than 2 * 0.015
        free = c.dist >= r
        comp = field.components(sites=free, connectivity=6)
        labels[r] = (int(comp.label_at(start)), int(comp.label_at(goal)))
        assert np.array_equal(comp.labels.cpu().numpy(), CC.components_ref(free.cpu().numpy(), 6)["label"])
    assert labels[0.025][0] > 0 and labels[0.025][1] > 0 and labels[0.025][0] != labels[0.025][1]
    assert labels[0.015][0] > 0 and labels[0.015][0] == labels[0.015][1]
