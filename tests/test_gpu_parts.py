"""Descriptor-gated links and the components over them on the device (d3f_volume_links, csrc/parts_kernels.hip;
d3f_volume_components_linked, csrc/ccl_kernels.hip; BakedField.links / parts / components(links=)) against the NumPy restatement of
tests/parts_cases.py: link bits, labels, counts and stats rows are compared byte for byte, no tolerance anywhere.

What each assert is there to catch:
  a sum that rounds differently from the contract (order, a fused operation, the vector against the scalar path)   test_channels: Gaussian rows whose
                                                                      thresholds sit among the pairs' own sums, at every channel count and both paths
  a halo row that is missing or taken from the wrong voxel, a link through memory instead of space                  test_tiles, test_straddling_pairs
  a z run that crosses a wave boundary or a line start, in the init kernel of the linked labelling                  test_lines_and_waves
  <= against <, the float64 verdict of the cosine rule                                                              test_ties
  NaN, Inf, signed zeros, zero rows, the first maximum                                                              test_specials
  a row read through a slot of -1, a tile that must leave early                                                     test_band
  a bit of a caller's link volume that is followed out of the volume or to a non-site                               test_all_ones_links_with_junk
  an output or workspace word read before it is written                                                             everything is poisoned with 0xA5
"""
import math

import numpy as np
import pytest
import torch

import ccl_cases as CC
import parts_cases as PC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run_links(dev, site, rows, rule, threshold, connectivity, valid=None, slot=None, stride=None, shift=0):
    """one d3f_volume_links launch on a poisoned output.  rows: [nx,ny,nz,C] without slot, the compacted [M, C] with it; stride: the row stride in
    floats (default C); shift: the rows begin that many floats into a 16-byte aligned buffer"""
    lib = _lib.load()
    nx, ny, nz = site.shape
    C = rows.shape[-1]
    flat = np.array(rows, np.float32).reshape(-1, C)                 # (a copy: the case arrays are read-only)
    stride = C if stride is None else stride
    buf = torch.full((shift + max(len(flat), 1) * stride + 4,), float("nan"), dtype=torch.float32, device=dev)      # NaN between and behind the rows
    if len(flat):
        buf[shift:shift + len(flat) * stride].view(len(flat), stride)[:, :C] = torch.from_numpy(flat).to(dev)
    data = buf[shift:]
    assert buf.data_ptr() % 16 == 0
    s = torch.from_numpy(np.array(site, np.uint8)).to(dev)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).to(dev)
    sl = None if slot is None else torch.from_numpy(np.ascontiguousarray(slot, np.int32)).to(dev)
    out = torch.full((nx, ny, nz), PC.POISON16 - 65536, dtype=torch.int16, device=dev)
    st = _lib.VolumeSet(data.data_ptr(), C, 0, stride, None)
    _lib.check(lib.d3f_volume_links(_lib.ptr(s), _lib.ptr(v), _lib.ptr(sl), nx, ny, nz, st, rule, float(threshold), connectivity, _lib.ptr(out),
                                    _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


def run_linked(dev, site, links, connectivity, min_voxels=1, capacity=0):
    """one d3f_volume_components_linked launch on poisoned outputs and workspace -> (label, count [2], stats or None)"""
    lib = _lib.load()
    nx, ny, nz = site.shape
    s = torch.from_numpy(np.array(site, np.uint8)).to(dev)
    lk = torch.from_numpy(np.array(links, np.uint16).view(np.int16)).to(dev)
    poison = int(CC.POISON)
    label = torch.full((nx, ny, nz), poison, dtype=torch.int32, device=dev)
    count = torch.full((2,), poison, dtype=torch.int32, device=dev)
    stats = torch.full((capacity, 8), poison, dtype=torch.int32, device=dev) if capacity > 0 else None
    ws_bytes = lib.d3f_volume_components_workspace_bytes(nx, ny, nz)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_volume_components_linked(_lib.ptr(s), _lib.ptr(lk), nx, ny, nz, connectivity, min_voxels, _lib.ptr(label), _lib.ptr(count), _lib.ptr(stats),
                                                capacity, _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return label.cpu().numpy(), count.cpu().numpy(), None if stats is None else stats.cpu().numpy()


def check_labels(ref, got, capacity, what):
    label, count, stats = got
    assert label.dtype == np.int32 and np.array_equal(label, ref["label"]), (what, int((label != ref["label"]).sum()))
    assert count.tolist() == [ref["K"], ref["found"]], (what, count.tolist())
    if capacity > 0:
        rows = min(capacity, ref["K"])
        assert np.array_equal(stats[:rows], ref["stats"][:rows]), what
        assert (stats[rows:] == CC.POISON).all(), (what, "a row at or beyond the capacity or K was written")


def same_links(got, ref, what):
    assert got.dtype == np.uint16 and np.array_equal(got, ref), (what, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())


def check_random(dev, name):
    site, rows, t2, tc = PC.random_volume(name)
    for rule, conn, thr in ((PC.L2, 26, t2), (PC.L2, 6, t2), (PC.COSINE, 18, tc), (PC.ARGMAX, 26, 0.0)):
        links_ref, comp_ref = PC.random_reference(name, rule, conn)
        links = run_links(dev, site, rows, rule, thr, conn)
        same_links(links, links_ref, (name, rule, conn))
        capacity = comp_ref["K"] + 3
        got = run_linked(dev, site, links, conn, capacity=capacity)
        check_labels(comp_ref, got, capacity, (name, rule, conn))
        again = run_linked(dev, site, run_links(dev, site, rows, rule, thr, conn), conn, capacity=capacity)      # determinism: the same bytes twice
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), (name, rule, conn, "two runs differ")
    m = 3                                                        # min_voxels reaches the shared numbering
    links_ref, full = PC.random_reference(name, PC.L2, 26)
    ref = PC.components_linked_ref(site, links_ref, 26, m)
    check_labels(ref, run_linked(dev, site, links_ref, 26, min_voxels=m, capacity=2), 2, (name, "min_voxels"))


@pytest.mark.parametrize("name", list(PC.LINES))
def test_lines_and_waves(dev, name):
    check_random(dev, name)


@pytest.mark.parametrize("name", list(PC.TILES))
def test_tiles(dev, name):
    check_random(dev, name)


def test_straddling_pairs(dev):
    for j, hi in PC.STRADDLES:
        site, rows = PC.straddle(j, hi)
        for conn in PC.CONNECTIVITIES:
            links = run_links(dev, site, rows, PC.L2, 0.0, conn)
            want = np.zeros(site.shape, np.uint16)
            if PC.allowed(j, conn):
                want[hi] = 1 << j
            same_links(links, want, (j, hi, conn))
            label, count, _ = run_linked(dev, site, links, conn)
            assert count.tolist() == [2 - int(PC.allowed(j, conn))] * 2 and int((label > 0).sum()) == 2


@pytest.mark.parametrize("C", PC.CHANNELS + (1024,))
def test_channels(dev, C):
    """Gaussian rows: the sums are inexact, so a different order of summation flips the pairs that sit next to the threshold -- and the thresholds
    ARE sums of pairs, one of them taken exactly"""
    shape = PC.CHANNEL_SHAPE
    rng = np.random.default_rng(100 + C)
    site = (rng.random(shape) < 0.9).astype(np.uint8)
    rows = PC.blocky_rows(shape, C, 200 + C, exact=False)
    sums = [PC.pair_sums(rows, off) for off in PC.OFFSETS]
    s = np.sort(np.concatenate([q["s"].reshape(-1) for q in sums]))
    with np.errstate(all="ignore"):
        cs = np.sort(np.concatenate([(q["dot"] / np.sqrt(q["na"].astype(np.float64) * q["nb"])).reshape(-1) for q in sums]))
    layouts = [(C, 0)] if C == 1024 else [(C, 0), (C + 4, 0), (C + 3, 0), (C, 1)]      # plain; padded rows (vector where C % 4 == 0); odd stride and off 16 bytes: scalar
    for stride, shift in layouts:
        for thr in (s[len(s) // 3], s[len(s) // 2]):
            ref = PC.links_ref(site != 0, rows, PC.L2, thr, 26)
            same_links(run_links(dev, site, rows, PC.L2, thr, 26, stride=stride, shift=shift), ref, (C, stride, shift, "l2", float(thr)))
        if C > 1:
            thr = float(np.clip(np.float32(cs[len(cs) // 2]), 0.0, 1.0))
            ref = PC.links_ref(site != 0, rows, PC.COSINE, thr, 26)
            same_links(run_links(dev, site, rows, PC.COSINE, thr, 26, stride=stride, shift=shift), ref, (C, stride, shift, "cosine", thr))
        ref = PC.links_ref(site != 0, rows, PC.ARGMAX, 0.0, 18)
        same_links(run_links(dev, site, rows, PC.ARGMAX, 0.0, 18, stride=stride, shift=shift), ref, (C, stride, shift, "argmax"))
    assert 0 < int((ref != 0).sum()) < ref.size


def pair_volume(a, b):
    """a 1 x 1 x 2 volume whose voxel 1 holds row a and voxel 0 row b -> (site, rows); the only possible bit is bit 12 of voxel 1"""
    rows = np.stack([np.asarray(b, np.float32), np.asarray(a, np.float32)]).reshape(1, 1, 2, -1)
    return np.ones((1, 1, 2), np.uint8), rows


def linked(dev, a, b, rule, thr):
    site, rows = pair_volume(a, b)
    got = run_links(dev, site, rows, rule, thr, 6)
    same_links(got, PC.links_ref(site != 0, rows, rule, thr, 6), (a, b, rule, thr))
    assert int(got[0, 0, 0]) == 0 and int(got[0, 0, 1]) in (0, 1 << 12)
    return bool(got[0, 0, 1])


def test_ties(dev):
    a, b = [3, -8, 0, 5, 1], [1, 8, 0, 5, -2]                   # small integers: s = 4 + 256 + 0 + 0 + 9 = 269 exactly
    below = float(np.nextafter(np.float32(269), np.float32(0)))
    assert linked(dev, a, b, PC.L2, 269.0) and not linked(dev, a, b, PC.L2, below) and linked(dev, a, b, PC.L2, math.inf)
    assert linked(dev, a, a, PC.L2, 0.0) and not linked(dev, a, b, PC.L2, 0.0)
    # cosine: dot = 1, na = 1, nb = 4: the cosine is exactly 1/2
    e, ones = [1, 0, 0, 0], [1, 1, 1, 1]
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert linked(dev, e, ones, PC.COSINE, 0.5) and not linked(dev, e, ones, PC.COSINE, above)
    assert linked(dev, [1, 2], [2, 4], PC.COSINE, 1.0) and not linked(dev, [1, 2], [2, 5], PC.COSINE, 1.0)          # c = 1: parallel rows only
    assert linked(dev, [1, 0], [0, 1], PC.COSINE, 0.0) and not linked(dev, [1, 0], [-1, 1], PC.COSINE, 0.0)         # c = 0: dot >= 0
    # the random cases carry many pairs exactly on their integer threshold
    site, rows, t2, tc = PC.random_volume("5x5x17")
    on = sum(int((PC.pair_sums(rows, off)["s"] == np.float32(t2)).sum()) for off in PC.OFFSETS)
    assert on > 100


def test_specials(dev):
    nan, inf = float("nan"), float("inf")
    for thr in (1e30, inf):
        assert not linked(dev, [nan, 1], [0, 1], PC.L2, thr) and not linked(dev, [0, 1], [nan, 1], PC.L2, thr) and not linked(dev, [inf, 1], [inf, 1], PC.L2, thr)
    assert not linked(dev, [inf, 1], [0, 1], PC.L2, 1e30) and not linked(dev, [0, 1], [-inf, 1], PC.L2, 3e38)
    assert linked(dev, [0.0, -0.0], [-0.0, 0.0], PC.L2, 0.0)                      # signed zeros are equal
    assert not linked(dev, [0, 0], [1, 1], PC.COSINE, 0.0) and not linked(dev, [1, 1], [0.0, -0.0], PC.COSINE, 0.0)      # a zero row links to nothing
    assert not linked(dev, [nan, 1], [1, 1], PC.COSINE, 0.0) and not linked(dev, [1, 1], [nan, 1], PC.COSINE, 0.0)
    # an infinity under the cosine rule is what IEEE makes of the contract's formula: Inf >= 0.25 * Inf holds, Inf >= 0 * Inf = NaN does not
    assert linked(dev, [inf, 1], [1, 1], PC.COSINE, 0.5) and not linked(dev, [inf, 1], [1, 1], PC.COSINE, 0.0) and not linked(dev, [inf, 1], [-1, 1], PC.COSINE, 0.5)
    assert linked(dev, [1e-30, 0], [1e-30, 0], PC.L2, 0.0) and not linked(dev, [1e-30, 0], [1e-30, 0], PC.COSINE, 1.0)    # the norms underflow to zero
    # argmax: the first maximum wins, a NaN never wins, a NaN at channel 0 stays
    assert linked(dev, [1, 1, 0], [1, 0, 0], PC.ARGMAX, 0.0) and not linked(dev, [0, 1, 1], [0, 0, 1], PC.ARGMAX, 0.0)
    assert linked(dev, [2, nan, 1], [3, 1, 2], PC.ARGMAX, 0.0) and linked(dev, [nan, 5], [7, 1], PC.ARGMAX, 0.0)
    assert not linked(dev, [1, inf], [inf, 1], PC.ARGMAX, 0.0) and linked(dev, [-0.0, 0.0], [0.0, -0.0], PC.ARGMAX, 0.0)
    # a special row inside a volume of ordinary ones poisons nothing but its own pairs
    site, rows, t2, tc = PC.random_volume("5x5x16")
    rows = rows.copy()
    rows[2, 2, 7] = nan
    rows[3, 1, 15, 2] = inf
    rows[1, 3, 0] = 0.0
    for rule, thr in ((PC.L2, t2), (PC.COSINE, tc), (PC.ARGMAX, 0.0)):
        same_links(run_links(dev, site, rows, rule, thr, 26), PC.links_ref(site != 0, rows, rule, thr, 26), ("specials", rule))


def test_band(dev):
    """rows behind a slot volume with holes: members are the stored sites that are valid; rows of other voxels do not exist"""
    shape, C = (9, 9, 33), 8
    rng = np.random.default_rng(41)
    site = (rng.random(shape) < 0.9).astype(np.uint8)
    valid = (rng.random(shape) < 0.9).astype(np.uint8)
    stored = rng.random(shape) < 0.7
    stored[4:8, 0:4, 16:32] = False                             # a whole tile without a stored voxel ...
    stored[0:4, 4:8, 0:16] = False
    stored[0, 4, 3] = True                                      # ... and one with a single stored voxel that is no site
    site[0, 4, 3] = 0
    slot = np.where(stored, np.cumsum(stored.reshape(-1)).reshape(shape) - 1, -1).astype(np.int32)
    dense = PC.blocky_rows(shape, C, 42)
    packed = dense[stored]
    member = PC.members_of(site, valid, slot)
    assert member.sum() > 500 and (site.astype(bool) & ~member).sum() > 300
    for rule, thr, conn in ((PC.L2, 4.0, 26), (PC.COSINE, 0.9, 18), (PC.ARGMAX, 0.0, 6)):
        ref = PC.links_ref(member, dense, rule, thr, conn)
        assert ref.any() and not ref[4:8, 0:4, 16:32].any()
        same_links(run_links(dev, site, packed, rule, thr, conn, valid=valid, slot=slot), ref, ("band", rule))
        same_links(run_links(dev, site, packed, rule, thr, conn, valid=valid, slot=slot, stride=C + 1), ref, ("band scalar", rule))
        # the empty band: no row is read, every voxel gets zero
        none = run_links(dev, site, np.zeros((0, C), np.float32), rule, thr, conn, valid=valid, slot=np.full(shape, -1, np.int32))
        assert not none.any()
    # labelling over the member mask: a link never reaches a non-member, whatever the site volume says
    links = PC.links_ref(member, dense, PC.L2, 4.0, 26)
    ref = PC.components_linked_ref(member, links, 26)
    check_labels(ref, run_linked(dev, member, links, 26, capacity=ref["K"]), ref["K"], "band labels")


def test_serpentine(dev):
    pos, path = PC.serpentine()
    site = np.ones(PC.SERPENTINE_SHAPE, np.uint8)
    n = site.size
    links = run_links(dev, site, pos, PC.L2, 1.0, 6)
    same_links(links, path, "serpentine")
    label, count, stats = run_linked(dev, site, links, 6, capacity=2)
    assert count.tolist() == [1, 1] and (label == 1).all() and stats[0].tolist() == [0, n, 0, 0, 0, 7, 7, 69]
    cut = links.copy()
    cut[PC.SERPENTINE_CUT] = 0
    ref = PC.components_linked_ref(site, cut, 6)
    assert ref["found"] == 2
    check_labels(ref, run_linked(dev, site, cut, 6, capacity=2), 2, "serpentine cut")
    check_labels(ref, run_linked(dev, site, cut, 26, capacity=2), 2, "serpentine cut, 26")      # the connectivity only removes bits


@pytest.mark.parametrize("name", ["9x8x10 30%", "2x3x65 50%", "3x4x300 30%", "wrap yz", "checkerboard", "nested", "all sites"])
def test_all_ones_links_with_junk(dev, name):
    """every bit set, the upper three too, also where it points out of the volume, through memory into the next line, or at a non-site: the
    plain components, byte for byte"""
    site = CC.site_volume(name)
    for conn in CC.CONNECTIVITIES:
        ref = CC.reference(name, conn)
        capacity = ref["K"] + 2
        check_labels(ref, run_linked(dev, site, np.full(site.shape, 0xFFFF, np.uint16), conn, capacity=capacity), capacity, (name, conn))
    junk = np.random.default_rng(2).integers(0, 1 << 16, site.shape).astype(np.uint16)
    ref = PC.components_linked_ref(site, junk, 26)
    check_labels(ref, run_linked(dev, site, junk, 26, capacity=ref["K"] + 2), ref["K"] + 2, (name, "random bits"))


# ---- BakedField.links / parts / components(links=) ------------------------------------------------------------------------------------
def scene_field(dev, sc, **extra):
    from d3fields_amd import BakedField
    sets = {k: torch.from_numpy(sc[k]).to(dev) for k in ("feat", "mask")}
    return BakedField.from_arrays((0.0, 0.0, 0.0), 0.01, torch.from_numpy(sc["dist"]).to(dev), **sets, **extra)


def same_components(a, b):
    return (torch.equal(a.labels, b.labels) and a.count == b.count and a.found == b.found and torch.equal(a.roots, b.roots) and torch.equal(a.sizes, b.sizes)
            and torch.equal(a.box_lo, b.box_lo) and torch.equal(a.box_hi, b.box_hi))


def test_touching_objects(dev):
    from d3fields_amd import Components
    sc = PC.touching_boxes()
    occupied = sc["dist"] <= 0
    f = scene_field(dev, sc)
    assert f.components().count == 1                                      # adjacency alone sees one object
    parts = f.parts("feat", tau=PC.TOUCHING_TAU, min_voxels=10)
    t2 = np.float32(PC.TOUCHING_TAU) * np.float32(PC.TOUCHING_TAU)
    ref = PC.components_linked_ref(occupied, PC.links_ref(occupied, sc["feat"], PC.L2, t2, 26), 26, 10)
    assert isinstance(parts, Components) and parts.count == parts.found == ref["K"] == 2 and (parts.connectivity, parts.min_voxels) == (26, 10)
    assert np.array_equal(parts.labels.cpu().numpy(), ref["label"]) and np.array_equal(parts.sites.cpu().numpy(), occupied)
    assert np.array_equal(torch.stack([parts.roots, parts.sizes], 1).cpu().numpy(), ref["stats"][:, :2])
    assert np.array_equal(torch.cat([parts.box_lo, parts.box_hi], 1).cpu().numpy(), ref["stats"][:, 2:])
    pooled = f.pool(parts, return_names=[], votes=["mask"])
    assert pooled["mask_votes"].argmax(dim=1).tolist() == [1, 2] and pooled["count"].tolist() == [640, 640]      # both instances are named
    assert pooled["mask_votes"].cpu().numpy().tolist() == [[0, 640, 0], [0, 0, 640]]
    # the same through the instance-mask rows, the cosine rule, links() + components(links=), and a banded field
    by_mask = f.parts("mask", rule="argmax", min_voxels=10)
    assert same_components(by_mask, parts)
    assert same_components(f.parts("feat", rule="cosine", cos=0.5, min_voxels=10), parts)
    lk = f.links("feat", tau=PC.TOUCHING_TAU)
    assert lk.dtype == torch.uint16 and tuple(lk.shape) == sc["shape"]
    assert np.array_equal(lk.cpu().view(torch.int16).numpy().view(np.uint16), PC.links_ref(occupied, sc["feat"], PC.L2, t2, 26))
    assert same_components(f.components(links=lk, min_voxels=10), parts) and same_components(f.components(links=lk.view(torch.int16), min_voxels=10), parts)
    own = lk.view(torch.int16) & ~torch.tensor(1 << 12, dtype=torch.int16, device=dev)      # a caller's own criterion ANDed in: no link along z
    cut = f.components(links=own.view(torch.uint16))
    assert np.array_equal(cut.labels.cpu().numpy(), PC.components_linked_ref(occupied, PC.links_ref(occupied, sc["feat"], PC.L2, t2, 26) & 0xEFFF, 26)["label"])
    b = f.to_band(0.02)
    stored = (b.slot >= 0).cpu().numpy()
    assert stored.any() and (occupied & ~stored).any()
    pb = b.parts("feat", tau=PC.TOUCHING_TAU)
    refb = PC.components_linked_ref(occupied & stored, PC.links_ref(occupied & stored, sc["feat"], PC.L2, t2, 26), 26)
    assert np.array_equal(pb.labels.cpu().numpy(), refb["label"]) and pb.count == refb["K"] == 2 and np.array_equal(pb.sites.cpu().numpy(), occupied & stored)
    assert torch.equal(b.parts("feat", tau=PC.TOUCHING_TAU).labels, pb.labels)                 # two runs, the same bytes
    assert torch.equal(f.clearance(sites=parts.mask(1)).sites, parts.labels == 1)


def test_every_pair_linked_equals_components(dev):
    """threshold = +Inf links every pair of finite rows: parts() is components(), byte for byte, at 6, 18 and 26"""
    from d3fields_amd import BakedField
    shape = (9, 10, 37)
    rng = np.random.default_rng(8)
    dist = rng.standard_normal(shape).astype(np.float32)
    valid = rng.random(shape) < 0.9
    rows = rng.standard_normal(shape + (6,)).astype(np.float32)
    f = BakedField.from_arrays((0.0, 0.0, 0.0), 0.02, torch.from_numpy(dist).to(dev), valid=torch.from_numpy(valid).to(dev), feat=torch.from_numpy(rows).to(dev))
    mine = torch.from_numpy(rng.random(shape) < 0.5).to(dev)
    for conn in (6, 18, 26):
        plain = f.components(iso=-0.8, connectivity=conn, min_voxels=2)
        assert plain.found > 5 and 0 < plain.count < plain.found
        assert same_components(f.parts("feat", tau=math.inf, iso=-0.8, connectivity=conn, min_voxels=2), plain)
        sited = f.parts("feat", tau=math.inf, sites=mine, connectivity=conn)
        assert same_components(sited, f.components(sites=mine & f.valid, connectivity=conn)) and torch.equal(sited.sites, mine & f.valid)
    empty = BakedField.from_arrays((0.0, 0.0, 0.0), 0.02, torch.full(shape, 10.0, device=dev), feat=torch.from_numpy(rows).to(dev)).to_band(0.05)
    assert empty.band_voxels.shape[0] == 0
    none = empty.parts("feat", tau=math.inf, iso=20.0)
    assert none.count == 0 and not none.labels.any() and not empty.links("feat", tau=1.0, iso=20.0).view(torch.int16).any()


def test_python_errors(dev):
    sc = PC.touching_boxes()
    f = scene_field(dev, sc)
    ok = torch.zeros(sc["shape"], dtype=torch.bool, device=dev)
    bad = [{"rule": "l1", "tau": 1.0}, {"rule": "l2"}, {"rule": "l2", "tau": -1.0}, {"rule": "l2", "tau": float("nan")}, {"rule": "l2", "tau": 1.0, "cos": 0.5},
           {"rule": "cosine"}, {"rule": "cosine", "cos": 1.5}, {"rule": "cosine", "cos": -0.1}, {"rule": "cosine", "cos": float("nan")},
           {"rule": "cosine", "cos": 0.5, "tau": 1.0}, {"rule": "argmax", "tau": 1.0}, {"rule": "argmax", "cos": 0.5}, {"tau": 1.0, "connectivity": 8},
           {"tau": 1.0, "iso": float("nan")}, {"tau": 1.0, "sites": ok, "iso": 0.1}, {"tau": 1.0, "sites": ok[:-1]}, {"tau": 1.0, "sites": ok.float()}]
    for kw in bad:
        with pytest.raises(ValueError):
            f.links("feat", **kw)
        with pytest.raises(ValueError):
            f.parts("feat", **kw)
    for kw in ({"min_voxels": 0}, {"min_voxels": 1.5}):
        with pytest.raises(ValueError):
            f.parts("feat", tau=1.0, **kw)
    with pytest.raises(KeyError):
        f.links("colour", tau=1.0)
    with pytest.raises(RuntimeError):
        f.parts("feat", tau=1.0, sites=ok.cpu())
    c = f.clearance()                                                     # a clearance field has no sets
    for call in (c.links, c.parts):
        with pytest.raises(ValueError):
            call("feat", tau=1.0)
    lk = f.links("feat", tau=1.0)
    for wrong in (lk[:-1], lk.view(torch.int16).int(), lk.cpu().numpy()):
        with pytest.raises(ValueError):
            f.components(links=wrong)
    with pytest.raises(RuntimeError):
        f.components(links=lk.cpu())
    assert f.parts("feat", tau=1.0, sites=ok).count == 0
