"""The exact Euclidean distance transform on the device (d3f_volume_edt, csrc/edt_kernels.hip; BakedField.clearance / nearest_site)
against the NumPy restatement of tests/edt_cases.py: equality everywhere, no tolerance.

What each assert is there to catch:
  a window or early exit that drops a winning site, a wrong kernel form at a boundary    test_d2_nearest_dist_equal_the_restatement (every case, every cap)
  a distance carried instead of the site, a wrong unpacking of the carried site          the same test (check_nearest: the index is a site AT true_d2)
  a result that depends on launch order                                                  two launches give identical bytes
  sqrtf or the product in another precision, INT32_MAX not mapped to inf                 out_dist compared as bits
  an output that is only right when another one is requested                             test_every_subset_of_the_outputs
  an output or workspace the kernels do not fully write                                  outputs are poisoned before every launch
"""
import itertools

import numpy as np
import pytest
import torch

import band_cases as BC
import edt_cases as EC
import raycast_cases as RC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu

STEPS = (0.5, 0.004)
INT32_MAX = int(EC.INT32_MAX)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run_edt(site, dev, step=0.5, max_d2=0, want=("d2", "nearest", "dist")):
    """one d3f_volume_edt launch on freshly poisoned outputs and workspace -> {name: NumPy array}"""
    lib = _lib.load()
    nx, ny, nz = site.shape
    s = torch.from_numpy(np.array(site)).to(dev)      # (a copy: the case arrays are read-only)
    out = {}
    if "d2" in want:
        out["d2"] = torch.full((nx, ny, nz), -77, dtype=torch.int32, device=dev)
    if "nearest" in want:
        out["nearest"] = torch.full((nx, ny, nz), -77, dtype=torch.int32, device=dev)
    if "dist" in want:
        out["dist"] = torch.full((nx, ny, nz), float("nan"), dtype=torch.float32, device=dev)
    ws_bytes = lib.d3f_volume_edt_workspace_bytes(nx, ny, nz)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    _lib.check(lib.d3f_volume_edt(_lib.ptr(s), nx, ny, nz, step, max_d2, _lib.ptr(out.get("d2")), _lib.ptr(out.get("nearest")), _lib.ptr(out.get("dist")),
                                  _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", EC.CASES)
def test_d2_nearest_dist_equal_the_restatement(dev, name):
    site = EC.site_volume(name)
    true = EC.true_d2(name)
    for cap in (0,) + EC.CAPS:
        ref = EC.capped(name, cap)
        for step in STEPS if cap in (0, 5) else STEPS[:1]:
            got = run_edt(site, dev, step=step, max_d2=cap)
            assert got["d2"].dtype == np.int32 and np.array_equal(got["d2"], ref), (name, cap, int((got["d2"] != ref).sum()))
            EC.check_nearest(site, true, got["nearest"], cap)
            assert same_bits(got["dist"], EC.dist_ref(ref, step)), (name, cap, step)
        again = run_edt(site, dev, step=step, max_d2=cap)
        assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got), (name, cap, "two launches differ")
    if name == "no site":
        got = run_edt(site, dev)
        assert np.isposinf(got["dist"]).all() and (got["d2"] == INT32_MAX).all() and (got["nearest"] == -1).all()
    if name in EC.CORNER_CASES:
        corner = EC.CORNER_CASES[name]
        far = tuple(n - 1 - c for n, c in zip(site.shape, corner))
        got = run_edt(site, dev)
        assert got["d2"][far] == sum((n - 1) ** 2 for n in site.shape) and (got["nearest"] == np.ravel_multi_index(corner, site.shape)).all()


SUBSETS = [c for r in (1, 2) for c in itertools.combinations(("d2", "nearest", "dist"), r)]


@pytest.mark.parametrize("name", ["9x8x10 2%", "65x3x67", "4x300x3", "no site"])
def test_every_subset_of_the_outputs(dev, name):
    site = EC.site_volume(name)
    for cap in (0, 5):
        full = run_edt(site, dev, step=0.004, max_d2=cap)
        for want in SUBSETS:
            got = run_edt(site, dev, step=0.004, max_d2=cap, want=want)
            assert set(got) == set(want)
            for k in want:
                assert np.array_equal(got[k].view(np.uint32), full[k].view(np.uint32)), (name, cap, want, k)


# ---- BakedField.clearance -----------------------------------------------------------------------------------------------------------
def field_of(vol, dev):
    from d3fields_amd import BakedField
    return BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev),
                                  valid=torch.from_numpy(vol["valid"]).to(dev))


def sites_of(vol, iso, unknown):
    with np.errstate(invalid="ignore"):
        s = vol["valid"] & (vol["dist"] <= np.float32(iso))
    return s | ~vol["valid"] if unknown == "occupied" else s


def max_d2_of(field, max_distance):
    return int(np.floor((float(max_distance) / field.step) ** 2))


def check_clearance(c, f, vol, iso=0.0, unknown="free", signed=False, max_distance=None):
    sites = sites_of(vol, iso, unknown)
    cap = 0 if max_distance is None else max_d2_of(f, max_distance)
    step = np.float32(f.step)
    d2, nearest, dist = c.d2.cpu().numpy(), c.nearest_voxel.cpu().numpy(), c.dist.cpu().numpy()
    assert c.d2.dtype == torch.int32 and c.nearest_voxel.dtype == torch.int32 and c.sites.dtype == torch.bool and c.dist.dtype == torch.float32
    assert np.array_equal(c.sites.cpu().numpy(), sites)
    true_out = EC.edt_true(sites)
    ref_d2 = EC.edt_ref(sites, cap)
    ref_dist = EC.dist_ref(ref_d2, step)
    own = np.arange(sites.size).reshape(sites.shape)
    if signed:
        true_in = EC.edt_true(~sites)
        d2_in = EC.edt_ref(~sites, cap)
        ref_d2 = np.where(sites, d2_in, ref_d2)
        ref_dist = np.where(sites, -EC.dist_ref(d2_in, step), ref_dist).astype(np.float32)
        EC.check_nearest(~sites, true_in, np.where(sites, nearest, own), cap)      # a site voxel names the nearest non-site voxel
        EC.check_nearest(sites, true_out, np.where(sites, own, nearest), cap)      # every other voxel the nearest site
    else:
        EC.check_nearest(sites, true_out, nearest, cap)
    assert np.array_equal(d2, ref_d2)
    assert same_bits(dist, ref_dist)
    assert np.array_equal(c.valid.cpu().numpy(), ref_d2 != INT32_MAX)
    assert c.origin == f.origin and c.step == f.step and c.boundaries == f.boundaries and c.grid_shape == f.grid_shape
    assert c.names() == [] and c.band is None
    return sites, ref_d2


CLEARANCE_CASES = [k for k in BC.CASES if not k.endswith("band 0.5h")]      # every case volume of tests/band_cases.py once


@pytest.mark.parametrize("name", CLEARANCE_CASES)
def test_clearance_equals_the_composition(dev, name):
    vol = BC.volume(name)
    assert not vol["valid"].all() or "holes" not in name
    f = field_of(vol, dev)
    assert f.d2 is None and f.nearest_voxel is None and f.sites is None
    h = float(vol["step"])
    sites, d2 = check_clearance(f.clearance(), f, vol)
    assert sites.any() and not sites.all()
    check_clearance(f.clearance(unknown="occupied"), f, vol, unknown="occupied")
    check_clearance(f.clearance(iso=1.5 * h), f, vol, iso=1.5 * h)
    check_clearance(f.clearance(iso=-0.5 * h, unknown="occupied"), f, vol, iso=-0.5 * h, unknown="occupied")
    check_clearance(f.clearance(signed=True), f, vol, signed=True)
    check_clearance(f.clearance(signed=True, unknown="occupied", max_distance=1.6 * h), f, vol, signed=True, unknown="occupied", max_distance=1.6 * h)
    c = f.clearance(max_distance=2.3 * h)
    assert max_d2_of(f, 2.3 * h) == 5
    _, d2c = check_clearance(c, f, vol, max_distance=2.3 * h)
    assert c.valid.all() and float(c.dist.max()) <= 2.3 * h
    # no site at all: invalid everywhere, inf; with a cap every voxel is valid and reads the clamp value
    none = f.clearance(iso=-1e3)
    check_clearance(none, f, vol, iso=-1e3)
    assert not none.valid.any() and torch.isposinf(none.dist).all() and (none.nearest_voxel == -1).all()
    capped = f.clearance(iso=-1e3, max_distance=2.3 * h)
    assert capped.valid.all() and (capped.d2 == 5).all() and (capped.nearest_voxel == -1).all()
    # a banded source gives the same clearance as its dense source
    b = f.to_band(float(BC.band_of(name)))
    cb = b.clearance(signed=True)
    cd = f.clearance(signed=True)
    for k in ("d2", "nearest_voxel", "sites", "valid"):
        assert torch.equal(getattr(cb, k), getattr(cd, k)), k
    assert same_bits(cb.dist.cpu().numpy(), cd.dist.cpu().numpy()) and cb.band is None and cb.names() == []


def test_clearance_at_voxel_centres_on_a_power_of_two_step(dev):
    vol = RC.make_volume("9x8x10", "sphere", "pow2", False)
    assert vol["valid"].all()
    f = field_of(vol, dev)
    for kw in ({}, {"signed": True}, {"max_distance": 3.0 * float(vol["step"])}):
        c = f.clearance(**kw)
        assert c.valid.all()
        pts = torch.from_numpy(BC.lattice_points(vol)).to(dev)
        out = c.eval(pts)
        assert out["valid_mask"].all()
        assert same_bits(out["dist"].cpu().numpy().reshape(vol["shape"]), c.dist.cpu().numpy()), kw
    # the gradient exists and points away from the obstacle: along +x clearance grows where the nearest site lies at smaller x
    c = f.clearance()
    p = torch.from_numpy(BC.inside_points(vol, 257, 3)).to(dev).requires_grad_(True)
    c.eval(p)["dist"].sum().backward()
    assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any()


def test_nearest_site(dev):
    vol = BC.volume("large sphere holes band 1h")
    f = field_of(vol, dev)
    shape = np.asarray(vol["shape"])
    h, o = float(f.step), np.asarray(f.origin, np.float64)
    rng = np.random.default_rng(11)
    g = rng.uniform(-1.5, shape + 0.5, size=(997, 3))
    g[:40] = np.round(g[:40])                                # lattice points, some of them outside
    g[40:60] = np.floor(g[40:60]) + 0.5                      # half-way between two voxels
    pts = (o + g * h).astype(np.float32)
    pts[60:64] = np.nan
    pts[64, 1] = np.inf
    pts[65] = [np.nan, pts[65, 1], pts[65, 2]]
    for kw in ({}, {"max_distance": 2.3 * h}, {"signed": True}):
        c = f.clearance(**kw)
        near = c.nearest_site(torch.from_numpy(pts).to(dev))
        assert near["voxel"].dtype == torch.int64 and near["valid_mask"].dtype == torch.bool and near["points"].dtype == torch.float32
        # on the host: float64, half away from zero, the box of the voxels' own cubes
        gg = (pts.astype(np.float64) - o) / h
        with np.errstate(invalid="ignore"):
            inside = np.all((gg >= -0.5) & (gg <= shape - 0.5), axis=1)
            i = np.clip(np.nan_to_num(np.sign(gg) * np.floor(np.abs(gg) + 0.5), nan=0.0, posinf=0.0, neginf=0.0), 0, shape - 1).astype(np.int64)
        vox = np.where(inside, c.nearest_voxel.cpu().numpy()[i[:, 0], i[:, 1], i[:, 2]].astype(np.int64), -1)
        assert inside.any() and (~inside).any() and (vox >= 0).any() and not inside[60:66].any()
        if "max_distance" in kw:
            assert (inside & (vox < 0)).any()                # inside, but no site within the cap
        assert np.array_equal(near["voxel"].cpu().numpy(), vox)
        assert np.array_equal(near["valid_mask"].cpu().numpy(), vox >= 0)
        centres = BC.lattice_points(vol)[np.maximum(vox, 0)]
        got = near["points"].cpu().numpy()
        assert same_bits(got[vox >= 0], centres[vox >= 0]) and np.isnan(got[vox < 0]).all()
        if not kw:
            assert c.sites.view(-1)[near["voxel"][near["valid_mask"]]].all()
            rows = f.eval(near["points"])                    # what the nearest obstacle IS: the source field at the site's centre
            assert rows["dist"].shape == (len(pts),)


def test_clearance_errors(dev):
    vol = BC.volume("5x4x6 sphere band 1.5h")
    f = field_of(vol, dev)
    for bad in ("unknown", None, "Free", 0):
        with pytest.raises(ValueError):
            f.clearance(unknown=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            f.clearance(iso=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 0.5 * f.step):
        with pytest.raises(ValueError):
            f.clearance(max_distance=bad)
    pts = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        f.nearest_site(pts)
    with pytest.raises(ValueError):
        f.to_band(float(BC.band_of("5x4x6 sphere band 1.5h"))).nearest_site(pts)
    assert f.clearance().nearest_site(pts)["voxel"].shape == (3,)
