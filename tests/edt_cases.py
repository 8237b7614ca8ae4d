"""NumPy restatement and case list of the exact Euclidean distance transform (d3f_volume_edt, include/d3fields_hip.h ABI 14; DESIGN.md
section 16), shared by tests/test_edt_host.py and tests/test_gpu_edt.py.

    true_d2(v) = min over the sites s of |v - s|^2 in integer voxel coordinates, INT32_MAX for a volume without a site
    cap        = max_d2 if max_d2 > 0 else INT32_MAX
    d2         = min(true_d2, cap)
    nearest    = the flat index of A site at true_d2, -1 where true_d2 > cap or there is no site

edt_ref is separable like the kernels but shares nothing else with them: per axis the full min_j f[j] + (i - j)^2 in int64, no window,
no early exit.  test_edt_host.py checks it against the brute-force minimum over all sites and, where scipy imports, against
scipy.ndimage.distance_transform_edt.
"""
import functools

import numpy as np

INT32_MAX = np.int32(2 ** 31 - 1)
_BIG = np.int64(1) << 40                      # "no site": above every true distance (3 * 16383^2 < 2^30) plus every (i - j)^2
CAPS = (1, 4, 5, 50)
_CHUNK_BYTES = 32 << 20                       # the [i, j, rest] block of one axis pass is formed in slabs of i of about this size


def _axis_pass(f, axis):
    """out[.., i, ..] = min_j f[.., j, ..] + (i - j)^2 along `axis`, int64"""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    rest = int(np.prod(f.shape[1:], dtype=np.int64))
    g = f.reshape(n, rest)
    out = np.empty_like(g)
    j = np.arange(n, dtype=np.int64)
    rows = max(1, int(_CHUNK_BYTES // (8 * n * max(rest, 1))))
    for i0 in range(0, n, rows):
        i = np.arange(i0, min(n, i0 + rows), dtype=np.int64)
        sq = (i[:, None] - j[None, :]) ** 2                                   # [i, j]
        out[i0:i0 + len(i)] = np.min(g[None, :, :] + sq[:, :, None], axis=1)
    return np.moveaxis(out.reshape(f.shape), 0, axis)


def edt_true(site):
    """true_d2 as int32 (INT32_MAX without a site)"""
    site = np.asarray(site) != 0
    assert site.ndim == 3
    f = np.where(site, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        f = _axis_pass(f, axis)
    return np.where(f >= _BIG, np.int64(INT32_MAX), f).astype(np.int32)


def edt_ref(site, max_d2=0):
    """d2 = min(true_d2, cap) as int32"""
    d2 = edt_true(site)
    return np.minimum(d2, np.int32(max_d2)) if max_d2 > 0 else d2


def brute_force(site):
    """true_d2 as the minimum over the explicit list of sites (small volumes only)"""
    site = np.asarray(site) != 0
    s = np.argwhere(site).astype(np.int64)
    if len(s) == 0:
        return np.full(site.shape, INT32_MAX, np.int32)
    v = np.argwhere(np.ones(site.shape, bool)).astype(np.int64)
    d = ((v[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)
    return d.reshape(site.shape).astype(np.int32)


def nearest_count(site):
    """how many sites lie at true_d2 of every voxel (small volumes only)"""
    site = np.asarray(site) != 0
    s = np.argwhere(site).astype(np.int64)
    v = np.argwhere(np.ones(site.shape, bool)).astype(np.int64)
    d = ((v[:, None, :] - s[None, :, :]) ** 2).sum(-1)
    return (d == d.min(1, keepdims=True)).sum(1).reshape(site.shape)


def check_nearest(site, d2_true, nearest, cap=0):
    """nearest == -1 exactly where the definition says; elsewhere it names a site at exactly true_d2"""
    site = np.asarray(site) != 0
    nearest = np.asarray(nearest).astype(np.int64)
    assert nearest.shape == site.shape
    d2_true = np.asarray(d2_true).astype(np.int64)
    none = (d2_true == int(INT32_MAX)) | ((d2_true > cap) if cap > 0 else False)
    assert np.array_equal(nearest == -1, np.broadcast_to(none, site.shape)), "nearest == -1 at %d voxels, expected at %d" % (
        int((nearest == -1).sum()), int(np.sum(none)))
    has = ~np.broadcast_to(none, site.shape)
    idx = nearest[has]
    assert np.all((idx >= 0) & (idx < site.size))
    assert np.all(site.reshape(-1)[idx]), "nearest names a voxel that is no site"
    s = np.stack(np.unravel_index(idx, site.shape), axis=-1).astype(np.int64)
    v = np.argwhere(has).astype(np.int64)
    assert np.array_equal(((v - s) ** 2).sum(-1), d2_true[has]), "nearest is not at true_d2"


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# name -> (shape, kind, density).  The long shapes put a line of every pass across each boundary between two kernel forms: 64 lanes
# of the z pass (65x3x67, 3x4x300), and 256 / 512 / 1280 entries of a y or x line (64 lines in 64 KiB, 32 lines in 64 KiB, 32 lines in
# up to 160 KiB, global memory).
def _random(shape, density, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    site = np.zeros(n, np.uint8)
    site[rng.choice(n, max(1, int(round(density * n))), replace=False)] = rng.integers(1, 256, max(1, int(round(density * n))))   # any non-zero byte
    return site.reshape(shape)


RANDOM = {
    "5x4x6 10%": ((5, 4, 6), 0.10), "9x8x10 2%": ((9, 8, 10), 0.02),
    "65x3x67": ((65, 3, 67), 0.005), "130x66x5": ((130, 66, 5), 0.002), "300x4x3": ((300, 4, 3), 0.01), "4x300x3": ((4, 300, 3), 0.01),
    "3x4x300": ((3, 4, 300), 0.01), "600x3x2": ((600, 3, 2), 0.004), "2x600x3": ((2, 600, 3), 0.004), "1300x2x3": ((1300, 2, 3), 0.002),
    "3x1300x2": ((3, 1300, 2), 0.002), "40x33x1": ((40, 33, 1), 0.01), "6x5x50": ((6, 5, 50), 0.02), "1x1x90": ((1, 1, 90), 0.03),
}
TIE_CASES = ("5x4x6 10%", "9x8x10 2%")                  # asserted on the host: voxels with more than one nearest site
CAP_CASES = ("corner 9x8x10", "65x3x67")                # asserted on the host: voxels below, exactly at and above every cap of CAPS


@functools.lru_cache(maxsize=None)
def site_volume(name):
    if name in RANDOM:
        shape, density = RANDOM[name]
        return _random(shape, density, 7000 + sorted(RANDOM).index(name))
    if name == "2x2x2 one site":
        site = np.zeros((2, 2, 2), np.uint8)
        site[1, 0, 1] = 1
    elif name == "all sites":
        site = np.ones((7, 5, 9), np.uint8)
    elif name == "no site":
        site = np.zeros((7, 5, 9), np.uint8)
    elif name == "corner 9x8x10":
        site = np.zeros((9, 8, 10), np.uint8)
        site[0, 0, 0] = 255
    elif name == "corner 70x3x66":                  # the far corner lies beyond one wave in z and one 64-entry step in x
        site = np.zeros((70, 3, 66), np.uint8)
        site[69, 2, 65] = 1
    elif name == "plane":
        site = np.zeros((9, 8, 10), np.uint8)
        site[:, 3, :] = 1
    elif name == "checkerboard":
        i = np.indices((9, 8, 10)).sum(0)
        site = (i % 2 == 0).astype(np.uint8)
    else:
        raise KeyError(name)
    site.setflags(write=False)
    return site


CORNER_CASES = {"corner 9x8x10": (0, 0, 0), "corner 70x3x66": (69, 2, 65)}
CASES = ["2x2x2 one site"] + list(RANDOM) + ["all sites", "no site", "corner 9x8x10", "corner 70x3x66", "plane", "checkerboard"]


@functools.lru_cache(maxsize=None)
def true_d2(name):
    """edt_true of a case, computed once and shared (read-only)"""
    d2 = edt_true(site_volume(name))
    d2.setflags(write=False)
    return d2


def capped(name, max_d2):
    d2 = true_d2(name)
    return np.minimum(d2, np.int32(max_d2)) if max_d2 > 0 else d2


def dist_ref(d2, step):
    """out_dist of the contract: sqrtf((float)d2) * step in float32, +inf where d2 == INT32_MAX"""
    with np.errstate(over="ignore"):
        d = np.sqrt(d2.astype(np.float32)) * np.float32(step)
    return np.where(d2 == INT32_MAX, np.float32(np.inf), d).astype(np.float32)
