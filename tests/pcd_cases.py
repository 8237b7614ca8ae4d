"""Case builders for the fp64 point-cloud kernels on the mask side (csrc/pcd_kernels.hip: d3f_backproject_view, d3f_pcd_nearest;
csrc/assoc_kernels.hip: d3f_voxel_downsample, d3f_vox_idx_iou), shared by tests/test_pcd_cases_host.py (CPU: every case has the property
it is named for, and the reference alone meets it) and tests/test_gpu_pcd_edges.py (the kernels against the expected results).

Every case is a dict of inputs plus the expected result of oracle/np_pcd.py, built once (lru_cache) from fixed seeds and handed out
read-only.  Nothing here is random at test time.

Near ties of the nearest-neighbour search.  The contract is np.argmin over np.linalg.norm: the first row with the smallest ROOTED
distance.  sqrt is monotone but not injective in floating point, so two rows of b whose squared distances to a query differ by an ulp
can share a root; numpy then returns the earlier row although the later one has the smaller square.  tie_case() searches, from a
fixed seed, for queries that see one pair of rows of b that way; cluster_case() does the same with 41 rows whose x coordinates are
consecutive doubles, shuffled.
"""
import functools

import numpy as np

from oracle import np_pcd

KBLOCK = 256                        # csrc/d3f_internal.h: lanes per workgroup = rows of b per LDS tile of nearest_kernel
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def same_bits(got, want):
    """float64 arrays equal bit for bit, except that any NaN matches any NaN (the sign and payload of a generated NaN are not
    part of IEEE arithmetic and differ between processors); -0.0 does not match 0.0"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan]))


# ---- nearest neighbour -------------------------------------------------------------------------------------------------------------
def d2_of(a, b):
    """[na, nb] squared distances in float64, in the kernel's and numpy's order: (dx*dx + dy*dy) + dz*dz"""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    with np.errstate(over="ignore", invalid="ignore"):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _nearest_case(name, a, b, **extra):
    with np.errstate(over="ignore", invalid="ignore"):
        md, am = np_pcd.nearest(a, b)
    return _frozen(dict(name=name, a=np.ascontiguousarray(a, np.float64), b=np.ascontiguousarray(b, np.float64), min_dist=md, argmin=am, **extra))


TIE_POSITIONS = {"same tile": (10, 200), "tile boundary": (KBLOCK - 1, KBLOCK), "different tiles": (3, 700)}
TIE_NB = 3 * KBLOCK + 1             # three full tiles and a one-row tail
TIE_ROWS = 12                       # queries with the property per case (the contract asks for at least 8)
TIE_OTHERS = 21                     # further queries of the same pool, whatever they see
ANCHOR = np.array([0.3125, -0.21875, 0.40625])
FAR = np.array([40.0, 0.0, 0.0])    # the other rows of b lie in a unit box this far away: never nearest


def _pool(rng, n):
    """queries 0.05 .. 0.5 beyond ANCHOR along +x (so that a larger x of a row of b is a smaller dx), either side in y and z"""
    off = rng.uniform(0.05, 0.5, (n, 3))
    off[:, 1:] *= rng.choice([-1.0, 1.0], (n, 2))
    return ANCHOR + off


@functools.lru_cache(maxsize=None)
def tie_case(position):
    """One pair of rows of b, (earlier, later) = TIE_POSITIONS[position]: the later row is the earlier one with x one ulp larger.  The
    first TIE_ROWS queries are the first of a seeded pool for which d2[later] < d2[earlier] and the two roots are equal."""
    earlier, later = TIE_POSITIONS[position]
    rng = np.random.default_rng(7100 + earlier)
    pe = ANCHOR.copy()
    pl = pe.copy()
    pl[0] = pe[0] + np.spacing(pe[0])
    pool = _pool(rng, 4096)
    d2 = d2_of(pool, np.stack([pe, pl]))
    tied = np.flatnonzero((d2[:, 1] < d2[:, 0]) & (np.sqrt(d2[:, 1]) == np.sqrt(d2[:, 0])))
    assert tied.size >= TIE_ROWS, "the seeded pool holds too few near ties"
    a = np.concatenate([pool[tied[:TIE_ROWS]], pool[:TIE_OTHERS]])
    b = ANCHOR + FAR + rng.random((TIE_NB, 3))
    b[earlier], b[later] = pe, pl
    return _nearest_case("near tie, " + position, a, b, earlier=np.full(TIE_ROWS, earlier), later=np.full(TIE_ROWS, later), rows=np.arange(TIE_ROWS))


CLUSTER = 41
CLUSTER_NB = KBLOCK + 44


@functools.lru_cache(maxsize=None)
def cluster_case():
    """41 rows of b whose x coordinates are consecutive doubles, shuffled over rows on both sides of the tile boundary; the first
    TIE_ROWS queries are the first of a seeded pool for which the first minimum of the squares is not the first minimum of the roots."""
    rng = np.random.default_rng(7300)
    x = ANCHOR[0] + np.spacing(ANCHOR[0]) * rng.permutation(CLUSTER)
    rows = np.sort(rng.choice(CLUSTER_NB, CLUSTER, replace=False))
    b = ANCHOR + FAR + rng.random((CLUSTER_NB, 3))
    b[rows] = ANCHOR
    b[rows, 0] = x
    pool = _pool(rng, 4096)
    d2 = d2_of(pool, b)
    by_square, by_root = d2.argmin(axis=1), np.sqrt(d2).argmin(axis=1)
    split = np.flatnonzero(by_square != by_root)
    assert split.size >= TIE_ROWS, "the seeded pool holds too few near ties"
    pick = split[:TIE_ROWS]
    a = np.concatenate([pool[pick], pool[:TIE_OTHERS]])
    return _nearest_case("near tie, 41 consecutive doubles", a, b, earlier=by_root[pick], later=by_square[pick], rows=np.arange(TIE_ROWS))


def tie_cases():
    return [tie_case(p) for p in TIE_POSITIONS] + [cluster_case()]


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """rows 5, 300 and 511 of b are one point, rows 17 and 18 another; the queries next to them see the first of each"""
    rng = np.random.default_rng(7400)
    b = rng.normal(size=(2 * KBLOCK + 1, 3))
    b[[5, 300, 511]] = [3.0, 3.0, 3.0]
    b[[18, 17]] = [-3.0, -3.0, 3.0]
    a = np.concatenate([b[5] + 0.01 * rng.normal(size=(40, 3)), b[17] + 0.01 * rng.normal(size=(40, 3)), b[[5, 17]], rng.normal(size=(20, 3))])
    return _nearest_case("duplicate rows", a, b, first={5: np.arange(0, 40).tolist() + [80], 17: np.arange(40, 80).tolist() + [81]})


NEAREST_NB = (1, KBLOCK - 1, KBLOCK, KBLOCK + 1, 2 * KBLOCK + 1)
NEAREST_NA = (1, KBLOCK - 1, KBLOCK + 1)


@functools.lru_cache(maxsize=None)
def sized_case(na, nb):
    """ragged sizes; half of each cloud lies on a quarter-unit lattice, so exact ties (and exact zeros) are everywhere"""
    rng = np.random.default_rng(7500 + 7 * na + nb)

    def cloud(n):
        c = rng.normal(size=(n, 3))
        c[: (n + 1) // 2] = rng.integers(-4, 5, ((n + 1) // 2, 3)) / 4.0
        return c[rng.permutation(n)]
    return _nearest_case("na %d nb %d" % (na, nb), cloud(na), cloud(nb))


NAN_ROWS = (300, 400)               # of b: the first one is numpy's answer


@functools.lru_cache(maxsize=None)
def nan_b_case():
    rng = np.random.default_rng(7600)
    b = rng.normal(size=(2 * KBLOCK + 1, 3))
    b[NAN_ROWS[0], 1] = np.nan
    b[NAN_ROWS[1]] = np.nan
    return _nearest_case("NaN rows in b", rng.normal(size=(KBLOCK + 1, 3)), b)


NAN_QUERIES = (0, 7, KBLOCK)


@functools.lru_cache(maxsize=None)
def nan_query_case():
    rng = np.random.default_rng(7700)
    a = rng.normal(size=(KBLOCK + 1, 3))
    a[NAN_QUERIES[0], 0] = np.nan
    a[NAN_QUERIES[1]] = np.nan
    a[NAN_QUERIES[2], 2] = np.nan
    return _nearest_case("NaN query rows", a, rng.normal(size=(2 * KBLOCK + 1, 3)))


@functools.lru_cache(maxsize=None)
def overflow_case():
    """coordinates of +-1e200 in opposite octants: every difference is about 2e200 in some axis and every square is inf"""
    rng = np.random.default_rng(7800)
    a = 1e200 * (1.0 + rng.random((KBLOCK + 1, 3)))
    b = -1e200 * (1.0 + rng.random((KBLOCK + 44, 3)))
    return _nearest_case("squares overflow", a, b)


# ---- back-projection ---------------------------------------------------------------------------------------------------------------
IDENTITY = np.eye(4)
SPECIAL_DEPTHS = (0.0, -0.0, 1.5, np.nextafter(1.5, 0.0), np.nextafter(1.5, 2.0), -0.25, np.nan, np.inf, -np.inf, 5e-324, 0.75, 3.0)
MASK_BYTES = (0, 1, 2, 255)
SHAPES = ((1, 1), (7, 37), (15, 17), (16, 16), (1, 257), (37, 7), (9, 57))         # 1, 259, 255, 256, 257, 259, 513 pixels


def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.normal(size=3)
    return T


def _view_case(name, depth, mask, cam, T, bounds, **extra):
    """mask: uint8 bytes or None; the reference sees `mask != 0`, the byte test of the kernel"""
    with np.errstate(invalid="ignore", over="ignore"):
        pts, pix = np_pcd.backproject_view(depth, None if mask is None else mask != 0, cam, T, bounds)
    return _frozen(dict(name=name, depth=np.ascontiguousarray(depth, np.float64), mask=mask, cam=tuple(float(c) for c in cam), T=np.asarray(T, np.float64),
                        bounds=None if bounds is None else tuple(float(x) for x in bounds), pts=pts.reshape(-1, 3), pix=pix.astype(np.int64), **extra))


@functools.lru_cache(maxsize=None)
def random_view_case(shape, masked, cropped):
    """a general camera and rigid transform; depths 0.2 .. 1.8 with a fifth of the pixels 0; the crop box cuts on every side"""
    H, W = shape
    rng = np.random.default_rng(8000 + 100 * H + W + 2 * masked + cropped)
    depth = rng.uniform(0.2, 1.8, shape) * (rng.random(shape) > 0.2)
    mask = rng.choice(np.array(MASK_BYTES, np.uint8), shape) if masked else None
    cam = (W * 0.9 + 0.37, W * 0.8 - 0.11, W / 2 - 0.3, H / 2 + 0.2)
    T = _rigid(rng)
    bounds = None
    if cropped:
        c = T[:3, 3] + T[:3, 2]                  # the world point one unit in front of the camera
        bounds = (c[0] - 0.4, c[0] + 0.3, c[1] - 0.3, c[1] + 0.5, c[2] - 0.5, c[2] + 0.4)
    return _view_case("random %dx%d%s%s" % (H, W, " mask" if masked else "", " crop" if cropped else ""), depth, mask, cam, T, bounds)


@functools.lru_cache(maxsize=None)
def survivors_case(shape, which, masked):
    """which: 'none', 'all', or 'last' (survivors only in the last workgroup of KBLOCK pixels)"""
    H, W = shape
    npix = H * W
    last = (npix - 1) // KBLOCK * KBLOCK
    depth = np.zeros(npix)
    if which == "all":
        depth[:] = 0.5 + 0.001 * np.arange(npix)
    elif which == "last":
        depth[last:] = 0.5 + 0.001 * np.arange(npix - last)
    mask = None
    if masked:
        mask = np.full(npix, 255, np.uint8)
        if which == "none":
            depth[:] = 1.0                       # the mask, not the depth, removes everything
            mask[:] = 0
        mask = mask.reshape(shape)
    rng = np.random.default_rng(8100 + npix)
    return _view_case("%s survive %dx%d%s" % (which, H, W, " mask" if masked else ""), depth.reshape(shape), mask, (W * 1.1, W * 1.2, W / 2, H / 2), _rigid(rng), None,
                      which=which, last=last)


@functools.lru_cache(maxsize=None)
def special_depth_case(masked):
    """every SPECIAL_DEPTHS value under every mask byte, 9x57 = 513 pixels.  Without a mask the gate is 0 < d < 1.5, with one it is
    byte != 0 and d > 0: 1.5, the double after it, 3.0 and +inf pass only the second."""
    H, W = 9, 57
    npix = H * W
    k = np.arange(npix)
    depth = np.array(SPECIAL_DEPTHS)[k % len(SPECIAL_DEPTHS)]
    mask = np.array(MASK_BYTES, np.uint8)[(k // len(SPECIAL_DEPTHS)) % len(MASK_BYTES)].reshape(H, W) if masked else None
    rng = np.random.default_rng(8200)
    return _view_case("special depths%s" % (" mask" if masked else ""), depth.reshape(H, W), mask, (61.3, 58.9, 28.5, 4.25), _rigid(rng), None)


ON_BOUND = (-2.0, 3.0, -1.0, 2.0, 0.5, 2.0)     # x, y: integer pixel offsets at depth 1; z: the depths 0.5 and 2 themselves


@functools.lru_cache(maxsize=None)
def on_bound_case(masked):
    """identity transform, fx = fy = 1, cx = 8, cy = 3, so world (x, y, z) = ((col - 8) d, (row - 3) d, d) exactly.  Depth 1 puts whole
    columns and rows on the x and y bounds; depths 0.5 and (with a mask) 2 sit on the z bounds.  All of them are outside: the
    inequalities are strict on both sides."""
    H, W = 7, 19
    depth = np.ones((H, W))
    depth[:, 9] = 0.5
    depth[:, 8] = 2.0 if masked else 1.25
    depth[0, :] = 0.75
    mask = np.full((H, W), 2, np.uint8) if masked else None
    return _view_case("on the crop bound%s" % (" mask" if masked else ""), depth, mask, (1.0, 1.0, 8.0, 3.0), IDENTITY, ON_BOUND)


def uncropped_points(case):
    """the reference's points before the crop, for the host test"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np_pcd.backproject_view(case["depth"], None if case["mask"] is None else case["mask"] != 0, case["cam"], case["T"], None)


def view_cases():
    out = [random_view_case(s, m, c) for s in SHAPES for m in (False, True) for c in (False, True)]
    out += [survivors_case(s, w, m) for s in ((1, 1), (7, 37), (16, 16), (9, 57)) for w in ("none", "all", "last") for m in (False, True)]
    out += [special_depth_case(m) for m in (False, True)] + [on_bound_case(m) for m in (False, True)]
    return out


# ---- voxel-grid mean ---------------------------------------------------------------------------------------------------------------
VOX_FIX = 2.0 ** -40                # csrc/assoc_kernels.hip: kVoxFix, the fixed point of the sums
MAX_PER_VOXEL = 8                   # of the cases checked to a tolerance: bounds the rounding of the reference's own sums
VOXEL_SIZES = (1e-4, 0.01, 0.25, 10.0)
AXIS_EXTENT = 2097150               # voxels between the two points of extent_case: the widest a 21-bit axis key holds (0 .. 2^21 - 1,
#                                     and the anchor half a voxel below the minimum puts the far point at 2097150.5)


def point_tol(points, voxel_size):
    """2^-40 voxel sides (each point's offset inside its voxel is truncated to that fixed point, so is their mean) + 8 ulp of max|p| (the
    reference adds at most MAX_PER_VOXEL points in float64: at most 7 roundings of at most an ulp of the mean each, and the kernel's
    anchor + offset is one more)"""
    return VOX_FIX * voxel_size + 8 * float(np.spacing(np.abs(points).max()))


def colour_tol(colours):
    """colours are stored at the same fixed point, not scaled by the voxel: 2^-40 absolute + 8 ulp of max|c|"""
    return VOX_FIX + 8 * float(np.spacing(np.abs(colours).max()))


def voxel_index(points, voxel_size):
    """open3d's voxel index of every point, as np_pcd.voxel_mean forms it"""
    points = np.asarray(points, np.float64)
    return np.floor((points - (points.min(axis=0) - voxel_size * 0.5)) / voxel_size).astype(np.int64)


def _voxel_case(name, points, voxel_size, colours=None, **extra):
    points = np.ascontiguousarray(points, np.float64)
    if colours is None:
        want_p, want_c = np_pcd.voxel_mean(points, voxel_size), None
    else:
        colours = np.ascontiguousarray(colours, np.float64)
        want_p, want_c = np_pcd.voxel_mean(points, voxel_size, colours)
    return _frozen(dict(name=name, points=points, voxel_size=float(voxel_size), colours=colours, want_points=want_p, want_colours=want_c, **extra))


@functools.lru_cache(maxsize=None)
def cloud_case(voxel_size, colours="unit"):
    """2000 points in a box of 15^3 voxels placed some 1e4 voxel sides from the origin (so |p| >> voxel_size: the subtraction of the voxel
    corner cancels most digits).  colours: 'unit' [0,1), 'negative' [-2,1), 'bytes' raw 0..255, None"""
    rng = np.random.default_rng(9000 + int(round(np.log10(voxel_size) * 10)) + {"unit": 0, "negative": 1, "bytes": 2, None: 3}[colours])
    pts = voxel_size * (np.array([3000.0, -7000.0, 11000.0]) + rng.uniform(0.0, 15.0, (2000, 3)))
    col = {"unit": lambda: rng.random((2000, 3)), "negative": lambda: rng.uniform(-2.0, 1.0, (2000, 3)),
           "bytes": lambda: rng.integers(0, 256, (2000, 3)).astype(np.float64), None: lambda: None}[colours]()
    return _voxel_case("cloud, voxel %g, %s colours" % (voxel_size, colours), pts, voxel_size, col)


@functools.lru_cache(maxsize=None)
def face_case():
    """voxel_size 0.25, every coordinate a multiple of 0.125 in -2 .. 2: the anchor is a multiple of 0.125 too, so every second lattice
    value lies exactly on a voxel face and belongs to the voxel above it.  All the arithmetic is exact; at most 8 points share a voxel."""
    rng = np.random.default_rng(9100)
    pts = rng.integers(-16, 17, (1500, 3)) * 0.125
    pts[0] = -2.0                               # the minimum itself on the lattice
    return _voxel_case("points on voxel faces", pts, 0.25, rng.random((1500, 3)))


@functools.lru_cache(maxsize=None)
def one_point_case():
    return _voxel_case("one point", np.array([[0.1234, -5.678, 9.0]]), 0.01, np.array([[0.25, 1.5, -3.0]]))


IDENTICAL = 4097


@functools.lru_cache(maxsize=None)
def identical_case():
    """4097 copies of a point of few mantissa bits at voxel_size 0.25: the reference's 4097-term sums are exact, so its mean is the point,
    bit for bit, and so must the kernel's be (offset exactly half a voxel, 4097 * 2^39 in the fixed-point sum)"""
    p, c = np.array([0.375, -1.25, 2.5]), np.array([0.5, 0.25, 200.0])
    return _voxel_case("4097 identical points", np.tile(p, (IDENTICAL, 1)), 0.25, np.tile(c, (IDENTICAL, 1)))


VOXEL_COUNTS = (KBLOCK - 1, KBLOCK, KBLOCK + 1, 27 ** 3)


@functools.lru_cache(maxsize=None)
def count_case(voxels):
    """exactly `voxels` occupied voxels of side 0.01: one point on each of the first `voxels` sites of a cubic lattice (the origin
    among them, so the anchor is -0.005 on every axis and site k lies at k + 0.5 voxels), and up to two more points per site 0 .. 0.4 voxels
    beyond it on every axis, which stay inside the site's voxel.  27^3 = 19683 sites: tens of thousands of points, many hash probes,
    77 rank tiles."""
    rng = np.random.default_rng(9200 + voxels)
    side = 8 if voxels <= 512 else 27
    k = np.arange(voxels)
    sites = np.stack([k % side, (k // side) % side, k // (side * side)], axis=1).astype(np.float64)
    extra = np.repeat(k, rng.integers(0, 3, voxels))
    pts = 0.01 * np.concatenate([sites, sites[extra] + rng.uniform(0.0, 0.4, (extra.size, 3))])
    order = rng.permutation(len(pts))
    return _voxel_case("%d voxels" % voxels, pts[order], 0.01, rng.random((len(pts), 3)), voxels=voxels)


@functools.lru_cache(maxsize=None)
def extent_case(axis):
    """two points AXIS_EXTENT voxels apart on one axis"""
    pts = np.zeros((2, 3))
    pts[1, axis] = AXIS_EXTENT * 0.01
    return _voxel_case("extent on axis %d" % axis, pts, 0.01, None, axis=axis)


def tolerance_voxel_cases():
    """cases compared to point_tol / colour_tol (identical_case is compared bit for bit instead)"""
    return [cloud_case(v) for v in VOXEL_SIZES] + [cloud_case(0.01, "negative"), cloud_case(0.01, "bytes"), cloud_case(0.25, None), face_case(), one_point_case()] \
        + [count_case(v) for v in VOXEL_COUNTS] + [extent_case(0), extent_case(2)]


# ---- voxel-index sets --------------------------------------------------------------------------------------------------------------
def _iou_case(name, a, b, **extra):
    a, b = np.asarray(a, np.int64).astype(np.int32), np.asarray(b, np.int64).astype(np.int32)
    return _frozen(dict(name=name, a=a, b=b, want=np_pcd.vox_idx_iou(a, b), **extra))


@functools.lru_cache(maxsize=None)
def iou_cases():
    rng = np.random.default_rng(9500)
    keys = rng.permutation(np.unique(rng.integers(INT32_MIN, INT32_MAX + 1, 2000)))[:520]
    run = np.arange(-1500, 1500)
    out = [
        _iou_case("extreme keys", [INT32_MIN, -1, 0, INT32_MAX, -1, 0], [-1, INT32_MAX, 0, INT32_MIN, -2, 5], distinct=6),
        _iou_case("extreme keys, disjoint", [-1, -1, INT32_MAX], [INT32_MIN, 0, -2], distinct=5),
        _iou_case("first empty", [], [1, 2, 2, 3], distinct=3),
        _iou_case("second empty", [4, 4, -4], [], distinct=2),
        _iou_case("one repeated key", [7] * 300, [7] * 500, distinct=1),
        _iou_case("two repeated keys", [-1] * 300, [7] * 500, distinct=2),
    ]
    for total in (512, 513):                    # the hash set doubles from 1024 to 2048 slots between n1 + n2 = 512 and 513
        out.append(_iou_case("%d distinct keys, disjoint" % total, keys[:256], keys[256:total], distinct=total, length=total))
        out.append(_iou_case("%d distinct keys, overlapping" % total, keys[:384], keys[128:total], distinct=total))
    out.append(_iou_case("dense run", rng.permutation(run[:2000]), rng.permutation(run[1000:]), distinct=3000))
    return out
