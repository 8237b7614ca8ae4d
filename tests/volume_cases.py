"""Float64 reference, float32 port and case generator of the baked-volume lookup (include/d3fields_hip.h, ABI 11; DESIGN.md
section 13), shared by tests/test_volume_host.py and tests/test_gpu_volume.py.

A volume is a dict: origin (3 x float32), step (float32), shape (nx, ny, nz), dist float32 [nx,ny,nz], valid bool [nx,ny,nz],
sets {name: float32 [nx,ny,nz,C]}, fills {name: float32 [C] or None}.

trilinear64 / trilinear_grad64 restate the contract in float64 NumPy: they take the float32 inputs as given and form g in
float64.  Besides values and validity they return, per entry,
    A = sum_c w_c |v_c|                 the scale of the chain's own rounding, and
    S = max_c v_c - min_c v_c           the corner spread: |d out / d t_a| <= S, the scale of the coordinate rounding
(for the gradient: B = sum |grad| sum_c |dw_c/dt_a| |v_c| / h and T = sum |grad| S / h, see grad_bound).
"""
import functools

import numpy as np

U = 2.0 ** -24
SENTINEL = np.float32(1e3)

# corner c = dx*4 + dy*2 + dz: the order of the chain
CORNERS = [(c >> 2, (c >> 1) & 1, c & 1) for c in range(8)]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def locate64(vol, pts):
    """(valid [N], i [N,3] int, t [N,3] float64) -- i / t are meaningful where inside"""
    n = np.asarray(vol["shape"])
    g = (pts.astype(np.float64) - np.asarray(vol["origin"], np.float64)) / float(vol["step"])
    with np.errstate(invalid="ignore"):
        inside = np.all((g >= 0) & (g <= n - 1), axis=1)                  # NaN compares false
    gi = np.where(inside[:, None], g, 0.0)
    i = np.minimum(np.floor(gi).astype(np.int64), n - 2)
    t = gi - i
    ok = inside.copy()
    for dx, dy, dz in CORNERS:
        ok &= vol["valid"][i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz]
    return ok, i, t


def _weights(t, dtype=np.float64):
    """[8, N] corner weights, products formed left to right"""
    one = dtype(1.0)
    a = [np.stack([one - t[:, k], t[:, k]]) for k in range(3)]
    return np.stack([a[0][dx] * a[1][dy] * a[2][dz] for dx, dy, dz in CORNERS])


def _corners(arr, i):
    """[8, N, ...] corner values"""
    return np.stack([arr[i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz] for dx, dy, dz in CORNERS])


def _arrays(vol, names):
    out = [("dist", vol["dist"][..., None], np.asarray([SENTINEL]))]
    for k in names:
        C = vol["sets"][k].shape[3]
        fill = vol["fills"].get(k)
        out.append((k, vol["sets"][k], np.zeros(C, np.float32) if fill is None else fill))
    return out


def trilinear64(vol, pts, names=None):
    """{'valid': bool [N], 'dist': (value [N], A, S), name: (value [N,C], A, S)}; not valid: the sentinel / the fill row, A = S = 0"""
    names = list(vol["sets"]) if names is None else list(names)
    ok, i, t = locate64(vol, pts)
    w = _weights(t)
    res = {"valid": ok}
    for k, arr, fill in _arrays(vol, names):
        v = np.where(ok[None, :, None], _corners(arr, i).astype(np.float64), 0.0)      # an invalid voxel's value is never used
        val = np.einsum("cn,cnk->nk", w, v)
        A = np.einsum("cn,cnk->nk", w, np.abs(v))
        S = v.max(axis=0) - v.min(axis=0)
        val = np.where(ok[:, None], val, fill.astype(np.float64)[None, :])
        A, S = np.where(ok[:, None], A, 0.0), np.where(ok[:, None], S, 0.0)
        res[k] = (val[:, 0], A[:, 0], S[:, 0]) if k == "dist" else (val, A, S)
    return res


def _dweights(t):
    """[3, 8, N]: d w_c / d t_a"""
    a = [np.stack([1.0 - t[:, k], t[:, k]]) for k in range(3)]
    sign = [-1.0, 1.0]
    out = np.empty((3, 8, t.shape[0]))
    for c, (dx, dy, dz) in enumerate(CORNERS):
        out[0, c] = sign[dx] * a[1][dy] * a[2][dz]
        out[1, c] = a[0][dx] * sign[dy] * a[2][dz]
        out[2, c] = a[0][dx] * a[1][dy] * sign[dz]
    return out


def trilinear_grad64(vol, pts, grad_dist=None, grads=None):
    """(grad_pts [N,3], B [N,3], T [N]) of sum(grad_dist * dist) + sum over names of sum(grad * rows): the analytic derivative of
    the chain for the cell the point lies in; zero rows where not valid.  grads: {name: [N,C] or None}."""
    grads = {k: g for k, g in (grads or {}).items() if g is not None}
    ok, i, t = locate64(vol, pts)
    dw = _dweights(t)
    h = float(vol["step"])
    N = pts.shape[0]
    grad, B, T = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N)
    todo = ([("dist", vol["dist"][..., None], np.asarray(grad_dist, np.float64)[:, None])] if grad_dist is not None else [])
    todo += [(k, vol["sets"][k], np.asarray(g, np.float64)) for k, g in grads.items()]
    for _, arr, g in todo:
        v = np.where(ok[None, :, None], _corners(arr, i).astype(np.float64), 0.0)
        grad += np.einsum("acn,cnk,nk->na", dw, v, g) / h
        B += np.einsum("acn,cnk,nk->na", np.abs(dw), np.abs(v), np.abs(g)) / h
        T += np.einsum("nk,nk->n", v.max(axis=0) - v.min(axis=0), np.abs(g)) / h
    grad[~ok], B[~ok], T[~ok] = 0.0, 0.0, 0.0
    return grad, B, T


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def coord_term(vol, S):
    """4 G 2^-24 S: with h a power of two the division is exact, the subtraction p - origin rounds once, so g (and t = g - i, an
    exact difference) is off by at most 2^-24 G per axis, G = max extent; |d out / d t_a| <= S; three axes, rounded up to 4."""
    return 4.0 * max(vol["shape"]) * U * S


def grad_coord_term(vol, T):
    """d out / d t_x depends on (t_y, t_z) only and changes by at most the spread of the four x-differences of the corners,
    <= 2 S, per unit of either: 2 axes x 2^-24 G x 2 S / h, weighted by |grad| and summed over the channels = 4 G 2^-24 T."""
    return 4.0 * max(vol["shape"]) * U * T


def worst_ratio(got, ref, scale, slack):
    """max over entries of (|got - ref| - slack) / scale, 0 where the slack covers the difference; inf where scale == 0 does not"""
    diff = np.abs(np.asarray(got, np.float64) - ref) - slack
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff <= 0, 0.0, diff / scale)
    return float(np.max(r)) if r.size else 0.0


def tolerance(port_worst):
    """three times the float32 port's worst ratio, capped at 16 x 2^-24"""
    return min(3.0 * port_worst, 16.0 * U)


# ---- a float32 NumPy port of the chain ----------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def locate32(vol, pts):
    f = np.float32
    n = np.asarray(vol["shape"])
    with np.errstate(invalid="ignore"):
        g = ((pts.astype(f) - np.asarray(vol["origin"], f)) / f(vol["step"])).astype(f)
        inside = np.all((g >= 0) & (g <= (n - 1).astype(f)), axis=1)
    gi = np.where(inside[:, None], g, f(0))
    i = np.minimum(np.floor(gi).astype(np.int64), n - 2)
    t = (gi - i.astype(f)).astype(f)
    ok = inside.copy()
    for dx, dy, dz in CORNERS:
        ok &= vol["valid"][i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz]
    return ok, i, t


def trilinear32(vol, pts, names=None):
    """{'valid', 'dist': [N], name: [N,C]} float32, operation by operation as the kernel"""
    names = list(vol["sets"]) if names is None else list(names)
    ok, i, t = locate32(vol, pts)
    w = _weights(t, np.float32).astype(np.float32)
    res = {"valid": ok}
    for k, arr, fill in _arrays(vol, names):
        v = np.where(ok[None, :, None], _corners(arr, i), np.float32(0))
        acc = w[0][:, None] * v[0]
        for c in range(1, 8):
            acc = _fma32(np.broadcast_to(w[c][:, None], v[c].shape), v[c], acc)
        acc = np.where(ok[:, None], acc, fill[None, :]).astype(np.float32)
        res[k] = acc[:, 0] if k == "dist" else acc
    return res


def trilinear_grad32(vol, pts, grad_dist=None, grads=None):
    """grad_pts [N,3] float32: per channel the derivative as the kernel forms it (face weights times corner differences, fma
    chain), summed over the channels one after the other in float32 -- the kernel's sum is a tree over sixteen lanes, whose
    rounding a sequential sum bounds from above in the usual case."""
    f = np.float32
    grads = {k: g for k, g in (grads or {}).items() if g is not None}
    ok, i, t = locate32(vol, pts)
    a = [np.stack([f(1) - t[:, k], t[:, k]]).astype(f) for k in range(3)]
    yz = [a[1][j >> 1] * a[2][j & 1] for j in range(4)]
    xz = [a[0][j >> 1] * a[2][j & 1] for j in range(4)]
    xy = [a[0][j >> 1] * a[1][j & 1] for j in range(4)]
    pairs = [(yz, [(4, 0), (5, 1), (6, 2), (7, 3)]), (xz, [(2, 0), (3, 1), (6, 4), (7, 5)]), (xy, [(1, 0), (3, 2), (5, 4), (7, 6)])]
    N = pts.shape[0]
    acc = np.zeros((N, 3), f)
    todo = ([(vol["dist"][..., None], np.asarray(grad_dist, f)[:, None])] if grad_dist is not None else [])
    todo += [(vol["sets"][k], np.asarray(g, f)) for k, g in grads.items()]
    for arr, g in todo:
        v = np.where(ok[None, :, None], _corners(arr, i), f(0))
        for ax, (wts, pr) in enumerate(pairs):
            d = wts[0][:, None] * (v[pr[0][0]] - v[pr[0][1]])
            for j in range(1, 4):
                d = _fma32(np.broadcast_to(wts[j][:, None], d.shape), v[pr[j][0]] - v[pr[j][1]], d)
            for ch in range(d.shape[1]):
                acc[:, ax] = _fma32(g[:, ch], d[:, ch], acc[:, ax])
    acc = (f(f(1) / f(vol["step"])) * acc).astype(f)
    acc[~ok] = 0
    return acc


# ---- cases --------------------------------------------------------------------------------------------------------------------
ORIGIN = (-0.5, -0.25, 0.125)
STEP = 2.0 ** -5
SHAPES = {"5x4x6": (5, 4, 6), "2x2x2": (2, 2, 2)}
SEEDS = tuple(range(12))


def make_volume(shape, channels, seed, invalid_frac=0.0, poison=False, fills=()):
    """Values: smooth + noise around an offset per channel (so that the chain's own rounding shows against A, not only the
    coordinate term against S); invalid voxels scattered; poison: NaN in dist and every row of an invalid voxel.  fills: indices
    of the sets that get a non-zero fill row."""
    rng = np.random.default_rng(1000 + seed)
    nx, ny, nz = shape
    vol = {"origin": np.asarray(ORIGIN, np.float32), "step": np.float32(STEP), "shape": tuple(shape), "sets": {}, "fills": {}}
    vol["dist"] = (0.3 * rng.standard_normal(shape) + rng.choice([0.0, 2.0])).astype(np.float32)
    valid = rng.random(shape) >= invalid_frac
    vol["valid"] = valid
    for s, C in enumerate(channels):
        offset = rng.choice([0.0, 3.0, -40.0], size=C)
        vol["sets"]["s%d" % s] = (rng.standard_normal(shape + (C,)) * rng.choice([0.05, 1.0], size=C) + offset).astype(np.float32)
        vol["fills"]["s%d" % s] = rng.standard_normal(C).astype(np.float32) if s in fills else None
    if poison:
        vol["dist"][~valid] = np.nan
        for k in vol["sets"]:
            vol["sets"][k][~valid] = np.nan
    return vol


def inside_points(shape, n, seed):
    """n float32 points with g = integer + U(0.01, 0.99) per axis.  Origin and step are short binary fractions, so the lattice is
    exact in float32; the ASSERT below -- in float64 on the float32 points -- is what lets validity be compared exactly: no
    point's g comes within 1e-4 of an integer, and the float32 g of the kernel is within 2^-24 G of it.  No point is filtered."""
    rng = np.random.default_rng(2000 + seed)
    cells = np.asarray(shape) - 1
    g = rng.integers(0, cells, size=(n, 3)) + rng.uniform(0.01, 0.99, size=(n, 3))
    pts = (np.asarray(ORIGIN, np.float64) + g * STEP).astype(np.float32)
    g32 = (pts.astype(np.float64) - np.asarray(ORIGIN, np.float64)) / STEP
    assert np.all(np.abs(g32 - np.round(g32)) >= 1e-4), "a generated point sits within 1e-4 of a lattice plane"
    assert np.all((g32 > 0) & (g32 < cells))
    return pts


def lattice_points(shape):
    """every lattice point, far faces included: exact in float32"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return (np.asarray(ORIGIN, np.float64) + idx * STEP).astype(np.float32)


def special_points(shape):
    """outside on every side (by half a cell, and by less than the 1e-4 margin of the random points: g = -2^-20 -- which
    float32 rounds onto the face for an axis whose origin is large enough, and both arithmetics agree on that -- and
    g = n - 1 + 2^-10), exactly on each near and far face, the two extreme corners, NaN / huge / infinite coordinates"""
    n = np.asarray(shape, np.float64)
    mid = (n - 1) / 2 + 0.25
    rows = []
    for a in range(3):
        for gval in (-0.5, n[a] - 0.5, -2.0 ** -20, n[a] - 1 + 2.0 ** -10, n[a] - 1, 0.0):
            g = mid.copy()
            g[a] = gval
            rows.append(g)
    rows += [n - 1, np.zeros(3)]
    pts = (np.asarray(ORIGIN, np.float64) + np.asarray(rows) * STEP).astype(np.float32)
    nan = np.repeat(pts[:1], 4, axis=0)
    nan[0, 0] = nan[1, 1] = nan[2, 2] = np.nan
    nan[3, :] = np.nan
    far = np.asarray([[1e30, 0, 0], [0, -1e30, 0], [np.inf, 0, 0], [0, 0, -np.inf]], np.float32)
    return np.concatenate([pts, nan, far])


@functools.lru_cache(maxsize=None)
def case(shape_name, channels, n, seed, invalid_frac=0.0, poison=False, fills=()):
    """(volume, points, float64 reference) -- built once per argument tuple and shared; callers do not modify it"""
    shape = SHAPES[shape_name]
    vol = make_volume(shape, channels, seed, invalid_frac, poison, fills)
    pts = inside_points(shape, n, seed)
    return vol, pts, trilinear64(vol, pts)
