"""Cases for channel sets STORED as IEEE half (d3f_volume_set's storage word D3F_DTYPE_F16).  NumPy only.

The volumes are volume_cases.make_volume's (same origin, step, dist, valid, fill rows) with every set re-drawn as float16 BIT PATTERNS:
  * uniformly random finite halves of both signs -- the exponent is uniform, so a twentieth of them are subnormal;
  * planted in the valid voxels where there is room: +0, -0, +-65504 (the largest finite half), the smallest and the largest subnormal
    of either sign (PLANTED);
  * channel 0 of the eight corners of cell (0, 0, 0) is negative, its corner (0, 0, 0) is -0, and the eight voxels are valid: at the
    lattice point (0, 0, 0) the weights are 1 and seven zeros, every product of the chain is -0, and the chain out = w0 * v0,
    fma(w_c, v_c, out) returns -0.  A first term formed as fma(w0, v0, +0) returns +0: other bits;
  * with `poison`, every row of an invalid voxel is half NaN, +Inf or -Inf in turn (dist is NaN there, as in volume_cases).
vol["bits"][name] is the uint16 array the field stores, vol["sets"][name] its exact widening to float32: the reference input of
volume_cases.trilinear32 / trilinear64 / trilinear_grad64, which take the volume as it is."""
import functools

import numpy as np

import band_cases as BC
import volume_cases as VC

SHAPES = VC.SHAPES                                      # "5x4x6", "2x2x2"
inside_points, lattice_points, special_points = VC.inside_points, VC.lattice_points, VC.special_points

H_NAN, H_INF, H_NINF = 0x7E00, 0x7C00, 0xFC00
H_NEG_ZERO = 0x8000
PLANTED = (0x0000, H_NEG_ZERO, 0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x83FF)      # +-0, +-65504, the extreme subnormals
CELL0 = [(dx, dy, dz) for dx, dy, dz in VC.CORNERS]                                # the corners of cell (0, 0, 0)


def widen(bits):
    """uint16 bit patterns -> the float32 of the same value (exact: every half is a float32)"""
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float32)


def make_volume(shape, channels, seed, invalid_frac=0.0, poison=False, fills=()):
    vol = VC.make_volume(shape, channels, seed, invalid_frac, poison, fills)
    rng = np.random.default_rng(7000 + seed)
    valid = vol["valid"]
    for dx, dy, dz in CELL0:
        valid[dx, dy, dz] = True
    if poison:                                          # (volume_cases poisoned dist before the eight voxels were made valid)
        fix = np.isnan(vol["dist"]) & valid
        vol["dist"][fix] = np.float32(0.25)
    vol["bits"] = {}
    for s, C in enumerate(channels):
        k = "s%d" % s
        bits = rng.integers(0, 0x7C00, size=tuple(shape) + (C,), dtype=np.uint16) | (rng.integers(0, 2, size=tuple(shape) + (C,), dtype=np.uint16) << 15)
        protected = np.zeros(bits.shape, bool)
        for dx, dy, dz in CELL0:
            bits[dx, dy, dz, 0] |= 0x8000
            bits[dx, dy, dz, 0] = max(int(bits[dx, dy, dz, 0]), 0x8001)            # negative and not zero
            protected[dx, dy, dz, 0] = True
        bits[0, 0, 0, 0] = H_NEG_ZERO
        room = np.flatnonzero((valid[..., None] & ~protected).reshape(-1))
        spots = rng.choice(room, size=min(len(PLANTED), room.size), replace=False) if room.size else []
        for at, value in zip(spots, PLANTED):
            bits.reshape(-1)[at] = value
        if poison:
            bad = np.argwhere(~valid)
            for j, (x, y, z) in enumerate(bad):
                bits[x, y, z, :] = (H_NAN, H_INF, H_NINF)[j % 3]
        vol["bits"][k] = bits
        vol["sets"][k] = widen(bits)
    return vol


def points(shape, n, seed):
    """n points: the lattice point (0, 0, 0) (where the -0 is decided), the special points (outside, the faces, NaN, infinite), the
    other lattice points (t = 0 and t = 1 on every axis) and random interior points, in that order, cut to n"""
    lat = lattice_points(shape)
    pool = np.concatenate([lat[:1], special_points(shape), lat[1:], inside_points(shape, 300, seed)])
    assert n <= len(pool)
    return np.ascontiguousarray(pool[:n])


@functools.lru_cache(maxsize=None)
def case(shape_name, channels, seed, invalid_frac=0.0, poison=False, fills=()):
    """the volume of a case: built once per argument tuple and shared; callers do not modify it"""
    return make_volume(SHAPES[shape_name], channels, seed, invalid_frac, poison, fills)


def band_of(vol):
    """a band (float32 world length) that no valid voxel's |dist| ties with and that splits them: the midpoint of the two middle values"""
    d = np.sort(np.abs(vol["dist"][vol["valid"]].astype(np.float64)))
    d = d[np.isfinite(d)]
    mid = len(d) // 2
    return np.float32((d[mid - 1] + d[mid]) / 2) if len(d) > 1 and d[mid] > d[mid - 1] else np.float32(d[-1] * 2 + 1)


def mark(vol, band):
    """band_cases.mark of the volume: the restatement of d3f_band_mark (slot, voxels, M, cell_band)"""
    return BC.mark({"shape": vol["shape"], "dist": vol["dist"], "valid": vol["valid"]}, np.float32(band))
