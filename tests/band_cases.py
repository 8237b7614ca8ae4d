"""NumPy restatement and case generator of the surface band of a baked volume (d3f_band_mark / d3f_band_sample, include/d3fields_hip.h
ABI 13), shared by tests/test_band_host.py and tests/test_gpu_band.py.

A volume is the dict of tests/raycast_cases.py (origin, step, shape, dist, valid, sets, fills, mu, kind, ...).  mark(vol, band) restates
the contract:
    seed    valid & |dist| < band (strict; NaN is no seed) -- both sides are float32 values, so the comparison is the same in any
            wider arithmetic; the generator keeps every valid voxel's |dist| at least 1e-3 band away from band all the same;
    kept    a cell whose eight corners are valid and that has a seed corner            -> cell_band [nx-1, ny-1, nz-1]
    stored  a voxel that is a corner of a kept cell                                    -> stored [nx, ny, nz]
    slot    rank among the stored voxels in ascending flat index, -1 elsewhere         -> slot int32 [nx, ny, nz], voxels [M]
in_band(vol, m, pts) is the float64 lookup's side: valid (volume_cases.locate64) and the point's cell kept.
"""
import functools

import numpy as np

import raycast_cases as RC
import volume_cases as VC

CORNERS = VC.CORNERS
SEED_MARGIN = 1e-3                  # of band: no valid voxel's |dist| lies closer to band
SELECTIVE = (0.25, 0.75)            # a selective case keeps this share of the valid cells


def mark(vol, band):
    """-> dict(band float32, seed, cell_valid, cell_band, stored (bool volumes), slot int32 [nx,ny,nz], voxels int32 [M], M)"""
    band = np.float32(band)
    assert np.isfinite(band) and band > 0
    nx, ny, nz = vol["shape"]
    with np.errstate(invalid="ignore"):
        seed = vol["valid"] & (np.abs(vol["dist"].astype(np.float64)) < np.float64(band))
    cv = RC.cell_valid(vol)
    any_seed = np.any([seed[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in CORNERS], axis=0)
    cell_band = cv & any_seed
    stored = np.zeros(vol["shape"], bool)
    for dx, dy, dz in CORNERS:
        stored[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] |= cell_band
    flat = stored.reshape(-1)
    voxels = np.flatnonzero(flat).astype(np.int32)
    slot = np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32).reshape(vol["shape"])
    return {"band": band, "seed": seed, "cell_valid": cv, "cell_band": cell_band, "stored": stored, "slot": slot, "voxels": voxels, "M": int(voxels.size)}


def in_band(vol, m, pts):
    """(valid [N], in_band [N]) of the float64 lookup"""
    ok, i, _ = VC.locate64(vol, pts)
    return ok, ok & m["cell_band"][i[:, 0], i[:, 1], i[:, 2]]


def seed_margin(vol, band):
    """min over the valid voxels of | |dist| - band | / band"""
    d = np.abs(vol["dist"][vol["valid"]].astype(np.float64))
    return float(np.min(np.abs(d - float(np.float32(band)))) / float(np.float32(band))) if d.size else np.inf


def kept_share(m):
    """kept cells / valid cells"""
    return float(m["cell_band"].sum()) / max(int(m["cell_valid"].sum()), 1)


# ---- volumes ----------------------------------------------------------------------------------------------------------------------
# The committed raycast fixtures (9x8x10, 5x4x6, 2x2x2; mu = 3 h) are too small to be selective: they are the "everything (or nearly
# everything) kept" cases.  Two larger volumes, built the same way (a plane through the box centre / a sphere around it, signed
# distance clamped to +- 3 h, 1 % holes with NaN in the invalid voxels), are: at band = h and band = h / 2 they keep between a
# quarter and three quarters of the valid cells, which test_band_host.py asserts.
# The plane's box is 17x12x11: in a 16x12x14 box the centred plane passes THROUGH voxels (dist = 0 there: no band lies below every
# |dist|) and band = h / 2 keeps 24 % of the cells, under the cap; 17x12x11 keeps 30-41 % and its smallest |dist| is 0.05 h.
LARGE = {"plane": (17, 12, 11), "sphere": (16, 12, 14)}
FAMILY = "4mm"                      # step 0.004, an origin that is no short binary fraction: |dist| never ties with band


@functools.lru_cache(maxsize=None)
def large_volume(kind, holes, channels=(), fills=()):
    shape = LARGE[kind]
    step, origin = RC.FAMILIES[FAMILY]
    origin = np.asarray(origin, np.float32)
    h = float(step)
    rng = np.random.default_rng(5000 + 5 * (kind == "sphere") + 3 * bool(holes))
    ext = (np.asarray(shape) - 1) * h
    centre = origin.astype(np.float64) + ext / 2
    X = np.stack(np.meshgrid(*[float(origin[a]) + h * np.arange(shape[a]) for a in range(3)], indexing="ij"), -1) - centre
    sd = X @ RC.PLANE_NORMAL if kind == "plane" else np.linalg.norm(X, axis=-1) - RC.RADIUS * ext.min()
    mu = RC.MU_STEPS * h
    vol = {"origin": origin, "step": step, "shape": shape, "mu": mu, "kind": kind, "centre": centre, "normal": RC.PLANE_NORMAL,
           "radius": RC.RADIUS * ext.min(), "dist": np.clip(sd, -mu, mu).astype(np.float32), "sets": {}, "fills": {}}
    valid = np.ones(shape, bool)
    if holes:
        valid.reshape(-1)[rng.choice(valid.size, max(1, int(RC.HOLES * valid.size)), replace=False)] = False
    vol["valid"] = valid
    for s, C in enumerate(channels):
        vol["sets"]["s%d" % s] = (rng.standard_normal(shape + (C,)) + rng.choice([0.0, 3.0], size=C)).astype(np.float32)
        vol["fills"]["s%d" % s] = rng.standard_normal(C).astype(np.float32) if s in fills else None
    vol["dist"][~valid] = np.nan
    for k in vol["sets"]:
        vol["sets"][k][~valid] = np.nan
    return vol


# name -> (builder key, band in steps, selective?)
def _cases():
    out = {}
    for kind in ("plane", "sphere"):
        for holes in (False, True):
            for steps in (1.0, 0.5):
                out["large %s%s band %gh" % (kind, " holes" if holes else "", steps)] = (("large", kind, holes), steps, True)
    for key in RC.VOLUMES:
        shape, kind, family, holes = key
        if family != FAMILY:
            continue
        out["%s %s%s band 1.5h" % (shape, kind, " holes" if holes else "")] = (("raycast",) + key, 1.5, False)
    return out


CASES = _cases()
ABOVE_MU = 3.5                      # in steps: above mu = 3 h, every valid cell is kept
BELOW_ALL = 1e-4                    # in steps: below the smallest |dist| of the EMPTY_CASES volumes (asserted on the host): M == 0
EMPTY_CASES = [k for k in CASES if not k.startswith("2x2x2")]      # the 2x2x2 plane passes through two of its eight voxels


def volume(case_name, channels=(), fills=()):
    key = CASES[case_name][0]
    if key[0] == "large":
        return large_volume(key[1], key[2], tuple(channels), tuple(fills))
    return RC.make_volume(*key[1:], channels=tuple(channels), fills=tuple(fills))


def band_of(case_name, steps=None):
    """the band of a case as the float32 world length the entry point gets"""
    vol = volume(case_name)
    return np.float32(float(vol["step"]) * (CASES[case_name][1] if steps is None else steps))


# ---- points -----------------------------------------------------------------------------------------------------------------------
def _to_volume(vol, pts_vc, shape):
    """volume_cases generates points for ITS origin and step; move them onto this volume's lattice (same g) in float64, round once"""
    g = (pts_vc.astype(np.float64) - np.asarray(VC.ORIGIN, np.float64)) / VC.STEP
    return (vol["origin"].astype(np.float64) + g * float(vol["step"])).astype(np.float32)


def inside_points(vol, n, seed):
    """volume_cases.inside_points on this volume's lattice; the 1e-4 margin from the lattice planes is asserted again after the move"""
    pts = _to_volume(vol, VC.inside_points(vol["shape"], n, seed), vol["shape"])
    g = (pts.astype(np.float64) - vol["origin"].astype(np.float64)) / float(vol["step"])
    assert np.all(np.abs(g - np.round(g)) >= 1e-4), "a generated point sits within 1e-4 of a lattice plane"
    assert np.all((g > 0) & (g < np.asarray(vol["shape"]) - 1))
    return pts


def lattice_points(vol):
    """every lattice point as the float32 sum the field itself forms for a voxel centre: origin + i * step, products and sums in float32"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in vol["shape"]], indexing="ij"), axis=-1).reshape(-1, 3)
    return (vol["origin"] + idx.astype(np.float32) * np.float32(vol["step"])).astype(np.float32)


def special_points(vol):
    """volume_cases.special_points (outside on every side, the faces, NaN, huge, infinite) on this volume's lattice.  Points ON a face or
    within 2^-10 of one are knife edges of `valid` for a step that is no power of two; the tests compare them against the DENSE field of
    the same device, never against float64."""
    return _to_volume(vol, VC.special_points(vol["shape"]), vol["shape"])


def rays(vol, n=257, seed=0):
    """raycast_cases.random_rays with the hand-made special rays in front"""
    o, d = RC.random_rays(vol, n, seed)
    so, sd = RC.special_rays(vol)
    o[:len(so)], d[:len(sd)] = so, sd
    return o, d
