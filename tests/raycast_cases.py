"""Float64 reference, float32 port and case generator of the ray march through a baked volume (d3f_volume_raycast,
include/d3fields_hip.h ABI 12), shared by tests/test_raycast_host.py and tests/test_gpu_raycast.py.

A volume is the dict of tests/volume_cases.py (origin, step, shape, dist, valid, sets, fills) plus mu (the truncation), kind
('plane' / 'sphere'), centre and normal (float64, the analytic surface).  march(vol, o, d, ..., f) restates the contract with every
operation in dtype f: f = float64 is the reference (it takes the float32 inputs as given), f = float32 the port, operation by
operation as the kernel.  Besides the outputs the reference returns per ray
    fragile   the ray sits on a knife edge of the contract (see FRAGILE below) and is left out of exact comparisons,
    scale     what one float32 rounding of the chain is worth in t* (scale_t) -- the bound's tol multiplies it --, and
    slack     the coordinate term 4 G 2^-24 S of section 13 propagated through prev / (prev - s)
(derivation: bound_terms below and DESIGN.md section 14).
"""
import functools
import itertools

import numpy as np

import volume_cases as VC

U = VC.U
CAP = 32.0 * U                      # at most 27 float32 roundings lie between the inputs and t*, each <= 2^-24 of a term of the scale
MAX_K = 131072.0
CORNERS = VC.CORNERS

# FRAGILE: thresholds of the knife edges
EPS_S = 1e-3                        # |s_k| < EPS_S mu at a sample up to the decision
EPS_FACE = 1e-4                     # a sample within this many lattice units of a face between cells of differing validity
EPS_K = 1e-3                        # (t1 - t0) / dt within this of an integer;  |t1 - t0| < EPS_K dt


def _fma(f):
    if f is np.float64:
        return lambda a, b, c: a * b + c
    return lambda a, b, c: VC._fma32(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))


def cell_valid(vol):
    v, (nx, ny, nz) = vol["valid"], vol["shape"]
    return np.all([v[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in CORNERS], axis=0)


MUTANTS = ("accumulated t_k", "back faces hit")


def march(vol, o, d, march_step=None, t_near=0.0, t_far=np.inf, f=np.float64, mutant=None):
    """-> dict(hit bool [N], t [N] (0: miss), points [N,3] (NaN: miss), samples int [N]); f = float64 adds fragile, scale_t, slack_t.
    mutant: one of MUTANTS breaks the contract on purpose -- t_k = t_{k-1} + dt instead of fma(k, dt, t0), or a - to + crossing taken
    for a hit -- so that the host tests can show which assert of the GPU tests catches that kernel."""
    assert mutant is None or mutant in MUTANTS
    ref = f is np.float64
    fma = _fma(f)
    n3 = np.asarray(vol["shape"])
    nm1 = (n3 - 1).astype(f)
    origin, h = vol["origin"].astype(f), f(vol["step"])
    ms = f(np.float32(vol["step"] if march_step is None else march_step))
    tn, tf = f(np.float32(t_near)), f(np.float32(t_far))
    o, d = np.asarray(o, np.float32).astype(f), np.asarray(d, np.float32).astype(f)
    N = o.shape[0]
    cv = cell_valid(vol)
    dist = vol["dist"]
    with np.errstate(all="ignore"):
        go, gd = ((o - origin) / h).astype(f), (d / h).astype(f)
        ln = np.sqrt(fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))).astype(f)
        live = np.isfinite(go).all(1) & np.isfinite(gd).all(1) & (ln > 0) & np.isfinite(ln)
        go, gd, ln = np.where(live[:, None], go, f(0)), np.where(live[:, None], gd, f(0)), np.where(live, ln, f(1))
        lo, hi = np.full(N, -np.inf, f), np.full(N, np.inf, f)
        for a in range(3):
            nz = gd[:, a] != 0
            den = np.where(nz, gd[:, a], f(1))
            ta, tb = ((f(0) - go[:, a]) / den).astype(f), ((nm1[a] - go[:, a]) / den).astype(f)
            lo = np.where(nz, np.maximum(lo, np.minimum(ta, tb)), lo)
            hi = np.where(nz, np.minimum(hi, np.maximum(ta, tb)), hi)
            live &= nz | ((go[:, a] >= 0) & (go[:, a] <= nm1[a]))
        t0, t1 = np.maximum(lo, tn), np.minimum(hi, tf)
        dt = (ms / ln).astype(f)
        q = ((t1 - t0) / dt).astype(f)
        Kf = np.floor(q)
        clipped = live.copy()
        live &= (t0 <= t1) & (Kf <= MAX_K)
    K = np.where(live, Kf, -1).astype(np.int64)
    t0 = np.where(live, t0, f(0))
    fragile = np.zeros(N, bool)
    if ref:
        with np.errstate(all="ignore"):
            fragile |= clipped & np.isfinite(t1 - t0) & (np.abs(t1 - t0) < EPS_K * dt)
            fragile |= live & (np.minimum(q - Kf, Kf + 1 - q) < EPS_K)
    prev = np.zeros(N, f)
    prev_terms = np.zeros((N, 3))                 # A, S, M of the sample that became prev
    hit, samples = np.zeros(N, bool), np.zeros(N, np.int64)
    t_hit = np.zeros(N, f)
    scale_t, slack_t = np.zeros(N), np.zeros(N)
    G = float(max(vol["shape"]))
    for k in range(int(K.max()) + 1 if N else 0):
        act = live & ~hit & (k <= K)
        if not act.any():
            break
        tk_before = fma(f(k - 1), dt, t0).astype(f)
        tk = fma(f(k), dt, t0).astype(f)
        if mutant == "accumulated t_k":
            tk_before = t0 if k == 0 else t_acc
            tk = t0 if k == 0 else (t_acc + dt).astype(f)
            t_acc = tk
        g = np.clip(fma(tk[:, None], gd, go).astype(f), f(0), nm1)
        g = np.where(act[:, None], g, f(0))
        i = np.minimum(np.floor(g).astype(np.int64), n3 - 2)
        tt = (g - i.astype(f)).astype(f)
        ok = cv[i[:, 0], i[:, 1], i[:, 2]]
        use = act & ok
        v = np.where(use[None, :], np.stack([dist[i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz] for dx, dy, dz in CORNERS]), np.float32(0)).astype(f)
        w = VC._weights(tt, f).astype(f)
        s = (w[0] * v[0]).astype(f)
        for c in range(1, 8):
            s = fma(w[c], v[c], s).astype(f)
        samples += act
        now = use & (prev > 0) & (s <= 0)
        if mutant == "back faces hit":
            now |= use & (prev < 0) & (s >= 0)
        with np.errstate(all="ignore"):
            th = fma(dt, (prev / (prev - s)).astype(f), tk_before).astype(f)
        t_hit = np.where(now, th, t_hit)
        if ref:
            A = np.einsum("cn,cn->n", w, np.abs(v))
            S = v.max(axis=0) - v.min(axis=0)
            M = (np.abs(go) + np.abs(tk[:, None] * gd)).sum(1)
            fragile |= use & (np.abs(s) < EPS_S * vol["mu"])
            for sg in itertools.product((-EPS_FACE, EPS_FACE), repeat=3):
                ip = np.minimum(np.floor(np.clip(g + np.asarray(sg), 0, nm1)).astype(np.int64), n3 - 2)
                fragile |= act & (cv[ip[:, 0], ip[:, 1], ip[:, 2]] != ok)
            with np.errstate(all="ignore"):
                den = (prev - s) ** 2
                sc = np.abs(th) + dt * (np.abs(s) * (prev_terms[:, 0] + prev_terms[:, 1] * prev_terms[:, 2]) + prev * (A + S * M)) / den
                sl = dt * (np.abs(s) * 4 * G * U * prev_terms[:, 1] + prev * 4 * G * U * S) / den
            scale_t, slack_t = np.where(now, sc, scale_t), np.where(now, sl, slack_t)
            prev_terms = np.where(use[:, None], np.stack([A, S, M], 1), prev_terms)
        prev = np.where(use, s, np.where(act, f(0), prev))
        hit |= now
    pts = np.where(hit[:, None], fma(t_hit[:, None], d, o).astype(f), f(np.nan))
    res = {"hit": hit, "t": t_hit, "points": pts, "samples": samples}
    if ref:
        res.update(fragile=fragile, scale_t=scale_t, slack_t=slack_t, d=d, o=o)
    return res


# ---- the bound --------------------------------------------------------------------------------------------------------------------
def bound_terms(ref):
    """(scale_t [N], slack_t [N], scale_p [N,3], slack_p [N,3]) at the reference's hits, zeros elsewhere.

    t* = t_{k-1} + dt r, r = p / (p - s) with p = prev > 0 >= s.  dr/dp = -s / (p - s)^2, dr/ds = p / (p - s)^2, so errors e_p, e_s of
    the two samples move t* by dt (|s| e_p + p e_s) / (p - s)^2.  A sample's error is tol (A + S M) + 4 G 2^-24 S: A = sum w_c |v_c| for
    the chain's own roundings, S M for the roundings of g_k beyond section 13's (|d out / d g_a| <= S; g_k = fma(t_k, gd, go) carries a
    few 2^-24 of |go_a| + |t_k gd_a|, summed over the axes = M, because a ray's origin may lie several boxes away), and section 13's
    coordinate term.  |t*| itself stands for the roundings of t_{k-1}, dt and the last fma.  A point is o + t* d."""
    st, sl, d, o = ref["scale_t"], ref["slack_t"], ref["d"], ref["o"]
    t = ref["t"]
    with np.errstate(invalid="ignore"):
        sp = np.abs(d) * st[:, None] + np.abs(o) + np.abs(t[:, None] * d)
        lp = np.abs(d) * sl[:, None]
    hit = ref["hit"]
    return st, sl, np.where(hit[:, None], sp, 0.0), np.where(hit[:, None], lp, 0.0)


def worst_ratios(got_t, got_p, ref, keep):
    """worst (|got - ref| - slack) / scale over t and the points of the rays in `keep` that hit"""
    st, sl, sp, lp = bound_terms(ref)
    m = keep & ref["hit"]
    if not m.any():
        return 0.0
    rt = VC.worst_ratio(np.asarray(got_t)[m], ref["t"][m], st[m], sl[m])
    rp = VC.worst_ratio(np.asarray(got_p)[m], ref["points"][m], sp[m], lp[m])
    return max(rt, rp)


def tolerance(port_worst):
    """three times the float32 port's worst ratio, capped at CAP"""
    return min(3.0 * port_worst, CAP)


def assert_equals_port(t, hit, pts, samples, port, keep, label=""):
    """On the rays in `keep` the kernel's outputs ARE the float32 port's: hit and sample count, and t and the points bit for bit.  The
    port does the contract's operations in the contract's order and every one of them is correctly rounded on both sides, so any
    other arithmetic -- an accumulated t_k, another fma order -- shows here however small its error.  samples may be None."""
    assert np.array_equal(np.asarray(hit)[keep], port["hit"][keep]), (label, "hit_mask differs from the float32 port")
    if samples is not None:
        assert np.array_equal(np.asarray(samples)[keep], port["samples"][keep]), (label, "sample counts differ from the float32 port")
    assert np.array_equal(np.asarray(t, np.float32)[keep], port["t"][keep]), (label, "t is not the float32 port's bit for bit")
    assert np.array_equal(np.asarray(pts, np.float32)[keep], port["points"][keep], equal_nan=True), (label, "points are not the float32 port's bit for bit")


# ---- volumes ----------------------------------------------------------------------------------------------------------------------
SHAPES = {"9x8x10": (9, 8, 10), "5x4x6": (5, 4, 6), "2x2x2": (2, 2, 2)}
FAMILIES = {"pow2": (np.float32(2.0 ** -5), (-0.5, -0.25, 0.125)), "4mm": (np.float32(0.004), (-0.35, 0.11, -0.2))}
PLANE_NORMAL = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
MU_STEPS = 3.0
HOLES = 0.01                        # of the voxels, at least one: 7 of 720 (up to 56 of 504 cells), 1 of 120 (up to 8 of 60 cells)
RADIUS = 0.45                       # of the smallest extent
# 2x2x2: no sphere (no ray hits one there) and no holes (3 % of eight voxels is none, and one would leave no cell)
VOLUMES = [(shape, kind, family, holes) for shape in SHAPES for kind in ("plane", "sphere") for family in FAMILIES for holes in (False, True)
           if not (shape == "2x2x2" and (kind == "sphere" or holes))]


@functools.lru_cache(maxsize=None)
def make_volume(shape_name, kind, family, holes, channels=(), fills=()):
    """A plane through the box centre (free space on the side of PLANE_NORMAL) or a sphere around it (free space outside), as a
    signed distance clamped to +- mu = 3 h and stored in float32; holes: <= 3 % invalid voxels, dist (and every row) NaN there."""
    shape = SHAPES[shape_name]
    step, origin = FAMILIES[family]
    origin = np.asarray(origin, np.float32)
    h = float(step)
    rng = np.random.default_rng(3000 + 17 * list(SHAPES).index(shape_name) + 5 * (kind == "sphere") + 3 * (family == "4mm"))
    ext = (np.asarray(shape) - 1) * h
    centre = origin.astype(np.float64) + ext / 2
    X = np.stack(np.meshgrid(*[float(origin[a]) + h * np.arange(shape[a]) for a in range(3)], indexing="ij"), -1) - centre
    sd = X @ PLANE_NORMAL if kind == "plane" else np.linalg.norm(X, axis=-1) - RADIUS * ext.min()
    mu = MU_STEPS * h
    vol = {"origin": origin, "step": step, "shape": shape, "mu": mu, "kind": kind, "centre": centre, "normal": PLANE_NORMAL,
           "radius": RADIUS * ext.min(), "dist": np.clip(sd, -mu, mu).astype(np.float32), "sets": {}, "fills": {}}
    valid = np.ones(shape, bool)
    if holes:
        valid.reshape(-1)[rng.choice(valid.size, max(1, int(HOLES * valid.size)), replace=False)] = False
    vol["valid"] = valid
    for s, C in enumerate(channels):
        vol["sets"]["s%d" % s] = (rng.standard_normal(shape + (C,)) + rng.choice([0.0, 3.0], size=C)).astype(np.float32)
        vol["fills"]["s%d" % s] = rng.standard_normal(C).astype(np.float32) if s in fills else None
    vol["dist"][~valid] = np.nan
    for k in vol["sets"]:
        vol["sets"][k][~valid] = np.nan
    return vol


# ---- rays -------------------------------------------------------------------------------------------------------------------------
def random_rays(vol, n, seed):
    """origins in free space (the + side of the plane / outside the sphere) one to two box sizes from the centre, each aimed at a
    random point of the box; |d| in [0.5, 2].  Every eighth ray starts BEHIND the surface instead (the - side of the plane at the
    same distance, inside the sphere): it meets the surface from - to +, which is no hit."""
    rng = np.random.default_rng(4000 + seed)
    h = float(vol["step"])
    ext = (np.asarray(vol["shape"]) - 1) * h
    c = vol["centre"]
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if vol["kind"] == "plane":
        u = np.where((u @ vol["normal"] < 0)[:, None], u - 2 * (u @ vol["normal"])[:, None] * vol["normal"], u)
    o = c + u * ext.max() * rng.uniform(1.0, 2.0, size=(n, 1))
    behind = (np.arange(n) % 8 == 7)[:, None]
    if vol["kind"] == "plane":
        o = np.where(behind, o - 2 * ((o - c) @ vol["normal"])[:, None] * vol["normal"], o)
    else:
        o = np.where(behind, c + u * vol["radius"] * rng.uniform(0.1, 0.6, size=(n, 1)), o)
    tgt = c + (rng.random((n, 3)) - 0.5) * ext
    d = tgt - o
    d *= rng.uniform(0.5, 2.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


SPECIALS = ["misses the box", "starts inside", "axis-parallel inside the slab", "axis-parallel outside the slab", "two zero components", "back face",
            "d = 0", "NaN origin", "NaN direction", "infinite origin", "d = 0 inside the box"]


def special_rays(vol):
    """the hand-made rays of SPECIALS, in that order"""
    h = float(vol["step"])
    n3 = np.asarray(vol["shape"])
    ext = (n3 - 1) * h
    c, org = vol["centre"], vol["origin"].astype(np.float64)
    nrm = vol["normal"]
    inside = org + (n3 - 1) * np.array([0.37, 0.41, 0.63]) * h               # a point of the box off every lattice plane
    top = inside.copy()
    top[2] = org[2] + (n3[2] - 1 - 0.37) * h                                 # ... near the +z face: an axis-parallel ray from here crosses a
    if vol["kind"] == "plane":                   # in the box on the free side, looking at the plane; behind the plane, looking through it
        start, back = (c + 0.3 * ext * nrm, -nrm * 0.9 + np.array([0.05, 0.02, 0.0])), (c - 1.5 * ext.max() * nrm, nrm + np.array([0.03, 0.0, 0.01]))
    else:                                        # in a corner of the box, looking at the centre; in the sphere, looking out
        corner = org + (n3 - 1) * np.array([0.93, 0.9, 0.94]) * h
        start, back = (corner, (c - corner) * 1.1 / np.linalg.norm(c - corner)), (c + 0.2 * vol["radius"] * nrm, nrm + np.array([0.03, 0.0, 0.01]))
    rows = [(c + np.array([3.0, 0.2, 0.1]) * ext.max(), np.array([0.1, 1.0, 0.2])),      # fractional number of steps (from outside it is ext / step, an integer)
            start,
            (top, np.array([0.0, 0.013, -0.77])),
            (top + np.array([2.0 * ext[0], 0.0, 0.0]), np.array([0.0, 0.013, -0.77])),
            (top, np.array([0.0, 0.0, -1.3])),
            back,
            (c + 1.5 * ext.max() * nrm, np.zeros(3)),
            (np.array([np.nan, c[1], c[2]]), -nrm),
            (c + 1.5 * ext.max() * nrm, np.array([0.0, np.nan, -1.0])),
            (np.array([np.inf, c[1], c[2]]), np.array([-1.0, 0.0, 0.0])),
            (inside, np.zeros(3))]
    assert len(rows) == len(SPECIALS)
    return np.asarray([r[0] for r in rows], np.float32), np.asarray([r[1] for r in rows], np.float32)


COUNTS = (1, 63, 1003)
# (march_step / h, window): the window's t_far is the 80th percentile of the default march's t*, which cuts a fifth of the hits off
VARIANTS = {"default": (1.0, False), "half step": (0.5, False), "double step": (2.0, False), "window": (1.0, True)}
# One seed per ray count.  The 63-ray cases use seed 1: with seed 0 fifteen of them miss a condition of
# test_raycast_host.py::test_every_case_keeps_its_conditions -- two fragile rays of 63 are 3.2 % (the 9x8x10 spheres and 2x2x2; the
# cap allows one), or fewer than a quarter of the rays hit (5x4x6 spheres with a hole, the window on the spheres) -- and with seed 1
# none does (seeds 2, 3 and 4 leave 6, 3 and 8).  The float64 reference alone decides this; the 1- and 1003-ray cases keep seed 0.
SEED_OF_COUNT = {1: 0, 63: 1, 1003: 0}


def case_list():
    """every (volume key, n, variant): the default march at every count on every volume, the variants at 63 and 1003 rays on the 9x8x10 volumes
    (a step of 2 h strides over most of what a 5x4x6 box holds)"""
    out = [(v, n, "default") for v in VOLUMES for n in COUNTS]
    out += [(v, n, var) for v in VOLUMES if v[0] == "9x8x10" for n in (63, 1003) for var in ("half step", "double step", "window")]
    return out


@functools.lru_cache(maxsize=None)
def case(volume_key, n, variant="default"):
    """(vol, o, d, kwargs of march, float64 reference) -- built once and shared; callers do not modify it.  From 63 rays on the first
    len(SPECIALS) rays are the hand-made ones."""
    vol = make_volume(*volume_key)
    seed = SEED_OF_COUNT[n]
    o, d = random_rays(vol, n, seed)
    if n >= 63:
        so, sd = special_rays(vol)
        o[:len(so)], d[:len(sd)] = so, sd
    factor, window = VARIANTS[variant]
    kw = {"march_step": np.float32(np.float32(vol["step"]) * np.float32(factor)), "t_near": 0.0, "t_far": np.inf}
    if window:
        base = march(vol, o, d, **kw)
        kw["t_near"] = np.float32(0.25 * np.median(base["t"][base["hit"]]))
        kw["t_far"] = np.float32(np.percentile(base["t"][base["hit"]], 80))
    return vol, o, d, kw, march(vol, o, d, **kw)


def camera_rays(K, pose, H, W):
    """(o [3] float32, d [H*W,3] float32) by the entry point's formulas: o = -R^T tc in float64, rounded; d in float32 fma chains"""
    K, pose = np.asarray(K, np.float32), np.asarray(pose, np.float32)[:3]
    R, tc = pose[:, :3], pose[:, 3]
    o = (-(R.astype(np.float64).T @ tc.astype(np.float64))).astype(np.float32)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    dcx = ((u.reshape(-1) - K[0, 2]) / K[0, 0]).astype(np.float32)
    dcy = ((v.reshape(-1) - K[1, 2]) / K[1, 1]).astype(np.float32)
    d = np.stack([(VC._fma32(np.broadcast_to(R[1, a], dcy.shape), dcy, (R[0, a] * dcx).astype(np.float32)) + R[2, a]).astype(np.float32) for a in range(3)], 1)
    return o, d
