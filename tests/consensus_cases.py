"""NumPy restatement, bounds and cases of the consensus poses (d3f_pose_consensus_* / d3f_pose_refit, include/d3fields_hip.h),
shared by tests/test_consensus_host.py and tests/test_gpu_consensus.py.

The contract, restated.  Model points p float32 [M, 3], candidates c float32 [M, k, 3] (a NaN coordinate: padding), triplets int32 [n_trip, 3]
with i < j < l.  A hypothesis is h = (trip * k + a) * k * k + b * k + c.  Only IEEE + - * / sqrt in the stated order and no fma, so NumPy gives
the device's bits and the tests ask for equality.
  gate (float64):  u = p_j - p_i, v = p_l - p_i, w = v - u;  U = c_jb - c_ia, V = c_lc - c_ia, W = V - U;  |x|^2 = (x0 x0 + x1 x1) + x2 x2;
    a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).  Rejected: a NaN candidate coordinate; not (|u|, |v|, |w| >= min_side); not
    (||U| - |u||, ... <= side_tol); not (|u x v|^2 >= (min_sin^2 |u|^2) |v|^2) or not the same of (U, V).  A rejected hypothesis has count 0.
  pose (float64):  e1 = u / |u|, e3 = (u x v) / |u x v|, e2 = e3 x e1; f the same of (U, V);  R_ab = (f1_a e1_b + f2_a e2_b) + f3_a e3_b;
    ps = ((p_i + p_j) + p_l) / 3, cs the same;  t_a = cs_a - ((R_a0 ps_0 + R_a1 ps_1) + R_a2 ps_2);  rounded once to float32.
  score (float32):  x_a = ((R_a0 p_x + R_a1 p_y) + R_a2 p_z) + t_a;  d2 = (dx dx + dy dy) + dz dz;  the assignment of q is the s with the smallest
    d2 <= tau2, ties to the lower s, else -1;  count = the assigned points.
  selection:  survivors have count >= min_inliers; ordered by (count descending, h ascending); the best max_survivors are kept; n_poses greedy
    rounds, each killing the survivors that share at least `shared` identical (point, candidate) assignments with the pick.  Integer-exact and
    order-independent.
  refit:  Horn's closed form in float64 over the assigned pairs; here by numpy.linalg.eigh, which is the reference of the device's Jacobi.
"""
import functools

import numpy as np

F = np.float32
MAX_M, MAX_K = 64, 8
EPS = 2.0 ** -53


def all_triplets(M):
    return np.array([(i, j, l) for i in range(M) for j in range(i + 1, M) for l in range(j + 1, M)], np.int32).reshape(-1, 3)


def _norm2(x):
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def digits_of(h, k):
    rem = h % (k ** 3)
    return h // (k ** 3), rem // (k * k), (rem // k) % k, rem % k


def gate_pose(p, c, trip, side_tol, min_side, min_sin):
    """-> (live bool [T], pose float32 [T, 12]: R row-major then t, zeros where rejected)"""
    p, c = np.asarray(p, F), np.asarray(c, F)
    k = c.shape[1]
    T = len(trip) * k ** 3
    tr, da, db, dc = digits_of(np.arange(T, dtype=np.int64), k)
    i, j, l = trip[tr, 0], trip[tr, 1], trip[tr, 2]
    pi, pj, pl = (p[x].astype(np.float64) for x in (i, j, l))
    ci, cj, cl = c[i, da].astype(np.float64), c[j, db].astype(np.float64), c[l, dc].astype(np.float64)
    with np.errstate(all="ignore"):
        nan = np.isnan(ci).any(1) | np.isnan(cj).any(1) | np.isnan(cl).any(1)
        u, v = pj - pi, pl - pi
        w = v - u
        U, V = cj - ci, cl - ci
        W = V - U
        u2, v2, U2, V2 = _norm2(u), _norm2(v), _norm2(U), _norm2(V)
        mu, mv, mw = np.sqrt(u2), np.sqrt(v2), np.sqrt(_norm2(w))
        oU, oV, oW = np.sqrt(U2), np.sqrt(V2), np.sqrt(_norm2(W))
        live = ~nan & (mu >= min_side) & (mv >= min_side) & (mw >= min_side)
        live &= (np.abs(oU - mu) <= side_tol) & (np.abs(oV - mv) <= side_tol) & (np.abs(oW - mw) <= side_tol)
        n, N = _cross(u, v), _cross(U, V)
        n2, N2 = _norm2(n), _norm2(N)
        ms2 = float(min_sin) * float(min_sin)
        live &= (n2 >= (ms2 * u2) * v2) & (N2 >= (ms2 * U2) * V2)
        e1, e3 = u / mu[:, None], n / np.sqrt(n2)[:, None]
        f1, f3 = U / oU[:, None], N / np.sqrt(N2)[:, None]
        e2, f2 = _cross(e3, e1), _cross(f3, f1)
        ps = ((pi + pj) + pl) / 3.0
        cs = ((ci + cj) + cl) / 3.0
        R = (f1[:, :, None] * e1[:, None, :] + f2[:, :, None] * e2[:, None, :]) + f3[:, :, None] * e3[:, None, :]
        t = cs - ((R[:, :, 0] * ps[:, None, 0] + R[:, :, 1] * ps[:, None, 1]) + R[:, :, 2] * ps[:, None, 2])
        pose = np.concatenate([R.reshape(T, 9), t], axis=1).astype(F)
    pose[~live] = 0
    return live, pose


def score(pose, p, c, tau2):
    """pose float32 [L, 12] -> (count int [L], assign int8 [L, M]) in float32, operation by operation"""
    pose, p, c, tau2 = np.asarray(pose, F), np.asarray(p, F), np.asarray(c, F), F(tau2)
    L, M = len(pose), len(p)
    assign = np.full((L, M), -1, np.int8)
    with np.errstate(all="ignore"):
        for lo in range(0, L, 4096):
            P = pose[lo:lo + 4096]
            x = [((P[:, None, 3 * a] * p[None, :, 0] + P[:, None, 3 * a + 1] * p[None, :, 1]) + P[:, None, 3 * a + 2] * p[None, :, 2]) + P[:, None, 9 + a] for a in range(3)]
            d = [x[a][:, :, None] - c[None, :, :, a] for a in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert d2.dtype == F
            ok = d2 <= tau2
            s = np.argmin(np.where(ok, d2, np.inf), axis=2)              # the first minimum: ties to the lower s
            assign[lo:lo + 4096] = np.where(ok.any(axis=2), s, -1)
    return (assign >= 0).sum(axis=1), assign


def order(count, h):
    """the indices that sort by (count descending, h ascending)"""
    return np.lexsort((h, -count.astype(np.int64)))


def greedy(h, count, assign, n_poses, shared):
    """h, count, assign of the kept survivors -> the picked indices into them, by rounds"""
    alive = np.ones(len(h), bool)
    rank = order(count, h)
    picks = []
    for _ in range(n_poses):
        live = rank[alive[rank]]
        if len(live) == 0:
            break
        w = live[0]
        picks.append(w)
        same = ((assign == assign[w]) & (assign >= 0)).sum(axis=1)
        alive &= same < shared
        alive[w] = False
    return picks


def horn(p, c):
    """the least-squares rigid motion c ~ R p + t over paired rows, float64 -> (R, t, eigenvalues ascending, the 4 x 4 matrix N)"""
    p, c = np.asarray(p, np.float64), np.asarray(c, np.float64)
    pm, cm = p.mean(axis=0), c.mean(axis=0)
    S = (p - pm).T @ (c - cm)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [0, S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [0, 0, -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [0, 0, 0, -S[0, 0] - S[1, 1] + S[2, 2]]])
    N = N + np.triu(N, 1).T
    lam, vec = np.linalg.eigh(N)
    q0, q1, q2, q3 = vec[:, 3]
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]]) / (vec[:, 3] @ vec[:, 3])
    return R, cm - R @ pm, lam, N


def kabsch(p, c):
    """the same motion by the SVD of the cross-covariance: the independent formulation"""
    p, c = np.asarray(p, np.float64), np.asarray(c, np.float64)
    pm, cm = p.mean(axis=0), c.mean(axis=0)
    Uu, _, Vt = np.linalg.svd((c - cm).T @ (p - pm))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Uu @ Vt))])
    R = Uu @ D @ Vt
    return R, cm - R @ pm


def refit_bound(p, c):
    """How far the device's refit may move a model point from the restatement's, as a world length.  Cyclic Jacobi in float64 returns the top
    eigenvector of N to within about n eps |N| / gap (n = 4, |N| the spectral norm, gap the distance of the largest eigenvalue from the next;
    Demmel & Veselic 1992 give the relative form); eigh carries the same bound.  The quaternion's error moves R by at most four times that, a
    point by 4 |p - pm|, and t = cm - R pm with it.  Before that, S itself is a sum of n_pairs products rounded in another order: n_pairs eps
    |N| / gap again.  Then both poses are rounded to float32: 2^-24 (|R p| + |t|) each, and the point is formed in float32 by the caller: the
    test measures in float64 from the float32 poses, so only the two roundings count.  A factor 100 covers the constants, in the style of
    the 100 cond 2^-53 of align's step test.  -> (bound, gap / |N|)"""
    p, c = np.asarray(p, np.float64), np.asarray(c, np.float64)
    _, t, lam, N = horn(p, c)
    gap = lam[3] - lam[2]
    norm = np.abs(lam).max()
    radius = np.linalg.norm(p - p.mean(axis=0), axis=1).max()
    scale = np.abs(p).max() * 3 + np.abs(t).max()
    return 100.0 * (4 + len(p)) * EPS * norm / gap * 4 * radius + 2 * 2.0 ** -24 * scale, gap / norm


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
TAU = 0.03
DEFAULTS = {"min_inliers": 4, "shared": 3, "max_survivors": 65536, "n_poses": 8}


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def planted(M, k, seed, groups=None, n_trip=None, subset=None, nan_rows=True, duplicate=False, kind="planted"):
    """M model points in the unit box and k candidates each.  `groups`: how many of the points follow each planted motion (default: all follow one);
    the rest are outlier keypoints whose candidates are all decoys.  A planted keypoint has its exact image (rounded to float32) at a random digit
    and decoys at the others; with nan_rows some trailing candidates are NaN padding; with `duplicate` digit 1 of every point repeats digit 0.
    kind 'collinear': the model points lie on a line; 'all_nan': every candidate is NaN.  n_trip: only the first n_trip of all triplets;
    subset: a sorted random subset of that many.
    -> dict(p, c, trip, tau, side_tol, min_side, min_sin, motions [(R, t, member indices)], digit)"""
    rng = np.random.default_rng(1000 * M + 10 * k + seed)
    p = rng.uniform(-0.5, 0.5, (M, 3))
    if kind == "collinear":
        p = np.array([0.1, -0.2, 0.05]) + np.linspace(-0.6, 0.6, M)[:, None] * np.array([0.6, 0.64, 0.48])
    p = p.astype(F)
    groups = (M,) if groups is None else groups
    members = np.split(rng.permutation(M), np.cumsum(groups))[:len(groups)]
    c = rng.uniform(-1.0, 1.0, (M, k, 3))
    digit = np.full(M, -1)
    motions = []
    for g, idx in enumerate(members):
        R = rotation(rng.standard_normal(3), np.deg2rad(40.0 + 70.0 * g))
        t = rng.uniform(-0.3, 0.3, 3)
        digit[idx] = rng.integers(0, k, len(idx))
        c[idx, digit[idx]] = p[idx].astype(np.float64) @ R.T + t
        motions.append((R, t, np.sort(idx)))
    if duplicate and k >= 2:                                   # digit 1 repeats digit 0 everywhere; an image that was at 1 is then found at 0
        moved = digit == 1
        c[moved, 0] = c[moved, 1]
        digit[moved] = 0
        c[:, 1] = c[:, 0]
    c = c.astype(F)
    if nan_rows and k >= 2:
        for q in range(0, M, 3):                               # every third point has fewer candidates than k: a NaN row at the end, as locate pads
            if digit[q] != k - 1 and not (duplicate and k == 2):
                c[q, k - 1] = np.nan
    if kind == "all_nan":
        c[:] = np.nan
    trip = all_triplets(M)
    if n_trip is not None:
        trip = trip[:n_trip]
    if subset is not None:
        trip = trip[np.sort(rng.choice(len(trip), subset, replace=False))]
    return {"p": p, "c": c, "trip": np.ascontiguousarray(trip), "tau": TAU, "side_tol": 2 * TAU, "min_side": 4 * TAU, "min_sin": 0.2, "motions": motions, "digit": digit}


def exact_refit_case(axis):
    """Eight corners of a box with dyadic coordinates about a dyadic centre, their exact images under a quarter turn about `axis` (0, 1, 2) and an
    integer translation, k = 1: every sum of Horn's form is exact, the 4 x 4 matrix couples only the two quaternion entries of the turn with
    equal diagonal entries, so the Jacobi angle is exactly 45 degrees and the pose comes out to the last bit.  -> (p, c [8, 1, 3], R, t)"""
    half = np.array([0.5, 1.25, 0.75])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * half + np.array([0.25, -0.5, 1.0])
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.zeros((3, 3))
    R[axis, axis] = 1.0
    R[b, a], R[a, b] = 1.0, -1.0                               # a quarter turn: e_a -> e_b, e_b -> -e_a
    t = np.array([3.0, -2.0, 5.0])
    c = corners @ R.T + t
    assert np.array_equal(corners.astype(F), corners) and np.array_equal(c.astype(F), c)
    return corners.astype(F), c.astype(F)[:, None, :], R.astype(F), t.astype(F)


# name -> (arguments of planted(), parameters that differ from DEFAULTS).  The shapes are the smallest at which a lane mapping, a queue or a cut
# can go wrong: M = 3, 4, 5, 17, 33, 64; k = 1, 2, 3, 8; n_trip = 1, 63, 64, 65 (T = 63, 64, 65 at k = 1: a wave; 504, 512, 520 at k = 2: the 256
# hypotheses of a flag workgroup); T above the 2048 hypotheses of one score workgroup; n_poses = 1, 2, 64; max_survivors = 1, 7 and the default.
CASES = {
    "m3k1": (dict(M=3, k=1, seed=0, nan_rows=False), dict(min_inliers=3, n_poses=1)),
    "m4k2": (dict(M=4, k=2, seed=0, nan_rows=False), dict(n_poses=2)),
    "m5k3": (dict(M=5, k=3, seed=0), dict()),
    "m17k1_t63": (dict(M=17, k=1, seed=1, n_trip=63), dict(n_poses=2)),
    "m17k1_t64": (dict(M=17, k=1, seed=1, n_trip=64), dict(n_poses=2)),
    "m17k1_t65": (dict(M=17, k=1, seed=1, n_trip=65), dict(n_poses=2)),
    "m17k2_t63": (dict(M=17, k=2, seed=2, n_trip=63), dict()),
    "m17k2_t64": (dict(M=17, k=2, seed=2, n_trip=64), dict()),
    "m17k2_t65": (dict(M=17, k=2, seed=2, n_trip=65), dict()),
    "m17k3": (dict(M=17, k=3, seed=3, groups=(12,)), dict(n_poses=64, min_inliers=3)),                         # 18360 hypotheses: nine score workgroups
    "m17k3_cut7": (dict(M=17, k=3, seed=3, groups=(12,)), dict(max_survivors=7)),               # the cut falls inside the run of count 12
    "m17k3_cut1": (dict(M=17, k=3, seed=3, groups=(12,)), dict(max_survivors=1, n_poses=2)),
    "m33k1": (dict(M=33, k=1, seed=4), dict(n_poses=2)),                                        # every hypothesis is live: the queue drains in full
    "two_objects": (dict(M=33, k=2, seed=5, groups=(14, 9)), dict()),
    "duplicates": (dict(M=17, k=3, seed=6, duplicate=True), dict()),
    "collinear": (dict(M=17, k=2, seed=7, kind="collinear"), dict()),
    "all_nan": (dict(M=5, k=2, seed=8, kind="all_nan"), dict()),
    "m64k2": (dict(M=64, k=2, seed=9, groups=(32,), subset=3000), dict(n_poses=64, min_inliers=3)),
    "m64k8": (dict(M=64, k=8, seed=10, groups=(32,), subset=200), dict()),                       # 102400 hypotheses
}


REFIT_CASES = ("m3k1", "m5k3", "m17k3", "two_objects", "m64k2", "m64k8")      # every selected pose of these is refit; their gaps are asserted on the host
MIN_GAP = 0.05                                                                 # (gap of the two largest eigenvalues) / |N|: comfortably away from zero


def case(name):
    args, params = CASES[name]
    return planted(**args), {**DEFAULTS, **params}


@functools.lru_cache(maxsize=None)
def scored(name):
    """the part of the reference that does not depend on the selection: live, pose [T, 12], count uint8 [T], assign int8 [T, M] (-1 where rejected)"""
    cs, _ = case(name)
    live, pose = gate_pose(cs["p"], cs["c"], cs["trip"], cs["side_tol"], cs["min_side"], cs["min_sin"])
    T, M = len(live), len(cs["p"])
    count = np.zeros(T, np.uint8)
    assign = np.full((T, M), -1, np.int8)
    tau2 = F(cs["tau"]) * F(cs["tau"])
    n, a = score(pose[live], cs["p"], cs["c"], tau2)
    count[live], assign[live] = n, a
    return {"live": live, "pose": pose, "count": count, "assign": assign, "tau2": tau2}


def survivors(count, min_inliers, max_survivors):
    """the h of the kept survivors, ascending"""
    h = np.flatnonzero(count >= min_inliers)
    keep = h[order(count[h], h)][:max_survivors]
    return np.sort(keep)


def reference(name, **override):
    """-> dict(count, pose, assign, live, n_gated, n_survivors, cut (the count at which max_survivors was reached, else min_inliers), hyp int32 [n_poses], inliers int32 [n_poses], sel_assign int8 [n_poses, 64], sel_pose
    float32 [n_poses, 12]), the ranks that do not exist padded with -1 and NaN"""
    cs, params = case(name)
    params = {**params, **override}
    sc = scored(name)
    M = len(cs["p"])
    h = survivors(sc["count"], params["min_inliers"], params["max_survivors"])
    picks = greedy(h, sc["count"][h], sc["assign"][h], params["n_poses"], params["shared"])
    H = params["n_poses"]
    hyp, inl = np.full(H, -1, np.int32), np.full(H, -1, np.int32)
    sel_assign, sel_pose = np.full((H, MAX_M), -1, np.int8), np.full((H, 12), np.nan, F)
    for r, w in enumerate(picks):
        hyp[r], inl[r] = h[w], sc["count"][h[w]]
        sel_assign[r, :M] = sc["assign"][h[w]]
        sel_pose[r] = sc["pose"][h[w]]
    return {**sc, "n_gated": int(sc["live"].sum()), "n_survivors": len(h), "found": len(picks), "hyp": hyp, "inliers": inl, "sel_assign": sel_assign, "sel_pose": sel_pose,
            "cut": int(sc["count"][h].min()) if len(h) == params["max_survivors"] else params["min_inliers"],
            "params": params, "survivors": h}


def pairs_of(cs, assign_row):
    """the assigned pairs of one pose: (p [n, 3], c [n, 3])"""
    q = np.flatnonzero(assign_row[:len(cs["p"])] >= 0)
    return cs["p"][q], cs["c"][q, assign_row[q]]


# ---- the chain: locate -> consensus -> align on a small scene -----------------------------------------------------------------------------------
SCENE_M, SCENE_K, SCENE_RADIUS = 12, 4, 2
SCENE_ABSENT = (2, 6, 10)                  # keypoints whose bump is missing from the field (occluded): locate can only offer decoys for them
SCENE_SIGMA = 1.5                          # voxels
SCENE_DECOY = 0.6                          # the amplitude of a decoy bump; a true bump has 1
SCENE_CLEAR, SCENE_CLEAR_OWN = 5.0, 7.5    # voxels between a decoy and every keypoint's image; and the image of its own channel's keypoint


@functools.lru_cache(maxsize=None)
def scene():
    """align_cases.scene()'s volume (two spheres, 24 x 20 x 18, step 2^-5) with another descriptor set: one Gaussian-bump channel per keypoint,
    centred on the keypoint's true image, two weaker decoy bumps per channel elsewhere on the surfaces, and no true bump for SCENE_ABSENT.  The 12
    keypoints lie on the surfaces, spread out; the true pose turns the model by 60 degrees about its centroid and shifts it by 4 voxels.  The targets
    are the descriptors of the complete object: the field with every true bump, sampled at the true images.
    -> dict(vol, p, R, t (the kernels' convention), x, targets, present)"""
    import align_cases as AC
    import volume_cases as VC
    h = VC.STEP
    origin = np.asarray(VC.ORIGIN, np.float64)
    vol = dict(AC.scene()["vol"])
    shape = vol["shape"]
    rng = np.random.default_rng(2323)
    surf = []
    for (ctr, r), count in zip(AC.SPHERES, (400, 200)):
        d = rng.standard_normal((count, 3))
        surf.append(np.asarray(ctr) + r * d / np.linalg.norm(d, axis=1, keepdims=True))
    surf = np.concatenate(surf)                                       # voxel units
    inside = ((surf > 2.5) & (surf < np.asarray(shape) - 3.5)).all(axis=1)
    surf = surf[inside]
    keys = [0]                                                        # farthest-point selection: the keypoints are spread out
    for _ in range(SCENE_M - 1):
        dmin = np.linalg.norm(surf[:, None] - surf[keys][None], axis=2).min(axis=1)
        keys.append(int(np.argmax(dmin)))
    xk = surf[keys]
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    bump = lambda at: np.exp(-((idx - at) ** 2).sum(-1) / (2 * SCENE_SIGMA ** 2))
    full = np.stack([bump(xk[q]) for q in range(SCENE_M)], -1)
    field = np.zeros_like(full)
    # decoys: in the band of two voxels about the surfaces, at least SCENE_CLEAR voxels from EVERY keypoint's image, so that near the images the
    # field is the complete object's but for the absent bumps, and the true pose is the optimum of the alignment
    pool = rng.uniform(2.5, np.asarray(shape) - 3.5, (20000, 3))
    sd = np.min([np.linalg.norm(pool - np.asarray(ctr), axis=1) - r for ctr, r in AC.SPHERES], axis=0)
    pool = pool[(np.abs(sd) < 1.5) & (np.linalg.norm(pool[:, None] - xk[None], axis=2).min(axis=1) >= SCENE_CLEAR)]
    assert len(pool) >= 2 * SCENE_M
    for q in range(SCENE_M):
        if q not in SCENE_ABSENT:
            field[..., q] = full[..., q]
        own = pool[np.linalg.norm(pool - xk[q], axis=1) >= SCENE_CLEAR_OWN]      # (an absent keypoint's residual is large: a decoy of its own channel nearby would pull the pose)
        for at in own[rng.choice(len(own), 2, replace=False)]:
            field[..., q] += SCENE_DECOY * bump(at)
    vol["sets"] = {"feat": field.astype(F)}
    vol["fills"] = {"feat": None}
    x = origin + xk * h
    c = x.mean(axis=0)
    R = rotation((0.4, 0.7, -0.5), np.deg2rad(60.0))
    shift = 4.0 * h * np.array([0.6, -0.64, 0.48])
    t = c - R @ c + shift
    R32, t32 = R.astype(F), t.astype(F)
    p = ((x - t32.astype(np.float64)) @ R32.astype(np.float64)).astype(F)
    x_true = AC.transform32(R32, t32, p)
    complete = dict(vol, sets={"feat": full.astype(F)})
    targets = VC.trilinear64(complete, x_true, ["feat"])["feat"][0].astype(F)
    present = np.array([q not in SCENE_ABSENT for q in range(SCENE_M)])
    return {"vol": vol, "p": p, "R": R32, "t": t32, "x": x_true, "targets": targets, "present": present}


def locate_ref(vol, name, targets, k, r):
    """BakedField.locate on a dense field, restated with tests/peaks_cases.py: l2 distances in float64 rounded to float32, the peaks, the k best, the
    refinement -> refined float64 [K, k, 3] (NaN rows: padding)"""
    import peaks_cases as PC
    shape = vol["shape"]
    rows = vol["sets"][name].reshape(-1, vol["sets"][name].shape[-1]).astype(np.float64)
    dist = np.sqrt(((rows[:, None, :] - np.asarray(targets, np.float64)[None]) ** 2).sum(-1)).astype(F)
    mask = vol["valid"].astype(np.uint8)
    out, _ = PC.peaks_keys_ref(shape, None, mask, dist, r)
    voxel, _ = PC.topk_ref(out, k)
    off = PC.refine_ref(shape, None, mask, dist, voxel)
    centre = np.stack(np.unravel_index(np.maximum(voxel, 0), shape), -1).astype(np.float64)
    pts = (np.asarray(vol["origin"], F)[None, None] + (centre.astype(F) * F(vol["step"]))).astype(np.float64)      # voxel centres in float32, as the field gives them
    return np.where((voxel >= 0)[..., None], pts + off * float(vol["step"]), np.nan)


def consensus_ref(p, c, tau, n_poses=8, min_inliers=4, shared=3, max_survivors=65536):
    """consensus_poses restated on all triplets -> (poses float32 [n, 12] refit by horn, inliers, assignments) of the ranks that exist"""
    trip = all_triplets(len(p))
    live, pose = gate_pose(p, c, trip, 2 * tau, 4 * tau, 0.2)
    count = np.zeros(len(live), np.int64)
    assign = np.full((len(live), len(p)), -1, np.int8)
    count[live], assign[live] = score(pose[live], p, c, F(tau) * F(tau))
    h = survivors(count, min_inliers, max_survivors)
    picks = greedy(h, count[h], assign[h], n_poses, shared)
    poses = []
    for w in picks:
        q = np.flatnonzero(assign[h[w]] >= 0)
        R, t, _, _ = horn(p[q], c[q, assign[h[w]][q]])
        poses.append(np.concatenate([R.reshape(9), t]).astype(F))
    return np.array(poses, F).reshape(-1, 12), [int(count[h[w]]) for w in picks], [assign[h[w]] for w in picks]
