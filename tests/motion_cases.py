"""NumPy restatement and case generators of the rigid motion per part (d3f_part_motion; include/d3fields_hip.h, the motion block; DESIGN.md
section 26), shared by tests/test_motion_host.py and tests/test_gpu_motion.py.

The contract, restated:
    volume      nx x ny x nz, z fastest, flat index v = (x*ny + y)*nz + z, n voxels
    pair        v is a pair of part k when label[v] == k with 1 <= k <= K, keep is None or keep[v] != 0, 0 <= target[v] < n and, with offset
                given, its three components at v are finite
    a, b        a = (x,y,z)(v) - ref_k (exact integers as float64); b = ((x,y,z)(target[v]) - ref_k) + offset[v]: the integer difference first,
                then one float64 add per axis (none with offset None); ref None: zeros
    row         {1, a0,a1,a2, b0,b1,b2, a_i*b_j (i major)}: 16 float64; +0.0 for a member that is no inlier of the current fit
    fold        the rows of a part in ascending flat index, chunks of 256 (a ragged last one), the next level folds the chunks' folds in order,
                256 at a time.  Inside a chunk: pad to 256 with +0.0; lane l of 64 holds (((0.0 + m_l) + m_{l+64}) + m_{l+128}) + m_{l+192};
                then for s = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l+s] for l < s.  No rows: +0.0
    fit         pm = A / n, cm = B / n, S_ij = M_ij - (A_i * B_j) / n; horn(S): the 4 x 4 matrix of S, 12 cyclic Jacobi sweeps that skip zero
                entries, the first largest diagonal entry, R = quaternion matrix / |q|^2.  Pose row: R row-major, ref + pm, ref + cm
    residual    u = a - pm, w = b - cm, e_i = ((R_i0 u0 + R_i1 u1) + R_i2 u2) - w_i, r2 = (e0 e0 + e1 e1) + e2 e2; inlier iff r2 <= tau2
    loop        fit 0 on every pair, fit f on the inliers under fit f-1; fewer than min_pairs at fit 0: TOO_FEW, NaN pose, fits 0; fewer at a
                later fit: THINNED, the pose of the last fit stays, fits = the fits done; else OK, fits = fits
    outputs     under the final pose: residual2 [n] (NaN where no pair or no pose), inlier [n], inliers [K], rmse = sqrt(fold(r2 of the inliers)
                / inliers) (NaN without inliers); sums [K,16]: the last fold a part took part in

motion_ref is that, one NumPy ufunc call per rounded operation.  motion_loop is a second formulation that shares nothing with it: plain sums,
np.linalg.svd Kabsch.  The case arrays are read-only."""
import functools
import math

import numpy as np

OK, THINNED, TOO_FEW = 0, 1, 2          # D3F_MOTION_OK / _THINNED / _TOO_FEW
MAX_FITS = 8                            # D3F_MOTION_MAX_FITS
CHUNK = 256                             # D3F_POOL_CHUNK
SUMS, POSE = 16, 15                     # D3F_MOTION_SUM_DOUBLES / _POSE_DOUBLES
SWEEPS = 12
POISON = 0xA5
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def coords(flat, shape):
    """int64 [m, 3]: (x, y, z) of flat indices"""
    flat = np.asarray(flat, np.int64)
    ny, nz = shape[1], shape[2]
    return np.stack((flat // (ny * nz), (flat // nz) % ny, flat % nz), axis=-1)


def pair_mask(label, K, target, keep=None, offset=None):
    """bool [n]: the pairs; a label outside 1..K or a target outside 0..n-1 indexes nothing"""
    lab, tgt = np.asarray(label).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    n = lab.size
    pair = (lab >= 1) & (lab <= K) & (tgt >= 0) & (tgt < n)
    if keep is not None:
        pair &= np.asarray(keep).reshape(-1) != 0
    if offset is not None:
        pair &= np.isfinite(np.asarray(offset, np.float64).reshape(n, 3)).all(axis=1)
    return pair


def points(idx, shape, target, offset, ref_k):
    """(a, b) float64 [m, 3] of the pairs idx (flat indices) of one part"""
    r = np.zeros(3, np.int64) if ref_k is None else np.asarray(ref_k, np.int64)
    a = (coords(idx, shape) - r).astype(np.float64)
    b = (coords(np.asarray(target).reshape(-1)[idx], shape) - r).astype(np.float64)
    if offset is not None:
        b = b + np.asarray(offset, np.float64).reshape(-1, 3)[idx]
    return a, b


def moment_rows(a, b, inlier=None):
    """float64 [m, 16]: {1, a, b, a_i*b_j (i major)}; +0.0 rows where inlier is False"""
    m = len(a)
    rows = np.empty((m, SUMS), np.float64)
    rows[:, 0] = 1.0
    rows[:, 1:4], rows[:, 4:7] = a, b
    for i in range(3):
        for j in range(3):
            rows[:, 7 + 3 * i + j] = a[:, i] * b[:, j]
    if inlier is not None:
        rows[~np.asarray(inlier, bool)] = 0.0
    return rows


def fold(rows):
    """float64 [NC]: the tree of the contract over rows [m, NC]"""
    rows = np.asarray(rows, np.float64)
    m, nc = rows.shape
    if m == 0:
        return np.zeros(nc, np.float64)
    while True:
        c = -(-m // CHUNK)
        pad = np.zeros((c * CHUNK, nc), np.float64)
        pad[:m] = rows
        r = pad.reshape(c, 4, 64, nc)
        v = 0.0 + r[:, 0]
        for j in (1, 2, 3):
            v = v + r[:, j]
        for s in (32, 16, 8, 4, 2, 1):
            v = v[:, :s] + v[:, s:2 * s]
        rows, m = v[:, 0], c
        if m == 1:
            return rows[0].copy()


def fold_recursive(rows):
    """the same tree written as a plain recursion over Python lists: one column at a time"""
    rows = [[float(x) for x in r] for r in rows]
    nc = len(rows[0]) if rows else 0

    def chunk(col):                                                  # col: up to 256 floats
        col = col + [0.0] * (CHUNK - len(col))
        v = [((0.0 + col[l]) + col[l + 64] + col[l + 128]) + col[l + 192] for l in range(64)]
        s = 32
        while s:
            v = [v[l] + v[l + s] for l in range(s)]
            s //= 2
        return v[0]

    def level(col):
        if len(col) <= CHUNK:
            return chunk(col)
        return level([chunk(col[i:i + CHUNK]) for i in range(0, len(col), CHUNK)])
    return np.array([level([r[e] for r in rows]) for e in range(nc)], np.float64)


def horn(S):
    """float64 [3, 3]: a line-for-line port of horn_rotation (csrc/d3f_horn.h) on NumPy float64 scalars"""
    f = np.float64
    S = np.asarray(S, np.float64)
    A = [[f(0.0)] * 4 for _ in range(4)]
    V = [[f(1.0) if i == j else f(0.0) for j in range(4)] for i in range(4)]
    with np.errstate(all="ignore"):
        A[0][0] = (S[0, 0] + S[1, 1]) + S[2, 2]
        A[1][1] = (S[0, 0] - S[1, 1]) - S[2, 2]
        A[2][2] = (S[1, 1] - S[0, 0]) - S[2, 2]
        A[3][3] = (S[2, 2] - S[0, 0]) - S[1, 1]
        A[0][1] = A[1][0] = S[1, 2] - S[2, 1]
        A[0][2] = A[2][0] = S[2, 0] - S[0, 2]
        A[0][3] = A[3][0] = S[0, 1] - S[1, 0]
        A[1][2] = A[2][1] = S[0, 1] + S[1, 0]
        A[1][3] = A[3][1] = S[2, 0] + S[0, 2]
        A[2][3] = A[3][2] = S[1, 2] + S[2, 1]
        for _ in range(SWEEPS):
            for i in range(3):
                for j in range(i + 1, 4):
                    apq = A[i][j]
                    if apq == 0.0:
                        continue
                    theta = (A[j][j] - A[i][i]) / (f(2.0) * apq)
                    t = (f(-1.0) if theta < 0.0 else f(1.0)) / (np.abs(theta) + np.sqrt(theta * theta + f(1.0)))
                    c = f(1.0) / np.sqrt(t * t + f(1.0))
                    s = t * c
                    A[i][i] = A[i][i] - t * apq
                    A[j][j] = A[j][j] + t * apq
                    A[i][j] = A[j][i] = f(0.0)
                    for m in range(4):
                        if m != i and m != j:
                            ami, amj = A[m][i], A[m][j]
                            A[m][i] = A[i][m] = c * ami - s * amj
                            A[m][j] = A[j][m] = s * ami + c * amj
                        vmi, vmj = V[m][i], V[m][j]
                        V[m][i] = c * vmi - s * vmj
                        V[m][j] = s * vmi + c * vmj
        top = 0
        for i in range(1, 4):
            if A[i][i] > A[top][top]:
                top = i
        q0, q1, q2, q3 = V[0][top], V[1][top], V[2][top], V[3][top]
        a0, a1, a2, a3 = q0 * q0, q1 * q1, q2 * q2, q3 * q3
        n2 = ((a0 + a1) + a2) + a3
        two = f(2.0)
        R = [[(((a0 + a1) - a2) - a3) / n2, (two * (q1 * q2 - q0 * q3)) / n2, (two * (q1 * q3 + q0 * q2)) / n2],
             [(two * (q1 * q2 + q0 * q3)) / n2, (((a0 - a1) + a2) - a3) / n2, (two * (q2 * q3 - q0 * q1)) / n2],
             [(two * (q1 * q3 - q0 * q2)) / n2, (two * (q2 * q3 + q0 * q1)) / n2, (((a0 - a1) - a2) + a3) / n2]]
    return np.array(R, np.float64)


def fit_sums(s):
    """(pm, cm, R) from a row of sums with s[0] > 0"""
    n, A, B, M = s[0], s[1:4], s[4:7], s[7:16].reshape(3, 3)
    with np.errstate(all="ignore"):
        pm, cm = A / n, B / n
        S = M - (A[:, None] * B[None, :]) / n
    return pm, cm, horn(S)


def residual2(a, b, pm, cm, R):
    with np.errstate(all="ignore"):
        u, w = a - pm, b - cm
        e = [((R[i, 0] * u[:, 0] + R[i, 1] * u[:, 1]) + R[i, 2] * u[:, 2]) - w[:, i] for i in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def members_by_part(label, K, pair):
    """per part the flat indices of its pairs, ascending"""
    lab = np.where(pair, np.asarray(label).reshape(-1).astype(np.int64), 0)
    order = np.argsort(lab, kind="stable")
    counts = np.bincount(lab[order], minlength=K + 1)[:K + 1]
    ends = np.cumsum(counts)
    return [order[ends[k - 1]:ends[k]] for k in range(1, K + 1)], counts[1:].astype(np.int32)


def empty_outputs(n, K):
    nan = np.nan
    return {"pose": np.full((K, POSE), nan), "inliers": np.zeros(K, np.int32), "rmse": np.full(K, nan), "status": np.full(K, TOO_FEW, np.int32),
            "fits": np.zeros(K, np.int32), "residual2": np.full(n, nan), "inlier": np.zeros(n, np.uint8), "sums": np.zeros((K, SUMS))}


def motion_ref(label, K, target, keep=None, offset=None, ref=None, fits=3, tau2=1.0, min_pairs=8, capacity=None):
    """every output of d3f_part_motion as a dict; over capacity only 'members' and 'pairs' (the others None)"""
    shape = np.asarray(label).shape
    n = int(np.prod(shape))
    pair = pair_mask(label, K, target, keep, offset)
    lists, pairs = members_by_part(label, K, pair)
    out = {"members": np.int64(pair.sum()), "pairs": pairs}
    if capacity is not None and out["members"] > capacity:
        out.update({k: None for k in empty_outputs(0, 0)})
        return out
    out.update(empty_outputs(n, K))
    for k in range(K):
        idx = lists[k]
        r = None if ref is None else np.asarray(ref, np.int64)[k]
        a, b = points(idx, shape, target, offset, r)
        inl = np.ones(len(idx), bool)
        cur, status, done = None, OK, 0
        for f in range(fits):
            s = fold(moment_rows(a, b, inl))
            out["sums"][k] = s
            if not s[0] >= min_pairs:
                status = TOO_FEW if f == 0 else THINNED
                break
            cur, done = fit_sums(s), f + 1
            inl = residual2(a, b, *cur) <= tau2
        out["status"][k], out["fits"][k] = status, done
        if status == TOO_FEW:
            continue
        pm, cm, R = cur
        r0 = np.zeros(3) if r is None else r.astype(np.float64)
        out["pose"][k] = np.concatenate((R.reshape(-1), r0 + pm, r0 + cm))
        r2 = residual2(a, b, pm, cm, R)
        inl = r2 <= tau2
        out["residual2"][idx], out["inlier"][idx] = r2, inl
        fs = fold(np.stack((inl.astype(np.float64), np.where(inl, r2, 0.0)), axis=1))
        out["inliers"][k] = int(fs[0])
        with np.errstate(all="ignore"):
            out["rmse"][k] = np.sqrt(fs[1] / fs[0]) if fs[0] > 0 else np.nan
    return out


def kabsch(a, b):
    """(pm, cm, R) by np.linalg.svd: the rotation that best takes a - pm onto b - cm"""
    pm, cm = a.mean(axis=0), b.mean(axis=0)
    H = (a - pm).T @ (b - cm)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return pm, cm, Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def motion_loop(label, K, target, keep=None, offset=None, ref=None, fits=3, tau2=1.0, min_pairs=8):
    """the second formulation: a plain float64 loop over the parts with SVD-Kabsch; the same keys as motion_ref but 'sums'"""
    lab, tgt = np.asarray(label), np.asarray(target).reshape(-1)
    shape, n = lab.shape, lab.size
    out = empty_outputs(n, K)
    del out["sums"]
    out["pairs"] = np.zeros(K, np.int32)
    total = 0
    for k in range(1, K + 1):
        idx = [v for v in np.flatnonzero(lab.reshape(-1) == k)
               if (keep is None or np.asarray(keep).reshape(-1)[v]) and 0 <= tgt[v] < n and (offset is None or np.isfinite(np.asarray(offset).reshape(-1, 3)[v]).all())]
        idx = np.array(idx, np.int64)
        out["pairs"][k - 1] = len(idx)
        total += len(idx)
        r = np.zeros(3) if ref is None else np.asarray(ref, np.float64)[k - 1]
        a = np.array(np.unravel_index(idx, shape), np.float64).T.reshape(-1, 3) - r
        b = np.array(np.unravel_index(tgt[idx], shape), np.float64).T.reshape(-1, 3) - r
        if offset is not None:
            b = b + np.asarray(offset, np.float64).reshape(-1, 3)[idx]
        if len(idx) < min_pairs:
            continue
        use = np.ones(len(idx), bool)
        status, done = OK, 0
        for f in range(fits):
            if use.sum() < min_pairs:
                status = THINNED
                break
            pm, cm, R = kabsch(a[use], b[use])
            done = f + 1
            r2 = (((a - pm) @ R.T - (b - cm)) ** 2).sum(axis=1)
            use = r2 <= tau2
        out["status"][k - 1], out["fits"][k - 1] = status, done
        out["pose"][k - 1] = np.concatenate((R.reshape(-1), r + pm, r + cm))
        out["residual2"][idx], out["inlier"][idx] = r2, use
        out["inliers"][k - 1] = use.sum()
        out["rmse"][k - 1] = math.sqrt(r2[use].sum() / use.sum()) if use.any() else np.nan
    out["members"] = np.int64(total)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues"""
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


PLANTED_SHAPE, PLANTED_PARTS = (24, 24, 24), 6
PLANTED_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def planted(seed, shape=PLANTED_SHAPE, parts=PLANTED_PARTS):
    """-> dict: label int32, target int32, offset float64 [.., 3], ref int32 [K, 3] (the parts' box_lo), truth bool (the planted inliers),
    R [K, 3, 3], src [K, 3], dst [K, 3] (q = R (p - src) + dst in voxel units).  Per part 40..400 voxels drawn from a 10^3 box in its own octant, a
    rotation of up to 25 degrees about a random axis through the part's centroid plus a shift of up to 3 voxels applied to the integer voxel
    coordinates; target = the rounded image clipped to the grid, offset = the remainder; a quarter of the pairs are outliers: their image is
    moved by 3 or 4 voxels with a random sign on every axis."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    label = np.zeros(shape, np.int32)
    target = np.full(shape, -1, np.int32)
    offset = np.full(shape + (3,), np.nan)
    truth = np.zeros(shape, bool)
    octants = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    Rs, srcs, dsts, refs = [], [], [], []
    for k in range(parts):
        o = np.array(octants[k]) * (np.array(shape) // 2) + 1
        m = int(rng.integers(40, 401))
        pick = rng.choice(1000, size=m, replace=False)
        p = np.stack(np.unravel_index(pick, (10, 10, 10)), axis=1) + o              # int [m, 3]
        R = rotation(rng.normal(size=3), math.radians(rng.uniform(0, 25)))
        c = p.mean(axis=0)
        shift = rng.uniform(-3, 3, size=3)
        q = (p - c) @ R.T + c + shift
        out = rng.random(m) < 0.25
        q = q + out[:, None] * rng.integers(3, 5, size=(m, 3)) * rng.choice([-1, 1], size=(m, 3))
        t = np.clip(np.rint(q), 0, np.array(shape) - 1).astype(np.int64)
        idx = tuple(p.T)
        label[idx] = k + 1
        target[idx] = np.ravel_multi_index(tuple(t.T), shape)
        offset[idx] = q - t
        truth[idx] = ~out
        Rs.append(R), srcs.append(c), dsts.append(c + shift), refs.append(p.min(axis=0))
    frozen(label, target, offset, truth)
    return {"label": label, "target": target, "offset": offset, "truth": truth, "K": parts, "ref": np.array(refs, np.int32), "R": np.array(Rs),
            "src": np.array(srcs), "dst": np.array(dsts)}


TREE_SHAPE = (41, 40, 41)
TREE_SMALL = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513)
TREE_LARGE = (65537, 1, 257)            # 65 537 members need a third level; the volume holds it with two small parts, not with all eleven
TREE_TAU2 = 600.0                       # random targets: about half of a part's pairs stay inliers, so every fit folds a mixed chunk


@functools.lru_cache(maxsize=None)
def tree_case(counts, seed):
    """one part per member count, the parts interleaved at random through TREE_SHAPE; random integer targets, random offsets in (-0.5, 0.5)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(TREE_SHAPE))
    assert sum(counts) <= n
    lab = np.zeros(n, np.int32)
    lab[:sum(counts)] = np.repeat(np.arange(1, len(counts) + 1), counts)
    lab = rng.permutation(lab).reshape(TREE_SHAPE).astype(np.int32)
    target = rng.integers(0, n, size=TREE_SHAPE).astype(np.int32)
    offset = rng.uniform(-0.5, 0.5, size=TREE_SHAPE + (3,))
    frozen(lab, target, offset)
    return {"label": lab, "target": target, "offset": offset, "K": len(counts)}


INTERLEAVED_SHAPE, INTERLEAVED_PARTS = (9, 10, 33), 300


@functools.lru_cache(maxsize=None)
def interleaved_case(seed=7):
    """300 parts of 1..40 voxels (most of them small: the volume has 2970 voxels) scattered so that no part is contiguous in flat order; the
    voxels left over carry the labels 0, -1, K+1 and INT32_MIN; some targets are -1, n and INT32_MAX; the others follow a shift per part, with noise"""
    rng = np.random.default_rng(seed)
    shape, K = INTERLEAVED_SHAPE, INTERLEAVED_PARTS
    n = int(np.prod(shape))
    sizes = 1 + np.floor(39 * rng.random(K) ** 4).astype(int)
    sizes[:4] = (1, 2, 40, 40)
    assert sizes.min() == 1 and sizes.max() == 40 and sizes.sum() < n - 100
    lab = np.concatenate((np.repeat(np.arange(1, K + 1), sizes), rng.choice([0, -1, K + 1, INT32_MIN], size=n - sizes.sum()))).astype(np.int64)
    lab = rng.permutation(lab)
    own = coords(np.arange(n), shape)
    shift = rng.integers(-1, 2, size=(K + 2, 3))                     # a shift per part, and noise of up to 2 voxels per axis on three pairs in ten
    noise = rng.integers(-2, 3, size=(n, 3)) * (rng.random(n) < 0.3)[:, None]
    t = np.clip(own + shift[np.clip(lab, 0, K + 1)] + noise, 0, np.array(shape) - 1)
    target = np.ravel_multi_index(tuple(t.T), shape).astype(np.int64)
    bad = rng.random(n) < 0.05
    target[bad] = rng.choice([-1, n, INT32_MAX], size=bad.sum())
    offset = rng.uniform(-0.5, 0.5, size=(n, 3))
    lab, target, offset = lab.astype(np.int32).reshape(shape), target.astype(np.int32).reshape(shape), offset.reshape(shape + (3,))
    keep = (rng.random(shape) < 0.9).astype(np.uint8) * 7
    frozen(lab, target, offset, keep)
    return {"label": lab, "target": target, "offset": offset, "keep": keep, "K": K}


@functools.lru_cache(maxsize=None)
def status_case():
    """12 x 12 x 12, min_pairs 8.  Part 1: 2 pairs (TOO_FEW).  Part 2: 12 pairs of which 6 follow one shift and 6 another, far apart: fit 0 lies
    between, no pair is within tau of it, so it thins at fit 1 with the pose of fit 0.  Part 3: no pair (its voxels have target -1).  Part 4: 30
    pairs, a clean shift: OK.  Part 5: no voxel at all."""
    shape = (12, 12, 12)
    label = np.zeros(shape, np.int32)
    target = np.full(shape, -1, np.int32)
    flat = lambda x, y, z: int(np.ravel_multi_index((x, y, z), shape))
    for z in (1, 2):
        label[0, 0, z], target[0, 0, z] = 1, flat(0, 1, z)
    for i in range(12):
        x, y, z = 2 + i % 3, 2 + (i // 3) % 2, 2 + i // 6
        label[x, y, z] = 2
        target[x, y, z] = flat(x, y, z + (0 if i % 2 else 6))
    label[6, 6, 0:5] = 3
    for i in range(30):
        x, y, z = 7 + i % 3, 7 + (i // 3) % 2, 1 + i // 6
        label[x, y, z] = 4
        target[x, y, z] = flat(x + 1, y - 1, z + 2)
    frozen(label, target)
    return {"label": label, "target": target, "K": 5}


def load_world(pose, origin, step):
    """(rot [K,3,3], trans [K,3], angle [K], shift [K,3]) in float64 NumPy: the formulas of PartMotions"""
    pose = np.asarray(pose, np.float64)
    o = np.asarray(origin, np.float64)
    rot = pose[:, :9].reshape(-1, 3, 3)
    src, dst = o + step * pose[:, 9:12], o + step * pose[:, 12:15]
    trans = dst - np.einsum("kij,kj->ki", rot, src)
    skew = np.stack((rot[:, 2, 1] - rot[:, 1, 2], rot[:, 0, 2] - rot[:, 2, 0], rot[:, 1, 0] - rot[:, 0, 1]), axis=-1)
    angle = np.arctan2(np.sqrt((skew * skew).sum(axis=-1)), np.trace(rot, axis1=1, axis2=2) - 1.0)
    return rot, trans, angle, dst - src
