"""NumPy restatement, float32 port, bounds and cases of the rigid alignment to a baked field (d3f_volume_align_*, include/d3fields_hip.h;
DESIGN.md section 22), shared by tests/test_align_host.py and tests/test_gpu_align.py.

A volume is the dict of tests/volume_cases.py; `mark` is band_cases.mark(vol, band) or None (a dense field).  A pose is (R [3,3], t [3])
float32 in the KERNELS' convention, x = R p + t -- the transpose of rigid.rigid_transform's `rot`.

accumulate64 restates the contract: the transformed points by the float32 fma chain (so they are the kernel's bit for bit), everything after
that in float64 on volume_cases.locate64 / _weights / _dweights.  Next to H, b and the cost it returns, per entry,
    A      the same sum with absolute values taken at every product (the scale of the fp32 rounding of the per-point arithmetic) and
    slack  what the rounding of g = (x - origin) / h (2^-24 G per axis: volume_cases.coord_term / grad_coord_term) can move the entry by.
accumulate32 is the float32 port of the per-point arithmetic, operation by operation and in the sixteen-lane order of the kernel.
step_ref / align_ref restate the Levenberg-Marquardt loop; they are the contract of d3f_volume_align_step.
"""
import functools
import math

import numpy as np

import volume_cases as VC

U = VC.U
F = np.float32
ROW, STATE, CHUNK = 32, 96, 256
RUNNING, CONVERGED, STALLED, NO_GRADIENT, FAILED = 0, 1, 2, 3, 4
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, DIAG_FLOOR = 1e-3, 1e-9, 1e6, 1e-9
S_MODEL, S_LAMBDA, S_COST, S_STATUS, S_STEPS, S_VALID, S_INBAND, S_DELTA, S_H, S_B = 24, 27, 28, 29, 30, 31, 32, 33, 39, 60      # the state block; [0, 12) the accepted pose, [12, 24) the candidate
TRIU = np.triu_indices(6)


# ---- the pose chain -------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    return VC._fma32(a, b, c)


def transform32(R, t, p):
    """x_a = fma(R_a2, p_z, fma(R_a1, p_y, R_a0 * p_x)) + t_a in float32; p [n,3]"""
    R, t, p = np.asarray(R, F), np.asarray(t, F), np.asarray(p, F)
    x = np.empty_like(p)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            acc = (R[a, 0] * p[:, 0]).astype(F)
            acc = _fma32(R[a, 1], p[:, 1], acc)
            acc = _fma32(R[a, 2], p[:, 2], acc)
            x[:, a] = (acc + t[a]).astype(F)
    return x


def centroid(p, w=None):
    """the model's weighted centroid over the weighted points with finite coordinates: float64 sums, rounded to float32; zeros when there is none"""
    with np.errstate(invalid="ignore"):
        w = np.ones(len(p)) if w is None else np.where(np.asarray(w) > 0, np.asarray(w, np.float64), 0.0)
    use = (w > 0) & np.isfinite(p).all(axis=1)
    s = w[use].sum()
    return ((w[use, None] * p[use].astype(np.float64)).sum(axis=0) / s).astype(F) if s > 0 else np.zeros(3, F)


def rodrigues(w):
    """Exp(w) in float64, as the step kernel forms it"""
    wx, wy, wz = (float(v) for v in w)
    th2 = wx * wx + wy * wy + wz * wz
    th = math.sqrt(th2)
    if th < 1e-4:
        ca, cb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        sh = math.sin(0.5 * th)
        ca, cb = math.sin(th) / th, 2.0 * sh * sh / th2
    return np.array([[1.0 + cb * (wx * wx - th2), -ca * wz + cb * wx * wy, ca * wy + cb * wx * wz],
                     [ca * wz + cb * wx * wy, 1.0 + cb * (wy * wy - th2), -ca * wx + cb * wy * wz],
                     [-ca * wy + cb * wx * wz, ca * wx + cb * wy * wz, 1.0 + cb * (wz * wz - th2)]])


def compose(R, t, model, delta):
    """the candidate pose: R <- Exp(w) R, t <- c + Exp(w)(t - c) + v about the pivot c = the float32 chain on the model centroid; float64,
    rounded to float32"""
    R, t = np.asarray(R, F), np.asarray(t, F)
    c = transform32(R, t, np.asarray(model, F)[None])[0].astype(np.float64)
    E = rodrigues(delta[:3])
    return (E @ R.astype(np.float64)).astype(F), (c + E @ (t.astype(np.float64) - c) + np.asarray(delta[3:], np.float64)).astype(F)


# ---- the normal equations in float64 ----------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _abs_cross(a, b):
    """the cross product with absolute values taken at every product (a, b >= 0)"""
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _mirror(H):
    """the upper triangle, mirrored: symmetric by construction, as a row of 21 entries is"""
    return np.triu(H) + np.triu(H, 1).T


def residuals64(vol, mark, name, x, w, targets, dist_targets, wd, wf):
    """Per point and residual k (0: the distance, 1..C: the channels of `name`): r, g [.., 3] and their absolute-value versions and coordinate
    slacks, zero where the residual does not apply.  -> dict; valid / in_band count weighted points only."""
    N = len(x)
    h = float(vol["step"])
    ok, i, tt = VC.locate64(vol, x)
    with np.errstate(invalid="ignore"):
        weighted = np.asarray(w) > 0
    ok_w = ok & weighted
    inb = ok_w if mark is None else ok_w & mark["cell_band"][i[:, 0], i[:, 1], i[:, 2]]
    wts, dw = VC._weights(tt), VC._dweights(tt)
    parts = [(vol["dist"][..., None], np.zeros((N, 1)) if dist_targets is None else np.asarray(dist_targets, np.float64)[:, None], float(F(wd)), ok_w)]
    if name is not None:
        parts.append((vol["sets"][name], np.asarray(targets, np.float64), float(F(wf)), inb))
    out = {k: [] for k in ("r", "g", "rabs", "gabs", "er", "eg", "spread")}
    for arr, tgt, wgt, use in parts:
        v = np.where(use[None, :, None], VC._corners(arr, i).astype(np.float64), 0.0)                 # [8, N, K]; never an invalid voxel's value
        val = np.einsum("cn,cnk->nk", wts, v)
        grad = np.einsum("acn,cnk->nka", dw, v) / h
        spread = v.max(axis=0) - v.min(axis=0)
        m = use[:, None]
        out["r"].append(np.where(m, wgt * (val - tgt), 0.0))
        out["g"].append(np.where(m[..., None], wgt * grad, 0.0))
        out["rabs"].append(np.where(m, wgt * (np.einsum("cn,cnk->nk", wts, np.abs(v)) + np.abs(tgt)), 0.0))
        # the derivative as the kernel forms it: face weights times corner DIFFERENCES (which round relative to themselves, not to the corners)
        gabs = np.stack([sum(np.abs(dw[a, c])[:, None] * np.abs(v[c] - v[c - (4 >> a)]) for c in range(8) if c & (4 >> a)) for a in range(3)], -1) / h
        out["gabs"].append(np.where(m[..., None], wgt * gabs, 0.0))
        out["spread"].append(np.where(m, wgt * spread, 0.0))                     # weight times the corner spread: |g_a| <= spread / h
        out["er"].append(np.where(m, wgt * VC.coord_term(vol, spread), 0.0))
        out["eg"].append(np.where(m, wgt * VC.grad_coord_term(vol, spread / h), 0.0))
    res = {k: np.concatenate(v, axis=1) for k, v in out.items()}
    res.update(valid=ok_w, in_band=inb, weighted=weighted)
    return res


def accumulate64(vol, mark, name, p, R, t, model, w=None, targets=None, dist_targets=None, wd=1.0, wf=1.0, outside=None):
    """ONE instance.  -> dict(H [6,6], b [6], cost, valid, in_band, A_H, A_b, A_cost, slack_H, slack_b, slack_cost, x [n,3] float32, pivot)"""
    p = np.asarray(p, F)
    w = np.ones(len(p), F) if w is None else np.asarray(w, F)
    outside = float(F(4.0 * float(vol["step"]) * wd)) if outside is None else float(F(outside))
    x = transform32(R, t, p)
    c = transform32(R, t, np.asarray(model, F)[None])[0].astype(np.float64)
    res = residuals64(vol, mark, name, x, w, targets, dist_targets, wd, wf)
    w64 = np.where(res["weighted"], w.astype(np.float64), 0.0)
    xs = np.where(res["valid"][:, None], x.astype(np.float64) - c, 0.0)
    ax = np.abs(xs)
    J = np.concatenate([_cross(xs[:, None, :], res["g"]), res["g"]], axis=-1)                      # [N, K, 6]
    Jabs = np.concatenate([_abs_cross(ax[:, None, :], res["gabs"]), res["gabs"]], axis=-1)
    arm = np.stack([ax[:, 1] + ax[:, 2], ax[:, 0] + ax[:, 2], ax[:, 0] + ax[:, 1], np.ones(len(p)), np.ones(len(p)), np.ones(len(p))], axis=-1)
    dJ = res["eg"][..., None] * arm[:, None, :]
    miss = w64 * (res["weighted"] & ~res["valid"]) * outside * outside
    r, rabs, er = res["r"], res["rabs"], res["er"]
    return {
        "H": _mirror(np.einsum("n,nki,nkj->ij", w64, J, J)), "b": np.einsum("n,nki,nk->i", w64, J, r), "cost": float(np.einsum("n,nk,nk->", w64, r, r) + miss.sum()),
        "valid": int(res["valid"].sum()), "in_band": int(res["in_band"].sum()),
        "A_H": np.einsum("n,nki,nkj->ij", w64, Jabs, Jabs), "A_b": np.einsum("n,nki,nk->i", w64, Jabs, rabs),
        "A_cost": float(np.einsum("n,nk,nk->", w64, rabs, rabs) + miss.sum()),
        "slack_H": np.einsum("n,nki,nkj->ij", w64, dJ, Jabs) + np.einsum("n,nki,nkj->ij", w64, Jabs, dJ) + np.einsum("n,nki,nkj->ij", w64, dJ, dJ),
        "slack_b": np.einsum("n,nki,nk->i", w64, dJ, rabs) + np.einsum("n,nki,nk->i", w64, Jabs, er) + np.einsum("n,nki,nk->i", w64, dJ, er),
        "slack_cost": float(np.einsum("n,nk,nk->", w64, 2.0 * np.abs(r) + er, er)),
        "x": x, "pivot": c, "J": J, "r": r,
    }


def row_of(acc):
    """the D3F_ALIGN_ROW_DOUBLES row of an accumulate64 / accumulate32 result"""
    row = np.zeros(ROW)
    row[:21], row[21:27], row[27], row[28], row[29] = acc["H"][TRIU], acc["b"], acc["cost"], acc["valid"], acc["in_band"]
    return row


def unpack_row(row):
    """(H [6,6] symmetric, b, cost, valid, in_band) of a row"""
    H = np.zeros((6, 6))
    H[TRIU] = row[:21]
    H = H + np.triu(H, 1).T
    return H, row[21:27].copy(), float(row[27]), int(row[28]), int(row[29])


# ---- the float32 port of the per-point arithmetic ---------------------------------------------------------------------------------------
def _residual32(w8, faces, v, tgt, wt, wth, acc):
    """kernel add_residual: v [8, N] float32 corner values, acc [10, N] float32 (G xx xy xz yy yz zz, q, e), updated in place"""
    val = (w8[0] * v[0]).astype(F)
    for c in range(1, 8):
        val = _fma32(w8[c], v[c], val)
    d = []
    for wts, pr in faces:
        a = (wts[0] * (v[pr[0][0]] - v[pr[0][1]])).astype(F)
        for j in range(1, 4):
            a = _fma32(wts[j], (v[pr[j][0]] - v[pr[j][1]]).astype(F), a)
        d.append(a)
    r = (wt * (val - tgt).astype(F)).astype(F)
    g = [(wth * a).astype(F) for a in d]
    for slot, (a, b) in enumerate([(g[0], g[0]), (g[0], g[1]), (g[0], g[2]), (g[1], g[1]), (g[1], g[2]), (g[2], g[2]), (g[0], r), (g[1], r), (g[2], r), (r, r)]):
        acc[slot] = _fma32(a, b, acc[slot])


def accumulate32(vol, mark, name, p, R, t, model, w=None, targets=None, dist_targets=None, wd=1.0, wf=1.0, outside=None, vec=False):
    """ONE instance: the kernel's fp32 per-point arithmetic (locate32, the eight-corner chain, the face-weight chain, one fma per term, the
    channels in the sixteen-lane order -- channel k in lane (k // 4) % 16 with 16-byte vectors (`vec`), k % 16 without --, the group folded
    8, 4, 2, 1, the distance term last), the expansion in float64, the sum across points by NumPy in float64.  -> dict(H, b, cost, valid, in_band)"""
    p = np.asarray(p, F)
    N = len(p)
    w = np.ones(N, F) if w is None else np.asarray(w, F)
    outside = F(4.0 * float(vol["step"]) * wd) if outside is None else F(outside)
    x = transform32(R, t, p)
    c = transform32(R, t, np.asarray(model, F)[None])[0].astype(np.float64)
    ok, i, tt = VC.locate32(vol, x)
    with np.errstate(invalid="ignore"):
        weighted = w > 0
    ok_w = ok & weighted
    inb = ok_w if mark is None else ok_w & mark["cell_band"][i[:, 0], i[:, 1], i[:, 2]]
    w8 = VC._weights(tt, F).astype(F)
    a = [np.stack([F(1) - tt[:, k], tt[:, k]]).astype(F) for k in range(3)]
    yz = [a[1][j >> 1] * a[2][j & 1] for j in range(4)]
    xz = [a[0][j >> 1] * a[2][j & 1] for j in range(4)]
    xy = [a[0][j >> 1] * a[1][j & 1] for j in range(4)]
    faces = [(yz, [(4, 0), (5, 1), (6, 2), (7, 3)]), (xz, [(2, 0), (3, 1), (6, 4), (7, 5)]), (xy, [(1, 0), (3, 2), (5, 4), (7, 6)])]
    rh = F(1) / F(vol["step"])
    wdh, wfh = F(wd) * rh, F(wf) * rh
    acc = np.zeros((10, N), F)
    with np.errstate(invalid="ignore", over="ignore"):
        if name is not None:
            arr = vol["sets"][name]
            C = arr.shape[3]
            v = np.where(inb[None, :, None], VC._corners(arr, i), F(0))                              # [8, N, C]
            lanes = np.zeros((16, 10, N), F)
            for k in range(C):
                lane = (k // 4) % 16 if vec else k % 16
                _residual32(w8, faces, v[:, :, k], np.asarray(targets, F)[:, k], F(wf), wfh, lanes[lane])
            for off in (8, 4, 2, 1):
                lanes = (lanes + lanes[np.arange(16) ^ off]).astype(F)
            acc = np.where(inb[None, :], lanes[0], F(0))
        vd = np.where(ok_w[None, :], VC._corners(vol["dist"], i), F(0))
        accd = acc.copy()
        _residual32(w8, faces, vd, np.zeros(N, F) if dist_targets is None else np.asarray(dist_targets, F), F(wd), wdh, accd)
    acc = np.where(ok_w[None, :], accd, F(0)).astype(np.float64)
    w64 = np.where(ok_w, w.astype(np.float64), 0.0)
    xs = np.where(ok_w[:, None], x.astype(np.float64) - c, 0.0)
    G = np.stack([np.stack([acc[0], acc[1], acc[2]], -1), np.stack([acc[1], acc[3], acc[4]], -1), np.stack([acc[2], acc[4], acc[5]], -1)], -2)   # [N, 3, 3]
    q = np.stack([acc[6], acc[7], acc[8]], -1)
    X = np.zeros((N, 3, 3))
    X[:, 0, 1], X[:, 0, 2], X[:, 1, 0], X[:, 1, 2], X[:, 2, 0], X[:, 2, 1] = -xs[:, 2], xs[:, 1], xs[:, 2], -xs[:, 0], -xs[:, 1], xs[:, 0]
    M = X @ G
    H = np.zeros((6, 6))
    H[:3, :3] = np.einsum("n,nij->ij", w64, M @ X.transpose(0, 2, 1))
    H[:3, 3:] = np.einsum("n,nij->ij", w64, M)
    H[3:, :3] = H[:3, 3:].T
    H[3:, 3:] = np.einsum("n,nij->ij", w64, G)
    b = np.concatenate([np.einsum("n,nij,nj->i", w64, X, q), np.einsum("n,ni->i", w64, q)])
    miss = np.where(weighted & ~ok, w.astype(np.float64), 0.0) * float(outside) * float(outside)
    return {"H": H, "b": b, "cost": float((w64 * acc[9]).sum() + miss.sum()), "valid": int(ok_w.sum()), "in_band": int(inb.sum())}


def ratios(got, ref, slack=True):
    """worst (|got - ref64| - slack) / A over the entries of H (upper triangle), b and the cost -> (H, b, cost); slack=False: an exact_case,
    whose coordinates do not round"""
    k = 1.0 if slack else 0.0
    return (VC.worst_ratio(got["H"][TRIU], ref["H"][TRIU], ref["A_H"][TRIU], k * ref["slack_H"][TRIU]),
            VC.worst_ratio(got["b"], ref["b"], ref["A_b"], k * ref["slack_b"]),
            VC.worst_ratio(np.array([got["cost"]]), np.array([ref["cost"]]), np.array([ref["A_cost"]]), np.array([k * ref["slack_cost"]])))


def cap(C):
    """The cap of the tolerance in units of 2^-24, from the longest fp32 chain behind one entry: a value carries the three
    products of its weight, the eight terms of the blend, the subtraction of the target and the product with the weight of the term (13); a
    derivative the product of its face weight, a corner difference, four terms and the product with weight / h (7, and 2 more for weight * (1 / h)
    itself); a term of G, q or e is one fma of two such factors (13 + 13 + 1 = 27 at most), summed over ceil(C / 16) terms in a lane, four levels
    of the group fold and the distance term.  The expansion is float64 and adds nothing."""
    return (27 + -(-C // 16) + 4 + 1) * U


def tolerance(port_worst, C):
    return min(3.0 * port_worst, cap(C))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def new_state(R, t, model):
    st = np.zeros(STATE)
    st[0:9], st[9:12] = np.asarray(R, F).reshape(9), np.asarray(t, F)
    st[12:24] = st[0:12]
    st[S_MODEL:S_MODEL + 3] = np.asarray(model, F)
    st[S_LAMBDA] = LAMBDA0
    return st


def _tri(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def solve_ref(Hu, b, lam):
    """(status, delta): (H + lam D) delta = -b by the kernel's Cholesky, Hu the 21 upper entries"""
    hmax = 0.0
    for i in range(6):
        if Hu[_tri(i, i)] > hmax:                     # (fmax drops a NaN)
            hmax = Hu[_tri(i, i)]
    if not hmax > 0.0:
        return NO_GRADIENT, np.zeros(6)
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            L[i, j] = Hu[_tri(j, i)] + (lam * max(Hu[_tri(i, i)], DIAG_FLOOR * hmax) if i == j else 0.0)
    for j in range(6):
        piv = L[j, j]
        for k in range(j):
            piv -= L[j, k] * L[j, k]
        if not (piv > 0.0) or not (piv <= 1.7976931348623157e308):
            return FAILED, np.zeros(6)
        d = math.sqrt(piv)
        L[j, j] = d
        for i in range(j + 1, 6):
            s = L[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / d
    y = np.zeros(6)
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k, i] * y[k]
        y[i] = s / L[i, i]
    return RUNNING, y


def _small(d, rot_tol, trans_tol):
    return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < rot_tol and math.sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) < trans_tol


def step_ref(st, row, it, iters, rot_tol, trans_tol):
    """d3f_volume_align_step on ONE instance: st (updated in place) and the row summed at the candidate -> (history entry, pose [12] float32 the
    next accumulate reads, skip)"""
    if int(st[S_STATUS]) != RUNNING:
        return st[S_COST], st[0:12].astype(F), 1
    lam, status = st[S_LAMBDA], RUNNING
    with np.errstate(invalid="ignore"):
        accept = it == 0 or row[27] < st[S_COST]
    if accept:
        st[0:12] = st[12:24]
        st[S_H:S_H + 21], st[S_B:S_B + 6] = row[:21], row[21:27]
        st[S_COST], st[S_VALID], st[S_INBAND] = row[27], row[28], row[29]
        if it > 0:
            lam = max(lam / 10.0, LAMBDA_MIN)
            st[S_STEPS] += 1.0
            if _small(st[S_DELTA:S_DELTA + 6], rot_tol, trans_tol):
                status = CONVERGED
    else:
        lam = min(lam * 10.0, LAMBDA_MAX)
        if lam >= LAMBDA_MAX:
            status = STALLED
    st[S_LAMBDA] = lam
    hist = st[S_COST]
    solved = False
    if status == RUNNING and it < iters:
        status, delta = solve_ref(st[S_H:S_H + 21], st[S_B:S_B + 6], lam)
        solved = status == RUNNING
        if solved and accept and _small(delta, rot_tol, trans_tol):
            status, solved = CONVERGED, False         # the step proposed at a pose just accepted is below both tolerances: not taken
    st[S_STATUS] = status
    if not solved:
        st[12:24] = st[0:12]
        return hist, st[0:12].astype(F), int(status != RUNNING)
    R, t = compose(st[0:9].reshape(3, 3), st[9:12], st[S_MODEL:S_MODEL + 3], delta)
    st[12:21], st[21:24] = R.reshape(9), t
    st[S_DELTA:S_DELTA + 6] = delta
    return hist, st[12:24].astype(F), 0


def align_ref(vol, mark, name, p, R0, t0, w=None, targets=None, dist_targets=None, wd=1.0, wf=1.0, outside=None, iters=20, rot_tol=1e-5, trans_tol=None,
              model=None):
    """ONE instance -> dict(R, t (float32, kernel convention), points, cost, valid, status, steps, history [iters + 1], state)"""
    trans_tol = 1e-3 * float(vol["step"]) if trans_tol is None else trans_tol
    model = centroid(np.asarray(p, F), w) if model is None else model
    st = new_state(R0, t0, model)
    pose = st[12:24].astype(F)
    history = np.zeros(iters + 1)
    skip = 0
    row = np.zeros(ROW)
    for it in range(iters + 1):
        if not skip:
            row = row_of(accumulate64(vol, mark, name, p, pose[:9].reshape(3, 3), pose[9:], model, w, targets, dist_targets, wd, wf, outside))
        history[it], pose, skip = step_ref(st, row, it, iters, rot_tol, trans_tol)
    R, t = st[0:9].reshape(3, 3).astype(F), st[9:12].astype(F)
    return {"R": R, "t": t, "points": transform32(R, t, p), "cost": st[S_COST], "valid": int(st[S_VALID]), "status": int(st[S_STATUS]), "steps": int(st[S_STEPS]),
            "history": history, "state": st}


# ---- cases: the entry-by-entry comparison ---------------------------------------------------------------------------------------------------
COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)       # 255 / 256 / 257 / 513 straddle the 256 points of a workgroup
CHANNELS = (1, 3, 4, 16, 20, 68)
BAND_QUANTILE = 0.1                                             # a tenth of the valid voxels seed the band: 1 - 0.9^8 = 57 % of the valid cells are kept


def band_of(vol):
    """a band (float32 world length) that keeps a part of the valid cells of a volume_cases volume, whose dist is noise around 0 or 2"""
    return F(np.quantile(np.abs(vol["dist"][vol["valid"]].astype(np.float64)), BAND_QUANTILE))


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    return rodrigues(axis / np.linalg.norm(axis) * angle)


@functools.lru_cache(maxsize=None)
def volume_of(shape_name, C, seed, invalid_frac=0.0):
    """volume_cases.make_volume with one set 's0' of C channels, NaN in its invalid voxels; built once, shared, not modified"""
    return VC.make_volume(VC.SHAPES[shape_name], (C,), seed, invalid_frac, poison=invalid_frac > 0)


@functools.lru_cache(maxsize=None)
def entry_case(shape_name, C, n, seed, invalid_frac=0.0, special=False, variant=0, away=False):
    """A volume of volume_cases with one set of C channels and n model points under a small pose whose images are volume_cases.inside_points
    (so validity is decided away from every lattice plane: the float32 and the float64 side agree on it); `special` replaces the leading
    points by images outside the volume, NaN coordinates and zero weights; `variant` draws other points and another pose in the SAME volume (the
    instances of one call); `away` moves the pose so that every image falls outside.  -> dict(vol, p, R, t, w, targets, dist_targets)"""
    vol = volume_of(shape_name, C, seed, invalid_frac)
    rng = np.random.default_rng(7000 + 13 * seed + n + 100003 * variant)
    R = rotation(rng.standard_normal(3), 0.2).astype(F)
    t = (0.05 * rng.standard_normal(3)).astype(F)
    x = VC.inside_points(VC.SHAPES[shape_name], n, seed + 50 * variant).astype(np.float64)
    if special and n >= 15:
        sp = VC.special_points(VC.SHAPES[shape_name]).astype(np.float64)[:n // 3]
        x[:len(sp)] = sp
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((x - t.astype(np.float64)) @ R.astype(np.float64)).astype(F)   # R^T (x - t); NaN and infinities stay what they are
    w = rng.uniform(0.5, 2.0, n).astype(F)
    if special:
        w[rng.random(n) < 0.15] = 0
    if away:
        t = (t + F(3.0)).astype(F)
    image = transform32(R, t, p)
    g = (image.astype(np.float64) - np.asarray(VC.ORIGIN, np.float64)) / VC.STEP
    with np.errstate(invalid="ignore"):
        near = np.isfinite(g).all(axis=1) & (np.abs(g - np.round(g)).min(axis=1) < 1e-5) & (g > -1).all(axis=1) & (g < np.asarray(VC.SHAPES[shape_name])).all(axis=1)
    w[near] = 0                      # an image that rounding put next to a lattice plane takes no part (the special points ON a face among them)
    with np.errstate(invalid="ignore"):
        w[np.isfinite(p).all(axis=1) & (np.abs(p) > 1e3).any(axis=1)] = 0      # nor one at 1e30: it would drag the pivot, and every bound, with it
    ref = VC.trilinear64(vol, image, ["s0"])
    targets = (ref["s0"][0] + 0.1 * rng.standard_normal((n, C))).astype(F)
    dist_targets = (0.05 * rng.standard_normal(n)).astype(F)
    return {"vol": vol, "p": p, "R": R, "t": t, "w": w, "targets": targets, "dist_targets": dist_targets}


@functools.lru_cache(maxsize=None)
def exact_case(shape_name, C, n, seed, invalid_frac=0.0):
    """The sibling of entry_case whose coordinates do not round: the identity pose (the chain returns p itself) and points at
    origin + (cell + k / 256) step, 3 <= k <= 253 -- p - origin, the division and t = g - i are exact in float32, so the float32 and the float64
    side see the SAME t, the coordinate slack is legitimately zero and what is left is the rounding of the per-point arithmetic against A."""
    vol = volume_of(shape_name, C, seed, invalid_frac)
    rng = np.random.default_rng(8000 + 13 * seed + n)
    cells = np.asarray(VC.SHAPES[shape_name]) - 1
    g = rng.integers(0, cells, size=(n, 3)) + rng.integers(3, 254, size=(n, 3)) / 256.0
    p = (np.asarray(VC.ORIGIN, np.float64) + g * VC.STEP).astype(F)
    assert np.array_equal((p.astype(np.float64) - np.asarray(VC.ORIGIN, np.float64)) / VC.STEP, g)
    assert np.array_equal(((p - np.asarray(VC.ORIGIN, F)) / F(VC.STEP)).astype(np.float64), g)
    w = rng.uniform(0.5, 2.0, n).astype(F)
    targets = (VC.trilinear64(vol, p, ["s0"])["s0"][0] + 0.1 * rng.standard_normal((n, C))).astype(F)
    return {"vol": vol, "p": p, "R": np.eye(3, dtype=F), "t": np.zeros(3, F), "w": w, "targets": targets, "dist_targets": (0.05 * rng.standard_normal(n)).astype(F)}


# ---- cases: the scene of the loop ---------------------------------------------------------------------------------------------------------
SCENE_SHAPE = (24, 20, 18)
SCENE_CHANNELS = 4
SCENE_BAND_STEPS = 2.0
SPHERES = (((9.0, 9.5, 8.5), 5.2), ((17.0, 10.5, 9.5), 3.4))     # centres and radii in voxels
STARTS = ((5.0, 1.5, 0), (10.0, 2.5, 1), (10.0, 2.5, 2), (7.0, 2.0, 3))      # degrees, voxels, seed of the direction


@functools.lru_cache(maxsize=None)
def scene():
    """Two spheres of different radii in a 24 x 20 x 18 volume with step 2^-5, dist clamped to +- 3 steps, four smooth descriptor channels that
    no rotation leaves unchanged, 225 surface points (150 + 75) as the model at a true pose, targets sampled from the field at that pose."""
    h = VC.STEP
    origin = np.asarray(VC.ORIGIN, np.float64)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in SCENE_SHAPE], indexing="ij"), -1).astype(np.float64)
    sd = np.min([np.linalg.norm(idx - np.asarray(c), axis=-1) - r for c, r in SPHERES], axis=0) * h
    vol = {"origin": np.asarray(VC.ORIGIN, F), "step": F(h), "shape": SCENE_SHAPE, "dist": np.clip(sd, -3 * h, 3 * h).astype(F),
           "valid": np.ones(SCENE_SHAPE, bool), "sets": {}, "fills": {"feat": None}}
    k = np.array([[0.23, 0.11, -0.07], [-0.09, 0.21, 0.13], [0.05, -0.12, 0.19], [0.16, 0.14, 0.10]])
    vol["sets"]["feat"] = np.sin(idx @ k.T + np.array([0.3, 1.1, 2.0, 0.7])).astype(F)
    rng = np.random.default_rng(424242)
    surf = []
    for (c, r), count in zip(SPHERES, (150, 75)):
        d = rng.standard_normal((count, 3))
        surf.append(np.asarray(c) + r * d / np.linalg.norm(d, axis=1, keepdims=True))
    q = origin + np.concatenate(surf) * h                                     # on the surface, in the field's frame
    R_true = rotation((0.3, -0.5, 0.8), np.deg2rad(12.0)).astype(F)
    t_true = (np.array([0.6, -0.4, 0.5]) * h).astype(F)
    p = ((q - t_true.astype(np.float64)) @ R_true.astype(np.float64)).astype(F)
    x_true = transform32(R_true, t_true, p)
    targets = VC.trilinear64(vol, x_true, ["feat"])["feat"][0].astype(F)
    return {"vol": vol, "p": p, "R": R_true, "t": t_true, "x": x_true, "targets": targets}


def scene_start(deg, voxels, seed):
    """the true pose moved by a rotation of `deg` degrees about the model's centroid image and a shift of `voxels` voxels, directions by `seed`"""
    s = scene()
    rng = np.random.default_rng(99 + seed)
    E = rotation(rng.standard_normal(3), np.deg2rad(deg))
    d = rng.standard_normal(3)
    shift = voxels * VC.STEP * d / np.linalg.norm(d)
    c = s["x"].astype(np.float64).mean(axis=0)
    R = (E @ s["R"].astype(np.float64)).astype(F)
    t = (c + E @ (s["t"].astype(np.float64) - c) + shift).astype(F)
    return R, t


def point_error_voxels(points):
    """the largest distance of a point from its place at the true pose, in voxels"""
    return float(np.linalg.norm(points.astype(np.float64) - scene()["x"].astype(np.float64), axis=1).max() / VC.STEP)
