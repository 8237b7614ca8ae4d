"""TEST INFRASTRUCTURE ONLY -- float64 gradients of the field query and of the tracking loss w.r.t. the points.

The backward kernels (csrc/fuse_backward.hip, the gradient inside csrc/track_kernels.hip) are checked against this module
point by point.  It is the op sequence of oracle/torch_port.py (Fusion.eval, fusion.py:305-394; Fusion.eval_dist, :396-436;
the tracking loss, :1643-1665) in float64, differentiated by autograd, with one change: every DISCRETE choice is taken
from float32 arithmetic written like the kernel's (csrc/d3f_device.h: project_point, nearest_depth, unnormalize,
in_bounds; the forward pins these bit for bit), and float64 only computes what is continuous given those choices.  A point
on a texel line or on a branch edge then gets the one-sided derivative the float32 code takes; no point is excluded.
The choices, per view:
  - ok = |zc| >= 1e-4 (else zc := 1e-3);
  - the nearest depth texel (and with it the depth value d);
  - validity: d > 0, ok, and dist > -mu (eval only);
  - the bilinear cell floor(((g+1)/2)*(size-1)) of every map and which of its corners are in bounds;
  - the branches of clamp(dist, -mu, mu) and of clamp(mu - |dist|, max=0) in the weight.
Non-finite values follow the reference's autograd: an in-bounds corner that holds a NaN / Inf reaches the gradient
through 0 * NaN even when its view is invalid, a NaN weight does the same, and so does a non-finite projection.

`scale` is, per point and coordinate, the sum over views, terms and channels of |each contribution| (|K| @ |pose| for the
projection): the size of the float32 rounding a kernel can make where contributions cancel.  A kernel passes when
|g - g64| <= TOL * scale elementwise; TOL is calibrated on the float32 torch port (tests/test_grad_ref.py).
"""
import torch

# Per-entry bound |g - g64| <= TOL * scale.  The float32 torch port's worst ratio over every case of
# tests/test_gpu_grad.py and tests/test_grad_ref.py is 2.76e-7 (tests/test_grad_ref.py::test_float32_port_within_bound_and_tol_calibrated
# measures it); TOL is a few times that.
TOL = 1e-6
PORT_WORST = 2.8e-7
F64 = torch.float64


def _krt32(K, pose):
    """KRt = K @ pose in float32, k-sequential and unfused (d3f_device.h: compute_krt)."""
    K, pose = K.float(), pose[:, :3, :].float()
    acc = torch.zeros(K.shape[0], 3, 4)
    for k in range(3):
        acc = acc + K[:, :, k:k + 1] * pose[:, k:k + 1, :]
    return acc


def decisions(obs, pts32, H, W, mu, maps=(), mode="eval"):
    """The float32 choices of every (view, point) as the kernels make them.  pts32 [N,3] float32; maps: [V,fh,fw,C]
    tensors (only their shapes matter).  Returns a dict of [V,N] tensors (and per map a dict of cells / corner flags)."""
    M = _krt32(obs["K"], obs["pose"])                                            # [V,3,4]
    p = pts32.float()
    px, py, pz = p[:, 0][None], p[:, 1][None], p[:, 2][None]

    def row(i):
        return ((M[:, i, 0:1] * px + M[:, i, 1:2] * py) + M[:, i, 2:3] * pz) + M[:, i, 3:4] * 1.0

    xc, yc, zc = row(0), row(1), row(2)
    ok = ~(zc.abs() < 1e-4)
    zc = torch.where(ok, zc, torch.full_like(zc, 1e-3))
    u, w = xc / zc, yc / zc
    gx = u / float(W - 1) * 2.0 - 1.0
    gy = w / float(H - 1) * 2.0 - 1.0
    rx = torch.round(((gx + 1.0) / 2.0) * float(W - 1))                          # rintf: half to even
    ry = torch.round(((gy + 1.0) / 2.0) * float(H - 1))
    inb = (rx > -1.0) & (rx < W) & (ry > -1.0) & (ry < H)
    V = M.shape[0]
    ix = torch.where(inb, rx, torch.zeros_like(rx)).long()
    iy = torch.where(inb, ry, torch.zeros_like(ry)).long()
    vv = torch.arange(V)[:, None].expand_as(ix)
    d = torch.where(inb, obs["depth"].float()[vv, iy, ix], torch.zeros_like(rx))
    dist = d - zc
    valid = (d > 0.0) & ok
    if mode == "eval":
        valid = valid & (dist > -mu)
    out = dict(ok=ok, d=d, dist=dist, valid=valid, gx=gx, gy=gy, zc=zc,
               clamp_pass=(dist >= -mu) & (dist <= mu), wgt_pass=(mu - dist.abs()) <= 0.0, cells=[])
    for m in maps:
        fh, fw = int(m.shape[1]), int(m.shape[2])
        fx = ((gx + 1.0) / 2.0) * float(fw - 1)
        fy = ((gy + 1.0) / 2.0) * float(fh - 1)
        x0, y0 = torch.floor(fx), torch.floor(fy)
        x1, y1 = x0 + 1.0, y0 + 1.0

        def ib(x, y):
            return (x > -1.0) & (x < fw) & (y > -1.0) & (y < fh)

        out["cells"].append(dict(x0=x0, y0=y0, inb=(ib(x0, y0), ib(x1, y0), ib(x0, y1), ib(x1, y1))))
    return out


def _gather(m, vv, yi, xi, inb):
    """[V,n,C] float64 texels at integer coordinates (out-of-bounds corners read texel 0 and are masked by the caller)."""
    xi = torch.where(inb, xi, torch.zeros_like(xi)).long()
    yi = torch.where(inb, yi, torch.zeros_like(yi)).long()
    return m[vv, yi, xi].to(F64)


def _field64(obs, p64, dec, H, W, mu, maps, mode, sl):
    """Fusion.eval / eval_dist of the rows `sl` in float64 from the float32 choices `dec` (autograd-ready)."""
    K, pose = obs["K"].to(F64), obs["pose"][:, :3, :].to(F64)
    M = K @ pose                                                                  # [V,3,4]
    n = p64.shape[0]
    homog = torch.cat((p64, p64.new_ones(n, 1)), dim=1)
    cam = torch.einsum("vij,nj->vni", M, homog)                                  # [V,n,3]
    ok = dec["ok"][:, sl]
    z = torch.where(ok, cam[..., 2], torch.full_like(cam[..., 2], 1e-3))       # z[degenerate] = 1e-3 (zero gradient there)
    uvx, uvy = cam[..., 0] / z, cam[..., 1] / z
    gx = uvx / (W - 1) * 2 - 1
    gy = uvy / (H - 1) * 2 - 1
    d = dec["d"][:, sl].to(F64)
    # the nearest-mode depth lookup: grid_sample passes an exact zero to the grid (0 / z is NaN where z is)
    sd = d - z + torch.where(torch.zeros_like(ok), gx + gy, torch.zeros_like(gx))
    livef = dec["valid"][:, sl].to(F64)
    count = livef.sum(0)
    empty = count == 0
    if mode == "eval_dist":
        return {"dist": (sd * livef).sum(0) / (count + 1e-6)}, None
    # clamp(sd, -mu, mu) and clamp(mu - |sd|, max=0) with the float32 branches; a NaN stays NaN like in torch.clamp
    cd = torch.where(dec["clamp_pass"][:, sl], sd, sd.detach().clamp(-mu, mu))
    t = mu - sd.abs()
    nan = torch.isnan(dec["dist"][:, sl])
    t = torch.where(dec["wgt_pass"][:, sl], t, torch.zeros_like(t)) + torch.where(nan, torch.full_like(d, float("nan")), torch.zeros_like(d))
    weight = torch.exp(t / mu)
    dist = (cd * livef).sum(0) / (count + 1e-6)
    out = {"dist": torch.where(empty, torch.full_like(dist, 1e3), dist)}
    V = M.shape[0]
    vv = torch.arange(V)[:, None].expand(V, n)
    samples = []                                                                  # per map [V,n,C]: the '<k>_inter' rows
    for k, m in enumerate(maps):
        if m is None:
            out["map%d" % k] = None
            samples.append(None)
            continue
        c = dec["cells"][k]
        fh, fw = int(m.shape[1]), int(m.shape[2])
        ix = ((gx + 1) / 2) * (fw - 1)
        iy = ((gy + 1) / 2) * (fh - 1)
        x0, y0 = c["x0"][:, sl].to(F64), c["y0"][:, sl].to(F64)
        tx, ty = ix - x0, iy - y0
        wts = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
        xs, ys = (c["x0"][:, sl], c["x0"][:, sl] + 1, c["x0"][:, sl], c["x0"][:, sl] + 1), (c["y0"][:, sl], c["y0"][:, sl], c["y0"][:, sl] + 1, c["y0"][:, sl] + 1)
        per_view = 0
        for q in range(4):
            inb = c["inb"][q][:, sl]
            val = _gather(m, vv, ys[q], xs[q], inb)
            val = torch.where(inb[..., None], val, torch.zeros_like(val))     # (texel 0 of a masked corner may be a NaN)
            # grid_sample sums over in-bounds corners only: an out-of-bounds corner passes no gradient, not even 0 * NaN
            per_view = per_view + torch.where(inb[..., None], val * wts[q][..., None], torch.zeros_like(val))
        fused = (per_view * livef[..., None] * weight[..., None]).sum(0) / (count[:, None] + 1e-6)
        out["map%d" % k] = torch.where(empty[:, None], torch.zeros_like(fused), fused)
        samples.append(per_view)
    return out, dict(M=M, z=z, uvx=uvx, uvy=uvy, weight=weight, livef=livef, count=count, empty=empty, samples=samples)


def corner_terms(m, c, sl, aux, H, W, vv):
    """The sizes a bound on one map is built from, per (view, point[, channel]) of the rows `sl` (no autograd): the float64
    sampling position ix, iy and fractions tx, ty (clamped to [0, 1]); va, the |texels| of the four corners (0 where out
    of bounds or non-finite); s = sum_q |w_q| |T_q|; dx, dy: bounds of d/dtx and d/dty of the bilinear value from the
    |texels| (what its derivatives are made of), ddx, ddy: |d/dtx| and |d/dty| of the value itself; px, py:
    the float32 rounding of the sampling position in units of eps (~ |ix| + fw)."""
    fh, fw = int(m.shape[1]), int(m.shape[2])
    gx = aux["uvx"] / (W - 1) * 2 - 1
    gy = aux["uvy"] / (H - 1) * 2 - 1
    ix, iy = ((gx + 1) / 2) * (fw - 1), ((gy + 1) / 2) * (fh - 1)
    tx = torch.nan_to_num(ix - c["x0"][:, sl].to(F64)).clamp(0, 1)
    ty = torch.nan_to_num(iy - c["y0"][:, sl].to(F64)).clamp(0, 1)
    x0, y0 = c["x0"][:, sl], c["y0"][:, sl]
    xs, ys = (x0, x0 + 1, x0, x0 + 1), (y0, y0, y0 + 1, y0 + 1)
    va = [torch.nan_to_num(_gather(m, vv, ys[q], xs[q], c["inb"][q][:, sl]), nan=0.0, posinf=0.0, neginf=0.0).abs()
          * c["inb"][q][:, sl][..., None] for q in range(4)]
    wts = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
    s = va[0] * wts[0][..., None] + va[1] * wts[1][..., None] + va[2] * wts[2][..., None] + va[3] * wts[3][..., None]
    dx = (va[0] + va[1]) * (1 - ty)[..., None] + (va[2] + va[3]) * ty[..., None]
    dy = (va[0] + va[2]) * (1 - tx)[..., None] + (va[1] + va[3]) * tx[..., None]
    # |d/dtx|, |d/dty| of the bilinear value itself (signed corner differences; the value is linear in tx, ty in a cell)
    t = [torch.nan_to_num(_gather(m, vv, ys[q], xs[q], c["inb"][q][:, sl]), nan=0.0, posinf=0.0, neginf=0.0)
         * c["inb"][q][:, sl][..., None] for q in range(4)]
    ddx = ((t[1] - t[0]) * (1 - ty)[..., None] + (t[3] - t[2]) * ty[..., None]).abs()
    ddy = ((t[2] - t[0]) * (1 - tx)[..., None] + (t[3] - t[1]) * tx[..., None]).abs()
    # float32 rounding of the sampling position (ix, iy: ~eps * (|ix| + fw)) moves the corner differences and weights
    px = (torch.nan_to_num(ix).abs() + fw).clamp(max=1e6)
    py = (torch.nan_to_num(iy).abs() + fh).clamp(max=1e6)
    return dict(fh=fh, fw=fw, ix=ix, iy=iy, tx=tx, ty=ty, va=va, wts=wts, s=s, dx=dx, dy=dy, ddx=ddx, ddy=ddy, px=px, py=py)


def _scale(obs, dec, H, W, mu, maps, mode, sl, gd, gks, aux):
    """Per (point, coordinate): sum over views / terms / channels of |contribution| (no autograd)."""
    with torch.no_grad():
        Ma = obs["K"].to(F64).abs() @ obs["pose"][:, :3, :].to(F64).abs()       # [V,3,4]
        z, livef = aux["z"].abs(), aux["livef"]
        A = 1.0 / (aux["count"] + 1e-6)
        wgt = torch.nan_to_num(aux["weight"], nan=1.0)
        ga = gd.abs()[None] * A * livef if gd is not None else 0.0                # dist-clamp term, per view
        g_u, g_w, g_wgt = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)         # |terms|
        p_u, p_w, p_wgt = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)         # their position rounding
        V, n = z.shape
        vv = torch.arange(V)[:, None].expand(V, n)
        for k, m in enumerate(maps):
            if m is None or gks[k] is None:
                continue
            ct = corner_terms(m, dec["cells"][k], sl, aux, H, W, vv)
            fh, fw, va, s, dx, dy, px, py = ct["fh"], ct["fw"], ct["va"], ct["s"], ct["dx"], ct["dy"], ct["px"], ct["py"]
            g = gks[k].to(F64).abs()[None]                                       # [1,n,C]
            cross = (g * (va[0] + va[1] + va[2] + va[3])).sum(-1)
            sdx, sdy = (g * dx).sum(-1), (g * dy).sum(-1)
            g_wgt = g_wgt + (g * s).sum(-1) * A * livef
            p_wgt = p_wgt + (sdx * px + sdy * py) * A * livef
            g_u = g_u + sdx * A * livef * wgt * (fw - 1) / (W - 1)
            p_u = p_u + cross * py * A * livef * wgt * (fw - 1) / (W - 1)
            g_w = g_w + sdy * A * livef * wgt * (fh - 1) / (H - 1)
            p_w = p_w + cross * px * A * livef * wgt * (fh - 1) / (H - 1)
        if mode == "eval":
            # weight branch: wgt = exp((mu - |dist|) / mu) carries dist's rounding (~eps * (|d| + |zc|)) times 1/mu
            amp = 1.0 + torch.where(dec["wgt_pass"][:, sl], (dec["d"][:, sl].to(F64).abs() + z) / mu, torch.zeros_like(z))
            amp = torch.nan_to_num(amp, nan=1.0, posinf=1.0)
            g_u, g_w, g_wgt = g_u * amp, g_w * amp, g_wgt * amp
        g_u, g_w, g_wgt = g_u + p_u, g_w + p_w, g_wgt + p_wgt
        g_dist = ga + (g_wgt * wgt / mu if mode == "eval" else 0.0)
        ua, wa = torch.nan_to_num(aux["uvx"]).abs(), torch.nan_to_num(aux["uvy"]).abs()
        g_xc, g_yc = g_u / z, g_w / z
        g_zc = (g_u * ua + g_w * wa) / z + g_dist
        # rounding of the projection itself: |zc| error ~ eps * (|M| . |p|); carried by the same terms
        sc = (torch.einsum("vn,vj->nj", g_xc, Ma[:, 0, :3]) + torch.einsum("vn,vj->nj", g_yc, Ma[:, 1, :3])
              + torch.einsum("vn,vj->nj", g_zc, Ma[:, 2, :3]))
        return sc


def field_grad(obs, pts, H, W, mu=0.02, maps=(), grad_dist=None, grad_maps=(), mode="eval", rows=None, dec=None, chunk_elems=1 << 22):
    """float64 d(loss)/d(pts) for loss = <grad_dist, dist> + sum_k <grad_maps[k], fused_k>  (eval) or <grad_dist, dist>
    (eval_dist), on rows `rows` (all by default).  maps: [V,fh,fw,C] tensors (fp32 or fp16, read as stored), None where
    the map is not queried; grad_maps[k] None: that map's output has no upstream gradient (it then plays no part).
    Returns (grad [n,3] float64, scale [n,3] float64, decisions)."""
    pts = pts.detach().cpu()
    rows = torch.arange(pts.shape[0]) if rows is None else torch.as_tensor(rows)
    p32 = pts[rows].float()
    obs = {k: v.detach().cpu() for k, v in obs.items()}
    maps = [None if m is None else m.detach().cpu() for m in maps]
    grad_maps = list(grad_maps) + [None] * (len(maps) - len(grad_maps))
    used = [m for m, g in zip(maps, grad_maps) if m is not None and g is not None]
    gks_all = [None if g is None else g.detach().cpu()[rows] for g in grad_maps]
    gmaps = [m if g is not None else None for m, g in zip(maps, grad_maps)]
    gd_all = None if grad_dist is None else grad_dist.detach().cpu()[rows].to(F64)
    if dec is None:
        dec = decisions(obs, p32, H, W, mu, [m if m is not None else torch.zeros(1, 1, 1, 1) for m in maps], mode)
    V = obs["depth"].shape[0]
    width = V * max([1] + [int(m.shape[3]) for m in used])
    step = max(1, chunk_elems // width)
    grads, scales = [], []
    for a in range(0, p32.shape[0], step):
        sl = slice(a, min(a + step, p32.shape[0]))
        p64 = p32[sl].to(F64).requires_grad_(True)
        out, aux = _field64(obs, p64, dec, H, W, mu, gmaps, mode, sl)
        loss = p64.new_zeros(())
        gd = None if gd_all is None else gd_all[sl]
        if gd is not None:
            loss = loss + (gd * out["dist"]).sum()
        gks = [None if g is None else g[sl] for g in gks_all]
        for k, g in enumerate(gks):
            if g is not None and mode == "eval":
                loss = loss + (g.to(F64) * out["map%d" % k]).sum()
        if loss.requires_grad:
            (gp,) = torch.autograd.grad(loss, p64)
        else:
            gp = torch.zeros_like(p64)
        grads.append(gp.detach())
        if aux is None:      # eval_dist: the dist term only, through zc
            with torch.no_grad():
                Ma = obs["K"].to(F64).abs() @ obs["pose"][:, :3, :].to(F64).abs()
                lv = dec["valid"][:, sl].to(F64)
                g_zc = gd.abs()[None] * lv / (lv.sum(0) + 1e-6)
                scales.append(torch.einsum("vn,vj->nj", g_zc, Ma[:, 2, :3]))
        else:
            scales.append(_scale(obs, dec, H, W, mu, gmaps, mode, sl, gd, gks, aux))
    # the kernels sum the V views of a point in order: recursive summation carries up to (V - 1) * eps of sum |terms|,
    # which TOL (~16 fp32 eps) covers for V <= 17
    return torch.cat(grads), torch.cat(scales) * max(1.0, (V - 1) / 16.0), dec


def check(g, g64, scale, tol=TOL):
    """(ok, worst ratio, message): the non-finite entries of g and g64 must coincide; finite ones |g-g64| <= tol*scale."""
    g = torch.as_tensor(g).detach().cpu().to(F64)
    nf, nf64 = ~torch.isfinite(g), ~torch.isfinite(g64)
    if not torch.equal(nf, nf64):
        bad = (nf != nf64).nonzero()
        return False, float("inf"), "non-finite sets differ at %d entries, first %s (kernel %s, reference %s)" % (
            bad.shape[0], bad[0].tolist(), g[bad[0, 0]].tolist(), g64[bad[0, 0]].tolist())
    fin = ~nf64
    err = (g - g64).abs()[fin]
    lim = scale[fin]
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > tol:
        i = int(ratio.argmax())
        rowcol = fin.nonzero()[i].tolist()
        return False, worst, "entry %s: got %.9g, float64 %.9g, scale %.3g (ratio %.3g > %.3g)" % (
            rowcol, float(g[tuple(rowcol)]), float(g64[tuple(rowcol)]), float(scale[tuple(rowcol)]), worst, tol)
    return True, worst, "ok"


# ---- the tracking loss (fusion.py:1643-1665) ------------------------------------------------------------------------------
def _so3_exp_map64(w, big):
    """pytorch3d's so3_exp_map in float64 with the float32 choice of the angle clamp (big: |w|^2 >= 1e-4)."""
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    o = torch.zeros_like(x)
    skew = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=1).view(-1, 3, 3)
    n2 = (w * w).sum(1)
    theta = torch.where(big, n2, n2.detach() * 0 + 1e-4).sqrt()
    a = (theta.sin() / theta)[:, None, None]
    b = ((1.0 - theta.cos()) / (theta * theta))[:, None, None]
    return a * skew + b * torch.bmm(skew, skew) + torch.eye(3, dtype=w.dtype)[None]


def track_grad(obs, H, W, descriptors, last, src, t, w, pts32, mu=0.02, dist_w=100.0, reg_w=1.0):
    """float64 d(loss)/d(t, w) [I,6] of one tracking step (loss of rigid.py::_iteration / fusion.py:1643-1665) at the
    parameters t, w [I,3]; pts32 [I*n,3]: the float32 keypoints the kernel evaluated (its choices are taken there).
    Returns (grad [I,6], scale [I,6])."""
    obs = {k: v.detach().cpu() for k, v in obs.items()}
    m = descriptors.detach().cpu()
    I, n = last.shape[0], last.shape[1]
    last64, src64 = last.detach().cpu().to(F64), src.detach().cpu().to(F64)
    t32, w32 = t.detach().cpu().float(), w.detach().cpu().float()
    big = (w32 * w32).sum(1) >= 1e-4
    dec = decisions(obs, pts32.detach().cpu().float(), H, W, mu, [m])
    t64 = t32.to(F64).requires_grad_(True)
    w64 = w32.to(F64).requires_grad_(True)
    cur = (torch.bmm(last64, _so3_exp_map64(w64, big)) + t64[:, None, :]).reshape(-1, 3)
    out, aux = _field64(obs, cur, dec, H, W, mu, [m], "eval", slice(None))
    live = (~aux["empty"]).to(F64)
    diff = out["map0"] - src64
    feat = (diff.norm(dim=-1) * live).mean()
    # clamp(dist * valid, min=0): the float32 branch (dist * valid >= 0) from the kernel's view-ordered mean
    dsum = torch.zeros(dec["dist"].shape[1])
    cnt = torch.zeros(dec["dist"].shape[1])
    for v in range(dec["dist"].shape[0]):
        vf = dec["valid"][v].float()
        dsum = dsum + dec["dist"][v].clamp(-mu, mu) * vf
        cnt = cnt + vf
    d32 = torch.where(cnt == 0, torch.full_like(dsum, 1e3), dsum / (cnt + 1e-6))
    pos = (d32 * (cnt != 0).float()) >= 0
    dv = out["dist"] * live
    dist_t = dist_w * torch.where(pos, dv, dv.detach() * 0).mean()
    reg = reg_w * (t64.norm() + w64.norm())
    loss = feat + dist_t + reg
    gt, gw = torch.autograd.grad(loss, (t64, w64))
    grad = torch.cat((gt, gw), 1)
    # scale: the field term through |d pts / d(t, w)| (|last| bounds the rotation's derivative near the tested angles)
    N = I * n
    with torch.no_grad():
        unit = diff / diff.norm(dim=-1, keepdim=True).clamp_min(1e-300)
        g_f = unit * live[:, None] / N
        g_d = dist_w * pos.to(F64) * live / N
    _, sc, _ = field_grad(obs, cur.detach().float(), H, W, mu, [m], g_d, [g_f], dec=dec)
    sc_pt = sc.sum(1).view(I, n)                                               # per keypoint, all coordinates
    lab = last64.abs().sum(-1).view(I, n) + 1.0
    scale = torch.cat(((sc_pt.sum(1))[:, None].expand(I, 3), (sc_pt * lab).sum(1)[:, None].expand(I, 3)), 1)
    scale = scale + reg_w * (torch.cat((t64.detach().abs() / max(float(t64.detach().norm()), 1e-30),
                                         w64.detach().abs() / max(float(w64.detach().norm()), 1e-30)), 1) + 1e-7)
    return grad.detach(), scale


def field_loss64(obs, p64, H, W, mu, maps, grad_dist, grad_maps, mode, dec):
    """Per-row float64 loss <grad_dist, dist> + sum_k <grad_maps[k], fused_k> at points p64 with the choices `dec` held
    fixed (for finite differences)."""
    with torch.no_grad():
        out, _ = _field64(obs, p64.to(F64), dec, H, W, mu, list(maps), mode, slice(None))
        loss = grad_dist.to(F64) * out["dist"]
        for k, g in enumerate(grad_maps):
            if g is not None and mode == "eval":
                loss = loss + (g.to(F64) * out["map%d" % k]).sum(-1)
        return loss


def same_choices(obs, pa, pb, H, W, mu, maps, mode, delta=1e-4):
    """Per row: the float32 choices are the same at p +- delta along pa - p (a point at least delta from every boundary)."""
    base = (pa + pb) / 2
    dirn = (pa - pb) / (pa - pb).abs().max()
    ds = [decisions(obs, (base + s * delta * dirn).float(), H, W, mu, maps, mode) for s in (0, 1, -1)]
    keys = ("ok", "valid", "clamp_pass", "wgt_pass", "d")
    same = torch.ones(base.shape[0], dtype=torch.bool)
    for d in ds[1:]:
        for k in keys:
            same &= (d[k] == ds[0][k]).all(0)
        for c, c0 in zip(d["cells"], ds[0]["cells"]):
            same &= ((c["x0"] == c0["x0"]) & (c["y0"] == c0["y0"])).all(0)
    return same
