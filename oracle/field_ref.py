"""TEST INFRASTRUCTURE ONLY -- the fused wide feature map of Fusion.eval / batch_eval in float64, entry by entry.

The forward kernels (csrc/fuse_direct.hip, fuse_window.hip, fuse_runs.hip, fuse_sliced.hip, fuse_rows.hip: every family
shares the fold of csrc/fuse_common.h) are checked against this module per (point, channel).  The value is
oracle/grad_ref.py's: every DISCRETE choice (validity, nearest depth texel, bilinear cell, which corners are in bounds,
the weight's branch) is taken by float32 arithmetic written like the kernel's (grad_ref.decisions), and float64 computes
what is continuous given those choices (grad_ref._field64), so a point on a texel line or a branch edge is compared on
the side the float32 code takes.  Non-finite entries follow the reference: a NaN / Inf texel in an in-bounds corner
reaches the row through 0 * NaN even where its view is invalid, and so does a NaN weight.

`scale`, per (point, channel), is the size of the float32 rounding an implementation of the reference's operation
sequence may make there, in units of float32 eps (TOL carries eps):
  - the sum over views and corners of |w_q T_q| * valid * wgt / (cnt + 1e-6): the bilinear chain, the product with the
    weight, the sum over views and the division (or the fold  w_q * wgt * rcp(cnt + 1e-6)  of fuse_common.h, which
    rounds the same products in another order);
  - the rounding of the sampling position: ix = ((u / (W - 1)) * 2 - 1 + 1) / 2 * (fw - 1) is off by ~eps * (|ix| + fw),
    plus the projection's own cancellation, |dxc| + |u| |dzc| over |zc| with |dxc| ~ eps * (|M| . |p, 1|) (|K| @ |pose|),
    times (fw - 1) / (W - 1); the value, linear in the position inside its cell, moves by that times |d/dtx|, |d/dty|
    (grad_ref.corner_terms ddx, ddy: the signed corner differences);
  - the rounding of the weight's exponent: wgt = exp((mu - |d - zc|) / mu) carries eps * (|d| + |zc| + |M_z| . |p, 1|
    + mu) / mu relatively where that branch is taken (wgt == 1 exactly elsewhere);
  - max(1, (V - 1) / 16) for the in-order sum over views (recursive summation: up to (V - 1) eps of the sum of |terms|);
  - an underflow floor: where a folded corner weight w_q * wgt / (cnt + 1e-6) is below the normal range (the float32
    weight is subnormal or zero from an exponent argument below about -87, or a small corner weight takes the product
    there), float32 holds it to an ABSOLUTE 2^-126 (flushed to zero on the device), float64 does not: that term may be
    off by |T_q| * 2^-126 whatever its size; and an entry below the normal range is itself rounded to an absolute grid
    (2^-149, or flushed), so every entry may be off by 2^-126.
The kernels use no operation the reference's sequence does not round in kind (four fma per view
and channel, one refined reciprocal), so one TOL applies to the float32 torch port, the C oracle and every kernel.
"""
import torch

from oracle import grad_ref

F64 = torch.float64
EPS32 = 2.0 ** -24
# Per-entry bound |got - f64| <= TOL * scale.  The worst ratio of the float32 implementations of the reference's order
# (the torch port and the C oracle) over the golden scenes and every case of oracle/field_cases.py is PORT_WORST
# (tests/test_field_ref.py::test_float32_port_and_oracle_within_bound_and_tol_calibrated measures it); TOL is a few
# times that.
TOL = 8e-7
PORT_WORST = 2.7e-7
# Over the thin maps (<= 256 bytes per texel) of field_cases.THIN_CASES alone the worst ratio is 2.13e-7 (the channel-range
# view of 20 channels; 2.0e-7 on C = 33, 1.96e-7 on the fp16 maps of 127 / 128 channels, 1.66e-7 and less in the
# views-in-parallel shapes with C <= 16, 1.13e-7 and less on the one-hot masks beside a wide map): no term of the scale is
# missing for the thin family.
# the underflow floor in units of eps: |T_q| * 2^-126 absolute
_FLOOR = 2.0 ** -126 / EPS32
_SUB = 2.0 ** -118                       # folded corner weights below this (with margin) may leave the normal range


def _scale(obs, dec, H, W, mu, m, k, sl, aux, p32, inter=None):
    """[n,C] float64: the bound of map k on the rows `sl` (see the module docstring), before the view-count factor.
    inter (a list): also appends [V,n,C], the bound of the per-view bilinear samples ('<k>_inter': the first two items of
    the docstring without weight, validity and division, plus the floor)."""
    Ma = obs["K"].to(F64).abs() @ obs["pose"][:, :3, :].to(F64).abs()          # [V,3,4]
    pa = torch.cat((p32.to(F64).abs(), torch.ones(p32.shape[0], 1, dtype=F64)), 1)
    pa = torch.nan_to_num(pa, nan=0.0, posinf=0.0)
    ex, ey, ez = (torch.einsum("vj,nj->vn", Ma[:, i, :], pa) for i in range(3))   # [V,n]: eps-units of xc, yc, zc
    z = aux["z"].abs()
    A = 1.0 / (aux["count"] + 1e-6)
    livef = aux["livef"]
    wgt = torch.nan_to_num(aux["weight"], nan=1.0)
    V, n = z.shape
    vv = torch.arange(V)[:, None].expand(V, n)
    ct = grad_ref.corner_terms(m, dec["cells"][k], sl, aux, H, W, vv)
    fh, fw = ct["fh"], ct["fw"]
    ua, wa = torch.nan_to_num(aux["uvx"]).abs(), torch.nan_to_num(aux["uvy"]).abs()
    proj_x = ((ex + ua * ez) / z * (fw - 1) / (W - 1)).nan_to_num(0.0).clamp(max=1e6)
    proj_y = ((ey + wa * ez) / z * (fh - 1) / (H - 1)).nan_to_num(0.0).clamp(max=1e6)
    px, py = ct["px"] + proj_x, ct["py"] + proj_y
    wpass = dec["wgt_pass"][:, sl]
    amp = 1.0 + torch.where(wpass, (dec["d"][:, sl].to(F64).abs() + z + ez + mu) / mu, torch.zeros_like(z))
    amp = torch.nan_to_num(amp, nan=1.0, posinf=1.0)
    if inter is not None:
        inter.append(ct["s"] + ct["ddx"] * px[..., None] + ct["ddy"] * py[..., None] + _FLOOR)
    fold = (livef * wgt * A)                                                    # [V,n]
    sc = (ct["s"] * amp[..., None] + ct["ddx"] * px[..., None] + ct["ddy"] * py[..., None]) * fold[..., None]
    under = 0.0
    for q in range(4):
        tiny = (livef * (ct["wts"][q] * wgt * A < _SUB)).to(F64)               # [V,n]
        under = under + ct["va"][q] * tiny[..., None]
    return (sc + under * _FLOOR).sum(0) + _FLOOR


def field64(obs, pts, H, W, mu, maps, rows=None, chunk_elems=1 << 22, parts=False):
    """Per map [n,C] float64 fused values and [n,C] float64 scale on the rows `rows` (all by default) of Fusion.eval.
    maps: [V,fh,fw,C] tensors read as stored (fp32, fp16 widened exactly, or a channel-range view whose texel stride
    exceeds C).  Returns (values, scales): two lists, one entry per map.  parts: a third item, dict(inter, inter_scale:
    per map the [V,n,C] per-view samples of '<k>_inter' and their bound; weight, livef [V,n], count [n]: the view weights
    exp(min(mu - |sd|, 0) / mu), the validity and the number of valid views)."""
    pts = pts.detach().cpu()
    rows = torch.arange(pts.shape[0]) if rows is None else torch.as_tensor(rows)
    p32 = pts[rows].float()
    obs = {k: v.detach().cpu() for k, v in obs.items()}
    maps = [m.detach().cpu() for m in maps]
    V = obs["depth"].shape[0]
    dec = grad_ref.decisions(obs, p32, H, W, mu, maps, "eval")
    step = max(1, chunk_elems // (V * max([1] + [int(m.shape[3]) for m in maps])))
    vals, scales = [[] for _ in maps], [[] for _ in maps]
    inter, inter_scale, per_point = [[] for _ in maps], [[] for _ in maps], {"weight": [], "livef": [], "count": []}
    with torch.no_grad():
        for a in range(0, p32.shape[0], step):
            sl = slice(a, min(a + step, p32.shape[0]))
            out, aux = grad_ref._field64(obs, p32[sl].to(F64), dec, H, W, mu, maps, "eval", sl)
            for k, m in enumerate(maps):
                vals[k].append(out["map%d" % k])
                scales[k].append(_scale(obs, dec, H, W, mu, m, k, sl, aux, p32[sl], inter_scale[k] if parts else None))
                if parts:
                    # a non-finite sampling position makes the four bilinear weights NaN, and grid_sample multiplies the
                    # (zeroed) out-of-bounds corners by them: the sample is NaN, whatever the texels
                    lost = ~(torch.isfinite(dec["gx"][:, sl]) & torch.isfinite(dec["gy"][:, sl]))
                    inter[k].append(torch.where(lost[..., None], torch.full_like(aux["samples"][k], float("nan")), aux["samples"][k]))
            if parts:
                for key, dim in (("weight", 1), ("livef", 1), ("count", 0)):
                    per_point[key].append(aux[key])
    vf = max(1.0, (V - 1) / 16.0)
    vals, scales = [torch.cat(v) for v in vals], [torch.cat(s) * vf for s in scales]
    if not parts:
        return vals, scales
    return vals, scales, dict(inter=[torch.cat(v, 1) for v in inter], inter_scale=[torch.cat(v, 1) for v in inter_scale],
                              weight=torch.cat(per_point["weight"], 1), livef=torch.cat(per_point["livef"], 1),
                              count=torch.cat(per_point["count"]))


_LAST = {}


def field64_shared(obs, pts, H, W, mu, maps, rows=None):
    """field64(...) that keeps the first map's value and scale of the latest call and reuses them when the next call has the
    same views, points, rows and first map: a case with thin companions beside a wide map follows the case it was derived
    from (field_cases.ordered_names), and the wide map's reference is nearly all of the time.  A map's value and scale do
    not depend on the other maps of the call."""
    rows = torch.arange(pts.shape[0]) if rows is None else torch.as_tensor(rows)
    key = [obs["depth"], obs["K"], obs["pose"], pts, rows, maps[0]]
    hit = _LAST.get("first")
    if hit is not None and hit[0] == (H, W, mu) and all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(hit[1], key)):
        vals, scales = field64(obs, pts, H, W, mu, maps[1:], rows=rows)
        return [hit[2]] + vals, [hit[3]] + scales
    vals, scales = field64(obs, pts, H, W, mu, maps, rows=rows)
    _LAST["first"] = ((H, W, mu), [t.detach().cpu().clone() for t in key], vals[0], scales[0])
    return vals, scales


def weight_sum_entries(obs, pts, H, W, mu, m, rows=None):
    """Where a one-hot map m makes the sampling position drop out: an entry (point, channel) whose texel is the same 0 or 1
    at all four (in-bounds) corners of every valid view of the point.  The bilinear weights sum to 1, so the fused value is
    sum_v w_v / (cnt + 1e-6) over the valid views, or 0.  Returns (expect [n,C] float64, scale [n,C], ones, zeros [n,C] bool:
    the entries that must be the weight sum / exactly 0, unseen [n] bool: rows no view sees, exactly 0)."""
    pts = pts.detach().cpu()
    rows = torch.arange(pts.shape[0]) if rows is None else torch.as_tensor(rows)
    vals, scales, parts = field64(obs, pts, H, W, mu, [m], rows=rows, parts=True)
    cell = grad_ref.decisions({k: v.detach().cpu() for k, v in obs.items()}, pts[rows].float(), H, W, mu, [m])["cells"][0]
    live = parts["livef"] > 0
    V, n = live.shape
    vv = torch.arange(V)[:, None].expand(V, n)
    x0, y0 = cell["x0"], cell["y0"]
    at = ((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))
    corners = [grad_ref._gather(m.detach().cpu(), vv, y, x, inb) for (x, y), inb in zip(at, cell["inb"])]      # [V,n,C] each
    flat = torch.stack([c == corners[0] for c in corners]).all(0) & torch.stack(cell["inb"]).all(0)[..., None]
    first = torch.where(live, torch.arange(V)[:, None], torch.full((V, n), V)).amin(0).clamp(max=V - 1)        # a valid view
    texel = corners[0][first, torch.arange(n)]                                                               # [n,C]
    agree = ((flat & (corners[0] == texel[None])) | ~live[..., None]).all(0) & (parts["count"] > 0)[:, None]
    expect = texel * ((parts["weight"] * parts["livef"]).sum(0) / (parts["count"] + 1e-6))[:, None]
    return expect, scales[0], agree & (texel == 1.0), agree & (texel == 0.0), parts["count"] == 0


def check(got, f64, scale, tol=TOL):
    """(ok, worst ratio, message): the non-finite entries of got and f64 must coincide; finite ones |got - f64| <= tol *
    scale (grad_ref.check's contract and messages)."""
    return grad_ref.check(got, f64, scale, tol)
