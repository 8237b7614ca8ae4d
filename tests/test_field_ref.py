"""The float64 fused-feature reference (oracle/field_ref.py) pinned on the CPU: against the reference's own outputs (the
golden scenes and the batch_eval sub-sample), the calibration of field_ref.TOL on the float32 torch port and the C oracle
over the cases of tests/test_gpu_field_ref.py (oracle/field_cases.py), and mutants of the port -- a dropped low-weight
view, a small channel off by 1e-4, a reweighted small corner, a reciprocal 64 ulp off -- that the norm-wise rel_err
accepts and field_ref.check rejects.  The thin family (masks, colours: oracle/field_cases.py THIN_CASES) has mutants of
its own: the ways a views-across-lanes gather goes wrong (test_thin_mutants_fail_the_pin lists them)."""
import numpy as np
import torch

from conftest import load_golden, rel_err
from oracle import c_oracle as O
from oracle import field_cases as FC
from oracle import field_ref as R
from oracle import grad_ref
from oracle import torch_port

SETS = ("dino_feats", "mask", "color_tensor")
SCENES = ("scene_denseK_1view", "scene_fullres_smooth", "scene_patchres_smooth", "scene_patchres_stress", "scene_wideC_9views")


def test_matches_reference_goldens():
    """Every fused set of every golden scene and of the batch_eval sub-sample, entry by entry; the fixtures hold the rows
    the bound exists for (valid, non-zero, max |entry| < 1e-5)."""
    tiny = 0
    for name in SCENES:
        g = load_golden(name)
        obs = {k: torch.from_numpy(g[k]) for k in ("depth", "K", "pose")}
        vals, scales = R.field64(obs, torch.from_numpy(g["pts"]), int(g["H"]), int(g["W"]), float(g["mu"]),
                                 [torch.from_numpy(g["in_" + k]) for k in SETS])
        for k, v, s in zip(SETS, vals, scales):
            ok, w, msg = R.check(torch.from_numpy(g[k]), v, s)
            assert ok, "%s / %s: %s" % (name, k, msg)
        rmax = torch.from_numpy(g["dino_feats"]).abs().amax(1)
        tiny += int(((rmax > 0) & (rmax < 1e-5) & torch.from_numpy(g["valid_mask"])).sum())
    assert tiny >= 100, tiny
    g = load_golden("batch_eval_130001")
    obs = {k: torch.from_numpy(g[k]) for k in ("depth", "K", "pose")}
    vals, scales = R.field64(obs, torch.from_numpy(g["pts_sub"]), int(g["H"]), int(g["W"]), float(g["mu"]),
                             [torch.from_numpy(g["in_dino_feats"]), torch.from_numpy(g["in_mask"])])
    for k, v, s in zip(("dino_feats_sub", "mask_sub"), vals, scales):
        ok, w, msg = R.check(torch.from_numpy(g[k]), v, s)
        assert ok, "batch_eval_130001 / %s: %s" % (k, msg)


def _port(case, rows):
    o = dict(case["obs"])
    o.update({k: case["maps"][k].float() for k in case["names"]})
    with torch.no_grad():
        return torch_port.field_query(o, case["pts"][rows], case["names"], case["H"], case["W"], case["mu"])


def test_float32_port_and_oracle_within_bound_and_tol_calibrated():
    """The float32 torch port and the C oracle meet |got - f64| <= TOL * scale on 2000 rows of every case (plus its
    controlled-distance rows) and on the non-finite variants; TOL is a few times their worst ratio (PORT_WORST)."""
    worst = 0.0
    shares = {}                     # case -> (share of rows the GPU test's sample leaves out, share of non-finite reference rows)
    worst_thin = 0.0                # ... over the thin maps of the thin cases (noted beside field_ref.PORT_WORST)
    print("\nworst |float32 port or C oracle - f64| / scale per case (TOL %.3g): all maps, thin maps; rows left out / non-finite:" % R.TOL)
    for name in FC.ordered_names():
        for bad in (False, True) if name == "direct V4 C384" else (False,):
            case = FC.CASES[name]()
            if bad:
                FC.poison(case)
            rows = FC.sample_rows(case, 2000)
            maps = [case["maps"][k] for k in case["names"]]
            vals, scales = R.field64_shared(case["obs"], case["pts"], case["H"], case["W"], case["mu"], maps, rows=rows)
            case_worst, thin_worst = 0.0, 0.0
            if not bad:
                N = case["pts"].shape[0]
                shares[name] = (1.0 - FC.sample_rows(case).numel() / N,
                                float(torch.stack([~torch.isfinite(v).all(1) for v in vals]).any(0).double().mean()))
            port = _port(case, rows)
            ref = O.eval_field(case["obs"]["depth"], case["obs"]["K"], case["obs"]["pose"], case["pts"][rows].numpy(),
                               [m.float().numpy() for m in maps], mu=case["mu"])
            for i, k in enumerate(case["names"]):
                for tag, got in (("port", port[k]), ("oracle", torch.from_numpy(ref["sets"][i]))):
                    ok, w, msg = R.check(got, vals[i], scales[i])
                    assert ok, "%s%s / %s / %s: %s" % (name, " (non-finite)" if bad else "", k, tag, msg)
                    case_worst = max(case_worst, w)
                    if k in FC.thin_names(case):
                        thin_worst = max(thin_worst, w)
            worst = max(worst, case_worst)
            if bad:
                assert bool(torch.isnan(vals[0]).any())
                continue
            print("  %-46s %-9.3g %-9s %.4f / %.4f" % (name, case_worst, "%.3g" % thin_worst if FC.thin_names(case) else "-", shares[name][0], shares[name][1]))
            if name in FC.THIN_CASES:
                worst_thin = max(worst_thin, thin_worst)
                # a thin case compares no smaller a share of its rows than the case it was derived from
                assert shares[name][0] <= shares[case["base"]][0] and shares[name][1] <= shares[case["base"]][1], (name, shares[name], shares[case["base"]])
    assert worst <= 1.5 * R.PORT_WORST, "port / oracle worst ratio %.3g: re-measure PORT_WORST" % worst
    # the bound is attainable for the thin family before any GPU run (the figures beside field_ref.PORT_WORST)
    print("  thin maps of the thin cases: worst %.3g" % worst_thin)
    assert 0.0 < worst_thin <= worst
    assert 2.0 * worst <= R.TOL <= 10.0 * max(worst, R.PORT_WORST), "TOL %.3g vs worst %.3g" % (R.TOL, worst)


# ---- the gap the bound closes: mutants the norm-wise check accepts ------------------------------------------------------
def _parts(case):
    """The float32 port's pieces (torch_port.field_query's op sequence): per_view [V,N,C], livef [V,N], weight [V,N]."""
    o, pts, H, W, mu = case["obs"], case["pts"], case["H"], case["W"], case["mu"]
    m = case["maps"][case["names"][0]].float()
    uv, ok, z = torch_port._pixel_coords(pts, o["pose"], o["K"])
    seen = torch_port._sample(o["depth"].unsqueeze(1), uv, H, W, "nearest")[..., 0]
    sd = seen - z
    livef = ((seen > 0.0) & ok & (sd > -mu)).float()
    weight = torch.exp(torch.clamp(mu - sd.abs(), max=0) / mu)
    per_view = torch_port._sample(m.permute(0, 3, 1, 2), uv, H, W, "bilinear")
    return per_view, livef, weight


def _fuse(per_view, livef, weight):
    count = livef.sum(0)
    fused = (per_view * livef.unsqueeze(-1) * weight.unsqueeze(-1)).sum(0) / (count.unsqueeze(-1) + 1e-6)
    fused[count == 0] = 0.0
    return fused


def test_mutants_pass_rel_err_and_fail_the_pin():
    """On off-surface points and channels of 1e-4 .. 1e2: each mutant of the float32 port is within rel_err <= 1e-5 of the
    port (the norm-wise check of tests/test_gpu_fuzz.py, test_gpu_walks.py, test_gpu_parity.py) and fails field_ref.check."""
    case = FC.CASES["direct V4 C384"]()
    m = case["maps"]["wide"]
    per_view, livef, weight = _parts(case)
    base = _fuse(per_view, livef, weight)
    vals, scales = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [m])
    f64, sc = vals[0], scales[0]
    assert R.check(base, f64, sc)[0]
    gmax = float(f64.abs().max())
    mutants = {}

    # 1. a low-weight view dropped: a row far off the surface (every entry < 1e-7 of the map's largest) seen by >= 2 views
    small_row = (f64.abs().amax(1) < 1e-7 * gmax) & (livef.sum(0) >= 2) & (f64.abs().amax(1) > 0)
    r = int(small_row.nonzero()[0])
    v = int(torch.where(livef[:, r] > 0, weight[:, r], torch.full_like(weight[:, r], 2.0)).argmin())
    lv = livef.clone()
    lv[v, r] = 0.0
    mutants["drop a low-weight view"] = _fuse(per_view, lv, weight)

    # 2. one small channel (max |entry| < 1e-2) scaled by 1 + 1e-4
    c = int((f64.abs().amax(0) < 1e-2).nonzero()[0])
    out = base.clone()
    out[:, c] *= 1.0 + 1e-4
    mutants["small channel * (1 + 1e-4)"] = out

    # 3. one corner whose bilinear weight is < 1e-3 counted twice, on a valid view of some row
    dec = grad_ref.decisions(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [m])
    cell = dec["cells"][0]
    fh, fw = m.shape[1], m.shape[2]
    tx = ((dec["gx"] + 1.0) / 2.0) * float(fw - 1) - cell["x0"]
    ty = ((dec["gy"] + 1.0) / 2.0) * float(fh - 1) - cell["y0"]
    w_nw = (1.0 - tx) * (1.0 - ty)
    pick = (livef > 0) & cell["inb"][0] & (w_nw > 0) & (w_nw < 1e-3)
    cand = pick.nonzero()
    vs, rs = cand[:, 0], cand[:, 1]
    tex = m[vs, cell["y0"][vs, rs].long(), cell["x0"][vs, rs].long()]                # [n,C]
    delta = (w_nw[vs, rs] * weight[vs, rs] / (livef.sum(0)[rs] + 1e-6))[:, None] * tex
    # the candidate the norm-wise check cannot see (every entry moves by < 1e-6 of the largest) that moves the most, per scale
    fit = torch.where(delta.abs().amax(1) < 1e-6 * gmax, (delta.abs().double() / sc[rs]).amax(1), torch.zeros(len(rs), dtype=torch.float64))
    j = int(fit.argmax())
    v, r = int(vs[j]), int(rs[j])
    pv = per_view.clone()
    pv[v, r] += w_nw[v, r] * tex[j]
    mutants["small corner weight doubled"] = _fuse(pv, livef, weight)

    # 4. the fold's reciprocal 64 ulp off: every row * (1 + 64 * 2^-24)
    mutants["reciprocal 64 ulp off"] = base * (1.0 + 64 * 2.0 ** -24)

    # the suite's norm-wise check holds an output to the float32 reference (the C oracle, bit-identical to the port here)
    for tag, got in mutants.items():
        assert rel_err(got.numpy(), base.numpy()) <= 1e-5, "%s: rel_err should accept it" % tag
        ok, w, msg = R.check(got, f64, sc)
        assert not ok, "%s: field_ref.check accepts it (worst ratio %.3g)" % (tag, w)


# ---- the thin family: the ways a views-across-lanes gather goes wrong -----------------------------------------------------------
def _thin_mutants(case):
    """name -> the float32 port with one defect of gather_map_thin (csrc/fuse_common.h) built in."""
    m = case["maps"][case["names"][0]].float()
    per_view, livef, weight = _parts(case)
    V, N, C = per_view.shape
    count = livef.sum(0)

    def fuse(term):
        fused = term.sum(0) / (count.unsqueeze(-1) + 1e-6)
        fused[count == 0] = 0.0
        return fused

    term = per_view * livef.unsqueeze(-1) * weight.unsqueeze(-1)
    out = {"port": fuse(term)}
    # 1. one view's term read from the next point's lane group: on the last, ragged group of 8 points (the last two rows where
    #    that group is a single point) view 1's terms move up by one point
    last = N - (N - 1) // 8 * 8
    lo = N - max(last, 2)
    if lo >= 0:
        t = term.clone()
        t[1, lo:] = term[1, lo:].roll(-1, 0)
        out["1 a view read from the next point's lanes"] = fuse(t)
    # 2. view V - 1 left out of the ordered sum
    t = term.clone()
    t[V - 1] = 0.0
    out["2 view V-1 dropped"] = fuse(t)
    # 3. min(g, cvec - 1) replaced by g: the last vector read past C, i.e. channel C - 1 taken from what follows the texel
    #    in memory, channel 0 of the next texel
    m2 = m.clone()
    flat = torch.cat((m.reshape(V, -1)[:, C::C], torch.zeros(V, 1)), 1)
    m2[..., C - 1] = flat.reshape(V, m.shape[1], m.shape[2])
    pv2, _, _ = _parts(dict(case, maps={case["names"][0]: m2}))
    out["3 last vector read past C"] = fuse(pv2 * livef.unsqueeze(-1) * weight.unsqueeze(-1))
    # 4. the weight of an invalid view not zeroed
    out["4 invalid view keeps its weight"] = fuse(per_view * weight.unsqueeze(-1))
    return out


def test_thin_mutants_fail_the_pin():
    """Each defect a views-in-parallel gather can have fails field_ref.check on a thin-alone case, which the unmutated
    float32 port passes (mutant -> the assert of tests/test_gpu_field_ref.py::test_family_against_float64 that catches it:
    compare()'s R.check on the case printed here):
      1 a view's term read from the next point's lane group (a shuffle past a ragged last group)
      2 view V - 1 dropped from the ordered sum (a wrong lane count per point)
      3 the last vector read past C (min(g, cvec - 1) -> g)
      4 the weight of an invalid view not zeroed (the skipped view must add +0)"""
    caught = {}
    for name in ("thin V2 C3", "thin V3 C6", "thin V4 C8", "thin V8 C16", "thin V4 C12", "thin V5 C1"):
        case = FC.CASES[name]()
        assert case["thin_form"] == "parallel"
        vals, scales = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [case["maps"]["thin"]])
        for tag, got in _thin_mutants(case).items():
            ok, w, msg = R.check(got, vals[0], scales[0])
            if tag == "port":
                assert ok, "%s: %s" % (name, msg)
            elif not ok:
                caught.setdefault(tag, []).append("%s (%.3g)" % (name, w))
    print("\nthin mutants -> the cases that catch them (worst ratio):")
    for tag in ("1 a view read from the next point's lanes", "2 view V-1 dropped", "3 last vector read past C", "4 invalid view keeps its weight"):
        print("  %-44s %s" % (tag, ", ".join(caught.get(tag, [])) or "NOT CAUGHT"))
        assert caught.get(tag), "%s: no thin-alone case fails field_ref.check" % tag


def test_onehot_weight_sum_is_attainable():
    """Where a one-hot mask is flat over the corners of every valid view, the float32 port is within the bound of
    sum_v w_v / (cnt + 1e-6) and exactly 0 elsewhere (what tests/test_gpu_field_ref.py::test_onehot_mask_is_the_weight_sum
    asks of the kernels); the float64 per-view samples of a map with non-finite texels and points match the port's."""
    case = FC.CASES["thin V4 C8 one-hot, batch_eval"]()
    m = case["maps"]["thin"]
    got = _port(case, torch.arange(case["pts"].shape[0]))["thin"]
    expect, scale, ones, zeros, unseen = R.weight_sum_entries(case["obs"], case["pts"], case["H"], case["W"], case["mu"], m)
    assert int(ones.sum()) >= 100 and int(zeros.sum()) >= 1000 and int(unseen.sum()) >= 10, (int(ones.sum()), int(zeros.sum()), int(unseen.sum()))
    ok, w, msg = R.check(got[ones], expect[ones], scale[ones])
    print("\none-hot: %d entries are the weight sum (worst ratio %.3g), %d exactly 0, %d unseen rows" % (int(ones.sum()), w, int(zeros.sum()), int(unseen.sum())))
    assert ok, msg
    assert bool((got[zeros] == 0.0).all()) and bool((got[unseen] == 0.0).all())
    # '<k>_inter': the per-view samples
    case = FC.poison(FC.CASES["thin V4 C8"](), name="thin")
    m = case["maps"]["thin"]
    o = dict(case["obs"], thin=m)
    with torch.no_grad():
        port = torch_port.field_query(o, case["pts"], ["thin"], case["H"], case["W"], case["mu"], keep_inter=True)
    vals, scales, parts = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [m], parts=True)
    ok, w, msg = R.check(port["thin_inter"], parts["inter"][0], parts["inter_scale"][0])
    print("per-view samples of the poisoned thin map: worst ratio %.3g" % w)
    assert ok, msg
    assert bool(torch.isnan(parts["inter"][0]).any())
