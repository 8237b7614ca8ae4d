"""Every kernel family of the fused wide-map query against the float64 reference (oracle/field_ref.py), entry by entry.

tests/test_gpu_walks.py pins the families to each other bit for bit; they share the fold of csrc/fuse_common.h, so a
mistake there would be bit-identical in all of them.  Here each family is held to |got - f64| <= TOL * scale per
(point, channel), where scale is the float32 rounding of the reference's operation sequence at that entry: rows far off
the surface (weights down to float32's subnormal range and zero), channels from 1e-4 to 1e2 with nearly cancelling
neighbours, texel lines and map borders, 1 to 9 views, 64 | 65 fp32 and 128 | 129 fp16 channels up to 1024, channel-range
views.  The plan of every query is recorded and the kernel that ran is asserted; together the cases reach every kernel a
query with a wide map can be routed to (oracle/field_cases.py: FAMILIES).

The thin family (<= 256 bytes per texel: the instance mask, colours, fp16 maps of up to 128 channels) keeps the reference's
operation order and has code of its own (csrc/fuse_common.h: gather_map_thin spreads the views across lanes and rebuilds the
ordered sum with shuffles; gather_map_u's one-vector-per-lane form carries thin maps along in the window, register-rows,
channel-sliced and cell-run kernels).  oracle/field_cases.py THIN_CASES holds it to the same bound: alone in the
views-in-parallel form (vector widths 4 / 2 / 1 on 1 / 2 / 4 lanes per point, 2 to 8 views, ragged last groups, N = 1 and 17,
map edges), alone outside that form, and beside a wide map once per big-batch family.  The recorded lane mapping is checked
against thin_map()'s condition, so a planner change cannot move the cases to another gather unnoticed.  What catches what
(the mutants of tests/test_field_ref.py::test_thin_mutants_fail_the_pin, each failing R.check on thin-alone cases):
  a view's term shuffled in from the next point's lanes, view V-1 left out of the sum, the last vector read past C, an
  invalid view keeping its weight    -> compare() in test_family_against_float64
  a gather that moves to another form -> the lane-mapping assert of test_family_against_float64, test_every_family_seen
  a mis-weighted or mis-normalised mask where the sampling position must not matter -> test_onehot_mask_is_the_weight_sum"""
import pytest
import torch

from oracle import field_cases as FC
from oracle import field_ref as R

pytestmark = pytest.mark.gpu
SEEN = {}                       # kernel family -> worst ratio |got - f64| / scale over its cases
THIN_SEEN = {}                  # kernel family -> worst ratio over the thin maps of its cases
BESIDE_SEEN = set()             # the cases (by the case they were derived from) seen with a thin map beside the wide one
BESIDE_FAMILIES = set()         # ... and their kernel families
FORMS_SEEN = {"parallel": 0, "outside": 0}     # thin maps per gather form (the lane-mapping assert)
SHARES = {}                     # case -> (share of rows left out of the comparison, share of rows with a non-finite reference)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def upload(m, dev):
    """m on the device with its layout: a channel-range view stays a view of the wider tensor (Tensor.to would compact it)."""
    if m.is_contiguous():
        return m.to(dev)
    return m._base.to(dev).as_strided(m.shape, m.stride(), m.storage_offset())


def fusion_for(dev, case):
    from d3fields_amd import Fusion, _lib
    V = case["obs"]["depth"].shape[0]
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: v.to(dev) for k, v in case["obs"].items()}
    f.curr_obs_torch.update({k: upload(m, dev) for k, m in case["maps"].items()})
    for k, m in case["maps"].items():
        assert f.curr_obs_torch[k].stride() == m.stride() and f.curr_obs_torch[k].storage_offset() == m.storage_offset(), k
    f.H, f.W, f.mu = case["H"], case["W"], case["mu"]
    f.reorder_points = case["reorder"]
    f.reference_rounding = case["reference_rounding"]
    for name in case["flags"]:
        f.tuning_flags |= getattr(_lib, name)
    f.record_plans = True
    return f


def query(f, case, pts, inter=False):
    with torch.no_grad():
        if case["call"] == "eval":
            out = f.eval(pts, return_names=case["names"], return_inter=inter)
        else:
            out = f.batch_eval(pts, return_names=case["names"])
    plan = f.last_plan()
    kernel = plan["kernel"]
    if plan["gated_window"] and f.last_gate()[1]:
        kernel = plan["window_side"]["kernel"]                  # the device gate opened the window side
    return out, kernel


def family(kernel):
    return [k for k in FC.FAMILIES if kernel.startswith(k)][0]


def compare(case, out, tag, inter=False):
    """(worst ratio over the queried maps, worst ratio over the thin ones); inter: the '<k>_inter' rows too, against the
    per-view float64 samples."""
    rows = FC.sample_rows(case)
    maps = [case["maps"][k] for k in case["names"]]
    if inter:
        vals, scales, parts = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], maps, rows=rows, parts=True)
    else:
        vals, scales = R.field64_shared(case["obs"], case["pts"], case["H"], case["W"], case["mu"], maps, rows=rows)
    worst, thin_worst = 0.0, 0.0
    thin = FC.thin_names(case)
    for i, (k, v, s) in enumerate(zip(case["names"], vals, scales)):
        ok, w, msg = R.check(out[k][rows.to(out[k].device)].cpu(), v, s)
        print("%s / %s: worst |got - f64| / scale %.3g" % (tag, k, w))
        assert ok, "%s / %s: %s" % (tag, k, msg)
        worst = max(worst, w)
        if k in thin:
            thin_worst = max(thin_worst, w)
        if inter:
            ok, w, msg = R.check(out[k + "_inter"][:, rows.to(out[k].device)].cpu(), parts["inter"][i], parts["inter_scale"][i])
            print("%s / %s_inter: worst |got - f64| / scale %.3g" % (tag, k, w))
            assert ok, "%s / %s_inter: %s" % (tag, k, msg)
    lost = torch.stack([~torch.isfinite(v).all(1) for v in vals]).any(0)
    SHARES[tag] = (1.0 - rows.numel() / case["pts"].shape[0], float(lost.double().mean()))
    return worst, thin_worst


def check_lane_mapping(name, case, plan):
    """thin_map()'s condition (csrc/fuse_common.h), recomputed from the recorded lane mapping (Fusion.last_lane_mapping): the thin maps of a 'parallel'
    case are gathered with the views across lanes, those of an 'outside' case view by view."""
    for k in FC.thin_names(case):
        form = "parallel" if FC.views_in_parallel(case, k, plan) else "outside"
        assert form == case["thin_form"], (name, k, form, plan)
        FORMS_SEEN[form] += 1


@pytest.mark.parametrize("name", FC.ordered_names())
def test_family_against_float64(dev, name):
    case = FC.CASES[name]()
    f = fusion_for(dev, case)
    out, kernel = query(f, case, case["pts"].to(dev))
    assert kernel.startswith(case["expect"]), (name, kernel, f.last_plan())
    if case["flags"] == ("TUNE_WINDOW_SIDE",):
        assert f.last_plan()["gated_window"], f.last_plan()
    torch.cuda.synchronize()
    worst, thin_worst = compare(case, out, name)
    fam = family(kernel)
    SEEN[fam] = max(SEEN.get(fam, 0.0), worst)
    if name in FC.THIN_CASES:
        check_lane_mapping(name, case, f.last_lane_mapping())
        THIN_SEEN[fam] = max(THIN_SEEN.get(fam, 0.0), thin_worst)
        if len(case["names"]) > len(FC.thin_names(case)):
            BESIDE_SEEN.add(case["base"])
            BESIDE_FAMILIES.add(fam)
        # no smaller a share of the rows is compared than in the case this one was derived from
        print("%s: rows left out %.4f, non-finite reference rows %.4f (%s: %s)" % ((name,) + SHARES[name] + (case["base"], SHARES.get(case["base"]))))
        if case["base"] in SHARES:
            assert SHARES[name][0] <= SHARES[case["base"]][0] and SHARES[name][1] <= SHARES[case["base"]][1], (SHARES[name], SHARES[case["base"]])


@pytest.mark.parametrize("name,points,poisoned,inter", [
    pytest.param("direct V4 C384", True, None, False, id="direct V4 C384-True"),
    pytest.param("rows V5 lattice", False, None, False, id="rows V5 lattice-False"),
    pytest.param("window cloud, cell-run side", True, None, False, id="window cloud, cell-run side-True"),
    # the thin family: alone with the views in parallel ('<k>_inter' requested: every point strict, the per-view samples held to
    # float64 too), and riding along in the channel-sliced kernel
    pytest.param("thin V4 C8", True, "thin", True, id="thin V4 C8-True-inter"),
    pytest.param("sliced lattice + mask", False, "mask", False, id="sliced lattice + mask-False")])
def test_strict_path_nonfinite_texels_and_points(dev, name, points, poisoned, inter):
    """A map that becomes non-finite in place after a first query (invalidate_map_checks) and NaN / Inf query points: the
    strict path's rows against the float64 reference, non-finite entries included."""
    case = FC.CASES[name]()
    f = fusion_for(dev, case)
    query(f, case, case["pts"].to(dev))                                         # the finiteness words of the clean maps
    FC.poison(case, points=points, name=poisoned)
    k0 = case["names"][0] if poisoned is None else poisoned
    f.curr_obs_torch[k0].copy_(case["maps"][k0].to(dev))
    f.invalidate_map_checks()
    out, kernel = query(f, case, case["pts"].to(dev), inter=inter)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[k0]).any()), "the NaN texel must reach some rows"
    if poisoned is not None:
        check_lane_mapping(name, case, f.last_lane_mapping())
    compare(case, out, name + " (non-finite)", inter=inter)


@pytest.mark.parametrize("name", ["thin V4 C8 one-hot, batch_eval", "sliced lattice + mask"])
def test_onehot_mask_is_the_weight_sum(dev, name):
    """A one-hot mask whose channel is the same 0 or 1 at all four corners of every valid view of a point: the bilinear
    weights sum to 1, the sampling position drops out, and the fused value is  sum_v w_v / (cnt + 1e-6)  over the valid views
    -- what fl32(sum w) / fl32(cnt + 1e-6) rounds, held within the bound -- or exactly 0; a row no view sees is exactly 0."""
    case = FC.CASES[name]()
    k = FC.thin_names(case)[-1]
    m = case["maps"][k]
    assert set(m.unique().tolist()) == {0.0, 1.0}
    f = fusion_for(dev, case)
    out, kernel = query(f, case, case["pts"].to(dev))
    torch.cuda.synchronize()
    rows = FC.sample_rows(case)
    got = out[k][rows.to(dev)].cpu()
    expect, scale, ones, zeros, unseen = R.weight_sum_entries(case["obs"], case["pts"], case["H"], case["W"], case["mu"], m, rows)
    print("%s / %s: %d entries must be the weight sum, %d exactly 0, %d rows no view sees" % (name, k, int(ones.sum()), int(zeros.sum()), int(unseen.sum())))
    assert int(ones.sum()) >= 100 and int(zeros.sum()) >= 1000 and int(unseen.sum()) >= 10
    ok, w, msg = R.check(got[ones], expect[ones], scale[ones])
    print("%s / %s: worst |got - sum w / (cnt + 1e-6)| / scale %.3g" % (name, k, w))
    assert ok, msg
    assert bool((got[zeros] == 0.0).all()), "a channel that is 0 at every corner of every valid view"
    assert bool((got[unseen] == 0.0).all()), "a row no view sees"


def test_every_family_seen():
    """The parametrised cases above reached every kernel a wide-map query can be routed to (worst ratios per family, and of
    the thin maps' entries per family); every big-batch family, lattice and cloud, was seen with a thin map beside the wide
    one, and thin maps were gathered in both forms."""
    print("\nworst |got - f64| / scale per family (TOL %.3g), all entries / thin maps' entries:" % R.TOL)
    for k in FC.FAMILIES:
        print("  %-28s %-10s %s%s" % (k, "%.3g" % SEEN[k] if k in SEEN else "not run", "%.3g" % THIN_SEEN[k] if k in THIN_SEEN else "no thin map",
                                      "  (beside a wide map)" if k in BESIDE_FAMILIES else ""))
    print("  thin maps gathered with the views in parallel: %d, view by view: %d" % (FORMS_SEEN["parallel"], FORMS_SEEN["outside"]))
    assert set(SEEN) == set(FC.FAMILIES), sorted(set(FC.FAMILIES) - set(SEEN))
    assert set(FC.BESIDE_BASES) <= BESIDE_SEEN, sorted(set(FC.BESIDE_BASES) - BESIDE_SEEN)
    assert FORMS_SEEN["parallel"] > 0 and FORMS_SEEN["outside"] > 0, FORMS_SEEN
