"""Every kernel family of the fused wide-map query against the float64 reference (oracle/field_ref.py), entry by entry.

tests/test_gpu_walks.py pins the families to each other bit for bit; they share the fold of csrc/fuse_common.h, so a
mistake there would be bit-identical in all of them.  Here each family is held to |got - f64| <= TOL * scale per
(point, channel), where scale is the float32 rounding of the reference's operation sequence at that entry: rows far off
the surface (weights down to float32's subnormal range and zero), channels from 1e-4 to 1e2 with nearly cancelling
neighbours, texel lines and map borders, 1 to 9 views, 64 | 65 fp32 and 128 | 129 fp16 channels up to 1024, channel-range
views.  The plan of every query is recorded and the kernel that ran is asserted; together the cases reach every kernel a
query with a wide map can be routed to (oracle/field_cases.py: FAMILIES)."""
import pytest
import torch

from oracle import field_cases as FC
from oracle import field_ref as R

pytestmark = pytest.mark.gpu
SEEN = {}                       # kernel family -> worst ratio |got - f64| / scale over its cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def fusion_for(dev, case):
    from d3fields_amd import Fusion, _lib
    V = case["obs"]["depth"].shape[0]
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: v.to(dev) for k, v in case["obs"].items()}
    f.curr_obs_torch.update({k: m.to(dev) for k, m in case["maps"].items()})
    f.H, f.W, f.mu = case["H"], case["W"], case["mu"]
    f.reorder_points = case["reorder"]
    f.reference_rounding = case["reference_rounding"]
    for name in case["flags"]:
        f.tuning_flags |= getattr(_lib, name)
    f.record_plans = True
    return f


def query(f, case, pts):
    with torch.no_grad():
        if case["call"] == "eval":
            out = f.eval(pts, return_names=case["names"])
        else:
            out = f.batch_eval(pts, return_names=case["names"])
    plan = f.last_plan()
    kernel = plan["kernel"]
    if plan["gated_window"] and f.last_gate()[1]:
        kernel = plan["window_side"]["kernel"]                  # the device gate opened the window side
    return out, kernel


def family(kernel):
    return [k for k in FC.FAMILIES if kernel.startswith(k)][0]


def compare(case, out, tag):
    rows = FC.sample_rows(case)
    maps = [case["maps"][k] for k in case["names"]]
    vals, scales = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], maps, rows=rows)
    worst = 0.0
    for k, v, s in zip(case["names"], vals, scales):
        ok, w, msg = R.check(out[k][rows.to(out[k].device)].cpu(), v, s)
        assert ok, "%s / %s: %s" % (tag, k, msg)
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("name", list(FC.CASES))
def test_family_against_float64(dev, name):
    case = FC.CASES[name]()
    f = fusion_for(dev, case)
    out, kernel = query(f, case, case["pts"].to(dev))
    assert kernel.startswith(case["expect"]), (name, kernel, f.last_plan())
    if case["flags"] == ("TUNE_WINDOW_SIDE",):
        assert f.last_plan()["gated_window"], f.last_plan()
    torch.cuda.synchronize()
    worst = compare(case, out, name)
    fam = family(kernel)
    SEEN[fam] = max(SEEN.get(fam, 0.0), worst)


@pytest.mark.parametrize("name,points", [("direct V4 C384", True), ("rows V5 lattice", False), ("window cloud, cell-run side", True)])
def test_strict_path_nonfinite_texels_and_points(dev, name, points):
    """A map that becomes non-finite in place after a first query (invalidate_map_checks) and NaN / Inf query points: the
    strict path's rows against the float64 reference, non-finite entries included."""
    case = FC.CASES[name]()
    f = fusion_for(dev, case)
    query(f, case, case["pts"].to(dev))                                         # the finiteness words of the clean maps
    FC.poison(case, points=points)
    k0 = case["names"][0]
    f.curr_obs_torch[k0].copy_(case["maps"][k0].to(dev))
    f.invalidate_map_checks()
    out, kernel = query(f, case, case["pts"].to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[k0]).any()), "the NaN texel must reach some rows"
    compare(case, out, name + " (non-finite)")


def test_every_family_seen():
    """The parametrised cases above reached every kernel a wide-map query can be routed to (worst ratios per family)."""
    print("\nworst |got - f64| / scale per family (TOL %.3g):" % R.TOL)
    for k in FC.FAMILIES:
        print("  %-28s %s" % (k, "%.3g" % SEEN[k] if k in SEEN else "not run"))
    assert set(SEEN) == set(FC.FAMILIES), sorted(set(FC.FAMILIES) - set(SEEN))
