"""The case table of tests/test_gpu_dirty_buffers.py: entry point -> a case that reaches it with every region of its workspace live.

A Case makes two inputs of the same shapes (A: the one that is compared; B: another problem, whose leftovers a replay run finds in
every buffer), runs a public wrapper -- or the C ABI through d3fields_amd._lib where no wrapper reaches the entry point or a capacity has
to be chosen -- on the device, and returns the DEFINED part of every output as a dict of tensors.  `check`, where a case has one,
compares the result of input A with the reference of the feature's own case module (the comparison the feature's GPU test applies).
Every buffer a case hands to an entry point comes from torch.empty, so that tests/dirty_buffers.py decides what it holds.

CASES maps every exported `int d3f_*` function with a non-const pointer parameter to its case (several entry points share a case when
one wrapper calls them in a row); EXEMPT names the others with a reason.  tests/test_dirty_cases_host.py holds the header to this.

Shapes follow DESIGN.md section 27: the smallest at which every region of the entry point's workspace layout is non-empty and every
launch of the call runs (a scan of more than 2048 ragged counters has two levels, 65 537 members fold in three levels, 2500 points are
three FPS workgroups, an image of more than 65 536 pixels takes the strided prefix loop, ...).  The `large` cases compare the fills
with each other only.
"""
import ctypes
import functools
import math

import numpy as np
import torch

DEV = "cuda:0"


class Case:
    def __init__(self, name, inputs, run, check=None, large=False, loose=None, undefined=None, min_replayed=0.4):
        self.name, self.inputs, self.run, self.check, self.large = name, inputs, run, check, large
        self.min_replayed = min_replayed        # the share of the buffers of A's replay run that must come from the run of B (some shapes depend on the data)
        self.loose = dict(loose or {})          # output key -> (rel, the sentence that allows it): |a - b| <= rel * max(1, |a|) instead of equal bytes
        self.undefined = undefined              # the header text that lets a part of an output stay out of the comparison, or None

    def __repr__(self):
        return "Case(%s)" % self.name


CASES = {}          # entry point -> Case
ALL = []            # every case once, in the order of this file (the large ones and the capacity runs of shared entry points included)
EXEMPT = {
    "d3f_eval_plan_query": "writes host memory only (the plan struct)",
    "d3f_eval_plan_query_lattice": "writes host memory only (the plan struct)",
    "d3f_track_step": "its scratch is documented must-be-zero and its waves wait on one another: not part of this work",
    "d3f_track_run": "its scratch is documented must-be-zero and its waves wait on one another: not part of this work",
}


def case(name, entry_points, **kw):
    def deco(fn):
        c = Case(name, fn.inputs, fn, **kw)
        ALL.append(c)
        for e in entry_points:
            assert e not in CASES, e
            CASES[e] = c
        return fn
    return deco


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device(DEV)


def T(a, dtype=None):
    """a device copy of a NumPy array (the case arrays are read-only)"""
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev())


def lib():
    from d3fields_amd import _lib
    return _lib


def stream():
    return lib().current_stream_handle(dev())


def tensors_of(obj, prefix=""):
    """every tensor an object or dict holds, by name (private attributes and the library handle left out)"""
    items = obj.items() if isinstance(obj, dict) else vars(obj).items()
    out = {}
    for k, v in items:
        if isinstance(v, torch.Tensor) and not str(k).startswith("_"):
            out[prefix + str(k)] = v
    return out


def plain_field(shape, step=1.0, origin=(0.0, 0.0, 0.0)):
    """a field that only lends its grid to the site-volume entry points (clearance, components, travel, ...)"""
    from d3fields_amd import BakedField
    return BakedField.from_arrays(origin, step, torch.zeros(shape, dtype=torch.float32, device=dev()))


def with_inputs(fn):
    def deco(run):
        run.inputs = functools.lru_cache(maxsize=None)(fn)
        return run
    return deco


def random_sites(shape, density, seed):
    s = np.random.default_rng(seed).random(shape) < density
    s.setflags(write=False)
    return s


# ---- the exact distance transform ---------------------------------------------------------------------------------------------------
def _edt_inputs():
    import edt_cases as EC
    a = EC.site_volume("65x3x67")
    return {"site": a}, {"site": random_sites(a.shape, 0.02, 77)}


def _edt_check(inp, out):
    import edt_cases as EC
    from test_gpu_edt import same_bits
    site = inp["site"]
    true = EC.edt_ref(site)
    assert np.array_equal(out["d2"].cpu().numpy(), true)
    EC.check_nearest(site, true, out["nearest_voxel"].cpu().numpy(), 0)
    assert same_bits(out["dist"].cpu().numpy(), EC.dist_ref(true, 0.5))
    capped = EC.edt_ref(site, 5)
    assert np.array_equal(out["cap_d2"].cpu().numpy(), capped)
    EC.check_nearest(site, true, out["cap_nearest_voxel"].cpu().numpy(), 5)


@case("edt", ["d3f_volume_edt"], check=_edt_check)
@with_inputs(_edt_inputs)
def run_edt(inp):
    site = T(inp["site"] != 0)
    f = plain_field(site.shape, step=0.5)
    c = f.clearance(sites=site)
    capped = f.clearance(sites=site, max_distance=0.5 * math.sqrt(5.0) + 1e-6)
    out = {"d2": c.d2, "nearest_voxel": c.nearest_voxel, "dist": c.dist}
    out.update({"cap_d2": capped.d2, "cap_nearest_voxel": capped.nearest_voxel, "cap_dist": capped.dist})
    return out


# ---- connected components -----------------------------------------------------------------------------------------------------------
def _ccl_inputs():
    import ccl_cases as CC
    a = CC.site_volume("65x3x67 25%")           # 13 065 voxels: seven scan workgroups, the last one ragged
    return {"site": a}, {"site": random_sites(a.shape, 0.4, 5)}


def _ccl_check(inp, out):
    import ccl_cases as CC
    ref = CC.components_ref(inp["site"], 6)
    assert np.array_equal(out["labels"].cpu().numpy(), ref["label"])
    assert out["count"].tolist() == [ref["K"], ref["found"]]
    assert np.array_equal(out["stats"].cpu().numpy(), ref["stats"])
    assert np.array_equal(out["short_stats"].cpu().numpy(), ref["stats"][:ref["K"] - 1])
    kept = CC.components_ref(inp["site"], 26, min_voxels=3)
    assert np.array_equal(out["kept_labels"].cpu().numpy(), kept["label"])


def _components_abi(site, connectivity, min_voxels, capacity, links=None):
    """d3f_volume_components (with links: d3f_volume_components_linked) with a chosen stats capacity -> (labels, count, stats[:min(K, capacity)])"""
    L = lib()
    l = L.load()
    nx, ny, nz = site.shape
    s8 = site.contiguous().view(torch.uint8)
    labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev())
    count = torch.empty(2, dtype=torch.int32, device=dev())
    stats = torch.empty((max(capacity, 1), 8), dtype=torch.int32, device=dev())
    ws_bytes = int(l.d3f_volume_components_workspace_bytes(nx, ny, nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    tail = (nx, ny, nz, connectivity, min_voxels, L.ptr(labels), L.ptr(count), L.ptr(stats) if capacity > 0 else None, capacity, L.ptr(ws), ws_bytes, stream())
    if links is None:
        L.check(l.d3f_volume_components(L.ptr(s8), *tail))
    else:
        L.check(l.d3f_volume_components_linked(L.ptr(s8), L.ptr(links), *tail))
    K = int(count[0])
    return labels, count, stats[:min(K, capacity)]


@case("components", ["d3f_volume_components"], check=_ccl_check,
      undefined="out_stats: 'Rows beyond the capacity are not written and out_count still reports K'")
@with_inputs(_ccl_inputs)
def run_components(inp):
    site = T(inp["site"] != 0)
    labels, count, stats = _components_abi(site, 6, 1, site.numel())
    K = int(count[0])
    exact = _components_abi(site, 6, 1, K)                     # exactly at capacity
    short = _components_abi(site, 6, 1, K - 1)                 # one below: K - 1 rows are defined, labels and count all the same
    comp = plain_field(site.shape).components(sites=site, connectivity=26, min_voxels=3)
    return {"labels": labels, "count": count, "stats": stats, "exact_stats": exact[2], "exact_labels": exact[0], "short_labels": short[0], "short_count": short[1],
            "short_stats": short[2], "kept_labels": comp.labels, "kept_roots": comp.roots, "kept_sizes": comp.sizes, "kept_lo": comp.box_lo, "kept_hi": comp.box_hi}


# ---- links, linked components, flow ---------------------------------------------------------------------------------------------------
PARTS_SHAPE, PARTS_C = (9, 9, 33), 5                     # 2673 voxels: the linked labelling's scan has two workgroups


def _parts_inputs():
    import parts_cases as PA
    out = []
    for seed in (3, 4):
        site, rows, tau2, cos = PA.random_case(PARTS_SHAPE, PARTS_C, seed)
        out.append({"site": site, "rows": rows, "tau2": tau2 + 0.5})      # the sums are integers: a threshold half way between two of them
    return tuple(out)


def _parts_check(inp, out):
    import parts_cases as PA
    member = inp["site"] != 0
    t32 = np.float32(math.sqrt(inp["tau2"]))
    links = PA.links_ref(member, inp["rows"], PA.L2, np.float32(t32 * t32), 26)            # float32(tau)^2 in float32, as BakedField.links squares it
    assert np.array_equal(out["links"].cpu().numpy().view(np.uint16), links)
    ref = PA.components_linked_ref(member, links, 26)
    assert np.array_equal(out["labels"].cpu().numpy(), ref["label"]) and np.array_equal(out["roots"].cpu().numpy(), ref["stats"][:, 0])
    assert np.array_equal(out["sizes"].cpu().numpy(), ref["stats"][:, 1])
    assert np.array_equal(out["exact_stats"].cpu().numpy(), ref["stats"]) and np.array_equal(out["short_stats"].cpu().numpy(), ref["stats"][:ref["K"] - 1])
    assert out["short_count"].tolist() == [ref["K"], ref["found"]] and np.array_equal(out["short_labels"].cpu().numpy(), ref["label"])


@case("parts", ["d3f_volume_links", "d3f_volume_components_linked"], check=_parts_check,
      undefined="out_stats: 'Rows beyond the capacity are not written and out_count still reports K'")
@with_inputs(_parts_inputs)
def run_parts(inp):
    from d3fields_amd import BakedField
    site = T(inp["site"] != 0)
    f = BakedField.from_arrays((0.0, 0.0, 0.0), 1.0, torch.zeros(PARTS_SHAPE, dtype=torch.float32, device=dev()), feat=T(inp["rows"], np.float32))
    tau = math.sqrt(inp["tau2"])
    links = f.links("feat", rule="l2", tau=tau, sites=site, connectivity=26)
    parts = f.parts("feat", rule="l2", tau=tau, sites=site, connectivity=26)
    members = f._members(site)
    exact = _components_abi(members, 26, 1, parts.count, links=links)          # the stats rows exactly at capacity, and one below
    short = _components_abi(members, 26, 1, parts.count - 1, links=links)
    return {"links": links.view(torch.int16), "labels": parts.labels, "roots": parts.roots, "sizes": parts.sizes, "lo": parts.box_lo, "hi": parts.box_hi,
            "exact_stats": exact[2], "short_stats": short[2], "short_count": short[1], "short_labels": short[0]}


FLOW = ((5, 6, 18), 5, 2)                                # shape, channels, radius: the cases of tests/flow_cases.py


def _flow_inputs():
    import flow_cases as FC
    out = []
    for seed in (1, 2):
        ma, ra, mb, rb = FC.random_case(FLOW[0], FLOW[1], seed)
        out.append({"ma": ma, "ra": ra, "mb": mb, "rb": rb})
    return tuple(out)


def _flow_check(inp, out):
    import flow_cases as FC
    ref = FC.flow_ref(inp["ma"], inp["ra"], inp["mb"], inp["rb"], FLOW[2], float("inf"))
    assert np.array_equal(out["target"].cpu().numpy(), ref["target"])
    for k in ("cost", "axis_cost"):
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), np.asarray(ref[k], np.float32).view(np.uint32)), k


@case("flow", ["d3f_volume_flow"], check=_flow_check)
@with_inputs(_flow_inputs)
def run_flow(inp):
    from d3fields_amd import BakedField
    z = torch.zeros(FLOW[0], dtype=torch.float32, device=dev())
    a = BakedField.from_arrays((0.0, 0.0, 0.0), 1.0, z, feat=T(inp["ra"], np.float32))
    b = BakedField.from_arrays((0.0, 0.0, 0.0), 1.0, z, feat=T(inp["rb"], np.float32))
    fl = a.flow(b, "feat", radius_voxels=FLOW[2], sites=T(inp["ma"]), other_sites=T(inp["mb"]))
    return {"target": fl.target, "cost": fl.cost, "axis_cost": fl.axis_cost}


# ---- pooling and part motion: three fold levels -----------------------------------------------------------------------------------------
POOL_C = (3, 4)                                          # a scalar and a vector mean row
POOL_VOTES = 6


def _pool_inputs():
    import pool_cases as PC
    lab, K = PC.volume("three levels")                   # 65 537 -> 257 -> 2 -> 1 rows: both ping-pong row buffers are read and written
    n = lab.size
    out = []
    for seed in (0, 1):
        l = lab if seed == 0 else np.roll(lab.reshape(-1), 12345).reshape(lab.shape)
        out.append({"label": l, "K": K, "a": PC.field_rows(n, POOL_C[0], 10 + seed), "b": PC.field_rows(n, POOL_C[1], 20 + seed),
                    "v": PC.vote_rows(n, POOL_VOTES, 30 + seed), "valid": np.random.default_rng(40 + seed).random(lab.shape) < 0.97})
    return tuple(out)


def _pool_check(inp, out):
    import pool_cases as PC
    lab, K, valid = inp["label"], inp["K"], inp["valid"]
    assert np.array_equal(out["count"].cpu().numpy(), PC.counts_ref(lab, K, valid))
    assert np.array_equal(out["moments"].cpu().numpy(), PC.moments_ref(lab, K, valid))
    for k in ("a", "b"):
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), PC.pool_ref(lab, K, inp[k], valid).view(np.uint32)), k
    assert np.array_equal(out["v_votes"].cpu().numpy(), PC.votes_ref(lab, K, inp["v"], valid))


def _pool_abi(f, labels, K, capacity):
    """d3f_volume_pool with a chosen member capacity (means of 'a' and 'b', votes of 'v') -> members, count and, where defined, the rest"""
    L = lib()
    l = L.load()
    nx, ny, nz = labels.shape
    names = [("a", L.POOL_MEAN), ("b", L.POOL_MEAN), ("v", L.POOL_VOTES)]
    out = {"count": torch.empty(K, dtype=torch.int32, device=dev()), "moments": torch.empty((K, 9), dtype=torch.int64, device=dev()),
           "members": torch.empty(1, dtype=torch.int64, device=dev())}
    for k, m in names:
        out[k] = torch.empty((K, f._channels(k)), dtype=torch.float32 if m == L.POOL_MEAN else torch.int32, device=dev())
    sets = f._set_array([k for k, _ in names])
    modes = (ctypes.c_int32 * 3)(*[m for _, m in names])
    rows = (ctypes.c_void_p * 3)(*[out[k].data_ptr() for k, _ in names])
    ws_bytes = int(l.d3f_volume_pool_workspace_bytes(nx, ny, nz, K, capacity, sum(POOL_C)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev())
    valid = f.valid.contiguous().view(torch.uint8)
    L.check(l.d3f_volume_pool(L.ptr(labels), nx, ny, nz, K, L.ptr(valid), None, sets, 3, modes, capacity, L.ptr(out["members"]), L.ptr(out["count"]),
                              L.ptr(out["moments"]), rows, L.ptr(ws), ws_bytes, stream()))
    return out


@case("pool", ["d3f_volume_pool"], check=_pool_check,
      undefined="'Over capacity (out_members > member_capacity): only out_members and out_count are defined'")
@with_inputs(_pool_inputs)
def run_pool(inp):
    from d3fields_amd import BakedField
    shape = inp["label"].shape
    sets = {k: T(inp[k], np.float32).reshape(shape + (-1,)) for k in ("a", "b", "v")}
    f = BakedField.from_arrays((0.0, 0.0, 0.0), 1.0, torch.zeros(shape, dtype=torch.float32, device=dev()), valid=T(inp["valid"]), **sets)
    labels = T(inp["label"], np.int32)
    got = f.pool(labels, return_names=["a", "b"], votes=["v"], count=inp["K"])
    out = {k: got[k] for k in ("count", "moments", "a", "b", "v_votes")}
    members = int(((labels > 0) & f.valid).sum())
    exact = _pool_abi(f, labels, inp["K"], members)                 # exactly at capacity: everything is defined
    out.update({"exact_" + k: v for k, v in exact.items()})
    over = _pool_abi(f, labels, inp["K"], members - 1)              # one below: the two counts only
    out.update({"over_members": over["members"], "over_count": over["count"]})
    return out


def _motion_inputs():
    import motion_cases as MC
    return tuple({k: v for k, v in MC.tree_case(MC.TREE_LARGE, seed).items()} for seed in (5, 6))


MOTION_KW = {"fits": 3, "min_pairs": 3}


def _motion_check(inp, out):
    import motion_cases as MC
    ref = MC.motion_ref(inp["label"], inp["K"], inp["target"], offset=inp["offset"], fits=3, tau2=MC.TREE_TAU2, min_pairs=3)
    from test_gpu_motion import DTYPES
    for key in ("members", "pairs", "pose", "inliers", "rmse", "status", "fits", "residual2", "inlier", "sums"):
        have = out["exact_" + key].cpu().numpy().reshape(-1)
        want = np.asarray(ref[key], DTYPES[key]).reshape(-1)
        assert have.tobytes() == want.tobytes(), key
    for key in ("pose", "pairs", "inliers", "fits", "status"):                       # the wrapper: the same bytes
        assert out[key].cpu().numpy().tobytes() == np.asarray(ref[key], DTYPES[key]).tobytes(), key
    assert np.array_equal(out["inlier"].cpu().numpy().reshape(-1), np.asarray(ref["inlier"]).reshape(-1).astype(bool))
    over = MC.motion_ref(inp["label"], inp["K"], inp["target"], offset=inp["offset"], fits=3, tau2=MC.TREE_TAU2, min_pairs=3, capacity=int(ref["members"]) - 1)
    assert int(out["over_members"]) == int(over["members"]) and np.array_equal(out["over_pairs"].cpu().numpy(), over["pairs"])


def _motion_abi(label, K, target, offset, tau2, capacity):
    """d3f_part_motion with a chosen member capacity, as tests/test_gpu_motion.py launches it, on torch.empty buffers"""
    L = lib()
    l = L.load()
    nx, ny, nz = label.shape
    n = nx * ny * nz
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev())
    buf = {"members": E(1, torch.int64), "pairs": E(K, torch.int32), "pose": E((K, L.MOTION_POSE_DOUBLES), torch.float64), "inliers": E(K, torch.int32),
           "rmse": E(K, torch.float64), "status": E(K, torch.int32), "fits": E(K, torch.int32), "residual2": E(n, torch.float64), "inlier": E(n, torch.uint8),
           "sums": E((K, L.MOTION_SUM_DOUBLES), torch.float64)}
    ws_bytes = int(l.d3f_part_motion_workspace_bytes(nx, ny, nz, K, capacity))
    ws = E(max(ws_bytes, 8), torch.uint8)
    L.check(l.d3f_part_motion(L.ptr(label), K, nx, ny, nz, None, L.ptr(target), L.ptr(offset), None, 3, float(tau2), 3, capacity, L.ptr(buf["members"]),
                              L.ptr(buf["pairs"]), L.ptr(buf["pose"]), L.ptr(buf["inliers"]), L.ptr(buf["rmse"]), L.ptr(buf["status"]), L.ptr(buf["fits"]),
                              L.ptr(buf["residual2"]), L.ptr(buf["inlier"]), L.ptr(buf["sums"]), L.ptr(ws), ws_bytes, stream()))
    return buf


@case("motion", ["d3f_part_motion"], check=_motion_check,
      undefined="'Over capacity (out_members > member_capacity): only out_members and out_pairs are defined'")
@with_inputs(_motion_inputs)
def run_motion(inp):
    import motion_cases as MC
    from d3fields_amd.baked import Flow
    label, target, offset = T(inp["label"], np.int32), T(inp["target"], np.int32), T(inp["offset"], np.float64)
    fl = Flow((0.0, 0.0, 0.0), 1.0, target, torch.zeros(label.shape, dtype=torch.float32, device=dev()))
    fl.offset = offset                                   # the sub-voxel corrections of the case instead of those of a cost volume
    pm = fl.motions(label, count=inp["K"], tau_voxels=math.sqrt(MC.TREE_TAU2), **MOTION_KW)
    out = tensors_of(pm)
    members = int(MC.pair_mask(inp["label"], inp["K"], inp["target"], None, inp["offset"]).sum())
    exact = _motion_abi(label, inp["K"], target, offset, MC.TREE_TAU2, members)
    out.update({"exact_" + k: v for k, v in exact.items()})
    over = _motion_abi(label, inp["K"], target, offset, MC.TREE_TAU2, members - 1)
    out.update({"over_members": over["members"], "over_pairs": over["pairs"]})
    return out


# ---- travel, paths, segments, shortcuts -----------------------------------------------------------------------------------------------
TRAVEL = ("9x20x33 55%", 26, (3, 4, 5))


def _travel_inputs():
    import geodesic_cases as GC
    free, seeds, _ = GC.case(TRAVEL[0])
    free = np.asarray(free) != 0
    seeds = np.asarray(seeds).reshape(-1)
    other = random_sites(free.shape, 0.7, 8)
    starts = np.random.default_rng(3).integers(0, free.size, size=300)
    return ({"free": free, "seeds": seeds, "starts": starts}, {"free": other, "seeds": np.flatnonzero(other.reshape(-1))[:len(seeds)], "starts": starts[::-1].copy()})


def _travel_check(inp, out):
    import geodesic_cases as GC
    import segment_cases as SC
    conn, w = TRAVEL[1], TRAVEL[2]
    cost, _ = GC.travel_ref(inp["free"], inp["seeds"], conn, w)
    nxt = GC.next_ref(cost, conn, w)
    assert np.array_equal(out["cost"].cpu().numpy(), cost) and np.array_equal(out["next_voxel"].cpu().numpy(), nxt)
    assert np.array_equal(out["dist"].cpu().numpy().view(np.uint32), GC.dist_ref(cost, 1.0, w[0]).view(np.uint32))
    L = sum(inp["free"].shape)
    vox, length, reached = GC.follow_ref(nxt, inp["starts"], L)
    assert np.array_equal(out["path_voxels"].cpu().numpy(), vox) and np.array_equal(out["path_length"].cpu().numpy(), length)
    assert np.array_equal(out["path_reached"].cpu().numpy(), reached.astype(bool))
    a, b = inp["starts"][:-1].astype(np.int32), inp["starts"][1:].astype(np.int32)
    clear, last, blocked, _, _ = SC.segments_ref(inp["free"], None, a, b, True)
    assert np.array_equal(out["seg_clear"].cpu().numpy(), clear.astype(bool)) and np.array_equal(out["seg_last_voxel"].cpu().numpy(), last)
    assert np.array_equal(out["seg_blocked_voxel"].cpu().numpy(), blocked)
    oi, ov, oc = SC.shorten_rows_ref(inp["free"], vox, length, L, True)
    assert np.array_equal(out["short_index"].cpu().numpy(), oi) and np.array_equal(out["short_voxels"].cpu().numpy(), ov)
    assert np.array_equal(out["short_length"].cpu().numpy(), oc)


@case("travel", ["d3f_volume_geodesic_init", "d3f_volume_geodesic_relax", "d3f_volume_geodesic_finish", "d3f_volume_follow", "d3f_volume_segments", "d3f_path_shorten"], check=_travel_check)
@with_inputs(_travel_inputs)
def run_travel(inp):
    free = T(inp["free"])
    f = plain_field(free.shape)
    t = f.travel(T(inp["seeds"], np.int64), free=free, connectivity=TRAVEL[1], weights=TRAVEL[2])
    starts = T(inp["starts"], np.int64)
    path = t.path(starts)
    seg = t.straight(starts[:-1], starts[1:])
    short = t.shortcut(path)
    out = {"cost": t.cost, "next_voxel": t.next_voxel, "dist": t.dist}
    out.update(tensors_of(path, "path_"))
    out.update(tensors_of(seg, "seg_"))
    out.update(tensors_of(short, "short_"))
    return out


# ---- the band, and lookups in dense and banded fields ----------------------------------------------------------------------------------------
def _band_volume(seed):
    """a plane through a 13 x 14 x 15 lattice (2730 voxels: two scan workgroups, the second ragged), a few holes, a narrow and a wide set"""
    rng = np.random.default_rng(seed)
    shape, step, origin = (13, 14, 15), np.float32(0.004), (-0.35, 0.11, -0.2)
    normal = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    centre = (np.array(shape) - 1) / 2.0 + rng.uniform(-0.3, 0.3, 3)
    dist = (((idx - centre) @ normal) * float(step)).astype(np.float32)
    valid = rng.random(shape) > 0.01
    pts = (np.array(origin) + rng.uniform(-0.5, np.array(shape) - 0.5, size=(1003, 3)) * float(step)).astype(np.float32)
    return {"shape": shape, "step": step, "origin": np.array(origin, np.float32), "dist": dist, "valid": valid, "narrow": rng.standard_normal(shape + (3,)).astype(np.float32),
            "wide": rng.standard_normal(shape + (20,)).astype(np.float32), "pts": pts, "g_dist": rng.standard_normal(1003).astype(np.float32),
            "g_narrow": rng.standard_normal((1003, 3)).astype(np.float32), "g_wide": rng.standard_normal((1003, 20)).astype(np.float32)}


def _band_inputs():
    return _band_volume(1), _band_volume(2)


def _band_check(inp, out):
    import band_cases as BC
    m = BC.mark(inp, 2.5 * float(inp["step"]))
    assert np.array_equal(out["cell_band"].cpu().numpy() != 0, m["cell_band"]) and np.array_equal(out["slot"].cpu().numpy(), m["slot"])
    assert np.array_equal(out["band_voxels"].cpu().numpy(), m["voxels"])
    assert int(out["count_exact"]) == m["M"] == int(out["count_short"])
    assert np.array_equal(out["voxels_exact"].cpu().numpy(), m["voxels"]) and np.array_equal(out["voxels_short"].cpu().numpy(), m["voxels"][:m["M"] - 1])


def _band_mark_abi(f, band, capacity):
    L = lib()
    nx, ny, nz = f.grid_shape
    cell_band = torch.empty((nx - 1, ny - 1, nz - 1), dtype=torch.uint8, device=dev())
    slot = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev())
    count = torch.empty(1, dtype=torch.int64, device=dev())
    voxels = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev())
    ws_bytes = int(f._lib.d3f_band_workspace_bytes(nx, ny, nz))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev())
    vol = f._volume()
    L.check(f._lib.d3f_band_mark(ctypes.byref(vol), float(band), L.ptr(cell_band), L.ptr(slot), L.ptr(voxels), capacity, L.ptr(count), L.ptr(ws), ws_bytes, stream()))
    return cell_band, slot, voxels[:min(int(count), capacity)], count


@case("band", ["d3f_volume_cell_valid", "d3f_volume_sample", "d3f_volume_sample_backward", "d3f_band_mark", "d3f_band_sample", "d3f_band_sample_backward"],
      check=_band_check, undefined="voxels_out: 'nothing is written beyond the capacity'")
@with_inputs(_band_inputs)
def run_band(inp):
    from d3fields_amd import BakedField
    f = BakedField.from_arrays(inp["origin"].tolist(), float(inp["step"]), T(inp["dist"]), valid=T(inp["valid"]), narrow=T(inp["narrow"]), wide=T(inp["wide"]))
    pts = T(inp["pts"])
    grads = {"narrow": T(inp["g_narrow"]), "wide": T(inp["g_wide"])}
    out = {"cell_valid": f.cell_valid}
    out.update(tensors_of(f.eval(pts), "dense_"))
    out["dense_grad"] = f.backward(pts, grad_dist=T(inp["g_dist"]), grad_sets=grads)
    band = 2.5 * float(inp["step"])
    b = f.to_band(band)
    out.update({"cell_band": b.cell_band, "slot": b.slot, "band_voxels": b.band_voxels})
    out.update(tensors_of(b.eval(pts), "band_"))
    out["band_grad"] = b.backward(pts, grad_dist=T(inp["g_dist"]), grad_sets=grads)
    M = int(b.band_voxels.shape[0])
    exact, short = _band_mark_abi(f, band, M), _band_mark_abi(f, band, M - 1)
    out.update({"cell_band_exact": exact[0], "slot_exact": exact[1], "voxels_exact": exact[2], "count_exact": exact[3], "slot_short": short[1],
                "voxels_short": short[2], "count_short": short[3]})
    return out


# ---- peaks and locate -------------------------------------------------------------------------------------------------------------------
PEAKS_SHAPE, PEAKS_K, PEAKS_R = (9, 10, 11), 5, 2


def _peaks_inputs():
    out = []
    for seed in (12, 13):
        rng = np.random.default_rng(seed)
        out.append({"score": rng.integers(0, 4, size=PEAKS_SHAPE + (PEAKS_K,)).astype(np.float32), "mask": rng.random(PEAKS_SHAPE) < 0.8,
                    "rows": rng.standard_normal(PEAKS_SHAPE + (8,)).astype(np.float32), "desc": rng.standard_normal((3, 8)).astype(np.float32)})
    return tuple(out)


def _peaks_check(inp, out):
    import peaks_cases as PK
    score = inp["score"].reshape(-1, PEAKS_K)
    sup, count, _ = PK.peaks_ref(PEAKS_SHAPE, None, inp["mask"].astype(np.uint8), score, PEAKS_R)
    assert np.array_equal(out["count"].cpu().numpy(), count)
    voxel, value = PK.topk_ref(sup, 4)
    assert np.array_equal(out["voxel"].cpu().numpy(), voxel) and np.array_equal(out["value"].cpu().numpy().view(np.uint32), value.view(np.uint32))


@case("peaks", ["d3f_volume_peaks", "d3f_topk_smallest"], check=_peaks_check)
@with_inputs(_peaks_inputs)
def run_peaks(inp):
    from d3fields_amd import BakedField
    f = BakedField.from_arrays((0.0, 0.0, 0.0), 0.01, torch.zeros(PEAKS_SHAPE, dtype=torch.float32, device=dev()), feat=T(inp["rows"]))
    out = tensors_of(f.peaks(T(inp["score"]), radius_voxels=PEAKS_R, k=4, mask=T(inp["mask"])))
    out.update(tensors_of(f.locate(T(inp["desc"]), "feat", k=3, radius_voxels=1), "locate_"))
    return out


# ---- alignment and consensus ----------------------------------------------------------------------------------------------------------------
ALIGN = ("5x4x6", 20, 513)                               # volume, channels (the sixteen-lane sampler), points: two full workgroups and one point


def _align_inputs():
    import align_cases as AC
    kinds = [dict(special=False), dict(special=False, away=True), dict(special=True)]          # the instances of tests/test_gpu_align.py
    out = []
    for seed in (3, 4):
        cases = [AC.entry_case(ALIGN[0], ALIGN[1], ALIGN[2], seed, 0.1, variant=v, **kinds[v]) for v in range(3)]
        inp = {k: np.stack([c[k] for c in cases]) for k in ("p", "w", "targets", "dist_targets")}
        inp["pose"] = np.stack([np.concatenate([c["R"].reshape(9), c["t"]]) for c in cases]).astype(np.float32)
        inp["cases"] = cases
        inp["starts"] = AC.STARTS if seed == 3 else AC.STARTS[::-1]
        out.append(inp)
    return tuple(out)


def _align_check(inp, out):
    import align_cases as AC
    import band_cases as BC
    import volume_cases as VC
    from test_gpu_align import check_rows
    check_rows(out["rows"].cpu().numpy(), out["centroids"].cpu().numpy(), inp["cases"], None, "s0", ALIGN[1], ALIGN[1] % 4 == 0)
    s = AC.scene()
    for prefix, banded in (("fit_", False), ("bandfit_", True)):          # the asserts of test_align_converges_on_the_scene
        hist = out[prefix + "history"].cpu().numpy()
        assert out[prefix + "status"].tolist() == [AC.CONVERGED] * len(AC.STARTS)
        assert np.all(np.diff(hist, axis=1) <= 0) and np.array_equal(hist[:, -1], out[prefix + "cost"].cpu().numpy())
        assert max(AC.point_error_voxels(x) for x in out[prefix + "points"].cpu().numpy()) < 0.1
        assert out[prefix + "valid"].tolist() == [225] * len(AC.STARTS)
        mark = BC.mark(s["vol"], AC.SCENE_BAND_STEPS * VC.STEP) if banded else None
        ref = AC.align_ref(s["vol"], mark, "feat", s["p"], *AC.scene_start(*inp["starts"][1]), targets=s["targets"])
        assert np.abs(out[prefix + "points"][1].cpu().numpy() - ref["points"]).max() < 1e-3 * VC.STEP and abs(ref["cost"] - hist[1, -1]) <= 1e-6 * hist[1, 0]


@case("align", ["d3f_volume_align_centroid", "d3f_volume_align_accumulate", "d3f_volume_align_step"], check=_align_check)
@with_inputs(_align_inputs)
def run_align(inp):
    from test_gpu_align import field_of, scene_inputs
    L = lib()
    l = L.load()
    f = field_of(inp["cases"][0]["vol"], dev())
    p, w, tg, dt, pose = T(inp["p"]), T(inp["w"]), T(inp["targets"]), T(inp["dist_targets"]), T(inp["pose"])
    I, n = int(p.shape[0]), int(p.shape[1])
    cen = torch.empty((I, 3), dtype=torch.float32, device=dev())
    L.check(l.d3f_volume_align_centroid(L.ptr(p), L.ptr(w), I, n, L.ptr(cen), stream()))
    ws_bytes = int(l.d3f_volume_align_workspace_bytes(I, n))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev())
    rows = torch.empty((I, L.ALIGN_ROW_DOUBLES), dtype=torch.float64, device=dev())
    vol = f._volume()
    L.check(l.d3f_volume_align_accumulate(ctypes.byref(vol), None, f._set_array(["s0"]), L.ptr(p), L.ptr(w), L.ptr(tg), L.ptr(dt), L.ptr(pose), L.ptr(cen), None, I, n,
                                          0.75, 1.25, 0.05, L.ptr(rows), L.ptr(ws), ws_bytes, stream()))
    out = {"rows": rows, "partial": ws, "centroids": cen}
    for prefix, banded in (("fit_", False), ("bandfit_", True)):
        sf, pts, tgs, rot, trans = scene_inputs(dev(), inp["starts"], banded)
        out.update(tensors_of(sf.align(pts, "feat", tgs, rot=rot, trans=trans, iters=20), prefix))
        out.update(tensors_of(sf.normal_equations(pts, rot, trans, name="feat", targets=tgs), prefix + "ne_"))
    return out


CONSENSUS = "m17k3"


def _consensus_inputs():
    import consensus_cases as CS
    cs, params = CS.case(CONSENSUS)
    args = CS.CASES[CONSENSUS][0]
    other = CS.planted(**dict(args, seed=args["seed"] + 1))
    return ({"p": cs["p"], "c": cs["c"], "trip": cs["trip"], "cs": cs, "params": params}, {"p": other["p"], "c": other["c"], "trip": other["trip"], "cs": other, "params": params})


def _consensus_check(inp, out):
    import consensus_cases as CS
    from test_gpu_consensus import check_refit
    sc = CS.scored(CONSENSUS)
    assert out["score_pose"].cpu().numpy().tobytes() == sc["pose"].tobytes()
    assert np.array_equal(out["score_count"].cpu().numpy(), sc["count"]) and np.array_equal(out["score_assign"].cpu().numpy(), sc["assign"])
    full = CS.reference(CONSENSUS)
    ns = full["n_survivors"]
    for prefix, ref in (("", full), ("exact_", CS.reference(CONSENSUS, max_survivors=ns)), ("short_", CS.reference(CONSENSUS, max_survivors=ns - 1))):
        assert out[prefix + "stats"].tolist() == [ref["found"], ref["n_gated"], ref["n_survivors"], ref["cut"]], prefix
        assert np.array_equal(out[prefix + "hyp"].cpu().numpy(), ref["hyp"]) and np.array_equal(out[prefix + "inliers"].cpu().numpy(), ref["inliers"]), prefix
        assert np.array_equal(out[prefix + "assign"].cpu().numpy(), ref["sel_assign"]) and out[prefix + "pose"].cpu().numpy().tobytes() == ref["sel_pose"].tobytes(), prefix
    check_refit(inp["cs"], inp["params"], full, out["refit_pose"].cpu().numpy(), out["refit_rmse"].cpu().numpy(), out["refit_inliers"].cpu().numpy())
    assert np.array_equal(out["api_hypothesis"].cpu().numpy(), full["hyp"][:8].astype(np.int64))


@case("consensus", ["d3f_pose_consensus_score", "d3f_pose_consensus_select", "d3f_pose_refit"], check=_consensus_check)
@with_inputs(_consensus_inputs)
def run_consensus(inp):
    """score, select and refit through the C ABI as tests/test_gpu_consensus.py calls them, on torch.empty buffers; the select also with max_survivors
    exactly at the number of survivors and one below"""
    from d3fields_amd.consensus import consensus_poses
    L = lib()
    l = L.load()
    cs, params = inp["cs"], inp["params"]
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev())
    p, c, trip = T(cs["p"]), T(cs["c"]), T(cs["trip"])
    M, k, n_trip, H = len(cs["p"]), cs["c"].shape[1], len(cs["trip"]), params["n_poses"]
    Tn = n_trip * k ** 3
    tau2 = float(np.float32(cs["tau"]) * np.float32(cs["tau"]))
    terms = (tau2, cs["side_tol"], cs["min_side"], cs["min_sin"])
    count, pose, assign = E(Tn, torch.uint8), E((Tn, 12), torch.float32), E((Tn, M), torch.int8)
    ws_bytes = int(l.d3f_pose_consensus_workspace_bytes(M, k, n_trip, params["max_survivors"]))
    ws = E(ws_bytes, torch.uint8)
    host_trip = np.ascontiguousarray(cs["trip"], np.int32)
    L.check(l.d3f_pose_consensus_score(L.ptr(p), L.ptr(c), M, k, L.ptr(trip), host_trip.ctypes.data, n_trip, *terms, L.ptr(count), L.ptr(pose), L.ptr(assign),
                                       L.ptr(ws), ws_bytes, stream()))
    out = {"score_count": count, "score_pose": pose, "score_assign": assign}

    def select(prefix, max_survivors):
        got = {"hyp": E(H, torch.int32), "inliers": E(H, torch.int32), "assign": E((H, 64), torch.int8), "pose": E((H, 12), torch.float32), "stats": E(4, torch.int32)}
        L.check(l.d3f_pose_consensus_select(L.ptr(p), L.ptr(c), M, k, L.ptr(trip), n_trip, *terms, L.ptr(count), params["min_inliers"], params["shared"], max_survivors, H,
                                            L.ptr(got["hyp"]), L.ptr(got["inliers"]), L.ptr(got["assign"]), L.ptr(got["pose"]), L.ptr(got["stats"]), L.ptr(ws), ws_bytes,
                                            stream()))
        out.update({prefix + key: v for key, v in got.items()})
        return got

    full = select("", params["max_survivors"])
    ns = int(full["stats"][2])
    select("exact_", ns)
    select("short_", ns - 1)
    rpose, rmse, rinl = E((H, 12), torch.float32), E(H, torch.float64), E(H, torch.int32)
    L.check(l.d3f_pose_refit(L.ptr(p), L.ptr(c), M, k, L.ptr(full["assign"]), H, tau2, L.ptr(rpose), L.ptr(rmse), L.ptr(rinl), stream()))
    out.update({"refit_pose": rpose, "refit_rmse": rmse, "refit_inliers": rinl})
    out.update(tensors_of(consensus_poses(p, c, cs["tau"], n_poses=8, min_inliers=params["min_inliers"], refit=True), "api_"))
    return out


def _consensus_large_inputs():
    import consensus_cases as CS
    return tuple({k: CS.planted(M=64, k=3, seed=seed, groups=(32,))[k] for k in ("p", "c")} for seed in (20, 21))


@case("consensus large", [], large=True)
@with_inputs(_consensus_large_inputs)
def run_consensus_large(inp):
    """C(64, 3) * 27 = 1 124 928 hypotheses: 4395 words per block scan, so both scans of the select take two levels"""
    import consensus_cases as CS
    from d3fields_amd.consensus import consensus_poses
    return tensors_of(consensus_poses(T(inp["p"], np.float32), T(inp["c"], np.float32), CS.TAU, refit=True))


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
RAYS = ((("9x8x10", "sphere", "4mm", True), 1003), (("9x8x10", "plane", "4mm", True), 1003))


def _ray_inputs():
    import raycast_cases as RC
    out = []
    for key, n in RAYS:
        vol, o, d, kw, ref = RC.case(key, n)
        out.append({"o": o, "d": d, "case": (key, n)})
    return tuple(out)


def _ray_check(inp, out):
    import raycast_cases as RC
    from test_gpu_raycast import check_march
    vol, o, d, kw, ref = RC.case(*inp["case"])
    check_march(vol, o, d, kw, ref, out["t"].cpu().numpy(), out["hit"].cpu().numpy(), out["points"].cpu().numpy(), out["samples"].cpu().numpy().astype(np.int64), "dirty")
    assert np.array_equal(out["api_t"].cpu().numpy(), out["t"].cpu().numpy()) and np.array_equal(out["api_hit_mask"].cpu().numpy(), out["hit"].cpu().numpy())


@case("raycast", ["d3f_volume_raycast"], check=_ray_check)
@with_inputs(_ray_inputs)
def run_raycast(inp):
    import raycast_cases as RC
    from test_gpu_raycast import camera_for, field_of
    vol, o, d, kw, ref = RC.case(*inp["case"])
    f = field_of(vol, dev())
    t, hit, pts, cnt = f._march(T(o), T(d), None, o.shape[0], kw["march_step"], kw["t_near"], kw["t_far"], samples=True)
    out = {"t": t, "hit": hit, "points": pts, "samples": cnt}
    out.update(tensors_of(f.raycast(T(o), T(d), normals=True, **kw), "api_"))
    K, pose = camera_for(vol, 31, 41)
    out.update(tensors_of(f.render(K, pose, 31, 41, march_step=kw["march_step"]), "render_"))
    return out


# ---- the mesh ----------------------------------------------------------------------------------------------------------------------------
def _mesh_inputs():
    import mesh_ref as MR
    shape = (21, 22, 23)
    return {"vol": MR.sphere(shape).astype(np.float32)}, {"vol": MR.torus(shape).astype(np.float32)}


def _mesh_check(inp, out):
    import mesh_ref as MR
    keys, t, tris = MR.reference_mesh(inp["vol"])
    assert np.array_equal(out["keys"].cpu().numpy(), keys) and np.array_equal(out["triangles"].cpu().numpy(), tris)
    from test_gpu_mesh import _t_reference
    assert float(np.max(np.abs(out["t"].cpu().numpy().astype(np.float64) - _t_reference(inp["vol"], keys, 0.0)))) <= 2.0 ** -22
    assert out["counts"].tolist() == [len(keys), len(tris)] == out["over_counts"].tolist()


def _mesh_abi(vol, cap_v, cap_t):
    L = lib()
    l = L.load()
    nx, ny, nz = vol.shape
    keys = torch.empty(max(cap_v, 1), dtype=torch.int64, device=dev())
    t = torch.empty(max(cap_v, 1), dtype=torch.float32, device=dev())
    tris = torch.empty((max(cap_t, 1), 3), dtype=torch.int32, device=dev())
    counts = torch.empty(2, dtype=torch.int64, device=dev())
    ws_bytes = int(l.d3f_mesh_workspace_bytes(nx, ny, nz))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev())
    L.check(l.d3f_mesh_extract(L.ptr(vol), None, nx, ny, nz, 0.0, cap_v, cap_t, L.ptr(keys), L.ptr(t), L.ptr(tris), L.ptr(counts), L.ptr(ws), ws_bytes, stream()))
    return keys, t, tris, counts


@case("mesh", ["d3f_mesh_count", "d3f_mesh_extract", "d3f_volume_gaussian"], check=_mesh_check,
      undefined="'nothing is written beyond the capacities, what was written is unspecified': over capacity only counts_out is compared")
@with_inputs(_mesh_inputs)
def run_mesh(inp):
    from d3fields_amd import mesh
    vol = T(inp["vol"])
    keys, t, tris = mesh.marching_cubes(vol, vol.shape, count_first=True)           # d3f_mesh_count, then an extract exactly at capacity
    out = {"keys": keys, "t": t, "triangles": tris, "smooth": mesh.gaussian_filter(vol, vol.shape, sigma=1.5)}
    nv, nt = int(keys.shape[0]), int(tris.shape[0])
    out["counts"] = _mesh_abi(vol, nv, nt)[3]
    out["over_counts"] = _mesh_abi(vol, nv - 1, nt - 1)[3]
    return out


def _mesh_large_inputs():
    import mesh_ref as MR
    shape = (129, 130, 131)                              # 2 196 870 points > 2048 * 1024: the totals are scanned in two levels
    return {"vol": MR.sphere(shape).astype(np.float32)}, {"vol": MR.smooth_noise(shape).astype(np.float32)}


@case("mesh large", [], large=True)
@with_inputs(_mesh_large_inputs)
def run_mesh_large(inp):
    from d3fields_amd import mesh
    vol = T(inp["vol"])
    keys, t, tris = mesh.marching_cubes(vol, vol.shape)
    return {"keys": keys, "t": t, "triangles": tris}


def _band_large_inputs():
    import scale_cases as SC
    out = []
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) for s in SC.A], indexing="ij"), axis=-1)
        dist = ((idx - (np.array(SC.A, np.float32) - 1) / 2 + rng.uniform(-0.3, 0.3, 3).astype(np.float32)) @ np.array([0.3, -0.5, 0.8], np.float32)).astype(np.float32)
        out.append({"dist": dist * np.float32(0.004)})
    return tuple(out)


@case("band mark large", [], large=True)
@with_inputs(_band_large_inputs)
def run_band_large(inp):
    """d3f_band_mark on 161 x 162 x 163 voxels: the scan takes three levels"""
    from d3fields_amd import BakedField
    b = BakedField.from_arrays((0.0, 0.0, 0.0), 0.004, T(inp["dist"])).to_band(0.01)
    return {"cell_band": b.cell_band, "slot": b.slot, "band_voxels": b.band_voxels}


# ---- point clouds on the mask side ----------------------------------------------------------------------------------------------------
IMAGE = (250, 301)                                       # 75 250 pixels: 294 workgroups, so the strided prefix loop of the write kernels runs


def _view_inputs():
    import pcd_cases as PC
    a = PC.random_view_case(IMAGE, True, True)
    rng = np.random.default_rng(9)
    b = dict(a)
    b["depth"] = rng.uniform(0.2, 1.4, size=IMAGE)
    b["mask"] = (rng.random(IMAGE) < 0.5).astype(np.uint8)
    return a, b


def _view_check(inp, out):
    import pcd_cases as PC
    n = len(inp["pix"])
    assert int(out["count"]) == n == int(out["short_count"])
    assert np.array_equal(out["pix"].cpu().numpy(), inp["pix"]) and PC.same_bits(out["pts"].cpu().numpy(), inp["pts"])
    assert np.array_equal(out["short_pix"].cpu().numpy(), inp["pix"][:n - 1]) and PC.same_bits(out["short_pts"].cpu().numpy(), inp["pts"][:n - 1])


def _backproject_abi(inp, capacity):
    """d3f_backproject_view as tests/test_gpu_pcd_edges.py calls it, on torch.empty buffers"""
    L = lib()
    l = L.load()
    H, W = inp["depth"].shape
    d = T(inp["depth"], np.float64)
    m = None if inp["mask"] is None else T(inp["mask"], np.uint8)
    pts = torch.empty((max(capacity, 1), 3), dtype=torch.float64, device=dev())
    pix = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev())
    cnt = torch.empty(1, dtype=torch.int64, device=dev())
    ws = torch.empty(int(l.d3f_backproject_workspace_bytes(H, W)), dtype=torch.uint8, device=dev())
    dbl = lambda v: (ctypes.c_double * len(v))(*[float(x) for x in v])
    L.check(l.d3f_backproject_view(L.ptr(d), L.ptr(m), H, W, dbl(inp["cam"]), dbl(np.asarray(inp["T"]).reshape(-1)),
                                   dbl(inp["bounds"]) if inp["bounds"] is not None else None, capacity, L.ptr(pts), L.ptr(pix), L.ptr(cnt), L.ptr(ws), stream()))
    n = min(int(cnt), capacity)
    return pts[:n], pix[:n], cnt


@case("backproject", ["d3f_backproject_view"], check=_view_check, undefined="out_pts / out_pixel: 'count_out ... (may exceed capacity)': rows up to min(count, capacity)")
@with_inputs(_view_inputs)
def run_backproject(inp):
    from d3fields_amd import pcd_utils
    pts, pix = pcd_utils._backproject(inp["depth"], inp["mask"], inp["cam"], inp["T"], inp["bounds"], dev())
    n = int(pts.shape[0])
    exact, short = _backproject_abi(inp, n), _backproject_abi(inp, n - 1)
    return {"pts": pts, "pix": pix, "exact_pts": exact[0], "exact_pix": exact[1], "count": exact[2], "short_pts": short[0], "short_pix": short[1], "short_count": short[2]}


def _nearest_inputs():
    import pcd_cases as PC
    a = PC.sized_case(257, 513)
    rng = np.random.default_rng(2)
    return a, {"a": rng.standard_normal((257, 3)), "b": rng.standard_normal((513, 3))}


def _nearest_check(inp, out):
    import pcd_cases as PC
    assert np.array_equal(out["argmin"].cpu().numpy(), inp["argmin"]) and PC.same_bits(out["min_dist"].cpu().numpy(), inp["min_dist"])


@case("pcd nearest", ["d3f_pcd_nearest"], check=_nearest_check)
@with_inputs(_nearest_inputs)
def run_nearest(inp):
    from d3fields_amd import pcd_utils
    md, am = pcd_utils._nearest(T(inp["a"], np.float64), T(inp["b"], np.float64), dev())
    return {"min_dist": md, "argmin": am}


def _keys_inputs():
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        out.append({"a": rng.integers(-40, 300, size=3001).astype(np.int32), "b": rng.integers(100, 420, size=2500).astype(np.int32),
                    "pts": rng.uniform(-0.065, 0.065, size=(3001, 3)), "col": rng.uniform(0.0, 1.0, size=(3001, 3)),
                    "far": rng.uniform(-3.0, 3.0, size=(777, 3))})
    return tuple(out)


def _keys_check(inp, out):
    import pcd_cases as PC
    from oracle import np_pcd
    inter, union = out["iou_counts"].tolist()
    assert (inter / union, len(inp["a"]) / union, len(inp["b"]) / union) == np_pcd.vox_idx_iou(inp["a"], inp["b"])
    lower, num = np.array([-3.0, -3.0, -3.0]), np.array([120, 120, 120], np.int32)
    assert np.array_equal(out["index"].cpu().numpy(), np_pcd.pcd_to_index(inp["far"], lower, 0.05, num)) and np.array_equal(out["voxel"].cpu().numpy(), np_pcd.pcd_to_voxel(inp["far"], lower, 0.05))
    case = PC._voxel_case("dirty", inp["pts"], 0.01, inp["col"])
    assert np.unique(PC.voxel_index(inp["pts"], 0.01), axis=0, return_counts=True)[1].max() <= PC.MAX_PER_VOXEL      # what point_tol assumes
    got = out["voxel_points"].cpu().numpy()
    assert got.shape == case["want_points"].shape and np.abs(got - case["want_points"]).max() <= PC.point_tol(inp["pts"], 0.01)
    assert np.abs(out["voxel_colours"].cpu().numpy() - case["want_colours"]).max() <= PC.colour_tol(inp["col"])


def _vox_iou_abi(a, b):
    L = lib()
    l = L.load()
    ws_bytes = int(l.d3f_vox_iou_workspace_bytes(a.numel(), b.numel()))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    counts = torch.empty(2, dtype=torch.int64, device=dev())
    L.check(l.d3f_vox_idx_iou(L.ptr(a), a.numel(), L.ptr(b), b.numel(), L.ptr(counts), L.ptr(ws), ws_bytes, stream()))
    return counts


def _voxel_mean_abi(pts, col, voxel_size):
    L = lib()
    l = L.load()
    n = pts.shape[0]
    out_p = torch.empty((n, 3), dtype=torch.float64, device=dev())
    out_c = torch.empty((n, 3), dtype=torch.float64, device=dev())
    cnt = torch.empty(1, dtype=torch.int64, device=dev())
    ws_bytes = int(l.d3f_voxel_downsample_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    L.check(l.d3f_voxel_downsample(L.ptr(pts), L.ptr(col), n, float(voxel_size), L.ptr(out_p), L.ptr(out_c), L.ptr(cnt), L.ptr(ws), ws_bytes, stream()))
    v = int(cnt)
    return out_p[:v], out_c[:v], cnt


@case("voxel keys", ["d3f_vox_idx_iou", "d3f_voxel_downsample", "d3f_pcd_to_index"], check=_keys_check,
      undefined="out_pts / out_colors: '[n,3] capacity; *count_out = the number of voxels': rows up to the count")
@with_inputs(_keys_inputs)
def run_keys(inp):
    from d3fields_amd import pcd_utils
    p, c, count = _voxel_mean_abi(T(inp["pts"], np.float64), T(inp["col"], np.float64), 0.01)       # 3001 points in about 1600 voxels
    closures = pcd_utils.init_low_level_memory([-3.0, -3.0, -3.0], [3.0, 3.0, 3.0], 0.05, [120, 120, 120])
    # (the wrapper of d3f_pcd_to_index returns NumPy: the tensors are rebuilt from it)
    return {"iou_counts": _vox_iou_abi(T(inp["a"]), T(inp["b"])), "voxel_points": p, "voxel_colours": c, "voxel_count": count,
            "index": T(closures[4](inp["far"])), "voxel": T(closures[0](inp["far"]))}


def _pixel_inputs():
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:IMAGE[0], 0:IMAGE[1]]
        blob = ((yy - 120 - 10 * seed) ** 2 + (xx - 150) ** 2 < 90 ** 2) & (rng.random(IMAGE) < 0.995)
        out.append({"mask": blob.astype(np.float32), "depth": rng.uniform(0.3, 1.4, size=IMAGE).astype(np.float32), "image": (rng.random(IMAGE) < 0.3).astype(np.uint8) * 255,
                    "dets": (rng.random((5, 4001)) < 0.3).astype(np.uint8), "owner": np.array([2, -1, 0, 4, 1], np.int32)})
    return tuple(out)


def _nonzero_abi(image, capacity):
    L = lib()
    l = L.load()
    H, W = image.shape
    rc = torch.empty((max(capacity, 1), 2), dtype=torch.int32, device=dev())
    count = torch.empty(1, dtype=torch.int64, device=dev())
    ws = torch.empty(int(l.d3f_backproject_workspace_bytes(H, W)), dtype=torch.uint8, device=dev())
    L.check(l.d3f_nonzero_pixels(L.ptr(image), H, W, capacity, L.ptr(rc), L.ptr(count), L.ptr(ws), stream()))
    return rc[:min(int(count), capacity)], count


def _pixel_check(inp, out):
    rc = np.array(inp["image"].nonzero()).T.astype(np.int32)
    assert int(out["nz_count"]) == len(rc) == int(out["nz_short_count"])
    assert np.array_equal(out["nz_rc"].cpu().numpy(), rc) and np.array_equal(out["nz_short_rc"].cpu().numpy(), rc[:len(rc) - 1])
    from oracle import np_assoc, np_pcd
    instances = [{"idx": {0: int(d[0])} if len(d) else {}} for d in (np.flatnonzero(inp["owner"] == k) for k in range(int(inp["owner"].max()) + 1))]
    assert np.array_equal(out["labels"].cpu().numpy(), np_assoc.label_images(instances, [inp["dets"].reshape(5, 1, -1) != 0])[0].reshape(-1))
    pix = np.array(inp["image"].nonzero()).T[:2500]
    _, idx, maxd = np_pcd.fps_int(pix, 5, 0)
    assert out["fps_idx"].tolist() == idx and float(out["fps_maxd"]) == maxd


@case("pixels", ["d3f_mask_gate", "d3f_erode", "d3f_nonzero_pixels", "d3f_fps_pixels", "d3f_compose_labels"], check=_pixel_check,
      undefined="out_row_col: '[capacity,2]; *count_out = the number found, also when it exceeds capacity': rows up to min(count, capacity)")
@with_inputs(_pixel_inputs)
def run_pixels(inp):
    from d3fields_amd import pcd_utils
    L = lib()
    sel, sel_depth = pcd_utils.masked_pixel_fps(T(inp["mask"]), T(inp["depth"]), 6, init_idx=0)     # gate -> erode -> nonzero -> fps of ~25 000 pixels
    image = T(inp["image"])
    n = int((image != 0).sum())
    exact, short = _nonzero_abi(image, n), _nonzero_abi(image, n - 1)
    dets, owner = T(inp["dets"]), T(inp["owner"])
    labels = torch.empty(dets.shape[1], dtype=torch.uint8, device=dev())
    L.check(L.load().d3f_compose_labels(L.ptr(dets), dets.shape[0], dets.shape[1], L.ptr(owner), L.ptr(labels), stream()))
    sel_pix, sel_idx, maxd = pcd_utils.fps_pixels(np.array(inp["image"].nonzero()).T[:2500], 5, init_idx=0)
    return {"sel": T(sel), "sel_depth": T(sel_depth), "nz_rc": exact[0], "nz_count": exact[1], "nz_short_rc": short[0], "nz_short_count": short[1], "labels": labels,
            "fps_idx": T(np.array(sel_idx, np.int64)), "fps_maxd": T(np.array([maxd]))}


def _fps_inputs():
    return tuple({"pts": np.random.default_rng(seed).uniform(-1.0, 1.0, size=(2500, 3)).astype(np.float32)} for seed in (1, 2))


def _fps_check(inp, out):
    from oracle import c_oracle as O
    idx, maxd = O.fps(inp["pts"], 5, 0)                  # fps_np restated in C: float32, numpy's summation order, first maximum
    assert out["idx"].tolist() == idx.tolist()


@case("fps", ["d3f_farthest_point_sampling"], check=_fps_check)
@with_inputs(_fps_inputs)
def run_fps(inp):
    """2500 points are three workgroups with a ragged chunk; k = 5 reads both parities of the maxima buffer"""
    L = lib()
    l = L.load()
    pts = T(inp["pts"])
    n, k = pts.shape[0], 5
    idx = torch.empty(k, dtype=torch.int64, device=dev())
    maxd = torch.empty(1, dtype=torch.float32, device=dev())
    ws = torch.empty(int(l.d3f_fps_workspace_bytes(n)), dtype=torch.uint8, device=dev())
    L.check(l.d3f_farthest_point_sampling(L.ptr(pts), n, k, 0, L.ptr(idx), L.ptr(maxd), L.ptr(ws), stream()))
    return {"idx": idx, "maxdist": maxd}


# ---- the fused query -----------------------------------------------------------------------------------------------------------------------
VIEWS = (4, 96, 128)


def _scene(seed, n, clump):
    from d3fields_amd import synth
    V, H, W = VIEWS
    sc = synth.make_scene(V, H, W, "smooth")
    pts = synth.random_cloud(n, seed=seed)
    if clump:                                            # more than 256 points in one counting cell: the rank runs in aligned pieces
        pts[:600] = pts[0] + 1e-5 * torch.randn(600, 3, generator=torch.Generator().manual_seed(seed))
    return {"depth": sc["depth"], "K": sc["K"], "pose": sc["pose"], "feats": synth.random_map(V, H // 8, W // 8, 48, seed=seed), "mask": synth.random_onehot_mask(V, H, W, 8, seed=seed + 1),
            "pts": pts}


def _fusion(inp):
    from d3fields_amd import Fusion
    f = Fusion(num_cam=VIEWS[0], device=DEV)
    d = dev()
    f.curr_obs_torch = {"depth": inp["depth"].to(d), "K": inp["K"].to(d), "pose": inp["pose"].to(d), "dino_feats": inp["feats"].to(d), "mask": inp["mask"].to(d)}
    f.H, f.W = VIEWS[1], VIEWS[2]
    f.cache_point_order = False
    f.async_probes = False
    return f


def _eval_check(inp, out):
    from oracle import c_oracle as O
    ref = O.eval_field(inp["depth"], inp["K"], inp["pose"], inp["pts"], [inp["feats"], inp["mask"]], mu=0.02)
    assert np.array_equal(out["valid_mask"].cpu().numpy(), ref["valid_mask"]) and np.array_equal(out["dist"].cpu().numpy(), ref["dist"])
    for k, r in (("dino_feats", ref["sets"][0]), ("mask", ref["sets"][1])):
        err = np.abs(out[k].cpu().numpy() - r).max() / max(np.abs(r).max(), 1.0)
        assert err <= 1e-5, (k, err)                     # the bound of smoke() and of tests/test_gpu_parity.py


@case("eval ordered", ["d3f_eval", "d3f_map_check_many", "d3f_points_probe"], check=_eval_check)
@with_inputs(lambda: (_scene(3, 70001, True), _scene(4, 70001, True)))
def run_eval(inp):
    """70 001 points >= the 65 536 from which the wrapper hands over scratch; TUNE_FORCE_REORDER and no cached order: the count table, the
    status words of the single-launch scan, the partial boxes, keys, ranks, slots and the order are all written and read in this call"""
    f = _fusion(inp)
    f.tuning_flags = lib().TUNE_FORCE_REORDER
    f.detect_lattice = False
    with torch.no_grad():
        out = dict(f.eval(inp["pts"].to(dev())))
    L = lib()
    probe = torch.empty(L.PROBE_WORDS, dtype=torch.int32, device=dev())
    p = inp["pts"].to(dev()).contiguous()
    L.check(L.load().d3f_points_probe(L.ptr(p), p.shape[0], L.ptr(probe), stream()))
    out["probe"] = probe                                 # 'every one of the D3F_PROBE_WORDS device words of `out` is written by the call'
    return out


def _lattice_scene(seed):
    from d3fields_amd import create_init_grid
    s = _scene(seed, 10, False)
    b = {"x_lower": -0.22, "x_upper": 0.22, "y_lower": -0.22, "y_upper": 0.22, "z_lower": 0.0 + 0.001 * seed, "z_upper": 0.18 + 0.001 * seed}
    s["pts"], s["shape"] = create_init_grid(b, 0.004)    # 110 x 110 x 45 = 544 500 points: 2127 blocks of 256, so the shell's scan has two levels, the last block ragged
    assert s["pts"].shape[0] > 2048 * 256 and s["pts"].shape[0] % 256 != 0
    s["bounds"] = b
    return s


def _oracle(inp):
    """the CPU oracle's answer for the lattice, computed once per input"""
    if "_ref" not in inp:
        from oracle import c_oracle as O
        inp["_ref"] = O.eval_field(inp["depth"], inp["K"], inp["pose"], inp["pts"], [inp["feats"], inp["mask"]], mu=0.02)
        inp["_ref_dist"] = O.eval_field(inp["depth"], inp["K"], inp["pose"], inp["pts"][:5003], [], mu=0.02, mode="eval_dist")
    return inp["_ref"], inp["_ref_dist"]


def _close(got, want):
    """the bound of smoke() and tests/test_gpu_parity.py"""
    return np.abs(got.cpu().numpy() - want).max() / max(np.abs(want).max(), 1.0) <= 1e-5


def _lattice_check(inp, out):
    ref, ref_d = _oracle(inp)
    valid = ref["valid_mask"].astype(bool)
    for prefix in ("lattice_", "grid_"):
        assert np.array_equal(out[prefix + "valid_mask"].cpu().numpy().reshape(-1), valid) and np.array_equal(out[prefix + "dist"].cpu().numpy().reshape(-1), ref["dist"]), prefix
        assert _close(out[prefix + "mask"].reshape(-1, 8), ref["sets"][1]), prefix
    assert _close(out["lattice_dino_feats"], ref["sets"][0])
    assert np.array_equal(out["dist_valid_mask"].cpu().numpy(), ref_d["valid_mask"].astype(bool)) and np.array_equal(out["dist_dist"].cpu().numpy(), ref_d["dist"], equal_nan=True)
    want = np.flatnonzero(valid & (np.abs(ref["dist"]) < np.float32(0.005)))            # fusion.py:1430, 1444, as tests/test_gpu_dist.py takes it
    assert np.array_equal(out["shell_idx"].cpu().numpy(), want) and np.array_equal(out["shell_pts"].cpu().numpy(), inp["pts"].numpy()[want])
    assert out["lattice_dims"].tolist() == [int(x) for x in inp["shape"]] + [0]
    near, far = out["locality"].tolist()
    assert 0 < near < 0.25 * far                                                        # a lattice is local: the rule of Fusion._parse_probe


@case("eval lattice", ["d3f_eval_lattice", "d3f_eval_grid", "d3f_grid_shell", "d3f_eval_dist", "d3f_lattice_probe", "d3f_point_order_locality"], check=_lattice_check)
@with_inputs(lambda: (_lattice_scene(1), _lattice_scene(2)))
def run_lattice(inp):
    L = lib()
    f = _fusion(inp)
    pts = inp["pts"].to(dev())
    with torch.no_grad():
        out = tensors_of(f.eval(pts), "lattice_")
        out.update(tensors_of(f.eval_grid(inp["bounds"], 0.004, ["mask"]), "grid_"))
        out.update(tensors_of(f.eval_dist(pts[:5003]), "dist_"))
        idx, shell = f.grid_shell(inp["bounds"], 0.004)
    out.update({"shell_idx": idx, "shell_pts": shell})
    dims = torch.empty(4, dtype=torch.int32, device=dev())
    dims[3] = 0                                          # 'the caller zeroes out_dims[3] before the call'
    L.check(L.load().d3f_lattice_probe(L.ptr(pts), pts.shape[0], L.ptr(dims), stream()))
    loc = torch.empty(2, dtype=torch.float32, device=dev())
    L.check(L.load().d3f_point_order_locality(L.ptr(pts), pts.shape[0], L.ptr(loc), stream()))
    out.update({"lattice_dims": dims, "locality": loc})
    return out


def _shell_abi(f, bounds, step, capacity):
    """d3f_grid_shell with a chosen capacity (and, for an empty grid, no point at all: the count is the call's own zero)"""
    L = lib()
    grid, axes = f._grid(bounds, step)
    views, keep, V = f._views(dev())
    n = grid.nx * grid.ny * grid.nz
    count = torch.empty(1, dtype=torch.int64, device=dev())
    idx = torch.empty(max(capacity, 1), dtype=torch.int64, device=dev())
    ws_bytes = int(f._lib.d3f_grid_shell_workspace_bytes(ctypes.byref(grid)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev())
    L.check(f._lib.d3f_grid_shell(ctypes.byref(views), ctypes.byref(grid), f.mu, 0.005, capacity, L.ptr(idx), L.ptr(count), L.ptr(ws), ws_bytes, stream()))
    return idx[:min(int(count), capacity)], count


def _shell_check(inp, out):
    ref, _ = _oracle(inp)
    want = np.flatnonzero(ref["valid_mask"].astype(bool) & (np.abs(ref["dist"]) < np.float32(0.005)))
    assert int(out["exact_count"]) == len(want) == int(out["short_count"]) and int(out["empty_count"]) == 0
    assert np.array_equal(out["exact_idx"].cpu().numpy(), want) and np.array_equal(out["short_idx"].cpu().numpy(), want[:len(want) - 1])


@case("grid shell capacity", [], check=_shell_check, undefined="idx_out: 'may exceed capacity: then only the first `capacity` indices were stored'")
@with_inputs(lambda: (_lattice_scene(1), _lattice_scene(2)))
def run_shell(inp):
    f = _fusion(inp)
    with torch.no_grad():
        idx, _ = f.grid_shell(inp["bounds"], 0.004)
    n = int(idx.shape[0])
    exact, short = _shell_abi(f, inp["bounds"], 0.004, n), _shell_abi(f, inp["bounds"], 0.004, max(n - 1, 0))
    empty = dict(inp["bounds"], x_upper=inp["bounds"]["x_lower"])                  # no grid point: only the call's own clear writes the count
    none = _shell_abi(f, empty, 0.004, 16)
    return {"idx": idx, "exact_idx": exact[0], "exact_count": exact[1], "short_idx": short[0], "short_count": short[1], "empty_count": none[1]}


def _shell_large_inputs():
    out = []
    for seed in (1, 2):
        s = _scene(seed, 10, False)
        s["bounds"] = {"x_lower": -0.21, "x_upper": 0.21, "y_lower": -0.21, "y_upper": 0.21, "z_lower": 0.001 * seed, "z_upper": 0.375 + 0.001 * seed}
        out.append(s)
    return tuple(out)


@case("grid shell tiled", [], large=True)
@with_inputs(_shell_large_inputs)
def run_shell_large(inp):
    """168 x 168 x 150 = 4 233 600 grid points >= 2^22: the depth lookups of the shell go to the tiled copy in the scratch behind the workspace proper"""
    f = _fusion(inp)
    with torch.no_grad():
        idx, pts = f.grid_shell(inp["bounds"], 0.0025)
    assert idx.shape[0] > 0
    return {"idx": idx, "pts": pts}


GRAD = (4, 48, 64, 5003, 48)                              # views, H, W, points, channels: the shapes of tests/test_gpu_grad.py


def _grad_inputs():
    from d3fields_amd import synth
    out = []
    for seed in (5, 6):
        V, H, W, N, C = GRAD
        obs = synth.make_scene(V, H, W, "stress")
        g = torch.Generator().manual_seed(seed)
        out.append({"obs": obs, "depth": obs["depth"], "K": obs["K"], "pose": obs["pose"], "pts": synth.random_cloud(N, seed=seed), "feats": synth.random_map(V, 12, 16, C, seed=seed),
                    "mask": synth.random_onehot_mask(V, H, W, 8, seed=seed + 1), "gd": torch.randn(N, generator=g), "gk": torch.randn(N, C, generator=g),
                    "head": torch.linspace(-1.0, 1.0, 3 * C).reshape(3, C) * (1.0 + 0.1 * seed)})
    return tuple(out)


def _grad_check(inp, out):
    from oracle import c_oracle as O
    from test_gpu_grad import compare
    V, H, W, N, C = GRAD
    compare(out["grad"].cpu(), inp["obs"], inp["pts"], H, W, 0.02, [inp["feats"]], inp["gd"], [inp["gk"]], "eval")
    compare(out["grad_dist"].cpu(), inp["obs"], inp["pts"], H, W, 0.02, [], inp["gd"], [], "eval_dist")
    ref = O.eval_field(inp["depth"], inp["K"], inp["pose"], inp["pts"], [inp["feats"], inp["mask"]], mu=0.02)
    assert _close(out["feats"], ref["sets"][0])
    want = ref["sets"][0].astype(np.float64) @ inp["head"].numpy().astype(np.float64).T
    import projection_cases as PJ
    A = np.abs(ref["sets"][0]).astype(np.float64) @ np.abs(inp["head"].numpy()).astype(np.float64).T
    query = 1e-5 * max(np.abs(ref["sets"][0]).max(), 1.0) * np.abs(inp["head"].numpy()).astype(np.float64).sum(1)      # the query's own bound (_close), through the head
    assert np.all(np.abs(out["projected"].cpu().numpy() - want) <= PJ.rounding_cap(C, V) * A + query)
    inst = O.onehot2instance(ref["sets"][1])
    assert np.array_equal(out["instance"].cpu().numpy(), inst) and np.array_equal(out["onehot"].cpu().numpy(), O.instance2onehot(inst, 8).astype(bool))
    assert int(out["finite_word"]) == 0


@case("eval backward", ["d3f_eval_backward", "d3f_eval_dist_backward", "d3f_map_check", "d3f_project_maps", "d3f_onehot2instance", "d3f_instance2onehot"], check=_grad_check)
@with_inputs(_grad_inputs)
def run_backward(inp):
    from d3fields_amd import onehot2instance, instance2onehot
    from test_gpu_grad import fusion, kernel_grad
    V, H, W, N, C = GRAD
    f = fusion(dev(), inp["obs"], {"dino_feats": inp["feats"], "mask": inp["mask"]}, H, W)
    res = {"grad": kernel_grad(f, inp["pts"], ["dino_feats"], inp["gd"], [inp["gk"]], "eval").to(dev()),
           "grad_dist": kernel_grad(f, inp["pts"], [], inp["gd"], [], "eval_dist").to(dev())}
    f.add_projection("pca3", source="dino_feats", components=inp["head"])
    with torch.no_grad():
        out = f.eval(inp["pts"].to(dev()), return_names=["dino_feats", "mask", "pca3"])
        res.update({"feats": out["dino_feats"], "projected": out["pca3"]})
        inst = onehot2instance(out["mask"])
        res["instance"] = inst
        res["onehot"] = instance2onehot(inst, 8)
    L = lib()
    m = f.curr_obs_torch["dino_feats"]
    desc = L.ChannelMap(m.data_ptr(), m.shape[1], m.shape[2], m.shape[3], L.DTYPE_F32, m.stride(0), m.stride(1), m.stride(2), None)
    word = torch.empty(1, dtype=torch.int32, device=dev())            # 'word_out: one device uint32 ...; the call overwrites it'
    L.check(L.load().d3f_map_check(ctypes.byref(desc), m.shape[0], L.ptr(word), stream()))
    res["finite_word"] = word
    return res


def _dist_large_inputs():
    out = []
    for seed in (1, 2):
        s = _scene(seed, 10, False)
        s["pts"] = torch.rand((1 << 22, 3), generator=torch.Generator().manual_seed(seed)) * torch.tensor([0.4, 0.4, 0.2]) - torch.tensor([0.2, 0.2, 0.0])
        out.append(s)
    return tuple(out)


@case("dist only tiled", [], large=True)
@with_inputs(_dist_large_inputs)
def run_dist_large(inp):
    """the distance-only pass over 2^22 points: the depth maps are first copied into tiles in the caller's scratch"""
    f = _fusion(inp)
    with torch.no_grad():
        return dict(f.eval(inp["pts"].to(dev()), return_names=[]))


# ---- descriptor similarity, moments, the closed-form tracking steps -------------------------------------------------------------------------
def _corr_inputs():
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        out.append({"src": rng.standard_normal((1537, 64)).astype(np.float32), "tgt": rng.standard_normal((67, 64)).astype(np.float32),
                    "map": rng.standard_normal((70, 64, 9, 11)).astype(np.float32), "w": rng.uniform(0.0, 1.0, size=4099).astype(np.float32),
                    "rows": rng.standard_normal((4099, 129)).astype(np.float32)})
    return tuple(out)


def _corr_check(inp, out):
    import pca_cases as PCA
    wsum, mean, S, A, a = PCA.moments64(torch.from_numpy(inp["rows"]), torch.from_numpy(inp["w"]))
    assert abs(float(out["wsum"]) - float(wsum)) <= PCA.CAP_MEAN * float(wsum)
    assert PCA.check(out["mean"], mean, a, PCA.CAP_MEAN)[0] and PCA.check(out["scatter"], S, A, PCA.CAP_SCATTER)[0]
    dist = np.sqrt(((inp["src"][:, None, :].astype(np.float64) - inp["tgt"][None].astype(np.float64)) ** 2).sum(-1))
    assert np.array_equal(out["knn_idx"].cpu().numpy()[0], dist.argmin(0)) and np.array_equal(out["nearest_idx"].cpu().numpy(), dist.argmin(0))


def _sharded_abi(src, tgt, parts=3):
    """the row-sharded softmax and k-NN on one device: d3f_pairwise_softmax_local per shard, d3f_softmax_merge, d3f_softmax_apply; d3f_topk_smallest per
    shard and d3f_topk_merge"""
    L = lib()
    l = L.load()
    B1, C = src.shape
    B2, k, scale = tgt.shape[0], 4, 0.5
    cuts = [B1 * i // parts for i in range(parts + 1)]
    stats = torch.empty((parts, B2, 2), dtype=torch.int64, device=dev())            # 16-byte records
    outs, idxs, vals = [], [], []
    for r in range(parts):
        rows = src[cuts[r]:cuts[r + 1]].contiguous()
        n = rows.shape[0]
        out = torch.empty((n, B2), dtype=torch.float32, device=dev())
        ws_bytes = int(l.d3f_softmax_workspace_bytes(n, B2))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev())
        L.check(l.d3f_pairwise_softmax_local(L.ptr(rows), L.ptr(tgt), n, B2, C, scale, L.DIST_L2, cuts[r], L.ptr(out), L.ptr(stats[r]), L.ptr(ws), ws_bytes, stream()))
        idx = torch.empty((k, B2), dtype=torch.int64, device=dev())
        val = torch.empty((k, B2), dtype=torch.float32, device=dev())
        tws_bytes = int(l.d3f_pairwise_topk_workspace_bytes(n, B2))
        tws = torch.empty(max(tws_bytes, 16), dtype=torch.uint8, device=dev())
        L.check(l.d3f_topk_smallest(L.ptr(out), n, B2, k, L.ptr(idx), L.ptr(val), L.ptr(tws), tws_bytes, stream()))
        outs.append(out)
        idxs.append(torch.where(idx >= 0, idx + cuts[r], idx))
        vals.append(val)
    merged = torch.empty((B2, 2), dtype=torch.int64, device=dev())
    argmax = torch.empty(B2, dtype=torch.int64, device=dev())
    L.check(l.d3f_softmax_merge(L.ptr(stats), parts, B2, L.ptr(merged), L.ptr(argmax), stream()))
    pidx, pval = torch.stack(idxs).contiguous(), torch.stack(vals).contiguous()
    top_idx = torch.empty((k, B2), dtype=torch.int64, device=dev())
    top_val = torch.empty((k, B2), dtype=torch.float32, device=dev())
    L.check(l.d3f_topk_merge(L.ptr(pidx), L.ptr(pval), parts, k, B2, L.ptr(top_idx), L.ptr(top_val), stream()))
    for out in outs:
        L.check(l.d3f_softmax_apply(L.ptr(out), out.shape[0], B2, scale, L.ptr(merged), stream()))
    return {"sharded_softmax": torch.cat(outs), "sharded_argmax": argmax, "sharded_topk_idx": top_idx, "sharded_topk_val": top_val}


@case("similarity", ["d3f_similarity_to_target", "d3f_pairwise_similarity", "d3f_pairwise_similarity_topk", "d3f_pairwise_softmax_local", "d3f_softmax_merge",
                     "d3f_softmax_apply", "d3f_topk_merge", "d3f_row_moments"], check=_corr_check)
@with_inputs(_corr_inputs)
def run_similarity(inp):
    from d3fields_amd import corr_utils, pca
    src, tgt, fmap = T(inp["src"]), T(inp["tgt"]), T(inp["map"])
    out = {"to_target_softmax": corr_utils.compute_similarity_tensor(fmap, tgt[0], 0.5), "to_target_dist": corr_utils.compute_dist_tensor(fmap, tgt[0])}
    out["multi"] = corr_utils.compute_similarity_tensor_multi(src, tgt, None, None, 0.5)
    out["nearest_sim"], out["nearest_idx"] = corr_utils.nearest_descriptor(src, tgt, 0.5)
    out["knn_sim"], out["knn_idx"], out["knn_val"] = corr_utils.knn_descriptors(src, tgt, 4, 0.5)
    out.update(_sharded_abi(src, tgt))
    out["wsum"], out["mean"], out["scatter"] = pca.row_moments(T(inp["rows"]), T(inp["w"]))
    return out


def _track_inputs():
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        I, n, C = 3, 67, 48
        out.append({"last": rng.uniform(-0.2, 0.2, size=(I, n, 3)).astype(np.float32), "t": rng.uniform(-0.01, 0.01, size=(I, 3)).astype(np.float32),
                    "w": rng.uniform(-0.05, 0.05, size=(I, 3)).astype(np.float32), "feats": rng.standard_normal((I * n, C)).astype(np.float32),
                    "src": rng.standard_normal((I * n, C)).astype(np.float32), "dist": rng.uniform(-0.02, 0.02, size=I * n).astype(np.float32),
                    "valid": (rng.random(I * n) < 0.9).astype(np.uint8), "grad": rng.standard_normal((I, n, 3)).astype(np.float32)})
    return tuple(out)


def _track_check(inp, out):
    """tests/test_gpu_parity.py::test_tracking_step_kernels_vs_autograd on this case's inputs: torch autograd on the same expressions, its bounds"""
    from d3fields_amd import rigid
    d = dev()
    last, t0, w0 = T(inp["last"]), T(inp["t"]), T(inp["w"])
    ref_pts = rigid.rigid_transform(last, rigid.so3_exp_map(w0), t0)
    assert (out["out_pts"] - ref_pts).abs().max().item() <= 1e-6
    assert abs(out["norms"][0].item() - t0.norm().item()) <= 1e-6 and abs(out["norms"][1].item() - w0.norm().item()) <= 1e-6
    feats, dist = T(inp["feats"]).requires_grad_(True), T(inp["dist"]).requires_grad_(True)
    valid = T(inp["valid"]) != 0
    feat_loss = (torch.norm(feats - T(inp["src"]), dim=-1) * valid).mean()
    dist_loss = 0.1 * torch.clamp(dist * valid, min=0).mean()
    (feat_loss + dist_loss).backward()
    assert (out["grad_feats"] - feats.grad).abs().max().item() <= 1e-7 and (out["grad_dist"] - dist.grad).abs().max().item() <= 1e-7
    assert abs(out["loss"][0].item() - feat_loss.item()) <= 1e-5 and abs(out["loss"][1].item() - dist_loss.item()) <= 1e-6
    t_ref, w_ref = t0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    opt = torch.optim.Adam([t_ref, w_ref], lr=0.01, betas=(0.9, 0.999))
    p = rigid.rigid_transform(last, rigid.so3_exp_map(w_ref), t_ref)
    ((p * T(inp["grad"])).sum() + 0.01 * (torch.norm(t_ref) + torch.norm(w_ref))).backward()
    opt.step()
    assert (out["t"] - t_ref.detach()).abs().max().item() <= 2e-6 and (out["w"] - w_ref.detach()).abs().max().item() <= 2e-6
    assert out["step"].tolist() == [1.0] * last.shape[0]


@case("tracking steps", ["d3f_rigid_transform", "d3f_track_loss_grad", "d3f_rigid_update"], check=_track_check,
      loose={"loss": (1e-5, "tests/test_gpu_callers.py: 'the loss terms are float atomics: order varies' (atomicAdd(loss + 0 / 1, ...) in "
                            "track_loss_grad_kernel), held there to 1e-5 * max(1, |loss|)")})
@with_inputs(_track_inputs)
def run_track(inp):
    L = lib()
    l = L.load()
    last, t, w = T(inp["last"]), T(inp["t"]), T(inp["w"])
    t, w = t.clone(), w.clone()
    I, n = last.shape[0], last.shape[1]
    N, C = inp["feats"].shape
    out_pts = torch.empty((I, n, 3), dtype=torch.float32, device=dev())
    norms = torch.empty(2, dtype=torch.float32, device=dev())
    L.check(l.d3f_rigid_transform(L.ptr(last), I, n, L.ptr(t), L.ptr(w), L.ptr(out_pts), L.ptr(norms), stream()))
    g_feats = torch.empty((N, C), dtype=torch.float32, device=dev())
    g_dist = torch.empty(N, dtype=torch.float32, device=dev())
    loss = torch.empty(2, dtype=torch.float32, device=dev())
    feats, src, dist, valid = T(inp["feats"]), T(inp["src"]), T(inp["dist"]), T(inp["valid"])
    L.check(l.d3f_track_loss_grad(L.ptr(feats), L.ptr(src), L.ptr(dist), L.ptr(valid), N, C, 0.1, L.ptr(g_feats), L.ptr(g_dist), L.ptr(loss), stream()))
    # the optimiser state is in/out and 'zero at the start of a frame' (the header): zeros, as the wrapper makes them
    m, v = torch.zeros((I, 6), dtype=torch.float32, device=dev()), torch.zeros((I, 6), dtype=torch.float32, device=dev())
    step = torch.zeros(I, dtype=torch.float32, device=dev())
    grad = T(inp["grad"])
    L.check(l.d3f_rigid_update(L.ptr(last), I, n, L.ptr(grad), L.ptr(t), L.ptr(w), L.ptr(m), L.ptr(v), L.ptr(step), L.ptr(norms), 0.01, 0.01, 0.9, 0.999, 1e-8, stream()))
    return {"out_pts": out_pts, "norms": norms, "grad_feats": g_feats, "grad_dist": g_dist, "loss": loss, "t": t, "w": w, "adam_m": m, "adam_v": v, "step": step}
