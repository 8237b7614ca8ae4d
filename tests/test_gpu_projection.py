"""The projected query (Fusion.add_projection: the maps through a linear head once per observation, the k-channel map
through the ordinary kernel families, minus b) against the float64 reference, entry by entry.

Reference: oracle.field_ref.field64 on the SOURCE map gives v[n,C] and the scales s[n,C]; expected (v - mean) W^T;
|got - ref| <= tol * A with A[n,j] = sum_c s[n,c] |W[j,c]| + sum_c |mean_c W[j,c]| and the non-finite entries coinciding
(tests/projection_cases.py).  tol = 3 x the worst ratio of the float32 port measured on the host
(tests/test_projection_host.py: PORT_WORST), capped by the worst-case rounding bound (C + 4V + 8) 2^-24."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import projection_cases as PC
from conftest import ROOT
from oracle import field_cases as FC
from oracle import field_ref as R
from test_projection_host import PORT_WORST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def fusion_for(dev, case, name="proj"):
    from d3fields_amd import Fusion, _lib
    V = case["obs"]["depth"].shape[0]
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: v.to(dev) for k, v in case["obs"].items()}
    f.curr_obs_torch.update({k: m.to(dev) for k, m in case["maps"].items()})
    f.H, f.W, f.mu = case["H"], case["W"], case["mu"]
    f.reorder_points = case["reorder"]
    for flag in case["flags"]:
        f.tuning_flags |= getattr(_lib, flag)
    f.add_projection(name, source=case["source"], components=case["head_W"], mean=case["head_mean"])
    return f


def tol_of(case):
    V, C = case["obs"]["depth"].shape[0], case["maps"][case["source"]].shape[3]
    return PC.tolerance(PORT_WORST, C, V)


def query(f, case, pts, names=("proj",)):
    with torch.no_grad():
        if case["call"] == "eval":
            return f.eval(pts, return_names=list(names))
        return f.batch_eval(pts, return_names=list(names))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_projected_query_against_float64(dev, name):
    case = PC.build(name)
    f = fusion_for(dev, case)
    out = query(f, case, case["pts"].to(dev))
    torch.cuda.synchronize()
    assert tuple(out["proj"].shape) == (case["pts"].shape[0], case["k"]) and out["proj"].dtype == torch.float32
    rows = FC.sample_rows(case)
    ref, A = PC.reference(case, rows=rows)
    ok, worst, msg = R.check(out["proj"][rows.to(dev)].cpu(), ref, A, tol=tol_of(case))
    print("\n  %-28s worst |got - f64| / A = %.3g (tol %.3g)" % (name, worst, tol_of(case)))
    assert ok, (name, msg)
    # all-invalid points give -b, the transform of the reference's zero row
    dead = ~out["valid_mask"]
    if bool(dead.any()):
        b = f._projections["proj"]["b"].to(dev)
        assert torch.equal(out["proj"][dead], (-b).expand(int(dead.sum()), -1))
    # the projected map itself against the float64 map W^T, entry by entry, A = sum |m W|
    m64 = case["maps"][case["source"]].to(torch.float64)
    W64 = case["head_W"].to(torch.float64)
    pm = f._projected["proj"][2].cpu()
    ok, worst, msg = R.check(pm.reshape(-1, case["k"]), (m64 @ W64.T).reshape(-1, case["k"]), (m64.abs() @ W64.abs().T).reshape(-1, case["k"]),
                             tol=tol_of(case))
    print("  %-28s projected map: worst ratio %.3g" % (name, worst))
    assert ok, (name, "projected map", msg)


def test_structure_hand_placed_map_two_runs_inter_and_gradient(dev):
    """Bit for bit: the query equals the query of the same [V,fh,fw,k] tensor placed by hand in curr_obs_torch as an ordinary
    map, minus b; so do '<name>_inter' and the gradient w.r.t. pts of sum(out * g); two runs are bit-identical."""
    for name in ("patch V4 C384 k3", "patch f16 C129 k64", "dense C1024 k64"):
        case = PC.build(name)
        f = fusion_for(dev, case)
        pts = case["pts"].to(dev)
        with torch.no_grad():
            out = f.eval(pts, return_names=["proj"], return_inter=True)
        pm = f._projected["proj"][2]
        b = f._projections["proj"]["b"].to(dev)
        hand = fusion_for(dev, case)
        hand.curr_obs_torch["hand"] = pm.clone()
        with torch.no_grad():
            ref = hand.eval(pts, return_names=["hand"], return_inter=True)
        assert torch.equal(out["proj"], ref["hand"] - b), name
        assert tuple(out["proj_inter"].shape) == (pm.shape[0], pts.shape[0], case["k"])
        assert torch.equal(out["proj_inter"], ref["hand_inter"] - b), name
        assert torch.equal(out["dist"], ref["dist"]) and torch.equal(out["valid_mask"], ref["valid_mask"])
        # a second projection of the same source (the cache dropped) and a second query
        f.invalidate_map_checks()
        with torch.no_grad():
            again = f.eval(pts, return_names=["proj"])
        assert f._projected["proj"][2] is not pm and torch.equal(f._projected["proj"][2], pm), name
        assert torch.equal(again["proj"], out["proj"]), name
        # the gradient through _FieldQueryFn and the existing backward kernel
        g = torch.randn(pts.shape[0], case["k"], generator=torch.Generator().manual_seed(5)).to(dev)
        p1 = pts.clone().requires_grad_(True)
        (f.eval(p1, return_names=["proj"])["proj"] * g).sum().backward()
        p2 = pts.clone().requires_grad_(True)
        (hand.eval(p2, return_names=["hand"])["hand"] * g).sum().backward()
        assert torch.equal(p1.grad, p2.grad) and bool(p1.grad.abs().sum() > 0), name


def test_eval_grid_and_a_second_map_in_the_same_call(dev):
    from d3fields_amd import create_init_grid, synth
    case = PC.build("patch V4 C384 k3")
    f = fusion_for(dev, case)
    step = 0.0107
    with torch.no_grad():
        out = f.eval_grid(synth.WORK_BOX, step, return_names=["proj", case["source"]])
    torch.cuda.synchronize()
    case["pts"] = create_init_grid(synth.WORK_BOX, step)[0]
    n = case["pts"].shape[0]
    assert tuple(out["proj"].shape) == (n, 3) and tuple(out[case["source"]].shape) == (n, 384)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(n))[:20000]
    ref, A = PC.reference(case, rows=rows)
    ok, worst, msg = R.check(out["proj"][rows.to(dev)].cpu(), ref, A, tol=tol_of(case))
    print("\n  eval_grid: worst ratio %.3g (tol %.3g)" % (worst, tol_of(case)))
    assert ok, msg
    # the wide map of the same call is what it is without the projected name
    with torch.no_grad():
        alone = f.eval_grid(synth.WORK_BOX, step, return_names=[case["source"]])
    assert torch.equal(alone[case["source"]], out[case["source"]])


@pytest.mark.parametrize("name", ["patch V4 C384 k3", "dense C1024 k64"])
def test_nan_texel_planted_after_a_first_query(dev, name):
    """A NaN written into the source through torch after a first query: the source is projected again, and exactly the rows
    the float64 reference marks are NaN."""
    case = PC.build(name)
    f = fusion_for(dev, case)
    pts = case["pts"].to(dev)
    first = query(f, case, pts)
    assert bool(torch.isfinite(first["proj"]).all())
    src = case["maps"][case["source"]].clone()
    src[0, 1, 1, 0] = float("nan")
    case["maps"][case["source"]] = src
    f.curr_obs_torch[case["source"]].copy_(src.to(dev))
    out = query(f, case, pts)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out["proj"]).any()), "the NaN texel must reach some rows"
    ref, A = PC.reference(case)
    ok, worst, msg = R.check(out["proj"].cpu(), ref, A, tol=tol_of(case))
    assert ok, msg
    nan_rows = torch.isnan(out["proj"]).any(1)
    assert torch.equal(torch.isnan(out["proj"]).all(1), nan_rows)                 # dense arithmetic: all k outputs of such a row


def test_descriptor_colours_on_the_device(dev):
    from d3fields_amd import mesh
    proj, mask = PC.colour_inputs()
    got = mesh.descriptor_colors(proj.to(dev), mask.to(dev), mask_out_bg=False)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (proj.shape[0], 4)
    ok, share, msg = PC.check_colours(got, proj, mask)
    print("\n  share of bytes that differ from the float64 rule's byte: %.3g" % share)
    assert ok, msg
    # and on a real projected query: 3 components of a dense map on its surface-like cloud
    case = PC.build("dense C1024 k3")
    f = fusion_for(dev, case)
    f.curr_obs_torch["mask"] = torch.nn.functional.one_hot(torch.randint(0, 4, (4, case["H"], case["W"]), generator=torch.Generator().manual_seed(2)), 4).float().to(dev)
    out = query(f, case, case["pts"].to(dev), names=("proj", "mask"))
    cols = mesh.descriptor_colors(out["proj"], out["mask"], True)
    ok, share, msg = PC.check_colours(cols, out["proj"].cpu(), out["mask"].cpu())
    assert ok, msg


# ---- two ranks on one device, as tests/test_gpu_sharding.py ------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from d3fields_amd import Fusion, sharding, synth
        dev = torch.device("cuda:0")
        V, H, W = 4, 120, 160
        sc = synth.make_scene(V, H, W, "stress")
        f = Fusion(num_cam=V, device="cuda:0")
        f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
        f.curr_obs_torch["dino_feats"] = synth.random_map(V, 12, 16, 96, seed=1, device=dev) if rank == 0 else torch.zeros(V, 12, 16, 96, device=dev)
        f.H, f.W = H, W
        g = torch.Generator().manual_seed(9)
        p_W, p_mean = torch.randn(3, 96, generator=g), torch.randn(96, generator=g)
        f.add_projection("pca", components=p_W, mean=p_mean)
        sharding.broadcast_observation(f, src=0)
        pts = synth.random_cloud(70001, seed=3).to(dev)
        with torch.no_grad():
            full = sharding.sharded_eval(f, pts, ["pca"])
            single = f.batch_eval(pts, return_names=["pca"])
            wide = f.batch_eval(pts, return_names=["dino_feats"])["dino_feats"]
        ok = all(torch.equal(full[k], single[k]) for k in single) and tuple(full["pca"].shape) == (70001, 3)
        # a per-frame loop: rank 0 gets a new observation and broadcasts it INTO the tensors every rank has already projected
        # (an in-place overwrite that leaves the version counters alone); the next query must see the new maps on every rank
        if rank == 0:
            f.curr_obs_torch["dino_feats"].copy_(synth.random_map(V, 12, 16, 96, seed=21, device=dev))
        sharding.broadcast_observation(f, src=0)
        with torch.no_grad():
            second = f.batch_eval(pts, return_names=["pca"])["pca"]
        fresh = Fusion(num_cam=V, device="cuda:0")
        fresh.curr_obs_torch = dict(f.curr_obs_torch)
        fresh.H, fresh.W = H, W
        fresh.add_projection("pca", components=p_W, mean=p_mean)
        with torch.no_grad():
            want2 = fresh.batch_eval(pts, return_names=["pca"])["pca"]
        ok = ok and torch.equal(second, want2) and not torch.equal(second, single["pca"])
        p = f._projections["pca"]
        want = wide.double() @ p["W"].double().T.to(dev) - p["b"].double().to(dev)
        err = float((single["pca"].double() - want).abs().max())
        q.put((rank, bool(ok), err))
    finally:
        dist.destroy_process_group()


def test_two_ranks_sharded_projected_query():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, ok, err in res:
        assert ok, "rank %d: the sharded projected query differs from the single-process one" % rank
        assert err <= 1e-3, "rank %d: projected query is off the projected wide rows by %g" % (rank, err)
