"""Consensus poses on the device (d3f_pose_consensus_* / d3f_pose_refit, csrc/consensus_kernels.hip; consensus.consensus_poses, BakedField.relocate)
against the NumPy restatement of tests/consensus_cases.py.

The score: count, the debug assignments and the debug poses equal the restatement byte for byte, from buffers poisoned one row too long; a second
run gives the same bytes; the poison beyond the written rows stays.  The selection: hypothesis indices, counts, assignments and poses of every rank,
n_gated and n_survivors, exactly.  The refit: to the last bit on exact quarter turns, within consensus_cases.refit_bound of the eigh restatement
elsewhere.  The chain: relocate recovers a pose 60 degrees from the identity that align alone does not.

Mutants of the kernels and the assert that catches each:
  a digit or a triplet column swapped, a cross product's sign, an fma contracted in            test_score_equals_the_restatement (poses, byte for byte)
  the queue slot of a lane off by one, a pose drained twice or never, the ring overwritten     the same test on m33k1 (every hypothesis live) and m17k3 (nine workgroups)
  < for <= at tau2, ties to the higher s, a NaN row assigned                                    the same test (assignments), duplicates
  the cut one count too high or low, the take counted from the wrong end, a block rank off     test_select_equals_the_restatement on m17k3_cut7 / _cut1 and the t63 / t64 / t65 cases
  a round that does not kill the winner, `shared` compared with > for >=                        the same test on m17k3 and m64k2 (n_poses = 64, eleven and thirteen rounds)
  a Jacobi rotation with the wrong sign, the quaternion's columns for rows                      test_refit_*
"""
import numpy as np
import pytest
import torch

import align_cases as AC
import consensus_cases as CC
import volume_cases as VC
from d3fields_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
POISON_BYTE, POISON = 0x5A, -7.5
SCORE_CASES = [n for n in CC.CASES if n not in ("m17k3_cut7", "m17k3_cut1")]       # (the same inputs as m17k3: only the selection differs)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def device_inputs(dev, cs):
    return torch.from_numpy(cs["p"]).to(dev), torch.from_numpy(cs["c"]).to(dev), torch.from_numpy(cs["trip"]).to(dev)


def run_score(dev, cs, max_survivors, debug=True):
    """d3f_pose_consensus_score through the C ABI on poisoned outputs one row too long -> (count, pose, assign, workspace) as torch tensors, the extra row included"""
    lib = _lib.load()
    p, c, trip = device_inputs(dev, cs)
    M, k, n_trip = len(cs["p"]), cs["c"].shape[1], len(cs["trip"])
    T = n_trip * k ** 3
    count = torch.full((T + 1,), POISON_BYTE, dtype=torch.uint8, device=dev)
    pose = torch.full((T + 1, 12), POISON, dtype=torch.float32, device=dev)
    assign = torch.full((T + 1, M), POISON_BYTE, dtype=torch.int8, device=dev)
    ws_bytes = int(lib.d3f_pose_consensus_workspace_bytes(M, k, n_trip, max_survivors))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), POISON_BYTE, dtype=torch.uint8, device=dev)
    tau2 = float(F(cs["tau"]) * F(cs["tau"]))
    _lib.check(lib.d3f_pose_consensus_score(_lib.ptr(p), _lib.ptr(c), M, k, _lib.ptr(trip), cs["trip"].ctypes.data, n_trip, tau2, cs["side_tol"], cs["min_side"],
                                            cs["min_sin"], _lib.ptr(count), _lib.ptr(pose) if debug else None, _lib.ptr(assign) if debug else None, _lib.ptr(ws), ws_bytes,
                                            _lib.current_stream_handle(dev)))
    return count, pose, assign, (ws, ws_bytes)


def run_select(dev, cs, params, count, ws):
    lib = _lib.load()
    p, c, trip = device_inputs(dev, cs)
    M, k, n_trip, H = len(cs["p"]), cs["c"].shape[1], len(cs["trip"]), params["n_poses"]
    hyp = torch.full((H + 1,), -77, dtype=torch.int32, device=dev)
    inl = torch.full((H + 1,), -77, dtype=torch.int32, device=dev)
    asg = torch.full((H + 1, 64), POISON_BYTE, dtype=torch.int8, device=dev)
    pose = torch.full((H + 1, 12), POISON, dtype=torch.float32, device=dev)
    stats = torch.full((5,), -77, dtype=torch.int32, device=dev)
    tau2 = float(F(cs["tau"]) * F(cs["tau"]))
    _lib.check(lib.d3f_pose_consensus_select(_lib.ptr(p), _lib.ptr(c), M, k, _lib.ptr(trip), n_trip, tau2, cs["side_tol"], cs["min_side"], cs["min_sin"], _lib.ptr(count),
                                             params["min_inliers"], params["shared"], params["max_survivors"], H, _lib.ptr(hyp), _lib.ptr(inl), _lib.ptr(asg), _lib.ptr(pose),
                                             _lib.ptr(stats), _lib.ptr(ws[0]), ws[1], _lib.current_stream_handle(dev)))
    out = {"hyp": hyp, "inliers": inl, "assign": asg, "pose": pose, "stats": stats}
    return {key: v.cpu().numpy() for key, v in out.items()}


@pytest.mark.parametrize("name", SCORE_CASES)
def test_score_equals_the_restatement(dev, name):
    cs, params = CC.case(name)
    ref = CC.scored(name)
    T = len(ref["count"])
    count, pose, assign, _ = run_score(dev, cs, params["max_survivors"])
    count, pose, assign = count.cpu().numpy(), pose.cpu().numpy(), assign.cpu().numpy()
    print(name, "T", T, "gated", int(ref["live"].sum()), "pose entries that differ", int((pose[:T].view(np.uint32) != ref["pose"].view(np.uint32)).sum()))
    assert pose[:T].tobytes() == ref["pose"].tobytes()
    assert np.array_equal(count[:T], ref["count"])
    assert np.array_equal(assign[:T], ref["assign"])
    assert count[T] == POISON_BYTE and (assign[T] == POISON_BYTE).all() and (pose[T] == POISON).all()
    again = run_score(dev, cs, params["max_survivors"])
    assert again[0].cpu().numpy().tobytes() == count.tobytes() and again[1].cpu().numpy().tobytes() == pose.tobytes() and again[2].cpu().numpy().tobytes() == assign.tobytes()
    # without the debug outputs the counts are the same
    assert np.array_equal(run_score(dev, cs, params["max_survivors"], debug=False)[0].cpu().numpy(), count)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_select_equals_the_restatement(dev, name):
    cs, params = CC.case(name)
    ref = CC.reference(name)
    H = params["n_poses"]
    count, _, _, ws = run_score(dev, cs, params["max_survivors"], debug=False)
    got = run_select(dev, cs, params, count, ws)
    print(name, "found", ref["found"], "gated", ref["n_gated"], "survivors", ref["n_survivors"], "device stats", got["stats"][:4].tolist())
    assert got["stats"][:4].tolist() == [ref["found"], ref["n_gated"], ref["n_survivors"], ref["cut"]] and got["stats"][4] == -77
    assert np.array_equal(got["hyp"][:H], ref["hyp"]) and np.array_equal(got["inliers"][:H], ref["inliers"])
    assert np.array_equal(got["assign"][:H], ref["sel_assign"])
    assert got["pose"][:H].tobytes() == ref["sel_pose"].tobytes()
    assert got["hyp"][H] == -77 and got["inliers"][H] == -77 and (got["assign"][H] == POISON_BYTE).all() and (got["pose"][H] == POISON).all()
    again = run_select(dev, cs, params, count, ws)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), key


def run_refit(dev, p, c, assign, tau2):
    lib = _lib.load()
    H, M, k = len(assign), len(p), c.shape[1]
    pd, cd, ad = torch.from_numpy(p).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(assign).to(dev)
    pose = torch.full((H + 1, 12), POISON, dtype=torch.float32, device=dev)
    rmse = torch.full((H + 1,), POISON, dtype=torch.float64, device=dev)
    inl = torch.full((H + 1,), -77, dtype=torch.int32, device=dev)
    _lib.check(lib.d3f_pose_refit(_lib.ptr(pd), _lib.ptr(cd), M, k, _lib.ptr(ad), H, float(tau2), _lib.ptr(pose), _lib.ptr(rmse), _lib.ptr(inl), _lib.current_stream_handle(dev)))
    pose, rmse, inl = pose.cpu().numpy(), rmse.cpu().numpy(), inl.cpu().numpy()
    assert (pose[H] == POISON).all() and rmse[H] == POISON and inl[H] == -77
    return pose[:H], rmse[:H], inl[:H]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refit_is_exact_on_a_quarter_turn(dev, axis):
    p, c, R, t = CC.exact_refit_case(axis)
    assign = np.full((2, 64), -1, np.int8)
    assign[0, :8] = 0                                       # the second row has no pair: padding
    pose, rmse, inl = run_refit(dev, p, c, assign, 0.25)
    print("axis", axis, "R", pose[0, :9], "t", pose[0, 9:], "rmse", rmse[0])
    assert np.array_equal(pose[0, :9].reshape(3, 3), R) and np.array_equal(pose[0, 9:], t)
    assert rmse[0] == 0.0 and inl[0] == 8
    assert np.isnan(pose[1]).all() and np.isnan(rmse[1]) and inl[1] == -1


def check_refit(cs, params, ref, pose, rmse, inl):
    """the refit outputs of ref['sel_assign'] against the Horn restatement -> the worst error / bound (shared with tests/dirty_cases.py)"""
    worst = 0.0
    for r in range(params["n_poses"]):
        if r >= ref["found"]:
            assert np.isnan(pose[r]).all() and np.isnan(rmse[r]) and inl[r] == -1
            continue
        pp, cc = CC.pairs_of(cs, ref["sel_assign"][r])
        bound, gap = CC.refit_bound(pp, cc)
        assert gap >= CC.MIN_GAP                            # (test_consensus_host asserts it of every case: the bound means something)
        R, t, _, _ = CC.horn(pp, cc)
        want = pp.astype(np.float64) @ R.T + t
        got = pp.astype(np.float64) @ pose[r, :9].reshape(3, 3).astype(np.float64).T + pose[r, 9:].astype(np.float64)
        err = np.linalg.norm(got - want, axis=1).max()
        worst = max(worst, err / bound)
        assert err <= bound, (r, err, bound, gap)
        want_rmse = np.sqrt(((got - cc.astype(np.float64)) ** 2).sum() / len(pp))
        assert abs(rmse[r] - want_rmse) <= 1e-12 * max(1.0, want_rmse) + 8 * CC.EPS * np.abs(cc).max()
        n, _ = CC.score(pose[r:r + 1], cs["p"], cs["c"], ref["tau2"])       # the count at the DEVICE's refit pose, by the restatement: exact
        assert inl[r] == n[0]
    return worst


@pytest.mark.parametrize("name", CC.REFIT_CASES)
def test_refit_against_the_horn_restatement(dev, name):
    cs, params = CC.case(name)
    ref = CC.reference(name)
    pose, rmse, inl = run_refit(dev, cs["p"], cs["c"], ref["sel_assign"], ref["tau2"])
    print(name, "refit: worst error / bound", check_refit(cs, params, ref, pose, rmse, inl))


# ---- the public layer ---------------------------------------------------------------------------------------------------------------------
def test_consensus_poses_is_the_kernels(dev):
    from d3fields_amd import consensus_poses
    from d3fields_amd.rigid import rigid_transform
    name = "two_objects"
    cs, params = CC.case(name)
    ref = CC.reference(name)
    p, c, _ = device_inputs(dev, cs)
    out = consensus_poses(p, c, cs["tau"], triplets=cs["trip"], **{key: params[key] for key in ("n_poses", "min_inliers", "shared", "max_survivors")})
    assert set(out) == {"rot", "trans", "inliers", "assignment", "hypothesis", "triplet", "digits", "count", "n_gated", "n_survivors", "refit_rot", "refit_trans", "rmse",
                        "refit_inliers"}
    assert all(v.device == p.device and not v.requires_grad for v in out.values())
    H, M, k = params["n_poses"], len(cs["p"]), cs["c"].shape[1]
    assert out["hypothesis"].dtype == torch.int64 and out["inliers"].dtype == torch.int32 and out["assignment"].dtype == torch.int32 and out["rmse"].dtype == torch.float64
    assert (out["count"].item(), out["n_gated"].item(), out["n_survivors"].item()) == (ref["found"], ref["n_gated"], ref["n_survivors"]) and ref["found"] == 2
    assert np.array_equal(out["hypothesis"].cpu().numpy(), ref["hyp"]) and np.array_equal(out["inliers"].cpu().numpy(), ref["inliers"])
    assert np.array_equal(out["assignment"].cpu().numpy(), ref["sel_assign"][:, :M])
    rot, trans = out["rot"].cpu().numpy(), out["trans"].cpu().numpy()
    for r in range(2):                                      # the row-vector convention: the kernels' R transposed
        assert np.array_equal(rot[r].T.reshape(9), ref["sel_pose"][r, :9]) and np.array_equal(trans[r], ref["sel_pose"][r, 9:])
        tr, a, b, cc = CC.digits_of(int(ref["hyp"][r]), k)
        assert out["triplet"][r].tolist() == cs["trip"][tr].tolist() and out["digits"][r].tolist() == [a, b, cc]
    assert np.isnan(rot[2:]).all() and np.isnan(trans[2:]).all() and (out["triplet"][2:] == -1).all() and (out["digits"][2:] == -1).all() and (out["hypothesis"][2:] == -1).all()
    assert (out["assignment"][2:] == -1).all() and torch.isnan(out["rmse"][2:]).all() and (out["refit_inliers"][2:] == -1).all()
    # the refit poses put the members of each planted motion onto their images
    for r, (R, t, idx) in enumerate(cs["motions"]):
        moved = rigid_transform(p[None], out["refit_rot"][r:r + 1], out["refit_trans"][r:r + 1])[0].cpu().numpy()
        want = cs["p"][idx].astype(np.float64) @ R.T + t
        assert np.abs(moved[idx] - want).max() < 1e-5 and out["rmse"][r].item() < 1e-6 and out["refit_inliers"][r].item() == len(idx)
    # all triplets by default; a fixed seed gives identical results on two calls, another seed other triplets
    small, _ = CC.case("m17k3")
    ps, cs_, _ = device_inputs(dev, small)
    full = consensus_poses(ps, cs_, small["tau"], n_poses=4)
    assert np.array_equal(full["hypothesis"].cpu().numpy()[:1], CC.reference("m17k3", min_inliers=4)["hyp"][:1])
    a = consensus_poses(ps, cs_, small["tau"], max_triplets=100, seed=3)
    b = consensus_poses(ps, cs_, small["tau"], max_triplets=100, seed=3)
    for key in a:
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    assert not torch.equal(a["triplet"], consensus_poses(ps, cs_, small["tau"], max_triplets=100, seed=4)["triplet"])
    # no refit
    assert "refit_rot" not in consensus_poses(ps, cs_, small["tau"], refit=False)


def test_public_layer_errors_and_empty_problems(dev):
    from d3fields_amd import consensus_poses
    cs, _ = CC.case("m5k3")
    p, c, _ = device_inputs(dev, cs)
    for bad in (dict(model_pts=p[0]), dict(model_pts=p[:2], candidates=c[:2]), dict(candidates=c[:4]), dict(candidates=c[:, :, :2]), dict(tau=0.0), dict(tau=float("nan")),
                dict(tau=-1.0), dict(n_poses=0), dict(n_poses=65), dict(min_inliers=2), dict(shared=0), dict(max_survivors=0), dict(min_sin=1.5), dict(side_tol=-1.0),
                dict(triplets=[[0, 1, 5]]), dict(triplets=[[1, 1, 2]]), dict(triplets=[[2, 1, 0]]), dict(triplets=[[0, 1]]), dict(triplets=[[0, 1, 2]], max_triplets=3),
                dict(candidates=torch.zeros((5, 9, 3), device=dev))):
        kw = {"model_pts": p, "candidates": c, "tau": 0.03, **bad}
        with pytest.raises(ValueError):
            consensus_poses(**kw)
    with pytest.raises(ValueError):
        consensus_poses(torch.zeros((65, 3), device=dev), torch.zeros((65, 1, 3), device=dev), 0.03)
    with pytest.raises(TypeError):
        consensus_poses(p.double(), c, 0.03)
    with pytest.raises(TypeError):
        consensus_poses(p, c.half(), 0.03)
    with pytest.raises(RuntimeError):
        consensus_poses(p.cpu(), c, 0.03)
    with pytest.raises(RuntimeError):
        consensus_poses(p, c.cpu(), 0.03)
    # no triplet: nothing is launched but the refit of the padding, zero poses
    for kw in (dict(triplets=np.zeros((0, 3), np.int32)), dict(max_triplets=0)):
        out = consensus_poses(p, c, 0.03, n_poses=3, **kw)
        assert out["count"].item() == 0 and out["n_gated"].item() == 0 and out["n_survivors"].item() == 0
        assert torch.isnan(out["rot"]).all() and (out["hypothesis"] == -1).all() and (out["assignment"] == -1).all() and (out["inliers"] == -1).all()
        assert tuple(out["rot"].shape) == (3, 3, 3) and tuple(out["assignment"].shape) == (3, 5) and torch.isnan(out["refit_rot"]).all() and (out["refit_inliers"] == -1).all()
    # inputs that require grad are detached
    out = consensus_poses(p.clone().requires_grad_(True), c, 0.03)
    assert not any(v.requires_grad for v in out.values())


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def field_of(vol, dev):
    from d3fields_amd import BakedField
    sets = {k: torch.from_numpy(v).to(dev) for k, v in vol["sets"].items()}
    return BakedField.from_arrays(np.asarray(vol["origin"]).tolist(), float(vol["step"]), torch.from_numpy(vol["dist"]).to(dev), valid=torch.from_numpy(vol["valid"]).to(dev),
                                  **sets)


def scene_error(points):
    s = CC.scene()
    return float(np.linalg.norm(points.astype(np.float64) - s["x"].astype(np.float64), axis=1).max() / VC.STEP)


@pytest.mark.parametrize("banded", [False, True])
def test_relocate_recovers_a_pose_that_align_alone_does_not(dev, banded):
    s = CC.scene()
    f = field_of(s["vol"], dev)
    if banded:
        f = f.to_band(AC.SCENE_BAND_STEPS * VC.STEP)
    pts, tg = torch.from_numpy(s["p"]).to(dev), torch.from_numpy(s["targets"]).to(dev)
    fit = f.relocate(pts, "feat", tg, k=CC.SCENE_K, radius_voxels=CC.SCENE_RADIUS, n_poses=8, iters=20)
    assert set(fit) == {"rot", "trans", "points", "cost", "valid", "status", "steps", "history", "best", "consensus"}
    assert not any(v.requires_grad for v in fit.values() if isinstance(v, torch.Tensor)) and not any(v.requires_grad for v in fit["consensus"].values())
    cons = fit["consensus"]
    best = fit["best"].item()
    errors = [scene_error(x) for x in fit["points"].cpu().numpy()]
    print("banded" if banded else "dense", "consensus inliers", cons["inliers"].tolist(), "count", cons["count"].item(), "status", fit["status"].tolist(), "best", best,
          "errors (voxels)", np.round(errors, 4), "rmse", cons["rmse"].tolist()[:2])
    assert best == 0                                        # the rank-0 consensus pose
    assert fit["status"][0].item() == AC.CONVERGED and errors[0] < 0.1
    assert cons["inliers"][0].item() >= int(s["present"].sum()) and cons["count"].item() >= 1
    assert (cons["assignment"][0].cpu().numpy()[s["present"]] >= 0).all()
    # the ranks the consensus did not fill start at a NaN pose and end NO_GRADIENT
    n = cons["count"].item()
    assert fit["status"][n:].tolist() == [AC.NO_GRADIENT] * (8 - n)
    # align from the identity on the same inputs does not get there: what the parent commit could do
    alone = f.align(pts[None], "feat", tg[None], iters=20)
    print("align from the identity: status", alone["status"].tolist(), "error", scene_error(alone["points"][0].cpu().numpy()))
    assert not (alone["status"][0].item() == AC.CONVERGED and scene_error(alone["points"][0].cpu().numpy()) < 0.1)
    # one model per call
    with pytest.raises(ValueError):
        f.relocate(pts[None], "feat", tg)
    with pytest.raises(RuntimeError):
        f.relocate(pts.cpu(), "feat", tg)
    with pytest.raises(TypeError):
        f.relocate(pts.double(), "feat", tg)
    with pytest.raises(KeyError):
        f.relocate(pts, "nope", tg)


def test_the_steady_state_does_not_make_the_host_wait(dev):
    """Once the triplet table of a key is on the device, consensus_poses only launches: under torch's sync debug mode, which raises at every
    operation that makes the host wait for the device, it runs through and gives the bytes of the warm-up call; so does the align that relocate
    chains after it.  (locate, the first step of relocate, builds small tensors from host values and does wait; it is not part of this change.)"""
    from d3fields_amd import consensus_poses
    cs, _ = CC.case("m17k3")
    p, c, _ = device_inputs(dev, cs)
    s = CC.scene()
    f = field_of(s["vol"], dev)
    pts, tg = torch.from_numpy(s["p"]).to(dev), torch.from_numpy(s["targets"]).to(dev)
    cand = f.locate(tg, "feat", k=CC.SCENE_K, radius_voxels=CC.SCENE_RADIUS)["refined"].to(torch.float32)

    def chain():
        cons = consensus_poses(pts, cand, 2 * float(VC.STEP))
        fit = f.align(pts[None].expand(8, -1, -1), "feat", tg[None].expand(8, -1, -1), rot=cons["refit_rot"], trans=cons["refit_trans"], iters=20)
        return {**cons, **{"align_" + key: v for key, v in fit.items()}}

    calls = (lambda: consensus_poses(p, c, cs["tau"]), lambda: consensus_poses(p, c, cs["tau"], max_triplets=100, seed=3), chain)
    warm = [call() for call in calls]                       # the first call of a key uploads its table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.zeros(1, device=dev).item()               # the mode is in force here
        again = [call() for call in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(warm, again):
        for key in a:
            assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    assert again[2]["align_status"][0].item() == AC.CONVERGED
