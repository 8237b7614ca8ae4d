"""The consensus poses on the host: the C ABI (symbols, bindings, every status code from planted bad arguments, no scratch), the NumPy restatement of
tests/consensus_cases.py against independent brute-force formulations, the planted facts of the case set that the GPU tests inherit, and the chain
locate -> consensus -> align on the small scene, restated."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as AC
import consensus_cases as CC
import volume_cases as VC
from conftest import ROOT
from d3fields_amd import _lib, build

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
F = np.float32
NAMES = ("d3f_pose_consensus_workspace_bytes", "d3f_pose_consensus_score", "d3f_pose_consensus_select", "d3f_pose_refit")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def _declared(hdr, name):
    decl = re.search(r"\b(?:int|int64_t) %s\(([^;]*)\);" % name, hdr).group(1)
    return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]


def test_consensus_symbols_and_unchanged_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
        assert len(_declared(hdr, name)) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define D3F_CONSENSUS_MAX_POINTS (\d+)", hdr).group(1)) == _lib.CONSENSUS_MAX_POINTS == CC.MAX_M
    assert int(re.search(r"#define D3F_CONSENSUS_MAX_CANDIDATES (\d+)", hdr).group(1)) == _lib.CONSENSUS_MAX_CANDIDATES == CC.MAX_K
    assert re.search(r"#define D3F_CONSENSUS_MAX_SURVIVORS \(1 << 16\)", hdr) and _lib.CONSENSUS_MAX_SURVIVORS == 1 << 16
    vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    assert _lib.SIGNATURES[NAMES[0]] == (i64, [i32, i32, i64, i64])
    assert _lib.SIGNATURES[NAMES[1]] == (ctypes.c_int, [vp, vp, i32, i32, vp, vp, i64, f32, f64, f64, f64, vp, vp, vp, vp, i64, vp])
    assert _lib.SIGNATURES[NAMES[2]] == (ctypes.c_int, [vp, vp, i32, i32, vp, i64, f32, f64, f64, f64, vp, i32, i32, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp])
    assert _lib.SIGNATURES[NAMES[3]] == (ctypes.c_int, [vp, vp, i32, i32, vp, i32, f32, vp, vp, vp, vp])
    assert _declared(hdr, NAMES[1]) == ["model", "cand", "M", "k", "triplets", "triplets_host", "n_trip", "tau2", "side_tol", "min_side", "min_sin", "count_out", "pose_out",
                                        "assign_out", "workspace", "workspace_bytes", "stream"]
    assert _declared(hdr, NAMES[3]) == ["model", "cand", "M", "k", "assign", "n_poses", "tau2", "pose_out", "rmse_out", "inliers_out", "stream"]
    assert "consensus_kernels.hip" in build.SOURCES
    # the workspace grows with the hypotheses and with the survivors (70 bytes each); 0 for shapes that are not served
    ws = lib.d3f_pose_consensus_workspace_bytes
    assert ws(17, 2, 64, 7) > 0 and ws(17, 2, 64, 65536) - ws(17, 2, 64, 1) == 65536 * 70 - 4 * 256 and ws(64, 8, 4000000, 65536) > ws(64, 8, 40000, 65536)
    assert ws(2, 2, 5, 7) == ws(65, 2, 5, 7) == ws(5, 0, 5, 7) == ws(5, 9, 5, 7) == ws(5, 2, -1, 7) == ws(5, 2, 5, 0) == ws(5, 2, 5, (1 << 16) + 1) == ws(5, 8, 1 << 23, 7) == 0


def test_consensus_validation_status_codes():
    lib = _lib.load()
    err = lib.d3f_last_error
    p, q, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p((1 << 20) + 2)
    table = np.array([[0, 1, 2], [0, 2, 4], [1, 3, 4]], np.int32)

    def score(model=p, cand=p, M=5, k=2, trip=p, host=table, n_trip=3, tau2=0.01, side_tol=0.1, min_side=0.2, min_sin=0.2, count=q, pose=None, assign=None, ws=q,
              ws_bytes=1 << 20):
        return lib.d3f_pose_consensus_score(model, cand, M, k, trip, None if host is None else host.ctypes.data, n_trip, tau2, side_tol, min_side, min_sin, count, pose, assign,
                                            ws, ws_bytes, None)

    def select(model=p, cand=p, M=5, k=2, trip=p, n_trip=3, tau2=0.01, side_tol=0.1, min_side=0.2, min_sin=0.2, count=q, min_inliers=4, shared=3, max_survivors=100,
               n_poses=8, hyp=q, inl=q, asg=q, pose=q, stats=q, ws=q, ws_bytes=1 << 20):
        return lib.d3f_pose_consensus_select(model, cand, M, k, trip, n_trip, tau2, side_tol, min_side, min_sin, count, min_inliers, shared, max_survivors, n_poses, hyp, inl,
                                             asg, pose, stats, ws, ws_bytes, None)

    def refit(model=p, cand=p, M=5, k=2, assign=q, n_poses=8, tau2=0.01, pose=q, rmse=q, inl=q):
        return lib.d3f_pose_refit(model, cand, M, k, assign, n_poses, tau2, pose, rmse, inl, None)

    # D3F_ERR_INVALID_ARG: NULL pointers, tau2 / tolerances / counts out of range
    for kw in ("model", "cand", "trip", "host", "count", "ws"):
        assert score(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    for kw in ("model", "cand", "trip", "count", "hyp", "inl", "asg", "pose", "stats", "ws"):
        assert select(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    for kw in ("model", "cand", "assign", "pose", "rmse", "inl"):
        assert refit(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert score(tau2=bad) == select(tau2=bad) == refit(tau2=bad) == _lib.ERR_INVALID_ARG and b"tau2" in err(), bad
    for kw in ("side_tol", "min_side", "min_sin"):
        for bad in (-1.0, float("nan"), float("inf")):
            assert score(**{kw: bad}) == select(**{kw: bad}) == _lib.ERR_INVALID_ARG, (kw, bad)
    assert score(min_sin=1.5) == _lib.ERR_INVALID_ARG and score(n_trip=-1) == select(n_trip=-1) == _lib.ERR_INVALID_ARG and b"negative" in err()
    for kw, bad in (("min_inliers", 2), ("min_inliers", 65), ("shared", 0), ("shared", 65), ("max_survivors", 0), ("max_survivors", (1 << 16) + 1)):
        assert select(**{kw: bad}) == _lib.ERR_INVALID_ARG and b"outside" in err(), (kw, bad)
    # D3F_ERR_BAD_SHAPE: M, k, n_poses out of range, a triplet outside [0, M) or not ascending, T above 2^31 - 1
    for kw, bad in (("M", 2), ("M", 65), ("k", 0), ("k", 9)):
        assert score(**{kw: bad}) == select(**{kw: bad}) == refit(**{kw: bad}) == _lib.ERR_BAD_SHAPE and b"outside" in err(), (kw, bad)
    assert select(n_poses=0) == select(n_poses=65) == refit(n_poses=-1) == refit(n_poses=65) == _lib.ERR_BAD_SHAPE and b"n_poses" in err()
    for bad in ([0, 1, 5], [-1, 1, 2], [1, 1, 2], [0, 3, 2], [2, 1, 0]):
        assert score(host=np.array([[0, 1, 2], bad, [1, 3, 4]], np.int32)) == _lib.ERR_BAD_SHAPE and b"triplet 1" in err(), bad
    assert score(k=8, n_trip=1 << 22) == select(k=8, n_trip=1 << 22) == _lib.ERR_BAD_SHAPE and b"2^31" in err()
    # D3F_ERR_BAD_LAYOUT: misaligned pointers
    for kw in ("model", "cand", "trip", "pose", "ws"):
        assert score(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    for kw in ("model", "cand", "trip", "hyp", "inl", "asg", "pose", "stats", "ws"):
        assert select(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    for kw in ("model", "cand", "pose", "inl"):
        assert refit(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    assert refit(rmse=ctypes.c_void_p((1 << 20) + 4)) == _lib.ERR_BAD_LAYOUT and b"8-byte" in err()
    # D3F_ERR_WORKSPACE
    need = lib.d3f_pose_consensus_workspace_bytes(5, 2, 3, 100)
    assert select(ws_bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in err() and score(ws_bytes=511) == _lib.ERR_WORKSPACE
    # n_trip == 0 (n_poses == 0 for the refit): D3F_OK and nothing launched, buffers may be NULL; validation still comes first
    assert score(n_trip=0, model=None, cand=None, trip=None, host=None, count=None, ws=None, ws_bytes=0) == _lib.OK
    assert select(n_trip=0, model=None, cand=None, trip=None, count=None, hyp=None, inl=None, asg=None, pose=None, stats=None, ws=None, ws_bytes=0) == _lib.OK
    assert refit(n_poses=0, model=None, cand=None, assign=None, pose=None, rmse=None, inl=None) == _lib.OK
    assert score(n_trip=0, tau2=0.0) == _lib.ERR_INVALID_ARG and select(n_trip=0, M=2) == _lib.ERR_BAD_SHAPE and select(n_trip=0, n_poses=0) == _lib.ERR_BAD_SHAPE
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(score(tau2=-1.0))
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "consensus_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("consensus_score_kernel", "consensus_cut_kernel", "consensus_eq_kernel", "consensus_flag_kernel", "consensus_rescore_kernel", "consensus_select_kernel",
                   "pose_refit_kernel"):
        assert kernel in names, (kernel, out)
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0, (name, vgpr, scratch, occ)
    src = open(os.path.join(ROOT, "d3fields_amd", "csrc", "consensus_kernels.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "fmaf" not in code and "fma(" not in code and "atomicAdd(&hist" in code and not re.search(r"atomicAdd\([^)]*(float|double)", code)


# ---- the restatement against brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m5k3", "m17k2_t65", "two_objects"])
def test_frame_pose_and_counts_against_brute_force(name):
    """Poses by SVD-Kabsch on the three pairs: where the two triangles are congruent (to rounding) the frame pose agrees to rounding; where they are
    not, both put the sample's centroid onto the observed centroid.  Counts by a plain loop in float64 with a margin at tau2."""
    cs, _ = CC.case(name)
    ref = CC.scored(name)
    p, c, trip, k = cs["p"].astype(np.float64), cs["c"].astype(np.float64), cs["trip"], cs["c"].shape[1]
    live = np.flatnonzero(ref["live"])
    assert len(live) > 0
    congruent = 0
    for h in live:
        tr, a, b, d = CC.digits_of(int(h), k)
        i, j, l = trip[tr]
        P, Q = p[[i, j, l]], np.stack([c[i, a], c[j, b], c[l, d]])
        assert i < j < l and np.linalg.norm(P[1] - P[0]) >= cs["min_side"] and abs(np.linalg.norm(Q[1] - Q[0]) - np.linalg.norm(P[1] - P[0])) <= cs["side_tol"]
        R, t = ref["pose"][h, :9].reshape(3, 3).astype(np.float64), ref["pose"][h, 9:].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
        assert np.abs(R @ P.mean(0) + t - Q.mean(0)).max() < 1e-6
        sides = lambda X: np.array([np.linalg.norm(X[1] - X[0]), np.linalg.norm(X[2] - X[0]), np.linalg.norm(X[2] - X[1])])
        if np.abs(sides(P) - sides(Q)).max() < 1e-6:
            congruent += 1
            Rk, tk = CC.kabsch(P, Q)
            assert np.abs(R - Rk).max() < 1e-5 and np.abs(t - tk).max() < 1e-5, h
        # the count by a plain loop: a point whose nearest candidate is clearly inside (outside) tau must (not) be assigned
        tau2 = cs["tau"] ** 2
        sure_in = sure_out = 0
        for q in range(len(p)):
            d2 = ((R @ p[q] + t - c[q]) ** 2).sum(axis=1)
            d2 = np.where(np.isnan(d2), np.inf, d2)
            s = int(np.argmin(d2))
            if d2[s] < tau2 * (1 - 1e-4):
                sure_in += 1
                if (np.sort(d2)[1:2] > d2[s] * (1 + 1e-4) + 1e-12).all():
                    assert ref["assign"][h, q] == s, (h, q)
                else:
                    assert ref["assign"][h, q] >= 0
            elif d2[s] > tau2 * (1 + 1e-4):
                sure_out += 1
                assert ref["assign"][h, q] == -1, (h, q)
        assert sure_in <= ref["count"][h] <= len(p) - sure_out
    assert congruent > 0
    assert not ref["count"][~ref["live"]].any() and (ref["assign"][~ref["live"]] == -1).all() and not ref["pose"][~ref["live"]].any()


@pytest.mark.parametrize("name", ["m17k3", "m17k3_cut7", "two_objects", "m64k2", "duplicates"])
def test_greedy_selection_does_not_depend_on_the_order(name):
    """The O(S^2) formulation: a survivor is picked iff no PICKED survivor that is better than it shares `shared` assignments with it -- decided by
    recursion, visiting the survivors in a shuffled order; the first n_poses picks in key order are the greedy rounds."""
    cs, params = CC.case(name)
    ref = CC.reference(name)
    h = ref["survivors"]
    count, assign = ref["count"][h].astype(np.int64), ref["assign"][h]
    S = len(h)
    assert S == ref["n_survivors"] and S > 0
    better = lambda a, b: (count[a], -h[a]) > (count[b], -h[b])
    share = ((assign[:, None, :] == assign[None, :, :]) & (assign[:, None, :] >= 0)).sum(axis=2) >= params["shared"] if S <= 600 else None
    for seed in range(3):
        picked = {}
        rank = {int(x): r for r, x in enumerate(CC.order(count, h))}

        def is_picked(x):
            if x not in picked:
                row = share[x] if share is not None else ((assign == assign[x]) & (assign >= 0)).sum(axis=1) >= params["shared"]
                picked[x] = not any(is_picked(int(y)) for y in sorted(np.flatnonzero(row), key=rank.get) if y != x and better(y, x))
            return picked[x]

        for x in np.random.default_rng(seed).permutation(S):
            is_picked(int(x))
        picks = sorted((x for x, yes in picked.items() if yes), key=rank.get)[:params["n_poses"]]
        assert [int(h[x]) for x in picks] == ref["hyp"][:ref["found"]].tolist(), seed
        assert len(picks) == ref["found"]


@pytest.mark.parametrize("name", CC.REFIT_CASES)
def test_horn_against_kabsch_and_the_gaps_of_the_refit_cases(name):
    cs, _ = CC.case(name)
    ref = CC.reference(name)
    assert ref["found"] >= 1
    for r in range(ref["found"]):
        pp, cc = CC.pairs_of(cs, ref["sel_assign"][r])
        assert len(pp) == ref["inliers"][r] >= 3
        R, t, lam, N = CC.horn(pp, cc)
        Rk, tk = CC.kabsch(pp, cc)
        assert np.abs(R - Rk).max() < 1e-9 and np.abs(t - tk).max() < 1e-9 and np.abs(N - N.T).max() == 0 and abs(np.trace(N)) < 1e-12
        bound, gap = CC.refit_bound(pp, cc)
        assert gap >= CC.MIN_GAP and bound < 1e-6, (r, gap, bound)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_exact_refit_case_is_exact(axis):
    p, c, R, t = CC.exact_refit_case(axis)
    Rh, th, lam, N = CC.horn(p, c[:, 0])
    assert np.abs(Rh - R).max() < 1e-15 and np.abs(th - t).max() < 1e-14
    assert np.array_equal(p.astype(np.float64) @ R.astype(np.float64).T + t, c[:, 0])           # the image is exact: rmse == 0 is attainable
    a, b = [(0, 1), (0, 2), (0, 3)][axis]
    off = [(i, j) for i in range(4) for j in range(i + 1, 4) if N[i, j] != 0]
    assert N[a, a] == N[b, b] and N[a, b] > 0 and (a, b) in off and all({i, j}.isdisjoint({a, b}) for i, j in off if (i, j) != (a, b))


# ---- the planted facts of the case set ------------------------------------------------------------------------------------------------------
def test_planted_facts():
    # an exact rigid image plus decoys: every point is an inlier at rank 0, and equal counts resolve to the lower h
    for name in ("m3k1", "m4k2", "m5k3", "m17k1_t64", "m17k2_t65", "m33k1", "duplicates"):
        cs, _ = CC.case(name)
        ref = CC.reference(name)
        M = len(cs["p"])
        assert ref["inliers"][0] == M and np.array_equal(ref["sel_assign"][0, :M], cs["digit"]), name
        assert ref["hyp"][0] == np.flatnonzero(ref["count"] == ref["count"].max())[0], name
        R, t, _ = cs["motions"][0]
        assert np.abs(ref["sel_pose"][0, :9].reshape(3, 3) - R).max() < 1e-5 and np.abs(ref["sel_pose"][0, 9:] - t).max() < 1e-5, name
    assert (CC.reference("m33k1")["count"] == 33).sum() > 2048                # more live hypotheses than a score workgroup takes: the queue wraps
    # two planted objects: two poses, the planted counts at ranks 0 and 1, their members assigned
    cs, _ = CC.case("two_objects")
    ref = CC.reference("two_objects")
    assert ref["found"] == 2 and ref["inliers"][:2].tolist() == [14, 9]
    for r, (R, t, idx) in enumerate(cs["motions"]):
        assert np.array_equal(np.flatnonzero(ref["sel_assign"][r] >= 0), idx) and np.array_equal(ref["sel_assign"][r, idx], cs["digit"][idx])
    # collinear model points and an all-NaN candidate table: zero poses
    for name in ("collinear", "all_nan"):
        ref = CC.reference(name)
        assert ref["found"] == 0 and ref["n_gated"] == 0 and ref["n_survivors"] == 0 and (ref["hyp"] == -1).all() and np.isnan(ref["sel_pose"]).all(), name
    # NaN rows are never assigned
    cs, _ = CC.case("m17k3")
    ref = CC.scored("m17k3")
    nan_rows = np.isnan(cs["c"]).any(axis=2)
    assert nan_rows.any() and not nan_rows[np.arange(17)[None, :], np.maximum(ref["assign"], 0)][ref["assign"] >= 0].any()
    # duplicate candidates resolve to the lower digit
    cs, _ = CC.case("duplicates")
    ref = CC.scored("duplicates")
    assert np.array_equal(cs["c"][:, 0], cs["c"][:, 1]) and (ref["assign"] == 0).any() and not (ref["assign"] == 1).any()
    # the max_survivors cut falls inside a run of equal counts: more hypotheses have the count at the cut than are kept of it
    for name, kept in (("m17k3_cut7", 7), ("m17k3_cut1", 1)):
        ref = CC.reference(name)
        h = ref["survivors"]
        cut = ref["count"][h].min()
        assert len(h) == kept and (ref["count"] == cut).sum() > (ref["count"][h] == cut).sum() >= 1
        assert np.array_equal(h[ref["count"][h] == cut], np.flatnonzero(ref["count"] == cut)[:(ref["count"][h] == cut).sum()])       # the lowest h of the run
    # n_poses = 64 is more than there are distinct poses: the rounds stop early
    assert 2 < CC.reference("m17k3")["found"] < 64 and 2 < CC.reference("m64k2")["found"] < 64


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def _scene_error(points):
    s = CC.scene()
    return float(np.linalg.norm(points.astype(np.float64) - s["x"].astype(np.float64), axis=1).max() / VC.STEP)


def test_the_restated_chain_recovers_the_pose_and_align_alone_does_not():
    s = CC.scene()
    angle = np.degrees(np.arccos((np.trace(s["R"].astype(np.float64)) - 1) / 2))
    moved = np.linalg.norm(s["x"].astype(np.float64).mean(0) - s["p"].astype(np.float64).mean(0)) / VC.STEP
    assert abs(angle - 60.0) < 1e-3 and abs(moved - 4.0) < 1e-3 and len(s["p"]) == CC.SCENE_M and int(s["present"].sum()) == CC.SCENE_M - 3
    refined = CC.locate_ref(s["vol"], "feat", s["targets"], CC.SCENE_K, CC.SCENE_RADIUS)
    d = np.linalg.norm(refined - s["x"].astype(np.float64)[:, None, :], axis=2) / VC.STEP
    with np.errstate(invalid="ignore"):
        nearest = np.nanmin(d, axis=1)
    assert (nearest[s["present"]] < 0.5).all() and (nearest[~s["present"]] > 2.0).all()       # the true image is among the k candidates of each present keypoint only
    tau = 2 * float(VC.STEP)
    poses, inliers, assign = CC.consensus_ref(s["p"], refined.astype(F), tau)
    assert inliers[0] >= int(s["present"].sum()) and inliers[1] < inliers[0] and (assign[0][s["present"]] >= 0).all()
    start = AC.transform32(poses[0][:9].reshape(3, 3), poses[0][9:], s["p"])
    fit = AC.align_ref(s["vol"], None, "feat", s["p"], poses[0][:9].reshape(3, 3), poses[0][9:], targets=s["targets"])
    print("start error", _scene_error(start), "final", _scene_error(fit["points"]), "status", fit["status"], "steps", fit["steps"])
    assert _scene_error(start) < 1.0 and fit["status"] == AC.CONVERGED and _scene_error(fit["points"]) < 0.1 / 4      # (a quarter of the device test's bound)
    alone = AC.align_ref(s["vol"], None, "feat", s["p"], np.eye(3, dtype=F), np.zeros(3, F), targets=s["targets"])
    assert not (alone["status"] == AC.CONVERGED and _scene_error(alone["points"]) < 0.1)
