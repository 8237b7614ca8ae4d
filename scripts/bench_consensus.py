"""Times the consensus poses (d3f_pose_consensus_* / d3f_pose_refit, csrc/consensus_kernels.hip; consensus.consensus_poses, BakedField.relocate) on an
MI355X and writes profiles/consensus/results.txt.  One run, no thresholds: the file reports, nothing is asserted, and nothing was tuned.

Method of scripts/bench_peaks.py: HIP events on the stream round the call, median of --runs runs after warm-up; the header carries the date, the
commit and the shader clock.  Part 1, planted candidates: M = 16 / 32 / 64 model points in the unit box, k = 4 / 8 candidates each, half of the
keypoints follow one planted motion (their image at a random digit, decoys at the others), the other half are outlier keypoints; all C(M, 3)
triplets, tau = 0.03.  Per line, measured in the same run:

    score       d3f_pose_consensus_score alone (no debug outputs), with the share of hypotheses that pass the gate, and the VALU floor of its
                second phase: live hypotheses x M (12 + 11 k) float32 operations (source-level count: 12 per point for the pose chain and the
                bookkeeping, 11 per candidate) as wave instructions of 2 cycles on 1024 SIMDs at the nominal clock
    poses       the whole consensus_poses call (score, select, refit and the Python around them)
    torch       the same counts by broadcasting in torch -- gate and pose in float64, the [chunk, M, k] distances in float32, chunked so that one
                chunk's distances stay under 1 GiB; code that needs nothing of this feature.  Timed once, after one warm-up call.

Part 2, relocate against the many-starts recipe of INTEGRATION.md 1m on the bench scene (synth smooth, the 64-component head baked at 4 mm):
32 shell points as the model, their descriptors sampled from the field; the model is turned by 20 / 45 / 90 degrees about a random axis through
its centroid and shifted by 4 voxels, 8 planted poses per angle; a pose counts as recovered when the best CONVERGED instance leaves every
point within one voxel of its place.

    python scripts/bench_consensus.py [--runs 5] [--out profiles/consensus/results.txt]
"""
import argparse
import datetime
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, _lib, consensus, synth     # noqa: E402
from d3fields_amd.rigid import so3_exp_map     # noqa: E402

TAU = 0.03
STEP = 0.004
SIMDS = 1024


def fmt(t):
    return "median %9.4f ms (min %.4f, max %.4f)" % t


def planted(M, k, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (M, 3))
    c = rng.uniform(-1.0, 1.0, (M, k, 3))
    idx = rng.permutation(M)[:M // 2]
    w = rng.standard_normal(3)
    R = so3_exp_map(torch.from_numpy(w / np.linalg.norm(w) * 1.2)[None].float())[0].double().numpy()
    c[idx, rng.integers(0, k, len(idx))] = p[idx] @ R + rng.uniform(-0.3, 0.3, 3)
    return p.astype(np.float32), c.astype(np.float32)


def _norm2(x):
    return (x * x).sum(-1)


def torch_counts(p, c, trip, tau, chunk_bytes=1 << 30):
    """the count of every hypothesis by broadcasting: gate and pose in float64, distances in float32 -> (count uint8 [T], live)"""
    M, k = c.shape[:2]
    T = trip.shape[0] * k ** 3
    chunk = max(1, chunk_bytes // (M * k * 4 * 8))          # the [chunk, M, k, 3] differences, their squares and the sums
    out = torch.zeros(T, dtype=torch.uint8, device=p.device)
    live_total = 0
    pd, cd = p.double(), c.double()
    for lo in range(0, T, chunk):
        h = torch.arange(lo, min(T, lo + chunk), device=p.device)
        tr, rem = h // k ** 3, h % k ** 3
        i, j, l = trip[tr, 0].long(), trip[tr, 1].long(), trip[tr, 2].long()
        ci, cj, cl = cd[i, rem // (k * k)], cd[j, (rem // k) % k], cd[l, rem % k]
        pi, pj, pl = pd[i], pd[j], pd[l]
        u, v, U, V = pj - pi, pl - pi, cj - ci, cl - ci
        mu, mv, mw = _norm2(u).sqrt(), _norm2(v).sqrt(), _norm2(v - u).sqrt()
        oU, oV, oW = _norm2(U).sqrt(), _norm2(V).sqrt(), _norm2(V - U).sqrt()
        n, N = torch.linalg.cross(u, v), torch.linalg.cross(U, V)
        live = (mu >= 4 * tau) & (mv >= 4 * tau) & (mw >= 4 * tau) & ((oU - mu).abs() <= 2 * tau) & ((oV - mv).abs() <= 2 * tau) & ((oW - mw).abs() <= 2 * tau)
        live &= (_norm2(n) >= 0.04 * _norm2(u) * _norm2(v)) & (_norm2(N) >= 0.04 * _norm2(U) * _norm2(V))
        sel = live.nonzero()[:, 0]
        live_total += int(sel.numel())
        if sel.numel() == 0:
            continue
        u, U, n, N = u[sel], U[sel], n[sel], N[sel]
        e1, e3 = u / mu[sel, None], n / _norm2(n).sqrt()[:, None]
        f1, f3 = U / oU[sel, None], N / _norm2(N).sqrt()[:, None]
        e2, f2 = torch.linalg.cross(e3, e1), torch.linalg.cross(f3, f1)
        R = f1[:, :, None] * e1[:, None, :] + f2[:, :, None] * e2[:, None, :] + f3[:, :, None] * e3[:, None, :]
        t = (ci[sel] + cj[sel] + cl[sel]) / 3 - (R @ ((pi[sel] + pj[sel] + pl[sel]) / 3)[:, :, None])[:, :, 0]
        x = (p[None] @ R.float().transpose(1, 2)) + t.float()[:, None, :]
        d2 = ((x[:, :, None, :] - c[None]) ** 2).sum(-1)
        out[h[sel]] = (d2 <= tau * tau).any(dim=2).sum(dim=1).to(torch.uint8)
    return out, live_total


def part_one(lines, runs, dev, flush):
    lib = _lib.load()
    try:
        clock_hz = torch.cuda.get_device_properties(0).clock_rate * 1e3
    except (AttributeError, RuntimeError):
        clock_hz = 2.4e9
    for M in (16, 32, 64):
        for k in (4, 8):
            p_np, c_np = planted(M, k, 100 * M + k)
            p, c = torch.from_numpy(p_np).to(dev), torch.from_numpy(c_np).to(dev)
            table = np.array(consensus.all_triplets(M), dtype=np.int32)
            trip = torch.from_numpy(table).to(dev)
            n_trip = len(table)
            T = n_trip * k ** 3
            ws_bytes = int(lib.d3f_pose_consensus_workspace_bytes(M, k, n_trip, 65536))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            count = torch.empty(T, dtype=torch.uint8, device=dev)
            tau2 = float(np.float32(TAU) * np.float32(TAU))

            def score():
                _lib.check(lib.d3f_pose_consensus_score(_lib.ptr(p), _lib.ptr(c), M, k, _lib.ptr(trip), table.ctypes.data, n_trip, tau2, 2 * TAU, 4 * TAU, 0.2,
                                                        _lib.ptr(count), None, None, _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(dev)))

            t_score = median_ms(score, runs, 1)
            out = consensus.consensus_poses(p, c, TAU)
            t_all = median_ms(lambda: consensus.consensus_poses(p, c, TAU), runs, 1)
            ref = []
            t_torch = median_ms(lambda: ref.append(torch_counts(p, c, trip, TAU)), 1, 1, warmup=1)
            live = int(out["n_gated"])
            agree = float((ref[-1][0] == count).float().mean())
            floor_ms = live / 64.0 * M * (12 + 11 * k) * 2 / (SIMDS * clock_hz) * 1e3
            lines.append("M = %2d, k = %d: %9d hypotheses, %7d pass the gate (%.3f %%), %d survivors, best pose %d of %d planted inliers" % (
                M, k, T, live, 100.0 * live / T, int(out["n_survivors"]), int(out["inliers"][0]), M // 2))
            lines.append("    score %s; phase-2 VALU floor %.4f ms; consensus_poses %s; torch broadcast %9.2f ms (counts agree on %.4f %% of the hypotheses)"
                         % (fmt(t_score), floor_ms, fmt(t_all), t_torch[0], 100 * agree))
            flush()
            del ws, count, ref
            torch.cuda.empty_cache()


def part_two(lines, dev, flush):
    gen = torch.Generator().manual_seed(0)
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, 384, seed=1).to(dev)
    f.H, f.W = H, W
    f.add_projection("head64", components=torch.randn(64, 384, generator=torch.Generator().manual_seed(3)))
    _, shell = f.grid_shell(synth.WORK_BOX, STEP)
    field = f.bake(synth.WORK_BOX, STEP, return_names=["head64"])
    x = shell[torch.randperm(shell.shape[0], generator=gen)[:32].to(dev)].contiguous()
    with torch.no_grad():
        targets = field.eval(x, return_names=["head64"])["head64"].contiguous()
    centre = x.mean(dim=0)
    lines.append("")
    lines.append("relocate against the many-starts recipe (INTEGRATION.md 1m: the k candidates of keypoint 0 as pure translations): %d x %d x %d at %g m, C = 64, "
                 "32 keypoints, k = 4, 8 planted poses per angle, recovered = best CONVERGED instance within one voxel at every point" % (*field.grid_shape, STEP))
    for deg in (20, 45, 90):
        got = {"relocate": 0, "recipe": 0}
        for trial in range(8):
            axis = torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0)
            rot = so3_exp_map((axis * math.radians(deg))[None])[0].to(dev)                      # row-vector convention: x = p @ rot + trans
            shift = torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0).to(dev) * (4 * STEP)
            trans = centre - centre @ rot + shift
            model = ((x - trans) @ rot.T).contiguous()                                       # the model at the identity: model @ rot + trans = x
            fit = field.relocate(model, "head64", targets, k=4, radius_voxels=2)
            best = int(fit["best"])
            if best >= 0 and float((fit["points"][best] - x).norm(dim=1).max()) < STEP:
                got["relocate"] += 1
            hits = field.locate(targets[:1], "head64", k=4, radius_voxels=2)["refined"][0].float()
            starts = torch.nan_to_num(hits - model[0], nan=0.0)
            many = field.align(model[None].expand(4, -1, -1), "head64", targets[None].expand(4, -1, -1), trans=starts.contiguous(), iters=20)
            cost = torch.where(many["status"] == 1, many["cost"], torch.full_like(many["cost"], float("inf")))
            b = int(torch.argmin(cost))
            if bool((many["status"] == 1).any()) and float((many["points"][b] - x).norm(dim=1).max()) < STEP:
                got["recipe"] += 1
        lines.append("    %2d degrees: relocate recovers %d of 8, the 1m recipe %d of 8" % (deg, got["relocate"], got["recipe"]))
        flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["consensus poses (d3f_pose_consensus_* / d3f_pose_refit; consensus_poses, BakedField.relocate), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, one run, nothing tuned; device times: HIP events round the call, median of %d runs after 3 warm-up calls (min, max); torch: one run after one warm-up call; "
             "planted candidates, half of the keypoints outliers, all C(M, 3) triplets, tau = %g, max_survivors 65536, n_poses 8" % (args.runs, TAU), ""]

    def flush():
        text = "\n".join(lines[:1] + [clock_line()] + lines[1:]) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        return text

    part_one(lines, args.runs, dev, flush)
    part_two(lines, dev, flush)
    print(flush())


if __name__ == "__main__":
    main()
