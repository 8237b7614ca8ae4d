"""Times the baked-volume lookup (BakedField, csrc/volume_kernels.hip) on the synthetic smooth scene (needs an MI355X) and writes
profiles/volume/results.txt.  No thresholds: the file reports, nothing is asserted.

Volume: the 200 x 175 x 55 grid (4 mm) of the reference's vis_repr.py:88, baked with `dist` only, with a 3-component head and
with a 384-channel set.  Points: the ~71 k grid points of the surface shell (Fusion.grid_shell) and a 1 M random cloud.
Per case, median of --runs runs after warm-up, HIP events on the stream around --reps back-to-back calls:

    baked_fwd      BakedField.eval
    baked_fwd_bwd  BakedField.eval with pts.requires_grad + backward of sum(dist) + sum(rows)
    fusion_eval    Fusion.eval of the same points and names (re-projects every point into the V views)
    copy_floor     a bare device copy of the bytes a perfect cache would move: every touched corner row once + the outputs

The clock line is what the box reports right after the timed loops, to tell a down-clocked box from a slow kernel.

    python scripts/bench_volume.py [--runs 20] [--out profiles/volume/results.txt]
"""
import argparse
import datetime
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3fields_amd import Fusion, synth     # noqa: E402


def median_ms(fn, runs, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times), min(times), max(times)


def touched_rows(field, pts):
    """number of distinct voxels the valid points' cells touch"""
    nx, ny, nz = field.grid_shape
    o = torch.tensor(field.origin, device=pts.device)
    g = (pts - o) / field.step
    inside = ((g >= 0) & (g <= torch.tensor([nx - 1, ny - 1, nz - 1], device=pts.device))).all(1)
    i = torch.minimum(g[inside].floor().long(), torch.tensor([nx - 2, ny - 2, nz - 2], device=pts.device))
    flat = (i[:, 0] * ny + i[:, 1]) * nz + i[:, 2]
    offs = torch.tensor([dx * ny * nz + dy * nz + dz for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], device=pts.device)
    return int(torch.unique((flat[:, None] + offs[None, :]).reshape(-1)).numel())


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown (no git)"
    except OSError:
        return "unknown (no git)"


def clock_line():
    """the shader clock the box reports right after the timed loops (a read-only query), next to the nominal maximum: tells a
    throttled or down-clocked box from a slow kernel"""
    try:
        nominal = "%d MHz" % (torch.cuda.get_device_properties(0).clock_rate // 1000)
    except (AttributeError, RuntimeError):
        nominal = "unknown"
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        sclk = [ln.split(":")[-1].strip() for ln in out.splitlines() if "sclk" in ln]
        measured = sclk[0] if sclk else "not reported"
    except (OSError, subprocess.SubprocessError):
        measured = "not reported (no rocm-smi)"
    return "shader clock after the timed loops: %s; nominal maximum %s" % (measured, nominal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, 384, seed=1).to(dev)
    f.H, f.W = H, W
    f.add_projection("pca3", components=torch.randn(3, 384, generator=torch.Generator().manual_seed(2)))
    step = 0.004
    _, shell = f.grid_shell(synth.WORK_BOX, step)
    cloud = synth.random_cloud(1000000, seed=3).to(dev)
    lines = ["baked-volume lookup, %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "HIP events, median of %d runs after warm-up (min, max); scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W), ""]
    for label, names in (("dist only", []), ("3-component head", ["pca3"]), ("384 channels", ["dino_feats"])):
        baked = f.bake(synth.WORK_BOX, step, return_names=names)
        nx, ny, nz = baked.grid_shape
        C = sum(baked._sets[k].shape[3] for k in names)
        for pname, pts in (("surface shell", shell), ("random cloud", cloud)):
            n = pts.shape[0]
            reps = 10 if n < 200000 else 2

            def fwd():
                with torch.no_grad():
                    return baked.eval(pts, return_names=names)

            def fwd_bwd():
                p = pts.detach().requires_grad_(True)
                out = baked.eval(p, return_names=names)
                loss = out["dist"].sum()
                for k in names:
                    loss = loss + out[k].sum()
                loss.backward()

            def fusion_eval():
                with torch.no_grad():
                    return f.eval(pts, return_names=names)

            valid = float(fwd()["valid_mask"].float().mean())
            rows = touched_rows(baked, pts)
            nbytes = rows * 4 * (1 + C) + n * (4 + 1 + 4 * C) + n * 12
            src = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev)      # a copy reads and writes its size: nbytes of traffic in all
            dst = torch.empty_like(src)
            res = {"baked_fwd": median_ms(fwd, args.runs, reps), "baked_fwd_bwd": median_ms(fwd_bwd, args.runs, reps),
                   "fusion_eval": median_ms(fusion_eval, args.runs, reps), "copy_floor": median_ms(lambda: dst.copy_(src), args.runs, reps)}
            lines.append("%d x %d x %d, %s, %s: %d points, %.1f %% valid, %d touched voxels, %.1f MB algorithmic"
                         % (nx, ny, nz, label, pname, n, 100 * valid, rows, nbytes / 1e6))
            for k, (med, lo, hi) in res.items():
                lines.append("    %-14s median %9.4f ms   (min %.4f, max %.4f)   x copy_floor %.2f" % (k, med, lo, hi, med / res["copy_floor"][0]))
            del src, dst
        del baked
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
