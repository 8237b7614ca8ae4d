"""Times the grid segments and the row shortcuts (d3f_volume_segments, d3f_path_shorten, csrc/segment_kernels.hip; BakedField.straight /
shortcut) on the synthetic smooth scene (needs an MI355X) and writes profiles/straight/results.txt.  No thresholds: the file reports, nothing
is asserted.

Method of scripts/bench_geodesic.py: HIP events on the stream, median of --runs runs after warm-up at 4 mm and of a quarter as many at 1 mm;
the header carries the date, the commit and the shader clock.  Scene: the 4 mm bake of the work box and the 1 mm grid of the same box,
c = clearance(unknown="occupied", min_voxels=50), free = c.valid & (c.dist >= 0.03), t = c.travel(goal, free=free) with the free voxel nearest
to the middle of the box as the goal.  A call is timed as the method runs it, so the time includes the torch passes round the kernel (voxel
indices, centres of the last voxels, the float64 lengths).  Next to every time, measured in the same run:

    straight   2^20 random pairs of free voxels: the share of clear segments under the rule, the mean Euclidean length of a pair in voxels; on the
               travel field (free only) and on the clearance field (free and the minimum of d2)
    shortcut   the 4096 random paths that bench_geodesic.py times: anchors per path, distance / distance_before (mean over the paths longer than one
               voxel), the longest path, and the time of path() itself

    python scripts/bench_straight.py [--runs 20] [--steps 0.004,0.001] [--out profiles/straight/results.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402

RADIUS = 0.03
PAIRS = 1 << 20
PATHS = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", default="0.004,0.001")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "straight", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["straight segments and shortcuts (d3f_volume_segments, d3f_path_shorten; BakedField.straight / shortcut), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; device times: HIP events around the whole method call, median of %d runs after warm-up (a quarter as many from 2^24 voxels on; "
             "min, max); scene: synth smooth, %d views of %d x %d; free = clearance(unknown='occupied', min_voxels=50).dist >= %g; travel: connectivity 26, "
             "weights (3, 4, 5)" % (args.runs, V, H, W, RADIUS), ""]

    def flush():
        text = "\n".join(lines[:1] + [clock_line()] + lines[1:]) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        return text

    for step in [float(s) for s in args.steps.split(",")]:
        field = f.bake(synth.WORK_BOX, step, return_names=[])
        c = field.clearance(unknown="occupied", min_voxels=50)
        del field
        nx, ny, nz = c.grid_shape
        n = nx * ny * nz
        free = (c.valid & (c.dist >= RADIUS)).contiguous()
        idx = torch.nonzero(free)
        centre = torch.tensor([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2], device=dev)
        g = idx[torch.argmin(((idx.float() - centre) ** 2).sum(dim=1))]
        goal = ((g[0] * ny + g[1]) * nz + g[2]).to(torch.int32).reshape(1)
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 4)
        lines.append("%d x %d x %d = %.2f M voxels (step %g m), %d free (%.2f %%), goal voxel %s; device times here: median of %d runs"
                     % (nx, ny, nz, n / 1e6, step, idx.shape[0], 100.0 * idx.shape[0] / n, tuple(g.tolist()), runs))
        t = c.travel(goal, free=free)

        def flat(rows):
            return ((rows[:, 0] * ny + rows[:, 1]) * nz + rows[:, 2]).to(torch.int32)

        pa, pb = idx[torch.randint(idx.shape[0], (PAIRS,), device=dev)], idx[torch.randint(idx.shape[0], (PAIRS,), device=dev)]
        mean_len = float(torch.sqrt(((pa - pb) ** 2).sum(dim=1).double()).mean())
        a, b = flat(pa), flat(pb)
        del pa, pb
        for what, call in (("travel field, strict     ", lambda: t.straight(a, b)), ("travel field, cut corners", lambda: t.straight(a, b, cut_corners=True)),
                           ("clearance field + min d2 ", lambda: c.straight(a, b, free=free))):
            out = call()
            med, lo, hi = median_ms(call, runs, 1)
            text = "    straight, %d pairs of free voxels (mean length %.1f voxels), %s: median %9.4f ms (min %.4f, max %.4f); %.2f %% clear" % (
                PAIRS, mean_len, what, med, lo, hi, 100.0 * float(out["clear"].float().mean()))
            if "min_d2" in out:
                seen = out["min_d2"] != 2 ** 31 - 1
                text += "; mean clearance on the way %.4f m" % float(out["clearance"][seen].double().mean())
            lines.append(text)
            del out
            flush()
        starts = flat(idx[torch.randperm(idx.shape[0], device=dev)[:PATHS]])
        pmed, plo, phi = median_ms(lambda: t.path(starts), runs, 1)
        paths = t.path(starts)
        lines.append("    path of %d random free starts, max_steps %d: median %.4f ms (min %.4f, max %.4f); %d reached, longest %d voxels, mean %.1f"
                     % (PATHS, nx + ny + nz, pmed, plo, phi, int(paths["reached"].sum()), int(paths["length"].max()), float(paths["length"].float().mean())))
        for what, cut in (("strict     ", False), ("cut corners", True)):
            out = t.shortcut(paths, cut_corners=cut)
            med, lo, hi = median_ms(lambda: t.shortcut(paths, cut_corners=cut), runs, 1)
            moved = out["distance_before"] > 0
            ratio = out["distance"][moved] / out["distance_before"][moved]
            lines.append("    shortcut of those paths, %s: median %9.4f ms (min %.4f, max %.4f); %.2f anchors per path (most %d), distance / distance_before "
                         "mean %.4f (min %.4f, max %.4f)" % (what, med, lo, hi, float(out["length"].float().mean()), int(out["length"].max()), float(ratio.mean()),
                                                            float(ratio.min()), float(ratio.max())))
            del out
            flush()
        lines.append("")
        flush()
        del c, t, free, idx, paths, a, b, starts
        torch.cuda.empty_cache()
    print(flush())


if __name__ == "__main__":
    main()
