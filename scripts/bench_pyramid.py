"""Times the pyramid of a baked field and the seeded flow (d3f_volume_coarsen_select / d3f_volume_coarsen_rows, csrc/pyramid_kernels.hip;
d3f_volume_flow_seeded, csrc/flow_seeded_kernels.hip; BakedField.coarsen / flow(seed=) / flow_pyramid) on the synthetic smooth scene (needs an
MI355X) and writes profiles/pyramid/results.txt.  No thresholds: the file reports, nothing is asserted.

Volume: the 200 x 175 x 55 bake (4 mm), dense, with the two fields of scripts/bench_flow.py (three prototypes plus noise; the second field is
the first rolled by one voxel along z plus noise) at C = 384 and C = 64.  Contenders, ALTERNATED inside one run, each timed --runs times with
device events after a warm-up round; medians (min, max):

    coarsen          BakedField.coarsen as a whole: the allocations, select, rows
    clone            a bare clone() of the fine rows it reads: the memory bound of reading them once (coarsen writes an eighth of that)
    flow r / seeded r   flow(refine=False) at radius r against flow(seed=zeros, refine=False) at the same radius, r = 1 and 2: the LDS-staged kernel
                     against one lane per candidate on the same work, with the same bytes out
    flow r=4         flow(radius_voxels=4), with its axis costs
    flow_pyramid     flow_pyramid(levels=2, radius_voxels=2) end to end: two coarsens per field, one flow at r = 2 on 1/64 of the voxels, two
                     seeded flows at r = 1, two Flow.seed in torch

    python scripts/bench_pyramid.py [--runs 7] [--out profiles/pyramid/results.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit     # noqa: E402
from bench_pool import with_set     # noqa: E402
from bench_warp import timed     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid", "results.txt"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five repetitions, so that the spread is visible"
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    step = 0.004
    base = f.bake(synth.WORK_BOX, step, return_names=[])
    nx, ny, nz = base.grid_shape
    n = nx * ny * nz
    lines = ["pyramid of a baked field and seeded flow (d3f_volume_coarsen_select, d3f_volume_coarsen_rows, d3f_volume_flow_seeded), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, ONE run of this script; device events, the contenders alternated, median of %d calls each after one warm-up round (min, max); "
             "scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W),
             "%d x %d x %d = %.2f M voxels (step %g m), dense; nothing was tuned: the seeded kernel is its first form" % (nx, ny, nz, n / 1e6, step), ""]
    for C in (384, 64):
        gen = torch.Generator(device=dev).manual_seed(17)
        proto = torch.randn((3, C), device=dev, generator=gen)
        dense_a = proto[torch.randint(0, 3, (n,), device=dev, generator=gen)] + 0.2 * torch.randn((n, C), device=dev, generator=gen)
        dense_b = torch.roll(dense_a.view(nx, ny, nz, C), 1, dims=2).reshape(n, C) + 0.1 * torch.randn((n, C), device=dev, generator=gen)
        A, B = with_set(base, "feat", dense_a.view(nx, ny, nz, C)), with_set(base, "feat", dense_b.view(nx, ny, nz, C))
        del dense_a, dense_b
        members = int(A._members(A._site_mask("bench", step, "free", None)).sum())
        zero = torch.zeros((nx, ny, nz, 3), dtype=torch.int32, device=dev)
        rows = A._sets["feat"]
        contenders = {"coarsen": lambda: A.coarsen(), "clone": lambda: rows.clone()}
        for r in (1, 2):
            contenders["flow r=%d" % r] = lambda r=r: A.flow(B, "feat", radius_voxels=r, iso=step, refine=False)
            contenders["seeded r=%d" % r] = lambda r=r: A.flow(B, "feat", radius_voxels=r, iso=step, refine=False, seed=zero)
        contenders["flow r=4"] = lambda: A.flow(B, "feat", radius_voxels=4, iso=step)
        contenders["flow_pyramid"] = lambda: A.flow_pyramid(B, "feat", levels=2, radius_voxels=2, iso=step)
        times = {k: [] for k in contenders}
        for rnd in range(args.runs + 1):                             # round 0 warms up
            for k, fn in contenders.items():
                t = timed(fn)
                if rnd > 0:
                    times[k].append(t)
        for r in (1, 2):                                             # what was timed is the same answer
            plain, seeded = contenders["flow r=%d" % r](), contenders["seeded r=%d" % r]()
            assert torch.equal(plain.target, seeded.target) and torch.equal(plain.cost, seeded.cost)
        chain = contenders["flow_pyramid"]()
        coarse = A.coarsen()
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append("C = %d: %.2f GB of fine rows per field, %d members; coarse grid %s, %d of its voxels valid; flow_pyramid matched %d, offset (0, 0, 1) at %d"
                     % (C, n * C * 4 / 1e9, members, tuple(coarse.grid_shape), int(coarse.valid.sum()), int(chain.matched.sum()),
                        int((chain.voxel_offset[chain.matched] == torch.tensor([0, 0, 1], dtype=torch.int32, device=dev)).all(1).sum())))
        for k, v in times.items():
            lines.append("    %-12s %9.3f ms (min %.3f, max %.3f)" % (k, med[k], min(v), max(v)))
        lines.append("    coarsen / clone = %.2f;  seeded / flow at r = 1: %.2f, at r = 2: %.2f;  flow r=4 / flow_pyramid = %.2f"
                     % (med["coarsen"] / med["clone"], med["seeded r=1"] / med["flow r=1"], med["seeded r=2"] / med["flow r=2"], med["flow r=4"] / med["flow_pyramid"]))
        lines.append("")
        del A, B, rows, contenders, chain, coarse, zero
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
