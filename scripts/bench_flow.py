"""Times the dense descriptor flow between two baked fields (d3f_volume_flow, csrc/flow_kernels.hip; BakedField.flow) on the synthetic smooth
scene (needs an MI355X) and writes profiles/flow/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_parts.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the commit and
the shader clock.  Configurations: the 200 x 175 x 55 bake (4 mm), dense and with a 5-mm band, with a set of 384 and of 64 channels, at
radius 1, 2 and 4.  Field A holds random rows (three prototypes plus noise); field B holds A's rows moved by one voxel along z plus noise,
so that the flow has something to find.  Sites are valid & dist <= one step on both sides.  Times are of flow(refine=False) -- the search
kernel alone -- and of flow(), which adds the axis-cost kernel and the torch arithmetic of the Flow object.  Next to them, in the same run:

    torch   the recipe flow() replaces, on dense fields only: per offset of the window a shifted difference of the two [nx, ny, nz, C] arrays,
            squared, summed, masked, and a running minimum (ties go to the lower j, not to the contract's key; the sums are torch's).  It
            works on every voxel of the volume, members or not, and makes one temporary of the row array's size per offset.  One run after
            one warm-up call at radius 1 and 2, one run without warm-up at radius 4.

    python scripts/bench_flow.py [--runs 5] [--out profiles/flow/results.txt]
"""
import argparse
import datetime
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from bench_pool import with_set     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402


def torch_flow(rows_a, rows_b, member_a, member_b, r):
    """the shift-loop recipe on two dense [nx, ny, nz, C] arrays -> (target int64, cost float32)"""
    nx, ny, nz, _ = rows_a.shape
    flat = torch.arange(nx * ny * nz, device=rows_a.device).view(nx, ny, nz)
    best = torch.full((nx, ny, nz), float("inf"), device=rows_a.device)
    target = torch.full((nx, ny, nz), -1, dtype=torch.int64, device=rows_a.device)
    for off in itertools.product(range(-r, r + 1), repeat=3):
        va = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip((nx, ny, nz), off))
        ub = tuple(slice(max(0, d), n - max(0, -d)) for n, d in zip((nx, ny, nz), off))
        s = (rows_a[va] - rows_b[ub]).square_().sum(-1)
        s = torch.where(member_a[va] & member_b[ub], s, torch.full_like(s, float("inf")))
        better = s < best[va]
        best[va] = torch.where(better, s, best[va])
        target[va] = torch.where(better, flat[ub], target[va])
    return target, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["dense descriptor flow (d3f_volume_flow), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, ONE run of this script; HIP events, median of %d runs after 3 warm-up calls (min, max); scene: synth smooth, %d views of %d x %d"
             % (args.runs, V, H, W), "nothing was tuned: tile, chunk width and sub-window widths are the first ones written down", ""]
    step = 0.004
    base = f.bake(synth.WORK_BOX, step, return_names=[])
    nx, ny, nz = base.grid_shape
    n = nx * ny * nz
    for band, C in ((None, 384), (0.005, 384), (None, 64), (0.005, 64)):
        mark = None if band is None else base._mark(band)
        rows_n = n if band is None else int(mark[2].shape[0])
        gen = torch.Generator(device=dev).manual_seed(17)
        proto = torch.randn((3, C), device=dev, generator=gen)
        dense_a = proto[torch.randint(0, 3, (n,), device=dev, generator=gen)] + 0.2 * torch.randn((n, C), device=dev, generator=gen)
        dense_b = torch.roll(dense_a.view(nx, ny, nz, C), 1, dims=2).reshape(n, C) + 0.1 * torch.randn((n, C), device=dev, generator=gen)
        if band is None:
            A, B = with_set(base, "feat", dense_a.view(nx, ny, nz, C)), with_set(base, "feat", dense_b.view(nx, ny, nz, C))
        else:
            idx = mark[2].long()
            A, B = with_set(base, "feat", dense_a.index_select(0, idx), mark, band), with_set(base, "feat", dense_b.index_select(0, idx), mark, band)
            del dense_a, dense_b
        members = A._members(A._site_mask("bench", step, "free", None))
        m = int(members.sum())
        lines.append("%s, C = %d: %d x %d x %d = %.2f M voxels, %d rows stored per field, %d members" % (
            "4-mm dense" if band is None else "4-mm grid, 5-mm band", C, nx, ny, nz, n / 1e6, rows_n, m))
        for r in (1, 2, 4):
            kmed, klo, khi = median_ms(lambda: A.flow(B, "feat", radius_voxels=r, iso=step, refine=False), args.runs, 1)
            fmed, flo, fhi = median_ms(lambda: A.flow(B, "feat", radius_voxels=r, iso=step), args.runs, 1)
            flow = A.flow(B, "feat", radius_voxels=r, iso=step)
            moved = int((flow.voxel_offset[flow.matched] == torch.tensor([0, 0, 1], dtype=torch.int32, device=dev)).all(1).sum())
            text = "    r = %d: flow(refine=False) %9.3f ms (min %.3f, max %.3f)    flow() %9.3f ms (min %.3f, max %.3f)    matched %d, offset (0, 0, 1) at %d" % (
                r, kmed, klo, khi, fmed, flo, fhi, int(flow.matched.sum()), moved)
            if band is None:
                tmed, _, _ = median_ms(lambda: torch_flow(A._sets["feat"], B._sets["feat"], members, members, r), 1, 1, warmup=1 if r < 4 else 0)
                text += "    torch shift loop, one run: %.3f ms (%.1f x the kernel)" % (tmed, tmed / kmed)
            else:
                text += "    torch shift loop: the rows are compacted, the recipe needs the dense [n, C] arrays (%.1f GB each)" % (4.0 * n * C / 1e9)
            lines.append(text)
            del flow
        lines.append("")
        del A, B, members
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
