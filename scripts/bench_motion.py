"""Times the rigid motion per part (d3f_part_motion, csrc/motion_kernels.hip; Flow.motions) on the synthetic smooth scene (needs an MI355X)
and writes profiles/motion/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_pool.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the commit and
the shader clock.  Volumes: the 200 x 175 x 55 bake (4 mm, dense) and the 1 mm grid of the same box in a band of two steps.  The field holds
one 4-channel set, the one-hot of four slabs along x, so that parts('mask', rule='argmax') cuts the occupied shell into the connected pieces
of each slab.  The flow is planted, not searched: every part turns by up to 10 degrees about its box centre and shifts by up to 2 voxels,
target is the rounded image (clipped to the grid), offset the remainder, and one pair in five is an outlier moved by 3 or 4 voxels per
axis; `keep` passes 9 voxels in 10.  Timed, in the same run:

    call     flow.motions(parts, keep=keep): fits = 3, tau = 1 voxel, min_pairs = 8 -- the capacity read, the workspace and the kernels
    chain    parts('mask', rule='argmax') followed by that call
    recipe   what the call replaces, in torch, for the --top largest parts only: per part a mask over the volume, a gather, and three
             rounds of torch.linalg.svd Kabsch with a trim at tau in between.  The call handles every part.

    python scripts/bench_motion.py [--runs 10] [--steps 0.004,0.001] [--out profiles/motion/results.txt]
"""
import argparse
import datetime
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from bench_pool import with_set     # noqa: E402
from d3fields_amd import Flow, Fusion, synth     # noqa: E402
from d3fields_amd.baked import _voxel_coords     # noqa: E402


def planted_flow(parts, gen):
    """a Flow whose matches follow one planted rigid motion per part (plus outliers), made with torch on the member voxels only"""
    dev = parts.labels.device
    shape = parts.grid_shape
    n = parts.labels.numel()
    K = parts.count
    vox = (parts.labels.view(-1) > 0).nonzero().view(-1)
    k = parts.labels.view(-1)[vox].long() - 1
    axis = torch.nn.functional.normalize(torch.randn((K, 3), dtype=torch.float64, device=dev, generator=gen), dim=1)
    angle = math.radians(10.0) * torch.rand((K,), dtype=torch.float64, device=dev, generator=gen)
    x, y, z = axis.unbind(1)
    zero = torch.zeros_like(x)
    skew = torch.stack((zero, -z, y, z, zero, -x, -y, x, zero), dim=1).view(K, 3, 3)
    rot = torch.eye(3, dtype=torch.float64, device=dev) + angle.sin()[:, None, None] * skew + (1 - angle.cos())[:, None, None] * (skew @ skew)
    centre = 0.5 * (parts.box_lo + parts.box_hi).double()
    shift = 4.0 * torch.rand((K, 3), dtype=torch.float64, device=dev, generator=gen) - 2.0
    p = _voxel_coords(vox, shape).double()
    q = ((rot[k] @ (p - centre[k])[:, :, None])[:, :, 0] + centre[k]) + shift[k]
    out = torch.rand(vox.shape[0], device=dev, generator=gen) < 0.2
    jump = torch.randint(3, 5, (vox.shape[0], 3), device=dev, generator=gen) * (2 * torch.randint(0, 2, (vox.shape[0], 3), device=dev, generator=gen) - 1)
    q = q + out[:, None] * jump
    hi = torch.tensor(shape, device=dev) - 1
    t = torch.minimum(torch.clamp(q.round(), min=0).long(), hi)
    target = torch.full((n,), -1, dtype=torch.int32, device=dev)
    target[vox] = ((t[:, 0] * shape[1] + t[:, 1]) * shape[2] + t[:, 2]).to(torch.int32)
    offset = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    offset[vox] = q - t
    flow = Flow(parts.origin, parts.step, target.view(shape), torch.zeros(shape, dtype=torch.float32, device=dev))
    flow.offset = offset.view(tuple(shape) + (3,))
    truth = torch.zeros(n, dtype=torch.bool, device=dev)
    truth[vox] = ~out
    return flow, truth.view(shape)


def torch_recipe(flow, parts, keep, ids, tau2=1.0, fits=3, min_pairs=8):
    """per part: a mask, a gather, SVD-Kabsch, three trims -> the rotations found"""
    shape = flow.grid_shape
    found = []
    for k in ids:
        idx = ((parts.labels == k) & keep & flow.matched).view(-1).nonzero().view(-1)
        a = _voxel_coords(idx, shape).double()
        b = _voxel_coords(flow.target.view(-1)[idx], shape).double() + flow.offset.view(-1, 3)[idx]
        use = torch.ones(idx.shape[0], dtype=torch.bool, device=idx.device)
        R = None
        for _ in range(fits):
            if int(use.sum()) < min_pairs:
                break
            pa, pb = a[use], b[use]
            pm, cm = pa.mean(0), pb.mean(0)
            U, _, Vt = torch.linalg.svd((pa - pm).T @ (pb - cm))
            d = torch.sign(torch.linalg.det(Vt.T @ U.T))
            R = Vt.T @ torch.diag(torch.stack((torch.ones_like(d), torch.ones_like(d), d))) @ U.T
            use = (((a - pm) @ R.T - (b - cm)) ** 2).sum(1) <= tau2
        found.append(R)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--steps", default="0.004,0.001")
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["rigid motion per part (d3f_part_motion), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, ONE run of this script; HIP events, median of %d runs after 3 warm-up calls (a third as many from 2^24 voxels on; min, max); "
             "scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W), "nothing was tuned: the first form written down", ""]
    gen = torch.Generator(device=dev).manual_seed(17)
    for step in [float(s) for s in args.steps.split(",")]:
        base = f.bake(synth.WORK_BOX, step, return_names=[])
        nx, ny, nz = base.grid_shape
        n = nx * ny * nz
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 3)
        slab = (torch.arange(nx, device=dev) * 4 // nx).view(nx, 1, 1).expand(nx, ny, nz).reshape(-1)
        if n < (1 << 24):
            kind = "dense"
            field = with_set(base, "mask", torch.nn.functional.one_hot(slab, 4).float().view(nx, ny, nz, 4))
        else:
            kind = "band of two steps"
            mark = base._mark(2.0 * step)
            field = with_set(base, "mask", torch.nn.functional.one_hot(slab[mark[2].long()], 4).float(), mark, 2.0 * step)
        del slab
        make_parts = lambda: field.parts("mask", rule="argmax", iso=step, min_voxels=30)
        parts = make_parts()
        flow, truth = planted_flow(parts, gen)
        keep = torch.rand((nx, ny, nz), device=dev, generator=gen) < 0.9
        pm = flow.motions(parts, keep=keep)
        sizes = pm.pairs.long()
        exact = int(((pm.inlier == (truth & keep)) | (parts.labels == 0)).all())
        lines.append("%d x %d x %d = %.2f M voxels (step %g m, %s): K %d parts, %d pairs (largest %d, median %d); status ok / thinned / too few: %d / %d / %d; "
                     "the inlier volume %s the planted one" % (nx, ny, nz, n / 1e6, step, kind, parts.count, int(sizes.sum()), int(sizes.max()), int(sizes.median()),
                                                               int((pm.status == pm.OK).sum()), int((pm.status == pm.THINNED).sum()),
                                                               int((pm.status == pm.TOO_FEW).sum()), "equals" if exact else "DIFFERS FROM"))
        cmed, clo, chi = median_ms(lambda: flow.motions(parts, keep=keep), runs, 1)
        pmed, plo, phi = median_ms(lambda: flow.motions(make_parts(), keep=keep), runs, 1)
        top = parts.largest(args.top).tolist()
        rmed, rlo, rhi = median_ms(lambda: torch_recipe(flow, parts, keep, top), max(1, runs // 3), 1, warmup=1)
        lines.append("    call %9.3f ms (min %.3f, max %.3f)    parts + call %9.3f ms (min %.3f, max %.3f)    torch recipe, the %d largest parts of %d only: "
                     "%9.3f ms (min %.3f, max %.3f) = %.1f x the call" % (cmed, clo, chi, pmed, plo, phi, len(top), parts.count, rmed, rlo, rhi, rmed / cmed))
        lines.append("")
        del field, parts, flow, truth, keep, pm, base
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
