"""Where is it now?  The first observation moved by the rigid motions of its parts (needs an MI355X; no reference code, no network):

    the scene of examples/flow_synthetic.py   two bakes of the synthetic scene, ONE sphere moved by a few voxels (and turned) in between
    parts, flow both ways, consistent, motions  as there: one rigid motion per part of the first bake
    a.owners(parts, margin_voxels=2)          every voxel near a part travels with it: the free side of its surface comes along
    a.warp(pm, owner, which=pm.moved(...))    the first bake as it would look after the parts that moved have moved: an ordinary field

and prints how well the occupied voxels of the first bake, before and after the warp, overlap those of the second (intersection over union,
over the whole volume and round the moved sphere), and the flow that is left between the second bake and the warped first on the moved sphere.

    python examples/warp_synthetic.py [--step 0.004] [--band 0.008] [--move 2,-1,0] [--turn 10]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flow_synthetic import C, NAMES, observe     # noqa: E402
from d3fields_amd import synth     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.008")
    ap.add_argument("--move", default="2,-1,0", help="how far sphere 1 moves between the observations, in voxels")
    ap.add_argument("--turn", type=float, default=0.0, help="degrees sphere 1 also turns about its own vertical axis")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--margin", type=float, default=2.0, help="how far round a part its voxels' owner label reaches, in voxels")
    ap.add_argument("--min-voxels", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda:0"
    V, H, W = 4, 240, 320
    move = [int(m) for m in args.move.split(",")]
    K, Rt = synth.ring_cameras(V, H, W)
    proto = np.random.default_rng(3).standard_normal((len(NAMES), C - 24)).astype(np.float32)
    before = list(synth._SPHERES)
    after = list(before)
    after[1] = tuple(c + m * args.step for c, m in zip(before[1][:3], move)) + (before[1][3],)
    a = observe(before, K, Rt, H, W, proto, dev).bake(synth.WORK_BOX, args.step, return_names=["mask", "feat"], band=args.band)
    b = observe(after, K, Rt, H, W, proto, dev, turn=math.radians(args.turn)).bake(synth.WORK_BOX, args.step, return_names=["mask", "feat"], band=args.band)
    iso = args.step
    fwd = a.flow(b, "feat", radius_voxels=args.radius, iso=iso)
    back = b.flow(a, "feat", radius_voxels=args.radius, iso=iso)
    parts = a.parts("mask", rule="argmax", iso=iso, min_voxels=args.min_voxels)
    pm = fwd.motions(parts, keep=fwd.consistent(back))
    which = pm.moved(min_shift=0.5 * args.step, min_angle=math.radians(2.0))
    owner = a.owners(parts, margin_voxels=args.margin)
    w = a.warp(pm, owner, which=which)
    print("volume %s at %.3f m%s, '%s' moved by %s voxels and turned %g degrees; %d parts, %d of them moved"
          % (tuple(a.grid_shape), args.step, "" if args.band is None else ", band %g m" % args.band, NAMES[2], tuple(move), args.turn, parts.count, int(which.sum())))
    for k in which.nonzero().view(-1).tolist():
        lo, hi = w.part_box_to[k].tolist()
        print("    part %d: %d voxels (%d with the margin) -> won %d voxels in the box %s .. %s" % (k + 1, int(parts.sizes[k]), int((owner == k + 1).sum()),
                                                                                                    int((w.source == k + 1).sum()), tuple(lo), tuple(hi)))
    print("    %d voxels stayed, %d came from a part, %d are unknown now (%d were before)" % (int((w.source == 0).sum()), int((w.source > 0).sum()),
                                                                                             int((w.source < 0).sum()), int((~a.valid).sum())))
    occupied = lambda f: f.valid & (f.dist <= iso)
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev) for n in a.grid_shape], indexing="ij"), dim=-1).double()
    world = torch.tensor(a.origin, dtype=torch.float64, device=dev) + grid * a.step
    near = lambda s: (world - torch.tensor(s[:3], dtype=torch.float64, device=dev)).norm(dim=-1) <= s[3] + 2 * args.step
    region = near(before[1]) | near(after[1])
    iou = lambda x, y: float((x & y).sum()) / max(float((x | y).sum()), 1.0)
    print("    occupied-set IoU with the second bake: %.3f before, %.3f after the warp (round the moved sphere: %.3f before, %.3f after)"
          % (iou(occupied(a), occupied(b)), iou(occupied(w), occupied(b)), iou(occupied(a) & region, occupied(b) & region),
             iou(occupied(w) & region, occupied(b) & region)))
    on_sphere = near(after[1]) & occupied(b)
    for name, first in (("the first bake", a), ("the warped first bake", w)):
        fl = b.flow(first, "feat", radius_voxels=args.radius, iso=iso)
        sel = on_sphere & fl.matched
        d = fl.displacement(refined=False)[sel].norm(dim=-1) / args.step
        print("    residual flow from the second bake to %s on the moved sphere: %d matched voxels, median %.2f voxels, 90 %% below %.2f"
              % (name, int(sel.sum()), float(d.median()) if d.numel() else math.nan, float(d.quantile(0.9)) if d.numel() else math.nan))


if __name__ == "__main__":
    main()
