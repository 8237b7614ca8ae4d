"""How far did it move?  Coarse-to-fine flow over a pyramid of bakes (needs an MI355X; no reference code, no network):

    bake(box, step, ['mask', 'feat'])     twice: the scene of examples/flow_synthetic.py, and the same scene with ONE sphere moved by about
                                           ten voxels -- beyond the 4 voxels a flow window reaches
    a.flow(b, 'feat', radius_voxels=4)     the direct flow: the moved sphere finds nothing of itself inside its window
    a.flow_pyramid(b, 'feat', levels=2)    both fields coarsened twice (BakedField.coarsen), flow at radius 2 on the coarsest level, then flow(seed=) at
                                           radius 1 round the prediction of the level above (Flow.seed) on each finer one
    parts('mask', rule='argmax')           the parts of the first bake: per part the share of its voxels that are matched, the median
                                           displacement in voxels and the share whose whole-voxel offset is exactly the planted move

    python examples/pyramid_synthetic.py [--step 0.004] [--band 0.008] [--move 8,-6,0] [--levels 2]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from d3fields_amd import synth     # noqa: E402
from flow_synthetic import C, NAMES, observe     # noqa: E402


def report(what, flow, parts, votes, move, step):
    print("%s: matched %d voxels" % (what, int(flow.matched.sum())))
    shift = torch.tensor(move, dtype=torch.int32, device=flow.target.device)
    for k in parts.largest(4).tolist():
        own = parts.labels == k
        hit = own & flow.matched
        disp = flow.displacement()[hit] / step
        med = disp.median(dim=0).values.tolist() if len(disp) else [float("nan")] * 3
        exact = int((flow.voxel_offset[hit] == shift).all(1).sum())
        print("    part %3d ('%s'): %6d voxels, matched %5.1f %%, median displacement (%+.2f, %+.2f, %+.2f) voxels, exactly on %s: %5.1f %%"
              % (k, NAMES[int(votes[k - 1].argmax())], int(own.sum()), 100.0 * int(hit.sum()) / max(int(own.sum()), 1), med[0], med[1], med[2], tuple(move),
                 100.0 * exact / max(int(own.sum()), 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.008")
    ap.add_argument("--move", default="8,-6,0", help="how far sphere 1 moves between the observations, in voxels")
    ap.add_argument("--levels", type=int, default=2)
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
    b = observe(after, K, Rt, H, W, proto, dev).bake(synth.WORK_BOX, args.step, return_names=["mask", "feat"], band=args.band)
    iso = args.step                                                           # a shell one step thick round the observed surfaces
    parts = a.parts("mask", rule="argmax", iso=iso, min_voxels=args.min_voxels)
    votes = a.pool(parts, return_names=[], votes=["mask"])["mask_votes"]
    print("volume %s at %.3f m, '%s' moved by %s voxels (%.1f voxels)" % (tuple(a.grid_shape), args.step, NAMES[2], tuple(move), float(np.linalg.norm(move))))
    report("direct flow, radius 4", a.flow(b, "feat", radius_voxels=4, iso=iso), parts, votes, move, args.step)
    chain = a.flow_pyramid(b, "feat", levels=args.levels, radius_voxels=2, fine_radius_voxels=1, iso=iso)
    print("pyramid: %s" % " <- ".join(str(tuple(f.grid_shape)) for f in [chain] + chain.coarse[::-1]))
    report("flow_pyramid, %d levels, radius 2 at the top, 1 below" % args.levels, chain, parts, votes, move, args.step)


if __name__ == "__main__":
    main()
