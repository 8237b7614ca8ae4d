"""What have I seen so far?  Two bakes of the synthetic scene from few views; in the second frame an occluder passes between every camera and
one object, so that bake alone has lost the object -- and bake1.merge(bake2) still has it (needs an MI355X; no reference code, no network):

    frame 1      the table and the spheres of d3fields_amd/synth.py, seen by --views cameras
    frame 2      the same scene with one extra sphere per camera on the line from the camera to the hidden object, outside the baked box
    bake1.merge(bake2)   keeps what is hidden now, averages what is seen twice (BakedField.merge)

and prints, for the hidden object's voxels (the ones valid round it in an un-occluded bake of frame 2), how many are valid in bake 2 alone
and in the merge, and the occupied-set IoU of each against the un-occluded bake of frame 2.  Nothing moves between the frames, so the
warp step of the full recipe (memory.warp(motions, owners) before the merge) is the identity and is left out.

    python examples/memory_synthetic.py [--step 0.004] [--band 0.008] [--views 2] [--hide 1]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3fields_amd import BakedField, Fusion, synth     # noqa: E402

C = 16


def observe(spheres, K, Rt, H, W, dev):
    """one observation: the ray-cast depth of the plane and these spheres, and a descriptor painted on the surface (sines of the world point)"""
    V = K.shape[0]
    depth = synth.raycast_depth(K, Rt, H, W, spheres)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    freqs = 2.0 * np.pi * np.array([8.0, 19.0, 43.0, 97.0])
    feat = np.zeros((V, H, W, C), np.float32)
    for v in range(V):
        Kv, R, t = K[v].astype(np.float64), Rt[v, :, :3].astype(np.float64), Rt[v, :, 3].astype(np.float64)
        d = depth[v].astype(np.float64)
        cam = np.stack([(uu - Kv[0, 2]) / Kv[0, 0] * d, (vv - Kv[1, 2]) / Kv[1, 1] * d, d], -1)
        world = (cam - t) @ R
        phase = (world[..., None, :2] * freqs[:, None]).reshape(H, W, 8)
        feat[v] = np.concatenate([np.sin(phase), np.cos(phase)], -1)
    f = Fusion(num_cam=V, device=dev)
    f.curr_obs_torch = {"depth": torch.from_numpy(depth).to(dev), "K": torch.from_numpy(K).to(dev), "pose": torch.from_numpy(Rt).to(dev),
                        "feat": torch.from_numpy(feat).to(dev)}
    f.H, f.W = H, W
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.008")
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--hide", type=int, default=1, help="which sphere of the scene the occluders hide")
    args = ap.parse_args()
    dev = "cuda:0"
    V, H, W = args.views, 240, 320
    K, Rt = synth.ring_cameras(V, H, W)
    scene = list(synth._SPHERES)
    hidden = scene[args.hide]
    occluders = []
    for v in range(V):                               # half way from the object to each camera: above the baked box, wide enough to cover the object
        centre = -Rt[v, :, :3].astype(np.float64).T @ Rt[v, :, 3].astype(np.float64)
        mid = 0.5 * (centre + np.array(hidden[:3]))
        occluders.append((float(mid[0]), float(mid[1]), float(mid[2]), 0.8 * hidden[3]))
    bake = lambda spheres: observe(spheres, K, Rt, H, W, dev).bake(synth.WORK_BOX, args.step, return_names=["feat"], band=args.band)
    bake1, free2, bake2 = bake(scene), bake(scene), bake(scene + occluders)
    memory = bake1.merge(bake2)
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev) for n in bake1.grid_shape], indexing="ij"), dim=-1).double()
    world = torch.tensor(bake1.origin, dtype=torch.float64, device=dev) + grid * bake1.step
    region = ((world - torch.tensor(hidden[:3], dtype=torch.float64, device=dev)).norm(dim=-1) <= hidden[3] + 2 * args.step) & free2.valid
    iso = args.step
    occupied = lambda f: f.valid & (f.dist <= iso)
    iou = lambda x, y: float((x & y).sum()) / max(float((x | y).sum()), 1.0)
    kinds = torch.bincount(memory.merged_from.view(-1).long(), minlength=5).tolist()
    print("volume %s at %.3f m%s, %d views; sphere %d hidden in frame 2 by %d occluders outside the box"
          % (tuple(bake1.grid_shape), args.step, "" if args.band is None else ", band %g m" % args.band, V, args.hide, V))
    print("    the hidden object's %d voxels: %d valid in bake 2 alone, %d in bake1.merge(bake2)" % (int(region.sum()), int((region & bake2.valid).sum()), int((region & memory.valid).sum())))
    print("    occupied-set IoU with the un-occluded bake of frame 2: %.3f bake 2 alone, %.3f the merge (round the object: %.3f, %.3f)"
          % (iou(occupied(bake2), occupied(free2)), iou(occupied(memory), occupied(free2)), iou(occupied(bake2) & region, occupied(free2) & region),
             iou(occupied(memory) & region, occupied(free2) & region)))
    print("    merged_from: %d unknown, %d kept from bake 1, %d new in bake 2, %d averaged, %d reset; rows known for %d of %d %s"
          % (kinds[BakedField.MERGE_NONE], kinds[BakedField.MERGE_KEEP], kinds[BakedField.MERGE_NEW], kinds[BakedField.MERGE_BLEND], kinds[BakedField.MERGE_RESET],
             int(memory.rows_known.sum()), memory.rows_known.numel(), "voxels" if args.band is None else "stored voxels"))


if __name__ == "__main__":
    main()
