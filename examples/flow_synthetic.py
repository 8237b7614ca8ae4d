"""How did it move?  Dense descriptor flow between two observations (needs an MI355X; no reference code, no network):

    bake(box, step, ['mask', 'feat'])     twice: the synthetic scene, and the same scene with ONE sphere moved by a few voxels.  The
                                           descriptors are painted on the objects (an instance prototype plus a Fourier code of the
                                           surface point in the object's own frame), so they move with the object
    a.flow(b, 'feat', radius_voxels=3)     for every occupied voxel of the first bake the voxel of the second with the closest row
    b.flow(a, ...), consistent(back)       the forward-backward test drops matches the way back does not confirm
    parts('mask', rule='argmax')           the parts of the first bake
    fwd.motions(parts, keep=consistent)    one rigid motion per part from its consistent matches, by a trim-and-refit loop on the device: the
                                           rotation angle, the shift, the inliers among the pairs and their rmse

    python examples/flow_synthetic.py [--step 0.004] [--band 0.008] [--move 2,-1,0] [--turn 10]

--turn DEG also turns the moved sphere, and with it its painted code, about its own vertical axis.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3fields_amd import Fusion, synth     # noqa: E402

NAMES = ["table"] + ["%s %d" % (n, i) for i, n in enumerate(synth._SPHERE_NAMES)]
C = 32


def observe(spheres, K, Rt, H, W, proto, dev, turn=0.0):
    """one observation of the scene with these spheres -> a Fusion holding depth, a one-hot mask and the painted descriptors; sphere 1 is
    turned by `turn` radians about the vertical through its centre (its shape stays, its painted code turns with it)"""
    V = K.shape[0]
    depth = synth.raycast_depth(K, Rt, H, W, spheres)
    labels = synth.sphere_label_images(K, Rt, depth, spheres)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    feat = np.zeros((V, H, W, C), np.float32)
    centres = np.array([(0.0, 0.0, 0.0)] + [s[:3] for s in spheres])
    freqs = 2.0 * np.pi * np.array([8.0, 19.0, 43.0, 97.0])                    # cycles per metre: from the object's size down to two voxels
    for v in range(V):
        Kv, R, t = K[v].astype(np.float64), Rt[v, :, :3].astype(np.float64), Rt[v, :, 3].astype(np.float64)
        d = depth[v].astype(np.float64)
        cam = np.stack([(uu - Kv[0, 2]) / Kv[0, 0] * d, (vv - Kv[1, 2]) / Kv[1, 1] * d, d], -1)
        local = (cam - t) @ R - centres[labels[v]]                             # the surface point in its object's frame
        if turn != 0.0:
            c, sn = math.cos(turn), math.sin(turn)
            Rz = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
            on = labels[v] == 2
            local[on] = local[on] @ Rz                                         # Rz^T (p - centre): where the point was before the turn
        phase = local[..., None, :] * freqs[:, None]                           # [H, W, 4, 3]
        code = np.concatenate([np.sin(phase), np.cos(phase)], -1).reshape(H, W, 24)
        feat[v] = np.concatenate([proto[labels[v]], 0.5 * code], -1)
    f = Fusion(num_cam=V, device=dev)
    f.curr_obs_torch = {"depth": torch.from_numpy(depth).to(dev), "K": torch.from_numpy(K).to(dev), "pose": torch.from_numpy(Rt).to(dev),
                        "mask": torch.nn.functional.one_hot(torch.from_numpy(labels), len(NAMES)).to(torch.float32).to(dev),
                        "feat": torch.from_numpy(feat).to(dev)}
    f.H, f.W = H, W
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.008")
    ap.add_argument("--move", default="2,-1,0", help="how far sphere 1 moves between the observations, in voxels")
    ap.add_argument("--turn", type=float, default=0.0, help="degrees sphere 1 also turns about its own vertical axis")
    ap.add_argument("--radius", type=int, default=3)
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
    iso = args.step                                                           # a shell one step thick round the observed surfaces
    fwd = a.flow(b, "feat", radius_voxels=args.radius, iso=iso)
    back = b.flow(a, "feat", radius_voxels=args.radius, iso=iso)
    members = a._members(a._site_mask("flow", iso, "free", None))
    ok = fwd.consistent(back)
    m = max(int(members.sum()), 1)
    print("volume %s at %.3f m, '%s' moved by %s voxels; %d occupied voxels, matched %.1f %%, forward-backward consistent %.1f %%"
          % (tuple(a.grid_shape), args.step, NAMES[2], tuple(move), m, 100.0 * int(fwd.matched.sum()) / m, 100.0 * int(ok.sum()) / m))
    parts = a.parts("mask", rule="argmax", iso=iso, min_voxels=args.min_voxels)
    votes = a.pool(parts, return_names=[], votes=["mask"])["mask_votes"]
    pm = fwd.motions(parts, keep=ok)                                          # one call: every part's rigid motion from its consistent matches
    verdict = {pm.OK: "ok", pm.THINNED: "thinned", pm.TOO_FEW: "too few"}
    for k in parts.largest(8).tolist():
        sh = (pm.shift[k - 1] / args.step).tolist()
        print("    part %3d ('%s'): %6d voxels, %6d consistent, turned %5.2f deg, shift (%+.2f, %+.2f, %+.2f) voxels, %d / %d inliers, rmse %.3f voxels, %s"
              % (k, NAMES[int(votes[k - 1].argmax())], int(parts.sizes[k - 1]), int(pm.pairs[k - 1]), math.degrees(float(pm.angle[k - 1])), sh[0], sh[1], sh[2],
                 int(pm.inliers[k - 1]), int(pm.pairs[k - 1]), float(pm.rmse[k - 1]) / args.step, verdict[int(pm.status[k - 1])]))


if __name__ == "__main__":
    main()
