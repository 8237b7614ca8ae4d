"""Which part is this?  Objects that touch, separated by what the field stores (needs an MI355X; no reference code, no network):

    bake(box, step, ['mask', 'feat'])     the synthetic scene: four spheres RESTING ON a table, so table and spheres touch
    components()                           labels by occupancy alone: the table and everything on it come out as one component
    parts('mask', rule='argmax')           neighbouring voxels belong together only if their fused instance-mask rows vote alike:
                                           one part per spatially connected piece of each instance
    parts('feat', rule='l2', tau=...)      the same from the wide descriptors, without a segmenter
    pool(parts, votes=['mask'])            every part's instance vote, centroid and size

    python examples/parts_synthetic.py [--step 0.004] [--band 0.008]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3fields_amd import Fusion, synth     # noqa: E402

NAMES = ["table"] + ["%s %d" % (n, i) for i, n in enumerate(synth._SPHERE_NAMES)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.008")
    ap.add_argument("--min-voxels", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda:0"
    V, H, W, C = 4, 240, 320, 32
    sc = synth.make_scene(V, H, W, "smooth")
    labels = torch.from_numpy(synth.sphere_label_images(sc["K"].numpy(), sc["pose"].numpy(), sc["depth"].numpy()))      # [V, H, W]: 0 table, s + 1 sphere s
    gen = torch.Generator().manual_seed(3)
    proto = torch.randn(len(NAMES), C, generator=gen)
    f = Fusion(num_cam=V, device=dev)
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["mask"] = torch.nn.functional.one_hot(labels, len(NAMES)).to(torch.float32).to(dev)
    f.curr_obs_torch["feat"] = (proto[labels] + 0.05 * torch.randn(V, H, W, C, generator=gen)).to(dev)      # a descriptor per instance, plus noise
    f.H, f.W = H, W
    baked = f.bake(synth.WORK_BOX, args.step, return_names=["mask", "feat"], band=args.band)
    iso = args.step                                                           # a shell one step thick round the observed surfaces
    plain = baked.components(iso=iso, min_voxels=args.min_voxels)
    print("volume %s at %.3f m; occupancy alone: %d component(s) of at least %d voxels, the largest of %d voxels"
          % (tuple(baked.grid_shape), args.step, plain.count, args.min_voxels, int(plain.sizes.max()) if plain.count else 0))
    # a fifth of the distance of the two closest prototypes: where two objects meet, the fused rows blend from one prototype to the other over a
    # voxel or two, and single linkage follows any chain of small steps -- the radius has to be below the steps of that blend
    tau = 0.2 * float(torch.cdist(proto, proto)[~torch.eye(len(NAMES), dtype=torch.bool)].min())
    for what, kw in (("instance-mask rows, argmax", {"name": "mask", "rule": "argmax"}), ("descriptors, l2 within %.2f" % tau, {"name": "feat", "rule": "l2", "tau": tau})):
        parts = baked.parts(iso=iso, min_voxels=args.min_voxels, **kw)
        pooled = baked.pool(parts, return_names=[], votes=["mask"])
        print("parts by %s: %d kept of %d found" % (what, parts.count, parts.found))
        votes = pooled["mask_votes"]
        for k in parts.largest(8).tolist():
            row = votes[k - 1]
            c = pooled["centroid"][k - 1].tolist()
            print("    part %3d: %6d voxels, %5.1f %% vote '%s', centroid (%.3f, %.3f, %.3f)"
                  % (k, int(parts.sizes[k - 1]), 100.0 * float(row.max()) / max(int(row.sum()), 1), NAMES[int(row.argmax())], c[0], c[1], c[2]))


if __name__ == "__main__":
    main()
