"""Bake the synthetic scene and render a view no camera had (needs an MI355X; no reference code, no network):

    bake(box, step, ['pca3'])        one grid query kept as a BakedField: dist, validity, a 3-component head of the descriptors
    render(K, pose, H, W, ...)       rays through the pixels of a camera halfway between two of the scene's cameras, marched to the
                                     first surface: depth, hit mask, surface points, normals and the head's row per pixel

Writes render_depth.npy and render_pca3.npy (and .png where PIL is installed) into --out.

    python examples/render_synthetic.py [--step 0.004] [--out .]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3fields_amd import Fusion, synth     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--band", type=float, default=None, help="bake channel rows only within this distance (m) of the surface, e.g. 0.005")
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    dev = "cuda:0"
    V, H, W, C = 4, 240, 320, 384
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=dev)
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, C, seed=2, device=dev)
    f.H, f.W = H, W
    f.add_projection("pca3", components=torch.randn(3, C, generator=torch.Generator().manual_seed(5)))
    baked = f.bake(synth.WORK_BOX, args.step, return_names=["pca3"], band=args.band)
    K = sc["K"][0]
    pose = torch.from_numpy(synth.ring_cameras(2 * V, H, W)[1][1])           # on the ring, halfway between cameras 0 and 1
    baked.render(K, pose, H, W, return_names=["pca3"], normals=True)        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = baked.render(K, pose, H, W, return_names=["pca3"], normals=True)
    torch.cuda.synchronize()
    hit = out["hit_mask"]
    print("volume %s at %.3f m; %d x %d view: %d of %d pixels hit a surface, depth %.3f .. %.3f m, %.2f ms"
          % (tuple(baked.grid_shape), args.step, W, H, int(hit.sum()), H * W, float(out["depth"][hit].min()), float(out["depth"][hit].max()),
             1e3 * (time.perf_counter() - t0)))
    if args.band is not None:
        print("band %.4f m: %.1f %% of the voxels hold rows; %d of the %d hits lie in the band"
              % (args.band, 100 * baked.stored_fraction, int(out["in_band"].sum()), int(hit.sum())))
    depth, pca = out["depth"].cpu().numpy(), out["pca3"].cpu().numpy()
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "render_depth.npy"), depth)
    np.save(os.path.join(args.out, "render_pca3.npy"), pca)
    try:
        from PIL import Image
    except ImportError:
        return
    m = hit.cpu().numpy()
    d8 = np.zeros((H, W), np.uint8)
    d8[m] = (255 - 200 * (depth[m] - depth[m].min()) / max(float(np.ptp(depth[m])), 1e-9)).astype(np.uint8)
    lo, hi = pca[m].min(0), pca[m].max(0)
    c8 = np.zeros((H, W, 3), np.uint8)
    c8[m] = (255 * (pca[m] - lo) / np.maximum(hi - lo, 1e-9)).astype(np.uint8)
    Image.fromarray(d8).save(os.path.join(args.out, "render_depth.png"))
    Image.fromarray(c8).save(os.path.join(args.out, "render_pca3.png"))


if __name__ == "__main__":
    main()
