"""Times the ray march through a baked volume (BakedField.render, csrc/raycast_kernels.hip) on the synthetic smooth scene (needs an
MI355X) and writes profiles/raycast/results.txt.  No thresholds: the file reports, nothing is asserted.

Volume: the 200 x 175 x 55 grid (4 mm) of the reference's vis_repr.py:88, baked with `dist` only, with a 3-component head and with a
384-channel set.  View: 480 x 640 from the scene's camera ring halfway between cameras 0 and 1, a pose no camera had.  Per case, median of --runs
runs after warm-up, HIP events on the stream around --reps back-to-back calls:

    march        d3f_volume_raycast alone (camera source): rays/s and samples/s (samples from the kernel's own per-ray count)
    march_rays   the same rays through the explicit source (origins / dirs arrays in pixel order, no 8 x 8 tiles)
    rows         d3f_volume_sample of the baked names at the marched points
    normals      d3f_volume_sample_backward with grad_dist = 1 plus the normalisation
    render       BakedField.render(return_names, normals=True): all of it

    python scripts/bench_raycast.py [--runs 20] [--out profiles/raycast/results.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from d3fields_amd import Fusion, synth     # noqa: E402
from bench_volume import clock_line, commit, median_ms     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, 384, seed=1).to(dev)
    f.H, f.W = H, W
    f.add_projection("pca3", components=torch.randn(3, 384, generator=torch.Generator().manual_seed(2)))
    K, pose = sc["K"][0], torch.from_numpy(synth.ring_cameras(2 * V, H, W)[1][1])      # on the ring, halfway between cameras 0 and 1
    lines = ["ray march through a baked volume, %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "HIP events, median of %d runs of %d calls after warm-up (min, max); scene: synth smooth, %d views of %d x %d; view: %d x %d, a pose no camera had, step = h"
             % (args.runs, args.reps, V, H, W, H, W), ""]
    for label, names in (("dist only", []), ("3-component head", ["pca3"]), ("384 channels", ["dino_feats"])):
        baked = f.bake(synth.WORK_BOX, 0.004, return_names=names)
        nx, ny, nz = baked.grid_shape
        cam = baked._camera(K, pose, H, W)
        n = H * W
        t, hit, pts, cnt = baked._march(None, None, cam, n, None, 0.0, float("inf"), samples=True)
        samples = int(cnt.sum())
        R, tc = pose[:, :3].double(), pose[:, 3].double()
        vv, uu = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        dc = torch.stack([(uu - float(K[0, 2])) / float(K[0, 0]), (vv - float(K[1, 2])) / float(K[1, 1]), torch.ones_like(uu)], -1).view(-1, 3)
        dirs = (dc @ R).float().to(dev).contiguous()
        origins = (-(R.T @ tc)).float().to(dev).expand(n, 3).contiguous()
        ones = torch.ones(n, dtype=torch.float32, device=dev)

        def normals():
            g = baked.backward(pts, ones)
            length = torch.linalg.vector_norm(g, dim=1, keepdim=True)
            return torch.where(length > 0, g / length, torch.zeros_like(g))

        res = {"march": median_ms(lambda: baked._march(None, None, cam, n, None, 0.0, float("inf")), args.runs, args.reps),
               "march_rays": median_ms(lambda: baked._march(origins, dirs, None, n, None, 0.0, float("inf")), args.runs, args.reps),
               "rows": median_ms(lambda: baked._sample(pts, names), args.runs, args.reps),
               "normals": median_ms(normals, args.runs, args.reps),
               "render": median_ms(lambda: baked.render(K, pose, H, W, return_names=names, normals=True), args.runs, args.reps)}
        lines.append("%d x %d x %d, %s: %d rays, %.1f %% hit, %d samples (%.1f per ray, at most %d)"
                     % (nx, ny, nz, label, n, 100 * float(hit.float().mean()), samples, samples / n, int(cnt.max())))
        for k, (med, lo, hi) in res.items():
            extra = ""
            if k.startswith("march"):
                extra = "   %.3g rays/s  %.3g samples/s" % (n / med * 1e3, samples / med * 1e3)
            lines.append("    %-11s median %9.4f ms   (min %.4f, max %.4f)%s" % (k, med, lo, hi, extra))
        lines.append("    the march is %.0f %% of march + rows + normals" % (100 * res["march"][0] / (res["march"][0] + res["rows"][0] + res["normals"][0])))
        del baked
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
