"""Times the banded baked field (BakedField.to_band / Fusion.bake(band=), csrc/band_kernels.hip) against the dense one on the
synthetic smooth scene (needs an MI355X) and writes profiles/band/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_volume.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the
commit and the shader clock.  Volume: the 200 x 175 x 55 grid (4 mm) of the reference's vis_repr.py:88 with a 3-component head, a
384-channel set and a 1024-channel set.  Per set, for the dense bake, band = 5 mm (the reference's dist_threshold) and band = 2 steps:

    bytes held       dist + valid + cell_valid + rows (+ slot + cell_band + the voxel list)
    stored_fraction  M / voxels
    bake             Fusion.bake, median of --bakes runs, wall clock around a device synchronisation (the band's count is read on the host)
    lookup           BakedField.eval on the ~71 k shell points (Fusion.grid_shell)
    fwd + bwd        eval with pts.requires_grad + backward of sum(dist) + sum(rows)

and one band bake at a 1 mm step (123.2 M voxels, the `dist_only` workload's grid), where the dense rows cannot exist.

    python scripts/bench_band.py [--runs 20] [--bakes 5] [--out profiles/band/results.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, synth     # noqa: E402


def held_bytes(field):
    tensors = [field.dist, field.valid, field.cell_valid] + list(field._sets.values())
    if field.band is not None:
        tensors += [field.slot, field.cell_band, field.band_voxels]
    return sum(t.numel() * t.element_size() for t in tensors)


def bake_ms(fn, runs):
    fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--bakes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.curr_obs_torch["dino_feats"] = synth.random_map(V, H // 10, W // 10, 384, seed=1).to(dev)
    f.curr_obs_torch["vitl_feats"] = synth.random_map(V, H // 10, W // 10, 1024, seed=5).to(dev)
    f.H, f.W = H, W
    f.add_projection("pca3", components=torch.randn(3, 384, generator=torch.Generator().manual_seed(2)))
    step = 0.004
    _, shell = f.grid_shell(synth.WORK_BOX, step)
    n = shell.shape[0]
    lines = ["banded baked field against the dense one, %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "HIP events, median of %d runs after warm-up (min, max); bakes: wall clock, median of %d; scene: synth smooth, %d views of %d x %d; %d shell points"
             % (args.runs, args.bakes, V, H, W, n), ""]
    for label, names in (("3-component head", ["pca3"]), ("384 channels", ["dino_feats"]), ("1024 channels", ["vitl_feats"])):
        for variant, band in (("dense", None), ("band 5 mm", 0.005), ("band 2 steps", 2 * step)):
            field = f.bake(synth.WORK_BOX, step, return_names=names, band=band)
            nx, ny, nz = field.grid_shape

            def fwd():
                with torch.no_grad():
                    return field.eval(shell, return_names=names)

            def fwd_bwd():
                p = shell.detach().requires_grad_(True)
                out = field.eval(p, return_names=names)
                loss = out["dist"].sum()
                for k in names:
                    loss = loss + out[k].sum()
                loss.backward()

            out = fwd()
            extra = "" if band is None else ", stored_fraction %.4f (M = %d), %.1f %% of the shell points in_band" % (
                field.stored_fraction, field.band_voxels.numel(), 100 * float(out["in_band"].float().mean()))
            lines.append("%d x %d x %d, %s, %s: %.1f MB held%s" % (nx, ny, nz, label, variant, held_bytes(field) / 1e6, extra))
            res = {"bake": bake_ms(lambda: f.bake(synth.WORK_BOX, step, return_names=names, band=band), args.bakes),
                   "lookup": median_ms(fwd, args.runs, 10), "fwd + bwd": median_ms(fwd_bwd, args.runs, 10)}
            for k, (med, lo, hi) in res.items():
                lines.append("    %-10s median %9.4f ms   (min %.4f, max %.4f)" % (k, med, lo, hi))
            del field, out
            torch.cuda.empty_cache()
    # the resolution of the reference's own distance volume: 1 mm, 123.2 M voxels
    lines.append("")
    for label, names, C in (("3-component head", ["pca3"], 3), ("384 channels", ["dino_feats"], 384)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        field = f.bake(synth.WORK_BOX, 0.001, return_names=names, band=0.005)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        nx, ny, nz = field.grid_shape
        nvox = nx * ny * nz
        lines.append("%d x %d x %d = %.1f M voxels, %s, band 5 mm: ONE bake %.1f ms wall clock; stored_fraction %.4f (M = %d); %.1f MB held, peak %.1f MB allocated; "
                     "dense rows would be %.1f GB" % (nx, ny, nz, nvox / 1e6, label, ms, field.stored_fraction, field.band_voxels.numel(), held_bytes(field) / 1e6,
                                                       torch.cuda.max_memory_allocated(dev) / 1e6, 4.0 * nvox * C / 1e9))
        del field
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
