"""Times the non-maximum suppression (d3f_volume_peaks, csrc/peaks_kernels.hip; BakedField.peaks / locate) on the synthetic smooth scene (needs
an MI355X) and writes profiles/peaks/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_straight.py: HIP events on the stream round the call, median of --runs runs after warm-up (a quarter as many on the
1 mm grid); the header carries the date, the commit and the shader clock.  Workloads: the 4 mm bake of the work box (200 x 175 x 55), dense
(one row per voxel) and as a band of 5 mm (one row per stored voxel behind the slot volume), with K = 1, 16, 100 columns of uniform random
scores and r = 1, 2, 4, 8; and the band of 5 mm of the 1 mm grid of the same box, where a dense [K, nx, ny, nz] array cannot exist, if it fits.
Per line, measured in the same run:

    peaks      one d3f_volume_peaks with out_count (the entry point alone: its memset and its kernel), and the peaks it finds per column
    copy       a bare copy of the same score bytes (torch copy_ of the [M, K] matrix): what reading and writing every entry once costs
    torch      dense only: the recipe -max_pool3d(-x, 2r+1, 1, r) == x on the [1, K, nx, ny, nz] layout it needs (the transposition is not
               timed); it marks every voxel that equals its box minimum, so plateaus give several marks where peaks gives one
    whole      BakedField.peaks(values, radius_voxels=r, k=8): suppression, the k best per column, points and the refinement

    python scripts/bench_peaks.py [--runs 10] [--out profiles/peaks/results.txt] [--no-fine]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, _lib, synth     # noqa: E402

BAND = 0.005
COLUMNS = (1, 16, 100)
RADII = (1, 2, 4, 8)


def fmt(t):
    return "median %9.4f ms (min %.4f, max %.4f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--no-fine", action="store_true", help="skip the 1 mm grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["non-maximum suppression (d3f_volume_peaks; BakedField.peaks), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; device times: HIP events round the call, median of %d runs after 3 warm-up calls (a quarter as many on the 1 mm grid; min, max); "
             "scene: synth smooth, %d views of %d x %d; scores: uniform random float32 in [0, 1); band %g m" % (args.runs, V, H, W, BAND), ""]

    def flush():
        text = "\n".join(lines[:1] + [clock_line()] + lines[1:]) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        return text

    def one_layout(field, banded, runs, columns, radii, whole):
        nx, ny, nz = field.grid_shape
        M = field.band_voxels.shape[0] if banded else nx * ny * nz
        slot = field.slot if banded else None
        for K in columns:
            score = torch.rand((M, K), dtype=torch.float32, device=dev)
            out = torch.empty_like(score)
            count = torch.empty(K, dtype=torch.int32, device=dev)
            copy = median_ms(lambda: out.copy_(score), runs, 1)
            lines.append("    K = %3d: %d rows, %.1f MB of scores; copy of the same bytes: %s" % (K, M, score.numel() * 4 / 1e6, fmt(copy)))
            x = None
            if not banded:
                try:
                    x = score.view(nx, ny, nz, K).permute(3, 0, 1, 2).contiguous()[None]
                except torch.OutOfMemoryError:
                    x = None
            for r in radii:
                def call():
                    with torch.cuda.device(dev):
                        _lib.check(lib.d3f_volume_peaks(_lib.ptr(slot), None, nx, ny, nz, _lib.ptr(score), M, K, K, r, float("inf"), _lib.ptr(out), K, _lib.ptr(count),
                                                        None, 0, _lib.current_stream_handle(dev)))
                t = median_ms(call, runs, 1)
                text = "        r = %d: peaks %s, %.1f peaks per column" % (r, fmt(t), float(count.float().mean()))
                if x is not None:
                    try:
                        t2 = median_ms(lambda: (-torch.nn.functional.max_pool3d(-x, 2 * r + 1, 1, r)) == x, max(3, runs // 2), 1)
                        text += "; torch %s" % fmt(t2)
                    except (RuntimeError, torch.OutOfMemoryError) as exc:
                        text += "; torch: failed (%s)" % str(exc).splitlines()[0][:60]
                if whole:
                    values = score if banded else score.view(nx, ny, nz, K)
                    t3 = median_ms(lambda: field.peaks(values, radius_voxels=r, k=8), max(3, runs // 2), 1)
                    text += "; whole %s" % fmt(t3)
                lines.append(text)
                flush()
            del score, out, count, x
            torch.cuda.empty_cache()

    dense = f.bake(synth.WORK_BOX, 0.004, return_names=[])
    nx, ny, nz = dense.grid_shape
    lines.append("%d x %d x %d = %.2f M voxels (step 0.004 m), dense: one row per voxel; %d runs" % (nx, ny, nz, nx * ny * nz / 1e6, args.runs))
    one_layout(dense, False, args.runs, COLUMNS, RADII, True)
    band = dense.to_band(BAND)
    lines.append("")
    lines.append("the same grid as a band: %d stored voxels (%.2f %%) behind the slot volume; %d runs" % (band.band_voxels.shape[0], 100 * band.stored_fraction, args.runs))
    one_layout(band, True, args.runs, COLUMNS, RADII, True)
    del dense, band
    torch.cuda.empty_cache()
    if not args.no_fine:
        lines.append("")
        try:
            fine = f.bake(synth.WORK_BOX, 0.001, return_names=[], band=BAND)
            nx, ny, nz = fine.grid_shape
            runs = max(3, args.runs // 4)
            lines.append("%d x %d x %d = %.1f M voxels (step 0.001 m) as a band: %d stored voxels (%.2f %%); dense scores of one column would be %.2f GB; %d runs"
                         % (nx, ny, nz, nx * ny * nz / 1e6, fine.band_voxels.shape[0], 100 * fine.stored_fraction, nx * ny * nz * 4 / 1e9, runs))
            one_layout(fine, True, runs, (1, 16), (1, 2, 8), False)
        except torch.OutOfMemoryError:
            lines.append("the 1 mm band did not fit in memory: not measured")
    print(flush())


if __name__ == "__main__":
    main()
