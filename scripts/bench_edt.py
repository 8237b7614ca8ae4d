"""Times the exact Euclidean distance transform (d3f_volume_edt, csrc/edt_kernels.hip; BakedField.clearance) on the synthetic smooth
scene (needs an MI355X) and writes profiles/edt/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_volume.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the
commit and the shader clock.  Volumes: the 200 x 175 x 55 bake (4 mm) of the reference's vis_repr.py:88 and the 1 mm grid of the same
box (123.2 M voxels); sites = valid & dist <= 0.  Each volume unbounded and with max_distance = 0.1 m, each with out_d2 + out_dist
and with out_nearest as well.  Next to every time, measured in the same run:

    copy    a bare device pass over the algorithmic bytes: one byte read and four bytes written per voxel for the first output (a
            uint8 -> int32 converting copy), four bytes written for every further output (a fill)
    scipy   scipy.ndimage.distance_transform_edt(~sites, return_indices=<out_nearest asked>) on the host, median of --host-runs, where
            scipy imports; at 1 mm only with --scipy-large (minutes, and several GB of host memory)

    python scripts/bench_edt.py [--runs 20] [--host-runs 3] [--scipy-large] [--out profiles/edt/results.txt]
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
from d3fields_amd import Fusion, _lib, synth     # noqa: E402


def host_ms(fn, runs):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--scipy-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt", "results.txt"))
    args = ap.parse_args()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["exact Euclidean distance transform (d3f_volume_edt), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; device times: HIP events, median of %d runs after warm-up (a quarter as many from 2^24 voxels on; min, max); host times: wall clock, median of %d; scene: synth smooth, %d views of %d x %d"
             % (args.runs, args.host_runs, V, H, W), ""]
    for step in (0.004, 0.001):
        field = f.bake(synth.WORK_BOX, step, return_names=[])
        nx, ny, nz = field.grid_shape
        n = nx * ny * nz
        sites = (field.valid & (field.dist <= 0.0)).contiguous()
        site_u8 = sites.view(torch.uint8)
        d2 = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        nearest = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        dist = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        ws_bytes = int(lib.d3f_volume_edt_workspace_bytes(nx, ny, nz))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = _lib.current_stream_handle(dev)
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 4)
        lines.append("%d x %d x %d = %.2f M voxels (step %g m), %d sites (%.2f %%), workspace %.1f MB; device times here: median of %d runs"
                     % (nx, ny, nz, n / 1e6, step, int(sites.sum()), 100.0 * float(sites.float().mean()), ws_bytes / 1e6, runs))
        host_sites = None
        for label, max_distance in (("unbounded", None), ("max_distance 0.1 m", 0.1)):
            max_d2 = 0 if max_distance is None else int((max_distance / field.step) ** 2)
            for with_nearest in (False, True):
                outs = "d2 + dist + nearest" if with_nearest else "d2 + dist"

                def edt():
                    _lib.check(lib.d3f_volume_edt(_lib.ptr(site_u8), nx, ny, nz, field.step, max_d2, _lib.ptr(d2), _lib.ptr(nearest) if with_nearest else None,
                                                  _lib.ptr(dist), _lib.ptr(ws), ws_bytes, stream))

                def copy():
                    d2.copy_(site_u8)
                    dist.fill_(1.0)
                    if with_nearest:
                        nearest.fill_(1)

                med, lo, hi = median_ms(edt, runs, 1)
                cmed, clo, chi = median_ms(copy, runs, 1)
                nbytes = n * (1 + 4 * (3 if with_nearest else 2))
                text = "    %-18s %-20s median %9.4f ms (min %.4f, max %.4f)   copy of %.1f MB: %.4f ms (min %.4f, max %.4f)" % (
                    label, outs, med, lo, hi, nbytes / 1e6, cmed, clo, chi)
                if ndimage is None:
                    text += "   scipy: not installed"
                elif n >= (1 << 24) and not args.scipy_large:
                    text += "   scipy: not run at this size"
                elif max_distance is not None:
                    text += "   scipy: has no cap (see unbounded)"
                else:
                    if host_sites is None:
                        host_sites = ~sites.cpu().numpy()
                    smed, slo, shi = host_ms(lambda: ndimage.distance_transform_edt(host_sites, sampling=field.step, return_indices=with_nearest), args.host_runs)
                    text += "   scipy on the host: %.1f ms (min %.1f, max %.1f)" % (smed, slo, shi)
                lines.append(text)
        med, lo, hi = median_ms(lambda: field.clearance(), runs, 1)
        lines.append("    BakedField.clearance() (site mask, all three outputs, cell_valid of the new field): median %.4f ms (min %.4f, max %.4f)" % (med, lo, hi))
        med, lo, hi = median_ms(lambda: field.clearance(signed=True, max_distance=0.1), runs, 1)
        lines.append("    BakedField.clearance(signed=True, max_distance=0.1): median %.4f ms (min %.4f, max %.4f)" % (med, lo, hi))
        lines.append("")
        del field, sites, site_u8, d2, nearest, dist, ws
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
