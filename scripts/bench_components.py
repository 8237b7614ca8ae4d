"""Times connected-component labelling (d3f_volume_components, csrc/ccl_kernels.hip; BakedField.components) on the synthetic smooth
scene (needs an MI355X) and writes profiles/components/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_edt.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the commit
and the shader clock.  Volumes: the 200 x 175 x 55 bake (4 mm) of the reference's vis_repr.py:88 and the 1 mm grid of the same box
(123.2 M voxels); sites = valid & dist <= 0 plus 0.1 % of the voxels as random single-voxel floaters.  Connectivity 6 and 26, min_voxels
1 and 50, labels and counts only (stats_capacity 0), and one row with the stats of every kept component.  Next to every time, measured
in the same run:

    copy    a bare device pass over the algorithmic bytes: one byte read and four bytes written per voxel (a uint8 -> int32
            converting copy)
    scipy   scipy.ndimage.label on the host with the matching structure, median of --host-runs, at 4 mm and where scipy imports

    python scripts/bench_components.py [--runs 20] [--host-runs 3] [--out profiles/components/results.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_edt import host_ms     # noqa: E402
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, _lib, synth     # noqa: E402

FLOATERS = 0.001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components", "results.txt"))
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
    lines = ["connected components (d3f_volume_components), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; device times: HIP events, median of %d runs after warm-up (a quarter as many from 2^24 voxels on; min, max); host times: wall clock, median of %d; scene: synth smooth, %d views of %d x %d"
             % (args.runs, args.host_runs, V, H, W), ""]
    gen = torch.Generator(device="cpu").manual_seed(17)
    for step in (0.004, 0.001):
        field = f.bake(synth.WORK_BOX, step, return_names=[])
        nx, ny, nz = field.grid_shape
        n = nx * ny * nz
        shell = field.valid & (field.dist <= 0.0)
        floaters = torch.zeros(n, dtype=torch.bool)
        floaters[torch.randint(0, n, (int(FLOATERS * n),), generator=gen)] = True
        sites = (shell | floaters.view(nx, ny, nz).to(dev)).contiguous()
        site_u8 = sites.view(torch.uint8)
        labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws_bytes = int(lib.d3f_volume_components_workspace_bytes(nx, ny, nz))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = _lib.current_stream_handle(dev)
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 4)
        lines.append("%d x %d x %d = %.2f M voxels (step %g m), %d sites (%.2f %%, %d of them outside the shell mask), workspace %.1f MB; device times here: median of %d runs"
                     % (nx, ny, nz, n / 1e6, step, int(sites.sum()), 100.0 * float(sites.float().mean()), int((sites & ~shell).sum()), ws_bytes / 1e6, runs))
        host_sites = None

        def copy():
            labels.copy_(site_u8)

        for conn in (6, 26):
            for min_voxels in (1, 50):
                def ccl(stats=None, capacity=0):
                    _lib.check(lib.d3f_volume_components(_lib.ptr(site_u8), nx, ny, nz, conn, min_voxels, _lib.ptr(labels), _lib.ptr(count), _lib.ptr(stats),
                                                         capacity, _lib.ptr(ws), ws_bytes, stream))

                med, lo, hi = median_ms(ccl, runs, 1)
                kept, found = count.tolist()
                cmed, clo, chi = median_ms(copy, runs, 1)
                text = "    connectivity %2d min_voxels %2d: K %8d of %8d found   median %9.4f ms (min %.4f, max %.4f)   copy of %.1f MB: %.4f ms (min %.4f, max %.4f)" % (
                    conn, min_voxels, kept, found, med, lo, hi, 5 * n / 1e6, cmed, clo, chi)
                if ndimage is None:
                    text += "   scipy: not installed"
                elif n >= (1 << 24):
                    text += "   scipy: not run at this size"
                elif min_voxels > 1:
                    text += "   scipy: label has no threshold (see min_voxels 1)"
                else:
                    if host_sites is None:
                        host_sites = sites.cpu().numpy()
                    structure = ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)
                    smed, slo, shi = host_ms(lambda: ndimage.label(host_sites, structure=structure), args.host_runs)
                    text += "   scipy.ndimage.label on the host: %.1f ms (min %.1f, max %.1f)" % (smed, slo, shi)
                lines.append(text)
                if kept > 0:
                    stats = torch.empty((kept, 8), dtype=torch.int32, device=dev)
                    med, lo, hi = median_ms(lambda: ccl(stats, kept), runs, 1)
                    lines.append("        ... with the stats rows of all K components: median %9.4f ms (min %.4f, max %.4f); largest component %d voxels"
                                 % (med, lo, hi, int(stats[:, 1].max())))
                    del stats
        med, lo, hi = median_ms(lambda: field.components(sites=sites, min_voxels=50), runs, 1)
        lines.append("    BakedField.components(sites=, min_voxels=50) (one launch with room for 4096 stats rows, one host read of the count): median %.4f ms (min %.4f, max %.4f)" % (med, lo, hi))
        med, lo, hi = median_ms(lambda: field.clearance(sites=sites), runs, 1)
        med2, lo2, hi2 = median_ms(lambda: field.clearance(sites=sites, min_voxels=50), runs, 1)
        lines.append("    BakedField.clearance(sites=): median %.4f ms (min %.4f, max %.4f); with min_voxels=50: median %.4f ms (min %.4f, max %.4f)" % (med, lo, hi, med2, lo2, hi2))
        lines.append("")
        del field, shell, sites, site_u8, labels, ws
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
