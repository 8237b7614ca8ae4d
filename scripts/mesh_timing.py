"""Times the iso-surface extraction and the volume Gaussian on the two distance volumes the project uses (needs an MI355X):

    200 x 175 x 55   the 4-mm grid of the reference's vis_repr.py:88
    800 x 700 x 220  the 1-mm grid of bench.py --workload dist_only

of the synthetic smooth scene.  Per volume, in ONE process and one run: the distance-only pass that produces the volume,
d3f_mesh_count + d3f_mesh_extract (capacities known, no host read-back inside the bracket), d3f_volume_gaussian (sigma 1),
and a bare device-to-device copy of the same volume as the yardstick (the extraction reads the volume a few times and writes
little).  Each figure is the median of --runs runs after warm-up, bracketed by HIP events on the stream; the bracket holds
--reps back-to-back calls so that it is long enough for the event clock.

    python scripts/mesh_timing.py [--runs 20] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3fields_amd import Fusion, _lib, create_init_grid, mesh, synth     # noqa: E402


def median_ms(fn, runs, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    rows = []
    for step in (0.004, 0.001):
        pts, shape = create_init_grid(synth.WORK_BOX, step)
        pts = pts.to(dev)
        nx, ny, nz = (int(s) for s in shape)
        n = nx * ny * nz
        reps = 20 if n < 10 ** 7 else 3
        with torch.no_grad():
            res = f.batch_eval(pts, return_names=[])
            t_dist = median_ms(lambda: f.batch_eval(pts, return_names=[]), args.runs, reps)
        dist, valid = res["dist"], res["valid_mask"]
        keys, t, tris = mesh.marching_cubes(dist, shape, valid=valid, count_first=True)
        nv, nt = keys.numel(), tris.shape[0]
        ws_bytes = int(lib.d3f_mesh_workspace_bytes(nx, ny, nz))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_handle(dev)

        def count():
            _lib.check(lib.d3f_mesh_count(_lib.ptr(dist), _lib.ptr(valid), nx, ny, nz, 0.0, _lib.ptr(counts), _lib.ptr(ws), ws_bytes, stream))

        def extract():
            _lib.check(lib.d3f_mesh_extract(_lib.ptr(dist), _lib.ptr(valid), nx, ny, nz, 0.0, nv, nt, _lib.ptr(keys), _lib.ptr(t), _lib.ptr(tris),
                                            _lib.ptr(counts), _lib.ptr(ws), ws_bytes, stream))

        def both():
            count()
            extract()

        out = torch.empty_like(dist)
        gws = torch.empty(n * 4, dtype=torch.uint8, device=dev)

        def gauss():
            _lib.check(lib.d3f_volume_gaussian(_lib.ptr(dist), _lib.ptr(out), nx, ny, nz, 1.0, 4.0, _lib.ptr(gws), n * 4, stream))

        row = {"shape": [nx, ny, nz], "points": n, "vertices": nv, "triangles": nt, "workspace_bytes": ws_bytes, "runs": args.runs, "reps": reps,
               "dist_only_ms": t_dist,
               "count_ms": median_ms(count, args.runs, reps),
               "extract_ms": median_ms(extract, args.runs, reps),
               "count_plus_extract_ms": median_ms(both, args.runs, reps),
               "gaussian_sigma1_ms": median_ms(gauss, args.runs, reps),
               "copy_d2d_ms": median_ms(lambda: out.copy_(dist), args.runs, reps)}
        rows.append(row)
        if not args.json:
            print("%d x %d x %d (%d points): %d vertices, %d triangles, workspace %d bytes" % (nx, ny, nz, n, nv, nt, ws_bytes))
            for k in ("dist_only_ms", "count_ms", "extract_ms", "count_plus_extract_ms", "gaussian_sigma1_ms", "copy_d2d_ms"):
                med, lo, hi = row[k]
                print("    %-24s median %8.3f ms   (min %.3f, max %.3f; x copy: %.2f)" % (k, med, lo, hi, med / row["copy_d2d_ms"][0]))
        del pts, res, dist, valid, keys, t, tris, out, gws
    if args.json:
        print(json.dumps({"device": torch.cuda.get_device_name(0), "clock": "HIP events, median of runs", "volumes": rows}))


if __name__ == "__main__":
    main()
