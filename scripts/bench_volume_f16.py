"""Times the baked-volume lookup on rows stored as float32 and as IEEE half (BakedField.half) in ONE process
(needs an MI355X) and writes profiles/volume_f16/results.txt.  No thresholds: the file reports, nothing is asserted.

Volume: the 200 x 175 x 55 grid (4 mm) of the synthetic smooth scene, dist / valid from Fusion.bake; the channel set is drawn at random
(standard normal, rounded to half FIRST so that both storages hold the same values), dense and as the 5 mm band of the same field, at
C = 64, 384 and 1024.  Points: 1 M random points inside the volume, the same for every case.  Per case, median of --runs runs after
warm-up, HIP events on the stream around --reps back-to-back calls:

    eval       BakedField.eval (no grad)                       backward   BakedField.backward with a gradient for dist and for the set
    copy       a bare device copy that moves the bytes of the eight corner rows of every row-reading point once (read + write = that size):
               the traffic of the rows with no reuse at all, the yardstick of "bound by those bytes"

and the stored row bytes of both storages.  The clock line is what the box reports right after the timed loops.

    python scripts/bench_volume_f16.py [--runs 20] [--channels 64 384 1024] [--out profiles/volume_f16/results.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import BakedField, Fusion, synth     # noqa: E402


def random_rows(m, C, dev, seed):
    """float16 [m, C] standard normal, drawn slab by slab so that no float32 array of the whole set exists"""
    rows = torch.empty((m, C), dtype=torch.float16, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    per = max(1, (1 << 28) // (4 * C))
    for q0 in range(0, m, per):
        q1 = min(q0 + per, m)
        rows[q0:q1] = torch.randn((q1 - q0, C), device=dev, generator=gen)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 384, 1024])
    ap.add_argument("--band", type=float, default=0.005)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_f16", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    geometry = f.bake(synth.WORK_BOX, 0.004, return_names=[])
    nx, ny, nz = geometry.grid_shape
    n = 1000000
    lo = torch.tensor(geometry.origin, device=dev)
    span = torch.tensor([nx - 1, ny - 1, nz - 1], device=dev) * geometry.step
    pts = (lo + torch.rand((n, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * span).contiguous()
    gd = torch.ones(n, device=dev)
    lines = ["baked-volume lookup on float32 and on half rows, %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "HIP events, median of %d runs of %d calls after warm-up (min, max); %d x %d x %d voxels, %d random points inside the volume; band %g"
             % (args.runs, args.reps, nx, ny, nz, n, args.band), ""]
    for C in args.channels:
        half_rows = random_rows(nx * ny * nz, C, dev, C).view(nx, ny, nz, C)
        dense16 = BakedField.from_arrays(geometry.origin, geometry.step, geometry.dist, valid=geometry.valid, rows_dtype=torch.float16, feat=half_rows)
        band16 = dense16.to_band(args.band)
        grad = torch.ones((n, C), device=dev)
        for kind, h in (("dense", dense16), ("band", band16)):
            w = h.float()                                   # the same values as float32 rows
            out = h.eval(pts)
            reads = out["valid_mask"] if kind == "dense" else out["in_band"]
            same = bool(torch.equal(out["feat"], w.eval(pts)["feat"]))
            del out
            res = {}
            for storage, field, width in (("float32", w, 4), ("half", h, 2)):
                def fwd(field=field):
                    with torch.no_grad():
                        return field.eval(pts)

                def bwd(field=field):
                    return field.backward(pts, gd, {"feat": grad})

                corner = int(reads.sum()) * 8 * C * width
                src = torch.empty(max(corner // 2, 1), dtype=torch.uint8, device=dev)      # a copy reads and writes its size
                dst = torch.empty_like(src)
                res[storage] = {"eval": median_ms(fwd, args.runs, args.reps), "backward": median_ms(bwd, args.runs, args.reps),
                                "copy": median_ms(lambda: dst.copy_(src), args.runs, args.reps), "corner": corner, "rows_bytes": field.rows_bytes}
                del src, dst
            lines.append("C = %d, %s: %d of %d points read rows (%.1f %%); half lookup == float32 lookup on the widened rows: %s"
                         % (C, kind, int(reads.sum()), n, 100.0 * float(reads.float().mean()), same))
            for storage in ("float32", "half"):
                r = res[storage]
                lines.append("    %-8s stored rows %8.1f MB   corner rows per call %8.1f MB" % (storage, r["rows_bytes"] / 1e6, r["corner"] / 1e6))
                for k in ("eval", "backward", "copy"):
                    med, mn, mx = r[k]
                    lines.append("        %-9s median %9.4f ms   (min %.4f, max %.4f)%s" % (k, med, mn, mx, "" if k == "copy" else "   x copy %.2f" % (med / r["copy"][0])))
            lines.append("    half / float32: eval %.3f, backward %.3f, stored bytes %.3f"
                         % (res["half"]["eval"][0] / res["float32"]["eval"][0], res["half"]["backward"][0] / res["float32"]["backward"][0],
                            res["half"]["rows_bytes"] / max(res["float32"]["rows_bytes"], 1)))
            del w
        del dense16, band16, half_rows, grad
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
