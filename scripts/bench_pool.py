"""Times per-component pooling (d3f_volume_pool, csrc/pool_kernels.hip; BakedField.pool) on the synthetic smooth scene (needs an MI355X)
and writes profiles/pool/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_components.py: HIP events on the stream, median of --runs runs after warm-up; the header carries the date, the
commit and the shader clock.  Volumes: the 200 x 175 x 55 bake (4 mm) and the 1 mm grid of the same box; components of valid & dist <= 0
plus 0.1 % of the voxels as random single-voxel floaters, connectivity 26, min_voxels 1 and 50.  Fields: one 384-channel set stored
densely (where the device has room for it), one 1024-channel set in a band of two steps; the rows are random numbers -- the time does not
depend on them.  Next to every time, measured in the same run:

    copy    a bare index_select copy of exactly the member rows: the byte floor of any pooling
    add     that copy followed by torch index_add_ into [K, C] and the division: float atomics, not reproducible
    loop    the per-object recipe pool replaces (a mask, the voxel centres, one eval, one mean per object) for the five largest objects

    python scripts/bench_pool.py [--runs 10] [--out profiles/pool/results.txt]
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
from d3fields_amd import Fusion, synth     # noqa: E402

FLOATERS = 0.001


def with_set(field, name, rows, mark=None, band=None):
    """a field that shares `field`'s dist / valid and holds one random set: dense [nx,ny,nz,C], or [M,C] behind the band's slot volume"""
    if mark is None:
        return type(field)(field.origin, field.step, field.dist, field.valid, {name: rows}, {name: None}, boundaries=field.boundaries, axes=field._axes)
    return field._banded(band, mark, {name: rows}, {name: None})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--steps", default="0.004,0.001")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool", "results.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["per-component pooling (d3f_volume_pool), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; HIP events, median of %d runs after warm-up (a third as many from 2^24 voxels on; min, max); scene: synth smooth, %d views of %d x %d"
             % (args.runs, V, H, W), ""]
    gen = torch.Generator(device="cpu").manual_seed(17)
    for step in [float(s) for s in args.steps.split(",")]:
        base = f.bake(synth.WORK_BOX, step, return_names=[])
        nx, ny, nz = base.grid_shape
        n = nx * ny * nz
        shell = base.valid & (base.dist <= 0.0)
        floaters = torch.zeros(n, dtype=torch.bool)
        floaters[torch.randint(0, n, (int(FLOATERS * n),), generator=gen)] = True
        sites = (shell | floaters.view(nx, ny, nz).to(dev)).contiguous()
        del shell, floaters
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 3)
        lines.append("%d x %d x %d = %.2f M voxels (step %g m); device times here: median of %d runs" % (nx, ny, nz, n / 1e6, step, runs))
        band = 2.0 * step
        mark = base._mark(band)
        for kind, C in (("dense", 384), ("band", 1024)):
            rows_n = n if kind == "dense" else int(mark[2].shape[0])
            need = 4 * rows_n * C
            free = torch.cuda.mem_get_info(dev)[0]
            if need > 0.45 * free:
                lines.append("  %s, %d channels: the rows alone are %.1f GB of %.1f GB free -- not run at this size" % (kind, C, need / 1e9, free / 1e9))
                continue
            rows = torch.empty((rows_n, C), dtype=torch.float32, device=dev).normal_()
            field = with_set(base, "feat", rows.view(nx, ny, nz, C)) if kind == "dense" else with_set(base, "feat", rows, mark, band)
            for min_voxels in (1, 50):
                comp = field.components(sites=sites, min_voxels=min_voxels)
                K = comp.count
                member = (comp.labels > 0) & field.valid
                if kind == "band":
                    member &= field.slot >= 0
                vox = member.view(-1).nonzero().view(-1)
                keys = (comp.labels.view(-1)[vox] - 1).long()
                at = vox if kind == "dense" else field.slot.view(-1)[vox].long()
                members = int(vox.numel())
                sizes = torch.bincount(keys, minlength=K)
                del member, vox
                med, lo, hi = median_ms(lambda: field.pool(comp), runs, 1)
                text = "  %-5s %4d channels, min_voxels %2d: K %7d, %9d members (largest %9d, median %d)   pool %9.3f ms (min %.3f, max %.3f)" % (
                    kind, C, min_voxels, K, members, int(sizes.max()) if K else 0, int(sizes.median()) if K else 0, med, lo, hi)
                gb = 4.0 * members * C / 1e9
                if 2 * 4 * members * C < 0.8 * torch.cuda.mem_get_info(dev)[0]:
                    cmed, clo, chi = median_ms(lambda: rows.index_select(0, at), runs, 1)
                    text += "   copy of %.2f GB: %.3f ms (min %.3f, max %.3f)" % (gb, cmed, clo, chi)

                    def add():
                        out = torch.zeros((K, C), dtype=torch.float32, device=dev)
                        out.index_add_(0, keys, rows.index_select(0, at))
                        return out / sizes[:, None]

                    amed, alo, ahi = median_ms(add, runs, 1)
                    text += "   copy + index_add_ + divide: %.3f ms (min %.3f, max %.3f)" % (amed, alo, ahi)
                else:
                    text += "   copy / index_add_: no room for the %.2f GB of gathered rows" % gb
                lines.append(text)
                top = comp.largest(5).tolist()

                def loop():
                    flat = comp.labels.view(-1)
                    for k in top:
                        if kind == "band":
                            pts = field.band_points()[flat[field.band_voxels.long()] == k]
                        else:
                            pts = field._voxel_centres((flat == k).nonzero().view(-1))
                        field.eval(pts)["feat"].mean(dim=0)

                lmed, llo, lhi = median_ms(loop, max(3, runs // 2), 1, warmup=1)
                lines.append("        the per-object loop for the %d largest objects (%d voxels): %.3f ms (min %.3f, max %.3f)" % (len(top), int(sizes[torch.tensor(top, device=dev) - 1].sum()) if top else 0, lmed, llo, lhi))
                del comp, keys, at, sizes
            del field, rows
            torch.cuda.empty_cache()
        lines.append("")
        del base, sites, mark
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
