"""Times the merge of two baked fields (d3f_volume_merge_select / d3f_volume_merge_rows, csrc/merge_kernels.hip; BakedField.merge) on the
synthetic smooth scene (needs an MI355X) and writes profiles/merge/results.txt.  No thresholds: the file reports, nothing is asserted.

Volume: the 200 x 175 x 55 bake (4 mm).  The older field is that bake; the newer one is the same bake with a box of voxels invalidated (an
occluder) and its distances shifted by a quarter step, so that every kind but RESET occurs.  Configurations: dense with one 384-channel set,
dense with one 64-channel set, and the 5 mm band with one 1024-channel set (both fields banded).  Contenders, ALTERNATED inside one run, each
timed --runs times with device events after a warm-up round; medians (min, max):

    select   d3f_volume_merge_select alone, on preallocated outputs
    rows     d3f_volume_merge_rows alone (dense: every voxel; banded: the stored voxels of the merged field)
    merge    BakedField.merge as a whole: the allocations, select, (banded: d3f_band_mark with its host read,) rows
    recipe   what the call replaces, dense only: torch.where / lerp passes over the dense arrays
    clone    a bare clone of the output rows: the memory bound of writing them once (the merge reads up to two rows per row written)

    python scripts/bench_merge.py [--runs 7] [--out profiles/merge/results.txt]
"""
import argparse
import ctypes
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit     # noqa: E402
from bench_pool import with_set     # noqa: E402
from bench_warp import timed     # noqa: E402
from d3fields_amd import Fusion, _lib, synth     # noqa: E402


def recipe(a, b, name):
    """the recipe the call replaces (equal scalar weights, no cap, no reset): several dense [nx,ny,nz,C] temporaries"""
    ua, ub = a.valid & ~a.dist.isnan(), b.valid & ~b.dist.isnan()
    both = ua & ub
    half = torch.full_like(a.dist, 0.5)
    dist = torch.where(both, torch.lerp(a.dist, b.dist, half), torch.where(ua, a.dist, torch.where(ub, b.dist, torch.full_like(a.dist, 1e3))))
    ra, rb = a._sets[name], b._sets[name]
    rows = torch.where(both[..., None], torch.lerp(ra, rb, 0.5), torch.where(ua[..., None], ra, torch.where(ub[..., None], rb, torch.zeros_like(ra))))
    return dist, ua | ub, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "results.txt"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five repetitions, so that the spread is visible"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    step = 0.004
    base = f.bake(synth.WORK_BOX, step, return_names=[])
    nx, ny, nz = base.grid_shape
    n = nx * ny * nz
    gen = torch.Generator(device=dev).manual_seed(29)
    valid_b = base.valid.clone()
    valid_b[nx // 3: nx // 2, ny // 4: ny // 2, :] = False
    newer = type(base)(base.origin, base.step, (base.dist + 0.25 * step).contiguous(), valid_b, {}, {}, boundaries=base.boundaries, axes=base._axes)
    lines = ["merge of two baked fields (d3f_volume_merge_select, d3f_volume_merge_rows), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, ONE run of this script; device events, the contenders alternated, median of %d calls each after one warm-up round (min, max); "
             "scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W),
             "%d x %d x %d = %.2f M voxels (step %g m); the newer field: %d voxels invalidated, distances shifted by a quarter step" % (nx, ny, nz, n / 1e6, step, int((base.valid & ~valid_b).sum())), ""]
    for kind, C in (("dense", 384), ("dense", 64), ("band 5 mm", 1024)):
        if kind == "dense":
            a = with_set(base, "feat", torch.randn((nx, ny, nz, C), device=dev, generator=gen))
            b = with_set(newer, "feat", torch.randn((nx, ny, nz, C), device=dev, generator=gen))
        else:
            mark_a, mark_b = base._mark(0.005), newer._mark(0.005)
            a = with_set(base, "feat", torch.randn((mark_a[2].shape[0], C), device=dev, generator=gen), mark_a, 0.005)
            b = with_set(newer, "feat", torch.randn((mark_b[2].shape[0], C), device=dev, generator=gen), mark_b, 0.005)
        m0 = a.merge(b)
        kinds = torch.bincount(m0.merged_from.view(-1).long(), minlength=5).tolist()
        # the two entry points alone, on buffers of their own
        out = {k: torch.empty_like(m0.dist) for k in ("dist", "weight", "beta")}
        out_valid, out_kind = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev), torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
        sel = _lib.MergeSelect(nx, ny, nz, 0, _lib.ptr(a.dist), _lib.ptr(a.valid), None, _lib.ptr(b.dist), _lib.ptr(b.valid), None, 1.0, 1.0, float("inf"), float("inf"),
                               _lib.ptr(out["dist"]), _lib.ptr(out["weight"]), _lib.ptr(out["beta"]), _lib.ptr(out_valid), _lib.ptr(out_kind))
        stream = _lib.current_stream_handle(dev)
        _lib.check(lib.d3f_volume_merge_select(ctypes.byref(sel), stream))
        voxels = None if m0.band is None else m0.band_voxels
        m = n if voxels is None else voxels.shape[0]
        out_rows, known = torch.empty((m, C), dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
        outs = (ctypes.c_void_p * 1)(out_rows.data_ptr())
        band_a, band_b = (None, None) if a.band is None else (a._band_struct(), b._band_struct())
        sets_a, sets_b = a._set_array(["feat"]), b._set_array(["feat"])
        rws = _lib.MergeRows(nx, ny, nz, 1, None if band_a is None else ctypes.pointer(band_a), None if band_b is None else ctypes.pointer(band_b), sets_a, sets_b,
                             _lib.ptr(out_kind), _lib.ptr(out["beta"]), _lib.ptr(voxels), m, outs, _lib.ptr(known), 0)
        contenders = {"select": lambda: _lib.check(lib.d3f_volume_merge_select(ctypes.byref(sel), stream)),
                      "rows": lambda: _lib.check(lib.d3f_volume_merge_rows(ctypes.byref(rws), stream)),
                      "merge": lambda: a.merge(b),
                      "clone": lambda: out_rows.clone()}
        if kind == "dense":
            contenders["recipe"] = lambda: recipe(a, b, "feat")
        times = {k: [] for k in contenders}
        for r in range(args.runs + 1):                               # round 0 warms up
            for k, fn in contenders.items():
                t = timed(fn)
                if r > 0:
                    times[k].append(t)
        assert torch.equal(out_kind, m0.merged_from) and torch.equal(out_rows, m0._sets["feat"].view(-1, C))
        med = {k: statistics.median(v) for k, v in times.items()}
        read = sum(int(kinds[k]) * w for k, w in ((1, 1), (2, 1), (3, 2), (4, 1))) if kind == "dense" else None
        lines.append("%s, C = %d: %d rows written (%.2f GB)%s; kinds none / keep / new / blend / reset = %s"
                     % (kind, C, m, m * C * 4 / 1e9, "" if read is None else ", %.2f GB of rows read" % (read * C * 4 / 1e9), " / ".join(str(k) for k in kinds)))
        for k, v in times.items():
            lines.append("    %-7s %9.3f ms (min %.3f, max %.3f)%s" % (k, med[k], min(v), max(v), "" if k in ("clone", "select") else "    = %.2f x clone" % (med[k] / med["clone"])))
        if "recipe" in med:
            lines.append("    recipe / merge = %.2f" % (med["recipe"] / med["merge"]))
        lines.append("")
        del a, b, m0, out_rows, known, out, contenders
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
