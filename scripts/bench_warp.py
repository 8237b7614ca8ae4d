"""Times the warp of a baked field by the rigid motions of its parts (d3f_volume_warp_select / d3f_volume_warp_rows, csrc/warp_kernels.hip;
BakedField.warp) on the synthetic smooth scene (needs an MI355X) and writes profiles/warp/results.txt.  No thresholds: the file reports,
nothing is asserted.

Volume: the 200 x 175 x 55 bake (4 mm).  Configurations: dense with one 384-channel set, and the 5 mm band with one 1024-channel set, each
with 1 and with 5 movers.  The parts are five slabs of the occupied shell along x, grown by owners(margin_voxels=2); every part has a planted
pose (a turn of up to 10 degrees about its centre, a shift of up to 2 voxels) and `which` selects the movers.  Contenders, ALTERNATED inside
one run, each timed --runs times with device events after a warm-up round; medians (min, max):

    select   d3f_volume_warp_select alone, on preallocated outputs
    rows     d3f_volume_warp_rows alone (dense: every voxel; banded: the stored voxels of the warped field)
    warp     BakedField.warp as a whole: the allocations, select, (banded: d3f_band_mark with its host read,) rows
    recipe   what the call replaces, dense only, existing code of this commit: per mover the inverse-mapped voxel centres, one eval() over the
             whole volume and torch.where on the distances
    clone    a bare clone of the row array: the memory bound of writing the rows once

    python scripts/bench_warp.py [--runs 7] [--out profiles/warp/results.txt]
"""
import argparse
import ctypes
import datetime
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit     # noqa: E402
from bench_pool import with_set     # noqa: E402
from d3fields_amd import Fusion, _lib, synth     # noqa: E402


def planted_poses(labels, K, gen):
    """float64 [K, 15]: a turn of up to 10 degrees about the part's centre and a shift of up to 2 voxels"""
    dev = labels.device
    axis = torch.nn.functional.normalize(torch.randn((K, 3), dtype=torch.float64, device=dev, generator=gen), dim=1)
    angle = math.radians(10.0) * torch.rand((K,), dtype=torch.float64, device=dev, generator=gen)
    x, y, z = axis.unbind(1)
    zero = torch.zeros_like(x)
    skew = torch.stack((zero, -z, y, z, zero, -x, -y, x, zero), dim=1).view(K, 3, 3)
    rot = torch.eye(3, dtype=torch.float64, device=dev) + angle.sin()[:, None, None] * skew + (1 - angle.cos())[:, None, None] * (skew @ skew)
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float64) for n in labels.shape], indexing="ij"), dim=-1)
    src = torch.stack([grid[labels == k + 1].mean(dim=0) for k in range(K)])
    shift = 4.0 * torch.rand((K, 3), dtype=torch.float64, device=dev, generator=gen) - 2.0
    return torch.cat((rot.reshape(K, 9), src, src + shift), dim=1)


def recipe(field, name, pose, movers, owner):
    """the recipe the call replaces: K full-volume lookups and K row arrays"""
    dev = field.device
    shape = field.grid_shape
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float64) for n in shape], indexing="ij"), dim=-1).view(-1, 3)
    origin = torch.tensor(field.origin, dtype=torch.float64, device=dev)
    moving = torch.zeros(pose.shape[0] + 1, dtype=torch.bool, device=dev)
    moving[torch.as_tensor(movers, device=dev) + 1] = True
    stays = field.valid.view(-1) & ~moving[owner.view(-1).long()]
    dist = torch.where(stays, field.dist.view(-1), torch.full_like(field.dist.view(-1), 1e3))
    rows = field._sets[name].view(-1, field._sets[name].shape[-1]).clone()
    hi = torch.tensor(shape, device=dev) - 1
    strides = torch.tensor([shape[1] * shape[2], shape[2], 1], device=dev)
    for k in movers:
        R, src, dst = pose[k, :9].view(3, 3), pose[k, 9:12], pose[k, 12:15]
        p = (grid - dst) @ R + src                                   # R^T (q - dst) + src
        out = field.eval((origin + p * field.step).float(), return_names=[name])
        idx = p.round().long()                                       # the voxel nearest to the image must be the part's own
        near = ((idx >= 0) & (idx <= hi)).all(dim=1) & (owner.view(-1)[(torch.minimum(idx.clamp(min=0), hi) * strides).sum(dim=1)] == k + 1)
        take = out["valid_mask"] & near & (out["dist"] < dist)
        dist = torch.where(take, out["dist"], dist)
        rows = torch.where(take[:, None], out[name], rows)
    return dist, rows


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp", "results.txt"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five repetitions, so that the spread is visible"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    step, K = 0.004, 5
    base = f.bake(synth.WORK_BOX, step, return_names=[])
    nx, ny, nz = base.grid_shape
    n = nx * ny * nz
    gen = torch.Generator(device=dev).manual_seed(23)
    shell = base.valid & (base.dist <= step)
    slab = (torch.arange(nx, device=dev) * K // nx).view(nx, 1, 1).expand(nx, ny, nz)
    labels = torch.where(shell, slab + 1, torch.zeros_like(slab)).to(torch.int32).contiguous()
    owner = base.owners(labels, margin_voxels=2)
    pose = planted_poses(labels, K, gen)
    lines = ["warp of a baked field by the rigid motions of its parts (d3f_volume_warp_select, d3f_volume_warp_rows), %s, %s, commit %s"
             % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine, ONE run of this script; device events, the contenders alternated, median of %d calls each after one warm-up round (min, max); "
             "scene: synth smooth, %d views of %d x %d" % (args.runs, V, H, W),
             "%d x %d x %d = %.2f M voxels (step %g m); %d parts (slabs of the occupied shell, %d voxels; owners with a margin of 2: %d voxels); "
             "one change since the first form: a box word is read before it is min / maxed (DESIGN.md 28.1)" % (nx, ny, nz, n / 1e6, step, K, int((labels > 0).sum()), int((owner > 0).sum())), ""]
    for kind, C in (("dense", 384), ("band 5 mm", 1024)):
        if kind == "dense":
            field = with_set(base, "feat", torch.randn((nx, ny, nz, C), device=dev, generator=gen))
            row_array = field._sets["feat"]
        else:
            mark = base._mark(0.005)
            field = with_set(base, "feat", torch.randn((mark[2].shape[0], C), device=dev, generator=gen), mark, 0.005)
            row_array = field._sets["feat"]
        for movers in ([2], list(range(K))):
            which = torch.zeros(K, dtype=torch.bool, device=dev)
            which[movers] = True
            masked = torch.where(which[:, None], pose, torch.full_like(pose, math.nan))
            w = field.warp(pose, owner, which=which)
            moved = int((w.source > 0).sum())
            # the two entry points alone, on the buffers of that result
            source, dist, valid = torch.empty_like(w.source), torch.empty_like(w.dist), torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
            boxes = torch.empty((K, 12), dtype=torch.int32, device=dev)
            sel = _lib.WarpSelect(field._volume(), _lib.ptr(owner), _lib.ptr(masked), K, 0, _lib.ptr(source), _lib.ptr(dist), _lib.ptr(valid), _lib.ptr(boxes))
            stream = _lib.current_stream_handle(dev)
            voxels = None if field.band is None else w.band_voxels
            m = n if voxels is None else voxels.shape[0]
            out_rows, known = torch.empty((m, C), dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
            outs = (ctypes.c_void_p * 1)(out_rows.data_ptr())
            band = None if field.band is None else field._band_struct()
            sets = field._set_array(["feat"])
            rws = _lib.WarpRows(field._volume(), None if band is None else ctypes.pointer(band), sets, 1, K, _lib.ptr(w.source), _lib.ptr(masked), _lib.ptr(voxels), m,
                                outs, _lib.ptr(known))
            contenders = {"select": lambda: _lib.check(lib.d3f_volume_warp_select(ctypes.byref(sel), stream)),
                          "rows": lambda: _lib.check(lib.d3f_volume_warp_rows(ctypes.byref(rws), stream)),
                          "warp": lambda: field.warp(pose, owner, which=which),
                          "clone": lambda: row_array.clone()}
            if kind == "dense":
                contenders["recipe"] = lambda: recipe(field, "feat", pose, movers, owner)
            times = {k: [] for k in contenders}
            for r in range(args.runs + 1):                               # round 0 warms up
                for k, fn in contenders.items():
                    t = timed(fn)
                    if r > 0:
                        times[k].append(t)
            assert torch.equal(source, w.source) and torch.equal(out_rows, w._sets["feat"].view(-1, C))
            med = {k: statistics.median(v) for k, v in times.items()}
            lines.append("%s, C = %d, %d mover%s: %d voxels won by a part, %d rows written (%.2f GB)"
                         % (kind, C, len(movers), "" if len(movers) == 1 else "s", moved, m, m * C * 4 / 1e9))
            for k, v in times.items():
                lines.append("    %-7s %9.3f ms (min %.3f, max %.3f)%s" % (k, med[k], min(v), max(v),
                                                                            "" if k in ("clone", "select") else "    = %.2f x clone" % (med[k] / med["clone"])))
            if "recipe" in med:
                lines.append("    recipe / warp = %.2f" % (med["recipe"] / med["warp"]))
            lines.append("")
            del w, source, dist, valid, out_rows, known
            torch.cuda.empty_cache()
        del field, row_array
        torch.cuda.empty_cache()
    lines.insert(1, clock_line())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
