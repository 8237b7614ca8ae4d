"""Timing of the projected query (Fusion.add_projection) on one MI355X -> profiles/projection/results.txt.

    python scripts/bench_projection.py [--runs 20] [--warmup 3] [--shapes ref_patch,c2_dense,c4_dense] [--out PATH]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_projection.py --trace ref_patch [--trace-k 3]

1. d3f_project_maps on the map shapes of bench.py's ref_patch / c2_dense / c4_dense workloads with heads of k = 3, 16, 64,
   against a plain streaming read of the same bytes in the same run (d3f_map_check: 16-byte loads, nothing else); both are
   one library call per timed run, the output allocated beforehand.  On a map of tens of megabytes an event pair around one
   launch is mostly launch, so --trace runs the two kernels of one row alone for a kernel trace, which gives kernel time.
2. End to end on ref_patch (the 1.925 M-point lattice and the surface cloud of vis_repr.py:97-103), k = 3: the projected
   query with and without the once-per-observation projection, against the old route batch_eval(['dino_feats']) +
   mesh.pca_project timed in the same run.
Every figure is the median of --runs runs after --warmup warm-up runs, the routes compared taking turns run by run, HIP
events on one stream, clocks as the device
runs them (not pinned; the current SCLK is printed).  There is no CPU fallback: without the device this script fails.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402  (workload shapes and point sets)
from d3fields_amd import _lib, mesh                   # noqa: E402


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating_medians(fns, runs, warmup):
    """[(median, min, max) ms] per function: every function is warmed up, then the functions take turns, one timed run each
    per round, so that none of them owns a quieter stretch of the machine."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            times[i].append(timed_ms(fn))
    return [(statistics.median(t), min(t), max(t)) for t in times]


class Head:
    def __init__(self, k, C, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.components_ = torch.randn(k, C, generator=g).numpy()
        self.mean_ = torch.randn(C, generator=g).numpy()


def kernel_pair(lib, src, k, dev):
    """(read, project): one launch each on `src` -- d3f_map_check, and d3f_project_maps through a k-row head into a
    buffer allocated here, so a timed run holds no allocation and no Python beyond one ctypes call."""
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    W = torch.from_numpy(Head(k, src.shape[3], seed=k).components_).to(dev, torch.float32).contiguous()
    dst = torch.empty(src.shape[0], src.shape[1], src.shape[2], k, dtype=torch.float32, device=dev)
    desc = _lib.ChannelMap(src.data_ptr(), src.shape[1], src.shape[2], src.shape[3], _lib.DTYPE_F16 if src.dtype == torch.float16 else _lib.DTYPE_F32,
                           src.stride(0), src.stride(1), src.stride(2), None)
    stream = _lib.current_stream_handle(dev)
    keep = (word, W, dst, desc)

    def read():
        _lib.check(lib.d3f_map_check(ctypes.byref(desc), src.shape[0], _lib.ptr(word), stream))

    def project():
        _lib.check(lib.d3f_project_maps(ctypes.byref(desc), src.shape[0], _lib.ptr(W), k, _lib.ptr(dst), stream))
    read.keep = project.keep = keep
    return read, project


def kernel_table(shapes, runs, warmup, dev, say):
    lib = _lib.load()
    say("1. d3f_project_maps against a streaming read of the same bytes (d3f_map_check); one launch per timed run, output pre-allocated")
    say("%-10s %-22s %8s %4s %10s %10s %8s %9s" % ("workload", "map", "GB", "k", "project ms", "read ms", "ratio", "TB/s"))
    for name in shapes:
        f, _, _, _, _ = bench.build_workload(name, dev, 0, 1, points="random")
        src = f.curr_obs_torch["dino_feats"]
        nbytes = src.numel() * src.element_size()
        for k in (3, 16, 64):
            read, project = kernel_pair(lib, src, k, dev)
            (rd, _, _), (pj, _, _) = alternating_medians([read, project], runs, warmup)
            say("%-10s %-22s %8.2f %4d %10.3f %10.3f %8.2f %9.2f" % (name, "%dx%dx%dx%d" % tuple(src.shape), nbytes / 1e9, k, pj, rd, pj / rd,
                                                                nbytes / (pj * 1e-3) / 1e12))
            del read, project
        del f, src
        torch.cuda.empty_cache()


def trace_loop(name, k, runs, warmup, dev):
    """The two kernels of one table row and nothing else, for a kernel trace: --warmup + --runs launches of each."""
    f, _, _, _, _ = bench.build_workload(name, dev, 0, 1, points="random")
    read, project = kernel_pair(_lib.load(), f.curr_obs_torch["dino_feats"], k, dev)
    for _ in range(warmup + runs):
        read()
        project()
    torch.cuda.synchronize()


def end_to_end(runs, warmup, dev, say):
    say("")
    say("2. end to end on ref_patch (4 views, 48x64x1024 fp32 patch maps), k = 3")
    say("%-28s %10s %18s %22s %22s" % ("points", "n", "old route ms", "projected, cached ms", "projected, incl. ms"))
    for points in ("surface", "grid"):
        f, pts, _, _, _ = bench.build_workload("ref_patch", dev, 0, 1, points=points)
        pca = Head(3, 1024, seed=3)
        f.add_projection("pca", pca=pca)

        def old():
            with torch.no_grad():
                return mesh.pca_project(pca, f.batch_eval(pts, return_names=["dino_feats"])["dino_feats"])

        def cached():
            with torch.no_grad():
                return f.batch_eval(pts, return_names=["pca"])["pca"]

        def included():
            f._projected.clear()
            return cached()
        err = float((cached().double() - old()).abs().max())
        o, c, i = alternating_medians([old, cached, included], runs, warmup)
        say("%-28s %10d %18s %22s %22s" % ("surface cloud" if points == "surface" else "lattice", pts.shape[0],
                                          "%.3f [%.3f, %.3f]" % o, "%.3f [%.3f, %.3f]" % c, "%.3f [%.3f, %.3f]" % i))
        say("    max |projected - old route| = %.3g;  projected route incl. projection is %.2fx the old route's time" % (err, i[0] / o[0]))
        del f
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ref_patch,c2_dense,c4_dense")
    ap.add_argument("--trace", default="", help="workload whose read and projection kernels run alone (under rocprofv3); writes no table")
    ap.add_argument("--trace-k", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection", "results.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_projection.py needs the MI355X; nothing is measured without it")
    if args.runs < 20:
        raise SystemExit("medians of at least 20 runs")
    dev = torch.device("cuda:0")
    if args.trace:
        trace_loop(args.trace, args.trace_k, args.runs, args.warmup, dev)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()
    try:
        clock = "%d MHz" % torch.cuda.clock_rate(dev)
    except Exception:
        clock = "not readable"
    say("device: %s; SCLK now: %s (clocks not pinned); median [min, max] of %d runs after %d warm-up runs, HIP events, one stream"
        % (torch.cuda.get_device_name(dev), clock, args.runs, args.warmup))
    kernel_table([s for s in args.shapes.split(",") if s], args.runs, args.warmup, dev, say)
    end_to_end(args.runs, args.warmup, dev, say)
    out.close()


if __name__ == "__main__":
    main()
