"""Timing of the PCA fit (d3fields_amd/pca.py, d3f_row_moments) on one MI355X -> profiles/pca_fit/results.txt.

    python scripts/bench_pca_fit.py [--runs 20] [--warmup 3] [--shapes ref_patch,c2_dense,c4_dense] [--out PATH]

Per map (the dino_feats maps of bench.py's ref_patch / c2_dense / c4_dense workloads; a map that does not fit the device is
skipped and said so): one d3f_row_moments call (workspace and outputs allocated beforehand) against a plain streaming read of
the same bytes (d3f_map_check: 16-byte loads, nothing else) and against torch's X^T X on the same rows (one fp32 matmul: an
UNCENTRED Gram matrix in a single fp32 accumulation, i.e. less than the fit needs), all in the same run, taking turns run by
run.  Then the host eigen-solve (numpy.linalg.eigh in float64) of the C x C scatter, wall clock.  Every device figure is the
median of --runs runs after --warmup warm-up runs, HIP events on one stream, clocks as the device runs them (not pinned).
There is no CPU fallback: without the device this script fails.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                          # noqa: E402  (workload shapes)
from d3fields_amd import _lib                         # noqa: E402


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


def routes(lib, src, dev):
    """(read, moments, gram, scatter tensor): one library call / one matmul per timed run on `src` [V,fh,fw,C]"""
    V, fh, fw, C = src.shape
    M = V * fh * fw
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    desc = _lib.ChannelMap(src.data_ptr(), fh, fw, C, _lib.DTYPE_F32, src.stride(0), src.stride(1), src.stride(2), None)
    out = torch.empty(1 + C + C * C, dtype=torch.float64, device=dev)
    nbytes = int(lib.d3f_row_moments_workspace_bytes(M, C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gram_out = torch.empty(C, C, dtype=torch.float32, device=dev)
    rows = src.view(M, C)
    stream = _lib.current_stream_handle(dev)

    def read():
        _lib.check(lib.d3f_map_check(ctypes.byref(desc), V, _lib.ptr(word), stream))

    def moments():
        _lib.check(lib.d3f_row_moments(_lib.ptr(src), _lib.DTYPE_F32, M, C, C, None, _lib.ptr(out[0:1]), _lib.ptr(out[1:1 + C]), _lib.ptr(out[1 + C:]),
                                       _lib.ptr(ws), nbytes, stream))

    def gram():
        torch.matmul(rows.T, rows, out=gram_out)
    read.keep = moments.keep = gram.keep = (word, desc, out, ws, gram_out, rows)
    return read, moments, gram, out[1 + C:].view(C, C), nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ref_patch,c2_dense,c4_dense")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_fit", "results.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca_fit.py needs the MI355X; nothing is measured without it")
    if args.runs < 20:
        raise SystemExit("medians of at least 20 runs")
    dev = torch.device("cuda:0")
    lib = _lib.load()
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
    say("d3f_row_moments against a streaming read of the same bytes (d3f_map_check) and torch's fp32 X^T X on the same rows")
    say("%-10s %-20s %7s %9s %24s %24s %24s %7s %7s %8s" % ("workload", "map", "GB", "Tflop", "moments ms", "read ms", "torch X^T X ms", "x read", "x gram",
                                                            "Tflop/s"))
    for name in [s for s in args.shapes.split(",") if s]:
        try:
            f, _, _, _, _ = bench.build_workload(name, dev, 0, 1, points="random")
            src = f.curr_obs_torch["dino_feats"]
            if src.dtype != torch.float32 or not src.is_contiguous():
                src = src.float().contiguous()
            read, moments, gram, scatter, ws_bytes = routes(lib, src, dev)
        except torch.cuda.OutOfMemoryError:
            say("%-10s does not fit this device next to its workspace: skipped" % name)
            torch.cuda.empty_cache()
            continue
        V, fh, fw, C = src.shape
        M = V * fh * fw
        nbytes, flop = src.numel() * 4, 2.0 * M * C * C
        rd, mo, gr = alternating_medians([read, moments, gram], args.runs, args.warmup)
        say("%-10s %-20s %7.2f %9.3f %24s %24s %24s %7.2f %7.2f %8.1f" % (name, "%dx%dx%dx%d" % tuple(src.shape), nbytes / 1e9, flop / 1e12,
                                                                         "%.3f [%.3f, %.3f]" % mo, "%.3f [%.3f, %.3f]" % rd, "%.3f [%.3f, %.3f]" % gr,
                                                                         mo[0] / rd[0], mo[0] / gr[0], flop / (mo[0] * 1e-3) / 1e12))
        S = scatter.cpu().numpy()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            np.linalg.eigh(S)
            t.append(time.perf_counter() - t0)
        say("    workspace %.1f MB; host numpy.linalg.eigh (float64, C = %d): %.3f s (best of 3)" % (ws_bytes / 1e6, C, min(t)))
        del f, src, read, moments, gram, scatter
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
