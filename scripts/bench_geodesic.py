"""Times the cost-to-go solve (d3f_volume_geodesic_init / _relax / _finish, csrc/geodesic_kernels.hip; BakedField.travel) on the synthetic
smooth scene (needs an MI355X) and writes profiles/geodesic/results.txt.  No thresholds: the file reports, nothing is asserted.

Method of scripts/bench_components.py: HIP events on the stream, median of --runs runs after warm-up at 4 mm and of a quarter as many at
1 mm; the header carries the date, the commit and the shader clock.  Scene: the 4 mm bake of the work box and the 1 mm grid of the same box,
c = clearance(unknown="occupied", min_voxels=50), free = c.valid & (c.dist >= 0.03), one goal: the free voxel nearest to the middle of the
box.  A solve is timed as BakedField.travel runs it -- init, batches of 16, 32, ... 256 rounds with one host read each, finish -- so the
time includes those reads.  Next to every time, measured in the same run:

    rounds, tile runs   from a second solve driven one round per call: the rounds until no tile is listed, and the tiles listed over all rounds
    copy                a bare device pass over the algorithmic bytes: one byte read and four bytes written per voxel
    scipy               scipy.sparse.csgraph.dijkstra on the host over the same graph (26 moves, weights 3 / 4 / 5), at 4 mm and where scipy imports

    python scripts/bench_geodesic.py [--runs 20] [--steps 0.004,0.001] [--out profiles/geodesic/results.txt]
"""
import argparse
import ctypes
import datetime
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_volume import clock_line, commit, median_ms     # noqa: E402
from d3fields_amd import Fusion, _lib, synth     # noqa: E402

RADIUS = 0.03
WEIGHTS = (3, 4, 5)


def count_rounds(lib, free_u8, goal, conn, dev):
    """one solve, one round per call -> (rounds until the list is empty, tile runs, tiles in the volume)"""
    nx, ny, nz = free_u8.shape
    cost = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
    pending = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.d3f_volume_geodesic_workspace_bytes(nx, ny, nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    w = (ctypes.c_int32 * 3)(*WEIGHTS)
    stream = _lib.current_stream_handle(dev)
    _lib.check(lib.d3f_volume_geodesic_init(_lib.ptr(free_u8), nx, ny, nz, _lib.ptr(goal), 1, _lib.ptr(cost), _lib.ptr(ws), ws_bytes, stream))
    listed = int(ws[:4].view(torch.int32).item())      # the workspace's first word: the length of the tile list
    rounds, runs = 0, 0
    while listed > 0:
        runs += listed
        rounds += 1
        _lib.check(lib.d3f_volume_geodesic_relax(_lib.ptr(free_u8), None, nx, ny, nz, conn, w, 2 ** 31 - 2, 1, _lib.ptr(cost), _lib.ptr(pending), _lib.ptr(ws),
                                                 ws_bytes, stream))
        listed = int(pending.item())
    return rounds, runs, (ws_bytes // 4 - 16) // 2


def host_dijkstra_ms(free, goal, conn):
    """wall clock of scipy's Dijkstra alone (the graph is built before the clock starts) -> (ms, cost int64 [n])"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    shape = np.array(free.shape)
    at = np.argwhere(free)
    rows, cols, vals = [], [], []
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1
        l1 = int(np.abs(d).sum())
        if l1 == 0 or l1 > {6: 1, 18: 2, 26: 3}[conn]:
            continue
        to = at + d
        ok = ((to >= 0) & (to < shape)).all(axis=1)
        ok[ok] = free[to[ok, 0], to[ok, 1], to[ok, 2]]
        rows.append(np.ravel_multi_index(at[ok].T, free.shape))
        cols.append(np.ravel_multi_index(to[ok].T, free.shape))
        vals.append(np.full(int(ok.sum()), float(WEIGHTS[l1 - 1])))
    graph = csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(free.size, free.size))
    t0 = time.perf_counter()
    d = dijkstra(graph, directed=True, indices=[goal], min_only=True)
    ms = 1e3 * (time.perf_counter() - t0)
    return ms, np.where(np.isinf(d), 2 ** 31 - 1, d).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", default="0.004,0.001")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic", "results.txt"))
    args = ap.parse_args()
    try:
        import scipy.sparse.csgraph     # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    lib = _lib.load()
    V, H, W = 4, 480, 640
    sc = synth.make_scene(V, H, W, "smooth")
    f = Fusion(num_cam=V, device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    lines = ["cost-to-go (d3f_volume_geodesic_*, BakedField.travel), %s, %s, commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), commit()),
             "one machine; device times: HIP events around the whole solve (init, batches of 16 .. 256 rounds with one host read each, finish), median of %d runs "
             "after warm-up (a quarter as many from 2^24 voxels on; min, max); host time: wall clock, one run; scene: synth smooth, %d views of %d x %d; "
             "free = clearance(unknown='occupied', min_voxels=50).dist >= %g; weights %s" % (args.runs, V, H, W, RADIUS, WEIGHTS), ""]

    def flush():
        text = "\n".join(lines[:1] + [clock_line()] + lines[1:]) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
        return text

    for step in [float(s) for s in args.steps.split(",")]:
        field = f.bake(synth.WORK_BOX, step, return_names=[])
        c = field.clearance(unknown="occupied", min_voxels=50)
        del field
        nx, ny, nz = c.grid_shape
        n = nx * ny * nz
        free = (c.valid & (c.dist >= RADIUS)).contiguous()
        idx = torch.nonzero(free)
        centre = torch.tensor([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2], device=dev)
        g = idx[torch.argmin(((idx.float() - centre) ** 2).sum(dim=1))]
        goal = ((g[0] * ny + g[1]) * nz + g[2]).to(torch.int32).reshape(1)
        runs = args.runs if n < (1 << 24) else max(3, args.runs // 4)
        lines.append("%d x %d x %d = %.2f M voxels (step %g m), %d free (%.2f %%), goal voxel %s; device times here: median of %d runs"
                     % (nx, ny, nz, n / 1e6, step, int(free.sum()), 100.0 * float(free.float().mean()), tuple(g.tolist()), runs))
        free_u8 = free.view(torch.uint8)
        scratch = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        cmed, clo, chi = median_ms(lambda: scratch.copy_(free_u8), runs, 1)
        for conn in (26, 6):
            t = c.travel(goal, free=free, connectivity=conn, weights=WEIGHTS)
            reached, far = int(t.valid.sum()), int(t.cost[t.valid].max()) if bool(t.valid.any()) else 0
            med, lo, hi = median_ms(lambda: c.travel(goal, free=free, connectivity=conn, weights=WEIGHTS), runs, 1)
            rounds, tile_runs, tiles = count_rounds(lib, free_u8, goal, conn, dev)
            text = ("    connectivity %2d: %d voxels reached, farthest cost %d (%.3f m); median %9.4f ms (min %.4f, max %.4f); %d rounds (2 launches each, +1 per "
                    "call), %d tile runs over %d tiles of 512 voxels = %.3f tile runs per tile, %.3f voxel relaxation slots per voxel; copy of %.1f MB: "
                    "%.4f ms (min %.4f, max %.4f)" % (conn, reached, far, far * step / WEIGHTS[0], med, lo, hi, rounds, tile_runs, tiles, tile_runs / tiles,
                                                       512.0 * tile_runs / n, 5 * n / 1e6, cmed, clo, chi))
            if not have_scipy:
                text += "; scipy: not installed"
            elif n >= (1 << 24):
                text += "; scipy: not run at this size"
            else:
                ms, want = host_dijkstra_ms(free.cpu().numpy(), int(goal.item()), conn)
                same = bool((want == t.cost.cpu().numpy().reshape(-1).astype(np.int64)).all())
                text += "; scipy.sparse.csgraph.dijkstra on the host (graph built beforehand): %.1f ms, costs %s" % (ms, "equal" if same else "DIFFER")
            lines.append(text)
            del t
            flush()
        starts = idx[torch.randperm(idx.shape[0], device=dev)[:4096]]
        starts = ((starts[:, 0] * ny + starts[:, 1]) * nz + starts[:, 2]).to(torch.int32)
        t = c.travel(goal, free=free)
        med, lo, hi = median_ms(lambda: t.path(starts), runs, 1)
        out = t.path(starts)
        lines.append("    BakedField.path of 4096 random free starts, max_steps %d: median %.4f ms (min %.4f, max %.4f); %d reached, longest %d voxels"
                     % (nx + ny + nz, med, lo, hi, int(out["reached"].sum()), int(out["length"].max())))
        lines.append("")
        flush()
        del c, t, free, free_u8, scratch, idx, out
        torch.cuda.empty_cache()
    print(flush())


if __name__ == "__main__":
    main()
