"""The argument table of tests/test_workspace_bytes_host.py: for every d3f_*_workspace_bytes function and d3f_eval_gate_offset the arguments
that return 0 (zero, negative, over the limit, NULL views), the smallest valid shape, both sides of every rounding boundary of the layout
behind it, and one workload-sized shape.  A row is the tuple of the function's arguments; views and grids are tuples of their integers (None: NULL).

    python tests/workspace_args.py LIBRARY     prints the record of that library as JSON (how tests/workspace_bytes.json was made, once,
                                               from the library of the commit before the layouts; see the test's docstring.  Rows added
                                               later go to the END of a function's list and of its record: the older values stay as they are)
    python tests/workspace_args.py --rows      prints "function arg arg ..." lines: the table for a program that is not Python
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from d3fields_amd import _lib  # noqa: E402

RECORD = os.path.join(HERE, "workspace_bytes.json")

S = 2048                    # items per workgroup of the scan (scan_kernels.hip: kScanPerBlock): one more level of scratch above S, above S * S
B = 256                     # kBlock: per-workgroup counts come one per 256 items
I31 = 0x7fffffff


def around(*edges):
    """both sides of every edge: the last value of one rounding step and the first of the next"""
    return [v for e in edges for v in (e, e + 1)]


def box(n, least=1):
    """(nx, ny, nz), every extent in [least, 16384], of n points -- or of the next count above n that has such factors (a handful more at most:
    the boundaries below are in units of 256 points and more, or the row before already sits on the last value of the step)"""
    while True:
        for nz in range(min(n, 16384), least - 1, -1):
            for ny in range(min(n // nz, 16384), least - 1, -1) if n % nz == 0 else ():
                if (n // nz) % ny == 0 and least <= n // nz // ny <= 16384:
                    return (n // nz // ny, ny, nz)
        n += 1


def boxes(counts, least=1):
    return [box(n, least) for n in counts]


BAD_BOXES = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, 4, -1)]
EDT_OVER = [(_lib.EDT_MAX_EXTENT + 1, 1, 1), (1, 1, _lib.EDT_MAX_EXTENT + 1), (2048, 2048, 512)]        # an extent, 2^31 voxels
SCAN_BOXES = boxes(around(S, S * S), 2) + [(2048, 2049, 2)]                                                # n = S, S + 1, S^2, > S^2 twice (extents >= 2: the band's and the mesh's rule)
VOLUME = (128, 128, 64)                                                                                 # the baked volume of the examples

ORDER_N = [0, -1, 1] + around(64, 1 << 14, 1 << 19) + [1000000, I31, I31 + 1]       # 256-byte pad of 4 n; 2 n = 2^15 and 2^20 counters
POOL_K = [0, 1] + around(63, S - 1) + [65535]                                      # K + 1 words: the 256-byte pad, the scan's second level
FPS_EDGES = [262144, 262145, 262399, 262400]                                       # 256 * 1024 and 256 * 1025 - 1: the window in which 1024 points per workgroup would need 257 of them
POOL_CAP = [0, 1] + around(256, 65536) + [1 << 21, 1 << 30]                        # fold levels; above n: clamped to n

TABLE = {
    "d3f_eval_workspace_bytes": [(n,) for n in ORDER_N],
    "d3f_eval_gate_offset": [(n,) for n in ORDER_N],
    # (V, H, W) or None, n: the 2^22-point threshold, the view limits, tiles of 8 x 4 pixels, 2^32 bytes of tiles and more
    "d3f_eval_dist_workspace_bytes": [(None, 1 << 22), ((4, 480, 640), 0), ((4, 480, 640), (1 << 22) - 1), ((4, 480, 640), 1 << 22), ((4, 480, 640), 1 << 24),
                                      ((0, 8, 4), 1 << 22), ((9, 8, 4), 1 << 22), ((1, 0, 4), 1 << 22), ((1, 8, 0), 1 << 22), ((1, 1, 1), 1 << 22),
                                      ((1, 8, 4), 1 << 22), ((1, 9, 4), 1 << 22), ((1, 8, 5), 1 << 22), ((8, 9, 5), 1 << 22), ((8, 2048, 2048), 1 << 22),
                                      ((8, 2048, 2049), 1 << 22), ((8, 32768, 32768), 1 << 22)],
    # (nx, ny, nz) or None: 256 points per count, 64 counts per 256 bytes, the scan's levels over the counts (S^2 counts: 2^30 points)
    "d3f_grid_shell_workspace_bytes": [(None,)] + [(g,) for g in BAD_BOXES + [(1, 1, 1)] + boxes(around(B, 64 * B, S * B)) + [(1024, 1024, 1024), (1025, 1024, 1024), VOLUME]],
    # 1024 points per workgroup, workgroups + 1 words: one word, 64 | 65 words, S | S + 1 words
    "d3f_mesh_workspace_bytes": BAD_BOXES + [(1, 2, 2), (2, 2, 2), (2, 2, 256), (2, 2, 257)] + boxes(around(63 * 1024, (S - 1) * 1024), 2) + [VOLUME, (1024, 1024, 682)],
    "d3f_volume_gaussian_workspace_bytes": BAD_BOXES + [(1, 1, 1), (3, 5, 7), VOLUME, (2048, 2048, 511)],
    "d3f_band_workspace_bytes": BAD_BOXES + [(1, 2, 2), (2, 2, 2)] + SCAN_BOXES + [VOLUME, (2048, 2048, 511), (2048, 2048, 512)],
    "d3f_volume_edt_workspace_bytes": BAD_BOXES + EDT_OVER + [(1, 1, 1), (1, 1, 2), (3, 3, 3), (1, 1, _lib.EDT_MAX_EXTENT), VOLUME, (2048, 2048, 511)],
    "d3f_volume_components_workspace_bytes": BAD_BOXES + EDT_OVER + [(1, 1, 1)] + SCAN_BOXES + [VOLUME, (2048, 2048, 511)],
    # tiles of 8 x 8 x 8 voxels
    "d3f_volume_geodesic_workspace_bytes": BAD_BOXES + EDT_OVER + [(1, 1, 1), (8, 8, 8), (9, 8, 8), (8, 9, 8), (8, 8, 9), (17, 9, 25), VOLUME, (2048, 2048, 511)],
    "d3f_volume_pool_workspace_bytes": ([b + (4, 100, 8) for b in BAD_BOXES] + [(4, 4, 4, -1, 10, 8), (4, 4, 4, 4, -1, 8), (4, 4, 4, 4, 10, -1), (1, 1, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1)]
                                        + [b + (4, 1 << 30, 8) for b in SCAN_BOXES]
                                        + [VOLUME + (K, 1 << 30, 8) for K in POOL_K]
                                        + [VOLUME + (64, cap, m) for cap in POOL_CAP for m in (0, 48)]
                                        + [VOLUME + (64, 1 << 20, m) for m in (1, 3, 4, 384, 2048)]),
    "d3f_part_motion_workspace_bytes": ([b + (4, 100) for b in BAD_BOXES] + [(4, 4, 4, -1, 10), (4, 4, 4, 4, -1), (1, 1, 1, 0, 0), (1, 1, 1, 1, 1)]
                                        + [b + (4, 1 << 30) for b in SCAN_BOXES]
                                        + [VOLUME + (K, 1 << 30) for K in POOL_K]
                                        + [VOLUME + (32, cap) for cap in POOL_CAP]),
    # 256 points per workgroup; I times the workgroups above 2^31 - 1
    "d3f_volume_align_workspace_bytes": [(0, 10), (10, 0), (-1, 10), (10, -1), (1, 1), (1, 256), (1, 257), (3, 512), (3, 513), (4, 4096), (I31, 256), (I31, 257), (1 << 23, 65537)],
    # (M, k, n_trip, max_survivors): T = n_trip k^3 hypotheses, 256 per count; survivors of 4, 1 and 64 bytes
    "d3f_pose_consensus_workspace_bytes": ([(2, 1, 1, 1), (65, 1, 1, 1), (3, 0, 1, 1), (3, 9, 1, 1), (3, 1, -1, 1), (3, 8, (I31 // 512) + 1, 1), (3, 1, 1, 0),
                                            (3, 1, 1, _lib.CONSENSUS_MAX_SURVIVORS + 1), (3, 1, 0, 1), (3, 1, 1, 1)]
                                           + [(8, 1, t, 64) for t in around(B, 64 * B, S * B)] + [(8, 8, 1 << 21, 64), (8, 8, (1 << 21) + 1, 64), (8, 8, I31 // 512, 64)]
                                           + [(8, 4, 1000, s) for s in around(4, 64, 256) + [4096, _lib.CONSENSUS_MAX_SURVIVORS]]),
    # distances of 4 and of 8 bytes, rounded up to 16; 256 workgroups of 1024 points, the last n they hold, and the first of 1025 and more each (FPS_EDGES)
    "d3f_fps_workspace_bytes": [(n,) for n in [0, -1, 1] + around(4, 8, 1024) + [200000, I31] + FPS_EDGES],
    "d3f_fps_pixels_workspace_bytes": [(n,) for n in [0, -1, 1] + around(2, 4, 1024) + [307200, I31] + FPS_EDGES],
    "d3f_backproject_workspace_bytes": [(0, 4), (4, 0), (-1, 4), (4, -1), (1, 1), (1, 256), (1, 257), (16, 16), (480, 640), (32768, 65535)],
    # the table doubles where 2 (n1 + n2) passes it
    "d3f_vox_iou_workspace_bytes": [(-1, 4), (4, -1), (0, 0), (1, 0), (512, 0), (512, 1), (0, 1024), (1, 1024), (100000, 90000), (1 << 29, 1 << 29)],
    "d3f_voxel_downsample_workspace_bytes": [(n,) for n in [0, -1, 1] + around(512, 1024, 1 << 17) + [200000, 0x3fffffff]],
    # 64 rows per block of column statistics
    "d3f_softmax_workspace_bytes": [(0, 4), (4, 0), (-1, 4), (4, -1), (1, 1), (64, 1), (65, 1), (64, 16), (65, 16), (128, 3), (129, 3), (4096, 1000), (64 * 65535, 4096)],
    # + the top-k levels: 256 rows per chunk, 8 candidates out of each -- one level more above 256, 8192, 262144 rows
    "d3f_pairwise_topk_workspace_bytes": ([(0, 4), (4, 0), (-1, 4), (4, -1), (1, 1)] + [(r, c) for r in around(64, 256, 8192, 262144) for c in (1, 16)]
                                          + [(4096, 1000), (64 * 65535, 4096)]),
    # (M, C): panels of 64 channels, sum chunks of 256, chains of 32 and stages of 64 rows, up to 2048 and 256 slabs
    "d3f_row_moments_workspace_bytes": ([(0, 8), (-1, 8), (8, 0), (8, -1), (8, _lib.MAX_MOMENT_CHANNELS + 1), (1, 1)]
                                        + [(1000, c) for c in around(64, 256, 2047)] + [(m, 384) for m in around(32, 64, 16384, 65536)] + [(m, 3) for m in around(32, 65536)]
                                        + [(200000, 384), (1 << 24, 1024), (I31, 2048)]),
}


def call(lib, fn, row):
    keep = []
    args = []
    for a, t in zip(row, _lib.SIGNATURES[fn][1]):
        if t is ctypes.POINTER(_lib.Views) or t is ctypes.POINTER(_lib.Grid):
            if a is not None:
                s = t._type_()
                for name, v in zip(("V", "H", "W") if t._type_ is _lib.Views else ("nx", "ny", "nz"), a):
                    setattr(s, name, v)
                keep.append(s)
                a = ctypes.byref(s)
        args.append(a)
    return int(getattr(lib, fn)(*args))


def load(path=None):
    """the library of the tree, or the one at path with the same signatures"""
    if path is None:
        return _lib.load()
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def flat(row):
    """a row as integers alone: a NULL view or grid as three -1"""
    out = []
    for a in row:
        out += [-1, -1, -1] if a is None else list(a) if isinstance(a, tuple) else [a]
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--rows":
        for fn in sorted(TABLE):
            for row in TABLE[fn]:
                print(fn, *flat(row))
    else:
        lib = load(sys.argv[1])
        rec = {fn: [call(lib, fn, row) for row in TABLE[fn]] for fn in sorted(TABLE)}
        print("{\n" + ",\n".join('  "%s": %s' % (fn, json.dumps(v)) for fn, v in rec.items()) + "\n}")
