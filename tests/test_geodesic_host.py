"""CPU: the cost-to-go entry points (d3f_volume_geodesic_workspace_bytes / _init / _relax / _finish, d3f_volume_follow) are declared by the
header, bound and exported with D3F_ABI_VERSION still 16; they validate their arguments on the host with the documented status codes and
launch nothing; the workspace size is 0 exactly for rejected shapes; the NumPy restatement (tests/geodesic_cases.py) equals
scipy.sparse.csgraph.dijkstra on a graph built from the definition; next_ref lowers the cost at every step and ends at a seed; the chamfer
ratio range of (3, 4, 5) is recomputed and compared with the closed form and the documents; no kernel of geodesic_kernels.hip uses scratch."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geodesic_cases as GC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_volume_geodesic_workspace_bytes", "d3f_volume_geodesic_init", "d3f_volume_geodesic_relax", "d3f_volume_geodesic_finish", "d3f_volume_follow")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_geodesic_symbols_and_unchanged_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name


REJECTED = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2048, 1024, 1024)]
ACCEPTED = [(1, 1, 1), (7, 9, 1), (1, 1, 130), (16384, 1, 2), (1, 16384, 1), (50, 50, 53), (256, 256, 256), (2047, 1024, 1024)]


def test_workspace_bytes_is_zero_exactly_for_rejected_shapes():
    lib = _lib.load()
    for shape in REJECTED:
        assert lib.d3f_volume_geodesic_workspace_bytes(*shape) == 0, shape
    for shape in ACCEPTED:
        got = lib.d3f_volume_geodesic_workspace_bytes(*shape)
        assert got > 0 and got % 4 == 0, (shape, got)
    assert lib.d3f_volume_geodesic_workspace_bytes(64, 64, 64) < lib.d3f_volume_geodesic_workspace_bytes(128, 64, 64)


def test_geodesic_validation_status_codes():
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)
    big = 1 << 62
    err = lib.d3f_last_error

    def weights(*w):
        return (ctypes.c_int32 * 3)(*w)

    def init(free=p, shape=(4, 5, 6), seeds=p, n_seeds=3, cost=p, ws=p, wsb=big):
        return lib.d3f_volume_geodesic_init(free, shape[0], shape[1], shape[2], seeds, n_seeds, cost, ws, wsb, None)

    def relax(free=p, penalty=None, shape=(4, 5, 6), conn=26, w=(3, 4, 5), max_cost=GC.NO_CAP, rounds=1, cost=p, pending=p, ws=p, wsb=big):
        return lib.d3f_volume_geodesic_relax(free, penalty, shape[0], shape[1], shape[2], conn, None if w is None else weights(*w), max_cost, rounds, cost,
                                             pending, ws, wsb, None)

    def finish(free=p, penalty=None, shape=(4, 5, 6), conn=26, w=(3, 4, 5), step=0.01, cost=p, nxt=p, dist=p):
        return lib.d3f_volume_geodesic_finish(free, penalty, shape[0], shape[1], shape[2], conn, None if w is None else weights(*w), step, cost, nxt, dist,
                                              None)

    def follow(nxt=p, n_voxels=120, starts=p, n=5, max_steps=8, voxels=p, length=p, reached=p):
        return lib.d3f_volume_follow(nxt, n_voxels, starts, n, max_steps, voxels, length, reached, None)

    # D3F_ERR_INVALID_ARG
    assert init(free=None) == _lib.ERR_INVALID_ARG and init(cost=None) == _lib.ERR_INVALID_ARG and b"NULL" in err()
    assert init(n_seeds=-1) == _lib.ERR_INVALID_ARG and b"n_seeds" in err()
    assert init(seeds=None) == _lib.ERR_INVALID_ARG and b"seeds" in err()
    assert relax(free=None) == _lib.ERR_INVALID_ARG and relax(cost=None) == _lib.ERR_INVALID_ARG and relax(pending=None) == _lib.ERR_INVALID_ARG
    for conn in (0, 4, 8, 27, -6):
        assert relax(conn=conn) == _lib.ERR_INVALID_ARG and finish(conn=conn) == _lib.ERR_INVALID_ARG and b"connectivity" in err(), conn
    for w in ((0, 1, 1), (-3, 4, 5), (2, 1, 3), (1, 3, 2), (3, 4, 256), (256, 256, 256), None):
        assert relax(w=w) == _lib.ERR_INVALID_ARG and finish(w=w) == _lib.ERR_INVALID_ARG, w
    for conn in (6, 18):                                 # all three weights are validated, whatever the connectivity uses
        assert relax(conn=conn, w=(1, 2, 1)) == _lib.ERR_INVALID_ARG and b"w1 <= w2 <= w3" in err()
    for bad in (0, -1, GC.INT32_MAX, -GC.INT32_MAX - 1):
        assert relax(max_cost=bad) == _lib.ERR_INVALID_ARG and b"max_cost" in err(), bad
    assert relax(rounds=0) == _lib.ERR_INVALID_ARG and relax(rounds=-5) == _lib.ERR_INVALID_ARG and b"rounds" in err()
    assert finish(free=None) == _lib.ERR_INVALID_ARG and finish(cost=None) == _lib.ERR_INVALID_ARG
    assert finish(nxt=None, dist=None) == _lib.ERR_INVALID_ARG and b"both NULL" in err()
    for step in (0.0, -1.0, math.inf, math.nan):
        assert finish(step=step) == _lib.ERR_INVALID_ARG and b"step" in err(), step
    for kw in ("nxt", "starts", "voxels", "length", "reached"):
        assert follow(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    assert follow(n=-1) == _lib.ERR_INVALID_ARG and b"n=" in err()
    assert follow(max_steps=0) == _lib.ERR_INVALID_ARG and follow(max_steps=-2) == _lib.ERR_INVALID_ARG and b"max_steps" in err()
    # D3F_ERR_BAD_SHAPE
    for bad in ((0, 5, 6), (4, 16385, 6), (4, 5, -2), (2048, 1024, 1024)):
        assert init(shape=bad) == _lib.ERR_BAD_SHAPE and relax(shape=bad) == _lib.ERR_BAD_SHAPE and finish(shape=bad) == _lib.ERR_BAD_SHAPE, bad
        assert b"extent" in err()
    assert follow(n_voxels=0) == _lib.ERR_BAD_SHAPE and follow(n_voxels=2 ** 31) == _lib.ERR_BAD_SHAPE and b"n_voxels" in err()
    # D3F_ERR_BAD_LAYOUT
    assert init(seeds=odd) == _lib.ERR_BAD_LAYOUT and init(cost=odd) == _lib.ERR_BAD_LAYOUT and init(ws=odd) == _lib.ERR_BAD_LAYOUT
    assert relax(penalty=odd) == _lib.ERR_BAD_LAYOUT and relax(cost=odd) == _lib.ERR_BAD_LAYOUT and relax(pending=odd) == _lib.ERR_BAD_LAYOUT
    assert relax(ws=odd) == _lib.ERR_BAD_LAYOUT and b"workspace" in err()
    assert finish(penalty=odd) == _lib.ERR_BAD_LAYOUT and finish(cost=odd) == _lib.ERR_BAD_LAYOUT and finish(nxt=odd) == _lib.ERR_BAD_LAYOUT
    assert finish(dist=odd) == _lib.ERR_BAD_LAYOUT and b"aligned" in err()
    for kw in ("nxt", "starts", "voxels", "length"):
        assert follow(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    # D3F_ERR_WORKSPACE: NULL, or one byte short of what the size function says
    need = lib.d3f_volume_geodesic_workspace_bytes(4, 5, 6)
    assert init(ws=None) == _lib.ERR_WORKSPACE and init(wsb=need - 1) == _lib.ERR_WORKSPACE and init(wsb=0) == _lib.ERR_WORKSPACE
    assert relax(ws=None) == _lib.ERR_WORKSPACE and relax(wsb=need - 1) == _lib.ERR_WORKSPACE and b"workspace" in err()
    # the legal forms pass every check before the workspace (and stop there: nothing is launched without a GPU)
    assert init(ws=None, free=odd) == _lib.ERR_WORKSPACE                      # free is bytes
    assert init(ws=None, seeds=None, n_seeds=0) == _lib.ERR_WORKSPACE
    assert init(ws=None, shape=(1, 1, 1)) == _lib.ERR_WORKSPACE and init(ws=None, shape=(7, 9, 1)) == _lib.ERR_WORKSPACE
    for conn, w in GC.CONFIGS + [(26, (255, 255, 255)), (6, (1, 1, 1)), (26, (1, 255, 255))]:
        assert relax(ws=None, conn=conn, w=w) == _lib.ERR_WORKSPACE, (conn, w)
    assert relax(ws=None, max_cost=1) == _lib.ERR_WORKSPACE and relax(ws=None, penalty=p, rounds=256) == _lib.ERR_WORKSPACE
    assert follow(n=0, nxt=None, starts=None, voxels=None, length=None, reached=None) == _lib.OK      # nothing to do, nothing launched
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(relax(rounds=0))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the restatement against Dijkstra -------------------------------------------------------------------------------------------------
def definition_graph(free, connectivity, w, penalty):
    """the moves of the definition, voxel by voxel from integer coordinates (no shifted copies): csr_matrix [n, n], entry [u, v] = the cost of
    the move u -> v.  Every cost is >= 1, so no explicit zero is stored."""
    from scipy.sparse import csr_matrix
    free = np.asarray(free) != 0
    shape = np.array(free.shape)
    at = np.argwhere(free)
    rows, cols, vals = [], [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                l1 = abs(dx) + abs(dy) + abs(dz)
                if l1 == 0 or l1 > {6: 1, 18: 2, 26: 3}[connectivity]:
                    continue
                to = at + np.array([dx, dy, dz])
                ok = ((to >= 0) & (to < shape)).all(axis=1)
                u, v = at[ok], to[ok]
                ok = free[v[:, 0], v[:, 1], v[:, 2]]
                u, v = u[ok], v[ok]
                charge = 0 if penalty is None else np.maximum(penalty[v[:, 0], v[:, 1], v[:, 2]].astype(np.int64), 0)
                rows.append(np.ravel_multi_index(u.T, free.shape))
                cols.append(np.ravel_multi_index(v.T, free.shape))
                vals.append(np.full(len(u), w[l1 - 1], np.int64) + charge)
    rows, cols, vals = (np.concatenate(a) for a in (rows, cols, vals))
    assert (vals >= 1).all()
    return csr_matrix((vals.astype(np.float64), (rows, cols)), shape=(free.size, free.size))


def dijkstra_cost(free, seeds, connectivity, w, penalty):
    from scipy.sparse.csgraph import dijkstra
    seeds = GC.accepted_seeds(free, seeds)
    if not seeds:
        return np.full(free.shape, GC.INT32_MAX, np.int32)
    d = dijkstra(definition_graph(free, connectivity, w, penalty), directed=True, indices=seeds, min_only=True)
    return np.where(np.isinf(d), GC.INT32_MAX, d).astype(np.int64).astype(np.int32).reshape(free.shape)


@pytest.mark.parametrize("name", GC.UNCAPPED)
def test_travel_ref_equals_dijkstra(name):
    free, seeds, penalty = GC.case(name)
    configs = GC.CONFIGS + ([(26, (255, 255, 255))] if name == "17x17x17 45%" else []) + ([(26, (1, 1, 1))] if name == "open 5x5x5" else [])
    for conn, w in configs:
        cost, nxt, _ = GC.reference(name, conn, w)
        want = dijkstra_cost(free, seeds, conn, w, penalty)
        assert cost.dtype == np.int32 and np.array_equal(cost, want), (name, conn, w, int((cost != want).sum()))
        assert (cost[np.asarray(free) == 0] == GC.INT32_MAX).all() and ((cost == 0).reshape(-1).nonzero()[0].tolist() == GC.accepted_seeds(free, seeds))


def test_pairs_are_reached_as_the_connectivity_says():
    for name, reached in GC.PAIRS.items():
        free, seeds, _ = GC.case(name)
        second = int(np.flatnonzero(free.reshape(-1))[1])
        for rank, (conn, w) in enumerate(GC.CONFIGS):
            cost = GC.reference(name, conn, w)[0].reshape(-1)
            assert (cost[second] != GC.INT32_MAX) == reached[rank], (name, conn)
            if reached[rank]:
                assert cost[second] == w[("face pair", "edge pair", "corner pair").index(name)]


def test_boundary_pairs_are_reached_as_the_connectivity_says():
    """the restatement on the seed-on-a-tile-boundary cases: the second voxel costs the move's weight where the connectivity has that move"""
    for name in list(GC.BOUNDARY) + list(GC.SMALL_BOUNDARY):
        shape, a, b = GC.boundary_pair(name)
        free, seeds, _ = GC.case(name)
        assert free.shape == shape and int((free != 0).sum()) == 2 and seeds.tolist() == [int(np.ravel_multi_index(a, shape))]
        if name in GC.BOUNDARY:
            assert all(min(p, q) == 31 and max(p, q) in (31, 32) for p, q in zip(a, b))      # astride 32 wherever they differ
        for rank, (conn, w) in enumerate(GC.CONFIGS):
            cost = GC.reference(name, conn, w)[0]
            moves = GC.l1(a, b)
            assert cost[a] == 0 and cost[b] == (w[moves - 1] if moves <= rank + 1 else GC.INT32_MAX), (name, conn)
    assert {GC.l1(*GC.BOUNDARY[k]) for k in GC.BOUNDARY} == {1, 2, 3}
    for conn, w in GC.CONFIGS:
        cost = GC.reference("corridor seed at 31", conn, w)[0].reshape(-1)
        assert cost.tolist() == [w[0] * abs(z - 31) for z in range(40)]
        cost = GC.reference("slab seed at 31", conn, w)[0]
        assert (cost[:32, :32, :32] != GC.INT32_MAX).all() and ((cost[32:, 32:, 32:] != GC.INT32_MAX).all() if conn == 26 else (cost[32:, 32:, 32:] == GC.INT32_MAX).all())


def test_serpentine_figures():
    free, chain = GC.serpentine()
    assert free.shape == (12, 12, 12) and int(free.sum()) == len(chain) == len(set(chain)) == 467
    cost, nxt, sweeps = GC.reference("serpentine", 6, (1, 1, 1))
    assert [int(cost[p]) for p in chain] == list(range(467)) and int(cost[cost != GC.INT32_MAX].max()) == 466 and sweeps >= 466


@pytest.mark.parametrize("name", ["13x11x19 70%", "17x17x17 45%", "serpentine", "open 5x5x5", "bad seeds", "2x3x130 60%"])
def test_next_ref_lowers_the_cost_and_ends_at_a_seed(name):
    free, seeds, penalty = GC.case(name)
    for conn, w in GC.CONFIGS + [(26, (1, 1, 1))]:
        cost, nxt, _ = GC.reference(name, conn, w)
        c, to = cost.reshape(-1).astype(np.int64), nxt.reshape(-1).astype(np.int64)
        reached = c != GC.INT32_MAX
        assert ((to == -1) == ~reached).all()
        seeds_at = np.flatnonzero(c == 0)
        assert (to[seeds_at] == seeds_at).all()
        moving = reached & (c > 0)
        assert (c[to[moving]] < c[moving]).all()                               # strictly: no cycle
        # every next is a neighbour under the connectivity, and the smallest index among the equal predecessors
        a, b = np.array(np.unravel_index(np.flatnonzero(moving), cost.shape)), np.array(np.unravel_index(to[moving], cost.shape))
        delta = np.abs(a - b)
        assert (delta.max(axis=0) <= 1).all() and (delta.sum(axis=0) <= {6: 1, 18: 2, 26: 3}[conn]).all() and (delta.sum(axis=0) >= 1).all()
        starts = np.flatnonzero(reached)[::7]
        voxels, length, ok = GC.follow_ref(nxt, starts, cost.size)
        assert ok.all() and (length >= 1).all() and all(c[voxels[i, length[i] - 1]] == 0 for i in range(len(starts)))
    if name == "open 5x5x5":                                                   # the tie rule, voxel by voxel in plain Python
        cost, nxt, _ = GC.reference(name, 26, (1, 1, 1))
        for v in range(125):
            x, y, z = np.unravel_index(v, (5, 5, 5))
            if cost[x, y, z] == 0:
                continue
            equal = [np.ravel_multi_index((x + o[0], y + o[1], z + o[2]), (5, 5, 5)) for o in GC.offsets(26)
                     if all(0 <= q < 5 for q in (x + o[0], y + o[1], z + o[2])) and cost[x + o[0], y + o[1], z + o[2]] + 1 == cost[x, y, z]]
            assert nxt[x, y, z] == min(equal)
    assert [len(GC.offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]


def test_follow_ref_padding_cut_and_bad_starts():
    cost, nxt, _ = GC.reference("serpentine", 6, (1, 1, 1))
    free, chain = GC.serpentine()
    far = int(np.ravel_multi_index(chain[40], cost.shape))
    wall = int(np.flatnonzero(np.asarray(free).reshape(-1) == 0)[0])
    voxels, length, reached = GC.follow_ref(nxt, [far, far, -1, wall, cost.size, int(np.ravel_multi_index(chain[0], cost.shape))], 41)
    assert length.tolist() == [41, 41, 0, 0, 0, 1] and reached.tolist() == [1, 1, 0, 0, 0, 1]
    assert voxels[0].tolist() == [int(np.ravel_multi_index(p, cost.shape)) for p in chain[40::-1]] and (voxels[2:5] == -1).all() and (voxels[5, 1:] == -1).all()
    voxels, length, reached = GC.follow_ref(nxt, [far], 40)                    # one step short: a full row, not reached
    assert length.tolist() == [40] and reached.tolist() == [0] and (voxels >= 0).all()


# ---- accuracy of the default weights ----------------------------------------------------------------------------------------------------
def test_chamfer_ratio_of_345_in_open_space():
    """cost / (3 * Euclidean voxel distance) over an empty 41^3 octant from the corner seed: the chamfer distance of an offset a >= b >= c >= 0 is
    3a + b + c (c corner moves, b - c edge moves, a - b face moves), so the ratio is lowest along (1, 1, 0) and highest along (3, 1, 1)."""
    free = np.ones((41, 41, 41), np.uint8)
    cost, _ = GC.travel_ref(free, [0], 26, (3, 4, 5))
    g = np.indices(free.shape).astype(np.int64)
    s = np.sort(g, axis=0)
    assert np.array_equal(cost, 3 * s[2] + s[1] + s[0])                        # the closed form, voxel by voxel
    d = np.sqrt((g ** 2).sum(axis=0).astype(np.float64))
    ratio = cost.reshape(-1)[1:] / (3.0 * d.reshape(-1)[1:])
    lo, hi = ratio.min(), ratio.max()
    assert abs(lo - 2 * math.sqrt(2) / 3) < 1e-12 and abs(hi - math.sqrt(11) / 3) < 1e-12
    at = [ratio[np.ravel_multi_index(o, free.shape) - 1] for o in ((1, 1, 0), (3, 1, 1))]      # (multiples such as (6, 2, 2) differ by an ulp of the division)
    assert abs(at[0] - lo) < 1e-12 and abs(at[1] - hi) < 1e-12
    for doc in ("include/d3fields_hip.h", "DESIGN.md", "INTEGRATION.md", "d3fields_amd/baked.py"):
        m = re.search(r"\[(0\.9\d+), (1\.1\d+)\]", open(os.path.join(ROOT, doc)).read())
        assert m, doc
        for stated, got in ((m.group(1), lo), (m.group(2), hi)):
            assert abs(float(stated) - got) <= 0.5 * 10 ** -len(stated.split(".")[1]) + 1e-12, (doc, stated, got)      # the figure, rounded to its digits


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "geodesic_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("geo_init_kernel", "geo_seed_kernel", "geo_compact_kernel", "geo_pending_kernel", "geo_follow_kernel", "geo_tile_kernelILi6E",
                   "geo_tile_kernelILi18E", "geo_tile_kernelILi26E", "geo_finish_kernelILi6E", "geo_finish_kernelILi18E", "geo_finish_kernelILi26E"):
        assert kernel in names, (kernel, out[-800:])
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0 and vgpr <= 128 and occ >= 4, (name, vgpr, scratch, occ)
