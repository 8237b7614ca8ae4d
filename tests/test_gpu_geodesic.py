"""The cost-to-go field on the device (d3f_volume_geodesic_init / _relax / _finish, d3f_volume_follow, csrc/geodesic_kernels.hip;
BakedField.travel / path) against the NumPy restatement of tests/geodesic_cases.py: integer data, equality of the cost, next and dist bytes
everywhere, no tolerance, and identical bytes from a second run.

What each assert is there to catch:
  a move made across a wrap or missed across a tile face, edge or corner, a halo word outside the volume     the pairs, the random volumes
  a tile that is not flagged when its neighbour changed, a list count that does not carry across calls       the serpentine, rounds = 1 per call
  a seed on a tile face, edge or corner whose neighbour tile is never run                                    the pairs astride 32, seed at 31
  a workspace word or an output the kernels do not write before reading                                      everything is poisoned with 0xA5
  a candidate that wraps int32, a cap that is off by one, a negative penalty that pays                       max_cost, saturation
  a next that follows the order in which something landed instead of the smallest index                      open 5x5x5 under (26, (1, 1, 1))
"""
import ctypes

import numpy as np
import pytest
import torch

import geodesic_cases as GC
from d3fields_amd import _lib
from d3fields_amd.baked import BakedField

pytestmark = pytest.mark.gpu

STEP = 0.0125      # dist = float32(cost) * (float32(step) / float32(w1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def poisoned(shape, dtype, dev):
    return torch.full(shape, 0xA5, dtype=torch.uint8, device=dev).view(dtype) if dtype != torch.uint8 else torch.full(shape, 0xA5, dtype=dtype, device=dev)


def run_geo(free, seeds, penalty, conn, w, dev, max_cost=GC.NO_CAP, rounds=None):
    """init, relax until nothing is pending (batches of 16 rounds doubling up to 256, or `rounds` per call) and finish, on freshly poisoned
    outputs and workspace -> (cost, next, dist, calls of relax)"""
    lib = _lib.load()
    nx, ny, nz = free.shape
    n = free.size
    f = torch.from_numpy(np.array(free)).to(dev)
    s = torch.from_numpy(np.array(seeds, dtype=np.int32)).to(dev)
    p = None if penalty is None else torch.from_numpy(np.array(penalty)).to(dev)
    cost = poisoned((nx, ny, nz * 4), torch.int32, dev)
    nxt = poisoned((nx, ny, nz * 4), torch.int32, dev)
    dist = poisoned((nx, ny, nz * 4), torch.float32, dev)
    pending = poisoned((4,), torch.int32, dev)
    ws_bytes = lib.d3f_volume_geodesic_workspace_bytes(nx, ny, nz)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    warr = (ctypes.c_int32 * 3)(*w)
    stream = _lib.current_stream_handle(dev)
    _lib.check(lib.d3f_volume_geodesic_init(_lib.ptr(f), nx, ny, nz, _lib.ptr(s) if len(seeds) else None, len(seeds), _lib.ptr(cost), _lib.ptr(ws), ws_bytes,
                                            stream))
    batch, total, calls = (16 if rounds is None else rounds), 0, 0
    while True:
        _lib.check(lib.d3f_volume_geodesic_relax(_lib.ptr(f), _lib.ptr(p), nx, ny, nz, conn, warr, max_cost, batch, _lib.ptr(cost), _lib.ptr(pending), _lib.ptr(ws),
                                                 ws_bytes, stream))
        total += batch
        calls += 1
        left = int(pending.item())
        assert 0 <= left <= ws_bytes // 8
        if left == 0:
            break
        assert total <= n, "after nx*ny*nz rounds every voxel is final"
        if rounds is None:
            batch = min(2 * batch, 256)
    _lib.check(lib.d3f_volume_geodesic_finish(_lib.ptr(f), _lib.ptr(p), nx, ny, nz, conn, warr, STEP, _lib.ptr(cost), _lib.ptr(nxt), _lib.ptr(dist), stream))
    torch.cuda.synchronize()
    return cost.cpu().numpy(), nxt.cpu().numpy(), dist.cpu().numpy(), calls


def check_case(name, conn, w, dev, max_cost=GC.NO_CAP, with_penalty=True, rounds=None):
    free, seeds, penalty = GC.case(name)
    penalty = penalty if with_penalty else None
    want_cost, want_next, _ = GC.reference(name, conn, w, max_cost, with_penalty)
    want_dist = GC.dist_ref(want_cost, STEP, w[0])
    got = run_geo(free, seeds, penalty, conn, w, dev, max_cost, rounds)
    what = (name, conn, w, max_cost, rounds)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want_cost), (what, "cost", int((got[0] != want_cost).sum()))
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want_next), (what, "next", int((got[1] != want_next).sum()))
    assert got[2].dtype == np.float32 and np.array_equal(got[2].view(np.int32), want_dist.view(np.int32)), (what, "dist")
    again = run_geo(free, seeds, penalty, conn, w, dev, max_cost, rounds)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], again[:3])), (what, "two runs differ")
    return got


@pytest.mark.parametrize("name", GC.DEGENERATE)
def test_degenerate_volumes(dev, name):
    for conn, w in GC.CONFIGS:
        cost = check_case(name, conn, w, dev)[0]
        if name in ("none free", "no seeds", "bad seeds"):
            assert (cost == GC.INT32_MAX).all()
        if name == "all free":
            assert (cost != GC.INT32_MAX).all() and int((cost == 0).sum()) == 2
        if name == "duplicate seeds":
            assert int((cost == 0).sum()) == 2


@pytest.mark.parametrize("name", list(GC.PAIRS))
def test_pairs_are_reached_as_the_connectivity_says(dev, name):
    free, _, _ = GC.case(name)
    second = int(np.flatnonzero(free.reshape(-1))[1])
    for rank, (conn, w) in enumerate(GC.CONFIGS):
        cost = check_case(name, conn, w, dev)[0]
        assert (cost.reshape(-1)[second] != GC.INT32_MAX) == GC.PAIRS[name][rank], (name, conn)


@pytest.mark.parametrize("name", GC.SEED_ON_BOUNDARY)
def test_a_seed_on_a_tile_boundary_reaches_the_neighbour_tile(dev, name):
    """only the seed is lowered on its side of the boundary: the tile across it must run because of the seed, under every connectivity that has the move"""
    for rank, (conn, w) in enumerate(GC.CONFIGS):
        cost = check_case(name, conn, w, dev)[0]
        if name in GC.BOUNDARY or name in GC.SMALL_BOUNDARY:
            _, a, b = GC.boundary_pair(name)
            moves = GC.l1(a, b)
            assert cost[a] == 0 and cost[b] == (w[moves - 1] if moves <= rank + 1 else GC.INT32_MAX), (name, conn)
        elif name == "corridor seed at 31":
            assert cost.reshape(-1).tolist() == [w[0] * abs(z - 31) for z in range(40)]
        else:
            assert (cost[32:, 32:, 32:] != GC.INT32_MAX).all() == (conn == 26) and cost[32, 32, 32] == (w[2] if conn == 26 else GC.INT32_MAX)


@pytest.mark.parametrize("name", GC.VOLUMES)
def test_random_volumes_equal_the_restatement(dev, name):
    for conn, w in GC.CONFIGS:
        cost = check_case(name, conn, w, dev)[0]
        assert 0 < int((cost != GC.INT32_MAX).sum()) < cost.size
    if name == "17x17x17 45%":
        check_case(name, 26, (255, 255, 255), dev)
        check_case(name, 26, (3, 4, 5), dev, with_penalty=False)             # penalty NULL


def test_serpentine_many_batches_and_one_round_per_call(dev):
    cost, _, _, calls = check_case("serpentine", 6, (1, 1, 1), dev)
    assert int(cost[cost != GC.INT32_MAX].max()) == 466 and int((cost != GC.INT32_MAX).sum()) == 467
    assert calls >= 2                                                        # 16 rounds do not cross 466 moves: several batches
    _, _, _, calls = check_case("serpentine", 6, (1, 1, 1), dev, rounds=1)   # the state carries across calls in cost and the workspace alone
    assert calls > 16
    check_case("serpentine", 26, (3, 4, 5), dev)


def test_max_cost_is_inclusive(dev):
    for conn, w, cap in ((6, (1, 1, 1), 7), (26, (3, 4, 5), 21), (18, (2, 3, 3), 15)):
        cost = check_case("corridor", conn, w, dev, max_cost=cap)[0].reshape(-1)
        last = cap // w[0]
        assert cost[last] == last * w[0] <= cap and (cost[last + 1:] == GC.INT32_MAX).all() and (cost[:last + 1] != GC.INT32_MAX).all()
    cost = check_case("corridor", 6, (1, 1, 1), dev, max_cost=1)[0].reshape(-1)
    assert cost[:3].tolist() == [0, 1, GC.INT32_MAX]
    free, seeds, penalty = GC.case("13x11x19 70%")
    full = GC.reference("13x11x19 70%", 26, (3, 4, 5))[0]
    reached = np.sort(full[full != GC.INT32_MAX])
    cap = int(reached[len(reached) // 2])                                  # a cost that occurs: voxels at exactly the cap stay
    capped = check_case("13x11x19 70%", 26, (3, 4, 5), dev, max_cost=cap)[0]
    assert np.array_equal(capped, np.where(full <= cap, full, GC.INT32_MAX)) and (capped == cap).any() and (full > cap).any()


def test_saturation_and_negative_penalty(dev):
    free, seeds, _ = GC.case("corridor")
    penalty = np.zeros(free.shape, np.int32)
    penalty[0, 0, 5] = penalty[0, 0, 6] = 2 ** 30
    penalty[0, 0, 2] = -5
    penalty[0, 0, 3] = -GC.INT32_MAX - 1
    want, _ = GC.travel_ref(free, seeds, 6, (1, 1, 1), penalty)
    assert want.reshape(-1)[:8].tolist() == [0, 1, 2, 3, 4, 5 + 2 ** 30, GC.INT32_MAX, GC.INT32_MAX]      # 6 + 2^31 does not fit: unreached, and all beyond
    for conn, w in GC.CONFIGS:
        want, _ = GC.travel_ref(free, seeds, conn, w, penalty)
        cost, nxt, dist, _ = run_geo(free, seeds, penalty, conn, w, dev)
        assert np.array_equal(cost, want) and (cost >= 0).all() and (cost.reshape(-1)[6:] == GC.INT32_MAX).all()
        assert np.array_equal(nxt, GC.next_ref(want, conn, w, penalty)) and np.array_equal(dist.view(np.int32), GC.dist_ref(want, STEP, w[0]).view(np.int32))
        zero = np.where(penalty < 0, 0, penalty).astype(np.int32)
        assert np.array_equal(run_geo(free, seeds, zero, conn, w, dev)[0], cost)                          # a negative entry behaves as 0
    # the largest legal weights beside the largest penalty: the sum stays below 2^32 and above every cap
    penalty[0, 0, 1] = GC.INT32_MAX
    cost = run_geo(free, seeds, penalty, 26, (255, 255, 255), dev)[0].reshape(-1)
    assert cost[0] == 0 and (cost[1:] == GC.INT32_MAX).all()


def test_next_ties_take_the_smallest_index(dev):
    _, nxt, _, _ = check_case("open 5x5x5", 26, (1, 1, 1), dev)
    cost = GC.reference("open 5x5x5", 26, (1, 1, 1))[0]
    assert int((cost == 2).sum()) == 98 and nxt[0, 0, 0] == 31 and nxt[2, 2, 2] == 62      # (0,0,0) steps to (1,1,1); the seed to itself
    for conn, w in GC.CONFIGS:
        check_case("open 5x5x5", conn, w, dev)


def run_follow(nxt, starts, max_steps, dev):
    lib = _lib.load()
    t = torch.from_numpy(np.array(nxt).reshape(-1)).to(dev)      # (a copy: the references are read-only)
    s = torch.from_numpy(np.array(starts, dtype=np.int32)).to(dev)
    N = len(starts)
    voxels = poisoned((N, max_steps * 4), torch.int32, dev)
    length = poisoned((N * 4,), torch.int32, dev)
    reached = poisoned((N,), torch.uint8, dev)
    _lib.check(lib.d3f_volume_follow(_lib.ptr(t), t.numel(), _lib.ptr(s), N, max_steps, _lib.ptr(voxels), _lib.ptr(length), _lib.ptr(reached),
                                     _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return voxels.cpu().numpy(), length.cpu().numpy(), reached.cpu().numpy()


def test_follow_equals_the_restatement(dev):
    for name, conn, w in (("serpentine", 6, (1, 1, 1)), ("17x17x17 45%", 26, (3, 4, 5)), ("13x11x19 70%", 18, (2, 3, 3))):
        cost, nxt, _ = GC.reference(name, conn, w)
        c = cost.reshape(-1)
        rng = np.random.default_rng(5)
        far = int(np.argmax(np.where(c == GC.INT32_MAX, -1, c)))
        unreached = np.flatnonzero(c == GC.INT32_MAX)[:3].tolist()
        starts = [far, -1, int(np.flatnonzero(c == 0)[0])] + unreached + rng.integers(0, c.size, 300).tolist() + [c.size, -GC.INT32_MAX - 1, GC.INT32_MAX]
        longest = int(GC.follow_ref(nxt, [far], c.size)[1][0])
        for max_steps in (longest + 3, longest, longest - 1, 1):
            want = GC.follow_ref(nxt, starts, max_steps)
            got = run_follow(nxt, starts, max_steps, dev)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, max_steps)
            assert got[1][0] == min(longest, max_steps) and got[2][0] == (max_steps >= longest) and got[1][1] == 0 and (got[1][3:3 + len(unreached)] == 0).all()
            assert (got[0][1] == -1).all() and (got[2][-3:] == 0).all() and (got[1][-3:] == 0).all()


# ---- BakedField.travel / path -------------------------------------------------------------------------------------------------------
ROOMS_SHAPE, ROOMS_STEP, ROOMS_R = (31, 14, 5), 0.05, 0.12


def rooms(dev):
    """three rooms along x: A | B | C.  The wall between A and B (x = 9) has a door 8 voxels wide (y = 3..10), the wall between B and C (x = 20)
    one 2 voxels wide (y = 6..7); r = 2.4 voxels: a body fits through the first (its middle is >= 3 voxels from a wall) and not the second"""
    dist = np.full(ROOMS_SHAPE, 1.0, np.float32)
    dist[9, :, :] = -1.0
    dist[9, 3:11, :] = 1.0
    dist[20, :, :] = -1.0
    dist[20, 6:8, :] = 1.0
    field = BakedField.from_arrays((0.0, 0.0, 0.0), ROOMS_STEP, torch.from_numpy(dist).to(dev))
    return field.clearance()


def flat(p):
    return int(np.ravel_multi_index(p, ROOMS_SHAPE))


def test_travel_and_path_equal_the_numpy_composition(dev):
    c = rooms(dev)
    goal_voxel, start_a, start_c = (15, 7, 2), (2, 2, 1), (27, 10, 3)
    goal = torch.tensor([[v * ROOMS_STEP for v in goal_voxel]], dtype=torch.float32, device=dev)
    t = c.travel(goal, radius=ROOMS_R)
    free = (c.valid & (c.dist >= ROOMS_R)).cpu().numpy()
    assert free[9, 6, 2] and free[9, 7, 2] and not free[9, 4, 2] and not free[20, 6, 2] and not free[20, 7, 2] and free[goal_voxel]
    want_cost, _ = GC.travel_ref(free, [flat(goal_voxel)], 26, (3, 4, 5))
    want_next = GC.next_ref(want_cost, 26, (3, 4, 5))
    assert np.array_equal(t.cost.cpu().numpy(), want_cost) and np.array_equal(t.next_voxel.cpu().numpy(), want_next)
    assert np.array_equal(t.dist.cpu().numpy().view(np.int32), GC.dist_ref(want_cost, np.float32(ROOMS_STEP), 3).view(np.int32))
    assert np.array_equal(t.valid.cpu().numpy(), want_cost != GC.INT32_MAX) and np.array_equal(t.free.cpu().numpy(), free)
    assert t.names() == [] and t.origin == c.origin and t.step == c.step and t.boundaries == c.boundaries and tuple(t.grid_shape) == ROOMS_SHAPE
    assert c.cost is None and c.next_voxel is None and c.free is None and t.d2 is None and t.nearest_voxel is None
    assert not t.dist.requires_grad and t.cost.dtype == torch.int32 and t.next_voxel.dtype == torch.int32 and t.free.dtype == torch.bool
    # the same field from indices, from an explicit free volume (bool and uint8), and from goals with a NaN / outside row dropped
    idx = torch.tensor([flat(goal_voxel)], dtype=torch.int64, device=dev)
    messy = torch.cat([goal, torch.tensor([[float("nan"), 0, 0], [99.0, 0, 0]], dtype=torch.float32, device=dev)])
    for other in (c.travel(idx, radius=ROOMS_R), c.travel(idx.int(), free=t.free), c.travel(messy, free=t.free.to(torch.uint8) * 7)):
        assert torch.equal(other.cost, t.cost) and torch.equal(other.next_voxel, t.next_voxel) and torch.equal(other.dist.view(torch.int32), t.dist.view(torch.int32))
    # paths: through the wide door the goal is reached over free voxels only; behind the narrow door nothing is
    starts = torch.tensor([[v * ROOMS_STEP for v in start_a], [v * ROOMS_STEP for v in start_c], [float("nan"), 0, 0]], dtype=torch.float32, device=dev)
    out = t.path(starts)
    L = sum(ROOMS_SHAPE)
    want = GC.follow_ref(want_next, [flat(start_a), flat(start_c), -1], L)
    assert tuple(out["voxels"].shape) == (3, L) and out["voxels"].dtype == torch.int32 and out["length"].dtype == torch.int32 and out["reached"].dtype == torch.bool
    assert np.array_equal(out["voxels"].cpu().numpy(), want[0]) and np.array_equal(out["length"].cpu().numpy(), want[1])
    assert out["reached"].tolist() == [True, False, False] and out["length"].tolist()[1:] == [0, 0]
    n0 = int(out["length"][0])
    walked = out["voxels"][0, :n0].cpu().numpy()
    assert walked[0] == flat(start_a) and walked[-1] == flat(goal_voxel) and free.reshape(-1)[walked].all()
    assert (np.abs(np.diff(np.array(np.unravel_index(walked, ROOMS_SHAPE)), axis=1)).max(axis=0) == 1).all()
    assert 9 in np.unravel_index(walked, ROOMS_SHAPE)[0]                                        # it went through the wall's plane: the door
    assert not bool(t.valid[start_c]) and bool(t.valid[start_a]) and bool(torch.isinf(t.dist[start_c]))
    pts = out["points"]
    assert tuple(pts.shape) == (3, L, 3) and pts.dtype == torch.float32 and not pts.requires_grad
    assert torch.equal(pts[0, :n0], t._voxel_centres(out["voxels"][0, :n0])) and bool(torch.isnan(pts[0, n0:]).all()) and bool(torch.isnan(pts[1:]).all())
    cut = t.path(torch.tensor([flat(start_a)], device=dev), max_steps=n0 - 1)                  # one step short: a full row, not reached
    assert cut["reached"].tolist() == [False] and cut["length"].tolist() == [n0 - 1] and np.array_equal(cut["voxels"][0].cpu().numpy(), walked[:-1])
    # connectivity, weights, penalty and max_distance reach the kernels
    pen = torch.from_numpy(np.random.default_rng(2).integers(0, 4, ROOMS_SHAPE).astype(np.int32)).to(dev)
    t6 = c.travel(idx, radius=ROOMS_R, connectivity=6, weights=(2, 2, 2), penalty=pen, max_distance=0.5)
    cap = int(np.floor(0.5 * 2 / c.step))
    want6, _ = GC.travel_ref(free, [flat(goal_voxel)], 6, (2, 2, 2), pen.cpu().numpy(), cap)
    assert np.array_equal(t6.cost.cpu().numpy(), want6) and (want6 == GC.INT32_MAX).sum() > (want_cost == GC.INT32_MAX).sum()
    assert np.array_equal(t6.dist.cpu().numpy().view(np.int32), GC.dist_ref(want6, np.float32(c.step), 2).view(np.int32))


def test_eval_is_the_trilinear_travel_distance_and_descends_to_the_goal(dev):
    shape, step = (17, 15, 13), 0.015625                                    # origin and step are exact in float32
    field = BakedField.from_arrays((0.125, -0.25, 0.375), step, torch.ones(shape, dtype=torch.float32, device=dev))
    goal_voxel = (11, 4, 8)
    everywhere = torch.ones(shape, dtype=torch.bool, device=dev)
    t = field.travel(torch.tensor([int(np.ravel_multi_index(goal_voxel, shape))], device=dev), free=everywhere)
    assert bool(t.valid.all())
    # eval = the trilinear interpolation of dist: against float64 NumPy at random interior points (fp32 chain: a few ulp of the largest corner)
    rng = np.random.default_rng(11)
    g = rng.uniform(0.0, np.array(shape) - 1.0, (500, 3))
    origin = np.array(t.origin)
    pts = torch.from_numpy((origin + g * t.step).astype(np.float32)).to(dev)
    got = t.eval(pts)
    assert bool(got["valid_mask"].all())
    gg = (pts.cpu().numpy().astype(np.float64) - origin) / t.step
    i = np.minimum(np.floor(gg).astype(np.int64), np.array(shape) - 2)
    f = gg - i
    d = t.dist.cpu().numpy().astype(np.float64)
    want = np.zeros(len(gg))
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                wgt = np.where(cx, f[:, 0], 1 - f[:, 0]) * np.where(cy, f[:, 1], 1 - f[:, 1]) * np.where(cz, f[:, 2], 1 - f[:, 2])
                want += wgt * d[i[:, 0] + cx, i[:, 1] + cy, i[:, 2] + cz]
    # fp32 on the device: the lattice coordinate (p - o) / h carries a few ulp of its size (< 16 voxels; 8 ulp allowed), and dist changes by at
    # most h per voxel along an axis (face neighbours differ by at most w1), over three axes; the blend chain adds a few ulp of the largest
    # distance (16 allowed)
    bound = 2.0 ** -24 * (8 * 16 * t.step * 3 + 16 * d.max())
    assert np.abs(got["dist"].cpu().numpy() - want).max() <= bound
    # descent along -grad from interior starts: every step moves closer to the goal (Euclid), until within two voxels of it
    goal = origin + np.array(goal_voxel) * t.step
    p = torch.from_numpy((origin + np.array([[1.3, 12.6, 1.2], [15.2, 13.1, 11.4], [2.5, 2.5, 10.5]]) * t.step).astype(np.float32)).to(dev)
    arrived = np.zeros(3, bool)
    for _ in range(200):
        q = p.clone().requires_grad_(True)
        t.eval(q)["dist"].sum().backward()
        grad = q.grad
        assert bool(torch.isfinite(grad).all())
        before = np.linalg.norm(p.cpu().numpy() - goal, axis=1)
        arrived |= before < 2 * t.step
        if arrived.all():
            break
        move = 0.5 * t.step * grad / torch.linalg.vector_norm(grad, dim=1, keepdim=True).clamp_min(1e-12)
        p = torch.where(torch.from_numpy(arrived).to(dev)[:, None], p, p - move)
        after = np.linalg.norm(p.cpu().numpy() - goal, axis=1)
        assert (after[~arrived] < before[~arrived]).all()
    assert arrived.all()


def test_travel_and_path_errors(dev):
    c = rooms(dev)
    plain = BakedField.from_arrays((0.0, 0.0, 0.0), ROOMS_STEP, torch.ones(ROOMS_SHAPE, dtype=torch.float32, device=dev))
    idx = torch.tensor([flat((15, 7, 2))], device=dev)
    free = torch.ones(ROOMS_SHAPE, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError):
        c.travel(idx)                                            # neither radius nor free
    with pytest.raises(ValueError):
        c.travel(idx, radius=0.1, free=free)                     # both
    with pytest.raises(ValueError):
        plain.travel(idx, radius=0.1)                            # radius on a field that is no clearance field
    for bad in (free[:-1], free.float(), free.int(), "free"):
        with pytest.raises(ValueError):
            c.travel(idx, free=bad)
    for bad in ((0, 1, 1), (3, 2, 5), (3, 4, 256), (3, 4), (3.0, 4.0, 5.0), None):
        with pytest.raises(ValueError):
            c.travel(idx, radius=0.1, weights=bad)
    for bad in (4, 8, 0, None):
        with pytest.raises(ValueError):
            c.travel(idx, radius=0.1, connectivity=bad)
    for bad in (torch.zeros(ROOMS_SHAPE, dtype=torch.int64, device=dev), torch.zeros((3, 3, 3), dtype=torch.int32, device=dev), 3):
        with pytest.raises(ValueError):
            c.travel(idx, radius=0.1, penalty=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), ROOMS_STEP / 3 * 0.9):
        with pytest.raises(ValueError):
            c.travel(idx, radius=0.1, max_distance=bad)
    for bad in (torch.zeros((2, 2), dtype=torch.float32, device=dev), torch.zeros((2, 3), dtype=torch.float64, device=dev), idx.float(), [5]):
        with pytest.raises(ValueError):
            c.travel(bad, radius=0.1)
    for kw in (dict(goals=idx.cpu(), radius=0.1), dict(goals=idx, free=free.cpu()), dict(goals=idx, radius=0.1, penalty=torch.zeros(ROOMS_SHAPE, dtype=torch.int32))):
        with pytest.raises(RuntimeError):
            c.travel(**kw)
    t = c.travel(idx, radius=0.1)
    with pytest.raises(ValueError):
        c.path(idx)                                              # not a travel field
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            t.path(idx, max_steps=bad)
    with pytest.raises(ValueError):
        t.path(idx.float())
    with pytest.raises(RuntimeError):
        t.path(idx.cpu())
    empty = t.path(torch.zeros((0, 3), dtype=torch.float32, device=dev), max_steps=4)
    assert tuple(empty["voxels"].shape) == (0, 4) and tuple(empty["points"].shape) == (0, 4, 3) and tuple(empty["reached"].shape) == (0,)
    none = c.travel(torch.zeros((0,), dtype=torch.int64, device=dev), radius=0.1)      # no goal: nothing is reached
    assert not bool(none.valid.any()) and bool((none.next_voxel == -1).all())
