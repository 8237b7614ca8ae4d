"""Keypoint selection (Fusion.select_features_rand, reference fusion.py:1418-1475) at the sizes where its two kernels change path.

The pre-filter (grid_kernels.hip: grid_shell_flag_fast_kernel) gives every wave ONE 256-point block below 2^18 blocks and FOUR consecutive
ones from there on (launch_shell_flag_fast: kShellBlocks), which is where the default call -- a 1-mm grid of 123 M points -- runs; the other
tests of the shell stop at 4.2 M points.  Here both sides of the switch, a grid whose last workgroup has waves without a block and a ragged
last block, against the distance-only kernel on EVERY lattice point (tests/test_gpu_dist.py pins that kernel to the CPU oracle bit for bit)
and against the CPU oracle itself on a sample built around the places a block loop can go wrong.  Nothing observable says which loop ran:
the asserts on the block count stand in for it.

Farthest point sampling (fps_round_kernel, shared by the float and the pixel variant) runs a round on fps_blocks(n) workgroups, each of which
owns one entry per round parity of a table of 2 x 256: the sizes around every change of that count, with a workspace of exactly the bytes the
size function names between guard bytes (tests/dirty_buffers.py).  For n = 262145 .. 262399 the count used to be 257: in odd rounds the last
workgroup wrote the 16 bytes behind the workspace, in even rounds entry 0 of the other parity, which the same launch reads.

Every comparison is exact -- indices, bits, guard bytes.  The only caps are the oracle's sample of at most 300 000 lattice points and the
bounds on the survivor count, both asserted below."""
import numpy as np
import pytest
import torch

from dirty_buffers import GUARD, DirtyBuffers

pytestmark = pytest.mark.gpu

H, W = 240, 320
SHELL_BLOCK = 256                       # kBlock: points of one block of the pre-filter
SHELL_BLOCKS_PER_WAVE = 4               # kShellBlocks, from SHELL_SWITCH blocks on
SHELL_SWITCH = 1 << 18
SAMPLE_MAX = 300000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cpu(x):
    return x.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def _fusion(dev, sc):
    from d3fields_amd import Fusion
    f = Fusion(num_cam=sc["K"].shape[0], device=str(dev))
    f.curr_obs_torch = {k: sc[k].to(dev) for k in ("depth", "K", "pose")}
    f.H, f.W = H, W
    return f


def _box(dims, step):
    """the box of test_grid_shell_fast_pass_keeps_the_same_survivors (tests/test_gpu_dist.py)"""
    return dict(x_lower=-dims[0] * step / 2, x_upper=dims[0] * step / 2 - step / 4, y_lower=-dims[1] * step / 2,
                y_upper=dims[1] * step / 2 - step / 4, z_lower=-0.05, z_upper=-0.05 + dims[2] * step - step / 4)


@pytest.fixture(scope="module")
def lattices():
    """(box, lattice on the host) of the last shape asked for: the two cases on one shape build it once"""
    held = {}

    def get(dims, step):
        from d3fields_amd import create_init_grid
        if (dims, step) not in held:
            held.clear()
            box = _box(dims, step)
            held[(dims, step)] = (box, create_init_grid(box, step)[0])
        return held[(dims, step)]

    yield get
    held.clear()


def shell_sample(n, seed):
    """at most SAMPLE_MAX flat indices, ascending: both ends of the grid, every point of the four blocks of wave 0, of a wave in the middle and of the
    last wave that owns a block, the indices around the last one of the last block's 256 (n - 1 is among them, or lies before them), random ones"""
    nb = (n + SHELL_BLOCK - 1) // SHELL_BLOCK
    waves = (nb + SHELL_BLOCKS_PER_WAVE - 1) // SHELL_BLOCKS_PER_WAVE
    parts = [np.arange(0, 2048), np.arange(n - 2048, n)]
    for wave in (0, waves // 2, waves - 1):
        first = wave * SHELL_BLOCKS_PER_WAVE
        assert first < nb
        parts.append(np.arange(first * SHELL_BLOCK, min(first + SHELL_BLOCKS_PER_WAVE, nb) * SHELL_BLOCK))
    parts.append(np.arange(nb * SHELL_BLOCK - 1 - 1024, nb * SHELL_BLOCK - 1 + 1024))
    fixed = np.unique(np.concatenate(parts))
    fixed = fixed[(fixed >= 0) & (fixed < n)]
    assert 2 * 2048 + 4 * SHELL_BLOCK <= fixed.size <= 2 * 2048 + 3 * 4 * SHELL_BLOCK + 2048      # (wave 0 lies inside the first 2048, the last wave near the last)
    rest = np.random.default_rng(seed).integers(0, n, SAMPLE_MAX - fixed.size)
    sample = np.unique(np.concatenate([fixed, rest]))
    assert SAMPLE_MAX - 2000 < sample.size <= SAMPLE_MAX and sample[0] == 0 and sample[-1] == n - 1       # (a few hundred random ones collide)
    return sample


# V, dims, what the shape is for: n, blocks, blocks per wave, blocks in the last workgroup's 16, points in the last block
SHELL_CASES = [
    (4, (512, 512, 256), dict(n=1 << 26, nb=1 << 18, per_wave=4, last_group=0, last_block=0)),          # the first size with four blocks per wave, every workgroup full
    (4, (189, 256, 1387), dict(n=(1 << 26) - 256, nb=(1 << 18) - 1, per_wave=1, last_group=15, last_block=0)),   # the last size with one block per wave
    (8, (409, 401, 410), dict(n=67243690, nb=262671, per_wave=4, last_group=15, last_block=170)),      # waves without a block, a ragged last block, two view batches
    (1, (409, 401, 410), dict(n=67243690, nb=262671, per_wave=4, last_group=15, last_block=170)),      # the same shape on the one-view instance
]


@pytest.mark.parametrize("V,dims,want", SHELL_CASES, ids=["V%d-%dx%dx%d" % ((c[0],) + c[1]) for c in SHELL_CASES])
def test_grid_shell_on_both_sides_of_the_block_loop_switch(dev, lattices, V, dims, want):
    from d3fields_amd import synth
    from oracle import c_oracle as O
    step, thr = 0.0008, 0.005
    n = dims[0] * dims[1] * dims[2]
    nb = (n + SHELL_BLOCK - 1) // SHELL_BLOCK
    assert n == want["n"] < 0xffffffff and nb == want["nb"] and nb % 16 == want["last_group"] and n % SHELL_BLOCK == want["last_block"]
    assert (SHELL_BLOCKS_PER_WAVE if nb >= SHELL_SWITCH else 1) == want["per_wave"]
    sc = synth.make_scene(V, H, W, "smooth")
    box, pts_c = lattices(dims, step)
    assert pts_c.shape[0] == n
    f = _fusion(dev, sc)
    idx, pts = f.grid_shell(box, step, thr)
    print("V=%d %s: %d of %d lattice points survive (%.2f %%)" % (V, dims, idx.numel(), n, 100.0 * idx.numel() / n))
    assert 1000 < idx.numel() < n // 16, "outside these bounds a second launch with the exact capacity would hide the first"
    assert idx.dtype == torch.int64 and bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < n

    # every point: the distance-only kernel on the materialised lattice
    lattice = pts_c.to(dev)
    with torch.no_grad():
        out = f.batch_eval(lattice, return_names=[])
    keep = out["valid_mask"] & (out["dist"].abs() < torch.tensor(np.float32(thr), device=dev))
    want_idx = torch.nonzero(keep).reshape(-1)
    del out, keep
    assert idx.numel() == want_idx.numel() and torch.equal(idx, want_idx)
    assert torch.equal(bits(pts), bits(lattice[idx]))
    del lattice, want_idx

    # a sample: the CPU oracle directly
    sample = shell_sample(n, seed=V)
    ref = O.eval_field(sc["depth"], sc["K"], sc["pose"], pts_c[torch.from_numpy(sample)], [])
    verdict = ref["valid_mask"].astype(bool) & (np.abs(ref["dist"]) < np.float32(thr))
    got = cpu(idx)
    at = np.minimum(np.searchsorted(got, sample), got.size - 1)
    member = got[at] == sample
    assert 100 < verdict.sum() < sample.size // 4, "the sample would say little"
    wrong = np.nonzero(member != verdict)[0]
    assert wrong.size == 0, ("flat indices whose membership differs from the oracle's verdict", sample[wrong][:8].tolist(), member[wrong][:8].tolist())
    torch.cuda.empty_cache()


def test_grid_shell_wrapper_runs_again_with_the_exact_capacity(dev, lattices):
    """a shell thicker than the first capacity (max(65536, n / 16) indices): Fusion.grid_shell must launch a second time with the count of the
    first -- every survivor against the oracle"""
    from d3fields_amd import synth
    from oracle import c_oracle as O
    dims, step, thr = (90, 81, 37), 0.004, 0.02
    n = dims[0] * dims[1] * dims[2]
    sc = synth.make_scene(3, H, W, "smooth")
    box, pts_c = lattices(dims, step)
    assert pts_c.shape[0] == n and max(1 << 16, n // 16) == 65536
    ref = O.eval_field(sc["depth"], sc["K"], sc["pose"], pts_c, [])
    want = np.nonzero(ref["valid_mask"].astype(bool) & (np.abs(ref["dist"]) < np.float32(thr)))[0]
    assert want.size == 109449 > 65536
    idx, pts = _fusion(dev, sc).grid_shell(box, step, thr)
    assert idx.numel() > 65536
    assert np.array_equal(cpu(idx), want)
    assert np.array_equal(cpu(pts).view(np.int32), pts_c.numpy()[want].view(np.int32))


# ---- farthest point sampling -------------------------------------------------------------------------------------------------------------------
FPS_K = 24
FPS_N = [1, 2, 1023, 1024, 1025, 262144, 262145, 262399, 262400]       # 1 | 2 workgroups, and 256 x 1024 points, the window that took 257, 256 x 1025
FPS_CASES = [(n, init) for n in FPS_N for init in sorted({0, n - 1})]
FPS_IDS = ["n%d-from%d" % c for c in FPS_CASES]
PIX_IMAGE = (520, 512)


def _frozen(a):
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def clouds():
    """the inputs at their full length, read-only; a case takes the first n rows"""
    top = max(FPS_N)
    normal = np.random.default_rng(11).normal(size=(top, 3)).astype(np.float32)
    tied = np.tile(np.random.default_rng(12).normal(size=(1000, 3)).astype(np.float32), ((top + 999) // 1000, 1))[:top]   # exact ties across every chunk border
    rows, cols = np.divmod(np.random.default_rng(13).permutation(PIX_IMAGE[0] * PIX_IMAGE[1]), PIX_IMAGE[1])
    pixels = np.stack([rows, cols], 1).astype(np.int64)
    assert pixels.shape[0] >= top and np.unique(pixels, axis=0).shape[0] == pixels.shape[0]
    return {"normal": _frozen(normal), "tied": _frozen(tied), "pixels": _frozen(pixels)}


def _guarded_fps(dev, monkeypatch, entry, size_fn, pts, init, maxd_dtype):
    """the C entry point on a workspace of exactly size_fn(n) bytes, 16-byte aligned, with GUARD bytes of a fixed value in front of it and behind
    it (and around both outputs): (indices, maximum distance, damage to the guards)"""
    from d3fields_amd import _lib
    assert GUARD >= 256
    n = pts.shape[0]
    db = DirtyBuffers(monkeypatch)
    with db.guarded(), _lib.on(dev) as q:
        nbytes = int(getattr(q, size_fn)(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        idx = torch.empty(FPS_K, dtype=torch.int64, device=dev)
        maxd = torch.empty(1, dtype=maxd_dtype, device=dev)
        assert ws.numel() == nbytes > 0 and ws.data_ptr() % 16 == 0
        getattr(q, entry)(pts, n, FPS_K, init, idx, maxd, ws)
        torch.cuda.synchronize()
    return cpu(idx), maxd.item(), db.damage()


@pytest.mark.parametrize("kind", ["normal", "tied"])
@pytest.mark.parametrize("n,init", FPS_CASES, ids=FPS_IDS)
def test_fps_at_the_workgroup_count_edges(dev, monkeypatch, clouds, kind, n, init):
    from oracle import c_oracle as O
    cloud = clouds[kind][:n]
    idx, maxd, damage = _guarded_fps(dev, monkeypatch, "d3f_farthest_point_sampling", "d3f_fps_workspace_bytes", torch.from_numpy(cloud.copy()).to(dev), init, torch.float32)
    assert not damage, ("(allocation, its bytes, side, changed guard bytes, offset of the first from the buffer's start); allocation 0 is the workspace", damage)
    want_idx, want_maxd = O.fps(cloud, FPS_K, init)
    assert idx.tolist() == want_idx.tolist() and maxd == want_maxd


@pytest.mark.parametrize("n,init", FPS_CASES, ids=FPS_IDS)
def test_fps_pixels_at_the_workgroup_count_edges(dev, monkeypatch, clouds, n, init):
    from oracle import np_pcd
    pix = clouds["pixels"][:n]
    idx, maxd, damage = _guarded_fps(dev, monkeypatch, "d3f_fps_pixels", "d3f_fps_pixels_workspace_bytes", torch.from_numpy(pix.astype(np.int32)).to(dev), init, torch.float64)
    assert not damage, ("(allocation, its bytes, side, changed guard bytes, offset of the first from the buffer's start); allocation 0 is the workspace", damage)
    _, want_idx, want_maxd = np_pcd.fps_int(pix, FPS_K, init)
    assert idx.tolist() == want_idx and maxd == want_maxd
