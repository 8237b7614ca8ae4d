"""GPU: the descriptor-similarity kernels (csrc/corr_kernels.hip) entry by entry against oracle/corr_ref.py's float64 bounds.

Every distance, similarity and softmax entry lies inside corr_ref's per-entry interval; every best match and k-NN list is
an admissible order (no unplaced row definitely better; NaN after +Inf; NaN rows and exact ties by row) and equals the
ranking of the kernel's own distances.  The MFMA path (B1 >= 512, C % 32 == 0, 16-byte aligned operands) and the direct
kernel run on identical data: a 4-byte-offset view of the same rows is not 16-byte aligned, so it takes the direct kernel
through the same C ABI.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

from oracle import corr_cases as K, corr_ref as R

pytestmark = pytest.mark.gpu
DT = {"l2": 0, "square": 1}
SIM_DIST, SIM_EXP, SIM_SOFTMAX = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cpu(x):
    return x.detach().cpu().numpy()


def to_dev(a, dev, offset=False):
    """a float32 array on the device; offset=True: a view 4 bytes into a larger buffer (not 16-byte aligned)"""
    t = torch.as_tensor(np.ascontiguousarray(a, np.float32))
    if not offset:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    buf[1:] = t.reshape(-1).to(dev)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


def pairwise(src, tgt, scale, dt, mode, argmax=True):
    """d3f_pairwise_similarity on device tensors src [B1,C], tgt [B2,C] (any alignment) -> (out, argmax or None)"""
    from d3fields_amd import _lib
    lib = _lib.load()
    dev = src.device
    B1, C = src.shape
    B2 = tgt.shape[0]
    out = torch.empty((B1, B2), dtype=torch.float32, device=dev)
    am = torch.full((B2,), -7, dtype=torch.int64, device=dev) if argmax else None
    nb = lib.d3f_softmax_workspace_bytes(B1, B2)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.d3f_pairwise_similarity(_lib.ptr(src), _lib.ptr(tgt), B1, B2, C, float(scale), DT[dt], mode, _lib.ptr(out),
                                               _lib.ptr(am), _lib.ptr(ws), nb, _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return out, am


def knn(src, tgt, k, scale, dt, mode):
    from d3fields_amd import _lib
    lib = _lib.load()
    dev = src.device
    B1, C = src.shape
    B2 = tgt.shape[0]
    out = torch.empty((B1, B2), dtype=torch.float32, device=dev)
    idx = torch.full((k, B2), -7, dtype=torch.int64, device=dev)
    val = torch.empty((k, B2), dtype=torch.float32, device=dev)
    nb = lib.d3f_pairwise_topk_workspace_bytes(B1, B2)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.d3f_pairwise_similarity_topk(_lib.ptr(src), _lib.ptr(tgt), B1, B2, C, float(scale), DT[dt], mode, k,
                                                    _lib.ptr(out), _lib.ptr(idx), _lib.ptr(val), _lib.ptr(ws), nb,
                                                    _lib.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return out, idx, val


def check_all(src, tgt, D, dt, scale, dev, offset=False, what=""):
    """one data set through the three modes (+ best match); returns the float32 distances of the kernel"""
    s, t = to_dev(src, dev, offset), to_dev(tgt, dev, offset)
    d, am = pairwise(s, t, scale, dt, SIM_DIST)
    d = cpu(d)
    R.check_dist(d, D, "distance " + what)
    R.check_ranked(cpu(am), D, scale=1.0, what="argmin " + what)
    assert np.array_equal(cpu(am), R.rank_order(d, 1)[0]), "argmin is not the smallest of the kernel's own distances " + what
    e, _ = pairwise(s, t, scale, dt, SIM_EXP, argmax=False)
    R.check_exp(cpu(e), D, scale, "exp " + what)
    p, am = pairwise(s, t, scale, dt, SIM_SOFTMAX)
    R.check_softmax(cpu(p), D, scale, "softmax " + what)
    R.check_ranked(cpu(am), D, scale=scale, what="softmax argmax " + what)
    return d


@pytest.mark.parametrize("B1,B2,C,dt,scale", [(4096, 300, 384, "l2", 1.0), (100000, 300, 384, "l2", 3.0),
                                              (2048, 80, 64, "square", 0.05), (513, 66, 32, "l2", 30.0),
                                              (1024, 70, 96, "square", -0.7)])
def test_mfma_and_direct_kernels_within_float64_bounds(dev, B1, B2, C, dt, scale):
    """guard edges on identical data through the MFMA path and the direct kernel: exact duplicates (d = 0), matches graded
    across the 1/4 threshold, an exact tie across two 64-row tiles and a near tie inside one, the offset column -- each in
    a SPARSE tile of column block 0 (asserted: the contraction and the wave's recompute handle them on the MFMA path) --
    plus a dense tile (> 96 flagged pairs: the direct form inside the MFMA kernel) and +Inf / NaN in sources and targets
    (a column tile of their own)"""
    src, tgt, info = K.guard_case(B1, B2, C, seed=B1 + C)
    c_inf, c_nan = K.add_nonfinite(src, tgt, inf_rows=scale > 0)
    tiles = K.flags_per_tile(*K.flags64(src, tgt))
    for r in K.edge_rows(info):
        assert 0 < tiles[r // 64, 0] <= 96, (r, tiles[r // 64, 0])
    assert tiles[info["dense"] // 64, 0] > 96
    D = R.pairwise(src, tgt, dt)
    d_mfma = check_all(src, tgt, D, dt, scale, dev, what="mfma %d" % B1)
    d_direct = check_all(src, tgt, D, dt, scale, dev, offset=True, what="direct %d" % B1)
    assert d_mfma[info["rows"][0], 0] == 0.0 and d_direct[info["rows"][0], 0] == 0.0
    assert d_mfma[70, 10] == 0.0 and d_mfma[200, 10] == 0.0
    _, am = pairwise(to_dev(src, dev), to_dev(tgt, dev), scale, dt, SIM_SOFTMAX)
    am = cpu(am)
    assert am[c_nan] == 0                                        # all-NaN column: row 0, never the INT64_MAX sentinel
    assert ((am >= 0) & (am < B1)).all()
    if scale > 0:
        assert am[10] == 70                                      # exact duplicate rows 70 / 200 in two row tiles: the lower
        assert (am[:5] == np.array(info["rows"][:5])).all()      # the graded matches well inside the guard's threshold


@pytest.mark.parametrize("nflag", [96, 97])
def test_guard_dense_threshold(dev, nflag):
    """one 64 x 64 tile with exactly 96 (wave recompute) and 97 (whole tile direct) pairs that fail the guard"""
    from oracle import corr_emul as E
    rng = np.random.default_rng(nflag)
    B1, B2, C = 1024, 128, 64
    src, tgt = K.randn(rng, B1, C), K.randn(rng, B2, C)
    base = K.randn(rng, C)
    src[128:140] = base + np.float32(0.05) * K.randn(rng, 12, C)
    tgt[64:72] = base + np.float32(0.05) * K.randn(rng, 8, C)
    if nflag == 97:
        tgt[72] = src[141]
    raw = E.contraction(src, tgt, guard=False)
    nsum = (E._norms(src)[:, None] + E._norms(tgt)[None, :]).astype(np.float32)
    tiles = K.flags_per_tile(raw, nsum)
    assert tiles[2, 1] == nflag and tiles.sum() == nflag
    D = R.pairwise(src, tgt, "l2")
    check_all(src, tgt, D, "l2", 2.0, dev, what="tile %d" % nflag)


_B1S = [1, 63, 64, 65, 511, 512, 513]
_B2S = [1, 15, 16, 17, 63, 64, 65, 300]
_CS = [1, 31, 32, 33, 384]
_SCALES = [0.0, 0.05, 3.0, 30.0, -0.7]


@pytest.mark.parametrize("B1", _B1S)
def test_shapes_tails_and_scales(dev, B1):
    """every B2 tail (NWT = 1..4 live 16-column groups), C around the 32-channel stage, all scales, both dist types"""
    for n, B2 in enumerate(_B2S):
        C = _CS[(n + B1) % len(_CS)]
        scale = _SCALES[(n + B1) % len(_SCALES)]
        dt = ("l2", "square")[n % 2]
        rng = np.random.default_rng(1000 * B1 + B2)
        src, tgt = K.randn(rng, B1, C), K.randn(rng, B2, C)
        tgt[0] = src[B1 // 2]
        if B1 > 3:
            src[B1 - 1] = src[1]                                 # an exact duplicate row
        D = R.pairwise(src, tgt, dt)
        check_all(src, tgt, D, dt, scale, dev, what="B1 %d B2 %d C %d" % (B1, B2, C))


@pytest.mark.parametrize("B1,B2,C", [(600, 70, 1000), (700, 301, 48), (600, 16387, 32), (520, 16400, 32)])
def test_wide_channels_and_both_softmax_apply_kernels(dev, B1, B2, C):
    """C = 1000; B2 % 4 != 0 and B2 / 4 > 4096 take the scalar softmax_apply_kernel, B2 = 70 / 300 the vector one"""
    rng = np.random.default_rng(B2)
    src, tgt = K.randn(rng, B1, C), K.randn(rng, B2, C)
    tgt[1] = src[3]
    D = R.pairwise(src, tgt, "l2")
    check_all(src, tgt, D, "l2", 0.9, dev, what="B2 %d C %d" % (B2, C))


def _dist_rows_chunked(src_dev, tgt, chunk=1 << 19):
    """float64 d^2 [B1, B2] of a large device matrix, copied to the host a row chunk at a time"""
    return np.concatenate([R.dist2(cpu(src_dev[i:i + chunk]), tgt) for i in range(0, src_dev.shape[0], chunk)])


def test_outputs_past_two_to_the_31(dev):
    """B1 * B2 > 2^31: 64-bit output offsets (the host turns the fast kernels off); a seeded sample of columns is copied
    back and checked completely"""
    B1, B2, C = (1 << 21) + 64, 1100, 32
    assert B1 * B2 > 1 << 31
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randn(B1, C, device=dev, generator=gen)
    tgt = torch.randn(B2, C, device=dev, generator=gen)
    tgt[B2 - 1] = src[B1 - 1]
    tgt[0] = src[B1 - 70]
    cols = np.sort(np.concatenate([[0, B2 - 1], np.random.default_rng(5).choice(np.arange(1, B2 - 1), 6, replace=False)]))
    tg = cpu(tgt)[cols]
    D = R.Dist(_dist_rows_chunked(src, tg), C, "l2")
    out, am = pairwise(src, tgt, 1.0, "l2", SIM_DIST)
    R.check_dist(cpu(out[:, torch.from_numpy(cols).to(dev)]), D, "distance past 2^31")
    R.check_ranked(cpu(am)[cols], D, scale=1.0, what="argmin past 2^31")
    del out
    out, am = pairwise(src, tgt, 0.5, "l2", SIM_SOFTMAX)
    R.check_softmax(cpu(out[:, torch.from_numpy(cols).to(dev)]), D, 0.5, "softmax past 2^31")
    R.check_ranked(cpu(am)[cols], D, scale=0.5, what="argmax past 2^31")
    assert cpu(am)[B2 - 1] == B1 - 1 and cpu(am)[0] == B1 - 70


def test_row_limit_and_sources_past_two_to_the_30(dev):
    """B1 = 64 * 65535 (the grid's row limit) with B1 * C > 2^30 (64-bit source offsets); one row more is refused"""
    from d3fields_amd import _lib
    B1, B2, C = 64 * 65535, 9, 257
    assert B1 * C > 1 << 30
    gen = torch.Generator(device=dev).manual_seed(7)
    src = torch.randn(B1, C, device=dev, generator=gen)
    tgt = torch.randn(B2, C, device=dev, generator=gen)
    tgt[3] = src[B1 - 1]
    tgt[4] = src[B1 // 2] + 1e-3
    D = R.Dist(_dist_rows_chunked(src, cpu(tgt)), C, "square")
    out, am = pairwise(src, tgt, 2.0, "square", SIM_SOFTMAX)
    R.check_softmax(cpu(out), D, 2.0, "softmax at the row limit")
    R.check_ranked(cpu(am), D, scale=2.0, what="argmax at the row limit")
    assert cpu(am)[3] == B1 - 1 and cpu(am)[4] == B1 // 2
    del out
    lib = _lib.load()
    with pytest.raises(_lib.D3FError):
        _lib.check(lib.d3f_pairwise_similarity(_lib.ptr(src), _lib.ptr(tgt), B1 + 1, B2, C, 1.0, 0, SIM_DIST, _lib.ptr(src), None, None, 0,
                                               _lib.current_stream_handle(dev)))


def test_tiny_and_huge_magnitudes(dev):
    """1e-20 descriptors (squares in the subnormal range) and 1e18 ones (d^2 near and past FLT_MAX), both kernels"""
    rng = np.random.default_rng(3)
    for mag, C in ((1e-20, 64), (1e18, 32), (1e18, 384)):
        src, tgt = (K.randn(rng, 700, C) * np.float32(mag)), (K.randn(rng, 40, C) * np.float32(mag))
        tgt[0] = src[5]
        D = R.pairwise(src, tgt, "square")
        scale = 1e37 if mag < 1 else 1e-36                       # logits of order 1
        for off in (False, True):
            check_all(src, tgt, D, "square", scale, dev, offset=off, what="magnitude %g C %d" % (mag, C))


@pytest.mark.parametrize("B1,B2,C", [(4096, 300, 384), (100000, 37, 64), (5, 3, 16), (700, 65, 33)])
def test_topk_admissible_and_self_consistent(dev, B1, B2, C):
    """k = 1..8: admissible against float64, equal to the header's order of the kernel's own distances, val = sim at the
    returned rows, -1 / NaN past B1, k = 1 equal to the fused argmax (same scale-1 logits); NaN and +Inf rows together"""
    src, tgt, _ = K.guard_case(B1, B2, C, seed=B1 * 3 + C)
    src[min(3, B1 - 1)] = np.inf
    src[1 % B1, 0] = np.nan
    D = R.pairwise(src, tgt, "l2")
    s, t = to_dev(src, dev), to_dev(tgt, dev)
    dist, am = pairwise(s, t, 1.0, "l2", SIM_DIST)
    dist, am = cpu(dist), cpu(am)
    for k in range(1, 9):
        mode = (SIM_DIST, SIM_EXP, SIM_SOFTMAX)[k % 3]
        out, idx, val = knn(s, t, k, 1.3, "l2", mode)
        idx, val, out = cpu(idx), cpu(val), cpu(out)
        R.check_ranked(idx, D, what="k-NN k=%d" % k)
        assert np.array_equal(idx, R.rank_order(dist, k)), k
        kk = min(k, B1)
        assert (idx[kk:] == -1).all() and np.isnan(val[kk:]).all()
        assert np.array_equal(val[:kk], np.take_along_axis(out, idx[:kk], 0), equal_nan=True)
        if k == 1:
            assert np.array_equal(idx[0], am)
    if B1 == 5:                                                  # every row placed: finite ones, then +Inf (row 3), then NaN (row 1)
        _, idx, _ = knn(s, t, 8, 1.0, "l2", SIM_DIST)
        assert cpu(idx)[3:5].tolist() == [[3] * B2, [1] * B2]


@pytest.mark.parametrize("splits", [(0, 1700, 1700, 5000), (0, 100, 2500, 4999, 5000), (0, 5000)])
def test_row_sharded_steps(dev, splits):
    """d3f_pairwise_softmax_local / merge / apply and d3f_topk_smallest / merge: ragged splits, a split inside a 64-row tile,
    an empty rank, non-finite rows; softmax, global best match and k-NN against float64"""
    from d3fields_amd.sharding import _HipSoftmaxKernels as S, _HipTopkKernels as T
    src, tgt, _ = K.guard_case(5000, 70, 64, seed=11)
    _, c_nan = K.add_nonfinite(src, tgt)
    D = R.pairwise(src, tgt, "l2")
    s, t = to_dev(src, dev), to_dev(tgt, dev)
    blocks = [(splits[i], splits[i + 1]) for i in range(len(splits) - 1)]
    local = [S.local(s[lo:hi].contiguous(), t, 0.7, 0, lo) for lo, hi in blocks]
    merged, am = S.merge(torch.stack([st for _, st in local]))
    rows = torch.cat([S.apply(o, 0.7, merged) for o, _ in local])
    torch.cuda.synchronize()
    R.check_softmax(cpu(rows), D, 0.7, "sharded softmax")
    R.check_ranked(cpu(am), D, scale=0.7, what="sharded argmax")
    assert cpu(am)[c_nan] == 0
    k = 5
    dist = [pairwise(s[lo:hi].contiguous(), t, 1.0, "l2", SIM_DIST, argmax=False)[0] for lo, hi in blocks]
    parts = []
    for (lo, hi), d in zip(blocks, dist):
        i, v = T.local_topk(d, k)
        parts.append((torch.where(i >= 0, i + lo, i), v))
    gi, gv = T.merge_topk(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
    gi = cpu(gi)
    R.check_ranked(gi, D, what="sharded k-NN")
    assert np.array_equal(gi, R.rank_order(cpu(torch.cat(dist)), k))


@pytest.mark.parametrize("layout,B,HW,C", [("bhwc", 3, (10, 12), 1), ("bhwc", 4, (7, 9), 63), ("bhwc", 2, (480, 640), 64),
                                           ("bhwc", 3, (5, 7), 65), ("bhwc", 3, (6, 11), 1000),
                                           ("bchw", 3, (480, 640), 64), ("bchw", 5, (7, 9), 384), ("bchw", 1, (3, 5), 1)])
def test_similarity_to_target(dev, layout, B, HW, C):
    """d3f_similarity_to_target in all three modes: channels contiguous (64 lanes per descriptor) and BCHW (one lane)"""
    from d3fields_amd import corr_utils as cu
    rng = np.random.default_rng(B * C + HW[0])
    fm = K.randn(rng, B, HW[0], HW[1], C)
    tgt = K.randn(rng, C)
    fm[B - 1, 0, 0] = tgt                                        # d = 0
    if B > 1:
        fm[0, 1, 1] = tgt + np.float32(1e-3)
    fm[0, HW[0] - 1, HW[1] - 1, 0] = np.nan
    inner = HW[0] * HW[1]
    D = R.to_target(fm.reshape(-1, C), tgt, "l2")
    Db = R.Dist(D.d.reshape(B, inner) ** 2, C, "l2")            # [B, inner] for softmax over B
    t = torch.from_numpy(tgt).to(dev)
    if layout == "bhwc":
        x = torch.from_numpy(fm).to(dev)
        axis = -1
    else:
        x = torch.from_numpy(np.ascontiguousarray(fm.transpose(0, 3, 1, 2))).to(dev)
        axis = 1
    for dt in ("l2", "square"):
        Dd = D if dt == "l2" else R.Dist(D.d ** 2, C, "square")
        Dbd = Db if dt == "l2" else R.Dist(Db.d ** 2, C, "square")
        d = cpu(cu._to_target(x, t, 1.0, dt, SIM_DIST, axis)).reshape(-1, 1)
        R.check_dist(d, Dd, "to_target dist %s %s" % (layout, dt))
        for scale in (0.0, 0.7, 30.0, -0.2):
            e = cpu(cu._to_target(x, t, scale, dt, SIM_EXP, axis)).reshape(-1, 1)
            R.check_exp(e, Dd, scale, "to_target exp %s %s %g" % (layout, dt, scale))
            p = cpu(cu._to_target(x, t, scale, dt, SIM_SOFTMAX, axis)).reshape(B, inner)
            R.check_softmax(p, Dbd, scale, "to_target softmax %s %s %g" % (layout, dt, scale))
