"""Multi-GPU sharding of the field query: one process per GPU, torch.distributed over RCCL/xGMI.

Query points are independent (no cross-point term in fusion.py:305-394), so a batch is split
into contiguous blocks, one per rank, evaluated by the single-GPU HIP kernel against
*replicated* maps, and the field is reassembled with ONE all-gather per output tensor.  There is
no other collective on the path.  The reference is single-GPU (fusion.py:203), so the only
parity statement is: gathered results == single-GPU results, bit for bit (same kernel, same
per-point arithmetic) -- tests/test_sharding_gloo.py checks the plumbing with world_size 2.

Cost note: gathering the full [N,C] field moves (P-1)/P * N*C*4 bytes into
every GPU and dwarfs the query itself; consumers that only need the distance volume (marching
cubes, fusion.py:1313-1330) should gather keys=('dist','valid_mask') and leave features sharded.
"""
import torch
import torch.distributed as dist

from . import _lib

__all__ = ["shard_bounds", "shard_points", "all_gather_field", "gather_bytes", "sharded_eval", "broadcast_observation",
           "sharded_similarity_multi", "sharded_knn_descriptors"]


def _world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def shard_bounds(n, rank, world):
    """Contiguous block [lo, hi) of rank `rank`; the first n % world ranks get one extra point."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_points(pts, rank=None, world=None, group=None):
    r, w = _world(group)
    rank = r if rank is None else rank
    world = w if world is None else world
    lo, hi = shard_bounds(pts.shape[0], rank, world)
    return pts[lo:hi]


class _PeerGather:
    """Pending ragged all-gather made of grouped point-to-point transfers (see _gather_rows_into).  wait() completes them."""

    def __init__(self, works, keep):
        self.works, self.keep = list(works), keep          # `keep`: the send buffer must outlive an asynchronous transfer

    def wait(self):
        for w in self.works:
            w.wait()
        self.works, self.keep = [], None
        return True


def _gather_rows_into(out, x, counts, group, async_op=False):
    """all-gather of per-rank row blocks (dim-0 sizes `counts`, ragged allowed) into the pre-sized C-contiguous `out`
    ([sum(counts), ...]).  Returns the pending works (objects with .wait()).

    Equal shards: one all_gather_into_tensor straight into `out` (no padding, no staging, no torch.cat).  Ragged shards
    (round 5): every rank copies its own rows into place and exchanges the others as ONE group of point-to-point transfers
    (batch_isend_irecv: P-1 sends of its block, P-1 receives straight into the peers' places in `out`) -- exactly the bytes
    the result holds, no staging buffer, any counts (also [N, 0, ..., 0]), and on xGMI's full mesh every pair's block travels
    on its own link.  (Round 4 padded every block to the largest shard and gathered into a world * max(counts) staging tensor
    first: for counts far from equal that moved and held up to `world` times the field; rounds 2-3 queued P broadcasts.)"""
    rank, world = _world(group)
    x = x.contiguous()
    if len(set(counts)) == 1:
        w = dist.all_gather_into_tensor(out, x, group=group, async_op=async_op)
        return [w] if async_op else []
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    if counts[rank]:
        out[offs[rank]:offs[rank + 1]].copy_(x)
    peer = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    ops = []
    for r in range(world):
        if r == rank:
            continue
        if counts[rank]:
            ops.append(dist.P2POp(dist.isend, x, peer(r), group))
        if counts[r]:
            ops.append(dist.P2POp(dist.irecv, out[offs[r]:offs[r + 1]], peer(r), group))
    pg = _PeerGather(dist.batch_isend_irecv(ops) if ops else [], x)
    if async_op:
        return [pg]
    pg.wait()
    return []


def _gather_rows(t, counts, group, async_op=False):
    """all-gather along dim 0 -> (full tensor, pending works)."""
    as_bool = t.dtype == torch.bool
    x = t.view(torch.uint8) if as_bool else t
    out = x.new_empty((sum(counts),) + tuple(x.shape[1:]))
    works = _gather_rows_into(out, x, counts, group, async_op)
    return (out.view(torch.bool) if as_bool else out), works


def gather_bytes(local_out, keys, counts):
    """Bytes one rank RECEIVES when `keys` of a sharded field are all-gathered (the xGMI cost of reassembly)."""
    total, own = sum(counts), None
    n_local = local_out["dist"].shape[0]
    recv = 0
    for k in keys:
        t = local_out[k]
        row = t.element_size() * (t.numel() // max(n_local, 1))          # bytes per query point of this output
        recv += (total - n_local) * row
    return recv


def all_gather_field(local_out, keys=None, counts=None, group=None, async_op=False):
    """Reassembles per-rank eval outputs into the full field on every rank.

    local_out: dict from Fusion.eval on this rank's shard.  keys: which entries to gather
    (default all).  '<k>_inter' entries ([V,n,C]) are gathered along their point axis, view by view, straight
    into the [V,N,C] result (each view's rows are one contiguous block of it).
    counts: per-rank shard sizes if already known (saves a tiny all-gather).
    async_op=True returns (field, works): the collectives run on RCCL's stream while the caller keeps launching
    (e.g. the next batch's query); the field -- and `local_out`, which the caller must keep alive -- may only be
    touched after `for w in works: w.wait()`.  Ragged shards are supported in both forms.
    """
    rank, world = _world(group)
    if world == 1:
        full = dict(local_out) if keys is None else {k: local_out[k] for k in keys}
        return (full, []) if async_op else full
    keys = list(local_out.keys()) if keys is None else list(keys)
    if counts is None:
        n_local = local_out["dist"].shape[0]
        c = torch.tensor([n_local], dtype=torch.int64, device=local_out["dist"].device)
        allc = torch.empty(world, dtype=torch.int64, device=c.device)
        dist.all_gather_into_tensor(allc, c, group=group)
        counts = [int(v) for v in allc.tolist()]
    full, works = {}, []
    for k in keys:
        t = local_out[k]
        if k.endswith("_inter"):
            out = t.new_empty((t.shape[0], sum(counts)) + tuple(t.shape[2:]))
            for v in range(t.shape[0]):
                works += _gather_rows_into(out[v], t[v], counts, group, async_op)
            full[k] = out
        else:
            full[k], w = _gather_rows(t, counts, group, async_op)
            works += w
    return (full, works) if async_op else full


def sharded_eval(fusion, pts, return_names=("dino_feats", "mask"), gather_keys=None, group=None, evaluator=None):
    """Evaluates the FULL batch `pts` (same tensor on every rank) cooperatively.

    Every rank queries its contiguous block with the HIP kernel (fusion.batch_eval) and the
    requested keys are all-gathered; keys not gathered are returned as this rank's shard under
    '<key>_local' together with 'local_range'.  `evaluator` replaces fusion.batch_eval in the
    CPU plumbing tests (gloo), where no GPU exists.
    """
    rank, world = _world(group)
    n = pts.shape[0]
    lo, hi = shard_bounds(n, rank, world)
    run = evaluator if evaluator is not None else (lambda p, names: fusion.batch_eval(p, return_names=list(names)))
    local = run(pts[lo:hi], return_names)
    counts = [shard_bounds(n, r, world)[1] - shard_bounds(n, r, world)[0] for r in range(world)]
    keys = list(local.keys()) if gather_keys is None else list(gather_keys)
    out = all_gather_field(local, keys=keys, counts=counts, group=group)
    for k, v in local.items():
        if k not in out:
            out[k + "_local"] = v
    out["local_range"] = (lo, hi)
    return out


def broadcast_observation(fusion, src=0, group=None, keys=None):
    """Replicates rank `src`'s curr_obs_torch tensors (maps, depth, K, pose) to every rank: the
    once-per-update setup cost of the sharded mode (dense C4 maps: 30 GB per rank -- pass `keys` to re-send only
    what the update changed, e.g. ('depth', 'mask') while the feature maps of a static scene stay).  Returns the
    bytes this rank received.  The in-place overwrite does not move the tensors' version counters, so the shim's cached
    "maps are finite" verdicts and the projected maps of add_projection's heads are dropped here by hand: the next query
    re-checks and re-projects the new data."""
    rank, world = _world(group)
    if world == 1:
        return 0
    received = 0
    for k in sorted(fusion.curr_obs_torch.keys()):
        t = fusion.curr_obs_torch[k]
        if isinstance(t, torch.Tensor) and (keys is None or k in keys):
            dist.broadcast(t, src=src, group=group)
            if rank != src:
                received += t.numel() * t.element_size()
    if hasattr(fusion, "_finite_cache"):
        fusion._finite_cache.clear()
    if hasattr(fusion, "_projected"):
        fusion._projected.clear()
    return received


class _HipSoftmaxKernels:
    """The three device steps of the row-sharded softmax (include/d3fields_hip.h); column records travel as
    raw [B2,16] uint8 tensors (d3f_col_stat: float max, float sum, int64 argmax)."""

    @staticmethod
    def local(src, tgt, scale, dist_code, row_offset):
        dev = src.device
        B1, C = src.shape
        B2 = tgt.shape[0]
        out = torch.empty((B1, B2), dtype=torch.float32, device=dev)
        stats = torch.empty((B2, 16), dtype=torch.uint8, device=dev)
        with _lib.on(dev) as q:
            ws, ws_bytes = q.workspace("d3f_softmax_workspace_bytes", B1, B2) if B1 > 0 else (None, 0)
            q.d3f_pairwise_softmax_local(src, tgt, B1, B2, C, float(scale), dist_code, int(row_offset), out, stats, ws, ws_bytes)
        return out, stats

    @staticmethod
    def merge(parts):
        dev = parts.device
        P, B2 = parts.shape[0], parts.shape[1]
        merged = torch.empty((B2, 16), dtype=torch.uint8, device=dev)
        am = torch.empty(B2, dtype=torch.int64, device=dev)
        with _lib.on(dev) as q:
            q.d3f_softmax_merge(parts, P, B2, merged, am)
        return merged, am

    @staticmethod
    def apply(out, scale, merged):
        with _lib.on(out.device) as q:
            q.d3f_softmax_apply(out, out.shape[0], out.shape[1], float(scale), merged)
        return out


class _HipTopkKernels:
    """Device steps of the row-sharded k-NN lookup: local k smallest per column, merge of the ranks' lists."""

    @staticmethod
    def local_topk(dist_local, k):
        dev = dist_local.device
        rows, cols = dist_local.shape
        idx = torch.empty((k, cols), dtype=torch.int64, device=dev)
        val = torch.empty((k, cols), dtype=torch.float32, device=dev)
        with _lib.on(dev) as q:
            ws, ws_bytes = q.workspace("d3f_pairwise_topk_workspace_bytes", rows, cols)
            q.d3f_topk_smallest(dist_local, rows, cols, k, idx, val, ws, ws_bytes)
        return idx, val

    @staticmethod
    def merge_topk(parts_idx, parts_val, k):
        dev = parts_idx.device
        P, _, cols = parts_idx.shape
        idx = torch.empty((k, cols), dtype=torch.int64, device=dev)
        val = torch.empty((k, cols), dtype=torch.float32, device=dev)
        with _lib.on(dev) as q:
            q.d3f_topk_merge(parts_idx, parts_val, P, k, cols, idx, val)
        return idx, val


def sharded_knn_descriptors(src_local, tgt_feats, k, scale=1.0, dist_type="l2", row_offset=None, group=None, kernels=None, topk=None):
    """corr_utils.knn_descriptors with the B1 source descriptors sharded over ranks (the multi-GPU form of the k-NN lookup,
    as sharded_similarity_multi is of nearest_descriptor).  Every rank selects the k nearest of ITS rows per target column
    on the raw distances, the ranks exchange those [k,B2] lists (k * 12 bytes per column) next to the softmax column
    records, and every rank merges them by (distance, global row).  Returns (similarity rows of this rank [B1_local,B2],
    index [k,B2] int64 GLOBAL rows (-1 where fewer than k rows exist), distance [k,B2] float32 of those rows).
    `kernels` / `topk` replace the HIP steps in the CPU plumbing tests (gloo)."""
    from .corr_utils import _dist_code
    if not 1 <= int(k) <= 8:
        raise ValueError("k must be in [1, 8]")
    k = int(k)
    code = _dist_code(dist_type)
    rank, world = _world(group)
    ks = kernels if kernels is not None else _HipSoftmaxKernels
    kt = topk if topk is not None else _HipTopkKernels
    assert src_local.dim() == 2 and tgt_feats.dim() == 2 and src_local.shape[1] == tgt_feats.shape[1]
    if kernels is None and not src_local.is_cuda:
        raise RuntimeError("src_local must be on the ROCm device; there is no CPU path")
    src_local = src_local.to(torch.float32).contiguous()
    tgt_feats = tgt_feats.to(device=src_local.device, dtype=torch.float32).contiguous()
    if row_offset is None:
        row_offset = 0
        if world > 1:
            c = torch.tensor([src_local.shape[0]], dtype=torch.int64, device=src_local.device)
            allc = torch.empty(world, dtype=torch.int64, device=c.device)
            dist.all_gather_into_tensor(allc, c, group=group)
            row_offset = int(allc[:rank].sum())
    out, stats = ks.local(src_local, tgt_feats, scale, code, row_offset)             # out: this rank's raw distances
    lidx, lval = kt.local_topk(out, k)
    lidx = torch.where(lidx >= 0, lidx + int(row_offset), lidx)                       # local rows -> global rows
    if world > 1:
        parts = stats.new_empty((world,) + tuple(stats.shape))
        dist.all_gather_into_tensor(parts.view(world * stats.shape[0], 16), stats, group=group)
        pidx = lidx.new_empty((world,) + tuple(lidx.shape))
        pval = lval.new_empty((world,) + tuple(lval.shape))
        dist.all_gather_into_tensor(pidx.view(world * k, -1), lidx, group=group)
        dist.all_gather_into_tensor(pval.view(world * k, -1), lval, group=group)
    else:
        parts, pidx, pval = stats.unsqueeze(0), lidx.unsqueeze(0), lval.unsqueeze(0)
    merged, _ = ks.merge(parts)
    gidx, gval = kt.merge_topk(pidx.contiguous(), pval.contiguous(), k)
    return ks.apply(out, scale, merged), gidx, gval


def sharded_similarity_multi(src_local, tgt_feats, scale, dist_type="l2", row_offset=None, group=None, kernels=None):
    """compute_similarity_tensor_multi (utils/corr_utils.py:63-106) with the B1 source descriptors sharded over ranks.

    src_local [B1_local,C] is THIS rank's contiguous block of rows (e.g. the features Fusion.eval returned for its
    shard of keypoints), tgt_feats [B2,C] is replicated.  softmax(dim=0) couples all rows, so the ranks exchange one
    16-byte record per target column (max, sum-exp, first argmax) -- a single all-gather of 16*B2 bytes -- and
    normalise locally.  Returns (similarity rows of this rank [B1_local,B2], argmax [B2] as GLOBAL row indices).
    row_offset: global index of this rank's first row (default: exclusive sum of the ranks' row counts).
    `kernels` replaces the HIP steps in the CPU plumbing tests (gloo)."""
    from .corr_utils import _dist_code
    code = _dist_code(dist_type)
    rank, world = _world(group)
    k = kernels if kernels is not None else _HipSoftmaxKernels
    assert src_local.dim() == 2 and tgt_feats.dim() == 2 and src_local.shape[1] == tgt_feats.shape[1]
    if kernels is None and not src_local.is_cuda:
        raise RuntimeError("src_local must be on the ROCm device; there is no CPU path")
    src_local = src_local.to(torch.float32).contiguous()
    tgt_feats = tgt_feats.to(device=src_local.device, dtype=torch.float32).contiguous()
    if row_offset is None:
        row_offset = 0
        if world > 1:
            c = torch.tensor([src_local.shape[0]], dtype=torch.int64, device=src_local.device)
            allc = torch.empty(world, dtype=torch.int64, device=c.device)
            dist.all_gather_into_tensor(allc, c, group=group)
            row_offset = int(allc[:rank].sum())
    out, stats = k.local(src_local, tgt_feats, scale, code, row_offset)
    if world > 1:
        parts = stats.new_empty((world,) + tuple(stats.shape))
        dist.all_gather_into_tensor(parts.view(world * stats.shape[0], 16), stats, group=group)
    else:
        parts = stats.unsqueeze(0)
    merged, am = k.merge(parts)
    return k.apply(out, scale, merged), am
