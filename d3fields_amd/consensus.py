"""Which pose explains these matches?  Consensus poses from M model points with k candidate places each (d3f_pose_consensus_* / d3f_pose_refit,
csrc/consensus_kernels.hip): every minimal sample of three (model point, candidate) pairs implies a rigid motion, the
motion is scored by how many model points find one of their candidates where it puts them, and the few best mutually distinct motions come
back as starts for BakedField.align.  There is no CPU path."""
import functools
import math
import operator

import numpy as np
import torch

from . import _lib


@functools.lru_cache(maxsize=None)
def all_triplets(M):
    """int32 [C(M, 3), 3]: every i < j < l below M, in lexicographic order (read-only: it is cached)"""
    i, j, l = np.meshgrid(np.arange(M), np.arange(M), np.arange(M), indexing="ij")
    keep = (i < j) & (j < l)
    out = np.stack([i[keep], j[keep], l[keep]], axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


def _tensor(who, what, t):
    """a tensor whose shape has been checked: on the GPU, float32, detached and contiguous"""
    if not t.is_cuda:
        raise RuntimeError("%s: %s must be on the GPU; there is no CPU path" % (who, what))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (who, what, t.dtype))
    return t.detach().contiguous()


def _int(who, what, v, lo, hi):
    try:
        i = None if isinstance(v, bool) else operator.index(v)
    except TypeError:
        i = None
    if i is None or not lo <= i <= hi:
        raise ValueError("%s: %s must be an integer in %d..%d, got %r" % (who, what, lo, hi, v))
    return i


def _length(who, what, v, positive=False):
    f = float(v)
    if not (math.isfinite(f) and (f > 0.0 if positive else f >= 0.0)):
        raise ValueError("%s: %s must be finite and %s 0, got %r" % (who, what, ">" if positive else ">=", v))
    return f


def _subset(M, n, seed):
    t = all_triplets(M)
    return np.ascontiguousarray(t[np.sort(np.random.default_rng(seed).choice(len(t), n, replace=False))])


@functools.lru_cache(maxsize=64)
def _cached_tables(M, n, seed, device):
    """(host table, its copy on `device`) of all C(M, 3) triplets (n None) or of the seeded subset of n: uploaded once per key, so that a
    call in the steady state uploads nothing -- a copy from pageable host memory makes the host wait for the stream"""
    host = np.array(all_triplets(M) if n is None else _subset(M, n, seed), dtype=np.int32)
    host.setflags(write=False)
    return host, torch.from_numpy(host.copy()).to(device)


def _triplet_tables(who, M, k, triplets, max_triplets, seed, dev):
    """-> (int32 [n_trip, 3] on the host, the same on dev)"""
    if triplets is not None:
        if max_triplets is not None:
            raise ValueError("%s: give triplets or max_triplets, not both" % who)
        t = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
        if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
            raise ValueError("%s: triplets must be an integer table [n_trip, 3], got %s %s" % (who, t.dtype, list(t.shape)))
        if t.size and not ((t[:, 0] >= 0) & (t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2]) & (t[:, 2] < M)).all():
            raise ValueError("%s: every triplet must be 0 <= i < j < l < M = %d" % (who, M))
        host = np.array(t, dtype=np.int32)
        both = host, torch.from_numpy(host).to(dev)             # (an explicit table is uploaded by every call: the host waits for the stream)
    else:
        n = None
        if max_triplets is not None:
            n = _int(who, "max_triplets", max_triplets, 0, 2 ** 31 - 1)
            n = None if n >= len(all_triplets(M)) else n
        if n is None or (isinstance(seed, int) and not isinstance(seed, bool)):
            both = _cached_tables(M, n, None if n is None else seed, dev)
        else:                                                   # (a seed that is no plain integer, None say, draws anew: nothing to cache)
            host = _subset(M, n, seed)
            both = host, torch.from_numpy(host).to(dev)
    if len(both[0]) * k ** 3 > 2 ** 31 - 1:
        raise ValueError("%s: %d triplets times k^3 = %d is more than 2^31 - 1 hypotheses; give max_triplets" % (who, len(both[0]), k ** 3))
    return both


def consensus_poses(model_pts, candidates, tau, n_poses=8, min_inliers=4, shared=3, side_tol=None, min_side=None, min_sin=0.2, triplets=None,
                    max_triplets=None, seed=0, max_survivors=65536, refit=True):
    """The n_poses best mutually distinct rigid motions x = p @ rot + trans that put the model points onto their candidates.

    model_pts     float32 [M, 3] on the GPU, 3 <= M <= 64
    candidates    float32 [M, k, 3] on the same device, 1 <= k <= 8: k candidate places per model point; a row with a NaN coordinate is
                  padding (BakedField.locate pads its 'refined' with NaN rows)
    tau           the inlier radius, a world length > 0;  side_tol (None: 2 tau), min_side (None: 4 tau), min_sin  the gate on a sample:
                  its three sides at least min_side long, each observed side within side_tol of its model side, the sine at the first
                  vertex at least min_sin on both triangles
    min_inliers   3..64: a hypothesis survives with at least this many assigned points;  max_survivors  only the best this many survive (at most 65536)
    shared        1..64: picking a pose kills every survivor that shares at least this many identical (point, candidate) assignments
    triplets      None: all C(M, 3); or an explicit integer table [n_trip, 3] with i < j < l;  max_triplets  a subset of all, drawn on the
                  host by numpy.random.default_rng(seed) and sorted, so that a call is reproducible
    refit         also fit the least-squares motion over each pose's assigned pairs (Horn's closed form, float64)
    A hypothesis is h = (trip * k + a) * k * k + b * k + c.  The arithmetic contract is in include/d3fields_hip.h; results are the same
    bytes on every run.
    -> {'rot': float32 [H, 3, 3], 'trans': float32 [H, 3] in rigid.rigid_transform's row-vector convention (the kernels' R transposed),
        'inliers': int32 [H], 'assignment': int32 [H, M] (-1: none), 'hypothesis': int64 [H], 'triplet': int32 [H, 3], 'digits': int32 [H, 3],
        'count': int32 [] how many of the H = n_poses ranks are real -- the others are padded with NaN and -1 --, 'n_gated': int32 [],
        'n_survivors': int32 []; with refit 'refit_rot', 'refit_trans', 'rmse' float64 [H], 'refit_inliers' int32 [H]}.
    Host synchronisation: none in the steady state.  The device copy of the triplet table is cached per (M, max_triplets, seed, device), so
    only the FIRST call with a key uploads it, and that upload (from pageable memory) makes the host wait for the stream; an explicit
    `triplets=` is uploaded by every call (a tensor is read back first), with the same wait.  Everything else is launches on the current
    stream.  No autograd: outputs never require grad."""
    who = "consensus_poses"
    if not isinstance(model_pts, torch.Tensor) or model_pts.dim() != 2 or model_pts.shape[1] != 3:
        raise ValueError("%s: model_pts must be a tensor of shape [M, 3], got %s" % (who, list(getattr(model_pts, "shape", ())) or type(model_pts).__name__))
    M = int(model_pts.shape[0])
    if not 3 <= M <= _lib.CONSENSUS_MAX_POINTS:
        raise ValueError("%s: M = %d model points, must be 3..%d" % (who, M, _lib.CONSENSUS_MAX_POINTS))
    if not isinstance(candidates, torch.Tensor) or candidates.dim() != 3 or candidates.shape[0] != M or candidates.shape[2] != 3:
        raise ValueError("%s: candidates must be a tensor of shape [M = %d, k, 3], got %s" % (who, M, list(getattr(candidates, "shape", ())) or type(candidates).__name__))
    k = int(candidates.shape[1])
    if not 1 <= k <= _lib.CONSENSUS_MAX_CANDIDATES:
        raise ValueError("%s: k = %d candidates per point, must be 1..%d" % (who, k, _lib.CONSENSUS_MAX_CANDIDATES))
    p = _tensor(who, "model_pts", model_pts)
    c = _tensor(who, "candidates", candidates)
    dev = p.device
    if c.device != dev:
        raise RuntimeError("%s: candidates are on %s, model_pts on %s" % (who, c.device, dev))
    tau = _length(who, "tau", tau, positive=True)
    side_tol = 2.0 * tau if side_tol is None else _length(who, "side_tol", side_tol)
    min_side = 4.0 * tau if min_side is None else _length(who, "min_side", min_side)
    min_sin = _length(who, "min_sin", min_sin)
    if min_sin > 1.0:
        raise ValueError("%s: min_sin must be in [0, 1], got %r" % (who, min_sin))
    H = _int(who, "n_poses", n_poses, 1, 64)
    min_inliers = _int(who, "min_inliers", min_inliers, 3, 64)
    shared = _int(who, "shared", shared, 1, 64)
    max_survivors = _int(who, "max_survivors", max_survivors, 1, _lib.CONSENSUS_MAX_SURVIVORS)
    table, trip_dev = _triplet_tables(who, M, k, triplets, max_triplets, seed, dev)
    n_trip = len(table)
    T = n_trip * k ** 3
    tau2 = float(np.float32(tau) * np.float32(tau))
    if not tau2 > 0.0:
        raise ValueError("%s: tau = %r squares to zero in float32" % (who, tau))

    if n_trip > 0:                                  # (the select kernel writes every rank, the ones that do not exist as -1 / NaN)
        hyp, inl = torch.empty(H, dtype=torch.int32, device=dev), torch.empty(H, dtype=torch.int32, device=dev)
        asg = torch.empty((H, _lib.CONSENSUS_MAX_POINTS), dtype=torch.int8, device=dev)
        pose = torch.empty((H, 12), dtype=torch.float32, device=dev)
    else:
        hyp = torch.full((H,), -1, dtype=torch.int32, device=dev)
        inl = torch.full((H,), -1, dtype=torch.int32, device=dev)
        asg = torch.full((H, _lib.CONSENSUS_MAX_POINTS), -1, dtype=torch.int8, device=dev)
        pose = torch.full((H, 12), float("nan"), dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev) if n_trip > 0 else torch.zeros(4, dtype=torch.int32, device=dev)      # (select writes all four)
    terms = (tau2, side_tol, min_side, min_sin)
    with _lib.on(dev) as q:
        if n_trip > 0:
            ws, ws_bytes = q.workspace("d3f_pose_consensus_workspace_bytes", M, k, n_trip, max_survivors)
            count = torch.empty(T, dtype=torch.uint8, device=dev)
            q.d3f_pose_consensus_score(p, c, M, k, trip_dev, table.ctypes.data, n_trip, *terms, count, None, None, ws, ws_bytes)
            q.d3f_pose_consensus_select(p, c, M, k, trip_dev, n_trip, *terms, count, min_inliers, shared, max_survivors, H, hyp, inl, asg, pose, stats, ws,
                                        ws_bytes)
        out = _result(hyp, inl, asg, pose, stats, trip_dev, M, k)
        if refit:
            rpose = torch.empty((H, 12), dtype=torch.float32, device=dev)          # (one wave per rank writes all three, NaN / -1 without three pairs)
            rmse = torch.empty(H, dtype=torch.float64, device=dev)
            rinl = torch.empty(H, dtype=torch.int32, device=dev)
            q.d3f_pose_refit(p, c, M, k, asg, H, tau2, rpose, rmse, rinl)
            out.update({"refit_rot": rpose[:, :9].reshape(H, 3, 3).transpose(1, 2).contiguous(), "refit_trans": rpose[:, 9:].contiguous(), "rmse": rmse,
                        "refit_inliers": rinl})
    return out


def _result(hyp, inl, asg, pose, stats, trip_dev, M, k):
    H = hyp.shape[0]
    real = hyp >= 0
    h = hyp.to(torch.int64)
    hc = torch.clamp(h, min=0)
    rem = hc % (k ** 3)
    digits = torch.stack((rem // (k * k), (rem // k) % k, rem % k), dim=1).to(torch.int32)
    if trip_dev.shape[0] > 0:
        triplet = trip_dev[hc // (k ** 3)]
    else:
        triplet = torch.zeros((H, 3), dtype=torch.int32, device=hyp.device)
    minus = torch.full_like(digits, -1)
    return {"rot": pose[:, :9].reshape(H, 3, 3).transpose(1, 2).contiguous(), "trans": pose[:, 9:].contiguous(), "inliers": inl,
            "assignment": asg[:, :M].to(torch.int32), "hypothesis": h, "triplet": torch.where(real[:, None], triplet, minus),
            "digits": torch.where(real[:, None], digits, minus), "count": stats[0].clone(), "n_gated": stats[1].clone(), "n_survivors": stats[2].clone()}
