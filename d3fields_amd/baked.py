"""`BakedField` -- bake once, look up many times.

`Fusion.bake(boundaries, step)` runs one grid query (`eval_grid`) and keeps its volume; `BakedField.eval(pts)` then reads that
volume at arbitrary points by trilinear interpolation (d3f_volume_sample, csrc/volume_kernels.hip): eight corner rows of one
array per point, no camera arithmetic, and a closed-form gradient w.r.t. the points (d3f_volume_sample_backward).  The lookup
interpolates the FUSED field -- it does not re-fuse -- so off the lattice it is not `Fusion.eval`.

`BakedField.raycast(origins, dirs)` and `BakedField.render(K, pose, H, W)` march rays through `dist` to the first surface they
meet (d3f_volume_raycast, csrc/raycast_kernels.hip) and read rows and normals at the hit points with the lookup above.

`BakedField.to_band(band)` / `Fusion.bake(..., band=)` keep channel rows only for the voxels a cell near the surface needs
(d3f_band_mark): `dist` / `valid` stay dense, one int32 slot per voxel names its row in a compacted `[M, C]`
array, and every lookup above goes through d3f_band_sample / d3f_band_sample_backward -- the same bits wherever the band covers the
point, the fill row and `in_band = False` elsewhere.

`BakedField.clearance()` answers "how far is this point from the nearest observed surface, and which surface is that": the exact
Euclidean distance transform of the occupied voxels (d3f_volume_edt, csrc/edt_kernels.hip) as a new field whose
`dist` is the distance to the nearest site and whose `nearest_voxel` names that site; `nearest_site(pts)` looks it up.

`BakedField.components()` labels the connected components of the occupied voxels, or of any site volume (d3f_volume_components,
csrc/ccl_kernels.hip): a `Components` with the label volume, each component's root, size and box; small
components are dropped by `min_voxels`, which `clearance(min_voxels=)` uses to keep floaters out of the transform.

`BakedField.pool(components)` pools the field per component (d3f_volume_pool, csrc/pool_kernels.hip): the mean
row of every baked set, hard votes over the channels of chosen sets, and each component's member count, centroid and covariance -- one
call for all components, the same bytes on every run.

`BakedField.parts(name, rule=, tau=)` answers "which part is this?": two neighbouring occupied voxels belong together only if their stored
rows agree (d3f_volume_links, csrc/parts_kernels.hip; d3f_volume_components_linked) -- a `Components` in which touching
objects with different descriptors are separate; `links()` gives the link volume alone and `components(links=)` labels over any such volume.

`BakedField.flow(other, name, radius_voxels=)` answers "how did it move?": for every occupied voxel the voxel of a second field on the same
grid, within a window, whose stored row is closest (d3f_volume_flow, csrc/flow_kernels.hip) -- a `Flow` with the
target, the cost, a sub-voxel offset, world displacements and the forward-backward test `consistent(back)`.

`Flow.motions(parts, keep=)` answers "how did each part move?": one rigid motion per part from the flow's dense correspondences, by a
trim-and-refit loop on the device (d3f_part_motion, csrc/motion_kernels.hip) -- a `PartMotions` with a rotation, a
translation, an inlier count, an rmse and a verdict per part, and the residual and inlier volumes; the same bytes on every run.

`BakedField.warp(motions, owner)` answers "where is it now?": this field as it would look after every part has moved by its rigid motion
(d3f_volume_warp_select / d3f_volume_warp_rows, csrc/warp_kernels.hip) -- an ordinary field on the same grid, dense or
banded as this one, with the part each voxel came from; `owners(parts, margin_voxels=)` grows the part labels by a margin so that the free side
of a part's surface travels with it.

`BakedField.travel(goals, radius=)` answers "how do I get there, and how far is it along the way": the cost-to-go field of a goal set
through the free voxels (d3f_volume_geodesic_*, csrc/geodesic_kernels.hip) -- exact shortest lattice paths with
integer weights, as a new field whose `dist` is the travel distance and whose `next_voxel` names the voxel to step to; `path(starts)`
walks it (d3f_volume_follow).

`BakedField.straight(a, b)` answers "can I go straight?": the exact grid segment between two voxels against a free volume
(d3f_volume_segments, csrc/segment_kernels.hip) -- whether it is clear, how far it gets, what blocks it and, on a
clearance field, how narrow it gets on the way; `shortcut(paths)` keeps only the waypoints of a route that cannot be skipped
(d3f_path_shorten).

`BakedField.peaks(values)` answers "where are the optima?": exact, order-independent non-maximum suppression of K value columns through
the slot volume (d3f_volume_peaks, csrc/peaks_kernels.hip) and the k best survivors per column, with a sub-voxel
refinement; `locate(descriptors, name)` runs it on the descriptor distances of a set: where in this observation are these descriptors?

`BakedField.align(points, name, targets)` answers "where did it go?": the rigid motion that puts point sets with descriptors onto the field,
by damped Gauss-Newton on the device (d3f_volume_align_*, csrc/align_kernels.hip) -- a pose, a cost and a verdict per
instance; `normal_equations(points, rot, trans)` gives the 6 x 6 systems alone.

There is no CPU path: volumes and points live on the ROCm device.
"""
import ctypes
import math
import operator

import torch

from . import _lib

__all__ = ["BakedField", "Components", "Flow", "PartMotions"]

_RESERVED = ("dist", "valid_mask", "grid_shape")
_POOL_KEYS = ("count", "moments", "centroid", "covariance")     # output keys of pool, next to one name + '_votes' per voted set
_RAY_KEYS = ("t", "depth", "hit_mask", "points", "normal")      # output keys of raycast / render: a set of that name cannot be asked for there


def _rows_in_place(t):
    """can the library read a [nx, ny, nz, C] set where it lies?  channels adjacent, voxels one constant stride >= C apart in flat order"""
    nx, ny, nz, C = t.shape
    sv = t.stride(2)
    return t.stride(3) == 1 and sv >= C and t.stride(1) == nz * sv and t.stride(0) == ny * nz * sv


def _check_band(band, who):
    try:
        value = float(band)
    except (TypeError, ValueError):
        raise TypeError("%s: band must be a number (a world length), got %r" % (who, band))
    if not (value > 0.0 and math.isfinite(value)):
        raise ValueError("%s: band must be a finite length > 0, got %r" % (who, band))
    return value


def _check_band_names(names):
    if "in_band" in names:
        raise ValueError("a set named 'in_band' cannot live in a banded field: 'in_band' is an output key of its lookups")


class _BakedQueryFn(torch.autograd.Function):
    """BakedField.eval as an autograd node: forward = d3f_volume_sample, backward = d3f_volume_sample_backward (d3f_band_sample and
    d3f_band_sample_backward on a banded field, whose 'in_band' follows 'valid_mask')."""

    @staticmethod
    def forward(ctx, pts, field, names):
        pts_c = pts.detach().contiguous()
        out = field._sample(pts_c, names)
        ctx.field, ctx.names, ctx.pts = field, names, pts_c
        masks = tuple(out[k] for k in field._mask_keys())
        ctx.mark_non_differentiable(*masks)
        return (out["dist"],) + masks + tuple(out[k] for k in names)

    @staticmethod
    def backward(ctx, grad_dist, *rest):
        grad_sets = rest[len(ctx.field._mask_keys()):]
        return ctx.field.backward(ctx.pts, grad_dist, dict(zip(ctx.names, grad_sets))), None, None


def _check_points(pts, device, who):
    assert type(pts) == torch.Tensor
    assert len(pts.shape) == 2
    assert pts.shape[1] == 3
    if not pts.is_cuda or pts.device != device:
        raise RuntimeError("%s: pts must be on %s (where the volume lives); there is no CPU path" % (who, device))
    if pts.dtype != torch.float32:
        raise TypeError("%s: pts must be float32, got %s" % (who, pts.dtype))


def _voxel_of(pts, origin, step, grid_shape):
    """(inside bool [N], flat int64 [N]): the voxel each point falls into -- g = (p - origin) / step in float64, rounded half away from
    zero and clipped to the lattice; inside while every -0.5 <= g_a <= n_a - 0.5 (NaN compares false).  The one voxel rule of
    BakedField.nearest_site and Components.label_at."""
    n = torch.tensor(tuple(grid_shape), dtype=torch.float64, device=pts.device)
    g = (pts.detach().double() - torch.tensor(origin, dtype=torch.float64, device=pts.device)) / step
    inside = ((g >= -0.5) & (g <= n - 0.5)).all(dim=1)
    r = torch.sign(g) * torch.floor(torch.abs(g) + 0.5)
    i = torch.minimum(torch.clamp(torch.nan_to_num(r, nan=0.0), min=0.0), n - 1).long()
    return inside, (i[:, 0] * grid_shape[1] + i[:, 1]) * grid_shape[2] + i[:, 2]


class Components:
    """The connected components of a site volume (BakedField.components).  Tensors only, on the field's device.

    labels      int32 [nx, ny, nz]: 1..count for the voxels of a kept component, 0 for a non-site or a dropped component
    count       K, the number of kept components (size >= min_voxels), numbered in ascending order of root; found: all components
    roots       int32 [K]: the smallest flat index (x*ny + y)*nz + z of each;  sizes int32 [K]: its voxel count
    box_lo, box_hi   int32 [K, 3]: the inclusive min and max of x, y, z
    sites       bool [nx, ny, nz]: the volume that was labelled;  connectivity (6, 18 or 26) and min_voxels as used
    origin, step, grid_shape   of the field it came from (label_at, boxes_world); no reference to the field itself"""

    def __init__(self, origin, step, labels, count, found, stats, sites, connectivity, min_voxels):
        self.origin, self.step, self.grid_shape = tuple(origin), float(step), torch.Size(labels.shape)
        self.labels, self.count, self.found = labels, int(count), int(found)
        self.roots, self.sizes = stats[:, 0].contiguous(), stats[:, 1].contiguous()
        self.box_lo, self.box_hi = stats[:, 2:5].contiguous(), stats[:, 5:8].contiguous()
        self.sites, self.connectivity, self.min_voxels = sites, int(connectivity), int(min_voxels)

    def mask(self, ids=None):
        """bool [nx, ny, nz]: the voxels of the components with these label ids (an int, a sequence or a tensor); None: every kept one"""
        if ids is None:
            return self.labels > 0
        ids = torch.as_tensor(ids, device=self.labels.device).reshape(-1).long()
        if ids.numel() and (int(ids.min()) < 1 or int(ids.max()) > self.count):
            raise ValueError("Components.mask: label ids must lie in 1..%d" % self.count)
        lut = torch.zeros(self.count + 1, dtype=torch.bool, device=self.labels.device)
        lut[ids] = True
        return lut[self.labels.long()]

    def largest(self, k=1):
        """int64 [min(k, count)]: label ids by descending size, the smaller id first among equal sizes"""
        k = int(k)
        if k < 0:
            raise ValueError("Components.largest: k must be >= 0, got %d" % k)
        order = torch.sort(self.sizes.long(), descending=True, stable=True).indices      # ids ascend already: stable keeps them so at ties
        return order[:k] + 1

    def boxes_world(self):
        """float32 [K, 2, 3]: lower and upper corner of each box in world coordinates, the outer faces of the voxels' cubes"""
        o = torch.tensor(self.origin, dtype=torch.float32, device=self.labels.device)
        h = torch.tensor(self.step, dtype=torch.float32, device=self.labels.device)
        lo = o + (self.box_lo.to(torch.float32) - 0.5) * h
        hi = o + (self.box_hi.to(torch.float32) + 0.5) * h
        return torch.stack((lo, hi), dim=1)

    def label_at(self, pts):
        """int32 [N]: the label of the voxel each point falls into, by the rounding and inside rule of BakedField.nearest_site; 0 for a
        point outside, a NaN coordinate, a non-site or a dropped component.  Plain torch indexing: not a hot path."""
        _check_points(pts, self.labels.device, "Components.label_at")
        inside, flat = _voxel_of(pts, self.origin, self.step, self.grid_shape)
        return torch.where(inside, self.labels.view(-1)[flat], torch.zeros_like(flat, dtype=torch.int32))


def _voxel_coords(flat, grid_shape):
    """int64 [..., 3]: (x, y, z) of flat voxel indices"""
    ny, nz = grid_shape[1], grid_shape[2]
    flat = flat.long()
    return torch.stack((flat // (ny * nz), (flat // nz) % ny, flat % nz), dim=-1)


class Flow:
    """Dense descriptor flow from one baked field to another on the same grid (BakedField.flow).  Tensors only, on the fields' device.

    target        int32 [nx, ny, nz]: the flat index (x*ny + y)*nz + z of the voxel of the other field whose row is closest, -1: unmatched
    cost          float32 [nx, ny, nz]: the squared L2 distance of the two rows (the float32 chain of d3f_volume_flow), +Inf where unmatched
    matched       bool [nx, ny, nz]: target >= 0
    voxel_offset  int32 [nx, ny, nz, 3]: the target's (x, y, z) minus the voxel's, 0 where unmatched
    axis_cost     float32 [nx, ny, nz, 6] or None (refine=False): the costs of the target's neighbours x-, x+, y-, y+, z-, z+, +Inf where one
                  takes no part
    offset        float64 [nx, ny, nz, 3] or None (refine=False): the sub-voxel correction in voxel units, per axis
                  0.5 (f- - f+) / (f- - 2 f0 + f+) clamped to [-0.5, 0.5]; 0 where a side is +Inf or the denominator is not > 0; NaN where unmatched
    coarse        the flows of the coarser levels, coarsest first, on the Flow that BakedField.flow_pyramid returns; None on every other flow
    origin, step, grid_shape   of the fields it came from; no reference to the fields themselves"""

    def __init__(self, origin, step, target, cost, axis_cost=None):
        self.origin, self.step, self.grid_shape = tuple(origin), float(step), torch.Size(target.shape)
        self.target, self.cost, self.axis_cost = target, cost, axis_cost
        self.coarse = None
        self.matched = target >= 0
        n = target.numel()
        own = _voxel_coords(torch.arange(n, device=target.device).view(self.grid_shape), self.grid_shape)
        to = _voxel_coords(torch.clamp(target, min=0), self.grid_shape)
        self.voxel_offset = torch.where(self.matched[..., None], to - own, torch.zeros_like(own)).to(torch.int32)
        self.offset = None
        if axis_cost is not None:
            inf = float("inf")
            f0 = cost.double()
            offs = []
            for a in range(3):
                fm, fp = axis_cost[..., 2 * a].double(), axis_cost[..., 2 * a + 1].double()
                den = fm - 2.0 * f0 + fp
                off = torch.clamp(0.5 * (fm - fp) / den, -0.5, 0.5)
                offs.append(torch.where((fm < inf) & (fp < inf) & (den > 0), off, torch.zeros_like(off)))
            out = torch.stack(offs, dim=-1)
            self.offset = torch.where(self.matched[..., None], out, torch.full_like(out, float("nan")))

    def displacement(self, refined=True):
        """float64 [nx, ny, nz, 3]: the world vector from each voxel to its match, (voxel_offset [+ offset]) * step; NaN where unmatched"""
        d = self.voxel_offset.double()
        if refined:
            if self.offset is None:
                raise ValueError("Flow.displacement: this flow was computed with refine=False; pass refined=False")
            return (d + self.offset) * self.step
        return torch.where(self.matched[..., None], d * self.step, torch.full_like(d, float("nan")))

    def seed(self, grid_shape, refined=True):
        """The prediction this flow makes for the next FINER grid (BakedField.coarsen halves a grid; this goes the other way) -> int32
        [nx, ny, nz, 3] in fine voxels, the `seed` of BakedField.flow on that grid.  Fine voxel (x, y, z) takes coarse voxel (x >> 1, y >> 1,
        z >> 1): where that voxel is matched the seed is 2 * voxel_offset, or with refined and an `offset` round(2 * (voxel_offset +
        offset)) (float64, round half to even); where it is unmatched the seed is 0.  grid_shape must halve to this flow's grid
        ((n + 1) // 2 per axis).  Torch indexing only, no kernel."""
        try:
            fine = tuple(int(e) for e in grid_shape)
        except (TypeError, ValueError):
            raise TypeError("Flow.seed: grid_shape must be three integers, got %r" % (grid_shape,))
        if len(fine) != 3 or tuple((e + 1) // 2 for e in fine) != tuple(self.grid_shape) or min(fine) < 1:
            raise ValueError("Flow.seed: grid_shape %s does not halve to this flow's grid %s" % (fine, tuple(self.grid_shape)))
        dev = self.target.device
        ix, iy, iz = (torch.arange(e, device=dev) >> 1 for e in fine)
        if refined and self.offset is not None:
            whole = torch.round(2.0 * (self.voxel_offset.double() + self.offset))
            whole = torch.where(self.matched[..., None], whole, torch.zeros_like(whole)).to(torch.int32)
        else:
            whole = 2 * self.voxel_offset      # (0 where unmatched)
        return whole[ix[:, None, None], iy[None, :, None], iz[None, None, :]].contiguous()

    def consistent(self, back, tol_voxels=1):
        """The forward-backward test -> bool [nx, ny, nz]: a voxel passes when it is matched, `back` (the flow of the other field to this one)
        has a target at its target, and that voxel lies within Chebyshev distance tol_voxels of the voxel itself.  The ambiguity filter:
        a match that the way back does not confirm is a repeated or featureless descriptor.  Integer torch indexing, no kernel."""
        if not isinstance(back, Flow) or back.grid_shape != self.grid_shape:
            raise ValueError("Flow.consistent: back must be a Flow on the same grid %s" % (tuple(self.grid_shape),))
        if back.target.device != self.target.device:
            raise ValueError("Flow.consistent: back is on %s, this flow on %s" % (back.target.device, self.target.device))
        if isinstance(tol_voxels, bool) or not isinstance(tol_voxels, int) or tol_voxels < 0:
            raise ValueError("Flow.consistent: tol_voxels must be an integer >= 0, got %r" % (tol_voxels,))
        ret = back.target.view(-1)[torch.clamp(self.target, min=0).long()]
        own = _voxel_coords(torch.arange(self.target.numel(), device=self.target.device).view(self.grid_shape), self.grid_shape)
        near = ((_voxel_coords(torch.clamp(ret, min=0), self.grid_shape) - own).abs().amax(dim=-1) <= tol_voxels)
        return self.matched & (ret >= 0) & near

    def motions(self, parts, keep=None, tau_voxels=1.0, fits=3, min_pairs=8, refined=True, count=None):
        """How did each part move?  One rigid motion per part from this flow's matches, by a trim-and-refit loop (d3f_part_motion,
        csrc/motion_kernels.hip) -> PartMotions.

        parts       a Components on this flow's grid (components() / parts() of the field the flow starts from), or an int32 [nx, ny, nz] label
                    volume on this device together with count=K, as pool takes it.  With a Components the moments are taken about each part's
                    box_lo; with a label volume about voxel (0, 0, 0)
        keep        None, or a bool [nx, ny, nz] volume: only these voxels are pairs -- typically consistent(back)
        tau_voxels  the inlier radius in voxels: a pair is an inlier of a pose when its residual is <= tau_voxels
        fits        1..8: fit 0 takes every pair, fit f the inliers under the pose of fit f-1
        min_pairs   >= 3: a part with fewer pairs gets no pose (TOO_FEW); one that falls below it later keeps its last pose (THINNED)
        refined     the match is target + offset (the flow must have been computed with refine=True); False: the target voxel alone
        A pair is a voxel with a label in 1..K that `keep` passes and that has a target (and a finite offset).  Sums are float64 in a fixed
        order: the same bytes on every run.  One host read (the member capacity).  Not differentiable."""
        dev = self.target.device
        nx, ny, nz = self.grid_shape
        ref = None
        if isinstance(parts, Components):
            if count is not None:
                raise ValueError("motions: count comes with a label tensor; a Components knows its own")
            if tuple(parts.grid_shape) != tuple(self.grid_shape) or tuple(parts.origin) != self.origin or float(parts.step) != self.step:
                raise ValueError("motions: the parts are of a grid %s at %s step %g, the flow of %s at %s step %g" % (
                    tuple(parts.grid_shape), tuple(parts.origin), parts.step, tuple(self.grid_shape), self.origin, self.step))
            labels, K, ref = parts.labels, parts.count, parts.box_lo
        elif isinstance(parts, torch.Tensor):
            if count is None or isinstance(count, bool) or not isinstance(count, int) or count < 0:
                raise ValueError("motions: a label tensor needs count=K, an integer >= 0, got %r" % (count,))
            if parts.dtype != torch.int32 or tuple(parts.shape) != tuple(self.grid_shape):
                raise ValueError("motions: labels must be an int32 tensor of shape %s, got %s %s" % (tuple(self.grid_shape), parts.dtype, tuple(parts.shape)))
            labels, K = parts.detach(), count
        else:
            raise ValueError("motions: parts must be a Components or an int32 label tensor, got %r" % type(parts).__name__)
        if labels.device != dev:
            raise ValueError("motions: the labels are on %s, this flow on %s" % (labels.device, dev))
        if K > nx * ny * nz:
            raise ValueError("motions: count = %d exceeds the %d voxels" % (K, nx * ny * nz))
        if keep is not None:
            if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != tuple(self.grid_shape):
                raise ValueError("motions: keep must be a bool tensor of shape %s" % (tuple(self.grid_shape),))
            if keep.device != dev:
                raise ValueError("motions: keep is on %s, this flow on %s" % (keep.device, dev))
        if isinstance(tau_voxels, bool) or not isinstance(tau_voxels, (int, float)) or not (0.0 < float(tau_voxels) < math.inf):
            raise ValueError("motions: tau_voxels must be a finite number > 0, got %r" % (tau_voxels,))
        if isinstance(fits, bool) or not isinstance(fits, int) or not 1 <= fits <= _lib.MOTION_MAX_FITS:
            raise ValueError("motions: fits must be an integer in 1..%d, got %r" % (_lib.MOTION_MAX_FITS, fits))
        if isinstance(min_pairs, bool) or not isinstance(min_pairs, int) or min_pairs < 3:
            raise ValueError("motions: min_pairs must be an integer >= 3, got %r" % (min_pairs,))
        if refined and self.offset is None:
            raise ValueError("motions: this flow was computed with refine=False; pass refined=False")
        if not dev.type == "cuda":
            raise RuntimeError("motions: the flow must live on the ROCm device; there is no CPU path")
        labels = labels.contiguous()
        target = self.target.contiguous()
        offset = self.offset.contiguous() if refined else None
        keep8 = None if keep is None else keep.contiguous().view(torch.uint8)
        ref = None if ref is None else ref.to(torch.int32).contiguous()
        n = nx * ny * nz
        tau2 = float(tau_voxels) * float(tau_voxels)
        # the call writes every output: the capacity below counts a superset of the pairs, so the list always fits, and under the final poses
        # motion_fill_kernel puts NaN / 0 into the two volumes before the pairs' own values land there
        pose = torch.empty((K, _lib.MOTION_POSE_DOUBLES), dtype=torch.float64, device=dev)
        pairs, inliers = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
        done, status = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
        rmse = torch.empty(K, dtype=torch.float64, device=dev)
        if K == 0:                                                       # (no part: nothing is launched, the per-part outputs are empty and the volumes are filled here)
            res2 = torch.full((nx, ny, nz), math.nan, dtype=torch.float64, device=dev)
            inlier = torch.zeros((nx, ny, nz), dtype=torch.uint8, device=dev)
        else:
            res2 = torch.empty((nx, ny, nz), dtype=torch.float64, device=dev)
            inlier = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
            passes = (labels > 0) & (target >= 0)
            capacity = int((passes if keep is None else passes & keep).sum())
            members = torch.empty(1, dtype=torch.int64, device=dev)
            with _lib.on(dev) as q:
                ws, ws_bytes = q.workspace("d3f_part_motion_workspace_bytes", nx, ny, nz, K, capacity)
                q.d3f_part_motion(labels, K, nx, ny, nz, keep8, target, offset, ref, fits, tau2, min_pairs, capacity, members, pairs, pose, inliers, rmse, status,
                                  done, res2, inlier, None, ws, ws_bytes)
        return PartMotions(self.origin, self.step, pose, pairs, inliers, done, rmse, status, res2, inlier.view(torch.bool))


class PartMotions:
    """One rigid motion per part (Flow.motions).  Tensors only, on the flow's device; K parts, part k is row k - 1.

    pose        float64 [K, 15] in voxel index units, as d3f_part_motion writes it: R row-major, src, dst with q = R (p - src) + dst; src is
                the centroid of the part's final inlier sources, dst of their matches.  NaN for a part without a pose
    rot, trans  float64 [K, 3, 3], [K, 3] in world coordinates: x' = rot x + trans, trans = (origin + step dst) - rot (origin + step src)
    angle       float64 [K]: the rotation angle in radians;  shift float64 [K, 3]: the world displacement of the part's source centroid
    pairs, inliers, fits   int32 [K]: the pairs, the inliers under the final pose, the fits done
    rmse        float64 [K]: root mean square residual of the inliers in world units, NaN without inliers
    status      int32 [K]: OK (0), THINNED (1: the inliers fell below min_pairs, the pose of the last fit stays), TOO_FEW (2: no pose)
    residual    float64 [nx, ny, nz]: the distance between a pair's match and its part's motion of it, world units, NaN where there is no pair
                or no pose;  inlier bool [nx, ny, nz]
    Collinear or coincident pairs leave the rotation about their axis undetermined; the pose is then whatever the solver leaves, the same on
    every run."""
    OK, THINNED, TOO_FEW = _lib.MOTION_OK, _lib.MOTION_THINNED, _lib.MOTION_TOO_FEW

    def __init__(self, origin, step, pose, pairs, inliers, fits, rmse_voxels, status, residual2_voxels, inlier):
        self.origin, self.step = tuple(origin), float(step)
        self.pose, self.pairs, self.inliers, self.fits, self.status, self.inlier = pose, pairs, inliers, fits, status, inlier
        self.count = pose.shape[0]
        self.grid_shape = torch.Size(inlier.shape)
        o = torch.tensor(self.origin, dtype=torch.float64, device=pose.device)
        self.rot = pose[:, 0:9].reshape(-1, 3, 3)
        src, dst = o + self.step * pose[:, 9:12], o + self.step * pose[:, 12:15]
        self.trans = dst - (self.rot @ src[:, :, None])[:, :, 0]
        self.shift = dst - src
        r = self.rot
        skew = torch.stack((r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]), dim=-1)
        self.angle = torch.atan2((skew * skew).sum(dim=-1).sqrt(), r[:, 0, 0] + r[:, 1, 1] + r[:, 2, 2] - 1.0)
        self.rmse = rmse_voxels * self.step
        self.residual = residual2_voxels.sqrt() * self.step

    def apply(self, points, ids):
        """float64 [N, 3]: world points moved by the poses of the parts `ids` (one label id in 1..K, or an integer tensor [N] of them); NaN
        rows for a part without a pose"""
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("PartMotions.apply: points must be a float64 [N, 3] tensor")
        if points.device != self.pose.device:
            raise ValueError("PartMotions.apply: points are on %s, the motions on %s" % (points.device, self.pose.device))
        ids = torch.as_tensor(ids, device=points.device)
        if ids.dtype not in (torch.int32, torch.int64) or ids.dim() > 1 or (ids.dim() == 1 and ids.shape[0] != points.shape[0]):
            raise ValueError("PartMotions.apply: ids must be one integer or an integer tensor [N]")
        ids = ids.long().expand(points.shape[0]) if ids.dim() == 0 else ids.long()
        if ids.numel() and (int(ids.min()) < 1 or int(ids.max()) > self.count):
            raise ValueError("PartMotions.apply: ids must lie in 1..%d" % self.count)
        return (self.rot[ids - 1] @ points[:, :, None])[:, :, 0] + self.trans[ids - 1]

    def moved(self, min_shift=None, min_angle=None):
        """bool [K]: the parts that have a pose whose shift is at least min_shift (a world length) or whose angle is at least min_angle
        (radians); a bound that is None does not count"""
        if min_shift is None and min_angle is None:
            raise ValueError("PartMotions.moved: give min_shift, min_angle or both")
        out = torch.zeros(self.count, dtype=torch.bool, device=self.pose.device)
        if min_shift is not None:
            out |= self.shift.norm(dim=-1) >= float(min_shift)
        if min_angle is not None:
            out |= self.angle >= float(min_angle)
        return out & (self.status != self.TOO_FEW)


class BakedField:
    """A regular volume of the field and its trilinear lookup.

    origin      (x0, y0, z0): the centre of voxel (0, 0, 0)
    step        the lattice step h > 0
    grid_shape  torch.Size([nx, ny, nz]), every extent >= 2, z fastest
    dist        float32 [nx, ny, nz];  valid: bool [nx, ny, nz]
    names()     the channel sets, each float32 [nx, ny, nz, C] -- or float16 after half() / Fusion.bake(rows_dtype=torch.float16): rows_dtype(name),
                rows_bytes; the lookups read either storage and give the same bits, the methods with row loops of their own need float()

    A CLEARANCE field (clearance()) has no sets; its dist is the distance to the nearest site, and it has d2 int32 [nx, ny, nz] (squared
    voxel distance), nearest_voxel int32 (flat index of that site, -1: none), sites bool, and nearest_site(pts).  They are None elsewhere.

    A TRAVEL field (travel()) has no sets; its dist is the travel distance to the nearest goal along the cheapest lattice path through the
    free voxels, and it has cost int32 [nx, ny, nz] (INT32_MAX: unreached), next_voxel int32 (the flat index of the voxel to step to; the
    voxel itself at a goal, -1: unreached), free bool, and path(starts).  They are None elsewhere.
    straight(a, b) tests grid segments against a free volume (a travel field's own, radius= on a clearance field, free= anywhere);
    shortcut(paths) keeps only the waypoints of a travel field's route that cannot be skipped.
    peaks(values, ...) gives the spatially distinct local optima of value columns on any field; locate(descriptors, name, ...) the k best
    spatially distinct matches of reference descriptors among the rows of a set.

    A WARPED field (warp()) is an ordinary dense or banded field that also has source int32 [nx, ny, nz] (0: the voxel stayed, k: it came from
    part k, -1: nothing is known there), rows_known bool ([nx, ny, nz], or [M] on a banded field: False where the row is the fill row),
    part_box_from and part_box_to int32 [K, 2, 3] (the inclusive boxes of each part's owner voxels and of the voxels it won; an empty box is
    lo = INT32_MAX, hi = INT32_MIN).  They are None elsewhere.

    A MERGED field (merge()) is an ordinary dense or banded field that also has weight float32 [nx, ny, nz] (the summed weight of what was
    seen there, 0 where nothing was; the next merge() uses it as this field's weights), merged_from uint8 [nx, ny, nz] (MERGE_NONE 0: neither
    field knew the voxel, MERGE_KEEP 1: only the older one, MERGE_NEW 2: only the newer one, MERGE_BLEND 3: both, averaged, MERGE_RESET 4: both,
    too far apart, the newer one taken) and rows_known bool as a warped field has it.  weight and merged_from are None elsewhere.

    A COARSENED field (coarsen() / pyramid()) is an ordinary dense or banded field at twice the step that also has children uint8 [nx, ny, nz]
    (bit c = 4i + 2j + k: the finer voxel (2x + i, 2y + j, 2z + k) was valid with a dist that is no NaN) and rows_known as a merged field has it.
    children is None elsewhere.

    A BANDED field (to_band / Fusion.bake(band=)) holds each set as [M, C] rows of the stored voxels instead, and has
    band (the world length), slot int32 [nx, ny, nz] (-1: no row), cell_band uint8 [nx-1, ny-1, nz-1], band_voxels int32 [M]
    (ascending flat indices), band_points() and stored_fraction; its lookups add 'in_band'.  A dense field has band = None.

    It holds tensors only -- no reference to the Fusion that made it -- and stays valid after Fusion.update()."""
    MERGE_NONE, MERGE_KEEP, MERGE_NEW, MERGE_BLEND, MERGE_RESET = _lib.MERGE_NONE, _lib.MERGE_KEEP, _lib.MERGE_NEW, _lib.MERGE_BLEND, _lib.MERGE_RESET

    def __init__(self, origin, step, dist, valid, sets, fills, boundaries=None, axes=None):
        self.origin = tuple(float(o) for o in origin)
        self.step = float(step)
        self.grid_shape = torch.Size(dist.shape)
        self.dist, self.valid = dist, valid
        self._sets, self._fills = dict(sets), dict(fills)
        nx, ny, nz = self.grid_shape
        if boundaries is None:
            lo = [o - self.step / 2 for o in self.origin]
            boundaries = {"x_lower": lo[0], "x_upper": lo[0] + nx * self.step, "y_lower": lo[1], "y_upper": lo[1] + ny * self.step,
                          "z_lower": lo[2], "z_upper": lo[2] + nz * self.step}
        self.boundaries = dict(boundaries)
        self.device = dist.device
        self._lib = _lib.load()
        self._axes = axes                 # the three axis tensors of the grid that was baked (Fusion.bake), or None: origin + i * step
        self.band = self.slot = self.cell_band = self.band_voxels = None
        self.d2 = self.nearest_voxel = self.sites = None      # a clearance field's (clearance()); None on every other field
        self.cost = self.next_voxel = self.free = None         # a travel field's (travel()); None on every other field
        self.source = self.rows_known = self.part_box_from = self.part_box_to = None      # a warped field's (warp()); None on every other field
        self.weight = self.merged_from = None                  # a merged field's (merge(), which sets rows_known too); None on every other field
        self.children = None                                   # a coarsened field's (coarsen(), which sets rows_known too); None on every other field
        self.cell_valid = torch.empty((nx - 1, ny - 1, nz - 1), dtype=torch.uint8, device=self.device)
        with self._on() as q:
            q.d3f_volume_cell_valid(self._volume(), self.cell_valid)

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, origin, step, dist, valid=None, fills=None, rows_dtype=None, **named):
        """A field from volumes made elsewhere (a Gaussian-smoothed `dist`, ...): dist [nx,ny,nz] float32, valid None (every
        voxel) or bool / uint8 of the same shape, named sets [nx,ny,nz,C] float32, all on one ROCm device; fills: None or
        {name: [C] row a point outside the valid cells gets} (default zeros).  Tensors are used in place where they are
        contiguous float32 / bool.
        rows_dtype: None (every set becomes float32), torch.float16 or {name: dtype}: a set given as float16 whose dtype this names
        is KEPT as half rows (half()); such a set is also used in place as a view whose voxels are a constant stride >= C apart."""
        origin = tuple(float(o) for o in origin)
        if len(origin) != 3:
            raise ValueError("from_arrays: origin must hold three coordinates")
        if not float(step) > 0.0:
            raise ValueError("from_arrays: step must be > 0, got %r" % (step,))
        if not isinstance(dist, torch.Tensor) or dist.dim() != 3 or min(dist.shape) < 2:
            raise ValueError("from_arrays: dist must be a [nx,ny,nz] tensor with every extent >= 2")
        shape = tuple(dist.shape)
        if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != shape):
            raise ValueError("from_arrays: valid must have dist's shape %s" % (shape,))
        fills = dict(fills or {})
        for k, t in named.items():
            if k in _RESERVED:
                raise ValueError("from_arrays: %r is an output key of eval" % k)
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[:3]) != shape:
                raise ValueError("from_arrays: set %r must be [nx,ny,nz,C] with dist's grid %s, got %s" % (k, shape, tuple(getattr(t, "shape", ()))))
            if not 1 <= t.shape[3] <= _lib.VOLUME_MAX_CHANNELS:
                raise ValueError("from_arrays: set %r has %d channels, outside 1..%d" % (k, t.shape[3], _lib.VOLUME_MAX_CHANNELS))
            if fills.get(k) is not None and tuple(fills[k].shape) != (t.shape[3],):
                raise ValueError("from_arrays: fill of %r must be [%d]" % (k, t.shape[3]))
        unknown = [k for k in fills if k not in named]
        if unknown:
            raise ValueError("from_arrays: fills name unknown sets %s" % unknown)
        if len(named) > _lib.MAX_MAPS:
            raise ValueError("from_arrays: at most %d sets" % _lib.MAX_MAPS)
        if shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:
            raise ValueError("from_arrays: more than 2^31 - 1 voxels")
        if not dist.is_cuda:
            raise RuntimeError("BakedField: the volume must live on the ROCm device; there is no CPU path")
        dev = dist.device
        for k, t in list(named.items()) + [("valid", valid)] + [("fill of " + k, f) for k, f in fills.items()]:
            if t is not None and t.device != dev:
                raise RuntimeError("BakedField: %s is on %s, dist on %s" % (k, t.device, dev))
        dist = dist.detach().to(torch.float32).contiguous()
        valid = torch.ones(shape, dtype=torch.bool, device=dev) if valid is None else (valid.detach() != 0).contiguous()
        if rows_dtype is not None and not isinstance(rows_dtype, dict):
            rows_dtype = {k: rows_dtype for k in named}
        rows_dtype = dict(rows_dtype or {})
        for k, d in rows_dtype.items():
            if k not in named:
                raise ValueError("from_arrays: rows_dtype names the unknown set %r" % (k,))
            if d not in (torch.float32, torch.float16):
                raise ValueError("from_arrays: rows_dtype of %r must be torch.float32 or torch.float16, got %r" % (k, d))
        sets = {}
        for k, t in named.items():
            t = t.detach()
            if rows_dtype.get(k) == torch.float16:
                t = t.to(torch.float16)
                sets[k] = t if _rows_in_place(t) else t.contiguous()
            else:
                sets[k] = t.to(torch.float32).contiguous()
        fills = {k: (None if fills.get(k) is None else fills[k].detach().to(torch.float32).contiguous()) for k in sets}
        return cls(origin, step, dist, valid, sets, fills)

    @classmethod
    def from_fusion(cls, fusion, boundaries, step_size, return_names=(), band=None, rows_dtype=None, max_rows_bytes=1 << 30):
        """Fusion.bake: one eval_grid, its tensors viewed (not copied) as the volume; a projected name's fill row is -b, what
        Fusion.eval returns for an all-invalid point.  With a band: the distance-only grid pass, d3f_band_mark, and ONE
        batch_eval of the M stored voxel centres (the grid's own axis values) whose [M, C] outputs are the row arrays -- no
        [nx, ny, nz, C] array exists at any time.
        rows_dtype=torch.float16: the rows are stored as half (half()) and never all held in float32 -- the voxel centres (banded: the M
        stored ones; dense: all, after the distance-only grid pass, in flat-index order) are evaluated in chunks of at most max_rows_bytes
        of float32 rows and each chunk is converted into the preallocated half array: the bytes of bake(...).half()."""
        from .fusion import _grid_axes
        names = list(return_names)
        if rows_dtype not in (None, torch.float32, torch.float16):
            raise ValueError("bake: rows_dtype must be None, torch.float32 or torch.float16, got %r" % (rows_dtype,))
        as_half = rows_dtype == torch.float16
        if as_half and (isinstance(max_rows_bytes, bool) or not isinstance(max_rows_bytes, int) or max_rows_bytes < 1):
            raise ValueError("bake: max_rows_bytes must be a positive integer, got %r" % (max_rows_bytes,))
        if band is not None:
            band = _check_band(band, "bake")
            _check_band_names(names)
        with torch.no_grad():
            res = fusion.eval_grid(boundaries, step_size, return_names=names if band is None and not as_half else [])
        nx, ny, nz = res["grid_shape"]
        if min(nx, ny, nz) < 2:
            raise ValueError("bake: the grid %s needs at least two voxels along every axis" % ((nx, ny, nz),))
        dev = res["dist"].device
        axes = [a.to(dev) for a in _grid_axes(boundaries, step_size)]
        origin = [float(a[0]) for a in axes]
        step = float(torch.tensor(step_size, dtype=torch.float32))
        fills = {k: (-fusion._head_on(k, dev)[1]).contiguous() if k in fusion._projections else None for k in names}
        dist, valid = res["dist"].view(nx, ny, nz), res["valid_mask"].view(nx, ny, nz)
        if band is None and not as_half:
            sets = {k: res[k].view(nx, ny, nz, -1) for k in names}
            return cls(origin, step, dist, valid, sets, fills, boundaries=boundaries, axes=axes)
        field = cls(origin, step, dist, valid, {}, {}, boundaries=boundaries, axes=axes)
        if band is None:                  # dense half rows: every voxel centre, slab by slab
            rows = field._half_rows(fusion, names, None, nx * ny * nz, max_rows_bytes)
            field._sets, field._fills = {k: rows[k].view(nx, ny, nz, -1) for k in names}, dict(fills)
            return field
        mark = field._mark(band)
        if as_half:
            return field._banded(band, mark, field._half_rows(fusion, names, mark[2], mark[2].shape[0], max_rows_bytes), fills)
        pts = field._voxel_centres(mark[2])
        with torch.no_grad():
            if pts.shape[0] > 0:
                rows = fusion.batch_eval(pts, return_names=names)
                rows = {k: rows[k] for k in names}
            else:                     # nothing within the band: empty row arrays of the widths the query would write
                rows = {k: torch.empty((0, fusion._query_map(k, dev).shape[3]), dtype=torch.float32, device=dev) for k in names}
        return field._banded(band, mark, rows, fills)

    def _half_rows(self, fusion, names, voxels, m, max_rows_bytes):
        """{name: float16 [m, C]}: the rows of the voxels with flat indices `voxels` (None: 0 .. m - 1), evaluated at their centres in
        chunks of at most max_rows_bytes of float32 rows (all names together; at least one voxel) and converted chunk by chunk"""
        dev = self.device
        widths = {k: fusion._query_map(k, dev).shape[3] for k in names}
        rows = {k: torch.empty((m, widths[k]), dtype=torch.float16, device=dev) for k in names}
        per = max(1, int(max_rows_bytes) // max(4 * sum(widths.values()), 1))
        with torch.no_grad():
            for q0 in range(0, m if names else 0, per):
                q1 = min(q0 + per, m)
                idx = torch.arange(q0, q1, device=dev) if voxels is None else voxels[q0:q1]
                part = fusion.batch_eval(self._voxel_centres(idx), return_names=names)
                for k in names:
                    rows[k][q0:q1] = part[k]      # (copy_ converts: round to nearest even, as .to(torch.float16))
        return rows

    # ---- the band -------------------------------------------------------------------------------------------------------------
    def _mark(self, band):
        """d3f_band_mark -> (cell_band, slot, voxels [M]); a capacity that turns out too small costs one re-run with the count"""
        dev = self.device
        nx, ny, nz = self.grid_shape
        n = nx * ny * nz
        cell_band = torch.empty((nx - 1, ny - 1, nz - 1), dtype=torch.uint8, device=dev)
        slot = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)        # (d3f_band_mark always writes it)
        vol = self._volume()
        capacity = min(n, max(1 << 12, n // 8))
        with self._on() as q:
            ws, ws_bytes = q.workspace("d3f_band_workspace_bytes", nx, ny, nz)
            while True:
                voxels = torch.empty(capacity, dtype=torch.int32, device=dev)
                q.d3f_band_mark(vol, float(band), cell_band, slot, voxels, capacity, count, ws, ws_bytes)
                found = int(count.item())
                if found <= capacity:
                    break
                capacity = found
        return cell_band, slot, voxels[:found].clone() if found < capacity else voxels

    def _voxel_centres(self, voxels):
        """[len, 3] centres of the voxels with these flat indices: the baked grid's own axis values where the field came from
        Fusion.bake (exactly the points eval_grid evaluated), origin + i * step in float32 otherwise"""
        nx, ny, nz = self.grid_shape
        q = voxels.long()
        iz, ixy = q % nz, q // nz
        ix, iy = ixy // ny, ixy % ny
        if self._axes is not None:
            return torch.stack((self._axes[0][ix], self._axes[1][iy], self._axes[2][iz]), dim=1)
        o = torch.tensor(self.origin, dtype=torch.float32, device=self.device)
        return o + torch.stack((ix, iy, iz), dim=1).to(torch.float32) * torch.tensor(self.step, dtype=torch.float32, device=self.device)

    def _banded(self, band, mark, rows, fills):
        """a field that shares this one's dist / valid / cell_valid and holds `rows` {name: [M, C]} behind the slot volume"""
        f = object.__new__(type(self))
        f.__dict__.update(self.__dict__)
        f.band = float(band)
        f.cell_band, f.slot, f.band_voxels = mark
        f._sets, f._fills = dict(rows), dict(fills)
        return f

    def to_band(self, band):
        """A new field with the same dist / valid / cell_valid (shared, not copied) whose sets keep only the rows of the voxels a
        cell within `band` (a world length > 0) of the surface needs: seed = valid & |dist| < band, a cell is kept if it is valid
        and has a seed corner, a voxel is stored if it is a corner of a kept cell.  Lookups give the same bits as this field where
        'in_band', the fill row elsewhere."""
        if self.band is not None:
            raise ValueError("to_band: this field is already banded (band = %g)" % self.band)
        band = _check_band(band, "to_band")
        _check_band_names(self.names())
        mark = self._mark(band)
        idx = mark[2].long()
        rows = {k: t.view(-1, t.shape[3]).index_select(0, idx) for k, t in self._sets.items()}
        return self._banded(band, mark, rows, self._fills)

    def _need_band(self, what):
        if self.band is None:
            raise AttributeError("%s: this field is dense; to_band(band) or Fusion.bake(..., band=) make a banded one" % what)

    def band_points(self):
        """[M, 3] float32: the centres of the stored voxels, in slot order"""
        self._need_band("band_points")
        return self._voxel_centres(self.band_voxels)

    @property
    def stored_fraction(self):
        """M / (nx * ny * nz)"""
        self._need_band("stored_fraction")
        nx, ny, nz = self.grid_shape
        return self.band_voxels.shape[0] / float(nx * ny * nz)

    def _band_struct(self):
        return _lib.Band(_lib.ptr(self.slot), _lib.ptr(self.cell_band), self.band_voxels.shape[0])

    def _mask_keys(self):
        return ("valid_mask",) if self.band is None else ("valid_mask", "in_band")

    def _channels(self, name):
        return self._sets[name].shape[-1]

    # ---- description ----------------------------------------------------------------------------------------------------------
    def names(self):
        return list(self._sets)

    def fill_row(self, name):
        """[C] row of `name` at a point that is not valid"""
        f = self._fills[name]
        return torch.zeros(self._channels(name), dtype=torch.float32, device=self.device) if f is None else f

    def _on(self):
        return _lib.on(self.device, self._lib)

    def _volume(self):
        nx, ny, nz = self.grid_shape
        return _lib.Volume(nx, ny, nz, (ctypes.c_float * 3)(*self.origin), self.step, 0, _lib.ptr(self.dist), _lib.ptr(self.valid),
                           _lib.ptr(self.cell_valid))

    def _set_array(self, names):
        """the d3f_volume_set array of `names`: the one place that builds them, so the storage word always follows the tensor's dtype"""
        arr = (_lib.VolumeSet * max(len(names), 1))()
        for s, k in enumerate(names):
            t = self._sets[k]
            word = _lib.DTYPE_F16 if t.dtype == torch.float16 else _lib.DTYPE_F32
            arr[s] = _lib.VolumeSet(t.data_ptr(), t.shape[-1], word, t.stride(-2), _lib.ptr(self._fills[k]))      # dense: the voxel stride; banded: the row stride (in elements)
        return arr

    # ---- storage of the rows ----------------------------------------------------------------------------------------------------
    def rows_dtype(self, name):
        """torch.float32 or torch.float16: how the rows of `name` are stored"""
        self._names([name])
        return self._sets[name].dtype

    @property
    def rows_bytes(self):
        """the bytes of all stored rows (every set; dist, valid and the band's volumes are not counted)"""
        return sum(t.numel() * t.element_size() for t in self._sets.values())

    def _with_sets(self, sets):
        """a field that shares everything of this one (dist / valid / cell_valid / slot / cell_band ...) but holds `sets`"""
        f = object.__new__(type(self))
        f.__dict__.update(self.__dict__)
        f._sets, f._fills = dict(sets), dict(self._fills)
        return f

    def half(self, names=None, check=False):
        """A new field whose named sets (None: all) are STORED as IEEE half: `.to(torch.float16)`, round to nearest even, a value beyond
        +-65504 becomes +-Inf.  dist / valid / cell_valid / slot / cell_band are shared, not copied.  eval / eval_dist / backward /
        autograd / raycast / render read such rows (d3f_volume_set's storage word): each half is widened exactly and takes the float32
        chain, so a lookup equals the lookup of float() bit for bit at half the row bytes.  Fill rows, outputs and gradients stay float32.
        The methods that read rows with loops of their own (pool, links / parts, flow, warp, align / normal_equations / relocate, locate)
        raise TypeError on a half set: call float() first.
        check=True: ValueError if a finite stored value of a valid voxel would not stay finite (one host synchronisation)."""
        names = self._names(self.names() if names is None else names)
        sets = dict(self._sets)
        for k in names:
            t = sets[k]
            if t.dtype == torch.float16:
                continue
            h = t.to(torch.float16)
            if check:
                lost = torch.isfinite(t) & ~torch.isfinite(h)
                if self.band is None:
                    lost &= self.valid.unsqueeze(-1)
                if bool(lost.any()):
                    raise ValueError("half: set %r holds %d finite values of valid voxels beyond the half range (+-65504)" % (k, int(lost.sum())))
            sets[k] = h
        return self._with_sets(sets)

    def float(self, names=None):
        """The inverse of half(): a new field whose named sets (None: all) are float32, every stored half widened exactly"""
        names = self._names(self.names() if names is None else names)
        sets = dict(self._sets)
        for k in names:
            sets[k] = sets[k].to(torch.float32)
        return self._with_sets(sets)

    def _need_float_rows(self, who, names):
        """the methods whose kernels read float32 rows only refuse a half set here, before any call into the library: converting on the
        quiet would allocate the very array the caller chose not to hold"""
        for k in names:
            t = self._sets.get(k)
            if t is not None and t.dtype != torch.float32:
                raise TypeError("%s: the rows of %r are stored as %s and this method reads float32 rows; use float([%r]) (or float()) first"
                                % (who, k, str(t.dtype).replace("torch.", ""), k))

    def _names(self, return_names):
        names = self.names() if return_names is None else list(return_names)
        for k in names:
            if k not in self._sets:
                raise KeyError("%r was not baked; this field holds %s" % (k, self.names()))
        if len(names) > _lib.MAX_MAPS:
            raise ValueError("at most %d names per lookup" % _lib.MAX_MAPS)
        return names

    # ---- the lookup -----------------------------------------------------------------------------------------------------------
    def _sample(self, pts_c, names):
        dev, n = self.device, pts_c.shape[0]
        out = {"dist": torch.empty(n, dtype=torch.float32, device=dev), "valid_mask": torch.empty(n, dtype=torch.bool, device=dev)}
        outs = (ctypes.c_void_p * max(len(names), 1))()
        if self.band is not None:
            out["in_band"] = torch.empty(n, dtype=torch.bool, device=dev)
        for s, k in enumerate(names):
            out[k] = torch.empty((n, self._channels(k)), dtype=torch.float32, device=dev)
            outs[s] = out[k].data_ptr()
        with self._on() as q:
            if self.band is None:
                q.d3f_volume_sample(self._volume(), pts_c, n, self._set_array(names), len(names), out["dist"], out["valid_mask"], outs)
            else:
                q.d3f_band_sample(self._volume(), self._band_struct(), pts_c, n, self._set_array(names), len(names), out["dist"], out["valid_mask"],
                                  out["in_band"], outs)
        return out

    def backward(self, pts, grad_dist=None, grad_sets=None):
        """grad_pts [N,3] = d(sum grad_dist * dist + sum over names of grad * row) / d pts (d3f_volume_sample_backward);
        grad_sets: {name: [N,C] or None}.  Banded (d3f_band_sample_backward): the dist term at every valid point, a set's term
        only where 'in_band'."""
        _check_points(pts, self.device, "BakedField.eval")
        pts_c = pts.detach().contiguous()
        dev, n = self.device, pts_c.shape[0]
        grad_sets = {k: g for k, g in (grad_sets or {}).items() if g is not None}
        names = self._names(list(grad_sets))
        grads = (ctypes.c_void_p * max(len(names), 1))()
        hold = []
        for s, k in enumerate(names):
            g = grad_sets[k].detach().to(torch.float32).contiguous()
            if tuple(g.shape) != (n, self._channels(k)) or g.device != dev:
                raise ValueError("backward: the gradient of %r must be [%d,%d] on %s" % (k, n, self._channels(k), dev))
            hold.append(g)
            grads[s] = g.data_ptr()
        gd = None
        if grad_dist is not None:
            gd = grad_dist.detach().to(torch.float32).contiguous()
            if tuple(gd.shape) != (n,) or gd.device != dev:
                raise ValueError("backward: grad_dist must be [%d] on %s" % (n, dev))
        grad_pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        with self._on() as q:
            if self.band is None:
                q.d3f_volume_sample_backward(self._volume(), pts_c, n, self._set_array(names), len(names), gd, grads, grad_pts)
            else:
                q.d3f_band_sample_backward(self._volume(), self._band_struct(), pts_c, n, self._set_array(names), len(names), gd, grads, grad_pts)
        return grad_pts

    def eval(self, pts, return_names=None):
        """The dict of Fusion.eval -- 'dist' [N], 'valid_mask' [N] bool, one [N,C] float32 per name (None: every baked name) --
        interpolated in the volume.  Not valid (outside, a NaN coordinate, a cell with an invalid corner): dist 1e3, the fill row.
        A banded field adds 'in_band' [N] bool after 'valid_mask' (valid and the point's cell is kept): rows are the dense field's
        where it is set and the fill row elsewhere; dist and valid_mask never depend on the band."""
        _check_points(pts, self.device, "BakedField.eval")
        names = self._names(return_names)
        if pts.requires_grad and torch.is_grad_enabled():
            res = _BakedQueryFn.apply(pts, self, tuple(names))
            out = dict(zip(("dist",) + self._mask_keys() + tuple(names), res))
            return out
        return self._sample(pts.detach().contiguous(), names)

    batch_eval = eval

    def eval_dist(self, pts):
        return self.eval(pts, return_names=[])

    # ---- clearance ------------------------------------------------------------------------------------------------------------
    def _edt(self, sites, max_d2):
        """one d3f_volume_edt on a bool volume -> (d2 int32, nearest int32, dist float32), each [nx, ny, nz]"""
        dev = self.device
        nx, ny, nz = self.grid_shape
        site = sites.contiguous().view(torch.uint8)
        d2 = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        nearest = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        dist = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        with self._on() as q:
            ws, ws_bytes = q.workspace("d3f_volume_edt_workspace_bytes", nx, ny, nz)
            q.d3f_volume_edt(site, nx, ny, nz, self.step, int(max_d2), d2, nearest, dist, ws, ws_bytes)
        return d2, nearest, dist

    def _site_mask(self, who, iso, unknown, sites):
        """the bool site volume of clearance / components: valid & (dist <= iso), plus the invalid voxels for unknown="occupied"; or the
        caller's own `sites` volume, which iso and unknown then must not accompany"""
        if unknown not in ("free", "occupied"):
            raise ValueError("%s: unknown must be 'free' or 'occupied', got %r" % (who, unknown))
        iso = float(iso)
        if not math.isfinite(iso):
            raise ValueError("%s: iso must be finite, got %r" % (who, iso))
        if sites is None:
            mask = self.valid & (self.dist <= iso)
            return mask | ~self.valid if unknown == "occupied" else mask
        if iso != 0.0 or unknown != "free":
            raise ValueError("%s: iso and unknown describe the field's own site mask; leave them at their defaults with sites=" % who)
        if not isinstance(sites, torch.Tensor) or tuple(sites.shape) != tuple(self.grid_shape) or sites.dtype not in (torch.bool, torch.uint8):
            raise ValueError("%s: sites must be a bool or uint8 tensor of shape %s" % (who, tuple(self.grid_shape)))
        if sites.device != self.device:
            raise RuntimeError("%s: sites is on %s, the field on %s" % (who, sites.device, self.device))
        return sites.detach() if sites.dtype == torch.bool else sites.detach() != 0

    @staticmethod
    def _check_ccl(who, connectivity, min_voxels):
        if connectivity not in (6, 18, 26):
            raise ValueError("%s: connectivity must be 6, 18 or 26, got %r" % (who, connectivity))
        if isinstance(min_voxels, bool) or not isinstance(min_voxels, int) or not 1 <= min_voxels <= 2 ** 31 - 1:
            raise ValueError("%s: min_voxels must be an integer >= 1, got %r" % (who, min_voxels))

    _STATS_ROWS = 4096      # the stats rows the first launch of _label has room for

    def _label(self, mask, connectivity, min_voxels, want_stats=True, links=None):
        """d3f_volume_components on a bool volume (with a link volume: d3f_volume_components_linked) -> (labels int32 [nx,ny,nz], K, found,
        stats int32 [K, 8] or None); one host read of the count; more kept components than the first launch had rows for cost one re-run
        with the count (as _mark)"""
        dev = self.device
        nx, ny, nz = self.grid_shape
        site = mask.contiguous().view(torch.uint8)
        labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        with self._on() as q:
            ws, ws_bytes = q.workspace("d3f_volume_components_workspace_bytes", nx, ny, nz)

            def launch(stats, capacity):
                tail = (nx, ny, nz, connectivity, min_voxels, labels, count, stats, capacity, ws, ws_bytes)
                if links is None:
                    q.d3f_volume_components(site, *tail)
                else:
                    q.d3f_volume_components_linked(site, links, *tail)
                return count.tolist()

            if not want_stats:
                kept, found = launch(None, 0)
                return labels, kept, found, None
            capacity = min(nx * ny * nz, self._STATS_ROWS)
            stats = torch.empty((capacity, 8), dtype=torch.int32, device=dev)
            kept, found = launch(stats, capacity)
            if kept > capacity:
                stats = torch.empty((kept, 8), dtype=torch.int32, device=dev)
                launch(stats, kept)
        return labels, kept, found, stats[:kept].clone() if kept < stats.shape[0] else stats

    def _check_links(self, who, links):
        """a caller's link volume: uint16 (or int16, the same bits) [nx, ny, nz] on this device"""
        if not isinstance(links, torch.Tensor) or tuple(links.shape) != tuple(self.grid_shape) or links.dtype not in (torch.uint16, torch.int16):
            raise ValueError("%s: links must be a uint16 (or int16) tensor of shape %s, as links() returns it" % (who, tuple(self.grid_shape)))
        if links.device != self.device:
            raise RuntimeError("%s: links is on %s, the field on %s" % (who, links.device, self.device))
        return links.detach().contiguous()

    def _members(self, sites):
        """the voxels of a site mask whose row exists: valid and, on a banded field, stored"""
        mask = sites & self.valid
        return mask if self.band is None else mask & (self.slot >= 0)

    def _link_rule(self, who, name, rule, tau, cos):
        """-> (the enum, the float threshold the kernel compares with) of links() / parts()"""
        if not self._sets:
            raise ValueError("%s: this field holds no sets (a clearance or travel field); link the field it came from" % who)
        self._names([name])
        if rule == "l2":
            if cos is not None or tau is None:
                raise ValueError("%s: rule 'l2' takes tau (a distance between rows) and no cos" % who)
            tau = float(tau)
            if not tau >= 0.0:
                raise ValueError("%s: tau must be a distance >= 0 (math.inf links every pair of finite rows), got %r" % (who, tau))
            t = torch.tensor(tau, dtype=torch.float32)
            return _lib.LINK_L2, float(t * t)              # float32(tau)^2, squared in float32
        if rule == "cosine":
            if tau is not None or cos is None:
                raise ValueError("%s: rule 'cosine' takes cos (the smallest cosine that links) and no tau" % who)
            cos = float(cos)
            if not 0.0 <= cos <= 1.0:
                raise ValueError("%s: cos must lie in [0, 1], got %r" % (who, cos))
            return _lib.LINK_COSINE, cos
        if rule == "argmax":
            if tau is not None or cos is not None:
                raise ValueError("%s: rule 'argmax' takes neither tau nor cos" % who)
            return _lib.LINK_ARGMAX, 0.0
        raise ValueError("%s: rule must be 'l2', 'cosine' or 'argmax', got %r" % (who, rule))

    def _links(self, name, rule, threshold, members, connectivity):
        """d3f_volume_links over a member mask (already reduced to valid and stored voxels) -> uint16 [nx, ny, nz]"""
        dev = self.device
        nx, ny, nz = self.grid_shape
        if self.band is not None and self.band_voxels.shape[0] == 0:      # an empty band has no row array to point at, and no member
            return torch.zeros((nx, ny, nz), dtype=torch.uint16, device=dev)
        out = torch.empty((nx, ny, nz), dtype=torch.uint16, device=dev)
        site = members.contiguous().view(torch.uint8)
        sets = self._set_array([name])
        with self._on() as q:
            q.d3f_volume_links(site, None, self.slot, nx, ny, nz, sets, rule, threshold, connectivity, out)
        return out

    def links(self, name, rule="l2", tau=None, cos=None, iso=0.0, sites=None, connectivity=26):
        """Which neighbouring voxels belong together by their stored rows (d3f_volume_links) -> uint16 [nx, ny, nz].

        Bit j of voxel v names its neighbour at offset j = 9*(dx+1) + 3*(dy+1) + (dz+1), j = 0..12 -- the 13 neighbours of lower flat index
        -- and is set iff both voxels are members, the connectivity allows the offset and the rule accepts their rows of `name`:
          rule="l2"      |a - b|^2 <= float32(tau)^2 (tau a distance between rows; math.inf links every pair of finite rows)
          rule="cosine"  the cosine of the two rows is at least cos in [0, 1] (a zero row links to nothing)
          rule="argmax"  both rows have their first maximum at the same channel: pool's vote rule, exact, for an instance-mask set
        Members are the sites -- valid & (dist <= iso), or the caller's bool / uint8 volume -- that are valid and, on a banded field,
        stored.  The sums are float32 in ascending channel order and reproducible bit for bit.  Callers may AND criteria of their own into
        the result (view it as int16 for torch's bitwise operators) and hand it to components(links=).  Not differentiable."""
        if connectivity not in (6, 18, 26):
            raise ValueError("links: connectivity must be 6, 18 or 26, got %r" % (connectivity,))
        code, threshold = self._link_rule("links", name, rule, tau, cos)
        self._need_float_rows("links", [name])
        members = self._members(self._site_mask("links", iso, "free", sites))
        return self._links(name, code, threshold, members, connectivity)

    def parts(self, name, rule="l2", tau=None, cos=None, iso=0.0, sites=None, connectivity=26, min_voxels=1):
        """The components of the occupied voxels whose neighbouring rows of `name` agree: links(), then the labelling over those links
        (d3f_volume_components_linked) -> Components, whose `sites` is the member mask (the sites that are valid and stored).  Two touching
        objects with different descriptors are two parts where components() sees one; on an instance-mask set rule="argmax" gives one part
        per spatially connected piece of each instance.  pool, mask, largest, label_at, boxes_world and clearance(sites=) take the result."""
        self._check_ccl("parts", connectivity, min_voxels)
        code, threshold = self._link_rule("parts", name, rule, tau, cos)
        self._need_float_rows("parts", [name])
        members = self._members(self._site_mask("parts", iso, "free", sites))
        links = self._links(name, code, threshold, members, connectivity)
        labels, kept, found, stats = self._label(members, connectivity, min_voxels, links=links)
        return Components(self.origin, self.step, labels, kept, found, stats, members, connectivity, min_voxels)

    def flow(self, other, name, radius_voxels=2, max_cost=None, iso=0.0, sites=None, other_sites=None, refine=True, seed=None):
        """How did it move?  For every member voxel of this field the voxel of `other` -- a field on the same grid -- within Chebyshev distance
        radius_voxels whose stored row of `name` is closest in L2 (d3f_volume_flow, csrc/flow_kernels.hip) -> Flow.

        other          a BakedField with the same grid_shape, origin and step on the same device; either field may be dense or banded
        radius_voxels  1..4: the half width of the search window in voxels
        max_cost       None, or a distance between rows >= 0: a candidate takes part only if its squared distance is <= float32(max_cost)^2
        iso, sites     this field's members, as links() takes them; other_sites: the other field's (None: its own valid & (dist <= iso))
        refine         also the costs of the target's six axis neighbours, and from them the sub-voxel `offset`
        seed           None, or an int32 [nx, ny, nz, 3] tensor on the device (Flow.seed of a coarser flow): the window of every member is centred
                       on voxel + seed instead of the voxel (d3f_volume_flow_seeded, csrc/flow_seeded_kernels.hip); ties
                       go to the candidate nearest that centre; a member whose seed leaves [-16384, 16384] stays unmatched.  A zero seed gives
                       the bytes of seed=None
        Members are the sites that are valid and, on a banded field, stored.  The costs are float32 sums in ascending channel order; ties go
        to the nearer candidate, then to the lower flat index: the same bytes on every run.  Not differentiable."""
        if not isinstance(other, BakedField):
            raise ValueError("flow: other must be a BakedField, got %r" % (type(other).__name__,))
        if not self._sets or not other._sets:
            raise ValueError("flow: a field without sets (a clearance or travel field) has no rows to compare; use the fields they came from")
        for f, who in ((self, "this field"), (other, "the other field")):
            if name not in f._sets:
                raise ValueError("flow: %r was not baked in %s, which holds %s" % (name, who, f.names()))
        if self._channels(name) != other._channels(name):
            raise ValueError("flow: %r has %d channels here and %d in the other field" % (name, self._channels(name), other._channels(name)))
        self._need_float_rows("flow", [name])
        other._need_float_rows("flow (the other field)", [name])
        if tuple(self.grid_shape) != tuple(other.grid_shape) or self.origin != other.origin or self.step != other.step:
            raise ValueError("flow: the fields must share one grid: %s at %s step %g here, %s at %s step %g there" % (
                tuple(self.grid_shape), self.origin, self.step, tuple(other.grid_shape), other.origin, other.step))
        if self.device != other.device:
            raise ValueError("flow: the other field is on %s, this one on %s" % (other.device, self.device))
        if isinstance(radius_voxels, bool) or not isinstance(radius_voxels, int) or not 1 <= radius_voxels <= _lib.FLOW_MAX_RADIUS:
            raise ValueError("flow: radius_voxels must be an integer in 1..%d, got %r" % (_lib.FLOW_MAX_RADIUS, radius_voxels))
        if seed is not None:
            if not isinstance(seed, torch.Tensor):
                raise TypeError("flow: seed must be None or an int32 tensor, got %s" % type(seed).__name__)
            if seed.dtype != torch.int32 or tuple(seed.shape) != tuple(self.grid_shape) + (3,):
                raise ValueError("flow: seed must be an int32 tensor of shape %s, got %s %s" % (tuple(self.grid_shape) + (3,), seed.dtype, tuple(seed.shape)))
            if seed.device != self.device:
                raise ValueError("flow: seed is on %s, the field on %s" % (seed.device, self.device))
        max_cost2 = math.inf
        if max_cost is not None:
            max_cost = float(max_cost)
            if not max_cost >= 0.0:
                raise ValueError("flow: max_cost must be a distance >= 0 (None: no threshold), got %r" % (max_cost,))
            t = torch.tensor(max_cost, dtype=torch.float32)
            max_cost2 = float(t * t)              # float32(max_cost)^2, squared in float32
        members_a = self._members(self._site_mask("flow", iso, "free", sites))
        members_b = other._members(other._site_mask("flow", iso if other_sites is None else 0.0, "free", other_sites))
        dev = self.device
        nx, ny, nz = self.grid_shape
        empty = any(f.band is not None and f.band_voxels.shape[0] == 0 for f in (self, other))      # no row array to point at, and no member
        if empty:
            target = torch.full((nx, ny, nz), -1, dtype=torch.int32, device=dev)
            cost = torch.full((nx, ny, nz), math.inf, dtype=torch.float32, device=dev)
            axis = torch.full((nx, ny, nz, 6), math.inf, dtype=torch.float32, device=dev) if refine else None
            return Flow(self.origin, self.step, target, cost, axis)
        target = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        cost = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        axis = torch.empty((nx, ny, nz, 6), dtype=torch.float32, device=dev) if refine else None
        site_a, site_b = members_a.contiguous().view(torch.uint8), members_b.contiguous().view(torch.uint8)
        set_a, set_b = self._set_array([name]), other._set_array([name])
        with self._on() as q:
            if seed is None:
                q.d3f_volume_flow(site_a, self.slot, set_a, site_b, other.slot, set_b, nx, ny, nz, radius_voxels, max_cost2, target, cost, axis)
            else:
                seed = seed.detach().contiguous()
                q.d3f_volume_flow_seeded(_lib.FlowSeeded(_lib.ptr(site_a), _lib.ptr(self.slot), set_a, _lib.ptr(site_b), _lib.ptr(other.slot), set_b, _lib.ptr(seed),
                                                         nx, ny, nz, radius_voxels, max_cost2, 0, _lib.ptr(target), _lib.ptr(cost), _lib.ptr(axis)))
        return Flow(self.origin, self.step, target, cost, axis)

    # ---- the pyramid ----------------------------------------------------------------------------------------------------------
    def coarsen(self, min_children=1, band=None, return_names=None):
        """This field at half the resolution (d3f_volume_coarsen_select / d3f_volume_coarsen_rows, csrc/pyramid_kernels.hip, declared by
        include/d3fields_hip_pyramid.h) -> a new BakedField of ceil(n / 2) voxels per axis with step 2 * step and
        origin + step / 2.  Coarse voxel (X, Y, Z) has the children (2X + i, 2Y + j, 2Z + k), i, j, k in {0, 1}, inside this grid.

        min_children  1..8: the coarse voxel is valid iff at least that many children are valid with a dist that is no NaN; its dist is their
                      float32 mean (summed in ascending flat index, times 1 / count), 1e3 elsewhere
        band          None: the result is dense iff this field is dense, else banded with self.band; a world length: banded with it
        return_names  the sets of the result (None: all)
        Rows: the float32 mean of the rows of the children that count and, on a banded field, are stored; none -> the fill row and
        rows_known False.  Half rows are widened exactly; the result is float32 (half() it).  The result also has `children` (uint8 masks)
        and rows_known.  A banded result goes select, d3f_band_mark on the coarse dist, the rows of the stored coarse voxels only: no dense
        coarse row array exists at any time.  Every extent must be at least 3.  No host read on the dense path, the one of d3f_band_mark
        on the banded one.  Not differentiable.  travel / components / locate / clearance accept the result as any field: a cheap first pass."""
        if isinstance(min_children, bool) or not isinstance(min_children, int):
            raise TypeError("coarsen: min_children must be an integer, got %s" % type(min_children).__name__)
        if not 1 <= min_children <= 8:
            raise ValueError("coarsen: min_children must lie in 1..8, got %r" % (min_children,))
        names = self._names(return_names)
        if band is not None:
            band = _check_band(band, "coarsen")
        elif self.band is not None:
            band = self.band
        if band is not None:
            _check_band_names(names)
        nx, ny, nz = self.grid_shape
        if min(nx, ny, nz) < 3:
            raise ValueError("coarsen: every extent must be at least 3 (a field needs 2 voxels per axis), this grid is %s" % (tuple(self.grid_shape),))
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("coarsen: the field must live on the ROCm device; there is no CPU path")
        cx, cy, cz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
        nc = cx * cy * cz
        dist = torch.empty((cx, cy, cz), dtype=torch.float32, device=dev)
        valid = torch.empty((cx, cy, cz), dtype=torch.uint8, device=dev)
        children = torch.empty((cx, cy, cz), dtype=torch.uint8, device=dev)
        sel = _lib.CoarsenSelect(nx, ny, nz, min_children, _lib.ptr(self.dist), _lib.ptr(self.valid), _lib.ptr(dist), _lib.ptr(valid), _lib.ptr(children), 0)
        with self._on() as q:
            q.d3f_volume_coarsen_select(sel)
        origin = tuple(o + self.step / 2 for o in self.origin)
        coarse = type(self)(origin, 2.0 * self.step, dist, valid.view(torch.bool), {}, {})
        if band is None:
            mark, voxels, m = None, None, nc
        else:
            mark = coarse._mark(band)
            voxels, m = mark[2], mark[2].shape[0]
        known = torch.empty(m, dtype=torch.uint8, device=dev)
        rows = {k: torch.empty((m, self._channels(k)), dtype=torch.float32, device=dev) for k in names}
        if m > 0:
            outs = (ctypes.c_void_p * max(len(names), 1))(*[rows[k].data_ptr() for k in names])
            src = None if self.band is None else self._band_struct()
            args = _lib.CoarsenRows(nx, ny, nz, len(names), None if src is None else ctypes.pointer(src), self._set_array(names), _lib.ptr(children), _lib.ptr(voxels),
                                    m, outs, _lib.ptr(known), 0)
            with self._on() as q:
                q.d3f_volume_coarsen_rows(args)
        fills = {k: self._fills[k] for k in names}
        if band is None:
            coarse._sets, coarse._fills = {k: rows[k].view(cx, cy, cz, -1) for k in names}, fills
            coarse.rows_known = known.view(torch.bool).view(cx, cy, cz)
        else:
            coarse = coarse._banded(band, mark, rows, fills)
            coarse.rows_known = known.view(torch.bool)
        coarse.children = children
        return coarse

    def _max_levels(self):
        """how often this grid halves before an extent drops below 2"""
        e, levels = min(self.grid_shape), 0
        while e >= 3:
            e, levels = (e + 1) // 2, levels + 1
        return levels

    def pyramid(self, levels, **kw):
        """[self, coarsen(**kw), its coarsen(**kw), ...]: `levels` coarser fields behind this one, each at half the resolution of the one before"""
        if isinstance(levels, bool) or not isinstance(levels, int):
            raise TypeError("pyramid: levels must be an integer, got %s" % type(levels).__name__)
        if levels < 0 or levels > self._max_levels():
            raise ValueError("pyramid: levels = %r, the grid %s allows 0..%d (every level needs extents of at least 2)" % (
                levels, tuple(self.grid_shape), self._max_levels()))
        out = [self]
        for _ in range(levels):
            out.append(out[-1].coarsen(**kw))
        return out

    def flow_pyramid(self, other, name, levels=2, radius_voxels=2, fine_radius_voxels=1, min_children=1, refine=True, **flow_kw):
        """How far did it move?  Coarse-to-fine flow over the pyramids of both fields -> the Flow of the finest level;
        its `coarse` lists the flows of the coarser levels, coarsest first.  The coarsest level runs flow() at radius_voxels; every finer
        level runs flow(seed=) at fine_radius_voxels round the prediction Flow.seed makes from the level above.  Reach: about radius_voxels *
        2**levels voxels of this grid, where flow() alone ends at 4.  flow_kw (max_cost, iso) goes to every level; sites / other_sites
        belong to one grid and are refused.  consistent, displacement and motions work on the result as on any Flow."""
        if not isinstance(other, BakedField):
            raise ValueError("flow_pyramid: other must be a BakedField, got %r" % (type(other).__name__,))
        if isinstance(levels, bool) or not isinstance(levels, int):
            raise TypeError("flow_pyramid: levels must be an integer, got %s" % type(levels).__name__)
        for what, rv in (("radius_voxels", radius_voxels), ("fine_radius_voxels", fine_radius_voxels)):
            if isinstance(rv, bool) or not isinstance(rv, int) or not 1 <= rv <= _lib.FLOW_MAX_RADIUS:
                raise ValueError("flow_pyramid: %s must be an integer in 1..%d, got %r" % (what, _lib.FLOW_MAX_RADIUS, rv))
        for k in flow_kw:
            if k not in ("max_cost", "iso"):
                raise TypeError("flow_pyramid: unexpected argument %r (max_cost and iso go to every level)" % (k,))
        if tuple(self.grid_shape) != tuple(other.grid_shape) or self.origin != other.origin or self.step != other.step:
            raise ValueError("flow_pyramid: the fields must share one grid: %s at %s step %g here, %s at %s step %g there" % (
                tuple(self.grid_shape), self.origin, self.step, tuple(other.grid_shape), other.origin, other.step))
        for f, who in ((self, "this field"), (other, "the other field")):
            if name not in f._sets:
                raise ValueError("flow_pyramid: %r was not baked in %s, which holds %s" % (name, who, f.names()))
        self._need_float_rows("flow_pyramid", [name])
        other._need_float_rows("flow_pyramid (the other field)", [name])
        mine = self.pyramid(levels, min_children=min_children, return_names=[name])
        theirs = other.pyramid(levels, min_children=min_children, return_names=[name])
        flows = [mine[-1].flow(theirs[-1], name, radius_voxels=radius_voxels, refine=refine, **flow_kw)]
        for a, b in zip(mine[-2::-1], theirs[-2::-1]):
            flows.append(a.flow(b, name, radius_voxels=fine_radius_voxels, refine=refine, seed=flows[-1].seed(a.grid_shape, refined=refine), **flow_kw))
        out = flows[-1]
        out.coarse = flows[:-1]
        return out

    # ---- warp -----------------------------------------------------------------------------------------------------------------
    def _check_label_volume(self, who, what, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != tuple(self.grid_shape):
            raise ValueError("%s: %s must be an int32 tensor of shape %s, got %s" % (
                who, what, tuple(self.grid_shape), "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != self.device:
            raise ValueError("%s: %s is on %s, the field on %s" % (who, what, t.device, self.device))
        return t.detach()

    def _check_same_grid(self, who, what, other):
        if tuple(other.grid_shape) != tuple(self.grid_shape) or tuple(other.origin) != self.origin or float(other.step) != self.step:
            raise ValueError("%s: %s is of a grid %s at %s step %g, the field of %s at %s step %g" % (
                who, what, tuple(other.grid_shape), tuple(other.origin), other.step, tuple(self.grid_shape), self.origin, self.step))

    def owners(self, parts, margin_voxels=2):
        """Which part does each voxel travel with? -> int32 [nx, ny, nz]: every voxel within margin_voxels (a Euclidean distance in voxels) of a
        part's voxels gets the label of its nearest part voxel (among equidistant ones the transform's own choice, the same on every run), all
        other voxels 0.  parts: a Components on this grid or an int32 label volume.  The margin is what carries the free side of a part's
        surface along with it in warp(); margin_voxels = 0 returns the labels themselves.  One clearance(sites=, max_distance=) and one gather."""
        if isinstance(parts, Components):
            self._check_same_grid("owners", "parts", parts)
            labels = parts.labels
        else:
            labels = parts
        labels = self._check_label_volume("owners", "the labels", labels)
        if isinstance(margin_voxels, bool) or not isinstance(margin_voxels, (int, float)) or not (0.0 <= float(margin_voxels) < math.inf):
            raise ValueError("owners: margin_voxels must be a finite number >= 0, got %r" % (margin_voxels,))
        cap = min(math.floor(float(margin_voxels) ** 2), 2 ** 31 - 2)
        if cap < 1:
            return labels
        # (the cap the transform derives is floor((max_distance / step)^2): aim at cap + 1/2, which no rounding of the quotient moves across an integer)
        c = self.clearance(sites=labels > 0, max_distance=self.step * math.sqrt(cap + 0.5))
        near = c.nearest_voxel
        got = labels.reshape(-1)[torch.clamp(near, min=0).long()]
        return torch.where((near >= 0) & (c.d2 <= cap), got, torch.zeros_like(got))

    def warp(self, motions, owner, which=None, return_names=None):
        """Where is it now?  This field after every part has moved by its rigid motion (d3f_volume_warp_select / d3f_volume_warp_rows,
        csrc/warp_kernels.hip) -> a BakedField on the same grid, dense where this one is dense, banded with the same
        band where it is banded (select, d3f_band_mark on the new dist, then the rows of the stored voxels only: no dense row array exists).

        motions       a PartMotions of this grid (Flow.motions), or a float64 [K, 15] pose tensor laid out as PartMotions.pose
        owner         int32 [nx, ny, nz]: the part each voxel travels with (owners(parts)), or a Components whose labels are taken as they are
        which         None, or bool [K], e.g. motions.moved(min_shift=0.5 * field.step): the parts not selected stay put and are not resampled
        return_names  the sets the result holds (None: every set of this field)
        A part without a pose (a NaN row) does not move.  Per destination voxel the candidates are the voxel itself, if it is valid and its
        owner does not move, and every moving part whose inverse motion puts the voxel next to one of the part's own voxels; the smallest
        signed distance wins, ties go to the background, then to the lower part.  A voxel a part has left is unknown (not valid): what was
        behind the part was never observed.  Rows are copied (background) or blended from eight corner rows (moved) in float32 without fused
        operations.  The result also has source, rows_known, part_box_from, part_box_to (see the class).  No host read on a dense field, the
        one of d3f_band_mark on a banded one.  Not differentiable."""
        self._need_float_rows("warp", self._names(return_names))
        if isinstance(motions, PartMotions):
            self._check_same_grid("warp", "motions", motions)
            pose = motions.pose
        elif isinstance(motions, torch.Tensor):
            pose = motions
        else:
            raise ValueError("warp: motions must be a PartMotions or a float64 [K, %d] pose tensor, got %r" % (_lib.MOTION_POSE_DOUBLES, type(motions).__name__))
        if pose.dtype != torch.float64 or pose.dim() != 2 or pose.shape[1] != _lib.MOTION_POSE_DOUBLES:
            raise ValueError("warp: the poses must be a float64 [K, %d] tensor, got %s %s" % (_lib.MOTION_POSE_DOUBLES, pose.dtype, tuple(pose.shape)))
        K = pose.shape[0]
        if K > _lib.WARP_MAX_PARTS:
            raise ValueError("warp: %d parts, at most %d: select the movers with which= and compact the labels" % (K, _lib.WARP_MAX_PARTS))
        if pose.device != self.device:
            raise ValueError("warp: the poses are on %s, the field on %s" % (pose.device, self.device))
        if isinstance(owner, Components):
            self._check_same_grid("warp", "owner", owner)
            if owner.count != K:
                raise ValueError("warp: owner has %d parts, there are %d poses" % (owner.count, K))
            owner = owner.labels
        owner = self._check_label_volume("warp", "owner", owner)
        if which is not None:
            if not isinstance(which, torch.Tensor) or which.dtype != torch.bool or tuple(which.shape) != (K,):
                raise ValueError("warp: which must be a bool [%d] tensor, one entry per pose" % K)
            if which.device != self.device:
                raise ValueError("warp: which is on %s, the field on %s" % (which.device, self.device))
        names = self._names(return_names)
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("warp: the field must live on the ROCm device; there is no CPU path")
        nx, ny, nz = self.grid_shape
        n = nx * ny * nz
        pose = pose.detach().contiguous()
        if which is not None:
            pose = torch.where(which[:, None], pose, torch.full_like(pose, math.nan))
        owner = owner.contiguous()
        source = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        dist = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        valid = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
        boxes = torch.empty((K, 12), dtype=torch.int32, device=dev)
        sel = _lib.WarpSelect(self._volume(), _lib.ptr(owner), _lib.ptr(pose) if K else None, K, 0, _lib.ptr(source), _lib.ptr(dist), _lib.ptr(valid),
                              _lib.ptr(boxes) if K else None)
        with self._on() as q:
            q.d3f_volume_warp_select(sel)
        moved = type(self)(self.origin, self.step, dist, valid.view(torch.bool), {}, {}, boundaries=self.boundaries, axes=self._axes)
        if self.band is None:
            mark, voxels, m = None, None, n
        else:
            mark = moved._mark(self.band)
            voxels, m = mark[2], mark[2].shape[0]
        known = torch.empty(m, dtype=torch.uint8, device=dev)
        rows = {k: torch.empty((m, self._channels(k)), dtype=torch.float32, device=dev) for k in names}
        if m > 0:
            outs = (ctypes.c_void_p * max(len(names), 1))(*[rows[k].data_ptr() for k in names])
            band = None if self.band is None else self._band_struct()
            args = _lib.WarpRows(self._volume(), None if band is None else ctypes.pointer(band), self._set_array(names), len(names), K, _lib.ptr(source),
                                 _lib.ptr(pose) if K else None, _lib.ptr(voxels), m, outs, _lib.ptr(known))
            with self._on() as q:
                q.d3f_volume_warp_rows(args)
        fills = {k: self._fills[k] for k in names}
        if self.band is None:
            moved._sets, moved._fills = {k: rows[k].view(nx, ny, nz, -1) for k in names}, fills
            moved.rows_known = known.view(torch.bool).view(nx, ny, nz)
        else:
            moved = moved._banded(self.band, mark, rows, fills)
            moved.rows_known = known.view(torch.bool)
        moved.source = source
        moved.part_box_from, moved.part_box_to = boxes[:, 0:6].reshape(K, 2, 3), boxes[:, 6:12].reshape(K, 2, 3)
        return moved

    # ---- merge ----------------------------------------------------------------------------------------------------------------
    def _merge_weight(self, who, what, w):
        """a scalar weight: a finite number > 0"""
        if isinstance(w, bool) or not isinstance(w, (int, float)):
            raise TypeError("%s: %s must be a number, got %s" % (who, what, type(w).__name__))
        if not (0.0 < float(w) < math.inf):
            raise ValueError("%s: %s must be finite and > 0, got %r" % (who, what, w))
        return float(w)

    def merge(self, other, weight=1.0, other_weight=1.0, max_weight=None, reset_gap=None, band=None, return_names=None):
        """What have I seen so far?  This field (the older one, the memory) and `other` (the newer observation) on the same grid merged into
        one (d3f_volume_merge_select / d3f_volume_merge_rows, csrc/merge_kernels.hip, declared by include/d3fields_hip_ext.h; DESIGN.md
        section 30) -> a new BakedField.  What only one of them knows is kept, what both know is averaged by their weights -- the running
        weighted average of a truncated distance volume, extended to the channel rows -- and where their distances differ by more than
        reset_gap the newer one wins:

            memory = a
            for b in later_bakes:
                pm        = b_prev.flow(...).motions(...)
                predicted = memory.warp(pm, owners, which=...)
                memory    = predicted.merge(b)

        other         a BakedField of this grid, dense or banded, its sets float32 or half (half rows are widened exactly; the result is float32)
        weight        this field's weight per voxel where it has no `weight` volume (a merged field has one, and then it is used instead)
        other_weight  a number, or a float32 [nx, ny, nz] tensor (a per-voxel view count, say); left at 1.0 with `other` a merged field: other.weight
        max_weight    the cap of the summed weight (None: no cap): with a cap the memory never outweighs a new frame by more than max_weight : w
        reset_gap     a world length in dist's units (None: never): both usable and |dist - other.dist| > reset_gap -> the voxel is `other`'s
        band          None: the result is dense iff both fields are dense, else banded with self.band or, this field being dense, other.band;
                      a world length: the result is banded with it
        return_names  the sets of the result (None: the names both fields hold); each must have equal channels on both sides
        A voxel is usable on a side iff it is valid there, its dist is not NaN and its weight is finite and > 0.  Rows: both fields have one
        -> a + beta * (b - a) per channel with beta = w_b / (w_a + w_b); one has -> that row, bit for bit; none (a banded side stores none
        there) -> this field's fill row and rows_known False.  The result also has weight, merged_from and rows_known (see the class).  A
        banded result goes select, d3f_band_mark on the merged dist, the rows of the stored voxels only: no dense row array exists at any
        time.  No host read on the dense path, the one of d3f_band_mark on the banded one.  Not differentiable."""
        if not isinstance(other, BakedField):
            raise TypeError("merge: other must be a BakedField, got %s" % type(other).__name__)
        self._check_same_grid("merge", "other", other)
        if other.device != self.device:
            raise ValueError("merge: other is on %s, the field on %s" % (other.device, self.device))
        if return_names is None:
            return_names = [k for k in self.names() if k in other._sets]
        names = self._names(return_names)
        other._names(names)
        for k in names:
            if self._channels(k) != other._channels(k):
                raise ValueError("merge: set %r has %d channels here and %d in other" % (k, self._channels(k), other._channels(k)))
        mine = getattr(self, "weight", None)
        wa = 1.0 if mine is not None else self._merge_weight("merge", "weight", weight)
        theirs, wb = None, 1.0
        if isinstance(other_weight, torch.Tensor):
            if other_weight.dtype != torch.float32 or tuple(other_weight.shape) != tuple(self.grid_shape):
                raise ValueError("merge: other_weight must be a number or a float32 tensor of shape %s, got %s %s" % (
                    tuple(self.grid_shape), other_weight.dtype, tuple(other_weight.shape)))
            if other_weight.device != self.device:
                raise ValueError("merge: other_weight is on %s, the field on %s" % (other_weight.device, self.device))
            theirs = other_weight.detach().contiguous()
        else:
            wb = self._merge_weight("merge", "other_weight", other_weight)
            if wb == 1.0 and getattr(other, "weight", None) is not None:
                theirs = other.weight
        if max_weight is None:
            max_weight = math.inf
        if isinstance(max_weight, bool) or not isinstance(max_weight, (int, float)):
            raise TypeError("merge: max_weight must be None or a number, got %s" % type(max_weight).__name__)
        if not float(max_weight) > 0.0:
            raise ValueError("merge: max_weight must be > 0 (None or inf: no cap), got %r" % (max_weight,))
        if reset_gap is None:
            reset_gap = math.inf
        if isinstance(reset_gap, bool) or not isinstance(reset_gap, (int, float)):
            raise TypeError("merge: reset_gap must be None or a number, got %s" % type(reset_gap).__name__)
        if not float(reset_gap) >= 0.0:
            raise ValueError("merge: reset_gap must be >= 0 (None or inf: never reset), got %r" % (reset_gap,))
        if band is not None:
            band = _check_band(band, "merge")
        elif self.band is not None or other.band is not None:
            band = self.band if self.band is not None else other.band
        if band is not None:
            _check_band_names(names)
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("merge: the field must live on the ROCm device; there is no CPU path")
        nx, ny, nz = self.grid_shape
        n = nx * ny * nz
        dist = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        wsum = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        beta = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        valid = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
        kind = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
        sel = _lib.MergeSelect(nx, ny, nz, 0, _lib.ptr(self.dist), _lib.ptr(self.valid), _lib.ptr(mine), _lib.ptr(other.dist), _lib.ptr(other.valid),
                               _lib.ptr(theirs), wa, wb, float(max_weight), float(reset_gap), _lib.ptr(dist), _lib.ptr(wsum), _lib.ptr(beta), _lib.ptr(valid),
                               _lib.ptr(kind))
        with self._on() as q:
            q.d3f_volume_merge_select(sel)
        merged = type(self)(self.origin, self.step, dist, valid.view(torch.bool), {}, {}, boundaries=self.boundaries, axes=self._axes)
        if band is None:
            mark, voxels, m = None, None, n
        else:
            mark = merged._mark(band)
            voxels, m = mark[2], mark[2].shape[0]
        known = torch.empty(m, dtype=torch.uint8, device=dev)
        rows = {k: torch.empty((m, self._channels(k)), dtype=torch.float32, device=dev) for k in names}
        if m > 0:
            outs = (ctypes.c_void_p * max(len(names), 1))(*[rows[k].data_ptr() for k in names])
            band_a = None if self.band is None else self._band_struct()
            band_b = None if other.band is None else other._band_struct()
            args = _lib.MergeRows(nx, ny, nz, len(names), None if band_a is None else ctypes.pointer(band_a), None if band_b is None else ctypes.pointer(band_b),
                                  self._set_array(names), other._set_array(names), _lib.ptr(kind), _lib.ptr(beta), _lib.ptr(voxels), m, outs, _lib.ptr(known), 0)
            with self._on() as q:
                q.d3f_volume_merge_rows(args)
        fills = {k: self._fills[k] for k in names}
        if band is None:
            merged._sets, merged._fills = {k: rows[k].view(nx, ny, nz, -1) for k in names}, fills
            merged.rows_known = known.view(torch.bool).view(nx, ny, nz)
        else:
            merged = merged._banded(band, mark, rows, fills)
            merged.rows_known = known.view(torch.bool)
        merged.weight, merged.merged_from = wsum, kind
        return merged

    def components(self, iso=0.0, unknown="free", connectivity=26, min_voxels=1, sites=None, links=None):
        """The connected components of the occupied voxels (d3f_volume_components) -> Components.

        sites         the mask of clearance(): valid & (dist <= iso), plus the invalid voxels for unknown="occupied"; or an explicit
                      bool / uint8 [nx, ny, nz] volume on this device (non-zero = site; iso and unknown must then keep their defaults)
        connectivity  6, 18 or 26: two sites are neighbours if they differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1
        min_voxels    components with fewer voxels are dropped: their voxels get label 0 and the kept ones are numbered 1..count in
                      ascending order of their root, the smallest flat index
        links         None, or a uint16 [nx, ny, nz] link volume (links(), possibly ANDed with the caller's own criteria): two neighbouring sites
                      are then united only if the higher one's bit for that offset is set (d3f_volume_components_linked); a bit that points
                      outside the volume or at a non-site is ignored
        Exact and reproducible: integer data, the same bytes on every run.  Works on a dense, a banded and a clearance field."""
        self._check_ccl("components", connectivity, min_voxels)
        mask = self._site_mask("components", iso, unknown, sites)
        if links is not None:
            links = self._check_links("components", links)
        labels, kept, found, stats = self._label(mask, connectivity, min_voxels, links=links)
        return Components(self.origin, self.step, labels, kept, found, stats, mask, connectivity, min_voxels)

    # ---- pooling --------------------------------------------------------------------------------------------------------------
    def pool(self, components, return_names=None, votes=(), count=None):
        """Pool the field over the voxels of every component in one call (d3f_volume_pool) -> a dict of tensors on the device.

        components    a Components of this field's grid (components()), or an int32 [nx, ny, nz] label volume on this device together with
                      count=K: label k in 1..K names component k, any other value belongs to none
        return_names  the sets whose MEAN row every component gets (None: every baked set); votes: the sets (at most 256 channels) whose
                      rows also cast a hard vote -- one per member, for the first channel that holds the row's maximum
        A voxel is a member of its component if it is valid and, on a banded field, stored: a banded field pools exactly its rows.
          'count'       int32 [K] members;  'moments' int64 [K, 9]: the sums of x, y, z, xx, xy, xz, yy, yz, zz over the members' voxel coordinates
          'centroid'    float32 [K, 3] = origin + step * sum / count;  'covariance' float32 [K, 3, 3]: the population covariance of the member
                        voxel centres in world units, in float64 from the integer moments (torch.linalg.eigh gives the principal axes)
          name          float32 [K, C]: the members' rows summed in ascending flat index, in chunks of 256 (a fixed tree of float32 adds),
                        divided by the count;  name + '_votes': int32 [K, C]
        A component without members has count 0, NaN rows in 'centroid' and 'covariance', the set's fill row as its mean and no votes.
        Reproducible: the same bytes on every run.  One host read (the member capacity).  No autograd: outputs never require grad.
        A clearance field has no sets: it returns the count and the geometry."""
        dev = self.device
        nx, ny, nz = self.grid_shape
        if isinstance(components, Components):
            if count is not None:
                raise ValueError("pool: count comes with a label tensor; a Components knows its own")
            if tuple(components.grid_shape) != tuple(self.grid_shape):
                raise ValueError("pool: the components are of a grid %s, the field of %s" % (tuple(components.grid_shape), tuple(self.grid_shape)))
            labels, K = components.labels, components.count
        elif isinstance(components, torch.Tensor):
            if count is None or isinstance(count, bool) or not isinstance(count, int) or count < 0:
                raise ValueError("pool: a label tensor needs count=K, an integer >= 0, got %r" % (count,))
            if components.dtype != torch.int32 or tuple(components.shape) != tuple(self.grid_shape):
                raise ValueError("pool: labels must be an int32 tensor of shape %s, got %s %s" % (tuple(self.grid_shape), components.dtype, tuple(components.shape)))
            labels, K = components.detach(), count
        else:
            raise ValueError("pool: components must be a Components or an int32 label tensor, got %r" % type(components).__name__)
        if labels.device != dev:
            raise RuntimeError("pool: the labels are on %s, the field on %s" % (labels.device, dev))
        if K > nx * ny * nz:
            raise ValueError("pool: count = %d exceeds the %d voxels" % (K, nx * ny * nz))
        names, voted = self._names(return_names), self._names(list(votes))
        self._need_float_rows("pool", names + voted)
        wide = [k for k in voted if self._channels(k) > _lib.POOL_MAX_VOTE_CHANNELS]
        if wide:
            raise ValueError("pool: votes over %s: more than %d channels" % (wide, _lib.POOL_MAX_VOTE_CHANNELS))
        keys = _POOL_KEYS + tuple(k + "_votes" for k in voted)
        clash = [k for k in names if k in keys]
        if clash:
            raise ValueError("pool: the set(s) %s carry the name of an output key %s" % (clash, keys))
        if len(names) + len(voted) > _lib.MAX_MAPS:
            raise ValueError("pool: at most %d means and votes per call" % _lib.MAX_MAPS)
        labels = labels.contiguous()
        out = {"count": torch.empty(K, dtype=torch.int32, device=dev), "moments": torch.empty((K, 9), dtype=torch.int64, device=dev)}
        for k in names:
            out[k] = torch.empty((K, self._channels(k)), dtype=torch.float32, device=dev)
        for k in voted:
            out[k + "_votes"] = torch.empty((K, self._channels(k)), dtype=torch.int32, device=dev)
        no_rows = self.band is not None and self.band_voxels.shape[0] == 0      # an empty band has no row arrays to point at, and no members
        call = [] if no_rows else [(k, _lib.POOL_MEAN, out[k]) for k in names] + [(k, _lib.POOL_VOTES, out[k + "_votes"]) for k in voted]
        sets = self._set_array([k for k, _, _ in call])
        modes = (ctypes.c_int32 * max(len(call), 1))(*[m for _, m, _ in call])
        rows = (ctypes.c_void_p * max(len(call), 1))(*[t.data_ptr() for _, _, t in call])
        capacity = int((labels > 0).sum())
        members = torch.empty(1, dtype=torch.int64, device=dev)
        mean_channels = sum(self._channels(k) for k, m, _ in call if m == _lib.POOL_MEAN)
        valid = self.valid.contiguous().view(torch.uint8)
        with self._on() as q:
            ws, ws_bytes = q.workspace("d3f_volume_pool_workspace_bytes", nx, ny, nz, K, capacity, mean_channels)
            if K > 0:                                                    # (no component: every output is empty, there is nothing to point at)
                q.d3f_volume_pool(labels, nx, ny, nz, K, valid, self.slot, sets, len(call), modes, capacity, members, out["count"], out["moments"], rows, ws,
                                  ws_bytes)
        if no_rows:
            for k in names:
                out[k] = self.fill_row(k).expand(K, -1).contiguous()
            for k in voted:
                out[k + "_votes"].zero_()
        m = out["moments"].to(torch.float64)
        n = out["count"].to(torch.float64)[:, None]
        mean = m[:, 0:3] / n                                         # 0 / 0 = NaN for a component without members
        second = m[:, [3, 4, 5, 4, 6, 7, 5, 7, 8]].view(K, 3, 3) / n[:, :, None]
        origin = torch.tensor(self.origin, dtype=torch.float64, device=dev)
        out["centroid"] = (origin + self.step * mean).to(torch.float32)
        out["covariance"] = ((second - mean[:, :, None] * mean[:, None, :]) * (self.step * self.step)).to(torch.float32)
        return out

    def clearance(self, iso=0.0, unknown="free", signed=False, max_distance=None, sites=None, min_voxels=1, connectivity=26):
        """The exact Euclidean distance from every voxel centre to the centre of the nearest SITE, as a new field (d3f_volume_edt).

        sites         valid & (dist <= iso) (iso rounded to float32, as dist is stored); unknown="occupied" makes every invalid voxel a
                      site too -- the conservative reading of "never observed"; unknown="free" (default) ignores them.
        max_distance  a world length or None: max_d2 = floor((max_distance / step)^2) caps the squared voxel distance (and bounds the
                      search); the clamp value of dist is therefore step * sqrt(max_d2) <= max_distance.  Rejected if max_d2 would be 0.
        signed        a second transform on the complement: a site voxel gets MINUS the distance to the nearest non-site voxel, and
                      its nearest_voxel / d2 are that voxel's.  Distances are centre to centre, so dist steps from +step to -step
                      across the boundary and is never in between; the source's own dist is the sub-voxel truth inside its shell.

        -> a BakedField (origin, step, boundaries of this one, no sets) with dist float32, d2 int32 (squared voxel distance, capped),
        nearest_voxel int32 (flat index of the nearest site, -1: none within the cap), sites bool; valid = d2 != INT32_MAX: a volume
        without sites is invalid everywhere, with max_distance every voxel is valid, so eval never blends an inf.  eval(pts)['dist']
        is the trilinear clearance and its gradient points away from the obstacle.  Works on a dense or a banded field.

        sites         an explicit bool / uint8 [nx, ny, nz] volume instead of that mask (iso and unknown must keep their defaults).
        min_voxels    > 1: the site mask first goes through components(connectivity=, min_voxels=) and only the voxels of kept
                      components stay sites -- floaters of a few voxels no longer cast a phantom obstacle; with signed=True this
                      happens before both transforms.  With the default 1 no labelling runs."""
        self._check_ccl("clearance", connectivity, min_voxels)
        sites = self._site_mask("clearance", iso, unknown, sites)
        max_d2 = 0
        if max_distance is not None:
            max_distance = float(max_distance)
            if not (math.isfinite(max_distance) and max_distance > 0.0):
                raise ValueError("clearance: max_distance must be a finite length > 0, got %r" % max_distance)
            max_d2 = min(math.floor((max_distance / self.step) ** 2), 2 ** 31 - 2)
            if max_d2 < 1:
                raise ValueError("clearance: max_distance = %g is less than one step (%g)" % (max_distance, self.step))
        if min_voxels > 1:
            sites = self._label(sites, connectivity, min_voxels, want_stats=False)[0] > 0
        d2, nearest, dist = self._edt(sites, max_d2)
        if signed:
            d2_in, nearest_in, dist_in = self._edt(~sites, max_d2)
            d2, nearest, dist = torch.where(sites, d2_in, d2), torch.where(sites, nearest_in, nearest), torch.where(sites, -dist_in, dist)
        c = type(self)(self.origin, self.step, dist, d2 != 2 ** 31 - 1, {}, {}, boundaries=self.boundaries, axes=self._axes)
        c.d2, c.nearest_voxel, c.sites = d2, nearest, sites
        return c

    def nearest_site(self, pts):
        """The site nearest to the voxel each point falls into (a clearance field only).  A point is rounded to its nearest voxel
        (g = (p - origin) / step in float64, half away from zero) and clipped to the lattice; it counts as inside while every
        -0.5 <= g_a <= n_a - 0.5 (the box of the voxels' own cubes).
        -> {'voxel': int64 [N] flat index of the site (-1: the point is outside or holds a NaN, or no site within the cap),
            'points': float32 [N,3] the centre of that site (a NaN row where voxel is -1), 'valid_mask': bool [N]}.
        Plain torch indexing: not a hot path."""
        if self.nearest_voxel is None:
            raise ValueError("nearest_site: this is not a clearance field; BakedField.clearance() makes one")
        _check_points(pts, self.device, "BakedField.eval")
        inside, flat = _voxel_of(pts, self.origin, self.step, self.grid_shape)
        voxel = torch.where(inside, self.nearest_voxel.view(-1)[flat].long(), torch.full_like(flat, -1))
        ok = voxel >= 0
        centres = self._voxel_centres(torch.clamp(voxel, min=0))
        return {"voxel": voxel, "points": torch.where(ok[:, None], centres, torch.full_like(centres, float("nan"))), "valid_mask": ok}

    # ---- travel ---------------------------------------------------------------------------------------------------------------
    _TRAVEL_FIRST_ROUNDS, _TRAVEL_MAX_ROUNDS = 16, 256      # rounds per d3f_volume_geodesic_relax call: 16 first, doubling up to 256

    def _voxel_indices(self, who, what, t):
        """int32 [N] flat voxel indices of float32 [N, 3] points (the one voxel rule, _voxel_of) or of an int32 / int64 index tensor; -1
        for a point outside or with a NaN and for an index outside the volume"""
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor of float32 [N, 3] points or of int32 / int64 flat voxel indices" % (who, what))
        if t.device != self.device:
            raise RuntimeError("%s: %s is on %s, the field on %s" % (who, what, t.device, self.device))
        nx, ny, nz = self.grid_shape
        if t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3:
            inside, flat = _voxel_of(t, self.origin, self.step, self.grid_shape)
        elif t.dtype in (torch.int32, torch.int64) and t.dim() == 1:
            flat = t.detach().long()
            inside = (flat >= 0) & (flat < nx * ny * nz)
        else:
            raise ValueError("%s: %s must be float32 [N, 3] points or a 1-D int32 / int64 tensor of flat voxel indices, got %s %s"
                             % (who, what, t.dtype, tuple(t.shape)))
        return torch.where(inside, flat, torch.full_like(flat, -1)).to(torch.int32).contiguous()

    def travel(self, goals, radius=None, free=None, connectivity=26, weights=(3, 4, 5), penalty=None, max_distance=None):
        """The cost-to-go field of a goal set: in every free voxel the cost of the cheapest lattice path to the nearest goal and the
        neighbour to step to next (d3f_volume_geodesic_init / _relax / _finish), as a new field.

        goals         float32 [G, 3] points on the device (rounded to their voxel as nearest_site does; points outside or with a NaN are
                      dropped), or an int32 / int64 tensor of flat voxel indices.  A goal on a non-free voxel is ignored.
        radius        (a clearance field only) free = valid & (dist >= radius): the voxels a body of that radius fits into.
        free          or an explicit bool / uint8 [nx, ny, nz] volume on this device (non-zero = traversable).  Exactly one of the two.
        connectivity  6, 18 or 26: a move joins two free voxels that differ by at most 1 on every axis and by at most 1 / 2 / 3 in L1.
        weights       (w1, w2, w3), integers with 1 <= w1 <= w2 <= w3 <= 255: the cost of a face / edge / corner move.  The default
                      (3, 4, 5) under connectivity 26 keeps cost / (3 * Euclidean voxel distance) inside [0.9428, 1.1055] in open space.
        penalty       None, or an int32 [nx, ny, nz] volume on this device, >= 0, added to the cost of every move INTO a voxel (negative
                      entries count as 0; a goal's own penalty is never charged).
        max_distance  a world length or None: max_cost = floor(max_distance * w1 / step) caps the cost; voxels beyond it stay unreached.
                      Rejected if max_cost would be below 1.

        -> a BakedField (origin, step, boundaries of this one, no sets) with dist float32 = cost * (step / w1) (+inf where unreached),
        cost int32 (INT32_MAX where unreached), next_voxel int32, free bool; valid = cost != INT32_MAX, so eval never blends an inf: a cell
        with an unreached corner is "not valid".  eval(pts)['dist'] is the trilinear travel distance and its negative gradient points
        along the way to the goal, without local minima; path(starts) gives the discrete route.
        Exact and reproducible: integer costs, the unique fixed point of the relaxation, the same bytes on every run.  One host read per
        batch of rounds.  No autograd: outputs never require grad."""
        who = "travel"
        dev = self.device
        nx, ny, nz = self.grid_shape
        n = nx * ny * nz
        if connectivity not in (6, 18, 26):
            raise ValueError("travel: connectivity must be 6, 18 or 26, got %r" % (connectivity,))
        try:
            w = tuple(weights)
        except TypeError:
            raise ValueError("travel: weights must be three integers, got %r" % (weights,))
        if len(w) != 3 or any(isinstance(x, bool) or not isinstance(x, int) for x in w) or not 1 <= w[0] <= w[1] <= w[2] <= 255:
            raise ValueError("travel: weights must be integers with 1 <= w1 <= w2 <= w3 <= 255, got %r" % (weights,))
        if (radius is None) == (free is None):
            raise ValueError("travel: give exactly one of radius= (on a clearance field) and free=")
        if radius is not None:
            if self.nearest_voxel is None:
                raise ValueError("travel: radius needs a clearance field (BakedField.clearance()); pass free= on any other field")
            radius = float(radius)
            if not math.isfinite(radius):
                raise ValueError("travel: radius must be finite, got %r" % radius)
            mask = self.valid & (self.dist >= radius)
        else:
            mask = self._site_mask(who, 0.0, "free", free)
        if penalty is not None:
            if not isinstance(penalty, torch.Tensor) or penalty.dtype != torch.int32 or tuple(penalty.shape) != tuple(self.grid_shape):
                raise ValueError("travel: penalty must be an int32 tensor of shape %s" % (tuple(self.grid_shape),))
            if penalty.device != dev:
                raise RuntimeError("travel: penalty is on %s, the field on %s" % (penalty.device, dev))
            penalty = penalty.detach().contiguous()
        max_cost = 2 ** 31 - 2
        if max_distance is not None:
            max_distance = float(max_distance)
            if not (math.isfinite(max_distance) and max_distance > 0.0):
                raise ValueError("travel: max_distance must be a finite length > 0, got %r" % max_distance)
            max_cost = min(math.floor(max_distance * w[0] / self.step), 2 ** 31 - 2)
            if max_cost < 1:
                raise ValueError("travel: max_distance = %g allows no move (step / w1 = %g)" % (max_distance, self.step / w[0]))
        seeds = self._voxel_indices(who, "goals", goals)
        seeds = seeds[seeds >= 0].contiguous()
        mask = mask.contiguous()
        site = mask.view(torch.uint8)
        cost = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        nxt = torch.empty((nx, ny, nz), dtype=torch.int32, device=dev)
        dist = torch.empty((nx, ny, nz), dtype=torch.float32, device=dev)
        pending = torch.empty(1, dtype=torch.int32, device=dev)
        warr = (ctypes.c_int32 * 3)(*w)
        with self._on() as q:
            ws, ws_bytes = q.workspace("d3f_volume_geodesic_workspace_bytes", nx, ny, nz)
            q.d3f_volume_geodesic_init(site, nx, ny, nz, seeds, seeds.shape[0], cost, ws, ws_bytes)
            rounds, total = self._TRAVEL_FIRST_ROUNDS, 0
            while True:
                q.d3f_volume_geodesic_relax(site, penalty, nx, ny, nz, connectivity, warr, max_cost, rounds, cost, pending, ws, ws_bytes)
                total += rounds
                if int(pending.item()) == 0:
                    break
                if total > n:      # after k rounds every voxel whose cheapest path has at most k moves is final: never reached
                    raise RuntimeError("travel: the relaxation did not settle within %d rounds" % total)
                rounds = min(2 * rounds, self._TRAVEL_MAX_ROUNDS)
            q.d3f_volume_geodesic_finish(site, penalty, nx, ny, nz, connectivity, warr, self.step, cost, nxt, dist)
        t = type(self)(self.origin, self.step, dist, cost != 2 ** 31 - 1, {}, {}, boundaries=self.boundaries, axes=self._axes)
        t.cost, t.next_voxel, t.free = cost, nxt, mask
        return t

    def path(self, starts, max_steps=None):
        """The discrete route from each start to its goal: a pointer walk along next_voxel (a travel field only; d3f_volume_follow).

        starts     float32 [N, 3] points (rounded to their voxel; outside or NaN: an empty path) or an int32 / int64 tensor of flat indices
        max_steps  the row length L (default nx + ny + nz); a path cut by it has reached = False and a full row
        -> {'voxels': int32 [N, L] the visited flat indices, the start voxel first, padded with -1; 'length': int32 [N]; 'reached': bool [N]
            (the walk arrived at a goal); 'points': float32 [N, L, 3] the voxel centres, NaN rows for the padding}.
        An unreached start (not valid on this field) has length 0 and reached = False.  No autograd: outputs never require grad."""
        if self.next_voxel is None:
            raise ValueError("path: this is not a travel field; BakedField.travel() makes one")
        dev = self.device
        nx, ny, nz = self.grid_shape
        if max_steps is None:
            max_steps = nx + ny + nz
        if isinstance(max_steps, bool) or not isinstance(max_steps, int) or not 1 <= max_steps <= 2 ** 31 - 1:
            raise ValueError("path: max_steps must be an integer >= 1, got %r" % (max_steps,))
        s = self._voxel_indices("path", "starts", starts)
        N = s.shape[0]
        voxels = torch.empty((N, max_steps), dtype=torch.int32, device=dev)
        length = torch.empty(N, dtype=torch.int32, device=dev)
        reached = torch.empty(N, dtype=torch.bool, device=dev)
        with self._on() as q:
            q.d3f_volume_follow(self.next_voxel, nx * ny * nz, s, N, max_steps, voxels, length, reached)
        flat = voxels.view(-1)
        centres = self._voxel_centres(torch.clamp(flat, min=0))
        points = torch.where((flat >= 0)[:, None], centres, torch.full_like(centres, float("nan"))).view(N, max_steps, 3)
        return {"voxels": voxels, "length": length, "reached": reached, "points": points}

    # ---- straight segments ------------------------------------------------------------------------------------------------------
    def _segment_free(self, who, radius, free):
        """the bool free volume of straight: radius on a clearance field, free= anywhere, a travel field's own free by default"""
        if radius is not None and free is not None:
            raise ValueError("%s: give radius= (on a clearance field) or free=, not both" % who)
        if radius is not None:
            if self.nearest_voxel is None:
                raise ValueError("%s: radius needs a clearance field (BakedField.clearance()); pass free= on any other field" % who)
            radius = float(radius)
            if not math.isfinite(radius):
                raise ValueError("%s: radius must be finite, got %r" % (who, radius))
            return self.valid & (self.dist >= radius)
        if free is not None:
            return self._site_mask(who, 0.0, "free", free)
        if self.free is None:
            raise ValueError("%s: give radius= (on a clearance field) or free=; only a travel field has a free volume of its own" % who)
        return self.free

    def _points_or_nan(self, voxel):
        """float32 [..., 3] centres of int32 flat indices, NaN rows for -1"""
        flat = voxel.reshape(-1)
        centres = self._voxel_centres(torch.clamp(flat, min=0))
        return torch.where((flat >= 0)[:, None], centres, torch.full_like(centres, float("nan"))).view(tuple(voxel.shape) + (3,))

    def straight(self, a, b, radius=None, free=None, cut_corners=False):
        """Can I go straight?  The grid segment between the voxels of a and b against a free volume (d3f_volume_segments).

        a, b         float32 [N, 3] points (rounded to their voxel; outside or NaN: not clear) or int32 / int64 tensors of flat indices; one of
                     them may have a single row and is then broadcast.
        radius       (a clearance field only) free = valid & (dist >= radius);  free  or an explicit bool / uint8 [nx, ny, nz] volume.  At
                     most one of the two; with neither, a travel field uses its own free volume and any other field raises.
        cut_corners  False (default): a voxel is touched when its closed cube meets the segment, so a segment through a lattice edge or
                     corner also needs the cubes round that point; True: the open cube, under which every move of path() is clear.
        -> {'clear': bool [N]; 'last_voxel': int32 [N] the last voxel reached before the first blocked one (b itself if clear, -1 if a is
            blocked or an end lies outside); 'blocked_voxel': int32 [N] (-1 if clear); 'points': float32 [N, 3] the centre of last_voxel, a
            NaN row for -1}, and on a clearance field also 'min_d2': int32 [N] the smallest d2 over the voxels touched before the blocked
            one (INT32_MAX: none), 'min_voxel': int32 [N] where it is, 'clearance': float32 [N] = float32(step * sqrt(float64(min_d2))),
            inf where none -- how narrow it gets on the way.
        Integer-exact, the same bytes on every run.  No autograd: outputs never require grad."""
        who = "straight"
        dev = self.device
        nx, ny, nz = self.grid_shape
        mask = self._segment_free(who, radius, free).contiguous()
        va, vb = self._voxel_indices(who, "a", a), self._voxel_indices(who, "b", b)
        if va.shape[0] != vb.shape[0]:
            if va.shape[0] == 1:
                va = va.expand(vb.shape[0]).contiguous()
            elif vb.shape[0] == 1:
                vb = vb.expand(va.shape[0]).contiguous()
            else:
                raise ValueError("straight: a has %d rows and b %d; they must agree, or one of them have a single row" % (va.shape[0], vb.shape[0]))
        N = va.shape[0]
        value = self.d2.contiguous() if self.d2 is not None else None
        clear = torch.empty(N, dtype=torch.bool, device=dev)
        last = torch.empty(N, dtype=torch.int32, device=dev)
        blocked = torch.empty(N, dtype=torch.int32, device=dev)
        min_d2 = torch.empty(N, dtype=torch.int32, device=dev) if value is not None else None
        min_voxel = torch.empty(N, dtype=torch.int32, device=dev) if value is not None else None
        flags = _lib.SEGMENT_CUT_CORNERS if cut_corners else 0
        if N > 0:                                      # (an empty tensor has no address: nothing to ask)
            with self._on() as q:
                q.d3f_volume_segments(mask.view(torch.uint8), value, nx, ny, nz, va, vb, N, flags, clear, last, blocked, min_d2, min_voxel)
        out = {"clear": clear, "last_voxel": last, "blocked_voxel": blocked, "points": self._points_or_nan(last)}
        if value is not None:
            world = (torch.sqrt(min_d2.double()) * self.step).float()
            out.update({"min_d2": min_d2, "min_voxel": min_voxel,
                        "clearance": torch.where(min_d2 == 2 ** 31 - 1, torch.full_like(world, float("inf")), world)})
        return out

    def _row_lengths(self, voxels, keep):
        """float64 [N]: the summed Euclidean voxel distances between the consecutive kept entries of each row (keep bool [N, L] marks a
        prefix of every row)"""
        nx, ny, nz = self.grid_shape
        q = torch.clamp(voxels.long(), min=0)
        xyz = torch.stack((q // (ny * nz), (q // nz) % ny, q % nz), dim=2)
        d = xyz[:, 1:] - xyz[:, :-1]
        hop = torch.sqrt((d * d).sum(dim=2).double())
        return torch.where(keep[:, 1:], hop, torch.zeros_like(hop)).sum(dim=1)

    def shortcut(self, paths, cut_corners=False, max_span=None):
        """Keep only the waypoints of a route that cannot be skipped (a travel field only; d3f_path_shorten): from each kept
        waypoint the route jumps to the farthest later one, at most max_span entries ahead, that it can reach by a clear straight segment
        through this field's free volume, and to the next one if there is none.

        paths        the dict path() returns ('voxels' int32 [N, L], 'length' int32 [N], 'reached'), or anything path() takes as starts
        cut_corners  as in straight().  Under the default strict rule an edge or corner move of the route whose side voxels are not all
                     free is not clear; it is kept all the same.
        max_span     how many entries ahead a jump may look (default: the row length L, no limit); any integer type
        -> {'voxels': int32 [N, L] the kept waypoints, padded with -1; 'index': int32 [N, L] their positions in the input row, padded
            with -1; 'length': int32 [N]; 'reached': passed through; 'points': float32 [N, L, 3], NaN rows for the padding; 'distance',
            'distance_before': float64 [N] = step times the summed Euclidean voxel distances between consecutive kept waypoints / between
            consecutive voxels of the input row}.
        A row made by hand may hold entries outside the volume inside its length (path() never writes one): they are kept as waypoints and
        never jumped to, but the two distances then mean nothing for that row -- such an entry is measured as if it were voxel 0.
        Integer-exact, the same bytes on every run.  No autograd: outputs never require grad."""
        if self.next_voxel is None:
            raise ValueError("shortcut: this is not a travel field; BakedField.travel() makes one")
        if not isinstance(paths, dict):
            paths = self.path(paths)
        dev = self.device
        nx, ny, nz = self.grid_shape
        if not all(k in paths for k in ("voxels", "length", "reached")):
            raise ValueError("shortcut: paths must be the dict path() returns, with 'voxels', 'length' and 'reached'")
        rows, length = paths["voxels"], paths["length"]
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] < 1:
            raise ValueError("shortcut: paths['voxels'] must be an int32 [N, L] tensor with L >= 1")
        if not isinstance(length, torch.Tensor) or length.dtype != torch.int32 or tuple(length.shape) != (rows.shape[0],):
            raise ValueError("shortcut: paths['length'] must be an int32 [N] tensor")
        for what, t in (("voxels", rows), ("length", length)):
            if t.device != dev:
                raise RuntimeError("shortcut: paths['%s'] is on %s, the field on %s" % (what, t.device, dev))
        N, L = rows.shape
        if max_span is None:
            max_span = L
        try:                                           # any integer type (a NumPy integer, a 0-d integer tensor); not a bool, not a float
            span = None if isinstance(max_span, bool) else operator.index(max_span)
        except TypeError:
            span = None
        if span is None or not 1 <= span <= 2 ** 31 - 1:
            raise ValueError("shortcut: max_span must be an integer >= 1, got %r" % (max_span,))
        max_span = span
        rows, length = rows.detach().contiguous(), length.detach().contiguous()
        mask = self.free.contiguous()
        voxels = torch.empty((N, L), dtype=torch.int32, device=dev)
        index = torch.empty((N, L), dtype=torch.int32, device=dev)
        count = torch.empty(N, dtype=torch.int32, device=dev)
        flags = _lib.SEGMENT_CUT_CORNERS if cut_corners else 0
        if N > 0:
            with self._on() as q:
                q.d3f_path_shorten(mask.view(torch.uint8), nx, ny, nz, rows, length, N, L, max_span, flags, index, voxels, count)
        at = torch.arange(L, device=dev)[None, :]
        return {"voxels": voxels, "index": index, "length": count, "reached": paths["reached"], "points": self._points_or_nan(voxels),
                "distance": self._row_lengths(voxels, at < count[:, None]) * self.step,
                "distance_before": self._row_lengths(rows, at < torch.clamp(length, 0, L)[:, None]) * self.step}

    # ---- peaks ----------------------------------------------------------------------------------------------------------------
    def _peak_radius(self, who, radius_voxels, separation):
        """r of peaks / locate from exactly one of radius_voxels and separation (a world length: r = max(1, ceil(separation / step) - 1)
        in float64, so that two peaks lie at least `separation` apart along some axis)"""
        if (radius_voxels is None) == (separation is None):
            raise ValueError("%s: give exactly one of radius_voxels and separation" % who)
        if separation is not None:
            sep = float(separation)
            if not (sep > 0.0 and math.isfinite(sep)):
                raise ValueError("%s: separation must be a finite length > 0, got %r" % (who, separation))
            r = max(1, int(math.ceil(sep / self.step)) - 1)
        else:
            try:
                r = None if isinstance(radius_voxels, bool) else operator.index(radius_voxels)
            except TypeError:
                r = None
            if r is None or r < 1:
                raise ValueError("%s: radius_voxels must be an integer >= 1, got %r" % (who, radius_voxels))
        if r > _lib.PEAKS_MAX_RADIUS:
            raise ValueError("%s: a suppression radius of %d voxels is not built; the largest is %d (separation <= %g at this step)"
                             % (who, r, _lib.PEAKS_MAX_RADIUS, (_lib.PEAKS_MAX_RADIUS + 1) * self.step))
        return r

    def _peak_mask(self, who, mask):
        if mask is None:
            return None
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(self.grid_shape) or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("%s: mask must be a bool or uint8 tensor of shape %s" % (who, tuple(self.grid_shape)))
        if mask.device != self.device:
            raise RuntimeError("%s: mask is on %s, the field on %s" % (who, mask.device, self.device))
        return mask.detach().contiguous().view(torch.uint8)

    @staticmethod
    def _peak_k(who, k):
        try:
            kk = None if isinstance(k, bool) else operator.index(k)
        except TypeError:
            kk = None
        if kk is None or not 1 <= kk <= 8:
            raise ValueError("%s: k must be an integer in 1..8 (more is not built), got %r" % (who, k))
        return kk

    def _peaks_rows(self, work, rows_banded, r, k, threshold, mask, refine):
        """peaks of the columns of work float32 [M, K] (contiguous; minima): d3f_volume_peaks, d3f_topk_smallest, the rows' voxels, and the
        refinement -> (voxel int32 [K, k], value float32 [K, k], count int32 [K], offset float64 [K, k, 3] in voxel units or None)"""
        dev = self.device
        nx, ny, nz = self.grid_shape
        M, K = work.shape
        if K == 0:                                     # no column: nothing is launched
            return (torch.empty((0, k), dtype=torch.int32, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev), torch.empty((0, k, 3), dtype=torch.float64, device=dev) if refine else None)
        slot = self.slot if rows_banded else None
        sup = torch.empty((M, K), dtype=torch.float32, device=dev)
        # (d3f_volume_peaks zeroes the counts itself before it adds to them; without rows it is not called)
        count = torch.empty(K, dtype=torch.int32, device=dev) if M > 0 else torch.zeros(K, dtype=torch.int32, device=dev)
        if M > 0:                                      # (d3f_topk_smallest writes every entry: -1 / NaN where there are fewer than k rows)
            idx, val = torch.empty((k, K), dtype=torch.int64, device=dev), torch.empty((k, K), dtype=torch.float32, device=dev)
        else:
            idx = torch.full((k, K), -1, dtype=torch.int64, device=dev)
            val = torch.full((k, K), float("inf"), dtype=torch.float32, device=dev)
        if M > 0:                                      # (an empty tensor has no address: nothing to ask)
            with self._on() as q:
                ws, ws_bytes = q.workspace("d3f_pairwise_topk_workspace_bytes", M, K)
                q.d3f_volume_peaks(slot, mask, nx, ny, nz, work, M, K, K, r, threshold, sup, K, count, None, 0)
                q.d3f_topk_smallest(sup, M, K, k, idx, val, ws, ws_bytes)
        idx, val = idx.t().contiguous(), val.t().contiguous()
        hit = (idx >= 0) & (val < float("inf"))       # fewer than k peaks: the list goes on with rows that hold +Inf (or, with M < k, none)
        row = torch.where(hit, idx, torch.zeros_like(idx))
        value = torch.where(hit, val, torch.full_like(val, float("inf")))
        if M == 0:
            flat = row
        else:
            flat = self.band_voxels.long()[row] if rows_banded else row
        voxel = torch.where(hit, flat, torch.full_like(flat, -1)).to(torch.int32)
        offset = None
        if refine:
            offset = self._peak_offsets(work, slot, mask, flat, row, hit)
        return voxel, value, count, offset

    def _peak_offsets(self, work, slot, mask, flat, row, hit):
        """float64 [K, k, 3]: per axis 0.5 (f- - f+) / (f- - 2 f0 + f+) at the hits, clamped to [-0.5, 0.5]; 0 where a neighbour does not take
        part or lies outside the volume, 0 where the denominator is not > 0; NaN rows where `hit` is false.  Plain float64 torch on K*k hits."""
        nx, ny, nz = self.grid_shape
        K, k = flat.shape
        col = torch.arange(K, device=self.device)[:, None].expand(K, k)
        inf = float("inf")
        if work.shape[0] == 0:
            return torch.full((K, k, 3), float("nan"), dtype=torch.float64, device=self.device)
        f0 = work[row, col].double()
        coords = (flat // (ny * nz), (flat // nz) % ny, flat % nz)
        offs = []
        for a, (n, stride) in enumerate(((nx, ny * nz), (ny, nz), (nz, 1))):
            side = []
            for sign in (-1, 1):
                c = coords[a] + sign
                inside = hit & (c >= 0) & (c < n)
                u = torch.where(inside, flat + sign * stride, torch.zeros_like(flat))
                m = u if slot is None else slot.view(-1)[u].long()
                part = inside & (m >= 0)
                if mask is not None:
                    part = part & (mask.view(-1)[u] != 0)
                f = work[torch.clamp(m, min=0), col]
                part = part & (f < inf)
                side.append((f.double(), part))
            (fm, pm), (fp, pp) = side
            den = fm - 2.0 * f0 + fp
            off = torch.clamp(0.5 * (fm - fp) / den, -0.5, 0.5)
            offs.append(torch.where(pm & pp & (den > 0), off, torch.zeros_like(off)))
        out = torch.stack(offs, dim=2)
        return torch.where(hit[..., None], out, torch.full_like(out, float("nan")))

    def _peaks_result(self, key, voxel, value, count, offset, largest):
        points = self._points_or_nan(voxel)
        out = {"voxel": voxel, key: -value if largest else value, "points": points, "count": count}
        if offset is not None:
            out["refined"] = points.double() + offset * self.step
        return out

    def peaks(self, values, radius_voxels=None, separation=None, k=8, threshold=None, largest=False, mask=None, refine=True):
        """Spatially distinct local optima of K value columns: exact, order-independent non-maximum suppression (d3f_volume_peaks,
        csrc/peaks_kernels.hip) and the k best survivors per column (d3f_topk_smallest).

        values         float32 [nx, ny, nz] or [nx, ny, nz, K] on any field; on a banded field also [M] or [M, K], one row per stored voxel
                       (voxels without a row then take no part)
        radius_voxels  the suppression radius r in voxels, 1..8; or  separation  a world length: r = max(1, ceil(separation / step) - 1),
                       so that two peaks lie at least `separation` apart along some axis.  Exactly one of the two; r > 8 is not built.
        k              how many peaks per column to return, 1..8;   threshold   only peaks with value <= threshold (>= under largest)
        largest        False: minima.  True: maxima (the values are negated on the way in and out, which is exact)
        mask           bool / uint8 [nx, ny, nz]: only these voxels take part;   refine   also return sub-voxel positions
        A voxel takes part when it has a row, passes the mask and its value is < +Inf (not NaN, not +Inf; > -Inf under largest).  It is a
        peak when no other voxel that takes part within r on all three axes has a smaller value, or the same value and a lower flat index.
        -> {'voxel': int32 [K, k] flat indices by ascending value (descending under largest), ties to the lower index, padded with -1;
            'value': float32 [K, k], padded with +Inf (-Inf under largest); 'points': float32 [K, k, 3] voxel centres, NaN rows as
            padding; 'count': int32 [K] the number of peaks, which may exceed k; with refine 'refined': float64 [K, k, 3] = the centre +
            step * offset, per axis offset = 0.5 (f- - f+) / (f- - 2 f0 + f+) clamped to [-0.5, 0.5], 0 where a neighbour does not take
            part or lies outside the volume or the denominator is not > 0}.  A [nx, ny, nz] or [M] input is one column: K = 1.
        The same bytes on every run.  No autograd: outputs never require grad."""
        who = "peaks"
        dev = self.device
        nx, ny, nz = self.grid_shape
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32:
            raise TypeError("peaks: values must be a float32 tensor")
        if not values.is_cuda or values.device != dev:
            raise RuntimeError("peaks: values must be on %s (where the volume lives); there is no CPU path" % dev)
        if values.dim() in (3, 4) and tuple(values.shape[:3]) == (nx, ny, nz):
            rows_banded = False
            work = values.detach().reshape(nx * ny * nz, -1)
        elif values.dim() in (1, 2) and self.band is not None and values.shape[0] == self.band_voxels.shape[0]:
            rows_banded = True
            work = values.detach().reshape(values.shape[0], -1)
        else:
            raise ValueError("peaks: values must be [nx, ny, nz] or [nx, ny, nz, K] with the grid %s%s, got %s"
                             % (tuple(self.grid_shape), "" if self.band is None else ", or [M] / [M, K] with M = %d stored voxels" % self.band_voxels.shape[0],
                                tuple(values.shape)))
        r = self._peak_radius(who, radius_voxels, separation)
        k = self._peak_k(who, k)
        mask = self._peak_mask(who, mask)
        thr = float("inf") if threshold is None else (-float(threshold) if largest else float(threshold))
        if math.isnan(thr):
            raise ValueError("peaks: threshold must not be NaN")
        work = (-work if largest else work).contiguous()
        voxel, value, count, offset = self._peaks_rows(work, rows_banded, r, k, thr, mask, refine)
        return self._peaks_result("value", voxel, value, count, offset, largest)

    def locate(self, descriptors, name, k=8, radius_voxels=None, separation=None, max_distance=None, dist_type="l2", mask=None, max_bytes=1 << 30):
        """Where are these descriptors?  For each of K reference descriptors the k best spatially distinct matches among the rows of set
        `name`: the distances of d3f_pairwise_similarity (D3F_SIM_DIST) as a [M, Kc] matrix, then peaks() on it.

        descriptors   float32 [K, C] on the field's device, C the width of `name`
        name          a baked set.  On a dense field its rows are all voxels and mask defaults to `valid`; on a banded field the stored rows
        k, radius_voxels, separation, mask   as in peaks();   max_distance   only matches with distance <= max_distance
        dist_type     "l2" or "square", as in corr_utils
        max_bytes     the columns are taken in chunks so that the distances and the suppressed copy of one chunk stay under this
        -> what peaks() returns, with 'distance' for 'value'; 'refined' interpolates the distances.  No autograd."""
        from .corr_utils import _dist_code
        who = "locate"
        names = self._names([name])
        self._need_float_rows(who, names)
        code = _dist_code(dist_type)
        dev = self.device
        if not isinstance(descriptors, torch.Tensor) or descriptors.dim() != 2:
            raise ValueError("locate: descriptors must be a [K, C] tensor")
        if not descriptors.is_cuda or descriptors.device != dev:
            raise RuntimeError("locate: descriptors must be on %s (where the volume lives); there is no CPU path" % dev)
        C = self._channels(names[0])
        if descriptors.shape[1] != C:
            raise ValueError("locate: descriptors have %d channels, set %r has %d" % (descriptors.shape[1], name, C))
        r = self._peak_radius(who, radius_voxels, separation)
        k = self._peak_k(who, k)
        banded = self.band is not None
        mask = self._peak_mask(who, self.valid if (mask is None and not banded) else mask)
        thr = float("inf") if max_distance is None else float(max_distance)
        if math.isnan(thr):
            raise ValueError("locate: max_distance must not be NaN")
        rows = self._sets[names[0]].reshape(-1, C).contiguous()
        tgt = descriptors.detach().to(torch.float32).contiguous()
        M, K = rows.shape[0], tgt.shape[0]
        per_chunk = K if M == 0 else max(1, min(K, int(max_bytes) // (8 * M)))
        parts = []
        for q0 in range(0, max(K, 1), max(per_chunk, 1)):          # (K = 0: one empty chunk, which launches nothing)
            Kc = min(per_chunk, K - q0)
            dist = torch.empty((M, Kc), dtype=torch.float32, device=dev)
            if M > 0 and Kc > 0:
                with self._on() as q:
                    q.d3f_pairwise_similarity(rows, tgt[q0:q0 + Kc], M, Kc, C, 1.0, code, _lib.SIM_DIST, dist, None, None, 0)
            parts.append(self._peaks_rows(dist, banded, r, k, thr, mask, True))
        voxel, value, count, offset = (torch.cat([p[i] for p in parts], dim=0) for i in range(4))
        return self._peaks_result("distance", voxel, value, count, offset, False)

    # ---- alignment ------------------------------------------------------------------------------------------------------------
    def _align_tensor(self, who, what, t, shape):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
            raise ValueError("%s: %s must be a tensor of shape %s, got %s" % (who, what, list(shape), list(getattr(t, "shape", ())) or type(t).__name__))
        if not t.is_cuda or t.device != self.device:
            raise RuntimeError("%s: %s must be on %s (where the volume lives); there is no CPU path" % (who, what, self.device))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s" % (who, what, t.dtype))
        return t.detach().contiguous()

    def _align_problem(self, who, points, name, targets, dist_targets, weights, dist_weight, feat_weight, outside):
        """the checked, contiguous inputs of one alignment problem and the model centroids (d3f_volume_align_centroid)"""
        self._need_float_rows(who, [] if name is None else [name])
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
            raise ValueError("%s: points must be [I, n, 3], got %s" % (who, list(getattr(points, "shape", ())) or type(points).__name__))
        I, n = int(points.shape[0]), int(points.shape[1])
        pts = self._align_tensor(who, "points", points, (I, n, 3))
        names = self._names([] if name is None else [name])
        if name is None and targets is not None:
            raise ValueError("%s: targets need the name of the set they are descriptors of" % who)
        if name is not None and targets is None:
            raise ValueError("%s: set %r needs targets [I, n, %d]" % (who, name, self._channels(name)))
        tg = None if name is None else self._align_tensor(who, "targets", targets, (I, n, self._channels(name)))
        dt = None if dist_targets is None else self._align_tensor(who, "dist_targets", dist_targets, (I, n))
        wt = None if weights is None else self._align_tensor(who, "weights", weights, (I, n))
        terms = {"dist_weight": float(dist_weight), "feat_weight": float(feat_weight)}
        terms["outside"] = 4.0 * self.step * terms["dist_weight"] if outside is None else float(outside)
        for k, v in terms.items():
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError("%s: %s must be finite and >= 0, got %r" % (who, k, v))
        # (d3f_volume_align_centroid writes every row, zeros where an instance has no weighted finite point; it is not called without points)
        centroid = (torch.empty if I > 0 and n > 0 else torch.zeros)((I, 3), dtype=torch.float32, device=self.device)
        with self._on() as q:
            if I > 0 and n > 0:
                q.d3f_volume_align_centroid(pts, wt, I, n, centroid)
            ws, ws_bytes = q.workspace("d3f_volume_align_workspace_bytes", I, n)
        return {"I": I, "n": n, "pts": pts, "names": names, "targets": tg, "dist_targets": dt, "weights": wt, "terms": terms, "centroid": centroid,
                "ws": ws.view(torch.float64), "ws_bytes": ws_bytes}          # (the kernels keep rows of doubles there)

    def _align_pose(self, who, I, rot, trans):
        """[I, 12] float32: the kernels' R (the TRANSPOSE of the row-vector `rot`) row-major, then t"""
        dev = self.device
        rot = torch.eye(3, dtype=torch.float32, device=dev).expand(I, 3, 3) if rot is None else self._align_tensor(who, "rot", rot, (I, 3, 3))
        trans = torch.zeros((I, 3), dtype=torch.float32, device=dev) if trans is None else self._align_tensor(who, "trans", trans, (I, 3))
        return torch.cat((rot.transpose(1, 2).reshape(I, 9), trans), dim=1).contiguous()

    def _align_accumulate(self, prob, pose, skip, out):
        band = None if self.band is None else self._band_struct()
        sets = self._set_array(prob["names"]) if prob["names"] else None
        t = prob["terms"]
        with self._on() as q:
            q.d3f_volume_align_accumulate(self._volume(), band, sets, prob["pts"], prob["weights"], prob["targets"], prob["dist_targets"], pose, prob["centroid"], skip,
                                          prob["I"], prob["n"], t["dist_weight"], t["feat_weight"], t["outside"], out, prob["ws"], prob["ws_bytes"])

    def normal_equations(self, points, rot, trans, name=None, targets=None, dist_targets=None, weights=None, dist_weight=1.0, feat_weight=1.0, outside=None):
        """The Gauss-Newton normal equations of aligning point sets to this field at given poses (d3f_volume_align_accumulate,
        csrc/align_kernels.hip), for callers with their own solver or their own priors.

        points        float32 [I, n, 3]: I instances of n model points;  weights  float32 [I, n] >= 0 or None (ones; 0 is padding)
        rot, trans    float32 [I, 3, 3] and [I, 3] in rigid.rigid_transform's row-vector convention, x = p @ rot + trans (None: the identity).
                      The kernels' R is the transpose of `rot`.
        name, targets one baked set and float32 [I, n, C] descriptors the points should meet, or None: the distance term alone
        dist_targets  float32 [I, n] distances the points should meet, or None (zeros: the points lie on the surface)
        dist_weight, feat_weight   the weights of the two kinds of residual;  outside  the residual of a weighted point that is not valid
                      (None: 4 * step * dist_weight), which enters the cost and nothing else
        Residuals: dist_weight (dist(x) - d) at every valid point and feat_weight (f_k(x) - s_k) per channel where the point has rows (valid;
        on a banded field in_band).  The parameters are (w, v): x <- c + Exp(w)(x - c) + v about the pivot c, the weighted centroid of the
        transformed points.
        -> {'H': float64 [I, 6, 6] = sum w_j J^T J (symmetric), 'b': float64 [I, 6] = sum w_j J^T r, 'cost': float64 [I] = sum w_j r^2,
            'valid': int32 [I] the weighted points that are valid, 'in_band': int32 [I] those that have rows, 'pivot': float64 [I, 3]}.
        The same bytes on every run.  No autograd: outputs never require grad."""
        who = "normal_equations"
        prob = self._align_problem(who, points, name, targets, dist_targets, weights, dist_weight, feat_weight, outside)
        I, dev = prob["I"], self.device
        pose = self._align_pose(who, I, rot, trans)
        if I > 0 and prob["n"] > 0:
            out = torch.empty((I, _lib.ALIGN_ROW_DOUBLES), dtype=torch.float64, device=dev)      # (without skip the fold writes every row)
            self._align_accumulate(prob, pose, None, out)
        else:
            out = torch.zeros((I, _lib.ALIGN_ROW_DOUBLES), dtype=torch.float64, device=dev)
        iu = torch.triu_indices(6, 6, device=dev)
        H = torch.zeros((I, 6, 6), dtype=torch.float64, device=dev)
        H[:, iu[0], iu[1]] = out[:, :21]
        H[:, iu[1], iu[0]] = out[:, :21]
        m = prob["centroid"]
        pivot = (pose[:, :9].reshape(I, 3, 3).double() @ m.double()[:, :, None])[:, :, 0] + pose[:, 9:].double()
        return {"H": H, "b": out[:, 21:27].clone(), "cost": out[:, 27].clone(), "valid": out[:, 28].to(torch.int32), "in_band": out[:, 29].to(torch.int32),
                "pivot": pivot}

    def align(self, points, name=None, targets=None, rot=None, trans=None, iters=20, rot_tol=1e-5, trans_tol=None, dist_targets=None, weights=None,
              dist_weight=1.0, feat_weight=1.0, outside=None):
        """Where did it go?  The rigid motion that puts point sets onto this field: damped Gauss-Newton (Levenberg-Marquardt) on the residuals
        of normal_equations(), every instance on its own, the whole loop on the device (d3f_volume_align_accumulate / d3f_volume_align_step,
        csrc/align_kernels.hip): 2 iters + 2 launches on the current stream, no synchronisation.

        points, name, targets, dist_targets, weights, dist_weight, feat_weight, outside   as in normal_equations()
        rot, trans    the starting poses, float32 [I, 3, 3] and [I, 3] in rigid.rigid_transform's row-vector convention (None: the identity);
                      they come out in the same convention: rigid_transform(points, fit['rot'], fit['trans']) is fit['points'].  The kernels' R
                      is the transpose of `rot`.
        iters         the number of iterations after the first evaluation;  rot_tol (rad), trans_tol (None: 1e-3 * step)  a step smaller than
                      both ends the instance as CONVERGED: one that was accepted, or one proposed at a pose that was just accepted (it is not
                      taken: it would lower the cost by less than the fp32 sums resolve)
        Iteration 0 evaluates the start.  Each further one solves (H + lambda D) delta = -b, D_jj = max(H_jj, 1e-9 max H), evaluates the
        candidate and accepts it when the cost fell (lambda / 10, at least 1e-9), else rejects it (10 lambda, at most 1e6).  lambda starts at
        1e-3.  status: 0 RUNNING (the iterations ran out), 1 CONVERGED, 2 STALLED (lambda reached its maximum), 3 NO_GRADIENT (no valid point
        or a flat field: the pose is unchanged), 4 FAILED (a Cholesky pivot that is not positive and finite; the pose is the last accepted one).
        -> {'rot': float32 [I, 3, 3], 'trans': float32 [I, 3], 'points': float32 [I, n, 3] the points at the final pose, 'cost': float64 [I],
            'valid': int32 [I], 'status': int32 [I], 'steps': int32 [I] accepted steps, 'history': float64 [I, iters + 1] the accepted cost
            after every iteration (its last column is the final cost)}.
        Many starts are just more instances: repeat the points with k starting poses -- the k candidates of locate(), say -- and keep
        argmin(cost) among the CONVERGED ones.  The same bytes on every run, and an instance's result does not depend on the others.
        No autograd: outputs never require grad."""
        who = "align"
        iters = operator.index(iters)
        if iters < 0:
            raise ValueError("align: iters must be >= 0, got %d" % iters)
        rot_tol = float(rot_tol)
        trans_tol = 1e-3 * self.step if trans_tol is None else float(trans_tol)
        for k, v in (("rot_tol", rot_tol), ("trans_tol", trans_tol)):
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError("align: %s must be finite and >= 0, got %r" % (k, v))
        prob = self._align_problem(who, points, name, targets, dist_targets, weights, dist_weight, feat_weight, outside)
        I, n, dev = prob["I"], prob["n"], self.device
        pose = self._align_pose(who, I, rot, trans)
        state = torch.zeros((I, _lib.ALIGN_STATE_DOUBLES), dtype=torch.float64, device=dev)
        state[:, 0:12] = pose
        state[:, 12:24] = pose
        state[:, 24:27] = prob["centroid"]
        state[:, 27] = 1e-3
        if I > 0 and n > 0:
            # state (beyond [0, 28)) and skip must be zero, as the header says; step `it` writes history[:, it] of every instance and step 0
            # writes every row of out (every instance is RUNNING then)
            history = torch.empty((I, iters + 1), dtype=torch.float64, device=dev)
            skip = torch.zeros(I, dtype=torch.int32, device=dev)
            out = torch.empty((I, _lib.ALIGN_ROW_DOUBLES), dtype=torch.float64, device=dev)
            for it in range(iters + 1):
                self._align_accumulate(prob, pose, skip, None)
                with self._on() as q:
                    q.d3f_volume_align_step(state, prob["ws"], prob["ws_bytes"], I, n, out, it, iters, rot_tol, trans_tol, pose, skip, history)
        else:
            history = torch.zeros((I, iters + 1), dtype=torch.float64, device=dev)
            state[:, 29] = _lib.ALIGN_NO_GRADIENT          # no point at all: nothing to align to
        R = state[:, 0:9].to(torch.float32).reshape(I, 3, 3)
        t = state[:, 9:12].to(torch.float32)
        p = prob["pts"]
        # the chain of the kernels, element by element (so that an instance's points do not depend on how many instances there are)
        moved = torch.addcmul(torch.addcmul(p[:, :, 0:1] * R[:, None, :, 0], p[:, :, 1:2], R[:, None, :, 1]), p[:, :, 2:3], R[:, None, :, 2]) + t[:, None, :]
        return {"rot": R.transpose(1, 2).contiguous(), "trans": t.contiguous(), "points": moved, "cost": state[:, 28].clone(),
                "valid": state[:, 31].to(torch.int32), "status": state[:, 29].to(torch.int32), "steps": state[:, 30].to(torch.int32), "history": history}

    def relocate(self, points, name, targets, k=4, separation=None, radius_voxels=None, tau=None, n_poses=8, iters=20, min_inliers=4, shared=3,
                 side_tol=None, min_side=None, min_sin=0.2, max_triplets=None, seed=0, max_survivors=65536, max_distance=None, dist_type="l2", **align_terms):
        """Where is it now, from no start at all?  locate(targets) gives k candidate places per model point, consensus.consensus_poses turns
        them into the n_poses best mutually distinct rigid motions (csrc/consensus_kernels.hip), and align() refines the refit
        poses as n_poses instances.  ONE model per call.

        points        float32 [M, 3], 3 <= M <= 64: the model's keypoints;  targets  float32 [M, C]: their descriptors in set `name`
        k, separation, radius_voxels, max_distance, dist_type   as in locate() (neither separation nor radius_voxels: radius_voxels = 2)
        tau           the inlier radius of the consensus, a world length (None: 2 * step)
        n_poses, min_inliers, shared, side_tol, min_side, min_sin, max_triplets, seed, max_survivors   as in consensus_poses() (its `triplets` and
                      `refit` are not taken: all or a seeded subset of the triplets, and always the refit);  iters and **align_terms (rot_tol, trans_tol, weights
                      [n_poses, M], dist_weight, feat_weight, outside)   as in align()
        -> what align() returns for the n_poses instances (a rank the consensus did not fill starts at a NaN pose and ends NO_GRADIENT), with
           'consensus': the dict of consensus_poses() and 'best': int64 [] the argmin of 'cost' among the CONVERGED instances, -1 if none.
        Host synchronisation: the consensus and the alignment add none in the steady state -- only what consensus_poses() states: the first
        call with a new (M, max_triplets, seed) uploads the triplet table.  locate() itself builds small tensors from host values and so makes
        the host wait for the stream, as it does on its own.  No autograd: outputs never require grad."""
        from .consensus import consensus_poses
        who = "relocate"
        self._need_float_rows(who, [name])
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("relocate: points must be [M, 3] (one model), got %s" % (list(getattr(points, "shape", ())) or type(points).__name__))
        M = int(points.shape[0])
        if not 3 <= M <= _lib.CONSENSUS_MAX_POINTS:             # (before locate runs: the consensus would refuse it only afterwards)
            raise ValueError("relocate: M = %d model points, must be 3..%d" % (M, _lib.CONSENSUS_MAX_POINTS))
        k = self._peak_k(who, k)
        pts = self._align_tensor(who, "points", points, (M, 3))
        tg = self._align_tensor(who, "targets", targets, (M, self._channels(self._names([name])[0])))
        if separation is None and radius_voxels is None:
            radius_voxels = 2
        tau = 2.0 * self.step if tau is None else float(tau)
        hits = self.locate(tg, name, k=k, radius_voxels=radius_voxels, separation=separation, max_distance=max_distance, dist_type=dist_type)
        cons = consensus_poses(pts, hits["refined"].to(torch.float32), tau, n_poses=n_poses, min_inliers=min_inliers, shared=shared, side_tol=side_tol,
                               min_side=min_side, min_sin=min_sin, max_triplets=max_triplets, seed=seed, max_survivors=max_survivors)
        H = cons["refit_rot"].shape[0]
        fit = self.align(pts[None].expand(H, M, 3), name, tg[None].expand(H, M, tg.shape[1]), rot=cons["refit_rot"], trans=cons["refit_trans"], iters=iters,
                         **align_terms)
        done = fit["status"] == _lib.ALIGN_CONVERGED
        cost = torch.where(done, fit["cost"], torch.full_like(fit["cost"], float("inf")))
        fit["best"] = torch.where(done.any(), torch.argmin(cost), torch.full((), -1, dtype=torch.int64, device=self.device))
        fit["consensus"] = cons
        return fit

    # ---- rays -----------------------------------------------------------------------------------------------------------------
    def _check_rays(self, origins, dirs):
        for who, t in (("origins", origins), ("dirs", dirs)):
            assert type(t) == torch.Tensor
            assert len(t.shape) == 2
            assert t.shape[1] == 3
            if not t.is_cuda or t.device != self.device:
                raise RuntimeError("BakedField.raycast: %s must be on %s (where the volume lives); there is no CPU path" % (who, self.device))
            if t.dtype != torch.float32:
                raise TypeError("BakedField.raycast: %s must be float32, got %s" % (who, t.dtype))
        if origins.shape[0] != dirs.shape[0]:
            raise ValueError("BakedField.raycast: %d origins but %d dirs" % (origins.shape[0], dirs.shape[0]))

    def _ray_names(self, return_names):
        names = self._names(list(return_names))
        keys = _RAY_KEYS + (("in_band",) if self.band is not None else ())
        clash = [k for k in names if k in keys]
        if clash:
            raise ValueError("raycast / render: the set(s) %s carry the name of an output key %s; read them with eval(out['points'])" % (clash, keys))
        return names

    def _march(self, origins, dirs, camera, n, march_step, t_near, t_far, samples=False):
        """one d3f_volume_raycast launch: (t [n], hit [n] bool, points [n,3], samples [n] int32 or None)"""
        dev = self.device
        step = self.step if march_step is None else float(march_step)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        hit = torch.empty(n, dtype=torch.bool, device=dev)
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if samples else None
        with self._on() as q:
            q.d3f_volume_raycast(self._volume(), origins, dirs, n, camera, step, float(t_near), float(t_far), t, hit, pts, cnt)
        return t, hit, pts, cnt

    def _at_hits(self, out, pts, names, normals):
        """rows and normals at the marched points through the lookup: a miss's NaN row is "not valid" there, so it gets the fill
        rows and a zero gradient"""
        if normals:
            grad = self.backward(pts, torch.ones(pts.shape[0], dtype=torch.float32, device=self.device))
            length = torch.linalg.vector_norm(grad, dim=1, keepdim=True)
            out["normal"] = torch.where(length > 0, grad / length, torch.zeros_like(grad))
        if names or self.band is not None:
            rows = self._sample(pts, names)
            if self.band is not None:
                out["in_band"] = rows["in_band"]      # of the hit point's cell: False for a miss, and for a hit outside the band (fill rows)
            for k in names:
                out[k] = rows[k]
        return out

    def raycast(self, origins, dirs, return_names=(), march_step=None, t_near=0.0, t_far=math.inf, normals=False):
        """The first surface each ray o + t d meets (d need not be unit): a march through `dist` in steps of `march_step` (a world
        length, default the lattice step) inside [t_near, t_far] and the volume, stopped at the first + to - crossing between two
        samples of valid cells and interpolated linearly there; holes are never bridged, back faces are no hits.

        -> {'t' [N] (0 for a miss), 'hit_mask' [N] bool, 'points' [N,3] (NaN rows for a miss), 'normal' [N,3] if `normals`
        (grad dist / |grad dist|, pointing into free space; zero for a miss or a zero gradient), name: [N,C] for every name}.
        Rows and normals are BakedField.eval / backward at 'points': a miss gets the fill row, and so does a hit whose own cell
        holds an invalid corner.  There is no autograd through the march: outputs never require grad."""
        self._check_rays(origins, dirs)
        names = self._ray_names(return_names)
        n = origins.shape[0]
        t, hit, pts, _ = self._march(origins.detach().contiguous(), dirs.detach().contiguous(), None, n, march_step, t_near, t_far)
        return self._at_hits({"t": t, "hit_mask": hit, "points": pts}, pts, names, normals)

    def _camera(self, K, pose, H, W):
        K = torch.as_tensor(K).detach().to("cpu", torch.float32)
        pose = torch.as_tensor(pose).detach().to("cpu", torch.float32)
        if tuple(K.shape) != (3, 3):
            raise ValueError("BakedField.render: K must be [3,3], got %s" % (tuple(K.shape),))
        if tuple(pose.shape) not in ((3, 4), (4, 4)):
            raise ValueError("BakedField.render: pose must be [3,4] or [4,4] (world -> camera), got %s" % (tuple(pose.shape),))
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("BakedField.render: H=%d W=%d must be >= 1" % (H, W))
        return _lib.Pinhole((ctypes.c_float * 9)(*K.reshape(-1).tolist()), (ctypes.c_float * 12)(*pose[:3].reshape(-1).tolist()), H, W)

    def render(self, K, pose, H, W, return_names=(), march_step=None, t_near=0.0, t_far=math.inf, normals=False):
        """raycast() through the pixels of a pinhole camera the observation need not have had: K [3,3], pose [3,4] or [4,4]
        world -> camera as curr_obs_torch['pose'] (tensors on any device, or arrays; read on the host), pixel (u, v) looks along
        R^T ((u - cx)/fx, (v - cy)/fy, 1) from -R^T tc, so 't' is the camera depth.
        -> {'depth' [H,W] (0: no surface), 'hit_mask' [H,W] bool, 'points' [H,W,3], 'normal' [H,W,3], name: [H,W,C]}."""
        names = self._ray_names(return_names)
        cam = self._camera(K, pose, H, W)
        H, W = cam.H, cam.W
        t, hit, pts, _ = self._march(None, None, cam, H * W, march_step, t_near, t_far)
        out = self._at_hits({"depth": t, "hit_mask": hit, "points": pts}, pts, names, normals)
        return {k: v.view((H, W) + tuple(v.shape[1:])) for k, v in out.items()}
