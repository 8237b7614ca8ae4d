"""Fitting a PCA head where the descriptors live: weighted row moments on the device (d3f_row_moments,
csrc/moment_kernels.hip), a float64 symmetric eigen-problem of size C on the host.

    fitted = fit_pca(rows, n_components=3, weights=None)        # rows [M,C] or a channels-last map [V,fh,fw,C]
    fusion.add_projection("pca", "dino_feats", pca=fitted)      # or Fusion.fit_projection, which does both

The reference fits its PCA offline with sklearn (scripts/precompute_pca.py) and pickles it; FittedPCA carries sklearn's
attribute names, so either object goes through mesh.pca_project, Fusion.add_projection and mesh.descriptor_mesh unchanged.
The arithmetic and its error analysis are DESIGN.md section 12.
"""
import numpy as np
import torch

from . import _lib


def _as_rows(rows, weights, who):
    if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 4):
        raise ValueError("%s: rows must be a [M,C] or [V,fh,fw,C] tensor" % who)
    if rows.dtype not in (torch.float32, torch.float16):
        raise ValueError("%s: rows must be float32 or float16, got %s" % (who, rows.dtype))
    C = rows.shape[-1]
    if not 1 <= C <= _lib.MAX_MOMENT_CHANNELS:
        raise ValueError("%s: C=%d outside 1..%d" % (who, C, _lib.MAX_MOMENT_CHANNELS))
    lead = tuple(rows.shape[:-1])
    M = int(np.prod(lead))
    if M < 1:
        raise ValueError("%s: no rows" % who)
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            weights = torch.as_tensor(weights)
        if tuple(weights.shape) != lead:
            raise ValueError("%s: weights have shape %s, rows %s" % (who, tuple(weights.shape), tuple(rows.shape)))
        if weights.dtype not in (torch.bool, torch.uint8) and not weights.dtype.is_floating_point:
            raise ValueError("%s: weights must be bool, uint8 or float, got %s" % (who, weights.dtype))
        weights = weights.to(device=rows.device, dtype=torch.float32).reshape(M).contiguous()
        if bool((weights < 0).any()):              # (NaN weights pass here and make every output NaN)
            raise ValueError("%s: negative weights" % who)
    return M, C, weights


def _flat_rows(rows, M, C):
    """(tensor that owns the storage, row stride in elements): the rows as stored when one stride walks them, else a copy"""
    if rows.stride(-1) == 1 or C == 1:
        stride, span = None, None
        for n, s in zip(reversed(rows.shape[:-1]), reversed(rows.stride()[:-1])):
            if n == 1:
                continue
            if stride is None:
                stride, span = s, s * n
            elif s == span:
                span = s * n
            else:
                stride = -1
                break
        if stride is None:
            return rows, C                         # a single row
        if stride >= C:
            return rows, stride
    return rows.reshape(M, C).contiguous(), C


def _row_moments_host(rows, M, C, weights):
    x = rows.reshape(M, C).to(torch.float64)
    w = torch.ones(M, dtype=torch.float64, device=x.device) if weights is None else weights.to(torch.float64)
    wsum = w.sum()
    mean = (w[:, None] * x).sum(0) / wsum
    d = x - mean
    return wsum, mean, (d * w[:, None]).T @ d


def row_moments(rows, weights=None):
    """(wsum, mean [C], scatter [C,C]) as float64 tensors where `rows` live: wsum = sum w, mean = sum w x / wsum,
    scatter = sum w (x - mean)(x - mean)^T.  rows: [M,C] or a channels-last map [V,fh,fw,C], float32 or float16, last stride 1
    (read as stored when one row stride walks it, e.g. a channel-range view; copied otherwise).  weights: None (all ones) or
    bool / uint8 / float of shape rows.shape[:-1], >= 0.  On the device one d3f_row_moments call on the current stream; CPU
    tensors take the same definition in float64 torch ops."""
    M, C, w = _as_rows(rows, weights, "row_moments")
    if not rows.is_cuda:
        return _row_moments_host(rows, M, C, w)
    flat, stride = _flat_rows(rows, M, C)
    out = torch.empty(1 + C + C * C, dtype=torch.float64, device=rows.device)
    with _lib.on(rows.device) as q:
        ws, nbytes = q.workspace("d3f_row_moments_workspace_bytes", M, C)
        q.d3f_row_moments(flat, _lib.DTYPE_F16 if flat.dtype == torch.float16 else _lib.DTYPE_F32, M, C, stride, w, out[0:1], out[1:1 + C], out[1 + C:],
                          ws, nbytes)
    return out[0], out[1:1 + C], out[1 + C:].view(C, C)


class FittedPCA:
    """The result of a fit, under sklearn.decomposition.PCA's attribute names (numpy float64)."""

    def __init__(self, mean, components, explained_variance, explained_variance_ratio, singular_values, n_samples, whiten):
        self.mean_ = mean
        self.components_ = components
        self.explained_variance_ = explained_variance
        self.explained_variance_ratio_ = explained_variance_ratio
        self.singular_values_ = singular_values
        self.n_components_ = int(components.shape[0])
        self.n_features_in_ = int(components.shape[1])
        self.n_samples_ = float(n_samples)
        self.whiten = bool(whiten)

    def transform(self, x):
        """(x - mean_) @ components_.T (divided by sqrt(explained_variance_) when whiten), float64 where x lives"""
        from . import mesh
        return mesh.pca_project(self, x)


def _host64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def pca_from_moments(wsum, mean, scatter, n_components, whiten=False):
    """Host only: the eigen-decomposition of the scatter matrix in float64 (numpy.linalg.eigh).  Components have unit norm, come
    in descending eigenvalue order, and the entry of largest magnitude of each is positive (what sklearn 1.7's PCA does with
    svd_solver='full')."""
    wsum = float(_host64(wsum))
    mean, scatter = _host64(mean), _host64(scatter)
    if mean.ndim != 1 or scatter.shape != (mean.shape[0], mean.shape[0]):
        raise ValueError("pca_from_moments: mean %s and scatter %s do not match" % (mean.shape, scatter.shape))
    C = mean.shape[0]
    if not (np.isfinite(wsum) and np.isfinite(mean).all() and np.isfinite(scatter).all()):
        raise ValueError("pca_from_moments: non-finite moments (a NaN or Inf row, or weights that sum to zero)")
    if wsum <= 1.0:
        raise ValueError("pca_from_moments: wsum=%g: more than one sample is needed" % wsum)
    if not 1 <= int(n_components) <= C:
        raise ValueError("pca_from_moments: n_components=%s outside 1..C=%d" % (n_components, C))
    k = int(n_components)
    lam, vec = np.linalg.eigh(0.5 * (scatter + scatter.T))
    lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
    comp = np.ascontiguousarray(vec[:, :k].T)
    big = np.abs(comp).argmax(axis=1)
    comp *= np.sign(comp[np.arange(k), big])[:, None]
    var = lam / (wsum - 1.0)
    return FittedPCA(mean.copy(), comp, var[:k].copy(), (lam[:k] / lam.sum()), np.sqrt(lam[:k]), wsum, whiten)


def fit_pca(rows, n_components=3, weights=None, whiten=False):
    """row_moments on the device, pca_from_moments on the host"""
    wsum, mean, scatter = row_moments(rows, weights)
    return pca_from_moments(wsum, mean, scatter, n_components, whiten)
