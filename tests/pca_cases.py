"""TEST INFRASTRUCTURE ONLY -- inputs, the float64 definition and the float32 port of the PCA fit (d3fields_amd/pca.py,
d3f_row_moments), shared by tests/test_pca_fit_host.py (CPU) and tests/test_gpu_pca_fit.py (MI355X).

Rows have a planted spectrum: 6 orthonormal directions scaled 8, 6, 4.5, 3, 2, 1.5, plus 0.3 N(0,1) noise, plus a
per-channel offset 5 N(0,1) (an uncentred Gram matrix is plainly wrong on them).

The definition (moments64): wsum = sum w, mean = sum w x / wsum, S = sum w (x - mean)(x - mean)^T in float64, with the
magnitudes an implementation may round at,
    A_ij = sum_m w_m |x_mi - mean_i| |x_mj - mean_j|     and     a_c = sum_m w_m |x_mc| / wsum.
The assertions are |S_got - S| <= tol A and |mean_got - mean| <= tol a, entry by entry.

The tolerance: 3 x the worst ratio of port32 below (a float32 torch port of the kernel's route: column sums in chains of 32
rows, rows centred at fp32(mean), products and chains of 64 rows in float32, chain sums in float64, the shift corrected), as
tests/test_pca_fit_host.py measures it and stores it in PORT_WORST / PORT_WORST_MEAN, capped by the a-priori bound of the
route: one rounding of the centred row, one of w d, and one per row of a chain of 64 -- (64 + 4) 2^-24
for the scatter; a chain of 32 and the division, (32 + 2) 2^-24, for the mean.
"""
import functools

import torch

F64 = torch.float64
EPS32 = 2.0 ** -24
SCALES = (8.0, 6.0, 4.5, 3.0, 2.0, 1.5)
SUM_CHAIN, ROW_CHAIN = 32, 64                    # csrc/moment_kernels.hip: kMomSumChain, kMomRows
CAP_SCATTER = (ROW_CHAIN + 4) * EPS32
CAP_MEAN = (SUM_CHAIN + 2) * EPS32


def planted(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = min(len(SCALES), C)
    Q = torch.linalg.qr(torch.randn(C, r, generator=g, dtype=F64))[0]
    z = torch.randn(M, r, generator=g, dtype=F64) * torch.tensor(SCALES[:r], dtype=F64)
    x = z @ Q.T + 0.3 * torch.randn(M, C, generator=g, dtype=F64) + 5.0 * torch.randn(C, generator=g, dtype=F64)
    return x.float()


def _plain(M, C, seed):
    return {"rows": planted(M, C, seed), "weights": None}


def _mask(M, C, seed):
    g = torch.Generator().manual_seed(seed + 100)
    return {"rows": planted(M, C, seed), "weights": torch.rand(M, generator=g) < 0.7}


def _soft(M, C, seed):
    g = torch.Generator().manual_seed(seed + 200)
    return {"rows": planted(M, C, seed), "weights": torch.rand(M, generator=g)}


def _half(M, C, seed):
    return {"rows": planted(M, C, seed).half(), "weights": None}


def _sliced(C, first, wide, seed):
    """a [2,5,7,C] map that is a channel range of a wider tensor: row stride `wide` > C, base pointer `first` elements in"""
    x = planted(2 * 5 * 7, wide, seed).reshape(2, 5, 7, wide)
    return {"rows": x[..., first:first + C], "weights": None}


# name -> builder.  Between them: C = 3 (one padded panel, a ragged stage), C = 129 (panel tail of one channel: neither a
# multiple of 4, 16 nor 64), more than one row slab and stage tails (M = 4099, 3001), 0/1 and fractional weights, full-width
# panels at C = 1024, fp16 storage, a row stride above C with an aligned and with an unaligned base pointer (the scalar path).
CASES = {
    "C3 M257": lambda: _plain(257, 3, 1),
    "C129 M1537": lambda: _plain(1537, 129, 2),
    "C384 M4099 mask": lambda: _mask(4099, 384, 3),
    "C1024 M3001 soft": lambda: _soft(3001, 1024, 4),
    "C129 M1537 f16": lambda: _half(1537, 129, 5),
    "C384 map slice": lambda: _sliced(384, 8, 400, 6),
    "C384 map slice unaligned": lambda: _sliced(384, 1, 401, 7),
}
SPECTRUM_CASES = ("C129 M1537", "C384 M4099 mask", "C1024 M3001 soft", "C129 M1537 f16")     # M > C: eigenvectors are determined
MASK_CASES = ("C384 M4099 mask",)


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()


def flat(case):
    """(x [M,C] as stored dtype, w [M] float64 or None)"""
    rows = case["rows"]
    x = rows.reshape(-1, rows.shape[-1])
    w = case["weights"]
    return x, (None if w is None else w.reshape(-1).to(F64))


def moments64(x, w=None, mutant=None):
    """(wsum, mean [C], S [C,C], A [C,C], a [C]) in float64 -- the definition; `mutant` breaks it on purpose:
    'about zero' (no centring), 'weights ignored', 'weights squared'."""
    x = x.to(F64)
    w = torch.ones(x.shape[0], dtype=F64) if (w is None or mutant == "weights ignored") else w.to(F64)
    if mutant == "weights squared":
        w = w * w
    wsum = w.sum()
    mean = (w[:, None] * x).sum(0) / wsum
    d = x if mutant == "about zero" else x - mean
    wd = w[:, None] * d
    return wsum, mean, wd.T @ d, wd.abs().T @ d.abs(), (w[:, None] * x.abs()).sum(0) / wsum


MUTANTS = ("about zero", "weights ignored", "weights squared")


@functools.lru_cache(maxsize=None)
def reference(name):
    x, w = flat(build(name))
    return moments64(x, w)


def check(got, ref, A, tol):
    """(ok, worst ratio): non-finite entries must coincide, finite ones satisfy |got - ref| <= tol * A"""
    got, ref, A = got.detach().cpu().to(F64), ref.to(F64), A.to(F64)
    fin = torch.isfinite(ref)
    if not torch.equal(torch.isfinite(got), fin):
        return False, float("inf")
    err = (got - ref).abs()[fin]
    worst = float((err / A[fin].clamp_min(1e-300)).max()) if err.numel() else 0.0
    return bool((err <= tol * A[fin]).all()), worst


def tol_scatter(port_worst):
    return min(3.0 * port_worst, CAP_SCATTER)


def tol_mean(port_worst_mean):
    return min(3.0 * port_worst_mean, CAP_MEAN)


def port32(x, w=None, max_cols=128):
    """The kernel's route in float32 torch ops on the host: (wsum, mean [C], S[:, cols], cols), float64 outputs.  Every
    chain is a sequential float32 accumulation of the kernel's length (products rounded separately, where the kernel fuses
    them: no better than the kernel); for C > 512 only `max_cols` columns spread over the panels are accumulated."""
    x = x.float()
    M, C = x.shape
    w32 = torch.ones(M) if w is None else w.float()

    def chains(v, n):
        """sum over rows of v [M,K] float32: sequential float32 chains of n rows, chain sums in float64"""
        pad = (-M) % n
        v = torch.cat((v, torch.zeros(pad, v.shape[1]))) if pad else v
        v = v.reshape(-1, n, v.shape[1])
        acc = torch.zeros(v.shape[0], v.shape[2])
        for r in range(n):
            acc = acc + v[:, r]
        return acc.to(F64).sum(0)

    wsum = chains(w32[:, None], SUM_CHAIN)[0]
    mean = chains(w32[:, None] * x, SUM_CHAIN) / wsum
    m32 = mean.float()
    d = x - m32
    wd = w32[:, None] * d
    cols = torch.arange(C) if C <= 512 else torch.arange(0, C, C // max_cols)[:max_cols]
    wdc = wd[:, cols].contiguous()
    S = torch.zeros(C, cols.numel(), dtype=F64)
    for r0 in range(0, M, ROW_CHAIN):
        acc = torch.zeros(C, cols.numel())
        for r in range(r0, min(M, r0 + ROW_CHAIN)):
            acc.addcmul_(d[r][:, None], wdc[r][None, :])
        S += acc.to(F64)
    delta = chains(wd, ROW_CHAIN) / wsum
    S -= (wsum * delta)[:, None] * delta[cols][None, :]
    return wsum, mean, S, cols


# ---- components ----------------------------------------------------------------------------------------------------------
def spectrum64(S, k):
    """(eigenvalues descending [C], the first k eigenvectors as rows [k,C] with the largest-magnitude entry positive, gap_i =
    distance from eigenvalue i to the rest of the spectrum)"""
    lam, vec = torch.linalg.eigh(S)
    lam, vec = lam.flip(0), vec.flip(1)
    v = vec[:, :k].T.clone()
    big = v.abs().argmax(1)
    v *= torch.sign(v[torch.arange(k), big])[:, None]
    gap = torch.stack([torch.min((lam[i] - torch.cat((lam[:i], lam[i + 1:]))).abs()) for i in range(k)])
    return lam, v, gap


# ---- a small scene for Fusion.fit_projection -----------------------------------------------------------------------------
def scene(C=129, seed=9):
    from d3fields_amd import synth
    V, H, W = 4, 96, 128
    sc = synth.make_scene(V, H, W, "smooth")
    feats = planted(V * 12 * 16, C, seed).reshape(V, 12, 16, C)
    pts = synth.random_cloud(3000, seed=3)
    return sc, feats, pts, H, W
