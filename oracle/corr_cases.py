"""TEST INFRASTRUCTURE ONLY -- seeded descriptor sets at the edges of the pairwise-distance kernels (csrc/corr_kernels.hip),
shared by tests/test_corr_ref.py (float32 emulations, CPU) and tests/test_gpu_corr.py (the kernels)."""
import numpy as np


def randn(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def guard_case(B1, B2, C, seed=0, offset_col=True, dense=True, sigma=1.0):
    """src [B1,C], tgt [B2,C] float32 with what the MFMA path's guard (d^2 < 1/4 (|a|^2 + |b|^2): recompute) must handle:
      columns 0..9   a match at graded distances eps * typical, across the guard's threshold (0.5 * typical on d);
      column 10      an exact duplicate of row 70 (d = 0), duplicated again in row 200 (an exact tie across two 64-row
                     tiles, one of them the dense one's neighbour);
      column 11      a near tie: two rows at mirrored differences from the target, equal in exact arithmetic but rounded
                     in float32 and summed in different channel orders by the kernels (the exact tie is column 10);
      column 12      an offset column (+40 on every channel: |b|^2 dwarfs every distance to it);
      rows d0..d0+63 x columns 32..63  (placed first; d0 = 384 when B1 >= 448, else 128; B2 >= 64) mutually near
                     descriptors: that whole 64 x 64 tile has more than 96 flagged pairs and takes the direct form.  With
                     d0 = 384 no other edge shares its tile, so every edge of columns 0..12 sits in a sparse tile (few
                     flagged pairs: contraction plus the wave's recompute) -- unless the caller adds more flagged pairs.
    Returns (src, tgt, info) with info = dict of the rows placed."""
    rng = np.random.default_rng(seed)
    src = randn(rng, B1, C) * np.float32(sigma)
    tgt = randn(rng, B2, C) * np.float32(sigma)
    d0 = 384 if B1 >= 448 else 128
    info = {"rows": []}
    if dense and B1 >= d0 + 64 and B2 >= 64:
        base = randn(rng, C)
        src[d0:d0 + 64] = base + np.float32(0.05) * randn(rng, 64, C)
        tgt[32:64] = base + np.float32(0.05) * randn(rng, 32, C)
        info["dense"] = d0
    typical = float(np.sqrt(2 * C)) * sigma
    eps = [0.0, 1e-4, 1e-2, 0.1, 0.3, 0.45, 0.49, 0.51, 0.55, 0.8]
    for k, e in enumerate(eps[:min(B2, len(eps))]):
        r = (37 * (k + 1)) % B1
        n = randn(rng, C)
        tgt[k] = src[r] + n * np.float32(e * typical / max(float(np.linalg.norm(n)), 1e-30))
        info["rows"].append(r)
    if B2 > 10 and B1 > 200:
        tgt[10] = src[70]
        src[200] = src[70]
        info["dup"] = (70, 200)
    if B2 > 11 and B1 > 21:
        t = B1 // 3 if B1 > 66 else 20
        tgt[11] = src[t] + np.float32(0.1) * randn(rng, C)
        src[t + 1] = tgt[11] + (src[t] - tgt[11])[::-1]
        info["tie"] = (t, t + 1)
    if offset_col and B2 > 12:
        tgt[12] = tgt[12] + np.float32(40.0)
    return src, tgt, info


def add_nonfinite(src, tgt, inf_rows=True):
    """+Inf / NaN in sources and targets, both kinds in one column, and a column whose every distance is NaN -- in columns
    64 and 65 (B2 >= 66), a column tile of their own: every pair of those columns fails the guard, and in the tile of
    guard_case's edges they would push it past 96 flagged pairs into the direct form.  A NaN source row would turn every
    softmax column NaN, as in the reference, so the k-NN tests place that one.  With scale <= 0 an Inf row also turns
    every column NaN: inf_rows=False leaves the rows finite."""
    B1, C = src.shape
    assert tgt.shape[0] >= 66
    if inf_rows:
        src[B1 - 5, C // 2] = np.inf             # +Inf distance to every finite target
        src[B1 - 3, C - 1] = np.inf              # ... and Inf - Inf = NaN against column 64
    tgt[64, C - 1] = np.inf                      # column 64: +Inf against every row, NaN against row B1 - 3
    tgt[65, 0] = np.nan                          # column 65: NaN everywhere -> best match 0
    return 64, 65


def edge_rows(info):
    """the rows of guard_case's edges in columns 0..11 that lie outside the dense block"""
    rows = list(info["rows"]) + list(info.get("dup", ())) + list(info.get("tie", ()))
    d0 = info.get("dense")
    return sorted(set(r for r in rows if d0 is None or not d0 <= r < d0 + 64))


def flags64(src, tgt):
    """the pairs the guard flags, predicted in float64: d^2 < 1/4 (|a|^2 + |b|^2), or a non-finite |a|^2 + |b|^2.  It equals
    the float32 decision except within float32 rounding of the threshold (guard_case keeps its pairs >= 4 % away from
    it; tests/test_corr_ref.py compares it with the emulation).  Returns (d2, nsum) for flags_per_tile."""
    a = np.asarray(src, np.float32).astype(np.float64)
    b = np.asarray(tgt, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        na, nb = (a * a).sum(1), (b * b).sum(1)
        fa, fb = np.isfinite(na), np.isfinite(nb)
        a0, b0 = np.where(fa[:, None], a, 0.0), np.where(fb[:, None], b, 0.0)
        nsum = na[:, None] + nb[None, :]
        d2 = (a0 * a0).sum(1)[:, None] + (b0 * b0).sum(1)[None, :] - 2.0 * (a0 @ b0.T)
    return d2, nsum


def flags_per_tile(d2_contraction, nsum):
    """how many pairs of each 64 x 64 tile fail the guard (for asserting that a case reaches a branch)"""
    f = ~((d2_contraction >= np.float32(0.25) * nsum) & (nsum < np.inf))
    B1, B2 = f.shape
    return np.array([[int(f[i:i + 64, j:j + 64].sum()) for j in range(0, B2, 64)] for i in range(0, B1, 64)])
