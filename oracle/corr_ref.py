"""TEST INFRASTRUCTURE ONLY -- float64 descriptor distances, similarities, best match and k-NN with per-entry bounds.

The descriptor-similarity kernels (csrc/corr_kernels.hip: pairwise_dist / pairwise_mfma, dist_to_target, the softmax and
top-k steps) are checked against this module entry by entry.  Plain numpy, float64:
  - d^2 = |a|^2 + |b|^2 - 2 a.b through BLAS, and the direct form sum (a - b)^2 for the pairs with d^2 <= 1e-3 (|a|^2 + |b|^2)
    and for rows or columns holding a non-finite value (so Inf - Inf gives NaN and a lone Inf gives +Inf, as in float32);
    d^2 > FLT_MAX counts as +Inf (what float32 accumulation reaches).
  - the bound is per entry and relative to d^2 itself: |d^2_32 - d^2_64| <= TOL * d^2_64 + C * FLT_MIN (the absolute term
    covers products that fall into the subnormal range).  The MFMA path's guard keeps every contracted pair at
    d^2 >= 1/4 (|a|^2 + |b|^2), so one relative bound covers both kernel forms.  An l2 distance takes the square root of
    the interval, widened by the rounding of sqrtf.
  - softmax(-scale * d, dim 0) by log-sum-exp, with the relative bound
        p_i * (|s| B_i + |s| sum_k p_k B_k + 8 u (1 + |z_i| + |z_max|) + 8 u log2(B1)) + FLT_MIN
    (B_i: the bound on d_i; z = -s d the logits; u = 2^-24): the distance errors moved through the softmax, the float32
    evaluation of the logits and expf, and the float32 column sum.
  - best match and k-NN as sets of admissible answers: a row may take a place if no remaining row is DEFINITELY better,
    i.e. with intervals [lo, hi] of what float32 can produce, no remaining x with hi_x < lo_row.  NaN ranks after +Inf,
    NaN rows among themselves by row index (include/d3fields_hip.h).

TOL was measured on the float32 emulations of the kernel forms (oracle/corr_emul.py) over the cases of
tests/test_corr_ref.py: the worst |d^2_32 - d^2_64| / d^2_64 was 8.1e-7 for the pairwise direct form (C = 1000), 8.1e-7
for the guarded contraction (C = 384) and 1.9e-6 for dist_to_target's one-lane chain of C = 1000 fmaf.  TOL = 4e-6 on
d^2 is 2e-6 on d, twice the worst chain and five times the worst pairwise form.  The unguarded contraction misses the
bound by orders of magnitude on near duplicates (the test asserts it).
"""
import numpy as np

TOL = 4e-6
EMUL_WORST_DIRECT = 8.2e-7
EMUL_WORST_GUARDED = 8.2e-7
EMUL_WORST_CHAIN = 1.9e-6
U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
F64 = np.float64


def dist2(src, tgt):
    """float64 d^2 [B1,B2] of float32 rows src [B1,C] and tgt [B2,C]."""
    a = np.asarray(src, np.float32).astype(F64)
    b = np.asarray(tgt, np.float32).astype(F64)
    fa, fb = np.isfinite(a).all(1), np.isfinite(b).all(1)
    na = np.where(fa, (np.where(np.isfinite(a), a, 0.0) ** 2).sum(1), 0.0)
    nb = np.where(fb, (np.where(np.isfinite(b), b, 0.0) ** 2).sum(1), 0.0)
    a0 = np.where(fa[:, None], a, 0.0)
    b0 = np.where(fb[:, None], b, 0.0)
    nsum = na[:, None] + nb[None, :]
    d2 = nsum - 2.0 * (a0 @ b0.T)
    redo = (d2 <= 1e-3 * nsum) | ~fa[:, None] | ~fb[None, :]
    ii, jj = np.nonzero(redo)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(ii), 1 << 14):
            i, j = ii[s:s + (1 << 14)], jj[s:s + (1 << 14)]
            d2[i, j] = ((a[i] - b[j]) ** 2).sum(1)
    d2[d2 > FLT_MAX] = np.inf
    return d2


class Dist:
    """Distances of one dist_type: d (float64; +Inf / NaN where float32 gives them), [lo, hi] = what float32 may return,
    B = max(hi - d, d - lo) (0 where d is not finite)."""

    def __init__(self, d2, C, dist_type):
        self.dist_type = dist_type
        self.nan = np.isnan(d2)
        with np.errstate(invalid="ignore", over="ignore"):
            err = TOL * d2 + C * FLT_MIN
            lo = np.maximum(d2 - err, 0.0)
            hi = d2 + err
            lo[np.isinf(d2)] = np.inf
            hi[hi > FLT_MAX] = np.inf
            if dist_type == "l2":
                d = np.sqrt(d2)
                lo, hi = np.sqrt(lo) * (1 - 2 * U), np.sqrt(hi) * (1 + 2 * U)
            else:
                d = d2
        lo[self.nan] = np.nan
        hi[self.nan] = np.nan
        self.d, self.lo, self.hi = d, lo, hi
        with np.errstate(invalid="ignore"):
            self.B = np.where(np.isfinite(d), np.maximum(hi - d, d - lo), 0.0)
        self.B[np.isinf(self.B)] = 0.0


def pairwise(src, tgt, dist_type):
    return Dist(dist2(src, tgt), np.asarray(src).shape[1], dist_type)


def to_target(src_rows, tgt, dist_type):
    """src_rows [N,C] against one target [C]: a [N,1] Dist."""
    return pairwise(src_rows, np.asarray(tgt, np.float32)[None], dist_type)


def _fail(what, bad, got, ref, extra=""):
    k = np.argwhere(bad)[:5]
    raise AssertionError("%s: %d entries outside the bound, first at %s: got %s, float64 %s %s"
                         % (what, int(bad.sum()), k.tolist(), [got[tuple(t)] for t in k], [ref[tuple(t)] for t in k], extra))


def check_dist(got, D, what="distance"):
    """every entry of got inside [lo, hi]; NaN exactly where float64 has NaN.  Returns the worst |got - d| / B."""
    got = np.asarray(got, F64).reshape(D.d.shape)
    gn = np.isnan(got)
    if not np.array_equal(gn, D.nan):
        _fail(what + " NaN pattern", gn != D.nan, got, D.d)
    ok = D.nan | ((got >= D.lo) & (got <= D.hi))
    if not ok.all():
        _fail(what, ~ok, got, D.d)
    fin = np.isfinite(got) & np.isfinite(D.d) & (D.B > 0)
    return float((np.abs(got[fin] - D.d[fin]) / D.B[fin]).max()) if fin.any() else 0.0


def _logits(D, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        z = -float(scale) * D.d
    z[np.abs(z) > FLT_MAX] = np.copysign(np.inf, z[np.abs(z) > FLT_MAX])        # float32 overflows there
    return z


def softmax(D, scale):
    """float64 softmax(-scale d, dim 0) [B1,B2] and its per-entry bound (NaN columns: bound NaN)."""
    z = _logits(D, scale)
    B1 = z.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        zmax = z.max(0)                                        # NaN if the column holds one
        e = np.exp(z - zmax)
        p = e / e.sum(0)
        s = abs(float(scale))
        carry = s * np.nansum(np.where(p > 0, p * D.B, 0.0), axis=0)
        rel = s * D.B + carry + 8 * U * (1 + np.abs(z) + np.abs(zmax)) + 8 * U * np.log2(max(B1, 2))
        rel = np.where(np.isfinite(z), rel, 0.0)
        bound = p * rel + FLT_MIN
    return p, bound


def check_softmax(got, D, scale, what="softmax"):
    got = np.asarray(got, F64).reshape(D.d.shape)
    p, bound = softmax(D, scale)
    pn = np.isnan(p)
    if not np.array_equal(np.isnan(got), pn):
        _fail(what + " NaN pattern", np.isnan(got) != pn, got, p)
    with np.errstate(invalid="ignore"):
        bad = ~pn & ~(np.abs(got - p) <= bound)
    if bad.any():
        _fail(what, bad, got, p, "(scale %g)" % scale)


def exp_sim(D, scale):
    """exp(-scale d) and its bound; a value past FLT_MAX is +Inf in float32 (a negative scale gets there)"""
    z = _logits(D, scale)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z)
        rel = abs(float(scale)) * D.B + 8 * U * (1 + np.abs(z))
        bound = np.where(np.isfinite(z), e * rel, 0.0) + FLT_MIN
    e[e > FLT_MAX] = np.inf
    return e, bound


def check_exp(got, D, scale, what="exp similarity"):
    got = np.asarray(got, F64).reshape(D.d.shape)
    e, bound = exp_sim(D, scale)
    en = np.isnan(e)
    if not np.array_equal(np.isnan(got), en):
        _fail(what + " NaN pattern", np.isnan(got) != en, got, e)
    with np.errstate(invalid="ignore"):
        bad = ~en & ~((np.abs(got - e) <= bound) | (got == e) | ((got == np.inf) & (e + bound > FLT_MAX)))
    if bad.any():
        _fail(what, bad, got, e, "(scale %g)" % scale)


def _keys(D, scale):
    """(lo, hi, last): the interval of each row's ranking key (smaller ranks first) and the rows that rank after every
    other (NaN key).  scale > 0 ranks by d, scale < 0 by -d; with scale == 0 every row with a finite logit ties."""
    if scale > 0:
        lo, hi = D.lo.copy(), D.hi.copy()
        last = D.nan.copy()
    elif scale < 0:
        lo, hi = -D.hi, -D.lo
        last = D.nan.copy()
    else:
        last = D.nan | np.isinf(D.d) | np.isinf(D.lo)          # -inf * 0 is NaN
        lo = np.zeros_like(D.d)
        hi = np.zeros_like(D.d)
    lo = np.where(last, np.inf, lo)
    hi = np.where(last, np.inf, hi)
    return lo, hi, last


def check_ranked(idx, D, scale=1.0, what="k-NN"):
    """idx [k,B2] (or [B2] for a best match) of rows, against the admissible orders of D's columns.  Row r of a column
    is admissible if every row not yet placed is no DEFINITELY better (NaN after everything, NaN rows by index; with
    scale == 0 every finite-logit row ties, so the lowest one must come first)."""
    idx = np.asarray(idx)
    one = idx.ndim == 1
    idx = idx.reshape(1, -1) if one else idx
    kk, B2 = idx.shape
    B1 = D.d.shape[0]
    lo, hi, last = _keys(D, scale)
    nplace = min(kk, B1)
    if (idx[nplace:] != -1).any():
        raise AssertionError("%s: rows past B1 = %d must be -1" % (what, B1))
    idx = idx[:nplace]
    if ((idx < 0) | (idx >= B1)).any():
        raise AssertionError("%s: index out of range: %s" % (what, idx[(idx < 0) | (idx >= B1)][:5]))
    # A non-NaN row c is beaten only by an unplaced row with hi < lo_c: the nplace + 1 smallest hi of a column always hold
    # the smallest unplaced one (ties among them, +Inf ones included, cannot satisfy hi < lo_c).  A row that ranks last
    # (NaN key) is beaten by ANY unplaced row that does not: counted per column, not searched among the candidates.
    m = min(nplace + 1, B1)
    hsort = np.argpartition(hi, m - 1, axis=0)[:m] if m < B1 else np.broadcast_to(np.arange(B1)[:, None], (B1, B2))
    n_first = (~last).sum(0)
    tie0 = scale == 0
    for j in range(B2):
        placed = set()
        placed_first = 0
        cand = [int(x) for x in hsort[:, j]]
        for r in range(nplace):
            c = int(idx[r, j])
            if c in placed:
                raise AssertionError("%s: column %d lists row %d twice" % (what, j, c))
            if last[c, j]:
                if placed_first < n_first[j]:
                    x = next(int(x) for x in np.flatnonzero(~last[:, j]) if int(x) not in placed)
                    raise AssertionError("%s: column %d place %d is row %d (NaN key) but row %d (key %s) is unplaced"
                                         % (what, j, r, c, x, D.d[x, j]))
            elif not tie0:
                for x in cand:
                    if x != c and x not in placed and hi[x, j] < lo[c, j]:
                        raise AssertionError("%s: column %d place %d is row %d (key %s) but row %d is better (key %s)"
                                             % (what, j, r, c, D.d[c, j], x, D.d[x, j]))
            if last[c, j] or tie0:                              # rows below c that rank with it: the lowest must come first
                same = np.flatnonzero(last[:c, j]) if last[c, j] else np.flatnonzero(~last[:c, j])
                if any(int(x) not in placed for x in same):
                    raise AssertionError("%s: column %d place %d is row %d, a lower tied row is unplaced" % (what, j, r, c))
            placed.add(c)
            placed_first += int(not last[c, j])


def rank_order(x, k):
    """[k,cols] rows of the k smallest entries of x [rows,cols] per column by the header's order: value ascending,
    +Inf before NaN, ties (and NaNs among themselves) to the lower row; -1 past `rows`."""
    x = np.asarray(x)
    rows, cols = x.shape
    out = np.full((k, cols), -1, np.int64)
    r = np.arange(rows)
    for c in range(cols):
        v = x[:, c]
        nan = np.isnan(v)
        o = np.lexsort((r, np.where(nan, 0, v), nan))[:k]
        out[:len(o), c] = o
    return out
