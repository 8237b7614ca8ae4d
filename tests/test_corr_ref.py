"""CPU: pins oracle/corr_ref.py (the float64 reference of the descriptor-similarity kernels) before any GPU test trusts it.

It agrees with the reference's own outputs (golden 'corr_utils') and with the C oracle within its bounds; the float32
emulations of both kernel forms (oracle/corr_emul.py) fall inside the bounds with margin on the cases where the
contraction is hardest -- near duplicates, ties, an offset column, several data scales and softmax scales -- and the
unguarded contraction is rejected, so the bound is tight enough to matter.  The worst ratios are printed (-s) and held
to the numbers corr_ref's docstring records."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import corr_cases as K, corr_emul as E, corr_ref as R

F32 = np.float32


def _ratio(d2_32, d2_64, C):
    fin = np.isfinite(d2_64) & np.isfinite(d2_32)
    r = np.abs(d2_32.astype(np.float64) - d2_64)[fin] / (d2_64[fin] + C * R.FLT_MIN)
    return float(r.max())


def _softmax32(d32, scale):
    """float32 softmax(-scale d, dim 0) as the kernels evaluate it (logit, max, sum of expf, expf / sum)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (-d32 * F32(scale)).astype(F32)
        m = v.max(0)
        s = np.exp((v - m).astype(F32)).sum(0, dtype=F32)
        return (np.exp((v - m).astype(F32)) / s).astype(F32)


def test_golden_corr_utils_within_bounds():
    """the reference's own float32 outputs (corr_utils.py on the golden inputs) lie inside corr_ref's bounds"""
    g = load_golden("corr_utils")
    for dt in ("l2", "square"):
        D = R.pairwise(g["multi_src"], g["multi_tgt"], dt)
        R.check_softmax(g["multi_" + dt], D, float(g["multi_scale"]), "golden multi " + dt)
        R.check_ranked(g["multi_argmax_" + dt], D, scale=float(g["multi_scale"]), what="golden argmax " + dt)
        fm = g["fmap_bhwc"]
        Dt = R.to_target(fm.reshape(-1, fm.shape[-1]), g["tgt"], dt)
        R.check_exp(g["similarity_" + dt].reshape(-1, 1), Dt, float(g["scale"]), "golden similarity " + dt)
        R.check_dist(g["dist_tensor_" + dt].reshape(-1, 1), Dt, "golden dist " + dt)
        Db = Dt.d.reshape(fm.shape[0], -1)                       # softmax over B (dim 0) of [B, H*W]
        Dsm = R.Dist(Db ** 2 if dt == "l2" else Db, fm.shape[-1], dt)
        R.check_softmax(g["similarity_tensor_" + dt].reshape(fm.shape[0], -1), Dsm, float(g["scale"]), "golden tensor " + dt)


@pytest.mark.parametrize("dt", ["l2", "square"])
def test_c_oracle_within_bounds(dt):
    from oracle import c_oracle as O
    src, tgt, _ = K.guard_case(700, 80, 48, seed=3)
    D = R.pairwise(src, tgt, dt)
    R.check_dist(O.pairwise(src, tgt, 1.0, dt, mode="dist"), D, "oracle dist")
    for scale in (0.05, 0.9, 3.0):
        sm, am = O.pairwise(src, tgt, scale, dt, return_argmax=True)
        R.check_softmax(sm, D, scale, "oracle softmax")
        R.check_ranked(am, D, scale=scale, what="oracle argmax")


_EMUL_CASES = [(256, 64, 64, 1.0, 1), (256, 64, 384, 1.0, 2), (256, 64, 64, 0.05, 3), (256, 64, 64, 30.0, 4),
               (192, 80, 96, 1.0, 5)]


def test_emulations_within_bound_and_tol_calibrated():
    """both kernel forms (and the one-lane chain of dist_to_target) inside the bound with margin; their worst ratios are
    the ones corr_ref records, so TOL stays a few times what float32 really does"""
    worst = {"direct": 0.0, "guarded": 0.0, "chain": 0.0}
    cases = [K.guard_case(B1, B2, C, seed=s, sigma=sg) for B1, B2, C, sg, s in _EMUL_CASES]
    cases.append(K.guard_case(300, 40, 1000, seed=2))
    for src, tgt, _ in cases:
        C = src.shape[1]
        d2 = R.dist2(src, tgt)
        forms = {"direct": E.direct(src, tgt), "chain": E.chain(src, tgt)}
        if C % 32 == 0:
            forms["guarded"] = E.contraction(src, tgt)
        for name, d32 in forms.items():
            worst[name] = max(worst[name], _ratio(d32, d2, C))
            for dt in ("l2", "square"):
                D = R.Dist(d2, C, dt)
                got = np.sqrt(d32) if dt == "l2" else d32
                R.check_dist(got, D, "%s %s" % (name, dt))
                for scale in (0.05, 0.9, 5.0, -0.3):
                    R.check_softmax(_softmax32(got.astype(F32), scale), D, scale, "%s %s" % (name, dt))
    print("\nworst |d2_32 - d2_64| / d2_64: direct %.3g, guarded contraction %.3g, one-lane chain %.3g (TOL %.1g)"
          % (worst["direct"], worst["guarded"], worst["chain"], R.TOL))
    assert worst["direct"] <= R.EMUL_WORST_DIRECT and worst["guarded"] <= R.EMUL_WORST_GUARDED
    assert worst["chain"] <= R.EMUL_WORST_CHAIN
    assert max(worst.values()) <= R.TOL / 2
    assert min(worst.values()) >= R.TOL / 50                       # the cases do exercise float32 rounding


def test_emulated_contraction_reaches_both_guard_branches():
    """the near-duplicate case flags pairs in sparse tiles (wave recompute) and >96 in the dense tile (direct tile)"""
    src, tgt, _ = K.guard_case(256, 64, 64, seed=1)
    raw = E.contraction(src, tgt, guard=False)
    nsum = (E._norms(src)[:, None] + E._norms(tgt)[None, :]).astype(F32)
    tiles = K.flags_per_tile(raw, nsum)
    assert tiles[2, 0] > 96 and 0 < tiles[0, 0] <= 96


@pytest.mark.parametrize("B1,B2,C", [(2048, 80, 64), (513, 66, 32), (1024, 70, 96)])
def test_guard_case_edges_take_the_contraction(B1, B2, C):
    """the layout of tests/test_gpu_corr.py's MFMA-vs-direct cases: guard_case's edges sit in sparse tiles (the contraction
    and the wave recompute handle them), the dense block and the non-finite columns elsewhere; the float64 prediction of
    the guard (what the GPU test asserts on) equals the emulated float32 guard on every tile"""
    for inf_rows in (True, False):
        src, tgt, info = K.guard_case(B1, B2, C, seed=B1 + C)
        K.add_nonfinite(src, tgt, inf_rows=inf_rows)
        raw = E.contraction(src, tgt, guard=False)
        nsum = (E._norms(src)[:, None] + E._norms(tgt)[None, :]).astype(F32)
        tiles = K.flags_per_tile(raw, nsum)
        assert np.array_equal(tiles, K.flags_per_tile(*K.flags64(src, tgt)))
        rows = K.edge_rows(info)
        assert len(rows) >= 10
        for r in rows:
            assert 0 < tiles[r // 64, 0] <= 96, (r, tiles[:, 0])
        assert tiles[info["dense"] // 64, 0] > 96


@pytest.mark.parametrize("dt", ["l2", "square"])
def test_unguarded_contraction_rejected(dt):
    src, tgt, _ = K.guard_case(256, 64, 64, seed=1, dense=False)
    D = R.pairwise(src, tgt, dt)
    raw = E.contraction(src, tgt, guard=False)
    with np.errstate(invalid="ignore"):
        got = np.sqrt(raw) if dt == "l2" else raw
    with pytest.raises(AssertionError):
        R.check_dist(got, D)
    # the same contraction clamped at 0 (no NaN from a negative d^2) is still rejected on the near pairs alone
    near = np.zeros_like(D.nan)
    near[[r for r in (37, 74, 111)], [0, 1, 2]] = True
    clamped = np.maximum(raw, 0)
    got = np.where(near, np.sqrt(clamped) if dt == "l2" else clamped, D.d)
    with pytest.raises(AssertionError):
        R.check_dist(got, D)


def test_ranking_contract():
    """NaN after +Inf, NaN rows by index, exact ties to the lower row; a row that is definitely worse is rejected"""
    x = np.array([[np.nan, 1.0], [np.inf, 1.0], [0.5, np.nan], [np.nan, 2.0]], F32)
    assert R.rank_order(x, 4).tolist() == [[2, 0], [1, 1], [0, 3], [3, 2]]
    src = np.array([[0.0], [np.inf], [np.nan], [1.0], [1.0]], F32)
    tgt = np.array([[1.0], [np.nan]], F32)
    D = R.pairwise(src, tgt, "l2")
    R.check_ranked([[3, 0], [4, 1], [0, 2], [1, 3], [2, 4]], D)
    for bad in ([[4, 0], [3, 1], [0, 2], [1, 3], [2, 4]],            # exact tie: not enforced by values, but NaN order is:
                [[3, 0], [4, 1], [0, 3], [1, 2], [2, 4]],            # column 1 all NaN -> by row
                [[3, 0], [4, 1], [2, 2], [1, 3], [0, 4]]):           # NaN before +Inf and before 1.0
        try:
            R.check_ranked(bad, D)
            ok = True
        except AssertionError:
            ok = False
        assert ok == (bad[0][0] == 4)                                # 3 and 4 are exact duplicates: either is admissible by value
    R.check_ranked([1, 0], D, scale=-1.0)                            # scale < 0: the largest distance (+Inf, row 1) first
    with pytest.raises(AssertionError):
        R.check_ranked([0, 0], D, scale=1.0)                         # row 0 (d = 1) is not the nearest of column 0
    R.check_ranked([0, 0], D, scale=0.0)                             # scale 0: every finite logit ties -> lowest row
    with pytest.raises(AssertionError):
        R.check_ranked([3, 0], D, scale=0.0)
    # more +Inf rows than places: a NaN row may not come before any of them
    src = np.array([[np.nan]] + [[np.inf]] * 6 + [[2.0]], F32)
    D = R.pairwise(src, np.array([[1.0]], F32), "l2")
    R.check_ranked([[7], [1], [2]], D)
    with pytest.raises(AssertionError):
        R.check_ranked([[7], [1], [0]], D)
    R.check_ranked([[7], [1], [2], [3], [4], [5], [6], [0]], D)
