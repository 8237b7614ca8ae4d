"""The PCA fit on the device (d3fields_amd/pca.py, d3f_row_moments) against the float64 definition, entry by entry.

Reference: tests/pca_cases.py: moments64.  |scatter - S64|_ij <= tol A_ij with A_ij = sum w |x_i - mean_i| |x_j - mean_j|, and
|mean - mean64|_c <= tol_mean sum w |x_c| / wsum.  tol = 3 x the worst ratio of the float32 port of the route measured on the
host (tests/test_pca_fit_host.py: PORT_WORST = 4.2e-7, PORT_WORST_MEAN = 1.6e-7), capped by the a-priori bounds of the route,
(64 + 4) 2^-24 and (32 + 2) 2^-24.  Components follow by the Davis-Kahan bound."""
import functools

import numpy as np
import pytest
import torch

import pca_cases as PC
from test_pca_fit_host import PORT_WORST, PORT_WORST_MEAN

pytestmark = pytest.mark.gpu

TOL = PC.tol_scatter(PORT_WORST)
TOL_MEAN = PC.tol_mean(PORT_WORST_MEAN)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on_device(case, dev):
    """rows on the device with the case's strides and base offset kept (a view stays a view of a wider device tensor)"""
    rows = case["rows"]
    if rows.is_contiguous():
        r = rows.to(dev)
    else:
        base = rows._base.to(dev)
        r = base.as_strided(rows.shape, rows.stride(), rows.storage_offset())
        assert r.stride() == rows.stride() and not r.is_contiguous()
    w = case["weights"]
    return r, (None if w is None else w.to(dev))


@functools.lru_cache(maxsize=None)
def device_moments(name):
    from d3fields_amd import pca
    dev = torch.device("cuda:0")
    r, w = on_device(PC.build(name), dev)
    out = pca.row_moments(r, w)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(PC.CASES))
def test_moments_against_float64(dev, name):
    wsum, mean, S = device_moments(name)
    assert S.is_cuda and S.dtype == mean.dtype == wsum.dtype == torch.float64
    wsum64, mean64, S64, A, a = PC.reference(name)
    C = S64.shape[0]
    assert tuple(S.shape) == (C, C) and tuple(mean.shape) == (C,) and wsum.dim() == 0
    ok_s, rs = PC.check(S, S64, A, TOL)
    ok_m, rm = PC.check(mean, mean64, a, TOL_MEAN)
    print("\n  %-26s scatter worst |got - f64| / A = %.3g (tol %.3g)   mean %.3g (tol %.3g)" % (name, rs, TOL, rm, TOL_MEAN))
    assert abs(float(wsum) - float(wsum64)) <= PC.CAP_MEAN * float(wsum64)
    assert ok_m, (name, "mean", rm)
    assert ok_s, (name, "scatter", rs)
    assert torch.equal(S, S.T), "scatter must be bitwise symmetric"


@pytest.mark.parametrize("name", ["C3 M257", "C384 M4099 mask", "C1024 M3001 soft", "C384 map slice unaligned"])
def test_two_runs_are_bit_identical(dev, name):
    from d3fields_amd import pca
    r, w = on_device(PC.build(name), dev)
    first = device_moments(name)
    again = pca.row_moments(r, w)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), name


def test_no_weights_equal_all_ones(dev):
    from d3fields_amd import pca
    for name in ("C3 M257", "C129 M1537", "C129 M1537 f16"):
        r, _ = on_device(PC.build(name), dev)
        ones = pca.row_moments(r, torch.ones(r.shape[0], device=dev))
        as_bool = pca.row_moments(r, torch.ones(r.shape[0], dtype=torch.bool, device=dev))
        assert all(torch.equal(a, b) for a, b in zip(device_moments(name), ones)), name
        assert all(torch.equal(a, b) for a, b in zip(ones, as_bool)), name


def test_mask_equals_the_gathered_subset(dev):
    from d3fields_amd import pca
    name = "C384 M4099 mask"
    r, w = on_device(PC.build(name), dev)
    wsum, mean, S = pca.row_moments(r[w].contiguous())
    wsum64, mean64, S64, A, a = PC.reference(name)
    assert float(wsum) == float(wsum64) == float(device_moments(name)[0])
    ok_s, rs = PC.check(S, S64, A, TOL)
    ok_m, rm = PC.check(mean, mean64, a, TOL_MEAN)
    print("\n  gathered subset: scatter ratio %.3g, mean ratio %.3g" % (rs, rm))
    assert ok_s and ok_m
    # uint8 weights are the same selection
    assert all(torch.equal(x, y) for x, y in zip(device_moments(name), pca.row_moments(r, w.to(torch.uint8))))


def test_map_shape_equals_flat_rows_and_non_finite_rows_show(dev):
    from d3fields_amd import pca
    x = PC.build("C129 M1537")["rows"][:1536].to(dev)
    flat = pca.row_moments(x)
    as_map = pca.row_moments(x.reshape(4, 12, 32, 129))
    assert all(torch.equal(a, b) for a, b in zip(flat, as_map))
    bad = x.clone()
    bad[700, 5] = float("nan")
    w = torch.ones(1536, device=dev)
    w[700] = 0.0
    wsum, mean, S = pca.row_moments(bad, w)                    # dense arithmetic: 0 * NaN = NaN
    assert bool(torch.isnan(mean[5])) and bool(torch.isnan(S[5]).all()) and bool(torch.isnan(S[:, 5]).all())
    assert bool(torch.isfinite(mean[:5]).all()) and bool(torch.isfinite(S[:5, :5]).all())
    with pytest.raises(ValueError, match="non-finite"):
        pca.fit_pca(bad, 3, weights=w)
    with pytest.raises(ValueError, match="non-finite"):
        pca.fit_pca(x, 3, weights=torch.zeros(1536, device=dev))
    with pytest.raises(ValueError, match="negative"):
        pca.row_moments(x, -w)


@pytest.mark.parametrize("name", PC.SPECTRUM_CASES)
def test_components_against_float64_eigenvectors(dev, name):
    from d3fields_amd import pca
    k = 4
    r, w = on_device(PC.build(name), dev)
    fitted = pca.fit_pca(r, n_components=k, weights=w)
    wsum64, mean64, S64, A, _ = PC.reference(name)
    lam, v64, gap = PC.spectrum64(S64, k)
    normA = float(torch.linalg.norm(A))
    comp = torch.from_numpy(fitted.components_)
    print()
    for i in range(k):
        dist = float(torch.linalg.norm(comp[i] - v64[i]))
        bound = 2.0 * TOL * normA / float(gap[i])               # Davis-Kahan: sin(theta) <= 2 |E|_F / gap
        rel = abs(fitted.explained_variance_[i] * (float(wsum64) - 1.0) - float(lam[i])) / float(lam[i])
        print("  %-22s component %d: |v - v64| = %.3g (bound %.3g)   eigenvalue rel %.3g (bound %.3g)" % (name, i, dist, bound, rel, TOL * normA / float(lam[i])))
        assert dist <= bound, (name, i, dist, bound)
        assert rel <= TOL * normA / float(lam[i]), (name, i, rel)
    assert (fitted.n_components_, fitted.n_features_in_) == (k, S64.shape[0]) and abs(fitted.n_samples_ - float(wsum64)) <= PC.CAP_MEAN * float(wsum64)
    assert np.allclose(fitted.singular_values_ ** 2, fitted.explained_variance_ * (fitted.n_samples_ - 1.0), rtol=1e-12, atol=0)


def test_device_result_fails_the_mutated_definitions(dev):
    """The device's scatter passes against the definition (above) and fails against each mutant of it on at least one case."""
    failed = {m: [] for m in PC.MUTANTS}
    for name in ("C3 M257", "C384 M4099 mask", "C1024 M3001 soft"):
        x, w = PC.flat(PC.build(name))
        S = device_moments(name)[2]
        for m in PC.MUTANTS:
            _, _, Sm, Am, _ = PC.moments64(x, w, mutant=m)
            if not PC.check(S, Sm, Am, TOL)[0]:
                failed[m].append(name)
    assert all(failed[m] for m in PC.MUTANTS), failed


def test_fit_projection_end_to_end(dev):
    from d3fields_amd import Fusion, mesh
    sc, feats, pts, H, W = PC.scene()

    def fusion():
        f = Fusion(num_cam=feats.shape[0], device=str(dev))
        f.curr_obs_torch = {"depth": sc["depth"].to(dev), "K": sc["K"].to(dev), "pose": sc["pose"].to(dev), "dino_feats": feats.to(dev),
                            "mask": torch.nn.functional.one_hot(torch.randint(0, 3, (feats.shape[0], H, W), generator=torch.Generator().manual_seed(2)), 3).float().to(dev)}
        f.H, f.W = H, W
        return f

    f = fusion()
    fg = torch.rand(feats.shape[:3], generator=torch.Generator().manual_seed(4)) < 0.6
    fitted = f.fit_projection("p", source="dino_feats", n_components=3, weights=fg.to(dev))
    assert f.projections()["p"] == ("dino_feats", 3)
    assert fitted.components_.shape == (3, feats.shape[3]) and fitted.n_samples_ == float(fg.sum())
    with torch.no_grad():
        out = f.batch_eval(pts.to(dev), return_names=["p", "dino_feats", "mask"])
    fresh = fusion()
    fresh.add_projection("p", "dino_feats", pca=fitted)
    with torch.no_grad():
        want = fresh.batch_eval(pts.to(dev), return_names=["p"])
    assert tuple(out["p"].shape) == (pts.shape[0], 3) and torch.equal(out["p"], want["p"])
    # the fit is the float64 fit of the selected texels
    x = feats.reshape(-1, feats.shape[3])
    _, _, S64, A, _ = PC.moments64(x, fg.reshape(-1).to(torch.float64))
    lam, v64, gap = PC.spectrum64(S64, 3)
    for i in range(3):
        assert float(torch.linalg.norm(torch.from_numpy(fitted.components_[i]) - v64[i])) <= 2.0 * TOL * float(torch.linalg.norm(A)) / float(gap[i])
    # and the object passes through descriptor_mesh as the reference's pickled PCA does
    n = pts.shape[0] // 3 * 3
    res = {"dino_feats": out["dino_feats"][:n], "mask": out["mask"][:n]}
    tri = torch.arange(n, device=dev).reshape(-1, 3)
    m = mesh.descriptor_mesh(pts[:n].to(dev), tri, res, {"pca": fitted}, True)
    assert m is not None
    proj = fitted.transform(out["dino_feats"][:n])
    assert tuple(proj.shape) == (n, 3) and torch.allclose(proj.float(), out["p"][:n], rtol=0, atol=1e-3 * float(proj.abs().max()))
