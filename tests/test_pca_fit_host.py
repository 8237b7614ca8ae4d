"""CPU: the host side of the PCA fit -- d3f_row_moments is exported, declared, bound, built and validates its arguments;
pca_from_moments agrees with sklearn's full-SVD PCA including the signs; a whitened fit folds into add_projection as sklearn's
transform; every ValueError is raised; the float32 port of the kernel's route (tests/pca_cases.py: port32) calibrates the
tolerance of tests/test_gpu_pca_fit.py against the float64 definition; and the definition's mutants fail that assertion."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pca_cases as PC
from conftest import ROOT
from d3fields_amd import Fusion, _lib, build, mesh, pca

# The worst |port - f64| / A (scatter) and / a (mean) of the float32 port over PC.CASES, as test_float32_port_against_float64
# measures and prints them.  The GPU test's tolerances are 3 x these, capped by the a-priori bounds PC.CAP_SCATTER / PC.CAP_MEAN.
PORT_WORST = 4.2e-7
PORT_WORST_MEAN = 1.6e-7


def test_symbols_are_exported_declared_bound_and_built():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "d3fields_hip.h")).read()
    assert re.search(r"int64_t d3f_row_moments_workspace_bytes\(int64_t M, int32_t C\);", hdr)
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int d3f_row_moments\(const void \*rows, int32_t dtype, int64_t M, int32_t C, int64_t row_stride,\s*const float \*weights\s*,"
                     r"\s*double \*wsum_out\s*, double \*mean_out\s*, double \*scatter_out\s*,\s*void \*workspace, int64_t workspace_bytes, void \*stream\);", flat)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _lib.SIGNATURES["d3f_row_moments_workspace_bytes"] == (i64, [i64, i32])
    assert _lib.SIGNATURES["d3f_row_moments"] == (ctypes.c_int, [vp, i32, i64, i32, i64, vp, vp, vp, vp, vp, i64, vp])
    assert hasattr(lib, "d3f_row_moments") and hasattr(lib, "d3f_row_moments_workspace_bytes")
    assert int(re.search(r"#define D3F_MAX_MOMENT_CHANNELS (\d+)", hdr).group(1)) == _lib.MAX_MOMENT_CHANNELS == 2048
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) >= 10
    assert "moment_kernels.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "moment_kernels.hip"))


def test_bad_arguments_return_status_codes():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    need = lib.d3f_row_moments_workspace_bytes(1000, 384)
    assert need > 0 and need % 16 == 0
    assert lib.d3f_row_moments_workspace_bytes(1000, 384) == need                      # a function of (M, C) alone
    assert lib.d3f_row_moments_workspace_bytes(0, 384) == 0 and lib.d3f_row_moments_workspace_bytes(10, 2049) == 0

    def call(rows=one, dtype=_lib.DTYPE_F32, M=1000, C=384, stride=384, w=None, out=one, ws=one, nbytes=need):
        return lib.d3f_row_moments(rows, dtype, M, C, stride, w, out, out, out, ws, nbytes, None)

    assert call(C=0) == _lib.ERR_BAD_SHAPE
    assert call(C=2049, stride=2049) == _lib.ERR_BAD_SHAPE and b"C=2049" in lib.d3f_last_error()
    assert call(M=0) == _lib.ERR_BAD_SHAPE
    assert call(stride=383) == _lib.ERR_BAD_LAYOUT
    assert call(dtype=7) == _lib.ERR_BAD_DTYPE
    assert call(ws=None) == _lib.ERR_WORKSPACE
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(rows=None) == _lib.ERR_INVALID_ARG
    assert call(out=None) == _lib.ERR_INVALID_ARG
    assert call(rows=ctypes.c_void_p(258)) == _lib.ERR_BAD_LAYOUT                      # fp32 rows need 4-byte alignment
    assert call(out=ctypes.c_void_p(260)) == _lib.ERR_BAD_LAYOUT                       # float64 outputs need 8


# ---- the float32 port of the route -------------------------------------------------------------------------------------
def test_float32_port_against_float64():
    worst_s = worst_m = 0.0
    print()
    for name in PC.CASES:
        x, w = PC.flat(PC.build(name))
        wsum64, mean64, S64, A, a = PC.reference(name)
        wsum, mean, S, cols = PC.port32(x, w)
        ok_s, rs = PC.check(S, S64[:, cols], A[:, cols], PC.CAP_SCATTER)
        ok_m, rm = PC.check(mean, mean64, a, PC.CAP_MEAN)
        print("  %-26s scatter worst |port - f64| / A = %.3g (cap %.3g)   mean %.3g (cap %.3g)" % (name, rs, PC.CAP_SCATTER, rm, PC.CAP_MEAN))
        assert ok_s and ok_m, name
        assert abs(float(wsum - wsum64)) <= PC.CAP_MEAN * float(wsum64)
        worst_s, worst_m = max(worst_s, rs), max(worst_m, rm)
    print("  worst over the cases: scatter %.3g (PORT_WORST %.3g), mean %.3g (PORT_WORST_MEAN %.3g)" % (worst_s, PORT_WORST, worst_m, PORT_WORST_MEAN))
    assert PORT_WORST / 4 <= worst_s <= PORT_WORST, "PORT_WORST does not describe the port: measured %.3g" % worst_s
    assert PORT_WORST_MEAN / 4 <= worst_m <= PORT_WORST_MEAN, "PORT_WORST_MEAN does not describe the port: measured %.3g" % worst_m


def test_mutants_fail_the_entry_check():
    """The float64 definition rounded to float32 passes the assertion of the GPU test; scatter about zero, weights ignored and
    weights squared each fail it on at least one case."""
    tol = PC.tol_scatter(PORT_WORST)
    failed = {m: [] for m in PC.MUTANTS}
    for name in ("C3 M257", "C129 M1537", "C384 M4099 mask", "C1024 M3001 soft"):
        x, w = PC.flat(PC.build(name))
        _, _, S64, A, _ = PC.reference(name)
        assert PC.check(S64.float(), S64, A, tol)[0], name
        for m in PC.MUTANTS:
            ok, worst = PC.check(PC.moments64(x, w, mutant=m)[2], S64, A, tol)
            if not ok:
                failed[m].append(name)
    print("\n  cases each mutant fails on: %s" % failed)
    assert all(failed[m] for m in PC.MUTANTS), failed
    assert "C3 M257" in failed["about zero"] and "C384 M4099 mask" in failed["weights ignored"] and "C1024 M3001 soft" in failed["weights squared"]


# ---- the eigen-problem -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.MASK_CASES + ("C129 M1537",))
def test_pca_from_moments_matches_sklearn(name):
    decomposition = pytest.importorskip("sklearn.decomposition")
    x, w = PC.flat(PC.build(name))
    kept = x.to(torch.float64) if w is None else x.to(torch.float64)[w > 0]
    wsum, mean, S, _, _ = PC.reference(name)
    fitted = pca.pca_from_moments(wsum, mean, S, 4)
    sk = decomposition.PCA(n_components=4, svd_solver="full").fit(kept.numpy())
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
    for attr in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
        assert rel(getattr(fitted, attr), getattr(sk, attr)) <= 1e-10, (attr, rel(getattr(fitted, attr), getattr(sk, attr)))
    assert (fitted.n_components_, fitted.n_features_in_, fitted.n_samples_, fitted.whiten) == (4, x.shape[1], float(kept.shape[0]), False)
    assert np.allclose(np.linalg.norm(fitted.components_, axis=1), 1.0, rtol=0, atol=1e-12)
    y = fitted.transform(kept[:50])
    assert float(np.abs(y.numpy() - sk.transform(kept[:50].numpy())).max()) <= 1e-9


def test_cpu_rows_take_the_float64_definition():
    case = PC.build("C384 map slice")
    wsum, mean, S = pca.row_moments(case["rows"])
    wsum64, mean64, S64, _, _ = PC.reference("C384 map slice")
    assert S.dtype == torch.float64 and tuple(S.shape) == (384, 384) and tuple(mean.shape) == (384,)
    assert float(wsum) == float(wsum64) == 70.0 and torch.allclose(mean, mean64, rtol=0, atol=1e-12) and torch.allclose(S, S64, rtol=1e-12, atol=1e-9)
    w = torch.rand(2, 5, 7, generator=torch.Generator().manual_seed(1)) < 0.5
    a = pca.row_moments(case["rows"], weights=w)
    b = pca.row_moments(case["rows"][w])
    assert float(a[0]) == float(w.sum()) and torch.allclose(a[2], b[2], rtol=1e-12, atol=1e-9)
    fitted = pca.fit_pca(PC.build("C129 M1537")["rows"], n_components=3)
    assert fitted.components_.shape == (3, 129)


def test_whitened_fit_folds_into_add_projection_like_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    x = PC.build("C129 M1537")["rows"].to(torch.float64)
    fitted = pca.fit_pca(PC.build("C129 M1537")["rows"], n_components=3, whiten=True)
    sk = decomposition.PCA(n_components=3, svd_solver="full", whiten=True).fit(x.numpy())
    f = Fusion(num_cam=2, device="cpu")
    f.add_projection("p", pca=fitted)
    assert f.projections() == {"p": ("dino_feats", 3)}
    p = f._projections["p"]
    got = x[:200] @ p["W"].double().T - p["b"].double()
    want = torch.from_numpy(sk.transform(x[:200].numpy()))
    W64 = p["W"].double()
    A = x[:200].abs() @ W64.abs().T + torch.from_numpy(sk.mean_).abs() @ W64.abs().T
    assert bool(((got - want).abs() <= 2.0 ** -22 * A).all()), float(((got - want).abs() / A).max())       # W and b rounded to float32 once
    assert torch.allclose(mesh.pca_project(fitted, x[:200]), want, rtol=0, atol=1e-9)


def test_value_errors():
    x = PC.build("C129 M1537")["rows"]
    with pytest.raises(ValueError, match="weights have shape"):
        pca.row_moments(x, weights=torch.ones(5))
    with pytest.raises(ValueError, match="negative"):
        pca.row_moments(x, weights=-torch.ones(x.shape[0]))
    with pytest.raises(ValueError, match="outside 1..2048"):
        pca.row_moments(torch.zeros(4, 2049))
    with pytest.raises(ValueError, match="must be a"):
        pca.row_moments(torch.zeros(4, 3, 5))
    with pytest.raises(ValueError, match="float32 or float16"):
        pca.row_moments(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="bool, uint8 or float"):
        pca.row_moments(x, weights=torch.ones(x.shape[0], dtype=torch.int64))
    with pytest.raises(ValueError, match="more than one sample"):
        pca.fit_pca(x[:1], n_components=1)                                         # M = 1
    with pytest.raises(ValueError, match="non-finite"):
        pca.fit_pca(x, n_components=1, weights=torch.zeros(x.shape[0]))            # all weights zero: NaN means
    wsum, mean, S, _, _ = PC.reference("C129 M1537")
    with pytest.raises(ValueError, match="n_components"):
        pca.pca_from_moments(wsum, mean, S, 130)
    with pytest.raises(ValueError, match="non-finite"):
        bad = S.clone()
        bad[3, 4] = float("nan")
        pca.pca_from_moments(wsum, mean, bad, 3)
    with pytest.raises(ValueError, match="more than one sample"):
        pca.pca_from_moments(1.0, mean, S, 3)
    # Fusion.fit_projection rejects what add_projection rejects, and more components than a head may have
    f = Fusion(num_cam=2, device="cpu")
    f.curr_obs_torch = {"dino_feats": x[:140].reshape(2, 7, 10, 129).clone()}
    with pytest.raises(ValueError, match="curr_obs_torch"):
        f.fit_projection("dino_feats")
    with pytest.raises(ValueError, match="collide"):
        f.fit_projection("x_inter")
    with pytest.raises(ValueError, match="outside 1..64"):
        f.fit_projection("p", n_components=65)
    with pytest.raises(KeyError):
        f.fit_projection("p", source="nothing")
    with pytest.raises(ValueError, match="weights have shape"):
        f.fit_projection("p", weights=torch.ones(2, 7))
    fitted = f.fit_projection("p", n_components=3, weights=torch.ones(2, 7, 10, dtype=torch.bool))
    assert f.projections() == {"p": ("dino_feats", 3)} and fitted.n_samples_ == 140.0
