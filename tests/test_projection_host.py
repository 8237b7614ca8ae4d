"""CPU: the projected query's host side -- d3f_project_maps is exported, declared, bound and validates its arguments;
Fusion.add_projection folds a PCA into (W, b) as mesh.pca_project defines it, rejects what it must, and projects a source
once per observation (the library call counted through a monkeypatch); a float32 port of the route (oracle.torch_port on
the float32-projected map) calibrates the tolerance of tests/test_gpu_projection.py against the float64 reference."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import projection_cases as PC
from conftest import ROOT
from d3fields_amd import Fusion, _lib, mesh
from oracle import field_ref as R
from oracle import torch_port

# The worst |port - f64| / A of the float32 port over PC.HOST_CASES, as test_float32_port_against_float64 measures and
# prints it (A: projection_cases.py).  The GPU test's tolerance is 3 x this, capped by the worst-case rounding bound.
PORT_WORST = 5.2e-8


def test_symbol_is_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "d3fields_hip.h")).read()
    assert re.search(r"int d3f_project_maps\(const d3f_channel_map \*src, int32_t V, const float \*W, int32_t k, float \*dst,\s*void \*stream\);", hdr)
    assert hasattr(lib, "d3f_project_maps") and "d3f_project_maps" in _lib.SIGNATURES
    assert int(re.search(r"#define D3F_MAX_PROJECTION (\d+)", hdr).group(1)) == _lib.MAX_PROJECTION == 64
    assert lib.d3f_abi_version() == _lib.ABI_VERSION >= 9


def test_bad_arguments_return_status_codes():
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def cmap(**kw):
        f = dict(data=16, fh=4, fw=4, C=8, dtype=_lib.DTYPE_F32, stride_v=128, stride_y=32, stride_x=8)
        f.update(kw)
        return _lib.ChannelMap(f["data"], f["fh"], f["fw"], f["C"], f["dtype"], f["stride_v"], f["stride_y"], f["stride_x"], None)

    call = lambda m, V=2, W=one, k=3, dst=one: lib.d3f_project_maps(ctypes.byref(m) if m is not None else None, V, W, k, dst, None)
    assert call(None) == _lib.ERR_INVALID_ARG
    assert call(cmap(), W=None) == _lib.ERR_INVALID_ARG
    assert call(cmap(), dst=None) == _lib.ERR_INVALID_ARG
    assert call(cmap(data=None)) == _lib.ERR_INVALID_ARG
    assert call(cmap(), k=0) == _lib.ERR_BAD_SHAPE
    assert call(cmap(), k=65) == _lib.ERR_BAD_SHAPE and b"k=65" in lib.d3f_last_error()
    assert call(cmap(), V=0) == _lib.ERR_BAD_SHAPE
    assert call(cmap(C=0)) == _lib.ERR_BAD_SHAPE
    assert call(cmap(dtype=7)) == _lib.ERR_BAD_DTYPE
    assert call(cmap(stride_x=4)) == _lib.ERR_BAD_LAYOUT                    # texel stride below C
    assert call(cmap(data=18)) == _lib.ERR_BAD_LAYOUT                       # fp32 needs 4-byte alignment
    assert call(cmap(), W=ctypes.c_void_p(18)) == _lib.ERR_BAD_LAYOUT


# ---- registration ----------------------------------------------------------------------------------------------------------
class _Pca:
    def __init__(self, k, C, seed=0, whiten=False):
        g = np.random.default_rng(seed)
        self.components_ = g.standard_normal((k, C))
        self.mean_ = g.standard_normal(C) * 3.0
        self.explained_variance_ = g.uniform(0.5, 9.0, k)
        self.whiten = whiten


def _fusion(V=2, fh=3, fw=4, C=16, dtype=torch.float32):
    f = Fusion(num_cam=V, device="cpu")
    f.curr_obs_torch = {"depth": torch.ones(V, 6, 8), "K": torch.eye(3).repeat(V, 1, 1), "pose": torch.eye(4)[:3].repeat(V, 1, 1),
                        "dino_feats": torch.randn(V, fh, fw, C, generator=torch.Generator().manual_seed(1)).to(dtype)}
    f.H, f.W = 6, 8
    return f


def test_registration_errors_and_listing():
    f = _fusion()
    with pytest.raises(ValueError, match="curr_obs_torch"):
        f.add_projection("dino_feats", components=np.ones((3, 16)))
    with pytest.raises(ValueError, match="outside 1..64"):
        f.add_projection("p", components=np.ones((65, 16)))
    with pytest.raises(ValueError, match="outside 1..64"):
        f.add_projection("p", components=np.ones((0, 16)))
    with pytest.raises(ValueError, match="mean has shape"):
        f.add_projection("p", components=np.ones((3, 16)), mean=np.ones(15))
    with pytest.raises(ValueError):
        f.add_projection("p", components=np.ones((3, 16)), pca=_Pca(3, 16))
    with pytest.raises(ValueError, match="collide"):
        f.add_projection("x_inter", components=np.ones((3, 16)))
    f.add_projection("pca", pca=_Pca(3, 16))
    f.add_projection("head", source="dino_feats", components=torch.ones(16, 16))
    assert f.projections() == {"pca": ("dino_feats", 3), "head": ("dino_feats", 16)}
    f.remove_projection("head")
    assert f.projections() == {"pca": ("dino_feats", 3)}
    # a channel count that does not match the source is found at query time, before anything is launched
    f.add_projection("narrow", components=np.ones((3, 12)))
    with pytest.raises(ValueError, match="C=12"):
        f._projected_map("narrow", torch.device("cpu"))
    # a name that BECOMES a key of curr_obs_torch later is rejected at query time
    f.curr_obs_torch["pca"] = torch.zeros(2, 3, 4, 3)
    with pytest.raises(ValueError, match="has become a key"):
        f._projected_map("pca", torch.device("cpu"))
    # update() keeps the reference's state layout: heads never enter curr_obs_torch
    del f.curr_obs_torch["pca"]
    assert set(f.curr_obs_torch) == {"depth", "K", "pose", "dino_feats"}


class _CountingLib:
    """The loaded library with d3f_project_maps replaced by a counter (there is no device here to run it on)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def d3f_project_maps(self, desc, V, W, k, dst, stream):
        m = desc._obj
        self.calls.append((int(V), int(m.fh), int(m.fw), int(m.C), int(m.dtype), int(k)))
        return 0


def test_projection_runs_once_per_observation(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "current_stream_handle", lambda dev: None)
    cpu = torch.device("cpu")
    f = _fusion(dtype=torch.float16)
    f._lib = lib = _CountingLib(f._lib)
    f.add_projection("pca", pca=_Pca(3, 16))
    a = f._projected_map("pca", cpu)
    b = f._projected_map("pca", cpu)
    assert a is b and tuple(a.shape) == (2, 3, 4, 3) and a.dtype == torch.float32
    assert lib.calls == [(2, 3, 4, 16, _lib.DTYPE_F16, 3)]                  # two queries on the same source: one projection
    obs = {"color": np.zeros((2, 6, 8, 3), np.uint8), "depth": np.ones((2, 6, 8), np.float32), "pose": np.zeros((2, 3, 4), np.float32),
           "K": np.zeros((2, 3, 3), np.float32), "dino_feats": np.ones((2, 3, 4, 16), np.float32)}
    f.update(obs)
    assert "pca" not in f.curr_obs_torch
    c = f._projected_map("pca", cpu)
    assert len(lib.calls) == 2 and c is not a and lib.calls[1][4] == _lib.DTYPE_F32      # again after update()
    f._projected_map("pca", cpu)
    assert len(lib.calls) == 2
    f.curr_obs_torch["dino_feats"] = f.curr_obs_torch["dino_feats"].clone()
    f._projected_map("pca", cpu)
    assert len(lib.calls) == 3                                                           # the source key was replaced
    f.invalidate_map_checks()
    f._projected_map("pca", cpu)
    assert len(lib.calls) == 4                                                           # invalidate_map_checks()
    f.curr_obs_torch["dino_feats"].add_(1.0)                                             # an in-place write through torch
    f._projected_map("pca", cpu)
    assert len(lib.calls) == 5
    f.add_projection("pca", pca=_Pca(3, 16, seed=5))                                     # a new head under the same name
    f._projected_map("pca", cpu)
    assert len(lib.calls) == 6
    # a channel-range view is passed as stored (texel stride above C), not copied
    f.curr_obs_torch["wide"] = torch.zeros(2, 3, 4, 20)
    f.curr_obs_torch["dino_feats"] = f.curr_obs_torch["wide"][..., 2:18]
    f._projected_map("pca", cpu)
    assert lib.calls[-1][:4] == (2, 3, 4, 16)


# ---- W and b ---------------------------------------------------------------------------------------------------------------
def _folding_matches(f, name, pca, C):
    p = f._projections[name]
    W, b = p["W"].double(), p["b"].double()
    x = torch.randn(50, C, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 5.0
    want = mesh.pca_project(pca, x)
    got = x @ W.T - b
    mean = torch.as_tensor(np.asarray(pca.mean_, dtype=np.float64))
    A = x.abs() @ W.abs().T + mean.abs() @ W.abs().T
    # W rounded to float32 once (2^-24 of every product) and b rounded once more
    assert bool(((got - want).abs() <= 2.0 ** -23 * A).all()), float(((got - want).abs() / A).max())
    assert p["W"].dtype == torch.float32 and p["b"].dtype == torch.float32
    b64 = (p["W"].double() @ mean)
    assert torch.equal(p["b"], b64.float())                                  # b = mean W^T in float64 on the rounded W, rounded once


@pytest.mark.parametrize("whiten", [False, True])
def test_plain_object_folds_like_pca_project(whiten):
    f = _fusion()
    pca = _Pca(3, 16, seed=2, whiten=whiten)
    f.add_projection("pca", pca=pca)
    _folding_matches(f, "pca", pca, 16)
    # components / mean passed directly give the same head as the object without whitening
    if not whiten:
        f.add_projection("direct", components=pca.components_, mean=pca.mean_)
        assert torch.equal(f._projections["direct"]["W"], f._projections["pca"]["W"])
        assert torch.equal(f._projections["direct"]["b"], f._projections["pca"]["b"])
    f.add_projection("nomean", components=pca.components_)
    assert not f._projections["nomean"]["b"].any()


@pytest.mark.parametrize("whiten", [False, True])
def test_sklearn_pca_folds_like_pca_project(whiten):
    decomposition = pytest.importorskip("sklearn.decomposition")
    x = np.random.default_rng(0).standard_normal((200, 16)) * np.linspace(0.5, 4.0, 16)
    pca = decomposition.PCA(n_components=3, whiten=whiten).fit(x)
    f = _fusion()
    f.add_projection("pca", pca=pca)
    _folding_matches(f, "pca", pca, 16)
    got = torch.as_tensor(x) @ f._projections["pca"]["W"].double().T - f._projections["pca"]["b"].double()
    assert np.allclose(got.numpy(), pca.transform(x), rtol=0, atol=1e-5)


def registered_head(case):
    """(W [k,C] float32, b [k] float32) as Fusion.add_projection stores them for the case's head"""
    f = Fusion(num_cam=case["obs"]["depth"].shape[0], device="cpu")
    f.add_projection("proj", source=case["source"], components=case["head_W"], mean=case["head_mean"])
    assert f.projections() == {"proj": (case["source"], case["k"])}
    return f._projections["proj"]["W"], f._projections["proj"]["b"]


# ---- the float32 port of the route ---------------------------------------------------------------------------------------
def port_query(case):
    """The projected query in float32 torch ops on the host: the map through the head (float32 matmul), oracle.torch_port on
    the k-channel map, minus b."""
    src = case["maps"][case["source"]]
    W32, b = registered_head(case)
    pm = (src.float() @ W32.T).contiguous()
    obs = dict(case["obs"], proj=pm)
    out = torch_port.field_query(obs, case["pts"], ["proj"], case["H"], case["W"], case["mu"])
    return out["proj"] - b


def test_float32_port_against_float64():
    worst = 0.0
    print()
    for name in PC.HOST_CASES:
        case = PC.build(name)
        ref, A = PC.reference(case)
        V, C = case["obs"]["depth"].shape[0], case["maps"][case["source"]].shape[3]
        ok, w, msg = R.check(port_query(case), ref, A, tol=PC.rounding_cap(C, V))
        print("  %-28s worst |port - f64| / A = %.3g   (3 x PORT_WORST %.3g, cap %.3g)" % (name, w, 3 * PORT_WORST, PC.rounding_cap(C, V)))
        assert ok, (name, msg)
        worst = max(worst, w)
    print("  worst over the cases: %.3g (PORT_WORST %.3g)" % (worst, PORT_WORST))
    assert worst <= PORT_WORST, "the stored constant no longer covers the port: measured %.3g" % worst
    assert worst >= PORT_WORST / 4, "the stored constant is stale: measured %.3g" % worst


def test_mutants_fail_the_assertion():
    """In the style of test_field_ref.py::test_mutants_pass_rel_err_and_fail_the_pin: a dropped channel, an unsubtracted b and
    the mean applied per view before weighting each stay inside the norm-wise rel_err <= 1e-5 ... or not, but all FAIL the
    per-entry assertion, while the float64 value rounded to float32 passes.  This tests the ASSERTION of
    tests/test_gpu_projection.py (reference, magnitude A and tolerance) with the head as add_projection registers it; it needs
    no device."""
    case = PC.build("patch V4 C384 k3")
    W32, b32 = registered_head(case)
    assert torch.equal(W32, case["head_W"])
    m = case["maps"][case["source"]]
    vals, scales = R.field64(case["obs"], case["pts"], case["H"], case["W"], case["mu"], [m, torch.ones(m.shape[:3] + (1,))])
    v, s, weight_sum = vals[0], scales[0], vals[1]                                 # weight_sum[n,1] = sum_v s_v (in-bounds corners)
    W64, mean = case["head_W"].double(), case["head_mean"]
    ref, A = PC.project64(v, s, case["head_W"], mean)
    tol = PC.tolerance(PORT_WORST, m.shape[3], m.shape[0])
    assert R.check(ref.float(), ref, A, tol=tol)[0]
    b = b32.double()                                                               # the constant the product subtracts
    contrib = (v.abs().amax(0) * W64.abs().amax(0))                                # the channel that matters most
    c = int(contrib.argmax())
    mutants = {"a dropped channel": ref - v[:, c:c + 1] * W64[:, c],
               "the last channel dropped": ref - v[:, -1:] * W64[:, -1],
               "b not subtracted": ref + b,
               "mean applied per view before weighting": v @ W64.T - weight_sum * b}
    for what, got in mutants.items():
        ok, worst, msg = R.check(got.float(), ref, A, tol=tol)
        print("  mutant %-42s worst ratio %.3g (tol %.3g)" % (what, worst, tol))
        assert not ok, what


def test_descriptor_colours_float32_port_under_the_cap():
    """mesh.descriptor_colors where its inputs live (here: the host, float32) against the float64 colour rule as an
    admissible set; these are the inputs the GPU test uses."""
    proj, mask = PC.colour_inputs()
    got = mesh.descriptor_colors(proj, mask, mask_out_bg=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (proj.shape[0], 4) and bool((got[:, 3] == 255).all())
    ok, share, msg = PC.check_colours(got, proj, mask)
    print("\n  share of bytes that differ from the float64 rule's byte: %.3g" % share)
    assert ok, msg
    bg = mask.argmax(1) == 0
    assert bool((got[bg][:, :3] == 204).all()) and bool(bg.any())
    # BGR: the first component drives the LAST colour byte
    top = int(proj[:, 0].masked_fill(bg, -1e9).argmax())
    assert int(got[top, 2]) == 255
