"""CPU: channel sets stored as IEEE half (d3f_volume_set.reserved = D3F_DTYPE_F16) -- the header and the binding,
the status codes of the nine entry points that take a set (nothing is launched: every call ends in a status or has n == 0), the case
generator, and BakedField's storage surface on host tensors with the call path into the library made to fail."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import volume_f16_cases as HC
from d3fields_amd import BakedField, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")


@pytest.fixture(scope="module")
def lib():
    """On a library that ignores the storage word, a call with a word of 1 or 7 and otherwise valid fake pointers would LAUNCH.  The Python
    surface and the library's check arrived together: without the former no call of this module is made."""
    assert hasattr(BakedField, "half") and hasattr(BakedField, "rows_dtype"), "this build has no half storage: no call with a storage word is made"
    return _lib.load()


# ---- header and binding ---------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    hdr = open(HEADER).read()
    # the struct keeps its text (tests/test_volume_host.py's pattern) and its layout
    m = re.search(r"typedef struct d3f_volume_set \{\s*const float \*data;\s*int32_t C;\s*int32_t reserved;[^}]*int64_t stride_voxel;\s*"
                  r"const float \*fill;[^}]*\} d3f_volume_set;", hdr)
    assert m
    S = _lib.VolumeSet
    assert ctypes.sizeof(S) == 32 and (S.data.offset, S.C.offset, S.reserved.offset, S.stride_voxel.offset, S.fill.offset) == (0, 8, 12, 16, 24)
    # both storage values are documented next to the struct: in the comment right above it and at the word itself
    above = hdr[:m.start()].rsplit("/*", 1)[1]
    assert above.rstrip().endswith("*/") and "D3F_DTYPE_F32 (0)" in above and "D3F_DTYPE_F16 (1)" in above
    assert "D3F_ERR_BAD_DTYPE" in above and "D3F_ERR_BAD_LAYOUT" in above and "2-byte aligned" in above and "ELEMENTS" in above
    assert "D3F_DTYPE_F32" in m.group(0) and "D3F_DTYPE_F16" in m.group(0)
    assert int(re.search(r"#define D3F_DTYPE_F32 (\d+)", hdr).group(1)) == _lib.DTYPE_F32 == 0
    assert int(re.search(r"#define D3F_DTYPE_F16 (\d+)", hdr).group(1)) == _lib.DTYPE_F16 == 1
    # no new exported function, no new size function, the same ABI
    assert len(_lib.SIGNATURES) == 106 and len(_lib.STREAMED) == 72
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 16
    sized = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    assert sized == sorted(set(re.findall(r"\b(d3f_\w+_workspace_bytes)\(", hdr)))
    assert not [n for n in _lib.SIGNATURES if "f16" in n or "half" in n]


# ---- status codes ---------------------------------------------------------------------------------------------------------------
P = 256                      # a fake device address, 16-byte aligned; no call below reads through it
V = ctypes.c_void_p


def _vol(shape=(4, 5, 6)):
    return _lib.Volume(shape[0], shape[1], shape[2], (ctypes.c_float * 3)(0, 0, 0), 0.5, 0, V(P), V(P), V(P))


def _set(word, data=P, C=8):
    return _lib.VolumeSet(data, C, word, C, None)


def _calls(lib):
    """name -> (accepts half?, call(word, data=P, n=5)) for the nine entry points that take a set"""
    outs = (ctypes.c_void_p * 1)(P)
    band = _lib.Band(V(P), V(P), 7)

    def sample(word, data=P, n=5):
        return lib.d3f_volume_sample(ctypes.byref(_vol()), V(P), n, (_lib.VolumeSet * 1)(_set(word, data)), 1, V(P), V(P), outs, None)

    def sample_backward(word, data=P, n=5):
        return lib.d3f_volume_sample_backward(ctypes.byref(_vol()), V(P), n, (_lib.VolumeSet * 1)(_set(word, data)), 1, None, outs, V(P), None)

    def band_sample(word, data=P, n=5):
        return lib.d3f_band_sample(ctypes.byref(_vol()), ctypes.byref(band), V(P), n, (_lib.VolumeSet * 1)(_set(word, data)), 1, V(P), V(P), V(P), outs, None)

    def band_sample_backward(word, data=P, n=5):
        return lib.d3f_band_sample_backward(ctypes.byref(_vol()), ctypes.byref(band), V(P), n, (_lib.VolumeSet * 1)(_set(word, data)), 1, None, outs, V(P), None)

    def pool(word, data=P, n=5):
        modes = (ctypes.c_int32 * 1)(_lib.POOL_MEAN)
        return lib.d3f_volume_pool(V(P), 4, 5, 6, 3, None, None, (_lib.VolumeSet * 1)(_set(word, data)), 1, modes, 50, V(P), V(P), V(P), outs, V(P), 1 << 62, None)

    def links(word, data=P, n=5):
        st = _set(word, data)
        return lib.d3f_volume_links(V(P), None, None, 4, 5, 6, ctypes.byref(st), _lib.LINK_L2, 1.0, 26, V(P), None)

    def flow_a(word, data=P, n=5):
        sa, sb = _set(word, data), _set(0)
        return lib.d3f_volume_flow(V(P), None, ctypes.byref(sa), V(P), None, ctypes.byref(sb), 4, 5, 6, 2, float("inf"), V(P), V(P), None, None)

    def flow_b(word, data=P, n=5):
        sa, sb = _set(0), _set(word, data)
        return lib.d3f_volume_flow(V(P), None, ctypes.byref(sa), V(P), None, ctypes.byref(sb), 4, 5, 6, 2, float("inf"), V(P), V(P), None, None)

    def align(word, data=P, n=5):
        st, vol = _set(word, data), _vol()
        return lib.d3f_volume_align_accumulate(ctypes.byref(vol), None, ctypes.byref(st), V(P), None, V(P), None, V(P), V(P), None, 2, n, 1.0, 1.0, 0.1, V(P), V(P),
                                               1 << 20, None)

    def warp_rows(word, data=P, n=5):
        vol = _lib.Volume(4, 5, 6, (ctypes.c_float * 3)(0, 0, 0), 1.0, 0, None, None, None)
        a = _lib.WarpRows(vol, None, (_lib.VolumeSet * 1)(_set(word, data)), 1, 3, V(P), V(P), V(P), 10, outs, V(P))
        return lib.d3f_volume_warp_rows(ctypes.byref(a), None)

    return {"volume_sample": (True, sample), "volume_sample_backward": (True, sample_backward), "band_sample": (True, band_sample),
            "band_sample_backward": (True, band_sample_backward), "volume_pool": (False, pool), "volume_links": (False, links),
            "volume_flow set_a": (False, flow_a), "volume_flow set_b": (False, flow_b), "volume_align_accumulate": (False, align),
            "volume_warp_rows": (False, warp_rows)}


def test_an_unknown_storage_word_is_bad_dtype_everywhere(lib):
    calls = _calls(lib)
    assert len({k.split()[0] for k in calls}) == 9
    for name, (_, call) in calls.items():
        assert call(7) == _lib.ERR_BAD_DTYPE, name
        msg = lib.d3f_last_error()
        assert name.split()[0].encode() in msg and b"set " in msg and b"storage word 7" in msg, (name, msg)
        assert call(-1) == _lib.ERR_BAD_DTYPE and call(2) == _lib.ERR_BAD_DTYPE, name


def test_entry_points_with_row_loops_of_their_own_refuse_half(lib):
    for name, (accepts, call) in _calls(lib).items():
        if accepts:
            continue
        assert call(_lib.DTYPE_F16) == _lib.ERR_BAD_DTYPE, name
        msg = lib.d3f_last_error()
        assert name.split()[0].encode() in msg and b"half" in msg and b"float32" in msg, (name, msg)
        which = b"set 1" if name.endswith("set_b") else b"set 0"
        assert which in msg, (name, msg)


def test_the_lookups_take_half_with_its_two_byte_rule(lib):
    for name, (accepts, call) in _calls(lib).items():
        if not accepts:
            continue
        assert call(_lib.DTYPE_F16, data=P + 1) == _lib.ERR_BAD_LAYOUT, name
        assert b"2-byte aligned" in lib.d3f_last_error(), name
        assert call(_lib.DTYPE_F32, data=P + 2) == _lib.ERR_BAD_LAYOUT and b"4-byte aligned" in lib.d3f_last_error(), name      # (unchanged)
        assert call(_lib.DTYPE_F16, n=0) == _lib.OK, name
        assert call(7, n=0) == _lib.ERR_BAD_DTYPE, name                     # the word is checked with the set's shape, before "nothing to do"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_cases_widen_exactly_and_hold_what_they_plant():
    vol = HC.case("5x4x6", (8, 136), 3, 0.2, True, (0,))
    for k, bits in vol["bits"].items():
        wide = vol["sets"][k]
        assert bits.dtype == np.uint16 and wide.dtype == np.float32 and wide.shape == bits.shape
        # widening is exact and half().float() is the identity: through NumPy and through torch
        assert np.array_equal(wide.astype(np.float16).view(np.uint16)[~np.isnan(wide)], bits[~np.isnan(wide)])
        t = torch.from_numpy(bits.view(np.float16).copy())
        assert torch.equal(t.to(torch.float32).view(torch.int32), torch.from_numpy(wide).view(torch.int32))
        assert torch.equal(t.to(torch.float32).to(torch.float16).view(torch.int16), t.view(torch.int16))
        ok = vol["valid"]
        stored = bits[ok]
        for value in HC.PLANTED:
            assert (stored == value).any(), (k, hex(value))
        assert ((stored & 0x7C00) == 0).sum() > len(HC.PLANTED)              # random subnormals too
        assert ((stored & 0x7C00) != 0x7C00).all()                           # every valid voxel is finite
        # the cell whose chain ends in -0
        assert all(ok[c] for c in HC.CELL0) and bits[0, 0, 0, 0] == HC.H_NEG_ZERO
        assert all(bits[c + (0,)] & 0x8000 for c in HC.CELL0)
        # invalid voxels are poisoned
        assert (~ok).any() and np.isin(bits[~ok], (HC.H_NAN, HC.H_INF, HC.H_NINF)).all() and np.isnan(vol["dist"][~ok]).all()
    # the chain at the lattice point (0, 0, 0): -0 with a plain first multiply, +0 with a fused one
    v = np.asarray([vol["sets"]["s0"][c + (0,)] for c in HC.CELL0], np.float32)
    w = np.asarray([1, 0, 0, 0, 0, 0, 0, 0], np.float32)
    out = w[0] * v[0]
    for c in range(1, 8):
        out = np.float32(np.float64(w[c]) * np.float64(v[c]) + np.float64(out))
    assert out == 0 and np.signbit(out)
    assert not np.signbit(np.float32(np.float64(w[0]) * np.float64(v[0]) + 0.0))
    port = VC_trilinear32_at_origin(vol)
    assert port == 0 and np.signbit(port)
    # the points: (0, 0, 0) first, then t = 0 and t = 1 on every axis among the rest
    pts = HC.points(vol["shape"], 257, 3)
    assert pts.shape == (257, 3) and np.array_equal(pts[0], HC.lattice_points(vol["shape"])[0]) and np.isnan(pts).any()
    m = HC.mark(vol, HC.band_of(vol))
    assert 0 < m["M"] < int(vol["valid"].sum())


def VC_trilinear32_at_origin(vol):
    import volume_cases as VC
    return VC.trilinear32(vol, HC.lattice_points(vol["shape"])[:1])["s0"][0, 0]


# ---- BakedField on host tensors ---------------------------------------------------------------------------------------------------
class _DeviceTensor(torch.Tensor):
    """a host tensor that says it lives on cuda:0 (as tests/test_call_host.py's)"""
    device = property(lambda self: torch.device("cuda", 0))
    is_cuda = property(lambda self: True)


def _init_without_library(self, origin, step, dist, valid, sets, fills, boundaries=None, axes=None):
    self.origin, self.step, self.grid_shape = tuple(float(o) for o in origin), float(step), torch.Size(dist.shape)
    self.dist, self.valid, self._sets, self._fills = dist, valid, dict(sets), dict(fills)
    self.boundaries, self.device, self._lib, self._axes, self.cell_valid = {}, dist.device, None, axes, None
    for k in ("band", "slot", "cell_band", "band_voxels", "d2", "nearest_voxel", "sites", "cost", "next_voxel", "free", "source", "rows_known",
              "part_box_from", "part_box_to"):
        setattr(self, k, None)


@pytest.fixture
def host_field(monkeypatch):
    """from_arrays on host tensors: the constructor's one library call is left out, and ANY use of the call path fails the test"""
    def no_library(*a, **k):
        raise AssertionError("the library's call path was entered")
    monkeypatch.setattr(_lib, "on", no_library)
    monkeypatch.setattr(BakedField, "__init__", _init_without_library)

    def make(rows_dtype=None, as_half=("s0", "s1")):
        vol = HC.case("5x4x6", (8, 136), 3, 0.2, True, (0,))
        g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).as_subclass(_DeviceTensor)
        sets = {k: g(vol["bits"][k].view(np.float16)) if k in as_half else g(vol["sets"][k]) for k in vol["sets"]}
        fills = {k: g(f) for k, f in vol["fills"].items() if f is not None}
        return vol, BakedField.from_arrays(vol["origin"].tolist(), float(vol["step"]), g(vol["dist"]), valid=g(vol["valid"]), fills=fills, rows_dtype=rows_dtype, **sets)
    return make


def test_from_arrays_keeps_float16_only_when_asked(host_field):
    vol, f = host_field(rows_dtype=None)
    assert f.rows_dtype("s0") == f.rows_dtype("s1") == torch.float32          # as before: everything becomes float32
    assert torch.equal(f._sets["s1"].view(torch.int32), torch.from_numpy(vol["sets"]["s1"]).view(torch.int32))
    n = 5 * 4 * 6
    assert f.rows_bytes == 4 * n * (8 + 136)
    vol, h = host_field(rows_dtype=torch.float16)
    assert h.rows_dtype("s0") == h.rows_dtype("s1") == torch.float16 and h.rows_bytes == 2 * n * (8 + 136)
    assert torch.equal(h._sets["s0"].view(torch.int16), torch.from_numpy(vol["bits"]["s0"].view(np.int16)))
    vol, m = host_field(rows_dtype={"s1": torch.float16}, as_half=("s1",))
    assert m.rows_dtype("s0") == torch.float32 and m.rows_dtype("s1") == torch.float16 and m.rows_bytes == n * (4 * 8 + 2 * 136)
    with pytest.raises(KeyError):
        m.rows_dtype("nope")
    with pytest.raises(ValueError, match="rows_dtype"):
        host_field(rows_dtype={"nope": torch.float16})
    with pytest.raises(ValueError, match="rows_dtype"):
        host_field(rows_dtype=torch.bfloat16)


def test_the_storage_word_follows_the_tensor(host_field):
    _, m = host_field(rows_dtype={"s1": torch.float16}, as_half=("s1",))
    arr = m._set_array(["s0", "s1"])
    assert (arr[0].reserved, arr[1].reserved) == (_lib.DTYPE_F32, _lib.DTYPE_F16)
    assert (arr[0].C, arr[0].stride_voxel, arr[1].C, arr[1].stride_voxel) == (8, 8, 136, 136)             # elements, in either storage
    assert arr[1].data == m._sets["s1"].data_ptr()


def test_half_and_float_convert_and_share(host_field):
    vol, f = host_field(rows_dtype=None)
    h = f.half()
    assert h is not f and h.dist is f.dist and h.valid is f.valid and h.names() == f.names()
    assert h.rows_dtype("s0") == torch.float16 and f.rows_dtype("s0") == torch.float32 and 2 * h.rows_bytes == f.rows_bytes
    ok = torch.from_numpy(vol["valid"])
    assert torch.equal(h._sets["s1"].view(torch.int16)[ok], torch.from_numpy(vol["bits"]["s1"].view(np.int16))[ok])
    back = h.float()
    assert back.rows_dtype("s1") == torch.float32 and torch.equal(back._sets["s1"].view(torch.int32)[ok], f._sets["s1"].view(torch.int32)[ok])
    one = f.half(["s1"])
    assert one.rows_dtype("s0") == torch.float32 and one._sets["s0"] is f._sets["s0"] and one.rows_dtype("s1") == torch.float16
    assert one.float(["s1"]).rows_dtype("s1") == torch.float32
    assert f.half(check=True).rows_dtype("s0") == torch.float16                # every valid voxel is a finite half; the Inf / NaN of invalid ones do not count
    with pytest.raises(KeyError):
        f.half(["nope"])
    big = f._sets["s0"].clone()
    big[0, 0, 0, 1] = 70000.0                                                  # voxel (0, 0, 0) is valid
    f._sets["s0"] = big
    assert bool(torch.isinf(f.half()._sets["s0"][0, 0, 0, 1]))                 # beyond +-65504: Inf, silently
    with pytest.raises(ValueError, match="65504"):
        f.half(check=True)
    assert f.half(["s1"], check=True).rows_dtype("s1") == torch.float16


def test_methods_with_row_loops_of_their_own_raise_before_the_library(host_field):
    _, h = host_field(rows_dtype=torch.float16)
    _, other = host_field(rows_dtype=None)
    labels = torch.zeros(5, 4, 6, dtype=torch.int32).as_subclass(_DeviceTensor)
    calls = {
        "pool": lambda f: f.pool(labels, count=1),
        "links": lambda f: f.links("s0", tau=1.0),
        "parts": lambda f: f.parts("s0", tau=1.0),
        "flow": lambda f: f.flow(other, "s0"),
        "warp": lambda f: f.warp(None, None),
        "normal_equations": lambda f: f.normal_equations(None, None, None, name="s0", targets=None),
        "align": lambda f: f.align(None, name="s0", targets=None),
        "relocate": lambda f: f.relocate(None, "s0", None),
        "locate": lambda f: f.locate(None, "s0"),
    }
    for who, call in calls.items():
        with pytest.raises(TypeError, match=r"float\(") as e:
            call(h)
        assert "float16" in str(e.value) and "s0" in str(e.value), who
    with pytest.raises(TypeError, match=r"float\("):
        other.flow(h, "s0")                                                   # either field
    # a field whose OTHER set is half is not refused for its float32 set
    _, m = host_field(rows_dtype={"s1": torch.float16}, as_half=("s1",))
    assert m._need_float_rows("links", ["s0"]) is None
    with pytest.raises(TypeError, match=r"float\("):
        m.links("s1", tau=1.0)
