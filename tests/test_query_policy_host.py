"""Host logic of the forward query of Fusion, with every device call stubbed out: which entry point a query takes, which point-order flags
and workspace it carries, how many probes and map checks it launches, and what the descriptors of its maps hold.  Fusion._launch and
Fusion.eval_grid run on CPU tensors against a recording fake of the library; big maps are one view expanded to V, so the 64 MiB and 256 MiB
sizes of the planner's thresholds (counted as numel * element_size, as the shim counts them) cost no memory."""
import contextlib
import ctypes

import pytest
import torch

from d3fields_amd import Fusion, _lib, fusion as fmod

V, H, W = 4, 8, 8
UNORDERED, LOCAL, REUSE = _lib.FLAG_UNORDERED_POINTS, _lib.FLAG_LOCAL_POINTS, _lib.FLAG_REUSE_POINT_ORDER
WS_BYTES, DIST_WS_BYTES = 12352, 4224                       # what the fake workspace-size calls answer
MIB = 1 << 20
TEXEL = 1536                                                # one texel of C = 384 fp32


class _Stream:
    cuda_stream = 0

    def wait_event(self, ev):
        pass


class _Event:
    def record(self, stream=None):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


class _FakeLib:
    """Every call appends (entry point, arguments); the answers are 0 (= D3F_OK, or no bytes) unless `answers` says otherwise."""

    def __init__(self, **answers):
        self.calls = []
        self.answers = answers

    def __getattr__(self, name):
        if not name.startswith("d3f_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "d3f_eval_plan_query":
                args[-1]._obj.reorder = self.answers.get("reorder", 0)
                return 0
            return self.answers.get(name, 0)
        return call

    def count(self, *names):
        return sum(1 for c in self.calls if c[0] in names)

    def last(self, name):
        return [c for c in self.calls if c[0] == name][-1][1]


class _On:
    """_lib.on() without its refusal of host tensors: the calls reach the fake library as they are"""

    def __init__(self, device, lib=None):
        self.lib = lib

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getattr__(self, name):
        return getattr(self.lib, name)


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: _Stream())
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(fmod._lib, "current_stream_handle", lambda dev: ctypes.c_void_p(0))
    monkeypatch.setattr(fmod._lib, "on", _On)

    def make(maps, probe=(None, False), answers=None, **knobs):
        """A Fusion on the CPU over `maps` (name -> tensor) whose library records, and whose probe answers `probe` = (dims, unordered)"""
        f = Fusion(num_cam=V, device="cpu")
        f._lib = _FakeLib(**dict({"d3f_eval_workspace_bytes": WS_BYTES}, **(answers or {})))
        f.H, f.W = H, W
        f.curr_obs_torch = dict({"depth": torch.ones(V, H, W), "K": torch.eye(3).repeat(V, 1, 1), "pose": torch.eye(4)[:3].repeat(V, 1, 1)}, **maps)
        f.cache_point_order = f.async_probes = False
        for k, v in knobs.items():
            assert hasattr(f, k)
            setattr(f, k, v)

        def probe_now(pts_c, stream):
            f._lib.calls.append(("d3f_points_probe", (pts_c, stream)))
            return probe
        f._probe_now = probe_now
        return f
    return make


def _big(h, w, C):
    """(V,h,w,C) fp32 that occupies one view's worth of (untouched) memory"""
    return torch.empty(1, h, w, C).expand(V, h, w, C)


def _maps(nbytes):
    """maps of `nbytes` in total: 64 or 256 MiB in one 16-channel map, the odd 1536 bytes in a second map of 2 x 3 texels"""
    whole, rest = nbytes // (64 * MIB) * (64 * MIB), nbytes % (64 * MIB)
    side = {64 * MIB: 512, 256 * MIB: 1024}[whole]
    out = {"wide": _big(side, side, 16)}
    if rest:
        assert rest == TEXEL
        out["thin"] = torch.empty(V, 2, 3, 16)
    assert sum(m.numel() * m.element_size() for m in out.values()) == nbytes
    return out


def _fields(d):
    return tuple(getattr(d, name) for name, _ in _lib.ChannelMap._fields_)


def _query(f, n, names):
    """One _launch of n points; -> (entry point, its arguments, what the call added to the log)"""
    before = len(f._lib.calls)
    pts = torch.zeros(n, 3)
    out, rec = f._launch(pts, names, False, "eval")
    new = f._lib.calls[before:]
    launches = [c for c in new if c[0] in ("d3f_eval", "d3f_eval_lattice", "d3f_eval_dist", "d3f_eval_grid")]
    assert len(launches) == 1
    assert out["dist"].shape == (n,) and out["valid_mask"].dtype == torch.bool and all(out[k].shape == (n, f.curr_obs_torch[k].shape[3]) for k in names)
    return launches[0][0], launches[0][1], [c[0] for c in new], (out, rec)


def _eval_args(args):
    """flags, workspace address (None = NULL), workspace_bytes, n_maps of a d3f_eval call"""
    return int(args[6]), args[11].value, int(args[12]), int(args[4])


# ---- (a) below the small-batch threshold -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [64 * MIB, 64 * MIB + TEXEL, 256 * MIB + TEXEL])
@pytest.mark.parametrize("detect_lattice", [False, True])
def test_small_batch_takes_no_probe_and_no_workspace(host, nbytes, detect_lattice):
    maps = _maps(nbytes)
    f = host(maps, probe=(None, True), detect_lattice=detect_lattice)
    entry, args, log, _ = _query(f, 65535, list(maps))
    flags, ws, ws_bytes, n_maps = _eval_args(args)
    assert entry == "d3f_eval" and n_maps == len(maps)
    assert not flags & (UNORDERED | LOCAL) and ws is None and ws_bytes == 0
    assert log.count("d3f_points_probe") == 0 and log.count("d3f_map_check_many") == 1 and log.count("d3f_map_check") == 0


# ---- (b) at the small-batch threshold, not a lattice --------------------------------------------------------------------------------
# (n, bytes of the maps, detect_point_order) -> is the point order probed?  which bit follows an unordered / a local verdict?
ORDER_ROWS = [
    (65536, 64 * MIB, True, True, UNORDERED, 0),
    (65536, 64 * MIB + TEXEL, True, True, 0, LOCAL),
    (65536, 256 * MIB, True, True, 0, LOCAL),
    (65536, 256 * MIB + TEXEL, True, False, 0, 0),
    (262144, 64 * MIB + TEXEL, True, False, 0, 0),
    (262143, 64 * MIB + TEXEL, True, True, 0, LOCAL),
    (65536, 64 * MIB, False, False, 0, 0),
    (65536, 64 * MIB + TEXEL, False, False, 0, 0),
    (65536, 256 * MIB + TEXEL, False, False, 0, 0),
]


@pytest.mark.parametrize("n,nbytes,detect_order,probed,if_unordered,if_local", ORDER_ROWS)
@pytest.mark.parametrize("unordered", [False, True])
@pytest.mark.parametrize("detect_lattice", [False, True])
def test_point_order_policy_at_the_thresholds(host, n, nbytes, detect_order, probed, if_unordered, if_local, unordered, detect_lattice):
    """detect_lattice=False shows the locality probe alone.  With detect_lattice=True every query of at least the small-batch size is probed
    for the lattice, and that one launch answers the locality question too: one probe in every row, the same bits."""
    maps = _maps(nbytes)
    f = host(maps, probe=(None, unordered), detect_point_order=detect_order, detect_lattice=detect_lattice)
    entry, args, log, _ = _query(f, n, list(maps))
    flags, ws, ws_bytes, n_maps = _eval_args(args)
    assert entry == "d3f_eval" and n_maps == len(maps)
    assert flags & (UNORDERED | LOCAL) == (if_unordered if unordered else if_local)
    assert ws is not None and ws_bytes == WS_BYTES
    assert log.count("d3f_points_probe") == (1 if (probed or detect_lattice) else 0)
    assert log.count("d3f_map_check_many") == 1 and log.count("d3f_map_check") == 0
    assert f._lib.last("d3f_eval_workspace_bytes") == (n,)


# ---- (c) a lattice -----------------------------------------------------------------------------------------------------------------
def test_detected_lattice_takes_the_lattice_entry_point(host):
    maps = _maps(64 * MIB + TEXEL)
    dims = (64, 32, 32)
    f = host(maps, probe=(dims, False), detect_lattice=True)
    entry, args, log, _ = _query(f, 65536, list(maps))
    assert entry == "d3f_eval_lattice" and tuple(args[2:5]) == dims and int(args[6]) == len(maps)
    assert not int(args[8]) & (UNORDERED | LOCAL)
    assert len(args) == 14                                   # (no workspace among the arguments of d3f_eval_lattice)
    assert "d3f_eval_workspace_bytes" not in log and log.count("d3f_points_probe") == 1
    assert log.count("d3f_map_check_many") == 1 and log.count("d3f_map_check") == 0
    # detect_lattice off: the same tensor is a cloud like any other of (b)
    f = host(maps, probe=(dims, False), detect_lattice=False)
    entry, args, log, _ = _query(f, 65536, list(maps))
    flags, ws, ws_bytes, n_maps = _eval_args(args)
    assert entry == "d3f_eval" and flags & (UNORDERED | LOCAL) == LOCAL and ws is not None and ws_bytes == WS_BYTES
    assert log.count("d3f_points_probe") == 1


# ---- (d), (e) no names -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 65536])
@pytest.mark.parametrize("dist_ws", [0, DIST_WS_BYTES])
def test_distance_only_query(host, n, dist_ws):
    f = host(_maps(64 * MIB), probe=(None, True), answers={"d3f_eval_dist_workspace_bytes": dist_ws})
    entry, args, log, _ = _query(f, n, [])
    flags, ws, ws_bytes, n_maps = _eval_args(args)
    assert entry == "d3f_eval" and n_maps == 0 and not flags & (UNORDERED | LOCAL)
    assert ws_bytes == dist_ws and (ws is None) == (dist_ws == 0)
    assert log.count("d3f_points_probe") == 0 and log.count("d3f_map_check_many") == 0 and log.count("d3f_map_check") == 0
    assert "d3f_eval_workspace_bytes" not in log
    f.reorder_points = False                                 # no scratch at all: the size is not even asked for
    entry, args, log, _ = _query(f, n, [])
    assert _eval_args(args)[1:3] == (None, 0) and "d3f_eval_dist_workspace_bytes" not in log


# ---- (f) the cached point order ----------------------------------------------------------------------------------------------------
def test_cached_point_order_is_reused(host):
    maps = _maps(64 * MIB + TEXEL)
    f = host(maps, probe=(None, True), answers={"reorder": 1}, cache_point_order=True)
    pts = torch.zeros(65536, 3)
    seen = []
    for _ in range(2):
        f._launch(pts, list(maps), False, "eval")
        seen.append(_eval_args(f._lib.last("d3f_eval")))
    (flags0, ws0, bytes0, _), (flags1, ws1, bytes1, _) = seen
    assert not flags0 & REUSE and flags1 & REUSE
    assert ws0 is not None and ws1 == ws0 and bytes0 == bytes1 == WS_BYTES
    assert f._lib.count("d3f_points_probe") == 1 and f._lib.count("d3f_map_check_many") == 1 and f._lib.count("d3f_eval_plan_query") == 2
    # another tensor of the same size: a new probe, a new order
    f._launch(torch.zeros(65536, 3), list(maps), False, "eval")
    assert not _eval_args(f._lib.last("d3f_eval"))[0] & REUSE and f._lib.count("d3f_points_probe") == 2


# ---- (g) binding -------------------------------------------------------------------------------------------------------------------
def test_channel_strided_map_goes_in_as_a_checked_copy(host):
    view = torch.arange(V * 4 * 4 * 10, dtype=torch.float32).reshape(V, 4, 4, 10)[..., ::2]
    assert view.stride(3) == 2
    f = host({"odd": view})
    _, args, log, held = _query(f, 100, ["odd"])
    d = args[3][0]
    assert d.data != view.data_ptr() and (d.fh, d.fw, d.C, d.dtype) == (4, 4, 5, _lib.DTYPE_F32) and (d.stride_v, d.stride_y, d.stride_x) == (80, 20, 5)
    got = torch.tensor(list((ctypes.c_float * view.numel()).from_address(d.data))).reshape(view.shape)     # (alive: `held` keeps the launch's record)
    assert torch.equal(got, view)
    descs, views, n, words = f._lib.last("d3f_map_check_many")[:4]
    assert n == 2 and _fields(descs[1])[:8] == _fields(d)[:8] and words[1] == d.nonfinite and views[1] == V
    assert "odd" not in f._finite_cache and "depth" in f._finite_cache
    _, args, log, _ = _query(f, 100, ["odd"])               # a new copy on every call: checked again, depth is not
    assert log.count("d3f_map_check_many") == 1 and f._lib.last("d3f_map_check_many")[2] == 1 and log.count("d3f_map_check") == 0


def test_half_map_gets_the_half_dtype(host):
    f = host({"half": torch.ones(V, 4, 4, 8, dtype=torch.float16), "full": torch.ones(V, 4, 4, 8)})
    _, args, _, _ = _query(f, 100, ["half", "full"])
    assert (args[3][0].dtype, args[3][1].dtype) == (_lib.DTYPE_F16, _lib.DTYPE_F32)
    assert args[3][0].data == f.curr_obs_torch["half"].data_ptr() and args[3][0].stride_x == 8


def test_too_many_names_and_malformed_maps_raise(host):
    f = host({"m%d" % i: torch.ones(V, 2, 2, 4) for i in range(_lib.MAX_MAPS + 1)})
    with pytest.raises(ValueError):
        f._launch(torch.zeros(10, 3), ["m%d" % i for i in range(_lib.MAX_MAPS + 1)], False, "eval")
    f._launch(torch.zeros(10, 3), ["m%d" % i for i in range(_lib.MAX_MAPS)], False, "eval")
    f.curr_obs_torch["flat"] = torch.ones(V, 4, 8)
    bounds = {"x_lower": 0.0, "x_upper": 0.04, "y_lower": 0.0, "y_upper": 0.03, "z_lower": 0.0, "z_upper": 0.02}
    launches = f._lib.count("d3f_eval", "d3f_eval_grid")
    with pytest.raises(ValueError):
        f._launch(torch.zeros(10, 3), ["flat"], False, "eval")
    with pytest.raises(ValueError):
        f.eval_grid(bounds, 0.01, return_names=["flat"])
    with pytest.raises(KeyError):
        f._launch(torch.zeros(10, 3), ["absent"], False, "eval")
    assert f._lib.count("d3f_eval", "d3f_eval_grid") == launches


# ---- (h) eval_grid -----------------------------------------------------------------------------------------------------------------
def test_eval_grid_binds_like_launch_and_checks_in_one_call(host):
    maps = {"a": torch.ones(V, 4, 6, 8), "b": torch.ones(V, 3, 5, 12, dtype=torch.float16)[:, :, :, :10]}
    f = host(maps)
    bounds = {"x_lower": 0.0, "x_upper": 0.04, "y_lower": 0.0, "y_upper": 0.03, "z_lower": 0.0, "z_upper": 0.02}
    out = f.eval_grid(bounds, 0.01, return_names=["a", "b"])
    n = 4 * 3 * 2
    assert tuple(out["grid_shape"]) == (4, 3, 2) and out["a"].shape == (n, 8) and out["b"].shape == (n, 10) and out["dist"].shape == (n,)
    assert f._lib.count("d3f_map_check_many") == 1 and f._lib.count("d3f_map_check") == 0
    assert f._lib.last("d3f_map_check_many")[2] == 3
    args = f._lib.last("d3f_eval_grid")
    grid_descs = [_fields(args[2][s]) for s in range(2)]
    assert int(args[3]) == 2 and args[0].depth_nonfinite
    _, largs, log, _ = _query(f, 50, ["a", "b"])
    assert [_fields(largs[3][s]) for s in range(2)] == grid_descs       # the cached verdicts: the same words too
    assert largs[0]._obj.depth_nonfinite == args[0].depth_nonfinite
    assert not any(name.startswith("d3f_map_check") for name in log)
    assert grid_descs[1][3:8] == (10, _lib.DTYPE_F16, 3 * 5 * 12, 5 * 12, 12) and all(d[8] for d in grid_descs)


# ---- (i) the shared constructor and the layout rule -------------------------------------------------------------------------------
def test_channel_map_constructor_and_layout_rule():
    t = torch.ones(3, 5, 7, 12, dtype=torch.float16)[:, 1:4, ::2, :9]
    hand = _lib.ChannelMap(t.data_ptr(), t.shape[1], t.shape[2], t.shape[3], _lib.DTYPE_F16, t.stride(0), t.stride(1), t.stride(2), 4096)
    assert _fields(_lib.channel_map(t, 4096)) == _fields(hand) and _lib.channel_map(t).nonfinite is None
    assert _lib.channel_map(t.float().contiguous()).dtype == _lib.DTYPE_F32
    d = torch.ones(3, 6, 8)[:, :, ::2]
    hand = _lib.ChannelMap(d.data_ptr(), d.shape[1], d.shape[2], 1, _lib.DTYPE_F32, d.stride(0), d.stride(1), max(d.stride(2), 1), 64)
    assert _fields(_lib.channel_map(d, 64)) == _fields(hand) and hand.stride_x == 2
    one = torch.ones(3, 6, 1).expand(3, 6, 8)                # stride(2) == 0: the descriptor says 1, the layout rule says no
    assert _lib.channel_map(one).stride_x == 1 and not _lib.readable_layout(one)
    assert _lib.readable_layout(t) and _lib.readable_layout(d) and _lib.readable_layout(torch.ones(1, 2, 2, 4).expand(3, 2, 2, 4))
    assert not _lib.readable_layout(torch.ones(2, 4, 4, 8, dtype=torch.float64))
    assert not _lib.readable_layout(torch.ones(2, 4, 4, 8)[..., ::2])                    # stride(3) == 2
    assert not _lib.readable_layout(torch.ones(2, 4, 8, 4).transpose(2, 3))             # stride(3) != 1 and stride(2) < C
    assert not _lib.readable_layout(torch.ones(2, 4, 1, 8).expand(2, 4, 4, 8))          # stride(2) == 0 < C
    assert not _lib.readable_layout(torch.ones(2, 4, 4, 8).as_strided((2, 4, 4, 8), (128, 32, 4, 1)))     # stride(2) == 4 < C, texels overlap
    assert not _lib.readable_layout(torch.ones(2, 6, 8, dtype=torch.float16))            # depth is float32 only

    class _Flipped:                                          # torch has no negative strides; a producer's wrapper may
        dtype = torch.float32
        shape = (2, 4, 4, 8)

        def dim(self):
            return 4

        def stride(self, d=None):
            s = (128, -32, 8, 1)
            return s if d is None else s[d]
    assert not _lib.readable_layout(_Flipped())


def test_planner_thresholds_steer_the_shim():
    """the four numbers the policy compares against are the library's, not literals of fusion.py"""
    import inspect
    src = inspect.getsource(fmod)
    assert not any(lit in src for lit in ("65536", "262144", "64 << 20", "256 << 20"))
    assert (_lib.PLAN_SMALL_BATCH, _lib.PLAN_WINDOW_CLOUD_MIN, _lib.PLAN_CACHE_RESIDENT_BYTES, _lib.PLAN_INFINITY_CACHE_BYTES) == (65536, 262144, 64 * MIB, 256 * MIB)
