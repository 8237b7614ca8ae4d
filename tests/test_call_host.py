"""CPU: the one call path from Python into the library (d3fields_amd/_lib.py, `on`) against a recording fake library: what each kind of
argument arrives as, where the stream goes, what a status and a foreign tensor do, and the one workspace rule.  No GPU, no real library."""
import contextlib
import ctypes

import pytest
import torch

from d3fields_amd import _lib

STREAM = ctypes.c_void_p(0x5EED)


class _FakeLib:
    """records (name, arguments) of every call; an entry point answers results[name] (default 0)"""

    def __init__(self, **results):
        self.calls, self.results = [], results

    def __getattr__(self, name):
        if not name.startswith("d3f_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.results.get(name, 0)
        return fn


class _DeviceTensor(torch.Tensor):
    """a host tensor that says it lives on cuda:0: what the device check reads, without a GPU"""
    device = property(lambda self: torch.device("cuda", 0))
    is_cuda = property(lambda self: True)


def _on_gpu(t):
    return t.as_subclass(_DeviceTensor)


@pytest.fixture
def host(monkeypatch):
    """a null device context and a counted, fixed stream -> the list of devices whose stream was read"""
    reads = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "current_stream_handle", lambda dev: reads.append(dev) or STREAM)
    return reads


def _addr(a):
    return ctypes.cast(a, ctypes.c_void_p).value


def test_each_kind_of_argument_arrives_converted_once(host):
    fake = _FakeLib()
    t = _on_gpu(torch.zeros(8))
    vol = _lib.Volume(2, 3, 4)
    arr = (ctypes.c_int32 * 3)(1, 2, 3)
    words = (ctypes.c_void_p * 2)(16, 32)
    with _lib.on("cuda:0", fake) as q:
        q.d3f_volume_cell_valid(vol, t)
        q.d3f_pcd_to_index(t, 8, arr, 0.5, words, None, 7)
    (_, (got_vol, got_t, _)), (_, (flat, n, got_arr, step, got_words, none, seven, _)) = fake.calls
    assert isinstance(got_t, ctypes.c_void_p) and got_t.value == t.data_ptr() != 0
    assert flat.value == t.data_ptr()
    assert none is None                                     # NULL: what ctypes makes of None for a pointer parameter
    vol.nx = 41                                             # written after the call was set up: a reference to the same object shows it
    assert ctypes.cast(got_vol, ctypes.POINTER(_lib.Volume)).contents.nx == 41 and _addr(got_vol) == ctypes.addressof(vol)
    assert got_arr is arr and got_words is words            # ctypes arrays: untouched
    assert (n, step, seven) == (8, 0.5, 7) and type(n) is int and type(step) is float


def test_stream_goes_last_where_the_header_has_one_and_is_read_once(host):
    fake = _FakeLib(d3f_volume_edt_workspace_bytes=4096)
    t = _on_gpu(torch.zeros(4))
    with _lib.on("cuda:0", fake) as q:
        assert q.stream is STREAM
        assert q.d3f_volume_edt_workspace_bytes(4, 4, 4) == 4096          # a size function: its value comes back, no stream goes in
        q.d3f_erode(t, 2, 2, 1, 1, t)
        q.d3f_softmax_apply(t, 2, 2, 1.0, t)
    size, erode, apply = fake.calls
    assert size == ("d3f_volume_edt_workspace_bytes", (4, 4, 4))
    assert len(erode[1]) == 7 and erode[1][-1] is STREAM
    assert len(apply[1]) == 6 and apply[1][-1] is STREAM
    assert host == [torch.device("cuda", 0)]                # two calls and a size in one block: one read of the current stream


def test_every_entry_point_is_streamed_or_not_by_the_table(host):
    assert _lib.STREAMED <= set(_lib.SIGNATURES) and _lib.STATUS <= set(_lib.SIGNATURES)
    fake = _FakeLib()
    with _lib.on("cuda:0", fake) as q:
        for name, (_, args) in _lib.SIGNATURES.items():
            streamed = name in _lib.STREAMED
            getattr(q, name)(*[None] * (len(args) - streamed))
            got = fake.calls[-1][1]
            assert len(got) == len(args) and (bool(got) and got[-1] is STREAM) == streamed, name
        with pytest.raises(AttributeError):
            q.d3f_no_such_entry_point


def test_a_status_raises_and_a_value_returns(host):
    fake = _FakeLib(d3f_erode=_lib.ERR_BAD_LAYOUT, d3f_track_run_max_keypoints=512, d3f_eval_plan_query=_lib.ERR_INVALID_ARG)
    t = _on_gpu(torch.zeros(4))
    with _lib.on("cuda:0", fake) as q:
        with pytest.raises(_lib.D3FError) as e:
            q.d3f_erode(t, 2, 2, 1, 1, t)
        assert e.value.code == -4 == _lib.ERR_BAD_LAYOUT
        assert q.d3f_track_run_max_keypoints() == 512      # an int that is no status
        with pytest.raises(_lib.D3FError) as e:
            q.d3f_eval_plan_query(None, 0, None, 0, 0, 0, 0, None)          # a status without a stream
        assert e.value.code == _lib.ERR_INVALID_ARG and len(fake.calls[-1][1]) == 8
        assert q.d3f_instance2onehot(t, 4, 2, t) is None    # OK: nothing to return


def test_a_tensor_that_is_not_on_the_device_is_refused_before_any_call(host):
    fake = _FakeLib()
    good = _on_gpu(torch.zeros(4))
    with _lib.on("cuda:1", fake) as q:
        with pytest.raises(RuntimeError, match=r"d3f_erode: argument 5 .*cuda:0.*cuda:1"):
            q.d3f_erode(None, 2, 2, 1, 1, good)             # on another GPU
    with _lib.on("cuda:0", fake) as q:
        with pytest.raises(RuntimeError, match=r"d3f_erode: argument 0 .*cpu"):
            q.d3f_erode(torch.zeros(4), 2, 2, 1, 1, good)   # host memory does not go in as a tensor
        with pytest.raises(RuntimeError, match=r"d3f_softmax_workspace_bytes: argument 1"):
            q.workspace("d3f_softmax_workspace_bytes", 4, torch.zeros(1))
    assert fake.calls == []


@pytest.mark.parametrize("said, allocated", [(0, 16), (1, 16), (16, 16), (1000, 1000)])
def test_workspace_is_never_null_and_reports_what_the_size_function_said(host, said, allocated):
    fake = _FakeLib(d3f_mesh_workspace_bytes=said)
    with _lib.on("cpu", fake) as q:                         # (the allocation is real: it has to happen where this machine has memory)
        ws, nbytes = q.workspace("d3f_mesh_workspace_bytes", 3, 4, 5)
    assert fake.calls == [("d3f_mesh_workspace_bytes", (3, 4, 5))]
    assert nbytes == said and type(nbytes) is int
    assert ws.dtype == torch.uint8 and ws.numel() == allocated and ws.device.type == "cpu" and ws.data_ptr() != 0


def test_the_library_defaults_to_the_loaded_one(host):
    assert _lib.on("cuda:0").lib is _lib.load()
