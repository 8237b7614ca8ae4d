"""tests/dirty_buffers.py on CPU tensors: the fills are what they claim for every dtype the wrappers allocate, replay returns the
storages of the run before in order, a mismatch falls back to a fresh 0xFF tensor, nothing live is aliased, the guarded mode reports a byte
written in front of or behind a tensor and nothing else, and the patches are gone when the block ends."""
import pytest
import torch

from dirty_buffers import GUARD, DirtyBuffers

# every dtype a wrapper of d3fields_amd passes to torch.empty
DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.uint16, torch.int32, torch.int64, torch.float16, torch.float32,
          torch.float64]


def raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_fill_sets_every_byte(monkeypatch, dtype, byte):
    db = DirtyBuffers(monkeypatch)
    with db.fill(byte):
        a = torch.empty((3, 5), dtype=dtype)
        b = torch.empty_like(a)
        c = a.new_empty(7)
        d = a.new_empty((2, 2), dtype=torch.float32)
    for t, shape, dt in ((a, (3, 5), dtype), (b, (3, 5), dtype), (c, (7,), dtype), (d, (2, 2), torch.float32)):
        assert t.shape == shape and t.dtype == dt
        assert bool((raw(t) == byte).all()), "a byte of the tensor is not the fill byte"
    if byte == 0xFF:
        if dtype.is_floating_point:
            assert bool(torch.isnan(a).all()), "0xFF bytes are a NaN in every float format"
        elif dtype == torch.bool:
            assert bool(a.all()), "a 0xFF byte reads as True"
        elif dtype in (torch.uint8, torch.uint16):
            assert bool((a.to(torch.int64) == (1 << (8 * a.element_size())) - 1).all())
        else:
            assert bool((a == -1).all())
    else:
        assert not bool(a.to(torch.float64).abs().sum())
    assert db.fresh == 4 and db.replayed == 0


def test_fill_reaches_a_used_block(monkeypatch):
    """the point of the thing: the values a tensor had before do not survive"""
    db = DirtyBuffers(monkeypatch)
    with db.fill(0xFF):
        t = torch.empty(64, dtype=torch.int32)
        t.zero_()
    with db.fill(0xFF):
        u = torch.empty(64, dtype=torch.int32)
    assert bool((u == -1).all())


def test_zeros_and_full_are_left_alone(monkeypatch):
    db = DirtyBuffers(monkeypatch)
    with db.fill(0xFF):
        assert not bool(torch.zeros(9, dtype=torch.int64).any())
        assert bool((torch.full((4,), 3.0) == 3.0).all())
        assert not bool(torch.zeros_like(torch.ones(3)).any())
        assert db.fresh == 0


def test_replay_returns_the_same_storages_in_order(monkeypatch):
    db = DirtyBuffers(monkeypatch)
    shapes = [((16,), torch.float32), ((4, 3), torch.float64), ((16,), torch.float32), ((5,), torch.uint8)]
    with db.replay():
        first = [torch.empty(s, dtype=d) for s, d in shapes]
        assert all(bool((raw(t) == 0xFF).all()) for t in first), "the first run has nothing to replay: fresh 0xFF"
        for i, t in enumerate(first):
            t.fill_(i + 1)
    assert db.fresh == 4 and db.replayed == 0
    with db.replay():
        again = [torch.empty(s, dtype=d) for s, d in shapes]
    assert db.replayed == 4 and db.fresh == 0
    assert [t.data_ptr() for t in again] == [t.data_ptr() for t in first]
    for i, t in enumerate(again):
        assert bool((t == i + 1).all()), "the storage still holds what the run before left there"


def test_replay_after_a_fill_run_sees_its_leftovers(monkeypatch):
    db = DirtyBuffers(monkeypatch)
    with db.fill(0x00):
        a = torch.empty(8, dtype=torch.int32)
        a.fill_(41)
    with db.replay():
        b = torch.empty(8, dtype=torch.int32)
    assert b.data_ptr() == a.data_ptr() and bool((b == 41).all())


@pytest.mark.parametrize("what", ["shape", "dtype", "more"])
def test_a_mismatch_falls_back_to_a_fresh_tensor(monkeypatch, what):
    db = DirtyBuffers(monkeypatch)
    with db.replay():
        a = torch.empty(32, dtype=torch.float32)
        keep = torch.empty(8, dtype=torch.int64)
        a.fill_(2.0)
        keep.fill_(5)
    with db.replay():
        if what == "shape":
            b = torch.empty(33, dtype=torch.float32)
        elif what == "dtype":
            b = torch.empty(32, dtype=torch.int32)
        else:
            b = torch.empty(32, dtype=torch.float32)
        k2 = torch.empty(8, dtype=torch.int64)
        extra = torch.empty(8, dtype=torch.int64)         # a third allocation: the run before had two
    if what == "more":
        assert b.data_ptr() == a.data_ptr()
    else:
        assert b.data_ptr() != a.data_ptr() and bool((raw(b) == 0xFF).all())
    assert k2.data_ptr() == keep.data_ptr() and bool((k2 == 5).all()), "a mismatch at one index does not shift the others"
    assert extra.data_ptr() not in (a.data_ptr(), keep.data_ptr()) and bool((extra == -1).all())


def test_nothing_live_is_aliased(monkeypatch):
    """two allocations of one run never share bytes, in any mode, also when a run frees its tensors at once; and a replayed run shares
    nothing with the fresh tensors of the same run"""
    db = DirtyBuffers(monkeypatch)

    def spans(n):
        out = []
        for _ in range(n):
            t = torch.empty(1024, dtype=torch.uint8)
            out.append((t.data_ptr(), t.data_ptr() + t.numel()))
            del t                                            # the caller drops it: the allocator underneath could reuse the block
        return out

    def disjoint(s):
        s = sorted(s)
        return all(s[i][1] <= s[i + 1][0] for i in range(len(s) - 1))

    with db.fill(0x00):
        assert disjoint(spans(20))
    with db.fill(0xFF):
        assert disjoint(spans(20))
    with db.replay():
        first = spans(10)
        assert disjoint(first)
    with db.replay():
        second = spans(15)                                   # ten replayed, five fresh
        assert db.replayed == 10 and db.fresh == 5
        assert second[:10] == first and disjoint(second)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_guarded_tensors_are_zeros_at_256_bytes_and_whole_writes_leave_no_damage(monkeypatch, dtype):
    db = DirtyBuffers(monkeypatch)
    with db.guarded():
        a = torch.empty((3, 5), dtype=dtype)
        b = torch.empty_like(a)
        c = a.new_empty(0)
        d = a.new_empty(1000, dtype=torch.float32, requires_grad=True)
        for t in (a, b, c, d):
            assert t.data_ptr() % 256 == 0 and t.is_contiguous() and not bool(raw(t.detach()).any())
        assert d.requires_grad and (a.shape, a.dtype, c.numel()) == ((3, 5), dtype, 0)
        raw(a).fill_(0xFF)
        raw(b).fill_(0x17)
        d.detach().fill_(3.0)
    assert db.fresh == 4 and db.damage() == []


def test_guarded_reports_a_write_in_front_and_behind(monkeypatch):
    db = DirtyBuffers(monkeypatch)
    with db.guarded():
        a = torch.empty(100, dtype=torch.int32)
        b = torch.empty(7, dtype=torch.uint8)
        c = torch.empty(64, dtype=torch.float64)
        whole_a, start_a, _ = db._guards[0]
        whole_c, start_c, _ = db._guards[2]
        whole_a[start_a + 400] = 0                      # the first byte behind a's 400
        whole_a[start_a + 400 + GUARD - 1] = 1          # and the last of that guard
        whole_c[start_c - 1] = 2                        # the last byte in front of c
        b.fill_(9)
    assert db.damage() == [(0, 400, "back", 2, 400), (2, 512, "front", 1, -1)]
    with db.guarded():
        torch.empty(3)
    assert db.damage() == [], "a new guarded run starts a new list"


def test_runs_do_not_nest(monkeypatch):
    db = DirtyBuffers(monkeypatch)
    with db.fill(0):
        with pytest.raises(RuntimeError):
            with db.fill(0xFF):
                pass


def test_the_patches_are_gone_after_the_block(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    db = DirtyBuffers(monkeypatch)
    with db.fill(0xFF):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(ZeroDivisionError):
        with db.replay():
            raise ZeroDivisionError
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert "new_empty" not in torch.Tensor.__dict__ or torch.Tensor.__dict__["new_empty"] is before[2]
