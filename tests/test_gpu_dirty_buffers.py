"""Which memory may an entry point assume is initialised?  None, says the header, but for the few buffers it names.
Every case of tests/dirty_cases.py runs its input A three times -- on workspaces and outputs filled with 0x00, filled with 0xFF (every
int -1, every float a NaN), and replayed: on the very storages a run of ANOTHER input B of the same shapes just used -- and the defined
part of every output must come out with the same bytes each time, and pass the comparison the feature's own test applies to its case.

What a failure means: a region of a workspace or an output that a kernel reads before anything in the call has written it -- a counter
that is added into, a ticket or status word, a table whose empty slot is ~0, a count that only one branch writes.  The fix is a clear
inside the call, on the caller's stream (it is a product bug, not a test to relax).

Bitwise equality is the rule; `Case.loose` names the only departures, each with the sentence of the code that says its summation order
varies.  `Case.undefined` quotes the header where a part of an output is left out because the header leaves it undefined.
"""
import time

import pytest
import torch

import dirty_cases as DC
from dirty_buffers import DirtyBuffers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device(DC.DEV)


def raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def compare(case, what, a, b):
    assert set(a) == set(b), (case.name, what, sorted(set(a) ^ set(b)))
    for k in sorted(a):
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (case.name, what, k, tuple(x.shape), tuple(y.shape), x.dtype, y.dtype)
        if k in case.loose:
            rel = case.loose[k][0]
            ok = bool(((x.double() - y.double()).abs() <= rel * x.double().abs().clamp_min(1.0)).all())
            assert ok, (case.name, what, k, "outside %g relative" % rel, x.reshape(-1)[:4].tolist(), y.reshape(-1)[:4].tolist())
            continue
        if x.numel() and not torch.equal(raw(x), raw(y)):
            bad = torch.nonzero(raw(x) != raw(y)).reshape(-1)
            at = int(bad[0]) // max(x.element_size(), 1)
            raise AssertionError((case.name, what, k, "%d of %d bytes differ, the first in element %d" % (bad.numel(), raw(x).numel(), at),
                                  x.reshape(-1)[at:at + 4].tolist(), y.reshape(-1)[at:at + 4].tolist()))


def run_case(case, db, mode, inp, keep=True):
    with mode:
        try:
            out = case.run(inp)
            torch.cuda.synchronize()
        except RuntimeError as e:                    # a device fault poisons the process: nothing more is started on the device
            if any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access", "status -5")):
                pytest.exit("device fault in case %r: %s" % (case.name, e), returncode=3)
            raise
    handed = db.fresh + db.replayed
    got = {k: v.detach().clone() for k, v in out.items()} if keep else None        # (cloned before the next run takes the storages)
    return got, handed


@pytest.mark.parametrize("case", DC.ALL, ids=lambda c: c.name)
def test_same_bytes_whatever_the_buffers_held(dev, monkeypatch, case):
    a, b = case.inputs()
    db = DirtyBuffers(monkeypatch)
    t0 = time.perf_counter()

    def run(mode, inp, keep=True):
        return run_case(case, db, mode, inp, keep)

    zeros, n0 = run(db.fill(0x00), a)
    ones, n1 = run(db.fill(0xFF), a)
    _, nb = run(db.replay(), b, keep=False)
    again, n2 = run(db.replay(), a)
    assert n0 > 0, (case.name, "the case allocates nothing through torch.empty: it tests nothing")
    assert n0 == n1 == n2, (case.name, "the runs of input A ask for different numbers of buffers", n0, n1, n2)
    assert db.replayed >= case.min_replayed * n2, (case.name, "the replay of A found only %d of its %d buffers in the run of B" % (db.replayed, n2))
    print("%s: %d buffers per run (%d of them replayed after input B), %.2f s" % (case.name, n0, db.replayed, time.perf_counter() - t0))
    compare(case, "0x00 against 0xFF", zeros, ones)
    compare(case, "0x00 against the replay", zeros, again)
    if case.check is not None:
        for what, got in (("0x00", zeros), ("0xFF", ones), ("replay", again)):
            try:
                case.check(a, got)
            except AssertionError as e:
                raise AssertionError((case.name, "the feature's own comparison fails on the %s run" % what) + e.args)
    if case.large:
        del zeros, ones, again
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", DC.ALL, ids=lambda c: c.name)
def test_nothing_is_written_outside_the_buffers(dev, monkeypatch, case):
    """every buffer a view with 4 KiB of a fixed byte in front and behind (DirtyBuffers.guarded): the guards come back whole -- no entry point
    writes outside the bytes its *_workspace_bytes function or its output's shape asked for -- and the outputs are those of the 0x00 run"""
    a, _ = case.inputs()
    db = DirtyBuffers(monkeypatch)
    t0 = time.perf_counter()
    zeros, n0 = run_case(case, db, db.fill(0x00), a)
    guarded, n1 = run_case(case, db, db.guarded(), a)
    damage = db.damage()
    print("%s: %d buffers behind guards, %.2f s" % (case.name, n1, time.perf_counter() - t0))
    assert n0 == n1 > 0, (case.name, "the runs ask for different numbers of buffers", n0, n1)
    assert not damage, (case.name, "(allocation, its bytes, side, changed guard bytes, offset of the first from the buffer's start)", damage)
    compare(case, "0x00 against the guarded run", zeros, guarded)
    if case.large:
        del zeros, guarded, db
        torch.cuda.empty_cache()
