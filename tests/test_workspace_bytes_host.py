"""CPU only: how many bytes every entry point asks for.  Every d3f_*_workspace_bytes function and d3f_eval_gate_offset is called with the rows of
tests/workspace_args.py -- the arguments that return 0, the smallest shape, both sides of every rounding boundary of the layout behind it, a
workload -- and compared with the record in tests/workspace_bytes.json: the sizes of the library before each workspace got ONE layout function
that both its size and its launcher read (csrc/d3f_workspace.h).  The record is compared and never rewritten from the code under test: a value
changes only by hand, with the region that grew or shrank and the reason beside it in the commit (DESIGN.md section 27 names the regions).
tests/layout_check.cpp walks the same rows in a stand-alone host program and checks the order of the regions inside each layout.

The size functions are host code; nothing is launched, so the module runs where no device exists."""
import json

import pytest

import workspace_args as WA
from d3fields_amd import _lib


@pytest.fixture(scope="module")
def record():
    with open(WA.RECORD) as fh:
        return json.load(fh)


def test_table_covers_every_size_function(record):
    sized = sorted(fn for fn in _lib.SIGNATURES if fn.endswith("_workspace_bytes") or fn == "d3f_eval_gate_offset")
    assert sorted(WA.TABLE) == sized == sorted(record)
    for fn in sized:
        rows, want = WA.TABLE[fn], record[fn]
        assert len(rows) == len(want) and len(set(rows)) == len(rows), (fn, "the table and the record list different rows")
        assert 0 in want and any(v > 0 for v in want), (fn, "no rejected row, or no accepted one")
    assert 200 <= sum(len(v) for v in record.values()) <= 500


@pytest.mark.parametrize("fn", sorted(WA.TABLE))
def test_sizes_equal_the_record(record, fn):
    lib = WA.load()
    got = [WA.call(lib, fn, row) for row in WA.TABLE[fn]]
    wrong = ["%s%r: recorded %d, now %d" % (fn, row, w, g) for row, g, w in zip(WA.TABLE[fn], got, record[fn]) if g != w]
    assert not wrong, "%d of %d rows differ from the record:\n%s" % (len(wrong), len(got), "\n".join(wrong))
