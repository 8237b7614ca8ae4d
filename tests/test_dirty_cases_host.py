"""The case table of tests/dirty_cases.py against the public header: every exported `int d3f_*(` function that takes a non-const pointer
-- a workspace, an output, in/out state -- is a key of CASES or of EXEMPT (with a one-line reason), so a new entry point cannot arrive
without a case; and the two inputs of every case have the same shapes, so that a replay run finds the storages of the run before."""
import os
import re

import pytest

import dirty_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")


def declarations():
    """name -> parameter list (text) of every `int d3f_*(...)` declaration of the header, comments removed"""
    with open(HEADER) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(d3f_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def writes_through_a_pointer(params):
    """a parameter whose pointee is not const, the stream handle aside (`void *stream` names a queue, not memory the call writes)"""
    for p in params.split(","):
        p = " ".join(p.split())
        if "*" not in p or p in ("void", ""):
            continue
        name = re.findall(r"(\w+)\s*$", p)[0]
        if name == "stream":
            continue
        if not p.startswith("const "):
            return True
    return False


def test_the_parser_sees_the_header():
    decl = declarations()
    assert len(decl) >= 70 and "d3f_eval" in decl and "d3f_part_motion" in decl and "d3f_abi_version" in decl
    assert not writes_through_a_pointer(decl["d3f_abi_version"])
    assert writes_through_a_pointer(decl["d3f_eval"]) and writes_through_a_pointer(decl["d3f_map_check"])
    assert writes_through_a_pointer("const float *a, float *const *out_fused, void *stream")
    assert not writes_through_a_pointer("const float *a, const void *workspace, int64_t n, void *stream")


def test_every_entry_point_has_a_case_or_a_reason():
    decl = declarations()
    writers = sorted(n for n, p in decl.items() if writes_through_a_pointer(p))
    missing = [n for n in writers if n not in DC.CASES and n not in DC.EXEMPT]
    assert not missing, "entry points without a case in tests/dirty_cases.py (or a reason in EXEMPT): %s" % missing
    both = [n for n in DC.CASES if n in DC.EXEMPT]
    assert not both, both
    unknown = [n for n in list(DC.CASES) + list(DC.EXEMPT) if n not in decl]
    assert not unknown, "not declared in include/d3fields_hip.h: %s" % unknown
    for n, reason in DC.EXEMPT.items():
        assert isinstance(reason, str) and 10 <= len(reason) and "\n" not in reason, n


def test_exemptions_are_of_the_allowed_kinds():
    """host memory only, or the two tracking launches whose scratch is documented must-be-zero"""
    for n, reason in DC.EXEMPT.items():
        assert reason.startswith("writes host memory only") or n in ("d3f_track_step", "d3f_track_run"), (n, reason)


def test_cases_are_well_formed():
    names = [c.name for c in DC.ALL]
    assert len(set(names)) == len(names)
    assert {id(c) for c in DC.CASES.values()} <= {id(c) for c in DC.ALL}
    for c in DC.ALL:
        assert callable(c.run) and callable(c.inputs)
        assert c.check is None or not c.large, (c.name, "a large case compares the fills with each other only")
        for k, (rel, sentence) in c.loose.items():
            assert 0 < rel <= 1e-4 and len(sentence) > 20, (c.name, k)


@pytest.mark.parametrize("case", [c for c in DC.ALL if not c.large], ids=lambda c: c.name)
def test_both_inputs_have_the_same_shapes(case):
    a, b = case.inputs()
    assert set(a) >= set(k for k in b if hasattr(b[k], "shape"))
    for k, v in a.items():
        if hasattr(v, "shape") and k in b:
            assert tuple(v.shape) == tuple(b[k].shape), (case.name, k)          # (the case converts both to one dtype on the way to the device)
    differ = [k for k, v in a.items() if hasattr(v, "shape") and k in b and v.shape and not _same(v, b[k])]
    assert differ, (case.name, "input B is input A: a replay would find its own leftovers")


def _same(x, y):
    import numpy as np
    import torch
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if np.asarray(x).dtype.kind == "f" else np.array_equal(np.asarray(x), np.asarray(y))
