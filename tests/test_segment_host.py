"""CPU: the segment entry points (d3f_volume_segments, d3f_path_shorten) are declared by the header, bound and exported with D3F_ABI_VERSION
still 16; they validate their arguments on the host with the documented status codes and launch nothing; the event walk of the restatement
(tests/segment_cases.py) touches exactly the voxels of the cube test under both rules, in non-decreasing t; clear is symmetric, the open rule
never blocks what the strict rule passes, and every move of a travel path is clear under the open rule; the case sets hold what the device
tests rely on (clear shares, segments on which the rules differ, an anchor whose jump passes a blocked nearer candidate); no kernel of
segment_kernels.hip uses scratch."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geodesic_cases as GC
import segment_cases as SC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_volume_segments", "d3f_path_shorten")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_segment_symbols_and_unchanged_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
    assert int(re.search(r"#define D3F_SEGMENT_CUT_CORNERS (\d+)u", hdr).group(1)) == _lib.SEGMENT_CUT_CORNERS == 1


def test_segment_validation_status_codes():
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)
    err = lib.d3f_last_error

    def segments(free=p, value=p, shape=(4, 5, 6), a=p, b=p, n=3, flags=0, clear=p, last=p, blocked=p, min_value=p, min_voxel=p):
        return lib.d3f_volume_segments(free, value, shape[0], shape[1], shape[2], a, b, n, flags, clear, last, blocked, min_value, min_voxel, None)

    def shorten(free=p, shape=(4, 5, 6), voxels=p, length=p, n=3, row_len=8, max_span=8, flags=0, index=p, out_voxels=p, count=p):
        return lib.d3f_path_shorten(free, shape[0], shape[1], shape[2], voxels, length, n, row_len, max_span, flags, index, out_voxels, count, None)

    # D3F_ERR_INVALID_ARG
    for kw in ("free", "a", "b"):
        assert segments(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    assert segments(clear=None, last=None, blocked=None, min_value=None, min_voxel=None) == _lib.ERR_INVALID_ARG and b"every output" in err()
    assert segments(value=None) == _lib.ERR_INVALID_ARG and b"need value" in err()
    assert segments(value=None, min_value=None) == _lib.ERR_INVALID_ARG and segments(value=None, min_voxel=None) == _lib.ERR_INVALID_ARG
    for flags in (2, 3, 4, 0x80000000):
        assert segments(flags=flags) == _lib.ERR_INVALID_ARG and shorten(flags=flags) == _lib.ERR_INVALID_ARG and b"flag" in err(), flags
    assert segments(n=-1) == _lib.ERR_INVALID_ARG and shorten(n=-1) == _lib.ERR_INVALID_ARG and b"n=" in err()
    for kw in ("free", "voxels", "length"):
        assert shorten(**{kw: None}) == _lib.ERR_INVALID_ARG and b"NULL" in err(), kw
    assert shorten(count=None) == _lib.ERR_INVALID_ARG and b"out_count" in err()
    assert shorten(index=None, out_voxels=None) == _lib.ERR_INVALID_ARG and b"both NULL" in err()
    assert shorten(row_len=0) == _lib.ERR_INVALID_ARG and shorten(row_len=-4) == _lib.ERR_INVALID_ARG and b"row_len" in err()
    assert shorten(max_span=0) == _lib.ERR_INVALID_ARG and shorten(max_span=-1) == _lib.ERR_INVALID_ARG and b"max_span" in err()
    # D3F_ERR_BAD_SHAPE
    for bad in ((0, 5, 6), (4, 16385, 6), (4, 5, -2), (2048, 1024, 1024)):
        assert segments(shape=bad) == _lib.ERR_BAD_SHAPE and shorten(shape=bad) == _lib.ERR_BAD_SHAPE and b"extent" in err(), bad
    # D3F_ERR_BAD_LAYOUT: every int32 pointer; free and out_clear are bytes
    for kw in ("value", "a", "b", "last", "blocked", "min_value", "min_voxel"):
        assert segments(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    for kw in ("voxels", "length", "index", "out_voxels", "count"):
        assert shorten(**{kw: odd}) == _lib.ERR_BAD_LAYOUT and b"aligned" in err(), kw
    # n == 0: D3F_OK and nothing launched, whatever the input pointers; the legal forms pass every check (and stop there without a GPU)
    assert segments(n=0) == _lib.OK and segments(n=0, free=None, a=None, b=None) == _lib.OK and segments(n=0, free=odd, clear=odd) == _lib.OK
    assert segments(n=0, value=None, min_value=None, min_voxel=None) == _lib.OK and segments(n=0, flags=1) == _lib.OK
    for only in ("clear", "last", "blocked", "min_value", "min_voxel"):
        rest = {k: None for k in ("clear", "last", "blocked", "min_value", "min_voxel") if k != only}
        assert segments(n=0, **rest) == _lib.OK, only
    assert segments(n=0, shape=(1, 1, 1)) == _lib.OK and segments(n=0, shape=(16384, 1, 2)) == _lib.OK and segments(n=0, shape=(2047, 1024, 1024)) == _lib.OK
    assert shorten(n=0) == _lib.OK and shorten(n=0, free=None, voxels=None, length=None) == _lib.OK and shorten(n=0, flags=1, free=odd) == _lib.OK
    assert shorten(n=0, index=None) == _lib.OK and shorten(n=0, out_voxels=None) == _lib.OK and shorten(n=0, row_len=1, max_span=2 ** 31 - 1) == _lib.OK
    assert segments(n=0, shape=(0, 1, 1)) == _lib.ERR_BAD_SHAPE and shorten(n=0, count=None) == _lib.ERR_INVALID_ARG      # validation comes first
    # more segments or rows than one launch holds (256 segments, 4 rows per workgroup, 2^31 - 1 workgroups): D3F_ERR_BAD_SHAPE, nothing launched
    assert segments(n=(2 ** 31 - 1) * 256 + 1) == _lib.ERR_BAD_SHAPE and b"too large" in err()
    assert shorten(n=(2 ** 31 - 1) * 4 + 1) == _lib.ERR_BAD_SHAPE and b"too large" in err()
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(shorten(max_span=0))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- the walk against the cube test ---------------------------------------------------------------------------------------------------
def check_walk(a, b):
    """both rules: the union of the events is the touched set of the definition, t never falls -> (edge ties, corner ties) of the strict walk"""
    for strict in (True, False):
        events = SC.walk_ref(a, b, strict)
        union = set(v for _, touched, _ in events for v in touched)
        assert union == SC.touched_ref(a, b, strict), (a, b, strict, sorted(union ^ SC.touched_ref(a, b, strict)))
        assert all(events[k][0] <= events[k + 1][0] for k in range(len(events) - 1)) and events[0][1] == [tuple(a)] and events[-1][2] == tuple(b)
        assert len(events) <= sum(abs(q - p) for p, q in zip(a, b)) + 1
        if not strict:
            assert all(len(touched) == 1 for _, touched, _ in events)
    events = SC.walk_ref(a, b, True)
    return sum(len(t) == 3 for _, t, _ in events), sum(len(t) == 7 for _, t, _ in events)


def signed(offset):
    return sorted(set(tuple(s * c for s, c in zip(signs, offset)) for signs in itertools.product((1, -1), repeat=3)))


def test_walk_equals_the_cube_test_on_the_listed_directions():
    o = (4, 4, 4)
    assert check_walk(o, o) == (0, 0) and SC.touched_ref(o, o, True) == SC.touched_ref(o, o, False) == {o}
    for axis in ((5, 0, 0), (0, 5, 0), (0, 0, 5), (-5, 0, 0), (0, -5, 0), (0, 0, -5)):
        assert check_walk(o, tuple(p + d for p, d in zip(o, axis))) == (0, 0)
    for base, ties in (((1, 1, 0), (1, 0)), ((1, 0, 1), (1, 0)), ((0, 1, 1), (1, 0)), ((1, 1, 1), (0, 1)), ((3, 3, 0), (3, 0)), ((0, 3, 3), (3, 0)),
                       ((3, 0, 3), (3, 0)), ((3, 3, 3), (0, 3))):
        for d in signed(base):
            assert check_walk(o, tuple(p + q for p, q in zip(o, d))) == ties, d
    for base in ((6, 3, 2), (9, 3, 1), (4, 2, 0)):
        for perm in set(itertools.permutations(base)):
            for d in signed(perm):
                a = tuple(9 if c < 0 else 0 for c in d)
                check_walk(a, tuple(p + q for p, q in zip(a, d)))
    # the two rules side by side on the smallest ties: an edge move touches its 2 side voxels, a corner move its 6, under the strict rule only
    assert SC.touched_ref((0, 0, 0), (1, 1, 0), False) == {(0, 0, 0), (1, 1, 0)}
    assert SC.touched_ref((0, 0, 0), (1, 1, 0), True) == {(0, 0, 0), (1, 1, 0), (1, 0, 0), (0, 1, 0)}
    assert SC.touched_ref((0, 0, 0), (1, 1, 1), False) == {(0, 0, 0), (1, 1, 1)}
    assert len(SC.touched_ref((0, 0, 0), (1, 1, 1), True)) == 8
    for name, (shape, a, b, sides) in SC.TIES.items():
        assert SC.touched_ref(a, b, True) - SC.touched_ref(a, b, False) == set(sides), name


def test_walk_equals_the_cube_test_on_random_pairs():
    rng = np.random.default_rng(3)
    edge = corner = 0
    for _ in range(400):
        a, b = tuple(rng.integers(0, 9, 3).tolist()), tuple(rng.integers(0, 9, 3).tolist())
        e, c = check_walk(a, b)
        edge, corner = edge + e, corner + c
    assert edge >= 100 and corner >= 20, (edge, corner)


# ---- properties of clear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.RANDOM))
def test_case_sets_hold_what_the_device_tests_rely_on(name):
    """on the restatement: the clear share of each random case lies inside [0.2, 0.8]; each 3-D case has at least 5 segments whose outputs
    differ between the rules; clear is symmetric in a, b; the open rule passes whatever the strict rule passes"""
    free, value, a, b = SC.volume(name)
    strict, open_ = SC.volume_reference(name, True, True), SC.volume_reference(name, False, True)
    for got in (strict, open_):
        assert 0.2 <= got[0].mean() <= 0.8, (name, got[0].mean())
    assert (open_[0] >= strict[0]).all()
    differ = sum(any(s[k] != o[k] for s, o in zip(strict, open_)) for k in range(SC.N_PAIRS))
    if name in SC.RANDOM_3D:
        assert differ >= 5, (name, differ)
    for rule, got in ((True, strict), (False, open_)):
        back = SC.segments_ref(free, None, b[:150], a[:150], rule)
        assert np.array_equal(back[0], got[0][:150]), (name, rule)
    # ties of the value occur: on at least 5 segments the minimum is taken at more than one of the voxels touched before the blocking event
    flat_free, flat_value, ties = free.reshape(-1), value.reshape(-1), 0
    for k in range(SC.N_PAIRS):
        if strict[4][k] < 0:
            continue
        seen = set()
        for _, touched, _ in SC.walk_ref(SC._coords(a[k], free.shape), SC._coords(b[k], free.shape), True):
            idx = [SC._flat(v, free.shape) for v in touched]
            if any(flat_free[i] == 0 for i in idx):
                break
            seen.update(idx)
        assert min(flat_value[i] for i in seen) == strict[3][k] and strict[4][k] in seen
        ties += sum(flat_value[i] == strict[3][k] for i in seen) >= 2
    assert ties >= 5, (name, ties)


def test_every_travel_move_is_clear_under_the_open_rule():
    for name, conn, w in (("17x17x17 45%", 26, (3, 4, 5)), ("13x11x19 70%", 18, (2, 3, 3)), ("serpentine", 26, (3, 4, 5))):
        free, _, _ = GC.case(name)
        cost, nxt, _ = GC.reference(name, conn, w)
        c = cost.reshape(-1)
        starts = np.flatnonzero(c != GC.INT32_MAX)[::23]
        rows, length, reached = GC.follow_ref(nxt, starts, free.size)
        assert reached.all()
        blocked_strict = 0
        for r in range(len(starts)):
            for k in range(int(length[r]) - 1):
                assert SC.clear_ref(free, rows[r, k], rows[r, k + 1], False) == 1, (name, r, k)
                blocked_strict += 1 - SC.clear_ref(free, rows[r, k], rows[r, k + 1], True)
        assert blocked_strict > 0, name                           # and the strict rule does refuse some diagonal moves past a wall


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def test_serpentine_and_pillar_figures():
    for conn, L in ((6, 467), (18, 397), (26, 397)):
        free, rows, length = SC.serpentine_rows(conn)
        assert rows.shape == (1, L) and int(length[0]) == L
        row = rows[0].tolist()
        memo = SC._CLEAR_MEMO.setdefault(("serpentine %d" % conn, True), {})            # shared with shorten_reference: the same segments
        not_clear = sum(1 - SC.clear_ref(free, row[k], row[k + 1], True, memo) for k in range(L - 1))
        assert not_clear == (0 if conn == 6 else 70), (conn, not_clear)
        oi, _, oc = SC.shorten_reference("serpentine %d" % conn, 64, True)           # (max_span 64 keeps this short)
        index = oi[0, :oc[0]].tolist()
        assert index[0] == 0 and index[-1] == L - 1 and len(index) > 64                 # several chunks of candidates, many anchors
        if conn != 6:                                                                  # the moves that are not clear are kept all the same
            kept = sum(1 for p, q in zip(index, index[1:]) if q == p + 1 and not SC.clear_ref(free, row[p], row[q], True, memo))
            assert kept == 70
    # 18 and 26 are one case, not two: the same row, and on it both rules keep the same anchors; the row of 6 tells the rules apart at max_span 2
    assert np.array_equal(SC.serpentine_rows(18)[1], SC.serpentine_rows(26)[1])
    assert all(np.array_equal(s, o) for s, o in zip(SC.shorten_reference("serpentine 26", 2, True), SC.shorten_reference("serpentine 26", 2, False)))
    assert (int(SC.shorten_reference("serpentine 6", 2, True)[2][0]), int(SC.shorten_reference("serpentine 6", 2, False)[2][0])) == (252, 234)
    free, rows, length = SC.pillar_rows()
    notes = {}
    for strict in (True, False):
        for r in range(len(SC.PILLAR_STARTS)):
            note = []
            index, vox = SC.shorten_ref(free, rows[r].tolist(), length[r], rows.shape[1], strict, note)
            notes[strict, r] = note
            assert index[0] == 0 and index[-1] == int(length[r]) - 1 and vox[-1] == SC._flat(SC.PILLAR_GOAL, SC.PILLAR_SHAPE) and len(index) < int(length[r])
    # visibility along a row is not monotone: the route from (5, 18, 2) has an anchor whose chosen j lies beyond a blocked nearer j, so a scan
    # that stops at the first blocked candidate cannot pass the device test
    assert notes[True, 2] and sum(len(v) for v in notes.values()) >= 1
    # a first-blocked scan does differ there
    row, L = rows[2].tolist(), int(length[2])
    i = notes[True, 2][0]
    j = i + 1
    while j + 1 < L and SC.clear_ref(free, row[i], row[j + 1], True):
        j += 1
    index, _ = SC.shorten_ref(free, row, L, L, True)
    assert index[index.index(i) + 1] > j


def test_shorten_ref_edge_cases():
    free, rows, length = SC.random_rows()
    assert length.tolist() == SC.RANDOM_ROW_LENGTHS and rows.shape == (6, SC.RANDOM_ROW_LEN)
    for strict in (True, False):
        oi, ov, oc = SC.shorten_reference("random", 1, strict)
        assert oc.tolist() == SC.RANDOM_ROW_LENGTHS                                      # max_span = 1 keeps every entry
        assert all(oi[r, :oc[r]].tolist() == list(range(oc[r])) and np.array_equal(ov[r, :oc[r]], rows[r, :oc[r]]) for r in range(6))
        assert ov[4, 30] == -1 and ov[5, 100] == free.size                               # entries outside the volume are kept as they are
        for span in (2, 64, 65, SC.RANDOM_ROW_LEN):
            oi, ov, oc = SC.shorten_reference("random", span, strict)
            assert oc[:3].tolist() == [0, 1, 2] and (oi[0] == -1).all() and oi[1, 0] == 0 and (oi[1, 1:] == -1).all()
            for r in range(2, 6):
                k = int(oc[r])
                assert oi[r, 0] == 0 and oi[r, k - 1] == length[r] - 1 and (np.diff(oi[r, :k]) >= 1).all() and (np.diff(oi[r, :k]) <= span).all()
                assert (oi[r, k:] == -1).all() and (ov[r, k:] == -1).all()
                # an entry outside the volume is never the end of a clear segment: it is reached by a single step only and left by one
                for bad in ((30,) if r == 4 else (100,) if r == 5 else ()):
                    at = oi[r, :k].tolist()
                    if bad in at:
                        q = at.index(bad)
                        assert at[q - 1] == bad - 1 and at[q + 1] == bad + 1
    # a length outside 0 .. row_len is clamped into it
    assert SC.shorten_ref(free, rows[5].tolist(), 10 ** 6, 4, True) == SC.shorten_ref(free, rows[5].tolist(), SC.RANDOM_ROW_LEN, 4, True)
    assert SC.shorten_ref(free, rows[5].tolist(), -3, 4, True) == ([], [])


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "segment_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("segment_kernelILb1ELb1E", "segment_kernelILb1ELb0E", "segment_kernelILb0ELb1E", "segment_kernelILb0ELb0E", "shorten_kernelILb1E",
                   "shorten_kernelILb0E"):
        assert kernel in names, (kernel, out[-800:])
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0 and vgpr <= 64 and occ >= 8, (name, vgpr, scratch, occ)
