"""CPU: ABI 16 (per-component pooling of the baked field, d3f_volume_pool) is declared by the header, the binding and the library; the entry
point validates its arguments on the host with the documented status codes and launches nothing; the workspace size is 0 exactly for
rejected arguments; the NumPy restatement (tests/pool_cases.py) equals independent plain-Python forms, stays inside the first-order error
bound of its summation order against float64, and follows the vote rule at ties and NaNs; no kernel of pool_kernels.hip uses scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pool_cases as PC
from conftest import ROOT
from d3fields_amd import _lib

HEADER = os.path.join(ROOT, "include", "d3fields_hip.h")
SYMBOLS = ("d3f_volume_pool_workspace_bytes", "d3f_volume_pool")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_pool_symbols_and_version():
    lib = _lib.load()
    hdr = open(HEADER).read()
    assert lib.d3f_abi_version() == _lib.ABI_VERSION == 16
    assert int(re.search(r"#define D3F_ABI_VERSION (\d+)", hdr).group(1)) == 16
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
    for macro, value in (("D3F_POOL_MEAN", _lib.POOL_MEAN), ("D3F_POOL_VOTES", _lib.POOL_VOTES), ("D3F_POOL_CHUNK", _lib.POOL_CHUNK),
                         ("D3F_POOL_MAX_VOTE_CHANNELS", _lib.POOL_MAX_VOTE_CHANNELS)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro
    assert PC.CHUNK == _lib.POOL_CHUNK == 256


REJECTED = [(0, 4, 4, 1, 8, 8), (4, 0, 4, 1, 8, 8), (4, 4, 0, 1, 8, 8), (-1, 4, 4, 1, 8, 8), (16385, 1, 1, 1, 8, 8), (2048, 1024, 1024, 1, 8, 8),
            (4, 4, 4, -1, 8, 8), (4, 4, 4, 65, 8, 8), (4, 4, 4, 3, -1, 8), (4, 4, 4, 3, 8, -1), (4, 4, 4, 3, 8, 8 * 4096 + 1)]
ACCEPTED = [(1, 1, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1), (4, 4, 4, 64, 64, 8 * 4096), (4, 5, 6, 3, 0, 7), (4, 5, 6, 3, 10 ** 12, 7), (16384, 1, 2, 5, 300, 0),
            (64, 64, 64, 1000, 70000, 1027), (256, 256, 256, 100000, 1 << 24, 384), (2047, 1024, 1024, 7, 1 << 20, 1024)]


def test_pool_workspace_bytes_is_zero_exactly_for_rejected_arguments():
    lib = _lib.load()
    for args in REJECTED:
        assert lib.d3f_volume_pool_workspace_bytes(*args) == 0, args
    for args in ACCEPTED:
        got = lib.d3f_volume_pool_workspace_bytes(*args)
        assert got > 0 and got % 8 == 0, (args, got)
    # more room costs more, and a capacity above the voxel count costs what the voxel count does
    assert lib.d3f_volume_pool_workspace_bytes(64, 64, 64, 10, 1000, 64) < lib.d3f_volume_pool_workspace_bytes(64, 64, 64, 10, 100000, 64)
    assert lib.d3f_volume_pool_workspace_bytes(4, 5, 6, 3, 120, 7) == lib.d3f_volume_pool_workspace_bytes(4, 5, 6, 3, 10 ** 12, 7)


def test_pool_validation_status_codes():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(258)
    half = ctypes.c_void_p(260)             # aligned to 4, not to 8
    shape = (4, 5, 6)

    def sets_of(*cs, data=256, stride=None, fill=None):
        arr = (_lib.VolumeSet * max(len(cs), 1))()
        for s, c in enumerate(cs):
            arr[s] = _lib.VolumeSet(data, c, 0, c if stride is None else stride, fill)
        return arr

    def pool(label=p, shape=shape, K=3, valid=None, slot=None, sets=None, n_sets=None, modes=(0,), cap=50, members=p, count=p, moments=p, rows=(256,), ws=p,
             wsb=None, null_modes=False, null_rows=False):
        sets_arr = sets_of(16) if sets is None else sets
        n = len(modes) if n_sets is None else n_sets
        marr = (ctypes.c_int32 * max(len(modes), 1))(*modes)
        rarr = (ctypes.c_void_p * max(len(rows), 1))(*rows)
        if wsb is None:
            wsb = 1 << 62
        return lib.d3f_volume_pool(label, shape[0], shape[1], shape[2], K, valid, slot, None if sets == "null" else sets_arr, n, None if null_modes else marr, cap,
                                   members, count, moments, None if null_rows else rarr, ws, wsb, None)

    err = lib.d3f_last_error
    # D3F_ERR_INVALID_ARG
    assert pool(label=None) == _lib.ERR_INVALID_ARG and b"label" in err()
    assert pool(members=None) == _lib.ERR_INVALID_ARG and pool(count=None) == _lib.ERR_INVALID_ARG
    assert pool(K=-1) == _lib.ERR_INVALID_ARG and b"K=" in err()
    assert pool(n_sets=-1) == _lib.ERR_INVALID_ARG and pool(n_sets=_lib.MAX_MAPS + 1) == _lib.ERR_INVALID_ARG and b"n_sets" in err()
    assert pool(sets="null") == _lib.ERR_INVALID_ARG and pool(null_modes=True) == _lib.ERR_INVALID_ARG and pool(null_rows=True) == _lib.ERR_INVALID_ARG
    assert pool(sets=sets_of(16, data=None)) == _lib.ERR_INVALID_ARG and b"data" in err()
    assert pool(rows=(None,)) == _lib.ERR_INVALID_ARG and b"out_rows" in err()
    for bad in (2, -1, 7):
        assert pool(modes=(bad,)) == _lib.ERR_INVALID_ARG and b"mode" in err(), bad
    assert pool(cap=-1) == _lib.ERR_INVALID_ARG and b"member_capacity" in err()
    # D3F_ERR_BAD_SHAPE
    for bad in ((0, 5, 6), (4, 16385, 6), (4, 5, -2)):
        assert pool(shape=bad) == _lib.ERR_BAD_SHAPE and b"extent" in err(), bad
    assert pool(shape=(2048, 1024, 1024)) == _lib.ERR_BAD_SHAPE and b"voxels" in err()
    assert pool(K=121) == _lib.ERR_BAD_SHAPE and b"K=" in err()
    assert pool(sets=sets_of(0)) == _lib.ERR_BAD_SHAPE and pool(sets=sets_of(4097)) == _lib.ERR_BAD_SHAPE and b"C=" in err()
    assert pool(sets=sets_of(257), modes=(_lib.POOL_VOTES,)) == _lib.ERR_BAD_SHAPE and b"votes" in err()
    # D3F_ERR_BAD_LAYOUT
    assert pool(label=odd) == _lib.ERR_BAD_LAYOUT and pool(slot=odd) == _lib.ERR_BAD_LAYOUT and pool(count=odd) == _lib.ERR_BAD_LAYOUT
    assert pool(members=half) == _lib.ERR_BAD_LAYOUT and pool(moments=half) == _lib.ERR_BAD_LAYOUT and b"aligned" in err()
    assert pool(sets=sets_of(16, stride=15)) == _lib.ERR_BAD_LAYOUT and b"stride_voxel" in err()
    assert pool(sets=sets_of(16, data=258)) == _lib.ERR_BAD_LAYOUT and pool(sets=sets_of(16, fill=258)) == _lib.ERR_BAD_LAYOUT
    assert pool(rows=(258,)) == _lib.ERR_BAD_LAYOUT and b"aligned" in err()
    assert pool(ws=half) == _lib.ERR_BAD_LAYOUT and b"workspace" in err()
    # D3F_ERR_WORKSPACE: NULL, or one byte short of what the size function says for the call's own mean channels
    need = lib.d3f_volume_pool_workspace_bytes(*shape, 3, 50, 16)
    assert pool(ws=None) == _lib.ERR_WORKSPACE and pool(wsb=need - 1) == _lib.ERR_WORKSPACE and pool(wsb=0) == _lib.ERR_WORKSPACE and b"workspace" in err()
    two = dict(sets=sets_of(16, 8), modes=(_lib.POOL_MEAN, _lib.POOL_VOTES), rows=(256, 512))
    assert pool(wsb=need - 1, **two) == _lib.ERR_WORKSPACE                      # the votes set adds no mean channels ...
    need2 = lib.d3f_volume_pool_workspace_bytes(*shape, 3, 50, 24)
    assert need2 >= need and pool(wsb=need2 - 1, sets=sets_of(16, 8), modes=(0, 0), rows=(256, 512)) == _lib.ERR_WORKSPACE      # ... a mean set does
    # the legal forms pass every check before the workspace (and stop there: nothing is launched without a GPU)
    assert pool(ws=None, valid=odd, moments=None) == _lib.ERR_WORKSPACE        # valid is bytes; out_moments is optional
    assert pool(ws=None, n_sets=0, sets="null", null_modes=True, null_rows=True) == _lib.ERR_WORKSPACE
    assert pool(ws=None, K=0) == _lib.ERR_WORKSPACE and pool(ws=None, K=120, cap=0) == _lib.ERR_WORKSPACE
    assert pool(ws=None, sets=sets_of(256, stride=300), modes=(_lib.POOL_VOTES,)) == _lib.ERR_WORKSPACE
    assert pool(ws=None, sets=sets_of(4096, data=260)) == _lib.ERR_WORKSPACE   # a base off by one float: the scalar path, not an error
    with pytest.raises(_lib.D3FError) as e:
        _lib.check(pool(K=-3))
    assert e.value.code == _lib.ERR_INVALID_ARG


# ---- fold ---------------------------------------------------------------------------------------------------------------------------
def plain_fold(rows):
    """the definition, recursively, one Python-level add per row"""
    if len(rows) <= 256:
        acc = rows[0]
        for r in rows[1:]:
            acc = acc + r
        return acc
    return plain_fold([plain_fold(rows[i:i + 256]) for i in range(0, len(rows), 256)])


@pytest.mark.parametrize("length", [1, 2, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537])
def test_fold_equals_the_plain_recursion(length):
    rows = PC.field_rows(length, 2, length)
    want = plain_fold([np.float32(x) for x in rows[:, 0]]), plain_fold([np.float32(x) for x in rows[:, 1]])
    got = PC.fold(rows)
    assert got.dtype == np.float32 and got.view(np.int32).tolist() == np.array(want, dtype=np.float32).view(np.int32).tolist(), length
    assert PC.fold_levels(length) == (1 if length <= 256 else 2 if length <= 65536 else 3)


def test_fold_of_one_row_is_that_row_and_negative_zero_stays():
    row = np.array([[-0.0, 1.5, -3.25]], dtype=np.float32)
    assert PC.fold(row).view(np.int32).tolist() == row[0].view(np.int32).tolist()
    zeros = np.full((300, 3), -0.0, dtype=np.float32)
    assert np.signbit(PC.fold(zeros)).all() and np.signbit(PC.fold(zeros) / np.float32(300)).all()


# ---- pool_ref -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x8x10", "65x3x67", "256 and 257", "three levels", "K 300"])
def test_pool_ref_is_inside_the_first_order_bound_of_its_order(name):
    label, K = PC.volume(name)
    rows = PC.field_rows(label.size, 5, 21)
    got = PC.pool_ref(label, K, rows)
    spare = []
    for k, members in enumerate(PC.member_lists(label, K)):
        if len(members) == 0:
            continue
        x = rows[members].astype(np.float64)
        L = PC.fold_levels(len(members))
        bound = 1.01 * (255 * L + 1) * 2.0 ** -24 * np.abs(x).mean(axis=0)
        err = np.abs(got[k].astype(np.float64) - x.mean(axis=0))
        assert (err <= bound).all(), (name, k, err.max(), bound.min())
        spare.append((bound / np.maximum(err, 1e-300)).min())
    assert len(spare) > 0


def brute_force(label, K, rows, valid=None, slot=None):
    """one Python step per voxel: the members' rows in flat order per component, then the chunked sums"""
    lists = [[] for _ in range(K)]
    flat = label.reshape(-1)
    for v in range(flat.size):
        k = int(flat[v])
        if not 1 <= k <= K:
            continue
        if valid is not None and valid.reshape(-1)[v] == 0:
            continue
        if slot is not None and slot.reshape(-1)[v] < 0:
            continue
        lists[k - 1].append(rows[v if slot is None else int(slot.reshape(-1)[v])].copy())
    out = np.zeros((K, rows.shape[1]), dtype=np.float32)
    for k, rws in enumerate(lists):
        if rws:
            out[k] = plain_fold(rws) / np.float32(len(rws))
    return out, [len(r) for r in lists]


@pytest.mark.parametrize("name", PC.SMALL)
def test_pool_ref_equals_the_per_voxel_loop(name):
    label, K = PC.volume(name)
    rng = np.random.default_rng(3)
    rows = PC.field_rows(label.size, 3, 22)
    valid = (rng.random(label.shape) < 0.8).astype(np.uint8)
    keep = rng.random(label.size) < 0.7
    slot = np.full(label.size, -1, dtype=np.int32)
    slot[keep] = rng.permutation(int(keep.sum())).astype(np.int32)
    for kw in ({}, {"valid": valid}, {"valid": valid, "slot": slot.reshape(label.shape)}):
        data = rows if "slot" not in kw else rows[:int(keep.sum())]
        want, counts = brute_force(label, K, data, **kw)
        got = PC.pool_ref(label, K, data, **kw)
        assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (name, sorted(kw))
        assert PC.counts_ref(label, K, **kw).tolist() == counts
        moments = PC.moments_ref(label, K, **kw)
        assert moments[:, 0].tolist() == [sum(int(np.unravel_index(v, label.shape)[0]) for v in m) for m in PC.member_lists(label, K, **kw)]


def test_pool_ref_fill_rows_and_foreign_labels():
    label, K = PC.volume("gaps")
    rows = PC.field_rows(label.size, 4, 23)
    fill = np.array([1, 2, 3, 4], dtype=np.float32)
    counts = PC.counts_ref(label, K)
    assert (counts[[1, 4, 5, 8]] == 0).all() and (np.delete(counts, [1, 4, 5, 8]) > 0).all()
    assert (PC.pool_ref(label, K, rows, fill=fill)[[1, 4, 5, 8]] == fill).all() and (PC.pool_ref(label, K, rows)[[1, 4, 5, 8]] == 0).all()
    assert (PC.moments_ref(label, K)[[1, 4, 5, 8]] == 0).all() and (PC.votes_ref(label, K, rows)[[1, 4, 5, 8]] == 0).all()
    foreign, K = PC.volume("foreign")
    assert {-1, K + 1, PC.INT32_MIN} <= set(np.unique(foreign).tolist())
    clean = np.where((foreign >= 1) & (foreign <= K), foreign, 0)
    assert PC.counts_ref(foreign, K).tolist() == PC.counts_ref(clean, K).tolist() and PC.counts_ref(foreign, K).sum() == (clean > 0).sum()


def test_case_conditions():
    label, K = PC.volume("three levels")
    assert label.shape == (41, 40, 41) and PC.counts_ref(label, K).tolist() == [65537, 255, 41 * 40 * 41 - 65537 - 255]
    assert PC.fold_levels(65537) == 3 and [-(-65537 // 256), -(-257 // 256)] == [257, 2]
    assert PC.counts_ref(*PC.volume("256 and 257")).tolist() == [256, 257]
    assert PC.volume("K 300")[1] >= 256 and (PC.counts_ref(*PC.volume("K 300")) > 0).all()
    assert PC.volume("65x3x67")[0].shape == (65, 3, 67) and PC.volume("2x3x33")[0].shape == (2, 3, 33)
    assert set(PC.SMALL) <= set(PC.VOLUMES)
    rows = PC.field_rows(1000, 7, 1, stride=9)
    assert rows.strides[0] == 36 and (np.abs(rows) >= 0.25).all() and (np.abs(rows) < 4).all() and (rows < 0).any()


# ---- votes --------------------------------------------------------------------------------------------------------------------------
def test_vote_rule_at_ties_and_nans():
    nan = np.nan
    rows = np.array([[1, 1, 1, 1], [0, 2, 2, 1], [nan, 5, 1, 1], [1, nan, 3, 3], [1, nan, nan, nan], [-0.0, 0.0, 0.0, -1], [nan, nan, nan, nan],
                     [-np.inf, -np.inf, nan, -np.inf], [3, 2, 1, 0], [0, 1, 2, 3], [np.inf, np.inf, 0, 0], [2, nan, 2, 5]], dtype=np.float32)
    want = [0, 1, 0, 2, 0, 0, 0, 0, 0, 3, 0, 3]
    assert PC.argmax_rule(rows).tolist() == want
    for row, w in zip(rows, want):          # the rule, as written
        best = 0
        for c in range(1, 4):
            if row[c] > row[best]:
                best = c
        assert best == w
    assert PC.argmax_rule(np.array([[7.0]], dtype=np.float32)).tolist() == [0] and PC.argmax_rule(np.array([[nan]], dtype=np.float32)).tolist() == [0]
    label, K = PC.volume("9x8x10")
    for C in PC.VOTE_CHANNELS:
        rows = PC.vote_rows(label.size, C, 40 + C)
        votes = PC.votes_ref(label, K, rows)
        assert votes.dtype == np.int32 and votes.sum(axis=1).tolist() == PC.counts_ref(label, K).tolist()
        if C > 1:
            top = np.nanmax(np.where(np.isnan(rows), -np.inf, rows), axis=1)
            assert ((rows == top[:, None]).sum(axis=1) > 1).mean() > 0.2 and np.isnan(rows[:, 0]).any()      # exact ties and NaNs at channel 0 are there


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_kernel_of_the_family_uses_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), "pool_kernels.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = [re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()]
    rows = [(m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5))) for m in rows if m]
    names = " ".join(r[0] for r in rows)
    for kernel in ("pool_zero_kernel", "pool_flag_kernel", "pool_compact_kernel", "pool_sort_count_kernel", "pool_sort_scatter_kernel", "pool_prep_kernel",
                   "pool_level_kernelILb1E", "pool_level_kernelILb0E", "pool_finish_kernel"):
        assert kernel in names, (kernel, out[-800:])
    for name, vgpr, scratch, occ in rows:
        assert scratch == 0 and vgpr <= 128 and occ >= 4, (name, vgpr, scratch, occ)
