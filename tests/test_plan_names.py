"""CPU: what Fusion.last_plan() reports -- the kernel instance, the point-order sentence, tile size, workgroups, family, the
gate and its window side -- over a matrix of plan queries, against the table recorded in plan_names.json.

bench.py finds a launch's row in the counter output by last_plan()["kernel"] and the GPU suites assert on it, so the string has
to be the name of the instance the launcher really takes.  The table pins every name and sentence: it is a record, compared
whole, and is never rewritten from the code under test (an entry changes only by hand, with the launcher's line as the reason).
No GPU is needed: d3f_eval_plan_query does no device work and Fusion._record_plan needs only the loaded library.

Not in the table, because no plan query reaches them: the distance-only instances with GRID = true (d3f_eval_grid: points from
axis arrays) and with MODE = 1 (d3f_eval_dist), and fused_eval_kernel<1>; plan queries describe d3f_eval / d3f_eval_lattice."""
import json
import os
import types

import pytest

from d3fields_amd import _lib
from d3fields_amd.fusion import Fusion

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_names.json")
F, U, L = _lib.FLAG_FINITE_MAPS, _lib.FLAG_UNORDERED_POINTS, _lib.FLAG_LOCAL_POINTS
DIRECT, NOGATE = _lib.TUNE_DIRECT_GATHER, _lib.TUNE_NO_WINDOW_GATE
FAMILIES = {"dist-only", "lds-window", "cell-runs", "channel-sliced", "direct", "register-rows"}

# (name, V, H, W, maps [(fh, fw, C)] wide map first, lattice dims or None, cloud sizes)
SHAPES = [
    # oracle/field_cases.py
    ("direct V4 C384", 4, 96, 128, [(12, 16, 384)], None, [3000]),
    ("direct V1 C1000", 1, 96, 128, [(12, 16, 1000)], None, [3000]),
    ("direct V9 C65 + C64", 9, 96, 128, [(12, 16, 65), (12, 16, 64)], None, [3000]),
    ("direct V2 C384 C1024", 2, 96, 128, [(12, 16, 384), (12, 16, 1024)], None, [2000]),
    ("direct C129 + C128", 4, 96, 128, [(12, 16, 129), (12, 16, 128)], None, [3000]),
    ("direct edges", 4, 96, 128, [(9, 17, 96), (96, 128, 72), (1, 16, 80), (12, 1, 80)], None, [3000]),
    ("wide dense C1024", 4, 96, 128, [(96, 128, 1024)], None, [4000]),
    ("strict V5", 5, 96, 128, [(12, 16, 384)], None, [3000]),
    ("batch V3 C256", 3, 96, 128, [(12, 16, 256)], None, [4000]),
    ("window C384", 4, 480, 640, [(48, 64, 384)], (74, 65, 20), [300001]),
    ("cell runs V8 C512", 8, 480, 640, [(24, 32, 512)], (74, 65, 20), [150001]),
    ("sliced 192x256", 4, 192, 256, [(192, 256, 384)], (74, 65, 20), [70001]),
    ("sliced 96x128", 4, 96, 128, [(96, 128, 384)], (74, 65, 20), [70001]),
    ("window V3 C256", 3, 480, 640, [(24, 32, 256)], (74, 65, 20), [300001]),
    ("rows V8", 8, 480, 640, [(36, 64, 1024)], (74, 65, 20), [150001]),
    ("rows V4", 4, 480, 640, [(24, 32, 1024)], (74, 65, 20), [100000]),
    ("rows V5", 5, 480, 640, [(24, 32, 1024)], (74, 65, 20), [100000]),
    ("rows V1", 1, 480, 640, [(48, 64, 1024)], (74, 65, 20), [66000]),
    # bench.py
    ("c2_dense", 4, 480, 640, [(480, 640, 384)], (160, 140, 44), [985600]),
    ("c2_patch", 4, 480, 640, [(48, 64, 384)], (160, 140, 44), [985600]),
    ("c3_dense", 4, 480, 640, [(480, 640, 384), (480, 640, 8)], (200, 175, 55), [1925000]),
    ("c3_patch", 4, 480, 640, [(48, 64, 384), (480, 640, 8)], (200, 175, 55), [1925000]),
    ("c4_patch", 8, 720, 1280, [(72, 128, 1024)], (40, 280, 88), [1000000]),
    ("c4_dense", 8, 720, 1280, [(720, 1280, 1024)], (40, 280, 88), [1000000]),
    ("c5_track", 4, 480, 640, [(48, 64, 384), (480, 640, 8)], None, [100000]),
    ("ref_patch", 4, 480, 640, [(48, 64, 1024), (480, 640, 8), (480, 640, 3)], (200, 175, 55), [1925000, 71000]),
    ("dist_only", 4, 480, 640, [], (800, 700, 220), [123200000]),
]
VIEWS = (1, 2, 3, 4, 5, 8, 16)
EDGES = (65535, 65536, 262143, 262144, (1 << 22) - 1, 1 << 22, (1 << 24) - 1, 1 << 24)
_BY_NAME = {s[0]: s for s in SHAPES}


def record(V, H, W, maps, n=0, flags=0, ws=True, inter=False, lattice=None, f16=False, wide_last=False):
    """Fusion._record_plan on a stub that holds only the library; the maps get dummy 16-aligned pointers."""
    lib = _lib.load()
    stub = types.SimpleNamespace(_lib=lib, _last_plan=None)
    v = _lib.Views(V, H, W, 16, 16, 16)
    order = list(maps[1:]) + list(maps[:1]) if wide_last else list(maps)
    arr = (_lib.ChannelMap * max(len(order), 1))()
    for i, (fh, fw, C) in enumerate(order):
        arr[i] = _lib.ChannelMap(16, fh, fw, C, _lib.DTYPE_F16 if (f16 and (fh, fw, C) == maps[0]) else _lib.DTYPE_F32,
                                 fh * fw * C, fw * C, C)
    if lattice is not None:
        n = lattice[0] * lattice[1] * lattice[2]
    Fusion._record_plan(stub, v, n, arr, len(order), flags, ws, inter, lattice)
    plan = stub._last_plan
    assert plan is not None, "plan query failed: %s" % lib.d3f_last_error().decode()
    return json.loads(json.dumps(plan))            # tuples -> lists, as the table holds them


def product_matrix():
    """key -> keyword arguments of record()"""
    out = {}

    def add(tag, **kw):
        key = "%s | %s" % (tag, " ".join("%s=%s" % (k, kw[k]) for k in sorted(kw) if k not in ("H", "W", "maps")))
        assert key not in out, key
        out[key] = kw

    for name, V, H, W, maps, dims, sizes in SHAPES:
        base = dict(V=V, H=H, W=W, maps=maps)
        cloud_flags = (0, F, F | U, F | L, F | DIRECT, F | U | NOGATE, U)
        for n in sizes:
            for flags in cloud_flags if maps else (0,):
                for ws in (True, False):
                    add(name, n=n, flags=flags, ws=ws, **base)
            if maps:
                add(name, n=n, flags=F | U, inter=True, **base)
                add(name, n=n, flags=F | U, f16=True, **base)
                add(name, n=n, flags=F | U, f16=True, ws=False, **base)
            if len(maps) > 1:
                add(name, n=n, flags=F | U, wide_last=True, **base)
        if dims is not None:
            for flags in (0, F, F | DIRECT) if maps else (0,):
                add(name, lattice=dims, flags=flags, ws=False, **base)
            if maps:
                add(name, lattice=dims, flags=F, ws=False, inter=True, **base)
                add(name, lattice=dims, flags=F, ws=False, f16=True, **base)
            if len(maps) > 1:
                add(name, lattice=dims, flags=F, ws=False, wide_last=True, **base)
    # every view count, on the shapes whose instance depends on it
    for V in VIEWS:
        for name in ("c2_patch", "c2_dense", "ref_patch", "dist_only"):
            _, _, H, W, maps, dims, sizes = _BY_NAME[name]
            if V == 4:
                continue
            add(name + " views", V=V, H=H, W=W, maps=maps, lattice=dims, flags=F if maps else 0, ws=False)
            add(name + " views", V=V, H=H, W=W, maps=maps, n=sizes[0], flags=(F | U) if maps else 0)
            if name == "c2_patch":
                add(name + " views", V=V, H=H, W=W, maps=maps, lattice=dims, flags=F, ws=False, f16=True)
        for n in ((1 << 22) - 1, 1 << 22):
            for ws in (True, False):
                add("dist_only views", V=V, H=480, W=640, maps=[], n=n, flags=0, ws=ws)
    # both sides of kSmallBatch, kWindowCloudMin and the distance-only pass's 2^22 / 2^24
    for n in EDGES:
        for name in ("c2_patch", "c2_dense", "c3_patch", "ref_patch", "c4_patch", "dist_only"):
            _, V, H, W, maps, _, _ = _BY_NAME[name]
            for flags in ((F | U, F | L) if maps else (0,)):
                for ws in (True, False):
                    add(name + " edge", V=V, H=H, W=W, maps=maps, n=n, flags=flags, ws=ws)
    return out


def experiments_matrix():
    """key -> (environment, keyword arguments of record()): the D3F_EXP_* knobs that reach the other rows of the launch ladders"""
    out = {}

    def add(env, name, **kw):
        _, V, H, W, maps, dims, sizes = _BY_NAME[name]
        kw = dict(dict(V=V, H=H, W=W, maps=maps, flags=F), **kw)
        key = "%s | %s | %s" % (" ".join("%s=%s" % (k[8:], env[k]) for k in sorted(env)), name,
                                " ".join("%s=%s" % (k, kw[k]) for k in sorted(kw) if k not in ("H", "W", "maps")))
        assert key not in out, key
        out[key] = (env, kw)

    def lattice_and_cloud(env, name, **kw):
        _, _, _, _, _, dims, sizes = _BY_NAME[name]
        add(env, name, lattice=dims, ws=False, **kw)
        add(env, name, n=sizes[0], **dict(dict(flags=F | U), **kw))

    for V in (3, 4, 8):
        for u in (2, 3, 4):
            for vc in (0, 2):
                env = {"D3F_EXP_WINDOW": "64", "D3F_EXP_WINDOW_U": str(u)}
                if vc:
                    env["D3F_EXP_WINDOW_VC"] = str(vc)
                lattice_and_cloud(env, "c2_patch" if u == 3 else "c4_patch", V=V)
        lattice_and_cloud({"D3F_EXP_WINDOW_VC": "2"}, "c2_patch", V=V)
        lattice_and_cloud({"D3F_EXP_WINDOW_VC": "2", "D3F_EXP_WINDOW_OCC": "3"}, "c2_patch", V=V)
        for occ in (2, 3, 5, 6):
            lattice_and_cloud({"D3F_EXP_WINDOW_OCC": str(occ)}, "c2_patch", V=V)
            lattice_and_cloud({"D3F_EXP_WINDOW_OCC": str(occ), "D3F_EXP_WINDOW_LPP": "32"}, "c2_patch", V=V)
        lattice_and_cloud({"D3F_EXP_WINDOW_LPP": "32"}, "c2_patch", V=V)
        lattice_and_cloud({"D3F_EXP_WINDOW": "128"}, "c2_patch", V=V)
        lattice_and_cloud({"D3F_EXP_DIST": "8"}, "dist_only", V=V, flags=0)
        add({"D3F_EXP_DIST": "8"}, "dist_only", V=V, flags=0, n=100000)
    lattice_and_cloud({"D3F_EXP_DIST": "-1"}, "dist_only", flags=0)
    lattice_and_cloud({"D3F_EXP_WINDOW": "-1"}, "c2_patch")
    lattice_and_cloud({"D3F_EXP_ROWS": "-1"}, "c4_patch")
    for sl in (1, 2, 3):
        for vc in (0, 1, 2, 4):
            env = {"D3F_EXP_SLICED": str(sl)}
            if vc:
                env["D3F_EXP_SLICED_VC"] = str(vc)
            lattice_and_cloud(env, "c2_dense")
            lattice_and_cloud(env, "c3_dense")
    lattice_and_cloud({"D3F_EXP_SLICED_VC": "4"}, "c2_dense")
    lattice_and_cloud({"D3F_EXP_SLICED_VC": "1"}, "c2_dense")
    lattice_and_cloud({"D3F_EXP_SLICED": "-1"}, "c2_dense")
    for runs in (2, 4, 8):
        for u in (0, 1, 2, 3):
            for occ in (0, 4, 5, 6):
                env = {"D3F_EXP_RUNS": str(runs)}
                if u:
                    env["D3F_EXP_RUNS_U"] = str(u)
                if occ:
                    env["D3F_EXP_RUNS_OCC"] = str(occ)
                lattice_and_cloud(env, "c2_patch")
                lattice_and_cloud(env, "c4_patch")
    for occ in (4, 5, 6):
        lattice_and_cloud({"D3F_EXP_RUNS_OCC": str(occ)}, "c2_patch", flags=F)
        lattice_and_cloud({"D3F_EXP_RUNS_OCC": str(occ)}, "cell runs V8 C512")
    return out


def _table():
    with open(TABLE) as fh:
        t = json.load(fh)
    return {sec: {k: t["plans"][i] for k, i in t[sec].items()} for sec in ("product", "experiments")}


def _compare(got, want):
    assert sorted(got) == sorted(want), "the matrix and the recorded table list different cases"
    wrong = ["%s\n    recorded %s\n    now      %s" % (k, want[k], got[k]) for k in sorted(got) if got[k] != want[k]]
    assert not wrong, "%d of %d plans differ from the record:\n%s" % (len(wrong), len(got), "\n".join(wrong[:40]))


# the rows of the launch ladders the planner reaches by itself (the product build holds no others)
PRODUCT_ROWS = (
    ["fused_eval_kernel<0>", "fused_eval_wide_kernel<0>", "fused_eval_f16_kernel<0>", "fused_eval_rows_kernel",
     "fused_eval_runs_kernel<0, 2, 8, 3>", "fused_eval_runs_kernel<0, 1, 4, 7>", "fused_eval_runs_kernel<0, 1, 8, 5>",
     "fused_eval_sliced_kernel<5, 2, 7>", "fused_eval_sliced_kernel<4, 2, 7, true>"]
    + ["fused_eval_window_kernel<1, 1, 4, 256, 16, %d, false%s>" % (vf, h) for vf in (0, 4, 8) for h in ("", ", true")]
    + ["fused_eval_dist_kernel<0, %d, %d, %s, false>" % (v, 8 if 1 <= v <= 2 else 6, t) for v in (0, 1, 2, 3, 4) for t in ("true", "false")])
# ... and on the window side of a cloud's gate (the touched-texel pool)
PRODUCT_WINDOW_SIDES = ["fused_eval_window_kernel<1, 1, 4, 256, 16, %d, true>" % vf for vf in (0, 4, 8)]


# the rows that only an experiments build holds (the #ifdef D3F_EXPERIMENTS parts of the variant lists), every one of them
_EXP_WINDOWS = [(1, 1, 6, 16), (1, 1, 5, 16), (1, 2, 4, 16), (1, 2, 3, 16), (1, 4, 4, 32), (1, 4, 3, 32), (1, 4, 2, 32), (2, 2, 2, 32), (2, 1, 2, 32),
                (3, 2, 2, 32), (3, 1, 2, 32), (4, 1, 2, 32)]
EXPERIMENT_ROWS = (
    ["fused_eval_runs_kernel<0, %d, %d, %d>" % r for r in ((3, 4, 4), (3, 2, 4), (2, 4, 4), (2, 8, 4), (1, 4, 6), (1, 8, 4), (1, 8, 6))]
    + ["fused_eval_sliced_kernel<%d, %d, %d>" % r for r in ((5, 4, 5), (4, 2, 7), (4, 1, 8), (4, 4, 5), (3, 2, 7), (3, 4, 5))]
    + ["fused_eval_window_kernel<%d, %d, %d, 256, %d, 0, false>" % r for r in _EXP_WINDOWS]
    + ["fused_eval_dist_kernel<0, %d, 8, %s, false>" % (v, t) for v in (0, 3, 4) for t in ("true", "false")])
EXPERIMENT_WINDOW_SIDES = ["fused_eval_window_kernel<%d, %d, %d, 256, %d, 0, true>" % r for r in _EXP_WINDOWS]


def test_plan_names_product(monkeypatch):
    for k in [k for k in os.environ if k.startswith("D3F_EXP_")]:
        monkeypatch.delenv(k)
    got = {key: record(**kw) for key, kw in product_matrix().items()}
    assert {p["family"] for p in got.values()} == FAMILIES
    seen = {p["kernel"] for p in got.values()}
    sides = {p["window_side"]["kernel"] for p in got.values() if p["gated_window"]}
    print("ladder rows seen:", sorted(seen), "window sides:", sorted(sides))
    assert seen == set(PRODUCT_ROWS), (sorted(seen - set(PRODUCT_ROWS)), sorted(set(PRODUCT_ROWS) - seen))
    assert sides == set(PRODUCT_WINDOW_SIDES)
    _compare(got, _table()["product"])


def test_plan_names_experiments(monkeypatch):
    if not _lib.load().d3f_build_has_experiments():
        pytest.skip("the D3F_EXP_* knobs exist in an experiments build only (python -m d3fields_amd.build --experiments)")
    got = {}
    for key, (env, kw) in experiments_matrix().items():
        for k in [k for k in os.environ if k.startswith("D3F_EXP_")]:
            monkeypatch.delenv(k)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        got[key] = record(**kw)
    seen = {p["kernel"] for p in got.values()}
    sides = {p["window_side"]["kernel"] for p in got.values() if p["gated_window"]}
    print("ladder rows seen:", sorted(seen), "window sides:", sorted(sides))
    assert set(EXPERIMENT_ROWS) <= seen, sorted(set(EXPERIMENT_ROWS) - seen)
    assert set(EXPERIMENT_WINDOW_SIDES) <= sides, sorted(set(EXPERIMENT_WINDOW_SIDES) - sides)
    _compare(got, _table()["experiments"])
