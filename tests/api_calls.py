"""Rejected calls of the C boundary (d3fields_amd/csrc/d3f_api.hip), generated: one valid base call per entry point, every single-argument
fault from a small pool per argument type, and every pair of such faults on two different arguments.  tests/api_status.json holds the status
the library returned for each row when the record was made; tests/test_api_status_host.py replays the rows and compares the lists whole.

Device pointers are made-up 256-byte aligned addresses: a recorded row is one the library rejects on the host, before any launch.  What the
library dereferences on the host (d3f_volume, d3f_band, d3f_volume_set, the weights of the geodesic calls, lower / voxel_num, the arrays of
output pointers) is real ctypes memory.  Nothing here is random; the order of the rows is the order of the code.

    python tests/api_calls.py record COMMIT [LIBRARY]

writes tests/api_status.json from LIBRARY (default: the library of the tree), built from COMMIT -- on a machine WITHOUT a GPU only, and only to
take the record of a library whose behaviour is the reference, never to make a test pass.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from d3fields_amd import _lib  # noqa: E402

RECORD = os.path.join(HERE, "api_status.json")
INVALID, SHAPE, DTYPE, LAYOUT, HIP, WORKSPACE = (_lib.ERR_INVALID_ARG, _lib.ERR_BAD_SHAPE, _lib.ERR_BAD_DTYPE, _lib.ERR_BAD_LAYOUT, _lib.ERR_HIP,
                                                 _lib.ERR_WORKSPACE)
VALIDATION = (INVALID, SHAPE, DTYPE, LAYOUT, WORKSPACE)
NAN, INF = float("nan"), float("inf")
NX, NY, NZ = 4, 5, 6

# kind -> the bad values of one argument of that kind, from its valid value
POOL = {
    "ptr": lambda a: [None, a + 1, a + 4],                 # a made-up device address
    "host": lambda a: [None],                              # real host memory: only ever NULL or whole
    "ext": lambda a: [0, -1, _lib.EDT_MAX_EXTENT + 1],
    "cnt": lambda a: [-1],
    "n": lambda a: [-1, 1 << 40],                          # a count that sizes a launch
    "flt": lambda a: [NAN, 0.0, -1.0, INF],
    "conn": lambda a: [7],
    "wsb": lambda a: [a - 1],
    "fix": lambda a: [],
}
N_FAULTS = {kind: len(POOL[kind](256)) for kind in POOL}


class S:
    """one scalar: a C argument, or a field of a struct"""
    def __init__(self, name, kind, base=None):
        self.name, self.field, self.kind, self.base = name, name, kind, base

    def leaves(self):
        return [self]

    def make(self, v, keep):
        return v[self.name]


class Struct:
    """a pointer to one host struct; its fields are arguments of their own"""
    def __init__(self, name, cls, fields):
        self.name, self.cls, self.fields, self.me = name, cls, fields, S(name, "host", True)
        for f in fields:
            f.name = "%s.%s" % (name, f.field)

    def leaves(self):
        return [self.me] + self.fields

    def fill(self, obj, v):
        for f in self.fields:
            setattr(obj, f.field, v[f.name])

    def make(self, v, keep):
        if v[self.name] is None:
            return None
        obj = self.cls()
        self.fill(obj, v)
        keep.append(obj)
        return obj


class StructArray:
    """a pointer to a host array of structs"""
    def __init__(self, name, cls, rows):
        self.name, self.cls, self.me = name, cls, S(name, "host", True)
        self.rows = [Struct("%s[%d]" % (name, i), cls, fields) for i, fields in enumerate(rows)]

    def leaves(self):
        return [self.me] + [f for r in self.rows for f in r.fields]

    def make(self, v, keep):
        if v[self.name] is None:
            return None
        arr = (self.cls * len(self.rows))()
        for i, r in enumerate(self.rows):
            r.fill(arr[i], v)
        keep.append(arr)
        return arr


class PtrArray:
    """a host array of device pointers"""
    def __init__(self, name, k):
        self.name, self.me = name, S(name, "host", True)
        self.items = [S("%s[%d]" % (name, i), "ptr") for i in range(k)]

    def leaves(self):
        return [self.me] + self.items

    def make(self, v, keep):
        if v[self.name] is None:
            return None
        arr = (ctypes.c_void_p * len(self.items))(*[v[i.name] for i in self.items])
        keep.append(arr)
        return arr


class HostArray:
    """a host array of numbers the library reads"""
    def __init__(self, name, ctype, values):
        self.name, self.ctype, self.values, self.me = name, ctype, values, S(name, "host", True)

    def leaves(self):
        return [self.me]

    def make(self, v, keep):
        if v[self.name] is None:
            return None
        arr = (self.ctype * len(self.values))(*self.values)
        keep.append(arr)
        return arr


def P(name):
    return S(name, "ptr")


def X():
    return [S("nx", "ext", NX), S("ny", "ext", NY), S("nz", "ext", NZ)]


def C(name, base):
    return S(name, "cnt", base)


def F(name, base):
    return S(name, "flt", base)


def FIX(name, base):
    return S(name, "fix", base)


def W(need):
    """workspace and workspace_bytes; need(lib, base values) -> the bytes the library asks for"""
    return [P("workspace"), S("workspace_bytes", "wsb", need)]


def VOL(name="vol"):
    return Struct(name, _lib.Volume, [S("nx", "ext", NX), S("ny", "ext", NY), S("nz", "ext", NZ), F("step", 0.01), P("dist"), P("valid"), P("cell_valid")])


def SET(width=8):
    return [P("data"), C("C", width), C("stride_voxel", width), P("fill")]


def BAND():
    return Struct("band", _lib.Band, [P("slot"), P("cell_band"), C("n_rows", 50)])


STREAM = FIX("stream", None)


class Spec:
    def __init__(self, fn, statuses, args):
        self.fn, self.statuses, self.args = fn, set(statuses), [a for a in args]
        self.leaves = [leaf for a in self.args for leaf in a.leaves()]
        assert len({leaf.name for leaf in self.leaves}) == len(self.leaves), fn
        k = 0
        for leaf in self.leaves:                              # distinct addresses, far apart, each 256-byte aligned
            if leaf.kind == "ptr":
                k += 1
                leaf.base = (1 << 32) + (k << 28)

    def base(self, lib):
        v = {leaf.name: leaf.base for leaf in self.leaves}
        for leaf in self.leaves:
            if leaf.kind == "wsb":
                v[leaf.name] = leaf.base(lib, v)
                assert v[leaf.name] > 0, (self.fn, "the base call asks for no workspace")
        return v

    def rows(self):
        """every row as a tuple of one or two (leaf index, fault index); the single faults first"""
        single = [(i, k) for i, leaf in enumerate(self.leaves) for k in range(N_FAULTS[leaf.kind])]
        return [(f,) for f in single] + [(f, g) for a, f in enumerate(single) for g in single[a + 1:] if g[0] != f[0]]

    def call(self, lib, base, row):
        v = dict(base)
        for i, k in row:
            leaf = self.leaves[i]
            v[leaf.name] = POOL[leaf.kind](base[leaf.name])[k]
        keep = []
        return getattr(lib, self.fn)(*[a.make(v, keep) for a in self.args])

    def describe(self, row):
        return " + ".join("%s#%d" % (self.leaves[i].name, k) for i, k in row)


def _ws(fn, *names):
    return lambda lib, v: getattr(lib, fn)(*[v[n] for n in names])


ALL4 = (INVALID, SHAPE, LAYOUT, WORKSPACE)
NO_WS = (INVALID, SHAPE, LAYOUT)

# fn, the statuses the entry point can return before a launch (read off d3f_api.hip), its arguments in the order of the header
SPECS = [
    Spec("d3f_pcd_to_index", (INVALID, SHAPE),
         [P("pts"), S("n", "n", 1000), HostArray("lower", ctypes.c_double, [0.0, 0.0, 0.0]), F("voxel_size", 0.1), HostArray("voxel_num", ctypes.c_int32, [8, 8, 8]),
          P("out_index"), P("out_voxel"), STREAM]),
    Spec("d3f_vox_idx_iou", ALL4,
         [P("idx1"), C("n1", 100), P("idx2"), C("n2", 100), P("out_counts"), *W(_ws("d3f_vox_iou_workspace_bytes", "n1", "n2")), STREAM]),
    Spec("d3f_voxel_downsample", ALL4,
         [P("pts"), P("colors"), C("n", 1000), F("voxel_size", 0.1), P("out_pts"), P("out_colors"), P("count_out"),
          *W(_ws("d3f_voxel_downsample_workspace_bytes", "n")), STREAM]),
    Spec("d3f_mesh_count", ALL4,
         [P("volume"), P("valid"), *X(), F("iso", 0.0), P("counts_out"), *W(_ws("d3f_mesh_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_mesh_extract", ALL4,
         [P("volume"), P("valid"), *X(), F("iso", 0.0), C("vertex_capacity", 100), C("triangle_capacity", 100), P("keys_out"), P("t_out"), P("triangles_out"),
          P("counts_out"), *W(_ws("d3f_mesh_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_gaussian", ALL4,
         [P("src"), P("dst"), *X(), F("sigma", 1.0), F("truncate", 4.0), *W(_ws("d3f_volume_gaussian_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_sample", NO_WS,
         [VOL(), P("pts"), C("n", 64), StructArray("sets", _lib.VolumeSet, [SET(), SET(12)]), C("n_sets", 2), P("out_dist"), P("out_valid"), PtrArray("out_sets", 2),
          STREAM]),
    Spec("d3f_volume_sample_backward", NO_WS,
         [VOL(), P("pts"), C("n", 64), StructArray("sets", _lib.VolumeSet, [SET()]), C("n_sets", 1), P("grad_dist"), PtrArray("grad_sets", 1), P("grad_pts"), STREAM]),
    Spec("d3f_band_mark", ALL4,
         [VOL(), F("band", 0.05), P("cell_band_out"), P("slot_out"), P("voxels_out"), C("capacity", 100), P("count_out"),
          *W(lambda lib, v: lib.d3f_band_workspace_bytes(v["vol.nx"], v["vol.ny"], v["vol.nz"])), STREAM]),
    Spec("d3f_band_sample", NO_WS,
         [VOL(), BAND(), P("pts"), C("n", 64), StructArray("sets", _lib.VolumeSet, [SET()]), C("n_sets", 1), P("out_dist"), P("out_valid"), P("out_in_band"),
          PtrArray("out_sets", 1), STREAM]),
    Spec("d3f_band_sample_backward", NO_WS,
         [VOL(), BAND(), P("pts"), C("n", 64), StructArray("sets", _lib.VolumeSet, [SET()]), C("n_sets", 1), P("grad_dist"), PtrArray("grad_sets", 1), P("grad_pts"),
          STREAM]),
    Spec("d3f_volume_edt", ALL4,
         [P("site"), *X(), F("step", 0.01), C("max_d2", 0), P("out_d2"), P("out_nearest"), P("out_dist"), *W(_ws("d3f_volume_edt_workspace_bytes", "nx", "ny", "nz")),
          STREAM]),
    Spec("d3f_volume_components", ALL4,
         [P("site"), *X(), S("connectivity", "conn", 26), C("min_voxels", 1), P("out_label"), P("out_count"), P("out_stats"), C("stats_capacity", 3),
          *W(_ws("d3f_volume_components_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_components_linked", ALL4,
         [P("site"), P("links"), *X(), S("connectivity", "conn", 26), C("min_voxels", 1), P("out_label"), P("out_count"), P("out_stats"), C("stats_capacity", 3),
          *W(_ws("d3f_volume_components_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_links", NO_WS,
         [P("site"), P("valid"), P("slot"), *X(), Struct("set", _lib.VolumeSet, SET()), C("rule", _lib.LINK_L2), F("threshold", 0.5), S("connectivity", "conn", 26),
          P("out_links"), STREAM]),
    Spec("d3f_volume_flow", NO_WS,
         [P("site_a"), P("slot_a"), Struct("set_a", _lib.VolumeSet, SET()), P("site_b"), P("slot_b"), Struct("set_b", _lib.VolumeSet, SET()), *X(), C("radius", 2),
          F("max_cost2", 1.0), P("out_target"), P("out_cost"), P("out_axis_cost"), STREAM]),
    Spec("d3f_volume_pool", ALL4,
         [P("label"), *X(), C("K", 3), P("valid"), P("slot"), StructArray("sets", _lib.VolumeSet, [SET(), SET()]), C("n_sets", 2),
          HostArray("modes", ctypes.c_int32, [_lib.POOL_MEAN, _lib.POOL_VOTES]), C("member_capacity", 100), P("out_members"), P("out_count"), P("out_moments"),
          PtrArray("out_rows", 2),
          *W(lambda lib, v: lib.d3f_volume_pool_workspace_bytes(v["nx"], v["ny"], v["nz"], v["K"], v["member_capacity"], 8)), STREAM]),
    Spec("d3f_part_motion", ALL4,
         [P("label"), C("K", 3), *X(), P("keep"), P("target"), P("offset"), P("ref"), C("fits", 2), F("tau2", 1.0), C("min_pairs", 3), C("member_capacity", 100),
          P("out_members"), P("out_pairs"), P("out_pose"), P("out_inliers"), P("out_rmse"), P("out_status"), P("out_fits"), P("out_residual2"), P("out_inlier"),
          P("out_sums"), *W(lambda lib, v: lib.d3f_part_motion_workspace_bytes(v["nx"], v["ny"], v["nz"], v["K"], v["member_capacity"])), STREAM]),
    Spec("d3f_volume_geodesic_init", ALL4,
         [P("free"), *X(), P("seeds"), C("n_seeds", 4), P("out_cost"), *W(_ws("d3f_volume_geodesic_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_geodesic_relax", ALL4,
         [P("free"), P("penalty"), *X(), S("connectivity", "conn", 26), HostArray("w", ctypes.c_int32, [3, 4, 5]), C("max_cost", 1000), C("rounds", 4), P("cost"),
          P("out_pending"), *W(_ws("d3f_volume_geodesic_workspace_bytes", "nx", "ny", "nz")), STREAM]),
    Spec("d3f_volume_geodesic_finish", NO_WS,
         [P("free"), P("penalty"), *X(), S("connectivity", "conn", 26), HostArray("w", ctypes.c_int32, [3, 4, 5]), F("step", 0.01), P("cost"), P("out_next"),
          P("out_dist"), STREAM]),
    Spec("d3f_volume_follow", NO_WS,
         [P("next"), C("n_voxels", NX * NY * NZ), P("starts"), S("n", "n", 100), C("max_steps", 50), P("out_voxels"), P("out_length"), P("out_reached"), STREAM]),
    Spec("d3f_volume_segments", NO_WS,
         [P("free"), P("value"), *X(), P("a"), P("b"), S("n", "n", 100), FIX("flags", 0), P("out_clear"), P("out_last"), P("out_blocked"), P("out_min_value"),
          P("out_min_voxel"), STREAM]),
    Spec("d3f_path_shorten", NO_WS,
         [P("free"), *X(), P("voxels"), P("length"), S("n", "n", 100), C("row_len", 16), C("max_span", 8), FIX("flags", 0), P("out_index"), P("out_voxels"),
          P("out_count"), STREAM]),
    Spec("d3f_volume_peaks", NO_WS,
         [P("slot"), P("mask"), *X(), P("score"), C("M", 100), C("K", 4), C("stride_row", 4), C("radius", 2), F("threshold", 0.5), P("out"), C("out_stride", 4),
          P("out_count"), FIX("workspace", None), FIX("workspace_bytes", 0), STREAM]),
    Spec("d3f_volume_align_accumulate", ALL4,
         [VOL(), BAND(), Struct("set", _lib.VolumeSet, SET()), P("points"), P("weights"), P("targets"), P("dist_targets"), P("pose"), P("centroids"), P("skip"),
          C("I", 2), C("n", 100), F("dist_weight", 1.0), F("feat_weight", 1.0), F("outside", 1.0), P("out"),
          *W(_ws("d3f_volume_align_workspace_bytes", "I", "n")), STREAM]),
    Spec("d3f_volume_raycast", NO_WS,
         [VOL(), P("origins"), P("dirs"), C("n", 100), FIX("camera", None), F("march_step", 0.01), F("t_near", 0.0), F("t_far", 10.0), P("out_t"), P("out_hit"),
          P("out_points"), P("out_samples"), STREAM]),
]
BY_NAME = {s.fn: s for s in SPECS}


def load(path=None):
    """the library of the tree, or the one at path with the same signatures"""
    if path is None:
        return _lib.load()
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def ranges(indices):
    """sorted indices -> [[first, end), ...]"""
    out = []
    for i in indices:
        if out and out[-1][1] == i:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1])
    return out


def unranges(rs):
    return [i for a, b in rs for i in range(a, b)]


def replay(lib, spec, kept):
    base, rows = spec.base(lib), spec.rows()
    return [spec.call(lib, base, rows[i]) for i in kept]


def record(lib):
    """status of every row; the rows the library does not reject on the host (D3F_OK, D3F_ERR_HIP) leave the record by index"""
    import torch
    assert torch.cuda.device_count() == 0, "the made-up addresses are harmless only where nothing can be launched"
    calls = {}
    for spec in SPECS:
        base, rows = spec.base(lib), spec.rows()
        assert spec.call(lib, base, ()) in (_lib.OK, HIP), (spec.fn, "the base call is rejected: %s" % lib.d3f_last_error().decode())
        status = [spec.call(lib, base, row) for row in rows]
        kept = [i for i, s in enumerate(status) if s in VALIDATION]
        assert set(status) <= set(VALIDATION) | {_lib.OK, HIP}, spec.fn
        calls[spec.fn] = {"rows": len(rows), "kept": ranges(kept), "status": [status[i] for i in kept]}
    return calls


def write(calls, parent, path=RECORD):
    with open(path, "w") as fh:
        fh.write('{"recorded_at": "%s",\n "calls": {\n' % parent)
        fh.write(",\n".join('  "%s": %s' % (fn, json.dumps(c, separators=(",", ":"))) for fn, c in calls.items()))
        fh.write("\n }}\n")


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "record":
        sys.exit("usage: python tests/api_calls.py record <commit the library was built from> [path of that library]")
    write(record(load(sys.argv[3] if len(sys.argv) > 3 else None)), sys.argv[2])
    print("wrote", RECORD, os.path.getsize(RECORD), "bytes")
