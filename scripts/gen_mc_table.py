"""Derives the marching-cubes case table of d3fields_amd/csrc/mc_table.h by tracing polygon loops -- nothing is typed in.

    python scripts/gen_mc_table.py            # prints the header
    python scripts/gen_mc_table.py --write    # rewrites d3fields_amd/csrc/mc_table.h

Conventions (the kernels of mesh_kernels.hip and the float64 reference of tests/mesh_ref.py use the same):

* corner c of a cell has the offsets (dx, dy, dz) = (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest corner;
  bit c of the case is set when that corner is INSIDE, i.e. value < iso.
* edge e = 4 * axis + j runs along `axis` (0 = x, 1 = y, 2 = z); the other two axes u < w carry the offsets
  (j & 1, j >> 1) of its lower endpoint.  An edge is crossed when its two corners differ.
* on every face the crossed edges (0, 2 or 4 of them) are joined into segments.  Four crossed edges (the ambiguous face:
  the inside corners sit on a diagonal) are resolved by ONE rule that sees the face's four corner bits only: every inside
  corner is cut off on its own (its two face edges are joined).  Two cells that share a face therefore draw the same
  segments on it, and the mesh is closed in every case.
* a segment is directed so that the loop runs counter-clockwise seen from the side where value > iso: with n the face's
  outward normal, d the segment's direction and m the direction from the inside to the outside endpoint of the crossed
  edge the segment starts on, (d x m) . n > 0.  The neighbour across the face has -n, hence the reversed segment.
* every crossed edge has one segment leaving and one arriving; following them closes the loops.  A loop is rotated to
  start at its smallest edge id and fan-triangulated from there; the loops of a case are ordered by that smallest id.
"""
import os
import sys

AXES = ((1, 2), (0, 2), (0, 1))          # the other two axes (u, w), u < w, of an edge along axis 0 / 1 / 2


def corner_offsets(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def edge_corners(e):
    """(lower corner id, upper corner id) of edge e."""
    axis, j = e >> 2, e & 3
    u, w = AXES[axis]
    lo = [0, 0, 0]
    lo[u], lo[w] = j & 1, j >> 1
    hi = list(lo)
    hi[axis] = 1
    return corner_id(lo), corner_id(hi)


def edge_between(ca, cb):
    for e in range(12):
        if set(edge_corners(e)) == {ca, cb}:
            return e
    raise ValueError((ca, cb))


def faces():
    """Six faces as (axis, side, corner cycle): the four corners in an order that walks round the face."""
    out = []
    for axis in range(3):
        u, w = AXES[axis]
        for side in (0, 1):
            cyc = []
            for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[w] = side, du, dw
                cyc.append(corner_id(off))
            out.append((axis, side, tuple(cyc)))
    return out


FACES = faces()


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _mid2(e):
    """Twice the midpoint of edge e (integers)."""
    a, b = edge_corners(e)
    return tuple(x + y for x, y in zip(corner_offsets(a), corner_offsets(b)))


def face_segments(face, inside):
    """Directed segments (edge from, edge to) a face draws, given inside[c] of its own four corners only."""
    axis, side, cyc = face
    normal = [0, 0, 0]
    normal[axis] = 1 if side else -1
    fedges = [edge_between(cyc[k], cyc[(k + 1) % 4]) for k in range(4)]          # face edge k joins cycle corners k, k+1
    crossed = [k for k in range(4) if inside[cyc[k]] != inside[cyc[(k + 1) % 4]]]
    if not crossed:
        return []
    if len(crossed) == 2:
        pairs = [(fedges[crossed[0]], fedges[crossed[1]])]
    else:                                                                      # ambiguous: cut every inside corner off on its own
        pairs = [(fedges[(k - 1) % 4], fedges[k]) for k in range(4) if inside[cyc[k]]]
    out = []
    for ea, eb in pairs:
        d = _sub(_mid2(eb), _mid2(ea))
        ca, cb = edge_corners(ea)
        cin, cout = (ca, cb) if inside[ca] else (cb, ca)
        m = _sub(corner_offsets(cout), corner_offsets(cin))
        s = _dot(_cross(d, m), normal)
        assert s != 0
        out.append((ea, eb) if s > 0 else (eb, ea))
    return out


def case_segments(case):
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for f in FACES:
        segs += face_segments(f, inside)
    return segs


def case_loops(case):
    """Closed loops of edge ids, each starting at its smallest id; loops ordered by that id."""
    segs = case_segments(case)
    nxt = {}
    for a, b in segs:
        assert a not in nxt, "edge %d leaves twice in case %d" % (a, case)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), "case %d: segments do not close" % case
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def case_edge_mask(case):
    mask = 0
    for e in range(12):
        a, b = edge_corners(e)
        if ((case >> a) & 1) != ((case >> b) & 1):
            mask |= 1 << e
    return mask


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for k in range(1, len(loop) - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))
    return tris


def build_table():
    """[(edge mask, [triangles])] for the 256 cases."""
    return [(case_edge_mask(c), case_triangles(c)) for c in range(256)]


def render_header():
    table = build_table()
    max_tris = max(len(t) for _, t in table)
    lines = [
        "// mc_table.h -- marching-cubes case table.  GENERATED by scripts/gen_mc_table.py (tests/test_mesh_table.py regenerates it and",
        "// compares byte for byte): do not edit.",
        "//",
        "// corner c = lowest corner + (c & 1, (c >> 1) & 1, (c >> 2) & 1); case bit c is set when value < iso at that corner (inside).",
        "// edge e = 4 * axis + j runs along axis (0 x, 1 y, 2 z); its lower endpoint is offset by (j & 1, j >> 1) along the other two",
        "// axes in ascending order.  Built by tracing loops: on each face the crossed edges are joined pairwise, a face with four",
        "// crossed edges cuts every inside corner off on its own (a rule of that face's four corner bits alone, so neighbours agree",
        "// and the mesh is closed in every case); each loop is fan-triangulated from its smallest edge id.",
        "// Winding: a triangle's normal (right-hand rule over its three vertices) points to the side where value > iso.",
        "// Degenerate triangles (a value equal to iso gives t = 0 on several edges) are emitted as the table says, not filtered.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#define D3F_MC_MAX_TRIANGLES %d" % max_tris,
        "#ifndef D3F_MC_TABLE_ATTR",
        "#define D3F_MC_TABLE_ATTR static const      /* mesh_kernels.hip: static __device__ const */",
        "#endif",
        "",
        "// crossed edges of a case, bit e",
        "D3F_MC_TABLE_ATTR uint16_t kMcEdgeMask[256] = {",
    ]
    for r in range(0, 256, 8):
        lines.append("    " + ", ".join("0x%03x" % table[c][0] for c in range(r, r + 8)) + ",")
    lines += ["};", "", "// triangles of a case", "D3F_MC_TABLE_ATTR uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join("%d" % len(table[c][1]) for c in range(r, r + 16)) + ",")
    lines += ["};", "", "// edge triples of a case, 255 = unused", "D3F_MC_TABLE_ATTR uint8_t kMcTriEdges[256][3 * D3F_MC_MAX_TRIANGLES] = {"]
    for c in range(256):
        flat = [e for t in table[c][1] for e in t]
        flat += [255] * (3 * max_tris - len(flat))
        lines.append("    {" + ", ".join("%d" % e for e in flat) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "d3fields_amd", "csrc", "mc_table.h")

if __name__ == "__main__":
    text = render_header()
    if "--write" in sys.argv:
        with open(HEADER_PATH, "w") as fh:
            fh.write(text)
        print(HEADER_PATH)
    else:
        sys.stdout.write(text)
