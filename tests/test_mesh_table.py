"""CPU: the marching-cubes case table (d3fields_amd/csrc/mc_table.h) is the generator's output, and every one of the 256 cases
is a closed, consistently oriented set of polygon loops whose face segments depend on the face's own corners alone."""
import itertools
import os
import re

import numpy as np

import mesh_ref
from conftest import ROOT

gen = mesh_ref.gen_mc_table
TABLE = mesh_ref.TABLE
HEADER = os.path.join(ROOT, "d3fields_amd", "csrc", "mc_table.h")


def test_committed_header_is_the_generators_output():
    with open(HEADER, "rb") as fh:
        assert fh.read() == gen.render_header().encode()


def test_header_numbers_parse_back_to_the_table():
    src = open(HEADER).read()
    max_tris = int(re.search(r"#define D3F_MC_MAX_TRIANGLES (\d+)", src).group(1))
    assert max_tris == max(len(t) for _, t in TABLE) == 5

    def numbers(name):
        body = re.search(name + r"\[256\][^=]*= \{(.*?)\};", src, flags=re.S).group(1)
        return [int(x, 0) for x in re.findall(r"0x[0-9a-f]+|\d+", body)]

    assert numbers("kMcEdgeMask") == [m for m, _ in TABLE]
    assert numbers("kMcTriCount") == [len(t) for _, t in TABLE]
    edges = np.asarray(numbers("kMcTriEdges")).reshape(256, 3 * max_tris)
    for c, (_, tris) in enumerate(TABLE):
        flat = [e for t in tris for e in t]
        assert edges[c].tolist() == flat + [255] * (3 * max_tris - len(flat))


def test_every_case_uses_exactly_its_crossed_edges_in_closed_oriented_loops():
    assert TABLE[0] == (0, []) and TABLE[255] == (0, [])
    for case in range(256):
        mask, tris = TABLE[case]
        crossed = {e for e in range(12) if (mask >> e) & 1}
        # crossed <=> the edge's two corners differ
        for e in range(12):
            a, b = gen.edge_corners(e)
            assert (e in crossed) == (((case >> a) & 1) != ((case >> b) & 1))
        assert {e for t in tris for e in t} == crossed, case
        assert len(tris) <= 5
        loops = gen.case_loops(case)
        # every crossed edge lies on exactly one loop
        on_loops = [e for l in loops for e in l]
        assert sorted(on_loops) == sorted(crossed), case
        assert all(l[0] == min(l) and len(l) >= 3 for l in loops)
        assert [l[0] for l in loops] == sorted(l[0] for l in loops)
        assert sum(len(l) - 2 for l in loops) == len(tris)
        # directed triangle edges: a loop segment occurs once (and never reversed), a fan diagonal twice with opposite direction
        segments = {(l[k], l[(k + 1) % len(l)]) for l in loops for k in range(len(l))}
        assert segments == set(gen.case_segments(case))
        directed = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
        assert len(set(directed)) == len(directed), case
        for d in directed:
            if d in segments:
                assert (d[1], d[0]) not in directed, case
            else:
                assert (d[1], d[0]) in directed and (d[1], d[0]) not in segments, case
        assert segments <= set(directed)


def test_face_segments_depend_on_the_face_alone_and_neighbours_agree():
    by_axis = {}
    for axis, side, cyc in gen.FACES:
        by_axis.setdefault(axis, {})[side] = (axis, side, cyc)
    seen_patterns = 0
    for axis in range(3):
        lo_face, hi_face = by_axis[axis][0], by_axis[axis][1]
        for bits in itertools.product((0, 1), repeat=4):
            seen_patterns += 2
            # the same four corner values on the upper face of one cell and on the lower face of its neighbour
            results = {}
            for face in (lo_face, hi_face):
                segs_for_rest = set()
                for rest in itertools.product((0, 1), repeat=4):          # whatever the other four corners are ...
                    inside = [0] * 8
                    for k, c in enumerate(face[2]):
                        inside[c] = bits[k]
                    others = [c for c in range(8) if c not in face[2]]
                    for k, c in enumerate(others):
                        inside[c] = rest[k]
                    case = sum(b << c for c, b in enumerate(inside))
                    face_edges = {gen.edge_between(face[2][k], face[2][(k + 1) % 4]) for k in range(4)}
                    # ... the segments the CASE draws on this face (both ends on the face, taken from the traced loops) ...
                    drawn = frozenset(s for s in gen.case_segments(case) if s[0] in face_edges and s[1] in face_edges)
                    assert drawn == frozenset(gen.face_segments(face, inside))
                    segs_for_rest.add(drawn)
                assert len(segs_for_rest) == 1                            # ... are a function of the face's four bits
                results[face[1]] = next(iter(segs_for_rest))
            # the neighbour across the face: its lower face carries the same corners; edge ids differ by the face offset, so
            # compare as pairs of (corner offsets inside the face)

            def as_geometry(face, segs):
                out = set()
                for a, b in segs:
                    ka = tuple(sorted(tuple(o for i, o in enumerate(gen.corner_offsets(c)) if i != face[0]) for c in gen.edge_corners(a)))
                    kb = tuple(sorted(tuple(o for i, o in enumerate(gen.corner_offsets(c)) if i != face[0]) for c in gen.edge_corners(b)))
                    out.add((ka, kb))
                return out

            up = as_geometry(hi_face, results[1])
            down = as_geometry(lo_face, results[0])
            assert up == {(b, a) for a, b in down}, (axis, bits)
    assert seen_patterns == 16 * 6


def test_winding_points_to_the_outside():
    """A single inside corner: the triangle's normal points away from it; its complement: towards the single outside corner."""
    for c in range(8):
        for case, sign in ((1 << c, 1.0), (255 ^ (1 << c), -1.0)):
            (tri,) = TABLE[case][1]
            p = [np.asarray(gen._mid2(e)) / 2.0 for e in tri]
            normal = np.cross(p[1] - p[0], p[2] - p[0])
            away = np.mean(p, axis=0) - np.asarray(gen.corner_offsets(c), dtype=np.float64)
            assert sign * float(normal @ away) > 0
