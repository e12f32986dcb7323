"""CPU: the generated marching-cubes case table (scripts/gen_mc_table.py -> csrc/mc_table.inc) is reproducible, closed inside every cell and consistent
across every shared face."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_mc_table as G      # noqa: E402


def _face_of_edge_pair(a, b):
    """The cube faces (axis, side) that contain both edges a and b."""
    out = []
    for axis, side, cyc in G.FACES:
        on = lambda e: all(G.corner_offset(c)[axis] == side for c in G.edge_corners(e))
        if on(a) and on(b):
            out.append((axis, side))
    return out


def test_regenerating_reproduces_the_committed_table():
    assert open(G.OUT).read() == G.render()


def test_empty_configurations_and_cell_maximum():
    table, mx = G.build_table()
    assert table[0] == [] and table[255] == []
    assert all(len(t) >= 1 for t in table[1:255])
    assert mx == max(len(t) for t in table) and ("#define MC_MAX_TRIS %d\n" % mx) in open(G.OUT).read()


def test_directed_edges_cancel_except_along_cube_faces():
    """Inside a cell the triangles of a configuration form closed patches: every directed edge that does not lie in a cube face is matched by its reverse,
    and the edges left over are exactly the face segments, each once."""
    table, _ = G.build_table()
    for cfg in range(256):
        d = {}
        for a, b, c in table[cfg]:
            for u, w in ((a, b), (b, c), (c, a)):
                d[(u, w)] = d.get((u, w), 0) + 1
        left = []
        for (u, w), n in d.items():
            assert n == 1, (cfg, u, w)
            if (w, u) not in d:
                left.append((u, w))
        assert sorted(left) == sorted(G.case_segments(cfg)), cfg
        for u, w in left:
            assert _face_of_edge_pair(u, w), (cfg, u, w)
        # every vertex of the configuration is a crossed edge, and every crossed edge is used
        crossed = {e for e in range(12) if ((cfg >> G.edge_corners(e)[0]) ^ (cfg >> G.edge_corners(e)[1])) & 1}
        assert {e for t in table[cfg] for e in t} == crossed, cfg


def test_cells_sharing_a_face_emit_the_same_segments_reversed():
    """For every classification of a face's four corners and every axis: the segments the lower cell draws on its upper face are those the upper cell draws on
    its lower face, reversed (both cells name the shared grid edges by the same in-face position)."""
    for axis in range(3):
        lo = next(f for f in G.FACES if f[0] == axis and f[1] == 0); hi = next(f for f in G.FACES if f[0] == axis and f[1] == 1)

        def in_face(e, side):               # a face edge -> the pair of in-face corner positions (the two other coordinates of its end points)
            return tuple(sorted(tuple(o for k, o in enumerate(G.corner_offset(c)) if k != axis) for c in G.edge_corners(e)))
        for cls in range(16):
            pos = [(0, 0), (1, 0), (1, 1), (0, 1)]
            inside_at = {p: (cls >> i) & 1 for i, p in enumerate(pos)}
            key = lambda c: tuple(o for k, o in enumerate(G.corner_offset(c)) if k != axis)
            seg_hi = G.face_segments(hi[2], [inside_at[key(c)] for c in hi[2]])       # the lower cell's upper face
            seg_lo = G.face_segments(lo[2], [inside_at[key(c)] for c in lo[2]])       # the upper cell's lower face
            a = sorted((in_face(u, 1), in_face(w, 1)) for u, w in seg_hi)
            b = sorted((in_face(w, 0), in_face(u, 0)) for u, w in seg_lo)
            assert a == b, (axis, cls)
            if cls in (0b0101, 0b1010):
                assert len(seg_hi) == 2                                             # the ambiguous face: two segments, inside corners separated
                for u, w in seg_hi:
                    shared = set(G.edge_corners(u)) & set(G.edge_corners(w))
                    assert len(shared) == 1 and inside_at[key(shared.pop())] == 1


def test_single_corner_normals_point_away_from_the_inside_corner():
    table, _ = G.build_table()
    mid = lambda e: (np.array(G.corner_offset(G.edge_corners(e)[0]), float) + np.array(G.corner_offset(G.edge_corners(e)[1]), float)) / 2
    for c in range(8):
        (a, b, d), = table[1 << c]
        n = np.cross(mid(b) - mid(a), mid(d) - mid(a))
        assert np.dot(n, (mid(a) + mid(b) + mid(d)) / 3 - np.array(G.corner_offset(c), float)) > 0
        (a, b, d), = table[255 ^ (1 << c)]
        n = np.cross(mid(b) - mid(a), mid(d) - mid(a))
        assert np.dot(n, (mid(a) + mid(b) + mid(d)) / 3 - np.array(G.corner_offset(c), float)) < 0


def test_no_fan_diagonal_lies_in_a_cube_face():
    """A triangle edge inside a cube face that is not one of the face's segments would be drawn by the neighbouring cell too (an edge with four triangles):
    every triangle edge is either a face segment or runs through the cell's interior."""
    table, _ = G.build_table()
    for cfg in range(256):
        segs = set(G.case_segments(cfg))
        for a, b, c in table[cfg]:
            for u, w in ((a, b), (b, c), (c, a)):
                assert (u, w) in segs or not _face_of_edge_pair(u, w), (cfg, u, w)
