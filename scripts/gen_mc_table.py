"""Generates mirres-restir_nerf_mesh_amd/csrc/mc_table.inc, the 256-entry marching-cubes case table of csrc/mcubes.hip, from the cube's faces (no table is typed in).

    python scripts/gen_mc_table.py            # rewrites the file
    python scripts/gen_mc_table.py --check    # exit status 1 if the committed file differs

Conventions (shared with csrc/mcubes.hip and tests/stage0_refs.py)
  corner c of a cell = lower grid point + (c & 1, (c >> 1) & 1, (c >> 2) & 1); bit c of a configuration is set when the corner is INSIDE (value >= iso);
  edge e = 4 * axis + k runs along `axis` from the corner whose offsets along the two other axes (in ascending axis order) are (k & 1, k >> 1).
Construction, per configuration
  every cube face, looked at from outside the cube, contributes directed segments between its crossed edges with the inside corners on the RIGHT of the
  direction of travel (a surface patch whose normal points from inside to outside is then bounded counter-clockwise, seen from the tip of its normal);
    one inside corner    : one segment that cuts it off;          three inside corners : one segment that cuts the outside corner off;
    two adjacent corners : one segment between the two other edges;
    two DIAGONAL corners : the fixed rule SEPARATE — two segments, each cutting one inside corner off (the inside corners are never joined across a face).
  The rule reads the face's four classifications only, so the two cells that share a face draw the same segments on it, in opposite directions (their outward
  normals are opposite): the surface has no cracks by construction.  Every crossed edge lies in two faces, once as the end and once as the start of a segment:
  the segments chain into closed loops, ordered by their lowest-numbered edge, and each is fan-triangulated, (l0, l_i, l_i+1), from its lowest-numbered vertex
  none of whose fan diagonals lies in a cube face.  A diagonal in a face (between two crossed edges of an ambiguous face that no segment joins) would be drawn
  by the neighbouring cell as well: four triangles on one edge, two of them flat in the face.  Every loop of the 256 configurations has such a vertex (checked
  here and in tests/test_mc_table.py); for 18 loops it is not the lowest-numbered one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "mirres-restir_nerf_mesh_amd", "csrc", "mc_table.inc")

OTHER = ((1, 2), (0, 2), (0, 1))          # the two other axes of an edge's axis, ascending


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_index(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def edge_corners(e):
    """(lower corner, upper corner) of edge e."""
    axis, k = divmod(e, 4)
    off = [0, 0, 0]
    off[OTHER[axis][0]] = k & 1; off[OTHER[axis][1]] = k >> 1
    lo = corner_index(off); off[axis] = 1
    return lo, corner_index(off)


def edge_of(c0, c1):
    for e in range(12):
        if set(edge_corners(e)) == {c0, c1}:
            return e
    raise ValueError((c0, c1))


def faces():
    """Six faces: (axis, side, the four corners counter-clockwise seen from outside the cube)."""
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3          # e_u x e_v = e_axis
        for side in (0, 1):
            cyc = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):      # counter-clockwise about +axis
                off = [0, 0, 0]; off[axis] = side; off[u] = du; off[v] = dv
                cyc.append(corner_index(off))
            if side == 0:                                # outward normal is -axis: the same cycle is clockwise from outside
                cyc.reverse()
            out.append((axis, side, tuple(cyc)))
    return out


FACES = faces()


def face_segments(cyc, inside):
    """Directed segments (edge from, edge to) of one face; cyc: its corners counter-clockwise from outside, inside: their classification."""
    n = sum(inside)
    segs = []

    def cut(i, flip):
        # the segment around corner i of the cycle.  Counter-clockwise cycle, corner on the right of the direction of travel: from the edge towards the
        # PREVIOUS corner to the edge towards the NEXT one (travelling counter-clockwise around the corner); flipped when the corner is the outside one.
        a = edge_of(cyc[i], cyc[(i - 1) % 4]); b = edge_of(cyc[i], cyc[(i + 1) % 4])
        segs.append((b, a) if flip else (a, b))

    if n == 1:
        cut(inside.index(1), False)
    elif n == 3:
        cut(inside.index(0), True)
    elif n == 2:
        if inside[0] == inside[2]:                       # diagonal: SEPARATE
            for i in range(4):
                if inside[i]:
                    cut(i, False)
        else:
            i = next(i for i in range(4) if inside[i] and inside[(i + 1) % 4])      # inside corners i, i + 1; outside i + 2, i + 3
            a = edge_of(cyc[(i + 3) % 4], cyc[i]); b = edge_of(cyc[(i + 1) % 4], cyc[(i + 2) % 4])
            segs.append((a, b))                          # travelling with the cycle's direction past the inside pair keeps it on the right
    return segs


def case_segments(cfg):
    segs = []
    for axis, side, cyc in FACES:
        segs += face_segments(cyc, [(cfg >> c) & 1 for c in cyc])
    return segs


def case_loops(cfg):
    nxt = {}
    for a, b in case_segments(cfg):
        assert a not in nxt, (cfg, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), cfg
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e); loop.append(e); e = nxt[e]
        assert e == start, cfg
        loops.append(loop)
    return loops


def on_one_face(a, b):
    """Do edges a and b lie in one cube face?"""
    return any(all(corner_offset(c)[axis] == side for e in (a, b) for c in edge_corners(e)) for axis, side, _ in FACES)


def fan_start(loop):
    """The loop rotated to its lowest-numbered vertex whose fan has no diagonal inside a cube face."""
    n = len(loop)
    for apex in sorted(loop):
        s = loop.index(apex)
        r = loop[s:] + loop[:s]
        if not any(on_one_face(r[0], r[i]) for i in range(2, n - 1)):
            return r
    raise AssertionError("no fan without an in-face diagonal: %r" % (loop,))


def case_triangles(cfg):
    tris = []
    for loop in case_loops(cfg):
        assert len(loop) >= 3, (cfg, loop)
        loop = fan_start(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def build_table():
    """-> (list of 256 triangle lists (edge triples), the per-cell maximum)."""
    table = [case_triangles(c) for c in range(256)]
    return table, max(len(t) for t in table)


def render():
    table, mx = build_table()
    lines = ["// mc_table.inc - generated by scripts/gen_mc_table.py; do not edit.  Corner, edge and winding conventions: see that script.",
             "#define MC_MAX_TRIS %d" % mx,
             "static __device__ const signed char MC_NTRI[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("static __device__ const signed char MC_TRI[256][%d] = {" % (3 * mx))
    for c in range(256):
        flat = [e for t in table[c] for e in t]
        flat += [-1] * (3 * mx - len(flat))
        lines.append("    {" + ", ".join("%2d" % e for e in flat) + "},   // %3d" % c)
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s (%d triangles at most per cell)" % (OUT, build_table()[1]))
