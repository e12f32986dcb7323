"""numpy restatements for the stage-0 tests (csrc/mcubes.hip, stage0.py): marching cubes from the same generated case table and the same fp32 expressions,
the Morton bit trick, one-ring selection dilatation, edge-connected components (union-find), mesh compaction, and the small test meshes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "scripts") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_mc_table as G      # noqa: E402

FLT_MAX = np.finfo(np.float32).max
_TABLE, MAX_TRIS = G.build_table()
NTRI = np.array([len(t) for t in _TABLE], np.int64)
TRI = np.full((256, MAX_TRIS, 3), -1, np.int64)
for _c, _t in enumerate(_TABLE):
    for _j, _tri in enumerate(_t):
        TRI[_c, _j] = _tri


def marching_cubes(vol, iso):
    """(vertices f32 [V, 3] index space, triangles i32 [T, 3]): one vertex per crossed grid edge numbered in (grid point, axis) order, grid points in the memory
    order of vol[x][y][z]; triangles in (cell, table) order; every fp32 step a single numpy float32 operation."""
    v = np.nan_to_num(np.asarray(vol, np.float32), nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(np.float32)
    iso = np.float32(iso)
    nx, ny, nz = v.shape
    inside = v >= iso
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    px, py, pz, ax = np.nonzero(cross)                      # row-major: (grid point, axis) order
    p = np.stack([px, py, pz], 1)
    q = p.copy(); q[np.arange(len(ax)), ax] += 1
    va = v[p[:, 0], p[:, 1], p[:, 2]]; vb = v[q[:, 0], q[:, 1], q[:, 2]]
    with np.errstate(all="ignore"):
        t = (iso - va) / (vb - va)
    t = np.fmin(np.fmax(t, np.float32(0)), np.float32(1)).astype(np.float32)
    verts = p.astype(np.float32)
    verts[np.arange(len(ax)), ax] = p[np.arange(len(ax)), ax].astype(np.float32) + t
    cfg = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = G.corner_offset(c)
        cfg |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    cx, cy, cz = np.nonzero(NTRI[cfg] > 0)
    ccfg = cfg[cx, cy, cz]
    g = (cx * ny + cy) * nz + cz
    rows = []
    for j in range(MAX_TRIS):
        sel = NTRI[ccfg] > j
        if not sel.any():
            break
        tri = np.empty((int(sel.sum()), 3), np.int64)
        for k in range(3):
            e = TRI[ccfg[sel], j, k]
            axis, kk = e // 4, e % 4
            off = np.zeros((len(e), 3), np.int64)
            for a in range(3):
                m = axis == a
                off[m, G.OTHER[a][0]] = kk[m] & 1; off[m, G.OTHER[a][1]] = kk[m] >> 1
            tri[:, k] = vid[cx[sel] + off[:, 0], cy[sel] + off[:, 1], cz[sel] + off[:, 2], axis]
        rows.append(np.concatenate([g[sel][:, None], np.full((len(tri), 1), j), tri], 1))
    if not rows:
        return verts.astype(np.float32).reshape(-1, 3), np.zeros((0, 3), np.int32)
    rows = np.concatenate(rows, 0)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    return verts.astype(np.float32).reshape(-1, 3), rows[:, 2:].astype(np.int32)


def morton_invert(i):
    """__morton3D_invert of raymarching.cu:73-81 for a 30-bit index, restated: every third bit compacted."""
    x = np.asarray(i, np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xC30C30C3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0F00F00F)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xFF0000FF)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000FFFF)
    return x


def unpack_morton(grid, S):
    """sigmas[tuple(morton3D_invert(arange).T)] = grid (nerf/renderer.py:513-515)."""
    i = np.arange(S ** 3, dtype=np.uint32)
    vol = np.zeros((S, S, S), np.float32)
    vol[morton_invert(i), morton_invert(i >> np.uint32(1)), morton_invert(i >> np.uint32(2))] = np.asarray(grid, np.float32)
    return vol


def dilate(tris, n_vertices, selected, rings):
    """MeshLab's loose dilatation: a vertex is selected if a selected face uses it, then a face if any of its vertices is; one ring per pass."""
    tris = np.asarray(tris, np.int64); sel = np.asarray(selected).astype(bool).copy()
    for _ in range(rings):
        vs = np.zeros(n_vertices, bool)
        vs[tris[sel].reshape(-1)] = True
        sel = vs[tris].any(axis=1)
    return sel


def edge_pairs(tris):
    """Pairs of faces that share an undirected edge (consecutive faces of every edge's sorted face list)."""
    tris = np.asarray(tris, np.int64)
    by_edge = {}
    for f, (a, b, c) in enumerate(tris):
        for u, w in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(u, w), max(u, w)), []).append(f)
    return [(fs[i], fs[i + 1]) for fs in by_edge.values() for i in range(len(fs) - 1)]


def components(tris):
    """Label = the smallest face index of the face's edge-connected component (union-find, the smaller root wins)."""
    T = len(tris)
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for a, b in edge_pairs(tris):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(f) for f in range(T)], np.int32)


def compact(verts, tris, keep):
    verts = np.asarray(verts, np.float32); tris = np.asarray(tris, np.int64); keep = np.asarray(keep).astype(bool)
    t = tris[keep]
    used = np.zeros(len(verts), bool); used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[t].astype(np.int32)


def mesh_edges_ok(tris):
    """Every undirected edge used by exactly two triangles, in opposite directions."""
    tris = np.asarray(tris, np.int64)
    d = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], 0)
    fwd = {}
    for a, b in d:
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    return all(n == 1 and fwd.get((b, a), 0) == 1 for (a, b), n in fwd.items())


def signed_volume(verts, tris):
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def euler_characteristic(n_vertices, tris):
    tris = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], 0), axis=1)
    return n_vertices - len(np.unique(e, axis=0)) + len(tris)


# ------------------------------------------------------------------------------------------------ test meshes
def icosphere(subdiv=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """Outward-wound icosphere: 20 * 4^subdiv faces."""
    ph = (1 + 5 ** 0.5) / 2
    v = [(-1, ph, 0), (1, ph, 0), (-1, -ph, 0), (1, -ph, 0), (0, -1, ph), (0, 1, ph), (0, -1, -ph), (0, 1, -ph), (ph, 0, -1), (ph, 0, 1), (-ph, 0, -1), (-ph, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid = {}; nf = []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]; v.append(x / np.linalg.norm(x)); mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.array(centre)).astype(np.float32), np.array(f, np.int32)


def cube(half=0.1, centre=(0.0, 0.0, 0.0)):
    """Closed cube, 8 vertices, 12 outward faces."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * half + np.array(centre)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v.astype(np.float32), np.array(f, np.int32)


def join(parts):
    vs, ts, n = [], [], 0
    for v, t in parts:
        vs.append(np.asarray(v, np.float32)); ts.append(np.asarray(t, np.int32) + n); n += len(v)
    return np.concatenate(vs, 0), np.concatenate(ts, 0)


def strip(n_faces):
    """A triangle strip: face f = (f, f + 1, f + 2) with alternating winding; every face shares an edge with the next: one component, the longest chain."""
    v = np.array([[0.5 * i, float(i & 1), 0.0] for i in range(n_faces + 2)], np.float32)
    t = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n_faces)], np.int32)
    return v, t


def orbit_cameras(n=6, radius=3.0, H=64, W=64, fov_deg=50.0):
    """n cam2world poses looking at the origin (camera looks down -z, y up) from +-x, +-y, +-z first, and the (fx, fy, cx, cy) they share."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)][:n]
    poses = []
    for d in dirs:
        z = np.array(d, np.float64)
        up = np.array((0, 0, 1.0)) if abs(z[2]) < 0.5 else np.array((0, 1.0, 0))
        x = np.cross(up, z); x /= np.linalg.norm(x); y = np.cross(z, x)
        p = np.eye(4); p[:3, 0] = x; p[:3, 1] = y; p[:3, 2] = z; p[:3, 3] = z * radius
        poses.append(p.astype(np.float32))
    f = 0.5 * W / np.tan(0.5 * np.radians(fov_deg))
    return poses, (f, f, W * 0.5, H * 0.5)
