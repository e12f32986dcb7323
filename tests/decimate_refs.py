"""Restatements for the decimation tests (csrc/decimate.hip, stage0.decimate_mesh), in float64 Python / numpy with the device's formulas in the device's order:
the per-vertex quadrics (gathered in CSR order), placement / cost / every validity reason per edge, the selection rule as a pure function, a sequential greedy
decimator with the same quadrics and rules (the quality yardstick), point-to-mesh distances, and the test meshes.  Constants as in decimate.hip."""
import heapq
import math

import numpy as np

BOUNDARY_WEIGHT = 1.0          # a boundary edge's constraint weighs this times its squared length
DET_REL = 1e-9                 # singular when |det| <= DET_REL * max|entry|^3
FLIP_COS = 0.2                 # a moved face keeps its normal within acos(0.2)
F_MULT, F_LINK, F_BOUNDARY, F_FLIP, F_FINITE = 1, 2, 4, 8, 16
KEY_NONE = 0x7FFFFFFFFFFFFFFF
FLIP_TOL, DET_TOL, TIE_TOL = 1e-9, 1e-6, 1e-12      # how near its threshold a deciding quantity must lie for the edge to be left out of the flag comparison


def f32(x):
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _add_plane(q, u, d, w):
    q[0] += w * (u[0] * u[0]); q[1] += w * (u[0] * u[1]); q[2] += w * (u[0] * u[2]); q[3] += w * (u[0] * d)
    q[4] += w * (u[1] * u[1]); q[5] += w * (u[1] * u[2]); q[6] += w * (u[1] * d)
    q[7] += w * (u[2] * u[2]); q[8] += w * (u[2] * d)
    q[9] += w * (d * d)


def q_eval(q, x, y, z):
    r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
    r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6]
    r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8]
    r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9]
    return ((x * r0 + y * r1) + z * r2) + r3


def topology(tris, V):
    """The round's sorts: distinct edge keys ascending, multiplicity, the edge of corner 3 f + k = (v_k, v_k+1), the vertex -> corner CSR (stable)."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    a = t.reshape(-1); b = t[:, [1, 2, 0]].reshape(-1)
    ekeys, corner_edge, emult = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_inverse=True, return_counts=True)
    vcorner = np.argsort(a, kind="stable")
    vstart = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=V))]).astype(np.int64)
    vflag = np.zeros(V, np.int64)
    ea, eb = ekeys >> 32, ekeys & 0xFFFFFFFF
    for bit, m in ((1, emult == 1), (2, emult > 2)):
        vflag[ea[m]] |= bit; vflag[eb[m]] |= bit
    return dict(ekeys=ekeys, ea=ea, eb=eb, emult=emult, corner_edge=corner_edge.reshape(-1), vcorner=vcorner, vstart=vstart, vflag=vflag, E=len(ekeys))


def vertex_faces(tp, V):
    """Per vertex the faces of its corners in CSR order (a face with a repeated index appears once per corner, as on the device)."""
    return [[int(c) // 3 for c in tp["vcorner"][tp["vstart"][v]:tp["vstart"][v + 1]]] for v in range(V)]


def quadrics(verts, tris, tp):
    """[V, 10] float64: per vertex, per corner in CSR order, the face's plane (unit normal, weight = area) then the boundary constraints of the face's edges k and
    k + 2 at that corner (the plane through the edge perpendicular to the face, weight = BOUNDARY_WEIGHT * squared length)."""
    P = np.asarray(verts, np.float32).astype(np.float64).tolist(); t = np.asarray(tris, np.int64).tolist()
    V = len(P); Q = np.zeros((V, 10))
    for v in range(V):
        q = [0.0] * 10
        for c in tp["vcorner"][tp["vstart"][v]:tp["vstart"][v + 1]]:
            f, k = int(c) // 3, int(c) % 3
            p = [P[t[f][0]], P[t[f][1]], P[t[f][2]]]
            n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0])); l2 = _dot(n, n)
            if not l2 > 0.0:
                continue
            l = math.sqrt(l2); u = (n[0] / l, n[1] / l, n[2] / l)
            _add_plane(q, u, -_dot(u, p[0]), 0.5 * l)
            for j in (k, (k + 2) % 3):
                if tp["emult"][tp["corner_edge"][3 * f + j]] != 1:
                    continue
                pu, pw = p[j], p[(j + 1) % 3]
                ed = _sub(pw, pu); m = _cross(ed, u); m2 = _dot(m, m)
                if not m2 > 0.0:
                    continue
                ml = math.sqrt(m2); w = (m[0] / ml, m[1] / ml, m[2] / ml)
                _add_plane(q, w, -_dot(w, pu), BOUNDARY_WEIGHT * _dot(ed, ed))
        Q[v] = q
    return Q


def _ring_keeps_normals(P, t, faces, moved, other, nv, c0, c1):
    """(ok, a face of the ring holds c0 and c1, smallest |cos - FLIP_COS| seen)."""
    ok, dup, margin = True, False, math.inf
    for f in faces:
        i = t[f]
        if other in i:
            continue
        p = [P[i[0]], P[i[1]], P[i[2]]]
        n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
        r = [nv if i[k] == moved else p[k] for k in range(3)]
        m = _cross(_sub(r[1], r[0]), _sub(r[2], r[0]))
        dt = _dot(n, m); nn = _dot(n, n); mm = _dot(m, m)
        if not (dt > 0.0 and dt * dt > (FLIP_COS * FLIP_COS) * (nn * mm)):
            ok = False
        margin = min(margin, abs(dt / math.sqrt(nn * mm) - FLIP_COS) if nn * mm > 0 else math.inf)
        if c1 >= 0 and c0 in i and c1 in i:
            dup = True
    return ok, dup, margin


def eval_edge(a, b, m, P, Q, t, vf, fa, fb, optimal):
    """Step 2 for the edge (a, b), a < b, of multiplicity m: P positions (lists of float64 holding fp32 values), Q quadrics, t faces, vf[v] the faces around v,
    fa / fb the end points' flags (bit 0 boundary, bit 1 on an edge with more than two faces).  -> dict(cost, pos, flags, near, scale): `near` is true when a
    deciding quantity lies within its tolerance of its threshold; `scale` = (sum of the plane weights in Q) * (largest squared distance from the origin in the
    edge's region), the size of the terms that cancel in v^T Q v."""
    if a >= b:
        return dict(cost=0.0, pos=(0.0, 0.0, 0.0), flags=F_MULT, near=False, scale=1.0)
    flags = 0; near = False
    if m < 1 or m > 2 or ((fa | fb) & 2):
        flags |= F_MULT
    if m == 2 and (fa & 1) and (fb & 1):
        flags |= F_BOUNDARY
    qa, qb = Q[a], Q[b]
    q = [qa[j] + qb[j] for j in range(10)]
    pa, pb = P[a], P[b]
    placed = False; v = None
    if optimal:
        c00 = q[4] * q[7] - q[5] * q[5]; c01 = q[2] * q[5] - q[1] * q[7]; c02 = q[1] * q[5] - q[2] * q[4]
        c11 = q[0] * q[7] - q[2] * q[2]; c12 = q[1] * q[2] - q[0] * q[5]; c22 = q[0] * q[4] - q[1] * q[1]
        det = (q[0] * c00 + q[1] * c01) + q[2] * c02
        s = max(abs(q[0]), abs(q[1]), abs(q[2]), abs(q[4]), abs(q[5]), abs(q[7]))
        thr = DET_REL * ((s * s) * s)
        if thr > 0 and abs(abs(det) / thr - 1.0) < DET_TOL:
            near = True
        if abs(det) > thr:
            v = (f32(-(((c00 * q[3] + c01 * q[6]) + c02 * q[8]) / det)), f32(-(((c01 * q[3] + c11 * q[6]) + c12 * q[8]) / det)),
                 f32(-(((c02 * q[3] + c12 * q[6]) + c22 * q[8]) / det)))
            placed = all(math.isfinite(x) for x in v)
    if placed:
        cost = q_eval(q, *v)
    else:
        mid = (f32(0.5 * (pa[0] + pb[0])), f32(0.5 * (pa[1] + pb[1])), f32(0.5 * (pa[2] + pb[2])))
        ca, cb, cm = q_eval(q, *pa), q_eval(q, *pb), q_eval(q, *mid)
        cost, v = ca, tuple(pa)
        if cb < cost: cost, v = cb, tuple(pb)
        if cm < cost: cost, v = cm, mid
        w = (q[0] + q[4] + q[7]) * max(_dot(pa, pa), _dot(pb, pb))
        gaps = [abs(x - y) for x, y in ((ca, cb), (ca, cm), (cb, cm))]
        if any(0.0 < g < TIE_TOL * w for g in gaps):
            near = True
    cost = cost if cost > 0.0 else (0.0 if cost == cost else cost)
    if not (math.isfinite(f32(cost)) and all(math.isfinite(x) for x in v)):
        flags |= F_FINITE
    c0 = c1 = -1; ncommon = 0
    fa_list, fb_list = vf[a], vf[b]
    r2 = max(_dot(pa, pa), _dot(pb, pb), _dot(v, v) if all(math.isfinite(x) for x in v) else 0.0)
    for i, f in enumerate(fa_list):
        has_b = b in t[f]
        for k in range(3):
            x = t[f][k]
            if x == a or x == b:
                continue
            if has_b:
                if c0 < 0: c0 = x
                elif c1 < 0 and x != c0: c1 = x
            if x in t[f][:k] or any(x in t[g] for g in fa_list[:i]):
                continue
            r2 = max(r2, _dot(P[x], P[x]))
            if any(x in t[g] for g in fb_list):
                ncommon += 1
    for f in fb_list:
        for x in t[f]:
            r2 = max(r2, _dot(P[x], P[x]))
    if ncommon != m:
        flags |= F_LINK
    ok_a, dup_a, g_a = _ring_keeps_normals(P, t, fa_list, a, b, v, c0, c1)
    ok_b, dup_b, g_b = _ring_keeps_normals(P, t, fb_list, b, a, v, c0, c1)
    if not (ok_a and ok_b):
        flags |= F_FLIP
    if dup_a and dup_b:
        flags |= F_LINK
    if min(g_a, g_b) < FLIP_TOL:
        near = True
    return dict(cost=cost, pos=v, flags=flags, near=near, scale=(q[0] + q[4] + q[7]) * r2)


def cost_key(cost, e):
    return (int(np.float32(cost).view(np.uint32)) << 32) | int(e)


def edge_table(verts, tris, optimal=True):
    """Step 2 for every edge of a mesh -> dict of arrays over the E edges (plus the topology and the quadrics)."""
    V = len(verts); tp = topology(tris, V)
    P = np.asarray(verts, np.float32).astype(np.float64).tolist(); t = [tuple(r) for r in np.asarray(tris, np.int64).tolist()]
    Q = quadrics(verts, tris, tp); Ql = Q.tolist(); vf = vertex_faces(tp, V)
    E = tp["E"]
    out = dict(tp, quadrics=Q, cost=np.zeros(E), pos=np.zeros((E, 3), np.float32), flags=np.zeros(E, np.int64), near=np.zeros(E, bool), scale=np.zeros(E), keys=np.zeros(E, np.int64))
    for e in range(E):
        a, b = int(tp["ea"][e]), int(tp["eb"][e])
        r = eval_edge(a, b, int(tp["emult"][e]), P, Ql, t, vf, int(tp["vflag"][a]), int(tp["vflag"][b]), optimal)
        out["cost"][e] = r["cost"]; out["pos"][e] = r["pos"]; out["flags"][e] = r["flags"]; out["near"][e] = r["near"]; out["scale"][e] = r["scale"]
        out["keys"][e] = KEY_NONE if r["flags"] else cost_key(r["cost"], e)
    return out


def region(a, b, t, vf):
    """a, b and every vertex of a face around a or b."""
    r = {a, b}
    for f in vf[a] + vf[b]:
        r.update(t[f])
    return r


def select(tris, ea, eb, keys, cand):
    """Step 4 as a pure function: every candidate takes the minimum of its key over its region; selected = the candidates whose whole region holds their key.
    -> ascending edge ids."""
    t = [tuple(r) for r in np.asarray(tris, np.int64).tolist()]
    V = int(max(max(r) for r in t)) + 1
    vf = vertex_faces(topology(tris, V), V)
    vkey = {}
    regions = {int(e): region(int(ea[e]), int(eb[e]), t, vf) for e in cand}
    for e, reg in regions.items():
        for w in reg:
            vkey[w] = min(vkey.get(w, KEY_NONE), int(keys[e]))
    return np.array(sorted(e for e, reg in regions.items() if all(vkey[w] == int(keys[e]) for w in reg)), np.int64)


def greedy_decimate(verts, tris, target, optimalplacement=True):
    """The sequential decimator: always the valid edge of the smallest key (fp32 cost, then the end points), one collapse at a time, the same quadrics, placement
    and validity rules; after a collapse every edge at the kept vertex or at one of its neighbours is evaluated again.  Float64 on fp32 positions.
    -> (vertices f32, triangles i32), compacted in the old order."""
    V = len(verts); tp = topology(tris, V)
    P = np.asarray(verts, np.float32).astype(np.float64).tolist(); t = [tuple(r) for r in np.asarray(tris, np.int64).tolist()]
    Q = quadrics(verts, tris, tp).tolist(); vf = vertex_faces(tp, V)
    stamp = [0] * V; T = len(t); heap = []

    def vflag(v):
        cnt = {}
        for f in vf[v]:
            for x in t[f]:
                if x != v: cnt[x] = cnt.get(x, 0) + 1
        return (1 if any(c == 1 for c in cnt.values()) else 0) | (2 if any(c > 2 for c in cnt.values()) else 0), cnt

    def push(a, b, m, fa, fb):
        r = eval_edge(a, b, m, P, Q, t, vf, fa, fb, optimalplacement)
        if r["flags"] == 0:
            heapq.heappush(heap, (f32(r["cost"]), a, b, stamp[a], stamp[b], r["pos"]))

    def push_around(vs):
        fl = {}
        def flag(v):
            if v not in fl: fl[v] = vflag(v)
            return fl[v]
        done = set()
        for v in vs:
            for x, m in flag(v)[1].items():
                a, b = min(v, x), max(v, x)
                if (a, b) not in done:
                    done.add((a, b)); push(a, b, m, flag(a)[0], flag(b)[0])

    for e in range(tp["E"]):
        a, b = int(tp["ea"][e]), int(tp["eb"][e])
        push(a, b, int(tp["emult"][e]), int(tp["vflag"][a]), int(tp["vflag"][b]))
    alive = [True] * len(t)
    while T > target and heap:
        c, a, b, sa, sb, pos = heapq.heappop(heap)
        if stamp[a] != sa or stamp[b] != sb:
            continue
        P[a] = list(pos); Q[a] = [Q[a][j] + Q[b][j] for j in range(10)]
        for f in vf[b]:
            if not alive[f]:
                continue
            if a in t[f]:
                alive[f] = False; T -= 1
                for x in t[f]:
                    if x != b: vf[x] = [g for g in vf[x] if g != f]
            else:
                t[f] = tuple(a if x == b else x for x in t[f]); vf[a].append(f)
        vf[b] = []
        vf[a].sort()
        ring = {a}
        for f in vf[a]:
            ring.update(t[f])
        for v in ring:
            stamp[v] += 1
        stamp[b] += 1
        push_around(sorted(ring))
    keep = np.array(alive, bool)
    tt = np.array([t[f] for f in range(len(t)) if alive[f]], np.int64).reshape(-1, 3)
    used = np.zeros(V, bool); used[tt.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.asarray(P, np.float64)[used].astype(np.float32), remap[tt].astype(np.int32)


# ------------------------------------------------------------------------------------------------ distances
def point_mesh_distance(points, verts, tris, chunk=256):
    """Distance from every point to the closest point of a triangle mesh (Ericson's closest point on a triangle, all regions), float64."""
    pts = np.asarray(points, np.float64); v = np.asarray(verts, np.float64); t = np.asarray(tris, np.int64)
    A, B, Cc = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    ab, ac = B - A, Cc - A
    out = np.empty(len(pts))
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk, None, :]
        ap = p - A
        d1 = (ab * ap).sum(-1); d2 = (ac * ap).sum(-1)
        bp = p - B; d3 = (ab * bp).sum(-1); d4 = (ac * bp).sum(-1)
        cp = p - Cc; d5 = (ab * cp).sum(-1); d6 = (ac * cp).sum(-1)
        va = d3 * d6 - d5 * d4; vb = d5 * d2 - d1 * d6; vc = d1 * d4 - d3 * d2
        with np.errstate(all="ignore"):
            denom = va + vb + vc
            vv = np.where(denom != 0, vb / denom, 0.0); ww = np.where(denom != 0, vc / denom, 0.0)
            q = A + ab * vv[..., None] + ac * ww[..., None]                                   # interior
            e_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0); tq = np.where(d1 - d3 != 0, d1 / (d1 - d3), 0.0)
            q = np.where(e_ab[..., None], A + ab * tq[..., None], q)
            e_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0); tq = np.where(d2 - d6 != 0, d2 / (d2 - d6), 0.0)
            q = np.where(e_ac[..., None], A + ac * tq[..., None], q)
            e_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0); tq = np.where((d4 - d3) + (d5 - d6) != 0, (d4 - d3) / ((d4 - d3) + (d5 - d6)), 0.0)
            q = np.where(e_bc[..., None], B + (Cc - B) * tq[..., None], q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], A, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], B, q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], Cc, q)
        out[s:s + chunk] = np.sqrt(((p - q) ** 2).sum(-1)).min(axis=1)
    return out


def rms_distance(points, verts, tris):
    d = point_mesh_distance(points, verts, tris)
    return float(np.sqrt((d * d).mean()))


def symmetric_rms(v0, t0, v1, t1):
    """RMS over both meshes' vertices of the distance to the other mesh."""
    d = np.concatenate([point_mesh_distance(v0, v1, t1), point_mesh_distance(v1, v0, t0)])
    return float(np.sqrt((d * d).mean()))


# ------------------------------------------------------------------------------------------------ test meshes and their checks
def perturbed_icosphere(subdiv, seed=3, amount=0.02):
    """An icosphere whose vertices are moved radially by up to +-amount (fixed seed)."""
    from stage0_refs import icosphere
    v, t = icosphere(subdiv, 1.0)
    r = 1.0 + amount * (2.0 * np.random.default_rng(seed).random(len(v)) - 1.0)
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), t


def hemisphere(subdiv=3, seed=3):
    """The faces of the perturbed icosphere whose centroid c has c . (0.3, 0.2, 1) > 0.1: an open surface with one jagged boundary loop (the tilted cut leaves
    interior edges between boundary vertices)."""
    from stage0_refs import compact
    v, t = perturbed_icosphere(subdiv, seed)
    keep = v[t.astype(np.int64)].mean(axis=1).astype(np.float64) @ np.array([0.3, 0.2, 1.0]) > 0.1
    return compact(v, t, keep)


def grid_cube(n=12):
    """The unit cube [-0.5, 0.5]^3, every face an n x n grid of two-triangle cells (12 n^2 faces), outward wound, vertices shared along the cube's edges."""
    idx = {}; verts = []; tris = []

    def vid(p):
        k = tuple(p)
        if k not in idx:
            idx[k] = len(verts); verts.append([c / n - 0.5 for c in k])
        return idx[k]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def pt(di, dj):
                        p = [0, 0, 0]; p[axis] = side; p[u] = i + di; p[w] = j + dj
                        return vid(p)
                    q = [pt(0, 0), pt(1, 0), pt(1, 1), pt(0, 1)]
                    if side == 0:
                        q = q[::-1]
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts, np.float32), np.array(tris, np.int32)


def torus(nu=48, nv=42, R=1.0, r=0.4):
    """A torus (genus 1), 2 nu nv faces, outward wound."""
    v = [[(R + r * math.cos(2 * math.pi * j / nv)) * math.cos(2 * math.pi * i / nu), (R + r * math.cos(2 * math.pi * j / nv)) * math.sin(2 * math.pi * i / nu),
          r * math.sin(2 * math.pi * j / nv)] for i in range(nu) for j in range(nv)]
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            t += [(a, b, c), (a, c, d)]
    return np.array(v, np.float32), np.array(t, np.int32)


def synthetic_volume_np(r=40):
    """stage0.synthetic_volume's analytic density (a dented ball and a small floater) evaluated in numpy float32, so that CPU and GPU tests cut the same volume."""
    ax = np.linspace(-1, 1, r, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    c = np.float32(0.2)
    d_ball = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - np.float32(0.85)
    d_dent = np.float32(0.35) - np.sqrt((x - c - np.float32(0.7)) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    d_float = np.sqrt((x + np.float32(0.9)) ** 2 + (y + np.float32(0.9)) ** 2 + (z + np.float32(0.9)) ** 2) - np.float32(0.28)
    sd = np.minimum(np.maximum(d_ball, d_dent), d_float)
    return np.ascontiguousarray(np.maximum(np.float32(-40.0) * sd, np.float32(0)).astype(np.float32))


def mc_mesh_np(r=40):
    """The cleaned marching-cubes mesh of synthetic_volume_np(r) at density 10 in world space, on the CPU: the restated marching cubes (stage0_refs), then the
    largest edge-connected component (what clean_mesh leaves of this scene: the floater goes)."""
    from stage0_refs import marching_cubes, components, compact
    v, t = marching_cubes(synthetic_volume_np(r), 10.0)
    v = (v / np.float32(r - 1.0) * np.float32(2) - np.float32(1)).astype(np.float32)
    lab = components(t)
    ids, n = np.unique(lab, return_counts=True)
    return compact(v, t, lab == ids[np.argmax(n)])


def boundary_loops(tris):
    """(number of boundary loops, every boundary vertex has exactly two boundary edges, no edge has more than two faces)."""
    t = np.asarray(tris, np.int64)
    tp = topology(t, int(t.max()) + 1)
    m = tp["emult"] == 1
    ea, eb = tp["ea"][m], tp["eb"][m]
    deg = {}
    for a, b in zip(ea, eb):
        deg.setdefault(int(a), []).append(int(b)); deg.setdefault(int(b), []).append(int(a))
    two = all(len(n) == 2 for n in deg.values())
    seen = set(); loops = 0
    for s in deg:
        if s in seen:
            continue
        loops += 1; stack = [s]
        while stack:
            x = stack.pop()
            if x in seen: continue
            seen.add(x); stack += deg[x]
    return loops, two, bool((tp["emult"] <= 2).all())


def invariants(verts, tris):
    """The output checks of a whole run that need no input: indices in range, no unreferenced vertex, no repeated index, no duplicate face."""
    t = np.asarray(tris, np.int64); V = len(verts)
    s = np.sort(t, axis=1)
    return bool(t.min() >= 0 and t.max() < V and len(np.unique(t)) == V and (s[:, 0] != s[:, 1]).all() and (s[:, 1] != s[:, 2]).all() and len(np.unique(s, axis=0)) == len(t)
                and np.isfinite(verts).all())
