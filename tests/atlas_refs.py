"""numpy restatement of the chart atlas (export.chart_atlas, csrc/atlas.hip) for tests/test_atlas_host.py and tests/test_gpu_atlas.py, written from the rules in
include/mirres.h, not from the kernels:

    classify_ref / neighbours_ref / smooth_ref / charts_ref     segmentation: fp32 normals, buckets, manifold neighbours, Jacobi rounds, charts
    bounds_ref / emit_ref                                       parametrisation: ordered-integer min / max, one UV vertex per (chart, mesh vertex)
    cover_hits / flagged_ref                                    the overlap check: every (triangle, covered texel centre) pair under the bake's coverage rule
    atlas_ref                                                   the whole of chart_atlas with these in place of the device calls (the packing is export.py's own)
    check_invariants                                            what must hold on any result, the device's or the restatement's
    cube / helicoid / hostile / confetti                        the meshes

Every floating-point step is a float32 numpy operation (rounded once) or a float64 one where the rule says fp64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bake_refs as R

AX_U = np.array([1, 2, 2, 0, 0, 1]); AX_V = np.array([2, 1, 0, 2, 1, 0])     # (U, V, d_k) right-handed, k = +x -x +y -y +z -z
U32 = 2.0 ** -24                                                              # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------------------------------------------- meshes
def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)          # index = 4 x + 2 y + z
    quads = [(4, 6, 7, 5), (0, 1, 3, 2), (2, 3, 7, 6), (0, 4, 5, 1), (1, 5, 7, 3), (0, 2, 6, 4)]   # +x -x +y -y +z -z, outward
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def helicoid(nr=4, nt=64, pitch=0.05, turns=2.0):
    """(r cos t, r sin t, pitch t), r in [0.3, 0.8] in nr steps, t in [0, turns 2 pi] in nt steps: 2 nr nt triangles, normals up, covers itself twice in xy."""
    r = np.linspace(0.3, 0.8, nr + 1); t = np.linspace(0.0, turns * 2.0 * np.pi, nt + 1)
    rr, tt = np.meshgrid(r, t, indexing="ij")
    v = np.stack((rr * np.cos(tt), rr * np.sin(tt), pitch * tt), -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: i * (nt + 1) + j
    f = []
    for i in range(nr):
        for j in range(nt):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, np.int32)


def hostile():
    """A tilted 4 x 4 quad sheet (32 faces) plus: a zero-area face, a face with a repeated index, a face on a NaN vertex, a fin (a third face on an interior
    edge), a copy of face 0, an isolated triangle, a face with an index past V and one with a negative index.  -> (v, f, names of the extra faces)."""
    g = np.linspace(0.0, 1.0, 5)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack((x, y, 0.25 * x + 0.125 * y), -1).reshape(-1, 3)                    # dyadic: every coordinate and product below is exact
    idx = lambda i, j: 5 * i + j
    f = []
    for i in range(4):
        for j in range(4):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, b, c), (a, c, d)]
    extra = np.array([[0.5, 0.5, 0.9], [np.nan, 0.3, 0.3], [3.0, 3.0, 3.0], [3.4, 3.0, 3.1], [3.0, 3.5, 3.0]])
    V0 = v.shape[0]; v = np.concatenate((v, extra)).astype(np.float32)
    names = ["zero_area", "repeated", "nan", "fin", "duplicate", "isolated", "past_v", "negative"]
    f += [(idx(0, 0), idx(2, 2), idx(4, 4)),                  # collinear on the sheet: the cross product is exactly 0
          (idx(1, 1), idx(1, 2), idx(1, 1)),
          (idx(0, 0), V0 + 1, idx(0, 1)),
          (idx(1, 1), idx(2, 2), V0),                         # the diagonal (1,1)-(2,2) belongs to two sheet faces already
          f[0],
          (V0 + 2, V0 + 3, V0 + 4),
          (idx(3, 3), idx(4, 3), v.shape[0] + 5),
          (idx(3, 3), -1, idx(3, 4))]
    return v, np.array(f, np.int32), {n: 32 + k for k, n in enumerate(names)}


def confetti(n=65537 + 300, seed=3):
    """n disjoint, well-shaped random triangles (no shared vertex): every one a chart of its own; sizes spread over a factor of 3."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    ang = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2])[None, :] + rng.uniform(-0.3, 0.3, (n, 3))
    a = rng.standard_normal((n, 3)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(a, rng.standard_normal((n, 3))); b /= np.linalg.norm(b, axis=1, keepdims=True)
    size = rng.uniform(0.01, 0.03, (n, 1, 1))
    v = c + size * (np.cos(ang)[..., None] * a[:, None, :] + np.sin(ang)[..., None] * b[:, None, :])
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


# ------------------------------------------------------------------------------------------------------------------------------- segmentation
def classify_ref(v, f):
    v = np.asarray(v, np.float32).reshape(-1, 3); f = np.asarray(f, np.int64).reshape(-1, 3)
    V = v.shape[0]
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    p = v[np.where(ok[:, None], f, 0)] if V else np.zeros((f.shape[0], 3, 3), np.float32)
    with np.errstate(all="ignore"):
        e1 = p[:, 1] - p[:, 0]; e2 = p[:, 2] - p[:, 0]
        n = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)
    assert n.dtype == np.float32
    ok &= np.isfinite(p).all((1, 2)) & np.isfinite(n).all(1) & (n != 0).any(1)
    n = np.where(ok[:, None], n, np.float32(0))
    vals = np.stack((n[:, 0], -n[:, 0], n[:, 1], -n[:, 1], n[:, 2], -n[:, 2]), 1)
    return n, np.where(ok, np.argmax(vals, 1), -1).astype(np.int32)          # argmax: the first of equal maxima = the lowest k


def neighbours_ref(f, V):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    nbr = np.full(f.shape, -1, np.int32)
    carried = {}
    for t, tri in enumerate(f.tolist()):
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            if a != b and 0 <= a < V and 0 <= b < V:
                carried.setdefault((min(a, b), max(a, b)), []).append((t, k))
    for lst in carried.values():
        if len(lst) == 2:
            (t, k), (u, m) = lst
            nbr[t, k] = u; nbr[u, m] = t
    return nbr


def smooth_ref(normal, bucket, nbr, cos_min):
    n = np.asarray(normal, np.float32).astype(np.float64); T = n.shape[0]
    c = float(np.float32(cos_min))
    thr = (c * c) * ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    vals = np.stack((n[:, 0], -n[:, 0], n[:, 1], -n[:, 1], n[:, 2], -n[:, 2]), 1)
    elig = (vals > 0) & (vals * vals >= thr[:, None])
    rows = np.arange(T); good = bucket >= 0
    votes = np.zeros((T, 6))
    own = np.where(good, bucket, 0)
    np.add.at(votes, (rows[good], own[good]), np.where(elig[rows[good], own[good]], 1.5, 0.0))
    for e in range(3):
        g = nbr[:, e]; has = good & (g >= 0)
        b = np.where(has, bucket[np.where(has, g, 0)], -1)
        has &= b >= 0
        has[has] = elig[rows[has], b[has]]
        np.add.at(votes, (rows[has], b[has]), 1.0)
    best = votes.max(1)
    tied = votes == best[:, None]
    new = np.where((best == 0) | tied[rows, own], own, np.argmax(tied, 1))
    return np.where(good, new, -1).astype(np.int32)


def charts_ref(bucket, nbr):
    """chart i32[T] (-1: degenerate), count: components of faces joined across manifold edges with one bucket on both sides, in order of their smallest face."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    T = bucket.shape[0]
    if T == 0:
        return np.zeros(0, np.int32), 0
    t = np.repeat(np.arange(T), 3); u = nbr.reshape(-1)
    ok = (u >= 0) & (bucket[t] >= 0)
    ok[ok] = bucket[u[ok]] == bucket[t[ok]]
    _, comp = connected_components(coo_matrix((np.ones(int(ok.sum())), (t[ok], u[ok])), shape=(T, T)), directed=False)
    good = bucket >= 0
    smallest = np.full(comp.max() + 1, T); np.minimum.at(smallest, comp[good], np.nonzero(good)[0])
    roots = np.unique(smallest[comp[good]])
    chart = np.full(T, -1, np.int32); chart[good] = np.searchsorted(roots, smallest[comp[good]])
    return chart, int(roots.shape[0])


# ---------------------------------------------------------------------------------------------------------------------------- parametrisation
def _ordered(x):
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def _unordered(e):
    return np.where(e >> 31 != 0, e & np.uint32(0x7FFFFFFF), ~e).astype(np.uint32).view(np.float32)


def bounds_ref(v, f, bucket, chart, n_charts):
    v = np.asarray(v, np.float32); f = np.asarray(f, np.int64)
    lo = np.full((n_charts, 2), 0xFFFFFFFF, np.uint32); hi = np.zeros((n_charts, 2), np.uint32)
    t = np.nonzero(chart >= 0)[0]
    for k in range(3):
        p = v[f[t, k]]
        uv = _ordered(np.stack((p[np.arange(t.size), AX_U[bucket[t]]], p[np.arange(t.size), AX_V[bucket[t]]]), 1))
        for a in (0, 1):
            np.minimum.at(lo[:, a], chart[t], uv[:, a]); np.maximum.at(hi[:, a], chart[t], uv[:, a])
    return np.concatenate((_unordered(lo), _unordered(hi)), 1)


def emit_ref(v, f, chart, bucket, bounds, origin, density, w0, h0):
    """(vt f32[n_uv,2] of the (chart, vertex) pairs in ascending (chart, vertex) order, ft i64[T,3] with -1 rows for the faces of no chart)."""
    v = np.asarray(v, np.float32); f = np.asarray(f, np.int64); V = max(v.shape[0], 1)
    t = np.nonzero(chart >= 0)[0]
    key, inv = np.unique((chart[t].astype(np.int64)[:, None] * V + f[t]).reshape(-1), return_inverse=True)
    c, m = key // V, key % V
    cb = np.zeros(bounds.shape[0], np.int64); cb[chart[t]] = bucket[t]
    s = np.float32(density)
    out = []
    for ax, col, size in ((AX_U, 0, w0), (AX_V, 1, h0)):
        coord = v[m, ax[cb[c]]]
        d = (coord - bounds[c, col]) * s
        tex = (origin[c, col].astype(np.float32) + np.float32(0.5)) + d
        out.append(tex / np.float32(size))
    vt = np.stack(out, 1) if key.size else np.zeros((0, 2), np.float32)
    assert vt.dtype == np.float32
    ft = np.full(f.shape, -1, np.int64); ft[t] = inv.reshape(-1, 3)
    return vt, ft


# ------------------------------------------------------------------------------------------------------------------------------ overlap check
def cover_hits(vt, ft, W, H, small=12):
    """(triangle i64[n], texel i64[n]): every (triangle, texel centre it covers) pair under mirres_uv_rasterize's rule (bake_refs: 1/256 snap, int64 edge
    functions, top-left rule).  Boxes up to `small` texels a side are walked one box offset at a time over all triangles, larger ones triangle by triangle."""
    s = R.tri_setup(vt, ft, W, H)
    tri, pix = [], []
    is_small = (s["bw"] <= small) & (s["bh"] <= small)
    for dr in range(small):
        for dc in range(small):
            t = np.nonzero(is_small & (s["bh"] > dr) & (s["bw"] > dc))[0]
            if t.size:
                c, r = s["c0"][t] + dc, s["r0"][t] + dr
                _, ins = R._weights(s, t, c * R.FIX + R.FIX // 2, r * R.FIX + R.FIX // 2)
                tri.append(t[ins]); pix.append((r * W + c)[ins])
    for t in np.nonzero(~is_small & (s["bw"] > 0))[0]:
        cc, rr = np.meshgrid(s["c0"][t] + np.arange(s["bw"][t]), s["r0"][t] + np.arange(s["bh"][t]))
        cc, rr = cc.reshape(-1), rr.reshape(-1)
        _, ins = R._weights(s, np.full(cc.size, t), cc * R.FIX + R.FIX // 2, rr * R.FIX + R.FIX // 2)
        tri.append(np.full(int(ins.sum()), t)); pix.append((rr * W + cc)[ins])
    if not tri:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(tri).astype(np.int64), np.concatenate(pix).astype(np.int64)


def flagged_ref(vt, ft, face_chart, n_charts, W, H):
    """u8[n_charts + 1]: the charts (last slot: faces of no chart) of every triangle that covers a centre covered more than once; and the number of such centres."""
    tri, pix = cover_hits(vt, ft, W, H)
    count = np.bincount(pix, minlength=W * H)
    c = face_chart[tri[count[pix] >= 2]]
    flagged = np.zeros(n_charts + 1, np.uint8)
    flagged[np.where(c >= 0, c, n_charts)] = 1
    return flagged, int((count >= 2).sum())


# --------------------------------------------------------------------------------------------------------------------------------- the whole
def atlas_ref(EX, v, f, h0, w0, ssaa=1, cos_min=0.5, smooth_rounds=2):
    """chart_atlas restated.  -> dict: normal, buckets (list: after classification and after every round), nbr, attempts (list per packing attempt of chart,
    n_charts, bounds, density, origin, vt, ft, flagged), and the final vt, ft, face_chart, n_charts, density, bounds, origin."""
    v = np.asarray(v, np.float32).reshape(-1, 3); f = np.asarray(f, np.int64).reshape(-1, 3)
    normal, bucket = classify_ref(v, f)
    nbr = neighbours_ref(f, v.shape[0])
    buckets = [bucket]
    for _ in range(smooth_rounds):
        buckets.append(smooth_ref(normal, buckets[-1], nbr, cos_min))
    bucket = buckets[-1]
    chart, n_charts = charts_ref(bucket, nbr)
    out = dict(normal=normal, buckets=buckets, nbr=nbr, attempts=[])
    for attempt in (0, 1):
        bounds = bounds_ref(v, f, bucket, chart, n_charts)
        density, origin, cell_vt, ft_rows = EX._chart_layout(v.astype(np.float64), f, np.nonzero(chart < 0)[0], bounds, h0, w0)
        vt_c, ft = emit_ref(v, f, chart, bucket, bounds, origin, density, w0, h0)
        ft = np.where(ft >= 0, ft, ft_rows + vt_c.shape[0])
        vt = np.concatenate((vt_c, cell_vt.reshape(-1, 2)))
        flagged, _ = flagged_ref(vt, ft, chart, n_charts, w0 * ssaa, h0 * ssaa)
        out["attempts"].append(dict(chart=chart, n_charts=n_charts, bounds=bounds, density=density, origin=origin, vt=vt, ft=ft.astype(np.int32), flagged=flagged))
        if not flagged.any():
            break
        assert attempt == 0 and not flagged[n_charts], "the restated layout still overlaps after the fallback"
        keep = flagged[:n_charts] == 0
        new_id = np.cumsum(keep) - 1
        chart = np.where((chart >= 0) & keep[np.maximum(chart, 0)], new_id[np.maximum(chart, 0)], -1).astype(np.int32)
        n_charts = int(keep.sum())
    out.update(out["attempts"][-1]); out["face_chart"] = out["chart"]
    return out


# -------------------------------------------------------------------------------------------------------------------------------- invariants
def face_groups(ft, face_chart):
    """A group id per face: its chart, or for a fallback face its cell (the smallest UV vertex of a cell is used by every face of the cell and by no other)."""
    g = face_chart.astype(np.int64).copy()
    fb = face_chart < 0
    g[fb] = int(face_chart.max(initial=-1)) + 1 + ft[fb].min(1)
    return g


def stretch_bounds(v, f, faces, density, cos_min, w0):
    """Per face the interval the singular values of its 3D -> export-texel map must lie in, [s cos_min (1 - eps), s (1 + eps)], with eps derived per face:
    - a texel coordinate is fl(fl(origin + 0.5) + fl(fl(c - min) s)) / size: the subtraction, the product, the sum and the quotient each add a relative
      2^-24 of a number below w0 texels, so a corner is off by at most delta = 4 * 2^-24 * w0 texels;
    - the map is E_uv pinv(E_3d) with E the two edge vectors: the four entries of E_uv move by at most 2 delta, its spectral norm by at most 4 delta, and
      so every singular value of the map by at most 4 delta / sigma_min(E_3d) (Weyl);
    - the exact map of a face projected along d has the singular values s and s (n . d) / |n|; the bucket rule bounds the cosine of the fp32 normal, whose
      components are each off by at most 6 * 2^-24 |e1| |e2| (two rounded edge components, two rounded products, one rounded difference, on terms of at
      most |e1| |e2| each), i.e. the cosine by at most 2 sqrt(3) 6 * 2^-24 |e1| |e2| / |n| <= 22 * 2^-24 / sin(angle between the edges)."""
    p = v[f[faces]].astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    E = np.stack((e1, e2), 2)                                                   # [n, 3, 2]
    smin = np.linalg.svd(E, compute_uv=False)[:, -1]
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    delta = 4 * U32 * w0
    shift = 4 * delta / smin
    s = float(density)
    return s * (cos_min - 22 * U32 / sin) - shift, s + shift


def texel_maps(v, f, vt, ft, faces, w0, h0):
    """Singular values [n, 2] of the 3D -> export-texel map of the faces, float64."""
    p = v[f[faces]].astype(np.float64); q = vt[ft[faces]].astype(np.float64) * np.array([w0, h0], np.float64)
    E3 = np.stack((p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), 2); E2 = np.stack((q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), 2)
    J = E2 @ np.linalg.pinv(E3)
    return np.linalg.svd(J, compute_uv=False)[:, :2], E2


def check_invariants(v, f, vt, ft, face_chart, density, bounds, origin, h0, w0, ssaa, cos_min, gap, owner=None):
    """Invariants 1-4 of the chart atlas on a finished layout.  `owner`: i64[H*W] triangle per bake texel (-1 none) from a raster record, or None to take the
    restatement's own coverage.  Returns the per-texel owner used."""
    v = np.asarray(v, np.float32); f = np.asarray(f, np.int64); vt = np.asarray(vt, np.float32); ft = np.asarray(ft, np.int64)
    T = f.shape[0]; W, H = w0 * ssaa, h0 * ssaa
    n_charts = bounds.shape[0]
    # 4. vertex sharing, ranges
    assert ft.shape == f.shape and face_chart.shape == (T,)
    if T == 0:
        return np.full(H * W, -1, np.int64)
    assert ft.min() >= 0 and ft.max() < vt.shape[0], "every face has UVs, in range"
    assert face_chart.max() < n_charts and face_chart.min() >= -1
    assert np.isfinite(vt).all() and vt.min() >= 0 and vt.max() <= 1, "no geometry outside [0, 1]^2"
    nbr = neighbours_ref(f, v.shape[0])
    for k in range(3):
        u = nbr[:, k]; inner = (u >= 0) & (face_chart >= 0)
        inner[inner] = face_chart[u[inner]] == face_chart[inner]
        t = np.nonzero(inner)[0]
        a, b = f[t, k], f[t, (k + 1) % 3]
        fu = f[u[t]]; ftu = ft[u[t]]
        ua = ftu[np.arange(t.size), np.argmax(fu == a[:, None], 1)]; ub = ftu[np.arange(t.size), np.argmax(fu == b[:, None], 1)]
        assert np.array_equal(ft[t, k], ua) and np.array_equal(ft[t, (k + 1) % 3], ub), "an interior edge of a chart shares both UV vertices"
    # 1. no double coverage
    tri, pix = cover_hits(vt, ft, W, H)
    count = np.bincount(pix, minlength=W * H)
    assert count.max(initial=0) <= 1, "%d bake texel centres are covered twice" % int((count > 1).sum())
    if owner is None:
        owner = np.full(H * W, -1, np.int64); owner[pix] = tri
    else:
        mine = np.full(H * W, -1, np.int64); mine[pix] = tri
        assert np.array_equal(owner, mine), "the raster record and the restated coverage name different triangles"
    # 2. separation: geometry inside its rectangle, rectangles and cells `gap` export texels apart, texels of two groups never closer than gap * ssaa
    ch = np.nonzero(face_chart >= 0)[0]
    if ch.size:
        q = vt[ft[ch]].astype(np.float64) * np.array([w0, h0], np.float64)
        c = face_chart[ch]
        ext = (bounds[:, 2:4] - bounds[:, 0:2]).astype(np.float32)
        size = np.ceil(ext * np.float32(density)).astype(np.int64) + 1
        tol = 4 * U32 * max(w0, h0)
        assert (q >= (origin[c] + 0.5)[:, None, :] - tol).all() and (q <= (origin[c] + size[c] - 0.5)[:, None, :] + tol).all(), "geometry outside its chart's rectangle"
        paint = np.zeros((h0 + gap, w0 + gap), np.int32)
        for (x, y), (w, h) in zip(origin.tolist(), size.tolist()):
            assert x >= 0 and y >= 0 and x + w <= w0 and y + h <= h0
            paint[y:y + h + gap, x:x + w + gap] += 1
        assert paint.max() <= 1, "two chart rectangles closer than the gap"
    from scipy.ndimage import maximum_filter, minimum_filter
    group = face_groups(ft, face_chart)
    gimg = np.where(owner >= 0, group[np.maximum(owner, 0)], -1).reshape(H, W)
    k = 2 * (gap * ssaa - 1) + 1                                                # Chebyshev distance < gap * ssaa
    big = int(gimg.max()) + 1
    hi = maximum_filter(gimg, size=k, mode="constant", cval=-1)
    lo = minimum_filter(np.where(gimg >= 0, gimg, big), size=k, mode="constant", cval=big)
    cov = gimg >= 0
    assert (hi[cov] == gimg[cov]).all() and (lo[cov] == gimg[cov]).all(), "texels of two charts closer than the gap"
    # 3. orientation and stretch of the chart faces
    if ch.size:
        sv, E2 = texel_maps(v, f, vt, ft, ch, w0, h0)
        assert (np.linalg.det(E2) > 0).all(), "a chart face with non-positive UV orientation"
        lo_b, hi_b = stretch_bounds(v, f, ch, density, cos_min, max(w0, h0))
        assert (sv[:, 1] >= lo_b).all() and (sv[:, 0] <= hi_b).all(), (float((sv[:, 1] - lo_b).min()), float((hi_b - sv[:, 0]).min()))
    return owner
