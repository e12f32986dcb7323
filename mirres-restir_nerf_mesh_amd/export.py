"""Stage-1 mesh export (nerf/renderer.py:319-476 `NeRFRenderer.export_stage1`, driven by Trainer.export_stage1, nerf/utils.py:1271-1281): per mesh
cascade an OBJ with UVs, its MTL and two baked textures of the material field — feat0 (kd, channels 0-2, the MTL's map_Kd) and feat1 (channels 3-5).

    vt, ft, fill = uv_atlas(v, f, h0, w0)                                   # xatlas in the reference (:334-347): a deterministic pair atlas here,
    vt, ft, info = chart_atlas(v, f, h0, w0, ssaa)                          # or axis-projected charts built on csrc/atlas.hip (atlas="charts")
    feat0, feat1 = bake_textures(mlp.sample_no_di, v, f, vt, ft, h0, w0, ssaa)["feat"]     # :349-422 on csrc/bake.hip
    export_stage1(path, vertices, triangles, v_cumsum, f_cumsum, mlp, texture_size=4096, ssaa=2)   # the cascade loop (:464-476)

The bake runs on an (h0 ssaa) x (w0 ssaa) grid: UV rasterisation (mirres_uv_rasterize), positions (mirres_interpolate), the field at the covered
texels, sRGB quantisation (mirres_bake_quantise), the 32-texel gutter inpaint (mirres_texture_inpaint) and the SSAA downsample
(mirres_texture_downsample).  Textures are written as PNG (meters.write_png, lossless) where the reference writes JPEG."""
import ctypes as C
import math
import os
import time

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, stream_ptr
from . import raster, meters

MAX_TRIANGLES = 1 << 24        # the triangle id of the raster record is stored in fp32
INPAINT_RADIUS = 32            # binary_dilation(mask, iterations=32) (renderer.py:403)
CELL_GAP = 2                   # export texels between two atlas cells
FIELD_BATCH = 1 << 22          # texels per call of the material field


def _check_sizes(T, h0, w0, ssaa):
    if int(h0) <= 0 or int(w0) <= 0:
        raise ValueError("texture size must be positive, got %s x %s" % (h0, w0))
    if int(ssaa) < 1:
        raise ValueError("ssaa must be >= 1, got %s" % ssaa)
    if T >= MAX_TRIANGLES:
        raise ValueError("%d triangles: the bake stores the triangle id in fp32 (fewer than 2^24 triangles per cascade)" % T)
    if (h0 * ssaa) * (w0 * ssaa) >= 1 << 31 or h0 * ssaa > 65536 or w0 * ssaa > 65536:
        raise ValueError("bake grid %d x %d is too large" % (h0 * ssaa, w0 * ssaa))


# ---------------------------------------------------------------------------------------------------------------------------- device operators
@torch.no_grad()
def uv_rasterize(vt, ft, W, H):
    """dr.rasterize(glctx, uv * 2 - 1, ft, (H, W)) (renderer.py:352-357) with exact integer coverage: vt f32[Nt,2], ft i32[T,3] -> rast f32[H*W,4]
    = (b0, b1, 0, triangle_id + 1), zeros where no triangle covers the texel centre (include/mirres.h)."""
    T = int(ft.shape[0])
    if T >= MAX_TRIANGLES:
        raise ValueError("uv_rasterize: %d triangles (the id is stored in fp32: fewer than 2^24)" % T)
    if W <= 0 or H <= 0:
        raise ValueError("uv_rasterize: bad grid %d x %d" % (W, H))
    dev = torch.device("cuda")
    uv = torch.as_tensor(vt, dtype=torch.float32).to(dev).contiguous()
    t = torch.as_tensor(ft).to(dev, torch.int32).contiguous()
    nbytes = int(lib().mirres_uv_rasterize_scratch(T))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    rast = torch.empty((H * W, 4), dtype=torch.float32, device=dev)
    check(lib().mirres_uv_rasterize(uv.data_ptr() if T else None, int(uv.shape[0]), t.data_ptr() if T else None, T, int(W), int(H), rast.data_ptr(),
                                    scratch.data_ptr(), nbytes, stream_ptr()), "mirres_uv_rasterize")
    return rast


@torch.no_grad()
def bake_quantise(feats, index, W, H):
    """renderer.py:390-398 on the covered texels: feats f32[n,6], index i32[n] -> two u8[H*W*3] planes (channels 0-2, 3-5), 0 elsewhere."""
    f = feats.contiguous().float(); idx = index.to(torch.int32).contiguous(); n = int(idx.shape[0])
    out0 = torch.empty(H * W * 3, dtype=torch.uint8, device=f.device); out1 = torch.empty_like(out0)
    check(lib().mirres_bake_quantise(f.data_ptr() if n else None, idx.data_ptr() if n else None, n, int(W), int(H), out0.data_ptr(), out1.data_ptr(),
                                     stream_ptr()), "mirres_bake_quantise")
    return out0, out1


@torch.no_grad()
def texture_inpaint(mask, in0, in1, W, H, radius=INPAINT_RADIUS):
    """renderer.py:400-414: texels within L1 distance `radius` of the mask copy their Euclidean-nearest covered texel, the rest outside it is 0."""
    m = mask.to(torch.uint8).contiguous()
    a0, a1 = in0.contiguous(), in1.contiguous()
    dy = torch.empty(H * W, dtype=torch.int8, device=m.device)
    out0 = torch.empty_like(a0); out1 = torch.empty_like(a1)
    check(lib().mirres_texture_inpaint(int(W), int(H), int(radius), m.data_ptr(), a0.data_ptr(), a1.data_ptr(), dy.data_ptr(), out0.data_ptr(),
                                       out1.data_ptr(), stream_ptr()), "mirres_texture_inpaint")
    return out0, out1


@torch.no_grad()
def texture_downsample(img, W, H, ssaa):
    """cv2.resize(img, (W / ssaa, H / ssaa), interpolation=INTER_LINEAR) (renderer.py:420-422) of a u8[H*W*3] plane -> u8[H/ssaa, W/ssaa, 3]."""
    if ssaa < 1 or W % ssaa or H % ssaa:
        raise ValueError("texture_downsample: %d x %d is not divisible by ssaa %d" % (W, H, ssaa))
    a = img.contiguous()
    out = torch.empty((H // ssaa, W // ssaa, 3), dtype=torch.uint8, device=a.device)
    check(lib().mirres_texture_downsample(int(W), int(H), int(ssaa), a.data_ptr(), out.data_ptr(), stream_ptr()), "mirres_texture_downsample")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- UV atlas
def pair_triangles(f):
    """Greedy maximal matching of triangles across shared edges, in triangle-index order: triangle t (unmatched) takes, on its first edge k = 0, 1, 2
    that has one, the lowest-index unmatched triangle sharing that edge.  Returns (pairs i64[P,4] = (t, u, a, b) with (a, b) the shared edge as t
    runs it (f[t, k], f[t, k+1]), singles i64[S])."""
    f = np.asarray(f, np.int64)
    T = f.shape[0]
    if T == 0:
        return np.zeros((0, 4), np.int64), np.zeros(0, np.int64)
    a = f.reshape(-1); b = f[:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * (int(f.max()) + 1) + hi
    key[lo == hi] = -1 - np.arange(int((lo == hi).sum()))        # an edge of a degenerate index triple pairs with nothing
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.searchsorted(ks, ks, side="left"); end = np.searchsorted(ks, ks, side="right")
    pos = np.empty(3 * T, np.int64); pos[order] = np.arange(3 * T)
    tri_of = (order // 3).tolist(); st = start[pos].tolist(); en = end[pos].tolist()
    matched = [False] * T
    pairs = []
    for t in range(T):
        if matched[t]:
            continue
        for k in range(3):
            s, e = st[3 * t + k], en[3 * t + k]
            if e - s < 2:
                continue
            u = -1
            for j in range(s, e):
                c = tri_of[j]
                if c != t and not matched[c]:
                    u = c
                    break
            if u >= 0:
                matched[t] = matched[u] = True
                pairs.append((t, u, int(f[t, k]), int(f[t, (k + 1) % 3])))
                break
    pairs = np.array(pairs, np.int64).reshape(-1, 4)
    singles = np.nonzero(~np.array(matched, bool))[0].astype(np.int64)
    return pairs, singles


def _shelf_pack(S, w0, h0, gap=CELL_GAP):
    """Cells of side S (export texels) on shelves, largest first (stable): origins (x, y) i64 or None when they do not fit w0 x h0."""
    n = S.shape[0]
    order = np.argsort(-S, kind="stable"); s = S[order]
    cum = np.concatenate(([0], np.cumsum(s + gap)))
    x = np.empty(n, np.int64); y = np.empty(n, np.int64)
    i = 0; ycur = 0
    while i < n:
        if s[i] > w0 or ycur + s[i] > h0:
            return None
        j = max(int(np.searchsorted(cum, cum[i] + w0 + gap, side="right")) - 1, i + 1)
        x[order[i:j]] = cum[i:j] - cum[i]; y[order[i:j]] = ycur
        ycur += int(s[i]) + gap; i = j
    return x, y


def uv_atlas(v, f, h0, w0):
    """Deterministic UV atlas in the reference's convention (texel (r, c) centred at ((c + 0.5) / w0, (r + 0.5) / h0), before the OBJ's 1 - v flip).
    Triangles are paired across shared edges (pair_triangles); a pair fills one square cell whose diagonal is the shared edge (the same two UV points
    in both triangles: no seam inside the pair), an unpaired triangle the lower-right half of a cell of its own.  Cell side in export texels:
    max(2, ceil(density x longest 3D edge of the cell)); cells sit on the export-texel grid, CELL_GAP texels apart, shelf-packed by side (largest first);
    `density` is the largest (by bisection) whose packing fits w0 x h0.  Returns (vt f32[Nt,2], ft i32[T,3], fill = cell area / texture area)."""
    v = np.asarray(v, np.float64); f = np.asarray(f, np.int64)
    T = f.shape[0]
    _check_sizes(T, h0, w0, 1)
    pairs, singles = pair_triangles(f)
    P, Sg = pairs.shape[0], singles.shape[0]
    elen = lambda t: np.linalg.norm(v[f[t][:, [1, 2, 0]]] - v[f[t]], axis=-1).max(axis=-1) if len(t) else np.zeros(0)
    L = np.concatenate((np.maximum(elen(pairs[:, 0]), elen(pairs[:, 1])), elen(singles)))
    L = np.where(np.isfinite(L), L, 0.0)
    side = lambda d: np.maximum(2, np.ceil(d * L)).astype(np.int64)
    packed = _shelf_pack(side(0.0), w0, h0)
    if packed is None:
        raise ValueError("uv_atlas: %d cells do not fit a %d x %d texture even at the smallest cell size" % (P + Sg, w0, h0))
    lo = 0.0
    if L.size and L.max() > 0:
        hi = 2.0 * math.sqrt(w0 * h0 / float((L * L).sum()))
        for _ in range(64):
            if _shelf_pack(side(hi), w0, h0) is None:
                break
            lo, hi = hi, 2.0 * hi
        for _ in range(48):
            mid = 0.5 * (lo + hi)
            if _shelf_pack(side(mid), w0, h0) is None:
                hi = mid
            else:
                lo = mid
            if hi - lo <= 1e-7 * hi:
                break
        packed = _shelf_pack(side(lo), w0, h0)
    S = side(lo); x, y = packed
    vt, ft = _cell_uvs(f, pairs, singles, S, x, y, w0, h0)
    fill = float((S[:P] ** 2).sum() + 0.5 * (S[P:] ** 2).sum()) / float(w0 * h0)
    return vt, ft.astype(np.int32), fill


def _cell_uvs(f, pairs, singles, S, x, y, w0, h0):
    """UVs of pair and single cells (sides S, origins (x, y) in export texels; the pairs' cells first): vt f32[4 P + 3 Sg, 2] and ft i64[T,3], of which
    only the rows of the faces in `pairs` / `singles` are set."""
    P, Sg = pairs.shape[0], singles.shape[0]
    # corners of a cell: A (x, y), B (x + S, y + S) on the diagonal, C (x + S, y) below it, D (x, y + S) above it
    corner = lambda dx, dy, sel: np.stack(((x[sel] + dx * S[sel]) / w0, (y[sel] + dy * S[sel]) / h0), -1)
    ps, ss = np.arange(P), P + np.arange(Sg)
    vt = np.concatenate((np.stack((corner(0, 0, ps), corner(1, 1, ps), corner(1, 0, ps), corner(0, 1, ps)), 1).reshape(-1, 2),
                         np.stack((corner(0, 0, ss), corner(1, 0, ss), corner(1, 1, ss)), 1).reshape(-1, 2))).astype(np.float32)
    ft = np.empty((f.shape[0], 3), np.int64)
    if P:
        t, u, a, b = pairs.T
        base = 4 * np.arange(P)
        for tri, other in ((t, base + 2), (u, base + 3)):          # t's third vertex -> C, u's -> D
            ft[tri] = other[:, None]
            ft[tri] = np.where(f[tri] == a[:, None], base[:, None], ft[tri])
            ft[tri] = np.where(f[tri] == b[:, None], base[:, None] + 1, ft[tri])
    if Sg:
        ft[singles] = 4 * P + 3 * np.arange(Sg)[:, None] + np.arange(3)[None, :]
    return vt, ft


# ------------------------------------------------------------------------------------------------------------------------------- chart atlas
N_BUCKETS = 6                  # +x, -x, +y, -y, +z, -z (include/mirres.h)


def seam_edges(f, ft):
    """How many mesh edges carried by exactly two faces are UV seams: the two faces do not use the same two UV vertices along it.  Boundary edges and
    edges of more than two faces are not counted; a face with a repeated index carries no edge.  One rule for every atlas."""
    f = np.asarray(f, np.int64).reshape(-1, 3); ft = np.asarray(ft, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return 0
    a = f.reshape(-1); b = f[:, [1, 2, 0]].reshape(-1); ua = ft.reshape(-1); ub = ft[:, [1, 2, 0]].reshape(-1)
    swap = a > b
    lo, hi = np.where(swap, b, a), np.where(swap, a, b)
    ulo, uhi = np.where(swap, ub, ua), np.where(swap, ua, ub)
    ok = (lo != hi) & ~(f[:, [0, 0, 1]] == f[:, [1, 2, 2]]).any(1).repeat(3)
    lo, hi, ulo, uhi = lo[ok], hi[ok], ulo[ok], uhi[ok]
    order = np.lexsort((hi, lo))
    lo, hi, ulo, uhi = lo[order], hi[order], ulo[order], uhi[order]
    new = np.concatenate(([True], (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])))
    start = np.nonzero(new)[0]; count = np.diff(np.concatenate((start, [lo.shape[0]])))
    s2 = start[count == 2]
    return int(((ulo[s2] != ulo[s2 + 1]) | (uhi[s2] != uhi[s2 + 1])).sum())


def _pack_rects(w, h, w0, h0, gap=CELL_GAP):
    """Rectangles w x h (export texels) on shelves, tallest first (stable), `gap` texels apart: origins (x, y) i64 or None when they do not fit w0 x h0."""
    n = w.shape[0]
    x = np.empty(n, np.int64); y = np.empty(n, np.int64)
    if n and int(w.max()) > w0:
        return None
    order = np.argsort(-h, kind="stable"); ws = w[order]; hs = h[order]
    cum = np.concatenate(([0], np.cumsum(ws + gap)))
    i = 0; ycur = 0
    while i < n:
        if ycur + hs[i] > h0:
            return None
        j = max(int(np.searchsorted(cum, cum[i] + w0 + gap, side="right")) - 1, i + 1)
        x[order[i:j]] = cum[i:j] - cum[i]; y[order[i:j]] = ycur
        ycur += int(hs[i]) + gap; i = j
    return x, y


@torch.no_grad()
def atlas_classify(v, f):
    """mirres_atlas_classify: (normal f32[T,3], bucket i32[T]) of device tensors v f32[V,3], f i32[T,3]."""
    T = int(f.shape[0])
    normal = torch.empty((T, 3), dtype=torch.float32, device=f.device); bucket = torch.empty(T, dtype=torch.int32, device=f.device)
    check(lib().mirres_atlas_classify(_lib.ptr(v) if v.numel() else None, int(v.shape[0]), _lib.ptr(f) if T else None, T, _lib.ptr(normal) if T else None,
                                      _lib.ptr(bucket) if T else None, stream_ptr()), "mirres_atlas_classify")
    return normal, bucket


@torch.no_grad()
def manifold_neighbours(f, V):
    """nbr i32[T,3] of device triangles f i32[T,3]: the face across edge (v_k, v_k+1) when exactly two face corners carry that edge, else -1.  A corner's edge
    counts when its two indices differ and lie in [0, V)."""
    T = int(f.shape[0])
    t64 = f.to(torch.int64)
    a = t64.reshape(-1); b = t64[:, [1, 2, 0]].reshape(-1)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    corner = torch.nonzero((lo != hi) & (lo >= 0) & (hi < V)).squeeze(1)
    keys, order = torch.sort((lo[corner] << 32) | hi[corner], stable=True)
    corner = corner[order]
    nbr = torch.full((3 * T,), -1, dtype=torch.int32, device=f.device)
    if keys.numel():
        _, inv, counts = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
        start = (torch.cumsum(counts, 0) - counts)[inv]
        pos = torch.arange(keys.shape[0], device=f.device)
        two = counts[inv] == 2
        partner = torch.where(pos == start, pos + 1, pos - 1)[two]
        nbr[corner[two]] = (corner[partner] // 3).to(torch.int32)
    return nbr.reshape(T, 3)


@torch.no_grad()
def atlas_smooth(normal, bucket, nbr, cos_min):
    """mirres_atlas_smooth: one relabelling round -> a new bucket tensor."""
    T = int(bucket.shape[0])
    out = torch.empty_like(bucket)
    check(lib().mirres_atlas_smooth(_lib.ptr(normal) if T else None, _lib.ptr(bucket) if T else None, _lib.ptr(nbr.contiguous()) if T else None, T, float(cos_min),
                                    _lib.ptr(out) if T else None, stream_ptr()), "mirres_atlas_smooth")
    return out


@torch.no_grad()
def atlas_charts(f, V, bucket, nbr):
    """(chart i32[T], n_charts): the connected components of faces joined across manifold edges whose two faces hold one bucket (mirres_mesh_components on edge
    keys whose lower vertex id carries the bucket), numbered in the order of each chart's smallest face; -1 for a degenerate face (bucket -1)."""
    T = int(f.shape[0])
    chart = torch.full((T,), -1, dtype=torch.int32, device=f.device)
    if T == 0:
        return chart, 0
    if N_BUCKETS * V >= 1 << 31:
        raise ValueError("chart_atlas: %d vertices: the edge keys carry the bucket in the vertex id (fewer than 2^31 / 6 vertices)" % V)
    t64 = f.to(torch.int64)
    a = t64.reshape(-1); b = t64[:, [1, 2, 0]].reshape(-1)
    bk = bucket.to(torch.int64).repeat_interleave(3)
    corner = torch.nonzero((nbr.reshape(-1) >= 0) & (bk >= 0)).squeeze(1)
    lo, hi = torch.minimum(a[corner], b[corner]), torch.maximum(a[corner], b[corner])
    keys, order = torch.sort(((bk[corner] * V + lo) << 32) | hi, stable=True)
    face = (corner[order] // 3).to(torch.int32).contiguous(); keys = keys.contiguous()
    label = torch.empty(T, dtype=torch.int32, device=f.device)
    flag = torch.zeros(1, dtype=torch.int32, device=f.device)
    check(lib().mirres_mesh_components(_lib.ptr(keys) if keys.numel() else None, _lib.ptr(face) if keys.numel() else None, int(keys.shape[0]), T, _lib.ptr(label),
                                       _lib.ptr(flag), 0, None, stream_ptr()), "mirres_mesh_components")
    good = bucket >= 0
    roots = torch.unique(label[good])                                        # ascending = by smallest face
    chart[good] = torch.searchsorted(roots, label[good]).to(torch.int32)
    return chart, int(roots.shape[0])


@torch.no_grad()
def atlas_bounds(v, f, bucket, chart, n_charts):
    """mirres_atlas_bounds: f32[n_charts,4] = (min U, min V, max U, max V) of every chart's projected vertices."""
    T = int(f.shape[0])
    bounds = torch.empty((n_charts, 4), dtype=torch.float32, device=f.device)
    check(lib().mirres_atlas_bounds(_lib.ptr(v) if v.numel() else None, int(v.shape[0]), _lib.ptr(f) if T else None, T, _lib.ptr(bucket) if T else None,
                                    _lib.ptr(chart) if T else None, n_charts, _lib.ptr(bounds) if n_charts else None, stream_ptr()), "mirres_atlas_bounds")
    return bounds


@torch.no_grad()
def atlas_emit(v, uv_chart, uv_vertex, chart_bucket, bounds, origin, density, w0, h0):
    """mirres_atlas_emit: vt f32[n_uv,2] of the (chart, mesh vertex) pairs."""
    n_uv = int(uv_chart.shape[0]); n_charts = int(chart_bucket.shape[0])
    vt = torch.empty((n_uv, 2), dtype=torch.float32, device=v.device)
    p = lambda t: _lib.ptr(t.contiguous()) if t.numel() else None
    check(lib().mirres_atlas_emit(p(v), int(v.shape[0]), p(uv_chart), p(uv_vertex), n_uv, p(chart_bucket), p(bounds), p(origin), n_charts, float(density), int(w0), int(h0),
                                  p(vt), stream_ptr()), "mirres_atlas_emit")
    return vt


@torch.no_grad()
def atlas_verify(vt, ft, face_chart, n_charts, W, H):
    """mirres_atlas_verify on the W x H bake grid: flagged u8[n_charts + 1] (device), the last entry for the faces of no chart."""
    dev = torch.device("cuda")
    uv = torch.as_tensor(vt, dtype=torch.float32).to(dev).contiguous(); t = torch.as_tensor(ft).to(dev, torch.int32).contiguous()
    fc = torch.as_tensor(face_chart).to(dev, torch.int32).contiguous()
    T = int(t.shape[0])
    if fc.shape[0] != T:
        raise ValueError("atlas_verify: %d chart labels for %d faces" % (fc.shape[0], T))
    nbytes = int(lib().mirres_atlas_verify_scratch(T, int(W), int(H)))
    if nbytes < 0:
        raise ValueError("atlas_verify: %d triangles on a %d x %d grid are out of range" % (T, W, H))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    flagged = torch.empty(n_charts + 1, dtype=torch.uint8, device=dev)
    check(lib().mirres_atlas_verify(uv.data_ptr() if T else None, int(uv.shape[0]), t.data_ptr() if T else None, T, fc.data_ptr() if T else None, int(n_charts), int(W), int(H),
                                    flagged.data_ptr(), scratch.data_ptr(), nbytes, stream_ptr()), "mirres_atlas_verify")
    return flagged


def _chart_layout(v, f, fallback, bounds, h0, w0):
    """The host step of chart_atlas: one density for the chart rectangles (ceil(extent x density) + 1 texels a side, extent and product in fp32) and the
    fallback faces' pair / single cells (max(2, ceil(density x longest edge))), shelf-packed together; the density (an fp32 number) is the largest, by
    bisection as in uv_atlas, whose packing fits.  Returns (density, chart origins i64[C,2], cell vt, cell ft rows i64[T,3])."""
    C = bounds.shape[0]
    ext = (bounds[:, 2:4] - bounds[:, 0:2]).astype(np.float32) if C else np.zeros((0, 2), np.float32)
    if not np.isfinite(ext).all():
        raise ValueError("chart_atlas: a chart without finite bounds")
    fl = f[fallback]
    fl = np.where(((fl >= 0) & (fl < v.shape[0])).all(1, keepdims=True), fl, 0)       # a face with an index out of range: a single cell of the smallest size
    pairs, singles = pair_triangles(fl)
    elen = lambda t: np.linalg.norm(v[fl[t][:, [1, 2, 0]]] - v[fl[t]], axis=-1).max(axis=-1) if len(t) else np.zeros(0)
    L = np.concatenate((np.maximum(elen(pairs[:, 0]), elen(pairs[:, 1])), elen(singles)))
    L = np.where(np.isfinite(L), L, 0.0)

    def sizes(d):
        s = np.float32(d)
        wh = np.ceil(ext * s).astype(np.int64) + 1
        S = np.maximum(2, np.ceil(float(s) * L)).astype(np.int64)
        return np.concatenate((wh[:, 0], S)), np.concatenate((wh[:, 1], S))
    fits = lambda d: _pack_rects(*sizes(d), w0, h0)
    packed = fits(0.0)
    if packed is None:
        raise ValueError("chart_atlas: %d charts and %d cells do not fit a %d x %d texture even at the smallest size" % (C, L.shape[0], w0, h0))
    lo = 0.0
    area = float((ext[:, 0].astype(np.float64) * ext[:, 1]).sum() + (L * L).sum())
    if area > 0:
        hi = 2.0 * math.sqrt(w0 * h0 / area)
        for _ in range(64):
            if fits(hi) is None:
                break
            lo, hi = hi, 2.0 * hi
        for _ in range(48):
            mid = 0.5 * (lo + hi)
            if fits(mid) is None:
                hi = mid
            else:
                lo = mid
            if hi - lo <= 1e-7 * hi:
                break
        packed = fits(lo)                                                              # sizes() rounds the density to fp32 itself
    w, h = sizes(lo); x, y = packed
    cell_vt, cell_ft = _cell_uvs(fl, pairs, singles, w[C:], x[C:], y[C:], w0, h0)
    ft_rows = np.full((f.shape[0], 3), -1, np.int64)
    ft_rows[fallback] = cell_ft
    return np.float32(lo), np.stack((x[:C], y[:C]), 1), cell_vt, ft_rows


@torch.no_grad()
def chart_atlas(v, f, h0, w0, ssaa=1, cos_min=0.5, smooth_rounds=2):
    """UV atlas of axis-projected charts (DESIGN.md section 5.7 "Chart atlas"; the rules are written out in include/mirres.h), in uv_atlas's
    conventions.  On the device: face normals and buckets (the axis direction a face looks along), `smooth_rounds` relabelling rounds, charts = connected faces of one bucket across
    manifold edges, per-chart bounds, one UV vertex per (chart, mesh vertex), and the overlap check on the (h0 ssaa) x (w0 ssaa) bake grid.  On the host:
    the shelf packing at one shared density.  Degenerate faces and the faces of charts the check flags (a chart that projects onto itself) fall back to
    uv_atlas's pair / single cells; after that second packing the check must pass.  Returns (vt f32[Nt,2], ft i32[T,3], info): fill (UV area of the
    triangles), density (export texels per world unit), n_charts, fallback_faces, seam_edges, face_chart i32[T] (-1 = fallback), host_s."""
    vn = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1, 3)); fn = np.ascontiguousarray(np.asarray(f, np.int64).reshape(-1, 3))
    T, V = fn.shape[0], vn.shape[0]
    _check_sizes(T, h0, w0, ssaa)
    if not 0.0 <= float(cos_min) <= 1.0 or int(smooth_rounds) < 0:
        raise ValueError("chart_atlas: cos_min in [0, 1] and smooth_rounds >= 0 (got %s, %s)" % (cos_min, smooth_rounds))
    if T and (fn.max() >= 1 << 31 or fn.min() < -(1 << 31)):
        raise ValueError("chart_atlas: a face index does not fit 32 bits")
    dev = torch.device("cuda")
    vd = torch.from_numpy(vn).to(dev); fd = torch.from_numpy(fn).to(dev, torch.int32).contiguous()
    normal, bucket = atlas_classify(vd, fd)
    nbr = manifold_neighbours(fd, V)
    for _ in range(int(smooth_rounds)):
        bucket = atlas_smooth(normal, bucket, nbr, cos_min)
    chart, n_charts = atlas_charts(fd, V, bucket, nbr)
    host_s = 0.0
    v64 = vn.astype(np.float64)
    for attempt in (0, 1):
        bounds = atlas_bounds(vd, fd, bucket, chart, n_charts)
        chart_np = chart.cpu().numpy()
        t0 = time.perf_counter()
        density, origin, cell_vt, ft_rows = _chart_layout(v64, fn, np.nonzero(chart_np < 0)[0], bounds.cpu().numpy(), h0, w0)
        host_s += time.perf_counter() - t0
        faces = torch.nonzero(chart >= 0).squeeze(1)
        pair_key, inv = torch.unique((chart[faces].to(torch.int64)[:, None] * max(V, 1) + fd[faces].to(torch.int64)).reshape(-1), return_inverse=True)
        first = torch.full((n_charts,), T, dtype=torch.int64, device=dev).scatter_reduce(0, chart[faces].long(), faces, "amin")
        vt_c = atlas_emit(vd, (pair_key // max(V, 1)).to(torch.int32), (pair_key % max(V, 1)).to(torch.int32), bucket[first], bounds,
                          torch.from_numpy(origin).to(dev, torch.int32), density, w0, h0)
        ft = torch.from_numpy(ft_rows).to(dev) + int(pair_key.shape[0])
        ft[faces] = inv.reshape(-1, 3)
        vt = torch.cat((vt_c, torch.from_numpy(cell_vt).to(dev).reshape(-1, 2)))
        ft = ft.to(torch.int32)
        flagged = atlas_verify(vt, ft, chart, n_charts, w0 * ssaa, h0 * ssaa).bool()
        if not bool(flagged.any()):
            break
        if attempt or bool(flagged[n_charts]):
            raise RuntimeError("chart_atlas: the layout still covers a bake texel twice after the fallback (%d charts flagged)" % int(flagged.sum()))
        keep = ~flagged[:n_charts]                                                  # the flagged charts' faces join the fallback; the rest stay in order
        new_id = torch.where(keep, torch.cumsum(keep, 0) - 1, -1).to(torch.int32)
        chart = torch.where(chart >= 0, new_id[chart.clamp(min=0).long()], chart)
        n_charts = int(keep.sum())
    vt_np, ft_np, chart_np = vt.cpu().numpy(), ft.cpu().numpy(), chart.cpu().numpy()
    q = vt_np[ft_np.astype(np.int64)].astype(np.float64) if T else np.zeros((0, 3, 2))
    fill = float(0.5 * np.abs((q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])).sum())
    info = {"fill": fill, "density": float(density), "n_charts": n_charts, "fallback_faces": int((chart_np < 0).sum()), "seam_edges": seam_edges(fn, ft_np),
            "face_chart": chart_np.astype(np.int32), "host_s": host_s}
    return vt_np, ft_np, info


# ------------------------------------------------------------------------------------------------------------------------------------- bake
def _sync_time(events, name):
    if events is not None:
        e = torch.cuda.Event(enable_timing=True); e.record()
        events.append((name, e, time.perf_counter()))


@torch.no_grad()
def bake_textures(field, v, f, vt, ft, h0, w0, ssaa, keep=False, events=None):
    """renderer.py:349-422 for one cascade: rasterise the atlas at (h0 ssaa) x (w0 ssaa), interpolate the 3D positions (raster.interpolate), evaluate
    `field` (xyz f32[n,3] -> f32[n,6]; MLPTexture3D.sample_no_di in export_stage1) on the covered texels, quantise, inpaint, downsample.
    Returns {"feat": (feat0, feat1) u8[h0, w0, 3] on the device, "fill": covered fraction}; with keep=True also the intermediate arrays.
    `events`: a list that receives (stage, cuda event, host time) after each stage (scripts/dev_export_time.py)."""
    T = int(np.asarray(ft.shape)[0])
    _check_sizes(T, h0, w0, ssaa)
    dev = torch.device("cuda")
    H, W = int(h0) * int(ssaa), int(w0) * int(ssaa)
    vd = torch.as_tensor(v, dtype=torch.float32).to(dev).contiguous(); fd = torch.as_tensor(f).to(dev, torch.int32).contiguous()
    _sync_time(events, "start")
    rast = uv_rasterize(vt, ft, W, H)
    _sync_time(events, "uv_rasterize")
    covered = rast[:, 3] > 0
    index = torch.nonzero(covered).squeeze(1).to(torch.int32)
    n = int(index.shape[0])
    xyz = raster.interpolate(vd, rast.index_select(0, index.long()), fd) if n else torch.zeros((0, 3), device=dev)
    _sync_time(events, "interpolate")
    feats = torch.empty((n, 6), dtype=torch.float32, device=dev)
    for s in range(0, n, FIELD_BATCH):
        feats[s:s + FIELD_BATCH] = field(xyz[s:s + FIELD_BATCH]).float()
    _sync_time(events, "field")
    q0, q1 = bake_quantise(feats, index, W, H)
    _sync_time(events, "quantise")
    mask = covered.to(torch.uint8)
    p0, p1 = texture_inpaint(mask, q0, q1, W, H)
    _sync_time(events, "inpaint")
    feat = (texture_downsample(p0, W, H, ssaa), texture_downsample(p1, W, H, ssaa))
    _sync_time(events, "downsample")
    out = {"feat": feat, "fill": n / float(H * W)}
    if keep:
        out.update(rast=rast, index=index, xyz=xyz, feats=feats, quant=(q0, q1), mask=mask, inpaint=(p0, p1))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------- files
def _fmt(x):
    return np.asarray(x, np.float32).astype(np.float64).ravel().tolist()


def write_obj(path, v, vt, f, ft, cas=0):
    """renderer.py:431-452: `mtllib mesh_{cas}.mtl`, `v x y z`, `vt u (1 - v)`, `usemtl defaultMat`, `f a/at b/bt c/ct` (1-based), each line ending in
    ' \\n' as the reference writes it.  Floats with 9 significant digits: every float32 reads back to itself."""
    v = np.asarray(v, np.float32).reshape(-1, 3); vt = np.asarray(vt, np.float32).reshape(-1, 2)
    f = np.asarray(f, np.int64).reshape(-1, 3); ft = np.asarray(ft, np.int64).reshape(-1, 3)
    if f.shape != ft.shape:
        raise ValueError("write_obj: f %s and ft %s differ" % (f.shape, ft.shape))
    vt_out = np.stack((vt[:, 0], np.float32(1) - vt[:, 1]), 1)
    idx = np.stack((f + 1, ft + 1), -1).reshape(-1).tolist()
    with open(path, "w") as fp:
        fp.write("mtllib mesh_%d.mtl \n" % cas)
        fp.write(("v %.9g %.9g %.9g \n" * v.shape[0]) % tuple(_fmt(v)))
        fp.write(("vt %.9g %.9g \n" * vt_out.shape[0]) % tuple(_fmt(vt_out)))
        fp.write("usemtl defaultMat \n")
        fp.write(("f %d/%d %d/%d %d/%d \n" * f.shape[0]) % tuple(idx))
    return path


def write_mtl(path, cas=0):
    """renderer.py:454-462 (the texture named .png: the one deviation from the reference)."""
    with open(path, "w") as fp:
        fp.write("newmtl defaultMat \nKa 1 1 1 \nKd 1 1 1 \nKs 0 0 0 \nTr 1 \nillum 1 \nNs 0 \nmap_Kd feat0_%d.png \n" % cas)
    return path


def read_obj(path):
    """v f32[V,3], vt f32[Nt,2] as written (the file's v'), f i32[T,3], ft i32[T,3] (0-based; -1 where a face corner has no UV) of a triangle OBJ."""
    v, vt, f, ft = [], [], [], []
    with open(path) as fp:
        for line in fp:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "vt":
                vt.append([float(x) for x in p[1:3]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError("%s: only triangles are read (%r)" % (path, line.strip()))
                c = [q.split("/") for q in p[1:4]]
                f.append([int(q[0]) - 1 for q in c]); ft.append([int(q[1]) - 1 if len(q) > 1 and q[1] else -1 for q in c])
    return (np.array(v, np.float32).reshape(-1, 3), np.array(vt, np.float32).reshape(-1, 2), np.array(f, np.int32).reshape(-1, 3),
            np.array(ft, np.int32).reshape(-1, 3))


def uv_from_obj(path, f=None):
    """A UV layout made elsewhere (e.g. xatlas) read from an OBJ -> (vt, ft) in the reference's convention (v = 1 - v').  When `f` is given the OBJ's
    faces must be the same triangles in the same order."""
    _, vt, fo, ft = read_obj(path)
    if (ft < 0).any():
        raise ValueError("%s: faces without texture coordinates" % path)
    if f is not None and not np.array_equal(np.asarray(f, np.int64), fo.astype(np.int64)):
        raise ValueError("%s: its faces are not the mesh's triangles (%d vs %d)" % (path, fo.shape[0], np.asarray(f).shape[0]))
    return np.stack((vt[:, 0], np.float32(1) - vt[:, 1]), 1).astype(np.float32), ft


def cascade_sizes(texture_size, cascades):
    """(h0, w0) per cascade: renderer.py:473-476 halves both after a cascade while both are > 2048 (non-SDF)."""
    h0 = w0 = int(texture_size); out = []
    for _ in range(cascades):
        out.append((h0, w0))
        if h0 > 2048 and w0 > 2048:
            h0 //= 2; w0 //= 2
    return out


def export_stage1(path, vertices, triangles, v_cumsum, f_cumsum, mlp, texture_size=4096, ssaa=2, uv=None, field=None, log=print, atlas="pairs"):
    """NeRFRenderer.export_stage1 (renderer.py:319-476) with h0 = w0 = texture_size (Trainer.export_stage1(resolution=opt.texture_size)):
    per cascade `mesh_{cas}.obj`, `mesh_{cas}.mtl`, `feat0_{cas}.png`, `feat1_{cas}.png` under `path`.  vertices f32[V,3] already include the
    stage-1 offsets (act_voffsets is the identity); v_cumsum / f_cumsum slice the cascades (CK.load_stage0_mesh).  `uv`: a list of (vt, ft) per
    cascade (or one pair for a one-cascade mesh) to bake onto instead of the built-in atlas; `atlas`: which built-in one, "pairs" (uv_atlas) or "charts"
    (chart_atlas).  `field` defaults to mlp.sample_no_di.  Returns the files."""
    if atlas not in ("pairs", "charts"):
        raise ValueError("export_stage1: atlas is 'pairs' or 'charts', got %r" % (atlas,))
    v_cumsum = [int(x) for x in v_cumsum]; f_cumsum = [int(x) for x in f_cumsum]
    ncas = len(v_cumsum) - 1
    if ncas < 1 or len(f_cumsum) != ncas + 1:
        raise ValueError("export_stage1: v_cumsum / f_cumsum describe no cascade")
    sizes = cascade_sizes(texture_size, ncas)
    for cas in range(ncas):
        _check_sizes(f_cumsum[cas + 1] - f_cumsum[cas], sizes[cas][0], sizes[cas][1], ssaa)
    if uv is not None and isinstance(uv, tuple):
        uv = [uv]
    if uv is not None and len(uv) != ncas:
        raise ValueError("export_stage1: %d UV layouts for %d cascades" % (len(uv), ncas))
    field = field if field is not None else mlp.sample_no_di
    V = torch.as_tensor(vertices).detach().float().cpu().numpy(); F = torch.as_tensor(triangles).detach().cpu().numpy().astype(np.int64)
    os.makedirs(path, exist_ok=True)
    files = []
    for cas in range(ncas):
        h0, w0 = sizes[cas]
        v = V[v_cumsum[cas]:v_cumsum[cas + 1]]; f = F[f_cumsum[cas]:f_cumsum[cas + 1]] - v_cumsum[cas]
        if uv is None and atlas == "charts":
            vt, ft, info = chart_atlas(v, f, h0, w0, ssaa)
            note = "chart atlas fill %.3f, %d charts, %d fallback faces, %d seam edges" % (info["fill"], info["n_charts"], info["fallback_faces"], info["seam_edges"])
        elif uv is None:
            vt, ft, fill = uv_atlas(v, f, h0, w0)
            note = "atlas fill %.3f" % fill
        else:
            vt, ft = (np.asarray(a) for a in uv[cas]); note = "given UVs"
            if ft.shape != f.shape:
                raise ValueError("export_stage1: cascade %d has %d triangles, its UV layout %d" % (cas, f.shape[0], ft.shape[0]))
        r = bake_textures(field, v, f, vt, ft, h0, w0, ssaa)
        for k in (0, 1):
            files.append(os.path.join(path, "feat%d_%d.png" % (k, cas)))
            meters.write_png(files[-1], r["feat"][k].cpu().numpy())
        files.append(write_obj(os.path.join(path, "mesh_%d.obj" % cas), v, vt, f, ft, cas))
        files.append(write_mtl(os.path.join(path, "mesh_%d.mtl" % cas), cas))
        if log:
            log("[export] cascade %d: v=%d f=%d, %dx%d (ssaa %d), %s, texel coverage %.3f -> %s" % (cas, v.shape[0], f.shape[0], w0, h0, ssaa, note,
                                                                                              r["fill"], files[-2]))
    return files


# ------------------------------------------------------------------------------------------------------------------- the asset read back
def srgb_decode_table():
    """decode[q] = srgb_to_linear(q / 255) (harness.srgb_to_linear): what a viewer does with an 8-bit sRGB texture.  The bake truncates when it
    quantises (mirres_bake_quantise), so the decoded value sits up to one LSB below the field's value, half an LSB on average."""
    from .harness import srgb_to_linear
    return srgb_to_linear(torch.arange(256, dtype=torch.float32) / 255.0).to(torch.float32)


class TexturedMaterial:
    """The exported stage-1 asset as a material source of the renderer (mirres_texmat_t): the concatenated render mesh (build the BVH from `verts` /
    `tris`), per-corner UVs in the reference's convention (v = 1 - v'), and per cascade one packed texel plane u8[H, W, 8] = (kd.rgb, roughness,
    metallic, 0, 0, 0) of the 8-bit sRGB bytes.  There is no gradient path through a lookup: training and the stepwise loop refuse it."""
    is_textured = True

    def __init__(self, verts, tris, vt, ft, tri_end, planes, roughness_min=0.08, device="cuda"):
        if not 1 <= len(planes) <= 8 or len(tri_end) != len(planes):
            raise ValueError("TexturedMaterial: 1 to 8 cascades, one triangle range each (%d planes, %d ranges)" % (len(planes), len(tri_end)))
        dev = torch.device(device)
        self.verts = torch.as_tensor(verts, dtype=torch.float32).to(dev).contiguous()
        self.tris = torch.as_tensor(tris).to(dev, torch.int32).contiguous()
        self.vt = torch.as_tensor(vt, dtype=torch.float32).to(dev).contiguous()
        self.ft = torch.as_tensor(ft).to(dev, torch.int32).contiguous()
        self.tri_end = [int(x) for x in tri_end]
        self.planes = [torch.as_tensor(p).to(dev, torch.uint8).contiguous() for p in planes]
        for p in self.planes:
            if p.dim() != 3 or p.shape[2] != 8:
                raise ValueError("TexturedMaterial: a texel plane is u8[H, W, 8], got %s" % (tuple(p.shape),))
        self.decode = srgb_decode_table().to(dev).contiguous()
        self.roughness_min = float(roughness_min)
        self.n_cas = len(self.planes)
        self._st = None

    def _struct(self):
        if self._st is None:
            st = _lib.TexMat()
            st.verts, st.tris, st.vt, st.ft = (t.data_ptr() for t in (self.verts, self.tris, self.vt, self.ft))
            st.n_cas = self.n_cas
            for c, p in enumerate(self.planes):
                st.tri_end[c] = self.tri_end[c]; st.H[c] = int(p.shape[0]); st.W[c] = int(p.shape[1]); st.texels[c] = p.data_ptr()
            st.decode = self.decode.data_ptr(); st.rough_min = self.roughness_min
            self._st = st
        return self._st

    @torch.no_grad()
    def lookup(self, prim, pos, occ=None, kd=None, rough_metal=None, use_scale=False, scale=(1.0, 1.0, 1.0)):
        """mirres_texmat_lookup: rows with occ >= 0.5 (all when occ is None) get kd f32[n,3] / (roughness, metallic) f32[n,2] of the texel under
        `pos` on triangle `prim`; other rows of `kd` / `rough_metal` (given or zeros) are left as they are, apart from the use_scale clamp of kd."""
        n = int(prim.shape[0])
        dev = self.verts.device
        prim = prim.to(dev, torch.int32).contiguous(); pos = pos.to(dev, torch.float32).contiguous()
        if pos.numel() != 3 * n or (occ is not None and occ.numel() != n):
            raise ValueError("TexturedMaterial.lookup: prim [%d], pos %s, occ %s" % (n, tuple(pos.shape), None if occ is None else tuple(occ.shape)))
        occ = occ.to(dev, torch.float32).contiguous() if occ is not None else None
        kd = torch.zeros((n, 3), dtype=torch.float32, device=dev) if kd is None else kd
        rough_metal = torch.zeros((n, 2), dtype=torch.float32, device=dev) if rough_metal is None else rough_metal
        for t, w in ((kd, 3), (rough_metal, 2)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != w * n:
                raise ValueError("TexturedMaterial.lookup: outputs are contiguous f32[n, 3] / f32[n, 2]")
        s3 = (C.c_float * 3)(*[float(x) for x in scale])
        check(lib().mirres_texmat_lookup(C.byref(self._struct()), occ.data_ptr() if occ is not None else None, prim.data_ptr(), pos.data_ptr(), n,
                                         kd.data_ptr(), rough_metal.data_ptr(), int(bool(use_scale)), s3, stream_ptr()), "mirres_texmat_lookup")
        return kd, rough_metal


def _read_texture(path_base):
    from PIL import Image
    for ext in (".png", ".jpg", ".jpeg"):
        if os.path.exists(path_base + ext):
            return np.asarray(Image.open(path_base + ext).convert("RGB"), np.uint8), path_base + ext
    raise FileNotFoundError("%s.png / .jpg: no such texture" % path_base)


def load_stage1(path, cascades=None, roughness_min=0.08, device="cuda"):
    """The stage-1 asset export_stage1 writes (`mesh_{cas}.obj`, `feat0_{cas}`, `feat1_{cas}` as .png or .jpg, e.g. the reference's own JPEG export) ->
    TexturedMaterial.  cascades=None: every cascade found from 0 on.  Cascades are concatenated with their vertex / UV indices shifted
    (checkpoint.load_stage0_mesh).  Refuses missing files, faces without UVs and feat0 / feat1 of different sizes."""
    if cascades is None:
        cascades = 0
        while os.path.exists(os.path.join(path, "mesh_%d.obj" % cascades)):
            cascades += 1
        if cascades == 0:
            raise FileNotFoundError("%s: no mesh_0.obj" % path)
    vs, vts, fs, fts, planes, tri_end = [], [], [], [], [], []
    nv = nt = nf = 0
    for cas in range(int(cascades)):
        obj = os.path.join(path, "mesh_%d.obj" % cas)
        if not os.path.exists(obj):
            raise FileNotFoundError("%s: no such mesh" % obj)
        v, vt_raw, f, ft = read_obj(obj)
        if f.shape[0] == 0:
            raise ValueError("%s: no faces" % obj)
        if (ft < 0).any():
            raise ValueError("%s: faces without texture coordinates" % obj)
        if f.max() >= v.shape[0] or f.min() < 0 or ft.max() >= vt_raw.shape[0]:
            raise ValueError("%s: a face refers to a vertex or texture coordinate that does not exist" % obj)
        t0, p0 = _read_texture(os.path.join(path, "feat0_%d" % cas))
        t1, p1 = _read_texture(os.path.join(path, "feat1_%d" % cas))
        if t0.shape != t1.shape:
            raise ValueError("%s is %dx%d, %s %dx%d: the two textures of a cascade must have one size" % (p0, t0.shape[1], t0.shape[0], p1, t1.shape[1], t1.shape[0]))
        plane = np.zeros(t0.shape[:2] + (8,), np.uint8)
        plane[..., 0:3] = t0; plane[..., 3] = t1[..., 1]; plane[..., 4] = t1[..., 2]
        vs.append(v); vts.append(np.stack((vt_raw[:, 0], np.float32(1) - vt_raw[:, 1]), 1).astype(np.float32))
        fs.append(f + nv); fts.append(ft + nt)
        nv += v.shape[0]; nt += vt_raw.shape[0]; nf += f.shape[0]
        planes.append(plane); tri_end.append(nf)
    return TexturedMaterial(np.concatenate(vs), np.concatenate(fs).astype(np.int32), np.concatenate(vts), np.concatenate(fts).astype(np.int32), tri_end, planes,
                            roughness_min=roughness_min, device=device)
