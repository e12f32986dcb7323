"""Stage-1 mesh export (nerf/renderer.py:319-476 `NeRFRenderer.export_stage1`, driven by Trainer.export_stage1, nerf/utils.py:1271-1281): per mesh
cascade an OBJ with UVs, its MTL and two baked textures of the material field — feat0 (kd, channels 0-2, the MTL's map_Kd) and feat1 (channels 3-5).

    vt, ft, fill = uv_atlas(v, f, h0, w0)                                   # xatlas in the reference (:334-347): a deterministic pair atlas here
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
    # corners of a cell: A (x, y), B (x + S, y + S) on the diagonal, C (x + S, y) below it, D (x, y + S) above it
    corner = lambda dx, dy, sel: np.stack(((x[sel] + dx * S[sel]) / w0, (y[sel] + dy * S[sel]) / h0), -1)
    ps, ss = np.arange(P), P + np.arange(Sg)
    vt = np.concatenate((np.stack((corner(0, 0, ps), corner(1, 1, ps), corner(1, 0, ps), corner(0, 1, ps)), 1).reshape(-1, 2),
                         np.stack((corner(0, 0, ss), corner(1, 0, ss), corner(1, 1, ss)), 1).reshape(-1, 2))).astype(np.float32)
    ft = np.empty((T, 3), np.int64)
    if P:
        t, u, a, b = pairs.T
        base = 4 * np.arange(P)
        for tri, other in ((t, base + 2), (u, base + 3)):          # t's third vertex -> C, u's -> D
            ft[tri] = other[:, None]
            ft[tri] = np.where(f[tri] == a[:, None], base[:, None], ft[tri])
            ft[tri] = np.where(f[tri] == b[:, None], base[:, None] + 1, ft[tri])
    if Sg:
        ft[singles] = 4 * P + 3 * np.arange(Sg)[:, None] + np.arange(3)[None, :]
    fill = float((S[:P] ** 2).sum() + 0.5 * (S[P:] ** 2).sum()) / float(w0 * h0)
    return vt, ft.astype(np.int32), fill


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


def export_stage1(path, vertices, triangles, v_cumsum, f_cumsum, mlp, texture_size=4096, ssaa=2, uv=None, field=None, log=print):
    """NeRFRenderer.export_stage1 (renderer.py:319-476) with h0 = w0 = texture_size (Trainer.export_stage1(resolution=opt.texture_size)):
    per cascade `mesh_{cas}.obj`, `mesh_{cas}.mtl`, `feat0_{cas}.png`, `feat1_{cas}.png` under `path`.  vertices f32[V,3] already include the
    stage-1 offsets (act_voffsets is the identity); v_cumsum / f_cumsum slice the cascades (CK.load_stage0_mesh).  `uv`: a list of (vt, ft) per
    cascade (or one pair for a one-cascade mesh) to bake onto instead of uv_atlas.  `field` defaults to mlp.sample_no_di.  Returns the files."""
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
        if uv is None:
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
