"""numpy restatement of the textured-material lookup (include/mirres.h above mirres_texmat_lookup; csrc/texmat.hip): fp32 barycentrics by the header's
formula, the UV blend, clamped bilinear taps of the packed texel planes decoded BEFORE filtering, the row rules of mirres_matnet_scatter.  `bary64`
swaps the fp32 barycentrics for float64 ones (an accuracy check of the fp32 formula, not a bit-for-bit one)."""
import numpy as np

f32 = np.float32


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def barycentrics(verts, tris, prim, pos, bary64=False):
    dt = np.float64 if bary64 else np.float32
    t = tris[prim].astype(np.int64)
    v0, v1, v2 = (verts[t[:, k]].astype(dt) for k in range(3))
    p = pos.astype(dt)
    e1, e2, d = v1 - v0, v2 - v0, p - v0
    d00, d01, d11, d20, d21 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(d, e1), _dot(d, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = d00 * d11 - d01 * d01
        b1 = (d11 * d20 - d01 * d21) / den
        b2 = (d00 * d21 - d01 * d20) / den
    b0 = (dt(1) - b1) - b2
    return b0.astype(f32), b1.astype(f32), b2.astype(f32)


def srgb_decode_table():
    q = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.where(q < f32(0.04045), q / f32(12.92), ((q + f32(0.055)) / f32(1.055)) ** f32(2.4)).astype(np.float32)


def pack_planes(feat0, feat1):
    """u8[H, W, 3] x 2 -> the packed u8[H, W, 8] plane (kd.rgb, roughness = feat1 G, metallic = feat1 B, 0, 0, 0)."""
    p = np.zeros(feat0.shape[:2] + (8,), np.uint8)
    p[..., 0:3] = feat0; p[..., 3] = feat1[..., 1]; p[..., 4] = feat1[..., 2]
    return p


def sample(verts, tris, vt, ft, tri_end, planes, decode, rough_min, prim, pos, bary64=False):
    """-> f32[n, 5] (kd rgb, roughness, metallic) of every row (prim must be valid)."""
    n = prim.shape[0]
    b0, b1, b2 = barycentrics(verts, tris, prim, pos, bary64)
    c = ft[prim].astype(np.int64)
    uv0, uv1, uv2 = vt[c[:, 0]], vt[c[:, 1]], vt[c[:, 2]]
    u = (b0 * uv0[:, 0] + b1 * uv1[:, 0]) + b2 * uv2[:, 0]
    v = (b0 * uv0[:, 1] + b1 * uv1[:, 1]) + b2 * uv2[:, 1]
    cas = np.zeros(n, np.int64)
    for k in range(1, len(planes)):
        cas[prim >= tri_end[k - 1]] = k
    out = np.zeros((n, 5), np.float32)
    for k, pl in enumerate(planes):
        m = cas == k
        if not m.any():
            continue
        H, W = pl.shape[:2]
        with np.errstate(invalid="ignore"):
            x = np.fmax(np.fmin(u[m] * f32(W) - f32(0.5), f32(W)), f32(-1)).astype(np.float32)
            y = np.fmax(np.fmin(v[m] * f32(H) - f32(0.5), f32(H)), f32(-1)).astype(np.float32)
        xf, yf = np.floor(x), np.floor(y)
        fx, fy = (x - xf).astype(np.float32), (y - yf).astype(np.float32)
        xi, yi = xf.astype(np.int64), yf.astype(np.int64)
        xa, xb = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
        ya, yb = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
        tap = lambda yy, xx: decode[pl[yy, xx, :5]]                                    # decoded BEFORE filtering
        t00, t10, t01, t11 = tap(ya, xa), tap(ya, xb), tap(yb, xa), tap(yb, xb)
        a = t00 + fx[:, None] * (t10 - t00)
        b = t01 + fx[:, None] * (t11 - t01)
        out[m] = a + fy[:, None] * (b - a)
    out[:, 3] = np.fmin(np.fmax(out[:, 3], f32(rough_min)), f32(1))
    return out


def lookup(verts, tris, vt, ft, tri_end, planes, decode, rough_min, occ, prim, pos, kd, rm, use_scale=False, scale=(1.0, 1.0, 1.0), bary64=False):
    """The row rules of mirres_texmat_lookup on copies of kd f32[n,3] / rm f32[n,2]."""
    kd = kd.copy(); rm = rm.copy()
    T = int(tri_end[-1])
    sel = (occ >= 0.5) if occ is not None else np.ones(prim.shape[0], bool)
    sel &= (prim >= 0) & (prim < T)
    if sel.any():
        o = sample(verts, tris, vt, ft, tri_end, planes, decode, rough_min, prim[sel], pos[sel], bary64)
        k = o[:, 0:3]
        if use_scale:
            k = k * np.asarray(scale, np.float32)[None]
        kd[sel] = k; rm[sel] = o[:, 3:5]
    if use_scale:
        kd = np.fmin(np.fmax(kd, f32(0)), f32(1))
    return kd, rm
