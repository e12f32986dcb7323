"""numpy restatements of the stage-1 texture bake (csrc/bake.hip) for tests/test_export_host.py and tests/test_gpu_export.py:

    raster_ref      the integer UV rasteriser (1/256-texel snapping, int64 edge functions, top-left fill rule, lowest triangle index wins)
    quantise_ref    nerf/renderer.py:395-398 in float32, as numpy evaluates it there
    inpaint_ref     nerf/renderer.py:400-414 the way the reference does it: scipy's dilation / erosion and a kd-tree over the search band
    downsample_ref  the integer-factor INTER_LINEAR rule of DESIGN.md §5"""
import numpy as np

FIX = 256
FIX_MAX = 1 << 28


def snap(u, n):
    u = np.asarray(u, np.float32).astype(np.float64)
    bad = ~np.isfinite(u)
    x = np.floor(np.where(bad, 0.0, u) * float(n) * FIX + 0.5)
    return np.clip(x, -FIX_MAX, FIX_MAX).astype(np.int64), bad


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by):
    dy, dx = by - ay, bx - ax
    return dy > 0 or (dy == 0 and dx < 0)


def raster_ref(vt, ft, W, H):
    """-> (tid i64[H*W] (-1: uncovered), b0 f64[H*W], b1 f64[H*W]) — exact barycentrics (weights of ft's v0, v1) of the snapped triangle."""
    vt = np.asarray(vt, np.float32).reshape(-1, 2); ft = np.asarray(ft, np.int64).reshape(-1, 3)
    tid = np.full(H * W, -1, np.int64); b0 = np.zeros(H * W); b1 = np.zeros(H * W)
    for t in range(ft.shape[0]):
        j = ft[t]
        if (j < 0).any() or (j >= vt.shape[0]).any():
            continue
        X, bx = snap(vt[j, 0], W); Y, by = snap(vt[j, 1], H)
        if bx.any() or by.any():
            continue
        X = [int(a) for a in X]; Y = [int(a) for a in Y]
        area = _edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
        if area == 0:
            continue
        flip = area < 0
        if flip:
            X[1], X[2] = X[2], X[1]; Y[1], Y[2] = Y[2], Y[1]
        c0 = max(-((-(min(X) - FIX // 2)) // FIX), 0); c1 = min((max(X) - FIX // 2) // FIX, W - 1)
        r0 = max(-((-(min(Y) - FIX // 2)) // FIX), 0); r1 = min((max(Y) - FIX // 2) // FIX, H - 1)
        if c1 < c0 or r1 < r0:
            continue
        cc, rr = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64), np.arange(r0, r1 + 1, dtype=np.int64))
        px, py = cc * FIX + FIX // 2, rr * FIX + FIX // 2
        w = [_edge(X[1], Y[1], X[2], Y[2], px, py), _edge(X[2], Y[2], X[0], Y[0], px, py), _edge(X[0], Y[0], X[1], Y[1], px, py)]
        own = [_owns(X[1], Y[1], X[2], Y[2]), _owns(X[2], Y[2], X[0], Y[0]), _owns(X[0], Y[0], X[1], Y[1])]
        ins = np.ones(px.shape, bool)
        for k in range(3):
            ins &= (w[k] > 0) | ((w[k] == 0) & own[k])
        p = (rr * W + cc)[ins]
        new = tid[p] < 0                                    # triangles run in index order: the first one to cover a texel keeps it
        p = p[new]
        A = float(area if not flip else -area)
        tid[p] = t
        b0[p] = w[0][ins][new] / A
        b1[p] = (w[2] if flip else w[1])[ins][new] / A
    return tid, b0, b1


def quantise_ref(feats):
    x = np.clip(np.asarray(feats, np.float32), 0, 1)
    x = np.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)
    return (x * 255).astype(np.uint8)


def inpaint_ref(mask, img, radius=32):
    """mask bool[H,W], img u8[H,W,C] -> u8[H,W,C] exactly as renderer.py:400-414 (sklearn's kd-tree when importable, else scipy's cKDTree)."""
    from scipy.ndimage import binary_dilation, binary_erosion
    out = img.copy()
    out[~mask] = 0
    if not mask.any():
        return out
    region = binary_dilation(mask, iterations=radius)
    region[mask] = 0
    search = mask.copy()
    search[binary_erosion(search, iterations=3)] = 0
    sc = np.stack(np.nonzero(search), -1); ic = np.stack(np.nonzero(region), -1)
    if ic.shape[0] == 0:
        return out
    try:
        from sklearn.neighbors import NearestNeighbors
        idx = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(sc).kneighbors(ic)[1][:, 0]
    except ImportError:
        from scipy.spatial import cKDTree
        idx = cKDTree(sc).query(ic, k=1)[1]
    out[tuple(ic.T)] = img[tuple(sc[idx].T)]
    return out


def downsample_ref(img, s):
    img = np.asarray(img, np.int64)
    H, W = img.shape[:2]
    h0, w0 = H // s, W // s
    if s % 2:
        c = (s - 1) // 2
        return img[c::s, c::s][:h0, :w0].astype(np.uint8)
    a = s // 2 - 1
    q = img[a::s, a::s][:h0, :w0] + img[a::s, a + 1::s][:h0, :w0] + img[a + 1::s, a::s][:h0, :w0] + img[a + 1::s, a + 1::s][:h0, :w0]
    return ((q + 2) >> 2).astype(np.uint8)
