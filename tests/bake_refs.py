"""numpy restatements of the stage-1 texture bake (csrc/bake.hip) for tests/test_export_host.py and tests/test_gpu_export.py:

    raster_ref      the integer UV rasteriser (1/256-texel snapping, int64 edge functions, top-left fill rule, lowest triangle index wins)
    raster_small_ref  the same rasteriser vectorised over many triangles with small texel boxes (tri_setup: k_uv_setup restated; chunk_first: the
                    scanned work-item counts; cell_grid_input / raster_split_ref: the input and reference of the scan tests)
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


def tri_setup(vt, ft, W, H):
    """k_uv_setup for every triangle at once -> dict: X, Y i64[T, 3] (snapped, v1 / v2 swapped where the UV triangle is clockwise), flip bool[T], area i64[T]
    (signed, before the swap), c0, r0, bw, bh i64[T] (the clamped texel box; bw = bh = 0 for a triangle that covers nothing: an index out of range, a
    non-finite coordinate, zero area, a box off the grid)."""
    vt = np.asarray(vt, np.float32).reshape(-1, 2); ft = np.asarray(ft, np.int64).reshape(-1, 3)
    ok = ((ft >= 0) & (ft < vt.shape[0])).all(1)
    j = np.where(ok[:, None], ft, 0)
    X, bx = snap(vt[j, 0], W); Y, by = snap(vt[j, 1], H)
    ok &= ~(bx.any(1) | by.any(1))
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    ok &= area != 0
    flip = area < 0
    X[flip] = X[flip][:, [0, 2, 1]]; Y[flip] = Y[flip][:, [0, 2, 1]]
    c0 = np.maximum(-((-(X.min(1) - FIX // 2)) // FIX), 0); c1 = np.minimum((X.max(1) - FIX // 2) // FIX, W - 1)
    r0 = np.maximum(-((-(Y.min(1) - FIX // 2)) // FIX), 0); r1 = np.minimum((Y.max(1) - FIX // 2) // FIX, H - 1)
    ok &= (c1 >= c0) & (r1 >= r0)
    return dict(X=X, Y=Y, flip=flip, area=area, c0=c0, r0=r0, bw=np.where(ok, c1 - c0 + 1, 0), bh=np.where(ok, r1 - r0 + 1, 0))


CHUNK = 32                                  # BK_CHUNK (csrc/bake.hip:17): box texels per work item


def chunk_first(vt, ft, W, H):
    """first[] of mirres_uv_rasterize restated, i64[T + 1]: the exclusive sum of every triangle's ceil(bw * bh / 32) work items, the total last."""
    s = tri_setup(vt, ft, W, H)
    n = (s["bw"] * s["bh"] + CHUNK - 1) // CHUNK
    return np.concatenate(([0], np.cumsum(n)))


def _weights(s, t, px, py):
    """The three edge functions of triangles t (indices into the set-up s) at the points (px, py), and whether the fill rule gives them the point."""
    X, Y = s["X"][t], s["Y"][t]
    ins = np.ones(len(t), bool); w = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        e = _edge(X[:, a], Y[:, a], X[:, b], Y[:, b], px, py)
        dy, dx = Y[:, b] - Y[:, a], X[:, b] - X[:, a]
        ins &= (e > 0) | ((e == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))
        w.append(e)
    return w, ins


def raster_small_ref(vt, ft, W, H, maxbox):
    """raster_ref for many small triangles, vectorised over them: the same snapping, int64 edge functions and top-left rule per texel of the box, one box offset
    at a time over all triangles, np.minimum.at for "the lowest index wins", then the winner's barycentrics per covered texel.  Every texel box must be at
    most maxbox wide and high (asserted).  -> (tid, b0, b1) as raster_ref."""
    s = tri_setup(vt, ft, W, H)
    assert s["bw"].max(initial=0) <= maxbox and s["bh"].max(initial=0) <= maxbox, "a texel box of %d x %d exceeds maxbox %d" % (s["bw"].max(), s["bh"].max(), maxbox)
    big = np.iinfo(np.int64).max
    tid = np.full(H * W, big, np.int64)
    for dr in range(maxbox):
        for dc in range(maxbox):
            t = np.nonzero((s["bh"] > dr) & (s["bw"] > dc))[0]
            if t.size == 0:
                continue
            c, r = s["c0"][t] + dc, s["r0"][t] + dr
            _, ins = _weights(s, t, c * FIX + FIX // 2, r * FIX + FIX // 2)
            np.minimum.at(tid, (r * W + c)[ins], t[ins])
    tid[tid == big] = -1
    b0 = np.zeros(H * W); b1 = np.zeros(H * W)
    p = np.nonzero(tid >= 0)[0]
    t = tid[p]
    w, ins = _weights(s, t, (p % W) * FIX + FIX // 2, (p // W) * FIX + FIX // 2)
    assert ins.all()
    A = np.abs(s["area"][t]).astype(np.float64)
    b0[p] = w[0] / A
    b1[p] = np.where(s["flip"][t], w[2], w[1]) / A
    return tid, b0, b1


def cell_grid_input(n=1024, seed=21, every=349, n_large=200, large=100):
    """The many-triangle input of the scan tests on an n x n bake grid -> (vt f32[Nt, 2], ft i32[T, 3], number of leading small triangles).
    The grid is tiled by 2 x 2-texel cells on the lattice of even texel corners (exact in fp32); every cell is split along a random diagonal, which passes through
    two of its four texel centres, and half of the triangles are reversed.  A zero-area triangle (a repeated index) sits at every `every`-th position of the
    list.  n_large random triangles with boxes of up to large x large texels follow the small ones."""
    rng = np.random.default_rng(seed)
    m = n // 2
    k = np.arange(m + 1, dtype=np.float64) * 2.0 / n
    gx, gy = np.meshgrid(k, k)                                                  # lattice point (row i, column j) has index i (m + 1) + j
    vt = np.stack((gx.ravel(), gy.ravel()), 1)
    i, j = (x.ravel() for x in np.meshgrid(np.arange(m), np.arange(m), indexing="ij"))
    a = i * (m + 1) + j; b = a + 1; c = a + m + 2; d = a + m + 1
    other = rng.random(m * m) < 0.5                                             # diagonal b - d instead of a - c
    t0 = np.where(other[:, None], np.stack((a, b, d), 1), np.stack((a, b, c), 1))
    t1 = np.where(other[:, None], np.stack((b, c, d), 1), np.stack((a, c, d), 1))
    ft = np.stack((t0, t1), 1).reshape(-1, 3)
    rev = rng.random(ft.shape[0]) < 0.5
    ft[rev] = ft[rev][:, [0, 2, 1]]
    at = np.arange(every - 1, ft.shape[0], every - 1)
    ft = np.insert(ft, at, ft[at][:, [0, 0, 1]], axis=0)                        # final positions every - 1, 2 every - 1, ...: each `every`-th triangle
    n_small = ft.shape[0]
    centre = rng.uniform(0, 1, (n_large, 1, 2)); half = rng.uniform(4, large / 2, (n_large, 1, 2)) / n
    big = centre + half * rng.uniform(-1, 1, (n_large, 3, 2))
    ft = np.concatenate((ft, vt.shape[0] + np.arange(3 * n_large).reshape(-1, 3)))
    vt = np.concatenate((vt, big.reshape(-1, 2)))
    return vt.astype(np.float32), ft.astype(np.int32), n_small


def raster_split_ref(vt, ft, n_small, W, H, maxbox):
    """raster_ref's result for a list whose first n_small triangles have small boxes: those through raster_small_ref, the rest through raster_ref, merged per
    texel by the lowest index."""
    tid, b0, b1 = raster_small_ref(vt, ft[:n_small], W, H, maxbox)
    lt, l0, l1 = raster_ref(vt, ft[n_small:], W, H)
    take = (lt >= 0) & ((tid < 0) | (lt + n_small < tid))
    return np.where(take, lt + n_small, tid), np.where(take, l0, b0), np.where(take, l1, b1)


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
