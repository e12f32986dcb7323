"""CPU restatements for the three operators in front of the path — dr.antialias, dr.interpolate, dr.texture (csrc/antialias.hip, csrc/raster.hip, raster.py) —
and the scenes their GPU tests run on.  numpy / torch float64 only; nothing here touches the HIP library.

All three operators take the raster record as an INPUT, so a scene is a hand-made clip-space mesh whose record comes from the float64 software rasteriser
of tests/util.py, rounded to fp32: the kernel and the restatement read the same fp32 arrays, and every comparison the algorithm makes on the record itself
(triangle ids, the depth order of two pixels) is the same decision on both sides.  What remains are the decisions taken on projected fp32 coordinates; aa_analyse
measures how far each of them is from flipping (`margin`, in pixels) and tests/test_raster_refs.py admits only scenes in which none is nearer than 1e-3 px —
three orders of magnitude above the fp32 rounding of a pixel coordinate — so the GPU tests compare every element, with no exclusions."""
import numpy as np
import torch

from util import rasterize_ref_homogeneous


class Scene:
    """pos f64[V,4] (fp32 values), tri i32[T,3], opp i32[T,3], rast f64[H*W,4] (fp32 values)."""

    def __init__(self, name, pos, tri, H, W, rast=None):
        from mirres_restir_nerf_mesh_amd.raster import antialias_topology
        self.name, self.H, self.W = name, int(H), int(W)
        self.pos_exact = np.asarray(pos, np.float64)
        self.pos = self.pos_exact.astype(np.float32).astype(np.float64)
        self.tri = np.ascontiguousarray(np.asarray(tri, np.int32))
        self.opp = antialias_topology(torch.from_numpy(self.tri)).numpy()
        if rast is None:
            rast = rasterize_ref_homogeneous(self.pos, self.tri, self.H, self.W)[0]
        self.rast = np.asarray(rast, np.float64).astype(np.float32).astype(np.float64)
        self._recs = None

    @property
    def recs(self):
        if self._recs is None:
            self._recs = aa_analyse(self.rast, self.pos, self.tri, self.opp, self.H, self.W)
        return self._recs


# ---------------------------------------------------------------------------------------------------------------------------------------- scenes

def scene(seed, H, W, behind=False, G=6, drop=0.15):
    """A jittered G x G grid of vertices in NDC, each with its own w in [0.6, 3] and z/w in [-0.5, 0.5], triangulated, about `drop` of the triangles removed
    (boundary edges, holes); in front of it a patch of 3 triangles with w in [0.4, 0.6] and z/w in [-0.9, -0.6] (triangle-over-triangle pairs).
    behind: one interior grid vertex gets w = -0.5 — its triangles are rasterised (clipped) but the operator makes no screen-space statement about them."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, G), np.linspace(-0.8, 0.8, G))
    ndc = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.12, 0.12, (G * G, 2))
    w = rng.uniform(0.6, 3.0, G * G)
    z = rng.uniform(-0.5, 0.5, G * G)
    tri = []
    for j in range(G - 1):
        for i in range(G - 1):
            a = j * G + i
            tri += [[a, a + 1, a + G], [a + 1, a + G + 1, a + G]]
    tri = np.array(tri)
    tri = tri[rng.random(len(tri)) > drop]
    n0 = G * G
    ndc2 = rng.uniform(-0.5, 0.5, (5, 2)); w2 = rng.uniform(0.4, 0.6, 5); z2 = rng.uniform(-0.9, -0.6, 5)
    tri2 = np.array([[n0, n0 + 1, n0 + 2], [n0 + 1, n0 + 3, n0 + 2], [n0 + 2, n0 + 3, n0 + 4]])
    ndc = np.concatenate([ndc, ndc2]); w = np.concatenate([w, w2]); z = np.concatenate([z, z2])
    pos = np.stack([ndc[:, 0] * w, ndc[:, 1] * w, z * w, w], 1)
    if behind:
        pos[2 * G + 2] = [0.3, -0.2, 0.1, -0.5]
    return Scene("random(seed=%d, %dx%d%s)" % (seed, W, H, ", behind" if behind else ""), pos, np.concatenate([tri, tri2]), H, W)


def _clip(px, py, H, W, zw=0.0, w=1.0):
    """Pixel coordinates -> clip space: pixel centre (i, j) <-> NDC ((2 i + 1) / W - 1, (2 j + 1) / H - 1).  Exact in fp32 for dyadic px, py, w and W, H powers of two."""
    return [(2.0 * px / W - 1.0) * w, (2.0 * py / H - 1.0) * w, zw * w, w]


def scene_fold():
    """Two triangles share the edge A-B and both lie to its right in screen space, over background: A-B has a neighbour across it and is a silhouette all the
    same (a fold).  The upper triangle (A, B, D) is nearer; w differs per vertex (0.5, 1, 2), so the d/dw term is exercised with exact inputs."""
    H = W = 8
    A = _clip(2.375, 0.25, H, W, 0.0, 2.0); B = _clip(3.875, 7.75, H, W, 0.0, 0.5)
    Cv = _clip(7.5625, 3.125, H, W, 0.25, 1.0); D = _clip(7.125, 6.625, H, W, -0.5, 1.0)
    return Scene("fold", [A, B, Cv, D], [[0, 1, 2], [1, 0, 3]], H, W)


def scene_sliver():
    """A triangle 0.31 px wide at its top, tapering downwards, whose two long edges both cross the segment between the centres of columns 3 and 4.  No pixel
    centre lies inside it, so a point-sampling rasteriser records nothing; the record here is written by hand and names the sliver in column 3 of rows 0..5,
    as a ray-cast rasteriser whose fp32 edge tests disagree with the projection by a rounding, or a conservative one, would.  From p0 (column 3) both long
    edges cross at u in [0, 1]; the nearer one decides (alpha = u_near - 1/2 < 0)."""
    H = W = 8
    pos = [_clip(3.5625, 0.25, H, W), _clip(3.875, 0.25, H, W), _clip(3.8125, 7.75, H, W, 0.0, 2.0)]
    rast = np.zeros((H * W, 4))
    for row in range(6):
        rast[row * W + 3] = [0.25, 0.25, 0.0, 1.0]
    return Scene("sliver", pos, [[0, 1, 2]], H, W, rast=rast)


def scene_shared_edge():
    """Two coplanar triangles form a quadrilateral over background: the pairs across the shared diagonal name different triangles and must blend nothing;
    the outline is a boundary silhouette."""
    H = W = 8
    pos = [_clip(1.25, 0.75, H, W), _clip(6.75, 1.75, H, W, 0.0, 2.0), _clip(7.375, 7.25, H, W), _clip(0.625, 6.25, H, W, 0.0, 0.5)]
    return Scene("shared interior edge", pos, [[0, 1, 2], [0, 2, 3]], H, W)


def scene_row():
    """W x 1 frame (one pixel high): only horizontal pairs exist; two triangles with a gap between them."""
    H, W = 1, 16
    pos = [_clip(1.25, -3.0, H, W), _clip(6.75, -2.0, H, W, 0.0, 2.0), _clip(4.0, 4.0, H, W, 0.0, 0.5),
           _clip(9.25, -3.0, H, W, -0.5), _clip(14.375, -1.0, H, W, -0.5, 2.0), _clip(11.0, 5.0, H, W, -0.5)]
    return Scene("row 16x1", pos, [[0, 1, 2], [3, 4, 5]], H, W)


def scene_column():
    """1 x H frame (one pixel wide): only vertical pairs exist."""
    H, W = 16, 1
    pos = [_clip(-3.0, 1.25, H, W), _clip(-2.0, 6.75, H, W, 0.0, 2.0), _clip(4.0, 4.0, H, W, 0.0, 0.5),
           _clip(-3.0, 9.25, H, W, -0.5), _clip(-1.0, 14.375, H, W, -0.5, 2.0), _clip(5.0, 11.0, H, W, -0.5)]
    return Scene("column 1x16", pos, [[0, 1, 2], [3, 4, 5]], H, W)


HAND_MADE = (scene_fold, scene_sliver, scene_shared_edge, scene_row, scene_column)

# The scenes of tests/test_gpu_raster_adjoints.py.  tests/test_raster_refs.py asserts of each that no pair has a margin below 1e-3 px; these seeds were chosen
# for that (of seeds 0..149, 39 satisfy it at both sizes with and without `behind`; 7 and 22 are the first two that also have every category count the CPU
# test asks for).  If a change to the generator breaks the property, choose other seeds — the threshold stays.
SEEDS = (7, 22)
SIZES = ((20, 24), (15, 17))                      # (H, W); 17 x 15 = 255 pixels
EXTRA = ((7, 16, 16), (7, 1, 257))                # (seed, H, W): 256 and 257 pixels — one block exactly, one block and one pixel
_cache = {}


def scene_specs():
    """[(key, constructor)] of every antialias scene the GPU tests use."""
    specs = [(("random", seed, H, W, behind), (lambda seed=seed, H=H, W=W, behind=behind: scene(seed, H, W, behind)))
             for seed in SEEDS for (H, W) in SIZES for behind in (False, True)]
    specs += [(("random", seed, H, W, False), (lambda seed=seed, H=H, W=W: scene(seed, H, W))) for seed, H, W in EXTRA]
    specs += [((f.__name__,), f) for f in HAND_MADE]
    return specs


def get_scene(key):
    """The scene of a key of scene_specs(), built and analysed once per process."""
    if key not in _cache:
        _cache[key] = dict(scene_specs())[key]()
    return _cache[key]


def scene_id(key):
    return key[0] if len(key) == 1 else "seed%d-%dx%d%s" % (key[1], key[3], key[2], "-behind" if key[4] else "")


# ---------------------------------------------------------------------------------------------------------------------------------------- antialias

class Pair:
    """One horizontally / vertically adjacent pixel pair whose records name different triangles, as aa_analyse decided it."""
    __slots__ = ("lo", "hi", "axis", "s", "p0", "p1", "t", "versus", "kind", "sil", "va", "vb", "u", "alpha", "n_cross", "n_opp_behind", "margin")

    @property
    def blend(self):
        return self.kind == "blend"

    @property
    def category(self):
        """(axis, s, sign of alpha) of a blend."""
        return (self.axis, int(self.s), "alpha>0" if self.alpha > 0 else "alpha<0")

    @property
    def label(self):
        if self.kind == "behind":
            return "skipped: a vertex of the examined triangle has w <= 0"
        tail = "triangle-vs-" + ("triangle" if self.versus == "tri" else "background")
        if self.n_opp_behind:
            tail += ", %d edge(s) skipped for an opposite vertex with w <= 0" % self.n_opp_behind
        if self.kind == "none":
            return "no crossing, " + tail
        return "axis %d, s %+d, %s, %s silhouette, %s%s" % (self.axis, int(self.s), "alpha>0" if self.alpha > 0 else "alpha<0", self.sil,
                                                           "two or more crossings, " if self.n_cross > 1 else "", tail)


def aa_analyse(rast, pos, tri, opp, H, W):
    """Float64 statement of the decisions of dr.antialias (header of csrc/antialias.hip) with, for every pair of adjacent pixels with different triangle ids,
    how far the nearest decision is from flipping.  Returns a list of Pair in the order (lower pixel ascending; its right pair, then its down pair):
      kind 'blend': (p0, p1, axis, s, va, vb, alpha), sil 'boundary' / 'fold', versus 'tri' / 'bg', n_cross = silhouette crossings with u in [0, 1];
      kind 'none' : no silhouette edge crosses the segment;      kind 'behind': a vertex of the examined triangle has w <= 0 (the pair is skipped);
      n_opp_behind: edges passed over because the vertex across them has w <= 0.
    margin (pixels): the smallest of |ao|, |bo| (an end point of a silhouette edge against the line through the two centres), |sc| / |e|, |so| / |e| (the
    third and the opposite vertex against the edge), |u|, |1 - u| of every crossing of that line, the gap between the best and the second-best u, and |alpha|.
    The arithmetic is that of util.antialias_ref expression for expression: [(r.p0, r.p1, r.alpha, r.va, r.vb) for blends] equals its `pairs` exactly."""
    rast = np.asarray(rast, np.float64); pos = np.asarray(pos, np.float64)
    out = []

    def proj(v, cx, cy):
        x, y, z, w = pos[v]
        if not w > 0:
            return None
        return np.array([(x / w + 1) * 0.5 * W - cx, (y / w + 1) * 0.5 * H - cy])

    for lo in range(H * W):
        for axis, hi in ((0, lo + 1 if (lo % W) + 1 < W else -1), (1, lo + W if lo + W < H * W else -1)):
            if hi < 0:
                continue
            t0, t1 = int(rast[lo, 3]) - 1, int(rast[hi, 3]) - 1
            if t0 == t1:
                continue
            r = Pair(); r.lo, r.hi, r.axis = lo, hi, axis
            first = t0 >= 0
            r.versus = "tri" if (t0 >= 0 and t1 >= 0) else "bg"
            if t0 >= 0 and t1 >= 0:
                first = not (rast[hi, 2] < rast[lo, 2])
            t = t0 if first else t1
            r.t = t
            r.p0, r.p1 = (lo, hi) if first else (hi, lo)
            r.s = 1.0 if first else -1.0
            r.va = r.vb = -1; r.u = r.alpha = None; r.sil = None; r.n_cross = 0; r.n_opp_behind = 0; r.margin = np.inf
            out.append(r)
            cx, cy = (r.p0 % W) + 0.5, (r.p0 // W) + 0.5
            P = [proj(int(v), cx, cy) for v in tri[t]]
            if any(q is None for q in P):
                r.kind = "behind"
                continue
            m = np.inf; cross = []
            for k in range(3):
                a, b, c = P[k], P[(k + 1) % 3], P[(k + 2) % 3]
                o = int(opp[t, k]); fold = False
                if o >= 0:
                    q = proj(o, cx, cy)
                    if q is None:
                        r.n_opp_behind += 1
                        continue
                    e = b - a
                    sc = e[0] * (c[1] - a[1]) - e[1] * (c[0] - a[0]); so = e[0] * (q[1] - a[1]) - e[1] * (q[0] - a[0])
                    L = np.hypot(e[0], e[1])
                    m = min(m, abs(sc) / L, abs(so) / L)
                    if (sc > 0) != (so > 0):
                        continue
                    fold = True
                ad, ao, bd, bo = a[axis], a[1 - axis], b[axis], b[1 - axis]
                m = min(m, abs(ao), abs(bo))
                if (ao > 0) == (bo > 0):
                    continue
                u = r.s * (ad * bo - bd * ao) / (bo - ao)
                m = min(m, abs(u), abs(1 - u))
                if not (0 <= u <= 1):
                    continue
                cross.append((u, int(tri[t][k]), int(tri[t][(k + 1) % 3]), fold))
            r.n_cross = len(cross)
            if not cross:
                r.kind = "none"; r.margin = m
                continue
            best = min(range(len(cross)), key=lambda i: (cross[i][0], i))          # the first of equal u wins, as `u < best` keeps it
            us = sorted(c_[0] for c_ in cross)
            if len(us) > 1:
                m = min(m, us[1] - us[0])
            r.u, r.va, r.vb = cross[best][0], cross[best][1], cross[best][2]
            r.sil = "fold" if cross[best][3] else "boundary"
            r.alpha = r.u - 0.5
            r.margin = min(m, abs(r.alpha))
            r.kind = "blend"
    return out


def aa_pairs(recs):
    """The blends in util.antialias_ref's form."""
    return [(r.p0, r.p1, r.alpha, r.va, r.vb) for r in recs if r.blend]


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


def aa_torch(color, pos, recs, H, W, pos_gradient_boost=1.0):
    """The blend with aa_analyse's decisions held fixed (which pairs blend, through which edge, on which side of alpha = 0), as a torch function of
    color [H*W, C] and of pos[:, (0, 1, 3)] in the dtype of `pos` (float64: the reference; float32: the noise floor of the same expression).
    pos_gradient_boost scales the gradient that reaches pos and nothing else.  Returns (out [H*W, C], alpha [number of blends])."""
    B = [r for r in recs if r.blend and r.alpha != 0]
    dt = pos.dtype
    if not B:
        return color.clone(), torch.zeros(0, dtype=dt)
    idx = lambda f: torch.tensor([f(r) for r in B], dtype=torch.int64)
    p0, p1, va, vb = idx(lambda r: r.p0), idx(lambda r: r.p1), idx(lambda r: r.va), idx(lambda r: r.vb)
    vert = idx(lambda r: r.axis) == 1
    s = torch.tensor([r.s for r in B], dtype=dt)
    plus = torch.tensor([r.alpha > 0 for r in B])
    xyw = _ScaleGrad.apply(pos[:, (0, 1, 3)], float(pos_gradient_boost))
    cx = (p0 % W).to(dt) + 0.5; cy = torch.div(p0, W, rounding_mode="floor").to(dt) + 0.5
    hw, hh = 0.5 * W, 0.5 * H

    def project(v):
        iw = 1.0 / xyw[v, 2]
        return (xyw[v, 0] * iw + 1.0) * hw - cx, (xyw[v, 1] * iw + 1.0) * hh - cy

    ax, ay = project(va); bx, by = project(vb)
    ad, ao = torch.where(vert, ay, ax), torch.where(vert, ax, ay)
    bd, bo = torch.where(vert, by, bx), torch.where(vert, bx, by)
    alpha = s * ((ad * bo - bd * ao) / (bo - ao)) - 0.5
    recv, give = torch.where(plus, p1, p0), torch.where(plus, p0, p1)
    wgt = torch.where(plus, alpha, -alpha)
    out = color.index_add(0, recv, wgt[:, None] * (color[give] - color[recv]))
    return out, alpha


def aa_receivers(recs, n):
    """For every pixel the blends it receives colour from: list of lists of (Pair, other pixel)."""
    got = [[] for _ in range(n)]
    for r in recs:
        if r.blend and r.alpha != 0:
            if r.alpha > 0:
                got[r.p1].append((r, r.p0))
            else:
                got[r.p0].append((r, r.p1))
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------- interpolate

def interpolate_torch(attr, rast, tri):
    """dr.interpolate's contract (header of csrc/raster.hip): out = u a[i0] + v a[i1] + (1 - u - v) a[i2] where the record names triangle id - 1 >= 0, else 0.
    attr [V,C], rast [n,4] (u, v, z/w, id + 1) in one floating dtype (either may require grad), tri int[T,3]."""
    t = rast[:, 3].detach().to(torch.int64) - 1
    on = t >= 0
    i = tri.to(torch.int64)[t.clamp(min=0)]
    u, v = rast[:, 0:1], rast[:, 1:2]
    out = u * attr[i[:, 0]] + v * attr[i[:, 1]] + (1 - u - v) * attr[i[:, 2]]
    return torch.where(on[:, None], out, torch.zeros_like(out))


def interpolate_db_torch(attr, rast, tri, rast_db, sel):
    """Image-space derivatives of the selected attributes by the chain rule through (u, v): d a / dX = du/dX (a0 - a2) + dv/dX (a1 - a2), likewise for Y;
    rast_db = (du/dX, du/dY, dv/dX, dv/dY).  Layout [n, 2 len(sel)]: (d/dX, d/dY) per selected attribute.  Zero where the record is empty."""
    t = rast[:, 3].to(torch.int64) - 1
    on = t >= 0
    i = tri.to(torch.int64)[t.clamp(min=0)]
    a0, a1, a2 = attr[i[:, 0]][:, sel], attr[i[:, 1]][:, sel], attr[i[:, 2]][:, sel]
    dX = rast_db[:, 0:1] * (a0 - a2) + rast_db[:, 2:3] * (a1 - a2)
    dY = rast_db[:, 1:2] * (a0 - a2) + rast_db[:, 3:4] * (a1 - a2)
    out = torch.stack((dX, dY), dim=-1).reshape(rast.shape[0], 2 * len(sel))
    return torch.where(on[:, None], out, torch.zeros_like(out))


# ---------------------------------------------------------------------------------------------------------------------------------------- texture

def _taps(uv, H, W):
    x = (uv[:, 0] * W - 0.5).clamp(0.0, float(W - 1)); y = (uv[:, 1] * H - 0.5).clamp(0.0, float(H - 1))
    xf, yf = torch.floor(x), torch.floor(y)
    x0, y0 = xf.to(torch.int64), yf.to(torch.int64)
    return x0, (x0 + 1).clamp(max=W - 1), y0, (y0 + 1).clamp(max=H - 1), x - xf, y - yf


def texture_torch(tex, uv):
    """dr.texture(filter_mode='linear', boundary_mode='clamp') as csrc/raster.hip states it: texel centres at ((i + 0.5) / W, (j + 0.5) / H), the continuous
    texel coordinate u W - 0.5 clamped to [0, W - 1], the four surrounding texels (the upper neighbour clamped to the edge) weighted bilinearly.
    tex [H,W,C] (may require grad), uv [n,2] constants, one floating dtype.  Returns [n,C]."""
    H, W, _ = tex.shape
    x0, x1, y0, y1, fx, fy = _taps(uv.detach(), H, W)
    fx, fy = fx[:, None], fy[:, None]
    return (tex[y0, x0] * (1 - fx) + tex[y0, x1] * fx) * (1 - fy) + (tex[y1, x0] * (1 - fx) + tex[y1, x1] * fx) * fy


def texture_touched(uv, H, W, slack=1e-4):
    """bool[H,W]: the texels some tap of some coordinate reads.  A coordinate that is a texel centre up to rounding has floor(u W - 0.5) decided by the last
    bit of an fp32 product (|u W| < 32: one ulp is 2e-6 texels), and either answer is right — the neighbour it brings in has weight ~1e-6 —, so the taps are
    taken for the texel coordinate moved by -slack, 0 and +slack (1e-4 texels: fifty ulps): a texel outside this set is read under no rounding."""
    m = torch.zeros((H, W), dtype=torch.bool)
    uv = uv.detach().double()
    for dx in (-slack, 0.0, slack):
        for dy in (-slack, 0.0, slack):
            x0, x1, y0, y1, _, _ = _taps(torch.stack((uv[:, 0] + dx / W, uv[:, 1] + dy / H), 1), H, W)
            for yy in (y0, y1):
                for xx in (x0, x1):
                    m[yy, xx] = True
    return m


def aa_alpha_noise(sc):
    """max |alpha32 - alpha64| over the blends of a scene: the same expression (aa_torch, decisions fixed) in float32 and in float64."""
    col = torch.zeros((sc.H * sc.W, 1), dtype=torch.float64)
    a64 = aa_torch(col, torch.from_numpy(sc.pos), sc.recs, sc.H, sc.W)[1]
    a32 = aa_torch(col.float(), torch.from_numpy(sc.pos).float(), sc.recs, sc.H, sc.W)[1]
    return float((a32.double() - a64).abs().max()) if a64.numel() else 0.0
