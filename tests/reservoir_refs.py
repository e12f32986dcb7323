"""Hostile inputs for the temporal and spatial reservoir passes, and a plain restatement of which clause decides each candidate.

The friendly fixture of test_gpu_passes.py (history G-buffer = current G-buffer, no motion vectors, reservoirs straight out of the previous pass, zero normals on
the background) never lets several clauses of csrc/passes.hip decide an outcome.  The fixtures here make every clause decide for a countable set of pixels, and
`classify_temporal` / `classify_spatial` say for which — in numpy float32 on top of oracle.seed / oracle.next1d, in the reference's order of tests
(oracle/orc_kernels.hpp temporal_pixel / spatial_pixel).  tests/test_reservoir_fixtures.py proves on the CPU that the classes are populated and that the oracle
agrees with the classification; tests/test_gpu_reservoir_hostile.py then compares the HIP passes with the oracle on these inputs.  No GPU here."""
import types

import numpy as np

f32 = np.float32

# temporal classes: the first clause of temporal_pixel that rejects the pixel
T_BACKGROUND, T_OUTSIDE, T_HIST_BG, T_NORMAL, T_DEPTH, T_BOTH, T_ACCEPTED = -1, 0, 1, 2, 3, 4, 5
T_NAMES = {T_OUTSIDE: "history pixel outside the frame", T_HIST_BG: "history pixel is background", T_NORMAL: "normal only", T_DEPTH: "depth only",
           T_BOTH: "normal and depth", T_ACCEPTED: "accepted"}
# spatial classes: the first clause of spatial_pixel's neighbour loop that rejects the candidate
S_NONE, S_OUTSIDE, S_GEOMETRY, S_M_ZERO, S_BACKGROUND, S_ACCEPTED = -1, 0, 1, 2, 3, 4
S_NAMES = {S_OUTSIDE: "out of bounds", S_GEOMETRY: "geometry", S_M_ZERO: "M == 0 alone", S_BACKGROUND: "background alone", S_ACCEPTED: "accepted"}

NEIGHBOR_OFFSET_COUNT, GATHER_RADIUS = 8192, f32(30.0)      # orc_kernels.hpp Config


def _dot3(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z in float32, every operation rounded (no contraction): dot() of orc_math.hpp / device_math.hpp."""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def _similar(nd_a, nd_b):
    """isValidNeighbor (res.slang:63-68) of G-buffer rows a (the canonical pixel) and b: (normal clause, depth clause)."""
    nd_a = np.asarray(nd_a, f32); nd_b = np.asarray(nd_b, f32)
    normal_ok = _dot3(nd_a[..., :3], nd_b[..., :3]).astype(f32) >= f32(0.5)
    depth_ok = np.abs((nd_a[..., 3] - nd_b[..., 3]).astype(f32)) <= (f32(0.1) * nd_a[..., 3]).astype(f32)
    return normal_ok, depth_ok


def _draws(O, fx, pixels, frameIndex, count):
    """The first `count` numbers of every listed pixel's generator (seed_generator(x, y, frameIndex), then next1d): float32 [len(pixels), count]."""
    out = np.zeros((len(pixels), count), f32)
    for j, pi in enumerate(pixels):
        s = O.seed(int(pi) % fx, int(pi) // fx, int(frameIndex))
        for c in range(count):
            out[j, c], s = O.next1d(s)
    return out


def _oct_codes(O, rng, n):
    """n valid octahedral light codes (1, ex, ey) of directions in the upper hemisphere, as the initial pass stores them."""
    d = rng.normal(size=(n, 3)); d[:, 2] = np.abs(d[:, 2]) + 0.2
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    out = np.ones((n, 3), f32)
    for i in range(n):
        out[i, 1:] = O.oct_encode(d[i])
    return out


def _edit_reservoirs(O, res, occ, rng, shares):
    """The hostile reservoir edits, on DISJOINT random subsets of the foreground: M = 0, M = 500, weight = 0, weight = +inf (shares = their fractions of the
    foreground, in that order); every background pixel gets a plausible non-empty reservoir (M = 3, weight 1, a valid light code)."""
    res = [a.copy() for a in res]
    fg = np.flatnonzero(occ > 0.5); bg = np.flatnonzero(~(occ > 0.5))
    order = rng.permutation(fg)
    cuts = np.cumsum([int(round(s * len(fg))) for s in shares])
    m0, m500, w0, winf = np.split(order[:cuts[-1]], cuts[:-1])
    res[2][m0] = 0
    res[2][m500] = 500
    res[3][w0] = 0.0
    res[3][winf] = np.inf
    res[0][bg] = _oct_codes(O, rng, len(bg)); res[1][bg] = f32(0.3); res[2][bg] = 3; res[3][bg] = f32(1.0)
    return res


def initial_reservoirs(O, F, frameIndex, frame=None):
    """A real oracle.initial result on frame F (light tiles of frameIndex - 2, as the render loop numbers them)."""
    fr = frame if frame is not None else F.frame
    tile_ld, _, tile_pdf = O.light_tiles(fr, frameIndex - 2)
    r = O.new_reservoirs(F.N)
    O.initial(fr, r, tile_ld, tile_pdf, frameIndex)
    return r


def merged_reservoirs(O, F, frameIndex):
    """What the spatial pass of a second sample reads: the initial result of frameIndex merged (oracle.temporal, friendly history) with the one of frameIndex - 20."""
    r = initial_reservoirs(O, F, frameIndex)
    O.temporal(F.frame, r, initial_reservoirs(O, F, frameIndex - 20), F.occ, F.normal_depth, F.brdf, F.ray_dir, frameIndex + 1)
    return r


def hostile_history(F, H, rng, frameIndex=1002):
    """History for the temporal pass of frame F that disagrees with F: (p_occ, p_nd, p_brdf, p_rd, motion, prev_reservoirs).
    About a third of the history G-buffer comes from H (another view of the scene, same size); about a third of the history depths is scaled to both sides of
    the 10 % threshold; the motion vectors are whole-pixel shifts of up to +-3 pixels (in units of the frame size), a few per cent +-1.5 (outside the frame);
    the history reservoirs are an oracle.initial result with the edits of _edit_reservoirs."""
    O, N = F.O, F.N
    p_occ, p_nd, p_brdf, p_rd = F.occ.copy(), F.normal_depth.copy(), F.brdf.copy(), F.ray_dir.copy()
    take = rng.random(N) < 1.0 / 3.0
    for dst, src in ((p_occ, H.occ), (p_nd, H.normal_depth), (p_brdf, H.brdf), (p_rd, H.ray_dir)):
        dst[take] = src[take]
    scaled = rng.random(N) < 1.0 / 3.0
    factor = rng.choice(np.array([1 - 0.12, 1 - 0.099, 1 + 0.099, 1 + 0.12], f32), N)
    p_nd[scaled, 3] = (p_nd[scaled, 3] * factor[scaled]).astype(f32)
    motion = np.stack([rng.integers(-3, 4, N) / F.fx, rng.integers(-3, 4, N) / F.fy], 1).astype(f32)
    far = rng.random(N) < 0.04
    motion[far, rng.integers(0, 2, int(far.sum()))] = rng.choice(np.array([-1.5, 1.5], f32), int(far.sum()))
    prev = _edit_reservoirs(O, initial_reservoirs(O, F, frameIndex), F.occ, rng, (0.08, 0.22, 0.08, 0.12))
    return p_occ, p_nd, p_brdf, p_rd, np.ascontiguousarray(motion), prev


def hostile_neighbours(F, rng, frameIndex=1022, stale_share=0.7, shares=(0.32, 0.10, 0.08, 0.08)):
    """Inputs for the spatial pass of frame F: (normal_depth, reservoirs).  The reservoirs are a temporally merged oracle result (merged_reservoirs) with the edits of
    _edit_reservoirs.  The G-buffer is F's, but a share of the background pixels carries the normal and depth of the nearest foreground pixel of its row while their occupancy stays 0 (a
    stale G-buffer): next to such a pixel the geometry clause accepts, the reservoir holds M = 3, and the occupancy clause alone rejects the neighbour.
    A third of the foreground reservoirs holds M = 0: accepting such a neighbour changes the canonical pixel's result only through the neighbour count and the
    generator's position, i.e. only where another neighbour is accepted as well — with a smaller share fewer than ten pixels of the 48 x 40 frame would notice
    a pass that forgot the `M != 0` clause."""
    O = F.O
    nd = F.normal_depth.copy()
    occ2 = (F.occ > 0.5).reshape(F.fy, F.fx)
    nd2 = nd.reshape(F.fy, F.fx, 4)
    for y in range(F.fy):
        xs = np.flatnonzero(occ2[y])
        if len(xs) == 0:
            continue
        for x in np.flatnonzero(~occ2[y]):
            if rng.random() < stale_share:
                nd2[y, x] = nd2[y, xs[np.argmin(np.abs(xs - x))]]
    return np.ascontiguousarray(nd), _edit_reservoirs(O, merged_reservoirs(O, F, frameIndex), F.occ, rng, shares)


def classify_temporal(O, fx, fy, occ, nd, brdf, rd, p_occ, p_nd, p_brdf, p_rd, motion, cur_M, prev_M, prev_weight, frameIndex, max_history=20):
    """Who decides every pixel of the temporal pass, in temporal_pixel's order: background pixel -> history pixel outside the frame -> history pixel is background
    -> isValidNeighbor (normal, depth or both clauses fail) -> accepted.  The history pixel is int((float)x + mv * (float)fx + jitter) in float32, as written in
    the shader.  Returns a namespace: cls [N] (T_*), qi [N] (history pixel, -1 where there is none) and, for accepted pixels only, the flags moved (history is
    another pixel), other_context (its normal, ray direction or BRDF scalars differ from the pixel's), m_zero (history M = 0), cap (min(M, M_cur * max_history)
    binds), w_zero, w_inf (history weight)."""
    N = fx * fy
    cls = np.full(N, T_BACKGROUND, np.int8); qi = np.full(N, -1, np.int64)
    fg = np.flatnonzero(~(np.asarray(occ, f32) < f32(0.1)))
    j = _draws(O, fx, fg, frameIndex, 2)
    x = (fg % fx).astype(np.uint32).astype(f32); y = (fg // fx).astype(np.uint32).astype(f32)
    mv = np.zeros((len(fg), 2), f32) if motion is None else np.asarray(motion, f32).reshape(N, 2)[fg]
    ppx = ((x + (mv[:, 0] * f32(fx)).astype(f32)).astype(f32) + j[:, 0]).astype(f32).astype(np.int32)      # conversion truncates towards zero, as (int) does
    ppy = ((y + (mv[:, 1] * f32(fy)).astype(f32)).astype(f32) + j[:, 1]).astype(f32).astype(np.int32)
    inside = ~((ppx >= fx) | (ppx < 0) | (ppy >= fy) | (ppy < 0))
    cls[fg[~inside]] = T_OUTSIDE
    p, q = fg[inside], (ppy[inside].astype(np.int64) * fx + ppx[inside])
    qi[p] = q
    hist_bg = np.asarray(p_occ, f32)[q] < f32(0.1)
    cls[p[hist_bg]] = T_HIST_BG
    p, q = p[~hist_bg], q[~hist_bg]
    n_ok, d_ok = _similar(np.asarray(nd, f32)[p], np.asarray(p_nd, f32)[q])
    cls[p] = np.where(n_ok & d_ok, T_ACCEPTED, np.where(d_ok, T_NORMAL, np.where(n_ok, T_DEPTH, T_BOTH)))
    acc = np.zeros(N, bool); acc[p[n_ok & d_ok]] = True
    a = np.flatnonzero(acc); qa = qi[a]

    def flag(v):
        o = np.zeros(N, bool); o[a] = v
        return o
    other = (np.asarray(p_nd, f32)[qa, :3] != np.asarray(nd, f32)[a, :3]).any(1) | (np.asarray(p_rd, f32)[qa] != np.asarray(rd, f32)[a]).any(1) | \
            (np.asarray(p_brdf, f32)[qa] != np.asarray(brdf, f32)[a]).any(1)
    pw = np.asarray(prev_weight, f32)[qa]; pM = np.asarray(prev_M)[qa]
    return types.SimpleNamespace(cls=cls, qi=qi, accepted=acc, moved=flag(qa != a), other_context=flag(other), m_zero=flag(pM == 0),
                                 cap=flag(pM > np.asarray(cur_M)[a] * max_history), w_zero=flag(pw == 0), w_inf=flag(np.isinf(pw)))


def classify_spatial(O, fx, fy, occ, nd, M, weight, noff, frameIndex, neighbor_count=5):
    """Who decides every candidate neighbour of the spatial pass, in spatial_pixel's order of `continue`s: in bounds -> isValidNeighbor -> neighbour reservoir
    M != 0 -> neighbour is foreground -> accepted.  Returns a namespace: cls [N, neighbor_count] (S_*; S_NONE on background pixels, which have no candidates),
    nb [N, neighbor_count] (the candidate pixel, -1 out of bounds) and the flags w_zero / w_inf [N, neighbor_count] of accepted candidates' weights."""
    N = fx * fy; k = neighbor_count
    occ = np.asarray(occ, f32); nd = np.asarray(nd, f32); noff = np.asarray(noff, f32).reshape(-1, 2)
    cls = np.full((N, k), S_NONE, np.int8); nb = np.full((N, k), -1, np.int64)
    fg = np.flatnonzero(~(occ < f32(0.1)))
    start = (_draws(O, fx, fg, frameIndex, 1)[:, 0] * f32(NEIGHBOR_OFFSET_COUNT)).astype(f32).astype(np.uint32)
    x = (fg % fx).astype(np.int64); y = (fg // fx).astype(np.int64)
    for i in range(k):
        ni = (start + np.uint32(i)) & np.uint32(NEIGHBOR_OFFSET_COUNT - 1)
        nx = x + (noff[ni, 0] * GATHER_RADIUS).astype(f32).astype(np.int32)
        ny = y + (noff[ni, 1] * GATHER_RADIUS).astype(f32).astype(np.int32)
        inside = (nx >= 0) & (ny >= 0) & (nx < fx) & (ny < fy)
        q = np.where(inside, ny * fx + nx, 0)
        n_ok, d_ok = _similar(nd[fg], nd[q])
        c = np.full(len(fg), S_ACCEPTED, np.int8)
        c[occ[q] < f32(0.1)] = S_BACKGROUND          # assigned in reverse order: an earlier clause overwrites a later one
        c[np.asarray(M)[q] == 0] = S_M_ZERO
        c[~(n_ok & d_ok)] = S_GEOMETRY
        c[~inside] = S_OUTSIDE
        cls[fg, i] = c; nb[fg, i] = np.where(inside, q, -1)
    w = np.asarray(weight, f32)[np.maximum(nb, 0)]
    acc = cls == S_ACCEPTED
    return types.SimpleNamespace(cls=cls, nb=nb, w_zero=acc & (w == 0), w_inf=acc & np.isinf(w))


def outside_offsets(count=NEIGHBOR_OFFSET_COUNT):
    """A neighbour-offset table whose every entry points outside any frame narrower than 3000 pixels: the spatial pass without neighbours (the oracle reads
    neighbor_count = 0 as "the reference's constant", so the empty neighbourhood is stated through the table; rejected candidates draw no random numbers)."""
    return np.full((count, 2), 100.0, f32)


class Hostile:
    """One frame with its hostile temporal and spatial inputs and the oracle's answers on them, computed once and shared by the tests (never modified)."""
    HISTORY_INDEX, CURRENT_INDEX, TEMPORAL_INDEX, SPATIAL_INDEX = 1002, 1022, 1023, 1024

    def __init__(self, O, S, fx=48, fy=40):
        from util import SmallFrame
        self.O = O
        self.F = F = SmallFrame(O, S, fx=fx, fy=fy)
        self.H = SmallFrame(O, S, fx=fx, fy=fy, view=(75.0, 18.0))
        self.p_occ, self.p_nd, self.p_brdf, self.p_rd, self.motion, self.prev = hostile_history(F, self.H, np.random.default_rng(11), self.HISTORY_INDEX)
        self.cur = initial_reservoirs(O, F, self.CURRENT_INDEX)
        self.snd, self.sres = hostile_neighbours(F, np.random.default_rng(12), self.CURRENT_INDEX)
        self._memo = {}

    def frame(self, nd=None, **constants):
        """The oracle's frame over F's arrays, with another normal / depth buffer and other ReSTIR constants where given."""
        F = self.F
        return self.O.make_frame(F.keep, F.fx, F.fy, F.occ, F.pos, F.normal_depth if nd is None else nd, F.brdf, F.ray_dir, (F.info, F.aabb), F.vert, F.tri, F.tex,
                                 F.Wc, F.Hc, F.tables, **constants)

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def temporal_classes(self, motion=True, max_history=20):
        F = self.F
        return self._once(("tc", motion, max_history), lambda: classify_temporal(
            self.O, F.fx, F.fy, F.occ, F.normal_depth, F.brdf, F.ray_dir, self.p_occ, self.p_nd, self.p_brdf, self.p_rd, self.motion if motion else None,
            self.cur[2], self.prev[2], self.prev[3], self.TEMPORAL_INDEX, max_history))

    def oracle_temporal(self, motion=True, max_history=20):
        def make():
            out = [a.copy() for a in self.cur]
            self.O.temporal(self.frame(max_history=max_history), out, self.prev, self.p_occ, self.p_nd, self.p_brdf, self.p_rd, self.TEMPORAL_INDEX,
                            motion=self.motion if motion else None)
            return out
        return self._once(("ot", motion, max_history), make)

    def oracle_temporal_benign(self):
        """The friendly case: the history G-buffer is the current one, no motion vectors, the history reservoirs as the initial pass wrote them."""
        def make():
            F = self.F; out = [a.copy() for a in self.cur]
            self.O.temporal(F.frame, out, initial_reservoirs(self.O, F, self.HISTORY_INDEX), F.occ, F.normal_depth, F.brdf, F.ray_dir, self.TEMPORAL_INDEX)
            return out
        return self._once("otb", make)

    def spatial_classes(self, k=5):
        F = self.F
        return self._once(("sc", k), lambda: classify_spatial(self.O, F.fx, F.fy, F.occ, self.snd, self.sres[2], self.sres[3], F.noff, self.SPATIAL_INDEX, k))

    def oracle_spatial(self, k=5, noff=None):
        def make():
            out = self.O.new_reservoirs(self.F.N)
            self.O.spatial(self.frame(nd=self.snd, neighbor_count=k), out, self.sres, self.F.noff if noff is None else noff, self.SPATIAL_INDEX)
            return out
        return self._once(("os", k, noff is None), make)

    def oracle_spatial_benign(self):
        def make():
            out = self.O.new_reservoirs(self.F.N)
            self.O.spatial(self.F.frame, out, merged_reservoirs(self.O, self.F, self.CURRENT_INDEX), self.F.noff, self.SPATIAL_INDEX)
            return out
        return self._once("osb", make)


# ------------------------------------------------------------------ thin frames: the moved history pixel inside whole frames
THIN_SHAPES, THIN_SPP, THIN_OFFSET = ((16384, 2), (2, 16384)), 6, 4242


class ThinFrame:
    """32768 surface pixels to be rendered as a 16384 x 2 and as a 2 x 16384 frame (same arrays, other fx / fy).  Without motion vectors the history pixel of the
    temporal pass is int((float)x + u): it is the pixel's right / lower neighbour only where (float)x + u rounds up, which needs a coordinate of several thousand
    (2^-11 of the draws at x >= 8192).  The pixels are the foreground pixels of a 256 x 256 SmallFrame in row order, repeated as needed, so that neighbours in the
    flat order are mostly geometrically similar and the moved history is accepted.  Constant material."""
    N = 32768

    def __init__(self, O, S):
        from util import SmallFrame
        B = SmallFrame(O, S, fx=256, fy=256, varied=False)
        sel = np.resize(np.flatnonzero(B.occ > 0.5), self.N)
        self.O, self.base = O, B
        for name in ("occ", "pos", "normal", "depth", "kd", "rm", "ray_dir_raw", "ray_dir", "normal_depth", "brdf"):
            setattr(self, name, np.ascontiguousarray(getattr(B, name)[sel]))
        for name in ("vert", "tri", "info", "aabb", "env"):
            setattr(self, name, getattr(B, name))

    def moved_and_accepted(self, fx, fy, spp, random_offset):
        """Pixels whose history pixel is another pixel and is accepted, per temporal pass of a frame of `spp` samples.  The temporal pass of sample s >= 1 is
        seeded with random_offset + 20 s + 3: oracle/mirres_oracle.cpp orc_render numbers 20 passes per sample (mTotalRISPasses), light tiles take pass 0,
        the initial pass 2 and the temporal pass 3.  Every pixel is foreground and the history G-buffer is the current one."""
        out = []
        for s in range(1, spp):
            c = classify_temporal(self.O, fx, fy, self.occ, self.normal_depth, self.brdf, self.ray_dir, self.occ, self.normal_depth, self.brdf, self.ray_dir,
                                  None, np.ones(self.N, np.int32), np.ones(self.N, np.int32), np.ones(self.N, f32), random_offset + 20 * s + 3)
            out.append(np.flatnonzero(c.moved))
        return out
