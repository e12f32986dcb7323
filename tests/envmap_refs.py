"""float64 statements of the environment light's importance tables and of their sampler, and the catalogue of maps the table, tile and frame tests run on.

Written from the published construction (Pharr et al., Distribution2D: a piecewise-constant 2-D distribution, rows normalised by their sums, a marginal over
the raw row sums, sampled by inverting the marginal and then the conditional CDF) with the reference's particulars: the texel weight is
luminance(env_le(ngp_dir(dir(h, w)))) x sin(theta) (make_sampleable.slang:34-60), a row whose sequential fp32 sum is below 1e-4 becomes uniform
(pdf = 1/W, cdf = x/W) while the marginal keeps its raw sum (make_sampleable.slang:62-86, GenerateLightTiles.py:4-29), and the interval search is an upper
bound (lightDi.slang:41-52).  Nothing here calls the oracle or the engine.

The tables chart WORLD directions with the pole along +y.  The map is looked up through ngp_dir (world (x, y, z) -> map (-x, z, y)): the map's own pole is
world z, and world +y is the point (theta' = pi/2, phi' = pi/2) on the map's equator.  So a table row is a cone around world +y, which crosses many map rows;
a map black on its lower half darkens half of every table row, and what makes WHOLE table rows dark is a map black where world y < 0 (its right half of
columns)."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of fp32
LUM = np.array([0.212671, 0.715160, 0.072169])
FALLBACK = 1e-4                                  # make_sampleable.slang:77: row_weight < 1e-4 -> uniform row


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): a sequential sum of n non-negative fp32 terms is within gamma_{n-1} x (its exact value) of that value."""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def flip(env):
    """renderer_restir.py:305-311 (k_flip_env): vertical flip + flatten to [H*W, 3] — the texture the tables are built from."""
    return np.ascontiguousarray(np.asarray(env, np.float32)[::-1].reshape(-1, 3))


# ------------------------------------------------------------------ the texel weights (make_sampleable.slang:34-60), float64
def table_dirs(H, W):
    """World direction of table cell (h, w): theta = pi (h + 1/2) / H from +y, phi = 2 pi (w + 1/2) / W.  [H, W, 3]."""
    th = np.pi * (np.arange(H) + 0.5) / H
    ph = 2 * np.pi * (np.arange(W) + 0.5) / W
    return np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones(W)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)


def texel_world_dirs(H, W):
    """World direction of the centre of caller texel (r, c): map angles theta' = pi (r + 1/2) / H, phi' = 2 pi (c + 1/2) / W (after the flip, env_le's
    v = 1 - theta' / pi), map direction (sin t' cos p', cos t', sin t' sin p'), world = ngp_dir^-1 (map) = (-map.x, map.z, map.y).  [H, W, 3]."""
    th = np.pi * (np.arange(H) + 0.5) / H
    ph = 2 * np.pi * (np.arange(W) + 0.5) / W
    mx = np.sin(th)[:, None] * np.cos(ph)[None]; my = np.cos(th)[:, None] * np.ones(W)[None]; mz = np.sin(th)[:, None] * np.sin(ph)[None]
    return np.stack([-mx, mz, my], -1)


def env_le64(tex, H, W, d):
    """env_le (lightDi.slang:119-132) in float64 for MAP-frame directions d [n, 3]: pole cut |sin theta| < 1e-4, clamp-to-edge bilinear with int() truncation
    (helper.slang:46-71) on the flipped texture tex [H*W, 3]."""
    t = np.asarray(tex, np.float64).reshape(H, W, 3)
    theta = np.arccos(np.clip(d[:, 1], -1, 1))
    phi = np.arctan2(d[:, 2], d[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    x = phi / (2 * np.pi) * W - 0.5; y = (1 - theta / np.pi) * H - 0.5
    x0 = np.trunc(x).astype(np.int64); y0 = np.trunc(y).astype(np.int64)
    x1 = np.clip(x0 + 1, 0, W - 1); y1 = np.clip(y0 + 1, 0, H - 1); x0 = np.clip(x0, 0, W - 1); y0 = np.clip(y0, 0, H - 1)
    u = (x - x0)[:, None]; v = (y - y0)[:, None]
    out = (t[y0, x0] * (1 - u) + t[y0, x1] * u) * (1 - v) + (t[y1, x0] * (1 - u) + t[y1, x1] * u) * v
    return np.where((np.abs(np.sin(theta)) < 1e-4)[:, None], 0.0, out)


def weights64(env, with_map_angles=False):
    """The texel weights of make_sampleable.slang:34-60 for a caller-layout map [H, W, 3], float64: [H, W] (and the map-frame theta', phi' of each cell)."""
    H, W = env.shape[:2]
    d = table_dirs(H, W).reshape(-1, 3)
    m = np.stack([-d[:, 0], d[:, 2], d[:, 1]], 1)                                   # ngp_dir
    le = env_le64(flip(env), H, W, m)
    w = (le @ LUM).reshape(H, W) * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]
    if not with_map_angles:
        return w
    th = np.arccos(np.clip(m[:, 1], -1, 1)); ph = np.arctan2(m[:, 2], m[:, 0]); ph = np.where(ph < 0, ph + 2 * np.pi, ph)
    return w, th.reshape(H, W), ph.reshape(H, W)


def check_weights(weights, env, what):
    """fp32 texel weights [H, W] (k_env_weight / the oracle) against weights64, texel by texel.  The fp32 lookup position carries an error of
    4 (W + H) u (1 + 1 / sin theta') texels (the footprint bound of tests/test_gpu_render_bwd.py); times the largest luminance within one texel of the
    lookup, times sin theta, that bounds the difference, plus a relative 1e-5 for the transcendental functions.  Exempt: cells whose lookup lies within
    1e-4 rad of the seam phi' = 0 (where clamp-to-edge jumps from column W - 1 to an extrapolation of columns 0 and 1) or of the 1e-4 pole cut."""
    H, W = env.shape[:2]
    w32 = np.asarray(weights, np.float64).reshape(H, W)
    w, th, ph = weights64(env, with_map_angles=True)
    lum = np.abs(flip(env).astype(np.float64) @ LUM).reshape(H, W)
    nb = lum.copy()                                                                   # max over the texel and its 8 neighbours (clamped), in tex layout
    p = np.pad(lum, 1, mode="edge")
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            nb = np.maximum(nb, p[dy:dy + H, dx:dx + W])
    x = np.clip((ph / (2 * np.pi) * W - 0.5).astype(np.int64), 0, W - 1); y = np.clip(((1 - th / np.pi) * H - 0.5).astype(np.int64), 0, H - 1)
    sin_t = np.abs(np.sin(th))
    pos = 4 * (W + H) * U * (1 + 1 / np.maximum(sin_t, 1e-4))
    tol = 1e-5 * np.abs(w) + 2 * pos * nb[y, x] * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]
    exempt = (np.minimum(ph, 2 * np.pi - ph) < 1e-4) | (np.abs(sin_t - 1e-4) < 1e-6)
    bad = (np.abs(w32 - w) > tol) & ~exempt
    assert not bad.any(), "%s: %d texel weights differ from float64 (first at %s: %r vs %r, allowed %.3e)" % (
        what, int(bad.sum()), np.unravel_index(np.argmax(bad), bad.shape), w32.ravel()[np.argmax(bad)], w.ravel()[np.argmax(bad)], tol.ravel()[np.argmax(bad)])


# ------------------------------------------------------------------ Distribution2D (make_sampleable.slang:62-86, GenerateLightTiles.py:4-29), float64
def distribution64(weights):
    """Tables from texel weights [H, W] (the fp32 weights the kernel computed, as float64): returns dict(pdf [H,W], cdf [H,W+1], mpdf [H], mcdf [H+1],
    fallback [H] bool, rowsum [H]).  A row falls back when its sum is below 1e-4; its marginal entry stays the raw sum."""
    w = np.asarray(weights, np.float64)
    H, W = w.shape
    c = np.concatenate([np.zeros((H, 1)), np.cumsum(w, 1)], 1)
    s = c[:, -1]
    fb = s < FALLBACK
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = np.where(fb[:, None], 1.0 / W, w / s[:, None])
        cdf = np.where(fb[:, None], np.arange(W + 1)[None] / W, c / s[:, None])
        cdf[:, W] = 1.0
        mc = np.concatenate([[0.0], np.cumsum(s)])
        total = mc[-1]
        mpdf = s / total; mcdf = mc / total
    mcdf[H] = 1.0
    return dict(pdf=pdf, cdf=cdf, mpdf=mpdf, mcdf=mcdf, fallback=fb, rowsum=s)


def check_tables(tables, weights, what):
    """The fp32 tables (pdf, cdf, mpdf, mcdf as returned by make_sampleable, any shape) against distribution64 of the fp32 texel weights [H, W]:
    exact where the construction is exact, elsewhere within the error bound of the fp32 sequential sums (gamma_n, no tuned slack).  Returns the
    float64 statement."""
    w = np.asarray(weights, np.float32)
    H, W = w.shape
    pdf = np.asarray(tables[0], np.float32).reshape(H, W); cdf = np.asarray(tables[1], np.float32).reshape(H, W + 1)
    mpdf = np.asarray(tables[2], np.float32).reshape(H); mcdf = np.asarray(tables[3], np.float32).reshape(H + 1)
    R = distribution64(w)
    s, fb = R["rowsum"], R["fallback"]
    # a row whose sum lies within the fp32 error of the threshold may fall either way: the catalogue must not contain one
    amb = np.abs(s - FALLBACK) <= gamma(W) * s
    assert not amb.any(), "%s: rows %s sit within fp32 error of the 1e-4 threshold" % (what, np.nonzero(amb)[0][:8])
    # exact properties
    assert (cdf[:, 0] == 0).all(), what + ": cdf[:, 0] != 0"
    assert (cdf[:, W] == 1).all(), what + ": cdf[:, W] != 1"
    assert mcdf[0] == 0 and mcdf[H] == 1, what + ": mcdf ends %r %r" % (mcdf[0], mcdf[H])
    assert (np.diff(cdf, axis=1) >= 0).all(), what + ": a conditional CDF decreases"
    assert (np.diff(mcdf) >= 0).all(), what + ": the marginal CDF decreases"
    assert (pdf >= 0).all() and (mpdf >= 0).all()
    x = np.arange(W)
    if fb.any():
        assert (pdf[fb] == np.float32(1.0 / W)).all(), what + ": fallback rows %s: pdf != 1/W" % np.nonzero(fb)[0][:8]
        assert (cdf[fb][:, :W] == (x / W).astype(np.float32)[None]).all(), what + ": fallback rows %s: cdf != x/W" % np.nonzero(fb)[0][:8]
    # bounded: row k of a conditional CDF = (sequential sum of k terms) / (sum of W terms), each rounded: gamma_{k + W + 1} relative
    n = ~fb
    if n.any():
        k = np.arange(W + 1)[None]
        tol = gamma(k + W + 1) * R["cdf"][n]
        err = np.abs(cdf[n].astype(np.float64) - R["cdf"][n])
        assert (err <= tol).all(), "%s: conditional CDF off by %.3e (bound %.3e) at row %d" % (
            what, err.max(), tol.ravel()[np.argmax(err - tol)], np.nonzero(n)[0][np.argmax((err - tol).max(1))])
        tol = gamma(W + 1) * R["pdf"][n]
        err = np.abs(pdf[n].astype(np.float64) - R["pdf"][n])
        assert (err <= tol).all(), "%s: conditional pdf off by %.3e (bound %.3e)" % (what, err.max(), tol.ravel()[np.argmax(err - tol)])
    # marginal: row sums (gamma_W) summed again (gamma_H over sums that carry gamma_W), then divided
    tol = gamma(2 * W + H + 1) * R["mpdf"]
    err = np.abs(mpdf.astype(np.float64) - R["mpdf"])
    assert (err <= tol).all(), "%s: marginal pdf off by %.3e (bound %.3e) at row %d" % (what, err.max(), tol[np.argmax(err - tol)], np.argmax(err - tol))
    tol = gamma(2 * W + H + np.arange(H + 1) + 1) * R["mcdf"]
    err = np.abs(mcdf.astype(np.float64) - R["mcdf"])
    assert (err <= tol).all(), "%s: marginal CDF off by %.3e (bound %.3e) at row %d" % (what, err.max(), tol[np.argmax(err - tol)], np.argmax(err - tol))
    return R


# ------------------------------------------------------------------ light tiles (GenerateLightTiles.slang:16-62), float64
def _interleave16(v):
    v = v & np.uint32(0xFFFF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x00FF00FF); v = (v | (v << np.uint32(4))) & np.uint32(0x0F0F0F0F)
    v = (v | (v << np.uint32(2))) & np.uint32(0x33333333); v = (v | (v << np.uint32(1))) & np.uint32(0x55555555)
    return v


def tile_randoms(frame_index, n):
    """The two uniforms tile sample i draws (random.slang: TEA seed of (i, i, frameIndex + 1) with 16-bit coordinates, then two LCG steps): [n], [n]."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint32)
        v0 = _interleave16(i) | (_interleave16(i) << np.uint32(1))
        v1 = np.full(n, (frame_index + 1) & 0xFFFFFFFF, np.uint32)
        s = np.uint32(0)
        for _ in range(16):
            s = np.uint32(s + np.uint32(0x9E3779B9))
            v0 = v0 + (((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4)))
            v1 = v1 + (((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E)))
        r = []
        st = v0
        for _ in range(2):
            st = np.uint32(1664525) * st + np.uint32(1013904223)
            r.append((st >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
    return r[0], r[1]


def sample64(tables, H, W, r0, r1):
    """InfiniteAreaLight_Sample_Li (lightDi.slang:67-105, 181-209) on the fp32 tables, in float64: the upper-bound interval search of lightDi.slang:41-52
    (np.searchsorted 'right' - 1: the LAST entry <= u, so a run of equal CDF values — a zero-width interval — is skipped), the continuous offset, the
    density pdf x mpdf x W x H / (2 pi^2 sin theta) (0 within 1e-4 of a pole).  Returns dict(row, col, frac_x, frac_y, theta, phi, pdf)."""
    pdf = np.asarray(tables[0], np.float64).reshape(H, W); cdf = np.asarray(tables[1], np.float64).reshape(H, W + 1)
    mpdf = np.asarray(tables[2], np.float64).reshape(H); mcdf = np.asarray(tables[3], np.float64).reshape(H + 1)
    row = np.clip(np.searchsorted(mcdf, r1, side="right") - 1, 0, H)
    with np.errstate(divide="ignore", invalid="ignore"):
        fy = np.clip((r1 - mcdf[row]) / mpdf[np.minimum(row, H - 1)], 0, 1)
        c = cdf[np.minimum(row, H - 1)]
        col = np.clip((c <= r0[:, None]).sum(1) - 1, 0, W)
        fx = np.clip((r0 - c[np.arange(len(r0)), col]) / pdf[np.minimum(row, H - 1), np.minimum(col, W - 1)], 0, 1)
    x = np.clip((fx + col) / W, 0, 1); y = np.clip((fy + row) / H, 0, 1)
    th, ph = np.pi * y, 2 * np.pi * x
    r2, c2 = np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)
    p = pdf[r2, c2] * mpdf[r2] * W * H
    st = np.sin(th)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(np.abs(st) >= 1e-4, p / (2 * np.pi ** 2 * st), 0.0)
    return dict(row=row, col=col, frac_x=fx, frac_y=fy, theta=th, phi=ph, pdf=p)


def oct_decode64(f):
    """The published octahedral decode (Cigolle et al. 2014; helperDi.slang:122-134), float64, batched."""
    f = 2 * np.asarray(f, np.float64) - 1
    n = np.stack([f[:, 0], f[:, 1], 1 - np.abs(f[:, 0]) - np.abs(f[:, 1])], 1)
    t = np.clip(-n[:, 2], 0, 1)
    n[:, 0] += np.where(n[:, 0] >= 0, -t, t); n[:, 1] += np.where(n[:, 1] >= 0, -t, t)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def check_tiles(tables, H, W, ld, uv, p, frame_index, what):
    """Light tile samples (light_data [n,3], light_uv [n,2] texel coordinates of the flipped map, pdf [n]) drawn with `frame_index` from `tables`, against
    sample64 fed with the same uniforms:
    - every sample the float64 sampler draws lies in an interval of positive width, with table pdf > 0 (zero-probability texels are never drawn);
    - the sample's texel is the float64 sampler's texel (bar a sample that fp32 rounding carries onto a texel border);
    - a sample is valid (light_data.x = 1, pdf > 0) exactly when the float64 density is > 0, and invalid samples are all zeros;
    - the stored pdf is the fp64 table density at the direction the sample DECODES to (its texel's pdf x mpdf x W x H) over 2 pi^2 sin(theta).
    Returns the float64 samples."""
    n = len(p)
    ld = np.asarray(ld, np.float64).reshape(n, 3); uv = np.asarray(uv).reshape(n, 2); p = np.asarray(p, np.float64).reshape(n)
    pdf = np.asarray(tables[0], np.float64).reshape(H, W); cdf = np.asarray(tables[1], np.float64).reshape(H, W + 1)
    mpdf = np.asarray(tables[2], np.float64).reshape(H); mcdf = np.asarray(tables[3], np.float64).reshape(H + 1)
    r0, r1 = tile_randoms(frame_index, n)
    S = sample64(tables, H, W, r0, r1)
    row, col = S["row"], S["col"]
    assert (row < H).all() and (col < W).all(), what + ": the search ran past the last interval"
    assert (mcdf[row + 1] > mcdf[row]).all(), what + ": %d samples in a zero-width marginal interval" % int((mcdf[row + 1] <= mcdf[row]).sum())
    assert (cdf[row, col + 1] > cdf[row, col]).all(), what + ": %d samples in a zero-width conditional interval" % int((cdf[row, col + 1] <= cdf[row, col]).sum())
    assert (pdf[row, col] > 0).all() and (mpdf[row] > 0).all(), what + ": a sample drawn on a texel of table pdf 0"
    # validity
    ok = ld[:, 0] == 1
    assert ((ld[:, 0] == 0) | ok).all()
    assert (ld[~ok] == 0).all() and (p[~ok] == 0).all() and (uv[~ok] == 0).all(), what + ": an invalid sample is not all zeros"
    near_cut = np.abs(np.abs(np.sin(S["theta"])) - 1e-4) < 1e-6
    bad = (ok != (S["pdf"] > 0)) & ~near_cut
    assert not bad.any(), "%s: %d samples valid where the float64 density is 0 or the reverse (first %d)" % (what, int(bad.sum()), int(np.argmax(bad)))
    assert (p[ok] > 0).all() and np.isfinite(p).all()
    # the texel: uv2xy of (x, 1 - y) (helper.slang:26-36), table row = H - 1 - texel row.  fp32 carries a sample whose offset within its texel lies within a
    # few ulps of (x + col) of a border over it: those are exempt (a handful at most)
    trow = H - 1 - uv[:, 1]; tcol = uv[:, 0]
    edge = (np.minimum(S["frac_x"], 1 - S["frac_x"]) <= 8 * (W + 1) * U) | (np.minimum(S["frac_y"], 1 - S["frac_y"]) <= 8 * (H + 1) * U)
    moved = ok & ((trow != row) | (tcol != col))
    # the texel every valid sample reports has table pdf > 0 (a sample carried over a border keeps the density of the texel it was drawn in, > 0 as
    # asserted above for the float64 texel; its stored pdf is > 0 as asserted above)
    stay = ok & ~moved
    assert (pdf[trow[stay], tcol[stay]] > 0).all() and (mpdf[trow[stay]] > 0).all(), what + ": a valid sample reports a texel of table pdf 0"
    assert not (moved & ~edge).any(), "%s: %d samples report another texel than the one drawn (first %d: %s vs %s)" % (
        what, int((moved & ~edge).sum()), int(np.argmax(moved & ~edge)), (trow[np.argmax(moved & ~edge)], tcol[np.argmax(moved & ~edge)]),
        (row[np.argmax(moved & ~edge)], col[np.argmax(moved & ~edge)]))
    assert moved.sum() <= max(4, n // 2000), "%s: %d samples moved over a texel border" % (what, int(moved.sum()))
    # the stored density at the decoded direction
    d = oct_decode64(ld[ok, 1:3])
    th = np.arccos(np.clip(d[:, 1], -1, 1)); ph = np.arctan2(d[:, 2], d[:, 0]); ph = np.where(ph < 0, ph + 2 * np.pi, ph)
    dr = np.clip((th / np.pi * H).astype(np.int64), 0, H - 1); dc = np.clip((ph / (2 * np.pi) * W).astype(np.int64), 0, W - 1)
    same = (dr == row[ok]) & (dc == col[ok])
    want = pdf[dr, dc] * mpdf[dr] * W * H / (2 * np.pi ** 2 * np.sin(th))
    # the density of a direction is continuous within its texel; what the fp32 chain adds is a few roundings of the product and the direction's
    # error through 1/sin(theta): |cot theta| x (angle error of the octahedral code, ~1e-6 rad)
    rtol = 16 * U + 4e-6 * np.abs(np.cos(th) / np.sin(th))
    s = same & (np.sin(th) > 1e-3)
    err = np.abs(p[ok][s] - want[s]) / want[s]
    assert (err <= rtol[s]).all(), "%s: stored pdf differs from the table density at its direction by %.3e (allowed %.3e)" % (
        what, err.max(), rtol[s][np.argmax(err - rtol[s])])
    assert same.mean() > 0.999, "%s: %.5f of the decoded directions lie in the drawn texel" % (what, same.mean())
    return S


def check_texel_frequencies(tables, H, W, ld, uv):
    """Chi-square of the texels drawn by the 65 536 independent tile samples (tiles 0-63; the reference's 16-bit seed mask makes 64-127 repeat them)
    against the probabilities the tables assign (differences of the CDFs the sampler inverts); texels of probability 0 are never drawn."""
    from scipy import stats
    cdf = np.asarray(tables[1], np.float64).reshape(H, W + 1); mcdf = np.asarray(tables[3], np.float64).reshape(H + 1)
    ld = np.asarray(ld).reshape(-1, 3); uv = np.asarray(uv).reshape(-1, 2)
    n = len(ld) // 2
    assert np.array_equal(ld[:n], ld[n:])
    uv, ok = uv[:n], ld[:n, 0] == 1
    assert ok.all()
    obs = np.bincount((H - 1 - uv[:, 1]) * W + uv[:, 0], minlength=H * W).astype(np.float64)
    prob = (np.diff(mcdf)[:, None] * np.diff(cdf, axis=1)).ravel()
    assert abs(prob.sum() - 1) < 1e-5
    assert (prob == 0).sum() > H * W // 4
    assert obs[prob == 0].sum() == 0, "%d samples on texels of probability 0" % int(obs[prob == 0].sum())
    e = n * prob
    k = e >= 5
    o2 = np.append(obs[k], obs[~k].sum()); e2 = np.append(e[k], e[~k].sum())
    if e2[-1] < 5: o2, e2 = o2[:-1], e2[:-1]
    p = stats.chisquare(o2, e2 * o2.sum() / e2.sum()).pvalue
    assert p > 1e-4, "texel frequencies: chi-square p = %.3g" % p


# ------------------------------------------------------------------ the catalogue
def sky(H, W, seed=0):
    """A smooth everywhere-positive sky: a gradient over the map's rows and a slow variation in azimuth."""
    rng = np.random.default_rng(seed)
    v = (np.arange(H) + 0.5) / H; u = (np.arange(W) + 0.5) / W
    a = rng.uniform(0, 2 * np.pi)
    g = (0.25 + 0.6 * (1 - v))[:, None] * (1 + 0.3 * np.cos(2 * np.pi * u + a))[None]
    return np.ascontiguousarray((g[..., None] * np.array([0.85, 0.95, 1.1])).astype(np.float32))


def with_sun(env, at=None, factor=1e5):
    """One texel `factor` x the median texel (per channel) — at `at` (caller row, column), by default a third of the way down and across."""
    env = np.array(env, np.float32)
    H, W = env.shape[:2]
    r, c = at if at is not None else (H // 3, W // 3)
    env[r, c] = np.float32(factor) * np.median(env.reshape(-1, 3), 0)
    return env


def black_ground(env):
    """Caller rows of the lower half of the map black (studio / clamped-ground HDRs): half of every table row goes dark."""
    env = np.array(env, np.float32)
    env[(env.shape[0] + 1) // 2:] = 0
    return env


def black_world_lower(env):
    """Black where the texel centre's WORLD direction has y < 0 (the right half of the columns): the tables' lower hemisphere, so whole table rows
    (theta > pi / 2 bar the bilinear seam) fall back to uniform."""
    env = np.array(env, np.float32)
    env[texel_world_dirs(*env.shape[:2])[..., 1] < 0] = 0
    return env


def threshold_caps(env, low=0.5e-4, high=2e-4):
    """Constant caps around world +y and -y, sized so that the first table row's weight is `low` (below the 1e-4 fallback) and the last row's is `high`
    (above it); the rows next to them (3x and 5x their sin theta) lie above.  Each cap reaches 1.6 texel diagonals past the third row, so that every
    bilinear tap of rows 0-2 and H-3..H-1 reads the cap alone."""
    env = np.array(env, np.float32)
    H, W = env.shape[:2]
    wy = texel_world_dirs(H, W)[..., 1]
    ang = np.arccos(np.clip(wy, -1, 1))
    reach = 2.5 * np.pi / H + 1.6 * np.hypot(np.pi / H, 2 * np.pi / W)
    s0 = np.sin(0.5 * np.pi / H)
    for cap, target in ((ang < reach, low), (ang > np.pi - reach, high)):
        lum = target / (W * s0)
        env[cap] = np.float32(lum / LUM.sum())                   # grey: luminance = value x sum(LUM)
    return env


SHAPES = [(1, 1), (1, 7), (5, 1), (7, 63), (9, 64), (11, 65), (33, 1023), (17, 1024), (9, 1025), (1025, 8), (1030, 2050)]
BIG = (2048, 4096)


def catalogue(big=False):
    """[(name, caller-layout map [H, W, 3] float32)]: every shape with the smooth sky and a one-texel sun, and on the shapes that resolve them the black
    ground, the black world-lower hemisphere and the threshold caps (whose dim rows
    next to the bright sky leave flat CDF runs: zero-width intervals of positive pdf).  `big`: the 2048 x 4096 map alone (sky, sun, black ground)."""
    if big:
        H, W = BIG
        return [("%dx%d_sun_ground" % BIG, black_ground(with_sun(sky(H, W))))]
    out = []
    for H, W in SHAPES:
        out.append(("%dx%d_sky" % (H, W), sky(H, W)))
        out.append(("%dx%d_sun" % (H, W), with_sun(sky(H, W, 1))))
    for H, W in ((33, 1023), (17, 1024), (9, 1025), (1025, 8), (1030, 2050), (11, 65)):
        out.append(("%dx%d_ground" % (H, W), black_ground(with_sun(sky(H, W, 2)))))
        out.append(("%dx%d_worldlower" % (H, W), black_world_lower(with_sun(sky(H, W, 3)))))
    for H, W in ((33, 1023), (17, 1024), (1025, 8), (1030, 2050), (64, 128)):
        out.append(("%dx%d_caps" % (H, W), threshold_caps(sky(H, W, 4))))
    return out


def chi_square_map():
    """The coarse map of the frequency test: a sun and a black world-lower half (a quarter of the table's texels have probability 0)."""
    return black_world_lower(with_sun(sky(16, 32, 7), at=(4, 5)))


def check_intent(name, env, R):
    """The catalogue's contents did what they are for (R: the float64 tables of check_tables)."""
    H, W = env.shape[:2]
    if name.endswith("_worldlower"):
        # the rows of the tables' lower hemisphere clear of the bilinear seam are black: they fall back
        th = np.pi * (np.arange(H) + 0.5) / H
        deep = np.cos(th) < -np.tan(2 * np.pi / W) - 2.0 / H
        assert R["fallback"][deep].all() and R["fallback"].sum() >= H // 4, name
    if name.endswith("_caps"):
        # the weights landed where intended, in float64 from the k_env_weight formula: row 0 at 0.5e-4 (falls back), row 1 at 1.5e-4 and row H-1 at 2e-4
        # (do not); the fp32 tables took the same decisions
        s = weights64(env).sum(1)
        np.testing.assert_allclose([s[0], s[1], s[-1]], [0.5e-4, 0.5e-4 * np.sin(1.5 * np.pi / H) / np.sin(0.5 * np.pi / H), 2e-4], rtol=0.02, err_msg=name)
        assert R["fallback"][0] and not R["fallback"][1] and not R["fallback"][-1], name
