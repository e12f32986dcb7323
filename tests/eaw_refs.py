"""Test infrastructure for the edge-avoiding a-trous denoiser (csrc/eaw.hip: k_eaw, k_eaw5, k_eaw_bwd, k_eaw_bwd_sums, k_eaw_bwd_gather; oracle/orc_kernels.hpp:
eaw_pixel): the hostile frames of tests/test_eaw_refs.py (host) and tests/test_gpu_eaw.py (GPU), and `restated`, a plain float64 numpy restatement of one pass
written from process_EAWDenoise (EAWDenoise.slang:50-174) — one pixel loop, the literal 25-entry offset and kernel tables of :78-138 — as the second opinion
beside the bit comparison of kernel and oracle, which were written by the same hand, and beside adjoint_refs.eaw (float64 torch, whole-frame gathers), whose
autograd is the reference of the adjoints.

What the Slang lines say, and `restated` repeats:
  * :63   a pixel with occ < 0.1f is copied (fp32 comparison: exactly 0.1f is foreground, so is NaN);
  * :146  uv = pixel + int2(offset[i] * stepWidth): float2 times int, truncated — stepWidth 0 puts all 25 taps on the centre;
  * :147  taps outside the frame are SKIPPED (isValidPixel on both coordinates, x against framedim_x); background taps are NOT skipped;
  * :152-162  each weight is min(exp(-d2 / phi), 1) with min / max as fminf / fmaxf (a NaN argument gives the other operand: a NaN weight becomes 1,
    a NaN squared distance of normals or positions becomes 0); the colour's d2 has no max;
  * :164-169  weight = c_w n_w p_w; out = sum ctmp weight kernel[i] / sum weight kernel[i].
The hand adjoint of csrc/eaw.hip equals autodiff of these lines for positive phis only (for phi <= 0 the clamp min(., 1) is active and autodiff passes no
gradient through it); non-positive phis are not tested."""
import functools

import numpy as np

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (17, 15), (16, 16), (257, 1), (1, 257), (19, 27)]      # 255, 256 and 513 px: ragged, full and three blocks
STEPS = [0, 1, 2, 4, 8, 64]
PHIS = [(2.0, 0.1, 0.001), (2.0, 0.5, 0.05)]
KINDS = ["rand", "smooth", "thresh", "island", "hole", "all_bg", "all_fg"]
THRESH_VALUES = [0.0, 0.0999999, 0.1, 0.1000001, 0.5, 1.0, -1.0]

ADJ_KINDS = ["rand", "smooth", "thresh", "island", "hole"]
ADJ_SIZES = [(1, 1), (7, 1), (3, 5), (17, 15), (16, 16), (19, 27)]
ADJ_STEPS = [0, 1, 2, 4]
CHAINS = [(2, 3), (4, 3), (8, 4), (1, 1)]          # (stepWidth, iter_time) of the drivers
ADJ_CHAINS = [(4, 3), (2, 3)]

# EAWDenoise.slang:78-107 and :109-138, as listed there
OFFSET = [(-2, -2), (-1, -2), (0, -2), (1, -2), (2, -2),
          (-2, -1), (-1, -1), (0, -1), (1, -1), (2, -1),
          (-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0),
          (-2, 1), (-1, 1), (0, 1), (1, 1), (2, 1),
          (-2, 2), (-1, 2), (0, 2), (1, 2), (2, 2)]
KERNEL = [1.0 / 256.0, 1.0 / 64.0, 3.0 / 128.0, 1.0 / 64.0, 1.0 / 256.0,
          1.0 / 64.0, 1.0 / 16.0, 3.0 / 32.0, 1.0 / 16.0, 1.0 / 64.0,
          3.0 / 128.0, 3.0 / 32.0, 9.0 / 64.0, 3.0 / 32.0, 3.0 / 128.0,
          1.0 / 64.0, 1.0 / 16.0, 3.0 / 32.0, 1.0 / 16.0, 1.0 / 64.0,
          1.0 / 256.0, 1.0 / 64.0, 3.0 / 128.0, 1.0 / 64.0, 1.0 / 256.0]
MUTATIONS = ["clamp_border", "fy_for_x", "step_min_1", "le_threshold", "skip_bg_taps", "corner_weight", "no_normal_weight", "shared_colour_weight"]


# ------------------------------------------------------------------------------------------------------------------------ frames
def _guides(fx, fy, rng, smooth):
    n = fx * fy
    if smooth:
        nrm = np.array([0.0, 0.0, 1.0]) + 0.03 * rng.normal(size=(n, 3))          # within a few degrees of +z
    else:
        nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    yy, xx = np.mgrid[0:fy, 0:fx]
    z = 0.02 * np.sin(0.7 * xx) * np.cos(0.5 * yy)
    pos = np.stack([0.01 * xx, 0.01 * yy, z], axis=-1).reshape(n, 3) + 0.002 * rng.normal(size=(n, 3))
    return nrm, pos.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _frame(kind, fx, fy, seed, nan):
    rng = np.random.default_rng([seed, fx, fy, KINDS.index(kind)])
    n = fx * fy
    col = (rng.random((n, 3)) * 2).astype(np.float32)
    nrm, pos = _guides(fx, fy, rng, smooth=(kind != "rand"))
    centre = (fy // 2) * fx + fx // 2
    if kind in ("rand", "smooth"):
        occ = (rng.random(n) >= 0.3).astype(np.float32)
    elif kind == "thresh":
        vals = np.array(THRESH_VALUES + ([np.nan] if nan else []), np.float32)
        occ = np.empty(n, np.float32)
        occ[rng.permutation(n)] = vals[(np.arange(n) + int(rng.integers(len(vals)))) % len(vals)]      # every value as often as the others
    elif kind == "island":
        occ = np.zeros(n, np.float32); occ[centre] = 1.0
    elif kind == "hole":
        occ = np.ones(n, np.float32); occ[centre] = 0.0
    elif kind == "all_bg":
        occ = np.zeros(n, np.float32)
    elif kind == "all_fg":
        occ = np.ones(n, np.float32)
    else:
        raise ValueError(kind)
    for a in (occ, col, nrm, pos):
        a.setflags(write=False)
    return occ, col, nrm, pos


def frame(kind, fx, fy, seed=0, nan=False):
    """-> (occ [N], col [N,3], nrm [N,3], pos [N,3]), float32, read-only (cached).
      rand:    unit random normals, positions on a bumpy sheet 0.01 per pixel apart plus jitter, occupancy 0 / 1 with about 30 % background, colours in [0, 2)
      smooth:  as rand with normals within a few degrees of +z: all three weights are alive at the default phis
      thresh:  smooth guides, occupancy drawn evenly from THRESH_VALUES (and NaN with nan=True: forward only, the float64 references are not given it)
      island / hole: one foreground pixel in background / one background pixel in foreground (the pixel (fx // 2, fy // 2))
      all_bg / all_fg"""
    return _frame(kind, int(fx), int(fy), int(seed), bool(nan))


DENORMAL = dict(fx=9, fy=7, step=1, phis=(3e38, 0.1, 0.001))


def denormal_frame():
    """9 x 7, all foreground, normals +z, step 1, phis (3e38, 0.1, 0.001).  Colour 0 on even (x + y), 1e18 on odd (|dc|^2 / c_phi = 0.01); all positions equal
    except that odd pixels are displaced in z by sqrt(95 * 0.001): a pair of unlike parity has p_w = exp(-95) = 5.5e-42, a denormal.  An even pixel's output
    is sum(1e18 w k) / sum(w k) over its odd taps, about 5e-24: non-zero only if the denormal weights and their products with k are kept.
    -> (occ, col, nrm, pos)"""
    fx, fy = DENORMAL["fx"], DENORMAL["fy"]
    n = fx * fy
    yy, xx = np.mgrid[0:fy, 0:fx]
    odd = ((xx + yy) % 2 == 1).reshape(n)
    col = np.zeros((n, 3), np.float32); col[odd] = 1e18
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    pos = np.zeros((n, 3), np.float32); pos[odd, 2] = np.float32(np.sqrt(95 * 0.001))
    return np.ones(n, np.float32), col, nrm, pos


NONFINITE_KINDS = ["colours", "positions", "normals", "phis"]
NONFINITE_DIMS = (17, 15)


def nonfinite(kind):
    """A 17 x 15 `rand` frame with one class of poison, sparse enough that most pixels stay finite -> list of (name, phis, (occ, col, nrm, pos)).
      colours:   +Inf, -Inf and NaN texels (Inf - Inf in the colour distance; a NaN weight that fminf turns into 1)
      positions: Inf, and 1e20, whose square overflows
      normals:   NaN (fmaxf turns the NaN squared distance into 0: weight 1)
      phis:      1e-30, 1e30, +Inf for all three, and (2.0, 0.1, 1e-38), on the clean frame: quotients that overflow to -inf, and -0"""
    fx, fy = NONFINITE_DIMS
    occ, col, nrm, pos = (a.copy() for a in frame("rand", fx, fy, seed=11))
    rng = np.random.default_rng(12)
    n = fx * fy
    if kind == "phis":
        g = (occ, col, nrm, pos)
        return [("phis 1e-30", (1e-30, 1e-30, 1e-30), g), ("phis 1e30", (1e30, 1e30, 1e30), g), ("phis inf", (np.inf, np.inf, np.inf), g), ("p_phi 1e-38", (2.0, 0.1, 1e-38), g)]
    pick = rng.permutation(n)[:6]
    if kind == "colours":
        col[pick[0]] = np.inf; col[pick[1]] = -np.inf; col[pick[2], 1] = np.nan; col[pick[3], 0] = np.inf; col[pick[4]] = np.nan; col[pick[5], 2] = -np.inf
    elif kind == "positions":
        pos[pick[0]] = np.inf; pos[pick[1]] = 1e20; pos[pick[2], 1] = -np.inf; pos[pick[3], 0] = 1e20; pos[pick[4]] = -1e20; pos[pick[5], 2] = np.inf
    elif kind == "normals":
        nrm[pick[0]] = np.nan; nrm[pick[1], 0] = np.nan; nrm[pick[2], 2] = np.nan; nrm[pick[3]] = np.nan
    else:
        raise ValueError(kind)
    occ[pick] = 1.0                                      # the poisoned pixels are foreground: centres as well as taps
    return [(kind, PHIS[0], (occ, col, nrm, pos)), (kind + " soft", PHIS[1], (occ, col, nrm, pos))]


def five_buffers(fx, fy, inf=False, seed=31):
    """The six per-sample sums of the frame's finish, deliberately unlike: [0] random (the total colour: averaged, not denoised), [1] all zeros, [2] constant,
    [3] random (replaced by [4] + [5]), [4] random scaled 1e4, [5] random.  inf=True: one +Inf value in buffer [2] only."""
    rng = np.random.default_rng([seed, fx, fy])
    n = fx * fy
    s = [rng.random((n, 3)).astype(np.float32) * 2 for _ in range(6)]
    s[1] = np.zeros((n, 3), np.float32)
    s[2] = np.full((n, 3), 0.37, np.float32)
    s[4] = (s[4] * np.float32(1e4)).astype(np.float32)
    if inf:
        s[2][(fy // 2) * fx + fx // 3, 1] = np.inf
    return s


def cotangent(fx, fy, seed=41):
    return np.random.default_rng([seed, fx, fy]).random((fx * fy, 3)).astype(np.float32)


def chain_steps(step_width, iters):
    """Denoising.py:154-251: `stepWidth /= 2` on a float, int(stepWidth) at the launch -> (2, 3) runs 2, 1, 0."""
    out, sw = [], step_width
    for _ in range(iters):
        out.append(int(sw)); sw /= 2
    return out


# ------------------------------------------------------------------------------------------------------------------------ float64 restatement
def restated(fx, fy, step, phis, occ, col, nrm, pos, mutate=None):
    """One a-trous pass in float64, pixel by pixel, from EAWDenoise.slang:50-174 (see the module docstring).  `col` is [N,3], or a list of buffers that share
    the guides (the five-buffer form; a list is returned).  `mutate` names ONE deliberate mistake (MUTATIONS) — the tests show that each changes the result."""
    assert mutate is None or mutate in MUTATIONS, mutate
    many = isinstance(col, (list, tuple))
    cols = [np.asarray(c, np.float32).astype(np.float64) for c in (col if many else [col])]
    occ32 = np.asarray(occ, np.float32).reshape(-1)
    N = np.asarray(nrm, np.float32).astype(np.float64); P = np.asarray(pos, np.float32).astype(np.float64)
    c_phi, n_phi, p_phi = (float(np.float32(v)) for v in phis)
    step = int(step)
    if mutate == "step_min_1":
        step = max(step, 1)
    kernel = list(KERNEL)
    if mutate == "corner_weight":
        kernel[0] = 1.0 / 64.0
    thr = np.float32(0.1)
    bg = (occ32 <= thr) if mutate == "le_threshold" else (occ32 < thr)
    outs = [c.copy() for c in cols]
    for pi in range(fx * fy):
        if bg[pi]:
            continue                                                        # :63-69, copied
        x, y = pi % fx, pi // fx
        taps, kw = [], []
        for i in range(25):
            ux, uy = x + int(float(OFFSET[i][0]) * step), y + int(float(OFFSET[i][1]) * step)
            if mutate == "clamp_border":
                ux, uy = min(max(ux, 0), fx - 1), min(max(uy, 0), fy - 1)
            if not (ux >= 0 and uy >= 0 and ux < (fy if mutate == "fy_for_x" else fx) and uy < fy):
                continue
            qi = min(uy * fx + ux, fx * fy - 1)                             # (only the fy_for_x mistake can leave the row)
            if mutate == "skip_bg_taps" and bg[qi]:
                continue
            taps.append(qi); kw.append(kernel[i])
        taps = np.array(taps); kw = np.array(kw)
        with np.errstate(all="ignore"):
            t = N[pi] - N[taps]; n_w = np.fmin(np.exp(-np.fmax((t * t).sum(1), 0.0) / n_phi), 1.0)
            t = P[pi] - P[taps]; p_w = np.fmin(np.exp(-np.fmax((t * t).sum(1), 0.0) / p_phi), 1.0)
            if mutate == "no_normal_weight":
                n_w = np.ones_like(n_w)
            for b, C in enumerate(cols):
                src = cols[0] if mutate == "shared_colour_weight" else C
                t = src[pi] - src[taps]; c_w = np.fmin(np.exp(-(t * t).sum(1) / c_phi), 1.0)
                w = c_w * n_w * p_w * kw
                outs[b][pi] = (C[taps] * w[:, None]).sum(0) / w.sum()
    return outs if many else outs[0]


def rel_err(got, ref):
    """max |got - ref| / (|ref| + 1e-6)"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-6))) if got.size else 0.0


def taps_inside(fx, fy, step):
    """Number of (pixel, off-centre tap) pairs of the frame whose tap lies inside it."""
    c = 0
    for y in range(fy):
        for x in range(fx):
            for ox, oy in OFFSET:
                if (ox, oy) != (0, 0) and 0 <= x + ox * step < fx and 0 <= y + oy * step < fy:
                    c += 1
    return c


# ------------------------------------------------------------------------------------------------------------------------ float64 / float32 autograd
def eaw_torch(fx, fy, steps, phis, occ, col, nrm, pos, dtype):
    """adjoint_refs.eaw chained over `steps` in `dtype` on the CPU -> (out, [col, nrm, pos] leaves)."""
    import torch
    import adjoint_refs as R
    x = [torch.from_numpy(np.array(a, np.float32)).to(dtype).requires_grad_(True) for a in (col, nrm, pos)]
    o = torch.from_numpy(np.array(occ, np.float32)).to(dtype)
    cur = x[0]
    for s in steps:
        cur = R.eaw(fx, fy, int(s), *[float(np.float32(v)) for v in phis], o, cur, x[1], x[2])          # the phis as the kernel receives them: rounded to fp32
    return cur, x


@functools.lru_cache(maxsize=None)
def _grads(kind, fx, fy, steps, phi_index, single):
    import torch
    occ, col, nrm, pos = frame(kind, fx, fy)
    out, x = eaw_torch(fx, fy, steps, PHIS[phi_index], occ, col, nrm, pos, torch.float32 if single else torch.float64)
    (out * torch.from_numpy(cotangent(fx, fy)).to(out.dtype)).sum().backward()
    return tuple(t.grad.numpy() for t in x)


def grads64(kind, fx, fy, steps, phi_index):
    """float64 autograd of adjoint_refs.eaw (chained over the tuple `steps`) for sum(out * cotangent(fx, fy)) -> (d/dcol, d/dnrm, d/dpos); computed once."""
    return _grads(kind, fx, fy, tuple(steps), phi_index, False)


def grads32(kind, fx, fy, steps, phi_index):
    """The same restatement evaluated and differentiated in float32 torch: what fp32 arithmetic alone costs against the bound the HIP adjoints are held to."""
    return _grads(kind, fx, fy, tuple(steps), phi_index, True)


def bound_ratio(got, want, rtol=1e-3, atol_scale=1e-4):
    """max |got - want| / (rtol |want| + atol_scale max |want|): util.elementwise's bound is met iff this is <= 1.  0 where `want` is identically zero and got too."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    if scale == 0:
        return 0.0 if not np.any(got) else np.inf
    return float(np.max(np.abs(got - want) / (rtol * np.abs(want) + atol_scale * scale)))


@functools.lru_cache(maxsize=None)
def oracle_eaw(kind, fx, fy, step, phi_index, nan=False):
    """oracle.eaw on frame(kind, fx, fy) — computed once, shared by the host and the GPU tests."""
    from oracle import oracle as O
    occ, col, nrm, pos = frame(kind, fx, fy, nan=nan)
    out = O.eaw(fx, fy, step, *PHIS[phi_index], occ, col, nrm, pos)
    out.setflags(write=False)
    return out
