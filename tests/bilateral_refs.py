"""Test infrastructure for the bilateral denoiser (csrc/eaw.hip: k_bilateral_pack, k_bilateral<0|2>, k_bilateral_pack5, k_bilateral5; oracle/mirres_oracle.cpp:
orc_bilateral): the input frames of tests/test_bilateral_refs.py (host) and tests/test_gpu_bilateral.py (GPU), and a plain float64 numpy restatement of the
filter written from nerf/renderutils/c_src/denoising.cu (forward :14-71, backward :74-130) and ops.py:164-199 — the second opinion beside the bit comparison of
kernel and oracle, which were written by the same hand.

The restatement builds the dense weight matrix of the frame (row = the pixel the thread computes, column = the tap), so it is limited to a few thousand pixels.

THE BOUND.  For every output element the restatement returns the sum  R = sum_t w_t x_t  and its companion  S = sum_t w_t |x_t|  (t over the window's taps,
x_t the tap's colour or incoming gradient, 1 for the weight sum).  An fp32 evaluation `got` (oracle or kernel) is held to

        |got - R|  <=  K * 2^-24 * S

per element, with no absolute term.  The impulse frames alone (and the host test that reads single weights off the oracle) add  taps * 2^-149  to the right-hand side: there S is a single tap's weight times a colour of
order 1, at sigma 0.4 and 1e-4 that weight lies below 2^-126 inside the window, and fp32 rounds it to a multiple of 2^-149 (`within(..., underflow=True)`).
K = 1024, in units of u = 2^-24 relative to a tap's own term, from the operations of one tap:
  * w_normal = clamp(n_t . n_c, 1e-4, 1)^128.  Both normals are the fp32-normalised ones the kernel reads (the restatement normalises in fp32 too, as the
    reference does in torch before its kernel).  The fp32 dot product rounds three products and two sums: first order <= 3 u (sum |a_i b_i|) <= 3 u, relative
    3 u / d for a dot product d; taps that carry weight have d ~ 1 (0.9^128 = 1.4e-6).  x^128 multiplies that by 128: 384 u.  The seven squarings of
    mrf_pow2k round once each and double what they inherit: 2^7 - 1 = 127 u.  Together 511 u.
  * w_xy = exp(-d^2 / (2 sigma^2)) and w_depth = exp(-|z_t - z_c| / max(dz dist, 1e-4)): a relative error e of an argument A becomes A e in the exponential.
    The first argument rounds once (the quotient; 2 sigma^2 is computed once in fp32, one more rounding: 2 u A); the second rounds the difference, the square
    root (half weight), the product and the quotient: 3.5 u A.  A tap whose weight is still a normal fp32 number has A <= 88 in each; the two arguments share
    one budget of 88 (beyond it the product underflows): <= 88 * 3.5 u = 308 u in the worst split, and the taps that make up S have A of a few units.
    mrf_exp itself is good to 2 ulp (include/mirres_fmath.h), twice: 4 u.  The two products of the three weights and the product with x: 3 u.
  * the summation, sequential over up to 63 x 63 = 3969 taps: worst case (taps - 1) u relative to S, which no frame attains because the Gaussian leaves a few
    hundred taps of comparable weight and the roundings do not align; sqrt(3969) = 63 u as the random-walk figure, allowed at three times that: 189 u.
  511 + 308 + 4 + 3 + 189 = 1015 -> K = 1024.
MEASURED on the CPU, fp32 oracle against this restatement (tests/test_bilateral_refs.py prints every figure with -s): the largest ratio over the finite frames of
the test matrix is 199 u (forward of `asymmetric` 50 x 47 at sigma 4; backward 176 u, weight sums alike; 132 u for the public op's gradient against K_OP), and
293 u for a single weight of the dense 20 x 15 matrix, i.e. the normal term at d ~ 1 and little else.  The kernels give the oracle's bits, hence the same figures
on the GPU.  (With the normals normalised in float64 instead — not what the reference's kernel is given — the same comparison reads 516 u.)
The public op's gradient (ops.py:190-199: out = sum / weight, differentiated through the division) feeds the backward with g / w, where w is the forward's fp32
weight sum (K u) divided once (1 u): K_OP = 2 K + 2."""
import math

import numpy as np

K_BOUND = 1024
K_OP = 2 * K_BOUND + 2
EPS = np.float32(0.0001)
U = 2.0 ** -24


def ref_radius(sigma):
    """denoising.cu:26,86: `int filter_rad = 2 * ceil(params.sigma * 2.5) + 1` — the float sigma times a double constant."""
    return 2 * int(math.ceil(float(np.float32(sigma)) * 2.5)) + 1


def float_radius(sigma):
    """The same expression with the product rounded to float (what the kernels computed before): 2 smaller whenever sigma * 2.5f rounds down onto an integer."""
    return 2 * int(math.ceil(float(np.float32(sigma) * np.float32(2.5)))) + 1


# ------------------------------------------------------------------------------------------------------------------------ frames
def benign(fx, fy, seed=3):
    """Colours in [0, 2), unnormalised normals around +z (the op normalises), a depth ramp with an edge in the middle, dz in [0.015, 0.025)."""
    rng = np.random.default_rng(seed)
    n = fx * fy
    col = rng.random((n, 3)).astype(np.float32) * 2
    nrm = rng.normal(size=(n, 3)).astype(np.float32); nrm[:, 2] += 2.5
    yy, xx = np.mgrid[0:fy, 0:fx]
    z = (1.0 + 0.01 * xx + 0.02 * yy + 0.3 * (xx > fx // 2)).astype(np.float32).reshape(-1)
    zdz = np.stack([z, np.full(n, 0.015, np.float32) + 0.01 * rng.random(n).astype(np.float32)], axis=1).astype(np.float32)
    return col, nrm, zdz


def asymmetric(fx, fy, seed=5):
    """`benign` with dz spread over two decades from pixel to pixel (1e-3 .. 1e-1 against depth steps of 0.01 .. 0.02 per pixel), so that the forward's
    w_depth (the CENTRE's dz) and the backward's (the TAP's dz, denoising.cu:118) differ by orders of magnitude for most pairs."""
    col, nrm, zdz = benign(fx, fy, seed)
    rng = np.random.default_rng(seed + 100)
    zdz[:, 1] = (10.0 ** rng.uniform(-3, -1, fx * fy)).astype(np.float32)
    return col, nrm, zdz


HOSTILE_KINDS = ("normals", "dz", "z", "colours", "dead")


def hostile(kind, fx, fy, nonfinite=False, seed=7):
    """One hostile guide or colour class mixed into a `benign` frame at about one pixel in ten.  nonfinite=False keeps every input finite (the float64 bound
    applies); True adds the NaN / inf members of the class (kernel and oracle must then agree in bits or be NaN together).
      normals: exactly zero; of length 1e-25 and 1e30 (the squared length underflows / overflows); antiparallel to the neighbours; [NaN]
      dz:      0, denormal, 1e30, negative; [NaN]
      z:       jumps of +-1e6; [+inf, -inf, one NaN]
      colours: 10^U(-30, 6) with exact zeros; [one NaN texel, one inf texel]
      dead:    zero normals on a 5 x 4 block and on scattered pixels: every weight of those pixels is 0, so out4.w = 1e-4 and the public op returns 0"""
    col, nrm, zdz = benign(fx, fy, seed)
    rng = np.random.default_rng(seed + 1)
    n = fx * fy
    pick = np.flatnonzero(rng.random(n) < 0.1)
    if len(pick) == 0:
        pick = np.array([0])
    k = np.arange(len(pick))
    if kind == "normals":
        unit = nrm[pick] / np.linalg.norm(nrm[pick], axis=1, keepdims=True)
        cls = k % 4
        nrm[pick[cls == 0]] = 0.0
        nrm[pick[cls == 1]] = (unit[cls == 1] * 1e-25).astype(np.float32)
        nrm[pick[cls == 2]] = (unit[cls == 2] * 1e30).astype(np.float32)
        nrm[pick[cls == 3]] = -nrm[pick[cls == 3]]
        if nonfinite:
            nrm[pick[0], 1] = np.nan; nrm[pick[len(pick) // 2]] = np.nan
    elif kind == "dz":
        vals = np.array([0.0, 1e-40, 1e30, -0.02], np.float32)
        zdz[pick, 1] = vals[k % 4]
        if nonfinite:
            zdz[pick[0], 1] = np.nan; zdz[pick[len(pick) // 2], 1] = np.nan
    elif kind == "z":
        zdz[pick, 0] += np.where(k % 2 == 0, 1e6, -1e6).astype(np.float32)
        if nonfinite:
            zdz[pick[0], 0] = np.inf; zdz[pick[1 % len(pick)], 0] = -np.inf; zdz[pick[len(pick) // 2], 0] = np.nan
    elif kind == "colours":
        col[:] = (10.0 ** rng.uniform(-30, 6, (n, 3))).astype(np.float32)
        col[pick] = 0.0
        if nonfinite:
            col[pick[0] + 1 if pick[0] + 1 < n else 0, 1] = np.nan; col[n // 2] = np.inf
    elif kind == "dead":
        m = np.zeros((fy, fx), bool)
        m[min(2, fy - 1):min(6, fy), min(3, fx - 1):min(8, fx)] = True
        m.reshape(-1)[pick] = True
        nrm[m.reshape(-1)] = 0.0
    else:
        raise ValueError(kind)
    return col, nrm, zdz


def impulse(fx, fy, at, value=(1.0, 0.5, 0.25)):
    """Colour 0 except pixel at = (x, y); flat guides (equal normals, constant z and dz): the output at a pixel is the single term w_xy(offset) w_normal col.
    -> (col, nrm, zdz, index of the pixel)."""
    n = fx * fy
    pi = at[1] * fx + at[0]
    col = np.zeros((n, 3), np.float32); col[pi] = value
    nrm = np.tile(np.array([0.3, -0.2, 0.9], np.float32), (n, 1))
    zdz = np.tile(np.array([2.0, 0.02], np.float32), (n, 1))
    return col, nrm, zdz, pi


def impulse_footprint(fx, fy, sigma, at, amplitude):
    """The window of the reference around `at`, clipped to the frame -> (must, may): boolean [N] masks.  Outside `may` an output must be exactly 0.  Inside
    `must` it must be non-zero: the taps whose weight exp(-d^2 / 2 sigma^2) times the smallest amplitude is a comfortable normal fp32 number (>= 2^-120).
    Between the two (sigma 0.4 and 1e-4 only: w_xy underflows inside the window) either is allowed."""
    r = ref_radius(sigma)
    yy, xx = np.mgrid[0:fy, 0:fx]
    dx, dy = (xx - at[0]).reshape(-1), (yy - at[1]).reshape(-1)
    may = (np.abs(dx) <= r) & (np.abs(dy) <= r)
    s = float(np.float32(sigma))
    with np.errstate(under="ignore"):
        w = np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2.0 * s * s))
    must = may & (w * float(amplitude) >= 2.0 ** -120)
    return must, may


def normalise32(nrm):
    """safe_normalize as the reference applies it in torch before its kernel (ops.py:164-169) and the product inside k_bilateral_pack: x / sqrt(max(x . x, 1e-20)), fp32."""
    x = np.ascontiguousarray(nrm, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        l2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
        ln = np.sqrt(np.fmax(l2, np.float32(1e-20)))
        return (x / ln[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ float64 restatement
def weights64(fx, fy, sigma, nrm, zdz, backward=False):
    """Dense float64 weight matrix W[p, t] of denoising.cu: p the pixel of the thread, t the tap.  Forward (:51-61): the depth term divides by the CENTRE's dz
    (c_zdz.y); backward (:110-120): by the TAP's (t_zdz.y).  Zero outside the (2 r + 1)^2 window, r = ref_radius(sigma).  Finite inputs only."""
    n = fx * fy
    nn = normalise32(nrm).astype(np.float64)
    z = np.asarray(zdz, np.float32)[:, 0].astype(np.float64); dz = np.asarray(zdz, np.float32)[:, 1].astype(np.float64)
    ys, xs = np.divmod(np.arange(n), fx)
    dx = xs[None, :] - xs[:, None]; dy = ys[None, :] - ys[:, None]
    r = ref_radius(sigma)
    inside = (np.abs(dx) <= r) & (np.abs(dy) <= r)
    d2 = (dx * dx + dy * dy).astype(np.float64)
    s = float(np.float32(sigma))
    with np.errstate(under="ignore", over="ignore"):
        w = np.exp(-d2 / (2.0 * (s * s)))
        w *= np.fmin(np.fmax(nn @ nn.T, float(EPS)), 1.0) ** 128
        den = np.fmax((dz[None, :] if backward else dz[:, None]) * np.sqrt(d2), float(EPS))
        w *= np.exp(-(np.abs(z[None, :] - z[:, None]) / den))
    w[~inside] = 0.0
    return w


def forward64(fx, fy, sigma, col, nrm, zdz, W=None):
    """-> (R [N,4] = (sum w col, sum w)  — the weight sum BEFORE its clamp at 1e-4 —, S [N,4] = (sum w |col|, sum w))."""
    W = weights64(fx, fy, sigma, nrm, zdz) if W is None else W
    x = np.concatenate([np.asarray(col, np.float32).astype(np.float64), np.ones((fx * fy, 1))], axis=1)
    return W @ x, W @ np.abs(x)


def backward64(fx, fy, sigma, nrm, zdz, grad4, Wb=None):
    """-> (col_grad [N,3] = sum_t w'(p, t) grad4[t].xyz, S [N,3]) (denoising.cu:122-129; the fourth channel of grad4 is not read)."""
    Wb = weights64(fx, fy, sigma, nrm, zdz, backward=True) if Wb is None else Wb
    g = np.asarray(grad4, np.float32)[:, :3].astype(np.float64)
    return Wb @ g, Wb @ np.abs(g)


def op_gradient64(fx, fy, sigma, col, nrm, zdz, G):
    """Gradient of sum(G * bilateral_denoiser(...)) with respect to the colour (ops.py:190-199: out = col_w[:, :3] / col_w[:, 3:4], autograd through the division,
    then the backward kernel on (G / w, .)) -> (col_grad [N,3], S [N,3])."""
    R, _ = forward64(fx, fy, sigma, col, nrm, zdz)
    g3 = np.asarray(G, np.float32).astype(np.float64) / np.maximum(R[:, 3:4], float(EPS))
    Wb = weights64(fx, fy, sigma, nrm, zdz, backward=True)
    return Wb @ g3, Wb @ np.abs(g3)


def clamp_weight(R):
    """The forward's stored value: (sum w col, max(sum w, 1e-4))."""
    out = np.array(R, np.float64)
    out[:, 3] = np.maximum(out[:, 3], float(EPS))
    return out


def units(got, R, S, floor=0.0):
    """The largest |got - R| in units of 2^-24 S over the elements (after subtracting `floor`, 0 except on the impulse frames); elements with S = 0 must be
    exactly equal (they count as inf otherwise)."""
    got = np.asarray(got, np.float64); R = np.asarray(R, np.float64); S = np.asarray(S, np.float64)
    assert got.shape == R.shape == S.shape, (got.shape, R.shape, S.shape)
    err = np.maximum(np.abs(got - R) - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (U * S))
    return float(np.max(q)) if q.size else 0.0


def within(got, R, S, sigma, what, K=K_BOUND, underflow=False):
    """assert |got - R| <= K 2^-24 S per element; prints the measured figure first (pytest -s).  underflow=True (impulse frames only): + taps * 2^-149."""
    taps = (2 * ref_radius(sigma) + 1) ** 2
    q = units(got, R, S, taps * 2.0 ** -149 if underflow else 0.0)
    print("%s: max |got - ref64| = %.1f x 2^-24 S (bound %d)" % (what, q, K))
    assert np.isfinite(np.asarray(got)).all(), what + ": non-finite output on a finite frame"
    assert q <= K, "%s: %.1f x 2^-24 S exceeds the bound %d" % (what, q, K)
    return q


# ------------------------------------------------------------------------------------------------------------------------ the test matrix
SHAPES_SIGMA4 = [(50, 47), (16, 16), (1, 1), (1, 50), (50, 1), (17, 45), (45, 17)]
SIGMAS = [1.0, 2.0, 1e-4, 0.4, 1.6, 4.4, 6.0]
SIGMA_SHAPES = [(37, 19), (50, 47)]


def finite_cases():
    """(name, fx, fy, sigma, (col, nrm, zdz)) of every finite frame of the matrix: the shapes at sigma 4, the sigmas on two shapes, the asymmetric-dz guides and the
    finite members of the hostile classes."""
    out = []
    for fx, fy in SHAPES_SIGMA4:
        out.append(("benign %dx%d s4" % (fx, fy), fx, fy, 4.0, benign(fx, fy)))
    out.append(("benign 40x28 s4", 40, 28, 4.0, benign(40, 28)))
    for fx, fy in SIGMA_SHAPES:
        for s in SIGMAS:
            out.append(("benign %dx%d s%g" % (fx, fy, s), fx, fy, s, benign(fx, fy)))
    out.append(("asymmetric 50x47 s4", 50, 47, 4.0, asymmetric(50, 47)))
    out.append(("asymmetric 37x19 s1.6", 37, 19, 1.6, asymmetric(37, 19)))
    for kind in HOSTILE_KINDS:
        out.append(("hostile %s 37x19 s2" % kind, 37, 19, 2.0, hostile(kind, 37, 19)))
    return out


def grad4_for(fx, fy, seed=9):
    return np.random.default_rng(seed).normal(size=(fx * fy, 4)).astype(np.float32)
