"""Independent numpy restatements for the stage-0 radiance network (no import from the package): the degree-4 spherical-harmonics direction encoder in float32 with
exactly the operation order DESIGN.md section 5.14 fixes (every numpy float32 operation rounds once, there is no fused multiply-add), the same functions in float64
from the published formulas, the five bias-free layers in float64, and the forward-error bound of their fp32 fmaf chains.

The bounds, derived (u = 2^-24, gamma_K = K u / (1 - K u); Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a chain of K fused multiply-adds from
0 has forward error <= gamma_K * sum |a_k| |w_k|):

  a layer out = W . a evaluated in fp32 on inputs a + da:   |d out| <= sum_k |da_k| |w_k| + gamma_K * sum_k (|a_k| + |da_k|) |w_k|;
  ReLU is 1-Lipschitz: it does not enlarge |d out|;
  sigma = mrf_exp(h16[0]), mrf_exp within 2 ulp:            |sigma - exp(h)| / exp(h) <= |dh| + 2 * 2^-23   (the density head's bound, tests/density_refs.py);
  rgb = mrf_sigmoid(h) = 1 / (1 + mrf_exp(-h)):             the logistic function has slope <= 1/4, so the chain's |dh| moves it by <= |dh| / 4; the evaluation
      itself: e' = e (1 + 4 u) (2 ulp), t = fl(1 + e') (one u), r = fl(1 / t) (one u): r / s - 1 = - e de / (1 + e) - d1 + d2, at most 6 u in magnitude,
      so |d rgb| <= |dh| / 4 + 6 u s (1 + 2^-10) + 2^-126 (second-order terms folded into the factor; the smallest normal number where mrf_exp over- or underflows).

  sh32 against sh64 on the same fp32 direction (sh_bound): s = (dx dx + dy dy) + dz dz is three products and two sums of non-negative numbers, relative error <=
  3 u; n = sqrt(s): 3 u / 2 + u; a component x = dx / n: 7 u / 2 <= 4 u.  Every output is a polynomial of degree <= 3 in components of magnitude <= 1; written
  as a sum of monomials c_m m its value and every intermediate are bounded by A = sum |c_m|.  A relative perturbation e of every component moves a monomial of degree
  p by p e |m|: at most 3 * 4 u A in all.  An output takes at most 6 rounded operations (out[9]: x2, y2, 3 x2, the sum, c y, the product), each moving the result
  by at most u A, and its fp32 literal differs from the published constant by at most u relative: |d out| <= (12 + 6 + 1) u A (1 + 2^-10)."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
ULP = 2.0 ** -23

# the reference's literals (shencoder/src/shencoder.cu:50-68), rounded to fp32 when used
C0 = F32(0.28209479177387814)
C1 = F32(0.48860251190291987)
C2A, C2B, C2C, C2D = F32(1.0925484305920792), F32(0.94617469575755997), F32(0.31539156525251999), F32(0.54627421529603959)
C3A, C3B, C3C, C3D, C3E = F32(0.59004358992664352), F32(2.8906114426405538), F32(0.45704579946446572), F32(0.3731763325901154), F32(1.4453057213202769)


def gamma(n):
    return n * U / (1.0 - n * U)


def sh32(d):
    """d f32 [n, 3] -> f32 [n, 16], bit for bit what csrc/radiance.hip computes; one operation per line."""
    d = np.asarray(d, F32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    out = np.empty((len(d), 16), F32)
    with np.errstate(all="ignore"):
        sxx = dx * dx
        syy = dy * dy
        szz = dz * dz
        s = sxx + syy
        s = s + szz
        n = np.sqrt(s)
        x = dx / n
        y = dy / n
        z = dz / n
        xy = x * y
        xz = x * z
        yz = y * z
        x2 = x * x
        y2 = y * y
        z2 = z * z
        out[:, 0] = C0                                 # a constant whatever the direction, as the reference's; a zero or NaN direction shows in outputs 1 .. 15
        out[:, 1] = -C1 * y
        out[:, 2] = C1 * z
        out[:, 3] = -C1 * x
        out[:, 4] = C2A * xy
        out[:, 5] = -C2A * yz
        t = C2B * z2
        out[:, 6] = t - C2C
        out[:, 7] = -C2A * xz
        t = C2D * x2
        v = C2D * y2
        out[:, 8] = t - v
        t = C3A * y
        v = F32(-3.0) * x2
        v = v + y2
        out[:, 9] = t * v
        t = C3B * xy
        out[:, 10] = t * z
        t = C3C * y
        v = F32(5.0) * z2
        v = F32(1.0) - v
        out[:, 11] = t * v
        t = C3D * z
        v = F32(5.0) * z2
        v = v - F32(3.0)
        out[:, 12] = t * v
        t = C3C * x
        v = F32(5.0) * z2
        v = F32(1.0) - v
        out[:, 13] = t * v
        t = C3E * z
        v = x2 - y2
        out[:, 14] = t * v
        t = C3A * x
        v = -x2
        w = F32(3.0) * y2
        v = v + w
        out[:, 15] = t * v
    return out


def sh64(d):
    """The real spherical harmonics of degree l < 4 of d / |d| in float64, in the reference's order and sign convention, from the published formulas with the
    constants computed here."""
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        u = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    pi = np.pi
    k1 = np.sqrt(3.0 / (4.0 * pi))
    k2 = 0.5 * np.sqrt(15.0 / pi)
    k3a, k3b, k3c, k3d, k3e = 0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi), 0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(7.0 / pi), 0.25 * np.sqrt(105.0 / pi)
    return np.stack([
        np.full_like(x, 0.5 * np.sqrt(1.0 / pi)),
        -k1 * y, k1 * z, -k1 * x,
        k2 * x * y, -k2 * y * z, 0.25 * np.sqrt(5.0 / pi) * (3.0 * z * z - 1.0), -k2 * x * z, 0.5 * k2 * (x * x - y * y),
        -k3a * y * (3.0 * x * x - y * y), k3b * x * y * z, -k3c * y * (5.0 * z * z - 1.0), k3d * z * (5.0 * z * z - 3.0), -k3c * x * (5.0 * z * z - 1.0),
        k3e * z * (x * x - y * y), -k3a * x * (x * x - 3.0 * y * y)], axis=1)


def sh_abs_coefficients():
    """A of the module docstring per output: the sum of the absolute coefficients of the output written as a sum of monomials."""
    pi = np.pi
    k1 = np.sqrt(3.0 / (4.0 * pi)); k2 = 0.5 * np.sqrt(15.0 / pi)
    k3a, k3b, k3c, k3d, k3e = 0.25 * np.sqrt(35.0 / (2.0 * pi)), 0.5 * np.sqrt(105.0 / pi), 0.25 * np.sqrt(21.0 / (2.0 * pi)), 0.25 * np.sqrt(7.0 / pi), 0.25 * np.sqrt(105.0 / pi)
    return np.array([0.5 * np.sqrt(1.0 / pi), k1, k1, k1, k2, k2, 0.25 * np.sqrt(5.0 / pi) * 4.0, k2, k2, 4.0 * k3a, k3b, 6.0 * k3c, 8.0 * k3d, 6.0 * k3c, 2.0 * k3e, 4.0 * k3a])


def sh_bound():
    """f64 [16]: the bound on |sh32(d) - sh64(d)| for a finite non-zero fp32 direction whose squares neither overflow nor underflow (module docstring)."""
    return 19.0 * U * sh_abs_coefficients() * (1.0 + 2.0 ** -10)


def _layer(a, da, w):
    """out = a . w^T in float64 and the bound on the fp32 chain's error, inputs off by at most da."""
    w = np.asarray(w).astype(np.float64)
    K = w.shape[1]
    with np.errstate(invalid="ignore"):
        out = a @ w.T
        dout = da @ np.abs(w).T + gamma(K) * ((np.abs(a) + da) @ np.abs(w).T)
    return out, dout


def _forward(feat, sh, weights, dsh=None):
    w0, w1, c0, c1, c2 = weights
    a = np.asarray(feat).astype(np.float64); s = np.asarray(sh).astype(np.float64)
    acc, d0 = _layer(a, np.zeros_like(a), w0)
    h1 = np.maximum(acc, 0.0)
    h16, d16 = _layer(h1, d0, w1)
    cin = np.concatenate([s, h16[:, 1:]], axis=1)
    dcin = np.concatenate([np.zeros_like(s) if dsh is None else np.broadcast_to(np.asarray(dsh, np.float64), s.shape), d16[:, 1:]], axis=1)
    nan = np.isnan(cin).any(axis=1)
    cin0 = np.where(nan[:, None], 0.0, cin)                       # rows with a NaN direction: evaluated apart, so that 0 * NaN of a zero weight stays out of the bound
    a0, da0 = _layer(cin0, dcin, c0)
    a1, da1 = _layer(np.maximum(a0, 0.0), da0, c1)
    h3, dh3 = _layer(np.maximum(a1, 0.0), da1, c2)
    with np.errstate(over="ignore"):
        sigma = np.exp(h16[:, 0])
        rgb = 1.0 / (1.0 + np.exp(-h3))
    rgb[nan] = np.nan                                             # NaN sh inputs meet every neuron of the first layer (fmaf(NaN, w, acc) is NaN for any w): NaN rgb
    return dict(h16=h16, sigma=sigma, rgb=rgb, h3=h3), dict(h16=d16, sigma_rel=d16[:, 0] + 2.0 * ULP, rgb=dh3 / 4.0 + 6.0 * U * rgb * (1.0 + 2.0 ** -10) + 2.0 ** -126)


def forward64(feat, sh, weights):
    """feat [n, 32] and sh [n, 16] (the device's own, bit-checked) and weights = (w0 [64, 32], w1 [16, 64], c0 [64, 31], c1 [64, 64], c2 [3, 64]) -> dict of float64
    h16 [n, 16], sigma [n] = exp(h16[:, 0]), rgb [n, 3] (NaN where the direction's sh is), h3 [n, 3] (the last layer before the logistic function)."""
    return _forward(feat, sh, weights)[0]


def forward_bound(feat, sh, weights, dsh=None):
    """The bound of the module docstring on the fp32 evaluation against forward64 on the same inputs -> dict of h16 [n, 16] (absolute), sigma_rel [n] (relative),
    rgb [n, 3] (absolute).  dsh [16]: the sh inputs themselves are off by at most this against the yardstick (a closed form in the exact direction), default 0."""
    return _forward(feat, sh, weights, dsh)[1]
