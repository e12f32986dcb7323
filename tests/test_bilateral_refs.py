"""Host checks of the bilateral denoiser's CPU oracle (oracle/mirres_oracle.cpp: orc_bilateral) against the float64 restatement of tests/bilateral_refs.py: the
reference alone stays inside the bound the GPU test applies to the kernels, its window is the reference's, and its backward is the transpose of its forward."""
import numpy as np
import pytest

import bilateral_refs as B
from util import same_bits

CASES = B.finite_cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_oracle_stays_inside_the_float64_bound(oracle, case):
    """Every finite frame of the matrix: forward (three colour sums and the weight sum) and backward of the fp32 oracle within K 2^-24 sum w |x| of float64, per element."""
    name, fx, fy, sigma, (col, nrm, zdz) = CASES[case]
    R, S = B.forward64(fx, fy, sigma, col, nrm, zdz)
    got = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
    B.within(got, B.clamp_weight(R), S, sigma, name + " forward")
    g4 = B.grad4_for(fx, fy)
    Rb, Sb = B.backward64(fx, fy, sigma, nrm, zdz, g4)
    B.within(oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), Rb, Sb, sigma, name + " backward")
    if "hostile dead" in name:      # every weight of a zero-normal pixel is 0 (its own too: the normalised zero vector has n . n = 0 -> 1e-4^128 = 0)
        dead = ~np.any(np.asarray(nrm) != 0, axis=1)
        assert dead.sum() >= 20 and np.all(got[dead, 3] == B.EPS) and np.all(got[dead, :3] == 0)


@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_oracle_public_op_gradient_inside_its_bound(oracle, sigma):
    """ops.py:190-199 restated with the oracle: out = out4[:, :3] / out4[:, 3:4] in fp32, the gradient of sum(G out) = backward of (G / w): within K_OP of float64."""
    fx, fy = 37, 19
    col, nrm, zdz = B.asymmetric(fx, fy)
    G = np.random.default_rng(4).normal(size=(fx * fy, 3)).astype(np.float32)
    out4 = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
    g4 = np.concatenate([G / out4[:, 3:4], np.zeros((fx * fy, 1), np.float32)], axis=1).astype(np.float32)
    R, S = B.op_gradient64(fx, fy, sigma, col, nrm, zdz, G)
    B.within(oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), R, S, sigma, "op gradient s%g" % sigma, K=B.K_OP)


def test_radius_is_the_reference_expression():
    """2 * ceil(sigma * 2.5) + 1 with the product in double (denoising.cu:26,86): where sigma * 2.5f rounds down onto an integer the float product's radius is 2 short."""
    table = {0.4: (3, 5), 0.8: (5, 7), 1.2: (7, 9), 1.6: (9, 11), 2.4: (13, 15), 3.2: (17, 19), 4.4: (23, 25), 1.0: (7, 7), 2.0: (11, 11), 4.0: (21, 21), 6.0: (31, 31), 1e-4: (3, 3)}
    for s, (fl, ref) in table.items():
        assert (B.float_radius(s), B.ref_radius(s)) == (fl, ref), s


@pytest.mark.parametrize("at", [(25, 23), (0, 0), (49, 46)], ids=["interior", "corner", "far_corner"])
@pytest.mark.parametrize("sigma", [0.4, 1.6, 4.0, 1e-4])
def test_oracle_impulse_footprint(oracle, sigma, at):
    """One non-zero colour (forward) or incoming gradient (backward) on flat guides: the non-zero outputs are exactly the reference's (2 r + 1)^2 window around it,
    clipped to the frame, and each value is within the bound of the single float64 term."""
    fx, fy = 50, 47
    col, nrm, zdz, pi = B.impulse(fx, fy, at)
    must, may = B.impulse_footprint(fx, fy, sigma, at, 0.25)
    got = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
    nz = got[:, :3] != 0
    for c in range(3):
        assert not (nz[:, c] & ~may).any(), "forward: non-zero output outside the reference's window (radius %d)" % B.ref_radius(sigma)
        assert (nz[:, c] | ~must).all(), "forward: %d outputs inside the reference's window (radius %d) are zero" % (int((must & ~nz[:, c]).sum()), B.ref_radius(sigma))
    R, S = B.forward64(fx, fy, sigma, col, nrm, zdz)
    B.within(got, B.clamp_weight(R), S, sigma, "impulse forward s%g" % sigma, underflow=True)
    g4 = np.zeros((fx * fy, 4), np.float32); g4[pi] = (1.0, -0.5, 0.25, 3.0)
    gb = oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4)
    nzb = gb != 0
    for c in range(3):
        assert not (nzb[:, c] & ~may).any(), "backward: non-zero gradient outside the reference's window"
        assert (nzb[:, c] | ~must).all(), "backward: %d gradients inside the reference's window (radius %d) are zero" % (int((must & ~nzb[:, c]).sum()), B.ref_radius(sigma))
    Rb, Sb = B.backward64(fx, fy, sigma, nrm, zdz, g4)
    B.within(gb, Rb, Sb, sigma, "impulse backward s%g" % sigma, underflow=True)


def test_oracle_backward_is_the_transpose_of_its_forward(oracle):
    """The dense weight matrices of a 20 x 15 frame with dz over two decades, read off the oracle with one-hot colours / gradients: W_bwd[p, t] = W_fwd[t, p] in
    every bit (the same three factors in the same order, the depth term's dz being the centre's in one and the tap's in the other), W_fwd is NOT symmetric (so
    the test can tell the two apart), and both are the float64 matrices within the single-term bound."""
    fx, fy, sigma = 20, 15, 2.0
    n = fx * fy
    _, nrm, zdz = B.asymmetric(fx, fy)
    Wf = np.zeros((n, n), np.float32); Wb = np.zeros((n, n), np.float32)
    for j in range(0, n, 3):
        col = np.zeros((n, 3), np.float32); g4 = np.zeros((n, 4), np.float32)
        for c in range(3):
            col[j + c, c] = 1.0; g4[j + c, c] = 1.0
        o = oracle.bilateral(fx, fy, sigma, col, nrm, zdz); b = oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4)
        for c in range(3):
            Wf[:, j + c] = o[:, c]; Wb[:, j + c] = b[:, c]
    same_bits(Wb, Wf.T.copy(), "backward weights against transposed forward weights")
    asym = np.abs(Wf - Wf.T) > 0.01 * np.maximum(Wf, Wf.T)
    assert asym.mean() > 0.2, "the guides do not make the weights asymmetric enough to tell forward from backward"
    W64 = B.weights64(fx, fy, sigma, nrm, zdz)
    q = B.units(Wf, W64, W64, 2.0 ** -149)           # single weights, as on the impulse frames: one fp32 spacing below 2^-126
    print("dense forward weights: %.1f x 2^-24 w" % q)
    assert q <= B.K_BOUND
    assert B.units(Wb, B.weights64(fx, fy, sigma, nrm, zdz, backward=True), W64.T, 2.0 ** -149) <= B.K_BOUND


def test_oracle_clamps_like_fmaxf(oracle):
    """denoising.cu clamps with CUDA's max / min, which return the non-NaN operand as fmaxf / fminf do (the kernels use those): a NaN normal is a normal that
    matches nothing — weight 1e-4^128 = 0 to and from every pixel — not a NaN in every pixel of its window; a NaN dz falls back to the 1e-4 denominator."""
    fx, fy, sigma = 20, 15, 2.0
    col, nrm, zdz = B.benign(fx, fy)
    ref = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
    nrm2 = nrm.copy(); nrm2[137, 1] = np.nan
    got = oracle.bilateral(fx, fy, sigma, col, nrm2, zdz)
    assert np.isfinite(got).all()
    assert got[137, 3] == B.EPS and np.all(got[137, :3] == 0)
    # the other pixels: the frame without pixel 137's contribution
    col0 = col.copy(); col0[137] = 0
    nrm0 = nrm.copy(); nrm0[137] = 0          # a zero normal also weighs 0 everywhere
    want = oracle.bilateral(fx, fy, sigma, col0, nrm0, zdz)
    same_bits(np.delete(got, 137, axis=0), np.delete(want, 137, axis=0), "NaN normal against zero normal")
    zdz2 = zdz.copy(); zdz2[137, 1] = np.nan
    got = oracle.bilateral(fx, fy, sigma, col, nrm, zdz2)
    assert np.isfinite(got).all()
    zdz3 = zdz.copy(); zdz3[137, 1] = 0.0     # dz 0 -> denominator 1e-4 as well
    same_bits(got, oracle.bilateral(fx, fy, sigma, col, nrm, zdz3), "NaN dz against zero dz")
    assert not np.array_equal(got, ref)
