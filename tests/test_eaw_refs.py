"""Host checks of the a-trous test infrastructure (tests/eaw_refs.py): the CPU oracle (oracle/orc_kernels.hpp: eaw_pixel, fp32) against the float64 restatement
written from EAWDenoise.slang:50-174 and against adjoint_refs.eaw on every frame of the matrix, the denormal frame, the deliberate mistakes (each must change the
restatement, or the frames cannot see it), conditions on the inputs so that no class quietly tests nothing, and what fp32 arithmetic alone costs the gradients
against the bound tests/test_gpu_eaw.py holds the HIP adjoints to.  Figures are printed (pytest -s)."""
import numpy as np
import pytest

import eaw_refs as E

BOUND = 2e-6       # relative, denominator |ref| + 1e-6: about three times the oracle's own 6e-7, two orders under any one-tap mistake


def _t64(fx, fy, steps, phis, occ, col, nrm, pos):
    import torch
    out, _ = E.eaw_torch(fx, fy, steps, phis, occ, col, nrm, pos, torch.float64)
    return out.detach().numpy()


@pytest.mark.parametrize("kind", E.KINDS)
def test_oracle_against_both_float64_restatements(oracle, kind):
    """Every SIZES x STEPS x PHIS frame of `kind` (thresh without NaN): oracle.eaw within 2e-6 relative (denominator |ref| + 1e-6) of `restated` and of
    adjoint_refs.eaw in float64.  Measured over the whole matrix: 6.1e-7 against either, on `hole` (the two float64 restatements agree to 1e-15)."""
    worst = [0.0, 0.0, 0.0]
    for fx, fy in E.SIZES:
        occ, col, nrm, pos = E.frame(kind, fx, fy)
        for step in E.STEPS:
            for k, phis in enumerate(E.PHIS):
                got = E.oracle_eaw(kind, fx, fy, step, k)
                r1 = E.restated(fx, fy, step, phis, occ, col, nrm, pos)
                r2 = _t64(fx, fy, [step], phis, occ, col, nrm, pos)
                e = (E.rel_err(got, r1), E.rel_err(got, r2), E.rel_err(r1, r2))
                worst = [max(a, b) for a, b in zip(worst, e)]
                assert e[0] <= BOUND and e[1] <= BOUND, "%s %dx%d step %d phis %r: oracle against restated %.3e, against adjoint_refs.eaw %.3e" % (kind, fx, fy, step, phis, e[0], e[1])
                assert e[2] <= 1e-12, "%s %dx%d step %d: the two float64 restatements differ by %.3e" % (kind, fx, fy, step, e[2])
                bg = occ < np.float32(0.1)
                assert np.array_equal(got[bg].view(np.uint32), col[bg].view(np.uint32)), "background pixels are copies"
    print("%s: oracle against restated %.3e, against adjoint_refs.eaw %.3e (bound %.0e); restatements apart %.1e" % (kind, worst[0], worst[1], BOUND, worst[2]))


@pytest.mark.parametrize("chain", E.CHAINS)
def test_oracle_chains_against_float64(oracle, chain):
    """The drivers' schedules (int() of the halved float step: (2, 3) runs 2, 1, 0) on 19 x 27 and 17 x 15, rand and smooth, both phis: the fp32 oracle chained
    against the float64 chain, same 2e-6.  Measured: 6.9e-7 after three passes, 7.3e-7 after four."""
    steps = E.chain_steps(*chain)
    worst = 0.0
    for fx, fy in ((19, 27), (17, 15)):
        for kind in ("rand", "smooth"):
            occ, col, nrm, pos = E.frame(kind, fx, fy)
            for phis in E.PHIS:
                cur = col
                for s in steps:
                    cur = oracle.eaw(fx, fy, s, *phis, occ, cur, nrm, pos)
                e = E.rel_err(cur, _t64(fx, fy, steps, phis, occ, col, nrm, pos))
                worst = max(worst, e)
                assert e <= BOUND, (chain, kind, fx, fy, phis, e)
    print("chain %r = steps %r: oracle against float64 %.3e (bound %.0e)" % (chain, steps, worst, BOUND))
    assert E.chain_steps(2, 3) == [2, 1, 0] and E.chain_steps(8, 4) == [8, 4, 2, 1] and E.chain_steps(1, 1) == [1]


def test_denormal_weights_reach_the_output(oracle):
    """denormal_frame: every weight between pixels of unlike parity is exp(-95) ~ 5.5e-42.  The oracle's output on the even pixels lies strictly between 0 and
    1e-20 (4.7e-24 .. 5.5e-24 here) — flushing the weights or their products with the kernel to zero would give exactly 0 — and within 1e-3 relative of
    float64 (a denormal weight carries 12 bits)."""
    d = E.DENORMAL
    occ, col, nrm, pos = E.denormal_frame()
    got = oracle.eaw(d["fx"], d["fy"], d["step"], *d["phis"], occ, col, nrm, pos)
    even = col[:, 0] == 0
    assert even.sum() == 32 and (~even).sum() == 31
    print("denormal frame: even pixels %.3e .. %.3e" % (got[even].min(), got[even].max()))
    assert (got[even] > 0).all() and (got[even] < 1e-20).all()
    ref = E.restated(d["fx"], d["fy"], d["step"], d["phis"], occ, col, nrm, pos)
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-3
    w = np.float32(np.exp(-95.0))
    assert 0 < w < np.finfo(np.float32).tiny


def _caught(mutate, cases):
    """The largest relative change `mutate` makes over the cases, and the case where."""
    best = (0.0, None)
    for name, fx, fy, step, phis, (occ, col, nrm, pos) in cases:
        a = E.restated(fx, fy, step, phis, occ, col, nrm, pos)
        b = E.restated(fx, fy, step, phis, occ, col, nrm, pos, mutate=mutate)
        e = max(E.rel_err(y, x) for x, y in zip(a, b)) if isinstance(a, list) else E.rel_err(b, a)
        if e > best[0]:
            best = (e, name)
    return best


def _case(kind, fx, fy, step, k=1):
    return ("%s %dx%d step %d" % (kind, fx, fy, step), fx, fy, step, E.PHIS[k], E.frame(kind, fx, fy))


def test_every_forward_mutation_is_seen_by_a_frame_of_the_set():
    """Each deliberate mistake of `restated` changes its output by more than 1e-3 relative on a frame of the matrix — so the bit comparison of kernel and oracle
    with these frames, and the 2e-6 comparison of the oracle with `restated`, cannot pass with that mistake in either:
      clamp_border         all_fg 2 x 2 step 1 (taps leave on two sides at once) and 17 x 15 step 2
      fy_for_x             all_fg 5 x 3 step 1 (`ux < fy` drops columns 3, 4); a square frame cannot see it
      step_min_1           smooth 17 x 15 step 0 (all 25 taps on the centre: the output is the input)
      le_threshold         thresh 17 x 15 step 1 (a pixel of occupancy exactly 0.1f is foreground)
      skip_bg_taps         hole 17 x 15 step 1 (the one background pixel IS a tap of its neighbours) and rand
      corner_weight        all_fg 16 x 16 step 1
      no_normal_weight     rand 17 x 15 step 1 (random unit normals)
      shared_colour_weight the five unlike buffers of the finish on smooth 19 x 27 guides."""
    table = {
        "clamp_border": [_case("all_fg", 2, 2, 1), _case("all_fg", 17, 15, 2)],
        "fy_for_x": [_case("all_fg", 5, 3, 1)],
        "step_min_1": [_case("smooth", 17, 15, 0)],
        "le_threshold": [_case("thresh", 17, 15, 1)],
        "skip_bg_taps": [_case("hole", 17, 15, 1), _case("rand", 17, 15, 1)],
        "corner_weight": [_case("all_fg", 16, 16, 1)],
        "no_normal_weight": [_case("rand", 17, 15, 1)],
    }
    occ, _, nrm, pos = E.frame("smooth", 19, 27)
    s = E.five_buffers(19, 27)
    table["shared_colour_weight"] = [("five buffers 19x27 step 2", 19, 27, 2, E.PHIS[0], (occ, [s[1], s[2], s[4] + s[5], s[4], s[5]], nrm, pos))]
    assert sorted(table) == sorted(E.MUTATIONS)
    for m in E.MUTATIONS:
        e, where = _caught(m, table[m])
        print("%-22s changes %-28s by %.3e" % (m, where, e))
        assert e > 1e-3, "%s goes unseen (largest change %.3e)" % (m, e)
    # a square frame cannot see fy_for_x: the reason the matrix has 3 x 5 and 5 x 3
    assert _caught("fy_for_x", [_case("all_fg", 16, 16, 1)])[0] == 0.0


def test_the_inputs_are_what_they_claim(oracle):
    """thresh holds every listed occupancy at 255 px (and NaN when asked); about 30 % background in rand; island / hole have one odd pixel; at step 64 no
    off-centre tap is inside any frame of SIZES up to 64 pixels long (on the two 257-pixel strips only the taps 64 and 128 along the strip), at step 8 some are; smooth normals lie within a few degrees of +z and all three weights are alive."""
    occ = E.frame("thresh", 17, 15)[0]
    for v in E.THRESH_VALUES:
        assert (occ == np.float32(v)).sum() >= 30, v
    assert not np.isnan(occ).any() and np.isnan(E.frame("thresh", 17, 15, nan=True)[0]).sum() >= 30
    assert np.float32(0.0999999) < np.float32(0.1) < np.float32(0.1000001)
    bgf = (E.frame("rand", 19, 27)[0] < 0.1).mean()
    assert 0.2 < bgf < 0.4
    for fx, fy in E.SIZES:
        if max(fx, fy) <= 64:
            assert E.taps_inside(fx, fy, 64) == 0, (fx, fy)
        else:       # the two 257-pixel strips: the taps 64 and 128 along the strip are inside, nothing across it
            assert E.taps_inside(fx, fy, 64) == 2 * ((257 - 64) + (257 - 128)), (fx, fy)
        assert (E.frame("island", fx, fy)[0] > 0.5).sum() == 1 and (E.frame("hole", fx, fy)[0] < 0.5).sum() == 1
        assert not E.frame("all_bg", fx, fy)[0].any() and E.frame("all_fg", fx, fy)[0].all()
    assert E.taps_inside(19, 27, 8) > 0 and E.taps_inside(17, 15, 8) > 0 and E.taps_inside(16, 16, 8) > 0 and E.taps_inside(7, 1, 8) == 0
    nrm = E.frame("smooth", 19, 27)[2]
    assert np.degrees(np.arccos(nrm[:, 2])).max() < 10 and np.allclose(np.linalg.norm(E.frame("rand", 19, 27)[2], axis=1), 1, atol=1e-6)
    # all three weights alive: dropping any one of them changes the smooth frame at the default phis
    occ, col, nrm, pos = E.frame("smooth", 19, 27)
    base = E.restated(19, 27, 1, E.PHIS[0], occ, col, nrm, pos)
    for k in range(3):
        ph = list(E.PHIS[0]); ph[k] = 1e30
        assert E.rel_err(E.restated(19, 27, 1, ph, occ, col, nrm, pos), base) > 1e-2, k


@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_nonfinite_frames_poison_some_outputs_and_spare_most(oracle, kind):
    """Every non-finite class leaves at least 60 % of the oracle's outputs finite and poisons at least 5 %, at steps 1 and 2.  `colours`: at least 5 % of the
    outputs are not finite.  The other three classes CANNOT produce a non-finite output, by the filter's own lines (EAWDenoise.slang:152-162): only colours are
    summed; a NaN or Inf - Inf squared distance of normals or positions becomes 0 through max(., 0) and its weight 1, an overflowing one gives weight 0; and the
    centre tap's three weights are min(exp(-0 / phi), 1) = 1 (or min(NaN, 1) = 1), so the weight sum is at least 9 / 64.  For them `poisoned` means: differs
    from the output on the clean guides at the frame's own phis — the weight of a poisoned tap became 0 or 1 — on at least 5 % of the outputs, all finite."""
    fx, fy = E.NONFINITE_DIMS
    clean = E.frame("rand", fx, fy, seed=11)
    for name, phis, (occ, col, nrm, pos) in E.nonfinite(kind):
        for step in (1, 2):
            out = oracle.eaw(fx, fy, step, *phis, occ, col, nrm, pos)
            fin = np.isfinite(out).mean()
            assert fin >= 0.6, (name, step, fin)
            if kind == "colours":
                hit = 1 - fin
            else:
                assert fin == 1.0, (name, step, fin)
                base = oracle.eaw(fx, fy, step, *(E.PHIS[0] if kind == "phis" else phis), occ, clean[1], clean[2], clean[3])
                hit = (out != base).mean()
            print("%s step %d: %.1f %% of the outputs finite, %.1f %% poisoned" % (name, step, 100 * fin, 100 * hit))
            assert hit >= 0.05, (name, step, hit)


@pytest.mark.parametrize("kind", E.ADJ_KINDS)
def test_float32_autograd_of_the_restatement_is_well_inside_the_gradient_bound(kind):
    """The bound tests/test_gpu_eaw.py applies to the HIP adjoints (util.elementwise at its defaults: rtol 1e-3 plus 1e-4 of the gradient's scale, against
    float64 autograd of adjoint_refs.eaw) has room for fp32 arithmetic: the same restatement evaluated and differentiated in float32 torch uses at most a few
    per cent of it on exactly the GPU test's inputs (measured: 0.012 of the bound for one pass, 0.008 through the chains), and where the float64 gradient
    is identically zero the float32 one is as well."""
    worst = 0.0
    for fx, fy in E.ADJ_SIZES:
        for step in E.ADJ_STEPS:
            for k in range(len(E.PHIS)):
                for a, b in zip(E.grads32(kind, fx, fy, (step,), k), E.grads64(kind, fx, fy, (step,), k)):
                    assert np.isfinite(b).all()
                    worst = max(worst, E.bound_ratio(a, b))
    chain = 0.0
    if kind in ("rand", "smooth"):
        for ch in E.ADJ_CHAINS:
            for k in range(len(E.PHIS)):
                for a, b in zip(E.grads32(kind, 19, 27, tuple(E.chain_steps(*ch)), k), E.grads64(kind, 19, 27, tuple(E.chain_steps(*ch)), k)):
                    chain = max(chain, E.bound_ratio(a, b))
    print("%s: float32 autograd uses %.4f of the gradient bound for one pass, %.4f through the chains" % (kind, worst, chain))
    assert worst <= 1.0 and chain <= 1.0
