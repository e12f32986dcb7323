"""Host checks of tests/normal_refs.py, the fp32 restatement of prepare_shading_normal's backward the GPU test compares csrc/normal.hip with bit for bit: it is the
gradient of the formula (float64 autograd, benign rows), and at the kinks it follows nerf/renderutils/c_src/normal.cu:40-44, 77-89 and vec3f.h:93-104."""
import numpy as np
import pytest

import normal_refs as N

FLAGS = [(True, True), (True, False), (False, True), (False, False)]


def _one(kind, two_sided=True, opengl=True, dout=(0.7, -1.3, 0.4)):
    row = [a[None] for a in N.kink_row(kind)]
    g, dp = N.backward32(*row, two_sided, opengl, np.asarray(dout, np.float32)[None])
    return dict(zip(N.NAMES, [x[0] for x in g])), float(dp[0]), row


def test_restatement_is_the_gradient_of_the_formula(oracle):
    """The wrapper's case (442 rows, view_pos and geom_nrm broadcast, their gradients summed): every element within util.elementwise of float64 autograd at the
    rtol recorded in normal_refs (the GPU test allows four times that), and the forward restatement (oracle.prepare_shading_normal) is the formula's value."""
    ins, dout = N.wrapper_inputs()
    worst = 0.0
    for two_sided, opengl in FLAGS:
        g32 = N.wrapper_gradients32(ins, two_sided, opengl, dout)
        g64 = N.gradients64(ins, two_sided, opengl, dout)
        for name, a, b in zip(N.NAMES, g32, g64):
            assert a.shape == b.shape and np.abs(b).max() > 0, name
            worst = max(worst, N.elementwise_rtol(a, b))
        import torch
        fwd64 = N.formula64(*[torch.from_numpy(np.asarray(a, np.float64)) for a in ins], two_sided, opengl).numpy()
        # dp carries a few ulp (1e-7) and is divided by 0.1 before it blends two unit-size vectors
        np.testing.assert_allclose(oracle.prepare_shading_normal(*ins, two_sided, opengl), fwd64, rtol=0, atol=5e-6)
    print("restatement against float64 autograd: rtol %.3e at atol_scale %g (recorded %.3e)" % (worst, N.WRAPPER_ATOL_SCALE, N.WRAPPER_RTOL_MEASURED))
    assert 0 < worst <= N.WRAPPER_RTOL_MEASURED


@pytest.mark.parametrize("two_sided,opengl", FLAGS)
def test_restatement_rows_against_float64(two_sided, opengl):
    """4096 independent benign rows, EVERY one: each gradient element within 1e-4 of the row's largest gradient magnitude (rows are not normalised:
    |v| ~ 0.1 .. 4; measured: 7e-6 at most).  The rows take every branch many times: dp below 0, inside (0, 0.1) and above, flipped and not."""
    ins = N.benign_rows(4096)
    dout = np.random.default_rng(5).normal(size=(4096, 3)).astype(np.float32)
    g32, dp = N.backward32(*ins, two_sided, opengl, dout)
    g64 = N.gradients64(ins, two_sided, opengl, dout)
    assert (dp < 0).sum() > 200 and ((dp > 0) & (dp < N.THRESHOLD)).sum() > 50 and (dp > N.THRESHOLD).sum() > 200
    view = N._safe_normalize(ins[1] - ins[0])
    flips = N._dot(view, ins[5]) < 0
    assert 1000 < flips.sum() < 3000
    for name, a, b in zip(N.NAMES, g32, g64):
        err = np.abs(a - b).max(axis=1); scale = np.abs(b).max(axis=1)
        bad = err > 1e-4 * scale + 1e-6
        assert not bad.any(), "%s: rows %r" % (name, np.flatnonzero(bad)[:8])


def test_clamp_passes_the_gradient_at_both_ends_and_not_outside():
    """normal.cu:86: d_dp = dp < 0 || dp > 0.1 ? 0 : d_t / 0.1 — passed at dp == 0 and dp == 0.1 exactly, zero either side."""
    g, dp, _ = _one("dp_zero")
    assert dp == 0.0 and np.abs(g["view_pos"]).max() > 0 and np.array_equal(g["pos"], -g["view_pos"])
    g, dp, _ = _one("dp_threshold")
    assert np.float32(dp) == N.THRESHOLD and np.abs(g["view_pos"]).max() > 0
    g, dp, _ = _one("dp_below_threshold")
    assert np.float32(dp) == np.nextafter(N.THRESHOLD, np.float32(0)) and np.abs(g["view_pos"]).max() > 0
    g, dp, _ = _one("dp_above_threshold")
    assert np.float32(dp) == np.nextafter(N.THRESHOLD, np.float32(1)) and not g["view_pos"].any() and not g["pos"].any()
    assert not g["geom_nrm"].any()                      # t == 1: the output is the shading normal alone
    g, dp, _ = _one("dp_negative")
    assert dp < 0 and not g["view_pos"].any() and not g["pos"].any()
    assert np.array_equal(g["geom_nrm"], np.asarray((0.7, -1.3, 0.4), np.float32))          # t == 0: the output is geom_nrm
    assert not g["perturbed_nrm"].any() and not g["smooth_nrm"].any() and not g["smooth_tng"].any()


def test_nothing_flows_through_a_clamped_perturbation_z():
    """normal.cu:40-44: `if (perturbed_nrm.z > 0.0f)` — at p.z == 0 and below, neither p.z nor (through that term) smooth_nrm receives anything."""
    for kind in ("pz_zero", "pz_negative"):
        g, _, row = _one(kind)
        assert g["perturbed_nrm"][2] == 0 and g["perturbed_nrm"][:2].any(), kind
    # smooth_nrm still receives through the bitangent; with p.y == 0 as well nothing is left
    row = [a[None].copy() for a in N.kink_row("pz_negative")]
    row[2][0, 1] = 0
    g, _ = N.backward32(*row, True, True, np.asarray([[0.7, -1.3, 0.4]], np.float32))
    assert not g[3].any()


def test_zero_length_vectors_pass_no_gradient():
    """vec3f.h:93-104: bwdSafeNormalize adds nothing for l == 0 (and safeNormalize returns 0)."""
    g, _, _ = _one("zero_nrm")
    assert not g["smooth_nrm"].any() and np.isfinite(np.concatenate(list(g.values()))).all()
    g, _, _ = _one("zero_tng")
    assert not g["smooth_tng"].any() and np.isfinite(np.concatenate(list(g.values()))).all()
    g, dp, _ = _one("zero_view")
    assert dp == 0.0 and not g["pos"].any() and not g["view_pos"].any()
    g, _, _ = _one("parallel")                          # bitangent = normalize(0) = 0: nothing flows back through the cross product
    assert np.isfinite(np.concatenate(list(g.values()))).all() and g["perturbed_nrm"][1] == 0


def test_two_sided_flip_is_strict():
    """normal.cu:117,156: the flip needs dot(view, geom) < 0 — at exactly 0 the row is not flipped; a flipped row's geom gradient changes sign with the flag."""
    row = [a[None] for a in N.kink_row("vg_zero")]
    d = np.asarray([[0.7, -1.3, 0.4]], np.float32)
    a, _ = N.backward32(*row, True, True, d); b, _ = N.backward32(*row, False, True, d)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    row = [a[None] for a in N.kink_row("vg_negative")]
    a, _ = N.backward32(*row, True, True, d); b, _ = N.backward32(*row, False, True, d)
    assert not np.array_equal(a[5], b[5])


def test_mixed_rows_hold_every_kink():
    ins, where = N.mixed_rows(255)
    assert set(where) == set(N.KINKS) and where[N.KINKS[-1]] == 254
    for kind, i in where.items():
        for a, v in zip(ins, N.kink_row(kind)):
            assert np.array_equal(a[i], v)
    assert N.mixed_rows(1)[1] == {}
    dout = np.random.default_rng(6).normal(size=(255, 3)).astype(np.float32)
    for two_sided, opengl in FLAGS:
        N.check_kink_conventions(N.backward32(*ins, two_sided, opengl, dout)[0], where, "restatement %d%d" % (two_sided, opengl))
