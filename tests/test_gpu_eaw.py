"""GPU parity of the edge-avoiding a-trous denoiser (csrc/eaw.hip: k_eaw, k_eaw5, k_eaw_bwd, k_eaw_bwd_sums, k_eaw_bwd_gather) on the hostile frames of
tests/eaw_refs.py: frames narrower than the footprint, non-square frames, ragged and exactly full last blocks, steps 0 (all taps on the centre) to 64 (no tap
inside), occupancies around the 0.1 threshold, lone foreground and background pixels, denormal weights, non-finite colours, guides and phis.

Forward kernels and the CPU oracle (oracle/orc_kernels.hpp: eaw_pixel) are the same sequence of IEEE fp32 operations in the same order, with the mrf_exp of
include/mirres_fmath.h on both sides, so they are compared bit for bit; tests/test_eaw_refs.py holds the oracle to two float64 restatements on the same frames
and shows that each of eight deliberate mistakes changes them.  The adjoints are compared element by element with float64 autograd of adjoint_refs.eaw at
util.elementwise's defaults (rtol 1e-3 plus 1e-4 of the gradient's scale), of which fp32 arithmetic alone uses about one per cent (test_eaw_refs.py)
and the HIP adjoints, measured on the MI355X, 0.011 for one pass in either form and 0.007 through the chains (printed with -s)."""
import ctypes as C

import numpy as np
import pytest

import eaw_refs as E
from util import same_bits, elementwise

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _cu(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _same_bits_or_both_nan(got, ref, what):
    """Equal bits, or NaN on both sides: the payload of a NaN the arithmetic itself makes (Inf - Inf, 0 * Inf) is the processor's choice."""
    g = np.ascontiguousarray(got, dtype=np.float32); r = np.ascontiguousarray(ref, dtype=np.float32)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    same = (g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))
    assert same.all(), "%s: %d of %d values differ; first: got %r want %r" % (what, int((~same).sum()), same.size, g[~same][:4], r[~same][:4])


def _abi_eaw(fx, fy, step, phis, d_occ, d_col, d_nrm, d_pos):
    """mirres_eaw through the C ABI into a buffer pre-filled with SENTINEL -> device tensor."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    out = torch.full((fx * fy, 3), SENTINEL, device="cuda")
    check(lib().mirres_eaw(fx, fy, int(step), *[float(v) for v in phis], d_occ.data_ptr(), d_col.data_ptr(), d_nrm.data_ptr(), d_pos.data_ptr(), out.data_ptr(), stream_ptr()), "mirres_eaw")
    return out


def _forward_both_ways(fx, fy, step, phis, dev, ref, what, compare=same_bits):
    """One pass through Denoising.EAWDenoise_run_no_di and through the C ABI with a sentinel-filled output, both against `ref`; background pixels are the input's bits."""
    from mirres_restir_nerf_mesh_amd.Denoising import EAWDenoise_run_no_di
    a = EAWDenoise_run_no_di(None, *phis, fx, fy, step, *dev).cpu().numpy()
    b = _abi_eaw(fx, fy, step, phis, *dev).cpu().numpy()
    compare(a, ref, what + " (EAWDenoise_run_no_di)")
    compare(b, ref, what + " (C ABI)")
    assert not (b == SENTINEL).any(), what + ": a pixel was not written"
    return b


# ------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("kind", E.KINDS)
def test_forward_bits_on_the_whole_matrix(oracle, kind):
    """k_eaw on every SIZES x STEPS x PHIS frame of `kind` (thresh also with NaN occupancies, which are foreground): equal to oracle.eaw in every bit, through
    the Python surface and through the C ABI; every pixel of a sentinel-filled output is written; background pixels carry the input's bits; all_bg returns
    the input."""
    for nan in ((False, True) if kind == "thresh" else (False,)):
        for fx, fy in E.SIZES:
            occ, col, nrm, pos = E.frame(kind, fx, fy, nan=nan)
            dev = [_cu(a) for a in (occ, col, nrm, pos)]
            bg = occ < np.float32(0.1)
            for step in E.STEPS:
                for k, phis in enumerate(E.PHIS):
                    got = _forward_both_ways(fx, fy, step, phis, dev, E.oracle_eaw(kind, fx, fy, step, k, nan=nan), "%s%s %dx%d step %d phis %d" % (kind, " +NaN" if nan else "", fx, fy, step, k))
                    assert np.array_equal(got[bg].view(np.uint32), col[bg].view(np.uint32)), "background pixels are not copies"
                    if kind == "all_bg":
                        assert np.array_equal(got.view(np.uint32), col.view(np.uint32))


def test_forward_keeps_denormal_weights(oracle):
    """eaw_refs.denormal_frame: every weight between unlike pixels is exp(-95) = 5.5e-42.  The kernel's output equals the oracle's in every bit, and on the
    even pixels it lies strictly between 0 and 1e-20: a kernel that flushed denormal weights, or their products with the spline weight, would return 0."""
    d = E.DENORMAL
    frame = E.denormal_frame()
    ref = oracle.eaw(d["fx"], d["fy"], d["step"], *d["phis"], *frame)
    got = _forward_both_ways(d["fx"], d["fy"], d["step"], d["phis"], [_cu(a) for a in frame], ref, "denormal frame")
    even = frame[1][:, 0] == 0
    assert (got[even] > 0).all() and (got[even] < 1e-20).all()


@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_forward_on_nonfinite_frames(oracle, kind):
    """Inf / NaN colours, Inf and overflowing positions, NaN normals, phis of 1e-30, 1e30, +Inf and 1e-38, at steps 1 and 2: equal bits, or NaN on both sides —
    NaNs are compared by position and everything else by bits, because the payload of a NaN that Inf - Inf or 0 * Inf makes differs between the host processor
    and the GPU (util.same_bits, which compares payloads, is not loosened; the three classes that cannot make a NaN are held to it).  fminf / fmaxf semantics
    decide the values here: min(NaN, 1) = 1, max(NaN, 0) = 0."""
    fx, fy = E.NONFINITE_DIMS
    for name, phis, frame in E.nonfinite(kind):
        dev = [_cu(a) for a in frame]
        for step in (1, 2):
            ref = oracle.eaw(fx, fy, step, *phis, *frame)
            got = _forward_both_ways(fx, fy, step, phis, dev, ref, "%s step %d" % (name, step), compare=_same_bits_or_both_nan if kind == "colours" else same_bits)
            assert np.isfinite(got).mean() >= 0.6


def test_forward_refuses_to_run_in_place():
    """mirres_eaw with color == out is an argument error (a pixel's taps would read what its neighbours wrote), and leaves the buffer alone."""
    from mirres_restir_nerf_mesh_amd._lib import lib, stream_ptr
    occ, col, nrm, pos = (_cu(a) for a in E.frame("smooth", 17, 15))
    before = col.cpu().numpy().copy()
    rc = lib().mirres_eaw(17, 15, 1, 2.0, 0.1, 0.001, occ.data_ptr(), col.data_ptr(), nrm.data_ptr(), pos.data_ptr(), col.data_ptr(), stream_ptr())
    assert rc < 0 and b"mirres_eaw" in lib().mirres_last_error()
    assert np.array_equal(col.cpu().numpy(), before)


@pytest.mark.parametrize("chain", E.CHAINS, ids=["%d_%d" % c for c in E.CHAINS])
def test_drivers_follow_the_reference_step_schedule(oracle, chain):
    """EAWDenoise_use_phi_no_di and EAWDenoise_use_phi with (stepWidth, iter_time) = `chain` on 19 x 27 and 17 x 15: the oracle chained with int() of the halved
    FLOAT step (Denoising.py:154-251: (2, 3) runs 2, 1, 0 — the last pass puts all 25 taps on the centre), bit for bit."""
    from mirres_restir_nerf_mesh_amd.Denoising import EAWDenoise_use_phi, EAWDenoise_use_phi_no_di
    steps = E.chain_steps(*chain)
    for fx, fy in ((19, 27), (17, 15)):
        for kind in ("rand", "smooth"):
            occ, col, nrm, pos = E.frame(kind, fx, fy)
            dev = [_cu(a) for a in (occ, col, nrm, pos)]
            for phis in E.PHIS:
                ref = col
                for s in steps:
                    ref = oracle.eaw(fx, fy, s, *phis, occ, ref, nrm, pos)
                for fn in (EAWDenoise_use_phi_no_di, EAWDenoise_use_phi):
                    got = fn(None, *phis, chain[0], chain[1], fx, fy, *dev)
                    same_bits(got.cpu().numpy(), ref, "%s %r on %s %dx%d" % (fn.__name__, chain, kind, fx, fy))


# ------------------------------------------------------------------------------------------------------------------------ the five-buffer finish
def _finish_outputs(fx, fy, spp, denoise_iter, step_width, sums6, g):
    """mirres_render_finish without gb_depth (the a-trous branch) on FRESH copies of the six sums (k_average divides them in place) -> six numpy outputs."""
    import torch
    from mirres_restir_nerf_mesh_amd import dist as D
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    N = fx * fy
    ctx = get_ctx(fx, fy)
    _, a, keep = D._finish_args(ctx, torch.full((8, 16, 3), 0.5, device="cuda"), g, spp, denoise_iter, step_width, *E.PHIS[0])
    sums = [_cu(s) for s in sums6]
    outs = [torch.full((N, 3), SENTINEL, device="cuda") for _ in range(6)]
    for k in range(6):
        a.outs[k] = outs[k].data_ptr()
    arr = (C.c_void_p * 6)(*[s_.data_ptr() for s_ in sums])
    check(lib().mirres_render_finish(ctx.h, C.byref(a), arr, stream_ptr()), "mirres_render_finish")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


FINISH_SCHEDULES = [(1, 1), (2, 2), (3, 2), (3, 4), (4, 8), (0, 2)]      # (denoise_iter, step_width)


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("dims", [(19, 27), (50, 47)], ids=["19x27", "50x47"])
def test_five_buffer_finish_is_five_single_buffer_chains(oracle, dims, spp):
    """k_eaw5 through mirres_render_finish, five deliberately unlike buffers (zeros, a constant, a sum, random scaled 1e4, random), for 1, 2, 3 and 4 iterations
    (the scratch / output ping-pong ends in the outputs for odd and even counts), step widths 1 to 8 halved as floats ((3, 2) ends at step 0), and
    denoise_iter = 0 (outputs 1..5 are the averages).  Outputs 1..5 equal oracle.finish AND the product's own single-buffer mirres_eaw chain over the averaged
    buffers (sums / spp and t4 + t5 formed in fp32 numpy) in every bit — k_eaw5's comment promises `bit for bit`; a colour weight taken from another buffer,
    or a tap read from it, would show.  Output 0 is the composite of the first three (renderer_restir.py:543-549).  With one Inf in the specular sum only, the
    other four outputs keep the bits of the clean run, the specular one equals the oracle (NaNs by position: their payload is the processor's)."""
    import torch
    fx, fy = dims
    N = fx * fy
    occ, _, nrm, pos = E.frame("smooth", fx, fy)
    rng = np.random.default_rng(21)
    kd = (0.25 + 0.6 * rng.random((N, 3))).astype(np.float32); rm = rng.random((N, 2)).astype(np.float32)
    z3 = torch.zeros((N, 3), device="cuda")
    g = dict(occ=_cu(occ[:, None]), normal=_cu(nrm), depth=torch.zeros((N, 1), device="cuda"), kd=_cu(kd), rm=_cu(rm), ray_dir=z3, pos=_cu(pos))
    dev = [_cu(a) for a in (occ, nrm, pos)]
    clean, dirty = E.five_buffers(fx, fy), E.five_buffers(fx, fy, inf=True)
    assert sum(int(np.isinf(s).sum()) for s in dirty) == 1 and np.isinf(dirty[2]).any() and all(np.isfinite(s).all() for s in clean)
    for it, sw in FINISH_SCHEDULES:
        tag = "%dx%d spp %d iter %d step %d: " % (fx, fy, spp, it, sw)
        outs = _finish_outputs(fx, fy, spp, it, sw, clean, g)
        ref = oracle.finish(fx, fy, spp, occ, nrm, pos, kd, rm, clean, it, sw, *E.PHIS[0])
        avg = [s / np.float32(spp) for s in clean]
        srcs = [avg[1], avg[2], avg[4] + avg[5], avg[4], avg[5]]
        for k in range(5):
            same_bits(outs[k + 1], ref[k + 1], tag + "output %d against oracle.finish" % (k + 1))
            cur = _cu(srcs[k])
            for s in E.chain_steps(sw, it):
                cur = _abi_eaw(fx, fy, s, E.PHIS[0], dev[0], cur, dev[1], dev[2])
            same_bits(outs[k + 1], cur.cpu().numpy(), tag + "output %d against the single-buffer chain" % (k + 1))
            if it == 0:
                same_bits(outs[k + 1], srcs[k], tag + "output %d is the average" % (k + 1))
        final = (kd * (np.float32(1.0) - rm[:, 1:2]) * outs[1] + outs[2]) + outs[3]
        final[occ <= 0.1] = 1.0
        same_bits(outs[0], final, tag + "final_color")
        same_bits(outs[0], ref[0], tag + "final_color against oracle.finish")
        # one Inf in the specular sum
        bad = _finish_outputs(fx, fy, spp, it, sw, dirty, g)
        ref_bad = oracle.finish(fx, fy, spp, occ, nrm, pos, kd, rm, dirty, it, sw, *E.PHIS[0])
        for k in (1, 3, 4, 5):
            same_bits(bad[k], outs[k], tag + "output %d with an Inf in another buffer" % k)
        _same_bits_or_both_nan(bad[2], ref_bad[2], tag + "the specular output with its Inf")
        assert not np.isfinite(bad[2]).all()
        same_bits(bad[0], ref_bad[0], tag + "final_color with an Inf (nan_to_num)")


# ------------------------------------------------------------------------------------------------------------------------ adjoints
def _hold(got, want, what):
    """util.elementwise at its defaults; where the float64 gradient is identically zero the HIP one is exactly zero.  -> share of the bound used"""
    import torch
    got = np.asarray(got); want = np.asarray(want)
    assert np.isfinite(got).all(), what + ": non-finite gradient"
    if not want.any():
        assert not got.any(), "%s: the float64 gradient is identically zero, the HIP one is not (max %.3e)" % (what, float(np.abs(got).max()))
        return 0.0
    elementwise(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want)), what)
    return E.bound_ratio(got, want)


def _abi_bwd(form, fx, fy, step, phis, dev, d_gout, grads):
    """mirres_eaw_bwd (form 'scatter') or mirres_eaw_bwd_gather through the C ABI; `grads` = [g_color, g_normal or None, g_pos or None], accumulated into."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    p = [t.data_ptr() if t is not None else None for t in grads]
    head = (fx, fy, int(step)) + tuple(float(v) for v in phis) + tuple(t.data_ptr() for t in dev) + (d_gout.data_ptr(),)
    if form == "scatter":
        check(lib().mirres_eaw_bwd(*head, *p, stream_ptr()), "mirres_eaw_bwd")
    else:
        scratch = torch.full((fx * fy, 4), float("nan"), device="cuda")
        check(lib().mirres_eaw_bwd_gather(*head, scratch.data_ptr(), *p, stream_ptr()), "mirres_eaw_bwd_gather")
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in grads]


NAMES = ("colour", "normal", "position")


@pytest.mark.parametrize("kind", E.ADJ_KINDS)
def test_adjoints_element_by_element(kind):
    """Autograd through EAWDenoise_run (k_eaw_bwd_sums + k_eaw_bwd_gather) and mirres_eaw_bwd (k_eaw_bwd, the scatter form): the gradients of colour, normal
    and position, element by element against float64 autograd of adjoint_refs.eaw, on ADJ_SIZES x steps 0, 1, 2, 4 x both PHIS — frames of one pixel, one row,
    narrower than the footprint, a ragged and a full block and three blocks; occupancies around the threshold (thresh); a foreground pixel whose taps are all
    background (island) and a background pixel that receives its copied gradient AND is a tap of its neighbours (hole).  At step 0 every tap is the centre:
    the normal and position gradients vanish identically, and the HIP ones are exactly zero."""
    import torch
    from mirres_restir_nerf_mesh_amd.Denoising import EAWDenoise_run
    worst = {"gather": 0.0, "scatter": 0.0}
    for fx, fy in E.ADJ_SIZES:
        frame = E.frame(kind, fx, fy)
        dev = [_cu(a) for a in frame]
        d_w = _cu(E.cotangent(fx, fy))
        for step in E.ADJ_STEPS:
            for k, phis in enumerate(E.PHIS):
                ref = E.grads64(kind, fx, fy, (step,), k)
                tag = "%s %dx%d step %d phis %d " % (kind, fx, fy, step, k)
                x = [t.clone().requires_grad_(True) for t in dev[1:]]
                out = EAWDenoise_run.apply(None, *phis, fx, fy, step, dev[0], *x)
                (out * d_w).sum().backward()
                gs = _abi_bwd("scatter", fx, fy, step, phis, dev, d_w, [torch.zeros_like(t) for t in dev[1:]])
                for nm, a, s, r in zip(NAMES, x, gs, ref):
                    worst["gather"] = max(worst["gather"], _hold(a.grad.cpu().numpy(), r, tag + "gather d/d" + nm))
                    worst["scatter"] = max(worst["scatter"], _hold(s, r, tag + "scatter d/d" + nm))
    print("%s: share of the gradient bound used: gather %.4f, scatter %.4f" % (kind, worst["gather"], worst["scatter"]))


@pytest.mark.parametrize("chain", E.ADJ_CHAINS, ids=["%d_%d" % c for c in E.ADJ_CHAINS])
def test_adjoint_through_the_driver_chain(chain):
    """EAWDenoise_use_phi with (4, 3) and (2, 3) on 19 x 27 (steps 4, 2, 1 and 2, 1, 0), rand and smooth, both PHIS: the three gradients through the chained
    passes against float64 autograd of the chained restatement, same bound."""
    from mirres_restir_nerf_mesh_amd.Denoising import EAWDenoise_use_phi
    fx, fy = 19, 27
    worst = 0.0
    for kind in ("rand", "smooth"):
        dev = [_cu(a) for a in E.frame(kind, fx, fy)]
        d_w = _cu(E.cotangent(fx, fy))
        for k, phis in enumerate(E.PHIS):
            x = [t.clone().requires_grad_(True) for t in dev[1:]]
            out = EAWDenoise_use_phi(None, *phis, chain[0], chain[1], fx, fy, dev[0], *x)
            (out * d_w).sum().backward()
            for nm, a, r in zip(NAMES, x, E.grads64(kind, fx, fy, tuple(E.chain_steps(*chain)), k)):
                worst = max(worst, _hold(a.grad.cpu().numpy(), r, "%s chain %r phis %d d/d%s" % (kind, chain, k, nm)))
    print("chain %r: share of the gradient bound used %.4f" % (chain, worst))


ABI_CASES = [("rand", 19, 27, 1, 1), ("thresh", 17, 15, 2, 1), ("hole", 16, 16, 1, 0), ("smooth", 17, 15, 0, 1), ("island", 3, 5, 1, 1)]


@pytest.mark.parametrize("case", ABI_CASES, ids=["%s_%dx%d_s%d" % c[:4] for c in ABI_CASES])
def test_adjoint_abi_accumulates_accepts_null_and_is_deterministic(case):
    """include/mirres.h: `Grads are ACCUMULATED`; g_normal / g_pos may be NULL.
      * Both forms on buffers pre-filled with random values of the gradient's own scale return prefill + gradient: (result - prefill) meets the float64 bound
        (the at most 27 roundings against the prefill cost 27 * 2^-24 * 2 scale = 3e-6 of the scale, against the bound's 1e-4); where the float64 gradient is
        identically zero the prefill comes back unchanged; the gather form, which adds once per element, returns fp32(prefill + its gradient) in every bit.
      * With NULL g_normal and g_pos the gather form's colour gradient keeps every bit; the scatter form's (float atomics in no fixed order) meets the bound.
      * The gather form run twice gives identical bits."""
    import torch
    kind, fx, fy, step, k = case
    phis = E.PHIS[k]
    dev = [_cu(a) for a in E.frame(kind, fx, fy)]
    d_w = _cu(E.cotangent(fx, fy))
    ref = E.grads64(kind, fx, fy, (step,), k)
    rng = np.random.default_rng(51)
    pre = [((rng.random(r.shape) * 2 - 1) * (np.abs(r).max() or 1.0)).astype(np.float32) for r in ref]
    zero = lambda: [torch.zeros((fx * fy, 3), device="cuda") for _ in range(3)]
    first = _abi_bwd("gather", fx, fy, step, phis, dev, d_w, zero())
    again = _abi_bwd("gather", fx, fy, step, phis, dev, d_w, zero())
    for nm, a, b, r in zip(NAMES, first, again, ref):
        same_bits(b, a, "gather form twice, d/d" + nm)
        _hold(a, r, "gather d/d" + nm)
    for form in ("gather", "scatter"):
        got = _abi_bwd(form, fx, fy, step, phis, dev, d_w, [_cu(p) for p in pre])
        for nm, a, p, r, f in zip(NAMES, got, pre, ref, first):
            _hold(a.astype(np.float64) - p.astype(np.float64), r, "%s form on a pre-filled buffer, d/d%s" % (form, nm))
            if form == "gather":
                same_bits(a, p + f, "gather form: prefill + gradient, d/d" + nm)
        only = _abi_bwd(form, fx, fy, step, phis, dev, d_w, [torch.zeros((fx * fy, 3), device="cuda"), None, None])[0]
        _hold(only, ref[0], "%s form with NULL g_normal / g_pos, d/dcolour" % form)
        if form == "gather":
            same_bits(only, first[0], "gather form with NULL g_normal / g_pos")


@pytest.mark.parametrize("form", ["gather", "scatter"])
def test_background_cotangent_comes_back_unchanged(form):
    """A cotangent that is zero on every foreground pixel and non-zero on the background: the forward copies background pixels, so the colour gradient is
    exactly that cotangent — a background centre receives its copied gradient while being a tap of foreground neighbours whose (gS, gW) are zero — and the
    normal and position gradients are exactly zero."""
    import torch
    for kind, fx, fy in (("rand", 19, 27), ("thresh", 17, 15), ("hole", 16, 16), ("island", 7, 1), ("smooth", 3, 5)):
        frame = E.frame(kind, fx, fy)
        bg = frame[0] < np.float32(0.1)
        assert bg.any() and (~bg).any()
        gout = E.cotangent(fx, fy) + np.float32(0.5)
        gout[~bg] = 0
        dev = [_cu(a) for a in frame]
        for step in (0, 1, 2):
            for phis in E.PHIS:
                gc, gn, gp = _abi_bwd(form, fx, fy, step, phis, dev, _cu(gout), [torch.zeros((fx * fy, 3), device="cuda") for _ in range(3)])
                what = "%s %s %dx%d step %d" % (form, kind, fx, fy, step)
                assert np.array_equal(gc, gout), what + ": the colour gradient is not the cotangent"
                assert not gn.any() and not gp.any(), what + ": a guide gradient is not zero"
