"""GPU parity of the two operators ported from nerf/renderutils: the bilateral denoiser (csrc/eaw.hip: k_bilateral_pack, k_bilateral<0|2>, k_bilateral_pack5,
k_bilateral5) and prepare_shading_normal (csrc/normal.hip).

Kernel and CPU oracle (orc_bilateral) are the same sequence of IEEE fp32 operations in the same order — the same mrf_exp / mrf_pow2k of include/mirres_fmath.h,
both built without contraction — so every comparison between them is bit for bit (equal bits or NaN on both sides where inputs are not finite).  The second
opinions: the float64 restatement of tests/bilateral_refs.py, per element within K 2^-24 sum w |x| (K derived there; tests/test_bilateral_refs.py holds the
oracle to the same bound on the host), and the reference's own kernels compiled from its tree (oracle/_ref, skipped when absent)."""
import ctypes as C

import numpy as np
import pytest

import bilateral_refs as B
import normal_refs as NR
from util import SmallFrame, same_bits, elementwise

pytestmark = pytest.mark.gpu


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _same_bits_or_both_nan(got, ref, what):
    g = np.ascontiguousarray(got, dtype=np.float32); r = np.ascontiguousarray(ref, dtype=np.float32)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    same = (g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))
    assert same.all(), "%s: %d of %d values differ; first: got %r want %r" % (what, int((~same).sum()), same.size, g[~same][:4], r[~same][:4])


def _forward(fx, fy, sigma, col, nrm, zdz):
    """mirres_bilateral through the C ABI -> f32[N,4]."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    n = fx * fy
    d = [_cu(col), _cu(nrm), _cu(zdz)]
    out = torch.full((n, 4), -7.0, device="cuda"); scratch = torch.empty((n, 8), device="cuda")
    check(lib().mirres_bilateral(fx, fy, float(sigma), *[t.data_ptr() for t in d], scratch.data_ptr(), out.data_ptr(), stream_ptr()), "mirres_bilateral")
    return out.cpu().numpy()


def _backward(fx, fy, sigma, nrm, zdz, g4):
    """mirres_bilateral_bwd through the C ABI -> f32[N,3]."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    n = fx * fy
    d = [_cu(nrm), _cu(zdz), _cu(g4)]
    out = torch.full((n, 3), -7.0, device="cuda"); scratch = torch.empty((n, 8), device="cuda")
    check(lib().mirres_bilateral_bwd(fx, fy, float(sigma), *[t.data_ptr() for t in d], scratch.data_ptr(), out.data_ptr(), stream_ptr()), "mirres_bilateral_bwd")
    return out.cpu().numpy()


def test_bilateral_forward_backward_match_oracle(oracle):
    """factor 2 -> sigma 4 -> 43 x 43 taps on the 40 x 28 frame, through the autograd Function and the public op: forward, backward and the op's quotient equal the
    oracle in every bit (the same IEEE operations in the same order; nothing of glibc or ocml is involved since include/mirres_fmath.h); the op's colour gradient,
    through the division, is within K_OP 2^-24 sum w |G / w| of float64 per element."""
    import torch
    from mirres_restir_nerf_mesh_amd.renderutils.ops import bilateral_denoiser, _bilateral_denoiser_func
    fx, fy = 40, 28
    col, nrm, zdz = B.benign(fx, fy)
    ref4 = oracle.bilateral(fx, fy, 4.0, col, nrm, zdz)
    got4 = _bilateral_denoiser_func.apply(_cu(col), _cu(nrm), _cu(zdz), 4.0, fy, fx).cpu().numpy()
    same_bits(got4, ref4, "autograd Function forward")
    g4 = B.grad4_for(fx, fy)
    c = _cu(col).requires_grad_(True)
    inp = torch.cat((c, _cu(nrm), _cu(zdz)), dim=-1)
    out4 = _bilateral_denoiser_func.apply(inp[:, 0:3], inp[:, 3:6], inp[:, 6:8], 4.0, fy, fx)
    out4.backward(_cu(g4))
    same_bits(c.grad.cpu().numpy(), oracle.bilateral(fx, fy, 4.0, None, nrm, zdz, grad4=g4), "autograd Function backward")
    c2 = _cu(col).requires_grad_(True)
    out = bilateral_denoiser(fy, fx, torch.cat((c2, _cu(nrm), _cu(zdz)), dim=-1), 2.0)
    same_bits(out.detach().cpu().numpy(), ref4[:, :3] / ref4[:, 3:4], "public op, factor 2")
    G = np.random.default_rng(4).normal(size=(fx * fy, 3)).astype(np.float32)
    (out * _cu(G)).sum().backward()
    R, S = B.op_gradient64(fx, fy, 4.0, col, nrm, zdz, G)
    B.within(c2.grad.cpu().numpy(), R, S, 4.0, "public op gradient, factor 2 (GPU)", K=B.K_OP)


CASES = B.finite_cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_bilateral_bits_on_every_finite_frame(oracle, case):
    """Every finite frame of the matrix (tests/bilateral_refs.py: the shapes at sigma 4 from one pixel to 4 x 3 ragged tiles with a full-window interior, seven sigmas
    on two shapes incl. factor 0 and the three whose float radius was short, dz over two decades, the finite hostile guides): forward (all four channels) and
    backward equal the oracle in every bit, and both stay inside the float64 bound, on every case."""
    name, fx, fy, sigma, (col, nrm, zdz) = CASES[case]
    got = _forward(fx, fy, sigma, col, nrm, zdz)
    same_bits(got, oracle.bilateral(fx, fy, sigma, col, nrm, zdz), name + " forward")
    g4 = B.grad4_for(fx, fy)
    gb = _backward(fx, fy, sigma, nrm, zdz, g4)
    same_bits(gb, oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), name + " backward")
    R, S = B.forward64(fx, fy, sigma, col, nrm, zdz)
    B.within(got, B.clamp_weight(R), S, sigma, name + " forward (GPU)")
    Rb, Sb = B.backward64(fx, fy, sigma, nrm, zdz, g4)
    B.within(gb, Rb, Sb, sigma, name + " backward (GPU)")
    if "hostile dead" in name:
        dead = ~np.any(np.asarray(nrm) != 0, axis=1)
        assert dead.sum() >= 20 and np.all(got[dead, 3] == B.EPS) and np.all(got[dead, :3] == 0)


@pytest.mark.parametrize("kind", ["normals", "dz", "z", "colours"])
def test_bilateral_nonfinite_guides_match_the_oracle(oracle, kind):
    """NaN normals, NaN dz (falls back to the 1e-4 denominator: fmaxf), +-inf and NaN depths, NaN and inf texels mixed into a benign frame: equal bits or NaN on both sides, forward and backward (the incoming
    gradient carries a NaN and an inf of its own).  A NaN normal must NOT poison its window: the clamps are fmaxf / fminf on both sides."""
    for fx, fy, sigma in ((37, 19, 2.0), (50, 47, 4.0)):
        col, nrm, zdz = B.hostile(kind, fx, fy, nonfinite=True)
        got = _forward(fx, fy, sigma, col, nrm, zdz)
        ref = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
        _same_bits_or_both_nan(got, ref, "%s %dx%d forward" % (kind, fx, fy))
        if kind in ("normals", "dz"):
            assert np.isfinite(got).all(), "a NaN %s reached the output" % kind
        else:
            assert np.isnan(ref).any() and np.isfinite(ref).any()
        g4 = B.grad4_for(fx, fy)
        if kind == "colours":
            g4[5, 0] = np.nan; g4[fx * fy // 2, 2] = np.inf
        _same_bits_or_both_nan(_backward(fx, fy, sigma, nrm, zdz, g4), oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), "%s %dx%d backward" % (kind, fx, fy))


@pytest.mark.parametrize("at", [(25, 23), (0, 0)], ids=["interior", "corner"])
@pytest.mark.parametrize("sigma", [0.4, 1.6, 4.0])
def test_bilateral_impulse_footprint_is_the_reference_window(oracle, sigma, at):
    """Colour (forward) / incoming gradient (backward) zero except one pixel, flat guides: the non-zero outputs are exactly the reference's window
    (r = 2 ceil(sigma * 2.5) + 1 with the product in double, denoising.cu:26,86) around it clipped to the frame, each value bit-equal to the oracle's single term.
    With the radius from the float product, sigma 0.4 and 1.6 leave the two outer rings of that window zero:
    'forward: 40 outputs inside the reference's window (radius 5) are zero' (sigma 0.4, interior; 12 in the corner),
    'forward: 168 outputs inside the reference's window (radius 11) are zero' (sigma 1.6, interior; 44 in the corner)."""
    fx, fy = 50, 47
    col, nrm, zdz, pi = B.impulse(fx, fy, at)
    must, may = B.impulse_footprint(fx, fy, sigma, at, 0.25)
    r = B.ref_radius(sigma)
    got = _forward(fx, fy, sigma, col, nrm, zdz)
    for c in range(3):
        nz = got[:, c] != 0
        assert not (nz & ~may).any(), "forward: non-zero output outside the reference's window (radius %d)" % r
        assert (nz | ~must).all(), "forward: %d outputs inside the reference's window (radius %d) are zero" % (int((must & ~nz).sum()), r)
    same_bits(got, oracle.bilateral(fx, fy, sigma, col, nrm, zdz), "impulse forward")
    g4 = np.zeros((fx * fy, 4), np.float32); g4[pi] = (1.0, -0.5, 0.25, 3.0)
    gb = _backward(fx, fy, sigma, nrm, zdz, g4)
    for c in range(3):
        nz = gb[:, c] != 0
        assert not (nz & ~may).any(), "backward: non-zero gradient outside the reference's window (radius %d)" % r
        assert (nz | ~must).all(), "backward: %d gradients inside the reference's window (radius %d) are zero" % (int((must & ~nz).sum()), r)
    same_bits(gb, oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), "impulse backward")


@pytest.mark.parametrize("factor", [0.5, 1.0])
def test_bilateral_public_op_and_its_gradient(oracle, factor):
    """renderutils.ops.bilateral_denoiser (sigma = 2 factor): the output is the fp32 quotient of the oracle's sums in every bit; the colour gradient of
    sum(G out), through the division and the backward kernel, is within K_OP 2^-24 sum w |G / w| of float64 per element (and no element is exempt)."""
    import torch
    from mirres_restir_nerf_mesh_amd.renderutils.ops import bilateral_denoiser
    fx, fy, sigma = 37, 19, 2.0 * factor
    col, nrm, zdz = B.asymmetric(fx, fy)
    G = np.random.default_rng(4).normal(size=(fx * fy, 3)).astype(np.float32)
    c = _cu(col).requires_grad_(True)
    out = bilateral_denoiser(fy, fx, torch.cat((c, _cu(nrm), _cu(zdz)), dim=-1), factor)
    ref4 = oracle.bilateral(fx, fy, sigma, col, nrm, zdz)
    same_bits(out.detach().cpu().numpy(), ref4[:, :3] / ref4[:, 3:4], "public op, factor %g" % factor)
    (out * _cu(G)).sum().backward()
    R, S = B.op_gradient64(fx, fy, sigma, col, nrm, zdz, G)
    assert np.abs(R).min() > 0
    B.within(c.grad.cpu().numpy(), R, S, sigma, "public op gradient, factor %g (GPU)" % factor, K=B.K_OP)


def test_bilateral_public_op_is_zero_where_every_weight_is_zero(oracle):
    """Zero normals on a block and on scattered pixels: every weight of those pixels is 0 (their own too), out4.w = 1e-4 and bilateral_denoiser itself returns
    exactly 0 there; everywhere the op is the fp32 quotient of the oracle's sums in every bit."""
    import torch
    from mirres_restir_nerf_mesh_amd.renderutils.ops import bilateral_denoiser
    fx, fy = 37, 19
    col, nrm, zdz = B.hostile("dead", fx, fy)
    out = bilateral_denoiser(fy, fx, torch.cat((_cu(col), _cu(nrm), _cu(zdz)), dim=-1), 1.0).cpu().numpy()
    ref4 = oracle.bilateral(fx, fy, 2.0, col, nrm, zdz)
    same_bits(out, ref4[:, :3] / ref4[:, 3:4], "public op on the dead frame")
    dead = ~np.any(nrm != 0, axis=1)
    assert dead.sum() >= 20 and np.all(ref4[dead, 3] == B.EPS) and np.all(out[dead] == 0) and np.abs(out[~dead]).min() > 0


def _finish_outputs(fx, fy, srcs6, normal, gb, occ, kd, rm):
    """mirres_render_finish on prepared per-sample sums (spp = 1, so the averages are the sums) with gb_depth given: the five-buffer bilateral finish."""
    import torch
    from mirres_restir_nerf_mesh_amd import dist as D
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    N = fx * fy
    ctx = get_ctx(fx, fy)
    z3 = torch.zeros((N, 3), device="cuda")
    g = dict(occ=_cu(occ), normal=_cu(normal), depth=torch.zeros((N, 1), device="cuda"), kd=_cu(kd), rm=_cu(rm), ray_dir=z3, pos=z3)
    _, a, keep = D._finish_args(ctx, torch.full((8, 16, 3), 0.5, device="cuda"), g, 1, 2, 2, 2.0, 0.1, 0.001)
    d_gb = _cu(gb); a.gb_depth = d_gb.data_ptr()
    sums = [_cu(s) for s in srcs6]
    outs = [torch.full((N, 3), -7.0, device="cuda") for _ in range(6)]
    for k in range(6):
        a.outs[k] = outs[k].data_ptr()
    arr = (C.c_void_p * 6)(*[s_.data_ptr() for s_ in sums])
    check(lib().mirres_render_finish(ctx.h, C.byref(a), arr, stream_ptr()), "mirres_render_finish")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("guides", ["benign", "asymmetric", "dead"])
def test_fused_five_buffer_bilateral_of_the_finish(oracle, guides):
    """k_bilateral_pack5 / k_bilateral5 through the frame's finish on a 50 x 47 context (ragged 4 x 3 tiles, interior pixels with the full 43 x 43 window), five
    DIFFERENT source buffers: outputs 1..5 equal oracle.bilateral(...)[:, :3] / [:, 3:4] in fp32 in every bit — a wrong entry of the LDS offset tables
    (s_wxy / s_dist), a swapped slot of the 80-byte record or a buffer read for another would each show — and final_color composes the first three
    (renderer_restir.py:543-549).  Also with dz over two decades and with zero normals (weight sum clamped at 1e-4, output 0)."""
    fx, fy = 50, 47
    N = fx * fy
    _, nrm, zdz = {"benign": B.benign, "asymmetric": B.asymmetric, "dead": lambda a, b: B.hostile("dead", a, b)}[guides](fx, fy)
    rng = np.random.default_rng(21)
    sums = [(rng.random((N, 3)) * (k + 1)).astype(np.float32) for k in range(6)]
    occ = (rng.random((N, 1)) > 0.15).astype(np.float32)
    kd = (0.25 + 0.6 * rng.random((N, 3))).astype(np.float32); rm = rng.random((N, 2)).astype(np.float32)
    outs = _finish_outputs(fx, fy, sums, nrm, zdz, occ, kd, rm)
    srcs = [sums[1], sums[2], sums[4] + sums[5], sums[4], sums[5]]
    den = []
    for k in range(5):
        r4 = oracle.bilateral(fx, fy, 4.0, srcs[k], nrm, zdz)
        den.append(r4[:, :3] / r4[:, 3:4])
        same_bits(outs[k + 1], den[k], "finish output %d (%s guides)" % (k + 1, guides))
    if guides == "dead":
        dead = ~np.any(nrm != 0, axis=1)
        assert dead.sum() >= 20 and all(np.all(outs[k + 1][dead] == 0) for k in range(5))
    final = (kd * (np.float32(1.0) - rm[:, 1:2]) * den[0] + den[1]) + den[2]
    final[occ[:, 0] <= 0.1] = 1.0
    same_bits(outs[0], final, "final_color (%s guides)" % guides)


def test_bilateral_against_the_reference_kernels(oracle):
    """oracle/_ref/libref_denoise.so = the reference's OWN bilateral_denoiser_fwd_kernel / _bwd_kernel (nerf/renderutils/c_src/denoising.cu) compiled by hipcc from
    the reference tree (oracle/Makefile `ref`; built where the tree exists, travels as a .so). The product's kernels (csrc/eaw.hip) and the CPU oracle are both held to
    what the reference's code computes on this GPU: forward (weighted colour sums and weight sum) and backward (colour gradient) — the 40 x 28 frame at sigma 4,
    the 50 x 47 frame (full-window interior) at sigma 4, 1.0 and 1.6 (the last: a radius the float product got wrong), dz over two decades, the impulse frames
    (the pattern of zero and non-zero outputs must be the reference's exactly) and NaN guides (NaN in the same places).  Value tolerance: that build contracts
    a * b + c into fma and calls the vendor's expf / powf, the product does neither (rtol 1e-4 on sums of ~10^3 weighted taps; x^128 amplifies the last bit of the
    normals' dot product 128 times)."""
    import torch
    L = oracle.ref_denoise_lib()
    if L is None:
        pytest.skip("oracle/_ref/libref_denoise.so was not built (no reference tree at build time)")

    def reference(fx, fy, sigma, col, nrm, zdz, g4):
        d_col, d_nrm, d_zdz, d_g4 = _cu(col), _cu(nrm), _cu(zdz), _cu(g4)
        # the reference normalises the guide normals in Python before its kernel (safe_normalize, ops.py:168-169, 194); the product's op does it inside
        d_unit = (d_nrm / torch.sqrt(torch.clamp((d_nrm * d_nrm).sum(-1, keepdim=True), min=1e-20))).contiguous()
        out = torch.zeros((fy * fx, 4), device="cuda"); gr = torch.zeros((fy * fx, 3), device="cuda")
        assert L.ref_bilateral_fwd(d_col.data_ptr(), d_unit.data_ptr(), d_zdz.data_ptr(), out.data_ptr(), 1, fy, fx, float(sigma), None) == 0
        assert L.ref_bilateral_bwd(d_col.data_ptr(), d_unit.data_ptr(), d_zdz.data_ptr(), d_g4.data_ptr(), gr.data_ptr(), 1, fy, fx, float(sigma), None) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy(), gr.cpu().numpy()

    frames = [("benign 40x28 s4", 40, 28, 4.0, B.benign(40, 28)), ("benign 50x47 s4", 50, 47, 4.0, B.benign(50, 47)), ("benign 50x47 s1", 50, 47, 1.0, B.benign(50, 47)),
              ("benign 50x47 s1.6", 50, 47, 1.6, B.benign(50, 47)), ("asymmetric 50x47 s4", 50, 47, 4.0, B.asymmetric(50, 47)), ("asymmetric 37x19 s1.6", 37, 19, 1.6, B.asymmetric(37, 19))]
    for name, fx, fy, sigma, (col, nrm, zdz) in frames:
        g4 = B.grad4_for(fx, fy)
        ref_out, ref_g = reference(fx, fy, sigma, col, nrm, zdz, g4)
        np.testing.assert_allclose(_forward(fx, fy, sigma, col, nrm, zdz), ref_out, rtol=1e-4, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(oracle.bilateral(fx, fy, sigma, col, nrm, zdz), ref_out, rtol=1e-4, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(_backward(fx, fy, sigma, nrm, zdz, g4), ref_g, rtol=2e-4, atol=5e-5, err_msg=name)
        np.testing.assert_allclose(oracle.bilateral(fx, fy, sigma, None, nrm, zdz, grad4=g4), ref_g, rtol=2e-4, atol=5e-5, err_msg=name)
    # impulse frames: the support is the reference's, tap for tap
    fx, fy = 50, 47
    for sigma in (0.4, 1.6, 4.0):
        for at in ((25, 23), (0, 0)):
            col, nrm, zdz, pi = B.impulse(fx, fy, at)
            g4 = np.zeros((fx * fy, 4), np.float32); g4[pi] = (1.0, -0.5, 0.25, 3.0)
            ref_out, ref_g = reference(fx, fy, sigma, col, nrm, zdz, g4)
            got, gb = _forward(fx, fy, sigma, col, nrm, zdz), _backward(fx, fy, sigma, nrm, zdz, g4)
            assert np.array_equal(got[:, :3] != 0, ref_out[:, :3] != 0), "sigma %g at %r: the forward's support is not the reference's" % (sigma, at)
            assert np.array_equal(gb != 0, ref_g != 0), "sigma %g at %r: the backward's support is not the reference's" % (sigma, at)
            assert (ref_out[:, :3] != 0).sum() > 3
            np.testing.assert_allclose(got, ref_out, rtol=1e-4, atol=0)
            np.testing.assert_allclose(gb, ref_g, rtol=1e-4, atol=0)
    # NaN guides: NaN in the same places as the reference
    for kind in ("normals", "dz", "z", "colours"):
        col, nrm, zdz = B.hostile(kind, 37, 19, nonfinite=True)
        g4 = B.grad4_for(37, 19)
        ref_out, ref_g = reference(37, 19, 2.0, col, nrm, zdz, g4)
        got, gb = _forward(37, 19, 2.0, col, nrm, zdz), _backward(37, 19, 2.0, nrm, zdz, g4)
        assert np.array_equal(np.isnan(got), np.isnan(ref_out)), kind + ": NaN pattern of the forward"
        assert np.array_equal(np.isnan(gb), np.isnan(ref_g)), kind + ": NaN pattern of the backward"
        ok = np.isfinite(ref_out)
        np.testing.assert_allclose(got[ok], ref_out[ok], rtol=1e-4, atol=1e-5, err_msg=kind)


def test_use_bi_de_branch_of_the_frame(oracle, scene_mod):
    """run_restir_di_with_pt with gb_depth (--use_bi_de, renderer_restir.py:529-541): the fused loop's bilateral finish equals the oracle's
    filter applied to the frame's own averaged sums in every bit, and final_color composes the three denoised buffers (:543-549), in every bit as well."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    F = SmallFrame(oracle, scene_mod, fx=48, fy=40)
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    mods = RR.load_m_for_restir(F.fx, F.fy)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N, spp = F.N, 3
    gb = np.stack([F.depth, 0.01 + 0.002 * F.depth], axis=1).astype(np.float32)
    args = lambda: (mods[0].ctx, W, None, False, (1, 1, 1), cu(F.env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm), cu(F.ray_dir_raw), cu(F.pos))
    sums, _, _ = RR.render_fused(*args(), spp, 2, 2, 2.0, 0.1, 0.001, 77, spp_range=(0, spp))
    outs, _, _ = RR.render_fused(*args(), spp, 2, 2, 2.0, 0.1, 0.001, 77, gb_depth=cu(gb))
    s = [x.cpu().numpy() / np.float32(spp) for x in sums]
    srcs = [s[1], s[2], s[4] + s[5], s[4], s[5]]
    den = []
    for k in range(5):
        r4 = oracle.bilateral(F.fx, F.fy, 4.0, srcs[k], F.normal, gb)
        den.append(r4[:, :3] / r4[:, 3:4])
        same_bits(outs[k + 1].cpu().numpy(), den[k], "frame output %d" % (k + 1))
    final = (F.kd * (np.float32(1.0) - F.rm[:, 1:2]) * den[0] + den[1]) + den[2]
    final[F.occ <= 0.1] = 1.0
    same_bits(outs[0].cpu().numpy(), final, "final_color")
    # the reference-shaped entry point accepts gb_depth on the stepwise (autograd) path too
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    RR.set_random_offset(77)
    env = cu(F.env).requires_grad_(True)
    z = lambda *sh: torch.zeros(sh, device="cuda")
    out2 = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, cu(gb), W, *mods[:8], *mods[8:17], env, cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm),
                                    cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, spp, 2, 2, 2.0, 0.1, 0.001)
    out2[0].sum().backward()
    assert torch.isfinite(env.grad).all() and float(env.grad.abs().sum()) > 0
    frac = (np.abs(out2[1].detach().cpu().numpy() - outs[1].cpu().numpy()).max(axis=1) <= 1e-3).mean()
    assert frac >= 0.99


# ------------------------------------------------------------------------------------------------------------------------ prepare_shading_normal
def _normal_abi(ins, two_sided, opengl, dout):
    """mirres_prepare_shading_normal / _bwd through the C ABI on n full rows (no broadcasting, no sum_to_size) -> (out, six gradients)."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    n = ins[0].shape[0]
    d = [_cu(a) for a in ins]
    out = torch.full((n, 3), -7.0, device="cuda")
    check(lib().mirres_prepare_shading_normal(n, *[t.data_ptr() for t in d], int(two_sided), int(opengl), out.data_ptr(), stream_ptr()), "mirres_prepare_shading_normal")
    g = [torch.full((n, 3), -7.0, device="cuda") for _ in range(6)]
    d_out = _cu(dout)
    check(lib().mirres_prepare_shading_normal_bwd(n, *[t.data_ptr() for t in d], int(two_sided), int(opengl), d_out.data_ptr(), *[t.data_ptr() for t in g], stream_ptr()),
          "mirres_prepare_shading_normal_bwd")
    return out.cpu().numpy(), [t.cpu().numpy() for t in g]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_prepare_shading_normal_bits_against_the_restatements(oracle, n):
    """k_shading_normal / k_shading_normal_bwd on n rows — below, at and above one 256-thread workgroup, and 274 workgroups with a ragged last one — for the four
    flag pairs: the forward equals oracle.prepare_shading_normal and all six gradients equal normal_refs.backward32 in every bit.  The rows mix in every kink
    (normal_refs.KINKS: zero-length normal / tangent / view vector, tangent parallel to the normal, dp exactly 0, exactly 0.1 and one ulp either side, negative dp,
    p.z zero and negative, dot(view, geom) zero and negative), the last row among them."""
    ins, where = NR.mixed_rows(n)
    assert n == 1 or len(where) == len(NR.KINKS)
    dout = np.random.default_rng(6).normal(size=(n, 3)).astype(np.float32)
    for two_sided in (True, False):
        for opengl in (True, False):
            out, grads = _normal_abi(ins, two_sided, opengl, dout)
            tag = "n %d flags %d%d " % (n, two_sided, opengl)
            same_bits(out, oracle.prepare_shading_normal(*ins, two_sided, opengl), tag + "forward")
            ref, _ = NR.backward32(*ins, two_sided, opengl, dout)
            for name, a, b in zip(NR.NAMES, grads, ref):
                same_bits(a, b, tag + "gradient of " + name)


def test_prepare_shading_normal_forward_and_backward(oracle):
    """renderutils.ops.prepare_shading_normal on shape (2, 13, 17, 3) with view_pos and geom_nrm of shape [1, 1, 1, 3] (their gradients are sums over the 442
    rows) and with perturbed_nrm=None: the forward equals the restatement in every bit; the gradients are held per element (util.elementwise) to float64 autograd
    of the formula at rtol 2.5e-5 with an absolute term of 1e-7 of the largest element — four times the 6.2e-6 measured on the CPU between the fp32 restatement
    and float64 on these inputs (tests/test_normal_refs.py), the factor for the different order of the sums.  Seen on the MI355X: 6.15e-6, the restatement's own figure (the
    test prints it).  Full-size gradients equal the restatement's bits."""
    import torch
    from mirres_restir_nerf_mesh_amd.renderutils.ops import prepare_shading_normal
    ins, dout = NR.wrapper_inputs()
    seen = 0.0
    for two_sided, opengl in ((True, True), (True, False), (False, True), (False, False)):
        t = [_cu(a).requires_grad_(True) for a in ins]
        out = prepare_shading_normal(*t, two_sided, opengl)
        assert tuple(out.shape) == NR.WRAPPER_SHAPE
        same_bits(out.detach().cpu().numpy(), oracle.prepare_shading_normal(*ins, two_sided, opengl), "wrapper forward %d%d" % (two_sided, opengl))
        (out * _cu(dout)).sum().backward()
        g32 = NR.wrapper_gradients32(ins, two_sided, opengl, dout)
        g64 = NR.gradients64(ins, two_sided, opengl, dout)
        for name, a, r32, r64 in zip(NR.NAMES, t, g32, g64):
            assert tuple(a.grad.shape) == r64.shape, name
            seen = max(seen, NR.elementwise_rtol(a.grad.cpu().numpy(), r64))
            elementwise(a.grad, torch.from_numpy(r64), "%s %d%d" % (name, two_sided, opengl), rtol=NR.WRAPPER_RTOL, atol_scale=NR.WRAPPER_ATOL_SCALE)
            if r64.shape == NR.WRAPPER_SHAPE:
                same_bits(a.grad.cpu().numpy(), r32, "wrapper gradient of %s %d%d" % (name, two_sided, opengl))
    print("shading-normal gradients against float64: rtol %.3e at atol_scale %g (allowed %.3e)" % (seen, NR.WRAPPER_ATOL_SCALE, NR.WRAPPER_RTOL))
    # the forward through the wrapper on the kink rows (zero-length inputs, clamped p.z, both flip outcomes), laid out [1, 1, 257, 3]
    rows, _ = NR.mixed_rows(257)
    rows = [a.reshape(1, 1, 257, 3) for a in rows]
    for two_sided, opengl in ((True, True), (True, False), (False, True), (False, False)):
        same_bits(prepare_shading_normal(*[_cu(a) for a in rows], two_sided, opengl).cpu().numpy(), oracle.prepare_shading_normal(*rows, two_sided, opengl), "wrapper forward on the kinks")
    # the default perturbation (0, 0, 1): not a leaf, no gradient; the tangent's gradient vanishes; the others as before
    t = [_cu(a).requires_grad_(True) for a in ins]
    out = prepare_shading_normal(t[0], t[1], None, t[3], t[4], t[5])
    ins0 = list(ins); ins0[2] = np.array([0, 0, 1], np.float32).reshape(1, 1, 1, 3)
    same_bits(out.detach().cpu().numpy(), oracle.prepare_shading_normal(*ins0), "wrapper forward, default perturbation")
    (out * _cu(dout)).sum().backward()
    g64 = NR.gradients64(ins0, True, True, dout)
    for k in (0, 1, 3, 5):
        elementwise(t[k].grad, torch.from_numpy(g64[k]), NR.NAMES[k] + " (default perturbation)", rtol=NR.WRAPPER_RTOL, atol_scale=NR.WRAPPER_ATOL_SCALE)
    assert not g64[4].any() and not t[4].grad.any()         # p = (0, 0, 1): the tangent enters with weight p.x = 0 and through the bitangent with p.y = 0


def test_prepare_shading_normal_against_the_reference_kernels(oracle):
    """oracle/_ref/libref_normal.so = the reference's OWN PrepareShadingNormalFwdKernel / BwdKernel (nerf/renderutils/c_src/normal.cu) compiled from its tree without
    contraction.  Forward: the same operations in the same order (safeNormalize, cross, the perturbation sum, the flip, the bend) — bit-equal to the product on
    257 mixed rows laid out [1, 1, 257, 3] and on the wrapper's broadcast case.  Backward: bwdSafeNormalize (vec3f.h:93-104) orders its arithmetic differently
    (component formulas times 1 / |v|^3 through powf), so product and reference are each held to float64 autograd at the wrapper's tolerance on the benign case,
    and on the kink rows both follow the same conventions (normal_refs.KINK_ZERO / KINK_PASS: which gradients vanish exactly, which pass)."""
    import torch
    L = oracle.ref_normal_lib()
    if L is None:
        pytest.skip("oracle/_ref/libref_normal.so was not built (no reference tree at build time)")

    def reference(ins, two_sided, opengl, dout):
        shapes = (C.c_int * 18)(*[int(v) for a in ins for v in a.shape[:3]])
        d = [_cu(a) for a in ins]
        full = tuple(max(a.shape[k] for a in ins) for k in range(3)) + (3,)
        out = torch.full(full, -7.0, device="cuda")
        ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in d])
        assert L.ref_shading_normal_fwd(C.byref(ptrs), C.byref(shapes), int(two_sided), int(opengl), out.data_ptr(), None) == 0
        g = [torch.full(full, -7.0, device="cuda") for _ in range(6)]
        gp = (C.c_void_p * 6)(*[t.data_ptr() for t in g])
        d_out = _cu(dout)
        assert L.ref_shading_normal_bwd(C.byref(ptrs), C.byref(shapes), int(two_sided), int(opengl), d_out.data_ptr(), C.byref(gp), None) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy(), [t.cpu().numpy() for t in g]

    rows, where = NR.mixed_rows(257)
    dout = np.random.default_rng(6).normal(size=(257, 3)).astype(np.float32)
    for two_sided, opengl in ((True, True), (True, False), (False, True), (False, False)):
        out, grads = _normal_abi(rows, two_sided, opengl, dout)
        r_out, r_g = reference([a.reshape(1, 1, 257, 3) for a in rows], two_sided, opengl, dout.reshape(1, 1, 257, 3))
        same_bits(out, r_out.reshape(257, 3), "forward against the reference's kernel %d%d" % (two_sided, opengl))
        NR.check_kink_conventions(grads, where, "product %d%d" % (two_sided, opengl))
        NR.check_kink_conventions([b.reshape(257, 3) for b in r_g], where, "reference %d%d" % (two_sided, opengl))
    ins, dw = NR.wrapper_inputs()
    from mirres_restir_nerf_mesh_amd.renderutils.ops import prepare_shading_normal
    for two_sided, opengl in ((True, True), (False, False)):
        r_out, r_g = reference(ins, two_sided, opengl, dw)
        t = [_cu(a) for a in ins]
        same_bits(prepare_shading_normal(*t, two_sided, opengl).cpu().numpy(), r_out, "wrapper forward against the reference's kernel")
        g64 = NR.gradients64(ins, two_sided, opengl, dw)
        for name, a, rg, r64 in zip(NR.NAMES, ins, r_g, g64):
            if a.shape != NR.WRAPPER_SHAPE:
                rg = rg.reshape(-1, 3).sum(axis=0, dtype=np.float32).reshape(a.shape)
            elementwise(torch.from_numpy(rg), torch.from_numpy(r64), "reference's gradient of %s %d%d" % (name, two_sided, opengl), rtol=NR.WRAPPER_RTOL, atol_scale=NR.WRAPPER_ATOL_SCALE)


def test_prepare_shading_normal_matches_the_reference_python_path():
    """csrc/normal.hip through renderutils.ops.prepare_shading_normal (the reference's call shape) against tests/golden/ref_shading_normal.npz: outputs AND
    gradients of the REFERENCE's own pure-torch implementation (nerf/renderutils/ops.py, use_python=True; tests/golden/gen_from_reference.py) — forward for the
    four flag combinations incl. zero-length inputs and the default perturbation, backward for every input under both flag settings."""
    import os
    import torch
    from mirres_restir_nerf_mesh_amd.renderutils.ops import prepare_shading_normal
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_shading_normal.npz"))
    names = ("pos", "view", "perturbed", "smooth_nrm", "smooth_tng", "geom_nrm")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [g[k] for k in names]
    for two_sided in (True, False):
        for opengl in (True, False):
            got = prepare_shading_normal(*[cu(a) for a in args], two_sided, opengl).cpu().numpy()
            np.testing.assert_allclose(got, g["fwd_%d%d" % (two_sided, opengl)], rtol=1e-5, atol=1e-6)   # torch.lerp vs normal.cu's a (1 - t) + b t: last-bit differences
    got = prepare_shading_normal(cu(args[0]), cu(args[1]), None, *[cu(a) for a in args[3:]]).cpu().numpy()
    np.testing.assert_allclose(got, g["fwd_default_perturbation"], rtol=1e-5, atol=1e-6)
    sl = (slice(None), slice(2, None))
    for two_sided, opengl in ((True, True), (False, False)):
        ins = [cu(a[sl] if a.shape[1] > 1 else a).requires_grad_(True) for a in args]
        out = prepare_shading_normal(*ins, two_sided, opengl)
        (out * cu(g["grad_weight"])).sum().backward()
        for name, a in zip(names, ins):
            ref = g["grad_%d%d_%s" % (two_sided, opengl, name)]
            np.testing.assert_allclose(a.grad.cpu().numpy(), ref, rtol=2e-4, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg="%s %d%d" % (name, two_sided, opengl))
