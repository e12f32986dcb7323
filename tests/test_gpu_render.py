"""GPU parity: whole frames through run_restir_di_with_pt (fused C path and the stepwise Python path) against the oracle."""
import os

import numpy as np
import pytest

from util import SmallFrame, psnr, pixel_parity

pytestmark = pytest.mark.gpu


def _setup(oracle, scene_mod, fx=48, fy=40, **kw):
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    F = SmallFrame(oracle, scene_mod, fx=fx, fy=fy, **kw)
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    mods = RR.load_m_for_restir(F.fx, F.fy)
    return F, W, mods, RR, torch


def _run(F, W, mods, RR, torch, spp, mlp, seed=4242):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    RR.set_random_offset(seed)
    N = F.N
    z = lambda *s: torch.zeros(s, device="cuda")
    occ = cu(F.occ[:, None].copy())
    out = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, None, W, *mods[:8], *mods[8:17], cu(F.env), occ, cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm),
                                   cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, spp, 2, 2, 2.0, 0.1, 0.001)
    return [o.detach().cpu().numpy() for o in out]


def test_one_spp_frame_matches_oracle(oracle, scene_mod):
    """1 spp, constant material at the indirect vertices: every output buffer of the frame equals the oracle's BIT FOR BIT (shared FP policy and
    shared transcendental arithmetic, include/mirres_fmath.h) — the north-star's 1e-3 per channel met with zero error in every pixel."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    got = _run(F, W, mods, RR, torch, 1, None)
    ref = oracle.render(F.fx, F.fy, 1, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=None)
    names = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]
    for g, n in zip(got, names):
        r = ref[n]
        pixel_parity(g, r, "one-sample frame / " + n, tol=0.0)
    assert np.array_equal(got[0][F.occ < 0.5], np.ones_like(got[0][F.occ < 0.5]))    # background := 1 (:546-547)


def test_frame_matches_the_reference_loop(oracle, scene_mod):
    """The HIP frame (one mirres_render call, hash-grid + MFMA material field, 3 samples) against tests/golden/ref_loop.npz: the REFERENCE's own
    Python frame loop executed over the oracle's kernels (tests/golden/gen_reference_loop.py). EVERY pixel within 1e-4 (observed 2.6e-5: the reference
    builds the importance tables with torch.cumsum, the engine sequentially; the MFMA material field is 3e-6 from the fp32 chain of torch.nn.Linear)."""
    import os
    if os.environ.get("MIRRES_TEST_SEED", "0") != "0":
        pytest.skip("the fixture holds the default frame (view / materials of sweep 0)")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loop.npz"))
    fx, fy, subdiv, ground, eh, ew = [int(v) for v in g["frame"]]
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=fx, fy=fy, subdiv=subdiv, ground=ground, env_hw=(eh, ew))
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    params, w0, w1, w2 = scene_mod.make_matnet_params(seed=0)
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.copy_(torch.from_numpy(params).cuda())
        for i, w in zip((0, 2, 4), (w0, w1, w2)):
            mlp.net.net[i].weight.copy_(torch.from_numpy(w).cuda())
    got = _run(F, W, mods, RR, torch, int(g["spp"]), mlp, seed=int(g["random_offset"]))
    for k, n in enumerate(["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]):
        r = g["outs"][k]
        pixel_parity(got[k], r, "reference loop frame / " + n, tol=1e-4)


def test_load_m_for_restir_matches_the_reference(oracle, scene_mod):
    """The 17-tuple of load_m_for_restir and the engine's default constants against what the REFERENCE's own load_m_for_restir produced
    (tests/golden/ref_loop.npz: buffer shapes / dtypes, neighbour offsets, the `defines` its Slang modules are compiled with)."""
    import os
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, _lib
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_loop.npz"))
    fx, fy = int(g["frame"][0]), int(g["frame"][1])
    mods = RR.load_m_for_restir(fx, fy)
    assert len(mods) == 17 and mods[15] == int(g["tile_count_size"][0]) and mods[16] == int(g["tile_count_size"][1])
    light_data, light_uv, light_inv_pdf, reservoirs, prev_reservoirs, final_samples, noff = mods[8:15]
    mine = ["%s %s" % (tuple(t.shape), str(t.dtype)) for t in (light_data, light_uv, light_inv_pdf, *reservoirs, *prev_reservoirs, *final_samples, noff)]
    assert mine == [str(x) for x in g["buffer_layout"]]
    assert np.array_equal(noff.cpu().numpy(), g["neighbor_offsets"])
    D = dict(zip([str(k_) for k_ in g["defines_keys"]], [int(v) for v in g["defines_vals"]]))
    c = _lib.default_config()
    assert (c.light_tile_count, c.light_tile_size, c.screen_tile_size, c.initial_light_samples, c.initial_brdf_samples, c.max_history, c.neighbor_offset_count,
            c.neighbor_count, int(c.gather_radius)) == tuple(D[k_] for k_ in ("LIGHT_TILE_COUNT", "LIGHT_TILE_SIZE", "SCREEN_TILE_SIZE", "INITIAL_LIGHT_SAMPLE_COUNT",
            "INITIAL_BRDF_SAMPLE_COUNT", "MAX_HISTORY_LENGTH", "NEIGHBOR_OFFSET_COUNT", "NEIGHBOR_COUNT", "GATHER_RADIUS"))
    assert c.max_bounce == 2 and abs(c.vis_near - 0.01) < 1e-9          # FinalShading.slang:7 MAX_Bounce, vis_near (:247)


def test_three_indirect_bounces_and_albedo_scale(oracle, scene_mod):
    """BASELINE configs[3] / [4] switches: `use_scale` albedo scaling of the looked-up materials (relighting, renderer_restir.py:404-408, with the
    clamp of the whole map) and a THIRD indirect bounce (MAX_Bounce is a runtime parameter here; the reference unrolls two) — one sample against the
    oracle, per-pixel, with the seeded hash-grid material field."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    sys_path = __import__("sys").path; sys_path.insert(0, __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden"))
    from gen_reference_loop import matnet_for
    F = SmallFrame(oracle, scene_mod)
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    params, w0, w1, w2 = scene_mod.make_matnet_params(seed=0)
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.copy_(torch.from_numpy(params).cuda())
        for i, w in zip((0, 2, 4), (w0, w1, w2)):
            mlp.net.net[i].weight.copy_(torch.from_numpy(w).cuda())
    mat, keep, _ = matnet_for(oracle, scene_mod)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    scale = (1.6, 0.7, 1.2)
    ctx = get_ctx(F.fx, F.fy, max_bounce=3)
    outs, _, _ = RR.render_fused(ctx, W, mlp, True, scale, cu(F.env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm), cu(F.ray_dir_raw),
                                 cu(F.pos), 1, 2, 2, 2.0, 0.1, 0.001, 4242)
    ref = oracle.render(F.fx, F.fy, 1, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=mat, max_bounce=3,
                        use_scale=True, scale=scale)
    two = oracle.render(F.fx, F.fy, 1, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=mat, max_bounce=2,
                        use_scale=True, scale=scale)
    assert np.abs(ref["indirect"] - two["indirect"]).max() > 1e-3          # the third bounce contributes
    for g_, n in zip(outs, ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]):
        g_ = g_.cpu().numpy(); r = ref[n]
        pixel_parity(g_, r, "three bounces + albedo scale / " + n, tol=0.0)        # the fp32-MFMA material field is an fmaf chain: bit-equal frame


def test_frame_with_other_restir_constants_matches_the_oracle(oracle, scene_mod):
    """The ReSTIR constants are runtime configuration (mirres_config_t): a frame with SEVEN spatial neighbours, 16 light candidates and a history cap of 7
    goes through the second instantiations of the spatial kernels inside mirres_render — k_spatial_gen<8, pixel pairs>, the traversal kernel's pair queue,
    k_spatial_resolve<8> on packed records — which the stepwise test of these constants (test_gpu_passes.py) does not reach. Bit for bit against the oracle's
    frame with the same constants, and different from the default constants' frame."""
    import torch
    from mirres_restir_nerf_mesh_amd import _lib, _ops
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    cfg = _lib.default_config(); cfg.neighbor_count, cfg.initial_light_samples, cfg.max_history = 7, 16, 7
    ctx = _ops.Context(F.fx, F.fy, cfg)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs, _, _ = RR.render_fused(ctx, W, None, False, (1, 1, 1), cu(F.env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm), cu(F.ray_dir_raw), cu(F.pos),
                                 4, 2, 2, 2.0, 0.1, 0.001, 4242)
    got = [o.cpu().numpy() for o in outs]
    args = (F.fx, F.fy, 4, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos)
    oracle.set_render_constants(7, 16, 7)
    try:
        ref = oracle.render(*args, mat=None)
    finally:
        oracle.set_render_constants()
    names = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]
    for g, n in zip(got, names):
        pixel_parity(g, ref[n], "frame with 7 neighbours / 16 candidates / history 7 / " + n, tol=0.0)
    dflt = oracle.render(*args, mat=None)
    assert not np.array_equal(dflt["diffuse"], ref["diffuse"])          # the constants reach the oracle's frame


def test_fused_equals_stepwise(oracle, scene_mod, monkeypatch):
    """The one-call fused loop and the reference-shaped Python loop run the same kernels; the only difference is that the stepwise path
    prepares ray_dir / brdf_map with torch ops (F.normalize rounds differently from the fused prep kernel by an ulp), so results agree to
    fp32 rounding on >= 99 % of the values (an ulp can still flip a discrete choice in a rare pixel)."""
    monkeypatch.setenv("MIRRES_TRAIN_FUSED", "0")     # the autograd path below must be the reference-shaped sample-by-sample loop
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    with torch.no_grad():
        mlp.encoder.params.mul_(1e3)
    fused = _run(F, W, mods, RR, torch, 3, mlp)
    env = torch.from_numpy(F.env).cuda().requires_grad_(True)    # forces the stepwise path
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = F.N; z = lambda *s: torch.zeros(s, device="cuda")
    RR.set_random_offset(4242)
    out = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, None, W, *mods[:8], *mods[8:17], env, cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]),
                                   cu(F.kd), cu(F.rm), cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, 3, 2, 2, 2.0, 0.1, 0.001)
    for a, b in zip(fused, out):
        b = b.detach().cpu().numpy()
        close = np.abs(a - b) <= 1e-5 + 1e-4 * np.abs(b)
        assert close.mean() >= 0.99, close.mean()
    out[0].sum().backward()
    assert env.grad is not None and float(env.grad.abs().sum()) > 0


def test_converges_to_oracle_statistically(oracle, scene_mod):
    """Many-sample means agree: the estimator (not just single decisions) is the same. 64 spp HIP vs 64 spp oracle, same seeds."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=32, fy=32, varied=False)
    got = _run(F, W, mods, RR, torch, 64, None)
    ref = oracle.render(F.fx, F.fy, 64, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=None)
    fg = F.occ > 0.5
    for g, n in zip(got, ["final_color", "diffuse", "spec", "indirect"]):
        a, b = g[fg].mean(0), ref[n][fg].mean(0)
        np.testing.assert_allclose(a, b, rtol=0.02, atol=2e-3, err_msg=n)
    assert psnr(np.clip(got[0], 0, 1), np.clip(ref["final_color"], 0, 1)) >= 30.0


def test_spp_slices_compose(oracle, scene_mod):
    """Multi-GPU sharding contract on one GPU: a slice [0,k) of the sample range leaves exactly the raw sums a k-spp frame accumulates, and
    mirres_render_finish on those sums reproduces the full frame; disjoint slices draw disjoint frame indices (sums differ)."""
    import ctypes as C
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = mods[0].ctx
    args = lambda: (ctx, W, None, False, (1, 1, 1), cu(F.env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm), cu(F.ray_dir_raw), cu(F.pos))
    full, _, _ = RR.render_fused(*args(), 3, 2, 2, 2.0, 0.1, 0.001, 555)
    sums, a, keep = RR.render_fused(*args(), 3, 2, 2, 2.0, 0.1, 0.001, 555, spp_range=(0, 3))
    outs = [torch.empty_like(s) for s in sums]
    for k in range(6):
        a.outs[k] = outs[k].data_ptr()
    arr = (C.c_void_p * 6)(*[s.data_ptr() for s in sums])
    check(lib().mirres_render_finish(ctx.h, C.byref(a), arr, stream_ptr()), "finish")
    for x, y in zip(full, outs):
        assert torch.equal(x, y)
    s01, _, _ = RR.render_fused(*args(), 3, 2, 2, 2.0, 0.1, 0.001, 555, spp_range=(0, 1))
    s13, _, _ = RR.render_fused(*args(), 3, 2, 2, 2.0, 0.1, 0.001, 555, spp_range=(1, 3))
    one, _, _ = RR.render_fused(*args(), 1, 0, 2, 2.0, 0.1, 0.001, 555, spp_range=(0, 1))
    assert torch.equal(s01[1], one[1])
    assert not torch.equal(s01[1], s13[1]) and float(s13[1].abs().sum()) > 0
    empty, _, _ = RR.render_fused(*args(), 3, 2, 2, 2.0, 0.1, 0.001, 555, spp_range=(3, 3))
    assert all(float(e.abs().sum()) == 0 for e in empty)
    # statistically equivalent: slice sums add up to the same mean radiance as the single-GPU run (within Monte-Carlo noise)
    tot = (s01[1] + s13[1]) / 3
    ref = sums[1]          # mirres_render_finish averaged the sums in place
    fg = torch.from_numpy(F.occ > 0.5).cuda()
    assert abs(float(tot[fg].mean()) - float(ref[fg].mean())) < 0.15 * float(ref[fg].mean()) + 1e-3


def test_stage1_training_step_backward(oracle, scene_mod):
    """BASELINE config 3 in miniature: kd / (roughness, metallic) from the material field (requires grad), learnable env map, stepwise
    run_restir_di_with_pt under autograd, image loss, backward. Gradients reach the hash grid, the MLP weights and the env map through
    FinalShading / EvaluateFinalSamples_di / EAWDenoise_run exactly where the reference's do (Resampling.py, Denoising.py)."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=40, fy=32)
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    torch.manual_seed(0)     # the MLP's kaiming init draws from the global generator: without this the test's inputs depend on what ran before it
    mn, mx = scene_mod.material_min_max(me_max=0.3)
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=11)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = F.N; z = lambda *s: torch.zeros(s, device="cuda")
    env = cu(F.env).requires_grad_(True)
    kdks = mlp.sample(cu(F.pos))                                   # nerf/renderer.py:1017-1022
    kd = kdks[:, 0:3].contiguous(); rm = torch.cat((kdks[:, 4:5], kdks[:, 5:6]), dim=-1).contiguous()
    normal = cu(F.normal).requires_grad_(True)
    RR.set_random_offset(777)
    out = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, None, W, *mods[:8], *mods[8:17], env, cu(F.occ[:, None].copy()), normal, cu(F.depth[:, None]), kd, rm,
                                   cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, 2, 2, 2, 2.0, 0.1, 0.001)
    RR.set_random_offset(None)
    target = torch.full((N, 3), 0.5, device="cuda")
    fg = cu(F.occ > 0.5)
    loss = (out[0][fg] - target[fg]).abs().mean() + 0.1 * (out[1][fg].mean() + out[2][fg].mean())
    loss.backward()
    for name, g in (("env", env.grad), ("grid", mlp.encoder.params.grad), ("w0", mlp.net.net[0].weight.grad), ("w2", mlp.net.net[4].weight.grad), ("normal", normal.grad)):
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, name
    # one optimiser step changes the loss in the right direction for a small enough step (first-order sanity of the whole chain)
    with torch.no_grad():
        env_new = (env - 1e-1 * env.grad / (env.grad.abs().max() + 1e-12)).clamp_(min=0.01)
    RR.set_random_offset(777)
    out2 = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, None, W, *mods[:8], *mods[8:17], env_new, cu(F.occ[:, None].copy()), normal.detach(), cu(F.depth[:, None]),
                                    kd.detach(), rm.detach(), cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, 2, 2, 2, 2.0, 0.1, 0.001)
    RR.set_random_offset(None)
    loss2 = (out2[0][fg] - target[fg]).abs().mean() + 0.1 * (out2[1][fg].mean() + out2[2][fg].mean())
    import os
    slack = 1e-4 if os.environ.get("MIRRES_TEST_SEED", "0") == "0" else 5e-4      # other views of the robustness sweep: the 2-spp loss is noisier than the step's gain
    assert float(loss2) < float(loss) + slack, (float(loss), float(loss2))


def test_pt_batch_is_bit_identical(oracle, scene_mod, monkeypatch):
    """mirres_render sends the path-tracing stages of K samples through one set of launches (K * N sample slots). Each slot uses the RNG stream
    its sample has in a sample-by-sample loop and the totals are added in sample / bounce order, so every output is bit-identical for any K
    (5 samples: K = 1, 2 with a ragged last batch, and 8 > spp)."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    with torch.no_grad():
        mlp.encoder.params.mul_(1e3)
    outs = {}
    for K in (1, 2, 8):
        monkeypatch.setenv("MIRRES_PT_BATCH", str(K))
        outs[K] = _run(F, W, mods, RR, torch, 5, mlp)
    for K in (2, 8):
        for a, b in zip(outs[1], outs[K]):
            assert np.array_equal(a, b), "K=%d differs from the sample-by-sample loop" % K


def test_strip_sharding_is_exact(oracle, scene_mod):
    """Multi-GPU strip scheme on one GPU (record / replay of the halo exchange): a rank that renders only its rows — local frame = own rows +
    30 halo rows, RNG seeded with global coordinates, halo rows of the packed reservoirs filled per sample with what the neighbouring rank
    computed — reproduces the single-GPU raw sums of its rows bit for bit (48 x 96 frame, two strips, 4 samples, material net)."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, dist as D, _lib
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=48, fy=96)
    fx, fy, spp = F.fx, F.fy, 4
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    with torch.no_grad():
        mlp.encoder.params.mul_(1e3)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = {"occ": cu(F.occ[:, None].copy()), "normal": cu(F.normal), "depth": cu(F.depth[:, None]), "kd": cu(F.kd), "rm": cu(F.rm), "ray_dir": cu(F.ray_dir_raw), "pos": cu(F.pos)}
    env = cu(F.env)
    def render(ctx, g, **kw):
        outs, _, _ = RR.render_fused(ctx, W, mlp, False, (1, 1, 1), env, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"], g["pos"],
                                     spp, 2, 2, 2.0, 0.1, 0.001, 909, **kw)
        torch.cuda.synchronize()
        return [o.clone() for o in outs]
    ctx_full = get_ctx(fx, fy)
    ref = render(ctx_full, full, spp_range=(0, spp))
    # the whole frame as a single strip: records every sample's pre-spatial reservoirs (what the ranks would exchange)
    rec = {}
    def recorder(user, records, sample, stream):
        rec[sample] = D.device_view(records, (fy, fx, 8)).clone()
        return 0
    one = render(ctx_full, full, strip=(fy, 0, 0, fy), halo=_lib.HALO_FN(recorder))
    assert sorted(rec) == list(range(spp))
    for a, b in zip(ref, one):
        assert torch.equal(a, b)
    for rank in range(2):
        y0, y1, lo, hi = D.strip_rows(fy, rank, 2)
        assert (hi - lo) < fy                                       # a real halo: the local frame is smaller than the image
        plan = D.halo_plan(fy, fx, rank, 2)
        loc = {k: v[lo * fx:hi * fx].contiguous() for k, v in full.items()}
        def replay(user, records, sample, stream, lo=lo, hi=hi, plan=plan):
            view = D.device_view(records, (hi - lo, fx, 8))
            for peer, send, (ra, rb) in plan:
                view[ra:rb].copy_(rec[sample][lo + ra:lo + rb])
            return 0
        got = render(get_ctx(fx, hi - lo), loc, strip=(fy, lo, y0 - lo, y1 - lo), halo=_lib.HALO_FN(replay))
        for a, b in zip(ref, got):
            assert torch.equal(a[y0 * fx:y1 * fx], b[(y0 - lo) * fx:(y1 - lo) * fx]), "rank %d" % rank
        # the same strip with the exchange off the chain (strip_overlap): the callback is handed the engine's side stream, the interior rows' spatial pass runs
        # before the halo rows have arrived, the border rows after — and not a bit changes
        seen = []
        def replay_side(user, records, sample, stream, lo=lo, hi=hi, plan=plan):
            seen.append(int(stream or 0))
            with D.on_stream(stream):
                view = D.device_view(records, (hi - lo, fx, 8))
                for peer, send, (ra, rb) in plan:
                    view[ra:rb].fill_(float("nan"))                       # whatever the interior pass may read too early would poison the frame
                    torch.cuda._sleep(200000)                           # a slow exchange: ~0.1 ms on the side stream
                    view[ra:rb].copy_(rec[sample][lo + ra:lo + rb])
            return 0
        got2 = render(get_ctx(fx, hi - lo), loc, strip=(fy, lo, y0 - lo, y1 - lo), halo=_lib.HALO_FN(replay_side), strip_overlap=True)
        assert len(seen) == spp and all(st != torch.cuda.current_stream().cuda_stream for st in seen)
        for a, b in zip(ref, got2):
            assert torch.equal(a[y0 * fx:y1 * fx], b[(y0 - lo) * fx:(y1 - lo) * fx]), "rank %d with strip_overlap" % rank


def _strip_rank(rank, world, port, out):
    import os, sys
    import numpy as np
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # both ranks share cuda:0; halos are staged through the host (dist.exchange_halos)
    torch.cuda.set_device(0)
    import mirres_restir_nerf_mesh_amd as M
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, dist as D, harness
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    S = M.scene
    v, t = S.make_mesh(3, 8)
    W = RR.restirbvhWorker(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()); W.update_mesh(W.vrt, W.v_ind)
    g = harness.build_gbuffer(W, 96, 128, 1)          # 96 rows: the boundary between two strips of at least 30 rows has room to move (measured balancing below)
    env = torch.from_numpy(S.make_env(16, 32)).cuda()
    ctx = get_ctx(g["fx"], g["fy"])
    outs = D.render_strips(ctx, W, None, env, g, 3, 4321, rank, world)
    res = {"outs": [o.cpu() for o in outs]}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # gloo stages the exchange through the host: dist.render_strips says so once and runs the in-line exchange
        over = D.render_strips(ctx, W, None, env, g, 3, 4321, rank, world, overlap=True)      # on gloo this is the FALLBACK: overlap requested, in-line exchange run
    res["overlap_requested_on_gloo"] = [o.cpu() for o in over]                                  # (the side-stream path over RCCL: test_gpu_rccl.py; single-process replay: above)
    # measured balancing (round 5): three frames whose boundaries move with the strips' own times — any partition must give the same bits
    bal = D.StripBalancer(g["fy"], world)
    res["balanced"], res["bounds"] = [], []
    for frame in range(3):
        if frame == 1:
            bal.corr[g["fy"] // 2:] *= 6.0; bal.corr /= bal.corr.mean()      # (and a deliberately lopsided correction, so that the boundary really moves)
        o = D.render_strips(ctx, W, None, env, g, 3, 4321, rank, world, balancer=bal)
        res["balanced"].append([x.cpu() for x in o]); res["bounds"].append(list(bal.last_bounds))
    res["history"] = len(bal.history)
    res["busy_total_waited"] = [bal.last_total_ms is not None and bal.last_wait_ms is not None and 0 <= bal.last_wait_ms < bal.last_total_ms]
    if rank == 0:
        ref = D.render_strips(ctx, W, None, env, g, 3, 4321, 0, 1)      # world == 1: the ordinary single-GPU frame
        res["ref"] = [o.cpu() for o in ref]
    torch.save(res, os.path.join(out, "strip%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_strip_render_equals_single_gpu(tmp_path):
    """End to end through dist.render_strips with two processes (gloo; both on this GPU): per-sample halo exchange, row all-gather and the
    replicated finish give, on every rank, the single-GPU frame bit for bit — all six output buffers."""
    import os
    import torch
    import torch.multiprocessing as mp
    port = 33500 + (os.getpid() % 2000)
    from util import spawn_ranks
    spawn_ranks(_strip_rank, (2, port, str(tmp_path)), 2)
    r0 = torch.load(os.path.join(tmp_path, "strip0.pt")); r1 = torch.load(os.path.join(tmp_path, "strip1.pt"))
    for k in range(6):
        assert torch.equal(r0["outs"][k], r0["ref"][k]), "rank 0 buffer %d" % k
        assert torch.equal(r1["outs"][k], r0["ref"][k]), "rank 1 buffer %d" % k
        assert torch.equal(r0["overlap_requested_on_gloo"][k], r0["ref"][k]) and torch.equal(r1["overlap_requested_on_gloo"][k], r0["ref"][k]), \
            "overlap requested on a host-staged backend (falls back to the in-line exchange), buffer %d" % k
        for frame in range(3):
            assert torch.equal(r0["balanced"][frame][k], r0["ref"][k]) and torch.equal(r1["balanced"][frame][k], r0["ref"][k]), "balanced frame %d, buffer %d" % (frame, k)
    assert r0["bounds"] == r1["bounds"] and len(set(tuple(b) for b in r0["bounds"])) >= 2, r0["bounds"]      # same partition on both ranks, and it moved
    assert r0["history"] == 2 and r1["history"] == 2                                                       # frames 2 and 3 used the times of frames 1 and 2
    assert r0["busy_total_waited"] == [True] and r1["busy_total_waited"] == [True]                         # the exchanged time is the strip's own: exchange waits taken out


def test_fused_training_gradients_match_the_stepwise_loop(oracle, scene_mod, monkeypatch):
    """Training path: the batched forward + single backward call (_FusedLoop: mirres_render with a tape, mirres_render_bwd) against the
    reference-shaped loop of per-sample autograd Functions (FinalShading / EvaluateFinalSamples_di), same random offset. The forward agrees
    like test_fused_equals_stepwise; gradients w.r.t. env map, normal, kd and (roughness, metallic) agree to fp32 summation order (atomics
    into the env texels) up to the rare pixel whose discrete choice flips on the F.normalize ulp."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    N = F.N; z = lambda *s: torch.zeros(s, device="cuda")
    wgt = torch.rand((N, 3), generator=torch.Generator().manual_seed(1)).cuda()
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MIRRES_TRAIN_FUSED", mode)
        RR.set_random_offset(4242)
        env = cu(F.env).requires_grad_(True); nrm = cu(F.normal).requires_grad_(True); kd = cu(F.kd).requires_grad_(True); rm = cu(F.rm).requires_grad_(True)
        out = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, mlp, None, W, *mods[:8], *mods[8:17], env, cu(F.occ[:, None].copy()), nrm, cu(F.depth[:, None]), kd, rm,
                                       cu(F.ray_dir_raw), cu(F.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), F.fx, F.fy, 3, 2, 2, 2.0, 0.1, 0.001)
        loss = (out[0] * wgt).sum() + 0.5 * (out[1] * wgt).sum() + 0.25 * out[2].sum()
        loss.backward()
        res[mode] = dict(out=[o.detach().cpu().numpy() for o in out], g=[t.grad.cpu().numpy() for t in (env, nrm, kd, rm)])
    for a, b in zip(res["0"]["out"], res["1"]["out"]):
        assert np.isclose(a, b, rtol=1e-4, atol=1e-6).mean() >= 0.99
    for name, a, b in zip(("env", "normal", "kd", "rm"), res["0"]["g"], res["1"]["g"]):
        assert np.isfinite(b).all() and np.abs(b).sum() > 0, name
        cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
        rel = float(np.linalg.norm(a - b) / (np.linalg.norm(a) + 1e-30))
        assert cos > 0.999 and rel < 0.05, "%s: cos %.6f rel %.4f" % (name, cos, rel)


def test_degenerate_frames(oracle, scene_mod):
    """Edge cases of the frame against the oracle: a frame that is not a multiple of any tile size (7 x 5), an all-background frame, a black environment
    (every row of the importance table takes the uniform fallback), and material extremes (roughness at its floor, metallic 1) — no NaN, background = 1,
    per-pixel agreement as in the 1-spp test."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    names = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def both(F, W, env, occ, kd, rm, spp=1, seed=31):
        outs, _, _ = RR.render_fused(get_ctx(F.fx, F.fy), W, None, False, (1, 1, 1), cu(env), cu(occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(kd), cu(rm),
                                     cu(F.ray_dir_raw), cu(F.pos), spp, 2, 2, 2.0, 0.1, 0.001, seed)
        ref = oracle.render(F.fx, F.fy, spp, seed, (F.info, F.aabb), F.vert, F.tri, env, occ, F.normal, F.depth, kd, rm, F.ray_dir_raw, F.pos, mat=None)
        return [o.cpu().numpy() for o in outs], ref

    def worker(F):
        W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
        return W
    # (a) ragged tiny frame, 2 samples
    F = SmallFrame(oracle, scene_mod, fx=7, fy=5, subdiv=2, ground=4, env_hw=(8, 16))
    W = worker(F)
    got, ref = both(F, W, F.env, F.occ, F.kd, F.rm, spp=2)
    for g_, n_ in zip(got, names):
        assert np.isfinite(g_).all()
        pixel_parity(g_, ref[n_], "ragged 7x5 frame / " + n_, tol=0.0)
    # (b) nothing but background
    got, ref = both(F, W, F.env, np.zeros_like(F.occ), F.kd, F.rm)
    assert all(np.isfinite(g_).all() for g_ in got) and (got[0] == 1.0).all() and (ref["final_color"] == 1.0).all() and all((g_ == 0).all() for g_ in got[1:])
    # (c) black environment: zero radiance everywhere, no NaN from the empty importance table
    F2 = SmallFrame(oracle, scene_mod, fx=24, fy=20, subdiv=2, ground=4, env_hw=(8, 16))
    W2 = worker(F2)
    got, ref = both(F2, W2, np.zeros_like(F2.env), F2.occ, F2.kd, F2.rm)
    fg = F2.occ > 0.5
    assert all(np.isfinite(g_).all() for g_ in got) and all((g_[fg] == 0).all() for g_ in got) and (ref["final_color"][fg] == 0).all() and (got[0][~fg] == 1).all()
    # (d) material extremes
    rm = F2.rm.copy(); rm[::2, 0] = 0.0; rm[1::2, 0] = 1.0; rm[::3, 1] = 1.0; rm[1::3, 1] = 0.0
    kd = F2.kd.copy(); kd[::5] = 0.0; kd[1::5] = 1.0
    got, ref = both(F2, W2, F2.env, F2.occ, kd, rm)
    for g_, n_ in zip(got, names):
        assert np.isfinite(g_).all()
        pixel_parity(g_, ref[n_], "material extremes / " + n_, tol=0.0)


def test_hostile_shading_inputs_match_the_oracle(oracle, scene_mod):
    """Shading-side hostile inputs against the oracle, bit for bit (NaNs must sit in the same places): the shading translation units divide
    and take square roots with short sequences (device_math.hpp mr_div / mr_sqrt) that equal IEEE division only inside 2^-102 .. 2^102 — these frames leave that
    comfort zone on purpose: (e) an HDR environment spanning 1e-30 .. 1e6 with exact zeros; (f) the same with NaN and +inf texels; (g) roughness on both sides of
    the alpha < 1e-4 switch (brdfDi.slang:169-199) and of the 0.01 clamp; (h) grazing shading normals (n.v ~ 1e-7) and normals facing away; (i) an environment
    whose importance pdfs underflow (radiance 1e-38 next to 1e-3)."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    names = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    F = SmallFrame(oracle, scene_mod, fx=24, fy=20, subdiv=2, ground=4, env_hw=(8, 16))
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)

    def check(what, env, normal, kd, rm, spp=2, seed=77):
        outs, _, _ = RR.render_fused(get_ctx(F.fx, F.fy), W, None, False, (1, 1, 1), cu(env), cu(F.occ[:, None].copy()), cu(normal), cu(F.depth[:, None]), cu(kd), cu(rm),
                                     cu(F.ray_dir_raw), cu(F.pos), spp, 2, 2, 2.0, 0.1, 0.001, seed)
        ref = oracle.render(F.fx, F.fy, spp, seed, (F.info, F.aabb), F.vert, F.tri, env, F.occ, normal, F.depth, kd, rm, F.ray_dir_raw, F.pos, mat=None)
        rep = os.environ.get("MIRRES_PARITY_REPORT")
        for o_, n_ in zip(outs, names):
            g_ = np.ascontiguousarray(o_.cpu().numpy(), dtype=np.float32); r_ = np.ascontiguousarray(ref[n_], dtype=np.float32)
            same = (g_.view(np.uint32) == r_.view(np.uint32)) | (np.isnan(g_) & np.isnan(r_))
            if rep:
                with open(rep, "a") as f:
                    f.write("hostile shading inputs / %s / %s: %d of %d values differ (NaN in the oracle: %d, inf: %d)\n" % (what, n_, int((~same).sum()), same.size, int(np.isnan(r_).sum()), int(np.isinf(r_).sum())))
            assert same.all(), "%s / %s: %d of %d values differ; first: got %r want %r" % (what, n_, int((~same).sum()), same.size, g_[~same][:4], r_[~same][:4])
        return ref
    rng = np.random.default_rng(12)
    Hc, Wc = 8, 16
    # (e) radiance over 36 decades, a tenth of the texels exactly zero
    env = (10.0 ** rng.uniform(-30, 6, (Hc, Wc, 3))).astype(np.float32)
    env[rng.random((Hc, Wc)) < 0.1] = 0.0
    ref = check("HDR 1e-30..1e6 with zeros", env, F.normal, F.kd, F.rm)
    assert np.isfinite(ref["final_color"]).all()
    # (f) + NaN and +inf texels
    env2 = env.copy(); env2[1, 3] = np.nan; env2[5, 9, 1] = np.inf; env2[6, 2] = np.inf
    check("HDR with NaN and +inf texels", env2, F.normal, F.kd, F.rm)
    # (g) roughness around the alpha = r^2 < 1e-4 switch and the 0.01 clamp; metallic extremes
    rm = F.rm.copy()
    vals = np.array([0.0, 0.0099, 0.0099999, 0.01, 0.0100001, 0.010001, 0.02, 1.0, 1e-30, 0.999999], np.float32)
    rm[:, 0] = vals[np.arange(F.N) % len(vals)]; rm[::7, 1] = 1.0; rm[3::7, 1] = 0.0
    check("roughness at the alpha switch", F.env, F.normal, F.kd, rm)
    # (h) grazing and back-facing shading normals
    v = -F.ray_dir
    t = np.cross(v, np.array([0.3, 0.5, 0.8], np.float32)); t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-20)
    nrm = F.normal.copy()
    sel = (np.arange(F.N) % 3 == 0) & (F.occ > 0.5)
    eps = np.where(np.arange(F.N) % 2 == 0, 1e-7, -1e-7).astype(np.float32)[:, None]
    g = t + eps * v; g /= np.linalg.norm(g, axis=1, keepdims=True)
    nrm[sel] = g[sel].astype(np.float32)
    back = (np.arange(F.N) % 11 == 5) & (F.occ > 0.5)
    nrm[back] = (-F.normal[back]).astype(np.float32)
    check("grazing and back-facing normals", F.env, nrm, F.kd, F.rm)
    # (i) importance pdfs that underflow: 1e-38 next to 1e-3 (the dark texels' pdf is a denormal)
    env3 = np.full((Hc, Wc, 3), 1e-38, np.float32); env3[2, 4] = 1e-3; env3[6, 11] = 7e-4
    check("underflowing pdfs", env3, F.normal, F.kd, F.rm)


def test_stage1_loop_with_reference_losses(scene_mod):
    """BASELINE config 3 as a loop: harness.render_stage1_outputs (moved mesh -> BVH -> G-buffer front half -> jittered material
    taps -> run_restir_di_with_pt under autograd -> tone curve / alpha) feeding losses.stage1_loss with main.py's default weights and
    losses.stage1_optimizer_step with the reference's three optimisers (geometry / material / light, nerf/utils.py:1565-1589).  Three steps at
    40 x 32, 2 spp: every loss is finite, all three parameter groups receive finite non-zero gradients and move, the light stays >= 0.01, and
    with the sampling seed pinned the loss of step 3 is below the loss of step 1."""
    import types
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness, losses
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    torch.manual_seed(0)
    v, t = scene_mod.make_mesh(4, 8)
    vt = torch.from_numpy(v).cuda(); tt = torch.from_numpy(t).cuda()
    W = RR.restirbvhWorker(vt, tt); W.update_mesh(W.vrt, W.v_ind)
    mn, mx = scene_mod.material_min_max(me_max=0.3)
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=11)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    H, Wd = 32, 40
    mods = RR.load_m_for_restir(Wd, H)
    env = torch.full((32, 64, 3), 0.5, device="cuda", requires_grad=True)          # create_trainable_env_rnd(scale=0, bias=0.5), network.py:126
    voff = torch.zeros_like(vt).requires_grad_(True)
    o_geo = torch.optim.Adam([voff], lr=1e-4); o_mat = torch.optim.Adam(mlp.parameters(), lr=1e-2); o_light = torch.optim.Adam([env], lr=3e-2)
    gt = torch.full((H * Wd, 3), 0.8, device="cuda"); gt_lin = gt ** 2.2
    opt = types.SimpleNamespace(use_brdf=True)
    p0 = [p.detach().clone() for p in (voff, mlp.encoder.params, mlp.net.net[0].weight, env)]
    vals = []
    for it in range(3):
        for o in (o_geo, o_mat, o_light):
            o.zero_grad()
        RR.set_random_offset(1234); torch.manual_seed(7)
        out = harness.render_stage1_outputs(W, vt, voff, tt, mlp, env, mods, H, Wd, 2, with_normal_ao=(it == 2))
        opt.lambda_extra_kd = 0.01 if it == 2 else 0.0          # the last step also runs process_normal_ao and the extra kd term
        fg = out["occ"][:, 0] > 0.5
        assert int(fg.sum()) > 100 and torch.equal(out["image_brdf"][~fg], torch.ones_like(out["image_brdf"][~fg]))      # background = bg_color
        loss = losses.stage1_loss(out, gt, gt_lin, opt, vertices=vt, voffsets=voff, triangles=tt)
        vals.append(losses.stage1_optimizer_step(loss, o_geo, o_mat, o_light, light_base=env, encoder_params=mlp.encoder.params))
        for name, p in (("voff", voff), ("grid", mlp.encoder.params), ("w0", mlp.net.net[0].weight), ("env", env)):
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            if it > 0 or name != "voff":       # at zero offsets the offset L2 has zero gradient; the Laplacian term moves them from step 1 on
                assert float(p.grad.abs().sum()) > 0, name
        assert float(env.detach().min()) >= np.float32(0.01)
    RR.set_random_offset(None)
    assert all(np.isfinite(vals)), vals
    for name, a, b in zip(("voff", "grid", "w0", "env"), p0, (voff, mlp.encoder.params, mlp.net.net[0].weight, env)):
        assert float((a - b.detach()).abs().max()) > 0, name
    assert vals[1] < vals[0], vals


def test_frame_refuses_wrongly_sized_inputs(oracle, scene_mod):
    """The per-pixel inputs are indexed as [N, width] rows by the kernels; the host mirror refuses any other size instead of launching."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod)
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd._lib import MirresError
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    good = dict(env=cu(F.env), occ=cu(F.occ[:, None].copy()), normal=cu(F.normal), depth=cu(F.depth[:, None]), kd=cu(F.kd), rm=cu(F.rm), rd=cu(F.ray_dir_raw), pos=cu(F.pos))
    def call(**over):
        a = dict(good); a.update(over)
        return RR.render_fused(get_ctx(F.fx, F.fy), W, None, False, (1, 1, 1), a["env"], a["occ"].clone(), a["normal"], a["depth"], a["kd"], a["rm"], a["rd"], a["pos"],
                               1, 2, 2, 2.0, 0.1, 0.001, 1)
    call()
    for key, bad in (("normal", good["normal"][:-1]), ("depth", torch.cat((good["depth"], good["depth"]), 1)), ("rm", good["rm"][:, :1]), ("pos", good["pos"][:10]),
                     ("occ", good["occ"][:-3]), ("env", good["env"].reshape(-1, 3))):
        with pytest.raises(MirresError):
            call(**{key: bad.contiguous()})


def test_context_cache_is_bounded_and_keyed_by_the_resolved_configuration(monkeypatch):
    """_ops.get_ctx: `max_bounce=None` and the configuration default share one context (one batch pool), the cache holds at most MIRRES_CTX_CACHE
    contexts (least recently used dropped first) and a dropped context is destroyed once nothing refers to it."""
    import gc, weakref
    from mirres_restir_nerf_mesh_amd import _ops, _lib
    monkeypatch.setenv("MIRRES_CTX_CACHE", "2")
    _ops._CTX_CACHE.clear()
    d = int(_lib.default_config().max_bounce)
    a = _ops.get_ctx(24, 16)
    assert _ops.get_ctx(24, 16, max_bounce=d) is a and _ops.get_ctx(24, 16, None) is a and len(_ops._CTX_CACHE) == 1
    b = _ops.get_ctx(24, 16, max_bounce=d + 1)
    assert b is not a and len(_ops._CTX_CACHE) == 2
    wa = weakref.ref(a); ha = a.h
    _ops.get_ctx(24, 16)                      # touch a: b is now the least recently used
    c = _ops.get_ctx(32, 16)
    assert len(_ops._CTX_CACHE) == 2 and _ops.get_ctx(24, 16) is a and _ops.get_ctx(32, 16) is c
    wb = weakref.ref(b); del b; gc.collect()
    assert wb() is None                       # evicted and unreferenced: destroyed (its pools are freed in __del__)
    del a; gc.collect()
    assert wa() is not None                   # still cached
    _ops._CTX_CACHE.clear(); del c; gc.collect()
    assert wa() is None


def test_batch_pool_fallback_keeps_the_frame_and_is_remembered(oracle, scene_mod, monkeypatch):
    """When the device cannot hold the K-sample batch pool, carve_batch halves K until it fits (MIRRES_POOL_LIMIT_MB stands in for a full HBM),
    remembers the size that fitted for the following frames, and — the frame being independent of the batch size — returns the same bits."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=40, fy=32)
    from mirres_restir_nerf_mesh_amd import _ops
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    def frame(ctx):
        outs, _, _ = RR.render_fused(ctx, W, None, False, (1, 1, 1), cu(F.env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm),
                                     cu(F.ray_dir_raw), cu(F.pos), 8, 2, 2, 2.0, 0.1, 0.001, 31337)
        torch.cuda.synchronize()
        return [o.clone() for o in outs]
    _ops._CTX_CACHE.clear()
    ref = frame(_ops.get_ctx(F.fx, F.fy))                 # 8 samples in one batch
    _ops._CTX_CACHE.clear()
    # ~670 B per slot x 1280 pixels ~ 0.86 MB per sample + 8 MB of light tiles per sample: a 30 MB cap admits a batch of 2 or 3, not 8
    monkeypatch.setenv("MIRRES_POOL_LIMIT_MB", "30")
    ctx = _ops.get_ctx(F.fx, F.fy)
    a = frame(ctx); b = frame(ctx)
    for x, y, z in zip(ref, a, b):
        assert torch.equal(x, y) and torch.equal(x, z)
    monkeypatch.setenv("MIRRES_POOL_LIMIT_MB", "1")       # not even one sample fits: a clean error, and the context recovers afterwards
    _ops._CTX_CACHE.clear()
    ctx = _ops.get_ctx(F.fx, F.fy)
    from mirres_restir_nerf_mesh_amd._lib import MirresError
    with pytest.raises(MirresError, match="batch pool"):
        frame(ctx)
    monkeypatch.delenv("MIRRES_POOL_LIMIT_MB")
    c = frame(ctx)
    for x, y in zip(ref, c):
        assert torch.equal(x, y)
    _ops._CTX_CACHE.clear()


def _scaled_mlp(scene_mod, torch):
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    with torch.no_grad():
        mlp.encoder.params.mul_(1e3)
    return mlp


def test_schedule_does_not_change_a_small_frame(oracle, scene_mod, monkeypatch):
    """Every schedule mirres_render can be switched to sends each sample through the same chain code (render.hip chain_sample) — on the caller's stream, or as
    bands of rows on up to three chain streams — and the other stages through one to four side streams. 48 x 144 (the smallest height band_count cuts into three
    bands of >= 48 rows), 7 samples in batches of 3, 3, 1: a first-of-batch temporal merge, fused merges and a ragged last batch. All six buffers, bit for bit,
    against the frame of one stream and sample-by-sample batches."""
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=48, fy=144)
    mlp = _scaled_mlp(scene_mod, torch)
    def frame(streams, batch, bands=None, chain=None):
        for k, v in (("MIRRES_STREAMS", streams), ("MIRRES_PT_BATCH", batch), ("MIRRES_BANDS", bands), ("MIRRES_CHAIN_STREAMS", chain)):
            monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, str(v))
        return [torch.from_numpy(o) for o in _run(F, W, mods, RR, torch, 7, mlp)]
    ref = frame(1, 1)
    assert len(ref) == 6
    for cfg in [(n, 3) for n in (2, 3, 4, 5)] + [(2, 3, 2, 1), (2, 3, 2, 2), (2, 3, 3, 3)]:
        for k, (a, b) in enumerate(zip(ref, frame(*cfg))):
            assert torch.equal(a, b), "streams / batch / bands / chain streams %r: buffer %d differs" % (cfg, k)


def test_a_frame_leaves_nothing_behind_in_the_context(oracle, scene_mod, monkeypatch):
    """What a frame needs beyond its arguments (strip offset, own-pixel occupancy, packed G records, row restriction, clean work heads) travels as arguments of
    its launches, so neither a strip frame with strip_overlap nor a frame that fails can change what the stepwise ABI computes afterwards on the same context:
    initial -> temporal -> spatial give the bits of a freshly created context. Rank 0 of the two-rank split of a 48 x 96 image (local frame: 78 rows)."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, Resampling as RS, dist as D, _lib, _ops
    F, W, mods, RR, torch = _setup(oracle, scene_mod, fx=48, fy=96)
    fx, fy, spp = F.fx, F.fy, 2
    mlp = _scaled_mlp(scene_mod, torch)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = {"occ": cu(F.occ[:, None].copy()), "normal": cu(F.normal), "depth": cu(F.depth[:, None]), "kd": cu(F.kd), "rm": cu(F.rm), "ray_dir": cu(F.ray_dir_raw), "pos": cu(F.pos)}
    env = cu(F.env)
    def render(ctx, g, n, **kw):
        outs, _, _ = RR.render_fused(ctx, W, mlp, False, (1, 1, 1), env, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"], g["pos"],
                                     n, 2, 2, 2.0, 0.1, 0.001, 909, **kw)
        torch.cuda.synchronize()
        return [o.clone() for o in outs]
    rec = {}
    def recorder(user, records, sample, stream):
        rec[sample] = D.device_view(records, (fy, fx, 8)).clone()
        return 0
    ref = render(_ops.Context(fx, fy), full, spp, strip=(fy, 0, 0, fy), halo=_lib.HALO_FN(recorder))
    y0, y1, lo, hi = D.strip_rows(fy, 0, 2)
    plan = D.halo_plan(fy, fx, 0, 2)
    loc = {k: v[lo * fx:hi * fx].contiguous() for k, v in full.items()}
    def replay_side(user, records, sample, stream):
        with D.on_stream(stream):
            view = D.device_view(records, (hi - lo, fx, 8))
            for peer, send, (ra, rb) in plan:
                view[ra:rb].copy_(rec[sample][lo + ra:lo + rb])
        return 0
    used, fresh = _ops.Context(fx, hi - lo), _ops.Context(fx, hi - lo)
    got = render(used, loc, spp, strip=(fy, lo, y0 - lo, y1 - lo), halo=_lib.HALO_FN(replay_side), strip_overlap=True)
    for a, b in zip(ref, got):
        assert torch.equal(a[y0 * fx:y1 * fx], b[(y0 - lo) * fx:(y1 - lo) * fx])      # the strip frame was the real thing
    monkeypatch.setenv("MIRRES_POOL_LIMIT_MB", "1")      # 8 samples need a larger batch pool than the strip frame left: refused, inside mirres_render
    with pytest.raises(_lib.MirresError, match="batch pool"):
        render(used, loc, 8)
    monkeypatch.delenv("MIRRES_POOL_LIMIT_MB")
    # the stepwise sequence of test_gpu_passes.py::test_reservoir_chain on a frame of the local size, on both contexts
    S = SmallFrame(oracle, scene_mod, fx=fx, fy=hi - lo)
    WS = RR.restirbvhWorker(cu(S.vert), cu(S.tri)); WS.update_mesh(WS.vrt, WS.v_ind)
    T = dict(occ=cu(S.occ[:, None]), pos=cu(S.pos), nd=cu(S.normal_depth), brdf=cu(S.brdf), rd=cu(S.ray_dir), tex=cu(S.tex), noff=cu(S.noff))
    pdf, cdf, mpdf, mcdf = (cu(t) for t in S.tables)
    tile_ld, _, tile_pdf = oracle.light_tiles(S.frame, 1000)
    tile_ld, tile_pdf = cu(tile_ld), cu(tile_pdf)
    new_res = lambda: (torch.zeros((S.N, 3), device="cuda"), torch.zeros((S.N, 1), device="cuda"), torch.zeros((S.N, 1), dtype=torch.int32, device="cuda"), torch.zeros((S.N, 1), device="cuda"))
    def stepwise(ctx):
        m = _ops.Module("stepwise", ctx)
        r0, r1, rs = new_res(), new_res(), new_res()
        for r, frame in ((r0, 1002), (r1, 1022)):
            WS.InitialResampling_(m, T["pos"], r, T["tex"], S.Wc, S.Hc, S.fx, S.fy, frame, T["occ"], T["nd"], T["brdf"], T["rd"], pdf, cdf, mpdf, mcdf, tile_ld, None, tile_pdf)
        RS.TemporalResampling(m, r1, r0, T["tex"], S.Wc, S.Hc, S.fx, S.fy, 1023, T["occ"], T["nd"], T["brdf"], T["rd"], T["occ"], T["nd"], T["brdf"], T["rd"], None)
        WS.SpatialResampling_(m, T["pos"], rs, r1, T["noff"], T["tex"], S.Wc, S.Hc, S.fx, S.fy, 1024, T["occ"], T["nd"], T["brdf"], T["rd"])
        torch.cuda.synchronize()
        return [t.clone() for r in (r0, r1, rs) for t in r]
    a, b = stepwise(used), stepwise(fresh)
    assert int(a[10].sum()) > 0                      # the spatial pass produced reservoirs (M of the spatial output)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "stepwise buffer %d differs after a strip frame and a failed frame on the same context" % k
