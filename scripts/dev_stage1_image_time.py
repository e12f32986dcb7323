"""Times the position adjoint of the stage-0 radiance network (csrc/radiance_pos.hip, stage0.RadianceField.backward_pos) and one stage-1 training step with and
without the NeRF colour branch (harness.render_stage1_outputs(field=...)), with the method of dev_radiance_bwd_time.py: windows of --inner back-to-back launches
between two device events, the cases taking turns within each of --reps rounds, one warm-up each.
  kernel     2^18 and 2^20 points, dev_radiance_bwd_time.py's point sets (seeded random table and weights; uniform in the ball of radius 0.6, all inside one cell
             of level 0, all out of bounds): backward_pos beside the forward (rgb alone) and mirres_radiance_points_bwd on the same points;
  step       one stage-1 step at scripts/train_step_bench.py's shape (800 x 800, spp 32, make_mesh(7, 64)) under a dataset camera — render_stage1_outputs,
             losses.stage1_loss, backward, the three optimisers — without the field, with it, and with --enable_offset_nerf_grad, the three alternated.
A record for DESIGN.md section 5.17, not a gate: no thresholds.

    python scripts/dev_stage1_image_time.py [--reps 5] [--inner 20] [--res 800] [--spp 32] [--skip_step] [--out profiles/stage1_image_time.json]
"""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_radiance_time import alternating  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5); p.add_argument("--inner", type=int, default=20); p.add_argument("--res", type=int, default=800)
    p.add_argument("--spp", type=int, default=32); p.add_argument("--skip_step", action="store_true"); p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np, torch
    import mirres_restir_nerf_mesh_amd as M
    from mirres_restir_nerf_mesh_amd import stage0, harness, losses, raster, renderer_restir as RR
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    from train_stage1 import orbit_pose
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    net, total = stage0.density_layout(1.0)
    rnd = stage0.RadianceField(torch.randn((total, 2), generator=g, device="cuda"), *(torch.randn(s, generator=g, device="cuda") * 0.15
                               for s in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))), bound=1.0)
    res = {"reps": a.reps, "inner": a.inner, "gathers_per_point": 128}
    for n in (1 << 18, 1 << 20):
        v = torch.randn((n, 3), generator=g, device="cuda")
        ball = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()
        s0 = float(net.scale[0])
        cell = ((torch.tensor([7.0, 5.0, 8.0], device="cuda") + 0.05 + 0.9 * torch.rand((n, 3), generator=g, device="cuda") - 0.5) / s0 * 2 - 1).contiguous()
        outside = (ball + 2.0).contiguous()
        d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        grgb = torch.randn((n, 3), generator=g, device="cuda")
        grads = [torch.zeros_like(getattr(rnd, k)) for k in rnd.PARAMETER_NAMES]
        cases = {"rgb_ball_ms": lambda: rnd.rgb(ball, d), "backward_pos_ball_ms": lambda: rnd.backward_pos(ball, d, None, grgb),
                 "backward_points_ball_ms": lambda: rnd.backward_points(ball, d, None, grgb, grads=grads),
                 "backward_pos_one_cell_ms": lambda: rnd.backward_pos(cell, d, None, grgb), "backward_pos_out_of_bounds_ms": lambda: rnd.backward_pos(outside, d, None, grgb)}
        r = alternating(cases, a.reps, a.inner)
        r["backward_pos_ball_Mpoints_per_s"] = n / r["backward_pos_ball_ms"][0] / 1e3
        res["points_%d" % n] = r
        print(json.dumps({n: r}), flush=True)
    if not a.skip_step:
        torch.manual_seed(0); np.random.seed(0)
        S = M.scene
        v, t = S.make_mesh(7, 64)
        vt, tt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        W = RR.restirbvhWorker(vt, tt); W.update_mesh(W.vrt, W.v_ind)
        params, w0, w1, w2 = S.make_matnet_params(seed=0); mn, mx = S.material_min_max()
        mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()))
        with torch.no_grad():
            mlp.encoder.params.copy_(torch.from_numpy(params).cuda())
            for i, w in zip((0, 2, 4), (w0, w1, w2)):
                mlp.net.net[i].weight.copy_(torch.from_numpy(w).cuda())
        H = a.res
        mods = RR.load_m_for_restir(H, H)
        env = torch.full((256, 512, 3), 0.5, device="cuda", requires_grad=True)
        voff = torch.zeros_like(vt).requires_grad_(True)
        field = stage0.RadianceField.init_random(1.0, seed=0)
        pose = torch.from_numpy(orbit_pose(30.0, 30.0)).cuda()
        focal = 0.5 * H / np.tan(0.5 * 0.6911); intr = (focal, focal, H * 0.5, H * 0.5)
        topo = raster.antialias_topology(tt)
        gt = torch.rand((H * H, 3), device="cuda") * 0.5 + 0.25; gt_lin = harness.srgb_to_linear(gt)
        o_geo = torch.optim.Adam([{"params": [voff], "lr": 1e-4}, {"params": field.parameters(), "lr": 1e-2}], eps=1e-15)
        o_mat = torch.optim.Adam(mlp.parameters(), lr=0.03); o_lgt = torch.optim.Adam([env], lr=0.09)
        opt = types.SimpleNamespace(use_brdf=True)

        def step(with_field, pos_grad=False):
            for o in (o_geo, o_mat, o_lgt):
                o.zero_grad(set_to_none=True)
            kw = dict(field=field, offset_nerf_grad=pos_grad) if with_field else {}
            out = harness.render_stage1_outputs(W, vt, voff, tt, mlp, env, mods, H, H, a.spp, 1, pose=pose, intrinsics=intr, topology=topo, **kw)
            loss = losses.stage1_loss(out, gt, gt_lin, opt, vertices=vt, voffsets=voff, triangles=tt)
            losses.stage1_optimizer_step(loss, o_geo, o_mat, o_lgt, light_base=env, encoder_params=mlp.encoder.params)
        cases = {"step_without_field_ms": lambda: step(False), "step_with_field_ms": lambda: step(True), "step_with_field_and_pos_grad_ms": lambda: step(True, True)}
        res["step"] = dict(alternating(cases, a.reps, 1), res=H, spp=a.spp, covered_pixels=int((harness.build_gbuffer_from_pose(W, pose, intr, H, H)["occ"] > 0.5).sum()))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
