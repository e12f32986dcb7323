"""Times the hash grid's total-variation regulariser (csrc/grid_tv.hip, stage0.DensityField.grad_total_variation) with the method of dev_radiance_time.py: windows
of --inner back-to-back launches between two device events, the cases taking turns within each of --reps rounds, one warm-up each.
  regulariser  2^18 and 2^20 points at T = 19 (levels 0-4 dense), seeded random table: uniform in the ball of radius 0.6, and all inside ONE cell of level 0 (the
               coarse levels' worst contention); mirres_radiance_points_bwd on the same points in the same session beside it, whose one-cell case is four times
               its uniform case.  The figure to read is that ratio for the regulariser.
  step         one training step of 4096 rays on the synthetic radiance checkpoint's density (scripts/train_stage0.py's step) without and with --lambda_tv.
A record for DESIGN.md section 5.16, not a gate: no thresholds.

    python scripts/dev_grid_tv_time.py [--reps 5] [--inner 20] [--out profiles/grid_tv_time.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_radiance_time import alternating  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5); p.add_argument("--inner", type=int, default=20); p.add_argument("--rays", type=int, default=4096)
    p.add_argument("--lambda_tv", type=float, default=1e-8); p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, harness
    from render_stage0 import orbit_poses
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    net, total = stage0.density_layout(1.0)
    rnd = stage0.RadianceField(torch.randn((total, 2), generator=g, device="cuda"), *(torch.randn(s, generator=g, device="cuda") * 0.15
                               for s in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))), bound=1.0)
    res = {"reps": a.reps, "inner": a.inner, "log2_hashmap_size": 19, "dense_levels": [l for l in range(net.num_levels) if not net.hashed[l]]}
    tgrad = torch.zeros_like(rnd.table)
    for n in (1 << 18, 1 << 20):
        v = torch.randn((n, 3), generator=g, device="cuda")
        ball = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()
        s0 = float(net.scale[0])
        cell = ((torch.tensor([7.0, 5.0, 8.0], device="cuda") + 0.05 + 0.9 * torch.rand((n, 3), generator=g, device="cuda") - 0.5) / s0 * 2 - 1).contiguous()
        d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        gs = torch.randn(n, generator=g, device="cuda"); grgb = torch.randn((n, 3), generator=g, device="cuda")
        grads = [torch.zeros_like(getattr(rnd, k)) for k in rnd.PARAMETER_NAMES]
        cases = {"tv_ball_ms": lambda: rnd.grad_total_variation(a.lambda_tv, ball, grad=tgrad), "tv_one_cell_ms": lambda: rnd.grad_total_variation(a.lambda_tv, cell, grad=tgrad),
                 "backward_ball_ms": lambda: rnd.backward_points(ball, d, gs, grgb, grads=grads), "backward_one_cell_ms": lambda: rnd.backward_points(cell, d, gs, grgb, grads=grads)}
        r = alternating(cases, a.reps, a.inner)
        r["tv_one_cell_over_ball"] = r["tv_one_cell_ms"][0] / r["tv_ball_ms"][0]
        r["backward_one_cell_over_ball"] = r["backward_one_cell_ms"][0] / r["backward_ball_ms"][0]
        res["points_%d" % n] = r
        print(json.dumps({n: r}), flush=True)
    # ---- one training step, without and with the regulariser
    ck = stage0.synthetic_radiance_checkpoint(S=128)
    m = ck["model"]
    init = stage0.RadianceField.init_random(1.0, seed=4)
    field = stage0.RadianceField(m["encoder.embeddings"], m["sigma_net.0.weight"], m["sigma_net.1.weight"], init.c0, init.c1, init.c2, bound=1.0)
    G = stage0.DensityGrid.from_checkpoint(ck, bound=1.0)
    G.update(field)
    size = 64
    o, dd = harness.get_rays(torch.from_numpy(np.asarray(orbit_poses(1)[0], np.float32)).cuda(), (0.5 * size / 0.45,) * 2 + (size * 0.5,) * 2, size, size)
    pix = torch.randint(size * size, (a.rays,), generator=g, device="cuda")
    o, dd = o[pix].contiguous(), dd[pix].contiguous()
    target = torch.rand((a.rays, 3), generator=g, device="cuda"); noises = torch.rand(a.rays, generator=g, device="cuda")
    params = field.parameters()
    opt = torch.optim.Adam(params, lr=1e-2, eps=1e-15)
    tv_events = []

    def step(lambda_tv, clock=False):
        out = stage0.render_stage0_train(field, G, o, dd, bg_color=1.0, perturb=True, noises=noises)
        loss = ((out["image"] - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if lambda_tv > 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); field.grad_total_variation(lambda_tv, out["xyzs"]); e1.record()
            if clock:
                tv_events.append((e0, e1))
        opt.step()
        return out["num_points"]
    st = {"rays": a.rays}
    for name, lam in (("step_ms", 0.0), ("step_lambda_tv_ms", a.lambda_tv)):
        for _ in range(3):
            step(lam)
        torch.cuda.synchronize()
        whole = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); st["samples"] = step(lam, True); e1.record(); torch.cuda.synchronize()
            whole.append(e0.elapsed_time(e1))
        st[name] = (sorted(whole)[len(whole) // 2], min(whole), max(whole))
    t = sorted(e0.elapsed_time(e1) for e0, e1 in tv_events)
    st["grad_total_variation_ms"] = (t[len(t) // 2], t[0], t[-1])
    res["step"] = st
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
