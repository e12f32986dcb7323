"""Times the adjoint of the stage-0 radiance network (csrc/radiance_bwd.hip, stage0.RadianceField.backward_points) and one whole training step, with the method of
dev_radiance_time.py: windows of --inner back-to-back launches between two device events, the cases taking turns within each of --reps rounds, one warm-up each.
  backward   2^18 and 2^20 points, seeded random table and weights: uniform in the ball of radius 0.6, and all inside ONE cell of level 0 (every point meets the same
             eight entries of the coarse levels: the scatter's worst contention); the forward on the same points beside it; and the backward of points that are all out
             of bounds, which gather and scatter nothing: the recomputed forward, its adjoint and the five weight GEMMs alone;
  step       one training step of 4096 rays on the synthetic radiance checkpoint's density with init_random colour weights (scripts/train_stage0.py's step), whole,
             and split by device events into march / forward / composite / backward (composite's and the network's) / Adam.
A record for DESIGN.md section 5.15, not a gate: no thresholds.

    python scripts/dev_radiance_bwd_time.py [--reps 5] [--inner 20] [--out profiles/radiance_bwd_time.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_radiance_time import alternating  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5); p.add_argument("--inner", type=int, default=20); p.add_argument("--rays", type=int, default=4096)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, harness, raymarching as RM
    from render_stage0 import orbit_poses
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    net, total = stage0.density_layout(1.0)
    rnd = stage0.RadianceField(torch.randn((total, 2), generator=g, device="cuda"), *(torch.randn(s, generator=g, device="cuda") * 0.15
                               for s in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))), bound=1.0)
    res = {"reps": a.reps, "inner": a.inner, "pair_requests_per_point": 128}
    for n in (1 << 18, 1 << 20):
        v = torch.randn((n, 3), generator=g, device="cuda")
        ball = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()
        s0 = float(net.scale[0])
        cell = ((torch.tensor([7.0, 5.0, 8.0], device="cuda") + 0.05 + 0.9 * torch.rand((n, 3), generator=g, device="cuda") - 0.5) / s0 * 2 - 1).contiguous()
        outside = (ball + 2.0).contiguous()                                         # no gather and no scatter: the two networks and the five GEMMs alone
        d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        gs = torch.randn(n, generator=g, device="cuda"); grgb = torch.randn((n, 3), generator=g, device="cuda")
        grads = [torch.zeros_like(getattr(rnd, k)) for k in rnd.PARAMETER_NAMES]
        cases = {"forward_ball_ms": lambda: rnd.forward(ball, d), "backward_ball_ms": lambda: rnd.backward_points(ball, d, gs, grgb, grads=grads),
                 "forward_one_cell_ms": lambda: rnd.forward(cell, d), "backward_one_cell_ms": lambda: rnd.backward_points(cell, d, gs, grgb, grads=grads),
                 "backward_out_of_bounds_ms": lambda: rnd.backward_points(outside, d, gs, grgb, grads=grads)}
        r = alternating(cases, a.reps, a.inner)
        r["backward_ball_Mpoints_per_s"] = n / r["backward_ball_ms"][0] / 1e3
        r["backward_ball_pair_requests_per_s"] = n * 128 / (r["backward_ball_ms"][0] * 1e-3)
        res["points_%d" % n] = r
        print(json.dumps({n: r}), flush=True)
    # ---- one training step
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
    acc = {}

    def clock(name, fn, on=True):
        if not on:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        acc.setdefault(name, []).append((e0, e1))
        return out

    def step(on):
        nears, fars = RM.near_far_from_aabb(o, dd, G.aabb_train, G.min_near)
        xyzs, dirs, ts, rays = clock("march", lambda: RM.march_rays_train(o, dd, G.bound, False, G.density_bitfield, G.cascade, G.grid_size, nears, fars, True, 0, 1024, noises), on)
        sig, rgb = clock("forward", lambda: field.forward_train(xyzs, stage0._safe_normalize(dirs)), on)
        _, ws, _, img = clock("composite", lambda: RM.composite_rays_train(sig, rgb, ts, rays, 1e-4, False), on)
        loss = (((img + (1 - ws).unsqueeze(-1)) - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        clock("backward", loss.backward, on)
        clock("adam", opt.step, on)
        return int(xyzs.shape[0])
    for _ in range(3):
        step(False)
    torch.cuda.synchronize()
    whole = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(False); e1.record(); torch.cuda.synchronize()
        whole.append(e0.elapsed_time(e1))
    samples = [step(True) for _ in range(a.reps)]
    torch.cuda.synchronize()
    st = {"rays": a.rays, "samples": samples[-1], "step_ms": (sorted(whole)[len(whole) // 2], min(whole), max(whole))}
    for name, evs in acc.items():
        t = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
        st[name + "_ms"] = t[len(t) // 2]
    res["step"] = st
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
