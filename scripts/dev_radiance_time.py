"""Times stage0.RadianceField (csrc/radiance.hip) and stage0.render_stage0 on the synthetic radiance checkpoint, and on a seeded random network of the same layout:
  forward    sigma and rgb of 2^20 points drawn inside the synthetic ball (radius 0.6), unit directions;
  rgb        the same with rgb_out only (NeRFNetwork.rgb);
  density    DensityField.density on the same points: the encoder and the 2112 FMAs of the density head, the share the colour path adds nothing to;
  encode     DensityField.encode: the gathers alone (plus 128 bytes of features written per point);
  torch      the same network as plain torch operations on the kernel's own encoder output (field.encode -> F.linear stack, field.sh for the directions);
  frame      one 800 x 800 render_stage0 frame from distance 3 (grid 128^3, updated once), whole, and split into march / network / composite by device events
             around each call of the loop, as dev_raymarch_time.infer_loop's clock does.
The point queries are timed in windows of --inner back-to-back launches between two device events, the queries taking turns within each of --reps rounds, one warm-up
each; the median (and min, max) per launch.  The frame: device events around the calls, one warm-up.  A record for DESIGN.md section 5.14, not a gate: no thresholds.

    python scripts/dev_radiance_time.py [--reps 7] [--inner 150] [--points 1048576] [--frame 800] [--skip_frame] [--out file.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FMA_DENSITY = 64 * 32 + 64                                        # per point: sigma_net.0 and row 0 of sigma_net.1
FMA_FORWARD = 64 * 32 + 16 * 64 + 64 * 31 + 64 * 64 + 3 * 64      # per point: all five layers


def torch_forward(field, x, d):
    """NeRFNetwork.forward by torch operations, fp32, from the kernels' encoder outputs."""
    import torch
    import torch.nn.functional as F
    h = F.linear(torch.relu(F.linear(field.encode(x), field.w0)), field.w1_full)
    sigma = torch.exp(h[:, 0])
    c = torch.cat([field.sh(d), h[:, 1:]], dim=-1)
    c = F.linear(torch.relu(F.linear(torch.relu(F.linear(c, field.c0)), field.c1)), field.c2)
    return sigma, torch.sigmoid(c)


def frame_loop(stage0, RM, field, G, o, d, clock, max_steps=1024, T_thresh=1e-4):
    """render_stage0's loop with a clock around each operator."""
    import torch
    N = o.shape[0]
    nears, fars = RM.near_far_from_aabb(o, d, G.aabb_train, G.min_near)
    ws = torch.zeros(N, device=o.device); dp = torch.zeros(N, device=o.device); im = torch.zeros(N, 3, device=o.device)
    alive = torch.arange(N, dtype=torch.int32, device=o.device); rays_t = nears.clone()
    step = rounds = points = 0
    while step < max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts = clock("march", lambda: RM.march_rays(n_alive, n_step, alive, rays_t, o, d, G.bound, False, G.density_bitfield, G.cascade, G.grid_size, nears, fars,
                                                                False, 0, max_steps))
        sig, rgb = clock("network", lambda: field.forward(xyzs, stage0._safe_normalize(dirs)))
        clock("composite", lambda: RM.composite_rays(n_alive, n_step, alive, rays_t, sig, rgb, ts, ws, dp, im, T_thresh, False))
        alive = alive[alive >= 0]
        step += n_step; rounds += 1; points += n_alive * n_step
    return ws, rounds, points


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def alternating(fns, reps, inner):
    """Per-launch time of each entry of `fns`: one warm-up each, then `reps` rounds that visit the entries in turn, each visit one window of `inner` back-to-back
    launches between two device events (a window of a tenth of a second at the default), so that drift of the clock or of the neighbours on the machine falls on all
    entries alike -> {name: (median, min, max)} in ms per launch."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                fn()
            e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=7); p.add_argument("--points", type=int, default=1 << 20); p.add_argument("--frame", type=int, default=800)
    p.add_argument("--inner", type=int, default=150, help="launches per timed window of the point queries")
    p.add_argument("--skip_frame", action="store_true", help="the point queries only (for a run under a kernel tracer)")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import torch
    from mirres_restir_nerf_mesh_amd import stage0, raymarching as RM
    from dev_raymarch_time import camera_rays
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    n = a.points
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    v = torch.randn((n, 3), generator=g, device="cuda")
    x = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()      # uniform in the ball
    d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    H = 128
    ck = stage0.synthetic_radiance_checkpoint(S=H)
    syn = stage0.RadianceField.from_checkpoint(ck, bound=1.0)
    net, total = stage0.density_layout(1.0)
    rnd = stage0.RadianceField(torch.randn((total, 2), generator=g, device="cuda"), *(torch.randn(s, generator=g, device="cuda") * 0.15
                               for s in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))), bound=1.0)
    res = {"points": n, "reps": a.reps, "inner": a.inner, "fma_per_point": {"density": FMA_DENSITY, "forward": FMA_FORWARD}, "gathers_per_point": 128}
    for name, f in (("synthetic", syn), ("random", rnd)):
        queries = {"forward_ms": lambda: f.forward(x, d), "rgb_ms": lambda: f.rgb(x, d), "density_ms": lambda: f.density(x), "encode_ms": lambda: f.encode(x),
                   "sh_ms": lambda: f.sh(d)}
        r = alternating(queries, a.reps, a.inner)
        r["torch_ms"] = timed(lambda: torch_forward(f, x, d), a.reps)
        s_k, c_k = f.forward(x, d); s_t, c_t = torch_forward(f, x, d)
        r["max_rel_sigma_diff_to_torch"] = float(((s_k - s_t).abs() / s_t).max()); r["max_rgb_diff_to_torch"] = float((c_k - c_t).abs().max())
        fw, dn = r["forward_ms"][0], r["density_ms"][0]
        r["forward_Mpoints_per_s"] = n / fw / 1e3
        r["forward_fma_TFLOPs"] = n * 2 * FMA_FORWARD / (fw * 1e-3) / 1e12
        # two points on a line time = gathers + FMAs * cost: the head's cost per FMA from the difference, the rest of the density query is the encoder
        per_fma = (fw - dn) / (FMA_FORWARD - FMA_DENSITY)
        r["head_ms_estimate"] = per_fma * FMA_FORWARD; r["encoder_ms_estimate"] = fw - per_fma * FMA_FORWARD
        res[name] = r
        print(json.dumps({name: r}), flush=True)
    if a.skip_frame:
        print(json.dumps(res), flush=True)
        return
    # ---- one inference frame of the synthetic checkpoint
    G = stage0.DensityGrid.from_checkpoint(ck, bound=1.0)
    G.update(syn)
    o, dd = camera_rays(a.frame)
    acc = {}

    def clock(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        acc.setdefault(name, []).append((e0, e1))
        return out
    whole = timed(lambda: stage0.render_stage0(syn, G, o, dd), max(1, min(a.reps, 3)))
    frame_loop(stage0, RM, syn, G, o, dd, lambda name, fn: fn())                                # warm-up of the loop below
    ws, rounds, points = frame_loop(stage0, RM, syn, G, o, dd, clock)
    torch.cuda.synchronize()
    fr = {"rays": a.frame ** 2, "frame_ms": whole, "rounds": rounds, "points": points, "opaque_rays": int((ws > 0.99).sum())}
    for name, evs in acc.items():
        fr[name + "_ms_total"] = sum(e0.elapsed_time(e1) for e0, e1 in evs)
    res["frame"] = fr
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
