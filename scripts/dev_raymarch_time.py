"""Times the stage-0 ray-marching operators (csrc/raymarch.hip; mirres_restir_nerf_mesh_amd.raymarching, stage0.DensityGrid) on the synthetic checkpoint, after an
end-to-end check of the whole chain as a smoke run:
  train      the reference's training shape: 4096 rays at max_steps 1024 on an H = 128 grid — near_far_from_aabb, march_rays_train (its three launches and the
             read-back of M), the density query, composite_rays_train forward and backward;
  infer      an 800 x 800 inference frame: the loop of nerf/renderer.py:784-828 (march_rays, density, composite_rays), per operator and as a whole;
  update     DensityGrid.update at H = 128 with 1 and 2 cascades.
Device events around the calls, one warm-up, the median of --reps runs.  A record for DESIGN.md section 5.13, not a gate: there is no earlier path to compare with.
The end-to-end check imports tests/raymarch_refs.py (the derived float32 bound of compositing and the Morton inverse live with the numpy restatement): a development
tool reaching into the tests, not something the package does.

    python scripts/dev_raymarch_time.py [--reps 5] [--frame 800] [--skip_check] [--out file.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)


def camera_rays(W, dist=3.0, tan_half=0.6, device="cuda"):
    """A W x W pinhole image from (0, 0, dist) looking at the origin -> rays_o, rays_d [W * W, 3] (unit directions)."""
    import torch
    ax = ((torch.arange(W, dtype=torch.float32, device=device) + 0.5) / W * 2 - 1) * tan_half
    y, x = torch.meshgrid(ax, ax, indexing="ij")
    d = torch.stack([x, -y, -torch.ones_like(x)], -1).reshape(-1, 3)
    d = d / d.norm(dim=1, keepdim=True)
    o = torch.tensor([0.0, 0.0, dist], device=device).expand_as(d).contiguous()
    return o, d.contiguous()


def infer_loop(RM, G, sigma_fn, o, d, nears, fars, max_steps=1024, T_thresh=1e-2, clock=None):
    """nerf/renderer.py:784-828 with white colours -> weights_sum, depth, image and the samples every ray was given, in order (for comparisons)."""
    import torch
    N = o.shape[0]
    ws = torch.zeros(N, device=o.device); dp = torch.zeros(N, device=o.device); im = torch.zeros(N, 3, device=o.device)
    rays_alive = torch.arange(N, dtype=torch.int32, device=o.device); rays_t = nears.clone()
    taken = torch.zeros(N, dtype=torch.int64, device=o.device)
    step = 0
    tick = clock if clock is not None else (lambda name, fn: fn())
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts = tick("march_rays", lambda: RM.march_rays(n_alive, n_step, rays_alive, rays_t, o, d, G.bound, False, G.density_bitfield, G.cascade, G.grid_size,
                                                                    nears, fars, False, 0, max_steps))
        sig = tick("density", lambda: sigma_fn(xyzs))
        taken.index_add_(0, rays_alive.long(), (ts.view(n_alive, n_step, 2)[:, :, 0] != 0).sum(1))
        tick("composite_rays", lambda: RM.composite_rays(n_alive, n_step, rays_alive, rays_t, sig, torch.ones_like(xyzs), ts, ws, dp, im, T_thresh, False))
        rays_alive = rays_alive[rays_alive >= 0]
        step += n_step
    return ws, dp, im, taken


def end_to_end_check(W=32, updates=3):
    """synthetic_checkpoint(S = 16) -> DensityGrid, updated a few times -> a W x W image from distance 3: near_far_from_aabb, march_rays_train, the density network at
    the samples, composite_rays_train with white colours, its backward, and the inference loop on the same rays.  Raises AssertionError; returns the figures."""
    import numpy as np
    import torch
    from mirres_restir_nerf_mesh_amd import stage0, raymarching as RM
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raymarch_refs as R                                                     # the derived float32 bound of compositing lives with the restatement
    H = 16
    ck = stage0.synthetic_checkpoint(S=H)
    field = stage0.DensityField.from_checkpoint(ck, bound=1.0)
    G = stage0.DensityGrid.from_checkpoint(ck, bound=1.0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for _ in range(updates):
        G.update(field, noise=torch.rand(1, H ** 3, 3, generator=gen, device="cuda"))
    assert G.iter_density == updates and 0 < G.mean_density < 30
    occ = (G.density_grid[0] > min(G.mean_density, G.density_thresh)).cpu().numpy()
    assert np.array_equal(np.packbits(occ, bitorder="little"), G.density_bitfield.cpu().numpy()) and 0 < occ.sum() < H ** 3
    centres = (R.morton3D_invert(np.arange(H ** 3, dtype=np.int32)) + 0.5) / H * 2.0 - 1.0
    radius = float(np.linalg.norm(centres[occ], axis=1).max()) + 2.0 * np.sqrt(3.0) / H       # the occupied radius read from the bitfield, plus one cell diagonal
    o, d = camera_rays(W)
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    nears, fars = RM.near_far_from_aabb(o, d, aabb, 0.2)
    xyzs, dirs, ts, rays = RM.march_rays_train(o, d, 1.0, False, G.density_bitfield, 1, H, nears, fars, False, 0, 1024)
    sigmas = field.density(xyzs).requires_grad_(True)
    weights, ws, depth, image = RM.composite_rays_train(sigmas, torch.ones_like(xyzs), ts, rays, 1e-4, False)
    tca = -(o * d).sum(1)
    dist = (o + tca[:, None] * d).norm(dim=1)                                                 # the ray's distance from the origin
    centre = dist < 0.1
    assert centre.sum() >= 1 and (ws[centre] > 0.99).all(), ws[centre]
    outside = dist > radius
    assert outside.sum() >= W and (rays[outside, 1] == 0).all() and (ws[outside] == 0).all()
    opaque = ws > 0.99
    entry = tca - torch.sqrt(torch.clamp(radius ** 2 - dist ** 2, min=0))
    mean_depth = depth / ws
    assert opaque.sum() >= W and (mean_depth[opaque] >= entry[opaque]).all() and (mean_depth[opaque] <= 3.0).all()
    image.sum().backward()
    g = sigmas.grad
    assert torch.isfinite(g).all() and (g != 0).any()
    # the inference loop: the same opacity mask at its own T_thresh ...
    iws, idp, iim, taken = infer_loop(RM, G, field.density, o, d, nears, fars)
    assert torch.equal(iws > 0.99, opaque) and torch.equal(iws == 0, ws == 0)
    # ... and, with no early termination on either side, the same depth where both marchers emit the same samples, within the float32 bound of compositing
    # (raymarch_refs.composite_error_bound, derived there)
    _, ws0, dp0, _ = RM.composite_rays_train(sigmas.detach(), torch.ones_like(xyzs), ts, rays, 0.0, False)
    iws0, idp0, _, taken0 = infer_loop(RM, G, field.density, o, d, nears, fars, T_thresh=0.0)
    same_samples = (taken0 == rays[:, 1].long()).cpu().numpy()
    bound = R.composite_error_bound(sigmas.detach().cpu().numpy(), ts.cpu().numpy(), rays.cpu().numpy(), False, ts[:, 0].cpu().numpy())
    err = (idp0 - dp0).abs().cpu().numpy().astype(np.float64)
    hit = same_samples & (rays[:, 1] > 0).cpu().numpy()
    assert hit.sum() >= W and (err[hit] <= bound[hit]).all(), (err[hit].max(), bound[hit].min())
    return {"rays": W * W, "points": int(xyzs.shape[0]), "occupied_cells": int(occ.sum()), "occupied_radius": radius, "opaque_rays": int(opaque.sum()),
            "empty_rays": int((ws == 0).sum()), "same_sample_rays": int(hit.sum()), "max_depth_diff": float(err[hit].max()), "bound_there": float(bound[hit][err[hit].argmax()]),
            "mean_density": G.mean_density}


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


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5); p.add_argument("--frame", type=int, default=800); p.add_argument("--skip_check", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import torch
    from mirres_restir_nerf_mesh_amd import stage0, raymarching as RM
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    res = {"reps": a.reps}
    if not a.skip_check:
        res["check"] = end_to_end_check()
        print(json.dumps({"check": res["check"]}), flush=True)
    H = 128
    ck = stage0.synthetic_checkpoint(S=H)
    field = stage0.DensityField.from_checkpoint(ck, bound=1.0)
    G = stage0.DensityGrid.from_checkpoint(ck, bound=1.0)
    G.update(field)
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device="cuda")
    # ---- the training shape
    o, d = camera_rays(64)
    N = o.shape[0]
    tr = {"rays": N, "max_steps": 1024, "H": H}
    tr["near_far_ms"] = timed(lambda: RM.near_far_from_aabb(o, d, aabb, 0.2), a.reps)
    nears, fars = RM.near_far_from_aabb(o, d, aabb, 0.2)
    march = lambda: RM.march_rays_train(o, d, 1.0, False, G.density_bitfield, 1, H, nears, fars, True, 0, 1024)
    tr["march_rays_train_ms"] = timed(march, a.reps)
    xyzs, dirs, ts, rays = march()
    M = int(xyzs.shape[0]); tr["points"] = M
    tr["density_ms"] = timed(lambda: field.density(xyzs), a.reps)
    sig = field.density(xyzs).requires_grad_(True); rgb = torch.rand(M, 3, device="cuda").requires_grad_(True)
    tr["composite_train_fwd_ms"] = timed(lambda: RM.composite_rays_train(sig.detach(), rgb.detach(), ts, rays, 1e-4, False), a.reps)
    outs = RM.composite_rays_train(sig, rgb, ts, rays, 1e-4, False)
    cot = [torch.rand_like(x) for x in outs]
    tr["composite_train_bwd_ms"] = timed(lambda: torch.autograd.grad(outs, [sig, rgb], cot, retain_graph=True), a.reps)
    used = int((outs[0] != 0).sum())                                                        # samples before the early stops: what the kernels actually touch
    tr["points_used"] = used
    tr["composite_train_fwd_GBps"] = (used * (4 + 12 + 8 + 4) + N * (8 + 20)) / (tr["composite_train_fwd_ms"][0] * 1e-3) / 1e9
    tr["composite_train_bwd_GBps"] = (used * (4 + 12 + 8 + 4 + 4 + 12) + N * (8 + 40)) / (tr["composite_train_bwd_ms"][0] * 1e-3) / 1e9
    res["train"] = tr
    # ---- an inference frame
    o, d = camera_rays(a.frame)
    nears, fars = RM.near_far_from_aabb(o, d, aabb, 0.2)
    acc = {}

    def clock(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        acc.setdefault(name, []).append((e0, e1))
        return out
    infer_loop(RM, G, field.density, o, d, nears, fars)                                       # warm-up
    whole = timed(lambda: infer_loop(RM, G, field.density, o, d, nears, fars), max(1, min(a.reps, 3)))
    acc.clear()
    ws = infer_loop(RM, G, field.density, o, d, nears, fars, clock=clock)[0]
    torch.cuda.synchronize()
    inf = {"rays": a.frame ** 2, "frame_ms": whole, "rounds": len(acc["march_rays"]), "opaque_rays": int((ws > 0.99).sum())}
    for name, evs in acc.items():
        inf[name + "_ms_total"] = sum(e0.elapsed_time(e1) for e0, e1 in evs)
    res["infer"] = inf
    # ---- the grid's upkeep
    up = {}
    for cas, bound in ((1, 1.0), (2, 2.0)):
        Gc = stage0.DensityGrid(bound=bound, grid_size=H)
        noise = torch.rand(cas, H ** 3, 3, device="cuda")
        up["update_%d_cascade_ms" % cas] = timed(lambda: Gc.update(field, noise=noise), a.reps)
    res["update"] = up
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
