"""Stage-0 training on the HIP path: Trainer.train of the reference for stage 0 (main.py:50-82, 231-287; nerf/utils.py:912-978, 1544-1575) over
stage0.render_stage0_train — the hash-grid radiance network (csrc/radiance.hip and its adjoint csrc/radiance_bwd.hip), the ray-marching operators and the density
grid's upkeep — from a NeRF-blender folder to `<workspace>/checkpoints/ngp.pth`, which scripts/render_stage0.py and scripts/export_stage0.py read.

    python scripts/train_stage0.py --path data/lego --workspace out/lego --bound 1 --scale 0.8 --mark_untrained --eval_views 4
    python scripts/train_stage0.py --synthetic --iters 300
    python scripts/train_stage0.py --path data/lego --workspace out/lego -O --bound 1 --scale 0.8 --lambda_tv 1e-8        # the reference's stage-0 recipe, in fp32

The reference's settings: Adam (lr 1e-2, eps 1e-15), the LambdaLR warm-up and decay of main.py:285 stepped every iteration, 7500 iterations of 4096 uniformly random
pixels of one training image each, white or random background with gt = rgb * a + bg * (1 - a), loss = lambda_rgb * MSE(rgb).mean(-1) + lambda_mask * MSE(weights_sum,
a) when the images have alpha, perturbed sampling, DensityGrid.update every --update_extra_interval steps before the step, an exponential moving average of the
parameters (decay 0.95) whose weights are what the checkpoint's `model` holds.

Built, and off unless asked for: --lambda_tv X, the in-place total-variation regulariser of the hash grid on the step's own sample points after loss.backward()
(nerf/utils.py:1152-1158, RadianceField.grad_total_variation; with --bound > 1 the points outside the unit box take 10 X); --adaptive_num_rays, which rescales the
ray count after every step so that a step marches about --num_points samples (utils.py:1133-1134, adapt_num_rays); --random_image_batch, which keeps every training
view on the device and draws each ray's image and pixel independently (harness.get_rays_at); -O, the reference's bundle as far as it is built: --mark_untrained
--random_image_batch --adaptive_num_rays.  Deviations: --lambda_tv defaults to 0 where the reference has 1e-8, so a run without new
options computes what it did before them; the ray count stays as it is after a step without samples and is clamped to [1, --max_num_rays].

Declared and NOT built: fp16 autocast and GradScaler (fp32 throughout, also under -O); --sdf, individual_codes, depth supervision,
--trainable_density_grid, error_map sampling and data-parallel training; the reference's partial grid updates after step 16 (every update here covers the whole
grid).

--synthetic needs no data: it renders ground-truth views of stage0.synthetic_radiance_checkpoint() at a small size from render_stage0.orbit_poses, trains a
RadianceField.init_random on them and prints the first-window and last-window loss and the held-out PSNR."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from render_stage0 import orbit_poses  # noqa: E402

WARMUP = 500                                                                      # main.py:285
EMA_DECAY = 0.95                                                                  # main.py:287, stage 0


def lr_factor(it, iters):
    """main.py:285: 0.01 + 0.99 * (it / 500) up to iteration 500, then 0.1 ** ((it - 500) / (iters - 500))."""
    return 0.01 + 0.99 * (it / WARMUP) if it <= WARMUP else 0.1 ** ((it - WARMUP) / (iters - WARMUP))


class EMA:
    """torch_ema.ExponentialMovingAverage's arithmetic on a list of tensors: with num_updates counted from 1, decay_t = min(decay, (1 + t) / (10 + t)) and
    shadow -= (1 - decay_t) * (shadow - param).  state_dict() has torch_ema's keys."""

    def __init__(self, params, decay=EMA_DECAY):
        self.decay, self.num_updates = float(decay), 0
        self.shadow = [p.detach().clone() for p in params]

    def update(self, params):
        import torch
        self.num_updates += 1
        d = min(self.decay, (1 + self.num_updates) / (10 + self.num_updates))
        with torch.no_grad():
            for s, p in zip(self.shadow, params):
                s.sub_((1.0 - d) * (s - p.detach()))

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow}


def adapt_num_rays(num_rays, num_points, target, max_num_rays):
    """nerf/utils.py:1133-1134: int(round(target / num_points * num_rays)) (Python's round: halves to even), clamped to [1, max_num_rays]; a step without
    samples (where the reference divides by zero) keeps the count it had."""
    if num_points <= 0:
        return int(num_rays)
    return max(1, min(int(max_num_rays), int(round(target / num_points * num_rays))))


def build_parser():
    p = argparse.ArgumentParser(description="Train a stage-0 radiance field on the HIP path (fp32; built and off by default: --lambda_tv, --adaptive_num_rays, "
                                            "--random_image_batch, bundled by -O; see the module docstring for what the reference has and this does not: "
                                            "fp16 autocast / GradScaler, --sdf, individual_codes, depth supervision, "
                                            "--trainable_density_grid, error_map sampling, data-parallel training)")
    p.add_argument("--path", default=None, help="a NeRF-blender folder: transforms_train.json (and transforms_test.json for --eval_views) with its images")
    p.add_argument("--workspace", default=None)
    p.add_argument("--synthetic", action="store_true"); p.add_argument("--views", type=int, default=12, help="--synthetic: the number of training views")
    p.add_argument("--iters", type=int, default=7500); p.add_argument("--num_rays", type=int, default=4096); p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--background", choices=["white", "random"], default="white")
    p.add_argument("--lambda_rgb", type=float, default=1.0); p.add_argument("--lambda_mask", type=float, default=0.1)
    p.add_argument("--update_extra_interval", type=int, default=16); p.add_argument("--mark_untrained", action="store_true")
    p.add_argument("--save_interval", type=int, default=0, help="also write the checkpoint every this many iterations (0: only at the end)")
    p.add_argument("--resume", action="store_true", help="continue from <workspace>/checkpoints/ngp.pth, optimiser state included")
    p.add_argument("--eval_views", type=int, default=0, help="render this many held-out views with render_stage0 at the end and print their PSNR")
    p.add_argument("--bound", type=float, default=1.0); p.add_argument("--scale", type=float, default=1.0); p.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    p.add_argument("--downscale", type=int, default=1); p.add_argument("--grid_size", type=int, default=128)
    p.add_argument("--max_steps", type=int, default=1024); p.add_argument("--T_thresh", type=float, default=1e-4); p.add_argument("--dt_gamma", type=float, default=0.0)
    p.add_argument("--min_near", type=float, default=0.2); p.add_argument("--density_thresh", type=float, default=10.0)
    p.add_argument("--color_space", choices=["srgb", "linear"], default="srgb")
    p.add_argument("--seed", type=int, default=0); p.add_argument("--window", type=int, default=50, help="iterations per reported loss window")
    p.add_argument("--lambda_tv", type=float, default=0.0, help="weight of the hash grid's total-variation regulariser on each step's sample points (0: off; the "
                                                                "reference's default is 1e-8); with --bound > 1 the points outside the unit box take ten times it")
    p.add_argument("--adaptive_num_rays", action="store_true", help="after every step, rescale the ray count so that a step marches about --num_points samples")
    p.add_argument("--num_points", type=int, default=1 << 18, help="--adaptive_num_rays: the target number of samples per step (ignored without it)")
    p.add_argument("--max_num_rays", type=int, default=1 << 18, help="--adaptive_num_rays: the ray count never exceeds this")
    p.add_argument("--random_image_batch", action="store_true", help="keep all training views on the device and draw every ray's image and pixel independently")
    p.add_argument("-O", dest="O", action="store_true", help="the reference's -O as far as it is built: --mark_untrained --random_image_batch --adaptive_num_rays "
                                                             "(fp16 stays unbuilt)")
    return p


def parse_args(argv=None):
    """Validates what can be validated without a device."""
    p = build_parser()
    a = p.parse_args(argv)
    if a.O:
        a.mark_untrained = a.random_image_batch = a.adaptive_num_rays = True
    if not (a.lambda_tv >= 0) or a.lambda_tv == float("inf"):
        p.error("--lambda_tv %r: not negative and finite" % a.lambda_tv)
    if a.num_points < 1 or a.max_num_rays < 1:
        p.error("--num_points and --max_num_rays at least 1")
    if a.synthetic:
        if a.path:
            p.error("--synthetic brings its own views: drop --path")
        if a.bound != 1.0:
            p.error("--synthetic: the synthetic checkpoint's hash grid is laid out for --bound 1")
        if a.color_space != "srgb":
            p.error("--synthetic: the ground truth is rendered, not read: --color_space does not apply")
        if a.views < 2:
            p.error("--views %d: at least 2" % a.views)
    else:
        if not a.path or not a.workspace:
            p.error("--path and --workspace are required (or --synthetic)")
        if not os.path.exists(os.path.join(a.path, "transforms_train.json")):
            p.error("%s has no transforms_train.json" % a.path)
    if a.resume and not a.workspace:
        p.error("--resume needs the --workspace that holds checkpoints/ngp.pth")
    if a.resume and not os.path.exists(os.path.join(a.workspace, "checkpoints", "ngp.pth")):
        p.error("--resume: %s does not exist" % os.path.join(a.workspace, "checkpoints", "ngp.pth"))
    if a.iters < 1 or a.num_rays < 1 or a.update_extra_interval < 1 or a.save_interval < 0 or a.eval_views < 0 or a.window < 1:
        p.error("--iters, --num_rays and --update_extra_interval at least 1, --save_interval and --eval_views not negative")
    if not (a.bound > 0) or a.downscale < 1 or a.max_steps < 1 or not (0 <= a.T_thresh < 1) or not (a.dt_gamma >= 0) or not (a.min_near >= 0):
        p.error("--bound positive, --downscale and --max_steps at least 1, --T_thresh in [0, 1), --dt_gamma and --min_near not negative")
    if a.grid_size < 2 or a.grid_size > 1024 or a.grid_size & (a.grid_size - 1):
        p.error("--grid_size %d: a power of two in [2, 1024]" % a.grid_size)
    return a


def pixels_to_gt(px, color_space):
    """uint8 pixels [..., C] (C = 3 or 4) -> (premultiplied rgb f32 [..., 3], alpha f32 [...] or None): load_blender's conversion, applied to pixels that were
    gathered first.  Division by 255 and the product are IEEE on host and device alike, so an srgb pixel has load_blender's bits; --color_space linear goes
    through the device's pow."""
    import torch
    from mirres_restir_nerf_mesh_amd import harness
    px = px.to(torch.float32) / 255.0
    rgb = px[..., :3]
    if color_space == "linear":
        rgb = harness.srgb_to_linear(rgb)
    alpha = px[..., 3] if px.shape[-1] == 4 else None
    return (rgb * alpha[..., None] if alpha is not None else rgb), alpha


def load_blender(a, split, limit=None, u8=False):
    """-> (H, W, focal, [(pose f32 [4, 4], premultiplied rgb f32 [H * W, 3], alpha f32 [H * W] or None)]) of transforms_<split>.json, on the host.
    u8 (--random_image_batch): the views are (pose, the image's own uint8 pixels [H * W, C], None); pixels_to_gt converts what a step gathers."""
    import numpy as np
    from PIL import Image
    from evaluate import nerf_pose
    from mirres_restir_nerf_mesh_amd import harness
    import torch
    tf = json.load(open(os.path.join(a.path, "transforms_%s.json" % split)))
    frames = tf["frames"][:limit] if limit else tf["frames"]
    views, H, W = [], None, None
    for fr in frames:
        f = os.path.join(a.path, fr["file_path"]); f = f if os.path.exists(f) else f + ".png"
        img = Image.open(f)
        if H is None:
            H, W = img.height // a.downscale, img.width // a.downscale
        if (img.height, img.width) != (H, W):
            img = img.resize((W, H), Image.BILINEAR)
        if u8:
            raw = torch.from_numpy(np.array(img, dtype=np.uint8))
            views.append((nerf_pose(fr["transform_matrix"], a.scale, a.offset), raw.reshape(H * W, -1).contiguous(), None))
            continue
        px = torch.from_numpy(np.asarray(img).astype(np.float32) / 255.0)
        rgb = px[..., :3]
        if a.color_space == "linear":
            rgb = harness.srgb_to_linear(rgb)
        alpha = px[..., 3].reshape(-1).contiguous() if px.shape[-1] == 4 else None
        rgb = rgb.reshape(-1, 3)
        views.append((nerf_pose(fr["transform_matrix"], a.scale, a.offset), (rgb * alpha[:, None] if alpha is not None else rgb).contiguous(), alpha))
    import numpy as np
    return H, W, 0.5 * W / np.tan(0.5 * tf["camera_angle_x"]), views


def synthetic_views(a, n_train, n_eval, size=48):
    """Ground truth rendered from the synthetic checkpoint: n_train + n_eval orbit views of size x size -> (H, W, focal, train views, held-out views)."""
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, harness
    ck = stage0.synthetic_radiance_checkpoint(S=32)
    field = stage0.RadianceField.from_checkpoint(ck, bound=1.0)
    grid = stage0.DensityGrid.from_checkpoint(ck, bound=1.0, min_near=a.min_near, density_thresh=a.density_thresh)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for _ in range(3):                                                            # the synthetic checkpoint stores no bitfield: the grid's own upkeep makes one
        grid.update(field, noise=torch.rand(grid.cascade, grid.grid_size ** 3, 3, generator=gen, device="cuda"))
    focal = 0.5 * size / 0.45
    views = []
    for pose in orbit_poses(n_train + n_eval):
        o, d = harness.get_rays(torch.from_numpy(np.asarray(pose, np.float32)).cuda(), (focal, focal, size * 0.5, size * 0.5), size, size)
        out = stage0.render_stage0(field, grid, o, d, bg_color=0.0, max_steps=a.max_steps, T_thresh=a.T_thresh)
        views.append((np.asarray(pose, np.float32), out["image"].cpu(), out["weights_sum"].cpu()))
    held = views[::max(1, (n_train + n_eval) // max(n_eval, 1))][:n_eval] if n_eval else []
    train = [v for v in views if not any(v is h for h in held)]
    return size, size, focal, train, held


def main(argv=None):
    a = parse_args(argv)
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, harness, checkpoint as CK
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    log = lambda m: print(m, flush=True)
    if a.synthetic:
        a.workspace = a.workspace or tempfile.mkdtemp(prefix="stage0_train_")
        H, W, focal, train, held = synthetic_views(a, a.views, max(a.eval_views, 2))
    else:
        H, W, focal, train = load_blender(a, "train", u8=a.random_image_batch)
        held = load_blender(a, "test", a.eval_views)[3] if a.eval_views and os.path.exists(os.path.join(a.path, "transforms_test.json")) else []
    intr = (focal, focal, W * 0.5, H * 0.5)
    ck_path = os.path.join(a.workspace, "checkpoints", "ngp.pth")
    step0 = 0
    if a.resume:
        ck = torch.load(ck_path, map_location="cpu", weights_only=False)
        field = stage0.RadianceField.from_checkpoint(ck, bound=a.bound)
        grid = stage0.DensityGrid.from_checkpoint(ck, bound=a.bound, min_near=a.min_near, density_thresh=a.density_thresh)
        step0 = int(ck.get("global_step", 0))
    else:
        field = stage0.RadianceField.init_random(a.bound, a.seed)
        grid = stage0.DensityGrid(bound=a.bound, grid_size=a.grid_size, density_thresh=a.density_thresh, min_near=a.min_near)
    params = field.parameters()
    # the reference's parameter groups: encoder, sigma_net, color_net (nerf/network.py:278-286), all at --lr
    opt = torch.optim.Adam([{"params": params[:1], "lr": a.lr}, {"params": params[1:3], "lr": a.lr}, {"params": params[3:], "lr": a.lr}], eps=1e-15)
    ema = EMA(params)
    if a.resume:
        if "ema" in ck:                                                           # `model` holds the averaged weights; training continues from the field's own
            with torch.no_grad():
                for p, own, sh in zip(params, ck["ema"]["collected_params"], ck["ema"]["shadow_params"]):
                    p.copy_(own.to(dev))
                ema.shadow = [sh.to(dev).clone() for sh in ck["ema"]["shadow_params"]]
            ema.num_updates = int(ck["ema"]["num_updates"])
        if "optimizer" in ck:
            opt.load_state_dict(ck["optimizer"])
        log("[INFO] resumed %s at iteration %d" % (ck_path, step0))
    for g in opt.param_groups:
        g["initial_lr"] = a.lr
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: lr_factor(it, a.iters), last_epoch=step0 - 1)
    if a.mark_untrained and not a.resume:
        poses = torch.from_numpy(np.stack([v[0] for v in train])).to(dev)
        log("[INFO] mark_untrained: %d cells no training camera covers" % grid.mark_untrained(poses, torch.tensor(intr)))
    gen = torch.Generator(device=dev); gen.manual_seed(a.seed + 1 + step0)

    def save(step):
        CK.save_stage0_checkpoint(ck_path, field, grid, epoch=step // max(len(train), 1), global_step=step, optimizer=opt, ema=ema.state_dict())

    if a.random_image_batch:                                                      # every training view on the device once
        all_poses = torch.from_numpy(np.stack([v[0] for v in train])).to(dev)
        all_pixels = torch.stack([v[1] for v in train]).to(dev)                   # [V, H * W, C]: uint8 as read from disk, f32 renders under --synthetic
        all_alpha = torch.stack([v[2] for v in train]).to(dev) if train[0][2] is not None else None

    losses = []
    num_rays = a.num_rays
    for step in range(step0, a.iters):
        if step % a.update_extra_interval == 0:
            grid.update(field, noise=torch.rand(grid.cascade, grid.grid_size ** 3, 3, generator=gen, device=dev))
        if a.random_image_batch:
            index = torch.randint(len(train), (num_rays,), generator=gen, device=dev)
            pix = torch.randint(H * W, (num_rays,), generator=gen, device=dev)
            rays_o, rays_d = harness.get_rays_at(all_poses[index], intr, H, W, pix)
            if all_pixels.dtype == torch.uint8:
                gt, al = pixels_to_gt(all_pixels[index, pix], a.color_space)
            else:
                gt, al = all_pixels[index, pix], (all_alpha[index, pix] if all_alpha is not None else None)
        else:
            pose, premult, alpha = train[int(torch.randint(len(train), (1,), generator=gen, device=dev).item())]
            pix = torch.randint(H * W, (num_rays,), generator=gen, device=dev)
            o, d = harness.get_rays(torch.from_numpy(pose).to(dev), intr, H, W)
            rays_o, rays_d = o[pix], d[pix]
            gt = premult.to(dev)[pix]
            al = alpha.to(dev)[pix] if alpha is not None else None
        bg = torch.rand(num_rays, 3, generator=gen, device=dev) if a.background == "random" else torch.ones(num_rays, 3, device=dev)
        if al is not None:
            gt = gt + bg * (1 - al[:, None])
        out = stage0.render_stage0_train(field, grid, rays_o, rays_d, bg_color=bg, perturb=True, dt_gamma=a.dt_gamma, max_steps=a.max_steps, T_thresh=a.T_thresh,
                                         noises=torch.rand(num_rays, generator=gen, device=dev))
        loss = a.lambda_rgb * ((out["image"] - gt) ** 2).mean(-1)
        if al is not None:
            loss = loss + a.lambda_mask * (out["weights_sum"] - al) ** 2
        loss = loss.mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if a.lambda_tv > 0 and field.table.grad is not None:                      # nerf/utils.py:1152-1158, on the step's own sample points
            xyzs = out["xyzs"]
            if a.bound > 1:
                inner = xyzs.abs().amax(-1) <= 1
                field.grad_total_variation(a.lambda_tv, xyzs[inner])
                field.grad_total_variation(a.lambda_tv * 10, xyzs[~inner])
            else:
                field.grad_total_variation(a.lambda_tv, xyzs)
        opt.step(); sched.step(); ema.update(params)
        losses.append(float(loss.item()))
        if (step + 1) % a.window == 0:
            log("[INFO] iteration %d: loss %.6f (mean of the last %d), %d rays, %d samples, lr %.3e" % (step + 1, float(np.mean(losses[-a.window:])), a.window, num_rays,
                                                                                                   out["num_points"], opt.param_groups[0]["lr"]))
        if a.adaptive_num_rays:
            num_rays = adapt_num_rays(num_rays, out["num_points"], a.num_points, a.max_num_rays)
        if a.save_interval and (step + 1) % a.save_interval == 0 and step + 1 < a.iters:
            save(step + 1)
    save(a.iters)
    log("[INFO] wrote %s" % ck_path)
    if losses:
        w = min(a.window, len(losses))
        log("[RESULT] first-window loss %.6e last-window loss %.6e (windows of %d iterations)" % (float(np.mean(losses[:w])), float(np.mean(losses[-w:])), w))
    if held and (a.eval_views or a.synthetic):
        with torch.no_grad():                                                     # the averaged weights, as the written checkpoint has them
            own = [p.detach().clone() for p in params]
            for p, s in zip(params, ema.shadow):
                p.copy_(s)
            psnrs = []
            for pose, premult, alpha in held:
                o, d = harness.get_rays(torch.from_numpy(pose).to(dev), intr, H, W)
                img = stage0.render_stage0(field, grid, o, d, bg_color=None, dt_gamma=a.dt_gamma, max_steps=a.max_steps, T_thresh=a.T_thresh)["image"]
                gt = premult.to(dev) + ((1 - alpha.to(dev))[:, None] if alpha is not None else 0)
                psnrs.append(harness.psnr(img, gt))
            for p, s in zip(params, own):
                p.copy_(s)
        log("[RESULT] held-out PSNR %.3f over %d views" % (float(np.mean(psnrs)), len(psnrs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
