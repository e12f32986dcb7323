"""Renders a stage-0 checkpoint's radiance field on the HIP path: the reference's `--stage 0 --test` (Trainer.test, nerf/utils.py:1319-1378, over the inference
branch of NeRFRenderer.render, nerf/renderer.py:702-839) — per view of a NeRF-blender `transforms_*.json` one stage0.render_stage0 frame, written as
`<workspace>/results/<name>_{i:04d}_rgb.png` and `_depth.png`.

    python scripts/render_stage0.py --workspace <ws> --ckpt <ws>/checkpoints/ngp_stage0_epXXXX.pth --transforms <data>/transforms_test.json --bound B \
        [--downscale 1 --max_steps 1024 --T_thresh 1e-4 --dt_gamma 0 --min_near 0.2 --color_space srgb|linear --H 800 --W 800 --scale 1 --offset 0 0 0]
    python scripts/render_stage0.py --synthetic [--workspace <ws>] [--H 128 --W 128 --views 3]

The checkpoint gives the network (stage0.RadianceField.from_checkpoint: torch-ngp's GridEncoder, sigma_net, the SH direction encoder and color_net, evaluated in
fp32 by one fused kernel per batch of samples) and the occupancy grid (stage0.DensityGrid.from_checkpoint: density_grid, density_bitfield — packed from the grid at
min(mean_density, --density_thresh) when the checkpoint has none —, aabb_train; `aabb_infer` bounds the rays when the checkpoint holds one).  `--bound` is the --bound
the checkpoint was trained with.  Rays are harness.get_rays of the frame's pose (nerf_matrix_to_ngp with --scale / --offset, as evaluate.py reads it); the image is
quantised to 8 bits as Trainer.test does ((x * 255).astype(uint8), after linear_to_srgb with `--color_space linear`), the depth is min-max normalised with the
reference's + 1e-6.  Where the frame's image file exists the PSNR against rgb * a + (1 - a) (eval_step's fixed white background) is reported, and the mean over
the views.  No video is written.

`--synthetic` renders stage0.synthetic_radiance_checkpoint() from a few orbit cameras at distance 3 into the workspace (a temporary one when none is given) and
holds every OPAQUE pixel (weights_sum >= 0.999) to the checkpoint's closed form in the two channels that depend on the view direction alone: the script exits
non-zero when a quantised value misses the quantised closed form by more than one step of 1/255, or when a view has no opaque pixel."""
import argparse, json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OPAQUE = 0.999                                # --synthetic: a pixel this opaque shows the closed form within (1 - OPAQUE) < 1 / 255


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workspace"); p.add_argument("--ckpt", default=None); p.add_argument("--transforms", default=None)
    p.add_argument("--bound", type=float, default=1.0, help="the --bound the checkpoint was trained with (fixes the hash-grid layout and the cascades)")
    p.add_argument("--downscale", type=int, default=1); p.add_argument("--H", type=int, default=None); p.add_argument("--W", type=int, default=None)
    p.add_argument("--scale", type=float, default=1.0); p.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    p.add_argument("--max_steps", type=int, default=1024); p.add_argument("--T_thresh", type=float, default=1e-4); p.add_argument("--dt_gamma", type=float, default=0.0)
    p.add_argument("--min_near", type=float, default=0.2); p.add_argument("--density_thresh", type=float, default=10.0)
    p.add_argument("--color_space", choices=["srgb", "linear"], default="srgb", help="linear: the network's output is linear radiance, tone-mapped before it is written")
    p.add_argument("--synthetic", action="store_true"); p.add_argument("--views", type=int, default=3, help="--synthetic: the number of orbit cameras")
    return p


def parse_args(argv=None):
    """Validates what can be validated without a device."""
    p = build_parser()
    a = p.parse_args(argv)
    if a.synthetic:
        if a.ckpt or a.transforms:
            p.error("--synthetic brings its own checkpoint and cameras: drop --ckpt / --transforms")
        if a.bound != 1.0:
            p.error("--synthetic: the synthetic checkpoint's hash grid is laid out for --bound 1")
        if a.color_space != "srgb":
            p.error("--synthetic compares the written values with a closed form: --color_space linear would tone-map them")
        if a.views < 1:
            p.error("--views %d: at least 1" % a.views)
    else:
        if not a.workspace:
            p.error("--workspace is required")
        if not a.ckpt or not a.transforms:
            p.error("--ckpt and --transforms are required (or --synthetic)")
        for f in (a.ckpt, a.transforms):
            if not os.path.exists(f):
                p.error("%s does not exist" % f)
    if (a.H is None) != (a.W is None):
        p.error("--H and --W go together")
    if a.H is not None and (a.H < 1 or a.W < 1):
        p.error("--H %d --W %d: positive sizes" % (a.H, a.W))
    if not (a.bound > 0):
        p.error("--bound %g: a positive number" % a.bound)
    if a.downscale < 1:
        p.error("--downscale %d: at least 1" % a.downscale)
    if a.max_steps < 1:
        p.error("--max_steps %d: at least 1" % a.max_steps)
    if not (0 <= a.T_thresh < 1):
        p.error("--T_thresh %g: in [0, 1)" % a.T_thresh)
    if not (a.dt_gamma >= 0) or not (a.min_near >= 0):
        p.error("--dt_gamma and --min_near: not negative")
    a.name = "synthetic" if a.synthetic else os.path.splitext(os.path.basename(a.ckpt))[0]      # the file names' prefix
    return a


def orbit_poses(n, dist=3.0):
    """n cam2world poses on a tilted circle of radius `dist` looking at the origin (columns: right, up, -forward)."""
    import numpy as np
    poses = []
    for k in range(n):
        az, el = 0.7 + 2.0 * np.pi * k / n, 0.35
        eye = dist * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        fwd = -eye / np.linalg.norm(eye); right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right); up = np.cross(right, fwd)
        pose = np.eye(4, dtype=np.float32); pose[:3, :3] = np.stack([right, up, -fwd], 1); pose[:3, 3] = eye
        poses.append(pose)
    return poses


def quantise(img):
    """Trainer.test (nerf/utils.py:1353-1354): float [H, W, 3] -> uint8."""
    import numpy as np
    return (img * 255).astype(np.uint8)


def quantise_depth(depth):
    """nerf/utils.py:1359-1361."""
    import numpy as np
    d = (depth - depth.min()) / (depth.max() - depth.min() + 1e-6)
    return (d * 255).astype(np.uint8)


def load_views(a):
    """The cameras of a run, without a device -> (H, W, focal, frames); a frame is its cam2world pose and the path of its image file (None: --synthetic).
    The size is --H / --W, else the transforms file's `h` / `w` (800 when it has none; 128 for --synthetic), divided by --downscale; the focal length follows the
    width as in evaluate.py."""
    import numpy as np
    if a.synthetic:
        Hh, Ww = (a.H, a.W) if a.H is not None else (128, 128)
        Hh, Ww = Hh // a.downscale, Ww // a.downscale
        return Hh, Ww, 0.5 * Ww / 0.45, [{"pose": p, "file": None} for p in orbit_poses(a.views)]
    from evaluate import nerf_pose
    tf = json.load(open(a.transforms))
    Hh, Ww = (a.H, a.W) if a.H is not None else (int(tf.get("h", 800)), int(tf.get("w", 800)))
    Hh, Ww = Hh // a.downscale, Ww // a.downscale
    focal = 0.5 * Ww / np.tan(0.5 * tf["camera_angle_x"])
    base = os.path.dirname(os.path.abspath(a.transforms))
    return Hh, Ww, focal, [{"pose": nerf_pose(fr["transform_matrix"], a.scale, a.offset), "file": os.path.join(base, fr["file_path"] + ".png")} for fr in tf["frames"]]


def main(argv=None):
    a = parse_args(argv)
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, harness, meters, raymarching
    torch.cuda.set_device(0)
    log = lambda m: print(m, flush=True)
    if a.synthetic:
        a.workspace = a.workspace or tempfile.mkdtemp(prefix="stage0_render_")
        ck = stage0.synthetic_radiance_checkpoint(S=32)
    else:
        ck = torch.load(a.ckpt, map_location="cpu", weights_only=False)
    Hh, Ww, focal, frames = load_views(a)
    model = ck["model"] if "model" in ck else ck
    field = stage0.RadianceField.from_checkpoint(ck, bound=a.bound)
    grid = stage0.DensityGrid.from_checkpoint(ck, bound=a.bound, min_near=a.min_near, density_thresh=a.density_thresh)
    if a.synthetic:
        gen = torch.Generator(device="cuda"); gen.manual_seed(3)
        for _ in range(3):                                                        # the synthetic checkpoint stores no bitfield: the grid's own upkeep makes one
            grid.update(field, noise=torch.rand(grid.cascade, grid.grid_size ** 3, 3, generator=gen, device="cuda"))
    elif "density_bitfield" not in model:
        thresh = min(grid.mean_density, grid.density_thresh)
        log("[INFO] the checkpoint has no density_bitfield: packed from its density_grid at %g" % thresh)
        grid.density_bitfield = raymarching.packbits(grid.density_grid, thresh, grid.density_bitfield)
    aabb = model.get("aabb_infer")
    out_dir = os.path.join(a.workspace, "results"); os.makedirs(out_dir, exist_ok=True)
    intr = (focal, focal, Ww * 0.5, Hh * 0.5)
    psnrs, bad = [], 0
    for i, fr in enumerate(frames):
        rays_o, rays_d = harness.get_rays(torch.from_numpy(np.asarray(fr["pose"], np.float32)).cuda(), intr, Hh, Ww)
        out = stage0.render_stage0(field, grid, rays_o, rays_d, bg_color=None, dt_gamma=a.dt_gamma, max_steps=a.max_steps, T_thresh=a.T_thresh, perturb=False, aabb=aabb)
        img = out["image"].reshape(Hh, Ww, 3); depth = out["depth"].reshape(Hh, Ww)
        shown = harness.linear2srgb(img) if a.color_space == "linear" else img
        u8 = quantise(shown.cpu().numpy())
        f_rgb = os.path.join(out_dir, "%s_%04d_rgb.png" % (a.name, i)); f_depth = os.path.join(out_dir, "%s_%04d_depth.png" % (a.name, i))
        meters.write_png(f_rgb, u8); meters.write_png(f_depth, quantise_depth(depth.cpu().numpy()))
        note = ""
        if fr["file"] and os.path.exists(fr["file"]):
            from PIL import Image
            gt = np.asarray(Image.open(fr["file"]).resize((Ww, Hh), Image.BILINEAR)).astype(np.float32) / 255.0
            if gt.ndim == 3 and gt.shape[-1] == 4:
                gt = gt[..., :3] * gt[..., 3:] + (1 - gt[..., 3:])                # eval_step's fixed white background (nerf/utils.py:1177-1179)
            gt_t = torch.from_numpy(np.ascontiguousarray(gt[..., :3])).cuda()
            if a.color_space == "linear":
                gt_t = harness.srgb_to_linear(gt_t)
            psnrs.append(harness.psnr(img, gt_t)); note = ", PSNR %.3f" % psnrs[-1]
        if a.synthetic:
            ws = out["weights_sum"].cpu().numpy()
            opaque = ws >= OPAQUE
            want = quantise(stage0.synthetic_radiance_color(rays_d.cpu().numpy(), np.zeros(Hh * Ww))[:, :2]).astype(np.int32)
            got = u8.reshape(-1, 3)[:, :2].astype(np.int32)
            miss = int((np.abs(got - want)[opaque] > 1).sum())
            note += ", %d opaque pixels, %d values off the closed form by more than 1/255" % (int(opaque.sum()), miss)
            bad += miss + (0 if opaque.any() else 1)
        log("[INFO] view %d: %s, %s%s" % (i, os.path.basename(f_rgb), os.path.basename(f_depth), note))
    if psnrs:
        log("[INFO] mean PSNR over %d views: %.3f" % (len(psnrs), float(np.mean(psnrs))))
    log("[INFO] wrote %d views to %s" % (len(frames), out_dir))
    if a.synthetic and bad:
        log("[ERROR] --synthetic: %d opaque values miss the closed form (or a view has no opaque pixel)" % bad)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
