"""`--test --spp N` evaluation of a reference workspace on the HIP path: stage-0 mesh (+ stage-1 vertex offsets), material field and
environment map from a reference checkpoint, dataset cameras from a NeRF-blender `transforms_*.json`, one fused frame per view, PNG results and
PSNR / SSIM against the dataset images when they can be read.

    python scripts/evaluate.py --workspace <ws> --ckpt <ws>/checkpoints/ngp_stage1_ep0100.pth --transforms <data>/transforms_test.json \
        [--spp 512 --ssaa 2 --downscale 1 --bound 2 --roughness_min 0.08 --me_max 0 --out <ws>/results_brdf --limit 0 --synthetic]
        [--export_mesh --texture_size 4096] [--textured_mesh <ws>/mesh_stage1]

`--export_mesh` (off by default) writes the stage-1 textured mesh after the views, as the reference's `--test` does unless `--test_no_mesh`
(main.py:256-258): <ws>/mesh_stage1/mesh_{cas}.obj / .mtl / feat0_{cas}.png / feat1_{cas}.png (mirres_restir_nerf_mesh_amd/export.py, with --ssaa).

`--textured_mesh DIR` renders the dataset views from an exported stage-1 asset (mesh_{cas}.obj + feat0 / feat1_{cas}.png or .jpg, export.load_stage1) instead
of the checkpoint's mesh and field: every primary and indirect hit reads the textures (mirres_texmat_lookup).  The environment map comes from the checkpoint
or from --envmap_path (relighting and albedo scale as usual).  With a checkpoint the field's own frames are rendered first and every textured frame
reports its PSNR against the field's frame at the same seed (what the export lost); with --export_mesh the asset is the one just written.

The material-field constants are the reference's CLI ones and MUST equal the training run's (nerf/network.py:119-125): `--bound` (hash-grid AABB
= +-bound, main.py:39 default 2; also the mesh cascade count 1 + ceil(log2(bound)), nerf/renderer.py:97, unless `--cascade` overrides it),
`--roughness_min` / `--me_max` (main.py:109-110,169-170) and, for completeness, `--kd_min` / `--kd_max` (main.py:167-168).  Checkpoints written by
this package record them (`material_config`); a flag given on the command line wins, a mismatch with the recorded value is reported.

Relighting (reference: `--test --envmap_path X.hdr --albedo_scale_x/y/z`, nerf/network.py:134-139, nerf/renderer.py:1025-1026, 1086-1089, 1109-1111):
`--envmap_path` replaces the trained environment map by a Radiance .hdr file (any size) and switches the albedo scaling on.  The three scales are what
`scripts/albedo_eval.py` measures (the reference's albedo_eval.py); `--albedo_scale_file <its albedo_scale.json>` passes them on without retyping.
`--use_hdr --exposure E` (every relighting command of configs/OWL/*.txt): radiance x 2**E before the clamp (nerf/renderer.py:1125-1127), and the saved
env_map scaled alike (:1343-1344).

Several GPUs (`python -m torch.distributed.run --nproc-per-node N scripts/evaluate.py ... --shard views|strips|spp`): `views` (default) deals the
dataset views round-robin to the ranks — no data-path communication, metrics reduced at the end; `strips` / `spp` render EVERY view on all ranks
(exact row strips with per-sample halo exchange and an all-gather of the radiance rows / sample slices with one all-reduce; dist.py) — what a single
large frame wants.  Rank 0 writes the images of the frames it holds (all of them for strips / spp).

`--synthetic` builds a throw-away workspace (synthetic mesh, random material field, sky map, four orbit cameras) first and evaluates that — the
smoke run of this script on a box without a reference workspace.  Camera convention: the blender `transform_matrix` is the cam2world pose with its
translation scaled by `--scale` and shifted by `--offset` (nerf_matrix_to_ngp, nerf/provider.py:18-21; pass the values the reference run used)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
import mirres_restir_nerf_mesh_amd as M
from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness, checkpoint as CK, meters, dist as MD
from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D


def nerf_pose(pose, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """nerf_matrix_to_ngp of this reference (nerf/provider.py:18-21): the rotation is kept, the translation is scaled and shifted."""
    p = np.array(pose, np.float32)
    p[:3, 3] = p[:3, 3] * scale + np.asarray(offset, np.float32)
    return p


def synthetic_workspace(root, H=100, W=100):
    os.makedirs(os.path.join(root, "mesh_stage0"), exist_ok=True); os.makedirs(os.path.join(root, "checkpoints"), exist_ok=True)
    v, t = M.scene.make_mesh(5, 16)
    CK.write_ply(os.path.join(root, "mesh_stage0", "mesh_0.ply"), v, t)
    mn, mx = M.scene.material_min_max()
    torch.manual_seed(0)
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    ck = os.path.join(root, "checkpoints", "ngp_stage1_ep0001.pth")
    CK.save_checkpoint(ck, mlp, torch.zeros(v.shape[0], 3), torch.from_numpy(M.scene.make_env(64, 128)), epoch=1,
                       material_config=CK.material_config(bound=1.0))
    frames = []
    for k in range(4):
        az, el = np.deg2rad(30.0 + 90.0 * k), np.deg2rad(30.0)
        eye = 3.2 * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        fwd = -eye / np.linalg.norm(eye); right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right); up = np.cross(right, fwd)
        pose = np.eye(4); pose[:3, :3] = np.stack([right, up, -fwd], 1); pose[:3, 3] = eye
        frames.append({"file_path": "./test/r_%d" % k, "transform_matrix": pose.tolist()})
    tf = os.path.join(root, "transforms_test.json")
    json.dump({"camera_angle_x": 0.6911, "w": W, "h": H, "frames": frames}, open(tf, "w"))
    return ck, tf


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--workspace"); p.add_argument("--ckpt"); p.add_argument("--transforms"); p.add_argument("--out")
    p.add_argument("--spp", type=int, default=512); p.add_argument("--ssaa", type=int, default=2); p.add_argument("--downscale", type=int, default=1)
    p.add_argument("--cascade", type=int, default=None, help="mesh cascades; default 1 + ceil(log2(bound)) as nerf/renderer.py:97")
    p.add_argument("--bound", type=float, default=None, help="main.py --bound (default 2): material-field AABB = +-bound")
    p.add_argument("--roughness_min", type=float, default=None, help="main.py --roughness_min (default 0.08)")
    p.add_argument("--me_max", type=float, default=None, help="main.py --me_max (default 0.0)")
    p.add_argument("--kd_min", type=float, nargs=3, default=None); p.add_argument("--kd_max", type=float, nargs=3, default=None)
    p.add_argument("--limit", type=int, default=0); p.add_argument("--H", type=int, default=800); p.add_argument("--W", type=int, default=800)
    p.add_argument("--save_maps", action="store_true", help="also write kd / ks / normal / env_map / diffuse and specular light as EXR files, like Trainer.test (nerf/utils.py:1372-1377)")
    p.add_argument("--scale", type=float, default=1.0); p.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0]); p.add_argument("--synthetic", action="store_true")
    p.add_argument("--envmap_path", default="None", help="main.py --envmap_path: Radiance .hdr environment map for relighting")
    p.add_argument("--albedo_scale_x", type=float, default=None, help="default 1.0"); p.add_argument("--albedo_scale_y", type=float, default=None, help="default 1.0")
    p.add_argument("--albedo_scale_z", type=float, default=None, help="default 1.0")
    p.add_argument("--albedo_scale_file", default=None, help="albedo_scale.json of scripts/albedo_eval.py: fills the three scales (not together with --albedo_scale_x/y/z)")
    p.add_argument("--use_hdr", action="store_true", help="main.py --use_hdr (the relighting commands of configs/OWL/*.txt): radiance and the saved env_map x 2**exposure")
    p.add_argument("--exposure", type=float, default=0.0, help="main.py --exposure, read with --use_hdr")
    p.add_argument("--shard", choices=("views", "strips", "spp"), default="views", help="how N > 1 ranks (torch.distributed.run) divide the work")
    p.add_argument("--lpips_vgg", default=None, help="torchvision vgg16 state dict (or a state dict of lpips.LPIPS): adds the reference's LPIPS (vgg) meter; no weights ship with the image")
    p.add_argument("--lpips_lin", default=None, help="the lpips package's weights/v0.1/vgg.pth (the five linear heads)")
    p.add_argument("--nerf_image", action="store_true", help="also write <name>_<i>_rgb.png, the NeRF colour branch's frame (Trainer.test's `image`: the stage-0 network's colour "
                   "at the surface), and print its PSNR; the network comes from --ckpt when it holds it, else from --stage0_ckpt")
    p.add_argument("--stage0_ckpt", default=None, help="--nerf_image: a stage-0 checkpoint, or `random` (RadianceField.init_random)")
    p.add_argument("--export_mesh", action="store_true", help="after the views, export the stage-1 textured mesh to <workspace>/mesh_stage1 (main.py:256-258; off by default)")
    p.add_argument("--texture_size", type=int, default=4096, help="main.py --texture_size: texture side of the first cascade of --export_mesh (baked at --ssaa)")
    p.add_argument("--atlas", choices=("pairs", "charts"), default="pairs", help="--export_mesh: the UV atlas, triangle pairs (export.uv_atlas) or axis-projected charts (export.chart_atlas)")
    p.add_argument("--textured_mesh", default=None, help="render the views from this exported stage-1 asset (mesh_{cas}.obj, feat0/feat1_{cas}.png|.jpg); with "
                   "--ckpt also report each textured frame's PSNR against the field's frame")
    return p


def parse_args(argv=None):
    """-> (args, parser); a.albedo_scale_x/y/z are floats afterwards (from the command line, from --albedo_scale_file, or 1.0) and a.exposure is the
    float harness.test_view takes, or None without --use_hdr."""
    p = build_parser()
    a = p.parse_args(argv)
    typed = [k for k in "xyz" if getattr(a, "albedo_scale_" + k) is not None]
    if a.albedo_scale_file is not None:
        if typed:
            p.error("--albedo_scale_file and --albedo_scale_%s are two sources for one number: give one" % "/".join(typed))
        from mirres_restir_nerf_mesh_amd import albedo
        a.albedo_scale_x, a.albedo_scale_y, a.albedo_scale_z = albedo.read_scale(a.albedo_scale_file)["scale"]
    if a.albedo_scale_file is not None and a.envmap_path == "None":
        p.error("--albedo_scale_file is read for relighting only: give --envmap_path (without it the albedo is not scaled)")
    for k in "xyz":
        if getattr(a, "albedo_scale_" + k) is None:
            setattr(a, "albedo_scale_" + k, 1.0)
    a.exposure = a.exposure if a.use_hdr else None
    return a, p


def main():
    a, p = parse_args()
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("MIRRES_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": torch.device("cuda", torch.cuda.current_device())} if backend == "nccl" else {}))
    if a.synthetic:
        a.workspace = a.workspace or os.path.join(ROOT, "gpurun_out", "eval_ws")
        if rank == 0:
            a.ckpt, a.transforms = synthetic_workspace(a.workspace, a.H // a.downscale, a.W // a.downscale)
        if world > 1:
            dist.barrier()
        a.ckpt, a.transforms = os.path.join(a.workspace, "checkpoints", "ngp_stage1_ep0001.pth"), os.path.join(a.workspace, "transforms_test.json")
    if a.textured_mesh and not a.ckpt and a.transforms:
        return textured_only(a, p, rank, world)
    if not (a.workspace and a.ckpt and a.transforms):
        p.error("--workspace, --ckpt and --transforms are required (or --synthetic)")
    out_dir = a.out or os.path.join(a.workspace, "results_brdf")
    ck = CK.read_checkpoint(a.ckpt)
    cfg = CK.resolve_material_config(ck.get("material_config"), bound=a.bound, roughness_min=a.roughness_min, me_max=a.me_max, kd_min=a.kd_min, kd_max=a.kd_max)
    cascade = a.cascade if a.cascade is not None else CK.cascade_of_bound(cfg["bound"])
    v, t, v_cumsum, f_cumsum = CK.load_stage0_mesh(a.workspace, cascade)
    aabb, mn, mx = CK.material_field_args(cfg)     # nerf/network.py:119-125
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()))
    voff, light = CK.apply_checkpoint(ck, mlp, n_vertices=v.shape[0])
    albedo_scale = None
    if a.envmap_path != "None":      # relighting: the external map as it is (no clamp), albedo scaling on (network.py:134-139, renderer.py:1109-1111)
        light = torch.from_numpy(np.ascontiguousarray(harness.read_hdr(a.envmap_path))).cuda()
        albedo_scale = (a.albedo_scale_x, a.albedo_scale_y, a.albedo_scale_z)
    if light is None:
        raise SystemExit("%s has no light_base (a --use_brdf stage-1 checkpoint is needed)" % a.ckpt)
    verts = torch.from_numpy(v).cuda() + (voff if voff is not None else 0)
    W = RR.restirbvhWorker(verts.contiguous(), torch.from_numpy(t).cuda()); W.update_mesh(W.vrt, W.v_ind)
    tf = json.load(open(a.transforms)); base = os.path.dirname(os.path.abspath(a.transforms))
    Hh, Ww = int(tf.get("h", a.H)) // a.downscale, int(tf.get("w", a.W)) // a.downscale
    focal = 0.5 * Ww / np.tan(0.5 * tf["camera_angle_x"])
    intr = (focal, focal, Ww * 0.5, Hh * 0.5)
    frames = tf["frames"][: a.limit] if a.limit > 0 else tf["frames"]
    pm, sm = meters.PSNRMeter(), meters.SSIMMeter()
    nerf = None
    if a.nerf_image:
        from mirres_restir_nerf_mesh_amd.stage0 import RadianceField
        ck_model = CK.stage0_model_of(a.ckpt)
        if all(k in ck_model for k in CK.STAGE0_WEIGHT_KEYS):
            nerf = RadianceField.from_checkpoint(ck_model, bound=cfg["bound"])
        elif a.stage0_ckpt == "random" or (a.synthetic and not a.stage0_ckpt):      # the synthetic workspace has no stage 0: a freshly initialised network
            nerf = RadianceField.init_random(bound=cfg["bound"])
        elif a.stage0_ckpt:
            nerf = RadianceField.from_checkpoint(torch.load(a.stage0_ckpt, map_location="cpu", weights_only=False), bound=cfg["bound"])
        else:
            p.error("--nerf_image: %s holds no stage-0 network; give --stage0_ckpt" % a.ckpt)
    pm_nerf = meters.PSNRMeter()
    lm = meters.LPIPSMeter(vgg=a.lpips_vgg, lin=a.lpips_lin) if a.lpips_vgg else None        # main.py:250: [PSNRMeter(), SSIMMeter(), LPIPSMeter(device=device)]
    name = os.path.splitext(os.path.basename(a.ckpt))[0]
    if world == 1 or a.shard == "views":
        # the engine context of the frame size and its batch pool (tens of GB: one hipMalloc + clear) are set up here, not inside the first view's timed region
        from mirres_restir_nerf_mesh_amd._ops import get_ctx
        get_ctx(Ww * a.ssaa, Hh * a.ssaa).reserve()
    t_render = 0.0
    n_mine = 0
    # exact strip sharding: the boundaries follow the strips' measured times from view to view (a test set's cameras move smoothly; same pixels for any boundaries)
    balancer = MD.StripBalancer(Hh * a.ssaa, world) if (world > 1 and a.shard == "strips") else None
    field_imgs = {}
    for i, fr in enumerate(frames):
        if world > 1 and a.shard == "views" and i % world != rank:
            continue
        n_mine += 1
        pose = nerf_pose(fr["transform_matrix"], a.scale, a.offset)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        img = harness.test_view(W, mlp, light, torch.from_numpy(pose), intr, Hh, Ww, a.spp, a.ssaa, random_offset=i * 7919, albedo_scale=albedo_scale, exposure=a.exposure,
                                shard=a.shard if world > 1 and a.shard != "views" else None, rank=rank, world=world, return_maps=a.save_maps, balancer=balancer)
        maps = None
        if a.save_maps:
            img, maps = img
        torch.cuda.synchronize(); t_render += time.perf_counter() - t0
        if a.textured_mesh:
            field_imgs[i] = img
        if world > 1 and a.shard != "views" and rank != 0:
            continue                                                       # every rank holds the whole frame; rank 0 writes and scores it
        img_nerf = harness.nerf_view(W, nerf, torch.from_numpy(pose), intr, Hh, Ww, a.ssaa) if nerf is not None else None
        files = meters.write_test_frame(out_dir, name, i, img, image=img_nerf)
        if maps is not None:                                               # kd / ks / normal / env_map / diffuse + specular light as EXR (utils.py:1372-1377)
            files += meters.write_test_maps(out_dir, name, i, maps)
        gt_path = os.path.join(base, fr["file_path"] + ".png")
        note = ""
        if os.path.exists(gt_path):
            from PIL import Image
            gt = np.asarray(Image.open(gt_path).resize((Ww, Hh), Image.BILINEAR)).astype(np.float32) / 255.0
            if gt.shape[-1] == 4:
                gt = gt[..., :3] * gt[..., 3:] + (1 - gt[..., 3:])                      # white background, as the reference's loader composes it
            gt_t = torch.from_numpy(gt).cuda()
            note = "  PSNR %.3f  SSIM %.4f" % (pm.update(img, gt_t), sm.update(img, gt_t))
            if lm is not None:
                note += "  LPIPS %.4f" % lm.update(img, gt_t)
            if img_nerf is not None:
                note += "  PSNR(rgb) %.3f" % pm_nerf.update(img_nerf, gt_t)
        print("[%d/%d] %s%s" % (i + 1, len(frames), os.path.basename(files[0]), note), flush=True)
    n = len(frames)
    if world > 1:      # wall time of the job = the slowest rank; metric sums over the ranks that scored frames
        red = torch.tensor([t_render, pm.V, float(pm.N), sm.V, float(sm.N), lm.V if lm else 0.0, float(lm.N) if lm else 0.0, pm_nerf.V, float(pm_nerf.N)], dtype=torch.float64, device="cuda")
        tmax = red[:1].clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); dist.all_reduce(red, op=dist.ReduceOp.SUM)
        t_render = float(tmax.item()); pm.V, pm.N, sm.V, sm.N = float(red[1]), int(red[2]), float(red[3]), int(red[4])
        if lm:
            lm.V, lm.N = float(red[5]), int(red[6])
        pm_nerf.V, pm_nerf.N = float(red[7]), int(red[8])
    if rank == 0:
        print("rendered %d views %dx%d ssaa %d spp %d on %d GPU(s)%s: %.1f ms/view (%.1f Msamples/s)" % (
            n, Ww, Hh, a.ssaa, a.spp, world, (" [%s]" % a.shard) if world > 1 else "", 1e3 * t_render / max(n, 1), n * Ww * Hh * a.ssaa ** 2 * a.spp / max(t_render, 1e-9) / 1e6))
        if pm.N:
            print(pm.report(), sm.report(), lm.report() if lm and lm.N else "")
        if pm_nerf.N:
            print("NeRF colour branch (_rgb.png): " + pm_nerf.report())
        if a.export_mesh:          # trainer.export_stage1(resolution=opt.texture_size) after the test views (main.py:256-258)
            from mirres_restir_nerf_mesh_amd import export as EX
            EX.export_stage1(os.path.join(a.workspace, "mesh_stage1"), verts, t, v_cumsum, f_cumsum, mlp, texture_size=a.texture_size, ssaa=a.ssaa, atlas=a.atlas)
    if a.textured_mesh:
        if world > 1:
            dist.barrier()                                                 # the asset may just have been written by rank 0
        render_textured(a, frames, base, intr, Hh, Ww, light, albedo_scale, out_dir, name, rank, world, field_imgs, cfg["roughness_min"])
    if world > 1:
        dist.destroy_process_group()


def render_textured(a, frames, base, intr, Hh, Ww, light, albedo_scale, out_dir, name, rank, world, field_imgs, roughness_min):
    """The views from the exported asset (export.load_stage1 -> mirres_texmat_t): BVH of the asset's own mesh, the same seeds as the field's views; per view
    the PSNR against the field's frame when there is one (the export's loss: atlas, 8-bit sRGB, gutter inpaint, SSAA downsample)."""
    from mirres_restir_nerf_mesh_amd import export as EX
    tex = EX.load_stage1(a.textured_mesh, roughness_min=roughness_min)
    Wt = RR.restirbvhWorker(tex.verts, tex.tris); Wt.update_mesh(Wt.vrt, Wt.v_ind)
    shard = a.shard if world > 1 and a.shard != "views" else None
    psnrs = []
    for i, fr in enumerate(frames):
        if world > 1 and a.shard == "views" and i % world != rank:
            continue
        pose = nerf_pose(fr["transform_matrix"], a.scale, a.offset)
        img = harness.test_view(Wt, tex, light, torch.from_numpy(pose), intr, Hh, Ww, a.spp, a.ssaa, random_offset=i * 7919, albedo_scale=albedo_scale, exposure=a.exposure,
                                shard=shard, rank=rank, world=world)
        if world > 1 and shard is not None and rank != 0:
            continue
        files = meters.write_test_frame(out_dir, name + "_textured", i, img)
        note = ""
        if i in field_imgs:
            v = harness.psnr(img, field_imgs[i]); psnrs.append(v)
            note = "  PSNR vs field %.3f" % v
        print("[textured %d/%d] %s%s" % (i + 1, len(frames), os.path.basename(files[0]), note), flush=True)
    if psnrs:
        print("textured vs field: mean PSNR %.3f over %d view(s)" % (float(np.mean(psnrs)), len(psnrs)), flush=True)


def textured_only(a, p, rank, world):
    """--textured_mesh without a checkpoint: the asset under --envmap_path (relighting; there is no trained environment map to take)."""
    if a.envmap_path == "None":
        p.error("--textured_mesh without --ckpt needs --envmap_path")
    if world > 1:
        import torch.distributed as dist
    light = torch.from_numpy(np.ascontiguousarray(harness.read_hdr(a.envmap_path))).cuda()
    albedo_scale = (a.albedo_scale_x, a.albedo_scale_y, a.albedo_scale_z)
    tf = json.load(open(a.transforms)); base = os.path.dirname(os.path.abspath(a.transforms))
    Hh, Ww = int(tf.get("h", a.H)) // a.downscale, int(tf.get("w", a.W)) // a.downscale
    focal = 0.5 * Ww / np.tan(0.5 * tf["camera_angle_x"])
    frames = tf["frames"][: a.limit] if a.limit > 0 else tf["frames"]
    out_dir = a.out or os.path.join(a.workspace or os.path.dirname(os.path.abspath(a.textured_mesh)), "results_textured")
    rmin = a.roughness_min if a.roughness_min is not None else 0.08
    render_textured(a, frames, base, (focal, focal, Ww * 0.5, Hh * 0.5), Hh, Ww, light, albedo_scale, out_dir, "asset", rank, world, {}, rmin)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
