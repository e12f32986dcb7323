"""Albedo evaluation with median scale alignment on the HIP path (the reference's albedo_eval.py, which reads the `_kd.exr` files of a finished `--test`
run): per test view the albedo of the workspace (harness.albedo_view: G-buffer and material lookup, no sample loop) against the dataset's
`<gt_dir>/test_XXX/diffuse-color.exr`; the channel-wise median of gt / albedo over the masked pixels of all views is the scale of the relighting
commands (`--albedo_scale_x/y/z`), and the aligned albedo is scored: PSNR of the linear and of the gamma 2.2 images, SSIM, LPIPS (vgg) when weights are given.

    python scripts/albedo_eval.py --workspace <ws> --ckpt <ws>/checkpoints/ngp_stage1_ep0075.pth --transforms <data>/transforms_test.json --gt_dir <data> \
        [--mask_thr 0.9 --ssaa 2 --textured_mesh <ws>/mesh_stage1 --limit 0 --out <ws>/albedo_eval --lpips_vgg X --lpips_lin Y]
    python scripts/evaluate.py ... --envmap_path <map>.hdr --albedo_scale_file <ws>/albedo_eval/albedo_scale.json        # the relighting step

`--mask_thr`: 0.3 for ficus and 0.9 for the other TensoIR scenes.  Written to --out: albedo_scale.json (albedo.write_scale) and gammaed_scaled_kd_{i}.png.
`--textured_mesh DIR` scores the exported stage-1 asset's albedo instead of the field's.  `--synthetic` builds evaluate.py's throw-away workspace and a
ground truth of its own (the workspace's albedo times (0.7, 1.3, 0.9), clipped to 1, alpha = coverage, written as diffuse-color.exr) — the smoke run.
The material-field and camera flags are evaluate.py's and must equal the training run's."""
import argparse, json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness, checkpoint as CK, meters, albedo
from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
from evaluate import nerf_pose, synthetic_workspace

SYNTHETIC_SCALE = (0.7, 1.3, 0.9)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workspace"); p.add_argument("--ckpt"); p.add_argument("--transforms"); p.add_argument("--gt_dir"); p.add_argument("--out")
    p.add_argument("--mask_thr", type=float, default=0.9); p.add_argument("--ssaa", type=int, default=2); p.add_argument("--downscale", type=int, default=1)
    p.add_argument("--cascade", type=int, default=None); p.add_argument("--bound", type=float, default=None); p.add_argument("--roughness_min", type=float, default=None)
    p.add_argument("--me_max", type=float, default=None); p.add_argument("--kd_min", type=float, nargs=3, default=None); p.add_argument("--kd_max", type=float, nargs=3, default=None)
    p.add_argument("--limit", type=int, default=0); p.add_argument("--H", type=int, default=800); p.add_argument("--W", type=int, default=800)
    p.add_argument("--scale", type=float, default=1.0); p.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0]); p.add_argument("--synthetic", action="store_true")
    p.add_argument("--textured_mesh", default=None, help="score the albedo of this exported stage-1 asset (export.load_stage1)")
    p.add_argument("--lpips_vgg", default=None); p.add_argument("--lpips_lin", default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    if a.synthetic:
        a.workspace = a.workspace or tempfile.mkdtemp(prefix="albedo_ws_")
        a.ckpt, a.transforms = synthetic_workspace(a.workspace, a.H // a.downscale, a.W // a.downscale)
        a.gt_dir = os.path.join(a.workspace, "gt")
    if not (a.workspace and a.ckpt and a.transforms and a.gt_dir):
        p.error("--workspace, --ckpt, --transforms and --gt_dir are required (or --synthetic)")
    out_dir = a.out or os.path.join(a.workspace, "albedo_eval")
    os.makedirs(out_dir, exist_ok=True)
    ck = CK.read_checkpoint(a.ckpt)
    cfg = CK.resolve_material_config(ck.get("material_config"), bound=a.bound, roughness_min=a.roughness_min, me_max=a.me_max, kd_min=a.kd_min, kd_max=a.kd_max)
    if a.textured_mesh:
        from mirres_restir_nerf_mesh_amd import export as EX
        mat = EX.load_stage1(a.textured_mesh, roughness_min=cfg["roughness_min"])
        W = RR.restirbvhWorker(mat.verts, mat.tris)
    else:
        cascade = a.cascade if a.cascade is not None else CK.cascade_of_bound(cfg["bound"])
        v, t, _, _ = CK.load_stage0_mesh(a.workspace, cascade)
        aabb, mn, mx = CK.material_field_args(cfg)
        mat = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()))
        voff, _ = CK.apply_checkpoint(ck, mat, n_vertices=v.shape[0])
        W = RR.restirbvhWorker((torch.from_numpy(v).cuda() + (voff if voff is not None else 0)).contiguous(), torch.from_numpy(t).cuda())
    W.update_mesh(W.vrt, W.v_ind)
    tf = json.load(open(a.transforms))
    Hh, Ww = int(tf.get("h", a.H)) // a.downscale, int(tf.get("w", a.W)) // a.downscale
    focal = 0.5 * Ww / np.tan(0.5 * tf["camera_angle_x"])
    intr = (focal, focal, Ww * 0.5, Hh * 0.5)
    frames = tf["frames"][: a.limit] if a.limit > 0 else tf["frames"]
    ev = albedo.AlbedoEvaluator(mask_thr=a.mask_thr, lpips_vgg=a.lpips_vgg, lpips_lin=a.lpips_lin)
    for i, fr in enumerate(frames):
        pose = torch.from_numpy(nerf_pose(fr["transform_matrix"], a.scale, a.offset))
        kd = harness.albedo_view(W, mat, pose, intr, Hh, Ww, a.ssaa, background=1.0)
        gt_path = os.path.join(a.gt_dir, "test_%03d" % i, "diffuse-color.exr")
        if a.synthetic:
            cover = harness.albedo_view(W, None, pose, intr, Hh, Ww, a.ssaa, gbuffer_consts=dict(kd=(1.0, 1.0, 1.0)))[..., :1]
            gt = torch.cat((torch.clamp(kd * torch.tensor(SYNTHETIC_SCALE, device=kd.device), max=1.0), (cover >= 1.0).float()), dim=-1)
            os.makedirs(os.path.dirname(gt_path), exist_ok=True)
            meters.write_exr(gt_path, gt)
        gt = meters.read_exr(gt_path)
        if gt.shape[:2] != (Hh, Ww) or gt.shape[2] != 4:
            raise SystemExit("%s: %s, expected (%d, %d, 4) RGBA" % (gt_path, gt.shape, Hh, Ww))
        kept = ev.add_view(kd, gt)
        print("[%d/%d] %s: %d of %d pixels masked in" % (i + 1, len(frames), os.path.relpath(gt_path, a.gt_dir), kept, Hh * Ww), flush=True)
    scale = ev.scale()
    albedo.write_scale(os.path.join(out_dir, "albedo_scale.json"), scale, ev.count, a.mask_thr)
    print("albedo scale (median of gt / albedo over %d pixels of %d views, mask_thr %g): x %r  y %r  z %r" % ((ev.count, len(frames), a.mask_thr) + scale))
    save = lambda i, p8, g8: meters.write_png(os.path.join(out_dir, "gammaed_scaled_kd_%d.png" % i), p8.cpu().numpy())
    res = ev.score(scale, on_view=save)
    for i, r in enumerate(res["views"]):
        print("view %d: " % i + "  ".join("%s %.6f" % kv for kv in r.items()), flush=True)
    print("aligned albedo, mean of %d views: " % len(frames) + "  ".join("%s %.6f" % kv for kv in res["mean"].items()))
    print("wrote %s" % os.path.join(out_dir, "albedo_scale.json"))


if __name__ == "__main__":
    main()
