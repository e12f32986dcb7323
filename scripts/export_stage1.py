"""Stage-1 textured mesh export of a workspace (Trainer.export_stage1(resolution=opt.texture_size), nerf/utils.py:1271-1281; run by the reference
at the end of training, main.py:314-315, and by `--test` unless `--test_no_mesh`, main.py:256-258): per mesh cascade `mesh_{cas}.obj` / `.mtl` and
the baked material textures `feat0_{cas}.png` (kd, the MTL's map_Kd) and `feat1_{cas}.png` (channels 3-5), on the HIP bake (csrc/bake.hip).

    python scripts/export_stage1.py --workspace <ws> --ckpt <ws>/checkpoints/ngp_stage1_ep0100.pth \
        [--texture_size 4096 --ssaa 2 --bound 2 --cascade N --atlas {pairs,charts} --uv_obj A.obj [B.obj ...] --out <ws>/mesh_stage1 --synthetic]

The checkpoint is read exactly as scripts/evaluate.py reads it (stage-0 mesh + stage-1 vertex offsets, material field with the training run's
constants: `--bound`, `--roughness_min`, `--me_max`, `--kd_min`, `--kd_max`).  `--uv_obj`: bake onto UV layouts made elsewhere (one OBJ per cascade,
whose faces are the cascade's triangles) instead of the built-in atlas, which `--atlas` selects (default: the pair atlas).  `--synthetic` exports scripts/evaluate.py's throw-away workspace, made in a
new temporary directory unless `--workspace` names one."""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch
from mirres_restir_nerf_mesh_amd import checkpoint as CK, export as EX
from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D


def load(workspace, ckpt, cascade=None, **material):
    """(vertices + offsets f32[V,3] on the device, triangles, v_cumsum, f_cumsum, material field) as scripts/evaluate.py builds them."""
    ck = CK.read_checkpoint(ckpt)
    cfg = CK.resolve_material_config(ck.get("material_config"), **material)
    cascade = cascade if cascade is not None else CK.cascade_of_bound(cfg["bound"])
    v, t, v_cumsum, f_cumsum = CK.load_stage0_mesh(workspace, cascade)
    aabb, mn, mx = CK.material_field_args(cfg)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()))
    voff, _ = CK.apply_checkpoint(ck, mlp, n_vertices=v.shape[0])
    verts = torch.from_numpy(v).cuda() + (voff if voff is not None else 0)       # act_voffsets is the identity (nerf/utils.py:341-346)
    return verts, t, v_cumsum, f_cumsum, mlp


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--workspace"); p.add_argument("--ckpt"); p.add_argument("--out")
    p.add_argument("--texture_size", type=int, default=4096, help="main.py --texture_size: h0 = w0 of the first cascade")
    p.add_argument("--ssaa", type=int, default=2, help="main.py --ssaa: the bake runs at texture_size x ssaa and is downsampled")
    p.add_argument("--cascade", type=int, default=None, help="mesh cascades; default 1 + ceil(log2(bound)) as nerf/renderer.py:97")
    p.add_argument("--bound", type=float, default=None); p.add_argument("--roughness_min", type=float, default=None)
    p.add_argument("--me_max", type=float, default=None)
    p.add_argument("--kd_min", type=float, nargs=3, default=None); p.add_argument("--kd_max", type=float, nargs=3, default=None)
    p.add_argument("--uv_obj", nargs="+", default=None, help="OBJ files (one per cascade) whose texture coordinates to bake onto")
    p.add_argument("--atlas", choices=("pairs", "charts"), default="pairs", help="the built-in UV atlas: triangle pairs (export.uv_atlas) or axis-projected charts (export.chart_atlas)")
    p.add_argument("--synthetic", action="store_true")
    a = p.parse_args(argv)
    if a.texture_size <= 0 or a.ssaa < 1:
        p.error("--texture_size must be > 0 and --ssaa >= 1")
    if a.synthetic:
        from evaluate import synthetic_workspace
        a.workspace = a.workspace or tempfile.mkdtemp(prefix="mirres_export_ws_")
        a.ckpt, _ = synthetic_workspace(a.workspace, 32, 32)
    if not (a.workspace and a.ckpt):
        p.error("--workspace and --ckpt are required (or --synthetic)")
    verts, t, v_cumsum, f_cumsum, mlp = load(a.workspace, a.ckpt, a.cascade, bound=a.bound, roughness_min=a.roughness_min, me_max=a.me_max,
                                             kd_min=a.kd_min, kd_max=a.kd_max)
    uv = None
    if a.uv_obj:
        if len(a.uv_obj) != len(v_cumsum) - 1:
            p.error("--uv_obj: %d files for %d cascades" % (len(a.uv_obj), len(v_cumsum) - 1))
        uv = [EX.uv_from_obj(path, t[f_cumsum[c]:f_cumsum[c + 1]] - v_cumsum[c]) for c, path in enumerate(a.uv_obj)]
    out = a.out or os.path.join(a.workspace, "mesh_stage1")
    t0 = time.perf_counter()
    files = EX.export_stage1(out, verts, t, v_cumsum, f_cumsum, mlp, texture_size=a.texture_size, ssaa=a.ssaa, uv=uv, atlas=a.atlas)
    print("[export] %d files in %s (%.1f s)" % (len(files), out, time.perf_counter() - t0))
    return files


if __name__ == "__main__":
    main()
