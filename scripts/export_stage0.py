"""Stage-0 mesh extraction on the HIP path (the reference's NeRFRenderer.export_stage0, nerf/renderer.py:498-570): writes `<workspace>/mesh_stage0/mesh_0.ply`, the
file train_stage1.py, evaluate.py, export_stage1.py and albedo_eval.py start from.

    python scripts/export_stage0.py --workspace <ws> [--ckpt <ws>/checkpoints/ngp_stage0_epXXXX.pth] [--density_thresh 10]        # the S^3 density grid (S = 128)
    python scripts/export_stage0.py --workspace <ws> [--ckpt ...] --mcubes_reso 512 [--bound 1]                                    # the checkpoint's density network, as the reference
    python scripts/export_stage0.py --workspace <ws> --volume sigma_512.npy [--ckpt ...] [--iso v] [--sdf]                         # a dense volume from elsewhere
    python scripts/export_stage0.py --workspace <ws> --mesh foreign.ply --transforms <data>/transforms_train.json                  # cull, clean and decimate only
    python scripts/export_stage0.py --synthetic [--workspace <ws>]                                                                 # analytic volume, smoke run
    python scripts/export_stage0.py --synthetic --network [--mcubes_reso 48]                                                       # a synthetic checkpoint's network, end to end
    python scripts/export_stage0.py --workspace <ws> --bound 2 --outer_meshes [--env_reso 256]                                     # + mesh_1.ply ...: the outer cascades of bound > 1
    python scripts/export_stage0.py --synthetic --bound 2 --outer_meshes                                                           # a synthetic 2-cascade checkpoint's grid, smoke run

Exactly one geometry source.  The checkpoint (default: the latest stage-0 checkpoint of the workspace): its density grid, or with `--mcubes_reso R` (the
reference's flag, 512 in its main.py; unset: the grid) its density network evaluated on the R^3 lattice of [-1, 1]^3 on the HIP path (stage0.DensityField: torch-ngp
hash-grid encoder + sigma_net + exp in fp32), masked by the grid and cut at min(mean_density, density_thresh).  `--bound` (default 1) is the --bound the checkpoint
was trained with: it fixes the hash-grid layout and is checked against the checkpoint's offsets; tiny-cuda-nn checkpoints are not supported.  Or `--volume` (a
[R, R, R] float .npy from elsewhere, e.g. a signed distance, which the density network cannot give; with `--ckpt` and without `--sdf` it is masked by the
checkpoint's grid and cut at min(mean_density, density_thresh),
otherwise at `--iso` / `--density_thresh`; `--sdf`: a signed distance, extracted as (-volume, 0)), or `--mesh`.  `--transforms` (with --H/--W/--downscale/--scale/
--offset as in evaluate.py) gives the training cameras of the visibility cull (--mesh_visibility_culling, which -O switches on); without it nothing is culled.
Above `--decimate_target` triangles (default 3e5 as in the reference's main.py; 0 switches it off) the cleaned mesh is decimated to it by quadric edge collapse
(stage0.decimate_mesh: deterministic rounds of independent collapses, the result has the target's face count or one less; `--no_optimal_placement` places a
collapsed vertex at the cheapest of the two end points and their midpoint instead of the quadric's minimum).  This holds for `--mesh` as well.
`--outer_meshes` (a checkpoint trained with `--bound` > 1, whose density grid has 1 + ceil(log2(bound)) cascades): after mesh_0.ply the reference's outer meshes
mesh_1.ply ... (nerf/renderer.py:632-698) are written, one per outer cascade, from the cascade's density grid resampled to `--env_reso`^3 (the reference's flag,
256), without the centre the cascades before it cover, decimated to half of --decimate_target and culled after decimation; a cascade with nothing left is skipped.
It conflicts with --sdf (the contracted outer mesh is not built), --volume and --mesh.  evaluate.py / train_stage1.py read the result with --cascade."""
import argparse, glob, json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workspace"); p.add_argument("--ckpt", default=None); p.add_argument("--density_thresh", type=float, default=10.0)
    p.add_argument("--volume", default=None); p.add_argument("--iso", type=float, default=None); p.add_argument("--sdf", action="store_true")
    p.add_argument("--mesh", default=None, help="a foreign mesh (PLY): visibility cull, cleaning and decimation only")
    p.add_argument("--transforms", default=None); p.add_argument("--H", type=int, default=800); p.add_argument("--W", type=int, default=800)
    p.add_argument("--downscale", type=int, default=1); p.add_argument("--scale", type=float, default=1.0); p.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    p.add_argument("--visibility_mask_dilation", type=int, default=5); p.add_argument("--clean_min_f", type=int, default=8); p.add_argument("--clean_min_d", type=float, default=5)
    p.add_argument("--decimate_target", type=float, default=3e5, help="decimate the cleaned mesh to this many triangles when it has more (0: never)")
    p.add_argument("--no_optimal_placement", action="store_true", help="decimation: the cheapest of the end points and the midpoint instead of the quadric's minimum")
    p.add_argument("--out", default=None); p.add_argument("--overwrite", action="store_true"); p.add_argument("--synthetic", action="store_true")
    p.add_argument("--resolution", type=int, default=64, help="--synthetic: the analytic volume's resolution")
    p.add_argument("--mcubes_reso", type=int, default=None, help="evaluate the checkpoint's density network on this lattice (the reference's flag; unset: the density grid)")
    p.add_argument("--bound", type=float, default=1.0, help="the --bound the checkpoint was trained with (fixes the hash-grid layout)")
    p.add_argument("--network", action="store_true", help="--synthetic: a synthetic checkpoint's density network instead of the analytic volume")
    p.add_argument("--outer_meshes", action="store_true", help="also write mesh_1.ply ... for the outer cascades of a checkpoint trained with --bound > 1")
    p.add_argument("--env_reso", type=int, default=256, help="--outer_meshes: the resolution an outer cascade's grid is resampled to (the reference's flag)")
    return p


def latest_stage0_checkpoint(workspace):
    files = sorted(glob.glob(os.path.join(workspace, "checkpoints", "*stage0*.pth")))
    return files[-1] if files else None


def parse_args(argv=None):
    """Validates what can be validated without a device: conflicting sources, missing inputs, an existing mesh_0.ply without --overwrite."""
    p = build_parser()
    a = p.parse_args(argv)
    if a.mcubes_reso is not None:
        if a.mesh or a.volume or a.sdf:
            p.error("--mcubes_reso queries the checkpoint's density network: it conflicts with --mesh, --volume and --sdf (a density is no signed distance)")
        if a.mcubes_reso < 2:
            p.error("--mcubes_reso %d: at least 2" % a.mcubes_reso)
        if a.synthetic and not a.network:
            p.error("--mcubes_reso with --synthetic needs --network (the analytic volume's size is --resolution)")
    if a.network and not a.synthetic:
        p.error("--network belongs to --synthetic")
    if not (a.bound > 0):
        p.error("--bound %g: a positive number" % a.bound)
    if a.outer_meshes:
        if a.mesh or a.volume or a.sdf:
            p.error("--outer_meshes reads the checkpoint's density grid: it conflicts with --mesh, --volume and --sdf (the contracted outer mesh is not built)")
        if a.synthetic and a.network:
            p.error("--outer_meshes with --synthetic uses the synthetic checkpoint's grid: drop --network (its hash grid is laid out for bound 1)")
        if not (2 <= a.env_reso <= 1024):
            p.error("--env_reso %d: between 2 and 1024" % a.env_reso)
        if a.synthetic and a.bound > 4:
            p.error("--synthetic --outer_meshes: --bound at most 4 (three cascades)")
    if a.synthetic:
        if a.mesh or a.volume or a.ckpt:
            p.error("--synthetic is a geometry source of its own: drop --mesh / --volume / --ckpt")
        a.workspace = a.workspace or tempfile.mkdtemp(prefix="stage0_ws_")
    if not a.workspace and not a.out:
        p.error("--workspace (or --out) is required")
    if a.mesh and (a.volume or a.ckpt):
        p.error("--mesh (cull and clean only) conflicts with --volume / --ckpt: give one geometry source")
    if a.sdf and not a.volume:
        p.error("--sdf needs --volume (a checkpoint's density grid is not a signed distance)")
    if a.sdf and a.iso is not None:
        p.error("--sdf extracts the zero level: --iso conflicts with it")
    if a.iso is not None and a.mesh:
        p.error("--iso has no meaning with --mesh")
    if not (a.synthetic or a.mesh or a.volume or a.ckpt):
        a.ckpt = latest_stage0_checkpoint(a.workspace) if a.workspace else None
        if a.ckpt is None:
            p.error("no stage-0 checkpoint under %s/checkpoints: give --ckpt, --volume, --mesh or --synthetic" % a.workspace)
    for f in (a.ckpt, a.volume, a.mesh, a.transforms):
        if f and not os.path.exists(f):
            p.error("%s does not exist" % f)
    a.out = a.out or os.path.join(a.workspace, "mesh_stage0")
    if os.path.exists(os.path.join(a.out, "mesh_0.ply")) and not a.overwrite:
        p.error("%s exists: pass --overwrite to replace it" % os.path.join(a.out, "mesh_0.ply"))
    if a.outer_meshes and not a.overwrite:
        old = sorted(f for f in glob.glob(os.path.join(a.out, "mesh_[1-9].ply")))
        if old:
            p.error("%s exists: pass --overwrite to replace it" % old[0])
    return a


def cameras_of(a):
    """(mvps, H, W) of the transforms file, as albedo_eval.py / evaluate.py read it."""
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import harness
    from evaluate import nerf_pose
    tf = json.load(open(a.transforms))
    Hh, Ww = int(tf.get("h", a.H)) // a.downscale, int(tf.get("w", a.W)) // a.downscale
    focal = 0.5 * Ww / np.tan(0.5 * tf["camera_angle_x"])
    intr = (focal, focal, Ww * 0.5, Hh * 0.5)
    mvps = [harness.mvp_from_pose(torch.from_numpy(nerf_pose(fr["transform_matrix"], a.scale, a.offset)).cuda(), intr, Hh, Ww) for fr in tf["frames"]]
    return mvps, Hh, Ww


def main(argv=None):
    a = parse_args(argv)
    import numpy as np, torch
    from mirres_restir_nerf_mesh_amd import stage0, checkpoint as CK
    torch.cuda.set_device(0)
    log = lambda m: print(m, flush=True)
    kw = dict(density_thresh=a.density_thresh, iso=a.iso, sdf=a.sdf, dilation=a.visibility_mask_dilation, min_f=a.clean_min_f, min_d=a.clean_min_d,
              decimate_target=a.decimate_target, optimalplacement=not a.no_optimal_placement, overwrite=a.overwrite, log=log)
    if a.outer_meshes:
        kw.update(outer=True, env_reso=a.env_reso, bound=a.bound)
    if a.synthetic and a.outer_meshes:
        kw["ckpt"] = stage0.synthetic_checkpoint(cascades=CK.cascade_of_bound(a.bound))
    elif a.synthetic and a.network:
        kw["ckpt"] = stage0.synthetic_checkpoint(); kw["resolution"] = a.mcubes_reso if a.mcubes_reso is not None else 48
    elif a.synthetic:
        kw["volume"] = stage0.synthetic_volume(a.resolution, sdf=a.sdf)
    elif a.mesh:
        kw["mesh"] = CK.read_ply(a.mesh)
    else:
        if a.ckpt:
            kw["ckpt"] = torch.load(a.ckpt, map_location="cpu", weights_only=False)
            if a.mcubes_reso is not None:
                kw["resolution"] = a.mcubes_reso; kw["bound"] = a.bound
        if a.volume:
            kw["volume"] = np.load(a.volume)
    if a.transforms:
        kw["cameras"] = cameras_of(a)
    else:
        log("[INFO] no --transforms: the visibility cull is skipped")
    return stage0.export_stage0(a.out, **kw)


if __name__ == "__main__":
    main()
