"""Where the time of the stage-1 mesh export goes (mirres_restir_nerf_mesh_amd/export.py): device time per bake stage (HIP events around each stage
of bake_textures) and host time of the atlas, the field-input compaction's host side, PNG encoding (zlib) and OBJ formatting, for one cascade at
--texture_size / --ssaa (default 4096 / 2, the reference's defaults: an 8192 x 8192 bake grid).  Meshes: `sphere` = scene.make_mesh(7, 64) (the
bench mesh, 335,872 triangles), `clustered` = scene.make_mesh_clustered() (~3e5 triangles in many small parts).  The material field is a randomly
initialised MLPTexture3D (its cost does not depend on the weights).  Kernel rows: run this under `rocprofv3 --kernel-trace --stats -- python ...`
in a run of its own.

    python scripts/dev_export_time.py [--mesh sphere clustered --atlas {pairs,charts} --texture_size 4096 --ssaa 2 --repeat 2 --out <dir for the files> --json X.json]"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
import mirres_restir_nerf_mesh_amd as M
from mirres_restir_nerf_mesh_amd import export as EX, meters, checkpoint as CK
from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D


def field_module():
    aabb, mn, mx = CK.material_field_args(CK.resolve_material_config(CK.material_config(bound=1.0)))
    torch.manual_seed(0)
    return MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()), seed=1)


def one(name, v, f, mlp, size, ssaa, repeat, out, atlas="pairs"):
    row = {"mesh": name, "V": int(v.shape[0]), "T": int(f.shape[0]), "texture": size, "ssaa": ssaa, "atlas": atlas}
    if atlas == "charts":
        for it in range(repeat):                   # as below: the last run is reported
            torch.cuda.synchronize(); t0 = time.perf_counter()
            vt, ft, info = EX.chart_atlas(v, f, size, size, ssaa)
            torch.cuda.synchronize(); total = time.perf_counter() - t0
        # host = the shelf packing and the fallback cells (numpy); device = everything else: kernels, torch's sorts and uniques, the copies of the results
        row["host_atlas_s"] = info["host_s"]; row["device_atlas_s"] = total - info["host_s"]; fill = info["fill"]
        row.update({k: info[k] for k in ("density", "n_charts", "fallback_faces", "seam_edges")})
    else:
        t0 = time.perf_counter(); vt, ft, fill = EX.uv_atlas(v, f, size, size); row["host_atlas_s"] = time.perf_counter() - t0
        row["device_atlas_s"] = 0.0; row["seam_edges"] = EX.seam_edges(f, ft)
    row["atlas_fill"] = fill
    for it in range(repeat):                       # the first run pays allocator growth and first-launch costs; the last one is reported
        ev = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = EX.bake_textures(mlp.sample_no_di, v, f, vt, ft, size, size, ssaa, events=ev)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    stages = {}
    for (a, ea, ha), (b, eb, hb) in zip(ev[:-1], ev[1:]):
        stages[b] = {"device_ms": ea.elapsed_time(eb), "host_enqueue_ms": 1e3 * (hb - ha)}
    row["bake_stages"] = stages
    row["bake_device_ms"] = ev[0][1].elapsed_time(ev[-1][1])
    row["bake_wall_s"] = wall
    row["texel_coverage"] = r["fill"]
    t0 = time.perf_counter(); imgs = [x.cpu().numpy() for x in r["feat"]]; row["host_copy_back_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for k, im in enumerate(imgs):
        meters.write_png(os.path.join(out, "feat%d_0.png" % k), im)
    row["host_png_s"] = time.perf_counter() - t0
    row["png_bytes"] = sum(os.path.getsize(os.path.join(out, "feat%d_0.png" % k)) for k in (0, 1))
    t0 = time.perf_counter(); EX.write_obj(os.path.join(out, "mesh_0.obj"), v, vt, f, ft); EX.write_mtl(os.path.join(out, "mesh_0.mtl"))
    row["host_obj_s"] = time.perf_counter() - t0
    row["obj_bytes"] = os.path.getsize(os.path.join(out, "mesh_0.obj"))
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mesh", nargs="+", default=["sphere", "clustered"]); p.add_argument("--texture_size", type=int, default=4096)
    p.add_argument("--ssaa", type=int, default=2); p.add_argument("--repeat", type=int, default=2); p.add_argument("--out", default=None)
    p.add_argument("--json", default=None); p.add_argument("--atlas", choices=("pairs", "charts"), default="pairs")
    a = p.parse_args()
    mlp = field_module()
    rows = []
    for name in a.mesh:
        v, f = M.scene.make_mesh(7, 64) if name == "sphere" else M.scene.make_mesh_clustered()
        out = a.out or tempfile.mkdtemp(prefix="export_time_")
        os.makedirs(out, exist_ok=True)
        row = one(name, v, f, mlp, a.texture_size, a.ssaa, a.repeat, out, a.atlas)
        rows.append(row)
        print("%s: T=%d, %d^2 x ssaa %d, atlas fill %.3f, texel coverage %.3f" % (name, row["T"], a.texture_size, a.ssaa, row["atlas_fill"], row["texel_coverage"]))
        print("  %s atlas: device %.3f s, %d seam edges%s" % (a.atlas, row["device_atlas_s"], row["seam_edges"], "" if a.atlas == "pairs" else
              ", density %.1f, %d charts, %d fallback faces" % (row["density"], row["n_charts"], row["fallback_faces"])))
        print("  host  atlas %.3f s | copy back %.3f s | PNG x2 %.3f s (%.1f MB, zlib level 6) | OBJ %.3f s (%.1f MB)" % (
            row["host_atlas_s"], row["host_copy_back_s"], row["host_png_s"], row["png_bytes"] / 1e6, row["host_obj_s"], row["obj_bytes"] / 1e6))
        print("  device bake %.2f ms (wall %.3f s):" % (row["bake_device_ms"], row["bake_wall_s"]))
        for k, s in row["bake_stages"].items():
            print("    %-13s %9.3f ms device  (%7.3f ms host between events)" % (k, s["device_ms"], s["host_enqueue_ms"]))
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
