"""Cost of the textured-mesh material source (csrc/texmat.hip): a size x size frame rendered from the exported asset against the same frame from the
material field, and the lookup kernel alone (mirres_texmat_lookup) against the production field lookup (k_mlp_mfma<1, 2> behind
mirres_debug_matnet_scatter_mfma) on the same points — in random order (what indirect hits look like) and sorted by triangle.

    python scripts/dev_texmat_time.py [--size 1600 --spp 32 --texture_size 2048 --reps 3 --n_lookup 4194304]"""
import argparse, ctypes as C, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
import mirres_restir_nerf_mesh_amd as M
from mirres_restir_nerf_mesh_amd import export as EX, harness, renderer_restir as RR, checkpoint as CK
from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
from mirres_restir_nerf_mesh_amd._ops import get_ctx
from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=1600); p.add_argument("--spp", type=int, default=32); p.add_argument("--texture_size", type=int, default=2048)
    p.add_argument("--reps", type=int, default=3); p.add_argument("--n_lookup", type=int, default=1 << 22); p.add_argument("--workspace", default=None)
    a = p.parse_args()
    ws = a.workspace or tempfile.mkdtemp(prefix="texmat_time_")
    v, f = M.scene.make_mesh(5, 16)
    aabb, mn, mx = CK.material_field_args(CK.resolve_material_config(CK.material_config(bound=1.0)))
    torch.manual_seed(0)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    t0 = time.perf_counter()
    EX.export_stage1(os.path.join(ws, "mesh_stage1"), v, f, [0, v.shape[0]], [0, f.shape[0]], mlp, texture_size=a.texture_size, ssaa=2, log=None)
    tex = EX.load_stage1(os.path.join(ws, "mesh_stage1"))
    print("mesh: %d triangles, texture %d^2 (%.1f MiB packed); export + load %.1f s" % (f.shape[0], a.texture_size, tex.planes[0].numel() / 2 ** 20, time.perf_counter() - t0))
    w = RR.restirbvhWorker(tex.verts, tex.tris); w.update_mesh(w.vrt, w.v_ind)
    env = torch.from_numpy(M.scene.make_env(256, 512)).cuda()
    S = a.size
    az, el = np.deg2rad(30.0), np.deg2rad(30.0)
    eye = 3.2 * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    fwd = -eye / np.linalg.norm(eye); right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right); up = np.cross(right, fwd)
    pose = np.eye(4); pose[:3, :3] = np.stack([right, up, -fwd], 1); pose[:3, 3] = eye
    focal = 0.5 * S / np.tan(0.5 * 0.6911); intr = (focal, focal, S * 0.5, S * 0.5)
    ctx = get_ctx(S, S); ctx.reserve()
    res = {}
    for name, mat in (("field", mlp), ("textured", tex)):
        g = harness.build_gbuffer_from_pose(w, torch.from_numpy(pose.astype(np.float32)), intr, S, S, 1, mat)
        run = lambda: RR.render_fused(ctx, w, mat, False, (1.0, 1.0, 1.0), env, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"], g["pos"],
                                      a.spp, 2, 2, 2.0, 0.1, 0.001, 777)
        res[name], ts = timed(run, a.reps)
        print("%s frame %d^2 x %d spp: %.1f ms (median of %s)" % (name, S, a.spp, res[name], ", ".join("%.1f" % t for t in ts)), flush=True)
    print("textured / field frame time: %.3f" % (res["textured"] / res["field"]))
    # the lookup kernels alone on n random surface points
    n = a.n_lookup
    rng = np.random.default_rng(0)
    prim = rng.integers(0, f.shape[0], n)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    pos = np.einsum("nk,nkc->nc", b, v[f[prim]]).astype(np.float32)
    occ = torch.ones(n, device="cuda")
    kd = torch.empty((n, 3), device="cuda"); rm = torch.empty((n, 2), device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda"); cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    L = lib(); L.mirres_debug_matnet_scatter_mfma.restype = C.c_int
    L.mirres_debug_matnet_scatter_mfma.argtypes = [C.c_void_p] * 8 + [C.c_void_p]
    L.mirres_debug_matnet_scatter_mfma.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    mst = mlp._struct(); tst = tex._struct()
    for order in ("random", "sorted by triangle"):
        o = np.argsort(prim, kind="stable") if order != "random" else np.arange(n)
        pr_t = torch.from_numpy(prim[o].astype(np.int32)).cuda(); po_t = torch.from_numpy(pos[o]).cuda()
        t_tex, _ = timed(lambda: check(L.mirres_texmat_lookup(C.byref(tst), occ.data_ptr(), pr_t.data_ptr(), po_t.data_ptr(), n, kd.data_ptr(), rm.data_ptr(), 0, None,
                                                              stream_ptr()), "mirres_texmat_lookup"), 5)
        t_mlp, _ = timed(lambda: check(L.mirres_debug_matnet_scatter_mfma(C.addressof(mst), occ.data_ptr(), po_t.data_ptr(), n, kd.data_ptr(), rm.data_ptr(), idx.data_ptr(),
                                                                          cnt.data_ptr(), stream_ptr()), "mirres_debug_matnet_scatter_mfma"), 5)
        print("lookup of %d points (%s): texture %.3f ms (%.0f Mlookups/s), field list + k_mlp_mfma<1,2> %.3f ms (%.0f M/s)" % (
            n, order, t_tex, n / t_tex / 1e3, t_mlp, n / t_mlp / 1e3), flush=True)


if __name__ == "__main__":
    main()
