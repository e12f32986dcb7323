"""Where the records go, on the frame's own rays: one line per run for profiles/sah_bottom_counts.txt.

    MIRRES_PRIVATE_TREE=2|3 [MIRRES_SAH_BOTTOM=64|128|256|512] python3 scripts/sah_bottom_counts.py counts <icosphere|clustered>
        8-spp frame of the bench scene with the counting kernels (ctx.set_instrument(1), as bench.py's traversal_roofline): records, box tests and leaves per ray
        of the shadow-ray and the ordered closest-hit kernel; reachable 4-wide nodes and levels of the layout.
    python3 scripts/sah_bottom_counts.py upgrade <icosphere|clustered> [--root DIR]
        HIP events around mirres_bvh_upgrade on a fresh level-1 build, median of 20 (MIRRES_PRIVATE_TREE unset). --root: another checkout of the project
        (the parent commit, whose upgrade stops at level 2)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    what, mesh = sys.argv[1], sys.argv[2]
    import numpy as np
    import torch
    import bench
    import mirres_restir_nerf_mesh_amd as M
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    from mirres_restir_nerf_mesh_amd._lib import lib
    S = M.scene
    dev = torch.device("cuda", 0)
    v, t = S.mesh_by_name(mesh, 7)
    W = RR.restirbvhWorker(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev))
    W.update_mesh(W.vrt, W.v_ind)
    tag = "%-9s tree %s L %s" % (mesh, os.environ.get("MIRRES_PRIVATE_TREE", "auto"), os.environ.get("MIRRES_SAH_BOTTOM", "default"))
    if what == "upgrade":
        ms = []
        for _ in range(21):
            W.update_mesh(W.vrt, W.v_ind)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); W.upgrade(); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = sorted(ms[1:])
        level = getattr(lib(), "mirres_bvh_tree_level", lib().mirres_bvh_private_level)(W.h)
        print("%s: mirres_bvh_upgrade to level %d: median %.3f ms (min %.3f, max %.3f) of 20  [%s]" % (tag, level, ms[len(ms) // 2], ms[0], ms[-1], ROOT))
        return
    mlp = bench.make_field(S, torch, dev)
    g = harness.build_gbuffer(W, 800, 800, 2, mlp_mat=mlp)
    env = torch.from_numpy(S.make_env(256, 512)).to(dev)
    ctx = get_ctx(g["fx"], g["fy"], max_bounce=2)
    ctx.set_instrument(1); ctx.stats(reset=True)
    RR.render_fused(ctx, W, mlp, False, (1, 1, 1), env, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"], g["pos"], 8, 2, 2, 2.0, 0.1, 0.001, 12345)
    torch.cuda.synchronize()
    st = ctx.stats(reset=True); ctx.set_instrument(0)
    from test_gpu_layout import check_layout, fetch_layout
    nodes, leaves, top = fetch_layout(W)
    lay = check_layout(nodes, leaves, top, len(t), v, t, W.LBVHNode_info.cpu().numpy(), W.LBVHNode_aabb.cpu().numpy())
    ra, rc = max(1, st["rays_any"]), max(1, st["rays_closest"])
    print("%s: shadow rays %d: records %.3f box tests %.3f leaves %.3f wave-it/ray %.4f | closest rays %d: records %.3f box tests %.3f leaves %.3f | reachable nodes %d levels %d unused %d | "
          "stack any %d closest %d overflow %d" % (tag, st["rays_any"], st["entered"] / ra, st["popped"] / ra, st["leaves"] / ra, st["any_wave_iters"] / ra, st["rays_closest"],
                                                    st["cl_entered"] / rc, st["cl_popped"] / rc, st["cl_leaves"] / rc, lay["reachable_nodes"], lay["levels"], lay["unused_entries"],
                                                    st["any_max_stack"], st["cl_max_stack"], st["any_stack_overflow"]))


if __name__ == "__main__":
    main()
