"""HIP-event times of the stage-0 extraction's stages on the synthetic volume (stage0.synthetic_volume) at 128^3 and 512^3 -> profiles/stage0_time.txt.

    python scripts/dev_stage0_time.py [--sizes 128 512] [--repeat 5] [--out profiles/stage0_time.txt]

Per size: marching cubes count (classification + both scans + the blocking read of the totals), emit, and the whole call; the six-camera visibility cull
at 800 x 800; cleaning; quadric decimation of the cleaned mesh (to --decimate_target, or to a fifth of its faces when it has fewer than that: one run, per round
the faces, the collapses and the device time of the edge build (the torch sorts, vertex flags, in round 1 the quadrics), k_dec_edge, the candidate cut with
claim / select, and apply with compaction).  Every other figure is the median of `--repeat` runs after one warm-up run, bracketed by events on the work's own stream; next to the
marching-cubes times stands the volume traffic they imply (4 bytes per grid point and pass, two passes) in GB/s.  No speed gate reads this file."""
import argparse, ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from mirres_restir_nerf_mesh_amd import stage0, harness, _lib as L


def timed(fn, repeat):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), out


def decimate_timed(v, t, target):
    """stage0.decimate_mesh's loop with events between the stages of every round -> (v, t, rows of (faces before, collapses, {stage: ms}))."""
    rows, q = [], None
    while t.shape[0] > target and len(rows) < stage0.DEC_MAX_ROUNDS:
        ev = [("start", torch.cuda.Event(enable_timing=True))]; ev[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True); e.record(); ev.append((name, e))
        T0 = t.shape[0]
        v, q, t, info = stage0.decimate_round(v, q, t, target, True, mark)
        torch.cuda.synchronize()
        rows.append((T0, info["selected"], {ev[i][0]: ev[i - 1][1].elapsed_time(ev[i][1]) for i in range(1, len(ev))}))
        if info["selected"] == 0:
            break
    return v, t, rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--decimate_target", type=float, default=3e5)
    p.add_argument("--sizes", type=int, nargs="+", default=[128, 512]); p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage0_time.txt"))
    a = p.parse_args()
    torch.cuda.set_device(0)
    lib = L.lib()
    lines = ["stage-0 extraction, synthetic volume, %s; median (min .. max) of %d runs after a warm-up, HIP events" % (torch.cuda.get_device_name(0), a.repeat)]
    for r in a.sizes:
        vol = stage0.synthetic_volume(r)
        nb = int(lib.mirres_mc_scratch_bytes(r, r, r)); scratch = torch.empty(nb, dtype=torch.uint8, device="cuda"); counts = (C.c_int * 2)()
        count = lambda: L.check(lib.mirres_mc_count(L.ptr(vol), r, r, r, 10.0, L.ptr(scratch), nb, counts, L.stream_ptr()), "mc_count")
        m_c = timed(count, a.repeat)
        V, T = counts[0], counts[1]
        verts = torch.empty((V, 3), device="cuda"); tris = torch.empty((T, 3), dtype=torch.int32, device="cuda")
        emit = lambda: L.check(lib.mirres_mc_emit(L.ptr(vol), r, r, r, 10.0, L.ptr(scratch), L.ptr(verts), V, L.ptr(tris), T, L.stream_ptr()), "mc_emit")
        m_e = timed(emit, a.repeat)
        m_all = timed(lambda: stage0.marching_cubes(vol, 10.0), a.repeat)
        gb = 4.0 * r ** 3 / 1e9
        lines.append("%d^3 (%.1f M points, volume %.3f GB, scratch %.3f GB): V %d, T %d" % (r, r ** 3 / 1e6, gb, nb / 1e9, V, T))
        lines.append("  marching cubes count   %9.3f ms (%.3f .. %.3f)   volume read at %.0f GB/s" % (m_c[0], m_c[1], m_c[2], gb / (m_c[0] * 1e-3)))
        lines.append("  marching cubes emit    %9.3f ms (%.3f .. %.3f)   volume read at %.0f GB/s" % (m_e[0], m_e[1], m_e[2], gb / (m_e[0] * 1e-3)))
        lines.append("  marching_cubes() whole %9.3f ms (%.3f .. %.3f)   incl. scratch / output allocation; volume read twice at %.0f GB/s" % (m_all[0], m_all[1], m_all[2], 2 * gb / (m_all[0] * 1e-3)))
        v = stage0.index_to_world(verts, r)
        f = 0.5 * 800 / np.tan(0.5 * np.radians(50.0))
        mvps = []
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            z = np.array(d, np.float64); up = np.array((0, 0, 1.0)) if abs(z[2]) < 0.5 else np.array((0, 1.0, 0))
            x = np.cross(up, z); x /= np.linalg.norm(x); pose = np.eye(4); pose[:3, 0] = x; pose[:3, 1] = np.cross(z, x); pose[:3, 2] = z; pose[:3, 3] = 3 * z
            mvps.append(harness.mvp_from_pose(torch.from_numpy(pose.astype(np.float32)).cuda(), (f, f, 400.0, 400.0), 800, 800))
        m_s = timed(lambda: stage0.mark_unseen_triangles(v, tris, mvps, 800, 800), a.repeat)
        unseen = m_s[3]
        m_r = timed(lambda: stage0.remove_masked_trigs(v, tris, unseen, 5), a.repeat)
        v2, t2 = m_r[3]
        m_k = timed(lambda: stage0.clean_mesh(v2, t2), a.repeat)
        lines.append("  mark unseen, 6 x 800^2 %9.3f ms (%.3f .. %.3f)   BVH build + 6 rasterised views; %d of %d unseen" % (m_s[0], m_s[1], m_s[2], int(unseen.sum()), T))
        lines.append("  dilate 5 + remove      %9.3f ms (%.3f .. %.3f)   -> V %d, T %d" % (m_r[0], m_r[1], m_r[2], v2.shape[0], t2.shape[0]))
        lines.append("  clean_mesh             %9.3f ms (%.3f .. %.3f)   -> V %d, T %d" % (m_k[0], m_k[1], m_k[2], m_k[3][0].shape[0], m_k[3][1].shape[0]))
        vk, tk = m_k[3]
        target = int(a.decimate_target) if tk.shape[0] > a.decimate_target else tk.shape[0] // 5
        stage0.decimate_mesh(vk, tk, target); torch.cuda.synchronize()                       # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); vd, td, rows = decimate_timed(vk, tk, target); e1.record(); torch.cuda.synchronize()
        tot = {k: sum(r[2].get(k, 0.0) for r in rows) for k in ("edges", "k_dec_edge", "select", "apply")}
        lines.append("  decimate_mesh          %9.3f ms (one run)             T %d -> %d (target %d), V -> %d; %d rounds, collapses first %d, last %d" % (
            e0.elapsed_time(e1), tk.shape[0], td.shape[0], target, vd.shape[0], len(rows), rows[0][1] if rows else 0, rows[-1][1] if rows else 0))
        lines.append("    all rounds: edge build (sorts) %.3f ms, k_dec_edge %.3f ms, cut + claim + select %.3f ms, apply + compact %.3f ms" % (tot["edges"], tot["k_dec_edge"], tot["select"], tot["apply"]))
        for i, (T0, nsel, ms) in enumerate(rows):
            if i < 3 or i >= len(rows) - 2:
                lines.append("    round %3d: T %8d, %7d collapses; edge build %.3f, k_dec_edge %.3f, select %.3f, apply %.3f ms" % (
                    i + 1, T0, nsel, ms.get("edges", 0.0), ms.get("k_dec_edge", 0.0), ms.get("select", 0.0), ms.get("apply", 0.0)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
