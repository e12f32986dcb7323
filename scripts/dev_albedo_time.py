"""Where the time of the albedo evaluation goes (mirres_restir_nerf_mesh_amd/albedo.py, csrc/albedo.hip): device time (HIP events) of the masked
compaction of --views synthetic --size^2 views into the pool, of the exact median over the pool and of the per-view score, and beside it the host's
way to the same three numbers: np.median of the float64 ratios of the same pool (the reference's albedo_eval.py:116-118), timed with the host clock
on the machine the script runs on, with and without the copy of the pool to the host.  The views are seeded noise with a disc-shaped mask (about
40 % of the pixels): the select's cost depends on the pool's size, not on what it holds.  Kernel rows: run this under
`rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.

    python scripts/dev_albedo_time.py [--views 200 --size 800 --repeat 5 --median_reps 50 --host_repeat 3 --json X.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from mirres_restir_nerf_mesh_amd import albedo


def make_view(gen, S):
    pred = torch.rand((S, S, 3), generator=gen, device="cuda") * 0.9 + 0.05
    gt = torch.empty((S, S, 4), device="cuda")
    gt[..., :3] = torch.clamp(pred * torch.tensor([0.7, 1.3, 0.9], device="cuda") * (1 + 0.1 * torch.randn((S, S, 3), generator=gen, device="cuda")), 0, 1)
    y, x = torch.meshgrid(torch.arange(S, device="cuda"), torch.arange(S, device="cuda"), indexing="ij")
    gt[..., 3] = (((x - S / 2) ** 2 + (y - S / 2) ** 2) < (0.357 * S) ** 2).float()
    return pred, gt


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    a.record(); r = fn(); b.record()
    torch.cuda.synchronize()
    return r, a.elapsed_time(b), 1e3 * (time.perf_counter() - t0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=200); p.add_argument("--size", type=int, default=800); p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--median_reps", type=int, default=50); p.add_argument("--host_repeat", type=int, default=3)
    p.add_argument("--json", default=None)
    a = p.parse_args()
    gen = torch.Generator(device="cuda"); gen.manual_seed(0)
    views = [make_view(gen, a.size) for _ in range(a.views)]
    row = {"views": a.views, "size": a.size, "rounds": []}
    for it in range(a.repeat + 1):                    # round 0 pays allocator growth and first-launch costs and is not reported
        ev = albedo.AlbedoEvaluator(mask_thr=0.9)
        ev._reserve(a.views * a.size * a.size)        # the pool's growth (a copy per doubling) is allocator work, not the kernels'
        r = {}
        # add_view reads the pool's count back after every view (a blocking 24-byte copy), so the host clock around the loop is the honest figure for the
        # compaction as the package runs it; the events bracket the same loop and can only agree with it
        _, r["compact_device_ms"], r["compact_wall_ms"] = timed(lambda: [ev.add_view(pr, gt) for pr, gt in views])
        scale, r["median_device_ms"], r["median_wall_ms"] = timed(ev.scale)
        _, r["median_x%d_device_ms" % a.median_reps], _ = timed(lambda: [ev.scale() for _ in range(a.median_reps)])      # a longer window: per call = / reps
        _, r["score_device_ms"], r["score_wall_ms"] = timed(lambda: [ev.score_view(pr, gt, scale) for pr, gt in views])
        if it > 0:
            row["rounds"].append(r)
    passes = 9 if ev.count % 2 == 0 else 8
    row["pool_pixels"] = ev.count
    row["median_bytes_needed"] = 24 * ev.count * passes
    row["scale"] = list(scale)
    t0 = time.perf_counter(); pp = ev.pool_pred[: ev.count].cpu().numpy(); pg = ev.pool_gt[: ev.count].cpu().numpy(); row["host_copy_s"] = time.perf_counter() - t0
    row["host_np_median_s"] = []
    for _ in range(a.host_repeat):
        t0 = time.perf_counter(); want = np.median(pg.astype(np.float64) / pp.astype(np.float64).clip(min=1e-6), axis=0); row["host_np_median_s"].append(time.perf_counter() - t0)
    row["equal_to_numpy"] = bool(np.all(want == np.asarray(scale)))
    col = lambda k: [r[k] for r in row["rounds"]]
    span = lambda v: "%.3f / %.3f / %.3f" % (min(v), sorted(v)[len(v) // 2], max(v))
    per_call = [x / a.median_reps for x in col("median_x%d_device_ms" % a.median_reps)]
    print("%d views of %d^2, %d pixels in the pool (%.1f %%); %d timed rounds after one warm-up round, figures are min / median / max over the rounds"
          % (a.views, a.size, ev.count, 100.0 * ev.count / (a.views * a.size ** 2), len(row["rounds"])))
    print("  compaction of the views   %s ms host clock (%s ms between events; one blocking count read per view)" % (span(col("compact_wall_ms")), span(col("compact_device_ms"))))
    print("  median, one call          %s ms between events (%s ms host clock)" % (span(col("median_device_ms")), span(col("median_wall_ms"))))
    print("  median, %3d calls in a row %s ms per call; %d passes need %.2f GB of pool reads per call: %.0f GB/s at the median (bytes needed over event time, not a kernel's share of peak)"
          % (a.median_reps, span(per_call), passes, row["median_bytes_needed"] / 1e9, row["median_bytes_needed"] / sorted(per_call)[len(per_call) // 2] / 1e6))
    print("  score of the views        %s ms between events (%s ms host clock)" % (span(col("score_device_ms")), span(col("score_wall_ms"))))
    print("  host    np.median of the float64 ratios of the same pool %s s over %d runs (+ %.3f s to copy the pool to the host); equal to the device's scale: %s"
          % (span(row["host_np_median_s"]), a.host_repeat, row["host_copy_s"], row["equal_to_numpy"]))
    print("  scale %r" % (tuple(scale),))
    if a.json:
        json.dump(row, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
