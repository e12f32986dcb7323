"""Times stage0.DensityField.volume(R) (csrc/density.hip; default R = 512, the reference's --mcubes_reso) on the reference's bound-1 hash-grid configuration with a
seeded random table: unmasked, and masked by a ball's occupancy grid (128^3, radius 0.5) — and the same volume by plain torch operations on the same device in
chunks of 128^3 points, as NeRFRenderer.export_stage0 walks its lattice (nerf/renderer.py:518-529).  Device events around the launches, one warm-up per shape, the
median of --reps runs.  A record for DESIGN.md section 5.11, not a gate: there is no earlier path to compare with.

    python scripts/dev_density_time.py [--resolution 512] [--reps 5] [--no_torch] [--out file.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)


def torch_volume(field, R, chunk=128):
    """The same query by torch operations (fp32; gathers by index, two matmuls, exp), chunked like the reference."""
    import torch
    net = field.net; dev = field.table.device
    M = 0xFFFFFFFF
    ax = torch.linspace(-1, 1, R).to(dev)
    out = torch.empty((R, R, R), dtype=torch.float32, device=dev)
    for x0 in range(0, R, chunk):
        for y0 in range(0, R, chunk):
            for z0 in range(0, R, chunk):
                xs, ys, zs = ax[x0:x0 + chunk], ax[y0:y0 + chunk], ax[z0:z0 + chunk]
                pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
                u = (pts + field.bound) / (2 * field.bound)
                feats = []
                for l in range(net.num_levels):
                    off, hs, s1 = int(net.offsets[l]), int(net.offsets[l + 1] - net.offsets[l]), int(net.resolution[l]) + 1
                    p = u * float(net.scale[l]) + 0.5
                    cell = torch.floor(p); f = p - cell; c = cell.long()
                    r = torch.zeros((pts.shape[0], 2), dtype=torch.float32, device=dev)
                    for idx in range(8):
                        w = torch.ones(pts.shape[0], dtype=torch.float32, device=dev); cc = []
                        for d in range(3):
                            bit = (idx >> d) & 1
                            w = w * (f[:, d] if bit else 1 - f[:, d]); cc.append(c[:, d] + bit)
                        if net.hashed[l]:
                            index = cc[0] ^ ((cc[1] * 2654435761) & M) ^ ((cc[2] * 805459861) & M)
                        else:
                            index = cc[0] + cc[1] * s1 + cc[2] * (s1 * s1)
                        r = r + w[:, None] * field.table[off + index % hs]
                    feats.append(r)
                h = torch.relu(torch.cat(feats, 1) @ field.w0.t()) @ field.w1
                out[x0:x0 + chunk, y0:y0 + chunk, z0:z0 + chunk] = torch.exp(h).reshape(len(xs), len(ys), len(zs))
    return out


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, default=512); p.add_argument("--reps", type=int, default=5); p.add_argument("--no_torch", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import torch
    from mirres_restir_nerf_mesh_amd import stage0
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    R = a.resolution
    net, total = stage0.density_layout(1.0)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    table = torch.randn((total, 2), generator=g, device="cuda")
    w0 = torch.randn((64, 32), generator=g, device="cuda") * 0.15; w1 = torch.randn((16, 64), generator=g, device="cuda") * 0.15
    field = stage0.DensityField(table, w0, w1, bound=1.0)
    S = 128
    cc = (torch.arange(S, device="cuda", dtype=torch.float32) + 0.5) / S * 2 - 1
    gx, gy, gz = torch.meshgrid(cc, cc, cc, indexing="ij")
    grid = ((gx * gx + gy * gy + gz * gz).sqrt() < 0.5).float().contiguous()
    res = {"resolution": R, "points": R ** 3, "table_entries": total, "reps": a.reps}
    res["unmasked_ms"] = timed(lambda: field.volume(R), a.reps)
    res["masked_ms"] = timed(lambda: field.volume(R, grid, 0.5), a.reps)
    vol = field.volume(R); mvol = field.volume(R, grid, 0.5)
    res["masked_fraction"] = float((mvol == 0).float().mean())
    n = R ** 3
    res["unmasked_Mpoints_per_s"] = n / res["unmasked_ms"][0] / 1e3
    res["unmasked_gathers_per_s"] = n * 128 / (res["unmasked_ms"][0] * 1e-3)
    res["unmasked_head_flops_per_s"] = n * 2 * (64 * 32 + 64) / (res["unmasked_ms"][0] * 1e-3)
    if not a.no_torch:
        res["torch_ms"] = timed(lambda: torch_volume(field, R), max(1, min(a.reps, 2)))
        ref = torch_volume(field, R)
        res["max_rel_diff_to_torch"] = float(((vol - ref).abs() / ref).max())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
