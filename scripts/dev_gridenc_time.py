"""Times the stand-alone grid encoder (csrc/gridenc.hip; encoding.GridEncoder) through the C ABI on preallocated tensors, with the method of dev_radiance_time.py:
windows of --inner back-to-back launches between two device events, the cases taking turns within each of --reps rounds, one warm-up each.
  reference configuration (D = 3, C = 2, 16 levels, base 16, 2^19, hash, align_corners False, linear), 2^20 points uniform in the ball of radius 0.6, seeded random
  table: forward, table backward, input backward — and in the same rounds the fused kernels on the same points: mirres_density_points with features (encoder +
  sigma head), RadianceField.forward, backward_points (the whole adjoint with the table scatter) and backward_pos;
  one other configuration, C = 4 (otherwise the same): forward, table backward, input backward.
The table backward's atomic requests: one per (point, level, corner) — an entry's C * 4 <= 32 bytes are one sector — against the 21 G requests/s of
scripts/ubench/atomic_rate.hip.  A record for DESIGN.md section 5.18, not a gate: no thresholds.

    python scripts/dev_gridenc_time.py [--reps 7] [--inner 20] [--points 1048576] [--out profiles/gridenc_time.json]
"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_radiance_time import alternating  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=7); p.add_argument("--inner", type=int, default=20); p.add_argument("--points", type=int, default=1 << 20)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import torch
    from mirres_restir_nerf_mesh_amd import stage0, encoding
    from mirres_restir_nerf_mesh_amd._lib import lib, check, ptr, stream_ptr
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    L = lib()
    n = a.points
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    v = torch.randn((n, 3), generator=g, device="cuda")
    ball = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()
    d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    gs = torch.randn(n, generator=g, device="cuda"); grgb = torch.randn((n, 3), generator=g, device="cuda")
    res = {"points": n, "reps": a.reps, "inner": a.inner, "atomic_request_roof_per_s": 21.0e9}

    def encoder_cases(level_dim, tag):
        enc, dim = encoding.get_encoder("hashgrid", level_dim=level_dim)
        enc.cuda()
        with torch.no_grad():
            enc.embeddings.copy_(torch.randn(tuple(enc.embeddings.shape), generator=g, device="cuda"))
        table = enc.embeddings.detach()
        out = torch.empty((n, dim), device="cuda"); go = torch.randn((n, dim), generator=g, device="cuda")
        gt = torch.zeros_like(table); gp = torch.empty((n, 3), device="cuda")
        lay = C.byref(enc._layout)
        fwd = lambda: check(L.mirres_grid_encode_fwd(lay, ptr(table), ptr(ball), n, 1.0, 16, ptr(out), stream_ptr()), "fwd")
        bt = lambda: check(L.mirres_grid_encode_bwd(lay, ptr(table), ptr(ball), n, 1.0, 16, ptr(go), ptr(gt), None, stream_ptr()), "bwd table")
        bp = lambda: check(L.mirres_grid_encode_bwd(lay, ptr(table), ptr(ball), n, 1.0, 16, ptr(go), None, ptr(gp), stream_ptr()), "bwd pos")
        return enc, {tag + "_forward_ms": fwd, tag + "_table_backward_ms": bt, tag + "_input_backward_ms": bp}

    enc2, cases = encoder_cases(2, "gridenc_c2")
    net, total = stage0.density_layout(1.0)
    rnd = stage0.RadianceField(enc2.embeddings.detach().clone(), *(torch.randn(s, generator=g, device="cuda") * 0.15 for s in ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))),
                               bound=1.0)
    grads = [torch.zeros_like(getattr(rnd, k)) for k in rnd.PARAMETER_NAMES]
    cases.update({"fused_density_points_with_features_ms": lambda: rnd._points(ball, True), "fused_radiance_forward_ms": lambda: rnd.forward(ball, d),
                  "fused_radiance_backward_points_ms": lambda: rnd.backward_points(ball, d, gs, grgb, grads=grads),
                  "fused_radiance_backward_pos_ms": lambda: rnd.backward_pos(ball, d, gs, grgb)})
    assert torch.equal(enc2(ball[:4096]).detach(), rnd.encode(ball[:4096]))            # the two paths on these points: the same bits
    r = alternating(cases, a.reps, a.inner)
    res.update(r)
    # where the table backward's time goes: the first max_level levels alone (the coarse levels take every point's adds on a few thousand entries)
    table2 = enc2.embeddings.detach(); go2 = torch.randn((n, 32), generator=g, device="cuda"); gt2 = torch.zeros_like(table2); lay2 = C.byref(enc2._layout)
    by_level = {"levels_%02d" % ml: (lambda ml=ml: check(L.mirres_grid_encode_bwd(lay2, ptr(table2), ptr(ball), n, 1.0, ml, ptr(go2), ptr(gt2), None, stream_ptr()), "bwd table"))
                for ml in (1, 2, 3, 5, 8, 12, 16)}
    res["gridenc_c2_table_backward_first_levels_ms"] = {k: t[0] for k, t in alternating(by_level, a.reps, a.inner).items()}
    enc4, cases4 = encoder_cases(4, "gridenc_c4")
    r4 = alternating(cases4, a.reps, a.inner)
    res.update(r4)
    req = n * 16 * 8
    for tag in ("gridenc_c2", "gridenc_c4"):
        t = res[tag + "_table_backward_ms"][0] * 1e-3
        res[tag + "_table_backward_requests_per_s"] = req / t
        res[tag + "_table_backward_share_of_roof"] = req / t / 21.0e9
        res[tag + "_forward_gathers_per_s"] = req / (res[tag + "_forward_ms"][0] * 1e-3)
        res[tag + "_forward_Mpoints_per_s"] = n / res[tag + "_forward_ms"][0] / 1e3
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
