"""Dev (GPU box): SHA-256 of the outputs of the fused hash-grid kernels that are reproducible run to run, at the size the timing scripts use — run once per library
build (MIRRES_LIB=...), each in a fresh process, and compare the lines to check that two builds compute the same bits.   python scripts/dev_grid_bits.py
Inputs: 2^20 seeded points uniform in the ball of radius 0.6 with 64 hostile ones in front (the cube's corners and faces, just outside, NaN, inf), seeded unit
directions and cotangents (dev_gridenc_time.py's kind); the synthetic radiance checkpoint with seeded noise added to every table entry, so that every level carries
values that differ from entry to entry.
  * mirres_density_points: features and sigma;
  * mirres_radiance_points: sigma, rgb, h16;
  * mirres_radiance_points_bwd_pos: grad_pos — one lane per point, no atomics;
  * mirres_radiance_points_bwd at max_blocks = 256: the five weight gradients — per-block partial sums added in block order;
  * mirres_grid_tv_grad: the gradient of the DENSE levels — integer counts, then one store per entry.
The table gradients that go through fp32 atomics (mirres_radiance_points_bwd's, and the total variation's on the hashed levels) depend on the order the adds arrive
in and are left out; tests/test_gpu_radiance_bwd.py and tests/test_gpu_grid_tv.py hold them against float64 scatters."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from mirres_restir_nerf_mesh_amd import stage0
sha = lambda t: hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

assert torch.cuda.is_available(), "the kernels need the GPU"
torch.cuda.set_device(0)
n = 1 << 20
g = torch.Generator(device="cuda"); g.manual_seed(7)
v = torch.randn((n, 3), generator=g, device="cuda")
x = (v / v.norm(dim=1, keepdim=True) * 0.6 * torch.rand((n, 1), generator=g, device="cuda") ** (1.0 / 3.0)).contiguous()
e = 1.0 + 2.0 ** -23
hostile = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)] + [[1.0, 0.3, -0.2], [0.1, -1.0, 0.4], [-0.7, 0.2, 1.0], [e, 0.0, 0.0], [0.0, -e, 0.0],
           [0.0, 0.0, 2.0], [float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [0.0, 0.0, 0.0], [-0.0, 1e-30, -1e-30]]
x[:len(hostile)] = torch.tensor(hostile, device="cuda")
d = torch.randn((n, 3), generator=g, device="cuda"); d = (d / d.norm(dim=1, keepdim=True)).contiguous()
gs = torch.randn(n, generator=g, device="cuda"); grgb = torch.randn((n, 3), generator=g, device="cuda")

m = stage0.synthetic_radiance_checkpoint(S=16)["model"]
table = m["encoder.embeddings"].to("cuda", torch.float32)
table = (table + 0.05 * torch.randn(tuple(table.shape), generator=g, device="cuda")).contiguous()
field = stage0.RadianceField(table, m["sigma_net.0.weight"], m["sigma_net.1.weight"], m["color_net.0.weight"], m["color_net.1.weight"], m["color_net.2.weight"], bound=1.0)
offsets = [int(field.net.offsets[l]) for l in range(17)]
assert all(bool((table[offsets[l]:offsets[l + 1]] != 0).any()) for l in range(16))

sigma, feat = field._points(x, True)
print("density_points  n=%d  features %s  sigma %s  (points with features %d)" % (n, sha(feat), sha(sigma), int((feat != 0).any(dim=1).sum())))
sigma, rgb, h16, _ = field._query(x, d, want_aux=True)
print("radiance_points  sigma %s  rgb %s  h16 %s" % (sha(sigma), sha(rgb), sha(h16)))
gp = field.backward_pos(x, d, gs, grgb)
print("radiance_points_bwd_pos  grad_pos %s  (nonzero rows %d)" % (sha(gp), int((gp != 0).any(dim=1).sum())))
grads = field.backward_points(x, d, gs, grgb, max_blocks=256)
print("radiance_points_bwd max_blocks=256  " + "  ".join("%s %s" % (k, sha(t)) for k, t in zip(field.PARAMETER_NAMES[1:], grads[1:])))
dense = max(l + 1 for l in range(16) if not field.net.hashed[l])
assert not any(field.net.hashed[l] for l in range(dense))
gt = torch.zeros_like(table)
field.grad_total_variation(weight=1e-3, inputs=x, grad=gt)
torch.cuda.synchronize()
print("grid_tv_grad  levels 0..%d %s  (entries touched %d of %d)" % (dense - 1, sha(gt[:offsets[dense]]), int((gt[:offsets[dense]] != 0).any(dim=1).sum()), offsets[dense]))
