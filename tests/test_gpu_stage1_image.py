"""The stage-1 NeRF colour branch (`image`, nerf/renderer.py:1046-1052) through harness.render_stage1_outputs(field=...), losses.stage1_loss,
checkpoint.save_checkpoint(field=...), scripts/train_stage1.py --stage0_ckpt and scripts/evaluate.py --nerf_image: a small icosphere under a dataset camera at
32 x 32 with ssaa 1 and 16 x 16 with ssaa 2, spp 1-2, the frame seed pinned by set_random_offset, the field from init_random on the T = 14 layout (the host's
float64 network then holds a small table).

voffsets.grad: the interpolation and antialias adjoints scatter the vertex gradients with fp32 atomics (csrc/raster.hip, csrc/antialias.hip), so two backward
passes of ONE graph differ in the last bits of voffsets.grad (measured: the first run of this file).  "offset_nerf_grad=False is the run whose positions are
detached by hand" is therefore held bit for bit where no atomic sits between the decision and the check: the cotangent that reaches rgbs has the same bits in both
runs and with the flag set, and the cotangent that reaches the G-buffer's positions is None in both and, with the flag set, backward_pos's bits at the covered
pixels and 0 elsewhere.  What remains of voffsets.grad (dr.antialias's visibility gradient) is one function of those bits in every run; with the flag set
voffsets.grad differs, and by more than the two detached runs differ from each other; those two agree to GRAD_ULPS ulp of the largest entry.

Measured on the MI355X when these tests were written: DESIGN.md section 5.17."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_refs as D                       # noqa: E402
import radiance_bwd_refs as B                  # noqa: E402

LOG2_T = 14
GRAD_ULPS = 64           # voffsets.grad of one graph twice: an entry is an fp32 sum of the m <= 32 pixel contributions of a vertex's triangles at 32 x 32 in two orders,
                         # each within gamma_m sum |terms| of the exact sum: 2 gamma_32 = 64 u, taken of the largest entry (the terms of an entry have its order of magnitude)


class Scene:
    def __init__(self):
        from mirres_restir_nerf_mesh_amd import renderer_restir as RR, raster, scene as scene_mod, stage0
        from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
        torch.manual_seed(0)
        v, t = scene_mod.make_mesh(3, 4)
        self.vt = torch.from_numpy(v).cuda(); self.tt = torch.from_numpy(t).cuda()
        self.W = RR.restirbvhWorker(self.vt, self.tt); self.W.update_mesh(self.W.vrt, self.W.v_ind)
        mn, mx = scene_mod.material_min_max(me_max=0.3)
        self.mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=11)
        with torch.no_grad():
            self.mlp.encoder.params.mul_(2e3)
        self.env = torch.full((32, 64, 3), 0.5, device="cuda")
        a, e = np.deg2rad(30.0), np.deg2rad(30.0)
        eye = 3.2 * np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
        fwd = -eye / np.linalg.norm(eye); right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right); up = np.cross(right, fwd)
        pose = np.eye(4, dtype=np.float32); pose[:3, :3] = np.stack([right, up, -fwd], 1); pose[:3, 3] = eye
        self.pose = torch.from_numpy(pose).cuda()
        self.topo = raster.antialias_topology(self.tt)
        self.field = stage0.RadianceField.init_random(1.0, seed=3, log2_hashmap_size=LOG2_T)
        self.field.bwd_max_blocks = 2
        self.RR = RR

    def intr(self, H, W):
        focal = 0.5 * W / np.tan(0.5 * 0.6911)
        return (focal, focal, W * 0.5, H * 0.5)

    def render(self, H, ssaa, spp, voff=None, seed=77, **kw):
        from mirres_restir_nerf_mesh_amd import harness
        voff = torch.zeros_like(self.vt) if voff is None else voff
        mods = self.RR.load_m_for_restir(H * ssaa, H * ssaa)                        # fresh reservoirs: a frame's temporal pass reads the previous frame's
        self.RR.set_random_offset(seed); torch.manual_seed(7)
        try:
            return harness.render_stage1_outputs(self.W, self.vt, voff, self.tt, self.mlp, self.env, mods, H, H, spp, ssaa, pose=self.pose,
                                                 intrinsics=self.intr(H, H), topology=self.topo, **kw)
        finally:
            self.RR.set_random_offset(None)


@pytest.fixture(scope="module")
def S():
    return Scene()


def _bits(x, y):
    """Equal bits (a NaN equals the same NaN)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def _bg(kind, n):
    return 1.0 if kind == "scalar" else torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).cuda()


@pytest.mark.parametrize("H,ssaa,spp", [(32, 1, 2), (16, 2, 1)])
@pytest.mark.parametrize("bg", ["scalar", "per-pixel"])
def test_image_is_the_composition_and_the_other_outputs_keep_their_bits(S, H, ssaa, spp, bg, monkeypatch):
    from mirres_restir_nerf_mesh_amd import harness, raster
    bgc = _bg(bg, H * H)
    # raster.auto_normals sums a vertex's face normals with index_add_, whose order is not fixed on the GPU: two runs of the EXISTING path then differ in the last
    # bit of the shading normal and by 1 to 3 ulp in the ReSTIR frame (measured, no field in either run).  That source is taken out here — the three runs share the
    # first run's vertex normals — so that "bit-identical with and without field=" can be asked of every argument of the sample loop and of every output.
    import inspect
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    normals = raster.auto_normals
    cache = {}
    monkeypatch.setattr(raster, "auto_normals", lambda v, t: cache.setdefault("n", normals(v, t)))
    loop = RR.run_restir_di_with_pt
    sig = inspect.signature(loop)
    maps = ("env_map", "occ_map", "normal_map", "depth_map", "diffuse_map", "roughness_specular", "ray_dir_map", "pos_map", "framedim_x", "framedim_y", "spp")
    seen = []

    def spy(*a, **k):
        args = sig.bind(*a, **k).arguments
        seen.append({n: args[n].detach().clone() if torch.is_tensor(args[n]) else args[n] for n in maps})
        return loop(*a, **k)
    monkeypatch.setattr(RR, "run_restir_di_with_pt", spy)
    det = lambda d: {k: v.detach() if torch.is_tensor(v) else v for k, v in d.items()}
    base, again, out = det(S.render(H, ssaa, spp, bg_color=bgc)), det(S.render(H, ssaa, spp, bg_color=bgc)), det(S.render(H, ssaa, spp, bg_color=bgc, field=S.field))
    assert set(out) - set(base) == {"image", "weights_sum"} and "image" not in base and "weights_sum" not in base
    assert len(seen) == 3
    for n in maps:
        x, y = seen[0][n], seen[2][n]
        assert _bits(x, y) if torch.is_tensor(x) else x == y, "the sample loop's %s" % n
    for k, v in base.items():
        if torch.is_tensor(v):
            print("%s: max |difference| without the field twice %.3e, with against without %.3e" % (k, float((v - again[k]).abs().max()), float((v - out[k]).abs().max())))
    for k, v in base.items():
        assert (_bits(v, again[k]) and _bits(v, out[k])) if torch.is_tensor(v) else v == out[k], k
    # the composition, written here from the product's own G-buffer
    h = H * ssaa; N = h * h
    g = harness.build_gbuffer_stage1(S.W, S.vt, S.tt, H, H, ssaa, mlp_mat=S.mlp, pose=S.pose, intrinsics=S.intr(H, H))
    dirs = harness.view_dirs(harness.get_rays(S.pose, S.intr(H, H), H, H)[1], H, H, ssaa)
    idx = torch.nonzero(g["occ"].view(-1) > 0).view(-1)
    assert 0 < idx.numel() < N
    rgbs = torch.zeros(N, 3, device="cuda")
    rgbs[idx] = S.field.rgb(g["pos"][idx], dirs[idx])
    tri32 = S.tt.to(torch.int32)
    aa = lambda x: raster.antialias(x.view(1, h, h, x.shape[-1]), g["rast"].view(1, h, h, 4), g["vertices_clip"][None], tri32, topology_hash=S.topo,
                                    pos_gradient_boost=1.0).view(N, x.shape[-1]).clamp(0, 1)
    alpha = aa(g["occ"])
    image = alpha * aa(rgbs)
    if ssaa > 1:
        image = harness.scale_img_hwc(image.view(h, h, 3), (H, H)).reshape(H * H, 3)
        alpha = harness.scale_img_hwc(alpha.view(h, h, 1), (H, H)).reshape(H * H, 1)
    image = image + (1 - alpha) * bgc
    assert out["image"].shape == (H * H, 3) and torch.equal(out["image"], image)
    assert out["weights_sum"].shape == (H * H,) and torch.equal(out["weights_sum"], alpha.reshape(-1)) and torch.equal(out["occ"], alpha)
    frac = ((alpha > 1e-4) & (alpha < 1 - 1e-4)).float().mean()
    assert 0 < float(frac) < 0.5                                                  # the silhouette's fractional coverage is in the mask


def _spy(field, rec, detach=False):
    """field.rgb_train, recording its inputs and the cotangent that reaches its output; detach: the positions are detached by hand before the call."""
    orig = type(field).rgb_train

    def rgb_train(x, d, pos_grad=False):
        rec["x_requires_grad"] = bool(x.requires_grad)
        out = orig(field, x.detach() if detach else x, d, pos_grad=pos_grad)
        rec["x"], rec["d"], rec["out"] = x.detach().clone(), d.detach().clone(), out
        out.register_hook(lambda g: rec.__setitem__("g", g.detach().clone()))
        return out
    return rgb_train


def test_field_gradients_of_one_step_against_the_float64_network(S, monkeypatch):
    from mirres_restir_nerf_mesh_amd import losses
    H = 32
    rec = {}
    monkeypatch.setattr(S.field, "rgb_train", _spy(S.field, rec), raising=False)
    params = S.field.parameters()
    for p in params:
        p.grad = None
    out = S.render(H, 1, 2, field=S.field)
    gen = torch.Generator().manual_seed(9)
    gt = torch.rand(H * H, 3, generator=gen).cuda(); mask = (torch.rand(H * H, 1, generator=gen) > 0.5).float().cuda()
    loss = losses.stage1_loss(out, gt, gt ** 2.2, types.SimpleNamespace(use_brdf=True), gt_mask=mask)
    loss.backward()
    assert not rec["x_requires_grad"] and rec["g"].shape == rec["x"].shape and rec["g"].abs().max() > 0
    got = [p.grad.cpu().numpy() for p in params]
    host = [p.detach().cpu().numpy() for p in params]
    pos, dd, grgb = (rec[k].cpu().numpy() for k in ("x", "d", "g"))
    L = D.layout(1.0, log2_T=LOG2_T)
    g64, terms = B.grads(host, L, pos, dd, 1.0, None, grgb, with_terms=True)
    g32 = B.grads(host, L, pos, dd, 1.0, None, grgb, dtype=torch.float32)
    for k, name in enumerate(B.NAMES):
        w = B.criterion(name, got[k], g64[k], g32[k], terms)
        print("stage-1 step %-5s: worst error / allowance %.3f, E %.3e, E_ref %.3e, largest floor %.3e" % ((name,) + w))
        assert w[0] <= 1.0, (name, w)
    assert np.abs(g64[0]).max() > 0 and np.abs(g64[3]).max() > 0 and not got[2][0].any()          # no grad_sigma: row 0 of w1 gets nothing
    for p in params:
        p.grad = None


def test_offset_nerf_grad_reaches_the_vertices_only_when_asked(S, monkeypatch):
    from mirres_restir_nerf_mesh_amd import harness
    H = 32
    gt = torch.rand(H * H, 3, generator=torch.Generator().manual_seed(9)).cuda()
    build = harness.build_gbuffer_stage1

    def run(flag, detach):
        rec, gb = {}, {}
        monkeypatch.setattr(S.field, "rgb_train", _spy(S.field, rec, detach), raising=False)
        monkeypatch.setattr(harness, "build_gbuffer_stage1", lambda *a, **k: gb.setdefault("g", build(*a, **k)))
        voff = torch.zeros_like(S.vt).requires_grad_(True)
        out = S.render(H, 1, 1, voff=voff, field=S.field, offset_nerf_grad=flag)
        g_rgb, g_pos, g_voff = torch.autograd.grad(((out["image"] - gt) ** 2).mean(), [rec["out"], gb["g"]["pos"], voff], allow_unused=True)
        return dict(rec, g=g_rgb, g_pos=g_pos, g_voff=g_voff, occ=gb["g"]["occ"])
    off, by_hand, on = run(False, False), run(True, True), run(True, False)      # by_hand: the flag set, the positions detached before they reach the field
    assert (off["x_requires_grad"], by_hand["x_requires_grad"], on["x_requires_grad"]) == (False, True, True)
    assert torch.equal(off["g"], by_hand["g"]) and torch.equal(off["g"], on["g"]) and torch.equal(off["x"], on["x"])
    assert off["g_pos"] is None and by_hand["g_pos"] is None                      # detached: nothing reaches the surface points
    idx = torch.nonzero(on["occ"].view(-1) > 0).view(-1)
    want = torch.zeros(H * H, 3, device="cuda").index_put((idx,), S.field.backward_pos(on["x"], on["d"], None, on["g"]))
    assert torch.equal(on["g_pos"], want) and float(want.abs().max()) > 0
    a, b, c = off["g_voff"], by_hand["g_voff"], on["g_voff"]
    noise, moved = float((a - b).abs().max()), float((c - a).abs().max())
    print("voffsets.grad: max |.| %.3e, flag off against detached by hand %.3e (the order of the atomic adds), flag on against off %.3e" % (float(a.abs().max()), noise, moved))
    assert torch.isfinite(c).all() and float(a.abs().sum()) > 0                   # the silhouette gradient of dr.antialias is there either way
    assert noise <= GRAD_ULPS * 2.0 ** -24 * float(a.abs().max())                 # the flag off IS the run with the positions detached by hand, up to the order of the adds
    assert moved > 0 and moved > noise


def test_checkpoint_round_trip(S, tmp_path):
    from mirres_restir_nerf_mesh_amd import checkpoint as CK, stage0
    path = str(tmp_path / "ngp_stage1.pth")
    CK.save_checkpoint(path, S.mlp, torch.zeros_like(S.vt), S.env, epoch=1, global_step=1, field=S.field)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(CK.STAGE0_WEIGHT_KEYS) | {"encoder.offsets", "vertices_offsets"} <= set(ck["model"]) and ck["model"]["encoder.offsets"].dtype == torch.int32
    back = stage0.RadianceField.from_checkpoint(ck, bound=1.0, log2_hashmap_size=LOG2_T)
    for k in S.field.PARAMETER_NAMES:
        assert torch.equal(getattr(back, k), getattr(S.field, k).detach()), k
    assert CK.read_checkpoint(path)["global_step"] == 1                          # the other reader is not disturbed
    CK.save_checkpoint(path, S.mlp, torch.zeros_like(S.vt), S.env)
    assert not set(CK.STAGE0_WEIGHT_KEYS) & set(torch.load(path, map_location="cpu", weights_only=False)["model"])


def _script(name, args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name)] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


NERF_LINE = r"NeRF colour branch \(`image`\): loss first-window ([0-9.eE+-]+) last-window ([0-9.eE+-]+) .*PSNR of view 0: ([0-9.]+) -> ([0-9.]+) dB"


def test_train_script_learns_the_image_saves_the_field_and_resumes(tmp_path):
    ws = str(tmp_path / "ws")
    common = ["--synthetic", "--workspace", ws, "--spp", "2", "--H", "48", "--W", "48", "--quiet", "--stage0_ckpt", "random", "--freeze", "geometry", "material", "light"]
    out = _script("train_stage1.py", common + ["--iters", "40", "--save_interval", "40"])
    m = re.search(NERF_LINE, out)
    assert m, out[-1500:]
    first, last, p0, p1 = (float(x) for x in m.groups())
    print("image loss %.6f -> %.6f, PSNR of view 0 %.2f -> %.2f dB" % (first, last, p0, p1))
    assert last < first and p1 > p0
    path = os.path.join(ws, "checkpoints", "ngp_stage1_ep0040.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 40 and len(ck["optimizer"]["param_groups"]) == 2 and len(ck["optimizer"]["param_groups"][1]["params"]) == 6
    from mirres_restir_nerf_mesh_amd import stage0
    trained = stage0.RadianceField.from_checkpoint(ck, bound=1.0)
    fresh = stage0.RadianceField.init_random(1.0, seed=0)
    assert not torch.equal(trained.c2, fresh.c2) and not torch.equal(trained.table, fresh.table)
    # resume: the field comes from the checkpoint (no --stage0_ckpt), the loop continues at step 40 and starts from the trained image
    out2 = _script("train_stage1.py", [a for a in common if a not in ("--stage0_ckpt", "random")] + ["--iters", "44", "--save_interval", "0", "--ckpt", path])
    m2 = re.search(NERF_LINE, out2)
    assert m2 and "stage-1 training 4 iterations" in out2, out2[-1500:]
    assert abs(float(m2.group(3)) - p1) < 0.05                                    # the same network and mesh, no sampling in this frame; the target PNGs are rendered again
    # images with an alpha channel: gt_mask and the mask term, and --background random (per-pixel noise under the target and under the frame), end to end
    from PIL import Image
    for f in sorted(os.listdir(os.path.join(ws, "train"))):
        im = np.asarray(Image.open(os.path.join(ws, "train", f)).convert("RGB"))
        alpha = np.where((im == 255).all(axis=-1), 0, 255).astype(np.uint8)      # the synthetic frames stand on white
        Image.fromarray(np.dstack([im, alpha])).save(os.path.join(ws, "train", f))
    out3 = _script("train_stage1.py", ["--workspace", ws, "--transforms", os.path.join(ws, "transforms_train.json"), "--bound", "1", "--light_probe_res_hw", "64", "128",
                                       "--spp", "2", "--quiet", "--stage0_ckpt", "random", "--background", "random", "--enable_offset_nerf_grad", "--iters", "6",
                                       "--save_interval", "0"])
    m3 = re.search(NERF_LINE, out3)
    assert m3 and "stage-1 training 6 iterations" in out3 and all(np.isfinite(float(x)) for x in m3.groups()), out3[-1500:]


def test_evaluate_writes_the_rgb_frame(tmp_path):
    ws = str(tmp_path / "ev")
    out = _script("evaluate.py", ["--synthetic", "--workspace", ws, "--nerf_image", "--H", "48", "--W", "48", "--spp", "4", "--ssaa", "2", "--limit", "1"])
    files = [f for f in os.listdir(os.path.join(ws, "results_brdf")) if f.endswith("_rgb.png")]
    assert len(files) == 1 and files[0].endswith("_0000_rgb.png") and os.path.exists(os.path.join(ws, "results_brdf", files[0].replace("_rgb.png", "_rgb_brdf.png")))
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(ws, "results_brdf", files[0])))
    assert im.shape == (48, 48, 3) and im.std() > 0
