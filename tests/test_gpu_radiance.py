"""The stage-0 radiance network on the device (csrc/radiance.hip) through stage0.RadianceField, and stage0.render_stage0 over it: the SH direction encoder bit for bit
against the numpy float32 restatement (tests/radiance_refs.py), sigma bit-equal to DensityField.density, every layer within the derived forward-error bound of the
float64 network on the device's own bit-checked features, the synthetic checkpoint's closed form per point, the inference loop bit-equal to the same loop written
out here from the public operators, its pixels against weights_sum * colour + (1 - weights_sum) * background within the derived bound of the accumulation, and
scripts/render_stage0.py --synthetic in a child process.  The bounds are derived (radiance_refs' docstring, and _image_bound below) and stay as they are."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import density_refs as D                       # noqa: E402
import radiance_refs as RR                     # noqa: E402
from test_gpu_density import Config, _points   # noqa: E402

U = 2.0 ** -24


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


class Net:
    """A RadianceField with its weights on the host (read-only), its layout and table for the restatement, and the DensityField of the same table."""

    def __init__(self, field, density, L, table, weights):
        self.field, self.density, self.L, self.table, self.weights = field, density, L, table, weights
        for a in weights:
            a.setflags(write=False)


@pytest.fixture(scope="module")
def nets(S0):
    out = {}
    for log2_T, seed in ((19, 101), (14, 102)):
        cfg = Config(S0, log2_T, seed)
        rng = np.random.default_rng(seed + 1000)
        c0 = (rng.normal(size=(64, 31)) * 0.15).astype(np.float32); c1 = (rng.normal(size=(64, 64)) * 0.15).astype(np.float32)
        c2 = (rng.normal(size=(3, 64)) * 0.5).astype(np.float32)
        f = S0.RadianceField(*(torch.tensor(a) for a in (cfg.table, cfg.w0, cfg.w1, c0, c1, c2)), bound=1.0, log2_hashmap_size=log2_T)
        out[log2_T] = Net(f, cfg.field, cfg.L, cfg.table, (cfg.w0, cfg.w1, c0, c1, c2))
    ck = S0.synthetic_radiance_checkpoint()
    m = ck["model"]
    w = tuple(m[k].numpy().copy() for k in ("sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight", "color_net.2.weight"))
    out["synthetic"] = Net(S0.RadianceField.from_checkpoint(ck, bound=1.0), S0.DensityField.from_checkpoint(ck, bound=1.0), D.layout(1.0), m["encoder.embeddings"].numpy(), w)
    return out


def _dirs(n, seed=21):
    """Hostile directions first, random ones after: the six axes, -0.0 components, lengths 1e-3 and 1e3, one zero and one NaN direction (rows 12 and 13)."""
    z = np.float32(-0.0)
    sp = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [z, 0.5, z], [0.25, z, -0.75], [z, z, -3.0],
          [3e-4, -5e-4, 8e-4], [-6e2, 2e2, 7e2], [1e-3, 0, 0], [0, 0, 0], [np.nan, 0.5, 0.5]]
    rng = np.random.default_rng(seed)
    rnd = rng.normal(size=(max(n, 1), 3)).astype(np.float32)
    rnd[::7] *= np.float32(1e-3); rnd[3::7] *= np.float32(1e3)
    return np.concatenate([np.array(sp, np.float32), rnd])[:n]


def _same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_sh_bit_for_bit(nets, n):
    d = _dirs(n)
    got = nets["synthetic"].field.sh(torch.from_numpy(d).cuda()).cpu().numpy()
    want = RR.sh32(d)
    assert got.shape == (n, 16) and got.dtype == np.float32
    diff = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    print("n=%d: %d of %d words differ, %d NaN" % (n, int(diff.sum()), diff.size, int(np.isnan(got).sum())))
    assert not diff.any(), "outputs with differences: %s" % sorted(set(np.nonzero(diff)[1].tolist()))
    if n >= 14:
        assert np.isnan(got[12:14, 1:]).all() and np.isfinite(np.delete(got, [12, 13], axis=0)).all() and (got[:, 0] == RR.C0).all()


@pytest.mark.parametrize("which", [19, 14, "synthetic"])
def test_forward_against_the_float64_network(nets, which):
    net = nets[which]; f = net.field
    n = 1543                                                                    # seven blocks, the last one partly filled
    pos, oob = _points(n - 9)
    # one ulp INSIDE each face, which _points does not have, in the bottom and the top cell of every level and still in bounds: below, u is the first fp32 value
    # above 0 that the rule can give (2^-25); above, x + bound = 2 - 2^-24 is a tie that rounds to 2, so u = 1 exactly, as for +bound itself and one ulp past it.
    # The last u < 1 (1 - 2^-24) belongs to the point TWO ulps inside +bound: rows 6 .. 8.
    b = np.float32(1.0); zero = np.float32(0.0)
    inner = np.tile(np.array([0.3, -0.2, 0.7], np.float32), (9, 1))
    for k, (axis, side) in enumerate((a, s) for a in range(3) for s in (1, -1)):
        inner[k, axis] = np.nextafter(np.float32(side) * b, zero)
    for axis in range(3):
        inner[6 + axis, axis] = np.nextafter(np.nextafter(b, zero), zero)
    pos = np.concatenate([pos, inner]); oob = np.concatenate([oob, np.zeros(9, bool)])
    with np.errstate(invalid="ignore"):
        u = (pos + b) / np.float32(np.float32(2.0) * b)
    assert np.array_equal(oob, ~((u >= 0) & (u <= 1)).all(axis=1)) and not oob[-9:].any()
    ui = u[-9:-3][np.arange(6), np.repeat(np.arange(3), 2)]
    assert (ui[0::2] == 1).all() and (ui[1::2] == np.float32(2.0 ** -25)).all() and (u[-3:][np.arange(3), np.arange(3)] == np.float32(1.0 - 2.0 ** -24)).all()
    d = np.roll(_dirs(n), 20, axis=0)                                           # the hostile directions meet in-bounds random positions, the hostile positions random directions
    x, dd = torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()
    sigma, rgb = f.forward(x, dd)
    s2, rgb2, h16, sh = f._query(x, dd, True, True)
    sigma, rgb, s2, rgb2, h16, sh = (t.cpu().numpy() for t in (sigma, rgb, s2, rgb2, h16, sh))
    assert sigma.shape == (n,) and rgb.shape == (n, 3) and h16.shape == (n, 16) and sh.shape == (n, 16)
    assert _same_bits(sigma, s2) and _same_bits(rgb, rgb2)                      # with and without the extra outputs: the same arithmetic
    assert _same_bits(rgb, f.rgb(x, dd).cpu().numpy())
    assert _same_bits(sigma, net.density.density(x).cpu().numpy()) and _same_bits(sigma, f.density(x).cpu().numpy())
    assert _same_bits(sh, f.sh(dd).cpu().numpy()) and _same_bits(sh, RR.sh32(d))
    feat = f.encode(x).cpu().numpy()
    assert _same_bits(feat, D.encode32(net.table, net.L, pos, 1.0))
    ref = RR.forward64(feat, sh, net.weights); bnd = RR.forward_bound(feat, sh, net.weights)
    eh = np.abs(h16.astype(np.float64) - ref["h16"])
    print("%s: max |dh16| %.3e (allowed there %.3e)" % (which, eh.max(), bnd["h16"].reshape(-1)[eh.argmax()]))
    assert (eh <= bnd["h16"]).all()
    assert (sigma[oob] == np.float32(1.0)).all() and (h16[oob] == 0).all()
    rel = np.abs(sigma.astype(np.float64) - ref["sigma"]) / ref["sigma"]
    print("  h in [%.3f, %.3f], max sigma rel err %.3e, allowed %.3e" % (ref["h16"][:, 0].min(), ref["h16"][:, 0].max(), rel.max(), bnd["sigma_rel"].max()))
    assert np.abs(ref["h16"][:, 0]).max() < 80 and (rel <= bnd["sigma_rel"]).all()
    nan = np.isnan(ref["rgb"]).any(axis=1)
    assert nan.sum() == 2 and np.isnan(rgb[nan]).all() and np.isfinite(rgb[~nan]).all()      # the zero and the NaN direction, nothing else
    er = np.abs(rgb.astype(np.float64) - ref["rgb"])[~nan]
    print("  max |drgb| %.3e, allowed there %.3e; rgb in [%.3f, %.3f]" % (er.max(), bnd["rgb"][~nan].reshape(-1)[er.argmax()], rgb[~nan].min(), rgb[~nan].max()))
    assert (er <= bnd["rgb"][~nan]).all()
    assert oob.sum() == 5 and not nan[oob].any()                                # an out-of-bounds point still has a colour
    s0, c0 = f.forward(x[:0], dd[:0])
    assert tuple(s0.shape) == (0,) and tuple(c0.shape) == (0, 3) and tuple(f.rgb(x[:0], dd[:0]).shape) == (0, 3) and tuple(f.sh(dd[:0]).shape) == (0, 16)
    with pytest.raises(ValueError):
        f.forward(x, dd[:-1])


def test_synthetic_closed_form_per_point(nets):
    net = nets["synthetic"]; f = net.field
    rng = np.random.default_rng(31)
    n = 2000
    pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    d = _dirs(n + 14)[14:]                                                       # the random part: finite, non-zero
    x, dd = torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()
    sigma, rgb = (t.cpu().numpy() for t in f.forward(x, dd))
    feat = f.encode(x).cpu().numpy(); sh = f.sh(dd).cpu().numpy()
    assert _same_bits(feat, D.encode32(net.table, net.L, pos, 1.0)) and _same_bits(sh, RR.sh32(d))
    F = feat[:, 0].astype(np.float64)
    u = d.astype(np.float64); u = u / np.sqrt((u * u).sum(axis=1, keepdims=True))
    SH0, SH1 = float(np.float32(0.28209479177387814)), float(np.float32(0.48860251190291987))
    sig = lambda h: 1.0 / (1.0 + np.exp(-h))
    want = np.stack([sig(4 * SH1 * u[:, 0]), sig(4 * SH1 * u[:, 2]), sig(2 * (1.5 * F - 4 * SH0))], axis=1)       # synthetic_radiance_checkpoint's docstring
    bnd = RR.forward_bound(feat, sh, net.weights, dsh=RR.sh_bound())           # the closed form is in the exact direction: the fp32 sh is within sh_bound of it
    err = np.abs(rgb.astype(np.float64) - want)
    print("max |rgb - closed form| per channel %s, allowed at least %s" % (err.max(axis=0), bnd["rgb"].min(axis=0)))
    assert (err <= bnd["rgb"]).all() and (bnd["rgb"] < 1e-4).all()                    # and the bound is far below a step of 1 / 255
    rel = np.abs(sigma.astype(np.float64) - np.exp(1.5 * F)) / np.exp(1.5 * F)
    assert (rel <= bnd["sigma_rel"]).all()
    assert np.ptp(want[:, 0]) > 0.6 and np.ptp(want[:, 1]) > 0.6 and np.ptp(want[:, 2]) > 0.2


# ---------------------------------------------------------------------------------------------------------------- render_stage0

W_IMG = 32
T_THRESH = 1e-4


@pytest.fixture(scope="module")
def scene(S0):
    """The cameras and grid of scripts/dev_raymarch_time.end_to_end_check: synthetic checkpoint at S = 16, three seeded grid updates, a 32 x 32 view from distance 3."""
    import dev_raymarch_time as DRT
    from mirres_restir_nerf_mesh_amd import raymarching as RM
    H = 16
    ck = S0.synthetic_radiance_checkpoint(S=H)
    field = S0.RadianceField.from_checkpoint(ck, bound=1.0)
    G = S0.DensityGrid.from_checkpoint(ck, bound=1.0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for _ in range(3):
        G.update(field, noise=torch.rand(1, H ** 3, 3, generator=gen, device="cuda"))
    o, d = DRT.camera_rays(W_IMG)
    return dict(DRT=DRT, RM=RM, field=field, G=G, o=o, d=d, N=o.shape[0])


def _own_loop(sc, bg, cam_near_far=None, max_steps=1024):
    """nerf/renderer.py:714-717, 778-839 from the public operators -> image, depth, weights_sum and an upper bound on the samples composited per ray."""
    RM, G, field, o, d, N = sc["RM"], sc["G"], sc["field"], sc["o"], sc["d"], sc["N"]
    nears, fars = RM.near_far_from_aabb(o, d, G.aabb_train, G.min_near)
    if cam_near_far is not None:
        nears = torch.maximum(nears, cam_near_far[:, 0]); fars = torch.minimum(fars, cam_near_far[:, 1])
    ws = torch.zeros(N, device="cuda"); dp = torch.zeros(N, device="cuda"); im = torch.zeros(N, 3, device="cuda")
    alive = torch.arange(N, dtype=torch.int32, device="cuda"); rays_t = nears.clone()
    taken = torch.zeros(N, dtype=torch.int64, device="cuda")
    step = 0
    while step < max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts = RM.march_rays(n_alive, n_step, alive, rays_t, o, d, G.bound, False, G.density_bitfield, G.cascade, G.grid_size, nears, fars, False, 0, max_steps)
        dirs = dirs / torch.sqrt(torch.clamp(torch.sum(dirs * dirs, -1, keepdim=True), min=1e-20))
        sigmas, rgbs = field.forward(xyzs, dirs)
        taken.index_add_(0, alive.long(), (ts.view(n_alive, n_step, 2)[:, :, 1] != 0).sum(1))
        RM.composite_rays(n_alive, n_step, alive, rays_t, sigmas, rgbs, ts, ws, dp, im, T_THRESH, False)
        alive = alive[alive >= 0]
        step += n_step
    im = im + (1 - ws).unsqueeze(-1) * (1 if bg is None else bg)
    return im, dp, ws, taken


def _bgs(N):
    g = torch.Generator(); g.manual_seed(5)
    return {"none": None, "scalar": 0.25, "rgb": torch.tensor([0.1, 0.6, 0.9]), "per_ray": torch.rand(N, 3, generator=g)}


@pytest.mark.parametrize("bg_kind", ["none", "scalar", "rgb", "per_ray"])
@pytest.mark.parametrize("clip", [False, True])
def test_render_is_the_loop_written_out(S0, scene, bg_kind, clip):
    N = scene["N"]
    bg = _bgs(N)[bg_kind]
    cnf = None
    if clip:
        cnf = torch.tensor([0.0, 1e9], device="cuda").repeat(N, 1)
        cnf[::2] = torch.tensor([2.6, 2.9], device="cuda")                      # every other ray starts inside the ball and ends before its far side
    out = S0.render_stage0(scene["field"], scene["G"], scene["o"], scene["d"], bg_color=bg, T_thresh=T_THRESH, cam_near_far=cnf)
    bg_dev = bg.cuda() if torch.is_tensor(bg) else bg
    im, dp, ws, _ = _own_loop(scene, bg_dev, cnf)
    assert sorted(out) == ["depth", "image", "weights_sum"] and tuple(out["image"].shape) == (N, 3) and tuple(out["depth"].shape) == (N,)
    for k, want in (("image", im), ("depth", dp), ("weights_sum", ws)):
        assert torch.equal(out[k].view(torch.int32), want.view(torch.int32)), k
    assert bool(torch.isfinite(out["image"]).all()) and int((out["weights_sum"] > 0.99).sum()) >= W_IMG
    if clip:
        full = S0.render_stage0(scene["field"], scene["G"], scene["o"], scene["d"], bg_color=bg, T_thresh=T_THRESH)
        changed = (full["depth"] != out["depth"])
        assert bool(changed[::2].any()) and not bool(changed[1::2].any())       # the clamp bites, and only where it was set


def _image_bound(c, ws, bg, image, n):
    """|image - (ws c + (1 - ws) bg)| for one channel, everything float64 arrays per ray; c the ray's colour (bit-constant along it), ws the fp32 weights_sum, n an
    upper bound on the samples composited.  With W the exact sum of the fp32 weights w_k (the same numbers in both accumulators, csrc/device_march.hpp
    rm_comp_infer): ws = W (1 + e), |e| <= gamma_n (n sequential additions, the first onto 0); the colour accumulator adds fl(w_k c) = w_k c (1 + d), |d| <= u:
    |acc - c W| <= (u + gamma_n (1 + u)) c W.  So |acc - c ws| <= (u + gamma_n (2 + u)) c W and W <= ws / (1 - gamma_n).  The last line of render, image =
    fl(acc + fl(fl(1 - ws) bg)): |fl(fl(1 - ws) bg) - (1 - ws) bg| <= (2 u + u^2) |1 - ws| |bg|, and one rounding of the sum, u |image|."""
    g = n * U / (1.0 - n * U)
    return (U + g * (2.0 + U)) * c * ws / (1.0 - g) + (2.0 * U + U * U) * np.abs(1.0 - ws) * np.abs(bg) + U * np.abs(image)


@pytest.mark.parametrize("bg_kind", ["none", "per_ray"])
def test_render_pixels_are_weights_sum_times_colour_plus_background(S0, scene, bg_kind):
    N, field, G, o, d, DRT, RM = (scene[k] for k in ("N", "field", "G", "o", "d", "DRT", "RM"))
    bg = _bgs(N)[bg_kind]
    out = S0.render_stage0(field, G, o, d, bg_color=bg, T_thresh=T_THRESH)
    image, depth, ws = (out[k].cpu().numpy().astype(np.float64) for k in ("image", "depth", "weights_sum"))
    taken = _own_loop(scene, None)[3].cpu().numpy().astype(np.float64)
    unit = d / torch.sqrt(torch.clamp(torch.sum(d * d, -1, keepdim=True), min=1e-20))
    col = field.rgb(torch.zeros_like(o), unit)
    rng = np.random.default_rng(2)
    elsewhere = torch.from_numpy(rng.uniform(-0.9, 0.9, size=(N, 3)).astype(np.float32)).cuda()
    assert torch.equal(field.rgb(elsewhere, unit)[:, :2].view(torch.int32), col[:, :2].view(torch.int32))      # r and g: the same bits wherever the sample lies
    col = col.cpu().numpy().astype(np.float64)
    bgn = np.ones((N, 3)) if bg is None else bg.numpy().astype(np.float64)
    worst = 0.0
    for ch in (0, 1):                                                           # the two channels that depend on the direction alone
        want = ws * col[:, ch] + (1.0 - ws) * bgn[:, ch]
        tol = _image_bound(col[:, ch], ws, bgn[:, ch], image[:, ch], np.maximum(taken, 1.0))
        err = np.abs(image[:, ch] - want)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (ch, float(err.max()), float(tol[err.argmax()]))
    print("bg %s: max err / bound %.3f over %d pixels, %d with samples, at most %d samples" % (bg_kind, worst, N, int((taken > 0).sum()), int(taken.max())))
    # (c) rays that miss: exactly the background, depth 0
    miss = ws == 0
    assert miss.sum() >= W_IMG and (depth[miss] == 0).all() and np.array_equal(out["image"].cpu().numpy()[miss], bgn[miss].astype(np.float32))
    assert ((taken > 0) == ~miss).all()
    # (d) colours do not steer termination: weights_sum and depth are the white-colour loop's of scripts/dev_raymarch_time.py, to the bit
    nears, fars = RM.near_far_from_aabb(o, d, G.aabb_train, G.min_near)
    iws, idp, _, _ = DRT.infer_loop(RM, G, field.density, o, d, nears, fars, T_thresh=T_THRESH)
    assert torch.equal(iws.view(torch.int32), out["weights_sum"].view(torch.int32)) and torch.equal(idp.view(torch.int32), out["depth"].view(torch.int32))


def test_render_script_synthetic_in_a_child_process(tmp_path):
    ws = str(tmp_path / "ws")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_stage0.py"), "--synthetic", "--workspace", ws, "--H", "64", "--W", "64", "--views", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(os.path.join(ws, "results"))) == ["synthetic_0000_depth.png", "synthetic_0000_rgb.png", "synthetic_0001_depth.png", "synthetic_0001_rgb.png"]
    assert "0 values off the closed form" in r.stdout and "opaque pixels" in r.stdout
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(ws, "results", "synthetic_0000_rgb.png")))
    assert img.shape == (64, 64, 3) and (img[0, 0] == 255).all() and (img[32, 32] < 255).any()      # white background in the corner, the ball in the middle


def test_render_script_on_a_checkpoint_file_and_a_transforms_file(S0, tmp_path, capsys):
    """The path a user takes: torch.load of a .pth (here the synthetic radiance checkpoint, with an aabb_infer and no density_bitfield: packed from the grid), the
    cameras of a transforms file, the PNGs under results/, and the PSNR against the frame's image — the script's own first output serves as that image, so the
    second run differs from it by the 8-bit quantisation alone: floor(255 x) / 255 is off by less than 1 / 255, PSNR > 20 log10(255) = 48.13 dB."""
    import json
    import shutil
    import render_stage0 as RS
    from PIL import Image
    ws = tmp_path / "ws"; data = tmp_path / "data"; (data / "test").mkdir(parents=True)
    ck = S0.synthetic_radiance_checkpoint(S=32)
    ck["model"]["aabb_infer"] = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    ckpt = tmp_path / "ngp_stage0_ep0001.pth"; torch.save(ck, str(ckpt))
    frames = [{"file_path": "./test/r_%d" % k, "transform_matrix": p.tolist()} for k, p in enumerate(RS.orbit_poses(2))]
    tf = data / "transforms_test.json"; tf.write_text(json.dumps({"camera_angle_x": 0.84, "w": 96, "h": 96, "frames": frames}))
    args = ["--workspace", str(ws), "--ckpt", str(ckpt), "--transforms", str(tf), "--bound", "1", "--downscale", "2"]
    assert RS.main(args) == 0
    out = capsys.readouterr().out
    assert "no density_bitfield" in out and "PSNR" not in out
    names = ["ngp_stage0_ep0001_%04d_%s.png" % (k, kind) for k in range(2) for kind in ("depth", "rgb")]
    assert sorted(os.listdir(ws / "results")) == names
    first = {n: (ws / "results" / n).read_bytes() for n in names}
    img = np.asarray(Image.open(ws / "results" / names[1]))
    assert img.shape == (48, 48, 3) and (img[0, 0] == 255).all() and (img[24, 24] < 255).any()      # white background in the corner, the ball in the middle
    for k in range(2):
        shutil.copy(ws / "results" / names[2 * k + 1], data / "test" / ("r_%d.png" % k))
    assert RS.main(args) == 0
    out = capsys.readouterr().out
    psnr = [float(l.split("PSNR")[1]) for l in out.splitlines() if l.startswith("[INFO] view ") and "PSNR" in l]
    assert len(psnr) == 2 and min(psnr) > 48.13 and "mean PSNR over 2 views" in out
    assert {n: (ws / "results" / n).read_bytes() for n in names} == first                             # the same files again
    assert RS.main(args + ["--color_space", "linear"]) == 0                                           # tone-mapped before it is written: other bytes, a PSNR all the same
    out = capsys.readouterr().out
    assert "mean PSNR over 2 views" in out and (ws / "results" / names[1]).read_bytes() != first[names[1]]
    with pytest.raises(ValueError, match="--bound"):
        RS.main(args[:6] + ["--bound", "2"])                                                          # the hash-grid layout of another bound: refused by name
