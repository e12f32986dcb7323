"""GPU: the stage-1 texture bake (csrc/bake.hip through mirres_restir_nerf_mesh_amd/export.py) against the numpy restatements of tests/bake_refs.py
(the reference's own arithmetic: renderer.py:349-462), and the exported files read back the way a viewer reads them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bake_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _rast_vs_ref(EX, vt, ft, W, H, ref=R.raster_ref):
    rast = EX.uv_rasterize(vt, ft, W, H).cpu().numpy()
    tid, b0, b1 = ref(vt, ft, W, H)
    assert np.array_equal(rast[:, 3].astype(np.int64) - 1, tid), "%d texels differ" % int((rast[:, 3].astype(np.int64) - 1 != tid).sum())
    cov = tid >= 0
    assert np.abs(rast[cov, 0] - b0[cov]).max(initial=0) <= 1e-6 and np.abs(rast[cov, 1] - b1[cov]).max(initial=0) <= 1e-6
    assert (rast[~cov] == 0).all() and (rast[:, 2] == 0).all()
    return tid


def test_uv_rasterize_atlas_matches_integer_restatement(EX, scene_mod):
    v, f = scene_mod.make_mesh(3, 4)
    h0 = w0 = 512; s = 2
    vt, ft, _ = EX.uv_atlas(v, f, h0, w0)
    tid = _rast_vs_ref(EX, vt, ft, w0 * s, h0 * s)
    n = np.bincount(tid[tid >= 0], minlength=f.shape[0])
    assert (n > 0).all(), "every triangle of the atlas covers a bake texel"
    # inside a pair's cell square every texel centre belongs to one of the two triangles
    pairs, _ = EX.pair_triangles(f)
    t2 = tid.reshape(h0 * s, w0 * s)
    for t, u, _, _ in pairs:
        q = vt[ft[t].astype(np.int64)] * np.array([w0 * s, h0 * s])
        x0, y0 = np.rint(q.min(0)).astype(int); x1, y1 = np.rint(q.max(0)).astype(int)
        blk = t2[y0:y1, x0:x1]
        assert np.isin(blk, (t, u)).all()


def test_uv_rasterize_adversarial(EX):
    rng = np.random.default_rng(7)
    W, H = 96, 64
    vt = [rng.uniform(-0.2, 1.2, (60, 2))]                                     # overlaps, both windings, partly outside [0, 1]
    c = np.stack(np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H), -1).reshape(-1, 2)
    vt.append(c[rng.integers(0, c.shape[0], 60)])                              # vertices on texel centres
    base = rng.uniform(0, 1, (10, 2)); vt.append(np.concatenate((base, base + [1e-4, 0.3], base + [2e-4, 0.6])))   # slivers
    vt = np.concatenate(vt).astype(np.float32)
    N = vt.shape[0]
    ft = np.concatenate((rng.integers(0, 60, (40, 3)), rng.integers(60, 120, (40, 3)),
                         np.stack((120 + np.arange(10), 130 + np.arange(10), 140 + np.arange(10)), 1),
                         [[0, 0, 1], [2, 3, 2]], rng.integers(0, N, (40, 3))))
    ft = np.concatenate((ft, ft[:, [0, 2, 1]]))                                # the same triangles reversed: the lower index wins
    _rast_vs_ref(EX, vt, ft, W, H)


def test_uv_rasterize_scans_more_than_two_rounds_of_block_sums(EX):
    """Branch: the carry of k_scan_sums (csrc/bake.hip:101) — one workgroup walks the block sums BK_BLOCK = 256 (:16) at a time, each sum covering BK_SCAN = 1024
    (:88) triangles, so a second round needs more than 262 144 triangles — with a ragged last round, a ragged last block of k_scan_local, zero-chunk
    triangles (equal neighbours in first[], which k_uv_cover's binary search must step over) and triangles of many chunks.
    Input (bake_refs.cell_grid_input): a 1024 x 1024 grid tiled by 2 x 2-texel cells, each split along a random diagonal through two texel centres (the fill
    rule decides them), half the triangles reversed, a zero-area triangle at every 349th position, 200 triangles with boxes of up to 100 x 100 texels last.
    Host assertions before the launch: T > 2 * 262 144, nb % 256 != 0, T % 1024 != 0, first[] restated has equal neighbours, every texel covered in the
    reference.  Observed: T = 525 994, nb = 514 block sums = 3 rounds (the last of 2), 1 507 zero-chunk triangles, 528 919 work items, up to 169 for one triangle."""
    BK_BLOCK, BK_SCAN = 256, 1024                                              # csrc/bake.hip:16 and :90
    W = H = 1024
    vt, ft, n_small = R.cell_grid_input(W)
    T = ft.shape[0]; nb = -(-T // BK_SCAN)
    first = R.chunk_first(vt, ft, W, H)
    ref = R.raster_split_ref(vt, ft, n_small, W, H, 2)
    print("T %d, nb %d, rounds %d, zero-chunk triangles %d, work items %d" % (T, nb, -(-nb // BK_BLOCK), int((np.diff(first) == 0).sum()), first[-1]))
    assert T > 2 * BK_BLOCK * BK_SCAN and -(-nb // BK_BLOCK) >= 3 and nb % BK_BLOCK != 0 and T % BK_SCAN != 0
    assert (np.diff(first) == 0).sum() >= n_small // 349 and np.diff(first).max() > 100
    assert (ref[0] >= 0).all() and len(np.unique(ref[0])) == n_small - n_small // 349
    tid = _rast_vs_ref(EX, vt, ft, W, H, ref=lambda *a: ref)
    assert np.array_equal(tid, ref[0])


def _mlp():
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    import mirres_restir_nerf_mesh_amd as M
    aabb, mn, mx = CK.material_field_args(CK.resolve_material_config(CK.material_config(bound=1.0)))
    torch.manual_seed(0)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    return mlp


def test_field_and_quantisation(EX, scene_mod):
    v, f = scene_mod.make_mesh(3, 4)
    vt, ft, _ = EX.uv_atlas(v, f, 256, 256)
    mlp = _mlp()
    r = EX.bake_textures(mlp.sample_no_di, v, f, vt, ft, 256, 256, 2, keep=True)
    from mirres_restir_nerf_mesh_amd import raster
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    xyz_all = raster.interpolate(vd, r["rast"], fd)
    idx = r["index"].long()
    assert torch.equal(r["xyz"], xyz_all[idx])
    assert torch.equal(r["feats"], mlp.sample_no_di(r["xyz"]))
    feats = r["feats"].cpu().numpy(); index = idx.cpu().numpy()
    for k in (0, 1):
        ref = np.zeros((512 * 512, 3), np.uint8)
        ref[index] = R.quantise_ref(feats[:, 3 * k:3 * k + 3])
        got = r["quant"][k].cpu().numpy().reshape(-1, 3)
        d = np.abs(got.astype(np.int32) - ref)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (d.max(), (d > 0).mean())


def _coded(H, W):
    """A plane whose bytes name their own texel (24 bits), and a second one that differs from it."""
    i = np.arange(H * W, dtype=np.uint32)
    a = np.stack((i & 255, (i >> 8) & 255, (i >> 16) & 255), 1).astype(np.uint8)
    return a, (255 - a).astype(np.uint8)


def _check_inpaint(EX, mask, radius=32):
    from scipy.ndimage import binary_dilation, distance_transform_edt
    H, W = mask.shape
    a, b = _coded(H, W)
    m = torch.from_numpy(mask.astype(np.uint8).ravel()).cuda()
    o0, o1 = EX.texture_inpaint(m, torch.from_numpy(a.ravel()).cuda(), torch.from_numpy(b.ravel()).cuda(), W, H, radius)
    o0 = o0.cpu().numpy().reshape(-1, 3).astype(np.int64); o1 = o1.cpu().numpy().reshape(-1, 3)
    region = binary_dilation(mask, iterations=radius) & ~mask if mask.any() else np.zeros_like(mask)
    flat = mask.ravel(); reg = region.ravel()
    assert np.array_equal(o0[flat], a[flat]) and np.array_equal(o1[flat], b[flat])
    other = ~flat & ~reg
    assert (o0[other] == 0).all() and (o1[other] == 0).all(), "texels outside the dilated region stay 0"
    if reg.any():
        src = o0[reg, 0] | (o0[reg, 1] << 8) | (o0[reg, 2] << 16)
        assert (src < H * W).all() and flat[src].all(), "region texels copy covered texels"
        assert np.array_equal(o1[reg], b[src]), "both planes from the same texel"
        p = np.nonzero(reg)[0]
        d2 = (p // W - src // W) ** 2 + (p % W - src % W) ** 2
        edt = distance_transform_edt(~mask).ravel()[reg]
        assert np.array_equal(d2.astype(np.float64), np.rint(edt ** 2)), "each copies a covered texel at the exact nearest distance"
    return region


def test_inpaint_random_masks(EX):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(11)
    H = W = 2048
    _check_inpaint(EX, np.zeros((H, W), bool))
    _check_inpaint(EX, np.ones((H, W), bool))
    noise = gaussian_filter(rng.standard_normal((H // 8, W // 8)), 2.0)
    blobs = np.kron(noise > 0.15, np.ones((8, 8), bool))
    blobs[:, :3] = True; blobs[-1, :] = True                                     # touching the border
    assert _check_inpaint(EX, blobs).any()
    sparse = rng.random((H, W)) < 2e-4                                         # isolated texels: ties and far gutters
    assert _check_inpaint(EX, sparse).any()
    _check_inpaint(EX, sparse[:777, :1031].copy(), radius=7)                    # sizes off the tiles, another radius


def test_inpaint_on_the_baked_mask_equals_the_reference(EX, scene_mod):
    v, f = scene_mod.make_mesh(3, 4)
    vt, ft, _ = EX.uv_atlas(v, f, 256, 256)
    field = lambda x: torch.cat((0.5 + 0.5 * torch.sin(4 * x), 0.5 + 0.5 * torch.cos(3 * x)), 1)
    r = EX.bake_textures(field, v, f, vt, ft, 256, 256, 2, keep=True)
    mask = r["mask"].cpu().numpy().reshape(512, 512).astype(bool)
    _check_inpaint(EX, mask)
    q0 = r["quant"][0].cpu().numpy().reshape(512, 512, 3); p0 = r["inpaint"][0].cpu().numpy().reshape(512, 512, 3)
    ref = R.inpaint_ref(mask, q0)
    # the coded planes above show the exact nearest texel; with the field's own bytes only the kd-tree's tie breaks can differ
    agree = (p0 == ref).all(-1)
    print("inpaint: %.4f of the texels equal the reference's bytes" % agree.mean())
    assert agree[mask].all() and agree.mean() > 0.9
    assert np.array_equal(R.downsample_ref(p0, 2), r["feat"][0].cpu().numpy())


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_downsample(EX, s):
    rng = np.random.default_rng(s)
    H, W = 12 * 7 * s, 12 * 11 * s
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = EX.texture_downsample(torch.from_numpy(img.ravel()).cuda(), W, H, s).cpu().numpy()
    assert np.array_equal(got, R.downsample_ref(img, s))


def _field(x):
    """A smooth analytic material field in [0.15, 0.85]."""
    return torch.cat((0.5 + 0.35 * torch.sin(2.0 * x + 0.3), 0.5 + 0.35 * torch.cos(1.7 * x[:, [1, 2, 0]] - 0.2)), 1)


def test_end_to_end_files_read_back_like_a_viewer(EX, scene_mod, tmp_path):
    from PIL import Image
    from mirres_restir_nerf_mesh_amd import raster
    v, f = scene_mod.make_mesh(4, 8)
    files = EX.export_stage1(str(tmp_path), v, f, [0, v.shape[0]], [0, f.shape[0]], mlp=None, texture_size=1024, ssaa=2, field=_field)
    assert sorted(os.path.basename(x) for x in files) == ["feat0_0.png", "feat1_0.png", "mesh_0.mtl", "mesh_0.obj"]
    vo, vto, fo, fto = EX.read_obj(str(tmp_path / "mesh_0.obj"))
    assert np.array_equal(vo, v) and np.array_equal(fo, f)
    assert "map_Kd feat0_0.png" in open(tmp_path / "mesh_0.mtl").read()
    rng = np.random.default_rng(5)
    for k in (0, 1):
        img = np.asarray(Image.open(tmp_path / ("feat%d_0.png" % k)).convert("RGB"))
        assert img.shape == (1024, 1024, 3)
        q = vto[fto.astype(np.int64)].astype(np.float64) * 1024
        area = 0.5 * np.abs((q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0]))
        cand = np.nonzero(area >= 4)[0]
        assert cand.size > 0.9 * f.shape[0]
        t = cand[rng.integers(0, cand.size, 10000)]
        b = rng.dirichlet((1, 1, 1), 10000)
        P = np.einsum("nk,nkc->nc", b, v[f[t]].astype(np.float64)).astype(np.float32)
        uvp = np.einsum("nk,nkc->nc", b, vto[fto[t]].astype(np.float64))
        uv = np.stack((uvp[:, 0], 1.0 - uvp[:, 1]), 1).astype(np.float32)             # image row 0 is the top: v = 1 - v'
        tex = torch.from_numpy(img.astype(np.float32)).cuda()
        got = raster.texture(tex, torch.from_numpy(uv).cuda()).cpu().numpy()
        want = R.quantise_ref(_field(torch.from_numpy(P).cuda()).cpu().numpy()[:, 3 * k:3 * k + 3]).astype(np.float64)
        err = np.abs(got - want).max(1)
        print("feat%d: |err| max %.2f, > 3 LSB on %.4f %% of the samples" % (k, err.max(), 100 * (err > 3).mean()))
        assert (err <= 3).mean() >= 0.999, (err.max(), (err > 3).mean())


def test_two_cascades(EX, scene_mod, tmp_path):
    v0, f0 = scene_mod.make_mesh(2, 4)
    v1 = v0 * np.float32(2.0)
    v = np.concatenate((v0, v1)); f = np.concatenate((f0, f0 + v0.shape[0]))
    files = EX.export_stage1(str(tmp_path), torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), [0, v0.shape[0], v.shape[0]],
                             [0, f0.shape[0], f.shape[0]], mlp=None, texture_size=256, ssaa=2, field=_field)
    from PIL import Image
    for cas in (0, 1):
        for k in (0, 1):
            assert Image.open(tmp_path / ("feat%d_%d.png" % (k, cas))).size == (256, 256)
        vo, vto, fo, fto = EX.read_obj(str(tmp_path / ("mesh_%d.obj" % cas)))
        assert np.array_equal(fo, f0) and np.array_equal(vo, (v0, v1)[cas])
        assert "mtllib mesh_%d.mtl" % cas in open(tmp_path / ("mesh_%d.obj" % cas)).readline()
    assert len(files) == 8


def test_export_script_synthetic(tmp_path):
    ws = tmp_path / "ws"; out = tmp_path / "out"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "export_stage1.py"), "--synthetic", "--workspace", str(ws),
                        "--texture_size", "512", "--ssaa", "2", "--out", str(out)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from mirres_restir_nerf_mesh_amd import export as EX
    from PIL import Image
    v, vt, f, ft = EX.read_obj(str(out / "mesh_0.obj"))
    assert v.shape[0] > 0 and f.shape[0] > 0 and (ft >= 0).all() and ft.max() < vt.shape[0]
    assert Image.open(out / "feat0_0.png").size == (512, 512) and Image.open(out / "feat1_0.png").size == (512, 512)
    img = np.asarray(Image.open(out / "feat0_0.png"))
    assert img.any()
