"""GPU: the textured-mesh material source (csrc/texmat.hip, mirres_texmat_lookup, mirres_render_args_t::tex) — the lookup kernel against the numpy
restatement of tests/texmat_refs.py, the triangle ids the path carries to its bounce vertices, a textured frame equal bit for bit to the constant-material
frame when every texel holds one value, and a frame of an exported asset whose indirect hits demonstrably read the textures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texmat_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _two_cascade_material(EX, scene_mod, rng, sizes=((96, 160), (80, 72))):
    """Two cascades (the second mesh scaled by 2, as the cascades of a stage-0 mesh are) with atlas UVs (seams between the cells), random textures and a
    few triangles whose UV corners coincide (degenerate UVs)."""
    v0, f0 = scene_mod.make_mesh(2, 4)
    verts, tris, vts, fts, planes, tri_end = [], [], [], [], [], []
    nv = nt = nf = 0
    for c, (H, W) in enumerate(sizes):
        v = v0 * np.float32(1 + c)
        vt, ft, _ = EX.uv_atlas(v, f0, H, W)
        ft = ft.astype(np.int32).copy()
        ft[::17, 1] = ft[::17, 0]; ft[::23] = ft[::23, :1]                       # degenerate UV triangles: a segment, a point
        verts.append(v); tris.append(f0 + nv); vts.append(vt); fts.append(ft + nt)
        planes.append(rng.integers(0, 256, (H, W, 8), dtype=np.uint8))
        nv += v.shape[0]; nt += vt.shape[0]; nf += f0.shape[0]; tri_end.append(nf)
    m = EX.TexturedMaterial(np.concatenate(verts), np.concatenate(tris), np.concatenate(vts).astype(np.float32), np.concatenate(fts), tri_end, planes,
                            roughness_min=0.08)
    return m


def _hits(m, rng, n):
    """Random points on random triangles: interior, on edges, on vertices."""
    tris = m.tris.cpu().numpy(); verts = m.verts.cpu().numpy()
    prim = rng.integers(0, tris.shape[0], n)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    b[: n // 8, 2] = 0; b[: n // 8] /= b[: n // 8].sum(1, keepdims=True)      # edges
    b[n // 8: n // 6] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, n // 6 - n // 8)]   # vertices
    pos = np.einsum("nk,nkc->nc", b, verts[tris[prim]]).astype(np.float32)
    return prim, pos


def _ref_args(m):
    return (m.verts.cpu().numpy(), m.tris.cpu().numpy(), m.vt.cpu().numpy(), m.ft.cpu().numpy(), m.tri_end, [p.cpu().numpy() for p in m.planes],
            m.decode.cpu().numpy(), m.roughness_min)


@pytest.mark.parametrize("use_scale", [False, True])
def test_lookup_matches_numpy(EX, scene_mod, use_scale):
    rng = np.random.default_rng(2 + int(use_scale))
    m = _two_cascade_material(EX, scene_mod, rng)
    n = 200000
    prim, pos = _hits(m, rng, n)
    occ = (rng.random(n) < 0.8).astype(np.float32)
    occ[rng.random(n) < 0.05] = 0.5                                                  # the threshold itself is occupied
    prim = prim.astype(np.int32); bad = rng.random(n) < 0.01
    prim[bad] = np.where(rng.random(bad.sum()) < 0.5, -1, m.tri_end[-1] + 3)          # occupied rows with no valid triangle: left unwritten
    scale = (1.7, 0.6, 2.5)
    kd0 = np.full((n, 3), np.nan, np.float32); rm0 = np.full((n, 2), np.nan, np.float32)   # NaN seed: every written row is visible
    kd_t = torch.from_numpy(kd0).cuda(); rm_t = torch.from_numpy(rm0).cuda()
    m.lookup(torch.from_numpy(prim).cuda(), torch.from_numpy(pos).cuda(), occ=torch.from_numpy(occ).cuda(), kd=kd_t, rough_metal=rm_t, use_scale=use_scale, scale=scale)
    kd, rm = kd_t.cpu().numpy(), rm_t.cpu().numpy()
    args = _ref_args(m)
    kd_r, rm_r = R.lookup(*args, occ, prim, pos, kd0, rm0, use_scale, scale)
    written = (occ >= 0.5) & (prim >= 0) & (prim < m.tri_end[-1])
    assert np.isnan(rm[~written]).all(), "rows that are not occupied (or have no triangle) are never written"
    if use_scale:
        assert np.array_equal(kd[~written], np.fmin(np.fmax(kd0[~written], 0), 1)), "the kd clamp of use_scale reaches every row"
    else:
        assert np.isnan(kd[~written]).all()
    assert np.isfinite(kd[written]).all() and np.isfinite(rm[written]).all()
    err = max(np.abs(kd[written] - kd_r[written]).max(), np.abs(rm[written] - rm_r[written]).max())
    print("fp32 barycentrics: max |err| %.3g over %d rows" % (err, written.sum()))
    assert err <= 1e-6
    assert (rm[written, 0] >= 0.08).all() and (rm[written, 0] <= 1).all()
    # the same with float64 barycentrics: how far the fp32 formula's rounding moves a lookup (uv error ~1e-7 x texture side x largest texel step)
    kd64, rm64 = R.lookup(*args, occ, prim, pos, kd0, rm0, use_scale, scale, bary64=True)
    e64 = max(np.abs(kd[written] - kd64[written]).max(), np.abs(rm[written] - rm64[written]).max())
    print("float64 barycentrics: max |err| %.3g" % e64)
    assert e64 <= 2e-3


def test_lookup_refuses_bad_material(EX, scene_mod):
    from mirres_restir_nerf_mesh_amd._lib import lib, MirresError
    m = _two_cascade_material(EX, scene_mod, np.random.default_rng(0))
    st = m._struct()
    st.n_cas = 9
    z = torch.zeros(4, dtype=torch.int32, device="cuda"); f = torch.zeros((4, 3), device="cuda"); r = torch.zeros((4, 2), device="cuda")
    assert lib().mirres_texmat_lookup(C.byref(st), None, z.data_ptr(), f.data_ptr(), 4, f.data_ptr(), r.data_ptr(), 0, None, None) < 0
    st.n_cas = 2
    m._st = None


def _gbuffer_worker(verts, tris):
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    w = RR.restirbvhWorker(verts.contiguous(), tris.contiguous()); w.update_mesh(w.vrt, w.v_ind)
    return w


def test_path_carries_the_hit_triangle(EX, scene_mod):
    """mirres_pt_new_dir with mirres_path_t::new_prim: the triangle of every next vertex equals what mirres_bvh_trace (mode 2, the path's closest-hit
    answer) reports for the same continuation ray; -1 where the ray missed."""
    from mirres_restir_nerf_mesh_amd import harness, _ops, _lib
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    v, f = scene_mod.make_mesh(4, 8)
    w = _gbuffer_worker(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())
    g = harness.build_gbuffer(w, 96, 96, kd=(0.5, 0.5, 0.5), roughness=0.3, metallic=0.0)
    N = g["fx"] * g["fy"]
    ctx = _ops.get_ctx(g["fx"], g["fy"])
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    prd, npos, nrd, nocc, nn = z(N, 5), z(N, 3), z(N, 3), z(N), z(N, 3)
    nprim = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    keep = []
    p = _ops.path_struct(g["occ"].view(-1), g["pos"], g["normal"], g["ray_dir"], g["kd"], g["rm"], prd, npos, nrd, nocc, nn, keep)
    p.new_prim = nprim.data_ptr()
    check(lib().mirres_pt_new_dir(ctx.h, w.h, C.byref(p), 11, 0, stream_ptr()), "mirres_pt_new_dir")
    torch.cuda.synchronize()
    hit = nocc > 0.5
    assert hit.sum() > 1000 and (nprim[~hit] == -1).all()
    vis_near = _lib.default_config().vis_near
    o = g["pos"][hit] + float(np.float32(vis_near)) * nrd[hit]
    n = int(hit.sum())
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = o; rays[:, 3] = 0.0; rays[:, 4:7] = nrd[hit]; rays[:, 7] = 1e7
    th = torch.empty(n, dtype=torch.int32, device="cuda"); tp = torch.empty(n, dtype=torch.int32, device="cuda"); pp = torch.empty((n, 3), device="cuda")
    check(lib().mirres_bvh_trace(w.h, rays.data_ptr(), n, 2, th.data_ptr(), None, pp.data_ptr(), None, tp.data_ptr(), None, stream_ptr()), "mirres_bvh_trace")
    torch.cuda.synchronize()
    assert (th == 1).all() and torch.equal(pp, npos[hit])
    assert torch.equal(tp, nprim[hit])


def _frame(RR, harness, worker, material, env, pose, intr, S, spp, seed, consts, const_mat=None, albedo_scale=None, max_bounce=2, gmat=None):
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    g = harness.build_gbuffer_from_pose(worker, pose, intr, S, S, 1, gmat if gmat is not None else material, **consts)
    use_scale = albedo_scale is not None
    scale = tuple(albedo_scale) if use_scale else (1.0, 1.0, 1.0)
    if use_scale:
        g["kd"] = (g["kd"] * torch.tensor(scale, dtype=torch.float32, device="cuda")[None, :]).contiguous()
    ctx = get_ctx(g["fx"], g["fy"], max_bounce=max_bounce)
    kw = dict(const_kd=const_mat[0], const_rm=const_mat[1]) if const_mat else {}
    outs = RR.render_fused(ctx, worker, material, use_scale, scale, env, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"], g["pos"],
                           spp, 2, 2, 2.0, 0.1, 0.001, seed, **kw)[0]
    torch.cuda.synchronize()
    return outs, g


def _pose(k=0, r=3.2):
    az, el = np.deg2rad(30.0 + 90.0 * k), np.deg2rad(30.0)
    eye = r * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    fwd = -eye / np.linalg.norm(eye); right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right); up = np.cross(right, fwd)
    pose = np.eye(4); pose[:3, :3] = np.stack([right, up, -fwd], 1); pose[:3, 3] = eye
    return torch.from_numpy(pose.astype(np.float32))


def _intr(S):
    focal = 0.5 * S / np.tan(0.5 * 0.6911)
    return (focal, focal, S * 0.5, S * 0.5)


@pytest.mark.parametrize("albedo_scale", [None, (1.3, 0.8, 1.1)])
def test_constant_texture_equals_constant_material(EX, scene_mod, albedo_scale):
    """Every texel = q: the textured frame equals the constant-material frame (const_kd = const_rm = decode(q), same G-buffer constants) bit for bit
    in all six outputs — every primary and indirect hit is looked up, on the right triangle, by the exact rule."""
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness
    q = 140
    v, f = scene_mod.make_mesh(2, 4)
    vt, ft, _ = EX.uv_atlas(v, f, 64, 96)
    m = EX.TexturedMaterial(v, f, vt, ft, [f.shape[0]], [np.full((64, 96, 8), q, np.uint8)], roughness_min=0.08)
    d = float(m.decode[q])
    assert d >= 0.08
    w = _gbuffer_worker(m.verts, m.tris)
    env = torch.from_numpy(scene_mod.make_env(32, 64)).cuda()
    consts = dict(kd=(d, d, d), roughness=d, metallic=d)
    a, ga = _frame(RR, harness, w, m, env, _pose(0), _intr(64), 64, 4, 1234, consts, albedo_scale=albedo_scale)
    b, gb = _frame(RR, harness, w, None, env, _pose(0), _intr(64), 64, 4, 1234, consts, const_mat=((d, d, d), (d, d)), albedo_scale=albedo_scale)
    assert torch.equal(ga["kd"], gb["kd"]) and torch.equal(ga["rm"], gb["rm"])
    for k in range(6):
        assert torch.equal(a[k], b[k]), "output %d differs" % k
    assert float(a[3].abs().sum()) > 0, "the frame has indirect light"


def _field():
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    aabb, mn, mx = CK.material_field_args(CK.resolve_material_config(CK.material_config(bound=1.0)))
    torch.manual_seed(0)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()), seed=1)
    with torch.no_grad():
        mlp.encoder.params.mul_(2e3)
    return mlp


def test_exported_asset_indirect_hits_are_textured(EX, scene_mod, tmp_path):
    """Synthetic workspace (evaluate.py --synthetic's mesh and field), export at 1024^2 (ssaa 2), one 96^2 view, same seed.
    (a) the textured frame's PSNR against the field's frame: 51.2 dB measured on an MI355X (64 spp; 50.9 dB at 16 spp; the floor leaves a margin);
    (b) with the texture replaced by its mean at the INDIRECT hits only (a second material in the render, the full texture in the G-buffer), the indirect
        outputs 3-5 move further from the field's frame than those of the full textured frame (measured: indirect MSE 2.58e-6 against 2.01e-6)."""
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, harness
    v, f = scene_mod.make_mesh(5, 16)
    mlp = _field()
    EX.export_stage1(str(tmp_path), v, f, [0, v.shape[0]], [0, f.shape[0]], mlp, texture_size=1024, ssaa=2, log=None)
    m = EX.load_stage1(str(tmp_path), roughness_min=0.08)
    assert torch.equal(m.verts.cpu(), torch.from_numpy(v)) and torch.equal(m.tris.cpu(), torch.from_numpy(f))
    env = torch.from_numpy(scene_mod.make_env(64, 128)).cuda()
    w = _gbuffer_worker(m.verts, m.tris)
    S, spp, seed = 96, 64, 4242
    pose, intr = _pose(0), _intr(S)
    field, gf = _frame(RR, harness, w, mlp, env, pose, intr, S, spp, seed, {})
    tex, gt = _frame(RR, harness, w, m, env, pose, intr, S, spp, seed, {})
    mean_planes = [p.float().mean((0, 1)).round().to(torch.uint8)[None, None].expand_as(p).contiguous() for p in m.planes]
    m_mean = EX.TexturedMaterial(m.verts, m.tris, m.vt, m.ft, m.tri_end, mean_planes, roughness_min=0.08)
    mean_ind, gm = _frame(RR, harness, w, m_mean, env, pose, intr, S, spp, seed, {}, gmat=m)
    assert torch.equal(gm["kd"], gt["kd"])
    img = lambda o, g: harness.postprocess(torch.nan_to_num(o[0], 0.0), g["occ"], S, S, 1)
    p_tex = harness.psnr(img(tex, gt), img(field, gf))
    occ = gf["occ"].view(-1) > 0.5
    mse = lambda a, b: sum(float(((a[k] - b[k])[occ] ** 2).mean()) for k in (3, 4, 5))
    e_tex, e_mean = mse(tex, field), mse(mean_ind, field)
    print("textured vs field: PSNR %.2f dB; indirect MSE textured %.4g, mean texture at indirect hits %.4g" % (p_tex, e_tex, e_mean))
    assert p_tex >= 45.0
    assert e_mean > 1.1 * e_tex


def test_render_refuses_tex_and_mat(EX, scene_mod):
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, _lib
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    v, f = scene_mod.make_mesh(2, 4)
    vt, ft, _ = EX.uv_atlas(v, f, 64, 64)
    m = EX.TexturedMaterial(v, f, vt, ft, [f.shape[0]], [np.zeros((64, 64, 8), np.uint8)])
    w = _gbuffer_worker(m.verts, m.tris)
    mlp = _field()
    ctx = get_ctx(16, 16)
    N = 256
    z = lambda c: torch.zeros((N, c), device="cuda")
    a = _lib.RenderArgs()
    keep = [z(1), z(3), z(1), z(3), z(2), z(3), z(3)] + [z(3) for _ in range(6)] + [torch.ones((8, 16, 3), device="cuda")]
    a.spp = 1; a.env_map, a.Hc, a.Wc = keep[-1].data_ptr(), 8, 16
    a.occ, a.normal, a.depth, a.kd, a.rough_metal, a.ray_dir, a.pos = (t.data_ptr() for t in keep[:7])
    for k in range(6):
        a.outs[k] = keep[7 + k].data_ptr()
    st_m = mlp._struct(); st_t = m._struct()
    a.mat = C.pointer(st_m); a.tex = C.pointer(st_t)
    assert _lib.lib().mirres_render(ctx.h, w.h, C.byref(a), _lib.stream_ptr()) == -1
    assert b"tex" in _lib.lib().mirres_last_error()
    # the stepwise / training paths cannot look a texture up by position: they refuse instead of falling back
    with pytest.raises(_lib.MirresError, match="gradient"):
        nm = torch.zeros((N, 3), device="cuda", requires_grad=True)
        RR.run_restir_di_with_pt(False, 1, 1, 1, m, None, w, *([None] * 17), torch.ones((8, 16, 3), device="cuda"), z(1), nm, z(1), z(3), z(2), z(3), z(3),
                                 None, None, None, None, 16, 16, 1, 0, 1)


def test_evaluate_synthetic_export_and_textured_mesh(tmp_path):
    ws = tmp_path / "ws"
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--synthetic", "--workspace", str(ws), "--H", "64",
                        "--W", "64", "--spp", "4", "--limit", "2", "--export_mesh", "--texture_size", "512", "--textured_mesh", str(ws / "mesh_stage1")],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("[textured")]
    assert len(lines) == 2 and all("PSNR vs field" in l for l in lines)
    assert any(f.startswith("ngp_stage1_ep0001_textured") for f in os.listdir(ws / "results_brdf"))
