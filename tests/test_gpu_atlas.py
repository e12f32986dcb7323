"""GPU: the chart atlas (csrc/atlas.hip through export.chart_atlas) against the numpy restatement of tests/atlas_refs.py, bit for bit at every stage —
normals, buckets after every round, neighbours, chart labels, bounds, UVs, flagged charts — the invariants of the finished layout checked on the bake's own
raster record, the position round trip at every covered texel, and the exported files read back through load_stage1 / mirres_texmat_lookup."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atlas_refs as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS_MIN = 0.5


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _stages_equal_restatement(EX, v, f, size, ssaa):
    """Every device stage on the restatement's inputs, then chart_atlas as a whole: equal bytes.  -> (restatement, (vt, ft, info))."""
    ref = A.atlas_ref(EX, v, f, size, size, ssaa, COS_MIN, 2)
    V = v.shape[0]
    vd = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(); fd = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    normal, bucket = EX.atlas_classify(vd, fd)
    assert np.array_equal(_bits(normal.cpu().numpy()), _bits(ref["normal"])), "normals"
    assert np.array_equal(bucket.cpu().numpy(), ref["buckets"][0]), "buckets"
    nbr = EX.manifold_neighbours(fd, V)
    assert np.array_equal(nbr.cpu().numpy(), ref["nbr"]), "manifold neighbours"
    for k in (1, 2):
        bucket = EX.atlas_smooth(normal, bucket, nbr, COS_MIN)
        assert np.array_equal(bucket.cpu().numpy(), ref["buckets"][k]), "buckets after round %d" % k
    a0 = ref["attempts"][0]
    chart, n_charts = EX.atlas_charts(fd, V, bucket, nbr)
    assert n_charts == a0["n_charts"] and np.array_equal(chart.cpu().numpy(), a0["chart"]), "chart labels"
    bounds = EX.atlas_bounds(vd, fd, bucket, chart, n_charts)
    assert np.array_equal(_bits(bounds.cpu().numpy()), _bits(a0["bounds"])), "bounds"
    t = np.nonzero(a0["chart"] >= 0)[0]
    key = np.unique((a0["chart"][t].astype(np.int64)[:, None] * max(V, 1) + f[t].astype(np.int64)).reshape(-1))
    cb = np.zeros(n_charts, np.int32); cb[a0["chart"][t]] = ref["buckets"][-1][t]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    vt_c = EX.atlas_emit(vd, dev(key // max(V, 1), np.int32), dev(key % max(V, 1), np.int32), dev(cb, np.int32), bounds, dev(a0["origin"].reshape(-1, 2), np.int32),
                         a0["density"], size, size)
    assert np.array_equal(_bits(vt_c.cpu().numpy()), _bits(a0["vt"][:key.shape[0]])), "chart UVs"
    flagged = EX.atlas_verify(a0["vt"], a0["ft"], a0["chart"], n_charts, size * ssaa, size * ssaa)
    assert np.array_equal(flagged.cpu().numpy(), a0["flagged"]), "flagged charts"
    vt, ft, info = EX.chart_atlas(v, f, size, size, ssaa, COS_MIN, 2)
    assert np.array_equal(_bits(vt), _bits(ref["vt"])) and np.array_equal(ft, ref["ft"]) and ft.dtype == np.int32, "chart_atlas: vt / ft"
    assert np.array_equal(info["face_chart"], ref["face_chart"]) and info["face_chart"].dtype == np.int32
    assert info["n_charts"] == ref["n_charts"] and info["density"] == float(ref["density"]) and info["fallback_faces"] == int((ref["face_chart"] < 0).sum())
    assert info["seam_edges"] == EX.seam_edges(f, ft) and 0 <= info["fill"] <= 1
    final = EX.atlas_verify(vt, ft, info["face_chart"], info["n_charts"], size * ssaa, size * ssaa)
    assert not bool(final.any()), "the device check passes on the final layout"
    return ref, (vt, ft, info)


def _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, size, ssaa):
    """Invariants 1-4 with the texel owners of mirres_uv_rasterize, then 5: the position mirres_interpolate gives at EVERY covered texel.
    Chart texels: the two selected coordinates equal min + (texel centre - origin - 0.5) / s.  The triangle the barycentrics come from has its corners snapped to
    1/256 bake texel (off by at most 1/512 bake texel per axis) on top of the UVs' own rounding (delta = 4 * 2^-24 * w0 export texels, atlas_refs.stretch_bounds);
    barycentrics of the centre in a triangle whose corners moved by at most eta are the exact barycentrics of a point at most eta away, and one export texel
    is exactly 1 / s world units in the selected coordinates: ((1 / 512) / ssaa + delta) / s.  The fp32 interpolation b0 a0 + b1 a1 + (1 - b0 - b1) a2 adds at
    most 12 * 2^-24 * max |coordinate| (two rounded barycentrics, a third from two subtractions, three products, two sums).
    Fallback texels (pair / single cells) of faces with finite, in-range corners: the position equals the exact barycentric mix at the texel centre within
    the same snap (sqrt(2) eta in the plane, times the spectral norm of the face's texel -> 3D map) and interpolation terms."""
    from mirres_restir_nerf_mesh_amd import raster
    W = H = size * ssaa
    rast = EX.uv_rasterize(vt, ft, W, H)
    owner = rast[:, 3].long().cpu().numpy() - 1
    A.check_invariants(v, f, vt, ft, info["face_chart"], info["density"], ref["bounds"], ref["origin"], size, size, ssaa, COS_MIN, EX.CELL_GAP, owner=owner)
    idx = np.nonzero(owner >= 0)[0]
    if idx.size == 0:
        return
    V = v.shape[0]
    usable = ((f >= 0) & (f < V)).all(1)
    usable &= np.isfinite(v[np.where(usable[:, None], f, 0)]).all((1, 2))
    f_safe = np.where(usable[:, None], f, 0).astype(np.int32)                   # mirres_interpolate trusts its indices
    xyz = raster.interpolate(torch.from_numpy(np.nan_to_num(v)).cuda(), rast[torch.from_numpy(idx).cuda()], torch.from_numpy(f_safe).cuda()).cpu().numpy().astype(np.float64)
    t = owner[idx]; c = info["face_chart"][t]; s = float(info["density"])
    M = np.abs(v[np.isfinite(v)]).max()
    eta = (1.0 / 512) / ssaa + 4 * A.U32 * size
    fp = 12 * A.U32 * M
    centre = np.stack(((idx % W + 0.5) / ssaa, (idx // W + 0.5) / ssaa), 1)     # export texels
    on = c >= 0
    if on.any():
        cb = np.zeros(ref["bounds"].shape[0], np.int64); cb[info["face_chart"][info["face_chart"] >= 0]] = ref["buckets"][-1][info["face_chart"] >= 0]
        b = cb[c[on]]
        got = np.stack((xyz[on, :][np.arange(on.sum()), A.AX_U[b]], xyz[on, :][np.arange(on.sum()), A.AX_V[b]]), 1)
        want = ref["bounds"][c[on], 0:2].astype(np.float64) + (centre[on] - ref["origin"][c[on]] - 0.5) / s
        err = np.abs(got - want).max()
        print("position round trip: %d chart texels, max |err| %.3g (bound %.3g)" % (on.sum(), err, eta / s + fp))
        assert err <= eta / s + fp
    off = ~on & usable[t]
    if off.any():
        tt = t[off]
        q = vt[ft[tt]].astype(np.float64) * size; p = v[f[tt]].astype(np.float64)
        E2 = np.stack((q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), 2); E3 = np.stack((p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), 2)
        J = E3 @ np.linalg.inv(E2)                                               # export texels -> world
        want = p[:, 0] + np.einsum("nij,nj->ni", J, centre[off] - q[:, 0])
        bound = np.linalg.norm(J, 2, axis=(1, 2)) * np.sqrt(2) * eta + np.sqrt(3) * fp
        err = np.linalg.norm(xyz[off] - want, axis=1)
        print("position round trip: %d fallback texels, max err / bound %.3g" % (off.sum(), (err / bound).max()))
        assert (err <= bound).all()


def test_cube(EX):
    v, f = A.cube()
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 64, 2)
    assert info["n_charts"] == 6 and info["seam_edges"] == 12 and info["fallback_faces"] == 0 and np.array_equal(info["face_chart"], np.repeat(np.arange(6), 2))
    q = vt[ft].astype(np.float64) * 64; p = v[f].astype(np.float64)
    for a, b in ((0, 1), (1, 2), (2, 0)):                                      # congruent up to s; coordinates 0 / 1: every fp32 step is exact
        assert np.array_equal(np.linalg.norm(q[:, a] - q[:, b], axis=1), info["density"] * np.linalg.norm(p[:, a] - p[:, b], axis=1))
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 64, 2)


def test_displaced_sphere(EX, scene_mod):
    v, f = scene_mod.make_mesh(3)
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 1024, 2)
    _, ft_pairs, _ = EX.uv_atlas(v, f, 1024, 1024)
    pairs = EX.seam_edges(f, ft_pairs)
    print("T %d: %d charts, %d seam edges (pair atlas %d), fill %.3f, density %.1f, %d fallback faces" % (f.shape[0], info["n_charts"], info["seam_edges"], pairs, info["fill"],
                                                                                                            info["density"], info["fallback_faces"]))
    assert 3 * info["seam_edges"] <= pairs
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 1024, 2)


def test_clustered_mesh_fewer_seams_and_deterministic(EX, scene_mod):
    v, f = scene_mod.make_mesh_clustered(20000)
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 1024, 2)
    _, ft_pairs, _ = EX.uv_atlas(v, f, 1024, 1024)
    pairs = EX.seam_edges(f, ft_pairs)
    print("T %d: %d charts, %d seam edges (pair atlas %d), fill %.3f, %d fallback faces" % (f.shape[0], info["n_charts"], info["seam_edges"], pairs, info["fill"], info["fallback_faces"]))
    assert info["seam_edges"] < pairs
    vt2, ft2, info2 = EX.chart_atlas(v, f, 1024, 1024, 2)
    assert vt.tobytes() == vt2.tobytes() and ft.tobytes() == ft2.tobytes() and info["face_chart"].tobytes() == info2["face_chart"].tobytes()
    assert all(info[k] == info2[k] for k in ("fill", "density", "n_charts", "fallback_faces", "seam_edges"))
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 1024, 2)


def test_helicoid_falls_back(EX):
    v, f = A.helicoid()
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 256, 2)
    assert ref["attempts"][0]["n_charts"] == 1 and ref["attempts"][0]["flagged"][0] == 1
    assert info["n_charts"] == 0 and info["fallback_faces"] == 512 and (info["face_chart"] == -1).all()
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 256, 2)


def test_hostile_mesh(EX):
    v, f, name = A.hostile()
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 128, 2)
    for k in ("zero_area", "repeated", "nan", "past_v", "negative", "duplicate"):
        assert info["face_chart"][name[k]] == -1, k
    assert info["face_chart"][name["isolated"]] >= 0 and info["face_chart"][name["fin"]] >= 0 and info["fallback_faces"] == 7
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 128, 2)
    vt0, ft0, info0 = EX.chart_atlas(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 32, 32, 2)
    assert vt0.shape == (0, 2) and ft0.shape == (0, 3) and info0["n_charts"] == 0 and info0["face_chart"].shape == (0,) and info0["seam_edges"] == 0
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32); f1 = np.array([[0, 1, 2]], np.int32)
    ref1, (vt1, ft1, info1) = _stages_equal_restatement(EX, v1, f1, 32, 2)
    assert info1["n_charts"] == 1 and vt1.shape == (3, 2)
    _invariants_on_the_raster_record(EX, v1, f1, ref1, vt1, ft1, info1, 32, 2)


def test_confetti_past_two_to_the_sixteen_charts(EX):
    v, f = A.confetti()
    assert f.shape[0] == 65537 + 300
    ref, (vt, ft, info) = _stages_equal_restatement(EX, v, f, 2048, 1)
    assert info["n_charts"] == f.shape[0] > 1 << 16 and info["fallback_faces"] == 0 and info["seam_edges"] == 0
    assert np.array_equal(info["face_chart"], np.arange(f.shape[0]))
    _invariants_on_the_raster_record(EX, v, f, ref, vt, ft, info, 2048, 1)


# ------------------------------------------------------------------------------------------------------------------------------- end to end
FIELD_A = np.array([[0.05, -0.03, 0.02, 0.0, 0.04, -0.02], [0.02, 0.04, -0.04, 0.0, -0.03, 0.03], [-0.03, 0.02, 0.03, 0.0, 0.02, 0.04]], np.float32)


def _affine_field(x):
    return 0.5 + x @ torch.from_numpy(FIELD_A).to(x.device)


def test_export_with_charts_reads_back_within_the_derived_bound(EX, scene_mod, tmp_path):
    """export_stage1(atlas="charts") on the synthetic workspace's mesh (scripts/evaluate.py: make_mesh(5, 16)) as cascade 0 and the same mesh scaled by 2 as
    cascade 1, 2048^2, ssaa 2, a field affine in position; the files read back by read_obj / load_stage1; mirres_texmat_lookup at the centroid of EVERY face.
    Bound = LSB + |grad| * reach:
    - a bake texel holds floor(255 srgb(L)), decoded by the lookup's table: at most one table step below L; the 2 x 2 downsample's byte lies between the
      smallest and the largest of its four bytes, and the bilinear mix is convex: the result is at most LSB = the largest table step in the field's range away
      from the field at SOME source position among the bake texels the taps read;
    - reach: the four taps' bake texels lie within 1.25 sqrt(2) export texels of the centroid's UV.  The disc of radius (2/3) r_in about the centroid lies in
      the face (r_in = the UV inradius; the centroid is at least 2/3 r_in from every edge) and every disc of radius sqrt(2)/2 bake texels holds a texel centre,
      so an uncovered tap texel has a covered one of the same face within 1.25 sqrt(2) - (2/3) r_in + sqrt(2) / ssaa; asserted below 1.75 export texels, the
      least distance to another chart's texels (rectangles CELL_GAP apart, geometry half a texel inside: 3 texels, less the taps' 1.25), so every source lies in
      the face's own chart, within 2 * 1.25 sqrt(2) export texels of the centroid; a chart face stretches 3D -> texels by at least s cos_min.
    The assumptions (no fallback faces, r_in) are asserted on the layout before the comparison."""
    v0, f0 = scene_mod.make_mesh(5, 16)
    v = np.concatenate((v0, v0 * np.float32(2))); f = np.concatenate((f0, f0 + v0.shape[0]))
    files = EX.export_stage1(str(tmp_path), v, f, [0, v0.shape[0], v.shape[0]], [0, f0.shape[0], f.shape[0]], mlp=None, texture_size=2048, ssaa=2, field=_affine_field,
                             atlas="charts", log=None)
    assert len(files) == 8
    m = EX.load_stage1(str(tmp_path), roughness_min=0.08)
    assert torch.equal(m.verts.cpu(), torch.from_numpy(v)) and torch.equal(m.tris.cpu(), torch.from_numpy(f.astype(np.int32)))
    decode = EX.srgb_decode_table().numpy().astype(np.float64)
    lsb = np.diff(decode)[decode[1:] <= 0.9].max()
    grad = np.linalg.norm(FIELD_A.astype(np.float64), axis=0).max()
    worst = 0.0
    for cas, scale in ((0, 1.0), (1, 2.0)):
        vo, vto, fo, fto = EX.read_obj(str(tmp_path / ("mesh_%d.obj" % cas)))
        vt = np.stack((vto[:, 0], np.float32(1) - vto[:, 1]), 1)
        vt_c, ft_c, info = EX.chart_atlas(vo, fo, 2048, 2048, 2)
        assert np.array_equal(ft_c, fto) and np.abs(vt_c - vt).max() <= 2 ** -23, "the OBJ holds the chart layout"
        assert info["fallback_faces"] == 0 and vto.shape[0] < 2 * vo.shape[0]
        q = vt_c[ft_c].astype(np.float64) * 2048
        e = [np.linalg.norm(q[:, a] - q[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))]
        area = 0.5 * np.abs(np.linalg.det(np.stack((q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), 2)))
        r_in = 2 * area / (e[0] + e[1] + e[2])
        assert (1.25 * np.sqrt(2) - (2.0 / 3) * r_in + np.sqrt(2) / 2 < 1.75).all(), "a face too small for the bound's derivation: r_in %.2f" % r_in.min()
        reach = 2 * 1.25 * np.sqrt(2) / (info["density"] * COS_MIN)
        bound = lsb + grad * reach + 1e-6
        n0 = 0 if cas == 0 else f0.shape[0]
        prim = torch.arange(n0, n0 + f0.shape[0], dtype=torch.int32)
        cen = vo[fo].astype(np.float64).mean(1)
        kd, rm = m.lookup(prim.cuda(), torch.from_numpy(cen.astype(np.float32)).cuda())
        want = 0.5 + cen @ FIELD_A.astype(np.float64)
        err = np.abs(np.concatenate((kd.cpu().numpy(), rm.cpu().numpy()), 1) - want[:, [0, 1, 2, 4, 5]]).max()
        print("cascade %d: density %.1f, max |err| %.4f, bound %.4f (LSB %.4f + gradient %.3f x reach %.4f)" % (cas, info["density"], err, bound, lsb, grad, reach))
        worst = max(worst, err / bound)
        assert err <= bound
    assert worst > 0.05, "an error this far below one LSB means the comparison is not looking at the textures"


def test_export_script_charts_and_default_unchanged(EX, tmp_path):
    """scripts/export_stage1.py --synthetic --atlas charts exits 0 in a fresh process; without --atlas its files equal export_stage1(atlas="pairs")'s, byte for byte."""
    ws = tmp_path / "ws"
    base = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "export_stage1.py"), "--synthetic", "--workspace", str(ws), "--texture_size", "512", "--ssaa", "2"]
    r = subprocess.run(base + ["--out", str(tmp_path / "charts"), "--atlas", "charts"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "chart atlas fill" in r.stdout
    vo, vto, fo, fto = EX.read_obj(str(tmp_path / "charts" / "mesh_0.obj"))
    assert (fto >= 0).all() and fto.max() < vto.shape[0] and vto.shape[0] < 2 * vo.shape[0]
    r = subprocess.run(base + ["--out", str(tmp_path / "default")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import export_stage1 as S
    verts, t, v_cumsum, f_cumsum, mlp = S.load(str(ws), str(ws / "checkpoints" / "ngp_stage1_ep0001.pth"))
    EX.export_stage1(str(tmp_path / "pairs"), verts, t, v_cumsum, f_cumsum, mlp, texture_size=512, ssaa=2, atlas="pairs", log=None)
    for name in ("mesh_0.obj", "mesh_0.mtl", "feat0_0.png", "feat1_0.png"):
        assert open(tmp_path / "default" / name, "rb").read() == open(tmp_path / "pairs" / name, "rb").read(), name
