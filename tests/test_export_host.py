"""CPU (no GPU calls): the stage-1 mesh export's host side (mirres_restir_nerf_mesh_amd/export.py) — UV atlas, OBJ / MTL files, cascade sizes,
argument checks — and the numpy restatements (tests/bake_refs.py) that tests/test_gpu_export.py holds the HIP bake against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bake_refs as R


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _meshes(scene_mod):
    return [("sphere", 512, *scene_mod.make_mesh(4, 8)), ("clustered", 1024, *scene_mod.make_mesh_clustered(4000))]


def _cells(vt, ft, w0, h0):
    """Export-texel box (x0, y0, x1, y1) of every triangle's UV image."""
    p = vt[ft.astype(np.int64)] * np.array([w0, h0], np.float64)
    return np.concatenate((p.min(1), p.max(1)), 1)


def test_atlas_layout(EX, scene_mod):
    for name, size, v, f in _meshes(scene_mod):
        vt, ft, fill = EX.uv_atlas(v, f, size, size)
        T = f.shape[0]
        assert ft.shape == (T, 3) and ft.dtype == np.int32 and vt.dtype == np.float32 and ft.min() >= 0 and ft.max() < vt.shape[0]
        assert (vt >= 0).all() and (vt <= 1).all(), name
        box = _cells(vt, ft, size, size)
        assert np.array_equal(box, np.round(box)), "cells sit on the export-texel grid"
        cells, inv = np.unique(box.astype(np.int64), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        assert np.bincount(inv).max() <= 2, "a cell holds one pair or one triangle"
        # disjoint with >= 2 texels between: the cells' texel rectangles grown by one texel on every side never overlap
        grid = np.zeros((size + 2, size + 2), np.int32)
        for x0, y0, x1, y1 in cells:
            assert x1 - x0 == y1 - y0 >= 2
            grid[y0:y1 + 2, x0:x1 + 2] += 1
        assert grid.max() == 1, name
        # pairs: share a 3D edge and its two UV points, and fill the square
        pairs, singles = EX.pair_triangles(f)
        assert 2 * pairs.shape[0] + singles.shape[0] == T and len(set(pairs[:, :2].ravel()) | set(singles)) == T
        for t, u, a, b in pairs:
            assert inv[t] == inv[u]
            assert {a, b} <= set(f[t]) and {a, b} <= set(f[u])
            for x in (a, b):
                assert ft[t][list(f[t]).index(x)] == ft[u][list(f[u]).index(x)]
        # every triangle (of nonzero 3D area or not) has a UV image of nonzero area
        q = vt[ft.astype(np.int64)].astype(np.float64)
        uv_area = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])
        area3 = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
        assert (uv_area[area3 > 0] != 0).all()
        # deterministic; the fill is only reported
        vt2, ft2, fill2 = EX.uv_atlas(v, f, size, size)
        assert np.array_equal(vt, vt2) and np.array_equal(ft, ft2) and fill == fill2
        print("%s: T=%d pairs=%d singles=%d fill=%.3f" % (name, T, pairs.shape[0], singles.shape[0], fill))
        assert fill > 0.2


def test_atlas_too_small_is_an_error(EX, scene_mod):
    v, f = scene_mod.make_mesh(4, 8)
    with pytest.raises(ValueError, match="do not fit"):
        EX.uv_atlas(v, f, 32, 32)


def _cover_count(vt, ft, W, H):
    """How many triangles cover each texel centre, each rasterised on its own."""
    n = np.zeros(H * W, np.int64)
    for t in range(len(ft)):
        tid, _, _ = R.raster_ref(vt, ft[t:t + 1], W, H)
        n += tid >= 0
    return n


def test_raster_ref_shared_edge_covers_each_centre_once():
    W = H = 8
    vt = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    for ft in (np.array([[0, 1, 2], [0, 2, 3]]), np.array([[0, 2, 1], [0, 2, 3]]), np.array([[0, 1, 2], [0, 3, 2]])):    # either winding
        assert (_cover_count(vt, ft, W, H) == 1).all()
        tid, _, _ = R.raster_ref(vt, ft, W, H)
        tid = tid.reshape(H, W)
        assert (tid[np.tril_indices(W, -1)] == 1).all() and (tid[np.triu_indices(W, 1)] == 0).all()   # row > col: above the diagonal v = u
    # a fan of four triangles around a centre that lies on every edge: still each texel exactly once
    vt = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [4.5 / 8, 3.5 / 8]], np.float32)
    ft = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])
    assert (_cover_count(vt, ft, 8, 8) == 1).all()


def test_raster_ref_barycentrics_and_interior():
    rng = np.random.default_rng(3)
    W, H = 40, 24
    for _ in range(20):
        vt = rng.uniform(-0.1, 1.1, (3, 2)).astype(np.float32)
        for ft in (np.array([[0, 1, 2]]), np.array([[0, 2, 1]])):
            tid, b0, b1 = R.raster_ref(vt, ft, W, H)
            c, r = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
            p = np.stack((c.ravel(), r.ravel()), 1)
            q = vt[ft[0]].astype(np.float64)
            A = np.array([[q[0, 0] - q[2, 0], q[1, 0] - q[2, 0]], [q[0, 1] - q[2, 1], q[1, 1] - q[2, 1]]])
            bb = np.linalg.solve(A, (p - q[2]).T).T
            inside = (bb[:, 0] > 1e-3) & (bb[:, 1] > 1e-3) & (1 - bb.sum(1) > 1e-3)
            outside = (bb[:, 0] < -1e-3) | (bb[:, 1] < -1e-3) | (1 - bb.sum(1) < -1e-3)
            assert (tid[inside] == 0).all() and (tid[outside] == -1).all()
            cov = tid == 0
            assert np.abs(b0[cov] - bb[cov, 0]).max(initial=0) < 1e-3 and np.abs(b1[cov] - bb[cov, 1]).max(initial=0) < 1e-3


def test_raster_ref_degenerate_and_overlap():
    vt = np.array([[0.1, 0.1], [0.5, 0.5], [0.9, 0.9], [0.1, 0.9], [0.9, 0.1]], np.float32)
    tid, _, _ = R.raster_ref(vt, np.array([[0, 1, 2], [0, 0, 3], [2, 2, 2]]), 16, 16)
    assert (tid == -1).all(), "zero-area triangles cover nothing"
    tid, _, _ = R.raster_ref(vt, np.array([[0, 3, 2], [0, 4, 2], [0, 2, 3]]), 16, 16)
    assert set(np.unique(tid)) == {-1, 0, 1}, "triangle 2 = triangle 0 reversed: the lower index wins everywhere"
    big = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    tid, _, _ = R.raster_ref(big, np.array([[0, 3, 2], [0, 1, 2]]), 16, 16)
    both = _cover_count(big, np.array([[0, 3, 2], [0, 1, 2]]), 16, 16) == 2
    assert both.any() and (tid[both] == 0).all()


def _same_raster(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_raster_small_ref_equals_raster_ref():
    """The vectorised restatement the many-triangle GPU test is held against is the loop restatement: ids and barycentrics equal to the last bit on the first
    6 000 triangles of that test's input (both diagonals, both windings, 17 zero-area triangles) and on 3 000 small random triangles across the atlas border
    (clamped boxes, boxes off the grid, overlaps: the lowest index wins); a box beyond maxbox is refused; chunk_first counts ceil(bw * bh / 32) work items per triangle on a case worked by hand."""
    vt, ft, n_small = R.cell_grid_input()
    W = H = 1024
    part = ft[:6000]
    assert (part[:, 0] == part[:, 1]).sum() == 6000 // 349
    want = R.raster_ref(vt, part, W, H)
    got = R.raster_small_ref(vt, part, W, H, 2)
    assert _same_raster(got, want) and len(np.unique(want[0][want[0] >= 0])) == 6000 - 6000 // 349 and (want[0] >= 0).sum() >= 4 * ((6000 - 6000 // 349) // 2)
    rng = np.random.default_rng(9)
    W, H = 48, 40
    c = np.where(rng.random((3000, 1, 2)) < 0.5, rng.choice([0.0, 1.0], (3000, 1, 2)), rng.uniform(0, 1, (3000, 1, 2)))     # a coordinate on the border or anywhere
    uv = (c + rng.uniform(-2.5, 2.5, (3000, 3, 2)) / np.array([W, H])).astype(np.float32).reshape(-1, 2)
    tri = np.arange(9000).reshape(-1, 3)
    tri[::7] = tri[::7][:, [0, 2, 1]]; tri[5::50, 2] = 9000; tri[6::50, 1] = -1                                               # some reversed, some out of range
    uv[30::301] = np.nan; uv[31::301] = np.inf
    s = R.tri_setup(uv, tri, W, H)
    assert s["bw"].max() <= 6 and s["bh"].max() <= 6 and (s["bw"] == 0).sum() > 100 and ((s["bw"] > 0) & (s["bw"] < 5) & (s["c0"] == 0)).any()
    want = R.raster_ref(uv, tri, W, H)
    assert _same_raster(R.raster_small_ref(uv, tri, W, H, 6), want) and (want[0] >= 0).mean() > 0.5 and (want[0] < 0).any()
    with pytest.raises(AssertionError, match="maxbox"):
        R.raster_small_ref(uv, tri, W, H, int(max(s["bw"].max(), s["bh"].max())) - 1)
    # boxes of 16 x 16 = 256, 0 and 7 x 5 = 35 texels: 8, 0 and 2 work items
    hand = np.array([[0, 0], [1, 0], [0, 1], [7 / 16, 0], [0, 5 / 16]], np.float32)
    assert R.chunk_first(hand, np.array([[0, 1, 2], [0, 0, 1], [0, 3, 4]]), 16, 16).tolist() == [0, 8, 8, 10]


def test_obj_and_mtl_format(EX, tmp_path, scene_mod):
    v, f = scene_mod.make_mesh(2, 4)
    v = v * np.float32(1.2345678) + np.float32(1e-6)
    vt, ft, _ = EX.uv_atlas(v, f, 256, 256)
    EX.write_obj(str(tmp_path / "mesh_3.obj"), v, vt, f, ft, cas=3)
    EX.write_mtl(str(tmp_path / "mesh_3.mtl"), cas=3)
    lines = open(tmp_path / "mesh_3.obj").read().split("\n")
    assert lines[0] == "mtllib mesh_3.mtl " and lines[-1] == ""
    V, Nt, T = v.shape[0], vt.shape[0], f.shape[0]
    assert all(l.startswith("v ") and l.endswith(" ") and len(l.split()) == 4 for l in lines[1:1 + V])
    assert all(l.startswith("vt ") and l.endswith(" ") and len(l.split()) == 3 for l in lines[1 + V:1 + V + Nt])
    assert lines[1 + V + Nt] == "usemtl defaultMat "
    fl = lines[2 + V + Nt:-1]
    assert len(fl) == T
    assert fl[0] == "f %d/%d %d/%d %d/%d " % (f[0, 0] + 1, ft[0, 0] + 1, f[0, 1] + 1, ft[0, 1] + 1, f[0, 2] + 1, ft[0, 2] + 1)
    v2, vt2, f2, ft2 = EX.read_obj(str(tmp_path / "mesh_3.obj"))
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(vt2.view(np.uint32), np.stack((vt[:, 0], np.float32(1) - vt[:, 1]), 1).view(np.uint32))     # written as (u, 1 - v)
    assert np.array_equal(f2, f) and np.array_equal(ft2, ft)
    vt3, ft3 = EX.uv_from_obj(str(tmp_path / "mesh_3.obj"), f)
    assert np.array_equal(ft3, ft) and np.abs(vt3 - vt).max() <= 2 ** -23
    assert open(tmp_path / "mesh_3.mtl").read() == ("newmtl defaultMat \nKa 1 1 1 \nKd 1 1 1 \nKs 0 0 0 \nTr 1 \nillum 1 \nNs 0 \n"
                                                     "map_Kd feat0_3.png \n")
    with pytest.raises(ValueError, match="not the mesh's triangles"):
        EX.uv_from_obj(str(tmp_path / "mesh_3.obj"), f[::-1])


def test_cascade_sizes(EX):
    assert EX.cascade_sizes(4096, 3) == [(4096, 4096), (2048, 2048), (2048, 2048)]
    assert EX.cascade_sizes(8192, 3) == [(8192, 8192), (4096, 4096), (2048, 2048)]
    assert EX.cascade_sizes(2048, 2) == [(2048, 2048), (2048, 2048)]
    assert EX.cascade_sizes(256, 2) == [(256, 256), (256, 256)]


def test_quantise_ref_is_the_reference_arithmetic():
    x = np.array([-1, 0, 0.001, 0.0031307, 0.0031309, 0.2, 0.5, 0.999, 1.0, 2.0, np.float32(0.2140)], np.float32)
    q = R.quantise_ref(x)
    lin = np.clip(x.astype(np.float32), 0, 1)
    s = np.where(lin < np.float32(0.0031308), np.float32(12.92) * lin, np.float32(1.055) * np.power(lin, np.float32(0.41666)) - np.float32(0.055))
    assert np.array_equal(q, (s * np.float32(255)).astype(np.uint8))
    assert q[0] == 0 and q[1] == 0 and q[-3] == q[-2]


def test_nearest_band_texel_is_nearest_covered_texel():
    """The premise of the windowed inpaint: for an uncovered texel the nearest texel of the search band (mask minus its 3-fold erosion)
    is as far as the nearest covered texel — random masks, the image border included."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, gaussian_filter
    rng = np.random.default_rng(0)
    for k in range(12):
        H, W = int(rng.integers(20, 90)), int(rng.integers(20, 90))
        noise = gaussian_filter(rng.standard_normal((H, W)), 1.0 + k % 4)
        mask = noise > np.quantile(noise, rng.uniform(0.3, 0.95))
        if k % 3 == 0:
            mask[0, :] = True; mask[:, -1] = True
        band = mask & ~binary_erosion(mask, iterations=3)
        d_cov = distance_transform_edt(~mask)
        d_band = distance_transform_edt(~band)
        assert np.array_equal(d_cov[~mask], d_band[~mask])


def test_inpaint_ref_on_a_known_case():
    mask = np.zeros((9, 9), bool); mask[4, 4] = True
    img = np.zeros((9, 9, 3), np.uint8); img[4, 4] = (10, 20, 30); img[0, 0] = 99
    out = R.inpaint_ref(mask, img, radius=2)
    l1 = np.abs(np.arange(9)[:, None] - 4) + np.abs(np.arange(9)[None, :] - 4)
    assert (out[l1 <= 2] == (10, 20, 30)).all() and (out[l1 > 2] == 0).all()


def test_downsample_ref_rule():
    img = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3)
    d = R.downsample_ref(img, 2)
    assert d[0, 0, 0] == (int(img[0, 0, 0]) + img[0, 1, 0] + img[1, 0, 0] + img[1, 1, 0] + 2) // 4
    assert np.array_equal(R.downsample_ref(img, 1), img)
    img9 = np.arange(9 * 9 * 3, dtype=np.uint8).reshape(9, 9, 3)
    assert np.array_equal(R.downsample_ref(img9, 3), img9[1::3, 1::3])


def test_argument_validation_without_gpu(EX):
    big = np.broadcast_to(np.zeros((1, 3), np.int32), (1 << 24, 3))
    v = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match="2\\^24"):
        EX.export_stage1("/nonexistent/never", v, big, [0, 3], [0, 1 << 24], mlp=None, texture_size=64, ssaa=1)
    with pytest.raises(ValueError, match="2\\^24"):
        EX.uv_rasterize(np.zeros((3, 2), np.float32), big, 64, 64)
    tri = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError, match="ssaa"):
        EX.export_stage1("/nonexistent/never", v, tri, [0, 3], [0, 1], mlp=None, texture_size=64, ssaa=0)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="texture size"):
            EX.export_stage1("/nonexistent/never", v, tri, [0, 3], [0, 1], mlp=None, texture_size=bad, ssaa=2)
    with pytest.raises(ValueError, match="texture size"):
        EX.uv_atlas(v, tri, 0, 64)
    assert not os.path.exists("/nonexistent/never")
