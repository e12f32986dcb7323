"""CPU: the chart atlas' rules as restated in tests/atlas_refs.py, run end to end with export.py's own host packing — the numbers the issue states for the
cube, the displaced sphere, the helicoid and the hostile mesh, the invariants on each — and the host pieces of export.chart_atlas: seam_edges, the
rectangle packer, the selector, and the C ABI's argument checks (which return before any device call)."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atlas_refs as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _ref_and_invariants(EX, v, f, size, ssaa):
    r = A.atlas_ref(EX, v, f, size, size, ssaa)
    A.check_invariants(v, f, r["vt"], r["ft"], r["face_chart"], r["density"], r["bounds"], r["origin"], size, size, ssaa, 0.5, EX.CELL_GAP)
    return r


def test_signature_and_selector(EX):
    sig = inspect.signature(EX.chart_atlas)
    assert list(sig.parameters) == ["v", "f", "h0", "w0", "ssaa", "cos_min", "smooth_rounds"]
    assert (sig.parameters["ssaa"].default, sig.parameters["cos_min"].default, sig.parameters["smooth_rounds"].default) == (1, 0.5, 2)
    assert inspect.signature(EX.export_stage1).parameters["atlas"].default == "pairs"
    v, f = A.cube()
    with pytest.raises(ValueError, match="atlas"):
        EX.export_stage1("/nonexistent/never", v, f, [0, 8], [0, 12], mlp=None, texture_size=64, ssaa=1, atlas="xatlas")
    with pytest.raises(ValueError):
        EX.chart_atlas(v, f, 64, 64, cos_min=1.5)
    with pytest.raises(ValueError):
        EX.chart_atlas(v, f, 0, 64)


def test_cube_six_charts_of_two_faces(EX):
    v, f = A.cube()
    r = _ref_and_invariants(EX, v, f, 64, 2)
    assert r["n_charts"] == 6 and np.array_equal(r["face_chart"], np.repeat(np.arange(6), 2)) and np.array_equal(r["buckets"][0], np.repeat(np.arange(6), 2))
    assert all(np.array_equal(b, r["buckets"][0]) for b in r["buckets"]), "relabelling leaves the cube alone"
    assert EX.seam_edges(f, r["ft"]) == 12 and (r["face_chart"] >= 0).all()
    # congruent up to the factor s: every UV edge, in export texels, is s times its 3D edge (coordinates 0 / 1 and s below 64: every step is exact)
    q = r["vt"][r["ft"]].astype(np.float64) * 64; p = v[f].astype(np.float64)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        assert np.array_equal(np.linalg.norm(q[:, a] - q[:, b], axis=1), float(r["density"]) * np.linalg.norm(p[:, a] - p[:, b], axis=1))


def test_displaced_sphere_has_a_third_of_the_pair_atlas_seams(EX, scene_mod):
    v, f = scene_mod.make_mesh(3)
    assert f.shape[0] == 1792
    r = _ref_and_invariants(EX, v, f, 1024, 2)
    _, ft_pairs, _ = EX.uv_atlas(v, f, 1024, 1024)
    seams, seams_pairs = EX.seam_edges(f, r["ft"]), EX.seam_edges(f, ft_pairs)
    n0 = A.charts_ref(r["buckets"][0], r["nbr"])[1]
    print("seam edges: charts %d, pairs %d; charts %d without relabelling, %d with; fallback %d" % (seams, seams_pairs, n0, r["n_charts"], (r["face_chart"] < 0).sum()))
    assert 3 * seams <= seams_pairs
    assert r["n_charts"] < n0, "the relabelling rounds absorb small islands"
    assert r["vt"].shape[0] < ft_pairs.max() + 1, "far fewer vt lines than the pair atlas"


def test_helicoid_is_flagged_and_falls_back(EX):
    v, f = A.helicoid()
    assert f.shape[0] == 512
    n, b = A.classify_ref(v, f)
    nz = n[:, 2].astype(np.float64) / np.linalg.norm(n.astype(np.float64), axis=1)
    assert nz.min() >= 0.986 and (b == 4).all()
    p = v[f].astype(np.float64)
    area = 0.5 * ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])).sum()
    assert abs(area - 3.43) < 0.03 and abs(np.pi * (0.8 ** 2 - 0.3 ** 2) - 1.73) < 0.01, area           # it covers its annulus twice
    r = _ref_and_invariants(EX, v, f, 256, 2)
    first = r["attempts"][0]
    assert first["n_charts"] == 1 and (first["chart"] == 0).all() and first["flagged"][0] == 1
    assert r["n_charts"] == 0 and (r["face_chart"] == -1).all() and not r["flagged"].any()


def test_hostile_mesh_classification(EX):
    v, f, name = A.hostile()
    r = _ref_and_invariants(EX, v, f, 128, 2)
    b, c = r["buckets"][-1], r["face_chart"]
    for k in ("zero_area", "repeated", "nan", "past_v", "negative"):
        assert b[name[k]] == -1 and c[name[k]] == -1, k                       # degenerate: no bucket, fallback
    assert (b[:32] == 4).all() and b[name["isolated"]] == 4 and b[name["duplicate"]] == 4
    # the fin hangs on an edge of three faces: it votes for nothing and joins nothing; the isolated triangle is a chart of its own
    assert (r["nbr"][name["fin"]] == -1).all() and (r["face_chart"] == c[name["fin"]]).sum() == 1 and (r["face_chart"] == c[name["isolated"]]).sum() == 1
    # face 0 and its copy share a two-face edge (face 0's boundary edge): one chart that covers itself, flagged, both fall back
    first = r["attempts"][0]
    assert first["chart"][0] == first["chart"][name["duplicate"]] and first["flagged"][first["chart"][0]] == 1 and first["flagged"].sum() == 1
    assert c[0] == -1 and c[name["duplicate"]] == -1 and (c[1:30] == c[1]).all() and c[1] >= 0
    # the faces with an index out of range still carry their in-range edge: the two edges of the last quad they hang on have three faces, which cuts the quad off
    assert c[30] == c[31] and c[30] not in (-1, c[1]) and (r["face_chart"] == c[30]).sum() == 2
    assert (c < 0).sum() == 7


def test_empty_and_single_face(EX):
    r = A.atlas_ref(EX, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 32, 32, 2)
    assert r["vt"].shape == (0, 2) and r["ft"].shape == (0, 3) and r["n_charts"] == 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32); f = np.array([[0, 1, 2]], np.int32)
    r = _ref_and_invariants(EX, v, f, 32, 2)
    assert r["n_charts"] == 1 and r["buckets"][-1][0] == 4 and r["vt"].shape == (3, 2)


def test_seam_edges_counts_two_face_edges_only(EX):
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 3, 5], [6, 6, 7]])       # (0,2) two faces; (0,3) three faces; a repeated-index face
    shared = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 3, 5], [6, 6, 7]])
    assert EX.seam_edges(f, shared) == 0
    split = shared.copy(); split[1] = [8, 9, 3]                                 # face 1 uses other UV vertices along (0,2): a seam
    assert EX.seam_edges(f, split) == 1
    half = shared.copy(); half[1] = [0, 9, 3]                                   # one shared UV vertex is not enough
    assert EX.seam_edges(f, half) == 1
    assert EX.seam_edges(np.zeros((0, 3), int), np.zeros((0, 3), int)) == 0
    v, fc = A.cube()
    vt, ft, _ = EX.uv_atlas(v, fc, 64, 64)
    assert EX.seam_edges(fc, ft) == 18 - EX.pair_triangles(fc)[0].shape[0], "the pair atlas: E - P, every edge but the one inside each pair"


def test_pack_rects(EX):
    rng = np.random.default_rng(4)
    w = rng.integers(1, 40, 300); h = rng.integers(1, 40, 300)
    packed = EX._pack_rects(w, h, 512, 512)
    assert packed is not None
    x, y = packed
    paint = np.zeros((512 + EX.CELL_GAP, 512 + EX.CELL_GAP), np.int32)
    for i in range(300):
        assert x[i] >= 0 and y[i] >= 0 and x[i] + w[i] <= 512 and y[i] + h[i] <= 512
        paint[y[i]:y[i] + h[i] + EX.CELL_GAP, x[i]:x[i] + w[i] + EX.CELL_GAP] += 1
    assert paint.max() == 1, "rectangles CELL_GAP texels apart"
    order = np.argsort(-h, kind="stable")
    assert (np.diff(y[order]) >= 0).all(), "tallest first, stable"
    assert EX._pack_rects(w, h, 128, 128) is None and EX._pack_rects(np.array([600]), np.array([1]), 512, 512) is None
    assert EX._pack_rects(np.zeros(0, np.int64), np.zeros(0, np.int64), 8, 8) is not None


def test_entry_points_reject_bad_arguments_without_a_device():
    from mirres_restir_nerf_mesh_amd._lib import lib
    L = lib()
    big = 1 << 24
    assert L.mirres_atlas_classify(None, 3, None, big, None, None, None) < 0 and b"mirres_atlas_classify" in L.mirres_last_error()
    assert L.mirres_atlas_classify(None, 3, None, 4, None, None, None) < 0                      # NULL with T > 0
    assert L.mirres_atlas_classify(None, 0, None, 0, None, None, None) == 0                     # NULL with T = 0
    assert L.mirres_atlas_smooth(None, None, None, 4, 0.5, None, None) < 0
    assert L.mirres_atlas_smooth(None, None, None, 0, 1.5, None, None) < 0 and b"cos_min" in L.mirres_last_error()
    assert L.mirres_atlas_smooth(None, None, None, 0, float("nan"), None, None) < 0
    assert L.mirres_atlas_smooth(None, None, None, 0, 0.5, None, None) == 0
    assert L.mirres_atlas_bounds(None, 3, None, 4, None, None, 5, None, None) < 0               # more charts than faces
    assert L.mirres_atlas_bounds(None, 0, None, 0, None, None, 0, None, None) == 0
    assert L.mirres_atlas_emit(None, 3, None, None, 4, None, None, None, 1, 1.0, 64, 64, None, None) < 0
    assert L.mirres_atlas_emit(None, 3, None, None, 0, None, None, None, 0, 1.0, 0, 64, None, None) < 0     # grid size
    assert L.mirres_atlas_emit(None, 3, None, None, 0, None, None, None, 0, -1.0, 64, 64, None, None) < 0   # density
    assert L.mirres_atlas_emit(None, 0, None, None, 0, None, None, None, 0, 1.0, 64, 64, None, None) == 0
    assert L.mirres_atlas_verify_scratch(big, 64, 64) == -1 and L.mirres_atlas_verify_scratch(4, 65537, 4) == -1 and L.mirres_atlas_verify_scratch(4, 65536, 65536) == -1
    assert L.mirres_atlas_verify_scratch(0, 64, 64) >= 2 * 64 * 64 // 8
    one = (C.c_uint8 * 1)()
    assert L.mirres_atlas_verify(None, 0, None, big, None, 0, 64, 64, one, None, 0, None) < 0 and b"2^24" in L.mirres_last_error()
    assert L.mirres_atlas_verify(None, 0, None, 4, None, 0, 64, 64, one, None, 0, None) < 0    # NULL with T > 0
    assert L.mirres_atlas_verify(None, 0, None, 0, None, 0, 0, 64, one, None, 0, None) < 0
    assert L.mirres_atlas_verify(None, 0, None, 0, None, 0, 64, 64, None, None, 0, None) < 0


def test_scripts_take_the_atlas_flag():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import evaluate
    a, _ = evaluate.parse_args(["--synthetic", "--export_mesh", "--atlas", "charts"])
    assert a.atlas == "charts" and evaluate.parse_args(["--synthetic"])[0].atlas == "pairs"
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--synthetic", "--atlas", "xatlas"])
