"""CPU: the restatements the decimation tests rely on (tests/decimate_refs.py) hold on their own — the selection rule on a hand-made key assignment, the per-edge
rules on the smallest shapes, how few edges of the per-edge inputs lie near a threshold, the distance helpers, and the greedy reference on every input of the GPU
quality tests (reaches the target, keeps the topology and a positive volume) together with the recorded results the GPU tests compare against."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage0_refs as R      # noqa: E402
import decimate_refs as D    # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "decimate_greedy.npz")


def quality_inputs():
    """name -> (vertices, triangles, target) of the GPU quality and boundary tests; the marching-cubes mesh is cut on the CPU from the same numpy volume."""
    hv, ht = D.hemisphere(3)
    mv, mt = D.mc_mesh_np(40)
    return {"sphere4": R.icosphere(4) + (1000,), "mc40": (mv, mt, len(mt) // 5), "torus": D.torus() + (800,), "hemi": (hv, ht, len(ht) // 4)}


def test_selection_rule_on_hand_made_keys():
    # a strip of 12 faces: vertices 0 .. 13, face f = (f, f + 1, f + 2); the edge (i, i + 1) has the region {i - 2 .. i + 3}
    v, t = R.strip(12)
    tp = D.topology(t, len(v))
    eid = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(tp["ea"], tp["eb"]))}
    keys = np.full(tp["E"], D.KEY_NONE, np.int64)
    e01, e45, e67, e1011, e56 = eid[(0, 1)], eid[(4, 5)], eid[(6, 7)], eid[(10, 11)], eid[(5, 6)]
    keys[e45] = 10; keys[e67] = 5; keys[e01] = 7; keys[e1011] = 9; keys[e56] = 20
    # (6, 7) holds the smallest key: wins; (4, 5) overlaps it and loses although nothing else beats it there; (0, 1) = {0 .. 3} overlaps (4, 5) = {2 .. 7} at vertices 2, 3, where
    # (4, 5) wrote 10 > 7: wins; (10, 11) = {8 .. 13} overlaps (6, 7) = {4 .. 9} at 8, 9: loses; (5, 6) loses
    cand = np.array([e45, e67, e01, e1011, e56])
    assert D.select(t, tp["ea"], tp["eb"], keys, cand).tolist() == sorted([e67, e01])
    assert D.select(t, tp["ea"], tp["eb"], keys, np.array([e45, e1011, e56])).tolist() == sorted([e45, e1011])      # without (6, 7) and (0, 1): disjoint regions both win
    assert D.select(t, tp["ea"], tp["eb"], keys, np.array([e56])).tolist() == [e56]
    # the order of the candidates does not matter
    assert D.select(t, tp["ea"], tp["eb"], keys, cand[::-1]).tolist() == sorted([e67, e01])


def test_tetrahedron_has_no_valid_edge_and_a_flat_fan_collapses_for_free():
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32); tt = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32)
    tab = D.edge_table(tv, tt)
    assert tab["E"] == 6 and (tab["flags"] & D.F_LINK).all() and (tab["keys"] == D.KEY_NONE).all()
    ov, ot = D.greedy_decimate(tv, tt, 2)
    assert np.array_equal(ov, tv) and np.array_equal(ot, tt)
    # a closed icosahedron: every edge passes the link condition
    ov_, ot_ = R.icosphere(0)
    assert not (D.edge_table(ov_, ot_)["flags"] & D.F_LINK).any()
    # the gridded cube: quadrics of flat vertices are singular, the three-way choice costs exactly nothing inside a face and the corners stay
    v, t = D.grid_cube(4)
    tab = D.edge_table(v, t)
    inner = (np.abs(v) == 0.5).sum(axis=1)
    flat = (inner[tab["ea"]] == 1) & (inner[tab["eb"]] == 1) & (tab["flags"] == 0)
    assert flat.sum() > 50 and (tab["cost"][flat] == 0).all()
    corner_moves = ((inner[tab["ea"]] == 3) | (inner[tab["eb"]] == 3)) & (tab["flags"] == 0)
    on = np.abs(np.abs(tab["pos"][corner_moves]) - 0.5).max(axis=1) < 1e-6
    assert on.all()                                                       # a valid collapse at a corner keeps the corner


def test_zero_area_faces_give_no_nan():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    t = np.array([(0, 1, 2), (0, 1, 3), (1, 4, 3), (1, 2, 4)], np.int32)                  # the first face is collinear
    tab = D.edge_table(v, t)
    assert np.isfinite(tab["quadrics"]).all() and np.isfinite(tab["cost"]).all() and np.isfinite(tab["pos"]).all()


@pytest.mark.parametrize("name", ["ico3", "hemi", "cube"])
def test_few_edges_of_the_per_edge_inputs_lie_near_a_threshold(name):
    v, t = {"ico3": lambda: D.perturbed_icosphere(3), "hemi": lambda: D.hemisphere(3), "cube": lambda: D.grid_cube(12)}[name]()
    for opt in (True, False):
        tab = D.edge_table(v, t, opt)
        assert tab["near"].mean() <= 0.01, (name, opt, tab["near"].mean())
        assert (tab["flags"] == 0).sum() > tab["E"] // 4                   # and the input exercises valid and invalid edges alike
    if name == "hemi":
        assert D.boundary_loops(t) == (1, True, True) and (tab["flags"] & D.F_BOUNDARY).any()


def test_distance_helpers():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64); t = np.array([[0, 1, 2]])
    pts = np.array([[0.25, 0.25, 2.0], [-1, -1, 0], [2, 0, 0], [0.5, -3, 0], [1, 1, 0], [0.2, 0.2, 0]], np.float64)
    want = [2.0, 2 ** 0.5, 1.0, 3.0, 0.5 ** 0.5, 0.0]
    assert np.allclose(D.point_mesh_distance(pts, v, t), want, atol=1e-12)
    sv, st = R.icosphere(2)
    assert D.symmetric_rms(sv, st, sv, st) < 1e-7
    assert abs(D.rms_distance(sv * 1.5, sv, st) - 0.5) < 1e-6


@pytest.mark.parametrize("name", ["sphere4", "mc40", "torus", "hemi"])
def test_greedy_reference_on_the_quality_inputs(name):
    v, t, target = quality_inputs()[name]
    ov, ot = D.greedy_decimate(v, t, target)
    assert target - 1 <= len(ot) <= target, len(ot)
    assert D.invariants(ov, ot)
    assert R.euler_characteristic(len(ov), ot) == R.euler_characteristic(len(np.unique(t)), t)
    assert len(np.unique(R.components(ot))) == len(np.unique(R.components(t)))
    if name == "hemi":
        assert D.boundary_loops(ot) == (1, True, True) and D.boundary_loops(t) == (1, True, True)
    else:
        assert R.mesh_edges_ok(ot) and R.mesh_edges_ok(t) and R.signed_volume(ov, ot) > 0
    g = np.load(GOLDEN)                                                   # what the GPU tests load instead of running the reference again
    assert np.array_equal(g[name + "_v"], ov) and np.array_equal(g[name + "_t"], ot)
    if name == "mc40":
        assert np.array_equal(g["mc40_in_v"], v) and np.array_equal(g["mc40_in_t"], t)
