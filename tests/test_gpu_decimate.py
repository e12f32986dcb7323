"""Quadric edge-collapse decimation on the device (csrc/decimate.hip, stage0.decimate_mesh / decimate_round): per-edge cost, placement, validity and keys against
the float64 restatement (tests/decimate_refs.py), the selection against the stated rule exactly, one applied round, whole runs (invariants, quality against the
sequential greedy reference, flat regions, a boundary, hostile and smallest shapes, determinism) and scripts/export_stage0.py --decimate_target end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage0_refs as R      # noqa: E402
import decimate_refs as D    # noqa: E402

# NOT YET MEASURED ON THE MI355X: no GPU run could be made when these tests were written.  The figures below come from a float64 emulation of the device's rounds
# with tests/decimate_refs.py (edge_table + select + the apply rule); the first GPU run has to print the device's own figures (run with -s) and confirm or replace them.
# Test 1.  cost: |device - restatement| / scale, scale = (sum of the plane weights in Q[a] + Q[b]) * (largest squared distance from the origin in the edge's region),
# the size of the terms that cancel in v^T Q v.  Device and restatement evaluate the same correctly rounded fp64 operations in the same order (the library is built
# without contraction), so the expected difference is 0, and 16 x 0 bounds nothing; the bound is instead what ONE differently associated fp64 sum over the ~64
# plane terms of a region may cost, 64 * 2^-53, times the 16 the comparison is allowed.
COST_BOUND = 16 * 64 * 2.0 ** -53
# position: fp32 roundings of an fp64 solve.  The number format's own precision is the bound: one fp32 ulp of the region's radius.
POS_BOUND = 2.0 ** -23
# Tests 5 and 7: bound = ratio x 1.25.  Emulated ratios device / greedy: 1.0000 on all four meshes — the rounds' result EQUALS the greedy result there, face for face
# (symmetric RMS sphere4 2.518537e-03, mc40 1.599972e-03, torus 4.481674e-03; relative volume change 3.772e-03, 2.680e-03, 6.382e-03; hemisphere 9.525e-03).
RMS_RATIO_MEASURED = {"sphere4": 1.0, "mc40": 1.0, "torus": 1.0}
VOL_RATIO_MEASURED = {"sphere4": 1.0, "mc40": 1.0, "torus": 1.0}
BOUNDARY_RATIO_MEASURED = 1.0

GOLDEN = os.path.join(ROOT, "tests", "golden", "decimate_greedy.npz")
TET = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32))
EDGE_INPUTS = {"ico3": lambda: D.perturbed_icosphere(3), "hemi": lambda: D.hemisphere(3), "cube": lambda: D.grid_cube(12)}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


_rounds, _tables, _runs = {}, {}, {}


def first_round(S0, name, opt):
    """Round 1 of the device on a per-edge input towards half its faces -> (input v, t, output v, q, t, info as numpy)."""
    if (name, opt) not in _rounds:
        v, t = EDGE_INPUTS[name]()
        ov, oq, ot, info = S0.decimate_round(cu(v), None, cu(t), len(t) // 2, opt)
        info = {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in info.items()}
        _rounds[(name, opt)] = (v, t, ov.cpu().numpy(), oq.cpu().numpy(), ot.cpu().numpy(), info)
    return _rounds[(name, opt)]


def table(name, opt):
    if (name, opt) not in _tables:
        _tables[(name, opt)] = D.edge_table(*EDGE_INPUTS[name](), optimal=opt)
    return _tables[(name, opt)]


def whole_run(S0, gold, name):
    """The device's whole run on a quality input -> (input v, t, target, output v, t, log lines)."""
    if name not in _runs:
        if name == "mc40":
            mv, mt = S0.marching_cubes(D.synthetic_volume_np(40), 10.0)                 # stage0.synthetic_volume's scene, evaluated in numpy: the CPU tests cut the same volume
            mv, mt = S0.clean_mesh(S0.index_to_world(mv, 40), mt)
            v, t = mv.cpu().numpy(), mt.cpu().numpy()
            target = len(t) // 5
        else:
            v, t, target = {"sphere4": lambda: R.icosphere(4) + (1000,), "torus": lambda: D.torus() + (800,), "hemi": lambda: D.hemisphere(3) + (len(D.hemisphere(3)[1]) // 4,)}[name]()
        lines = []
        ov, ot = S0.decimate_mesh(cu(v), cu(t), target, log=lines.append)
        _runs[name] = (v, t, target, ov.cpu().numpy(), ot.cpu().numpy(), lines)
    return _runs[name]


def greedy_of(gold, name, v, t, target):
    """The greedy reference's result on a quality input: the recorded one (tests/golden, checked against a fresh run by tests/test_decimate_refs.py) when the
    input is the recorded input bit for bit, else a fresh run."""
    if name != "mc40" or (np.array_equal(v, gold["mc40_in_v"]) and np.array_equal(t, gold["mc40_in_t"])):
        return gold[name + "_v"], gold[name + "_t"]
    return D.greedy_decimate(v, t, target)


# ------------------------------------------------------------------------------------------------ 1 per-edge quantities
@pytest.mark.parametrize("opt", [True, False])
@pytest.mark.parametrize("name", ["ico3", "hemi", "cube"])
def test_per_edge_quantities_equal_the_restatement(S0, name, opt):
    v, t, _, _, _, info = first_round(S0, name, opt)
    tab = table(name, opt)
    assert info["E"] == tab["E"] and np.array_equal(info["ekeys"], tab["ekeys"]) and np.array_equal(info["emult"], tab["emult"])
    assert np.array_equal(info["vflag"], tab["vflag"])
    q = info["quadrics"]
    qscale = np.abs(tab["quadrics"]).max(axis=1, keepdims=True) + 1e-300
    print("%s opt %d: quadrics max rel diff %.3e" % (name, opt, float((np.abs(q - tab["quadrics"]) / qscale).max())))
    assert (np.abs(q - tab["quadrics"]) <= 64 * 2.0 ** -53 * qscale).all()
    near = tab["near"]
    assert near.mean() <= 0.01
    use = ~near
    assert np.array_equal(info["flags"][use], tab["flags"][use]), np.nonzero(info["flags"] != tab["flags"])[0][:10]
    for bit in (D.F_MULT, D.F_LINK, D.F_BOUNDARY, D.F_FLIP, D.F_FINITE):                       # every reason on its own
        assert np.array_equal((info["flags"][use] & bit) != 0, (tab["flags"][use] & bit) != 0), bit
    dc = np.abs(info["cost"] - tab["cost"])[use] / tab["scale"][use]
    radius = np.sqrt(tab["scale"][use] / np.maximum(tab["quadrics"][tab["ea"]][:, [0, 4, 7]].sum(1) + tab["quadrics"][tab["eb"]][:, [0, 4, 7]].sum(1), 1e-300)[use])
    dp = np.abs(info["position"].astype(np.float64) - tab["pos"].astype(np.float64)).max(axis=1)[use] / radius
    print("%s opt %d: E %d, %d valid, %d near a threshold; max scaled cost diff %.3e, max scaled position diff %.3e" % (name, opt, tab["E"], int((tab["flags"] == 0).sum()), int(near.sum()),
                                                                                                                    float(dc.max()), float(dp.max())))
    assert dc.max() <= COST_BOUND and dp.max() <= POS_BOUND
    valid = use & (tab["flags"] == 0)
    want = np.array([D.cost_key(c, e) for e, c in enumerate(info["cost"])], np.int64)           # the key is the device's own fp32 cost and the edge id
    assert np.array_equal(info["keys"][valid], want[valid]) and (info["keys"][info["flags"] != 0] == D.KEY_NONE).all() and (info["keys"] >= 0).all()


# ------------------------------------------------------------------------------------------------ 2 selection
@pytest.mark.parametrize("name", ["ico3", "hemi", "cube"])
def test_selection_is_the_stated_rule_exactly(S0, name):
    v, t, _, _, _, info = first_round(S0, name, True)
    T = len(t); n = (T - T // 2 + 1) // 2
    order = np.sort(info["keys"])
    n_cand = min(n, int((order != D.KEY_NONE).sum()))
    assert n_cand > 10 and np.array_equal(info["cand"], (order[:n_cand] & 0xFFFFFFFF).astype(np.int32))          # the n smallest valid keys, cheapest first
    ea, eb = info["ekeys"] >> 32, info["ekeys"] & 0xFFFFFFFF
    got = np.sort(info["cand"][info["sel"] != 0].astype(np.int64))
    assert np.array_equal(got, D.select(t, ea, eb, info["keys"], info["cand"])) and len(got) == info["selected"] > 0
    assert (info["flags"][got] == 0).all() and set(got) <= set(info["cand"].tolist())
    assert info["cand"][0] in got                                                                             # the globally smallest candidate
    tt = [tuple(r) for r in t.astype(np.int64).tolist()]
    vf = D.vertex_faces(D.topology(t, len(v)), len(v))
    seen = set()
    for e in got:
        reg = D.region(int(ea[e]), int(eb[e]), tt, vf)
        assert not (reg & seen), "regions overlap at edge %d" % e
        seen |= reg


# ------------------------------------------------------------------------------------------------ 3 one round applied
@pytest.mark.parametrize("name", ["ico3", "hemi", "cube"])
def test_one_round_applies_exactly_the_selected_collapses(S0, name):
    v, t, ov, oq, ot, info = first_round(S0, name, True)
    ea, eb = info["ekeys"] >> 32, info["ekeys"] & 0xFFFFFFFF
    sel = info["cand"][info["sel"] != 0].astype(np.int64)
    remap = np.arange(len(v)); remap[eb[sel]] = ea[sel]
    assert np.array_equal(info["remap"], remap)
    mapped = remap[t.astype(np.int64)]
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    assert np.array_equal(info["keep"].astype(bool), keep)
    assert (~keep).sum() == info["emult"][sel].sum() == len(t) - len(ot)                                      # exactly the faces on the selected edges disappear
    moved = v.copy(); moved[ea[sel]] = info["position"][sel]
    rv, rt = R.compact(moved, mapped, keep)                                                                    # order-preserving: every other face is unchanged up to remap
    assert np.array_equal(ot, rt) and np.array_equal(ov.view(np.uint32), rv.view(np.uint32))
    q = info["quadrics"].copy(); q[ea[sel]] = info["quadrics"][ea[sel]] + info["quadrics"][eb[sel]]            # one fp64 addition per component: bit for bit
    used = np.zeros(len(v), bool); used[mapped[keep].reshape(-1)] = True
    assert np.array_equal(oq.view(np.uint64), q[used].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 4, 5, 9 whole runs
@pytest.mark.parametrize("name", ["sphere4", "mc40", "torus"])
def test_whole_runs_keep_the_invariants(S0, gold, name):
    v, t, target, ov, ot, lines = whole_run(S0, gold, name)
    assert target - 1 <= len(ot) <= target and not any("WARN" in l for l in lines)
    assert any(l == "[INFO] mesh decimation: %s --> %s, %s --> %s" % (v.shape, ov.shape, t.shape, ot.shape) for l in lines)
    assert ov.dtype == np.float32 and ot.dtype == np.int32 and D.invariants(ov, ot)
    assert R.mesh_edges_ok(ot)
    assert R.euler_characteristic(len(ov), ot) == R.euler_characteristic(len(v), t) == {"sphere4": 2, "mc40": 2, "torus": 0}[name]
    assert len(np.unique(R.components(ot))) == len(np.unique(R.components(t))) == 1
    assert R.signed_volume(ov, ot) > 0
    if name == "sphere4":
        p = ov[ot.astype(np.int64)].astype(np.float64)
        assert (np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(axis=1)) > 0).all()       # every normal points away from the centre


def test_quality_against_the_greedy_reference(S0, gold):
    for name in ("sphere4", "mc40", "torus"):
        v, t, target, ov, ot, _ = whole_run(S0, gold, name)
        gv, gt = greedy_of(gold, name, v, t, target)
        rms_d, rms_g = D.symmetric_rms(v, t, ov, ot), D.symmetric_rms(v, t, gv, gt)
        vol = R.signed_volume(v, t)
        dv_d, dv_g = abs(R.signed_volume(ov, ot) - vol) / vol, abs(R.signed_volume(gv, gt) - vol) / vol
        print("%s: symmetric RMS device %.6e greedy %.6e ratio %.4f; relative volume change device %.6e greedy %.6e ratio %.4f" % (name, rms_d, rms_g, rms_d / rms_g, dv_d, dv_g, dv_d / dv_g))
        assert rms_d / rms_g <= 1.5                                                                            # past this the candidate rule is to be fixed, not the bound
        assert rms_d / rms_g <= RMS_RATIO_MEASURED[name] * 1.25
        assert dv_d / dv_g <= VOL_RATIO_MEASURED[name] * 1.25


def test_runs_are_deterministic(S0, gold):
    v, t, target, ov, ot, _ = whole_run(S0, gold, "sphere4")
    ov2, ot2 = S0.decimate_mesh(cu(v), cu(t), target)
    assert torch.equal(ov2.cpu(), torch.from_numpy(ov)) and torch.equal(ot2.cpu(), torch.from_numpy(ot))


# ------------------------------------------------------------------------------------------------ 6 flat regions
@pytest.mark.parametrize("opt", [True, False])
def test_gridded_cube_stays_a_cube(S0, opt):
    v, t = D.grid_cube(12)
    assert len(t) == 1728
    ov, ot = S0.decimate_mesh(cu(v), cu(t), 200, optimalplacement=opt)
    ov, ot = ov.cpu().numpy(), ot.cpu().numpy()
    assert 199 <= len(ot) <= 200 and D.invariants(ov, ot) and R.mesh_edges_ok(ot)
    assert np.abs(np.abs(ov).max(axis=1) - 0.5).max() <= 1e-5 and np.abs(ov).max() <= 0.5 + 1e-5           # every vertex on the surface
    corners = (np.abs(np.abs(ov) - 0.5) <= 1e-5).all(axis=1)
    assert corners.sum() == 8 and len(np.unique(np.sign(ov[corners]), axis=0)) == 8
    assert abs(R.signed_volume(ov, ot) - 1.0) <= 1e-4


# ------------------------------------------------------------------------------------------------ 7 boundary
def test_open_hemisphere_keeps_its_boundary_loop(S0, gold):
    v, t, target, ov, ot, lines = whole_run(S0, gold, "hemi")
    assert target - 1 <= len(ot) <= target and D.invariants(ov, ot)
    assert D.boundary_loops(t) == (1, True, True) and D.boundary_loops(ot) == (1, True, True)                # one loop, two boundary edges per boundary vertex, manifold inside
    assert R.euler_characteristic(len(ov), ot) == 1

    def worst(vv, tt):
        tp = D.topology(tt, len(vv)); tp0 = D.topology(t, len(v))
        bnd = np.unique(np.concatenate([tp["ea"][tp["emult"] == 1], tp["eb"][tp["emult"] == 1]]))
        a, b = v[tp0["ea"][tp0["emult"] == 1]].astype(np.float64), v[tp0["eb"][tp0["emult"] == 1]].astype(np.float64)
        p = vv[bnd].astype(np.float64)[:, None, :]
        s = np.clip(((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(-1), 0, 1)
        return float(np.sqrt(((p - (a + s[..., None] * (b - a))) ** 2).sum(-1)).min(axis=1).max())
    w_d, w_g = worst(ov, ot), worst(gold["hemi_v"], gold["hemi_t"])
    print("hemisphere: worst boundary vertex off the original boundary polyline: device %.6e greedy %.6e ratio %.4f" % (w_d, w_g, w_d / w_g))
    assert w_d <= w_g * BOUNDARY_RATIO_MEASURED * 1.25


# ------------------------------------------------------------------------------------------------ 8 hostile and smallest shapes
def test_tetrahedron_stalls_at_once(S0):
    lines = []
    ov, ot = S0.decimate_mesh(cu(TET[0]), cu(TET[1]), 2, log=lines.append)
    assert np.array_equal(ov.cpu().numpy(), TET[0]) and np.array_equal(ot.cpu().numpy(), TET[1])
    assert sum("[WARN]" in l for l in lines) == 1 and "4 faces" in [l for l in lines if "[WARN]" in l][0] and "stall" in [l for l in lines if "[WARN]" in l][0]


def test_non_manifold_parts_are_left_as_they_are(S0):
    sv, st = R.icosphere(2)
    # two tetrahedra that share one vertex
    t2v = np.concatenate([TET[0] + 3, -TET[0][1:] + 3], 0); t2t = np.concatenate([TET[1], np.where(TET[1] == 0, 0, TET[1] + 3)[:, [0, 2, 1]]], 0)
    # three faces on one edge
    fv = np.array([[5, 0, 0], [5, 0, 1], [6, 0, 0.5], [5, 1, 0.5], [4.3, -0.7, 0.5]], np.float32); ft = np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], np.int32)
    v, t = R.join([(sv, st), (t2v.astype(np.float32), t2t.astype(np.int32)), (fv, ft)])
    lines = []
    ov, ot = S0.decimate_mesh(cu(v), cu(t), 100 + 8 + 3, log=lines.append)
    ov, ot = ov.cpu().numpy(), ot.cpu().numpy()
    assert np.isfinite(ov).all() and D.invariants(ov, ot)
    assert len(ot) in (110, 111) or any("stall" in l for l in lines)
    n = len(ov)
    assert np.array_equal(ov[n - 12:], v[len(sv):]) and np.array_equal(ot[-11:] - (n - 12), t[len(st):] - len(sv))        # both non-manifold pieces, untouched and in place
    assert R.mesh_edges_ok(ot[:-11]) and R.euler_characteristic(n - 12, ot[:-11]) == 2


def test_zero_area_faces_and_identical_vertices_give_a_finite_mesh(S0):
    sv, st = R.icosphere(2)
    v = np.concatenate([sv, sv[[7]], [[0, 0, 2], [1, 0, 2], [2, 0, 2]]], 0).astype(np.float32)                # vertex 162 is vertex 7 again, bit for bit
    t = st.copy(); rows = np.nonzero((t == 7).any(axis=1))[0][:2]; t[rows] = np.where(t[rows] == 7, 162, t[rows])
    t = np.concatenate([t, [[163, 164, 165], [7, 162, 20]]], 0).astype(np.int32)                                # a collinear face and a face without area between the twins
    ov, ot = S0.decimate_mesh(cu(v), cu(t), 120)
    ov, ot = ov.cpu().numpy(), ot.cpu().numpy()
    assert np.isfinite(ov).all() and len(ot) <= len(t) and ot.min() >= 0 and ot.max() < len(ov)


def test_nothing_to_do_and_bad_inputs(S0):
    sv, st = R.icosphere(1)
    v, t = cu(sv), cu(st)
    for target in (len(st), len(st) + 5):
        ov, ot = S0.decimate_mesh(v, t, target)
        assert ov.cpu().numpy().tobytes() == sv.tobytes() and ot.cpu().numpy().tobytes() == st.tobytes()
    ov, ot = S0.decimate_mesh(v, t[:0], 10)
    assert ov.cpu().numpy().tobytes() == sv.tobytes() and tuple(ot.shape) == (0, 3)
    bad = sv.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        S0.decimate_mesh(cu(bad), t, 20)
    tb = st.copy(); tb[5, 2] = len(sv)
    with pytest.raises(ValueError, match="out of range"):
        S0.decimate_mesh(v, cu(tb), 20)
    tb[5, 2] = -1
    with pytest.raises(ValueError, match="out of range"):
        S0.decimate_mesh(v, cu(tb), 20)


def test_max_rounds_stops_after_exactly_one_round(S0):
    sv, st = R.icosphere(3)
    lines = []
    ov, ot = S0.decimate_mesh(cu(sv), cu(st), 100, max_rounds=1, log=lines.append)
    r1 = S0.decimate_round(cu(sv), None, cu(st), 100)
    assert torch.equal(ov, r1[0]) and torch.equal(ot, r1[2]) and 100 < ot.shape[0] < len(st)
    assert sum("[WARN]" in l for l in lines) == 1 and "max_rounds" in [l for l in lines if "[WARN]" in l][0] and "%d faces" % ot.shape[0] in [l for l in lines if "[WARN]" in l][0]
    ov, ot = S0.decimate_mesh(cu(sv), cu(st), 100)                                                            # the library is usable afterwards
    assert ot.shape[0] in (99, 100)


# ------------------------------------------------------------------------------------------------ 10 end to end
def test_export_stage0_decimates_end_to_end(S0, tmp_path):
    ws = str(tmp_path / "ws")
    script = os.path.join(ROOT, "scripts", "export_stage0.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--workspace", ws, "--resolution", "64", "--decimate_target", "4000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh decimation" in r.stdout and "not built" not in r.stdout
    from mirres_restir_nerf_mesh_amd import checkpoint as CK, harness, scene
    from mirres_restir_nerf_mesh_amd.renderer_restir import restirbvhWorker
    v, t, vc, fc = CK.load_stage0_mesh(ws, 1)
    assert 3999 <= len(t) <= 4000 and len(np.unique(R.components(t))) == 1 and R.signed_volume(v, t) > 0
    W = restirbvhWorker(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()); W.update_mesh(W.vrt, W.v_ind)
    poses, intr = R.orbit_cameras(1, 3.0, 32, 32)
    env = torch.from_numpy(scene.make_env(32, 64)).cuda()
    img = harness.test_view(W, None, env, torch.from_numpy(poses[0]), intr, 32, 32, 2)
    assert tuple(img.shape) == (32, 32, 3) and torch.isfinite(img).all() and float(img.min()) >= 0 and float((img < 0.999).float().mean()) > 0.05
    # the default target (3e5) is above this mesh: nothing is decimated and the file is the cleaned marching-cubes mesh, as before
    r2 = subprocess.run([sys.executable, script, "--synthetic", "--workspace", ws, "--resolution", "64", "--overwrite"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "mesh decimation" not in r2.stdout and "WARN" not in r2.stdout, r2.stdout + r2.stderr
    v2, t2, _, _ = CK.load_stage0_mesh(ws, 1)
    mv, mt = S0.marching_cubes(S0.synthetic_volume(64), 10.0)
    cv, ct = S0.clean_mesh(S0.index_to_world(mv, 64), mt)
    assert np.array_equal(v2, cv.cpu().numpy()) and np.array_equal(t2, ct.cpu().numpy())
