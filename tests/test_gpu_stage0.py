"""The stage-0 extraction on the device (csrc/mcubes.hip) through the C ABI: marching cubes bit for bit against the numpy restatement (tests/stage0_refs.py, same
generated table, same fp32 expressions), surface properties, the checkpoint's density grid, visibility marking against raster.rasterize's own output, ring
dilatation, compaction, edge-connected components against scipy, cleaning, and scripts/export_stage0.py --synthetic end to end; last, the same kernels at sizes
where the second level of their prefix sums has more than one workgroup total per scan thread, each test asserting on the host that its input gets there."""
import ctypes as C
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


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


def _mc_abi(vol, iso):
    """(rc_count, rc_emit, verts, tris) through the C ABI."""
    from mirres_restir_nerf_mesh_amd import _lib as L
    lib = L.lib()
    nx, ny, nz = vol.shape
    v = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda()
    nb = int(lib.mirres_mc_scratch_bytes(nx, ny, nz))
    assert nb > 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    counts = (C.c_int * 2)(-1, -1)
    rc = lib.mirres_mc_count(L.ptr(v), nx, ny, nz, float(iso), L.ptr(scratch), nb, counts, L.stream_ptr())
    if rc:
        return rc, None, None, None
    V, T = counts[0], counts[1]
    verts = torch.full((V, 3), -7.0, dtype=torch.float32, device="cuda"); tris = torch.full((T, 3), -7, dtype=torch.int32, device="cuda")
    rc2 = lib.mirres_mc_emit(L.ptr(v), nx, ny, nz, float(iso), L.ptr(scratch), L.ptr(verts) if V else None, V, L.ptr(tris) if T else None, T, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, rc2, verts.cpu().numpy(), tris.cpu().numpy()


def _check_mc(vol, iso, what, ref=None):
    rc, rc2, v, t = _mc_abi(vol, iso)
    assert rc == 0 and rc2 == 0, what
    rv, rt = ref if ref is not None else R.marching_cubes(vol, iso)
    assert t.shape == rt.shape and np.array_equal(t, rt), "%s: triangles differ (%s vs %s)" % (what, t.shape, rt.shape)
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32)), "%s: %d of %d vertex words differ" % (
        what, int((v.view(np.uint32) != rv.view(np.uint32)).sum()) if v.shape == rv.shape else -1, rv.size)
    return v, t


def test_all_256_single_cells():
    rng = np.random.default_rng(1)
    for cfg in range(256):
        inside = np.array([(cfg >> c) & 1 for c in range(8)], bool)
        vals = np.where(inside, 0.5 + rng.random(8), 0.5 - rng.random(8) - 1e-3).astype(np.float32)
        vol = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            vol[c & 1, (c >> 1) & 1, (c >> 2) & 1] = vals[c]
        v, t = _check_mc(vol, 0.5, "configuration %d" % cfg)
        assert len(t) == R.NTRI[cfg]


@pytest.mark.parametrize("shape", [(5, 7, 9), (40, 33, 70)])
def test_random_volumes_bit_equal(shape):
    vol = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32)
    v, t = _check_mc(vol, 0.1, "random %s" % (shape,))
    assert len(t) > 0 and t.min() == 0 and t.max() == len(v) - 1


def test_values_on_the_iso_level_and_non_finite_values():
    rng = np.random.default_rng(5)
    vol = rng.normal(size=(9, 8, 11)).astype(np.float32)
    flat = vol.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:60]] = 0.25; flat[idx[60:80]] = np.nan; flat[idx[80:100]] = np.inf; flat[idx[100:120]] = -np.inf
    flat[idx[120:130]] = np.finfo(np.float32).max; flat[idx[130:140]] = 1e-42          # a subnormal
    v, t = _check_mc(vol, 0.25, "hostile volume")
    assert np.isfinite(v).all() and (v >= 0).all() and (v <= np.array(vol.shape, np.float32) - 1).all()
    _check_mc(vol, 0.0, "hostile volume, iso 0 (the value NaN becomes)")


def test_no_crossing_and_bad_sizes():
    from mirres_restir_nerf_mesh_amd import _lib as L
    rc, rc2, v, t = _mc_abi(np.zeros((6, 5, 4), np.float32), 1.0)
    assert rc == 0 and rc2 == 0 and v.shape == (0, 3) and t.shape == (0, 3)
    rc, rc2, v, t = _mc_abi(np.full((3, 3, 3), 5.0, np.float32), 1.0)
    assert rc == 0 and rc2 == 0 and len(v) == 0 and len(t) == 0
    lib = L.lib()
    buf = torch.zeros(64, device="cuda"); counts = (C.c_int * 2)()
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 2, 2), (-3, 2, 2)):
        assert lib.mirres_mc_scratch_bytes(*dims) == L.lib().mirres_mc_scratch_bytes(*dims) < 0
        assert lib.mirres_mc_count(L.ptr(buf), dims[0], dims[1], dims[2], 0.5, L.ptr(buf), 256, counts, L.stream_ptr()) == -1
        assert lib.mirres_mc_emit(L.ptr(buf), dims[0], dims[1], dims[2], 0.5, L.ptr(buf), L.ptr(buf), 1, L.ptr(buf), 1, L.stream_ptr()) == -1
    assert lib.mirres_mc_count(None, 4, 4, 4, 0.5, L.ptr(buf), 256, counts, L.stream_ptr()) == -1
    assert lib.mirres_mc_count(L.ptr(buf), 4, 4, 4, float("nan"), L.ptr(buf), 256, counts, L.stream_ptr()) == -1
    assert lib.mirres_mc_count(L.ptr(buf), 4, 4, 4, 0.5, L.ptr(buf), 8, counts, L.stream_ptr()) == -1 and b"scratch" in lib.mirres_last_error()


def test_random_closed_surface_is_a_two_manifold_of_edges(S0):
    vol = np.random.default_rng(11).normal(size=(24, 24, 24)).astype(np.float32)
    vol[0] = vol[-1] = -3; vol[:, 0] = vol[:, -1] = -3; vol[:, :, 0] = vol[:, :, -1] = -3
    v, t = S0.marching_cubes(vol, 0.0)
    t = t.cpu().numpy()
    assert len(t) > 5000 and R.mesh_edges_ok(t)


def test_sphere_topology_orientation_and_determinism(S0):
    ax = np.linspace(-1, 1, 48, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    sd = (np.sqrt(x * x + y * y + z * z) - np.float32(0.7)).astype(np.float32)
    dens = np.maximum(-40 * sd, 0).astype(np.float32)
    v, t = S0.marching_cubes(dens, 10.0)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert R.mesh_edges_ok(tn) and R.euler_characteristic(len(vn), tn) == 2 and R.signed_volume(vn, tn) > 0
    vs, ts = S0.marching_cubes(-torch.from_numpy(sd), 0.0)                      # --sdf: (-vol, 0)
    assert R.mesh_edges_ok(ts.cpu().numpy()) and R.euler_characteristic(len(vs), ts.cpu().numpy()) == 2 and R.signed_volume(vs.cpu().numpy(), ts.cpu().numpy()) > 0
    v2, t2 = S0.marching_cubes(dens, 10.0)
    assert vn.tobytes() == v2.cpu().numpy().tobytes() and tn.tobytes() == t2.cpu().numpy().tobytes()
    w = S0.index_to_world(v, 48).cpu().numpy()
    assert np.abs(np.linalg.norm(w, axis=1) - 0.45).max() < 0.03               # density 10 lies 0.25 inside radius 0.7


def test_density_grid_of_a_checkpoint(S0, tmp_path):
    S = 16
    ax = np.linspace(-1, 1, S, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (np.maximum(30 * (0.8 - np.sqrt(x * x + 1.5 * y * y + 2 * z * z)), 0) + np.random.default_rng(2).random((S, S, S)) * 0.01).astype(np.float32)
    grid = np.zeros((2, S ** 3), np.float32)
    grid[0][S0.morton_indices(S).reshape(-1)] = vol.reshape(-1); grid[1] = 99.0
    ck = {"model": {"density_grid": torch.from_numpy(grid)}, "mean_density": 4.5}
    got = S0.unpack_density_grid(ck["model"]["density_grid"]).cpu().numpy()
    assert np.array_equal(got, vol) and np.array_equal(got, R.unpack_morton(grid[0], S))
    v0, t0 = S0.marching_cubes(vol, 4.5)
    lines = []
    out = S0.export_stage0(str(tmp_path), ckpt=ck, min_f=0, min_d=0, log=lines.append)
    assert any("cascade 0 only" in l for l in lines)
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    v, t = CK.read_ply(out)
    assert np.array_equal(t, t0.cpu().numpy()) and np.array_equal(v, S0.index_to_world(v0, S).cpu().numpy())
    with pytest.raises(FileExistsError):
        S0.export_stage0(str(tmp_path), ckpt=ck, log=lines.append)
    # a denser volume beside the checkpoint is masked by the nearest-upsampled grid > thresh (F.interpolate's index rule)
    Rr = 40
    dense = np.random.default_rng(4).random((Rr, Rr, Rr)).astype(np.float32) * 9 + 1
    dense[3, 3, 3] = np.nan; dense[20, 20, 20] = np.inf
    want = torch.from_numpy(dense) * (torch.nn.functional.interpolate(torch.from_numpy(vol)[None, None], size=[Rr] * 3, mode="nearest")[0, 0] > 4.5)
    got = S0.mask_by_density_grid(dense, vol, 4.5).cpu()
    assert torch.equal(torch.nan_to_num(got, 0), torch.nan_to_num(want, 0)) and torch.equal(torch.isnan(got), torch.isnan(want))


# ------------------------------------------------------------------------------------------------ visibility, dilation, removal
@pytest.fixture(scope="module")
def hidden_cube_scene(S0):
    """An icosphere (320 faces) with a small closed cube hidden inside it, 6 cameras at 64 x 64; the last face of the mesh belongs to the cube."""
    from mirres_restir_nerf_mesh_amd import harness
    v, t = R.join([R.icosphere(2, 1.0), R.cube(0.1)])
    poses, intr = R.orbit_cameras(6, 3.0, 64, 64)
    mvps = [harness.mvp_from_pose(torch.from_numpy(p).cuda(), intr, 64, 64) for p in poses]
    return dict(v=v, t=t, mvps=mvps, n_sphere=320, n_sphere_v=162)


def test_seen_faces_equal_the_ids_of_the_rasteriser(S0, hidden_cube_scene):
    from mirres_restir_nerf_mesh_amd import raster, _lib as L
    from mirres_restir_nerf_mesh_amd.renderer_restir import restirbvhWorker
    sc = hidden_cube_scene
    v, t = torch.from_numpy(sc["v"]).cuda(), torch.from_numpy(sc["t"]).cuda()
    T = len(sc["t"])
    seen = S0.seen_faces(v, t, sc["mvps"], 64, 64).cpu().numpy()
    W = restirbvhWorker(v, t); W.update_mesh(v, t)
    ids = set(); background = 0
    for mvp in sc["mvps"]:
        rast, _ = raster.rasterize(raster.RasterizeContext(W), (torch.nn.functional.pad(v, (0, 1), value=1.0) @ mvp.t())[None], t, (64, 64), grad_db=False, mvp=mvp)
        k = rast[..., 3].long().reshape(-1).cpu().numpy()
        background += int((k == 0).sum()); ids |= set((k[k > 0] - 1).tolist())
    assert background > 0 and len(ids) > 100
    want = np.zeros(T, np.uint8); want[sorted(ids)] = 1
    assert np.array_equal(seen, want)
    assert seen[-1] == 0 and not seen[sc["n_sphere"]:].any()                      # background marks nothing (not the last face); no cube face is seen
    assert np.array_equal(S0.mark_unseen_triangles(v, t, sc["mvps"], 64, 64).cpu().numpy(), want == 0)
    # id 0 and ids beyond T mark nothing
    rast = torch.zeros((5, 4), device="cuda"); rast[1, 3] = 3.0; rast[2, 3] = T + 1.0; rast[3, 3] = float("nan"); rast[4, 3] = -2.0
    flags = torch.zeros(T + 1, dtype=torch.uint8, device="cuda")
    assert L.lib().mirres_mesh_mark_seen(L.ptr(rast), 5, T, L.ptr(flags), L.stream_ptr()) == 0
    assert flags.cpu().numpy().nonzero()[0].tolist() == [2]


@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_dilation_rings_equal_the_restatement(S0, hidden_cube_scene, k):
    sc = hidden_cube_scene
    seen = S0.seen_faces(sc["v"], sc["t"], sc["mvps"], 64, 64).cpu().numpy()
    for sel in (seen, np.eye(1, len(sc["t"]), 17, dtype=np.uint8)[0]):
        got = S0.dilate_selection(sc["t"], len(sc["v"]), sel, k).cpu().numpy()
        assert np.array_equal(got.astype(bool), R.dilate(sc["t"], len(sc["v"]), sel, k)), k


def test_remove_masked_trigs_drops_the_hidden_cube_and_keeps_the_order(S0, hidden_cube_scene):
    sc = hidden_cube_scene
    unseen = S0.mark_unseen_triangles(sc["v"], sc["t"], sc["mvps"], 64, 64)
    v, t = S0.remove_masked_trigs(sc["v"], sc["t"], unseen, dilation=5)
    assert np.array_equal(t.cpu().numpy(), sc["t"][: sc["n_sphere"]]) and np.array_equal(v.cpu().numpy(), sc["v"][: sc["n_sphere_v"]])
    # an arbitrary mask, no dilation: order-preserving compaction against the restatement
    mask = np.random.default_rng(8).random(len(sc["t"])) < 0.6
    v, t = S0.remove_masked_trigs(sc["v"], sc["t"], mask, dilation=0)
    rv, rt = R.compact(sc["v"], sc["t"], ~mask)
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(t.cpu().numpy(), rt)


# ------------------------------------------------------------------------------------------------ cleaning
def _dirty_mesh():
    """Pieces in order: icosphere (320 faces, with 3 of its vertices duplicated bit for bit and one face repeated with rotated indices, a zero-area face), a 6-face
    fragment, a tiny far-away closed tetrahedron, two 10-face fans touching at one vertex only, an unreferenced vertex."""
    sv, st = R.icosphere(2, 1.0)
    dup = np.array([5, 40, 100]); sv2 = np.concatenate([sv, sv[dup]], 0)           # duplicated vertices 162, 163, 164
    st2 = st.copy()
    for j, d in enumerate(dup):
        rows = np.nonzero((st2 == d).any(axis=1))[0][:2]                           # two of the faces around d use the duplicate instead
        st2[rows] = np.where(st2[rows] == d, 162 + j, st2[rows])
    extra = np.array([st2[7][[1, 2, 0]], [0, 1, 1], [10, 10, 10]], np.int32)        # a duplicate face (rotated), two faces with a repeated index
    sphere = (np.concatenate([sv2, np.array([[0, 0, 2], [1, 0, 2], [2, 0, 2]], np.float32)], 0), np.concatenate([st2, extra, np.array([[165, 166, 167]], np.int32)], 0))   # + a collinear (zero-area) face
    fan = lambda c, z, n: (np.array([[c, 0, z]] + [[c + 0.6 * np.cos(a), 0.6 * np.sin(a), z] for a in np.linspace(0, np.pi, n + 1)], np.float32),
                           np.array([(0, i + 1, i + 2) for i in range(n)], np.int32))
    frag = fan(3.0, 0.0, 6)
    tet = (np.array([[8, 8, 8], [8.01, 8, 8], [8, 8.01, 8], [8, 8, 8.01]], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32))
    fa = fan(0.0, 3.0, 10)
    fb_v, fb_t = fan(0.0, 3.0, 10); fb_v = fb_v * np.array([1, -1, 1], np.float32); fb_t = fb_t[:, [0, 2, 1]]
    fb_v[0] = fa[0][0]                                                              # the second fan's centre is bit-identical to the first one's: merged, then shared
    lone = (np.array([[4, 4, 4]], np.float32), np.zeros((0, 3), np.int32))
    return R.join([sphere, frag, tet, fa, (fb_v, fb_t), lone])


def _scipy_labels(tris):
    from test_stage0_host import _scipy_labels as f
    return f(tris)


def test_components_equal_scipy_and_ignore_shared_vertices(S0):
    v, t = _dirty_mesh()
    lab, rounds = S0.face_components(t)
    lab = lab.cpu().numpy()
    assert np.array_equal(lab, _scipy_labels(t)) and np.array_equal(lab, R.components(t)) and 1 <= rounds <= 64
    assert all(lab[f] == np.nonzero(lab == lab[f])[0].min() for f in range(len(t)))
    # after the vertex merge the two fans share ONE vertex and still are two components
    vc, tc = S0.clean_mesh(v, t, min_f=0, min_d=0)
    lc = S0.face_components(tc)[0].cpu().numpy()
    assert np.array_equal(lc, _scipy_labels(tc.cpu().numpy()))
    tcn = tc.cpu().numpy()
    fans = [l for l in np.unique(lc) if (lc == l).sum() == 10]
    assert len(fans) == 2 and len(set(tcn[lc == fans[0]].reshape(-1)) & set(tcn[lc == fans[1]].reshape(-1))) == 1
    perm = np.random.default_rng(6).permutation(len(t))
    assert np.array_equal(S0.face_components(t[perm])[0].cpu().numpy(), _scipy_labels(t[perm]))


def test_clean_mesh_keeps_exactly_the_expected_pieces_in_order(S0):
    v, t = _dirty_mesh()
    vc, tc = S0.clean_mesh(v, t, min_f=0, min_d=0)
    vc, tc = vc.cpu().numpy(), tc.cpu().numpy()
    # steps 1-3: 3 duplicate vertices, 3 zero-area-face vertices and the lone vertex leave; the duplicate face, the two repeated-index faces and the collinear face leave
    assert len(vc) == len(v) - 3 - 3 - 1 - 1 and len(tc) == len(t) - 4              # (- 1: the second fan's centre merges into the first one's)
    sv, st = R.icosphere(2, 1.0)
    assert np.array_equal(tc[:320], st) and np.array_equal(vc[:162], sv)            # the sphere is the clean icosphere again, order kept
    v8, t8 = S0.clean_mesh(v, t, min_f=8, min_d=5)
    v8, t8 = v8.cpu().numpy(), t8.cpu().numpy()
    # min_d = 5 % of the mesh's diagonal (~15.6, i.e. 0.78): the tetrahedron (0.017) leaves, the fans and the fragment (1.34) do not; min_f = 8: the 6-face fragment leaves; sphere and both 10-face fans stay, in order
    assert len(t8) == 320 + 10 + 10
    lab = R.components(tc); keep = np.array([(lab == l).sum() >= 8 and np.ptp(vc[tc[lab == l].reshape(-1)], axis=0).max() > 0.1 for l in lab])
    rv, rt = R.compact(vc, tc, keep)
    assert np.array_equal(t8, rt) and np.array_equal(v8, rv)
    vd, td = S0.clean_mesh(v, t, min_f=0, min_d=5)
    assert len(td) == 320 + 6 + 10 + 10


def test_strip_converges_and_a_forced_round_cap_is_an_error(S0):
    from mirres_restir_nerf_mesh_amd import _lib as L
    v, t = R.strip(3000)
    lab, rounds = S0.face_components(t)
    assert np.array_equal(lab.cpu().numpy(), np.zeros(3000, np.int32)) and rounds <= 64
    print("strip of 3000 faces: %d rounds" % rounds)
    with pytest.raises(L.MirresError, match="still changing after 1 rounds"):
        S0.face_components(t, max_rounds=1)
    lab, rounds = S0.face_components(t)                                             # the library is usable after the error
    assert not lab.any()


def test_export_stage0_synthetic_end_to_end(S0, tmp_path):
    ws = str(tmp_path / "ws")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_stage0.py"), "--synthetic", "--workspace", ws, "--resolution", "48"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "marching cubes" in r.stdout and "mesh cleaning" in r.stdout
    from mirres_restir_nerf_mesh_amd import checkpoint as CK, harness, scene
    from mirres_restir_nerf_mesh_amd.renderer_restir import restirbvhWorker
    v, t, vc, fc = CK.load_stage0_mesh(ws, 1)
    assert len(t) > 1000 and R.signed_volume(v, t) > 0
    assert len(np.unique(R.components(t))) == 1                                       # the floater is gone
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_stage0.py"), "--synthetic", "--workspace", ws], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 2 and "--overwrite" in r2.stderr
    W = restirbvhWorker(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()); W.update_mesh(W.vrt, W.v_ind)
    poses, intr = R.orbit_cameras(1, 3.0, 32, 32)
    env = torch.from_numpy(scene.make_env(32, 64)).cuda()
    img = harness.test_view(W, None, env, torch.from_numpy(poses[0]), intr, 32, 32, 2)
    assert tuple(img.shape) == (32, 32, 3) and torch.isfinite(img).all() and float(img.min()) >= 0 and float((img < 0.999).float().mean()) > 0.05


# ------------------------------------------------------------------------------------------------ past the first chunk of the second-level scans
MC_BLOCK, MC_SCAN_BLOCK = 256, 1024                                                  # csrc/mcubes.hip:25 and :26


def _scan_split(n_items):
    """How k_scan_ints (csrc/mcubes.hip:75-80) splits the workgroup totals of n_items elements -> (nb totals, `per` totals per scan thread, whether the last scan
    thread's chunk is empty (its i0 = 1023 per is not below nb), whether the last non-empty chunk is shorter than per)."""
    nb = -(-n_items // MC_BLOCK); per = -(-nb // MC_SCAN_BLOCK)
    return nb, per, (MC_SCAN_BLOCK - 1) * per >= nb, nb % per != 0


def _mc_structure(vol, iso):
    """What the kernels of csrc/mcubes.hip see of a volume, restated: the number of crossed owned edges per grid point g (k_mc_count's popc(eflags)), the point
    that owns each vertex (vertices are numbered in (g, axis) order) and the point whose cell emits each triangle (triangles are numbered in (g, table) order)."""
    v = np.nan_to_num(np.asarray(vol, np.float32), nan=0.0, posinf=R.FLT_MAX, neginf=-R.FLT_MAX)
    nx, ny, nz = v.shape
    inside = v >= np.float32(iso)
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    n_edges = cross.reshape(-1, 3).sum(1)
    cfg = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1                              # corner c of a cell (csrc/mcubes.hip:36)
        cfg |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    cx, cy, cz = np.nonzero(R.NTRI[cfg] > 0)
    return n_edges, np.repeat(np.arange(n_edges.size), n_edges), np.repeat((cx * ny + cy) * nz + cz, R.NTRI[cfg[cx, cy, cz]])


def _max_block_prefix(n_edges):
    """The largest exclusive vertex prefix inside a 256-point workgroup at a point that owns a vertex: the 10-bit field of local[g] (csrc/mcubes.hip:70)."""
    b = np.zeros(-(-n_edges.size // MC_BLOCK) * MC_BLOCK, np.int64); b[:n_edges.size] = n_edges
    b = b.reshape(-1, MC_BLOCK)
    return int(((np.cumsum(b, 1) - b) * (b > 0)).max())


_MC_CASES = {}


def _mc_case(shape):
    """(volume, reference vertices, reference triangles) of normal noise in `shape`, computed once per process and read-only."""
    if shape not in _MC_CASES:
        vol = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32)
        rv, rt = R.marching_cubes(vol, 0.8)
        for a in (vol, rv, rt):
            a.setflags(write=False)
        _MC_CASES[shape] = (vol, rv, rt)
    return _MC_CASES[shape]


BIG = (67, 65, 64)                                                                  # the volume whose mesh the mesh tools below work on


# the third entry: is the last non-empty chunk of k_scan_ints shorter than `per` (three of the four shapes)
@pytest.mark.parametrize("shape,far,ragged", [((3, 3, 40000), False, True), ((40000, 3, 3), False, True), ((2, 131073, 2), True, False), (BIG, False, True)])
def test_marching_cubes_past_the_first_scan_chunk(shape, far, ragged):
    """Branch: k_scan_ints (csrc/mcubes.hip:75) with per = ceil(nb / MC_SCAN_BLOCK) >= 2 — the chunk loops at :80 and :83, threads whose chunk is empty, and for
    three of the four shapes a last non-empty chunk shorter than per — with the large stride of blk_v[q / MC_BLOCK] in k_mc_emit (:148) on each axis in turn.
    Host assertions before the launch: nb = ceil(points / 256) > 1024, per >= 2, (1024 - 1) per >= nb, nb % per != 0 where `ragged`; for (2, 131073, 2), whose
    x stride is 262 146 points, a triangle of the reference mesh uses a vertex owned by a point more than 1024 workgroups after the emitting cell's.
    Observed (nb, per, vertices, triangles): (3, 3, 40000) 1407, 2, 280 853, 268 345; (40000, 3, 3) 1407, 2, 281 130, 268 322; (2, 131073, 2) 2049, 3,
    349 060, 218 128, of which 1 479 triangles read 1025 workgroups ahead; (67, 65, 64) 1089, 2, 274 043, 442 622."""
    vol, rv, rt = _mc_case(shape)
    nb, per, empty, short = _scan_split(vol.size)
    print("%s: nb %d, per %d, %d vertices, %d triangles" % (shape, nb, per, len(rv), len(rt)))
    assert nb > MC_SCAN_BLOCK and per >= 2 and empty and short == ragged
    if far:
        n_edges, owner, cell = _mc_structure(vol, 0.8)
        assert len(owner) == len(rv) and len(cell) == len(rt)
        reach = owner[rt].max(1) // MC_BLOCK - cell // MC_BLOCK
        print("%d triangles read blk_v more than %d workgroups ahead (at most %d)" % (int((reach > MC_SCAN_BLOCK).sum()), MC_SCAN_BLOCK, reach.max()))
        assert (reach > MC_SCAN_BLOCK).any()
    v, t = _check_mc(vol, 0.8, "noise %s" % (shape,), ref=(rv, rt))
    assert t.min() == 0 and t.max() == len(v) - 1


@pytest.mark.parametrize("shape", [(12, 11, 13), (3, 3, 40000)])
def test_checkerboard_sets_the_top_bit_of_the_prefix_field(shape):
    """Branch: bit 9 of the 10-bit vertex prefix k_mc_count packs into local[g] under the edge flags (csrc/mcubes.hip:70), which k_mc_emit masks out with 1023
    (:148).  A checkerboard sign * (1 + u) at iso 0 crosses every edge, so a workgroup of MC_BLOCK = 256 points owns close to 3 * 256 vertices.
    Host assertion before the launch: the largest exclusive prefix inside a workgroup at a point that owns a vertex, computed as k_mc_count does, is >= 512.
    Observed: 733 at (12, 11, 13), 765 at (3, 3, 40000); the noise volumes above stop at 322."""
    rng = np.random.default_rng(sum(shape))
    x, y, z = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    vol = (np.where((x + y + z) & 1, -1.0, 1.0) * (1.0 + rng.random(shape))).astype(np.float32)
    top = _max_block_prefix(_mc_structure(vol, 0.0)[0])
    print("%s: largest prefix %d" % (shape, top))
    assert 512 <= top < 1024
    v, t = _check_mc(vol, 0.0, "checkerboard %s" % (shape,))
    assert len(v) == sum((shape[a] - 1) * shape[a - 1] * shape[a - 2] for a in range(3))      # every edge of the grid carries a vertex


def test_sphere_at_128_scans_eight_totals_per_thread(S0):
    """Branch: k_scan_ints (csrc/mcubes.hip:75) at per = 8 on the scene the export's smoke run uses, S0.synthetic_volume(128) at iso 10: a dented ball and a small
    floater, two closed surfaces of genus 0.
    Host assertion before the launch: 128^3 points are nb = 8192 workgroups of MC_BLOCK = 256, per = 8 for MC_SCAN_BLOCK = 1024 scan threads, none of them empty.
    Checked: bit-equal to the restatement, every edge shared by two triangles in opposite directions, two components of Euler characteristic 2 each, outward
    orientation, two runs byte-identical.  Observed: 27 360 vertices, 54 712 triangles, components of 140 (the floater, first in memory order) and 54 572 faces."""
    nb, per, empty, short = _scan_split(128 ** 3)
    assert (nb, per, empty, short) == (8192, 8, False, False)
    vol = S0.synthetic_volume(128).cpu().numpy()
    v, t = _check_mc(vol, 10.0, "synthetic_volume(128)")
    lab = _scipy_labels(t)
    parts = [t[lab == l] for l in np.unique(lab)]
    print("%d vertices, %d triangles, components of %s faces" % (len(v), len(t), [len(p) for p in parts]))
    assert R.mesh_edges_ok(t) and len(parts) == 2 and R.signed_volume(v, t) > 0
    assert all(R.euler_characteristic(len(np.unique(p)), p) == 2 for p in parts)
    v2, t2 = S0.marching_cubes(vol, 10.0)
    assert v.tobytes() == v2.cpu().numpy().tobytes() and t.tobytes() == t2.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def big_mesh():
    """The reference mesh of the (67, 65, 64) noise volume: both ceil(V / 256) and ceil(T / 256) exceed 1024, so every k_scan_ints of mirres_mesh_compact runs
    with per = 2, an empty last thread and a ragged last chunk."""
    vol, rv, rt = _mc_case(BIG)
    return dict(v=rv, t=rt, V=len(rv), T=len(rt))


def _keep_mask(name, T):
    keep = np.zeros(T, np.uint8)
    if name == "all": keep[:] = 1
    elif name == "last": keep[-1] = 1
    elif name == "first": keep[0] = 1
    elif name == "random": keep[:] = np.random.default_rng(12).random(T) < 0.3
    elif name == "beyond": keep[MC_SCAN_BLOCK * MC_BLOCK:] = 1
    return keep


@pytest.mark.parametrize("mask", ["all", "none", "last", "first", "random", "beyond"])
def test_compaction_past_the_first_scan_chunk(S0, big_mesh, mask):
    """Branch: both k_scan_ints launches of mirres_mesh_compact (csrc/mcubes.hip:448, :451) with per >= 2 over the totals of k_flag_sums, for masks that put the
    kept elements everywhere, nowhere, in the last or first workgroup only, at random, and ("beyond") exactly in the workgroups after the first
    MC_SCAN_BLOCK * MC_BLOCK = 262 144 faces, whose offsets come from the second entry of a scan thread's chunk on.
    Host assertion before the launch: ceil(V / 256) > 1024 and ceil(T / 256) > 1024 (per >= 2), the last scan thread's chunk empty; "beyond" keeps a face.
    Observed: V = 274 043 (1071 totals, per 2), T = 442 622 (1729 totals, per 2); "random" keeps 132 681 faces and 219 154 vertices, "beyond" 180 478 and 113 683."""
    m = big_mesh
    for n in (m["V"], m["T"]):
        nb, per, empty, short = _scan_split(n)
        assert nb > MC_SCAN_BLOCK and per >= 2 and empty
    keep = _keep_mask(mask, m["T"])
    assert keep.sum() == {"all": m["T"], "none": 0, "last": 1, "first": 1}.get(mask, keep.sum())
    if mask == "beyond":
        assert keep[MC_SCAN_BLOCK * MC_BLOCK:].all() and len(keep) > MC_SCAN_BLOCK * MC_BLOCK and not keep[:MC_SCAN_BLOCK * MC_BLOCK].any()
    rv, rt = R.compact(m["v"], m["t"], keep)
    print("%s: keeps %d faces, %d vertices" % (mask, len(rt), len(rv)))
    v, t = S0.compact_mesh(m["v"], m["t"], keep)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert t.shape == rt.shape and np.array_equal(t, rt)
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32))


@pytest.mark.parametrize("rings", [1, 3])
def test_dilation_on_a_mesh_of_many_workgroups(S0, big_mesh, rings):
    """mirres_mesh_dilate (csrc/mcubes.hip:417) over 1729 workgroups of faces and 1071 of vertices, from a random 1 % of the faces, against stage0_refs.dilate.
    Host assertion before the launch: ceil(T / 256) > 1024, the selection and its complement are not empty.  Observed: 4 501 faces selected, 46 321 after one
    ring, 122 721 after three."""
    m = big_mesh
    assert -(-m["T"] // MC_BLOCK) > MC_SCAN_BLOCK
    sel = (np.random.default_rng(13).random(m["T"]) < 0.01).astype(np.uint8)
    want = R.dilate(m["t"], m["V"], sel, rings)
    print("%d faces selected, %d after %d rings" % (sel.sum(), want.sum(), rings))
    assert 0 < sel.sum() < want.sum() < m["T"]
    got = S0.dilate_selection(m["t"], m["V"], sel, rings).cpu().numpy()
    assert np.array_equal(got.astype(bool), want)


def test_components_of_a_mesh_of_many_workgroups(S0, big_mesh):
    """mirres_mesh_components (csrc/mcubes.hip:463) on 442 622 faces in 23 733 components (noise at iso 0.8: many small pieces), against
    scipy's connected components; the hook / jump rounds stay within MESH_MAX_ROUNDS = 64 (:26).
    Host assertion before the launch: ceil(T / 256) > 1024 and the reference finds more than 1000 components, one of them larger than a workgroup.
    Observed: 23 733 components, the largest of 564 faces, 5 rounds."""
    m = big_mesh
    want = _scipy_labels(m["t"])
    sizes = np.bincount(want)
    print("%d components, the largest of %d faces" % (int((sizes > 0).sum()), sizes.max()))
    assert -(-m["T"] // MC_BLOCK) > MC_SCAN_BLOCK and (sizes > 0).sum() > 1000 and sizes.max() > MC_BLOCK
    lab, rounds = S0.face_components(m["t"])
    print("%d rounds" % rounds)
    assert np.array_equal(lab.cpu().numpy(), want) and 1 <= rounds <= 64


@pytest.mark.parametrize("S", [128, 256])
def test_unpack_density_grid_at_checkpoint_sizes(S0, S):
    """Branch: the `<< 8` step of spread3 (csrc/mcubes.hip:134), which moves bits 4-7 of a coordinate and so does nothing below S = 32; checkpoints use S = 128.
    Host assertion before the launch: S - 1 has a bit in 4-7 set; the two host restatements (the bit trick of stage0_refs.unpack_morton and the per-bit loop
    of stage0.morton_indices) agree.  Exact against both."""
    assert (S - 1) & 0xF0 and S <= 256
    grid = np.random.default_rng(S).random(S ** 3, dtype=np.float32)
    want = R.unpack_morton(grid, S)
    assert np.array_equal(want, grid[S0.morton_indices(S)])
    got = S0.unpack_density_grid(grid).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("Rr,S", [(129, 128), (200, 128), (255, 64), (128, 128)])
def test_mask_by_density_grid_at_other_ratios(S0, Rr, S):
    """k_mask_nearest (csrc/mcubes.hip:148) at ratios where floor(dst * (float)(S / R)) lands beside the exact quotient or needs its clamp: one more than the grid,
    a non-integer ratio, almost four to one, and one to one; NaN and infinities under both values of the mask.  Exact against F.interpolate(mode='nearest').
    Host assertion before the launch: the reference mask has both values, and non-finite cells lie under a cleared and under a set mask."""
    rng = np.random.default_rng(Rr + S)
    grid = (rng.random((S, S, S)) * 9).astype(np.float32)
    dense = (rng.random((Rr, Rr, Rr)) * 9 + 1).astype(np.float32)
    flat = dense.reshape(-1)
    bad = rng.choice(flat.size, 300, replace=False)
    flat[bad[:100]] = np.nan; flat[bad[100:200]] = np.inf; flat[bad[200:]] = -np.inf
    mask = torch.nn.functional.interpolate(torch.from_numpy(grid)[None, None], size=[Rr] * 3, mode="nearest")[0, 0] > 4.5
    under = mask.reshape(-1).numpy()[bad]
    assert 0.3 < float(mask.float().mean()) < 0.7 and under.any() and not under.all()
    want = torch.from_numpy(dense) * mask
    got = S0.mask_by_density_grid(dense, grid, 4.5).cpu()
    assert torch.equal(torch.nan_to_num(got, 0), torch.nan_to_num(want, 0)) and torch.equal(torch.isnan(got), torch.isnan(want))
    assert np.array_equal(got.numpy()[~np.isnan(got.numpy())].view(np.uint32), want.numpy()[~np.isnan(want.numpy())].view(np.uint32))
