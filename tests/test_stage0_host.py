"""CPU: the host side of the stage-0 extraction — Morton order, iso selection, the command line's refusals, the PLY hand-over to load_stage0_mesh, and the numpy
restatements of tests/stage0_refs.py against scipy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage0_refs as R      # noqa: E402


@pytest.mark.parametrize("S", [4, 8])
def test_morton_indices_match_the_bit_trick(S):
    from mirres_restir_nerf_mesh_amd import stage0
    m = stage0.morton_indices(S)
    assert sorted(m.reshape(-1).tolist()) == list(range(S ** 3))
    i = np.arange(S ** 3, dtype=np.uint32)
    x, y, z = R.morton_invert(i), R.morton_invert(i >> np.uint32(1)), R.morton_invert(i >> np.uint32(2))
    assert np.array_equal(m[x, y, z], i.astype(np.int64))
    grid = np.random.default_rng(S).random(S ** 3).astype(np.float32)
    assert np.array_equal(grid[m], R.unpack_morton(grid, S))
    with pytest.raises(ValueError):
        stage0.morton_indices(6)


def test_iso_is_the_smaller_of_mean_density_and_threshold():
    from mirres_restir_nerf_mesh_amd import stage0
    assert stage0.select_iso(3.5, 10.0) == 3.5 and stage0.select_iso(42.0, 10.0) == 10.0 and stage0.select_iso(np.float32(0.25), 10) == 0.25


def test_cli_rejects_conflicts_and_refuses_to_overwrite(tmp_path, capsys):
    import export_stage0 as E
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    ws = str(tmp_path / "ws"); os.makedirs(os.path.join(ws, "mesh_stage0"))
    ply = str(tmp_path / "in.ply"); vol = str(tmp_path / "v.npy")
    v, t = R.cube()
    CK.write_ply(ply, v, t); np.save(vol, np.zeros((4, 4, 4), np.float32))
    for argv in (["--workspace", ws, "--mesh", ply, "--volume", vol], ["--workspace", ws, "--sdf"], ["--workspace", ws, "--synthetic", "--mesh", ply],
                 ["--workspace", ws, "--volume", vol, "--sdf", "--iso", "1"], ["--workspace", ws], ["--mesh", ply], ["--workspace", ws, "--mesh", str(tmp_path / "none.ply")]):
        with pytest.raises(SystemExit) as e:
            E.parse_args(argv)
        assert e.value.code == 2, argv
    a = E.parse_args(["--workspace", ws, "--mesh", ply])
    assert a.out == os.path.join(ws, "mesh_stage0") and a.visibility_mask_dilation == 5 and a.clean_min_f == 8 and a.clean_min_d == 5 and a.decimate_target == 3e5 and a.density_thresh == 10
    CK.write_ply(os.path.join(ws, "mesh_stage0", "mesh_0.ply"), v, t)
    with pytest.raises(SystemExit):
        E.parse_args(["--workspace", ws, "--mesh", ply])
    assert "--overwrite" in capsys.readouterr().err
    assert E.parse_args(["--workspace", ws, "--mesh", ply, "--overwrite"]).overwrite


def test_extracted_mesh_round_trips_through_load_stage0_mesh(tmp_path):
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    ax = np.linspace(-1, 1, 12, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    v, t = R.marching_cubes(0.7 - np.sqrt(x * x + y * y + z * z), 0.0)
    assert len(t) > 100 and R.mesh_edges_ok(t) and R.signed_volume(v, t) > 0 and R.euler_characteristic(len(v), t) == 2
    os.makedirs(tmp_path / "mesh_stage0")
    CK.write_ply(str(tmp_path / "mesh_stage0" / "mesh_0.ply"), v, t)
    v2, t2, vc, fc = CK.load_stage0_mesh(str(tmp_path), 1)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, t) and vc[-1] == len(v) and fc[-1] == len(t)


def _scipy_labels(tris):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    T = len(tris)
    tris = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], 0), axis=1)
    f = np.tile(np.arange(T), 3)
    order = np.lexsort((f, e[:, 1], e[:, 0])); e, f = e[order], f[order]
    same = (e[1:] == e[:-1]).all(axis=1)
    a, b = f[:-1][same], f[1:][same]
    n, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(T, T)), directed=False)
    smallest = np.full(n, T); np.minimum.at(smallest, lab, np.arange(T))
    return smallest[lab].astype(np.int32)


def test_component_and_dilation_restatements_against_scipy():
    va, ta = R.icosphere(1); vb, tb = R.cube(0.1, (3, 0, 0))
    # two fans that touch at one vertex only: vertex 0 shared, no shared edge
    vf = np.array([[0, 0, 5], [1, 0, 5], [1, 1, 5], [0, 1, 5], [-1, 0, 5], [-1, -1, 5], [0, -1, 5]], np.float32)
    tf = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5], [0, 5, 6]], np.int32)
    v, t = R.join([(va, ta), (vb, tb), (vf, tf)])
    t = t[np.random.default_rng(3).permutation(len(t))]
    lab = R.components(t)
    assert np.array_equal(lab, _scipy_labels(t))
    assert len(np.unique(lab)) == 4                                       # the two fans stay apart
    vs, ts = R.strip(50)
    assert np.array_equal(R.components(ts), np.zeros(50, np.int32)) and np.array_equal(_scipy_labels(ts), np.zeros(50, np.int32))
    # dilation: k rings from one face of the strip reach exactly the faces within vertex distance k
    sel = np.zeros(50, bool); sel[20] = True
    for k in (0, 1, 2, 5):
        got = R.dilate(ts, len(vs), sel, k)
        want = np.zeros(50, bool); want[max(0, 20 - 2 * k): 20 + 2 * k + 1] = True
        assert np.array_equal(got, want), k
    # and as a graph statement: one ring = the faces that share a vertex with a selected face (scipy: neighbours in the vertex-adjacency graph)
    from scipy.sparse import coo_matrix
    T = len(t)
    inc = coo_matrix((np.ones(3 * T), (np.repeat(np.arange(T), 3), t.reshape(-1))), shape=(T, len(v))).tocsr()
    adj = (inc @ inc.T) > 0
    s0 = np.zeros(T, bool); s0[[0, 7]] = True
    assert np.array_equal(R.dilate(t, len(v), s0, 1), np.asarray(adj[s0].sum(axis=0)).reshape(-1) > 0)
    assert np.array_equal(R.dilate(t, len(v), s0, 2), np.asarray((adj @ adj)[s0].sum(axis=0)).reshape(-1) > 0)
