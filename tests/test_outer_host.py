"""CPU (no GPU calls): the numpy restatement the outer-cascade kernels are held to (tests/outer_refs.py) against torch's own F.interpolate(mode='trilinear'),
the box predicates on vertices that lie on the faces, the synthetic multi-cascade checkpoint, and the argument checks of export_outer_meshes /
export_stage0(outer=True) / scripts/export_stage0.py --outer_meshes that need no device."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import outer_refs as OR      # noqa: E402
import stage0_refs as R      # noqa: E402


def _torch_trilinear(vol, Rr):
    return torch.nn.functional.interpolate(torch.from_numpy(np.asarray(vol, np.float32))[None, None], [Rr] * 3, mode="trilinear")[0, 0].numpy()


@pytest.mark.parametrize("S,Rr", OR.SHAPES)
def test_restatement_thresholds_as_torch_does(S, Rr):
    """|a - b| <= 8 * 2^-24 * sum |w_i v_i| per voxel for two fp32 evaluations a, b of the same eight-term sum, so a > thresh and b > thresh can only differ where
    the fp64 value lies within that bound of thresh; thresh is strictly between two adjacent grid values, which keeps all but a few voxels out of that band.
    The restatement itself stays within the bound of the fp64 sum over the same fp32 weights (asserted).  torch's value is only printed against the bound: its
    weights may differ from the restatement's by an ulp of the source coordinate (how its compiler contracts scale * (d + 0.5) - 0.5), which the derivation
    leaves out; the printed ratio was 0 to 1.9 on the six shapes.  What is asserted of torch is what the export depends on: the same side of thresh."""
    vol = OR.lognormal_grid(S, 1000 * S + Rr)
    a = OR.trilinear_fp32(vol, Rr); b = _torch_trilinear(vol, Rr)
    v64, bound = OR.trilinear_fp64(vol, Rr)
    assert a.shape == b.shape == (Rr, Rr, Rr) and np.isfinite(a).all() and (bound > 0).all()
    worst = float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / bound).max())
    print("S %d R %d: max |restatement - torch| / bound = %.3f, max |restatement - fp64| / bound = %.3f" % (S, Rr, worst, float((np.abs(a - v64) / bound).max())))
    assert (np.abs(a.astype(np.float64) - v64) <= bound).all()
    for k in (None, S ** 3 // 4, 3 * S ** 3 // 4):
        thresh = OR.thresh_between(vol, k)
        band = np.abs(v64 - np.float64(np.float32(thresh))) <= bound
        share = float(band.mean())
        print("  thresh %.6g: %d of %d voxels within the bound of it" % (thresh, int(band.sum()), band.size))
        assert share <= 1e-3
        assert np.array_equal((a > np.float32(thresh))[~band], (b > np.float32(thresh))[~band])
        occ, val = OR.occupancy(vol, Rr, thresh)
        assert np.array_equal(occ, (a > np.float32(thresh)).astype(np.float32)) and 0 < occ.mean() < 1
    if Rr == S:
        assert np.array_equal(a, vol) and np.array_equal(b, vol)


def test_non_finite_cells_spread_as_in_torch():
    vol = OR.lognormal_grid(4, 5); vol[0, 0, 0] = np.nan
    a = OR.trilinear_fp32(vol, 9); b = _torch_trilinear(vol, 9)
    assert int(np.isnan(a).sum()) == 27 == int(np.isnan(b).sum()) and np.array_equal(np.isnan(a), np.isnan(b))      # the 3^3 outputs whose i0 is 0 on every axis
    vol = OR.hostile_grid()
    a = OR.trilinear_fp32(vol, 9); b = _torch_trilinear(vol, 9)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a).sum() > 27
    assert np.isinf(b).any() and np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
    fin = np.isfinite(a)
    assert np.array_equal(a[fin] > 2.0, b[fin] > 2.0) and np.array_equal(a[fin] > 0.0, b[fin] > 0.0)
    assert (a[fin] < 0).any()                                                                                        # the -1 cells pull their neighbourhood below zero
    occ, _ = OR.occupancy(vol, 9, 2.0)
    assert not occ[np.isnan(a)].any() and occ[np.isposinf(a)].all() and not occ[np.isneginf(a)].any()              # nan_to_num(., 0), then > thresh


def test_border_clamps_of_the_smallest_grid():
    """S = 2: every output voxel clamps on some axis (src < 0 -> 0 at the low end, i1 = S - 1 at the high end)."""
    i0, i1, l0, l1 = OR.axis_weights(2, 5)
    assert i0.tolist() == [0, 0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1, 1] and l1[0] == 0 and l1[-1] > 0 and (l0 + l1 == 1).all()
    vol = OR.lognormal_grid(2, 3)
    a = OR.trilinear_fp32(vol, 5); v64, bound = OR.trilinear_fp64(vol, 5)
    assert (np.abs(a - v64) <= bound).all() and (np.abs(_torch_trilinear(vol, 5) - v64) <= 2 * bound).all()
    assert a[0, 0, 0] == vol[0, 0, 0]                                                      # src clamped to 0: weights 1 and 0
    assert np.allclose(a[::4, ::4, ::4], vol, rtol=2 ** -21, atol=0)                       # the high end: l0 v + l1 v of the same corner (i0 = i1 = S - 1)


def test_box_predicates_on_the_faces():
    box = (-0.45, -0.25, -0.5, 0.45, 0.25, 0.5)
    f = np.float32
    v = np.array([[0.45, 0.25, 0.5], [-0.45, 0, 0], [0, 0, 0], [np.nextafter(f(0.45), f(1)), 0, 0], [np.nextafter(f(0.45), f(0)), 0, 0], [0, 0.25, 0.6], [2, 2, 2],
                  [np.nan, 0, 0]], np.float32)
    # float32(0.45) is smaller than the double 0.45: the fp32 vertex "on" that face of a decimal box is strictly inside it, the next float up is outside
    assert np.float64(f(0.45)) < 0.45 < np.float64(np.nextafter(f(0.45), f(1)))
    assert OR.select_box(v, box, False).tolist() == [True, True, True, False, True, False, False, False]
    assert OR.select_box(v, box, True).tolist() == [True, False, False, True, False, True, True, False]         # vertex 0 lies on the y and z faces; NaN is selected by neither
    box2 = (-0.5, -0.25, -0.5, 0.5, 0.25, 0.5)                                          # bounds fp32 holds exactly: on a face means selected both ways
    w = np.array([[0.5, 0, 0], [0, -0.25, 0], [0.5, 0.25, -0.5], [0.25, 0.125, 0.25], [0.75, 0, 0]], np.float32)
    assert OR.select_box(w, box2, False).tolist() == [True, True, True, True, False]
    assert OR.select_box(w, box2, True).tolist() == [True, True, True, False, True]
    t = np.array([[0, 3, 4], [3, 3, 3], [4, 4, 4]], np.int32)
    ov, ot = OR.remove_selected(w, t, box2, True)                                        # a face with one selected vertex goes; so does the vertex only it used
    assert ot.tolist() == [[0, 0, 0]] and np.array_equal(ov, w[3:4])


def test_synthetic_checkpoint_default_is_unchanged_and_cascades_add_rows():
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    want = {"density_grid": "cdb81185337f730e51af570ffb5cc1ec46fe85c6285dc9178949f4fc4fa65529",
            "encoder.embeddings": "404ceec0fe3adb21e00b1469e541eaf75350104c4f097445dbf2c880d7f2dd50",
            "encoder.offsets": "36f0a04e7262aea81cdb1d500db7f310c8563a5f011b54a42532c0bfacb76302",
            "sigma_net.0.weight": "6e12e9e642732ec852b3c46e3af99f7d1991408f67f1bf8abbc297038d622679",
            "sigma_net.1.weight": "f7e4b7df98e2b9533216f4a9c1261224bda07083b93fe9357ea76c0f83477cee"}
    for ck in (S0.synthetic_checkpoint(), S0.synthetic_checkpoint(cascades=1)):
        assert sorted(ck) == ["mean_density", "model"] and ck["mean_density"] == 8.166169912567646 and sorted(ck["model"]) == sorted(want)
        assert tuple(ck["model"]["density_grid"].shape) == (1, 4096) and ck["model"]["encoder.offsets"].dtype == torch.int32
        for k, h in want.items():
            assert hashlib.sha256(ck["model"][k].contiguous().numpy().tobytes()).hexdigest() == h, k
    ck = S0.synthetic_checkpoint(S=8, radius=0.5)
    assert ck["mean_density"] == 9.487735836358526
    assert hashlib.sha256(ck["model"]["density_grid"].numpy().tobytes()).hexdigest() == "b362746150a73e3644f3c515c53d67a119fc2e5816c5a3e0063a69758a479658"
    one = S0.synthetic_checkpoint()["model"]["density_grid"]
    for n in (2, 3):
        ck = S0.synthetic_checkpoint(cascades=n)
        g = ck["model"]["density_grid"]
        assert tuple(g.shape) == (n, 4096) and g.dtype == torch.float32 and torch.equal(g[:1], one) and ck["mean_density"] == 8.166169912567646
        b = float(2 ** (n - 1))
        assert ck["model"]["aabb_train"].dtype == torch.float32 and ck["model"]["aabb_train"].tolist() == [-b, -b, -b, b, b, b]
        cc = (np.arange(16) + 0.5) / 16 * 2 - 1
        x, y, z = np.meshgrid(cc, cc, cc, indexing="ij")
        cheb = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
        for k in range(1, n):
            vol = R.unpack_morton(g[k].numpy(), 16)
            occ = vol > ck["mean_density"]
            assert (vol == -1).sum() == 16 and np.isfinite(vol).all()
            assert occ[cheb < 0.1].all()                                                # the ball, well inside the 0.45 box
            outer = occ & (cheb > 0.5)
            assert outer.sum() > 300 and cheb[outer].min() > 0.55 and cheb[outer].max() < 0.9      # this cascade's slab and dome
            assert outer[z < -0.55].sum() > 100 and outer[z > 0.25].sum() > 100
            assert not (occ & (cheb > 0.45) & (cheb < 0.55)).any()                      # nothing straddles the box the cascade's centre is cut with
    with pytest.raises(ValueError, match="cascades"):
        S0.synthetic_checkpoint(cascades=4)


def test_outer_arguments_are_checked_without_a_device(tmp_path):
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    ck1, ck2, ck3 = (S0.synthetic_checkpoint(cascades=n) for n in (1, 2, 3))
    out = str(tmp_path)
    never = lambda m: (_ for _ in ()).throw(AssertionError("logged before the arguments were checked: " + m))
    for ck, bound in ((ck2, 1.0), (ck2, 4.0), (ck1, 2.0), (ck3, 2.0), (ck3, 8.0)):
        with pytest.raises(ValueError, match="cascades"):
            S0.export_outer_meshes(out, ck, bound, log=never)
        with pytest.raises(ValueError, match="cascades"):
            S0.export_stage0(out, ckpt=ck, bound=bound, outer=True, log=never)
    with pytest.raises(NotImplementedError, match="sdf"):
        S0.export_outer_meshes(out, ck2, 2.0, sdf=True, log=never)
    with pytest.raises(NotImplementedError, match="sdf"):
        S0.export_stage0(out, ckpt=ck2, volume=np.zeros((4, 4, 4), np.float32), sdf=True, bound=2.0, outer=True, log=never)
    with pytest.raises(ValueError, match="outer needs a checkpoint"):
        S0.export_stage0(out, volume=np.zeros((4, 4, 4), np.float32), outer=True, log=never)
    with pytest.raises(ValueError, match="outer needs a checkpoint"):
        S0.export_stage0(out, mesh=R.cube(), outer=True, log=never)
    with pytest.raises(ValueError, match="no ckpt"):
        S0.export_outer_meshes(out, None, 2.0, log=never)
    with pytest.raises(ValueError, match="env_reso"):
        S0.export_outer_meshes(out, ck2, 2.0, env_reso=1, log=never)
    with pytest.raises(ValueError, match="env_reso"):
        S0.export_stage0(out, ckpt=ck2, bound=2.0, outer=True, env_reso=2048, log=never)
    with pytest.raises(KeyError, match="mean_density"):
        S0.export_outer_meshes(out, {"model": ck2["model"]}, 2.0, log=never)
    open(os.path.join(out, "mesh_2.ply"), "wb").close()
    with pytest.raises(FileExistsError, match="mesh_2.ply"):
        S0.export_outer_meshes(out, ck3, 4.0, log=never)
    with pytest.raises(FileExistsError, match="mesh_2.ply"):                               # before mesh_0.ply is written
        S0.export_stage0(out, ckpt=ck3, bound=4.0, outer=True, log=never)
    assert os.listdir(out) == ["mesh_2.ply"]
    with pytest.raises(ValueError, match="inside"):
        S0.remove_selected_verts(np.zeros((0, 3)), np.zeros((0, 3)), (0, 0, 0, 1, 1, 1), where="within")
    with pytest.raises(ValueError, match="box"):
        S0.remove_selected_verts(np.zeros((0, 3)), np.zeros((0, 3)), (0, 0, 0, 1, 1))
    with pytest.raises(ValueError, match="not an outer"):
        S0.outer_shell(np.zeros((4, 4, 4)), 0, 2.0, 8, 1.0, (-2, -2, -2, 2, 2, 2))


def test_command_line_checks_outer_meshes_without_a_device(tmp_path, capsys):
    import export_stage0 as E
    ws = str(tmp_path / "ws")
    a = E.parse_args(["--synthetic", "--bound", "2", "--outer_meshes", "--workspace", ws])
    assert a.outer_meshes and a.env_reso == 256 and a.bound == 2.0
    assert not E.parse_args(["--synthetic", "--workspace", ws]).outer_meshes
    for bad in (["--sdf", "--volume", __file__], ["--network"], ["--env_reso", "1"], ["--env_reso", "2000"], ["--bound", "8"], ["--mesh", __file__]):
        with pytest.raises(SystemExit):
            E.parse_args(["--synthetic", "--bound", "2", "--outer_meshes", "--workspace", ws] + bad)
        assert "error" in capsys.readouterr().err
    os.makedirs(os.path.join(ws, "mesh_stage0"))
    open(os.path.join(ws, "mesh_stage0", "mesh_1.ply"), "wb").close()
    with pytest.raises(SystemExit):
        E.parse_args(["--synthetic", "--bound", "2", "--outer_meshes", "--workspace", ws])
    assert "mesh_1.ply" in capsys.readouterr().err
    E.parse_args(["--synthetic", "--workspace", ws])                                        # without --outer_meshes the file is nobody's business
    assert E.parse_args(["--synthetic", "--bound", "2", "--outer_meshes", "--workspace", ws, "--overwrite"]).overwrite
