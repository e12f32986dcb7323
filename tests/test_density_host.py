"""CPU: the host side of the stage-0 density network — the hash-grid level layout against its known answers and against tests/density_refs.py, the numpy
restatements of the encoder against an answer that comes from no code (trilinear interpolation reproduces an affine function), DensityField.from_checkpoint's
refusals, and the command line's conflicts around --mcubes_reso."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_refs as D      # noqa: E402


@pytest.mark.parametrize("bound,total,dense_sizes", [(1.0, 6119864, [4920, 13824, 32768, 85184, 216000]), (2.0, 6328848, None)])
def test_layout_known_answers(bound, total, dense_sizes):
    from mirres_restir_nerf_mesh_amd import stage0
    L = D.layout(bound)
    net, n = stage0.density_layout(bound)
    sizes = np.diff(L["offsets"]).tolist()
    assert L["total"] == total and n == total
    if dense_sizes:
        assert sizes == dense_sizes + [524288] * 11
    assert L["hashed"].tolist() == [False] * 5 + [True] * 11 and all(s == 524288 for s in sizes[5:]) and all(s % 8 == 0 for s in sizes)
    # the library's table is the restatement's, the scales bit for bit
    assert net.num_levels == 16 and [net.offsets[i] for i in range(17)] == L["offsets"].tolist()
    assert [net.resolution[i] for i in range(16)] == L["resolution"].tolist() and [bool(net.hashed[i]) for i in range(16)] == L["hashed"].tolist()
    assert np.array_equal(np.array([net.scale[i] for i in range(16)], np.float32).view(np.uint32), L["scale"].view(np.uint32))
    assert L["scale"][0] == 15.0 and L["resolution"][0] == 16 and L["resolution"][15] == int(2048 * bound)


def test_layout_with_a_small_hash_table_and_bad_arguments():
    from mirres_restir_nerf_mesh_amd import stage0, _lib
    L = D.layout(1.0, log2_T=14)
    net, n = stage0.density_layout(1.0, log2_hashmap_size=14)
    assert n == L["total"] and L["hashed"].tolist() == [False, False] + [True] * 14
    assert np.diff(L["offsets"]).tolist()[:3] == [4920, 13824, 16384] and 4920 & (4920 - 1) and 13824 & (13824 - 1)      # dense sizes that are no powers of two
    assert [bool(net.hashed[i]) for i in range(16)] == L["hashed"].tolist()
    for kw in (dict(num_levels=17), dict(num_levels=0), dict(base_resolution=0), dict(log2_hashmap_size=40), dict(desired_resolution=1.0)):
        with pytest.raises(_lib.MirresError, match="mirres_density_layout"):
            stage0.density_layout(1.0, **kw)


def _levels(t, n=16):
    return ([t.offsets[i] for i in range(n + 1)], [t.resolution[i] for i in range(n)], [bool(t.hashed[i]) for i in range(n)],
            np.array([t.scale[i] for i in range(n)], np.float32).view(np.uint32).tolist())


def _want(desired):
    L = D.layout(desired=desired)
    assert all(b > a for a, b in zip(L["offsets"].tolist(), L["offsets"].tolist()[1:])) and L["offsets"][-1] == L["total"]
    return L["total"], (L["offsets"].tolist(), L["resolution"].tolist(), L["hashed"].tolist(), L["scale"].view(np.uint32).tolist())


@pytest.mark.parametrize("desired", [2 ** 21, 2 ** 22, 2 ** 24])
def test_layout_of_a_fine_grid_does_not_overflow(desired):
    """(resolution + 1)^3 passes 2^63 from a finest resolution of 2^21: taken in 64-bit integers before the clamp to 2^19 it wrapped to a negative level size at 2^21
    (at 2^22 and 2^24 the wrapped value happened to lie above the clamp).  The restatement's Python integers cannot overflow."""
    from mirres_restir_nerf_mesh_amd import stage0
    total, want = _want(desired)
    net, n = stage0.density_layout(1.0, desired_resolution=float(desired))
    assert n == total and net.num_levels == 16 and _levels(net) == want


@pytest.mark.parametrize("desired,wrapped", [(2 ** 21, []), (2 ** 22, [10]), (2 ** 24, [9])])
def test_gridenc_layout_of_a_fine_grid_has_the_density_layouts_numbers(desired, wrapped):
    """mirres_gridenc_layout with the same per_level_scale against the same restatement: total, offsets, resolutions and scale words of every level, and the hashed
    flag of every level but those whose stride product does not fit 32 bits.  There the two entries may differ, by design (csrc/grid_layout.hpp's `wrap`): the reference's
    uint32 product wraps (resolution + 1 = 65537: 65537^2 = 2^32 + 131073) and the level is indexed densely with wrapped strides, which mirres_gridenc_layout and its
    kernels restate and tests/gridenc_refs.py, the restatement of that loop, holds; density_refs.layout multiplies in Python integers and calls the level hashed.  Which
    levels those are is worked out here in Python integers, not read from either layout."""
    from mirres_restir_nerf_mesh_amd import encoding
    import gridenc_refs as GR
    total, want = _want(desired)
    pls = np.exp2(np.log2(desired / 16) / 15)
    g, m = encoding.gridenc_layout(per_level_scale=pls)
    got = _levels(g)
    assert m == total and g.num_levels == 16 and got[0] == want[0] and got[1] == want[1] and got[3] == want[3]
    sizes = np.diff(want[0]).tolist()
    over = [l for l in range(16) if any((want[1][l] + 1) ** k <= sizes[l] and (want[1][l] + 1) ** (k + 1) >= 2 ** 32 for k in (1, 2))]
    assert [got[2][l] for l in range(16) if l not in over] == [want[2][l] for l in range(16) if l not in over]
    differ = [l for l in range(16) if got[2][l] != want[2][l]]                      # an overflowed product matters only where what is left of it is below the size
    assert differ == wrapped and set(differ) <= set(over) and all(want[2][l] and not got[2][l] for l in differ)
    assert got[2] == GR.layout(pls=pls)["hashed"].tolist()


def test_the_largest_layout_fits_the_32_bit_offsets():
    """Both entries refuse a table of more than 2^31 - 1 entries, whose offsets would not fit an int.  Their own argument limits (16 levels, log2_hashmap_size <= 26)
    cap a table at 16 * 2^26 = 2^30 entries, so no accepted argument list reaches the refusal; what can be held is that the largest one comes out exact."""
    from mirres_restir_nerf_mesh_amd import stage0, encoding
    sizes = [min(2 ** 26, (10000 + 1) ** 3)] * 16                                  # per_level_scale 1: every level at the base resolution
    assert sizes == [2 ** 26] * 16 and sum(sizes) == 2 ** 30 < 2 ** 31 - 1
    g, m = encoding.gridenc_layout(per_level_scale=1.0, base_resolution=10000, log2_hashmap_size=26)
    assert m == 2 ** 30 and [g.offsets[i] for i in range(17)] == [i * 2 ** 26 for i in range(17)] and all(g.hashed[i] for i in range(16))
    net, n = stage0.density_layout(1.0, base_resolution=10000, log2_hashmap_size=26, desired_resolution=10000.0)
    assert n == 2 ** 30 and [net.offsets[i] for i in range(17)] == [i * 2 ** 26 for i in range(17)] and all(net.hashed[i] for i in range(16))


def test_affine_vertex_values_are_reproduced_at_the_half_cell_offset():
    """Not drawn from any code: trilinear interpolation reproduces an affine function exactly, so with a * v + b stored at the integer vertex v of a dense level the
    encoding of a point is a * (u * scale + 0.5) + b.  A wrong half-cell offset shifts it, a wrong corner order or stride permutes the axes' coefficients."""
    L = D.layout(1.0)
    rng = np.random.default_rng(11)
    pos = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    u = (pos.astype(np.float64) + 1.0) / 2.0
    table = np.zeros((L["total"], 2), np.float64)
    coef = {}
    for l in (0, 1, 4):
        assert not L["hashed"][l]
        s1 = int(L["resolution"][l]) + 1
        v = np.stack(np.meshgrid(np.arange(s1), np.arange(s1), np.arange(s1), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        a = rng.normal(size=(2, 3)); b = rng.normal(size=2)
        idx = (v[:, 0] + v[:, 1] * s1 + v[:, 2] * s1 * s1).astype(np.int64)
        assert idx.max() < L["offsets"][l + 1] - L["offsets"][l]
        table[L["offsets"][l] + idx] = v @ a.T + b
        coef[l] = (a, b)
    got = D.encode64(table, L, pos, 1.0)
    for l, (a, b) in coef.items():
        want = (u * float(L["scale"][l]) + 0.5) @ a.T + b
        err = np.abs(got[:, 2 * l: 2 * l + 2] - want).max() / np.abs(want).max()
        assert err <= 1e-12, (l, err)


@pytest.mark.parametrize("log2_T", [19, 14])
def test_float32_restatement_matches_float64(log2_T):
    L = D.layout(1.0, log2_T=log2_T)
    rng = np.random.default_rng(log2_T)
    table = rng.normal(size=(L["total"], 2)).astype(np.float32)
    pos = rng.uniform(-1, 1, size=(2000, 3)).astype(np.float32)
    pos[:4] = [[-1, -1, -1], [1, 1, 1], [np.nan, 0, 0], [0, np.inf, 0]]
    f32 = D.encode32(table, L, pos, 1.0); f64 = D.encode64(table, L, pos, 1.0)
    assert f32.dtype == np.float32 and (f32[2:4] == 0).all() and (f64[2:4] == 0).all() and np.abs(f32[:2]).max() > 0
    # Derived, per level: u, u * scale and + 0.5 each round once in fp32 (relative 2^-24 of a value <= scale + 1), so the interpolation point moves by at most
    # dp = 3 * 2^-24 * (scale + 1) cells; along one axis the interpolant's slope is a difference of two convex combinations of entries, <= 2 M per cell with M the
    # largest entry, three axes -> 6 M dp (the interpolant is continuous, so a cell picked differently on a face costs no more).  The interpolation itself: weights
    # of three factors each from one subtraction (4 roundings), a product and a sum per corner, eight corners -> well under 32 * 2^-24 M.
    M = float(np.abs(table).max())
    for l in range(16):
        tol = (6 * 3 * 2.0 ** -24 * (float(L["scale"][l]) + 1.0) + 32 * 2.0 ** -24) * M
        err = np.abs(f32[:, 2 * l: 2 * l + 2] - f64[:, 2 * l: 2 * l + 2]).max()
        assert err <= tol, (l, err, tol)


def _fake_model(L, **over):
    import torch
    m = {"encoder.embeddings": torch.zeros(8, 2), "encoder.offsets": torch.tensor(L["offsets"].tolist(), dtype=torch.int32),
         "sigma_net.0.weight": torch.zeros(64, 32), "sigma_net.1.weight": torch.zeros(16, 64), "density_grid": torch.zeros(1, 8)}
    m.update(over)
    return m


def test_from_checkpoint_refuses_what_it_cannot_evaluate():
    import torch
    from mirres_restir_nerf_mesh_amd import stage0
    F = stage0.DensityField
    with pytest.raises(ValueError, match="--bound"):                       # a bound-2 checkpoint read with the default bound
        F.from_checkpoint({"model": _fake_model(D.layout(2.0))}, bound=1.0)
    with pytest.raises(ValueError, match="--bound"):
        F.from_checkpoint(_fake_model(D.layout(1.0)), bound=2.0)
    tc = {"encoder.encoder.params": torch.zeros(16), "sigma_net.0.weight": torch.zeros(64, 32), "sigma_net.1.weight": torch.zeros(16, 64)}
    with pytest.raises(NotImplementedError, match="not supported"):
        F.from_checkpoint({"model": tc})
    with pytest.raises(ValueError, match="32 -> 64 -> 16"):
        F.from_checkpoint(_fake_model(D.layout(1.0), **{"sigma_net.0.weight": torch.zeros(64, 16)}))
    with pytest.raises(ValueError, match="32 -> 64 -> 16"):
        F.from_checkpoint(_fake_model(D.layout(1.0), **{"sigma_net.1.weight": torch.zeros(1, 64)}))
    m = _fake_model(D.layout(1.0)); del m["encoder.offsets"]
    with pytest.raises(KeyError, match="encoder.offsets"):
        F.from_checkpoint(m)


def test_cli_conflicts_of_mcubes_reso(tmp_path):
    import export_stage0 as E
    from mirres_restir_nerf_mesh_amd import checkpoint as CK
    ws = str(tmp_path / "ws"); os.makedirs(ws)
    ply = str(tmp_path / "in.ply"); vol = str(tmp_path / "v.npy"); ck = str(tmp_path / "c.pth")
    CK.write_ply(ply, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    np.save(vol, np.zeros((4, 4, 4), np.float32)); open(ck, "wb").close()
    for argv in (["--workspace", ws, "--mesh", ply, "--mcubes_reso", "64"], ["--workspace", ws, "--volume", vol, "--mcubes_reso", "64"],
                 ["--workspace", ws, "--volume", vol, "--sdf", "--mcubes_reso", "64"], ["--workspace", ws, "--ckpt", ck, "--sdf", "--mcubes_reso", "64"],
                 ["--workspace", ws, "--synthetic", "--mcubes_reso", "48"], ["--workspace", ws, "--ckpt", ck, "--network"],
                 ["--workspace", ws, "--ckpt", ck, "--mcubes_reso", "1"], ["--workspace", ws, "--ckpt", ck, "--mcubes_reso", "64", "--bound", "0"]):
        with pytest.raises(SystemExit) as e:
            E.parse_args(argv)
        assert e.value.code == 2, argv
    a = E.parse_args(["--workspace", ws, "--ckpt", ck, "--mcubes_reso", "512", "--bound", "2"])
    assert a.mcubes_reso == 512 and a.bound == 2.0
    a = E.parse_args(["--workspace", ws, "--ckpt", ck])
    assert a.mcubes_reso is None and a.bound == 1.0                         # unset: the density grid, as before
    a = E.parse_args(["--synthetic", "--network", "--mcubes_reso", "48"])
    assert a.network and a.mcubes_reso == 48
