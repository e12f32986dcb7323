"""CPU, no GPU calls: what the hash grid's total-variation regulariser and the stage-0 training options rest on apart from the kernel.  The fp32 restatement of
the term (tests/tv_refs.py) against its float64 twin and against cases worked by hand; mirres_grid_tv_grad's refusals before a device is touched and
mirres_grid_tv_workspace_bytes; the adaptive ray count; the new options of scripts/train_stage0.py; harness.get_rays_at against get_rays; the uint8 view store
against load_blender's float images."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tv_refs as TV                           # noqa: E402

F32 = np.float32


def test_the_layouts_the_gpu_tests_rely_on():
    L14, L19 = TV.layout(1.0, log2_T=14), TV.layout(1.0, log2_T=19)
    assert TV.dense_levels(L14) == [0, 1] and TV.hashed_levels(L14) == list(range(2, 16))
    assert TV.dense_levels(L19) == [0, 1, 2, 3, 4]
    assert int(L14["resolution"][0]) == 16 and float(L14["scale"][0]) == 15.0 and int(L14["resolution"][1]) + 1 == 24


def test_fp32_restatement_against_float64():
    """|v32 - v64| <= gamma(14) * w * sum |diff| / sqrt(idelta + 1e-9): six differences and their sum, the squares' sum, sqrt, the reciprocal, w and two products."""
    rng = np.random.default_rng(5)
    L = TV.layout(1.0, log2_T=14)
    for gain in (1e-4, 1.0, 300.0):
        table = (rng.normal(size=(L["total"], 2)) * gain).astype(F32)
        pos = rng.uniform(-1, 1, size=(500, 3)).astype(F32)
        pos[:8] = np.array([[-1, -1, -1], [1, 1, 1], [-1, 1, 0], [0, 0, 0], [1, -1, 1], [-1, 0, 1], [0.5, -1, -1], [1, 1, -1]], F32)
        _, cs = TV.cells(L, pos, 1.0)
        worst = 0.0
        for l in range(L["num_levels"]):
            e32, v32, _ = TV.cell_values(table, L, l, cs[l], 1e-3)
            e64, v64, s64 = TV.cell_values(table, L, l, cs[l], 1e-3, f64=True)
            assert np.array_equal(e32, e64) and v32.dtype == F32 and v64.dtype == np.float64
            err = np.abs(v32.astype(np.float64) - v64); allow = TV.gamma(14) * s64
            assert (err <= allow).all(), (gain, l, float((err / allow).max()))
            worst = max(worst, float((err / np.maximum(allow, 1e-300)).max()))
        print("gain %g: worst error / allowance %.3f" % (gain, worst))


def _one_cell(table_entries, c, weight=6.0, level=0):
    """The term of cell c of a level-0 table that is zero but for table_entries {(x, y, z): (ch0, ch1)} -> value f32 [2]."""
    L = TV.layout(1.0, log2_T=14)
    table = np.zeros((L["total"], 2), F32)
    s1 = int(L["resolution"][level]) + 1
    for (x, y, z), v in table_entries.items():
        table[int(L["offsets"][level]) + x + y * s1 + z * s1 * s1] = v
    e, v, _ = TV.cell_values(table, L, level, np.array([c], np.uint32), weight)
    assert int(e[0]) == c[0] + c[1] * s1 + c[2] * s1 * s1
    return v[0]


def test_hand_computed_cells():
    # weight 6: w = 1 exactly.  The corner cell (0, 0, 0) has three neighbours, all to the right: diffs of channel 0 are 0.5 - 0.25, 0.5 - 0, 0.5 - (-0.5) =
    # 0.25, 0.5, 1 -> res 1.75, idelta 0.0625 + 0.25 + 1 = 1.3125; channel 1: -1 - 1, -1 - 0, -1 - 0 = -2, -1, -1 -> res -4, idelta 6
    v = _one_cell({(0, 0, 0): (0.5, -1.0), (1, 0, 0): (0.25, 1.0), (0, 1, 0): (0.0, 0.0), (0, 0, 1): (-0.5, 0.0)}, (0, 0, 0))
    assert v[0] == pytest.approx(1.75 / np.sqrt(1.3125 + 1e-9), rel=4e-7) and v[1] == pytest.approx(-4.0 / np.sqrt(6.0 + 1e-9), rel=4e-7)
    # six neighbours would have added three more differences against entries that do not exist: 0.5 each on channel 0 -> res 3.25
    assert abs(float(v[0]) - 3.25 / np.sqrt(1.3125 + 0.75)) > 0.1
    # the top cell, where u = 1 puts a point: c = floor(1 * 15 + 0.5) = 15 < resolution 16, so both neighbours of every axis count (16 is a vertex of the level).
    # only the cell is non-zero: six diffs of 1 (channel 0) and of 2 (channel 1) -> res 6, idelta 6; res 12, idelta 24
    L = TV.layout(1.0, log2_T=14)
    _, cs = TV.cells(L, np.array([[1.0, 1.0, 1.0]], F32), 1.0)
    assert cs[0].tolist() == [[15, 15, 15]]
    v = _one_cell({(15, 15, 15): (1.0, 2.0)}, (15, 15, 15))
    assert v[0] == pytest.approx(6.0 / np.sqrt(6.0 + 1e-9), rel=4e-7) and v[1] == pytest.approx(12.0 / np.sqrt(24.0 + 1e-9), rel=4e-7)
    # a vertex at the resolution itself (no point lands there, the rule is the reference's): no right neighbour
    v = _one_cell({(16, 3, 3): (1.0, 0.0)}, (16, 3, 3))
    assert v[0] == pytest.approx(5.0 / np.sqrt(5.0 + 1e-9), rel=4e-7) and v[1] == 0.0
    # a constant table: every diff is 0, the value is exactly 0 (not a NaN from 0 / sqrt(1e-9))
    table = np.full((L["total"], 2), 0.37, F32)
    for l, (e, val) in enumerate(TV.point_terms(table, L, np.array([[0.1, -0.7, 0.3], [-1, -1, -1]], F32), 1.0, 1e-3)):
        assert np.array_equal(val.view(np.uint32), np.zeros_like(val).view(np.uint32)), l


def test_out_of_bounds_and_non_finite_points_contribute_nothing():
    L = TV.layout(1.0, log2_T=14)
    one = np.nextafter(F32(1), F32(2))
    pos = np.array([[0, 0, 0], [one, 0, 0], [0, -one, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 1, 1], [-1, -1, -1]], F32)
    keep, cs = TV.cells(L, pos, 1.0)
    # one ulp above +bound: (1 + 2^-23) + 1 rounds to 2 in fp32, u = 1, inside; one ulp below -bound: -2^-23 exactly, u < 0, outside — the encoder's own rule
    assert keep.tolist() == [True, True, False, False, False, False, True, True] and all(len(c) == 4 for c in cs)
    assert cs[0][1].tolist() == [15, 8, 8]


def test_expected_dense_and_hashed_bookkeeping():
    rng = np.random.default_rng(2)
    L = TV.layout(1.0, log2_T=14)
    table = rng.normal(size=(L["total"], 2)).astype(F32); grad0 = rng.normal(size=(L["total"], 2)).astype(F32)
    pos = np.repeat(rng.uniform(-1, 1, size=(20, 3)).astype(F32), 3, axis=0)      # every cell three times
    want, touched = TV.expected_dense(grad0, table, L, pos, 1.0, 1e-2)
    dm = TV.level_mask(L, [0, 1])
    assert touched.sum() > 0 and not touched[~dm].any() and np.array_equal(want[~touched], grad0[~touched])
    pt = TV.point_terms(table, L, pos, 1.0, 1e-2)
    e, v = pt[0][0][0], pt[0][1][0]
    assert np.array_equal(want[e], grad0[e] + F32(3) * v)
    H = TV.expected_hashed(grad0, table, L, pos, 1.0, 1e-2)
    assert (H["terms"] % 3 == 0).all() and H["terms"].sum() == 60 * 14 and (H["allow"] > 0).all()
    # the sum of the refs is what check accepts, and a single wrong entry is not
    got = want.copy()
    got[H["entry"]] = H["sum64"].astype(F32)
    assert TV.check(got, grad0, table, L, pos, 1.0, 1e-2) == (0, len(H["entry"]))
    bad = got.copy(); bad[e, 0] = np.nextafter(bad[e, 0], F32(9))
    with pytest.raises(AssertionError, match="dense"):
        TV.check(bad, grad0, table, L, pos, 1.0, 1e-2)
    bad = got.copy(); k = H["entry"][0]; bad[k] += 4 * H["allow"][0].astype(F32) + F32(1e-30)
    with pytest.raises(AssertionError, match="hashed"):
        TV.check(bad, grad0, table, L, pos, 1.0, 1e-2)


def test_adaptive_num_rays():
    import train_stage0 as T
    f = T.adapt_num_rays
    assert f(4096, 262144, 262144, 1 << 18) == 4096
    assert f(4096, 131072, 262144, 1 << 18) == 8192
    # halves go to the even neighbour, as Python's round does: 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 -> the lower clamp
    assert f(1, 2, 3, 100) == 2 and f(1, 2, 5, 100) == 2 and f(1, 2, 7, 100) == 4 and f(1, 2, 1, 100) == 1
    assert f(5, 2, 1, 100) == 2 and f(7, 2, 1, 100) == 4                               # 2.5 -> 2, 3.5 -> 4 through the ray count
    assert f(4096, 0, 262144, 1 << 18) == 4096 and f(17, 0, 1, 5) == 17                # no samples: the count stays (the reference divides by zero)
    assert f(4096, 1, 262144, 1 << 18) == 1 << 18 and f(1000, 10, 1000, 5000) == 5000  # the upper clamp
    assert f(10, 1 << 30, 1, 100) == 1                                                 # the lower clamp
    assert isinstance(f(3, 7, 11, 100), int)


def test_entry_refuses_bad_arguments_before_touching_a_device():
    """Every call fails an argument check (MIRRES_E_ARG exactly, not a device error) or has nothing to do: the pointers are host memory."""
    from mirres_restir_nerf_mesh_amd import _lib as L, stage0 as S0
    lib = L.lib()
    E_ARG = -1
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    net, total = S0.density_layout(1.0, log2_hashmap_size=14)
    need = int(lib.mirres_grid_tv_workspace_bytes(C.byref(net)))
    L14 = TV.layout(1.0, log2_T=14)
    dense_entries = lambda Lr: int(sum(Lr["offsets"][l + 1] - Lr["offsets"][l] for l in TV.dense_levels(Lr)))
    assert total == L14["total"] and need == 4 * dense_entries(L14) == 4 * (4920 + 13824)
    net19, _ = S0.density_layout(1.0)
    assert int(lib.mirres_grid_tv_workspace_bytes(C.byref(net19))) == 4 * dense_entries(TV.layout(1.0, log2_T=19))
    assert lib.mirres_grid_tv_workspace_bytes(None) == E_ARG and b"mirres_grid_tv_workspace_bytes" in lib.mirres_last_error()

    def call(net_=net, pos=p, n=4, bound=1.0, weight=1e-3, grad=p, ws=p, ws_bytes=need):
        return lib.mirres_grid_tv_grad(C.byref(net_) if net_ is not None else None, pos, n, bound, weight, grad, ws, ws_bytes, None)

    def refused(what, **kw):
        assert call(**kw) == E_ARG, kw
        err = lib.mirres_last_error()
        assert b"mirres_grid_tv_grad" in err and what in err, (kw, err)
    refused(b"NULL", net_=None)
    refused(b"NULL table")                                                             # density_layout leaves the pointers NULL
    net.table = p                                                                      # w0 and w1 stay NULL: they are not read
    bad = L.DensityNet(); C.memmove(C.byref(bad), C.byref(net), C.sizeof(bad)); bad.num_levels = 17
    refused(b"num_levels", net_=bad)
    bad = L.DensityNet(); C.memmove(C.byref(bad), C.byref(net), C.sizeof(bad)); bad.hashed[5] = 0
    refused(b"marked dense", net_=bad)
    refused(b"n ", n=-1); refused(b"n ", n=(1 << 31) + 1)
    refused(b"pos", pos=None)
    refused(b"grad_table", grad=None)
    for w in (-1e-3, float("nan"), float("inf"), float("-inf")):
        refused(b"weight", weight=w)
    for b in (0.0, -1.0, float("nan"), float("inf")):
        refused(b"bound", bound=b)
    refused(b"workspace", ws=None); refused(b"workspace", ws_bytes=need - 1); refused(b"workspace", ws_bytes=0)
    assert call(n=0, pos=None) == 0 and call(weight=0.0) == 0 and call(n=0, weight=0.0) == 0      # nothing to do, no launch
    refused(b"grad_table", n=0, grad=None); refused(b"workspace", weight=0.0, ws=None)          # the refusals come first
    assert call(n=1 << 31, ws_bytes=need - 4) == E_ARG
    assert not any(host)


def test_python_method_refuses_without_a_gradient():
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    assert S0.RadianceField.grad_total_variation is S0.DensityField.grad_total_variation
    import inspect
    sig = inspect.signature(S0.DensityField.grad_total_variation)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("weight", 1e-7), ("inputs", None), ("grad", None), ("B", 1000000), ("generator", None)]
    fake = types.SimpleNamespace(table=torch.zeros(8, 2), bound=1.0)
    with pytest.raises(ValueError, match="grad is None, should be called after loss.backward"):
        S0.DensityField.grad_total_variation(fake)
    with pytest.raises(TypeError):
        S0.DensityField.grad_total_variation(fake, grad=torch.zeros(8, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        S0.DensityField.grad_total_variation(fake, grad=np.zeros((8, 2), F32))
    with pytest.raises(ValueError, match="the table has"):
        S0.DensityField.grad_total_variation(fake, grad=torch.zeros(2, 8))
    with pytest.raises(ValueError, match="not contiguous"):
        S0.DensityField.grad_total_variation(fake, grad=torch.zeros(2, 8).t())


def test_train_script_new_options(tmp_path, capsys):
    import train_stage0 as T
    a = T.parse_args(["--synthetic"])
    assert a.lambda_tv == 0.0 and not a.adaptive_num_rays and not a.random_image_batch and not a.O and a.num_points == 1 << 18 and a.max_num_rays == 1 << 18
    assert (a.iters, a.num_rays, a.lr, a.update_extra_interval) == (7500, 4096, 1e-2, 16) and a.background == "white" and not a.mark_untrained
    a = T.parse_args(["--synthetic", "-O", "--lambda_tv", "1e-8", "--num_points", "65536"])
    assert a.mark_untrained and a.random_image_batch and a.adaptive_num_rays and a.lambda_tv == 1e-8 and a.num_points == 65536
    a = T.parse_args(["--synthetic", "--num_points", "1000"])                          # accepted and ignored without --adaptive_num_rays
    assert a.num_points == 1000 and not a.adaptive_num_rays
    a = T.parse_args(["--synthetic", "--adaptive_num_rays", "--max_num_rays", "9000"])
    assert a.adaptive_num_rays and a.max_num_rays == 9000 and not a.random_image_batch and not a.mark_untrained
    for bad in (["--lambda_tv", "-1e-8"], ["--lambda_tv", "nan"], ["--lambda_tv", "inf"], ["--num_points", "0"], ["--max_num_rays", "0"], ["--num_points", "-5"],
                ["--lambda_tv"], ["--max_num_rays", "x"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--synthetic"] + bad)
        assert "error" in capsys.readouterr().err, bad
    help_text = T.build_parser().format_help()
    for word in ("GradScaler", "lambda_tv", "adaptive_num_rays", "sdf", "random_image_batch", "num_points", "max_num_rays", "-O"):
        assert word in help_text, word
    doc = T.__doc__.split("NOT built")[1]
    assert "lambda_tv" not in doc and "adaptive_num_rays" not in doc and "GradScaler" in doc


def test_get_rays_at_against_get_rays():
    """Per component the two differ by the order of a three-term sum alone: |a - b| <= 2 gamma(3) * sum |terms|."""
    from mirres_restir_nerf_mesh_amd import harness
    from render_stage0 import orbit_poses
    H, W = 11, 7
    intr = (9.3, 8.7, 3.4, 5.6)
    poses = torch.from_numpy(np.stack([np.asarray(p, np.float32) for p in orbit_poses(5)]))
    gen = torch.Generator().manual_seed(4)
    index = torch.randint(5, (300,), generator=gen); pix = torch.randint(H * W, (300,), generator=gen)
    pix[:4] = torch.tensor([0, W - 1, H * W - W, H * W - 1])
    o, d = harness.get_rays_at(poses[index], intr, H, W, pix)
    assert o.shape == d.shape == (300, 3) and o.dtype == d.dtype == torch.float32 and o.is_contiguous() and d.is_contiguous()
    full = [harness.get_rays(p, intr, H, W) for p in poses]
    want_o = torch.stack([full[int(v)][0][int(k)] for v, k in zip(index, pix)]); want_d = torch.stack([full[int(v)][1][int(k)] for v, k in zip(index, pix)])
    assert torch.equal(o, want_o)
    i = (pix % W).double() + 0.5; j = (pix // W).double() + 0.5
    cam = torch.stack(((i - intr[2]) / intr[0], -(j - intr[3]) / intr[1], -torch.ones_like(i)), -1)
    mag = (cam[:, None, :].abs() * poses[index][:, :3, :3].double().abs()).sum(-1)
    err = (d.double() - want_d.double()).abs()
    assert (err <= 2 * TV.gamma(3) * mag).all(), float((err / mag).max())
    assert (d.double() - (cam[:, None, :] * poses[index][:, :3, :3].double()).sum(-1)).abs().max() < 1e-5
    with pytest.raises(ValueError, match="get_rays_at"):
        harness.get_rays_at(poses, intr, H, W, pix)


def test_uint8_view_store_gives_load_blender_its_bits(tmp_path):
    """--random_image_batch keeps the images' own bytes and converts what it gathers: an srgb pixel has the bits of load_blender's float image."""
    Image = pytest.importorskip("PIL.Image")
    import train_stage0 as T
    rng = np.random.default_rng(1)
    frames = []
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, size=(6, 5, 4), dtype=np.uint8), "RGBA").save(str(tmp_path / ("r_%d.png" % k)))
        m = np.eye(4); m[:3, 3] = rng.normal(size=3)
        frames.append({"file_path": "r_%d" % k, "transform_matrix": m.tolist()})
    (tmp_path / "transforms_train.json").write_text(json.dumps({"camera_angle_x": 0.7, "frames": frames}))
    a = types.SimpleNamespace(path=str(tmp_path), downscale=1, color_space="srgb", scale=0.8, offset=[0.0, 0.1, 0.0])
    H, W, focal, views = T.load_blender(a, "train")
    H8, W8, focal8, raw = T.load_blender(a, "train", u8=True)
    assert (H, W, focal) == (H8, W8, focal8) == (6, 5, focal) and len(raw) == 3
    pixels = torch.stack([v[1] for v in raw])
    assert pixels.dtype == torch.uint8 and tuple(pixels.shape) == (3, 30, 4)
    gen = torch.Generator().manual_seed(0)
    index = torch.randint(3, (64,), generator=gen); pix = torch.randint(30, (64,), generator=gen)
    gt, al = T.pixels_to_gt(pixels[index, pix], "srgb")
    want_gt = torch.stack([views[int(v)][1][int(k)] for v, k in zip(index, pix)]); want_al = torch.stack([views[int(v)][2][int(k)] for v, k in zip(index, pix)])
    assert torch.equal(gt.view(torch.int32), want_gt.view(torch.int32)) and torch.equal(al.view(torch.int32), want_al.view(torch.int32))
    assert all(np.array_equal(r[0], v[0]) for r, v in zip(raw, views))
