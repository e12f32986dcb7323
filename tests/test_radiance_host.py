"""CPU (no GPU calls): the restatement the stage-0 radiance network is held to (tests/radiance_refs.py) — the float64 spherical harmonics are orthonormal, the
float32 restatement of the fixed arithmetic stays within its derived bound of them and has every sign right —, the synthetic radiance checkpoint's closed form, the
refusals of RadianceField.from_checkpoint, and the argument checks of mirres_radiance_points / mirres_sh_encode / render_stage0 / scripts/render_stage0.py that
need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import radiance_refs as RR      # noqa: E402

PI = np.pi
K1, K3A, K3C, K3D = np.sqrt(3 / (4 * PI)), 0.25 * np.sqrt(35 / (2 * PI)), 0.25 * np.sqrt(21 / (2 * PI)), 0.25 * np.sqrt(7 / PI)
K20, K22 = 0.25 * np.sqrt(5 / PI), 0.25 * np.sqrt(15 / PI)


def test_sh64_is_orthonormal_over_the_sphere():
    """Products of two outputs are polynomials of degree <= 6: a 5-point Gauss-Legendre rule in z (exact to degree 9) times 9 equally spaced azimuths (exact for
    trigonometric degree <= 8) integrates them exactly."""
    z, wz = np.polynomial.legendre.leggauss(5)
    phi = 2 * PI * np.arange(9) / 9
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1 - zz * zz)
    d = np.stack([s * np.cos(pp), s * np.sin(pp), zz], -1).reshape(-1, 3)
    w = (wz[:, None] * np.full_like(pp, 2 * PI / 9)).reshape(-1)
    Y = RR.sh64(d)
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(16)).max() <= 1e-12, np.abs(gram - np.eye(16)).max()


def _directions(n, seed=7):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 4] *= np.float32(1e-3); d[n // 4: n // 2] *= np.float32(1e3)
    d[-1] = [0.3, -0.0, 0.0]; d[-2] = [-0.0, -0.0, 2.0]
    return d


def test_sh32_within_the_derived_bound_of_sh64():
    d = _directions(20000)
    got = RR.sh32(d).astype(np.float64); want = RR.sh64(d.astype(np.float64))
    err = np.abs(got - want); bound = RR.sh_bound()
    print("max |sh32 - sh64| / bound per output:", (err.max(axis=0) / bound).round(3))
    assert bound.shape == (16,) and (bound < 4e-6).all() and (err <= bound).all()
    assert np.array_equal(RR.sh32(d * np.float32(4.0)).view(np.uint32), RR.sh32(d).view(np.uint32))      # a power of two scales s and n exactly: the same bits
    bad = RR.sh32(np.array([[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0]], np.float32))
    assert np.isnan(bad[:2, 1:]).all() and np.isnan(bad[2, 3]) and (bad[:, 0] == RR.C0).all()            # 0 / 0, NaN, inf / inf (the x terms); output 0 is a constant


AXES = {  # direction -> the non-zero outputs past the constant 0 and the constant 6 (every other output is +-0)
    (1, 0, 0): {3: -K1, 8: K22, 13: K3C, 15: -K3A}, (-1, 0, 0): {3: K1, 8: K22, 13: -K3C, 15: K3A},
    (0, 1, 0): {1: -K1, 8: -K22, 9: K3A, 11: K3C}, (0, -1, 0): {1: K1, 8: -K22, 9: -K3A, 11: -K3C},
    (0, 0, 1): {2: K1, 12: 2 * K3D}, (0, 0, -1): {2: -K1, 12: -2 * K3D}}


@pytest.mark.parametrize("axis", sorted(AXES))
def test_known_answers_on_the_axes_pin_every_sign(axis):
    want = np.zeros(16); want[0] = 0.5 * np.sqrt(1 / PI); want[6] = K20 * (3.0 * axis[2] ** 2 - 1.0)
    for k, v in AXES[axis].items():
        want[k] = v
    d = np.array([axis], np.float64) * 2.5
    assert np.abs(RR.sh64(d)[0] - want).max() <= 1e-15
    assert (np.abs(RR.sh32(d.astype(np.float32))[0].astype(np.float64) - want) <= RR.sh_bound()).all()


def _sigmoid(h):
    return 1.0 / (1.0 + np.exp(-h))


def _weights_of(ck):
    m = ck["model"]
    return tuple(m[k].numpy() for k in ("sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight", "color_net.2.weight"))


def test_synthetic_radiance_checkpoint_is_its_closed_form():
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    before = S0.synthetic_checkpoint()
    ck = S0.synthetic_radiance_checkpoint()
    plain = S0.synthetic_checkpoint()
    assert sorted(plain["model"]) == ["density_grid", "encoder.embeddings", "encoder.offsets", "sigma_net.0.weight", "sigma_net.1.weight"]      # unchanged by the call
    assert sorted(ck["model"]) == sorted(list(plain["model"]) + ["color_net.0.weight", "color_net.1.weight", "color_net.2.weight"])
    assert ck["mean_density"] == plain["mean_density"] == before["mean_density"]
    for k in plain["model"]:
        assert torch.equal(plain["model"][k], before["model"][k]), k
        if k != "sigma_net.1.weight":
            assert torch.equal(ck["model"][k], plain["model"][k]), k
    w1 = ck["model"]["sigma_net.1.weight"]
    assert torch.equal(w1[0], plain["model"]["sigma_net.1.weight"][0]) and not w1[1:15].any() and w1[15].tolist() == [1.0] + [0.0] * 63
    assert [tuple(ck["model"]["color_net.%d.weight" % l].shape) for l in range(3)] == [(64, 31), (64, 64), (3, 64)]
    # the docstring's closed form, restated: hand-made features (F in column 0; the other columns are noise no weight reads) and exact directions
    rng = np.random.default_rng(11)
    n = 500
    feat = rng.normal(size=(n, 32)); F = rng.uniform(0.3, 2.0, size=n); feat[:, 0] = F
    d = _directions(n)
    sh = RR.sh32(d)
    out = RR.forward64(feat, sh, _weights_of(ck))
    u = d.astype(np.float64); u = u / np.sqrt((u * u).sum(axis=1, keepdims=True))
    SH0, SH1 = float(np.float32(0.28209479177387814)), float(np.float32(0.48860251190291987))
    want = np.stack([_sigmoid(4 * SH1 * u[:, 0]), _sigmoid(4 * SH1 * u[:, 2]), _sigmoid(2 * (1.5 * F - 4 * SH0))], axis=1)
    assert np.allclose(out["sigma"], np.exp(1.5 * F), rtol=1e-14) and np.abs(out["h16"][:, 1:15]).max() == 0 and np.allclose(out["h16"][:, 15], 1.5 * F, rtol=1e-15)
    # r and g read the fp32 encoder's sh[3] and sh[2]: off the exact direction's by at most sh_bound, times the gain 4 and the logistic function's slope 1/4
    tol = np.array([RR.sh_bound()[3], RR.sh_bound()[2], 0.0]) + 1e-15
    assert (np.abs(out["rgb"] - want) <= tol).all(), np.abs(out["rgb"] - want).max(axis=0)
    assert np.allclose(S0.synthetic_radiance_color(d, F), want, rtol=0, atol=1e-15)
    assert want[:, 0].min() < 0.2 and want[:, 0].max() > 0.8 and want[:, 2].min() < 0.25 and want[:, 2].max() > 0.95     # the channels move


def test_from_checkpoint_refusals():
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    good = S0.synthetic_radiance_checkpoint()

    def variant(**changes):
        ck = {"mean_density": good["mean_density"], "model": dict(good["model"])}
        for k, v in changes.items():
            k = k.replace("__", ".")
            if v is None:
                del ck["model"][k]
            else:
                ck["model"][k] = v
        return ck
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        S0.RadianceField.from_checkpoint(variant(encoder__encoder__params=torch.zeros(8)))
    with pytest.raises(KeyError, match="not a stage-0 radiance network"):
        S0.RadianceField.from_checkpoint(S0.synthetic_checkpoint())
    for l in range(3):
        with pytest.raises(KeyError, match="color_net.%d.weight: not a stage-0 radiance network" % l):
            S0.RadianceField.from_checkpoint(variant(**{"color_net__%d__weight" % l: None}))
    with pytest.raises(KeyError, match="not a stage-0 density network"):
        S0.RadianceField.from_checkpoint(variant(sigma_net__0__weight=None))
    for key, shape in (("color_net__0__weight", (64, 32)), ("color_net__1__weight", (64, 63)), ("color_net__2__weight", (4, 64)), ("color_net__2__weight", (64, 3))):
        with pytest.raises(ValueError, match="31 -> 64 -> 64 -> 3"):
            S0.RadianceField.from_checkpoint(variant(**{key: torch.zeros(shape)}))
    with pytest.raises(ValueError, match="32 -> 64 -> 16"):
        S0.RadianceField.from_checkpoint(variant(sigma_net__1__weight=torch.zeros(1, 64)))
    for l in range(3):
        with pytest.raises(ValueError, match="bias"):
            S0.RadianceField.from_checkpoint(variant(**{"color_net__%d__bias" % l: torch.zeros(3)}))
    with pytest.raises(ValueError, match="bias"):
        S0.RadianceField.from_checkpoint(variant(sigma_net__0__bias=torch.zeros(64)))
    with pytest.raises(ValueError, match="--bound"):
        S0.RadianceField.from_checkpoint(good, bound=2.0)
    m = good["model"]
    args = [m["encoder.embeddings"], m["sigma_net.0.weight"], m["sigma_net.1.weight"], m["color_net.0.weight"], m["color_net.1.weight"], m["color_net.2.weight"]]
    for i, bad in ((2, torch.zeros(64)), (2, torch.zeros(1, 64)), (3, torch.zeros(64, 32)), (4, torch.zeros(64, 32)), (5, torch.zeros(64, 3))):
        a = list(args); a[i] = bad
        with pytest.raises(ValueError, match="RadianceField"):
            S0.RadianceField(*a)


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    """Every call below must fail an argument check (MIRRES_E_ARG exactly, not a device error) or have nothing to do: the pointers are not device memory."""
    from mirres_restir_nerf_mesh_amd import _lib as L, stage0 as S0
    lib = L.lib()
    E_ARG = -1
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    net = L.RadianceNet()
    dn, _ = S0.density_layout(1.0)
    net.grid = dn
    rp = lambda net_, pos, dirs, n, bound, sig, rgb: lib.mirres_radiance_points(C.byref(net_) if net_ is not None else None, pos, dirs, n, bound, sig, rgb, None, None, None)
    assert rp(None, p, p, 4, 1.0, p, p) == E_ARG and b"mirres_radiance_points" in lib.mirres_last_error()
    assert rp(net, p, p, 4, 1.0, p, p) == E_ARG and b"NULL table" in lib.mirres_last_error()              # dn_net_ok on the grid
    net.grid.table = net.grid.w0 = net.grid.w1 = p
    assert rp(net, p, p, 4, 1.0, p, p) == E_ARG and b"w1 / c0 / c1 / c2" in lib.mirres_last_error()
    for missing in ("w1", "c0", "c1", "c2"):
        net.w1 = net.c0 = net.c1 = net.c2 = p
        setattr(net, missing, None)
        assert rp(net, p, p, 4, 1.0, p, p) == E_ARG and b"w1 / c0 / c1 / c2" in lib.mirres_last_error()
    net.w1 = net.c0 = net.c1 = net.c2 = p
    bad = L.RadianceNet.from_buffer_copy(net); bad.grid.num_levels = 17
    assert rp(bad, p, p, 4, 1.0, p, p) == E_ARG and b"num_levels" in lib.mirres_last_error()
    for n, bound in ((-1, 1.0), ((1 << 38) + 1, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        assert rp(net, p, p, n, bound, p, p) == E_ARG, (n, bound)
    assert rp(net, None, p, 4, 1.0, p, p) == E_ARG and rp(net, p, None, 4, 1.0, p, p) == E_ARG and rp(net, p, p, 4, 1.0, p, None) == E_ARG
    assert rp(net, None, None, 0, 1.0, None, None) == 0                                                     # nothing to do is no error, and no launch
    assert lib.mirres_sh_encode(None, 4, p, None) == E_ARG and b"mirres_sh_encode" in lib.mirres_last_error()
    assert lib.mirres_sh_encode(p, 4, None, None) == E_ARG and lib.mirres_sh_encode(p, -1, p, None) == E_ARG and lib.mirres_sh_encode(p, (1 << 38) + 1, p, None) == E_ARG
    assert lib.mirres_sh_encode(None, 0, None, None) == 0
    assert not any(host)
    rays = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="RadianceField"):
        S0.render_stage0(object(), object(), rays, rays)


def test_render_script_argument_conflicts(tmp_path, capsys):
    import render_stage0 as RS
    ws = str(tmp_path)
    a = RS.parse_args(["--synthetic", "--workspace", ws])
    assert a.synthetic and a.name == "synthetic" and a.T_thresh == 1e-4 and a.max_steps == 1024 and a.color_space == "srgb" and a.H is None
    assert RS.parse_args(["--synthetic"]).workspace is None                                 # the temporary workspace is made when the run starts, not by parsing
    here = __file__
    a = RS.parse_args(["--workspace", ws, "--ckpt", here, "--transforms", here, "--bound", "2", "--color_space", "linear", "--H", "40", "--W", "30"])
    assert a.name == "test_radiance_host" and a.bound == 2.0 and (a.H, a.W) == (40, 30)
    real = ["--workspace", ws, "--ckpt", here, "--transforms", here]
    for bad in (["--synthetic", "--ckpt", here], ["--synthetic", "--transforms", here], ["--synthetic", "--bound", "2"], ["--synthetic", "--color_space", "linear"],
                ["--synthetic", "--views", "0"], ["--synthetic", "--H", "64"], ["--synthetic", "--max_steps", "0"], ["--synthetic", "--T_thresh", "1"],
                ["--ckpt", here, "--transforms", here], ["--workspace", ws, "--ckpt", here], ["--workspace", ws, "--transforms", here],
                ["--workspace", ws, "--ckpt", here + ".nope", "--transforms", here], real + ["--bound", "0"], real + ["--downscale", "0"], real + ["--color_space", "hdr"],
                real + ["--dt_gamma", "-1"], real + ["--H", "0", "--W", "4"]):
        with pytest.raises(SystemExit):
            RS.parse_args(bad)
        assert "error" in capsys.readouterr().err, bad


def test_render_script_reads_its_views_without_a_device(tmp_path):
    """parse_args through the frame list on a transforms file: sizes, --downscale, the focal length from camera_angle_x, nerf_matrix_to_ngp's --scale / --offset on
    the translation alone, and the image path next to the transforms file."""
    import json
    import render_stage0 as RS
    data = tmp_path / "data"; data.mkdir()
    pose = np.eye(4); pose[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; pose[:3, 3] = [1.0, -2.0, 3.0]
    tf = data / "transforms_test.json"
    tf.write_text(json.dumps({"camera_angle_x": 0.8, "w": 120, "h": 80, "frames": [{"file_path": "./test/r_0", "transform_matrix": pose.tolist()},
                                                                                   {"file_path": "./test/r_1", "transform_matrix": np.eye(4).tolist()}]}))
    ckpt = tmp_path / "ngp_stage0_ep0007.pth"; ckpt.write_bytes(b"")
    base = ["--workspace", str(tmp_path), "--ckpt", str(ckpt), "--transforms", str(tf)]
    a = RS.parse_args(base + ["--downscale", "2", "--scale", "0.5", "--offset", "0.1", "0.2", "0.3"])
    assert a.name == "ngp_stage0_ep0007"
    H, W, focal, frames = RS.load_views(a)
    assert (H, W) == (40, 60) and abs(focal - 0.5 * 60 / np.tan(0.4)) < 1e-9 and len(frames) == 2
    p0 = np.asarray(frames[0]["pose"], np.float64)
    assert p0.shape == (4, 4) and np.array_equal(p0[:3, :3], pose[:3, :3]) and np.allclose(p0[:3, 3], [0.6, -0.8, 1.8], atol=1e-6)
    assert [os.path.normpath(f["file"]) for f in frames] == [str(data / "test" / "r_0.png"), str(data / "test" / "r_1.png")]
    H, W, focal, _ = RS.load_views(RS.parse_args(base + ["--H", "30", "--W", "50"]))
    assert (H, W) == (30, 50) and abs(focal - 0.5 * 50 / np.tan(0.4)) < 1e-9
    H, W, focal, frames = RS.load_views(RS.parse_args(["--synthetic", "--views", "4"]))
    assert (H, W) == (128, 128) and len(frames) == 4 and all(f["file"] is None for f in frames)
    for f in frames:                                                                       # orbit cameras: orthonormal, at distance 3, looking at the origin
        P = np.asarray(f["pose"], np.float64)
        assert np.allclose(P[:3, :3].T @ P[:3, :3], np.eye(3), atol=1e-6) and abs(np.linalg.norm(P[:3, 3]) - 3.0) < 1e-6
        assert np.allclose(-P[:3, 2], -P[:3, 3] / 3.0, atol=1e-6)
