"""CPU, no GPU calls: what the stage-0 training path rests on apart from the kernel.  The float64 restatement of the radiance network (tests/radiance_bwd_refs.py)
against central differences on a T = 14 network, ReLU at exactly 0 and trunc_exp's +-15 clamp in it; the criterion's floor; save_stage0_checkpoint's layout and its
round trip through torch.load and the stage-0 loaders' own checks; the learning-rate schedule of main.py:285 at iterations 0, 500 and the last, evaluated by hand;
the EMA arithmetic; mirres_radiance_points_bwd's refusals before a device is touched; scripts/train_stage0.py's argument conflicts."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import density_refs as D                       # noqa: E402
import radiance_bwd_refs as B                  # noqa: E402


def _net(seed=7, log2_T=14, table_gain=1.0):
    L = D.layout(1.0, log2_T=log2_T)
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.normal(size=s)
    return L, [g(L["total"], 2) * table_gain, g(64, 32) * 0.15, g(16, 64) * 0.15, g(64, 31) * 0.15, g(64, 64) * 0.15, g(3, 64) * 0.5]


def _inputs(n, seed=3):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    return pos, dirs, rng.normal(size=n), rng.normal(size=(n, 3))


def _loss(params, L, pos, dirs, gs, grgb):
    net = B.network(params, L, pos, dirs, 1.0)
    return float(((torch.tensor(gs) * net["sigma"]).sum() + (torch.tensor(grgb) * net["rgb"]).sum()).detach())


def test_float64_gradients_against_central_differences():
    L, params = _net()
    pos, dirs, gs, grgb = _inputs(24)
    g = B.grads(params, L, pos, dirs, 1.0, gs, grgb)
    rng = np.random.default_rng(11)
    # the table entries that matter: those a point touches
    _, idx, _ = B.corners(L, pos, 1.0)
    for k, name in enumerate(B.NAMES):
        flat = params[k].reshape(-1)
        if name == "table":
            picks = [int(e) * 2 + int(c) for e, c in zip(rng.choice(np.unique(idx), 12), rng.integers(0, 2, 12))]
        else:
            picks = rng.choice(flat.size, 12, replace=False)
        for j in picks:
            h = 1e-6
            old = flat[j]
            flat[j] = old + h; up = _loss(params, L, pos, dirs, gs, grgb)
            flat[j] = old - h; dn = _loss(params, L, pos, dirs, gs, grgb)
            flat[j] = old
            fd = (up - dn) / (2 * h)
            got = g[k].reshape(-1)[j]
            # central differences of a piecewise-smooth function: h^2 f''' / 6 plus rounding 2 ulp(loss) / h, far inside 1e-6 of the tensor's scale here
            assert abs(fd - got) <= 1e-6 * max(1.0, np.abs(g[k]).max()), (name, j, fd, got)


def test_relu_at_zero_and_the_exp_clamp():
    L, params = _net()
    pos, dirs, gs, grgb = _inputs(8)
    # colour net, layer 0: a zeroed row gives a pre-activation of exactly 0 -> nothing passes: the row's gradient and its column of c1's gradient are 0
    p = [a.copy() for a in params]
    p[3][5, :] = 0.0
    g = B.grads(p, L, pos, dirs, 1.0, gs, grgb)
    assert (g[3][5] == 0).all() and (g[4][:, 5] == 0).all() and np.abs(g[3]).max() > 0
    # sigma_net's hidden layer likewise
    p = [a.copy() for a in params]
    p[1][9, :] = 0.0
    g = B.grads(p, L, pos, dirs, 1.0, gs, grgb)
    assert (g[1][9] == 0).all() and (g[2][:, 9] == 0).all()
    # trunc_exp: beyond +-15 the backward uses exp(+-15), not exp(h)
    for target in (40.0, -40.0):
        p = [a.copy() for a in params]
        net = B.network(p, L, pos, dirs, 1.0)
        h1 = torch.relu(net["z1"]).detach().numpy()
        # one row of w1 scaled so that point 0's h16[0] is the target
        h0 = float(h1[0] @ p[2][0])
        p[2][0] *= target / h0
        net = B.network(p, L, pos[:1], dirs[:1], 1.0)
        assert abs(float(net["h16"][0, 0].detach()) - target) < 1e-9
        g = B.grads(p, L, pos[:1], dirs[:1], 1.0, np.ones(1), np.zeros((1, 3)))
        want = np.exp(np.clip(target, -15, 15)) * torch.relu(net["z1"]).detach().numpy()[0]
        assert np.allclose(g[2][0], want, rtol=1e-12, atol=0)


def test_criterion_floor_and_zero_tensors():
    L, params = _net()
    pos, dirs, gs, grgb = _inputs(40)
    g64, terms = B.grads(params, L, pos, dirs, 1.0, gs, grgb, with_terms=True)
    g32 = B.grads(params, L, pos, dirs, 1.0, gs, grgb, dtype=torch.float32)
    for k, name in enumerate(B.NAMES):
        tsum, m = terms[name]
        assert tsum.shape == g64[k].shape and (np.abs(g64[k]) <= tsum * (1 + 1e-12) + 1e-300).all()       # |sum| <= sum |terms|
        worst, e, e_ref, floor = B.criterion(name, g32[k], g64[k], g32[k], terms)
        assert worst <= 0.5 + 1e-12 and e == e_ref                                                       # the yardstick against itself: half its own allowance
        assert B.criterion(name, g64[k] + 3.0 * np.abs(g64[k]).max() * max(e_ref, floor), g64[k], g32[k], terms)[0] > 1.0
    tsum, m = terms["table"]
    assert m.sum() == 40 * 16 * 8 * 2 and (tsum[m == 0] == 0).all() and terms["w0"][1].min() == 40      # every point in bounds: 8 corners per level and channel
    zero = [np.zeros_like(a) for a in g64]
    assert B.criterion("c2", zero[5], zero[5], zero[5], terms)[0] == 0.0 and B.criterion("c2", zero[5] + 1e-30, zero[5], zero[5], terms)[0] == np.inf


def _stand_ins(bound=1.0):
    from mirres_restir_nerf_mesh_amd import stage0 as S0
    net, total = S0.density_layout(bound)
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(s, generator=g)
    field = types.SimpleNamespace(PARAMETER_NAMES=("table", "w0", "w1_full", "c0", "c1", "c2"), net=net, table=r(total, 2), w0=r(64, 32), w1_full=r(16, 64), c0=r(64, 31),
                                  c1=r(64, 64), c2=r(3, 64))
    H = 16
    grid = types.SimpleNamespace(density_grid=r(1, H ** 3), density_bitfield=torch.randint(0, 256, (H ** 3 // 8,), generator=g, dtype=torch.uint8),
                                 aabb_train=torch.tensor([-1.0, -1, -1, 1, 1, 1]), mean_density=3.25)
    return field, grid, total


def test_save_stage0_checkpoint_round_trip(tmp_path):
    from mirres_restir_nerf_mesh_amd import checkpoint as CK, stage0 as S0
    field, grid, total = _stand_ins()
    path = str(tmp_path / "checkpoints" / "ngp.pth")
    opt = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=1e-2, eps=1e-15)
    shadow = [getattr(field, k) * 0.5 for k in field.PARAMETER_NAMES]
    CK.save_stage0_checkpoint(path, field, grid, epoch=3, global_step=77, optimizer=opt, ema={"decay": 0.95, "num_updates": 77, "shadow_params": shadow})
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert {"epoch", "global_step", "stats", "mean_density", "model", "optimizer", "ema"} <= set(ck) and ck["epoch"] == 3 and ck["global_step"] == 77
    assert ck["mean_density"] == 3.25
    m = ck["model"]
    # the names and shapes a NeRFNetwork's state dict has with --cuda_ray (nerf/network.py, nerf/renderer.py:399-421)
    want = {"aabb_train": (6,), "aabb_infer": (6,), "density_grid": (1, 4096), "density_bitfield": (512,), "encoder.embeddings": (total, 2), "encoder.offsets": (17,),
            "sigma_net.0.weight": (64, 32), "sigma_net.1.weight": (16, 64), "color_net.0.weight": (64, 31), "color_net.1.weight": (64, 64), "color_net.2.weight": (3, 64)}
    assert {k: tuple(v.shape) for k, v in m.items()} == want
    assert m["density_bitfield"].dtype == torch.uint8 and m["encoder.offsets"].dtype == torch.int32 and all(m[k].dtype == torch.float32 for k in CK.STAGE0_WEIGHT_KEYS)
    # `model` holds the averaged weights, `ema` keeps the field's own
    for k, name in zip(CK.STAGE0_WEIGHT_KEYS, field.PARAMETER_NAMES):
        assert torch.equal(m[k], getattr(field, name) * 0.5)
    assert all(torch.equal(a, getattr(field, k)) for a, k in zip(ck["ema"]["collected_params"], field.PARAMETER_NAMES)) and ck["ema"]["num_updates"] == 77
    assert torch.equal(m["density_grid"], grid.density_grid) and torch.equal(m["density_bitfield"], grid.density_bitfield)
    # what the loaders check before they copy anything, and the other reader of checkpoints
    S0.DensityField._checked_model(ck, 1.0, {})
    with pytest.raises(ValueError, match="bound"):
        S0.DensityField._checked_model(ck, 2.0, {})
    assert CK.read_checkpoint(path)["global_step"] == 77
    # without ema: the field's own weights
    CK.save_stage0_checkpoint(path, field, grid, epoch=0, global_step=1)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert "ema" not in ck and "optimizer" not in ck and torch.equal(ck["model"]["color_net.2.weight"], field.c2)
    with pytest.raises(ValueError, match="shadow_params"):
        CK.save_stage0_checkpoint(path, field, grid, ema={"decay": 0.95, "num_updates": 1, "shadow_params": shadow[::-1]})


def test_lr_schedule_is_main_py_285():
    import train_stage0 as T
    iters = 7500
    assert T.lr_factor(0, iters) == 0.01                                            # 0.01 + 0.99 * 0
    assert T.lr_factor(500, iters) == 1.0                                           # 0.01 + 0.99 * 1
    assert T.lr_factor(250, iters) == pytest.approx(0.01 + 0.99 * 0.5, rel=1e-15)
    assert T.lr_factor(iters, iters) == pytest.approx(0.1, rel=1e-15)               # 0.1 ** 1
    assert T.lr_factor(4000, iters) == pytest.approx(0.1 ** 0.5, rel=1e-15)         # half way through the decay
    # through torch's LambdaLR, stepped every iteration, and restarted in the middle as --resume does
    w = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([w], lr=1e-2, eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: T.lr_factor(it, iters))
    seen = []
    for it in range(600):
        seen.append(opt.param_groups[0]["lr"])
        opt.step(); sched.step()
    assert seen[0] == pytest.approx(1e-4) and seen[500] == pytest.approx(1e-2) and seen[599] == pytest.approx(1e-2 * 0.1 ** (99 / 7000))
    opt2 = torch.optim.Adam([w], lr=1e-2, eps=1e-15)
    opt2.param_groups[0]["initial_lr"] = 1e-2
    torch.optim.lr_scheduler.LambdaLR(opt2, lambda it: T.lr_factor(it, iters), last_epoch=299)
    assert opt2.param_groups[0]["lr"] == pytest.approx(seen[300])


def test_ema_arithmetic():
    import train_stage0 as T
    p = [torch.tensor([1.0, 2.0]), torch.tensor([[4.0]])]
    ema = T.EMA(p)
    assert ema.decay == 0.95 and all(torch.equal(s, q) and s is not q for s, q in zip(ema.shadow, p))
    want = [q.clone().double() for q in p]
    for t in range(1, 40):
        for q in p:
            q.add_(1.0)
        ema.update(p)
        d = min(0.95, (1 + t) / (10 + t))
        want = [d * s + (1 - d) * q.double() for s, q in zip(want, p)]
    assert ema.num_updates == 39 and min(0.95, (1 + 39) / (10 + 39)) < 0.95 and min(0.95, 400 / 409) == 0.95
    for s, wnt in zip(ema.shadow, want):
        assert torch.allclose(s.double(), wnt, rtol=1e-5)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params"} and sd["num_updates"] == 39


def test_bwd_entry_refuses_bad_arguments_before_touching_a_device():
    """Every call must fail an argument check (MIRRES_E_ARG exactly, not a device error) or have nothing to do: the pointers are not device memory."""
    from mirres_restir_nerf_mesh_amd import _lib as L, stage0 as S0
    lib = L.lib()
    E_ARG = -1
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    net = L.RadianceNet()
    dn, _ = S0.density_layout(1.0)
    net.grid = dn
    PARTIAL = 9344 * 4

    def call(net_=net, pos=p, dirs=p, n=4, bound=1.0, gs=p, grgb=p, outs=(p,) * 6, ws=p, ws_bytes=PARTIAL, max_blocks=1):
        return lib.mirres_radiance_points_bwd(C.byref(net_) if net_ is not None else None, pos, dirs, n, bound, gs, grgb, *outs, ws, ws_bytes, max_blocks, None)
    assert call(net_=None) == E_ARG and b"mirres_radiance_points_bwd" in lib.mirres_last_error()
    assert call() == E_ARG and b"NULL table" in lib.mirres_last_error()
    net.grid.table = net.grid.w0 = net.grid.w1 = p
    assert call() == E_ARG and b"w1 / c0 / c1 / c2" in lib.mirres_last_error()
    net.w1 = net.c0 = net.c1 = net.c2 = p
    for kw in (dict(n=-1), dict(n=(1 << 38) + 1), dict(bound=0.0), dict(bound=float("nan")), dict(bound=float("inf")), dict(max_blocks=-1), dict(pos=None), dict(dirs=None),
               dict(grgb=None)):
        assert call(**kw) == E_ARG and b"bad argument" in lib.mirres_last_error(), kw
    for k in range(6):
        outs = [p] * 6; outs[k] = None
        assert call(outs=tuple(outs)) == E_ARG and b"gradient output is NULL" in lib.mirres_last_error()
    assert call(ws=None) == E_ARG and b"workspace" in lib.mirres_last_error()
    assert call(ws_bytes=PARTIAL - 1) == E_ARG and b"workspace" in lib.mirres_last_error()
    assert call(n=600, max_blocks=2, ws_bytes=2 * PARTIAL - 1) == E_ARG and call(n=600, max_blocks=0, ws_bytes=2 * PARTIAL) == E_ARG      # three tiles by default
    assert call(n=0, pos=None, dirs=None, gs=None, grgb=None, outs=(None,) * 6, ws=None, ws_bytes=0) == 0                                  # nothing to do, no launch
    wb = lib.mirres_radiance_bwd_workspace_bytes
    assert wb(0, 0) == 0 and wb(1, 0) == PARTIAL and wb(256, 0) == PARTIAL and wb(257, 0) == 2 * PARTIAL and wb(600, 2) == 2 * PARTIAL and wb(600, 0) == 3 * PARTIAL
    assert wb(1 << 30, 0) == 1024 * PARTIAL and wb(1 << 30, 7) == 7 * PARTIAL and wb(-1, 0) == E_ARG and wb(4, -1) == E_ARG
    assert not any(host)
    rays = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="RadianceField"):
        S0.render_stage0_train(object(), object(), rays, rays)


def test_train_script_argument_conflicts(tmp_path, capsys):
    import train_stage0 as T
    a = T.parse_args(["--synthetic"])
    assert a.synthetic and a.workspace is None and (a.iters, a.num_rays, a.lr, a.update_extra_interval) == (7500, 4096, 1e-2, 16) and a.background == "white"
    assert (a.lambda_rgb, a.lambda_mask, a.T_thresh, a.max_steps, a.color_space) == (1.0, 0.1, 1e-4, 1024, "srgb") and not a.mark_untrained and not a.resume
    data = tmp_path / "lego"; data.mkdir(); (data / "transforms_train.json").write_text("{}")
    ws = str(tmp_path / "ws")
    a = T.parse_args(["--path", str(data), "--workspace", ws, "--background", "random", "--mark_untrained", "--bound", "2", "--iters", "300"])
    assert a.background == "random" and a.mark_untrained and a.bound == 2.0 and a.iters == 300
    real = ["--path", str(data), "--workspace", ws]
    for bad in (["--synthetic", "--path", str(data)], ["--synthetic", "--bound", "2"], ["--synthetic", "--color_space", "linear"], ["--synthetic", "--views", "1"],
                ["--synthetic", "--resume"], ["--path", str(data)], ["--workspace", ws], ["--path", str(tmp_path), "--workspace", ws], real + ["--resume"],
                real + ["--iters", "0"], real + ["--num_rays", "0"], real + ["--update_extra_interval", "0"], real + ["--background", "black"], real + ["--bound", "0"],
                real + ["--T_thresh", "1"], real + ["--grid_size", "48"], real + ["--dt_gamma", "-1"], real + ["--save_interval", "-1"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
        assert "error" in capsys.readouterr().err, bad
    help_text = T.build_parser().format_help()
    for word in ("GradScaler", "lambda_tv", "adaptive_num_rays", "sdf"):
        assert word in help_text
