"""The adjoint of the stage-0 radiance network on the device (csrc/radiance_bwd.hip) through stage0.RadianceField.backward_points / forward_train, the training
branch stage0.render_stage0_train over it, and scripts/train_stage0.py --synthetic: every element of the six gradients against the float64 network of
tests/radiance_bwd_refs.py under that module's criterion — |g - g64| / max |g64| <= max(2 E_ref, floor), E_ref what fp32 torch autograd loses on the same inputs,
floor the bound of an fp32 sum of the element's terms in any order; nothing tuned, no element left out — on the T = 19 and T = 14 layouts of test_gpu_density.py
(small tables: hash collisions inside one cell occur), at tile edges, on hostile positions, under contention, at ReLU's kink and beyond trunc_exp's clamp.
max_blocks is always given.

Zero and NaN directions are not sent: their spherical harmonics are NaN (0 / 0, as in the reference), so every gradient they touch is NaN in the reference as well,
and the marcher emits no sample for a ray with such a direction (raymarch.hip), so the training path never meets one.

Measured on the MI355X when these tests were written (DESIGN.md section 5.15 has the table): the worst element of any tensor and case sits at 0.87 of its allowance
(n = 1, c2), the --synthetic run's last-window loss at 9.7e-4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import density_refs as D                       # noqa: E402
import radiance_bwd_refs as B                  # noqa: E402
from test_gpu_density import Config, _points   # noqa: E402
from test_gpu_radiance import _dirs, _same_bits  # noqa: E402

@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


class Net:
    """A seeded RadianceField and its parameters on the host (read-only)."""

    def __init__(self, S0, log2_T, seed, edit=None):
        cfg = Config(S0, log2_T, seed)
        rng = np.random.default_rng(seed + 1000)
        c0 = (rng.normal(size=(64, 31)) * 0.15).astype(np.float32); c1 = (rng.normal(size=(64, 64)) * 0.15).astype(np.float32)
        c2 = (rng.normal(size=(3, 64)) * 0.5).astype(np.float32)
        self.L, self.log2_T = cfg.L, log2_T
        self.params = [np.array(a) for a in (cfg.table, cfg.w0, cfg.w1, c0, c1, c2)]
        if edit:
            edit(self.params)
        for a in self.params:
            a.setflags(write=False)
        self.field = S0.RadianceField(*(torch.tensor(a) for a in self.params), bound=1.0, log2_hashmap_size=log2_T)


@pytest.fixture(scope="module")
def nets(S0):
    return {19: Net(S0, 19, 101), 14: Net(S0, 14, 102)}


def _good_dirs(n, seed=21):
    d = _dirs(n + 2, seed)
    return np.delete(d, [12, 13], axis=0)[:n] if n + 2 > 13 else d[:n]           # without the zero and the NaN direction (module docstring)


def _cotangents(n, seed=9):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def _device_grads(net, pos, dirs, gs, grgb, max_blocks, grads=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = net.field.backward_points(t(pos), t(dirs), t(gs), t(grgb), grads=grads, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in out]


def _table_order_bound(net, pos, dirs, gs, grgb, start=None):
    """What two fp32 sums of a table entry's terms in different orders may differ by: each is within gamma_(m+1) sum |terms| of the exact sum (radiance_bwd_refs'
    floor); with `start` the sums begin from that value, one more term."""
    _, terms = B.grads(net.params, net.L, pos, dirs, 1.0, gs, grgb, with_terms=True)
    tsum, m = terms["table"]
    return 2.0 * B.gamma(m + 2) * (tsum + (0.0 if start is None else np.abs(start)))


def _hold(net, pos, dirs, gs, grgb, max_blocks, label):
    """The criterion on all six tensors, every element; prints each figure before it asserts."""
    got = _device_grads(net, pos, dirs, gs, grgb, max_blocks)
    g64, terms = B.grads(net.params, net.L, pos, dirs, 1.0, gs, grgb, with_terms=True)
    g32 = B.grads(net.params, net.L, pos, dirs, 1.0, gs, grgb, dtype=torch.float32)
    worst = {}
    for k, name in enumerate(B.NAMES):
        assert got[k].shape == g64[k].shape and got[k].dtype == np.float32
        worst[name] = B.criterion(name, got[k], g64[k], g32[k], terms)
        print("%s %-5s: worst error / allowance %.3f, E %.3e, E_ref %.3e, largest floor %.3e" % ((label, name) + worst[name]))
    for name, w in worst.items():
        assert w[0] <= 1.0, (label, name, w)
    return got, g64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_every_element_against_float64_at_tile_edges(nets, n):
    net = nets[14]
    pos, _ = _points(n)                                                           # the hostile positions first: corners, faces, one ulp outside, NaN, inf
    gs, grgb = _cotangents(n)
    _hold(net, pos, _good_dirs(n), gs, grgb, 4, "T=14 n=%d" % n)


@pytest.mark.parametrize("log2_T", [19, 14])
def test_a_block_that_loops_and_a_reduce_over_partials(nets, log2_T):
    n = 600                                                                       # three tiles on two blocks: block 0 takes tiles 0 and 2
    pos, oob = _points(n - 9)
    b = np.float32(1.0); zero = np.float32(0.0)
    inner = np.tile(np.array([0.3, -0.2, 0.7], np.float32), (9, 1))               # one ulp INSIDE each face, two ulps inside +bound: test_gpu_radiance.py's points
    for k, (axis, side) in enumerate((a, s) for a in range(3) for s in (1, -1)):
        inner[k, axis] = np.nextafter(np.float32(side) * b, zero)
    for axis in range(3):
        inner[6 + axis, axis] = np.nextafter(np.nextafter(b, zero), zero)
    pos = np.concatenate([pos, inner]); oob = np.concatenate([oob, np.zeros(9, bool)])
    assert oob.sum() == 5
    gs, grgb = _cotangents(n)
    net = nets[log2_T]
    got, g64 = _hold(net, pos, _good_dirs(n), gs, grgb, 2, "T=%d n=600 max_blocks=2" % log2_T)
    # two runs: the weight gradients bit for bit
    again = _device_grads(net, pos, _good_dirs(n), gs, grgb, 2)
    for k in range(1, 6):
        assert _same_bits(got[k], again[k]), B.NAMES[k]
    # an out-of-bounds point scatters nothing and gives sigma_net nothing, but its colour path counts: alone, it leaves table, w0 and w1 at exactly 0
    only = _device_grads(net, pos[oob], _good_dirs(n)[oob], gs[oob], grgb[oob], 2)
    assert not only[0].any() and not only[1].any() and not only[2].any() and only[3].any() and only[4].any() and only[5].any()


def _one_cell(L, level, n, seed):
    """n points inside one cell of `level` (strictly inside, away from its faces)."""
    rng = np.random.default_rng(seed)
    s = float(L["scale"][level])
    cell = np.array([int(s * 0.55), int(s * 0.35), int(s * 0.6)], np.float64)
    u = (cell + rng.uniform(0.05, 0.95, size=(n, 3)) - 0.5) / s                   # u * s + 0.5 in cell + (0.05, 0.95)
    pos = (u * 2.0 - 1.0).astype(np.float32)
    _, idx, _ = B.corners(L, pos, 1.0)
    assert (idx[:, level, :] == idx[0, level, :]).all()
    return pos


@pytest.mark.parametrize("level", [15, 0])
def test_contended_sums_in_one_cell(nets, level):
    net = nets[14]
    n = 4096
    pos = _one_cell(net.L, level, n, 40 + level)
    gs, grgb = _cotangents(n, 12)
    _hold(net, pos, _good_dirs(n, 5), gs, grgb, 8, "T=14 one cell of level %d" % level)


def test_colliding_corners_of_one_cell_both_land(nets):
    net = nets[14]
    L = net.L
    rng = np.random.default_rng(77)
    cand = rng.uniform(-0.9, 0.9, size=(4000, 3)).astype(np.float32)
    _, idx, _ = B.corners(L, cand, 1.0)
    hashed = np.nonzero(L["hashed"])[0]
    dup = np.array([[len(np.unique(idx[i, l])) < 8 for l in hashed] for i in range(len(cand))])
    rows = np.nonzero(dup.any(axis=1))[0]
    assert len(rows) > 0, "no candidate with two corners of one hashed cell in the same entry"
    i = rows[0]
    l = hashed[np.nonzero(dup[i])[0][0]]
    assert len(np.unique(idx[i, l])) < 8 and L["hashed"][l]
    pos = cand[i:i + 1]
    gs, grgb = _cotangents(1, 3)
    got, g64 = _hold(net, pos, _good_dirs(1), gs, grgb, 1, "T=14 collision at level %d" % l)
    # the shared entry holds the sum of both corners' shares
    e, cnt = np.unique(idx[i, l], return_counts=True)
    shared = e[cnt > 1][0]
    assert g64[0][shared].any()                                                    # the criterion above has held this entry to the sum of both shares


def test_null_grad_sigma_is_zeros_and_zero_grad_rgb_leaves_the_colour_net_alone(nets):
    net = nets[14]
    n = 300
    pos, _ = _points(n)
    d = _good_dirs(n)
    gs, grgb = _cotangents(n)
    a = _device_grads(net, pos, d, None, grgb, 2)
    b = _device_grads(net, pos, d, np.zeros(n, np.float32), grgb, 2)
    for k in range(1, 6):
        assert _same_bits(a[k], b[k]), B.NAMES[k]
    assert (np.abs(a[0].astype(np.float64) - b[0]) <= _table_order_bound(net, pos, d, None, grgb)).all()      # the table is summed by atomics: equal up to the order of the adds
    got, _ = _hold(net, pos, d, gs, np.zeros((n, 3), np.float32), 2, "T=14 grad_rgb = 0")
    assert not got[3].any() and not got[4].any() and not got[5].any() and got[1].any() and got[2][0].any() and not got[2][1:].any()


def test_relu_at_exactly_zero(S0):
    def edit(p):
        p[3][5, :] = 0.0                                                          # colour layer 0, neuron 5: pre-activation exactly 0 at every point
        p[4][7, :] = 0.0                                                          # colour layer 1, neuron 7
        p[1][9, :] = 0.0                                                          # sigma_net's hidden neuron 9
    net = Net(S0, 14, 102, edit)
    n = 257
    pos, _ = _points(n)
    gs, grgb = _cotangents(n)
    got, _ = _hold(net, pos, _good_dirs(n), gs, grgb, 2, "T=14 zeroed rows")
    assert not got[3][5].any() and not got[4][:, 5].any() and not got[4][7].any() and not got[5][:, 7].any() and not got[1][9].any() and not got[2][:, 9].any()
    assert got[3][4].any() and got[4][6].any() and got[1][8].any()


@pytest.mark.parametrize("scale", [40.0, -40.0])
def test_sigma_beyond_the_clamp(S0, scale):
    probe = Net(S0, 14, 102)
    n = 64
    pos = np.random.default_rng(8).uniform(-0.9, 0.9, size=(n, 3)).astype(np.float32)
    h0 = B.network(probe.params, probe.L, pos, _good_dirs(n), 1.0)["h16"][:, 0].detach().numpy()

    def edit(p):
        p[2][0] *= np.float32(scale / np.abs(h0).max())                           # row 0 of w1: the largest |h16[0]| becomes 40
    net = Net(S0, 14, 102, edit)
    h = B.network(net.params, net.L, pos, _good_dirs(n), 1.0)["h16"][:, 0].detach().numpy()
    assert (np.abs(h) > 15).any() and (np.abs(h) < 15).any() and h.max() < 80
    gs, grgb = _cotangents(n)
    _hold(net, pos, _good_dirs(n), gs, grgb, 1, "T=14 |h16[0]| up to 40")


def test_accumulates_into_its_outputs_and_n_zero_touches_nothing(nets):
    net = nets[14]
    n = 130
    pos, _ = _points(n)
    gs, grgb = _cotangents(n)
    fresh = _device_grads(net, pos, _good_dirs(n), gs, grgb, 2)
    rng = np.random.default_rng(1)
    start = [rng.normal(size=g.shape).astype(np.float32) for g in fresh]
    bufs = [torch.from_numpy(s.copy()).cuda() for s in start]
    got = _device_grads(net, pos, _good_dirs(n), gs, grgb, 2, grads=bufs)
    for k in range(1, 6):
        assert _same_bits(got[k], start[k] + fresh[k]), B.NAMES[k]               # one fp32 addition of the reduced sum
    assert (np.abs(got[0].astype(np.float64) - (start[0].astype(np.float64) + fresh[0])) <= _table_order_bound(net, pos, _good_dirs(n), gs, grgb, start[0])).all()
    before = [b.clone() for b in bufs]
    e = torch.empty((0, 3), device="cuda")
    net.field.backward_points(e, e, None, e, grads=bufs, max_blocks=2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))


def test_forward_train_keeps_the_bits_and_density_follows_w1(S0):
    net = Net(S0, 14, 102)
    f = net.field
    n = 300
    pos, _ = _points(n)
    x, d = torch.from_numpy(pos).cuda(), torch.from_numpy(_good_dirs(n)).cuda()
    s0, c0 = f.forward(x, d)
    dens0 = f.density(x)
    params = f.parameters()
    assert [tuple(p.shape) for p in params] == [tuple(a.shape) for a in net.params] and all(p.is_leaf and p.requires_grad for p in params)
    assert params[2].data_ptr() == f.w1_full.data_ptr() and f.w1.data_ptr() == f.w1_full.data_ptr()
    s1, c1 = f.forward_train(x, d)
    assert s1.requires_grad and c1.requires_grad and _same_bits(s0.cpu().numpy(), s1.detach().cpu().numpy()) and _same_bits(c0.cpu().numpy(), c1.detach().cpu().numpy())
    assert _same_bits(f.rgb(x, d).cpu().numpy(), c0.cpu().numpy()) and _same_bits(dens0.cpu().numpy(), s0.cpu().numpy())
    gs, grgb = _cotangents(n)
    f.bwd_max_blocks = 2
    ((s1 * torch.from_numpy(gs).cuda()).sum() + (c1 * torch.from_numpy(grgb).cuda()).sum()).backward()
    direct = _device_grads(net, pos, _good_dirs(n), gs, grgb, 2)
    for k, p in enumerate(params):
        assert p.grad is not None and p.grad.shape == p.shape
        if k:
            assert _same_bits(p.grad.cpu().numpy(), direct[k]), B.NAMES[k]
    assert x.grad is None and d.grad is None
    # an optimiser's in-place step on w1_full reaches density() and the radiance query alike
    with torch.no_grad():
        f.w1_full[0].mul_(0.5)
    dens1 = f.density(x).cpu().numpy()
    s2 = f.forward(x, d)[0].cpu().numpy()
    assert _same_bits(dens1, s2) and not _same_bits(dens1, dens0.cpu().numpy())
    w = [np.array(a) for a in net.params]; w[2][0] *= np.float32(0.5)
    ref = S0.DensityField(torch.tensor(w[0]), torch.tensor(w[1]), torch.tensor(w[2]), bound=1.0, log2_hashmap_size=14)
    assert _same_bits(ref.density(x).cpu().numpy(), dens1)


def test_one_whole_training_step_against_the_float64_network(S0):
    """render_stage0_train -> MSE -> backward on the synthetic checkpoint's density with init_random colour weights, against the same chain with the float64 network
    in the middle on the product's own samples: the cotangents of sigma and rgb are taken from the product's composite (its adjoint is tested on its own), so the
    criterion above applies to the six gradients unchanged."""
    ck = S0.synthetic_radiance_checkpoint(S=32)
    rnd = S0.RadianceField.init_random(1.0, seed=4)
    m = ck["model"]
    field = S0.RadianceField(m["encoder.embeddings"], m["sigma_net.0.weight"], m["sigma_net.1.weight"], rnd.c0, rnd.c1, rnd.c2, bound=1.0)
    grid = S0.DensityGrid.from_checkpoint(ck, bound=1.0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for _ in range(3):
        grid.update(field, noise=torch.rand(grid.cascade, grid.grid_size ** 3, 3, generator=gen, device="cuda"))
    from render_stage0 import orbit_poses
    from mirres_restir_nerf_mesh_amd import harness
    o, d = harness.get_rays(torch.from_numpy(np.asarray(orbit_poses(1)[0], np.float32)).cuda(), (80.0, 80.0, 4.0, 4.0), 8, 8)      # 64 rays through the ball
    noises = torch.rand(64, generator=gen, device="cuda")
    target = torch.rand(64, 3, generator=gen, device="cuda")
    params = field.parameters()
    field.bwd_max_blocks = 2
    out = S0.render_stage0_train(field, grid, o, d, bg_color=1.0, perturb=True, noises=noises)
    assert set(out) == {"image", "depth", "weights_sum", "weights", "num_points", "xyzs"} and out["num_points"] > 256 and out["xyzs"].shape == (out["num_points"], 3)
    ((out["image"] - target) ** 2).mean().backward()
    got = [p.grad.cpu().numpy() for p in params]
    # the same samples again, with the cotangents of sigma and rgb caught on the way
    from mirres_restir_nerf_mesh_amd import raymarching as RM
    nears, fars = RM.near_far_from_aabb(o, d, grid.aabb_train, grid.min_near)
    xyzs, dirs, ts, rays = RM.march_rays_train(o, d, grid.bound, False, grid.density_bitfield, grid.cascade, grid.grid_size, nears, fars, True, 0, 1024, noises)
    assert torch.equal(xyzs, out["xyzs"])
    dn = S0._safe_normalize(dirs)
    sig, rgb = field.forward(xyzs, dn)
    sig.requires_grad_(True); rgb.requires_grad_(True)
    _, ws, _, img = RM.composite_rays_train(sig, rgb, ts, rays, 1e-4, False)
    (((img + (1 - ws).unsqueeze(-1) * 1.0) - target) ** 2).mean().backward()
    pos, dd, gs, grgb = (t.detach().cpu().numpy() for t in (xyzs, dn, sig.grad, rgb.grad))
    host = [p.detach().cpu().numpy() for p in params]
    L = D.layout(1.0)
    g64, terms = B.grads(host, L, pos, dd, 1.0, gs, grgb, with_terms=True)
    g32 = B.grads(host, L, pos, dd, 1.0, gs, grgb, dtype=torch.float32)
    for k, name in enumerate(B.NAMES):
        w = B.criterion(name, got[k], g64[k], g32[k], terms)
        print("whole step %-5s: worst error / allowance %.3f, E %.3e, E_ref %.3e, largest floor %.3e" % ((name,) + w))
        assert w[0] <= 1.0, (name, w)
    assert np.abs(g64[3]).max() > 0 and np.abs(g64[0]).max() > 0


SYNTHETIC_LAST_WINDOW_LOSS = 9.7e-4                                                 # measured on the MI355X for --seed 0; the test allows twice


def test_train_script_synthetic_run_learns_and_its_checkpoint_is_consumed(S0, tmp_path):
    ws = str(tmp_path / "ws")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_stage0.py"), "--synthetic", "--workspace", ws, "--iters", "160", "--num_rays", "1024",
                        "--window", "20", "--views", "8", "--grid_size", "64"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    line = [l for l in r.stdout.splitlines() if l.startswith("[RESULT] first-window")][0].split()
    first, last = float(line[3]), float(line[6])
    assert last < first, (first, last)
    assert last < 2.0 * SYNTHETIC_LAST_WINDOW_LOSS, (last, SYNTHETIC_LAST_WINDOW_LOSS)
    assert "held-out PSNR" in r.stdout
    path = os.path.join(ws, "checkpoints", "ngp.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 160 and "ema" in ck and "optimizer" in ck
    # render_stage0.py's loader, and the mesh export
    field = S0.RadianceField.from_checkpoint(ck, bound=1.0)
    grid = S0.DensityGrid.from_checkpoint(ck, bound=1.0)
    from render_stage0 import orbit_poses
    from mirres_restir_nerf_mesh_amd import harness
    o, d = harness.get_rays(torch.from_numpy(np.asarray(orbit_poses(1)[0], np.float32)).cuda(), (35.0, 35.0, 16.0, 16.0), 32, 32)
    out = S0.render_stage0(field, grid, o, d)
    assert torch.isfinite(out["image"]).all() and float(out["weights_sum"].max()) > 0.5
    mesh = S0.export_stage0(os.path.join(ws, "mesh_stage0"), ckpt=ck, decimate_target=0, log=lambda m: None)
    assert os.path.exists(mesh)
