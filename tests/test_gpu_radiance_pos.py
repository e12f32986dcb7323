"""The position adjoint of the stage-0 radiance network on the device (csrc/radiance_pos.hip) through stage0.RadianceField.backward_pos and rgb_train: every
element of grad_pos against the float64 network of tests/radiance_pos_refs.py (the position a differentiable leaf; cell and in-bounds decision by the fp32 rule)
under the project's criterion — |g - g64| / max |g64| <= max(2 E_ref, floor[e]), E_ref what the same restatement loses in fp32, floor[e] = gamma_(m+1) sum |terms| /
max |g64| with m = 128 products per element in bounds; nothing tuned, no element left out — on the T = 14 and T = 19 layouts of test_gpu_density.py, at block
edges, on hostile positions (corners, faces, one ulp outside, NaN, inf: exactly 0 where out of bounds), with colliding corners in a hashed cell, beyond trunc_exp's
clamp, at ReLU's kink.  Zero and NaN directions are not sent, as in test_gpu_radiance_bwd.py.

Measured on the MI355X when these tests were written: DESIGN.md section 5.17."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radiance_bwd_refs as B                  # noqa: E402
import radiance_pos_refs as P                  # noqa: E402
from test_gpu_density import _points           # noqa: E402
from test_gpu_radiance import _same_bits       # noqa: E402
from test_gpu_radiance_bwd import Net, _good_dirs, _cotangents      # noqa: E402


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


@pytest.fixture(scope="module")
def nets(S0):
    return {19: Net(S0, 19, 101), 14: Net(S0, 14, 102)}


def _device(net, pos, dirs, gs, grgb):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = net.field.backward_pos(t(pos), t(dirs), t(gs), t(grgb))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _hold(net, pos, dirs, gs, grgb, label):
    """The criterion on every element of grad_pos; prints each figure before it asserts."""
    got = _device(net, pos, dirs, gs, grgb)
    g64, terms = P.grad_pos(net.params, net.L, pos, dirs, 1.0, gs, grgb, with_terms=True)
    g32 = P.grad_pos(net.params, net.L, pos, dirs, 1.0, gs, grgb, dtype=torch.float32)
    assert got.shape == g64.shape == (len(pos), 3) and got.dtype == np.float32
    w = P.criterion(got, g64, g32, terms)
    print("%s: worst error / allowance %.3f, E %.3e, E_ref %.3e, largest floor %.3e, max |g64| %.3e" % ((label,) + w + (float(np.abs(g64).max()),)))
    assert w[0] <= 1.0, (label, w)
    ok = P.cells(net.L, pos, 1.0)[0]
    assert not got[~ok].any(), "a point out of bounds must get exactly 0"
    return got, g64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_every_element_against_float64_at_block_edges(nets, n):
    pos, _ = _points(n)                                                           # the hostile positions first: corners, faces, one ulp outside, NaN, inf
    gs, grgb = _cotangents(n)
    _hold(nets[14], pos, _good_dirs(n), gs, grgb, "T=14 n=%d" % n)


@pytest.mark.parametrize("log2_T", [19, 14])
def test_three_blocks_hostile_positions_and_two_runs(nets, log2_T):
    n = 600
    pos, oob = _points(n)
    assert oob.sum() == 5
    gs, grgb = _cotangents(n)
    net = nets[log2_T]
    got, g64 = _hold(net, pos, _good_dirs(n), gs, grgb, "T=%d n=600" % log2_T)
    assert not got[oob].any() and not g64[oob].any() and got[~oob].any(axis=1).all()
    assert _same_bits(got, _device(net, pos, _good_dirs(n), gs, grgb))            # no atomics: equal inputs, equal bits


def test_colliding_corners_of_one_hashed_cell(nets):
    net = nets[14]
    L = net.L
    cand = np.random.default_rng(77).uniform(-0.9, 0.9, size=(4000, 3)).astype(np.float32)
    _, idx, _ = B.corners(L, cand, 1.0)
    hashed = np.nonzero(L["hashed"])[0]
    dup = np.array([[len(np.unique(idx[i, l])) < 8 for l in hashed] for i in range(len(cand))])
    rows = np.nonzero(dup.any(axis=1))[0]
    assert len(rows) > 0, "no candidate with two corners of one hashed cell in the same entry"
    pos = cand[rows[:4]]
    gs, grgb = _cotangents(len(pos), 3)
    _hold(net, pos, _good_dirs(len(pos)), gs, grgb, "T=14 collisions")


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
    _hold(net, pos, _good_dirs(n), gs, grgb, "T=14 |h16[0]| up to 40")


def test_null_grad_sigma_zero_grad_rgb_and_n_zero(nets):
    net = nets[14]
    n = 300
    pos, _ = _points(n)
    d = _good_dirs(n)
    gs, grgb = _cotangents(n)
    a, _ = _hold(net, pos, d, None, grgb, "T=14 NULL grad_sigma")
    assert _same_bits(a, _device(net, pos, d, np.zeros(n, np.float32), grgb))
    z = _device(net, pos, d, None, np.zeros((n, 3), np.float32))
    assert z.shape == (n, 3) and not z.any()                                      # nothing to carry: exactly zero
    _hold(net, pos, d, gs, np.zeros((n, 3), np.float32), "T=14 grad_rgb = 0")     # the sigma path alone
    e = torch.empty((0, 3), device="cuda")
    assert tuple(net.field.backward_pos(e, e, None, e).shape) == (0, 3)


def test_relu_at_exactly_zero(S0):
    def edit(p):
        p[3][5, :] = 0.0                                                          # colour layer 0, neuron 5: pre-activation exactly 0 at every point
        p[4][7, :] = 0.0                                                          # colour layer 1, neuron 7
        p[1][9, :] = 0.0                                                          # sigma_net's hidden neuron 9
    net = Net(S0, 14, 102, edit)
    n = 257
    pos, _ = _points(n)
    gs, grgb = _cotangents(n)
    got, _ = _hold(net, pos, _good_dirs(n), gs, grgb, "T=14 zeroed rows")
    # nothing passes those neurons: the weights that read them cannot matter, bit for bit
    def edit2(p):
        edit(p)
        p[4][:, 5] = 3.0; p[5][:, 7] = -2.0; p[2][:, 9] = 5.0
    assert _same_bits(got, _device(Net(S0, 14, 102, edit2), pos, _good_dirs(n), gs, grgb))


def test_rgb_train(S0):
    net = Net(S0, 14, 102)
    f = net.field
    n = 300
    pos, oob = _points(n)
    dn = _good_dirs(n)
    _, grgb = _cotangents(n)
    d = torch.from_numpy(dn).cuda()
    g = torch.from_numpy(grgb).cuda()
    params = f.parameters()
    f.bwd_max_blocks = 2
    want_rgb = f.rgb(torch.from_numpy(pos).cuda(), d).cpu().numpy()
    direct = [t.cpu().numpy() for t in f.backward_points(torch.from_numpy(pos).cuda(), d, None, g, max_blocks=2)]
    direct_pos = _device(net, pos, dn, None, grgb)
    for pos_grad in (True, False):
        for p in params:
            p.grad = None
        x = torch.from_numpy(pos).cuda().requires_grad_(True)
        rgb = f.rgb_train(x, d, pos_grad=pos_grad)
        assert rgb.requires_grad and _same_bits(rgb.detach().cpu().numpy(), want_rgb)
        (rgb * g).sum().backward()
        for k, p in enumerate(params):
            assert p.grad is not None and p.grad.shape == p.shape
            if k:                                                                 # the table is scattered with atomics
                assert _same_bits(p.grad.cpu().numpy(), direct[k]), B.NAMES[k]
        if pos_grad:
            assert x.grad is not None and _same_bits(x.grad.cpu().numpy(), direct_pos) and not x.grad[torch.from_numpy(oob).cuda()].any()
        else:
            assert x.grad is None
    # pos_grad without a position that asks for a gradient: none is computed; frozen parameters: the position's alone
    x = torch.from_numpy(pos).cuda()
    assert f.rgb_train(x, d, pos_grad=True).requires_grad and x.grad is None
    for p in params:
        p.requires_grad_(False)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    (f.rgb_train(x, d, pos_grad=True) * g).sum().backward()
    assert _same_bits(x.grad.cpu().numpy(), direct_pos)
