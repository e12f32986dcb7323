"""CPU, no GPU calls: what the stage-1 NeRF colour branch rests on apart from the kernel.  The float64 restatement of the radiance network with the position as a
leaf (tests/radiance_pos_refs.py) against central differences of the float64 network on a T = 14 layout (dense and hashed levels), out-of-bounds points, a ReLU at
exactly 0, a point on a cell face; the criterion's floor; mirres_radiance_points_bwd_pos's refusals before a device is touched; losses.stage1_loss's mask term."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_refs as D                       # noqa: E402
import radiance_bwd_refs as B                  # noqa: E402
import radiance_pos_refs as P                  # noqa: E402


def _net(seed=7, log2_T=14, table_gain=0.02):
    L = D.layout(1.0, log2_T=log2_T)
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.normal(size=s)
    return L, [g(L["total"], 2) * table_gain, g(64, 32) * 0.15, g(16, 64) * 0.15, g(64, 31) * 0.15, g(64, 64) * 0.15, g(3, 64) * 0.5]


def _interior_points(L, n, seed=3, margin=0.02):
    """n points whose fraction lies in (margin, 1 - margin) on every axis of every level."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cand = rng.uniform(-0.95, 0.95, size=(64, 3)).astype(np.float32)
        u = (cand.astype(np.float64) + 1.0) / 2.0
        f = u[:, None, :] * np.asarray(L["scale"], np.float64)[None, :, None] + 0.5
        f = f - np.floor(f)
        out.extend(cand[((f > margin) & (f < 1 - margin)).all(axis=(1, 2))])
    return np.array(out[:n], np.float32)


def _cot(n, seed=5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=(n, 3)).astype(np.float32)


def _signs(net):
    return [np.sign(net[k].detach().numpy()) for k in ("z1", "z2", "z3")]


def test_float64_position_gradient_against_central_differences():
    L, params = _net()
    assert L["hashed"].any() and not L["hashed"].all()                           # dense and hashed levels
    n = 12
    pos = _interior_points(L, n)
    gs, grgb, dirs = _cot(n)
    g = P.grad_pos(params, L, pos, dirs, 1.0, gs, grgb)
    assert g.shape == (n, 3) and np.abs(g).max() > 0
    # the float64 network that is differenced is radiance_bwd_refs' own (its weights are constants of the position inside a cell)
    def f(p):
        net = B.network(params, L, p, dirs, 1.0)
        return float(((torch.tensor(gs) * net["sigma"]).sum() + (torch.tensor(grgb) * net["rgb"]).sum()).detach()), _signs(net)
    h = 2.0 ** -20                                                                # ~1e-6, exact in fp32 at these magnitudes: the points stay fp32 values
    _, s0 = f(pos)
    checked = 0
    for i in range(n):
        for a in range(3):
            up = pos.copy(); up[i, a] += np.float32(h)
            dn = pos.copy(); dn[i, a] -= np.float32(h)
            step = float(up[i, a]) - float(dn[i, a])
            (lu, su), (ld, sd) = f(up), f(dn)
            if not all((x == y).all() and (x == z).all() for x, y, z in zip(s0, su, sd)):
                continue                                                          # a ReLU changed sides inside the step: no derivative to compare with
            fd = (lu - ld) / step
            # the rule of test_radiance_bwd_host.py: h^2 f''' / 6 plus rounding 2 ulp(loss) / h, inside 1e-6 of the tensor's scale
            assert abs(fd - g[i, a]) <= 1e-6 * max(1.0, np.abs(g).max()), (i, a, fd, g[i, a])
            checked += 1
    assert checked >= 30
    # NULL grad_sigma is zeros
    g0 = P.grad_pos(params, L, pos, dirs, 1.0, None, grgb)
    assert np.array_equal(g0, P.grad_pos(params, L, pos, dirs, 1.0, np.zeros(n), grgb)) and not np.array_equal(g0, g)


def test_out_of_bounds_points_and_cell_faces():
    L, params = _net()
    b = np.float32(1.0)
    pos = _interior_points(L, 6, seed=9)
    pos[1, 0] = np.nextafter(b, np.float32(2.0))                                  # rounds to u = 1: inside by the fp32 rule
    pos[2, 1] = np.float32(1.5); pos[3, 2] = np.nan; pos[4, 0] = -np.inf
    pos[5] = np.float32(-1.0)                                                     # the corner: on a face of every level
    gs, grgb, dirs = _cot(6)
    g64, terms = P.grad_pos(params, L, pos, dirs, 1.0, gs, grgb, with_terms=True)
    ok = P.cells(L, pos, 1.0)[0]
    assert list(ok) == [True, True, False, False, False, True]
    assert not g64[~ok].any() and np.abs(g64[ok]).min() > 0 and np.isfinite(g64).all()
    tsum, m = terms["pos"]
    assert (m[ok] == 128).all() and (m[~ok] == 0).all() and not tsum[~ok].any() and (np.abs(g64) <= tsum * (1 + 1e-12)).all()
    # at the corner the cell the fp32 rule picks has f = 0.5 at every level (u * scale + 0.5 - 0): the gradient is that cell's, not a neighbour's
    net = P.network(params, L, pos, dirs, 1.0)
    assert (net["f"].detach().numpy()[5] == 0.5).all() and not net["cell"][5].any()
    # the fp32 restatement is the criterion's yardstick: against itself it sits at half its allowance
    g32 = P.grad_pos(params, L, pos, dirs, 1.0, gs, grgb, dtype=torch.float32)
    assert g32.dtype == np.float32 and not g32[~ok].any()
    worst, e, e_ref, floor = P.criterion(g32, g64, g32, terms)
    assert worst <= 0.5 + 1e-12 and e == e_ref and 0 < e_ref < 1e-3 and floor > 0      # f = u scale + 0.5 - cell cancels: ulp(2047) in fp32
    assert P.criterion(g64 + 3.0 * np.abs(g64).max() * max(e_ref, floor), g64, g32, terms)[0] > 1.0
    zero = np.zeros_like(g64)
    assert P.criterion(zero, zero, zero, terms)[0] == 0.0 and P.criterion(zero + 1e-30, zero, zero, terms)[0] == np.inf


def test_relu_at_exactly_zero_passes_nothing():
    L, params = _net()
    pos = _interior_points(L, 8, seed=4)
    gs, grgb, dirs = _cot(8)
    rng = np.random.default_rng(1)
    # a zeroed row gives a pre-activation of exactly 0: nothing passes, so the weights that read that neuron do not reach the position
    base = P.network(params, L, pos, dirs, 1.0)
    for row_of, col_of, z in ((3, 4, "z2"), (1, 2, "z1"), (4, 5, "z3")):          # colour layer 0 -> c1's column, sigma_net's hidden layer -> w1's, colour layer 1 -> c2's
        k = int(np.argmax((base[z].detach().numpy() > 0).sum(axis=0)))            # a neuron that passes at some point as the weights stand
        p = [a.copy() for a in params]
        p[row_of][k, :] = 0.0
        g = P.grad_pos(p, L, pos, dirs, 1.0, gs, grgb)
        q = [a.copy() for a in p]
        q[col_of][:, k] = rng.normal(size=q[col_of].shape[0])
        assert np.array_equal(g, P.grad_pos(q, L, pos, dirs, 1.0, gs, grgb)) and np.abs(g).max() > 0
        assert not np.array_equal(g, P.grad_pos(params, L, pos, dirs, 1.0, gs, grgb))


def test_pos_entry_refuses_bad_arguments_before_touching_a_device():
    """Every call must fail an argument check (MIRRES_E_ARG exactly, not a device error) or have nothing to do: the pointers are not device memory."""
    from mirres_restir_nerf_mesh_amd import _lib as L, stage0 as S0
    lib = L.lib()
    E_ARG = -1
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    net = L.RadianceNet()
    dn, _ = S0.density_layout(1.0)
    net.grid = dn

    def call(net_=net, pos=p, dirs=p, n=4, bound=1.0, gs=p, grgb=p, out=p):
        return lib.mirres_radiance_points_bwd_pos(C.byref(net_) if net_ is not None else None, pos, dirs, n, bound, gs, grgb, out, None)
    assert call(net_=None) == E_ARG and b"mirres_radiance_points_bwd_pos" in lib.mirres_last_error()
    assert call() == E_ARG and b"NULL table" in lib.mirres_last_error()
    net.grid.table = net.grid.w0 = net.grid.w1 = p
    assert call() == E_ARG and b"w1 / c0 / c1 / c2" in lib.mirres_last_error()
    net.w1 = net.c0 = net.c1 = net.c2 = p
    for kw in (dict(n=-1), dict(n=(1 << 38) + 1), dict(bound=0.0), dict(bound=-1.0), dict(bound=float("nan")), dict(bound=float("inf")), dict(pos=None), dict(dirs=None),
               dict(grgb=None), dict(out=None)):
        assert call(**kw) == E_ARG and b"bad argument" in lib.mirres_last_error(), kw
    assert call(n=0, pos=None, dirs=None, gs=None, grgb=None, out=None) == 0      # nothing to do, no launch
    assert not any(host)


def _outputs(n=48, seed=2, image=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g)
    out = dict(image_brdf=r(n, 3), diffuse_light=r(n, 3), specular_light=r(n, 3), img_brdf_indirect=r(n, 3) * 0.1, kd_grad=r(n, 3), ks_grad=r(n, 3),
               normal_grad=r(n, 3), weights_sum=r(n))
    if image:
        out["image"] = r(n, 3)
    return out, r(n, 3), r(n, 3), r(n, 1)


@pytest.mark.parametrize("image", [True, False])
def test_stage1_loss_mask_term(image):
    from mirres_restir_nerf_mesh_amd import losses
    out, gt, gt_lin, mask = _outputs(image=image)
    opt = types.SimpleNamespace()
    base = losses.stage1_loss(out, gt, gt_lin, opt)
    # gt_mask = None: the bits of a call without the argument, with and without weights_sum in the dict
    assert torch.equal(base, losses.stage1_loss(out, gt, gt_lin, opt, gt_mask=None))
    assert torch.equal(base, losses.stage1_loss({k: v for k, v in out.items() if k != "weights_sum"}, gt, gt_lin, opt))
    # the formula by hand (nerf/utils.py:1003-1021): the per-pixel terms are added before the mean
    pix = 0.02 * (out["image_brdf"] - gt).abs().mean(-1)
    if image:
        pix = 1.0 * ((out["image"] - gt) ** 2).mean(-1) + pix
    for lam, o in ((0.1, opt), (0.7, types.SimpleNamespace(lambda_mask=0.7))):
        want = (pix + lam * (out["weights_sum"] - mask[:, 0]) ** 2).mean() + (losses.stage1_loss(out, gt, gt_lin, o) - pix.mean())
        for m in (mask, mask[:, 0]):                                              # [H W, 1] and [H W]
            got = losses.stage1_loss(out, gt, gt_lin, o, gt_mask=m)
            assert got.shape == () and abs(float(got) - float(want)) <= 4 * 2.0 ** -24 * abs(float(want)) and float(got) > float(base)
    # lambda_mask = 0 switches the term off (utils.py:1014); a mask without weights_sum is an error
    assert torch.equal(base, losses.stage1_loss(out, gt, gt_lin, types.SimpleNamespace(lambda_mask=0.0), gt_mask=mask))
    with pytest.raises(ValueError, match="weights_sum"):
        losses.stage1_loss({k: v for k, v in out.items() if k != "weights_sum"}, gt, gt_lin, opt, gt_mask=mask)
    # without use_brdf the image alone carries the loss; with neither there is nothing to optimise
    if image:
        only = losses.stage1_loss(out, gt, gt_lin, types.SimpleNamespace(use_brdf=False), gt_mask=mask)
        assert abs(float(only) - float((((out["image"] - gt) ** 2).mean(-1) + 0.1 * (out["weights_sum"] - mask[:, 0]) ** 2).mean())) < 1e-6
    else:
        with pytest.raises(ValueError, match="neither"):
            losses.stage1_loss(out, gt, gt_lin, types.SimpleNamespace(use_brdf=False), gt_mask=mask)
