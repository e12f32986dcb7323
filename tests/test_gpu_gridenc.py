"""The stand-alone encoders on the device (csrc/gridenc.hip through encoding.GridEncoder / SHEncoder): the forward and the input gradient bit for bit against the
numpy float32 restatement (tests/gridenc_refs.py), the reference's configuration bit for bit against the fused path (stage0.DensityField.encode), the table gradient
and the input gradient against the float64 polynomials within the Higham bounds gridenc_refs derives (table: gamma_(m + D + 2) * sum |terms| per entry; input:
gamma_(D + 2^(D-1) + L C + 5) * sum |terms| per axis), max_level, and the modules under autograd, load_state_dict, autocast and the regulariser.

The shapes are the smallest at which the kernels can go wrong: n = 1, 63, 65, 257 (a wave and a block and their neighbours), 1, 3 and 16 levels, base resolution 2
with 2^4 .. 2^6 entries (a dense level, the dense-to-hashed transition and a tiled wrap within a few levels), D = 2 and 3, C = 1, 2, 4, 8, both align_corners,
both interpolations, hash and tiled.  A configuration's reference is computed once on 257 points; the shorter runs are held to its first rows.
No bound here is measured: every one is derived in gridenc_refs / radiance_bwd_refs and stays as it is whatever a device run shows.

Measured on the MI355X when these tests were written: all pass; no forward or input-gradient word differs from the restatement; the worst
table-gradient element sits at 0.50 of its allowance (D = 2, C = 8, tiled, smoothstep, n = 63), the worst input-gradient element at 0.23, a single term (the level
without collisions) at 0.38; the modules' table gradient at 0.50 of radiance_bwd_refs' allowance against float64 (E = E_ref) and at 0.33 / 0.67 against the fused
backward's grad_table."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_refs as D      # noqa: E402
import gridenc_refs as G      # noqa: E402
import radiance_bwd_refs as B  # noqa: E402

F32 = np.float32
NS = (1, 63, 65, 257)


@pytest.fixture(scope="module")
def E():
    from mirres_restir_nerf_mesh_amd import encoding
    return encoding


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == np.float32 and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Case:
    """One seeded table on the host (read-only), its layout by the restatement, and the GridEncoder over it on the device."""

    def __init__(self, E, D_, C_, nl, log2_T, gridtype="hash", align=False, interp="linear", seed=0, base=2, pls=2.0):
        self.D, self.C, self.nl = D_, C_, nl
        self.L = G.layout(D=D_, C=C_, num_levels=nl, pls=pls, base=base, log2_T=log2_T, gridtype=gridtype, align=align, interp=interp)
        rng = np.random.default_rng(seed)
        self.table = rng.normal(size=(self.L["total"], C_)).astype(F32)
        self.table.setflags(write=False)
        self.enc = E.GridEncoder(input_dim=D_, num_levels=nl, level_dim=C_, per_level_scale=pls, base_resolution=base, log2_hashmap_size=log2_T, gridtype=gridtype,
                                 align_corners=align, interpolation=interp)
        assert self.enc.offsets.tolist() == self.L["offsets"].tolist()
        self.enc.load_state_dict({"embeddings": torch.tensor(self.table), "offsets": self.enc.offsets})
        self.enc.cuda()

    def fwd(self, pos, bound, max_level=None):
        with torch.no_grad():
            out = self.enc(torch.from_numpy(np.ascontiguousarray(pos, F32)).cuda(), bound=bound, max_level=max_level)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def bwd(self, pos, bound, go, max_level=None, want_pos=True):
        """-> (grad of the table, grad of the positions or None) through autograd."""
        self.enc.embeddings.grad = None
        x = torch.from_numpy(np.ascontiguousarray(pos, F32)).cuda().requires_grad_(want_pos)
        out = self.enc(x, bound=bound, max_level=max_level)
        out.backward(torch.from_numpy(np.ascontiguousarray(go, F32)).cuda())
        torch.cuda.synchronize()
        gt = self.enc.embeddings.grad.cpu().numpy()
        self.enc.embeddings.grad = None
        return gt, (x.grad.cpu().numpy() if want_pos else None)


def _hostile(L, bound, n, seed):
    """Hostile points first, random ones after: exactly -bound and +bound, points on the cell faces of level 1 (level 0 where there is one level: u * scale + half an
    integer; the first and the last face inside the box), nextafter outside the box on every axis and side, NaN, +inf, -inf, -0.0.  Which of them are in bounds is
    the restatement's decision (u in fp32)."""
    Dn = L["D"]; b = F32(bound); half = F32(0.0 if L["align"] else 0.5); s0 = F32(L["scale"][min(1, L["num_levels"] - 1)])
    face = lambda k: F32(F32(F32(k) - half) / s0 * F32(2.0) - F32(1.0)) * b
    k2 = max(1, int(s0))
    base = [0.3, -0.2, 0.7][:Dn]
    sp = [[-b] * Dn, [b] * Dn, [b, -b, F32(0.25)][:Dn], [face(1), face(k2), face(1)][:Dn], [face(1), 0.1, face(k2)][:Dn], [-0.0] * Dn, [0.0, -0.0, 0.0][:Dn]]
    for d in range(Dn):
        for side in (1, -1):
            p = list(base); p[d] = np.nextafter(F32(side) * b, F32(side) * F32(np.inf)); sp.append(p)
    for bad in (np.nan, np.inf, -np.inf):
        p = list(base); p[Dn - 1] = bad; sp.append(p)
    sp = np.array(sp, F32)
    rnd = np.random.default_rng(seed).uniform(-bound, bound, size=(max(n, 1), Dn)).astype(F32)
    return np.concatenate([sp, rnd])[:n]


CONFIGS = list(itertools.product((1, 3, 16), (4, 5, 6), ("hash", "tiled"), (False, True), ("linear", "smoothstep")))


@pytest.mark.parametrize("D_,C_", [(d, c) for d in (2, 3) for c in (1, 2, 4, 8)])
def test_forward_bits_equal_the_float32_restatement_over_the_sweep(E, D_, C_):
    bad = []
    for k, (nl, log2_T, gridtype, align, interp) in enumerate(CONFIGS):
        case = Case(E, D_, C_, nl, log2_T, gridtype, align, interp, seed=k)
        bound = (1.0, 1.5, 2.0)[k % 3]                               # 1.5: the division by 2 * bound is no multiplication by a power of two
        pos = np.random.default_rng(1000 + k).uniform(-bound, bound, size=(257, D_)).astype(F32)
        want = G.encode32(case.table, case.L, pos, bound)
        assert np.abs(want).max() > 0
        for n in NS:
            got = case.fwd(pos[:n], bound)
            assert got.shape == (n, nl * C_) and got.dtype == np.float32
            if not _bits(got, want[:n]):
                diff = got.view(np.uint32) != want[:n].view(np.uint32)
                bad.append((nl, log2_T, gridtype, align, interp, n, int(diff.sum()), sorted(set((np.nonzero(diff)[1] // C_).tolist()))))
    print("D=%d C=%d: %d configurations x %s points, %d with differing words" % (D_, C_, len(CONFIGS), NS, len(bad)))
    assert not bad, bad[:8]


@pytest.mark.parametrize("bound", [1.0, 2.0, 1.5])
def test_reference_configuration_has_the_fused_paths_bits(E, S0, bound):
    ck = S0.synthetic_radiance_checkpoint()["model"]
    rng = np.random.default_rng(7)
    table = ck["encoder.embeddings"].clone()
    table += torch.from_numpy(rng.normal(size=tuple(table.shape)).astype(F32) * 0.1)       # the synthetic table is zero outside level 0: give every level something
    # the same table under every bound: both sides are told desired_resolution = 2048, so the layout is the checkpoint's and `bound` only maps the points
    field = S0.DensityField(table, ck["sigma_net.0.weight"], ck["sigma_net.1.weight"], bound=bound, desired_resolution=2048)
    enc, dim = E.get_encoder("hashgrid", desired_resolution=2048)
    enc.load_state_dict({"embeddings": table, "offsets": ck["encoder.offsets"]})
    enc.cuda()
    Lg = G.layout(pls=G.per_level_scale(2048.0, 16, 16))
    pos = _hostile(Lg, bound, 257, 3)
    x = torch.from_numpy(pos).cuda()
    want = field.encode(x).cpu().numpy()
    for n in NS:
        with torch.no_grad():
            got = enc(x[:n], bound=bound).cpu().numpy()
        assert dim == 32 and _bits(got, want[:n]), (n, int((got.view(np.uint32) != want[:n].view(np.uint32)).sum()))
    assert np.abs(want).max() > 0 and (want[np.isnan(pos).any(axis=1)] == 0).all()
    # the input gradient: no atomics, two runs give the same bits; and the restatement's
    go = rng.normal(size=(257, 32)).astype(F32)
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        enc(xg, bound=bound).backward(torch.from_numpy(go).cuda())
        runs.append(xg.grad.cpu().numpy())
    assert _bits(runs[0], runs[1]) and np.abs(runs[0]).max() > 0
    assert _bits(runs[0], G.input_grad32(table.numpy(), Lg, pos, bound, go))


@pytest.mark.parametrize("D_,C_,gridtype,align,interp", [(3, 2, "hash", False, "linear"), (2, 4, "tiled", True, "smoothstep"), (3, 8, "hash", True, "smoothstep"),
                                                         (2, 1, "hash", False, "linear")])
def test_hostile_points_against_the_restatement(E, D_, C_, gridtype, align, interp):
    case = Case(E, D_, C_, 3, 5, gridtype, align, interp, seed=11)
    for bound in (1.0, 1.5):
        pos = _hostile(case.L, bound, 65, 4)
        _, ok = G.unit32(case.L, pos, bound)
        assert ok[:7].all() and (~ok).sum() >= 3 + D_ and ok.sum() > 40          # the corners, the faces and -0.0 are inside; NaN, +-inf and below -bound are not
        got = case.fwd(pos, bound)
        want = G.encode32(case.table, case.L, pos, bound)
        assert _bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert (got[~ok] == 0).all() and (np.abs(got[ok]).max(axis=1) > 0).all()
        go = np.random.default_rng(5).normal(size=got.shape).astype(F32)
        gt, gp = case.bwd(pos, bound, go)
        assert _bits(gp, G.input_grad32(case.table, case.L, pos, bound, go)) and (gp[~ok] == 0).all() and not np.signbit(gp[~ok]).any()
        # an out-of-bounds point scatters nothing: alone, the table's gradient stays exactly 0
        only, only_p = case.bwd(pos[~ok], bound, go[~ok])
        assert not only.any() and not only_p.any()


def _hold_table(case, pos, bound, go, label, max_level=None):
    """The table gradient against the float64 scatter, every entry and channel: |g - g64| <= gamma_(m + D + 2) * sum |terms|; prints the worst ratio before it asserts."""
    gt, _ = case.bwd(pos, bound, go, max_level, want_pos=False)
    g64, tsum, m = G.grads64(case.table, case.L, pos, bound, go, max_level)["table"]
    allow = G.gamma(G.table_k(m, case.D)) * tsum
    err = np.abs(gt.astype(np.float64) - g64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / allow)
    print("%s: worst error / allowance %.3f, largest m %d, %d entries touched of %d" % (label, float(ratio.max()), int(m.max()), int((m[:, 0] > 0).sum()), len(m)))
    assert gt.dtype == np.float32 and np.abs(g64).max() > 0
    assert (err <= allow).all(), (label, float(ratio.max()))
    return gt, m


@pytest.mark.parametrize("D_,C_,nl,log2_T,gridtype,align,interp", [(3, 2, 16, 6, "hash", False, "linear"), (2, 1, 3, 4, "hash", True, "linear"),
                                                                   (3, 4, 3, 5, "tiled", False, "smoothstep"), (2, 8, 16, 6, "tiled", True, "smoothstep"),
                                                                   (3, 8, 1, 4, "hash", False, "smoothstep"), (2, 2, 16, 5, "hash", False, "linear"),
                                                                   (3, 1, 16, 4, "tiled", True, "linear"), (2, 4, 3, 6, "hash", False, "smoothstep")])
def test_table_gradient_against_the_float64_scatter(E, D_, C_, nl, log2_T, gridtype, align, interp):
    case = Case(E, D_, C_, nl, log2_T, gridtype, align, interp, seed=21)
    pos = _hostile(case.L, 1.5, 257, 6)
    go = np.random.default_rng(8).normal(size=(257, nl * C_)).astype(F32)
    for n in NS:
        _hold_table(case, pos[:n], 1.5, go[:n], "D=%d C=%d L=%d T=%d %s align=%s %s n=%d" % (D_, C_, nl, log2_T, gridtype, align, interp, n))


@pytest.mark.parametrize("D_,C_", [(3, 2), (2, 8), (3, 1)])
def test_table_gradient_under_full_contention_and_without_collisions(E, D_, C_):
    # 4096 identical points: every level's 2^D entries take 4096 terms each (more where corners collide)
    case = Case(E, D_, C_, 3, 5, "hash", False, "linear", seed=31)
    p = np.array([[0.123, -0.456, 0.789][:D_]], F32)
    pos = np.repeat(p, 4096, axis=0)
    go = np.random.default_rng(9).normal(size=(4096, 3 * C_)).astype(F32)
    _, m = _hold_table(case, pos, 1.0, go, "D=%d C=%d 4096 points in one cell" % (D_, C_))
    assert m.max() >= 4096 and (m[m > 0] % 4096 == 0).all()
    # one dense level of 65^D vertices, one point per cell and the cells two apart: every touched entry takes exactly one term, the bound is that of one product
    case = Case(E, D_, C_, 1, 19, "hash", False, "linear", seed=32, base=64)
    assert not case.L["hashed"][0] and case.L["scale"][0] == 63.0
    cells = np.stack(np.meshgrid(*([np.arange(1, 60, 3)] * D_), indexing="ij"), -1).reshape(-1, D_)[:300]
    u = (cells + np.random.default_rng(3).uniform(0.1, 0.9, size=cells.shape) - 0.5) / 63.0
    pos = (u * 2.0 - 1.0).astype(F32)
    go = np.random.default_rng(10).normal(size=(len(pos), C_)).astype(F32)
    _, m = _hold_table(case, pos, 1.0, go, "D=%d C=%d one dense level without collisions" % (D_, C_))
    assert m.max() == 1 and (m > 0).sum() == len(pos) * (1 << D_) * C_


@pytest.mark.parametrize("D_,C_,nl,log2_T,gridtype,align,interp", [(3, 2, 16, 6, "hash", False, "linear"), (2, 4, 3, 4, "tiled", True, "smoothstep"),
                                                                   (3, 8, 3, 5, "hash", False, "smoothstep"), (2, 1, 16, 5, "hash", True, "linear"),
                                                                   (3, 1, 1, 4, "tiled", False, "linear"), (2, 8, 16, 6, "tiled", False, "smoothstep"),
                                                                   (3, 4, 16, 4, "hash", True, "smoothstep"), (2, 2, 3, 6, "hash", False, "linear")])
def test_input_gradient_bits_and_against_the_float64_derivative(E, D_, C_, nl, log2_T, gridtype, align, interp):
    case = Case(E, D_, C_, nl, log2_T, gridtype, align, interp, seed=41)
    pos = _hostile(case.L, 1.5, 257, 12)
    go = np.random.default_rng(13).normal(size=(257, nl * C_)).astype(F32)
    want32 = G.input_grad32(case.table, case.L, pos, 1.5, go)
    R = G.grads64(case.table, case.L, pos, 1.5, go)
    g64, psum = R["pos"]; ok = R["ok"]
    allow = G.gamma(G.pos_k(D_, nl, C_)) * psum
    for n in NS:
        _, gp = case.bwd(pos[:n], 1.5, go[:n])
        assert _bits(gp, want32[:n]), (n, int((gp.view(np.uint32) != want32[:n].view(np.uint32)).sum()))
        err = np.abs(gp.astype(np.float64) - g64[:n])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / allow[:n])
        print("D=%d C=%d L=%d n=%d: worst error / allowance %.3f" % (D_, C_, nl, n, float(ratio.max())))
        assert (err <= allow[:n]).all(), (n, float(ratio.max()))
        assert (gp[~ok[:n]] == 0).all()
    assert (~ok).sum() >= 3 and np.abs(g64).max() > 0


@pytest.mark.parametrize("D_,C_,nl", [(3, 2, 16), (2, 4, 3)])
def test_max_level(E, D_, C_, nl):
    case = Case(E, D_, C_, nl, 5, "hash", False, "linear", seed=51)
    pos = _hostile(case.L, 1.0, 65, 14)
    go = np.random.default_rng(15).normal(size=(65, nl * C_)).astype(F32)
    full = case.fwd(pos, 1.0)
    for ml in (0, 1, nl - 1, nl, nl + 3):
        run = min(ml, nl)
        got = case.fwd(pos, 1.0, ml)
        assert _bits(got, G.encode32(case.table, case.L, pos, 1.0, ml))
        assert _bits(got[:, :run * C_], full[:, :run * C_]) and (got[:, run * C_:] == 0).all()
        gt, gp = case.bwd(pos, 1.0, go, ml)
        assert not gt[int(case.L["offsets"][run]):].any()                                   # levels >= max_level carry no gradient
        assert _bits(gp, G.input_grad32(case.table, case.L, pos, 1.0, go, ml))
        if run > 0:
            _hold_table(case, pos, 1.0, go, "max_level %d of %d" % (ml, nl), ml)
        else:
            assert not gt.any() and not gp.any()
    assert _bits(case.fwd(pos, 1.0, None), full)


class _TorchNet(torch.nn.Module):
    """NeRFNetwork.forward (nerf/network.py:146-174) from the stand-alone encoders and bias-free nn.Linear layers."""

    def __init__(self, E, weights, **grid):
        super().__init__()
        self.encoder, _ = E.get_encoder("hashgrid", **grid)
        self.encoder_dir, _ = E.get_encoder("sh")
        lin = lambda w: torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
        self.sigma_net = torch.nn.ModuleList([lin(weights[0]), lin(weights[1])])
        self.color_net = torch.nn.ModuleList([lin(w) for w in weights[2:]])
        with torch.no_grad():
            for layer, w in zip(list(self.sigma_net) + list(self.color_net), weights):
                layer.weight.copy_(torch.as_tensor(w))

    def forward(self, x, d):
        h = self.sigma_net[1](torch.relu(self.sigma_net[0](self.encoder(x, bound=1.0))))
        sigma = B._TruncExp.apply(h[:, 0])
        c = torch.cat([self.encoder_dir(d), h[:, 1:]], dim=1)
        rgb = torch.sigmoid(self.color_net[2](torch.relu(self.color_net[1](torch.relu(self.color_net[0](c))))))
        return sigma, rgb


def _module_against_fused(E, S0, params, log2_T, label, literal):
    Ld = D.layout(1.0, log2_T=log2_T)
    rf = S0.RadianceField(*(torch.tensor(np.asarray(a)) for a in params), bound=1.0, log2_hashmap_size=log2_T)
    net = _TorchNet(E, params[1:], log2_hashmap_size=log2_T)
    net.encoder.load_state_dict({"embeddings": torch.tensor(np.asarray(params[0])), "offsets": torch.tensor(Ld["offsets"].tolist(), dtype=torch.int32)})
    net.cuda()
    n = 257
    pos = _hostile(G.layout(pls=G.per_level_scale(2048.0, 16, 16), log2_T=log2_T), 1.0, n, 16)
    rng = np.random.default_rng(17)
    dirs = rng.normal(size=(n, 3)).astype(F32)
    gs, grgb = rng.normal(size=n).astype(F32), rng.normal(size=(n, 3)).astype(F32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, d = cu(pos), cu(dirs)
    sigma, rgb = net(x, d)
    assert _bits(net.encoder(x).detach().cpu().numpy(), rf.encode(x).cpu().numpy())
    ((sigma * cu(gs)).sum() + (rgb * cu(grgb)).sum()).backward()
    torch.cuda.synchronize()
    got = net.encoder.embeddings.grad.cpu().numpy()
    fused = rf.backward_points(x, d, cu(gs), cu(grgb), max_blocks=4)[0].cpu().numpy()
    g64, terms = B.grads(params, Ld, pos, dirs, 1.0, gs, grgb, with_terms=True)
    g32 = B.grads(params, Ld, pos, dirs, 1.0, gs, grgb, dtype=torch.float32)
    w_mod = B.criterion("table", got, g64[0], g32[0], terms)
    w_fus = B.criterion("table", fused, g64[0], g32[0], terms)
    w_lit = B.criterion("table", got, fused.astype(np.float64), g32[0], terms)
    for name, w in (("module vs float64", w_mod), ("fused vs float64", w_fus), ("module vs fused", w_lit)):
        print("%s, %s: worst error / allowance %.3f, E %.3e, E_ref %.3e, largest floor %.3e" % ((label, name) + w))
    assert np.abs(g64[0]).max() > 0 and got.dtype == np.float32 and got.shape == fused.shape
    assert w_mod[0] <= 1.0 and w_fus[0] <= 1.0, (label, w_mod, w_fus)
    if literal:
        assert w_lit[0] <= 1.0, (label, w_lit)
    return net, x


def test_module_autograd_on_the_synthetic_checkpoint_against_the_fused_backward(E, S0):
    m = S0.synthetic_radiance_checkpoint()["model"]
    params = [m[k].numpy() for k in ("encoder.embeddings", "sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight", "color_net.2.weight")]
    net, x = _module_against_fused(E, S0, params, 19, "synthetic checkpoint", literal=True)
    enc = net.encoder
    # load_state_dict round trip: a second encoder built from the state dict gives the same bits
    enc2, _ = E.get_encoder("hashgrid")
    enc2.load_state_dict(enc.state_dict())
    enc2.cuda()
    with torch.no_grad():
        a, b2 = enc(x), enc2(x[:, None, :].expand(-1, 2, -1))                               # any prefix shape
        assert tuple(b2.shape) == (len(x), 2, 32) and _bits(a.cpu().numpy(), b2[:, 0].contiguous().cpu().numpy()) and torch.equal(b2[:, 0], b2[:, 1])
        # fp32 whatever the context: under autocast and for half inputs (from the half values) the output is fp32
        with torch.autocast("cuda", dtype=torch.float16):
            c = enc(x)
        assert c.dtype == torch.float32 and torch.equal(c, a)
        h = enc(x.half())
        assert h.dtype == torch.float32 and torch.equal(h, enc(x.half().float()))
    # inputs on another device than the table are refused, not moved (their gradient would come back on the wrong device)
    with pytest.raises(ValueError, match="move the inputs"):
        enc(x.cpu())
    # a forward and a backward read nothing back from the device: no synchronising call (the offsets buffer is checked when a state dict is loaded, not here)
    xs = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enc(xs, bound=1.0).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert xs.grad is not None and enc.embeddings.grad is not None
    enc.embeddings.grad = None
    # the regulariser goes through mirres_grid_tv_grad like DensityField's: the same bits on the same points (on this table every hashed level adds exact zeros and
    # level 0 is dense, so no atomic's order shows)
    field = S0.DensityField.from_checkpoint({"model": m})
    g0 = torch.from_numpy(np.random.default_rng(2).normal(size=tuple(enc.embeddings.shape)).astype(F32) * 1e-4).cuda()
    enc.embeddings.grad = g0.clone()
    want = g0.clone()
    assert enc.grad_total_variation(1e-3, x, 1.0) is None
    field.grad_total_variation(1e-3, x, grad=want)
    assert torch.equal(enc.embeddings.grad, want) and not torch.equal(want, g0)


def test_module_autograd_on_a_seeded_network_against_float64(E, S0):
    rng = np.random.default_rng(61)
    Ld = D.layout(1.0, log2_T=14)
    params = [rng.normal(size=(Ld["total"], 2)).astype(F32), (rng.normal(size=(64, 32)) * 0.15).astype(F32), (rng.normal(size=(16, 64)) * 0.15).astype(F32),
              (rng.normal(size=(64, 31)) * 0.15).astype(F32), (rng.normal(size=(64, 64)) * 0.15).astype(F32), (rng.normal(size=(3, 64)) * 0.5).astype(F32)]
    _module_against_fused(E, S0, params, 14, "seeded T=14", literal=False)


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_encoder_has_the_radiance_fields_bits(E, S0, degree):
    rng = np.random.default_rng(degree)
    d = rng.normal(size=(257, 3)).astype(F32)
    d[:3] = [[0, 0, 2], [1e-20, 0, 0], [-3, 4, 0]]
    rf = S0.RadianceField.from_checkpoint(S0.synthetic_radiance_checkpoint())
    x = torch.from_numpy(d).cuda()
    want = rf.sh(x).cpu().numpy()
    enc, dim = E.get_encoder("sh", degree=degree)
    got = enc(x)
    assert dim == degree * degree and got.dtype == torch.float32 and _bits(got.cpu().numpy(), want[:, :dim])
    assert tuple(enc(x.reshape(257, 1, 3)).shape) == (257, 1, dim)
