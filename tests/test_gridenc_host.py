"""CPU: the host side of the stand-alone encoders (encoding.py, csrc/gridenc.hip's entries before a launch) — GridEncoder's level table against the independent
restatement tests/gridenc_refs.py over a sweep of configurations and, for the reference's configuration, against stage0.density_layout; the restatement itself
against tests/density_refs.py (bits), against its float64 form (derived bound), against finite differences and against its own float32 gradient (derived bound);
the C ABI's refusals without a device; what the modules refuse; the state_dict."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_refs as D      # noqa: E402
import gridenc_refs as G      # noqa: E402

# base 2 with 2^4 .. 2^6 entries: within a few levels a dense level, the dense-to-hashed transition and a tiled wrap all occur
SWEEP = [dict(D=d, C=c, num_levels=nl, base=2, log2_T=t, pls=p, gridtype=gt, align=al)
         for d, c, nl, t, p, gt, al in itertools.product((2, 3), (1, 2, 4, 8), (1, 3, 16), (4, 6), (2.0, 1.3819), ("hash", "tiled"), (False, True))]


def _encoder(cfg, interp="linear"):
    from mirres_restir_nerf_mesh_amd import encoding
    return encoding.GridEncoder(input_dim=cfg["D"], num_levels=cfg["num_levels"], level_dim=cfg["C"], per_level_scale=cfg["pls"], base_resolution=cfg["base"],
                                log2_hashmap_size=cfg["log2_T"], gridtype=cfg["gridtype"], align_corners=cfg["align"], interpolation=interp)


def _same_layout(lay, L):
    nl = L["num_levels"]
    assert lay.num_levels == nl and lay.input_dim == L["D"] and lay.level_dim == L["C"]
    assert [lay.offsets[i] for i in range(nl + 1)] == L["offsets"].tolist()
    assert [lay.resolution[i] for i in range(nl)] == L["resolution"].tolist()
    assert [bool(lay.hashed[i]) for i in range(nl)] == L["hashed"].tolist()
    assert np.array_equal(np.array([lay.scale[i] for i in range(nl)], np.float32).view(np.uint32), L["scale"].view(np.uint32))


def test_layout_matches_the_formula_over_a_sweep():
    seen = set()
    for cfg in SWEEP:
        L = G.layout(**cfg)
        enc = _encoder(cfg)
        assert enc.offsets.dtype == torch.int32 and enc.offsets.tolist() == L["offsets"].tolist(), cfg
        _same_layout(enc._layout, L)
        assert tuple(enc.embeddings.shape) == (L["total"], cfg["C"]) and enc.n_params == L["total"] * cfg["C"] and enc.output_dim == cfg["num_levels"] * cfg["C"]
        assert 0 < float(enc.embeddings.detach().abs().max()) <= 1e-4
        # what the sweep is for: dense levels, hashed levels, and tiled levels whose index wraps (the stride loop stopped early)
        for l in range(cfg["num_levels"]):
            short = any(s == 0 for s in L["strides"][l])
            seen.add(("hashed" if L["hashed"][l] else ("tiled-wrap" if short else "dense"), cfg["D"]))
    assert seen == {(k, d) for k in ("hashed", "tiled-wrap", "dense") for d in (2, 3)}, seen


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_reference_configuration_fills_density_layouts_numbers(bound):
    from mirres_restir_nerf_mesh_amd import stage0, encoding
    net, total = stage0.density_layout(bound)
    enc, dim = encoding.get_encoder("hashgrid", desired_resolution=2048 * bound)
    assert dim == 32 and enc.offsets.tolist() == [net.offsets[i] for i in range(17)] and tuple(enc.embeddings.shape) == (total, 2)
    lay = enc._layout
    assert [lay.resolution[i] for i in range(16)] == [net.resolution[i] for i in range(16)] and [lay.hashed[i] for i in range(16)] == [net.hashed[i] for i in range(16)]
    assert [np.float32(lay.scale[i]).view(np.uint32) for i in range(16)] == [np.float32(net.scale[i]).view(np.uint32) for i in range(16)]
    L = G.layout(pls=G.per_level_scale(2048 * bound, 16, 16))
    _same_layout(lay, L)
    assert enc.per_level_scale == G.per_level_scale(2048 * bound, 16, 16) and enc.max_params == 2 ** 19
    for k in ("input_dim", "num_levels", "level_dim", "per_level_scale", "output_dim", "n_params", "max_params", "gridtype", "interpolation", "align_corners"):
        assert hasattr(enc, k), k


@pytest.mark.parametrize("log2_T", [19, 14])
@pytest.mark.parametrize("bound", [1.0, 1.5])
def test_restatement_has_density_refs_bits_for_the_reference_configuration(log2_T, bound):
    Ld = D.layout(bound, log2_T=log2_T)
    Lg = G.layout(pls=G.per_level_scale(2048.0 * bound, 16, 16), log2_T=log2_T)
    assert Lg["offsets"].tolist() == Ld["offsets"].tolist() and Lg["hashed"].tolist() == Ld["hashed"].tolist()
    rng = np.random.default_rng(log2_T)
    table = rng.normal(size=(Ld["total"], 2)).astype(np.float32)
    pos = rng.uniform(-bound, bound, size=(700, 3)).astype(np.float32)
    pos[:6] = [[-bound] * 3, [bound] * 3, [np.nan, 0, 0], [0, np.inf, 0], [-0.0, 0.0, -0.0], [np.nextafter(np.float32(-bound), np.float32(-9)), 0, 0]]
    want = D.encode32(table, Ld, pos, bound)
    got = G.encode32(table, Lg, pos, bound)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[[2, 3, 5]] == 0).all() and np.abs(got[:2]).max() > 0


def _case(cfg, interp, n, seed, bound=1.0):
    L = G.layout(interp=interp, **cfg)
    rng = np.random.default_rng(seed)
    table = rng.normal(size=(L["total"], cfg["C"])).astype(np.float32)
    pos = rng.uniform(-bound, bound, size=(n, cfg["D"])).astype(np.float32)
    return L, table, pos


SMALL = [c for c in SWEEP if c["num_levels"] == 16 and c["log2_T"] == 6 and c["pls"] == 2.0 and c["C"] in (1, 4)]


@pytest.mark.parametrize("interp", ["linear", "smoothstep"])
def test_float32_restatement_within_the_derived_bound_of_float64(interp):
    for k, cfg in enumerate(SMALL):
        L, table, pos = _case(cfg, interp, 300, k, bound=1.5)
        pos[:2] = [[-1.5] * cfg["D"], [1.5] * cfg["D"]]
        f32 = G.encode32(table, L, pos, 1.5); f64 = G.encode64(table, L, pos, 1.5)
        M = float(np.abs(table).max()); C_ = cfg["C"]
        for l in range(16):
            err = np.abs(f32[:, l * C_:(l + 1) * C_] - f64[:, l * C_:(l + 1) * C_]).max()
            assert err <= G.encode_tolerance(L, l, M), (cfg, l, err, G.encode_tolerance(L, l, M))
        assert np.abs(f64).max() > 0.1


@pytest.mark.parametrize("interp", ["linear", "smoothstep"])
def test_float64_gradients_against_finite_differences_and_linearity(interp):
    """Not drawn from the gradient code: the features are linear in the table, so <grad_out, encode64(table)> = <grad_table, table>; and the input gradient is the
    central difference of encode64 inside a cell.  grads64 starts from the float32 s (gridenc_refs' docstring), encode64 from float64 coordinates: the two differ by
    the interpolation point's rounding, relative D * 3 * gamma_4 * (scale + 0.5) of sum |terms| (encode_tolerance's first term)."""
    for k, cfg in enumerate(c for c in SWEEP if c["num_levels"] == 3 and c["log2_T"] == 4 and c["pls"] == 2.0 and c["C"] == 2):
        L, table, pos = _case(cfg, interp, 200, 50 + k)
        rng = np.random.default_rng(k)
        go = rng.normal(size=(200, 3 * 2))
        R = G.grads64(table, L, pos, 1.0, go)
        gt, tsum, _ = R["table"]
        lhs = float((go * G.encode64(table, L, pos, 1.0)).sum()); rhs = float((gt * table.astype(np.float64)).sum())
        top = float((tsum * np.abs(table)).sum()); M = float(np.abs(table).max())
        tol = sum(float(np.abs(go[:, 2 * l: 2 * l + 2]).sum()) * cfg["D"] * 3 * G.gamma(4) * (float(L["scale"][l]) + 0.5) * M for l in range(3))
        assert abs(lhs - rhs) <= tol + 1e-12 * top, (cfg, lhs, rhs, tol)
        # central differences, for points at least 0.05 of a finest cell away from a face
        h = 1e-4 / float(L["scale"][-1] + 1)
        keep = np.ones(200, bool)
        u, _ = G.unit32(L, pos, 1.0)
        for l in range(3):
            _, f, *_ = G.cells32(L, l, u)
            keep &= ((f > 0.05) & (f < 0.95)).all(axis=1)
        assert keep.sum() > 50
        gp, psum = R["pos"]
        p64 = pos.astype(np.float64)
        for a in range(cfg["D"]):
            # encode64 reads fp32 coordinates: difference the interpolant directly by shifting the float64 u through `bound`-free algebra
            e = np.zeros_like(p64); e[:, a] = h
            fd = ((_encode64_at(table, L, p64 + e) - _encode64_at(table, L, p64 - e)) * go).sum(axis=1) / (2 * h)
            # the largest gradient any table of this size allows: |d r / d s| <= 2 M, |d s / d f| <= 1.5, d f / d x = scale / 2; a wrong axis, pair or factor errs by its order
            big = sum(np.abs(go[:, 2 * l: 2 * l + 2]).sum(axis=1) * float(L["scale"][l]) * 1.5 * M for l in range(3))
            err = np.abs(fd - gp[:, a])
            assert (err[keep] <= 1e-4 * big[keep]).all(), (cfg, a, float((err / big)[keep].max()))


def _encode64_at(table, L, p64):
    """encode64's interpolant at float64 positions (bound 1), the cell picked in float64: for points away from faces."""
    t = np.asarray(table).astype(np.float64)
    u = (p64 + 1.0) / 2.0
    out = np.zeros((len(u), L["num_levels"] * L["C"]))
    for l in range(L["num_levels"]):
        p = u * float(L["scale"][l]) + (0.0 if L["align"] else 0.5)
        cell = np.floor(p); f = p - cell
        s = f * f * (3.0 - 2.0 * f) if L["smooth"] else f
        w = G.weights(s, 1.0 - s, np.float64)
        c = cell.astype(np.uint32)
        idx = np.stack([G.grid_index(L, l, [c[:, d] + np.uint32((k >> d) & 1) for d in range(L["D"])]) for k in range(1 << L["D"])], 1) + int(L["offsets"][l])
        out[:, l * L["C"]:(l + 1) * L["C"]] = (w[:, :, None] * t[idx]).sum(axis=1)
    return out


@pytest.mark.parametrize("interp", ["linear", "smoothstep"])
def test_float32_input_gradient_within_the_derived_bound_of_float64(interp):
    for k, cfg in enumerate(SMALL):
        L, table, pos = _case(cfg, interp, 200, 90 + k)
        pos[0] = 2.0                                                 # out of bounds: exactly 0
        go = np.random.default_rng(k).normal(size=(200, 16 * cfg["C"])).astype(np.float32)
        for ml in (None, 3):
            g32 = G.input_grad32(table, L, pos, 1.0, go, ml)
            gp, psum = G.grads64(table, L, pos, 1.0, go, ml)["pos"]
            assert g32.dtype == np.float32 and (g32[0] == 0).all() and np.abs(gp).max() > 0
            bound = G.gamma(G.pos_k(cfg["D"], 16, cfg["C"])) * psum
            assert (np.abs(g32 - gp) <= bound).all(), (cfg, ml, float((np.abs(g32 - gp) - bound).max()))


def _lay(**kw):
    from mirres_restir_nerf_mesh_amd import encoding
    return encoding.gridenc_layout(**kw)[0]


def test_c_abi_refuses_before_a_device_is_touched():
    from mirres_restir_nerf_mesh_amd import _lib
    L = _lib.lib()
    g = _lay(num_levels=3, base_resolution=2, log2_hashmap_size=4)
    buf = (C.c_float * 64)()                                        # host memory, 16-byte aligned or not: never dereferenced
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    err = lambda: L.mirres_last_error().decode()
    fwd = lambda g_, t, x, n, b, ml, o: L.mirres_grid_encode_fwd(C.byref(g_) if g_ is not None else None, t, x, n, b, ml, o, None)
    bwd = lambda g_, t, x, n, b, ml, go, gt, gp: L.mirres_grid_encode_bwd(C.byref(g_) if g_ is not None else None, t, x, n, b, ml, go, gt, gp, None)
    assert fwd(g, p, p, 0, 1.0, 3, p) == 0 and bwd(g, p, p, 0, 1.0, 3, p, p, p) == 0 and fwd(g, None, None, 0, 1.0, 3, None) == 0      # n == 0 launches nothing
    assert fwd(None, p, p, 4, 1.0, 3, p) < 0 and "mirres_grid_encode_fwd" in err()
    for args in ((None, p, 4, 1.0, 3, p), (p, None, 4, 1.0, 3, p), (p, p, 4, 1.0, 3, None), (p, p, -1, 1.0, 3, p), (p, p, (1 << 31) + 1, 1.0, 3, p),
                 (p, p, 4, 0.0, 3, p), (p, p, 4, -1.0, 3, p), (p, p, 4, float("inf"), 3, p), (p, p, 4, float("nan"), 3, p), (p, p, 4, 1.0, -1, p),
                 (C.c_void_p(p.value + 4), p, 4, 1.0, 3, p)):
        assert fwd(g, *args) == -1 and "mirres_grid_encode_fwd" in err(), args
    for args in ((None, p, 4, 1.0, 3, p, p, p), (p, None, 4, 1.0, 3, p, p, p), (p, p, 4, 1.0, 3, None, p, p), (p, p, -1, 1.0, 3, p, p, p),
                 (p, p, (1 << 31) + 1, 1.0, 3, p, p, p), (p, p, 4, 0.0, 3, p, p, p), (p, p, 4, float("nan"), 3, p, p, p)):
        assert bwd(g, *args) == -1 and "mirres_grid_encode_bwd" in err(), args
    # a layout the library would not have filled
    def broken(edit):
        b = _lay(num_levels=3, base_resolution=2, log2_hashmap_size=4); edit(b); return b
    edits = [lambda b: setattr(b, "input_dim", 4), lambda b: setattr(b, "input_dim", 1), lambda b: setattr(b, "level_dim", 3), lambda b: setattr(b, "level_dim", 16),
             lambda b: setattr(b, "num_levels", 0), lambda b: setattr(b, "num_levels", 17), lambda b: setattr(b, "gridtype", 2), lambda b: setattr(b, "align_corners", 2),
             lambda b: setattr(b, "interpolation", -1), lambda b: b.offsets.__setitem__(2, b.offsets[1]), lambda b: b.offsets.__setitem__(0, 8),
             lambda b: b.scale.__setitem__(1, float("nan")), lambda b: b.resolution.__setitem__(0, 0), lambda b: b.hashed.__setitem__(2, 1 - b.hashed[2])]
    for k, e in enumerate(edits):
        b = broken(e)
        assert fwd(b, p, p, 4, 1.0, 3, p) == -1, k
        assert bwd(b, p, p, 4, 1.0, 3, p, p, p) == -1, k
    for kw in (dict(input_dim=4), dict(input_dim=1), dict(level_dim=3), dict(num_levels=17), dict(num_levels=0), dict(per_level_scale=0.0), dict(per_level_scale=float("nan")),
               dict(base_resolution=0), dict(log2_hashmap_size=40), dict(per_level_scale=0.5)):
        with pytest.raises(_lib.MirresError, match="mirres_gridenc_layout"):
            _lay(**kw)
    with pytest.raises(KeyError):
        _lay(gridtype="dense")


def test_what_the_modules_refuse_and_what_get_encoder_returns():
    from mirres_restir_nerf_mesh_amd import encoding as E, _lib
    with pytest.raises(NotImplementedError, match="degree 5"):
        E.SHEncoder(degree=5)
    with pytest.raises(NotImplementedError):
        E.get_encoder("sh", degree=8)
    with pytest.raises(ValueError):
        E.SHEncoder(degree=9)
    with pytest.raises(ValueError):
        E.SHEncoder(input_dim=2)
    with pytest.raises(NotImplementedError, match="hashgrid_tcnn"):
        E.get_encoder("hashgrid_tcnn")
    with pytest.raises(NotImplementedError, match="unknown encoding 'dense'"):
        E.get_encoder("dense")
    sh, dim = E.get_encoder("sh", degree=3)
    assert isinstance(sh, E.SHEncoder) and dim == 9 and sh.output_dim == 9 and sh.degree == 3
    with pytest.raises(NotImplementedError, match="requires grad"):
        sh(torch.ones(2, 3, requires_grad=True))
    ident, dim = E.get_encoder("None", input_dim=5)
    x = torch.arange(10.0).reshape(2, 5)
    assert dim == 5 and ident(x, bound=3) is x
    for name in ("frequency", "frequency_torch"):
        fr, dim = E.get_encoder(name, input_dim=2, multires=3)
        xs = torch.tensor([[0.1, -0.7], [1.3, 0.25]])
        want = np.concatenate([xs.numpy()] + [f(xs.numpy() * np.float32(2.0 ** k)) for k in range(3) for f in (np.sin, np.cos)], axis=1)
        got = fr(xs)
        assert isinstance(fr, E.FreqEncoder) and dim == 2 + 2 * 2 * 3 and tuple(got.shape) == (2, dim) and np.abs(got.numpy() - want).max() <= 1e-6
    for name, gt in (("hashgrid", "hash"), ("tiledgrid", "tiled")):
        enc, dim = E.get_encoder(name, input_dim=2, num_levels=4, level_dim=4, base_resolution=4, log2_hashmap_size=8, desired_resolution=64, align_corners=True,
                                 interpolation="smoothstep")
        assert isinstance(enc, E.GridEncoder) and dim == 16 and (enc.gridtype, enc.align_corners, enc.interpolation, enc.input_dim, enc.level_dim) == (gt, True, "smoothstep", 2, 4)
        with pytest.raises(NotImplementedError, match="level_dim=4"):
            enc.grad_total_variation(1e-7, None, 1)
        with pytest.raises(_lib.MirresError, match="no CPU fallback"):
            enc(torch.zeros(3, 2))
        with pytest.raises(ValueError, match="input_dim"):
            enc(torch.zeros(3, 3))


def test_state_dict_keys_and_a_reference_checkpoints_encoder_loads():
    from mirres_restir_nerf_mesh_amd import encoding as E
    enc = E.GridEncoder(num_levels=4, base_resolution=4, log2_hashmap_size=8, desired_resolution=64)
    sd = enc.state_dict()
    assert sorted(sd) == ["embeddings", "offsets"] and sd["offsets"].dtype == torch.int32 and sd["embeddings"].dtype == torch.float32
    assert [n for n, _ in enc.named_parameters()] == ["embeddings"] and enc.embeddings.requires_grad
    L = G.layout(num_levels=4, pls=G.per_level_scale(64, 4, 4), base=4, log2_T=8)
    ck = {"embeddings": torch.randn(L["total"], 2), "offsets": torch.tensor(L["offsets"].tolist(), dtype=torch.int32)}
    enc.load_state_dict(ck)
    assert torch.equal(enc.embeddings.detach(), ck["embeddings"]) and torch.equal(enc.offsets, ck["offsets"])

    class Net(torch.nn.Module):                                     # the key names a reference checkpoint has: encoder.embeddings, encoder.offsets
        def __init__(self):
            super().__init__()
            self.encoder, self.in_dim = E.get_encoder("hashgrid", num_levels=4, base_resolution=4, log2_hashmap_size=8, desired_resolution=64)
            self.encoder_dir, self.in_dim_dir = E.get_encoder("sh")
    assert sorted(Net().state_dict()) == ["encoder.embeddings", "encoder.offsets"]
    other = E.GridEncoder(num_levels=4, base_resolution=4, log2_hashmap_size=9, desired_resolution=64)
    with pytest.raises(RuntimeError, match="size mismatch"):
        other.load_state_dict(ck)
    # the same sizes but another configuration's offsets (the kernels read the layout, not the buffer: a foreign table must not load silently)
    wrong = {"embeddings": ck["embeddings"], "offsets": ck["offsets"].clone()}
    wrong["offsets"][1] += 8
    with pytest.raises(RuntimeError, match="offsets .* are not this encoder's layout"):
        enc.load_state_dict(wrong)
    enc.load_state_dict({"embeddings": ck["embeddings"]}, strict=False)                 # without offsets: nothing to compare
    assert "GridEncoder(" in repr(enc) and "levels=4 x 2" in repr(enc)
