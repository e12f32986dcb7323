"""GPU: the fused training backward (mirres_render_bwd -> k_direct_bwd, csrc/backward.hip) ELEMENT BY ELEMENT against float64 autograd of the frame's
direct sums restated from the forward's own tape (tests/adjoint_refs.py:direct_sums).

The tape records, per sample and pixel, the merged reservoir and its visibility: every discrete choice the forward made.  So the float64 restatement takes the
same choices, and the gradients can be held to the tolerances of tests/test_gpu_adjoints.py instead of a whole-vector cosine.  Each case first holds the
restatement to the forward's own direct sums (the backward must not be consistent with a wrong tape), then compares every element of the environment, normal,
kd and (roughness, metallic) gradients.  The shape matrix reaches every path of k_direct_bwd: fewer samples than the MR_DBW_SPLIT lanes of a pixel, sample
counts that are no multiple of them, pixel counts that are no multiple of a workgroup's 32 pixels, a non-2:1 environment (W / H swap, row flip), tapes written
in several forward batches with a short last one, and the three stages of the environment scatter: LDS hash table, LDS overflow list, direct global atomics."""
import ctypes as C

import numpy as np
import pytest

from util import SmallFrame, elementwise

pytestmark = pytest.mark.gpu

TABLE, LIST = 2048, 2048      # backward.hip: MR_DBW_TABLE keys and MR_DBW_LIST entries per workgroup
WG_PX = 32                    # pixels per workgroup of k_direct_bwd: 256 threads / MR_DBW_SPLIT lanes per pixel


def _frame(oracle, scene_mod, fx, fy, env_hw, env_kind=None, rough=False):
    """env_kind: None = SmallFrame's sky with a sun lobe; "flat"; "black_lower_sun"."""
    F = SmallFrame(oracle, scene_mod, fx=fx, fy=fy, env_hw=env_hw)
    env = F.env
    if env_kind == "black_lower_sun":     # black where world y < 0 (whole table rows fall back) next to a one-texel sun 1e5 x the median (tests/envmap_refs.py)
        import envmap_refs as E
        env = E.black_world_lower(E.with_sun(E.sky(env_hw[0], env_hw[1], 2)))
    elif env_kind == "flat":     # low contrast, no sun: light samples spread over the whole sky instead of the few texels of a sun lobe
        env = (0.4 + 0.25 * scene_mod.make_env(env_hw[0], env_hw[1], sun=0.0)).astype(np.float32)
    rm = F.rm.copy()
    if rough:
        rm[:, 0] = 0.6 + 0.4 * (rm[:, 0] - 0.15) / 0.7
        rm[:, 1] = 0.0
    return F, env, rm


def _worker(F):
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    return W


def _forward(F, W, env, rm, spp, seed):
    """The training forward (what _FusedLoop.forward runs) with a NaN-filled tape. Returns the inputs, the three direct sums, the tape and the call's arguments."""
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    x = dict(env=cu(env), occ=cu(F.occ[:, None]), normal=cu(F.normal), depth=cu(F.depth[:, None]), kd=cu(F.kd), rm=cu(rm), rd=cu(F.ray_dir_raw), pos=cu(F.pos))
    ctx = get_ctx(F.fx, F.fy)
    tape = torch.full((spp * F.N, 8), float("nan"), dtype=torch.float32, device="cuda")
    sums, a, keep = RR.render_fused(ctx, W, None, False, (1.0, 1.0, 1.0), x["env"], x["occ"], x["normal"], x["depth"], x["kd"], x["rm"], x["rd"], x["pos"], spp, 0, 1,
                                    1.0, 1.0, 1.0, seed, spp_range=(0, spp), tape=tape)
    return dict(x=x, sums=sums, tape=tape, a=a, keep=keep, ctx=ctx, spp=spp)


def _backward(fw, cot, g_env=None, fill=float("nan"), samples=None, args=None):
    """mirres_render_bwd through ctypes: returns (rc, g_normal, g_kd, g_rough_metal, g_env). The per-pixel buffers start filled with `fill`."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, stream_ptr
    N = fw["ctx"].N
    g = [torch.full((N, k), fill, dtype=torch.float32, device="cuda") for k in (3, 3, 2)]
    if g_env is None:
        g_env = torch.zeros_like(fw["x"]["env"])
    rc = lib().mirres_render_bwd(fw["ctx"].h, C.byref(args if args is not None else fw["a"]), fw["spp"] if samples is None else samples, cot[0].data_ptr(),
                                 cot[1].data_ptr(), cot[2].data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g_env.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rc, g[0], g[1], g[2], g_env


def _cotangents(N, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.rand((N, 3), device="cuda", generator=gen) for _ in range(3)]


def _footprints(tape, occ, N, H, W, weights=False):
    """The environment texels (caller's layout) k_direct_bwd scatters into, per tape row: [rows, 4] indices of the rows that contribute (non-empty reservoir,
    visible, foreground pixel, not at a pole), and those rows. float64 restatement of env_le_footprint(ngp_dir(oct_decode(light_data.yz)))."""
    S = tape.shape[0] // N
    on = (tape[:, 0] > 0.1) & (tape[:, 6] > 0) & np.tile(occ > 0.1, S)
    rows = np.nonzero(on)[0]
    f = tape[rows, 1:3].astype(np.float64) * 2.0 - 1.0
    z = 1.0 - np.abs(f[:, 0]) - np.abs(f[:, 1])
    t = np.clip(-z, 0.0, 1.0)
    lx = f[:, 0] + np.where(f[:, 0] >= 0, -t, t); ly = f[:, 1] + np.where(f[:, 1] >= 0, -t, t)
    ln = np.sqrt(lx * lx + ly * ly + z * z)
    dx, dy, dz = -lx / ln, z / ln, ly / ln                 # ngp_dir
    theta = np.arccos(np.clip(dy, -1.0, 1.0))
    keep = np.abs(np.sin(theta)) >= 1e-4
    rows, theta, dx, dz = rows[keep], theta[keep], dx[keep], dz[keep]
    phi = np.arctan2(dz, dx); phi = np.where(phi < 0, phi + 6.2831853, phi)
    x, y = phi * 0.1591549 * W - 0.5, (1.0 - theta * 0.31830988) * H - 0.5
    x0, y0 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    caller = lambda yy, xx: (H - 1 - yy) * W + xx         # tex row y = caller's row H - 1 - y (k_flip_env)
    idx = np.stack((caller(y0, x0), caller(y0, x1), caller(y1, x0), caller(y1, x1)), 1)
    if not weights:
        return idx, rows
    u, v = x - x0, y - y0                                 # against the clamped corner, as helper.slang:46-71
    return idx, rows, np.stack(((1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v), 1)


def _f32_footprints(oracle, ld, H, W):
    """The kernel's own footprints, env_le_footprint(ngp_dir(oct_decode(light_data.yz))) in fp32, for tape rows ld [n, 3]: texel indices (caller layout)
    and weights [n, 4].  Read off the oracle's env_le, which evaluates the same fp32 arithmetic (include/mirres_fmath.h) and is linear in the texture: the four
    texels of a footprint have the four parities (x % 2, y % 2), so a texture that is 1 on one parity class returns that corner's weight exactly
    ((1 - u) * (1 - v) and so on: the other products are 0), and one that holds x or y on it returns weight * x or weight * y.  A clamped corner (x1 = x0)
    shares its texel's class and adds to its weight, as the scatter adds it to the texel."""
    d = np.stack([oracle.oct_decode(f) for f in np.asarray(ld, np.float32)[:, 1:3]]).astype(np.float32)
    m = np.ascontiguousarray(np.stack([-d[:, 0], d[:, 2], d[:, 1]], 1))                       # ngp_dir: exact in fp32
    ty, tx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cls = ((tx % 2) + 2 * (ty % 2)).ravel()
    idx = np.full((len(m), 4), -1, np.int64); w = np.zeros((len(m), 4))
    for c in range(4):
        on = (cls == c).astype(np.float32)
        probe = np.ascontiguousarray(np.stack([on, on * tx.ravel(), on * ty.ravel()], 1).astype(np.float32))
        r = oracle.env_le(probe, W, H, m).astype(np.float64)
        nz = r[:, 0] != 0
        xx = np.rint(r[nz, 1] / r[nz, 0]).astype(np.int64); yy = np.rint(r[nz, 2] / r[nz, 0]).astype(np.int64)
        assert ((xx % 2) + 2 * (yy % 2) == c).all() and (xx >= 0).all() and (xx < W).all() and (yy >= 0).all() and (yy < H).all()
        idx[nz, c] = (H - 1 - yy) * W + xx; w[nz, c] = r[nz, 0]
    return idx, w


def _env_grad_past_2e22(oracle, tape, x, cot, g_env, ref64, N, H, W):
    """The environment gradient of a map with more than 2^22 texels.  At W = 4096 the fp32 texel coordinate x = phi / 2 pi W - 1/2 of a footprint carries an
    error of order W x a few ulp, up to ~1e-3 of a texel, so the kernel's bilinear weights and the float64 reference's differ by that much; a texel reached
    by one heavy sample near its far edge then differs by more than the element-wise tolerance.  So the element-wise check, at its usual tolerances, is made
    against a float64 scatter of the reference's per-sample derivative W x d/dLi through the KERNEL's fp32 footprints (weights and texels, _f32_footprints);
    and the difference between that scatter and the pure float64 gradient is shown to be a weight difference within the fp32 error bound, with texel
    choices that differ only at texel borders."""
    import torch
    import adjoint_refs as R
    t = tape.cpu().numpy()
    rows = np.nonzero(t[:, 0] > 0.1)[0]
    gl = R.direct_emission_cotangent(tape.double(), x["env"].double(), x["occ"].double(), x["normal"].double(), x["rd"].double(), x["kd"].double(),
                                     x["rm"].double(), [c.double() for c in cot]).detach().cpu().numpy()[rows]
    idx32, w32 = _f32_footprints(oracle, t[rows], H, W)
    ref32 = np.zeros((H * W, 3))
    for k in range(4):
        ok = idx32[:, k] >= 0
        np.add.at(ref32, idx32[ok, k], gl[ok] * w32[ok, k, None])
    elementwise(g_env, torch.from_numpy(ref32.reshape(H, W, 3)), "k_direct_bwd d/d(env texel), fp32 footprints")
    # the whole gap to the float64 gradient is in the weights: per (sample, texel) the float64 minus the fp32 footprint weight
    idx64, rows64, w64 = _footprints(t, x["occ"][:, 0].cpu().numpy(), N, H, W, weights=True)
    pos = np.searchsorted(rows, rows64)
    HW = H * W
    keys = np.concatenate([(pos[:, None] * HW + idx64).ravel(), (np.arange(len(rows))[:, None] * HW + np.maximum(idx32, 0)).ravel()])
    vals = np.concatenate([w64.ravel(), -np.where(idx32 >= 0, w32, 0).ravel()])
    uk, inv = np.unique(keys, return_inverse=True)
    dw = np.zeros(len(uk)); np.add.at(dw, inv, vals)
    r_of, tex_of = uk // HW, uk % HW
    live = np.abs(gl[r_of]).sum(1) > 0
    # fp32 error of a footprint weight: the texel coordinates x = W phi / 2 pi, y = H theta / pi of an fp32 direction that is a few ulp off; phi = atan2 and
    # theta = acos are ill-conditioned by 1 / sin(theta) near the map's poles; with the roundings of the products, 4 (W + H) u (1 + 1 / sin theta) bounds
    # both with room.  A corner that changes texel at a border has a weight within that bound of 0
    f = t[rows, 1:3].astype(np.float64) * 2 - 1
    z = 1 - np.abs(f[:, 0]) - np.abs(f[:, 1]); c = np.clip(-z, 0, 1)
    lx = f[:, 0] + np.where(f[:, 0] >= 0, -c, c); ly = f[:, 1] + np.where(f[:, 1] >= 0, -c, c)
    cos_t = z / np.sqrt(lx * lx + ly * ly + z * z)                                    # map-frame y = world z (ngp_dir)
    sin_t = np.sqrt(np.maximum(1 - cos_t * cos_t, 0.0))
    bound = 4 * (W + H) * 2.0 ** -24 * (1 + 1 / np.maximum(sin_t[r_of], 1e-4))
    over = np.abs(dw) > bound
    assert not (over & live).any(), "%d footprint weights differ from float64 by more than the fp32 bound (max ratio %.2f): not an fp32 weight error" % (
        int((over & live).sum()), float((np.abs(dw) / bound)[live].max()))
    g = ref64.detach().cpu().numpy().reshape(-1, 3)
    gap = np.abs(g - ref32)
    lim = np.zeros((HW, 3)); np.add.at(lim, tex_of, np.abs(gl[r_of]) * np.abs(dw)[:, None])
    assert (gap <= lim + 1e-12 * np.abs(g).max()).all()
    scale = np.abs(g).max()
    n_out = int((gap > 1e-3 * np.abs(g) + 1e-4 * scale).sum())
    print("[env %dx%d] fp32 vs float64 footprint weights: max difference %.3e (%.2f of its bound); %d gradient elements off the pure float64 gradient by "
          "more than the element-wise tolerance, max %.3e" % (H, W, np.abs(dw[live]).max(), float((np.abs(dw) / bound)[live].max()), n_out, gap.max()))


def _distinct_per_workgroup(idx, rows, N, HW):
    wg = (rows % N) // WG_PX
    keys = np.unique((wg[:, None] * HW + idx).ravel())
    return np.bincount(keys // HW, minlength=(N + WG_PX - 1) // WG_PX)


# frame fx x fy, env H x W, samples, MIRRES_PT_BATCH, env kind (_frame), rough materials
CASES = [
    pytest.param((37, 23, (24, 80), 1, None, None, False), id="37x23_env24x80_1spp"),              # S < MR_DBW_SPLIT; N % 32 != 0; non-2:1 env (W/H swap, row flip)
    pytest.param((37, 23, (24, 80), 9, "4", None, False), id="37x23_env24x80_9spp_batch4"),        # S % 8 != 0; batches of 4, 4, 1 samples: tape offsets
    pytest.param((48, 40, (8, 16), 17, None, None, False), id="48x40_env8x16_17spp"),              # many samples onto few texels: same-key contention
    pytest.param((64, 32, (256, 512), 1024, None, "flat", True), id="64x32_env256x512_1024spp_flat"),  # table, overflow list and direct global atomics
    pytest.param((32, 24, (2048, 4096), 16, None, "flat", False), id="32x24_env2048x4096_16spp_flat"),  # texel indices past 2^22: the hash's whole key range
    pytest.param((48, 40, (64, 128), 8, None, "black_lower_sun", False), id="48x40_env64x128_8spp_black_lower_sun"),  # fallback rows next to a sun
]


@pytest.mark.parametrize("case", CASES)
def test_fused_backward_matches_float64_reference_from_the_tape(case, oracle, scene_mod, monkeypatch):
    import torch
    import adjoint_refs as R
    fx, fy, env_hw, spp, batch, env_kind, rough = case
    if batch is not None:
        monkeypatch.setenv("MIRRES_PT_BATCH", batch)
    else:
        monkeypatch.delenv("MIRRES_PT_BATCH", raising=False)
    F, env, rm = _frame(oracle, scene_mod, fx, fy, env_hw, env_kind, rough)
    W = _worker(F)
    fw = _forward(F, W, env, rm, spp, seed=777)
    x, N, (H, Wd) = fw["x"], F.N, env_hw
    tape = fw["tape"]
    # the forward wrote every record of every sample (a short last batch included), and nothing is NaN or infinite
    assert bool(torch.isfinite(tape).all()), "%d tape values not written or not finite" % int((~torch.isfinite(tape)).sum())
    fg = (x["occ"][:, 0] > 0.1)
    assert int(fg.sum()) >= 100 and int((~fg).sum()) > 0
    # float64 restatement from the tape = the forward's own direct sums on foreground pixels (the forward tolerance of test_final_shading_adjoint_element_by_element)
    x64 = {k: x[k].double().requires_grad_(True) for k in ("env", "normal", "kd", "rm")}
    c64 = R.direct_sums(tape.double(), x64["env"], x["occ"].double(), x64["normal"], x["rd"].double(), x64["kd"], x64["rm"])
    for k, nm in enumerate(("color", "diffuse", "specular")):
        np.testing.assert_allclose(c64[k].detach()[fg].cpu().numpy(), fw["sums"][k][fg].cpu().numpy(), rtol=5e-4, atol=2e-6, err_msg="direct " + nm + " sum")
    assert float(c64[0].detach()[fg].abs().sum()) > 0
    cot = _cotangents(N, seed=spp)
    sum((c * w.double()).sum() for c, w in zip(c64, cot)).backward()
    rc, g_n, g_kd, g_rm, g_env = _backward(fw, cot)
    assert rc == 0
    for nm, got, ref in (("normal", g_n, x64["normal"]), ("kd", g_kd, x64["kd"]), ("rough_metal", g_rm, x64["rm"])):
        assert bool(torch.isfinite(got).all()), nm
        assert float(got[~fg].abs().sum()) == 0.0, nm + ": background pixels carry no gradient"
        elementwise(got, ref.grad, "k_direct_bwd d/d" + nm)
    assert bool(torch.isfinite(g_env).all())
    if H * Wd <= 1 << 22:
        elementwise(g_env, x64["env"].grad, "k_direct_bwd d/d(env texel)")
    else:
        _env_grad_past_2e22(oracle, tape, x, cot, g_env, x64["env"].grad, N, H, Wd)
    # texels that no footprint reaches (nor a neighbour of one: a boundary sample's truncation may fall either way in fp32) receive exactly nothing
    idx, rows = _footprints(tape.cpu().numpy(), x["occ"][:, 0].cpu().numpy(), N, H, Wd)
    touched = np.zeros(H * Wd, bool); touched[idx.ravel()] = True
    t2 = touched.reshape(H, Wd)
    near = t2.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(np.roll(t2, dy, 0), dx, 1)
    ge = g_env.cpu().numpy()
    assert (ge[~near] == 0).all(), "%d texels that no sample reaches received a gradient" % int((ge[~near] != 0).any(-1).sum())
    assert (ge[t2] != 0).any(-1).mean() > 0.5
    distinct = _distinct_per_workgroup(idx, rows, N, H * Wd)
    print("[%dx%d env %dx%d %d spp] %d contributing samples, %d texels touched, distinct texels per workgroup: max %d, median %d" % (
        fx, fy, H, Wd, spp, len(rows), int(touched.sum()), int(distinct.max()), int(np.median(distinct))))
    if env_kind == "black_lower_sun":
        bright = np.argmax(env.reshape(-1, 3).sum(1))
        assert touched[bright] and (env.reshape(-1, 3)[touched].sum(1) == 0).any(), "no footprint on both the sun and a black texel"
    if env_hw == (256, 512):
        # a workgroup with more distinct texels than the table holds spills into the list; with more than table + list, the list is full and the rest
        # goes to global memory directly (each texel outside the table appends at least one list entry)
        assert int(distinct.max()) > TABLE, "no workgroup overflows the LDS table (max %d distinct texels)" % int(distinct.max())
        assert int(distinct.max()) > TABLE + LIST, "no workgroup fills the LDS overflow list (max %d distinct texels)" % int(distinct.max())


def test_render_bwd_api_contract(oracle, scene_mod, monkeypatch):
    """include/mirres.h: g_env accumulates, the per-pixel gradients are overwritten (background pixels 0), and a call without samples or without a tape is
    refused with MIRRES_E_ARG and a message."""
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, RenderArgs
    monkeypatch.delenv("MIRRES_PT_BATCH", raising=False)
    F, env, rm = _frame(oracle, scene_mod, 37, 23, (24, 80))
    fw = _forward(F, _worker(F), env, rm, 3, seed=91)
    cot = _cotangents(F.N, seed=5)
    fg = fw["x"]["occ"][:, 0] > 0.1
    rc, g_n0, g_kd0, g_rm0, g_env0 = _backward(fw, cot, fill=0.0)
    assert rc == 0
    c = 0.25
    rc, g_n, g_kd, g_rm, g_env = _backward(fw, cot, g_env=torch.full_like(fw["x"]["env"], c), fill=float("nan"))
    assert rc == 0
    for nm, got, ref in (("normal", g_n, g_n0), ("kd", g_kd, g_kd0), ("rough_metal", g_rm, g_rm0)):
        assert bool(torch.isfinite(got).all()), nm + ": NaN-filled output buffer not overwritten everywhere"
        assert float(got[~fg].abs().sum()) == 0.0, nm
        assert torch.equal(got, ref), nm + ": depends on what the buffer held"
    e0, e = g_env0.cpu().numpy().astype(np.float64), g_env.cpu().numpy().astype(np.float64)
    assert (e0 != 0).sum() > 0
    assert (e[e0 == 0] == c).all(), "g_env is not accumulated into"
    np.testing.assert_allclose(e, c + e0, rtol=1e-5, atol=1e-5 * np.abs(e0).max() + 1e-7)
    for samples in (0, -1):
        rc = _backward(fw, cot, samples=samples)[0]
        assert rc == -1 and "mirres_render_bwd" in lib().mirres_last_error().decode(), samples
    args = RenderArgs(); C.memmove(C.byref(args), C.byref(fw["a"]), C.sizeof(RenderArgs)); args.tape = None
    rc = _backward(fw, cot, args=args)[0]
    assert rc == -1 and "tape" in lib().mirres_last_error().decode()


def test_two_forwards_before_their_backwards(oracle, scene_mod, monkeypatch):
    """Several views accumulated in one step: forward A, forward B (same context: another view and another environment of the same size), backward A,
    backward B give what forward A -> backward A and forward B -> backward B give. The backward re-flips its own env into the context's shared texture, so
    it must read nothing a later forward left behind. Per-pixel gradients bit for bit; the environment gradient, a sum of fp32 atomics whose order is not
    fixed, to fp32 summation order."""
    import torch
    monkeypatch.delenv("MIRRES_PT_BATCH", raising=False)
    FA, envA, rmA = _frame(oracle, scene_mod, 48, 40, (32, 64))
    monkeypatch.setenv("MIRRES_TEST_SEED", "1")             # another view of the same mesh (tests/util.py:SmallFrame)
    FB, _, rmB = _frame(oracle, scene_mod, 48, 40, (32, 64))
    monkeypatch.delenv("MIRRES_TEST_SEED")
    envB = scene_mod.make_env(32, 64, seed=3, sun=40.0)
    assert not np.array_equal(FA.ray_dir_raw, FB.ray_dir_raw) and not np.array_equal(envA, envB)
    W = _worker(FA)
    cotA, cotB = _cotangents(FA.N, seed=21), _cotangents(FB.N, seed=22)
    seq, tapes = [], []
    for F, env, rm, cot, seed in ((FA, envA, rmA, cotA, 11), (FB, envB, rmB, cotB, 12)):
        fw = _forward(F, W, env, rm, 5, seed)
        seq.append(_backward(fw, cot)[1:]); tapes.append(fw["tape"])
    fA = _forward(FA, W, envA, rmA, 5, 11)
    fB = _forward(FB, W, envB, rmB, 5, 12)
    assert torch.equal(fA["tape"], tapes[0]) and torch.equal(fB["tape"], tapes[1])    # the forward itself is reproducible
    both = [_backward(fA, cotA)[1:], _backward(fB, cotB)[1:]]
    for view, got, ref in zip("AB", both, seq):
        for nm, g, r in zip(("normal", "kd", "rough_metal"), got[:3], ref[:3]):
            assert torch.equal(g, r), "view %s d/d%s differs when another forward ran in between" % (view, nm)
        ge, re_ = got[3].cpu().numpy(), ref[3].cpu().numpy()
        assert np.abs(re_).max() > 0
        np.testing.assert_allclose(ge, re_, rtol=1e-5, atol=1e-6 * np.abs(re_).max(), err_msg="view %s d/d(env texel)" % view)
