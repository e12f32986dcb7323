"""The stage-0 ray-marching operators on the device (csrc/raymarch.hip through mirres_restir_nerf_mesh_amd.raymarching and stage0.DensityGrid), bit for bit against the
numpy float32 restatement (tests/raymarch_refs.py), which tests/test_raymarch_host.py holds to known answers and to the device header built for the host.  Every input
set first passes through the restatement on the host, and nothing is launched unless no ray needs more than 1e5 loop passes; the hostile rays (zero direction, NaN
near, origin at 1e7) are part of the device inputs because the host tests show them to end within that cap.  Two NaNs count as equal whatever their sign bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raymarch_refs as R      # noqa: E402
from test_raymarch_host import same      # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def RM():
    from mirres_restir_nerf_mesh_amd import raymarching
    return raymarching


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- integer helpers, near / far
def test_integer_helpers_bit_equal(RM):
    rng = np.random.default_rng(1)
    coords = rng.integers(0, 1024, size=(5001, 3)).astype(np.int32)
    coords[:3] = [[0, 0, 0], [1023, 1023, 1023], [127, 0, 127]]
    idx = host(RM.morton3D(dev(coords)))
    assert np.array_equal(idx, R.morton3D(coords))
    assert np.array_equal(host(RM.morton3D_invert(dev(idx))), coords) and np.array_equal(R.morton3D_invert(idx), coords)
    H, Cn, thresh = 16, 2, F(0.37)
    grid = rng.uniform(0, 1, size=(Cn, H ** 3)).astype(np.float32)
    grid[0, :8] = [thresh, np.nextafter(thresh, F(1)), np.nextafter(thresh, F(0)), -1.0, np.nan, np.inf, 0.0, thresh]
    got = host(RM.packbits(dev(grid), float(thresh)))
    assert got.dtype == np.uint8 and got.shape == (Cn * H ** 3 // 8,) and np.array_equal(got, R.packbits(grid, thresh))
    assert got[0] == 0b00100010                                              # equal to the threshold, -1 and NaN: not occupied
    pre = torch.full((Cn * H ** 3 // 8,), 255, dtype=torch.uint8, device="cuda")
    assert RM.packbits(dev(grid), float(thresh), pre) is pre and np.array_equal(host(pre), got)
    counts = rng.integers(0, 9, size=700).astype(np.int32); counts[5] = 0
    rays = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1).astype(np.int32)
    M = int(counts.sum()) - 3                                                # the last rays' spans leave [0, M): skipped, never written past the end
    assert np.array_equal(host(RM.flatten_rays(dev(rays), M)), R.flatten_rays(rays, M))


def test_near_far_bit_equal(RM):
    o, d, aabb = R.near_far_inputs()                                         # zero components on each axis, -0.0, a miss, origins inside
    N = o.shape[0]
    near, far = RM.near_far_from_aabb(dev(o), dev(d), dev(aabb), 0.2)
    wn, wf = R.near_far_from_aabb(o, d, aabb, 0.2)
    assert same(host(near), wn) and same(host(far), wf)
    miss = wn == R.FLT_MAX
    assert miss[9] and 100 < miss.sum() < N - 100 and (wf[miss] == R.FLT_MAX).all() and (wn[:1024][~miss[:1024]] == F(0.2)).all()


# ---------------------------------------------------------------------------------------------------------------- march_rays_train
def run_march_train(RM, c):
    assert c["trips"].max() <= R.TRIP_CAP                                    # before anything is launched
    return RM.march_rays_train(dev(c["o"]), dev(c["d"]), c["bound"], c["contract"], dev(c["bits"]), c["C"], c["H"], dev(c["nears"]), dev(c["fars"]), c["perturb"],
                               c["dt_gamma"], c["max_steps"], noises=dev(c["noises"]))


def check_march_train(RM, c):
    xyzs, dirs, ts, rays = run_march_train(RM, c)
    r = host(rays)
    assert r.dtype == np.int32 and np.array_equal(r, c["rays"])
    assert np.array_equal(r[:, 0], np.concatenate([[0], np.cumsum(r[:, 1])[:-1]])) and xyzs.shape[0] == r[:, 1].sum()      # M is the total
    assert same(host(xyzs), c["xyzs"]) and same(host(dirs), c["dirs"]) and same(host(ts), c["ts"])
    return xyzs, dirs, ts, rays


@pytest.mark.parametrize("shape_i", range(len(R.GRID_SHAPES)))
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_march_rays_train_bit_equal(RM, kind, shape_i):
    """Every parameter set on every grid, 65 rays (more than one wave, no multiple of 64), the hostile rays among them."""
    capped = 0
    for pi in range(len(R.MARCH_PARAMS)):
        c = R.march_train_case(kind, shape_i, pi, 65)
        check_march_train(RM, c)
        capped += int((c["rays"][:, 1] == c["max_steps"]).sum())
        assert (c["rays"][:R.N_HOSTILE - 1, 1] == 0).all()
    if kind == "full":
        assert capped > 0                                                    # some rays hit max_steps
    if kind == "empty":
        assert all(R.march_train_case(kind, shape_i, pi, 65)["rays"][:, 1].sum() == 0 for pi in range(len(R.MARCH_PARAMS)) if not R.MARCH_PARAMS[pi]["contract"])


# k_rm_scan (csrc/raymarch.hip:123) gives each of its RM_SCAN_BLOCK = 1024 threads a run of ceil(N / 1024) rays: 1025, 2050 and 3073 make runs of 2, 3 and 4,
# a last non-empty thread (512, 683, 768) that holds ONE ray, and empty threads after it; 2048 divides evenly
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2048, 1025, 2050, 3073])
def test_march_rays_train_ray_counts_and_repeatability(RM, N):
    for pi in (0, 15):                                                       # (dt_gamma 0, no perturb, no contract, 64 steps) and (1/256, perturb, contract, 1024)
        c = R.march_train_case("random", 1, pi, N)
        a = check_march_train(RM, c)
        b = run_march_train(RM, c)
        for x, y in zip(a, b):
            assert torch.equal(x, y)                                         # no atomic counter: two runs give identical tensors
    if N >= 16:
        c = R.march_train_case("random", 0, 1, N)
        assert c["rays"][3, 1] == 0 and c["nears"][3] == R.FLT_MAX           # the ray that misses
        assert c["rays"][4:9, 1].sum() > 0                                   # the rays along cell faces and from inside do sample


def _scan_fill(kind, N):
    """int32 counts [N] for k_rm_scan, which reads them as uint32.  'all': every count 0xFFFFFFFF.  'edges': zeros, and 0xFFFFFFFF at every ray of scan threads
    31, 32, 63 and 64 (lane 0 of the second wave) and at the first and the last ray of every other eighth thread's run (thread 0 among them) and of the last
    thread that holds a ray; a run is ceil(N / 1024) rays, so runs of 4 keep zeros between their ends."""
    if kind == "all":
        return np.full(N, -1, np.int32)
    run = -(-N // 1024)
    last_thread = (N - 1) // run
    counts = np.zeros(N, np.int32)
    for t in range(last_thread + 1):
        a, b = t * run, min((t + 1) * run, N)
        if t in (31, 32, 63, 64):
            counts[a:b] = -1
        elif t % 8 == 0 or t == last_thread:
            counts[a] = counts[b - 1] = -1
    return counts


@pytest.mark.parametrize("N", [64, 65, 1024, 1025, 3073])
@pytest.mark.parametrize("kind", ["all", "edges"])
def test_march_train_scan_carries_past_32_bits(kind, N):
    """mirres_rm_march_train_scan on counts whose prefix sums pass 2^32 (with 'all' at the second ray): the 64-bit workgroup scan (block_excl_scan of
    csrc/device_scan.hpp on unsigned long long, whose wave step shuffles a value as two 32-bit halves) must carry between the halves inside a wave, across waves
    and across the threads' runs.  Called through ctypes: march_rays_train refuses such totals.  Offsets = the exclusive sums clamped at 2^31 - 1, total = the
    exact sum (at most 3073 (2^32 - 1)), the counts untouched — all from numpy int64.  This is the one place the library's u64 scan can be driven past 2^32 at
    test sizes: csrc/bake.hip's and csrc/albedo.hip's u64 scans would need more than 2^32 work items or pixels through their entry points, and they share the
    primitive this test drives there."""
    from mirres_restir_nerf_mesh_amd._lib import lib, check, ptr, stream_ptr
    counts = _scan_fill(kind, N)
    c64 = counts.astype(np.uint32).astype(np.int64)
    if kind == "edges":
        run = -(-N // 1024)
        assert c64[0] == 0xFFFFFFFF and c64[31 * run] == 0xFFFFFFFF and c64[min(64 * run - 1, N - 1)] == 0xFFFFFFFF and 3 <= (c64 != 0).sum() < N
    excl = np.cumsum(c64) - c64
    assert excl[1] == 0xFFFFFFFF and excl[-1] + c64[-1] >= 2 ** 32 and excl.max() < 2 ** 62         # the sums are exact in int64 and pass 32 bits
    rays = np.stack([np.full(N, 0x5A5A5A5A, np.int32), counts], 1)             # column 0 arrives dirty: every offset is written
    g_rays = dev(rays)
    total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    check(lib().mirres_rm_march_train_scan(ptr(g_rays), N, ptr(total), stream_ptr()), "mirres_rm_march_train_scan")
    got = host(g_rays)
    assert np.array_equal(got[:, 0].astype(np.int64), np.minimum(excl, 2 ** 31 - 1))
    assert int(total.item()) == int(c64.sum())
    assert np.array_equal(got[:, 1], counts)


def test_march_perturb_without_noises_draws_on_the_device(RM):
    c = R.march_train_case("full", 0, 0, 65)
    torch.manual_seed(5)
    a = RM.march_rays_train(dev(c["o"]), dev(c["d"]), 1.0, False, dev(c["bits"]), 1, 16, dev(c["nears"]), dev(c["fars"]), True, 0.0, 64)
    torch.manual_seed(5)
    noises = torch.rand(65, dtype=torch.float32, device="cuda")
    b = RM.march_rays_train(dev(c["o"]), dev(c["d"]), 1.0, False, dev(c["bits"]), 1, 16, dev(c["nears"]), dev(c["fars"]), False, 0.0, 64, noises=noises)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[2], run_march_train(RM, c)[2])


# ---------------------------------------------------------------------------------------------------------------- the inference loop
def sigma_of(xyzs):
    """R.sigma_of in torch on the device: the same operations in float32."""
    r2 = (xyzs[:, 0] * xyzs[:, 0] + xyzs[:, 1] * xyzs[:, 1]) + xyzs[:, 2] * xyzs[:, 2]
    return (0.49 - r2).clamp(min=0) * 800.0


def test_inference_loop_bit_equal(RM):
    """The loop of nerf/renderer.py:784-828 as it stands, against R.infer_case — the host's run of the same loop, whose every round tests/test_raymarch_host.py has put
    through the host build of the device header under the cap."""
    c = R.infer_case()
    N, H, max_steps, T_thresh = c["N"], c["H"], c["max_steps"], c["T_thresh"]
    want = c["rounds"]
    assert max(r["trips"].max() for r in want) <= R.TRIP_CAP                 # before anything is launched
    go, gd, gb, gn, gf = dev(c["o"]), dev(c["d"]), dev(c["bits"]), dev(c["nears"]), dev(c["fars"])
    ws = torch.zeros(N, device="cuda"); dp = torch.zeros(N, device="cuda"); im = torch.zeros(N, 3, device="cuda")
    tcol = dev(R.INFER_COLOUR)
    got = []
    n_alive, rays_alive, rays_t, step = N, torch.arange(N, dtype=torch.int32, device="cuda"), gn.clone(), 0
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts = RM.march_rays(n_alive, n_step, rays_alive, rays_t, go, gd, 1.0, False, gb, 1, H, gn, gf, False, 0.0, max_steps)
        RM.composite_rays(n_alive, n_step, rays_alive, rays_t, sigma_of(xyzs), tcol.expand(n_alive * n_step, 3), ts, ws, dp, im, T_thresh, False)
        got.append((n_step, host(xyzs), host(ts), host(rays_alive), host(rays_t), host(dirs)))
        rays_alive = rays_alive[rays_alive >= 0]
        step += n_step
    assert len(got) == len(want) and len(want) >= 4
    by_opacity = by_gap = 0
    for g, w in zip(got, want):
        assert g[0] == w["n_step"] and same(g[1], w["xyzs"]) and same(g[2], w["ts"]) and np.array_equal(g[3], w["alive_after"]) and same(g[4], w["t_after"])
        assert same(g[5], w["dirs"])
        full = (w["ts"].reshape(-1, w["n_step"], 2)[:, :, 0] != 0).all(1)
        by_opacity += int(((w["alive_after"] < 0) & full).sum()); by_gap += int(((w["alive_after"] < 0) & ~full).sum())
    assert by_opacity > 50 and by_gap > 50                                   # rays ended by opacity and rays ended by ts[0] == 0
    assert same(host(ws), c["weights_sum"]) and same(host(dp), c["depth"]) and same(host(im), c["image"])
    assert (c["weights_sum"] > 0.99).sum() > 50 and (c["weights_sum"] == 0).sum() > 50


# ---------------------------------------------------------------------------------------------------------------- composite_rays_train
train_composite_inputs = R.train_composite_inputs      # shared with tests/test_gpu_ref_raymarch.py and the host tests


@pytest.mark.parametrize("alpha_mode", [False, True])
def test_composite_rays_train_forward_and_backward_bit_equal(RM, alpha_mode):
    sig, rgb, ts, rays, M = train_composite_inputs(alpha_mode)
    N, T_thresh = rays.shape[0], 1e-4
    w, ws, dp, im, used = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, alpha_mode)
    assert used[4] == 1 and used[5] == 31 and used[3] == 63 and used[6] == 1024 and used[0] == 0 and used[-1] == 0
    ts_, tc = dev(sig).requires_grad_(True), dev(rgb).requires_grad_(True)
    gw, gws, gdp, gim = RM.composite_rays_train(ts_, tc, dev(ts), dev(rays), T_thresh, alpha_mode)
    assert same(host(gw), w) and same(host(gws), ws) and same(host(gdp), dp) and same(host(gim), im)
    last = slice(int(rays[-1, 0]), M)
    assert ws[-1] == 0 and dp[-1] == 0 and (im[-1] == 0).all() and (host(gw)[last] == 0).all()               # offset + n > M: outputs 0, weights left at 0
    rng = np.random.default_rng(3)
    cot = [rng.normal(size=s).astype(np.float32) for s in ((M,), (N,), (N,), (N, 3))]
    assert all((np.abs(c) > 0).all() for c in cot)                          # non-zero cotangents on all four outputs
    torch.autograd.backward([gw, gws, gdp, gim], [dev(c) for c in cot])
    gs, gc = R.composite_rays_train_backward(cot[0], cot[1], cot[2], cot[3], sig, rgb, ts, rays, ws, dp, im, T_thresh, alpha_mode)
    assert same(host(ts_.grad), gs) and same(host(tc.grad), gc)
    assert (gs[last] == 0).all() and (gc[last] == 0).all() and np.isfinite(gs[:int(rays[10, 0])]).all() and np.abs(gs).max() > 0


def test_composite_rays_train_takes_half_inputs_like_the_reference(RM):
    """The reference casts under custom_fwd(cast_inputs=torch.float32): a half sigma is composited as its float value and receives a half gradient."""
    sig, rgb, ts, rays, M = train_composite_inputs(False)
    sig = np.where(np.isfinite(sig), np.minimum(sig, 6e4), 6e4).astype(np.float16)
    h = dev(sig).requires_grad_(True)
    f = dev(sig.astype(np.float32)).requires_grad_(True)
    outs_h = RM.composite_rays_train(h, dev(rgb), dev(ts), dev(rays), 1e-4, False)
    outs_f = RM.composite_rays_train(f, dev(rgb), dev(ts), dev(rays), 1e-4, False)
    assert all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(outs_h, outs_f))
    outs_h[3].sum().backward(); outs_f[3].sum().backward()
    assert h.grad.dtype == torch.float16 and torch.equal(h.grad, f.grad.half())


# ---------------------------------------------------------------------------------------------------------------- DensityGrid
def cameras():
    """5 cameras looking at the origin, two of them from BEHIND the scene looking away (their forward axis points off it), per-camera intrinsics and near / far."""
    poses = np.zeros((5, 4, 4), np.float32)
    eyes = np.array([[0, 0, 3.0], [2.5, 0.5, 1.0], [-1.0, 2.8, 0.6], [0, 0, 3.0], [3.0, 0.2, 0.1]])
    for b, e in enumerate(eyes):
        fwd = -e / np.linalg.norm(e)
        if b >= 3:
            fwd = -fwd                                                       # looks away: nothing of the scene is in front of it
        right = np.cross(fwd, [0.0, 1.0, 0.1]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        poses[b, :3, 0], poses[b, :3, 1], poses[b, :3, 2], poses[b, :3, 3] = right, up, -fwd, e      # the camera looks down -z
        poses[b, 3, 3] = 1
    K = np.array([[300, 300, 60, 60], [400, 380, 50, 70], [250, 260, 64, 64], [300, 300, 200, 200], [300, 300, 200, 200]], np.float32)
    nf = np.array([[2.6, 6], [2.2, 6], [2.9, 6], [0.1, 6], [0.1, 6]], np.float32)
    return poses, K, nf


def test_mark_untrained_equals_the_restatement(S0):
    H, bound = 16, 2.0
    poses, K, nf = cameras()
    aabb = np.array([-2, -2, -1.5, 2, 1.2, 2], np.float32)
    for kw, ref_kw in ((dict(cam_near_far=dev(nf)), dict(cam_near_far=nf)), (dict(), dict())):
        G = S0.DensityGrid(bound=bound, grid_size=H)
        assert G.cascade == 2 and tuple(G.density_grid.shape) == (2, H ** 3)
        G.density_grid.fill_(0.5)
        n = G.mark_untrained(dev(poses), dev(K), dev(aabb), 0.35, **kw)
        want = R.mark_untrained(np.full((2, H ** 3), 0.5, np.float32), H, bound, poses, K, aabb, 0.35, **ref_kw)
        g = host(G.density_grid)
        assert np.array_equal(g == -1, want) and (g[~want] == 0.5).all() and n == want.sum() and 0.05 < want.mean() < 0.95
    only_behind = S0.DensityGrid(bound=bound, grid_size=H)
    assert only_behind.mark_untrained(dev(poses[3:]), dev(K[3:]), dev(aabb), 0.35) == 2 * H ** 3      # cameras that look away cover nothing


def unfused_update(S0, field, grid, noise, H, bound, decay):
    """The composition the fused kernel replaces: the points in torch in the stated order, field.density, torch.maximum under the validity mask."""
    Cn = grid.shape[0]
    coords = torch.from_numpy(R.morton3D_invert(np.arange(H ** 3, dtype=np.int32))).cuda()
    # 2 i / (H - 1) - 1 with an IEEE division: the divisor is a device tensor, since torch may turn a division by a Python number into a product with its reciprocal
    xyzs = 2 * coords.float() / torch.tensor(float(H - 1), device="cuda") - 1
    out = grid.clone()
    for cas in range(Cn):
        b = min(2 ** cas, bound)
        hgs = b / H
        p = xyzs * (b - hgs)
        p = p + (noise[cas] * 2 - 1) * hgs
        sig = field.density(p)
        valid = (grid[cas] >= 0) & (sig >= 0)
        out[cas][valid] = torch.maximum(grid[cas][valid] * decay, sig[valid])
    return out


@pytest.mark.parametrize("which", ["synthetic", "random"])
def test_density_grid_update_equals_the_unfused_composition(S0, RM, which):
    H = 16
    if which == "synthetic":
        ck = S0.synthetic_checkpoint(S=H)
        field = S0.DensityField.from_checkpoint(ck, bound=1.0)
        G = S0.DensityGrid.from_checkpoint(ck, bound=1.0)
        bound = 1.0
    else:
        from test_gpu_density import Config
        field = Config(S0, 14, 102).field                                    # a seeded random network, evaluated with its own bound 1 on a 2-cascade grid
        bound = 2.0
        G = S0.DensityGrid(bound=bound, grid_size=H)
        G.density_grid.copy_(torch.rand(2, H ** 3, device="cuda") * 3)
    Cn = G.cascade
    assert Cn == (1 if which == "synthetic" else 2) and G.grid_size == H
    G.density_grid[:, 5:300:7] = -1.0
    dead = host(G.density_grid) == -1
    rng = np.random.default_rng(6)
    noise = dev(rng.random((Cn, H ** 3, 3)).astype(np.float32))
    before = G.density_grid.clone()
    for it in (1, 2):                                                        # the second update decays and re-maximises what the first left
        want = unfused_update(S0, field, before, noise, H, bound, 0.95)
        assert G.update(field, decay=0.95, noise=noise) is None
        got = G.density_grid
        assert same(host(got), host(want)) and (host(got)[dead] == -1).all() and (host(got)[~dead] >= 0).all()
        assert G.iter_density == it and G.mean_density == torch.mean(got.clamp(min=0)).item()
        assert torch.equal(G.density_bitfield, RM.packbits(got, min(G.mean_density, G.density_thresh)))
        assert np.array_equal(host(G.density_bitfield), R.packbits(host(got), min(G.mean_density, G.density_thresh)))
        before = got.clone()
    G.update(field)                                                          # noise=None draws torch.rand
    assert G.iter_density == 3


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_the_synthetic_checkpoint():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import dev_raymarch_time as T
    report = T.end_to_end_check()
    print(report)
