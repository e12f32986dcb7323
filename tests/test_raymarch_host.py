"""CPU: the stage-0 ray-marching operators without a device.  tests/raymarch_refs.py (the numpy float32 restatement the device tests compare against bit for bit) is
held to answers that do not come from itself — Morton codes, the slab formula, step counts on full / empty / one-cell grids, cascades, contraction, the closed form of
compositing — its float64 run to autograd of an independent cumprod implementation, its float32 run to the float64 one within a DERIVED bound; csrc/device_march.hpp,
compiled for the host by the library's compiler, is compared with the restatement bit for bit on the device tests' inputs, the hostile ones included, under an iteration
cap (the termination guards are exercised HERE, not on the device); and the Python wrappers refuse bad arguments before they touch a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raymarch_refs as R      # noqa: E402

F = np.float32


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """Bit for bit; two NaNs count as equal whatever their sign and payload (IEEE 754 leaves both to the implementation)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    eq = bits_of(a) == bits_of(b)
    if a.dtype == np.float32:
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_morton_known_values_and_round_trip():
    assert R.morton3D([[1, 0, 0], [0, 1, 0], [0, 0, 1], [127, 127, 127]]).tolist() == [1, 2, 4, 2097151]
    idx = np.arange(128 ** 3, dtype=np.int32)
    c = R.morton3D_invert(idx)
    assert c.min() == 0 and c.max() == 127 and np.array_equal(R.morton3D(c), idx)
    assert len(np.unique(c.astype(np.int64) @ np.array([1, 128, 128 * 128]))) == 128 ** 3


def _slab64(o, d, lo, hi):
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    a, b = np.fmin(t0, t1), np.fmax(t0, t1)
    return np.nanmax(a, axis=1), np.nanmin(b, axis=1)


def test_near_far_against_the_slab_formula():
    o = np.array([[-3, 0.2, 0.1], [0.3, -4, 0.1], [0.1, 0.2, 5], [2, 2, 2], [-2, -3, 1.5], [0.1, 0.1, 0.1], [-3, 2, 0]], np.float32)
    d = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [-1, -1, -1], [2, 3, -1.5], [0.5, 0.2, -0.1], [1, 0, 0]], np.float32)
    d[3] /= np.sqrt(3).astype(np.float32)
    near, far = R.near_far_from_aabb(o, d, [-1, -1, -1, 1, 1, 1], 0.05)
    wn, wf = _slab64(o, d, -1.0, 1.0)
    hit = wn <= wf
    assert hit.tolist() == [True] * 6 + [False]
    assert np.allclose(near[:5], wn[:5], rtol=4 * R.U, atol=0) and np.allclose(far[:6], wf[:6], rtol=4 * R.U, atol=0)
    assert near[5] == F(0.05) and wn[5] < 0                                   # from inside: min_near
    assert near[6] == R.FLT_MAX and far[6] == R.FLT_MAX                       # a miss: both FLT_MAX
    near2, _ = R.near_far_from_aabb(o, d, [-1, -1, -1, 1, 1, 1], 2.5)
    assert near2[0] == F(2.5) and near2[2] == near[2] == F(4.0)               # min_near lifts a nearer entry only


def _axis_rays(n, bound=1.0):
    """n parallel rays along +x through the cube, entering at x = -bound."""
    rng = np.random.default_rng(4)
    o = np.stack([np.full(n, -2.0 * bound), rng.uniform(-0.8, 0.8, n) * bound, rng.uniform(-0.8, 0.8, n) * bound], 1).astype(np.float32)
    d = np.tile(np.array([[1, 0, 0]], np.float32), (n, 1))
    near, far = R.near_far_from_aabb(o, d, [-bound] * 3 + [bound] * 3, 0.2)
    return o, d, near, far


@pytest.mark.parametrize("max_steps", [64, 1024])
def test_full_grid_takes_dt_min_steps(max_steps):
    H = 16
    o, d, near, far = _axis_rays(8)
    bits = R.grid_bits("full", H, 1)
    xyzs, dirs, ts, rays, trips = R.march_rays_train(o, d, 1.0, False, bits, 1, H, near, far, np.zeros(8, np.float32), 0.0, max_steps)
    dt_min = F(2) * R.SQRT3 / F(max_steps)
    assert abs(float(dt_min) - 2 * np.sqrt(3) / max_steps) < 1e-7 and (ts[:, 1] == dt_min).all()
    for n in range(8):
        t, k, run = near[n], 0, []
        while t < far[n] and k < max_steps:                                   # the number of t_k = near + k dt_min (summed in float32) below far, capped
            t = F(t + dt_min); run.append(t); k += 1
        assert rays[n, 1] == k and rays[n, 0] == sum(int(c) for c in rays[:n, 1])
        assert np.array_equal(ts[rays[n, 0]:rays[n, 0] + k, 0], np.array(run, np.float32))
        assert abs(k - min(max_steps, int(np.ceil((float(far[n]) - float(near[n])) / float(dt_min))))) <= 1
    assert (trips == rays[:, 1]).all() and same(dirs, np.repeat(d, rays[:, 1], 0))


def test_empty_grid_skips_whole_cells():
    H = 16
    o, d, near, far = _axis_rays(8)
    xyzs, dirs, ts, rays, trips = R.march_rays_train(o, d, 1.0, False, R.grid_bits("empty", H, 1), 1, H, near, far, np.zeros(8, np.float32), 0.0, 1024)
    assert xyzs.shape == (0, 3) and (rays == 0).all()
    dt_min = 2 * np.sqrt(3) / 1024
    small = np.ceil(2.0 / dt_min)                                             # what stepping dt_min through the cube costs
    # 16 cells of 36.96 dt_min each: one outer pass per cell entered plus the skipping passes; every skip ends at or just past a cell face, so the outer passes
    # number 16 (17 when a face is re-entered by rounding), nowhere near one per dt_min
    assert (trips >= small).all() and (trips <= small + 2 * H + 2).all()
    outer = trips - np.floor((far - near) / dt_min)
    assert (outer >= H - 1).all() and (outer <= 2 * H + 2).all()


def test_one_occupied_cell_and_every_sample_inside_it():
    H = 16
    cell = np.array(R.single_cell_coords(H))
    lo, hi = cell / H * 2.0 - 1.0, (cell + 1) / H * 2.0 - 1.0
    rng = np.random.default_rng(9)
    tgt = rng.uniform(lo, hi, size=(64, 3))
    o = rng.normal(size=(64, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * 2.5
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    near, far = R.near_far_from_aabb(o, d, [-1] * 3 + [1] * 3, 0.2)
    xyzs, dirs, ts, rays, trips = R.march_rays_train(o, d, 1.0, False, R.grid_bits("single", H, 1), 1, H, near, far, np.zeros(64, np.float32), 0.0, 1024)
    assert (rays[:, 1] > 0).sum() >= 60 and len(xyzs) > 500
    assert ((xyzs >= lo - 1e-6) & (xyzs <= hi + 1e-6)).all()
    # the sample is the point BEFORE the step: o + (t - dt) d
    back = np.repeat(o, rays[:, 1], 0) + (ts[:, :1] - ts[:, 1:]) * dirs
    assert np.abs(back - xyzs).max() < 1e-5


def test_second_cascade_serves_the_samples_beyond_the_unit_cube():
    H, Cn, bound = 16, 2, 2.0
    occ = np.zeros((Cn, H ** 3), np.float32)
    occ[1] = 1.0                                                              # cascade 1 full, cascade 0 empty
    bits = R.packbits(occ, 0.5)
    o, d, near, far = _axis_rays(16, bound)
    xyzs, dirs, ts, rays, trips = R.march_rays_train(o, d, bound, False, bits, Cn, H, near, far, np.zeros(16, np.float32), 0.0, 1024)
    linf = np.abs(xyzs).max(1)
    assert len(xyzs) > 1000 and (linf >= 1.0).all() and linf.max() <= 2.0      # nothing from inside [-1, 1]^3, where cascade 0 (empty) is asked
    occ[:] = 0; occ[0] = 1.0
    x0 = R.march_rays_train(o, d, bound, False, R.packbits(occ, 0.5), Cn, H, near, far, np.zeros(16, np.float32), 0.0, 1024)[0]
    assert len(x0) > 300 and (np.abs(x0).max(1) <= 1.0).all()


def test_contraction_emits_outside_samples_whatever_the_grid_says():
    H, Cn, bound = 16, 2, 2.0
    o, d, near, far = _axis_rays(16, bound)
    xyzs, dirs, ts, rays, trips = R.march_rays_train(o, d, bound, True, R.grid_bits("empty", H, Cn), Cn, H, near, far, np.zeros(16, np.float32), 0.0, 64)
    assert len(xyzs) > 100
    t0 = ts[:, 0] - ts[:, 1]
    raw = np.repeat(o, rays[:, 1], 0).astype(np.float64) + t0[:, None].astype(np.float64) * dirs
    mag = np.abs(raw).max(1)
    assert (mag > 1.0 - 1e-6).all()                                           # only points outside the unit cube are emitted from an empty grid
    want = raw * ((2.0 - 1.0 / mag) / mag)[:, None]
    assert np.abs(want - xyzs).max() < 1e-5 and np.abs(xyzs).max() <= 1.5 + 1e-6   # contracted: |x|inf = 2 - 1 / mag <= 1.5 at bound 2


@pytest.mark.parametrize("sigma,dt,n", [(3.0, 0.01, 50), (40.0, 0.004, 200), (0.5, 0.02, 7)])
def test_compositing_constant_sigma_closed_form(sigma, dt, n):
    sig = np.full(n, sigma, np.float32); ts = np.stack([0.5 + dt * np.arange(1, n + 1), np.full(n, dt)], 1).astype(np.float32)
    rgb = np.ones((n, 3), np.float32); rays = np.array([[0, n]], np.int32)
    w, ws, dp, im, used = R.composite_rays_train_forward(sig, rgb, ts, rays, 0.0, False)
    want = 1.0 - np.exp(-float(F(sigma)) * float(F(dt)) * n)
    bound = R.composite_error_bound(sig, ts, rays, False)[0]
    print("constant sigma: weights_sum %.9g, closed form %.9g, error %.3g, bound %.3g" % (ws[0], want, abs(ws[0] - want), bound))
    assert used[0] == n and abs(float(ws[0]) - want) <= bound and same(im[0], np.repeat(ws, 3))


# ---------------------------------------------------------------------------------------------------------------- compositing: adjoint and error
def composite_inputs(seed, alpha_mode, N=24, hostile=False):
    """Rays of lengths 0, 1, 2 and random ones, one with offset + n > M, alphas in [0, 0.9]; with `hostile`, sigma = 0 and sigma = +inf samples."""
    rng = np.random.default_rng(seed)
    counts = np.concatenate([[0, 1, 2, 40], rng.integers(3, 30, N - 5), [9]])
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts[:-1].sum()) + 4                                            # the last ray's span leaves [0, M)
    rays = np.stack([offs, counts], 1).astype(np.int32)
    dt = rng.uniform(0.005, 0.02, M)
    alpha = rng.uniform(0.0, 0.9, M)
    alpha[offs[3]:offs[3] + 40] = rng.uniform(0.0, 0.05, 40)                  # a ray T_thresh never cuts
    sig = alpha if alpha_mode else -np.log1p(-alpha) / dt
    if hostile:
        sig[offs[5] + 1] = 0.0; sig[offs[6] + 2] = np.inf if not alpha_mode else 1.0
    ts = np.stack([1.0 + np.cumsum(dt) * 0.1, dt], 1)
    rgb = rng.uniform(0, 1, (M, 3))
    return sig.astype(np.float32), rgb.astype(np.float32), ts.astype(np.float32), rays, M


@pytest.mark.parametrize("alpha_mode", [False, True])
def test_backward_is_the_adjoint_of_the_cumprod_implementation(alpha_mode):
    """The float64 run of the restatement's backward against autograd.  grad_weights is non-zero but CONSTANT along a ray: the reference adds the sample's
    grad_weights to the ray's grad_weights_sum (raymarching.cu:676), which is the adjoint of the weights output exactly when that cotangent does not vary along the
    ray (it multiplies the later samples' weights too)."""
    sig, rgb, ts, rays, M = composite_inputs(21, alpha_mode)
    T_thresh = 1e-2
    N = rays.shape[0]
    rng = np.random.default_rng(5)
    gws, gd, gi = rng.normal(size=N), rng.normal(size=N), rng.normal(size=(N, 3))
    gw_ray = rng.normal(size=N)
    off, cnt, ok = R._spans(rays, M)
    gw = np.zeros(M)
    for n in np.nonzero(ok)[0]:
        gw[off[n]:off[n] + cnt[n]] = gw_ray[n]
    assert (gw != 0).sum() > M // 2
    s64 = torch.tensor(sig.astype(np.float64), requires_grad=True); c64 = torch.tensor(rgb.astype(np.float64), requires_grad=True)
    w, ws, dp, im = R.composite_train_torch64(s64, c64, ts.astype(np.float64), rays, T_thresh, alpha_mode)
    loss = (w * torch.tensor(gw)).sum() + (ws * torch.tensor(gws)).sum() + (dp * torch.tensor(gd)).sum() + (im * torch.tensor(gi)).sum()
    loss.backward()
    fw, fws, fdp, fim, used = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, alpha_mode, dtype=np.float64)
    for a, b in ((fw, w), (fws, ws), (fdp, dp), (fim, im)):
        assert np.abs(a - b.detach().numpy()).max() <= 1e-12
    assert used[0] == 0 and used[-1] == 0 and used[3] == 40 and (used[4:-1] < cnt[4:-1]).any() and (used[1:3] == [1, 2]).all()    # empty, out of range, never cut, cut
    gs, gc = R.composite_rays_train_backward(gw, gws, gd, gi, sig, rgb, ts, rays, fws, fdp, fim, T_thresh, alpha_mode, dtype=np.float64)
    for got, want in ((gs, s64.grad.numpy()), (gc, c64.grad.numpy())):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print("adjoint, alpha_mode %s: max relative difference %.3g" % (alpha_mode, rel))
        assert rel <= 1e-10
    assert (gs[off[-1]:] == 0).all() and (gc[off[-1]:] == 0).all()                  # the ray with offset + n > M has no gradient


@pytest.mark.parametrize("alpha_mode", [False, True])
def test_float32_forward_within_the_derived_bound_of_float64(alpha_mode):
    """The bound is composite_error_bound's derivation (operation counts per step, gamma_k * sum |terms|, mrf_exp's 2 ulp), evaluated on the float64 values.  It covers
    the arithmetic only: a ray is compared when the float64 transmittance stays clear of T_thresh by more than ITS bound k (A + 2) u, so both runs stop at the same
    sample."""
    sig, rgb, ts, rays, M = composite_inputs(33, alpha_mode, N=64)
    T_thresh = 1e-2
    w32, ws32, dp32, im32, used32 = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, alpha_mode)
    w64, ws64, dp64, im64, used64 = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, alpha_mode, dtype=np.float64)
    off, cnt, ok = R._spans(rays, M)
    trunc = rays.copy(); trunc[:, 1] = np.where(ok, used64, rays[:, 1])       # the samples the float64 run used
    clear = ok.copy()
    A = 0.0 if alpha_mode else 5.4
    for n in np.nonzero(ok)[0]:
        sl = slice(off[n], off[n] + cnt[n])
        a = sig[sl].astype(np.float64) if alpha_mode else 1.0 - np.exp(-sig[sl].astype(np.float64) * ts[sl, 1].astype(np.float64))
        T = np.cumprod(1.0 - a)[:used64[n]]
        clear[n] = (np.abs(T - T_thresh) > (np.arange(1, len(T) + 1) * (A + 2.0) * R.U)).all()
    assert clear.sum() >= ok.sum() - 2 and (used32[clear] == used64[clear]).all()
    for name, a32, a64, vals in (("weights_sum", ws32, ws64, None), ("depth", dp32, dp64, ts[:, 0]), ("red", im32[:, 0], im64[:, 0], rgb[:, 0])):
        bound = R.composite_error_bound(sig, ts, trunc, alpha_mode, vals)
        err = np.abs(a32.astype(np.float64) - a64)
        print("%s: max error %.3g, bound there %.3g" % (name, err[clear].max(), bound[clear][err[clear].argmax()]))
        assert (err[clear] <= bound[clear]).all(), name


# ---------------------------------------------------------------------------------------------------------------- the device header, built for the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mirres_csrc_build", os.path.join(ROOT, "mirres-restir_nerf_mesh_amd", "csrc", "build.py"))
    B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)          # the compiler build.py uses
    so = str(tmp_path_factory.mktemp("rmh") / "librmh.so")
    cmd = [B.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "mirres-restir_nerf_mesh_amd", "csrc"), os.path.join(ROOT, "tests", "raymarch_host.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(so)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def host_march(L, o, d, bits, bound, contract, dt_gamma, max_steps, Cn, H, near, far, t_start, noises, num_steps, eps, max_trips):
    N = o.shape[0]
    ns = np.ascontiguousarray(np.broadcast_to(np.asarray(num_steps, np.int64), (N,)))
    cap = int(ns.max())
    out = np.zeros((N, cap, 5), np.float32); steps = np.zeros(N, np.int64); trips = np.zeros(N, np.int64); t_end = np.zeros(N, np.float32)
    arrs = [np.ascontiguousarray(x, np.float32) for x in (o, d, near, far, t_start, noises)]
    bits = np.ascontiguousarray(bits)
    L.rmh_march(C.c_longlong(N), P(arrs[0]), P(arrs[1]), P(bits), C.c_float(bound), int(bool(contract)), C.c_float(dt_gamma), int(max_steps), int(Cn), int(H), P(arrs[2]),
                P(arrs[3]), P(arrs[4]), P(arrs[5]), P(ns), C.c_float(eps), C.c_uint(max_trips), C.c_longlong(cap), P(out), P(steps), P(trips), P(t_end))
    return out, steps, trips, t_end


@pytest.mark.parametrize("shape_i", range(len(R.GRID_SHAPES)))
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_host_build_marches_like_the_restatement(host, kind, shape_i):
    """Every march_rays_train case of the device tests (tests/test_gpu_raymarch.py), hostile rays included: samples, counts, loop passes and the final t, bit for bit,
    all of it under the cap the device tests demand before they launch."""
    for pi in range(len(R.MARCH_PARAMS)):
        c = R.march_train_case(kind, shape_i, pi, 65)
        assert c["trips"].max() <= R.TRIP_CAP
        out, steps, trips, t_end = host_march(host, c["o"], c["d"], c["bits"], c["bound"], c["contract"], c["dt_gamma"], c["max_steps"], c["C"], c["H"], c["nears"],
                                              c["fars"], c["nears"], c["noises"], c["max_steps"], 0.0, R.TRIP_CAP)
        assert np.array_equal(steps, c["rays"][:, 1]) and np.array_equal(trips, c["trips"]), (kind, shape_i, pi)
        keep = np.arange(out.shape[1])[None, :] < steps[:, None]
        flat = out[keep]
        assert same(flat[:, :3], c["xyzs"]) and same(flat[:, 3:5], c["ts"]), (kind, shape_i, pi)
        assert (steps[:R.N_HOSTILE - 1] == 0).all() and (trips[:R.N_HOSTILE - 1] == 0).all()          # zero direction, NaN near: no pass at all


@pytest.mark.parametrize("N", [1, 63, 64, 2048])
def test_host_build_marches_the_other_ray_counts(host, N):
    """The remaining march_rays_train launches of the device tests (test_march_rays_train_ray_counts_and_repeatability; N = 65 is covered above)."""
    for kind, shape_i, pi in (("random", 1, 0), ("random", 1, 15), ("random", 0, 1)):
        c = R.march_train_case(kind, shape_i, pi, N)
        assert c["trips"].max() <= R.TRIP_CAP
        out, steps, trips, t_end = host_march(host, c["o"], c["d"], c["bits"], c["bound"], c["contract"], c["dt_gamma"], c["max_steps"], c["C"], c["H"], c["nears"],
                                              c["fars"], c["nears"], c["noises"], c["max_steps"], 0.0, R.TRIP_CAP)
        assert np.array_equal(steps, c["rays"][:, 1]) and np.array_equal(trips, c["trips"]), (N, pi)
        flat = out[np.arange(out.shape[1])[None, :] < steps[:, None]]
        assert same(flat[:, :3], c["xyzs"]) and same(flat[:, 3:5], c["ts"]), (N, pi)


def test_host_build_marches_the_inference_loop_like_the_restatement(host):
    """The march_rays form of the marcher — 1 / (d + 1e-10f), the start at rays_t, n_step samples per ray and round — on every round of the device tests' inference
    loop (R.infer_case: the rays with the hostile ones), bit for bit and under the cap, before tests/test_gpu_raymarch.py sends those rounds to the device."""
    c = R.infer_case()
    o, d, nears, fars = c["o"], c["d"], c["nears"], c["fars"]
    assert len(c["rounds"]) >= 4
    saw_hostile = False
    for r in c["rounds"]:
        j = r["rays_alive"].astype(np.int64)
        n_alive, n_step = r["n_alive"], r["n_step"]
        assert r["trips"].max() <= R.TRIP_CAP
        out, steps, trips, t_end = host_march(host, o[j], d[j], c["bits"], 1.0, False, 0.0, c["max_steps"], 1, c["H"], nears[j], fars[j], r["rays_t"][j],
                                              np.zeros(n_alive, np.float32), n_step, 1e-10, R.TRIP_CAP)
        assert np.array_equal(trips, r["trips"])
        assert same(out[..., :3].reshape(-1, 3), r["xyzs"]) and same(out[..., 3:5].reshape(-1, 2), r["ts"])
        filled = np.arange(n_step)[None, :] < steps[:, None]
        assert same(np.where(filled[..., None], d[j][:, None, :], F(0)).reshape(-1, 3).astype(np.float32), r["dirs"])
        hostile = j < R.N_HOSTILE
        if hostile.any():
            saw_hostile = True
            assert (steps[hostile & (j < 2)] == 0).all() and (trips[hostile & (j < 2)] == 0).all()      # zero direction, NaN near: no pass; they leave after round one
    assert saw_hostile and (c["rounds"][0]["rays_alive"][:R.N_HOSTILE] == np.arange(R.N_HOSTILE)).all()
    assert (c["rounds"][0]["alive_after"][:R.N_HOSTILE] == -1).all()


def test_termination_guards_under_the_cap(host):
    """A zero direction, a NaN near, a NaN far, an infinite direction: no pass.  An origin at 1e7 with a finite far: t + dt == t at once — on an empty grid the ray ends
    after one outer pass (the reference spins for ever), on a full grid it takes max_steps samples with t standing still.  A finite far beyond the absorption point
    (dt_gamma 0): t is absorbed only after ~2^21 / dt_min passes, far beyond what a test may spend, so there the CAP ends it — in both implementations alike."""
    H, cap = 16, 4000
    o = np.array([[0, 0, -3], [0, 0, -3], [0, 0, -3], [0, 0, -3], [1e7, 0, 0], [0, 0, -3]], np.float32)
    d = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 1], [0, np.inf, 1], [-1, 0, 0], [0, 0, 1]], np.float32)
    near = np.array([2, np.nan, 2, 2, 1e7 - 1, 2], np.float32); far = np.array([4, 4, np.nan, 4, 1e7 + 1, 3e38], np.float32)
    z = np.zeros(6, np.float32)
    for kind, want_steps in (("empty", [0, 0, 0, 0, 0, 0]), ("full", [0, 0, 0, 0, 64, 64])):
        bits = R.grid_bits(kind, H, 1)
        ref = R._march(o, d, bits, 1.0, False, 0.0, 64, 1, H, near, far, near, z, 64, 0.0, cap)
        got = host_march(host, o, d, bits, 1.0, False, 0.0, 64, 1, H, near, far, near, z, 64, 0.0, cap)
        assert got[1].tolist() == want_steps and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and same(got[3], ref[3]) and same(got[0], ref[0])
        assert (got[2][:4] == 0).all() and got[2][4] == (1 if kind == "empty" else 64)
        if kind == "empty":
            assert cap <= got[2][5] <= cap + 1                                 # only the cap ends this one in reasonable time: such a far never reaches the device tests
            assert got[3][4] == near[4]                                       # t never moved


def test_host_build_composites_like_the_restatement(host):
    for alpha_mode in (False, True):
        sig, rgb, ts, rays, M = composite_inputs(8, alpha_mode, N=40, hostile=True)
        N = rays.shape[0]
        w, ws, dp, im, used = R.composite_rays_train_forward(sig, rgb, ts, rays, 1e-2, alpha_mode)
        hw = np.zeros(M, np.float32); hws = np.zeros(N, np.float32); hdp = np.zeros(N, np.float32); him = np.zeros((N, 3), np.float32)
        host.rmh_composite_train_fwd(P(sig), P(rgb), P(ts), P(rays), C.c_longlong(M), C.c_longlong(N), C.c_float(1e-2), int(alpha_mode), P(hw), P(hws), P(hdp), P(him))
        assert same(hw, w) and same(hws, ws) and same(hdp, dp) and same(him, im)
        rng = np.random.default_rng(2)
        g = [rng.normal(size=s).astype(np.float32) for s in ((M,), (N,), (N,), (N, 3))]
        gs, gc = R.composite_rays_train_backward(g[0], g[1], g[2], g[3], sig, rgb, ts, rays, ws, dp, im, 1e-2, alpha_mode)
        hgs = np.zeros(M, np.float32); hgc = np.zeros((M, 3), np.float32)
        host.rmh_composite_train_bwd(P(g[0]), P(g[1]), P(g[2]), P(g[3]), P(sig), P(rgb), P(ts), P(rays), P(ws), P(dp), P(im), C.c_longlong(M), C.c_longlong(N),
                                     C.c_float(1e-2), int(alpha_mode), P(hgs), P(hgc))
        assert same(hgs, gs) and same(hgc, gc)
        # inference: 8 rays x 4 slots, one slot left empty by the marcher (ts == 0), one ray id out of range
        n_alive, n_step = 8, 4
        alive = np.array([3, 1, 7, 0, 99, 5, 2, 6], np.int32)
        s2, c2, t2 = sig[:32].copy(), rgb[:32].copy(), ts[:32].copy()
        t2[9] = 0
        st = [np.zeros(10, np.float32), rng.uniform(0, 0.3, 10).astype(np.float32), rng.uniform(0, 1, 10).astype(np.float32), rng.uniform(0, 1, (10, 3)).astype(np.float32)]
        want = R.composite_rays(n_alive, n_step, alive, st[0], s2, c2, t2, st[1], st[2], st[3], 1e-2, alpha_mode)
        ha, ht, hws2, hdp2, him2 = alive.copy(), st[0].copy(), st[1].copy(), st[2].copy(), st[3].copy()
        host.rmh_composite(C.c_longlong(n_alive), n_step, C.c_longlong(10), C.c_float(1e-2), int(alpha_mode), P(ha), P(ht), P(s2), P(c2), P(t2), P(hws2), P(hdp2), P(him2))
        assert np.array_equal(ha, want[0]) and same(ht, want[1]) and same(hws2, want[2]) and same(hdp2, want[3]) and same(him2, want[4])
        assert ha[4] == -1 and ha[2] == -1 and (ha >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- what may reach the reference's own kernels
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_reference_gate_passes_every_case_without_hostile_rays_and_stops_the_hostile_ones(kind):
    """tests/test_gpu_ref_raymarch.py launches the reference's marchers, whose loops have no termination guard, only on inputs for which R.reference_loops_end — the
    restatement with the product-only guards off — shows every ray to end within TRIP_CAP passes.  Without the hostile rays that holds for every case of
    GRID_KINDS x GRID_SHAPES x MARCH_PARAMS at 65 rays, so the device test leaves none out.
    With them, the gate rejects hostile rows and nothing else: the zero direction (row 0: the distance to the next voxel is +inf) and the origin at 1e7 (row 2:
    t + dt == t) wherever they meet an empty cell — both on an empty grid marched without contraction, neither on a full grid, where they take max_steps samples
    and end, in the reference too.  The NaN near (row 1) is never rejected: `NaN < far` is false, so the reference's loop ends before its first pass (no sample);
    it is kept from the reference by hostile=False all the same."""
    for shape_i in range(len(R.GRID_SHAPES)):
        for pi in range(len(R.MARCH_PARAMS)):
            assert R.train_case_loops_end(R.march_train_case(kind, shape_i, pi, 65, False)).all(), (kind, shape_i, pi)
    for shape_i, pi in ((0, 0), (1, 5), (2, 10), (3, 15), (0, 3), (3, 8)):
        c = R.march_train_case(kind, shape_i, pi, 65, True)
        rejected = np.nonzero(~R.train_case_loops_end(c))[0].tolist()
        assert set(rejected) <= {0, 2} and c["rays"][1, 1] == 0, (kind, shape_i, pi, rejected)
        if kind == "full":
            assert rejected == [], (shape_i, pi, rejected)
        if kind == "empty" and not R.MARCH_PARAMS[pi]["contract"]:
            assert rejected == [0, 2], (shape_i, pi, rejected)


def test_reference_gate_on_the_other_ray_counts_and_the_inference_loop():
    """The remaining reference launches of tests/test_gpu_ref_raymarch.py pass the gate; the device tests' inference case WITH the hostile rays does not (row 2)."""
    for N in (1, 63, 64, 2048):
        for pi in (0, 15):
            assert R.train_case_loops_end(R.march_train_case("random", 1, pi, N, False)).all()
    c = R.infer_case(hostile=False)
    assert all(R.infer_round_loops_end(c, r).all() for r in c["rounds"]) and len(c["rounds"]) >= 4
    ch = R.infer_case()
    ends = R.infer_round_loops_end(ch, ch["rounds"][0])
    assert not ends[2] and ends[R.N_HOSTILE:].all()


def test_restatement_equals_what_the_reference_kernels_wrote():
    """tests/golden/ref_raymarch.npz holds what the reference's own march_rays_train and near_far_from_aabb kernels computed on an MI355X (tests/golden/
    gen_ref_raymarch.py): samples per ray and a SHA-256 of xyzs / dirs / ts in ray order for every 65-ray case with max_steps 64.  The restatement — which the host
    build of device_march.hpp and the device kernels are held to bit for bit — must reproduce them; this runs where neither a GPU nor the reference tree exists."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_raymarch.npz"))
    cases = R.golden_cases()
    assert np.array_equal(g["cases"], np.array(cases, np.int32)) and len(cases) == 128
    for i, (k, s, p) in enumerate(cases):
        c = R.march_train_case(R.GRID_KINDS[k], s, p, 65, False)
        assert np.array_equal(c["rays"][:, 1], g["counts"][i]), cases[i]
        for j, name in enumerate(("xyzs", "dirs", "ts")):
            assert np.array_equal(R.digest(c[name]), g["sha"][i, j]), (cases[i], name)
    assert g["counts"].sum() > 100000
    o, d, aabb = R.near_far_inputs()
    near, far = R.near_far_from_aabb(o, d, aabb, 0.2)
    assert np.array_equal(R.digest(near), g["near_far_sha"][0]) and np.array_equal(R.digest(far), g["near_far_sha"][1])


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_compositing_inputs_of_the_reference_comparison_stay_clear_of_the_threshold(T_thresh):
    """tests/test_gpu_ref_raymarch.py compares sample counts exactly except for rays whose float64 transmittance comes within a relative 1e-5 of T_thresh; by the
    float64 computation alone that leaves out at most 2 % of the rays of each input set."""
    sets = [R.train_composite_inputs(False) + (False,), R.train_composite_inputs(True) + (True,), R.constant_sigma_rays() + (False,)]
    for sig, rgb, ts, rays, M, am in sets:
        near = R.transmittance_near_threshold(sig, ts, rays, T_thresh, am)
        print("alpha_mode %s, T_thresh %g: %d of %d rays near the threshold" % (am, T_thresh, near.sum(), rays.shape[0]))
        assert near.sum() <= 0.02 * rays.shape[0]


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_composite_rays_float64_and_its_bound_on_the_stand_alone_sets(T_thresh):
    """R.composite_rays_sets, the inputs of the device comparison of composite_rays with the reference kernel: by float64 alone at most 2 % of the rays come near
    T_thresh; away from it the float32 restatement ends the same rays, leaves the same rays_t and stays within composite_rays_float64's derived bound; rays end by
    opacity, by an empty slot, and go on."""
    for name, am, n, ns, alive, rays_t, sig, rgb, ts, ws, dp, im in R.composite_rays_sets():
        acc, stays, t64, near, bound = R.composite_rays_float64(ns, alive, ws, dp, im, sig, rgb, ts, T_thresh, bool(am))
        assert near.sum() <= 0.02 * n and 0 < stays.sum() < n
        a2, t2, ws2, dp2, im2 = R.composite_rays(n, ns, alive, rays_t, sig, rgb, ts, ws, dp, im, T_thresh, bool(am))
        ok = ~near
        assert np.array_equal(a2[:n][ok] >= 0, stays[ok]) and same(t2[alive][ok & stays], t64[ok & stays].astype(np.float32)) and same(t2[alive][~stays], rays_t[alive][~stays])
        got = np.stack([im2[alive, 0], im2[alive, 1], im2[alive, 2], ws2[alive], dp2[alive]], 1).astype(np.float64)
        err = np.abs(got - acc)
        print("%s, T_thresh %g: %d of %d rays stay; largest error %s, bound %s" % (name, T_thresh, stays.sum(), n, err[ok].max(0), bound[ok].max(0)))
        assert (err[ok] <= bound[ok]).all() and np.isfinite(bound).all()
        wider = R.composite_rays_float64(ns, alive, ws, dp, im, sig, rgb, ts, T_thresh, bool(am), exp_ulps=(2.0, 1.0))[4]
        assert (wider >= bound).all() and ((wider > bound).any() != bool(am))
        if name != "constant":
            empty_slot = (ts.reshape(n, ns, 2)[:, :, 0] == 0).any(1)
            assert empty_slot.sum() > 20 and not stays[empty_slot].any()


def test_error_bound_constant_for_another_exponential():
    """composite_error_bound's exp_ulps: the default is today's constant; a larger or growing error widens the bound, never narrows it."""
    sig, rgb, ts, rays, M = composite_inputs(33, False, N=16)
    b2 = R.composite_error_bound(sig, ts, rays, False)
    assert np.array_equal(b2, R.composite_error_bound(sig, ts, rays, False, exp_ulps=2))
    b3, b21 = R.composite_error_bound(sig, ts, rays, False, exp_ulps=3), R.composite_error_bound(sig, ts, rays, False, exp_ulps=(2.0, 1.0))
    live = b2 > 0
    assert live.sum() >= 10 and (b3[live] > b2[live]).all() and (b21[live] > b2[live]).all() and (b3[~live] == 0).all()
    assert np.array_equal(R.composite_error_bound(sig, ts, rays, True), R.composite_error_bound(sig, ts, rays, True, exp_ulps=(9.0, 9.0)))      # alpha mode: no exponential


# ---------------------------------------------------------------------------------------------------------------- the wrappers' refusals
def test_wrappers_refuse_bad_arguments_before_touching_a_device():
    from mirres_restir_nerf_mesh_amd import raymarching as RM
    H = 16
    bits = torch.zeros(H ** 3 // 8, dtype=torch.uint8)
    o = torch.zeros(4, 3); n = torch.zeros(4)
    ok = dict(rays_o=o, rays_d=o, bound=1.0, contract=False, density_bitfield=bits, C=1, H=H, nears=n, fars=n)
    bad = [(dict(H=12), ValueError, "power of two"), (dict(H=2048), ValueError, "power of two"), (dict(density_bitfield=bits[:-1]), ValueError, "C \\* H\\^3 / 8"),
           (dict(density_bitfield=bits.float()), TypeError, "uint8"), (dict(C=2), ValueError, "C \\* H\\^3 / 8"), (dict(C=0), ValueError, "cascades"),
           (dict(rays_d=torch.zeros(3, 3)), ValueError, "differ"), (dict(rays_o=torch.zeros(4, 2), rays_d=torch.zeros(4, 2)), ValueError, "3-vectors"),
           (dict(nears=torch.zeros(5)), ValueError, "nears"), (dict(fars=torch.zeros(4, 1)), ValueError, "fars"), (dict(rays_o=torch.zeros(4, 3, dtype=torch.int32)), TypeError, "floating"),
           (dict(bound=0.0), ValueError, "bound"), (dict(max_steps=0), ValueError, "max_steps"), (dict(dt_gamma=-1.0), ValueError, "dt_gamma"),
           (dict(noises=torch.zeros(3)), ValueError, "noises")]
    for over, exc, msg in bad:
        with pytest.raises(exc, match=msg):
            RM.march_rays_train(**{**ok, **over})
    alive = torch.arange(4, dtype=torch.int32)
    with pytest.raises(TypeError, match="int32"):
        RM.march_rays(4, 2, alive.long(), n, o, o, 1.0, False, bits, 1, H, n, n)
    with pytest.raises(ValueError, match="n_alive"):
        RM.march_rays(5, 2, alive, n, o, o, 1.0, False, bits, 1, H, n, n)
    with pytest.raises(ValueError, match="n_step"):
        RM.march_rays(4, 0, alive, n, o, o, 1.0, False, bits, 1, H, n, n)
    with pytest.raises(ValueError, match="power of two"):
        RM.march_rays(4, 2, alive, n, o, o, 1.0, False, bits, 1, 24, n, n)
    rays = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="rgbs"):
        RM.composite_rays_train(torch.zeros(6), torch.zeros(5, 3), torch.zeros(6, 2), rays)
    with pytest.raises(ValueError, match="ts"):
        RM.composite_rays_train(torch.zeros(6), torch.zeros(6, 3), torch.zeros(6, 3), rays)
    with pytest.raises(TypeError, match="int32"):
        RM.composite_rays_train(torch.zeros(6), torch.zeros(6, 3), torch.zeros(6, 2), rays.long())
    with pytest.raises(ValueError, match="sigmas"):
        RM.composite_rays(4, 2, alive, n, torch.zeros(7), torch.zeros(8, 3), torch.zeros(8, 2), n.clone(), n.clone(), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="multiple of 8"):
        RM.packbits(torch.zeros(1, 12), 0.5)
    with pytest.raises(ValueError, match="aabb"):
        RM.near_far_from_aabb(o, o, torch.zeros(5))
    with pytest.raises(TypeError, match="integer"):
        RM.morton3D(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="nothing in the reference calls it"):
        RM.sph_from_ray(o, o, 1.0)


def test_density_grid_refusals():
    from mirres_restir_nerf_mesh_amd import stage0
    with pytest.raises(NotImplementedError, match="sdf"):
        stage0.DensityGrid(sdf=True)
    with pytest.raises(NotImplementedError, match="trainable_density_grid"):
        stage0.DensityGrid(trainable_density_grid=True)
    with pytest.raises(ValueError, match="power of two"):
        stage0.DensityGrid(grid_size=48)
    with pytest.raises(ValueError, match="density_grid"):
        stage0.DensityGrid(bound=2.0, grid_size=16, density_grid=torch.zeros(1, 16 ** 3))
    with pytest.raises(ValueError, match="density_bitfield"):
        stage0.DensityGrid(grid_size=16, density_bitfield=torch.zeros(7, dtype=torch.uint8))


def test_entries_refuse_counts_beyond_one_launch_and_name_the_missing_buffer():
    from mirres_restir_nerf_mesh_amd._lib import lib
    L = lib()
    assert L.mirres_rm_near_far(None, None, None, 2 ** 31 + 1, 0.2, None, None, None) < 0 and b"outside [0, 2^31]" in L.mirres_last_error()
    assert L.mirres_rm_packbits(None, 2 ** 38, 0.5, None, None) < 0 and b"outside [0, 2^31]" in L.mirres_last_error()
    assert L.mirres_rm_grid_mark_untrained(None, 1, 16, 1.0, None, 0, None, 0, None, 0.2, None, None) < 0 and b"density grid NULL" in L.mirres_last_error()
    assert L.mirres_rm_march_train_count(None, None, None, 1.0, 0, 0.0, 64, 4, 1, 16, None, None, None, None, None) < 0 and b"bitfield NULL" in L.mirres_last_error()
