"""The stage-0 ray-marching operators against the REFERENCE'S OWN kernels: oracle/_ref/libref_raymarch.so is raymarching/src/raymarching.cu of the reference tree,
compiled by hipcc without contraction (oracle/Makefile `ref`, oracle/ref_raymarch_driver.hip).  tests/test_gpu_raymarch.py holds csrc/raymarch.hip to
tests/raymarch_refs.py, a restatement with the same author as the kernels; this module holds BOTH to the reference's program.  Everything that uses no transcendental
function — near / far, the integer helpers, both marchers — is compared bit for bit (two NaNs count as equal).  The compositors differ by design in the exponential
(mrf_exp for the __expf intrinsic): how many samples each ray uses is compared exactly away from T_thresh, the sums within a derived bound of float64.

The reference's marching loops have no termination guard, so no input reaches them before the restatement, run with the product-only guards off, has shown on the
host that every ray ends by itself within TRIP_CAP loop passes (R.reference_loops_end); the hostile rays of R.make_rays are never sent.  A driver entry that returns
a HIP error ends the whole run: nothing more is launched after a fault."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raymarch_refs as R      # noqa: E402
from test_raymarch_host import same      # noqa: E402
from test_gpu_raymarch import dev, host, run_march_train, sigma_of      # noqa: E402
from oracle import oracle as O      # noqa: E402

REF = O.ref_raymarch_lib()
if REF is None:
    pytest.skip("oracle/_ref/libref_raymarch.so was not built (no reference tree at build time)", allow_module_level=True)

F = np.float32


@pytest.fixture(scope="module")
def RM():
    from mirres_restir_nerf_mesh_amd import raymarching
    return raymarching


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    rc = getattr(REF, name)(*args)
    if rc != 0:
        pytest.exit("oracle/_ref/libref_raymarch.so: %s returned HIP error %d; nothing more is launched" % (name, rc), returncode=3)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------------------------- exact: near / far, integer helpers
def test_near_far_against_the_reference_kernel(RM):
    """The 4096 rays of test_near_far_bit_equal: zero components, -0.0, a miss, origins inside."""
    o, d, aabb = R.near_far_inputs()
    go, gd, ga = dev(o), dev(d), dev(aabb)
    near, far = RM.near_far_from_aabb(go, gd, ga, 0.2)
    rn, rf = zeros(o.shape[0]), zeros(o.shape[0])
    call("ref_near_far_from_aabb", p(go), p(gd), p(ga), o.shape[0], 0.2, p(rn), p(rf))
    wn, wf = R.near_far_from_aabb(o, d, aabb, 0.2)
    assert same(host(rn), host(near)) and same(host(rf), host(far)) and same(host(rn), wn) and same(host(rf), wf)


def test_integer_helpers_against_the_reference_kernels(RM):
    """The inputs of test_integer_helpers_bit_equal; flatten_rays with M equal to the sum of the counts (the reference does not look at M and would write past the
    end of a shorter buffer: the product's skipping of such spans is a declared deviation and is not handed to it)."""
    rng = np.random.default_rng(1)
    coords = rng.integers(0, 1024, size=(5001, 3)).astype(np.int32)
    coords[:3] = [[0, 0, 0], [1023, 1023, 1023], [127, 0, 127]]
    gc = dev(coords)
    ri = zeros(5001, dtype=torch.int32)
    call("ref_morton3D", p(gc), 5001, p(ri))
    assert np.array_equal(host(ri), host(RM.morton3D(gc))) and np.array_equal(host(ri), R.morton3D(coords))
    rc = zeros(5001, 3, dtype=torch.int32)
    call("ref_morton3D_invert", p(ri), 5001, p(rc))
    assert np.array_equal(host(rc), coords) and np.array_equal(host(RM.morton3D_invert(ri)), coords)
    H, Cn, thresh = 16, 2, F(0.37)
    grid = rng.uniform(0, 1, size=(Cn, H ** 3)).astype(np.float32)
    grid[0, :8] = [thresh, np.nextafter(thresh, F(1)), np.nextafter(thresh, F(0)), -1.0, np.nan, np.inf, 0.0, thresh]
    gg = dev(grid)
    nb = Cn * H ** 3 // 8
    rb = torch.full((nb,), 255, dtype=torch.uint8, device="cuda")
    call("ref_packbits", p(gg), nb, float(thresh), p(rb))
    assert np.array_equal(host(rb), host(RM.packbits(gg, float(thresh)))) and np.array_equal(host(rb), R.packbits(grid, thresh)) and host(rb)[0] == 0b00100010
    counts = rng.integers(0, 9, size=700).astype(np.int32); counts[5] = 0
    rays = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1).astype(np.int32)
    M = int(counts.sum())
    gr = dev(rays)
    rr = zeros(M, dtype=torch.int32)                                         # zero-initialised, as the reference's Python does
    call("ref_flatten_rays", p(gr), 700, M, p(rr))
    assert np.array_equal(host(rr), host(RM.flatten_rays(gr, M))) and np.array_equal(host(rr), R.flatten_rays(rays, M))


# ---------------------------------------------------------------------------------------------------------------- exact: march_rays_train
def ref_march_train(c):
    """The reference's two passes the way its raymarching.py drives them (a zeroed counter, pass one with no outputs, M read back, pass two) -> xyzs, dirs, ts, rays."""
    assert R.train_case_loops_end(c).all()                                    # THE GATE: before anything reaches the reference's loops
    N = c["o"].shape[0]
    go, gd, gb, gn, gf, gz = (dev(c[k]) for k in ("o", "d", "bits", "nears", "fars", "noises"))
    rays, counter = zeros(N, 2, dtype=torch.int32), zeros(2, dtype=torch.int32)
    head = (p(go), p(gd), p(gb), float(c["bound"]), int(c["contract"]), float(c["dt_gamma"]), int(c["max_steps"]), N, c["C"], c["H"], p(gn), p(gf))
    call("ref_march_rays_train", *head, None, None, None, p(rays), p(counter), p(gz))
    M = int(counter[0].item())
    r = host(rays)
    assert M == int(r[:, 1].sum()) and (r[:, 1] >= 0).all() and (r[:, 1] <= c["max_steps"]).all()
    order = np.argsort(r[:, 0], kind="stable")
    live = order[r[order, 1] > 0]
    assert np.array_equal(r[live, 0], np.concatenate([[0], np.cumsum(r[live, 1])[:-1]])[:len(live)])      # disjoint spans, in some order, covering [0, M)
    assert ((r[:, 0] >= 0) & (r[:, 0] + r[:, 1] <= M)).all()                  # so pass two stays inside its buffers
    xyzs, dirs, ts = zeros(max(M, 1), 3), zeros(max(M, 1), 3), zeros(max(M, 1), 2)
    call("ref_march_rays_train", *head, p(xyzs), p(dirs), p(ts), p(rays), p(counter), p(gz))
    return host(xyzs)[:M], host(dirs)[:M], host(ts)[:M], r


def in_ray_order(a, rays):
    idx = np.concatenate([np.arange(o, o + n) for o, n in rays] + [np.zeros(0, np.int64)]).astype(np.int64)
    return a[idx]


def check_against_reference(RM, c):
    rx, rd, rt, rr = ref_march_train(c)
    hx, hd, ht, hr = (host(t) for t in run_march_train(RM, c))
    assert np.array_equal(rr[:, 1], hr[:, 1]) and np.array_equal(rr[:, 1], c["rays"][:, 1])
    for ref, hip, want in ((rx, hx, c["xyzs"]), (rd, hd, c["dirs"]), (rt, ht, c["ts"])):
        ref = in_ray_order(ref, rr)
        assert same(ref, in_ray_order(hip, hr)) and same(ref, want)
    return int(rr[:, 1].sum())


@pytest.mark.parametrize("shape_i", range(len(R.GRID_SHAPES)))
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_march_rays_train_against_the_reference_kernel(RM, kind, shape_i):
    """Every parameter set on every grid at 65 rays, none of them hostile, noises passed explicitly; per ray, through each side's own offsets."""
    total = sum(check_against_reference(RM, R.march_train_case(kind, shape_i, pi, 65, False)) for pi in range(len(R.MARCH_PARAMS)))
    if kind == "empty" and R.GRID_SHAPES[shape_i][2] == 1.0:
        assert total == 0                                                    # an empty grid yields samples only through contraction, beyond the unit cube
    if kind == "full":
        assert total > 65 * 16


@pytest.mark.parametrize("N", [1, 63, 64, 2048])
def test_march_rays_train_ray_counts_against_the_reference_kernel(RM, N):
    for pi in (0, 15):
        check_against_reference(RM, R.march_train_case("random", 1, pi, N, False))


# ---------------------------------------------------------------------------------------------------------------- the inference loop
def state_rows(ws, dp, im, idx):
    """(r, g, b, weights_sum, depth) of the rays idx, as float64 rows."""
    ws, dp, im = host(ws), host(dp), host(im)
    return np.stack([im[idx, 0], im[idx, 1], im[idx, 2], ws[idx], dp[idx]], 1).astype(np.float64)


def check_composite_rays(RM, exp_error, n_alive, n_step, rays_alive, rays_t, sig, rgb, ts, ws, dp, im, T_thresh, am, tag):
    """composite_rays of the reference on copies of the state and of the product in place (device tensors), both against R.composite_rays_float64 on the same
    float32 inputs: rays_alive / rays_t exactly, and weights_sum / depth / image within the derived bound (the reference's with the measured error of its __expf, the
    product's with mrf_exp's 2 ulp), for every ray that stays clear of T_thresh.  -> how many rays were left out."""
    idx = host(rays_alive)[:n_alive].astype(np.int64)
    if not am:
        x = host(sig).astype(np.float64) * host(ts)[:, 1]
        assert x[np.isfinite(x)].max() <= exp_error[2]                        # inside the range the exponential's error was measured on
    acc, stays, t64, near, b_hip = R.composite_rays_float64(n_step, idx, host(ws), host(dp), host(im), host(sig), host(rgb), host(ts), T_thresh, bool(am))
    b_ref = R.composite_rays_float64(n_step, idx, host(ws), host(dp), host(im), host(sig), host(rgb), host(ts), T_thresh, bool(am), exp_ulps=exp_error[:2])[4]
    t_before = host(rays_t)
    ra, rtt, rws, rdp, rim = rays_alive.clone(), rays_t.clone(), ws.clone(), dp.clone(), im.clone()
    call("ref_composite_rays", n_alive, n_step, float(T_thresh), int(am), p(ra), p(rtt), p(sig), p(rgb), p(ts), p(rws), p(rdp), p(rim))
    RM.composite_rays(n_alive, n_step, rays_alive, rays_t, sig, rgb, ts, ws, dp, im, T_thresh, bool(am))
    ok = ~near
    ha, ra = host(rays_alive)[:n_alive], host(ra)[:n_alive]
    assert np.array_equal(ha[ok], ra[ok]) and np.array_equal(ra[ok] >= 0, stays[ok]) and (ra[ok][stays[ok]] == idx[ok][stays[ok]]).all(), tag
    want_t = np.where(stays, t64.astype(np.float32), t_before[idx])           # a ray that ended keeps its rays_t
    assert same(host(rtt)[idx[ok]], want_t[ok]) and same(host(rays_t)[idx[ok]], want_t[ok]), tag
    e_ref, e_hip = np.abs(state_rows(rws, rdp, rim, idx) - acc), np.abs(state_rows(ws, dp, im, idx) - acc)
    assert (e_ref[ok] <= b_ref[ok]).all() and (e_hip[ok] <= b_hip[ok]).all(), (tag, e_ref[ok].max(0), b_ref[ok].max(0), e_hip[ok].max(0), b_hip[ok].max(0))
    return int(near.sum()), e_ref[ok].max(0), e_hip[ok].max(0), b_ref[ok].max(0)


def test_inference_loop_against_the_reference_kernels(RM, exp_error):
    """The loop of test_inference_loop_bit_equal without the hostile rays, driven by the product's kernels; in every round the reference's march_rays gets the same
    rays_alive / rays_t (after the gate) and must return the same xyzs / dirs / ts, zero rows included, and the reference's composite_rays, on copies of the
    state, must end the same rays, leave the same rays_t and — like the product's — accumulate weights_sum / depth / image within the derived bound of the round's
    float64 evaluation (check_composite_rays), except rays whose float64 transmittance comes within a relative 1e-5 of T_thresh."""
    c = R.infer_case(hostile=False)
    N, H, max_steps, T_thresh = c["N"], c["H"], c["max_steps"], c["T_thresh"]
    go, gd, gb, gn, gf = dev(c["o"]), dev(c["d"]), dev(c["bits"]), dev(c["nears"]), dev(c["fars"])
    ws, dp, im = zeros(N), zeros(N), zeros(N, 3)
    tcol = dev(R.INFER_COLOUR)
    rays_alive, rays_t, step, rounds, left_out, compared = torch.arange(N, dtype=torch.int32, device="cuda"), gn.clone(), 0, 0, 0, 0
    worst = np.zeros((2, 5))
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        want = c["rounds"][rounds]
        assert np.array_equal(host(rays_alive), want["rays_alive"]) and same(host(rays_t), want["rays_t"])
        assert R.infer_round_loops_end(c, want).all()                         # THE GATE
        xyzs, dirs, ts = RM.march_rays(n_alive, n_step, rays_alive, rays_t, go, gd, 1.0, False, gb, 1, H, gn, gf, False, 0.0, max_steps)
        rx, rd, rt = zeros(n_alive * n_step, 3), zeros(n_alive * n_step, 3), zeros(n_alive * n_step, 2)
        gz = zeros(n_alive)
        call("ref_march_rays", n_alive, n_step, p(rays_alive), p(rays_t), p(go), p(gd), 1.0, 0, 0.0, max_steps, 1, H, p(gb), p(gn), p(gf), p(rx), p(rd), p(rt), p(gz))
        assert same(host(rx), host(xyzs)) and same(host(rd), host(dirs)) and same(host(rt), host(ts)), rounds
        assert same(host(rx), want["xyzs"]) and same(host(rt), want["ts"])
        sig, rgb = sigma_of(xyzs).contiguous(), tcol.expand(n_alive * n_step, 3).contiguous()
        out, e_ref, e_hip, b_ref = check_composite_rays(RM, exp_error, n_alive, n_step, rays_alive, rays_t, sig, rgb, ts, ws, dp, im, T_thresh, 0, rounds)
        worst = np.maximum(worst, np.stack([e_ref, e_hip]))
        left_out += out; compared += n_alive
        rays_alive = rays_alive[rays_alive >= 0]
        step += n_step; rounds += 1
    print("inference loop: %d rounds, %d ray-rounds compared, %d left out near T_thresh; largest per-round error of r, g, b, weights_sum, depth: reference %s, product %s"
          % (rounds, compared, left_out, worst[0], worst[1]))
    assert rounds == len(c["rounds"]) >= 4 and left_out <= 0.02 * N


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_composite_rays_against_the_reference_kernel(RM, exp_error, T_thresh):
    """composite_rays on its own: R.composite_rays_sets (both alpha modes, slots the marcher left empty, a state that starts from non-zero sums, rays_alive a
    permutation into a larger state), both thresholds."""
    for name, am, n_alive, n_step, alive, rays_t, sig, rgb, ts, ws, dp, im in R.composite_rays_sets():
        g = [dev(x.copy()) for x in (alive, rays_t, sig, rgb, ts, ws, dp, im)]
        untouched = np.setdiff1d(np.arange(ws.shape[0]), alive)
        out, e_ref, e_hip, b_ref = check_composite_rays(RM, exp_error, n_alive, n_step, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], T_thresh, am, name)
        print("composite_rays %s, T_thresh %g: %d rays x %d, %d left out, %d stay; largest error of r, g, b, weights_sum, depth: reference %s (bound %s), product %s" %
              (name, T_thresh, n_alive, n_step, out, (host(g[0]) >= 0).sum(), e_ref, b_ref, e_hip))
        assert out <= 0.02 * n_alive and same(host(g[5])[untouched], ws[untouched]) and same(host(g[1])[untouched], rays_t[untouched])
        assert 0 < (host(g[0]) >= 0).sum() < n_alive                         # some rays end, some go on


# ---------------------------------------------------------------------------------------------------------------- compositing
def composite_sets():
    out = [("random-%d" % am, am) + R.train_composite_inputs(bool(am)) for am in (0, 1)]
    return out + [("constant", 0) + R.constant_sigma_rays()]


def measure_fast_exp(X, extra):
    """The reference build's __expf over [-X, 0] (and at the tests' own arguments) against float64 -> (a, b): the error is within a + b |x| ulp at every point tried."""
    x = np.concatenate([-np.linspace(0.0, X, 1 << 20), extra]).astype(np.float32)
    gx, gy = dev(x), zeros(x.shape[0])
    call("ref_fast_exp", p(gx), p(gy), x.shape[0])
    exact = np.exp(x.astype(np.float64))
    ulps = np.abs(host(gy).astype(np.float64) - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
    small = np.abs(x) <= 1.0
    a = float(ulps[small].max())
    b = float(np.maximum((ulps[~small] - a) / np.abs(x[~small]).astype(np.float64), 0.0).max()) if (~small).any() else 0.0
    print("reference __expf on [-%.4g, 0]: max error %.3f ulp overall, %.3f ulp on [-1, 0], slope %.4f ulp per unit |x|" % (X, ulps.max(), a, b))
    return a, b


@pytest.fixture(scope="module")
def exp_error():
    xs = []
    for name, am, sig, rgb, ts, rays, M in composite_sets():
        if not am:
            x = sig.astype(np.float32) * ts[:, 1]
            xs.append(-x[np.isfinite(x)])
    xs = np.concatenate(xs)
    X = float(-xs.min())
    return measure_fast_exp(X, xs) + (X,)


def run_both_forward(RM, sig, rgb, ts, rays, M, T_thresh, am):
    """-> (weights, weights_sum, depth, image) of the reference and of the product; weights buffers pre-filled with NaN, so that what a kernel wrote can be counted."""
    N = rays.shape[0]
    gs, gc, gt, gr = dev(sig), dev(rgb), dev(ts), dev(rays)
    outs = []
    for side in ("ref", "hip"):
        w = torch.full((M,), float("nan"), device="cuda"); ws, dp, im = zeros(N), zeros(N), zeros(N, 3)
        if side == "ref":
            call("ref_composite_rays_train_forward", p(gs), p(gc), p(gt), p(gr), M, N, float(T_thresh), am, p(w), p(ws), p(dp), p(im))
        else:
            RM.check(RM.lib().mirres_rm_composite_train_fwd(RM.ptr(gs), RM.ptr(gc), RM.ptr(gt), RM.ptr(gr), M, N, float(T_thresh), am, RM.ptr(w), RM.ptr(ws), RM.ptr(dp),
                                                            RM.ptr(im), RM.stream_ptr()), "mirres_rm_composite_train_fwd")
            torch.cuda.synchronize()
        outs.append((host(w), host(ws), host(dp), host(im)))
    return outs


def written(w, rays, M):
    off, cnt, ok = R._spans(rays, M)
    return np.array([int((~np.isnan(w[off[n]:off[n] + cnt[n]])).sum()) if ok[n] else 0 for n in range(len(cnt))])


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_composite_rays_train_forward_against_the_reference_kernel(RM, exp_error, T_thresh):
    """Discrete: the number of weights each ray wrote, equal on both sides and to the float64 count, for every ray whose float64 transmittance stays clear of T_thresh
    (at most 2 % are left out).  Float: the reference kernel's sums within composite_error_bound of float64, with the MEASURED error of its exponential."""
    for name, am, sig, rgb, ts, rays, M in composite_sets():
        near = R.transmittance_near_threshold(sig, ts, rays, T_thresh, bool(am))
        assert near.sum() <= 0.02 * rays.shape[0]
        ref, hip = run_both_forward(RM, sig, rgb, ts, rays, M, T_thresh, am)
        w64, ws64, dp64, im64, used64 = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, bool(am), dtype=np.float64)
        n_ref, n_hip = written(ref[0], rays, M), written(hip[0], rays, M)
        print("%s, T_thresh %g: %d rays, %d left out; samples used: %d (float64), differing rays among those left out: %d" %
              (name, T_thresh, rays.shape[0], near.sum(), used64.sum(), (n_ref != n_hip)[near].sum()))
        assert np.array_equal(n_ref[~near], n_hip[~near]) and np.array_equal(n_ref[~near], used64[~near]), name
        off, cnt, ok = R._spans(rays, M)
        trunc = rays.copy(); trunc[:, 1] = np.where(ok, used64, rays[:, 1])
        fin = ok & ~near
        for what, k, a64, vals in (("weights_sum", 1, ws64, None), ("depth", 2, dp64, ts[:, 0]), ("red", 3, im64[:, 0], rgb[:, 0]), ("green", 4, im64[:, 1], rgb[:, 1]),
                                   ("blue", 5, im64[:, 2], rgb[:, 2])):
            got_ref = ref[k] if k < 3 else ref[3][:, k - 3]
            got_hip = hip[k] if k < 3 else hip[3][:, k - 3]
            b_ref = R.composite_error_bound(sig, ts, trunc, bool(am), vals, exp_ulps=exp_error[:2])
            b_hip = R.composite_error_bound(sig, ts, trunc, bool(am), vals)
            e_ref, e_hip = np.abs(got_ref.astype(np.float64) - a64), np.abs(got_hip.astype(np.float64) - a64)
            print("  %s: reference kernel max error %.3g (bound there %.3g), product %.3g (bound there %.3g)" %
                  (what, e_ref[fin].max(), b_ref[fin][e_ref[fin].argmax()], e_hip[fin].max(), b_hip[fin][e_hip[fin].argmax()]))
            assert (e_ref[fin] <= b_ref[fin]).all() and (e_hip[fin] <= b_hip[fin]).all(), (name, what)


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_composite_rays_train_backward_against_the_reference_kernel(RM, T_thresh):
    """No derived bound: both kernels against the float64 adjoint, per ray scaled by the ray's largest |gradient|.  E_ref is the reference kernel's own largest error;
    the product — another float32 evaluation of the same sums — must stay within 2 E_ref."""
    for name, am, sig, rgb, ts, rays, M in composite_sets():
        N = rays.shape[0]
        near = R.transmittance_near_threshold(sig, ts, rays, T_thresh, bool(am))
        ref, hip = run_both_forward(RM, sig, rgb, ts, rays, M, T_thresh, am)
        rng = np.random.default_rng(3)
        cot = [rng.normal(size=s).astype(np.float32) for s in ((M,), (N,), (N,), (N, 3))]
        gs, gc, gt, gr, gcot = dev(sig), dev(rgb), dev(ts), dev(rays), [dev(x) for x in cot]
        rgs, rgc = zeros(M), zeros(M, 3)
        fwd = [dev(x) for x in ref[1:]]                                       # the reference's own forward results, kept alive over the call
        call("ref_composite_rays_train_backward", *[p(x) for x in gcot], p(gs), p(gc), p(gt), p(gr), p(fwd[0]), p(fwd[1]), p(fwd[2]), M, N, float(T_thresh), am,
             p(rgs), p(rgc))
        s_, c_ = dev(sig).requires_grad_(True), dev(rgb).requires_grad_(True)
        torch.autograd.backward(list(RM.composite_rays_train(s_, c_, gt, gr, T_thresh, bool(am))), gcot)
        w64, ws64, dp64, im64, used64 = R.composite_rays_train_forward(sig, rgb, ts, rays, T_thresh, bool(am), dtype=np.float64)
        gs64, gc64 = R.composite_rays_train_backward(cot[0], cot[1], cot[2], cot[3], sig, rgb, ts, rays, ws64, dp64, im64, T_thresh, bool(am), dtype=np.float64)
        off, cnt, ok = R._spans(rays, M)
        E = {"ref": [0.0, 0.0], "hip": [0.0, 0.0]}
        rays_compared = 0
        for n in np.nonzero(ok & ~near)[0]:
            sl = slice(off[n], off[n] + cnt[n])
            if not (np.isfinite(gs64[sl]).all() and np.isfinite(gc64[sl]).all()) or np.abs(gs64[sl]).max() == 0 or np.abs(gc64[sl]).max() == 0:
                continue
            rays_compared += 1
            for side, (a, b) in (("ref", (host(rgs), host(rgc))), ("hip", (host(s_.grad), host(c_.grad)))):
                E[side][0] = max(E[side][0], np.abs(a[sl] - gs64[sl]).max() / np.abs(gs64[sl]).max())
                E[side][1] = max(E[side][1], np.abs(b[sl] - gc64[sl]).max() / np.abs(gc64[sl]).max())
        print("%s, T_thresh %g backward: grad_sigmas E_ref %.3g, product %.3g; grad_rgbs E_ref %.3g, product %.3g" %
              (name, T_thresh, E["ref"][0], E["hip"][0], E["ref"][1], E["hip"][1]))
        assert rays_compared >= 0.9 * (ok & ~near).sum() and 0 < E["ref"][0] < np.inf and E["hip"][0] <= 2 * E["ref"][0] and E["hip"][1] <= 2 * E["ref"][1], name
