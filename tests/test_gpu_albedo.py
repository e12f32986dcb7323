"""Albedo evaluation on the device (csrc/albedo.hip) through the C ABI, against numpy in float64 stating the formulas of the reference's albedo_eval.py:
the exact channel-wise median of gt / pred.clip(min=1e-6) (:116-118) over a compacted pool (:93-111), the per-view aligned score (:142-172), the
synthetic workspace end to end, and the --use_hdr exposure of the frame.  Inputs are generated from seeds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from mirres_restir_nerf_mesh_amd import _lib
    return _lib


def _scratch(L):
    return torch.zeros(int(L.lib().mirres_albedo_scratch_bytes()), dtype=torch.uint8, device="cuda")


def _np_median(pred, gt):
    """albedo_eval.py:117 — float64 throughout."""
    return np.median(gt.astype(np.float64) / pred.astype(np.float64).clip(min=1e-6), axis=0)


def _median(L, pred, gt, count=None):
    """pred, gt float32 [n, 3] numpy -> (rc, f64[3]) of mirres_albedo_median over a pool holding exactly these pairs."""
    p, g = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda()
    out = torch.full((3,), -123.0, dtype=torch.float64, device="cuda")
    rc = L.lib().mirres_albedo_median(L.ptr(p), L.ptr(g), pred.shape[0] if count is None else count, L.ptr(out), L.ptr(_scratch(L)), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check_median(L, pred, gt, what):
    rc, got = _median(L, pred, gt)
    assert rc == 0, L.lib().mirres_last_error()
    want = _np_median(pred, gt)
    print("%s: n %d  device %r  numpy %r" % (what, pred.shape[0], got.tolist(), want.tolist()))
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.all((got == want) | both_nan), (what, got, want)                  # == on fp64 values: no tolerance (-0 equals +0)
    return got


def _pairs(rng, n):
    """Three channels with different distributions: log-normal ratio, uniform albedo pair, a few discrete levels (many ties)."""
    pred = np.empty((n, 3), np.float32); gt = np.empty((n, 3), np.float32)
    pred[:, 0] = rng.uniform(0.05, 1.0, n); gt[:, 0] = np.minimum(pred[:, 0] * np.exp(rng.normal(-0.2, 0.5, n)), 1.0)
    pred[:, 1] = rng.uniform(0.0, 1.0, n); gt[:, 1] = rng.uniform(0.0, 1.0, n)
    pred[:, 2] = rng.integers(1, 9, n) / 8.0; gt[:, 2] = rng.integers(0, 9, n) / 8.0
    return pred, gt


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1000000, 1000001])
def test_median_exact_small_and_around_a_million(L, n):
    pred, gt = _pairs(np.random.default_rng(100 + n), n)
    _check_median(L, pred, gt, "seeded pool")


def test_median_exact_above_2_pow_24_pixels(L):
    """Float counters or 32-bit prefix sums fail here: 2^24 + 4100 pixels (an even count), then one fewer (odd)."""
    n = (1 << 24) + 4100
    pred, gt = _pairs(np.random.default_rng(7), n)
    _check_median(L, pred, gt, "above 2^24, even")
    _check_median(L, pred[:-1], gt[:-1], "above 2^24, odd")


def test_median_ties_and_the_clip(L):
    rng = np.random.default_rng(9)
    n = 4096
    one = lambda v: np.full((n, 3), v, np.float32)
    _check_median(L, one(0.4), one(0.3), "all ratios equal")
    _check_median(L, one(0.4)[:-1], one(0.3)[:-1], "all ratios equal, odd count")
    # sorted ratios r_0 <= ... <= r_{n-1}, middle ranks n/2 - 1 and n/2: a run of one value over both / over exactly the lower / exactly the upper one
    base = np.sort(rng.uniform(0.1, 0.9, n)).astype(np.float32)
    for name, lo, hi in (("ties cover both middle ranks", n // 2 - 5, n // 2 + 5), ("ties cover the lower middle rank only", n // 2 - 7, n // 2),
                         ("ties cover the upper middle rank only", n // 2, n // 2 + 9)):
        g = base.copy(); g[lo:hi] = g[lo]
        perm = rng.permutation(n)
        gt = np.stack([g[perm], g[rng.permutation(n)], g[::-1]], 1)
        _check_median(L, np.ones((n, 3), np.float32), gt, name)
    # pred 0, 1e-7 and 1e-6 (fp32 1e-6 lies just below the double 1e-6: all three are clipped), negative and tiny predictions, next to ordinary ones
    pred = rng.choice(np.array([0.0, 1e-7, 1e-6, -0.5, 1.0000001e-6, 2e-6, 0.5], np.float32), (n, 3))
    gt = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    _check_median(L, pred, gt, "pred at and below the clip")
    _check_median(L, pred[:, :] * 0, gt, "pred all zero")
    gt0 = gt.copy(); gt0[rng.random((n, 3)) < 0.6] = 0.0
    got = _check_median(L, np.full((n, 3), 0.5, np.float32), gt0, "gt zero in more than half the pool")
    assert np.all(got == 0.0)
    gtm = gt0.copy(); gtm[gtm == 0.0] = -0.0
    _check_median(L, np.full((n, 3), 0.5, np.float32), gtm, "minus zeros")
    # ratios spanning 1e-6 ... 1e6, and negative ratios on one channel
    r = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), (n + 1, 3)))
    pred = np.exp(rng.uniform(np.log(1e-5), 0.0, (n + 1, 3))).astype(np.float32)
    gt = (r * pred).astype(np.float32); gt[:, 2] *= rng.choice([-1.0, 1.0], n + 1).astype(np.float32)
    _check_median(L, pred, gt, "ratios over twelve decades, odd count")
    _check_median(L, pred[:-1], gt[:-1], "ratios over twelve decades, even count")
    inf = gt.copy(); inf[5, 0] = np.inf; inf[6, 1] = -np.inf
    _check_median(L, pred, inf, "infinite ratios")


def test_median_nan_and_empty_pool(L):
    rng = np.random.default_rng(12)
    pred, gt = _pairs(rng, 10001)
    gt[77, 1] = np.nan
    got = _check_median(L, pred, gt, "one NaN in channel 1")
    assert np.isnan(got[1]) and not np.isnan(got[0]) and not np.isnan(got[2])
    pred2, gt2 = _pairs(rng, 10000)
    pred2[5, 2] = np.nan
    got = _check_median(L, pred2, gt2, "a NaN prediction in channel 2")
    assert np.isnan(got[2]) and not np.isnan(got[0])
    rc, out = _median(L, pred, gt, count=0)
    assert rc < 0 and b"empty" in L.lib().mirres_last_error() and np.all(out == -123.0)      # an error, not a number


def _compact(L, views, thr, cap=None, slack=0):
    """views: list of (pred [n, 3], gt_rgba [n, 4]) float32 numpy -> (pool_pred, pool_gt, state) after one mirres_albedo_compact per view.  The pools
    are allocated `slack` rows longer than the capacity the kernels are told."""
    total = sum(v[0].shape[0] for v in views)
    cap = total if cap is None else cap
    pp = torch.full((max(cap, 1) + slack, 3), -7.0, device="cuda"); pg = torch.full((max(cap, 1) + slack, 3), -7.0, device="cuda")
    state = torch.zeros(3, dtype=torch.int64, device="cuda")
    sc = _scratch(L)
    for pred, gt in views:
        p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        rc = L.lib().mirres_albedo_compact(L.ptr(p), L.ptr(g), pred.shape[0], thr, L.ptr(pp), L.ptr(pg), cap, L.ptr(state), L.ptr(sc), L.stream_ptr())
        assert rc == 0, L.lib().mirres_last_error()
    torch.cuda.synchronize()
    return pp.cpu().numpy(), pg.cpu().numpy(), state.cpu().numpy()


def _view(rng, n, p_keep=0.4):
    pred = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    gt[:, 3] = np.where(rng.random(n) < p_keep, rng.uniform(0.9, 1.0, n), rng.uniform(0.0, 0.9, n)).astype(np.float32)
    return pred, gt


def test_compaction_order_threshold_and_pool_of_views(L):
    rng = np.random.default_rng(31)
    thr = 0.9
    views = [_view(rng, n) for n in (1, 777, 4096, 250001, 3, 64 * 1024 + 5, 1023)]          # seven views of different sizes
    pp, pg, st = _compact(L, views, thr)
    keep = [v[1][:, 3].astype(np.float64) >= thr for v in views]                             # :94-95 on the float64 copy of the file
    want_p = np.concatenate([v[0][k] for v, k in zip(views, keep)]); want_g = np.concatenate([v[1][k, :3] for v, k in zip(views, keep)])
    n = want_p.shape[0]
    assert st.tolist() == [n, 0, 0]
    assert np.array_equal(pp[:n], want_p) and np.array_equal(pg[:n], want_g)                 # pixel order, view after view
    assert np.all(pp[n:] == -7.0)
    cat = (np.concatenate([v[0] for v in views]), np.concatenate([v[1] for v in views]))
    pp1, pg1, st1 = _compact(L, [cat], thr)
    assert st1[0] == n and np.array_equal(pp1[:n], pp[:n]) and np.array_equal(pg1[:n], pg[:n])
    rc, got = _median(L, pp[:n], pg[:n])
    rc1, got1 = _median(L, pp1[:n], pg1[:n])
    assert rc == 0 and rc1 == 0 and np.array_equal(got, got1) and np.array_equal(got, _np_median(want_p, want_g))
    # alpha == mask_thr is kept, the next float below is dropped (thresholds that are fp32 values, and 0.9, which is not: fp32(0.9) < 0.9 is dropped)
    for t in (0.5, 0.30000001192092896, 0.9):
        t32 = np.float32(t)
        al = np.array([t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1)), 1.0, 0.0], np.float32)
        pred = np.arange(15, dtype=np.float32).reshape(5, 3) / 16
        gt = np.concatenate([pred * 0.5, al[:, None]], 1).astype(np.float32)
        pp, pg, st = _compact(L, [(pred, gt)], t)
        k = al.astype(np.float64) >= t
        assert st[0] == k.sum() and np.array_equal(pp[: st[0]], pred[k]), (t, st, k)
        assert bool(k[0]) == (float(t32) >= t) and not k[1] and k[2]
    # a pool that is too small: nothing is written beyond it, the overflow is reported
    # (the second view overflows it; the third runs on the full pool: the count stays at the capacity, the flag stays set, rows past the capacity untouched)
    pp, pg, st = _compact(L, views[:3], thr, cap=100, slack=4096)
    assert st[0] == 100 and st[2] == 1 and np.array_equal(pp[:100], want_p[:100]) and np.array_equal(pg[:100], want_g[:100])
    assert np.all(pp[100:] == -7.0) and np.all(pg[100:] == -7.0)
    # no pixel kept: the count stays 0 and the median of that pool is an error
    pred, gt = _view(rng, 500); gt[:, 3] = 0.0
    assert _compact(L, [(pred, gt)], thr)[2].tolist() == [0, 0, 0]


def test_evaluator_errors_are_errors(L):
    from mirres_restir_nerf_mesh_amd import albedo
    rng = np.random.default_rng(5)
    ev = albedo.AlbedoEvaluator(mask_thr=0.9)
    with pytest.raises(ValueError, match="no pixel"):
        ev.scale()
    pred, gt = _view(rng, 64 * 48)
    sh = lambda x: torch.from_numpy(x.reshape(48, 64, -1))
    ev.add_view(sh(pred).cuda(), sh(gt))
    kept = int((gt[:, 3].astype(np.float64) >= 0.9).sum())
    assert ev.count == kept
    bad = gt.copy()
    i = int(np.nonzero(bad[:, 3] >= 0.9)[0][3]); bad[i, 1] = 1.0000001
    with pytest.raises(ValueError, match="view 1"):                                         # the second view, named
        ev.add_view(sh(pred).cuda(), sh(bad))
    assert ev.count == kept and len(ev.views) == 1
    out = gt.copy(); j = int(np.nonzero(out[:, 3] < 0.9)[0][0]); out[j, 0] = 7.0             # above 1 outside the mask: not an error
    ev.add_view(sh(pred).cuda(), sh(out))
    assert ev.count == 2 * kept
    k = gt[:, 3].astype(np.float64) >= 0.9
    assert ev.scale() == tuple(_np_median(np.concatenate([pred[k], pred[k]]), np.concatenate([gt[k, :3], gt[k, :3]])).tolist())
    nan = gt.copy(); nan[i, 2] = np.nan
    ev.add_view(sh(pred).cuda(), sh(nan))
    with pytest.raises(ValueError, match="NaN"):
        ev.scale()


# ------------------------------------------------------------------------------------------------ (c) the per-view score
def _np_score(pred, gt_rgba, thr, scale):
    """The script's per-view score in float64 for one view (pred [n, 3], gt_rgba [n, 4]): pixels whose alpha is not below the threshold take the scaled
    prediction clipped to [0, 1] and the ground truth as it is; every other pixel is 1 in both images; squared differences of the images and of their
    1 / 2.2 powers are summed; the gamma images x 255 are what becomes the 8-bit images."""
    gt64, pred64 = gt_rgba.astype(np.float64), pred.astype(np.float64)
    inside = ~(gt64[:, 3] < thr)[:, None]
    aligned = np.where(inside, np.clip(pred64 * np.asarray(scale, np.float64)[None, :], 0.0, 1.0), 1.0)
    truth = np.where(inside, gt64[:, :3], 1.0)
    ga, gt_ = aligned ** (1 / 2.2), truth ** (1 / 2.2)
    return float(((truth - aligned) ** 2).sum()), float(((gt_ - ga) ** 2).sum()), ga * 255, gt_ * 255


def _score(L, pred, gt, thr, scale):
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    p8 = torch.zeros(pred.shape, dtype=torch.uint8, device="cuda"); g8 = torch.zeros(pred.shape, dtype=torch.uint8, device="cuda")
    h = (C.c_double * 3)(*scale) if scale is not None else None
    rc = L.lib().mirres_albedo_score(L.ptr(p), L.ptr(g), pred.shape[0], thr, h, L.ptr(sums), L.ptr(p8), L.ptr(g8), L.ptr(_scratch(L)), L.stream_ptr())
    assert rc == 0, L.lib().mirres_last_error()
    torch.cuda.synchronize()
    return sums.cpu().numpy(), p8.cpu().numpy(), g8.cpu().numpy()


@pytest.mark.parametrize("n", [800 * 800, 12345, 1])
def test_score_sums_images_and_determinism(L, n):
    rng = np.random.default_rng(41 + n)
    pred, gt = _view(rng, n, 0.5)
    gt[:, :3] = np.clip(pred * np.array([0.7, 1.3, 0.9], np.float32) + rng.normal(0, 0.05, (n, 3)).astype(np.float32), 0, 1)
    gt[:: 7, 0] = 0.0; pred[:: 11, 1] = 0.0; pred[:: 13, 2] = -0.25; gt[:: 17, 2] = 1.0
    scale = (0.71, 1.2999999, 0.93)
    for sc in (scale, None):
        sums, p8, g8 = _score(L, pred, gt, 0.9, sc)
        lin, gam, f_now, f_gt = _np_score(pred, gt, 0.9, sc if sc is not None else (1.0, 1.0, 1.0))
        n_val = 3 * n
        psnr = lambda s: -10.0 * np.log(s / n_val) / np.log(10.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            print("n %d scale %r: linear sum %.17g (numpy %.17g), gamma sum %.17g (numpy %.17g), PSNR differences %.3g / %.3g dB"
                  % (n, sc, sums[0], lin, sums[1], gam, abs(psnr(sums[0]) - psnr(lin)), abs(psnr(sums[1]) - psnr(gam))))
        same = lambda a, b: a == b or abs(psnr(a) - psnr(b)) <= 1e-8                          # (both sums 0: a view without a masked pixel)
        assert same(sums[0], lin) and same(sums[1], gam)
        for got, f in ((p8, f_now), (g8, f_gt)):
            want = f.astype("uint8")
            # where x ** (1 / 2.2) * 255 lies within a few ulp of an integer, the two pow implementations may truncate to neighbouring levels
            near = np.abs(f - np.rint(f)) <= 16 * np.spacing(np.maximum(f, 1.0))
            diff = got != want
            print("  u8 image: %d of %d values near an integer, %d differ" % (int(near.sum()), near.size, int(diff.sum())))
            assert not np.any(diff & ~near)
            assert np.all(np.abs(got.astype(int) - want.astype(int))[diff] == 1)
        again = _score(L, pred, gt, 0.9, sc)
        assert again[0].tobytes() == sums.tobytes() and np.array_equal(again[1], p8) and np.array_equal(again[2], g8)       # two runs: same bits


# ------------------------------------------------------------------------------------------------ the synthetic workspace, end to end
def _evaluate_script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mirres_evaluate_script", os.path.join(ROOT, "scripts", "evaluate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _workspace(tmp_path, S):
    import json
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR, checkpoint as CK
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    ES = _evaluate_script()
    ws = str(tmp_path / "ws")
    ck_path, tf_path = ES.synthetic_workspace(ws, S, S)
    ck = CK.read_checkpoint(ck_path)
    cfg = CK.resolve_material_config(ck.get("material_config"))
    v, t, _, _ = CK.load_stage0_mesh(ws, CK.cascade_of_bound(cfg["bound"]))
    aabb, mn, mx = CK.material_field_args(cfg)
    mlp = MLPTexture3D(aabb, channels=6, min_max=(mn.cuda(), mx.cuda()))
    voff, light = CK.apply_checkpoint(ck, mlp, n_vertices=v.shape[0])
    W = RR.restirbvhWorker((torch.from_numpy(v).cuda() + (voff if voff is not None else 0)).contiguous(), torch.from_numpy(t).cuda()); W.update_mesh(W.vrt, W.v_ind)
    tf = json.load(open(tf_path))
    focal = 0.5 * S / np.tan(0.5 * tf["camera_angle_x"])
    poses = [torch.from_numpy(ES.nerf_pose(fr["transform_matrix"])) for fr in tf["frames"]]
    return ws, ck_path, tf_path, W, mlp, light, poses, (focal, focal, S * 0.5, S * 0.5)


def test_synthetic_workspace_end_to_end(tmp_path):
    from mirres_restir_nerf_mesh_amd import albedo, harness
    S = 64
    ws, ck_path, tf_path, W, mlp, light, poses, intr = _workspace(tmp_path, S)
    s = np.array([0.7, 1.3, 0.9], np.float32)
    ev = albedo.AlbedoEvaluator(mask_thr=0.9)
    for i, pose in enumerate(poses):
        kd = harness.albedo_view(W, mlp, pose, intr, S, S, 1)
        img, maps = harness.test_view(W, mlp, light, pose, intr, S, S, 2, 1, random_offset=i, return_maps=True)
        assert kd.shape == (S, S, 3) and torch.equal(kd, maps["kd"])                         # bit-equal at ssaa 1
        cover = harness.albedo_view(W, None, pose, intr, S, S, 1, gbuffer_consts=dict(kd=(1.0, 1.0, 1.0)))[..., :1]
        assert 0.05 < float(cover.mean()) < 0.95
        gt = torch.cat((kd * torch.from_numpy(s).cuda(), cover), dim=-1)                     # fp32(pred * s), alpha 1 on the object and 0 elsewhere
        assert float(gt[..., :3].max()) <= 1.0                                               # the evaluator refuses a masked ground truth above 1: s must leave room
        print("view %d: %d object pixels, albedo in [%.4f, %.4f], ground truth max %.4f" % (i, int(cover.sum()), float(kd[cover[..., 0] > 0].min()), float(kd.max()), float(gt[..., :3].max())))
        ev.add_view(kd, gt)
    got = ev.scale()
    rel = [abs(g / x - 1.0) for g, x in zip(got, (0.7, 1.3, 0.9))]                          # against the decimal s, not its fp32 rounding
    print("recovered scale %r of (0.7, 1.3, 0.9) (as fp32: %r): relative errors %r (bound 2^-23 = %.3g)" % (got, s.tolist(), rel, 2.0 ** -23))
    assert all(r <= 2.0 ** -23 for r in rel)
    aligned, plain = ev.score(got), ev.score((1.0, 1.0, 1.0))
    print("psnr_exr aligned %.3f dB, unaligned %.3f dB; means %r" % (aligned["mean"]["psnr_exr"], plain["mean"]["psnr_exr"], aligned["mean"]))
    assert aligned["mean"]["psnr_exr"] > plain["mean"]["psnr_exr"] and aligned["mean"]["psnr_png"] > plain["mean"]["psnr_png"]
    assert aligned["mean"]["ssim"] >= plain["mean"]["ssim"] and set(aligned["views"][0]) == {"psnr_exr", "psnr_png", "ssim"} and len(aligned["views"]) == len(poses)
    up = harness.albedo_view(W, mlp, poses[0], intr, S, S, 2)                                # the SSAA down-scale of the kd image
    _, maps2 = harness.test_view(W, mlp, light, poses[0], intr, S, S, 2, 2, random_offset=0, return_maps=True)
    assert maps2["kd"].shape == (2 * S, 2 * S, 3) and torch.equal(up, harness.scale_img_hwc(maps2["kd"], (S, S)))
    white = harness.albedo_view(W, mlp, poses[0], intr, S, S, 2, background=1.0)             # the reference composes the kd image over white before the down-scale
    occ2 = harness.albedo_view(W, None, poses[0], intr, S, S, 2, gbuffer_consts=dict(kd=(1.0, 1.0, 1.0)))[..., :1]
    assert torch.allclose(white, up + (1 - occ2), atol=1e-6) and torch.equal(white[occ2[..., 0] == 1], up[occ2[..., 0] == 1])
    assert up.shape == (S, S, 3) and bool(torch.isfinite(up).all()) and 0.0 <= float(up.min()) and float(up.max()) <= 1.0
    # evaluate.py --albedo_scale_file: the same frame bytes as the same three numbers typed by hand
    f = albedo.write_scale(str(tmp_path / "albedo_scale.json"), got, ev.count, 0.9)
    env = str(tmp_path / "sky.hdr")
    from mirres_restir_nerf_mesh_amd import scene
    harness.write_hdr(env, scene.make_env(32, 64))
    base = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--workspace", ws, "--ckpt", ck_path, "--transforms", tf_path,
            "--spp", "2", "--ssaa", "1", "--limit", "1", "--envmap_path", env, "--use_hdr", "--exposure", "-1"]
    outs = []
    for name, extra in (("by_file", ["--albedo_scale_file", f]), ("by_hand", ["--albedo_scale_x", repr(got[0]), "--albedo_scale_y", repr(got[1]), "--albedo_scale_z", repr(got[2])])):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out", out] + extra, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(open(os.path.join(out, sorted(os.listdir(out))[0]), "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 100


def test_albedo_eval_script_synthetic(tmp_path):
    """scripts/albedo_eval.py --synthetic: its own workspace and ground truth (albedo x (0.7, 1.3, 0.9)); the files it promises, and the scale in them."""
    from mirres_restir_nerf_mesh_amd import albedo
    ws = str(tmp_path / "ws")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "scripts", "albedo_eval.py"), "--synthetic", "--workspace", ws, "--H", "64", "--W", "64",
                        "--limit", "2"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-1500:])
    out = os.path.join(ws, "albedo_eval")
    d = albedo.read_scale(os.path.join(out, "albedo_scale.json"))
    assert all(abs(g / w - 1) < 1e-6 for g, w in zip(d["scale"], (0.7, 1.3, 0.9))) and d["n_pixels"] > 100 and d["mask_thr"] == 0.9
    assert os.path.exists(os.path.join(out, "gammaed_scaled_kd_0.png")) and os.path.exists(os.path.join(out, "gammaed_scaled_kd_1.png"))
    assert os.path.exists(os.path.join(ws, "gt", "test_001", "diffuse-color.exr"))


def test_exposure_of_the_test_frame(tmp_path):
    from mirres_restir_nerf_mesh_amd import harness, renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    S, spp, seed = 48, 4, 1234
    ws, ck_path, tf_path, W, mlp, light, poses, intr = _workspace(tmp_path, S)
    light = (light * 4.0).contiguous()                                                       # bright enough that the clamp at 1 bites for positive exposures
    pose = poses[1]
    for ssaa in (1, 2):
        g = harness.build_gbuffer_from_pose(W, pose, intr, S, S, ssaa, mlp)
        out = RR.render_fused(get_ctx(g["fx"], g["fy"]), W, mlp, False, (1.0, 1.0, 1.0), light, g["occ"].clone(), g["normal"], g["depth"], g["kd"], g["rm"], g["ray_dir"],
                              g["pos"], spp, 2, 2, 2.0, 0.1, 0.001, seed)[0]
        raw = torch.nan_to_num(out[0], 0.0)                                                  # the unclamped frame of a run with the same seed
        today = harness.test_view(W, mlp, light, pose, intr, S, S, spp, ssaa, random_offset=seed)
        assert torch.equal(today, harness.postprocess(raw, g["occ"], S, S, ssaa))
        none, maps0 = harness.test_view(W, mlp, light, pose, intr, S, S, spp, ssaa, random_offset=seed, exposure=None, return_maps=True)
        assert torch.equal(none, today) and torch.equal(maps0["env_map"], light)
        frames = {}
        for e in (-2, 0, 1):                                                                 # powers of two: the product is exact
            img, maps = harness.test_view(W, mlp, light, pose, intr, S, S, spp, ssaa, random_offset=seed, exposure=e, return_maps=True)
            assert torch.equal(img, harness.postprocess(raw * (2.0 ** e), g["occ"], S, S, ssaa)), (ssaa, e)
            assert torch.equal(maps["env_map"], light * (2.0 ** e)) and torch.equal(maps["kd"], maps0["kd"])
            frames[e] = img
        assert torch.equal(frames[0], today) and not torch.equal(frames[1], today) and float(frames[-2].mean()) != float(today.mean())
        assert float((raw * 2.0 > 1.0).float().mean()) > 0.0                                 # the clamp comes after the factor, and is reached
