"""Albedo evaluation with median scale alignment (the reference's albedo_eval.py; csrc/albedo.hip): the step of the TensoIR protocol that
produces the `--albedo_scale_x/y/z` of the relighting commands (configs/tensoir_synthetic/*.txt) and reports the aligned albedo's PSNR (linear and
gamma 2.2), SSIM and LPIPS.

    ev = AlbedoEvaluator(mask_thr=0.9)             # 0.3 for ficus, 0.9 for the other scenes (albedo_eval.py:15)
    for view: ev.add_view(harness.albedo_view(...), meters.read_exr(".../test_XXX/diffuse-color.exr"))
    sx, sy, sz = ev.scale()                        # channel-wise median of gt / pred.clip(min=1e-6) over the masked pixels of all views (:116-118)
    res = ev.score()                               # per view and mean: psnr_exr, psnr_png, ssim (, lpips_vgg)

The masked (prediction, ground truth) pairs are compacted into a device pool as the views arrive, the median is an exact radix select over that pool and
the per-view sums are taken in fp64 on the device; the host sees three doubles and two doubles per view.  The script's `alex` LPIPS variant needs a
network this package does not restate and is left out; `lpips_vgg` is meters.LPIPS and is reported when weights are given.  SSIM and LPIPS read the
8-bit gamma images (what the script saves as gammaed_scaled_kd_{i}.png) divided by 255."""
import ctypes as C
import json
import math

import numpy as np
import torch

from . import _lib, meters

__all__ = ["AlbedoEvaluator", "write_scale", "read_scale"]


class AlbedoEvaluator:
    def __init__(self, mask_thr=0.9, lpips_vgg=None, lpips_lin=None, device=None, keep_views=True):
        """`lpips_vgg` / `lpips_lin`: weights as for meters.LPIPS (None: no LPIPS column).  `keep_views` False keeps only the pool (scale() alone)."""
        self.mask_thr = float(mask_thr)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros(3, dtype=torch.int64, device=self.device)          # pairs in the pool, kept pixels with gt > 1, overflow flag
        self.scratch = torch.zeros(int(_lib.lib().mirres_albedo_scratch_bytes()), dtype=torch.uint8, device=self.device)
        self.pool_pred = torch.empty((0, 3), dtype=torch.float32, device=self.device)
        self.pool_gt = torch.empty((0, 3), dtype=torch.float32, device=self.device)
        self.count = 0
        self.views = []
        self.keep_views = keep_views
        self.lpips = meters.LPIPS(vgg=lpips_vgg, lin=lpips_lin).eval().to(self.device) if lpips_vgg is not None else None

    def _reserve(self, n):
        cap = self.pool_pred.shape[0]
        if self.count + n <= cap:
            return
        new_cap = max(self.count + n, 2 * cap)
        for name in ("pool_pred", "pool_gt"):
            old = getattr(self, name)
            new = torch.empty((new_cap, 3), dtype=torch.float32, device=self.device)
            new[: self.count] = old[: self.count]
            setattr(self, name, new)

    def _prep(self, pred, gt_rgba):
        pred = torch.as_tensor(pred).to(self.device, torch.float32)
        gt = torch.as_tensor(np.ascontiguousarray(gt_rgba) if isinstance(gt_rgba, np.ndarray) else gt_rgba).to(self.device, torch.float32)
        if pred.shape[-1] != 3 or gt.shape[-1] != 4 or pred.shape[:-1] != gt.shape[:-1]:
            raise ValueError("albedo: expected pred [..., 3] and gt_rgba [..., 4] over the same pixels, got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
        return pred.contiguous(), gt.contiguous()

    def add_view(self, pred, gt_rgba):
        """pred [H, W, 3] (the view's albedo, harness.albedo_view), gt_rgba [H, W, 4] (diffuse-color.exr; tensor or numpy).  Returns the number of
        pixels the mask kept.  A kept ground-truth value above 1 raises, naming the view (albedo_eval.py:98-100)."""
        pred, gt = self._prep(pred, gt_rgba)
        n = pred.numel() // 3
        self._reserve(n)
        L = _lib.lib()
        _lib.check(L.mirres_albedo_compact(_lib.ptr(pred), _lib.ptr(gt), n, self.mask_thr, _lib.ptr(self.pool_pred), _lib.ptr(self.pool_gt),
                                           self.pool_pred.shape[0], _lib.ptr(self.state), _lib.ptr(self.scratch), _lib.stream_ptr()), "mirres_albedo_compact")
        count, bad, overflow = (int(x) for x in self.state.tolist())
        view = len(self.views)
        if overflow:                                                 # cannot happen after _reserve; the view is not taken
            self.state[2] = 0; self.state[1] = 0; self.state[0] = self.count
            raise _lib.MirresError("albedo: the pool overflowed at view %d (%d pairs)" % (view, count))
        if bad:
            self.state[1] = 0; self.state[0] = self.count            # the view is not taken
            raise ValueError("albedo: view %d has %d masked pixel(s) with a ground-truth albedo above 1" % (view, bad))
        kept, self.count = count - self.count, count
        self.views.append((pred, gt) if self.keep_views else None)
        return kept

    def scale(self):
        """The three channel scales as Python floats (fp64): np.median(gt64 / pred64.clip(min=1e-6), axis=0) over the pool, exactly."""
        if self.count == 0:
            raise ValueError("albedo: no pixel passed the mask (mask_thr %r, %d view(s)): there is no scale" % (self.mask_thr, len(self.views)))
        out = torch.empty(3, dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().mirres_albedo_median(_lib.ptr(self.pool_pred), _lib.ptr(self.pool_gt), self.count, _lib.ptr(out), _lib.ptr(self.scratch),
                                                   _lib.stream_ptr()), "mirres_albedo_median")
        s = tuple(float(x) for x in out.tolist())
        if any(math.isnan(x) for x in s):
            raise ValueError("albedo: a NaN in the prediction or the ground truth makes the scale %r" % (s,))
        return s

    def score_view(self, pred, gt_rgba, scale):
        """One view (albedo_eval.py:142-172): (sum of squared differences of the linear images, of the gamma 2.2 images, pred u8 [.., 3], gt u8 [.., 3])."""
        pred, gt = self._prep(pred, gt_rgba)
        n = pred.numel() // 3
        sums = torch.empty(2, dtype=torch.float64, device=self.device)
        p8 = torch.empty(pred.shape, dtype=torch.uint8, device=self.device); g8 = torch.empty(pred.shape, dtype=torch.uint8, device=self.device)
        h_scale = (C.c_double * 3)(*[float(x) for x in scale]) if scale is not None else None
        _lib.check(_lib.lib().mirres_albedo_score(_lib.ptr(pred), _lib.ptr(gt), n, self.mask_thr, h_scale, _lib.ptr(sums), _lib.ptr(p8), _lib.ptr(g8),
                                                  _lib.ptr(self.scratch), _lib.stream_ptr()), "mirres_albedo_score")
        lin, gam = (float(x) for x in sums.tolist())
        return lin, gam, p8, g8

    def score(self, scale=None, on_view=None):
        """Scores every added view with `scale` (None: self.scale(); (1, 1, 1): the unaligned albedo).  Returns dict(scale=, n_pixels=, views=[dict(psnr_exr=,
        psnr_png=, ssim= [, lpips_vgg=])], mean=dict(...)).  `on_view(i, pred_u8, gt_u8)` receives the two 8-bit gamma images (device tensors)."""
        if not self.keep_views:
            raise RuntimeError("albedo: score() needs the views (keep_views=True)")
        scale = self.scale() if scale is None else tuple(float(x) for x in scale)
        rows = []
        for i, (pred, gt) in enumerate(self.views):
            lin, gam, p8, g8 = self.score_view(pred, gt, scale)
            n_val = pred.numel()
            row = dict(psnr_exr=-10.0 * math.log(lin / n_val) / math.log(10.0) if lin > 0 else math.inf,                 # :166-167
                       psnr_png=-10.0 * math.log(gam / n_val) / math.log(10.0) if gam > 0 else math.inf)                 # :170-171
            a, b = p8.reshape(-1, p8.shape[-2], 3).to(torch.float32) / 255.0, g8.reshape(-1, g8.shape[-2], 3).to(torch.float32) / 255.0
            row["ssim"] = float(meters.ssim_script(a, b, 1.0))                                                           # :173
            if self.lpips is not None:
                with torch.no_grad():
                    row["lpips_vgg"] = float(self.lpips(b.permute(2, 0, 1)[None], a.permute(2, 0, 1)[None], normalize=True).item())   # :174 (gt first)
            if on_view is not None:
                on_view(i, p8, g8)
            rows.append(row)
        mean = {k: sum(r[k] for r in rows) / len(rows) for k in rows[0]} if rows else {}
        return dict(scale=scale, n_pixels=self.count, views=rows, mean=mean)


def write_scale(path, scale, n_pixels, mask_thr):
    """A small JSON file for `evaluate.py --albedo_scale_file`: the floats as their repr (which round-trips a double exactly)."""
    sx, sy, sz = (float(x) for x in scale)
    with open(path, "w") as f:
        json.dump({"albedo_scale_x": repr(sx), "albedo_scale_y": repr(sy), "albedo_scale_z": repr(sz), "n_pixels": int(n_pixels), "mask_thr": repr(float(mask_thr))}, f, indent=1)
    return path


def read_scale(path):
    """-> dict(scale=(x, y, z), n_pixels=, mask_thr=) of a file written by write_scale."""
    d = json.load(open(path))
    try:
        scale = tuple(float(d["albedo_scale_" + k]) for k in "xyz")
    except KeyError as e:
        raise ValueError("%s: not an albedo scale file (missing %s)" % (path, e))
    return dict(scale=scale, n_pixels=int(d.get("n_pixels", 0)), mask_thr=float(d.get("mask_thr", "nan")))
