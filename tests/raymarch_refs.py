"""numpy restatements of the stage-0 ray-marching operators (csrc/raymarch.hip, csrc/device_march.hpp) in the FIXED arithmetic of DESIGN.md section 5.13: float32,
every operation rounded on its own, IEEE division, the reference's C++ promotions (the cell index is a double product of a float sum, rounded to float at the clamp
and truncated; mip_from_dt's dt * H * 0.5 likewise), exact frexp / ldexp, and mrf_exp (include/mirres_fmath.h, evaluated by the fmath checker's fmath_eval, function
3) as the compositing exponential.  The marchers also return, per ray, how many loop passes they executed (outer passes + passes of the voxel-skipping loop) — the
figure the GPU tests bound before anything is launched.  The compositing functions take a dtype: float64 runs the SAME code with numpy's exp (the adjoint tests), and
composite_train_torch64 is an independent float64 torch implementation (cumprod, the early-termination mask detached) to hold them against.

Vectorised over rays as a state machine: in every tick a ray either makes one pass of the outer loop or one pass of the skipping loop, so a call costs
max-passes-per-ray ticks whatever the number of rays."""
import ctypes as C
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLT_MAX = np.finfo(np.float32).max
SQRT3 = F(1.7320508075688772)
NO_CAP = 0xffffffff
U = 2.0 ** -24                                       # unit roundoff of binary32


@functools.lru_cache(maxsize=None)
def _fmath():
    from oracle import oracle as O
    O.lib()                                          # builds the checker next to the CPU reference library when it is missing
    L = C.CDLL(os.path.join(ROOT, "oracle", "libfmathcheck.so"))
    L.fmath_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    return L


def mrf_exp(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    if x.size:
        _fmath().fmath_eval(3, x.ctypes.data, None, out.ctypes.data, x.size)
    return out


def _exp(x):
    return mrf_exp(x) if x.dtype == np.float32 else np.exp(x)


def clamp(x, lo, hi):
    return np.fmin(hi, np.fmax(lo, x))               # fminf(hi, fmaxf(lo, x)): a NaN x gives lo


# ---------------------------------------------------------------------------------------------------------------- integer helpers
def expand_bits(v):
    v = np.asarray(v).astype(np.uint32)
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return v


def morton3D(coords):
    c = np.asarray(coords).astype(np.int32).view(np.uint32).reshape(-1, 3)
    with np.errstate(over="ignore"):
        return (expand_bits(c[:, 0]) | (expand_bits(c[:, 1]) << np.uint32(1)) | (expand_bits(c[:, 2]) << np.uint32(2))).view(np.int32)


def _invert1(x):
    x = x & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xc30c30c3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0f00f00f)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xff0000ff)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000ffff)
    return x


def morton3D_invert(indices):
    ind = np.asarray(indices).astype(np.int32)       # `ind >> k` on the signed value, as the reference has it
    return np.stack([_invert1((ind >> k).view(np.uint32)) for k in range(3)], -1).view(np.int32)


def packbits(grid, thresh):
    g = np.asarray(grid, np.float32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        b = g > F(thresh)
    return (b.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(1).astype(np.uint8)


def _spans(rays, M):
    rays = np.asarray(rays, np.int32)
    offset = rays[:, 0].view(np.uint32).astype(np.int64)
    count = rays[:, 1].view(np.uint32).astype(np.int64)
    return offset, count, (count != 0) & (offset + count <= M)


def flatten_rays(rays, M):
    offset, count, ok = _spans(rays, M)
    res = np.zeros(M, np.int32)
    for n in np.nonzero(ok)[0]:
        res[offset[n]:offset[n] + count[n]] = n
    return res


# ---------------------------------------------------------------------------------------------------------------- near / far
def near_far_from_aabb(rays_o, rays_d, aabb, min_near):
    o = np.asarray(rays_o, np.float32).reshape(-1, 3); d = np.asarray(rays_d, np.float32).reshape(-1, 3); a = np.asarray(aabb, np.float32)
    with np.errstate(all="ignore"):
        r = F(1) / d
        lo = [(a[k] - o[:, k]) * r[:, k] for k in range(3)]
        hi = [(a[3 + k] - o[:, k]) * r[:, k] for k in range(3)]
        for k in range(3):
            sw = lo[k] > hi[k]
            lo[k], hi[k] = np.where(sw, hi[k], lo[k]), np.where(sw, lo[k], hi[k])
        near, far = lo[0], hi[0]
        miss = (near > hi[1]) | (lo[1] > far)
        near = np.where(lo[1] > near, lo[1], near); far = np.where(hi[1] < far, hi[1], far)
        miss |= (near > hi[2]) | (lo[2] > far)
        near = np.where(lo[2] > near, lo[2], near); far = np.where(hi[2] < far, hi[2], far)
        near = np.where(near < F(min_near), F(min_near), near)
    return np.where(miss, FLT_MAX, near).astype(np.float32), np.where(miss, FLT_MAX, far).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the marchers
def _mip(mx, top):
    e = np.frexp(mx)[1].astype(np.float32)
    return np.fmin(top, np.fmax(F(0), e)).astype(np.int32)


def _march(o, d, bits, bound, contract, dt_gamma, max_steps, Cn, H, near, far, t_start, noises, num_steps, eps, max_trips=NO_CAP, guards=True):
    """Every ray from t_start (+ the noise offset) for at most num_steps[n] samples -> samples f32 [N, cap, 5] (cx, cy, cz, t after the step, dt), counts, the loop
    passes per ray, t at the end.  guards=False leaves out the three termination guards the reference does not have (rm_ray_ok, the skipping loop's t + dt == t and
    t >= far tests): the loops as raymarching.cu:396-465 / :759-827 has them, ended by max_trips alone where they would spin.  A ray that provably never ends (t + dt == t in
    the skipping loop: it spins there, or the outer loop repeats one pass for ever; or tt = +inf) is charged max_trips passes at once, without being walked."""
    o = np.asarray(o, np.float32).reshape(-1, 3); d = np.asarray(d, np.float32).reshape(-1, 3)
    N = o.shape[0]
    bits = np.asarray(bits, np.uint8)
    bound, g = F(bound), F(dt_gamma)
    dt_min = F(2) * SQRT3 / F(max_steps)
    dt_max = F(2) * SQRT3 * bound / F(H)
    rH = F(1) / F(H)
    Hf, Cf, top, H3 = F(H), F(Cn), F(H - 1), int(H) ** 3
    near = np.asarray(near, np.float32); far = np.asarray(far, np.float32)
    num_steps = np.broadcast_to(np.asarray(num_steps, np.int64), (N,)).copy()
    cap = int(num_steps.max()) if N else 0
    out = np.zeros((N, cap, 5), np.float32)
    with np.errstate(all="ignore"):
        rd = F(1) / (d + F(eps))
        t = np.asarray(t_start, np.float32).copy()
        t = t + clamp(t * g, dt_min, dt_max) * np.asarray(noises, np.float32)
        m = np.fmax(np.abs(d[:, 0]), np.fmax(np.abs(d[:, 1]), np.abs(d[:, 2])))
        done = ~((d == d).all(1) & (m > 0) & (m < np.inf) & (near == near) & (far == far)) if guards else np.zeros(N, bool)
        step = np.zeros(N, np.int64); trips = np.zeros(N, np.int64)
        inner = np.zeros(N, bool); tt = np.zeros(N, np.float32)
        sgn = np.copysign(F(1), d)
        while True:
            lo = np.nonzero(~done & ~inner & (t < far) & (step < num_steps))[0]
            li = np.nonzero(~done & inner)[0]
            if lo.size == 0 and li.size == 0:
                break
            if li.size:                                                     # one pass of the voxel-skipping do-while
                ts = t[li]
                tn = ts + clamp(ts * g, dt_min, dt_max)
                adv = ~(tn == ts)
                if not guards:      # t stands still: the do-while spins below tt, and past it the outer loop repeats the same pass (t and step as before); tt = +inf
                    spin = ~adv | ((tt[li] == np.inf) & (tn < tt[li]))
                    trips[li[spin]] = max_trips
                    adv = ~spin
                done[li[~adv]] = True                                       # absorbed
                a = li[adv]
                t[a] = tn[adv]; trips[a] += 1
                capped = trips[a] >= max_trips
                done[a[capped]] = True
                inner[li] = False
                inner[a] = ~capped & (tn[adv] < tt[a]) & ((tn[adv] < far[a]) if guards else True)
            if lo.size:                                                     # one pass of the outer loop
                trips[lo] += 1
                capped = trips[lo] >= max_trips
                done[lo[capped]] = True
                lo = lo[~capped]
                tc = t[lo]
                p = [clamp(o[lo, k] + tc * d[lo, k], -bound, bound) for k in range(3)]
                dt = clamp(tc * g, dt_min, dt_max)
                mag = np.fmax(np.abs(p[0]), np.fmax(np.abs(p[1]), np.abs(p[2])))
                level = np.maximum(_mip(mag, Cf - F(1)), _mip(((dt * Hf).astype(np.float64) * 0.5).astype(np.float32), Cf - F(1)))
                mip_bound = np.fmin(np.ldexp(F(1), level).astype(np.float32), bound)
                rb = F(1) / mip_bound
                outer = bool(contract) & (mag > 1)
                s = (F(2) - F(1) / mag) / mag
                c = [np.where(outer, p[k] * s, p[k]) for k in range(3)]
                n = [clamp(((0.5 * (c[k] * rb + F(1)).astype(np.float64)) * float(H)).astype(np.float32), F(0), top).astype(np.int32) for k in range(3)]
                index = level.astype(np.int64) * H3 + morton3D(np.stack(n, -1)).astype(np.int64)
                occ = ((bits[index >> 3] >> (index & 7).astype(np.uint8)) & 1).astype(bool)
                take = occ | outer
                a = lo[take]
                tn = tc[take] + dt[take]
                out[a, step[a], 0] = c[0][take]; out[a, step[a], 1] = c[1][take]; out[a, step[a], 2] = c[2][take]
                out[a, step[a], 3] = tn; out[a, step[a], 4] = dt[take]
                step[a] += 1; t[a] = tn
                sk = ~take
                b = lo[sk]
                tx = [(((n[k][sk].astype(np.float32) + F(0.5) + F(0.5) * sgn[b, k]) * rH * F(2) - F(1)) * mip_bound[sk] - c[k][sk]) * rd[b, k] for k in range(3)]
                tt[b] = tc[sk] + np.fmax(F(0), np.fmin(tx[0], np.fmin(tx[1], tx[2])))
                inner[b] = True
    return out, step, trips, t


def march_rays_train(rays_o, rays_d, bound, contract, bits, Cn, H, nears, fars, noises, dt_gamma=0.0, max_steps=1024, max_trips=NO_CAP):
    """-> xyzs [M, 3], dirs [M, 3], ts [M, 2], rays i32 [N, 2] (exclusive prefix sum, count), loop passes per ray."""
    d = np.asarray(rays_d, np.float32).reshape(-1, 3)
    out, step, trips, _ = _march(rays_o, d, bits, bound, contract, dt_gamma, max_steps, Cn, H, nears, fars, nears, noises, max_steps, 0.0, max_trips)
    N = d.shape[0]
    rays = np.zeros((N, 2), np.int32)
    rays[:, 1] = step
    rays[:, 0] = np.concatenate([[0], np.cumsum(step)[:-1]]) if N else 0
    keep = np.arange(out.shape[1])[None, :] < step[:, None]
    flat = out[keep]
    dirs = np.repeat(d, step, axis=0)
    return flat[:, :3].copy(), dirs, flat[:, 3:5].copy(), rays, trips


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, contract, bits, Cn, H, nears, fars, noises, dt_gamma=0.0, max_steps=1024, max_trips=NO_CAP):
    """-> xyzs [n_alive * n_step, 3], dirs, ts [n_alive * n_step, 2] (unfilled slots zero), loop passes per alive ray."""
    o = np.asarray(rays_o, np.float32).reshape(-1, 3); d = np.asarray(rays_d, np.float32).reshape(-1, 3)
    idx = np.asarray(rays_alive, np.int32)[:n_alive].astype(np.int64)
    ok = (idx >= 0) & (idx < o.shape[0])
    j = np.where(ok, idx, 0)
    steps = np.where(ok, n_step, 0)
    out, step, trips, _ = _march(o[j], d[j], bits, bound, contract, dt_gamma, max_steps, Cn, H, np.asarray(nears, np.float32)[j], np.asarray(fars, np.float32)[j],
                                 np.asarray(rays_t, np.float32)[j], noises, steps, 1e-10, max_trips)
    full = np.zeros((n_alive, n_step, 5), np.float32)
    full[:, :out.shape[1]] = out[:, :n_step]
    filled = np.arange(n_step)[None, :] < step[:, None]
    dirs = np.where(filled[..., None], d[j][:, None, :], F(0))
    return full[..., :3].reshape(-1, 3).copy(), dirs.reshape(-1, 3).astype(np.float32), full[..., 3:5].reshape(-1, 2).copy(), trips


def reference_loops_end(o, d, bits, bound, contract, dt_gamma, max_steps, Cn, H, near, far, t_start, noises, num_steps, eps):
    """The gate in front of every launch of the REFERENCE'S marchers (oracle/_ref/libref_raymarch.so), whose loops have no termination guard: per ray, whether the
    loops as the reference has them (guards=False) end by themselves within TRIP_CAP passes.  A launch happens only when this is true of every ray."""
    return _march(o, d, bits, bound, contract, dt_gamma, max_steps, Cn, H, near, far, t_start, noises, num_steps, eps, TRIP_CAP, guards=False)[2] < TRIP_CAP


def train_case_loops_end(c):
    """reference_loops_end for a march_train_case."""
    return reference_loops_end(c["o"], c["d"], c["bits"], c["bound"], c["contract"], c["dt_gamma"], c["max_steps"], c["C"], c["H"], c["nears"], c["fars"], c["nears"],
                               c["noises"], c["max_steps"], 0.0)


def infer_round_loops_end(c, r):
    """reference_loops_end for one round of an infer_case: the march_rays form (start at rays_t, 1 / (d + 1e-10f), n_step samples)."""
    j = r["rays_alive"].astype(np.int64)
    return reference_loops_end(c["o"][j], c["d"][j], c["bits"], 1.0, False, 0.0, c["max_steps"], 1, c["H"], c["nears"][j], c["fars"][j], r["rays_t"][j],
                               np.zeros(r["n_alive"], np.float32), r["n_step"], 1e-10)


# ---------------------------------------------------------------------------------------------------------------- compositing
def _alpha(sigma, dt, alpha_mode):
    return sigma if alpha_mode else (sigma.dtype.type(1) - _exp(-sigma * dt))


def composite_rays_train_forward(sigmas, rgbs, ts, rays, T_thresh, alpha_mode, dtype=np.float32):
    """-> weights [M], weights_sum [N], depth [N], image [N, 3], and per ray how many samples it used.  dtype float64: the same code with numpy's exp."""
    sig = np.asarray(sigmas, dtype); rgb = np.asarray(rgbs, dtype).reshape(-1, 3); ts = np.asarray(ts, dtype).reshape(-1, 2)
    M, N = sig.shape[0], np.asarray(rays).shape[0]
    offset, count, ok = _spans(rays, M)
    one, Tt = dtype(1), dtype(T_thresh)
    weights = np.zeros(M, dtype)
    T = np.ones(N, dtype); acc = np.zeros((N, 5), dtype)                    # r, g, b, ws, d
    used = np.zeros(N, np.int64)
    alive = ok.copy()
    with np.errstate(all="ignore"):
        for k in range(int(count[ok].max()) if ok.any() else 0):
            a = np.nonzero(alive & (k < count))[0]
            if a.size == 0:
                break
            p = offset[a] + k
            alpha = _alpha(sig[p], ts[p, 1], alpha_mode)
            w = alpha * T[a]
            weights[p] = w
            acc[a, 0] += w * rgb[p, 0]; acc[a, 1] += w * rgb[p, 1]; acc[a, 2] += w * rgb[p, 2]
            acc[a, 3] += w
            acc[a, 4] += w * ts[p, 0]
            T[a] = T[a] * (one - alpha)
            used[a] += 1
            alive[a[T[a] < Tt]] = False
    return weights, acc[:, 3].copy(), acc[:, 4].copy(), acc[:, :3].copy(), used


def composite_rays_train_backward(grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, T_thresh, alpha_mode,
                                  dtype=np.float32):
    """-> grad_sigmas [M], grad_rgbs [M, 3]."""
    A = lambda x: np.asarray(x, dtype)
    gw, gws, gd, gi = A(grad_weights), A(grad_weights_sum), A(grad_depth), A(grad_image).reshape(-1, 3)
    sig, rgb, ts = A(sigmas), A(rgbs).reshape(-1, 3), A(ts).reshape(-1, 2)
    fin = np.concatenate([A(image).reshape(-1, 3), A(weights_sum)[:, None], A(depth)[:, None]], 1)
    M, N = sig.shape[0], fin.shape[0]
    offset, count, ok = _spans(rays, M)
    one, Tt = dtype(1), dtype(T_thresh)
    gs = np.zeros(M, dtype); gc = np.zeros((M, 3), dtype)
    T = np.ones(N, dtype); acc = np.zeros((N, 5), dtype)
    alive = ok.copy()
    with np.errstate(all="ignore"):
        for k in range(int(count[ok].max()) if ok.any() else 0):
            a = np.nonzero(alive & (k < count))[0]
            if a.size == 0:
                break
            p = offset[a] + k
            alpha = _alpha(sig[p], ts[p, 1], alpha_mode)
            w = alpha * T[a]
            acc[a, 0] += w * rgb[p, 0]; acc[a, 1] += w * rgb[p, 1]; acc[a, 2] += w * rgb[p, 2]
            acc[a, 3] += w
            acc[a, 4] += w * ts[p, 0]
            T[a] = T[a] * (one - alpha)
            Ta = T[a]
            for c in range(3):
                gc[p, c] = gi[a, c] * w
            scale = (one / (one - alpha)) if alpha_mode else ts[p, 1]
            gs[p] = scale * (gi[a, 0] * (Ta * rgb[p, 0] - (fin[a, 0] - acc[a, 0])) + gi[a, 1] * (Ta * rgb[p, 1] - (fin[a, 1] - acc[a, 1])) +
                             gi[a, 2] * (Ta * rgb[p, 2] - (fin[a, 2] - acc[a, 2])) + (gws[a] + gw[p]) * (Ta - (fin[a, 3] - acc[a, 3])) +
                             gd[a] * (Ta * ts[p, 0] - (fin[a, 4] - acc[a, 4])))
            alive[a[Ta < Tt]] = False
    return gs, gc


def composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh, alpha_mode):
    """In place on copies -> rays_alive, rays_t, weights_sum, depth, image."""
    alive_ids = np.asarray(rays_alive, np.int32).copy(); rays_t = np.asarray(rays_t, np.float32).copy()
    ws = np.asarray(weights_sum, np.float32).copy(); dp = np.asarray(depth, np.float32).copy(); im = np.asarray(image, np.float32).reshape(-1, 3).copy()
    sig = np.asarray(sigmas, np.float32); rgb = np.asarray(rgbs, np.float32).reshape(-1, 3); ts = np.asarray(ts, np.float32).reshape(-1, 2)
    N = ws.shape[0]
    idx = alive_ids[:n_alive].astype(np.int64)
    ok = (idx >= 0) & (idx < N)
    alive_ids[:n_alive][~ok] = -1
    rows = np.nonzero(ok)[0]
    j = idx[rows]
    acc = np.stack([im[j, 0], im[j, 1], im[j, 2], ws[j], dp[j]], 1)
    t = np.zeros(rows.size, np.float32); step = np.zeros(rows.size, np.int64); going = np.ones(rows.size, bool)
    Tt = F(T_thresh)
    with np.errstate(all="ignore"):
        for k in range(n_step):
            p = rows * n_step + k
            going &= ~(ts[p, 0] == 0)
            a = np.nonzero(going)[0]
            if a.size == 0:
                break
            pa = p[a]
            alpha = _alpha(sig[pa], ts[pa, 1], alpha_mode)
            T = F(1) - acc[a, 3]
            w = alpha * T
            acc[a, 3] += w
            t[a] = ts[pa, 0]
            acc[a, 4] += w * t[a]
            acc[a, 0] += w * rgb[pa, 0]; acc[a, 1] += w * rgb[pa, 1]; acc[a, 2] += w * rgb[pa, 2]
            stop = T < Tt
            going[a[stop]] = False
            step[a[~stop]] += 1
    ended = step < n_step
    alive_ids[rows[ended]] = -1
    rays_t[j[~ended]] = t[~ended]
    im[j, 0], im[j, 1], im[j, 2], ws[j], dp[j] = acc[:, 0], acc[:, 1], acc[:, 2], acc[:, 3], acc[:, 4]
    return alive_ids, rays_t, ws, dp, im


def composite_train_torch64(sigmas, rgbs, ts, rays, T_thresh, alpha_mode):
    """Independent of the code above: float64 torch, per ray alpha -> exclusive cumprod of (1 - alpha) -> weights, with the early-termination mask (a sample counts
    while every transmittance before it stayed >= T_thresh) detached.  sigmas / rgbs may require grad.  -> weights, weights_sum, depth, image."""
    import torch
    M = sigmas.shape[0]
    offset, count, ok = _spans(rays, M)
    ts = torch.as_tensor(ts, dtype=torch.float64)
    weights = torch.zeros(M, dtype=torch.float64)
    ws, dp, im = [], [], []
    for n in range(len(count)):
        if not ok[n]:
            ws.append(torch.zeros((), dtype=torch.float64)); dp.append(ws[-1]); im.append(torch.zeros(3, dtype=torch.float64))
            continue
        sl = slice(int(offset[n]), int(offset[n] + count[n]))
        alpha = sigmas[sl] if alpha_mode else 1.0 - torch.exp(-sigmas[sl] * ts[sl, 1])
        Tin = torch.cumprod(1.0 - alpha, 0)                                 # transmittance AFTER each sample
        Tex = torch.cat([torch.ones(1, dtype=torch.float64), Tin[:-1]])
        cut = (Tin.detach() < T_thresh).to(torch.float64)
        mask = (torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(cut, 0)[:-1]]) == 0).to(torch.float64)
        w = alpha * Tex * mask
        weights = weights + torch.zeros(M, dtype=torch.float64).index_put((torch.arange(sl.start, sl.stop),), w)
        ws.append(w.sum()); dp.append((w * ts[sl, 0]).sum()); im.append((w[:, None] * rgbs[sl]).sum(0))
    return weights, torch.stack(ws), torch.stack(dp), torch.stack(im)


def alpha_error_constant(alpha_mode, exp_ulps=2):
    """A of composite_error_bound: |d alpha| <= A u for alpha = fl(1 - exp(-fl(sigma dt))) with the given error of the exponential (the derivation is there)."""
    ea, eb = exp_ulps if isinstance(exp_ulps, tuple) else (exp_ulps, 0.0)
    return 0.0 if alpha_mode else (5.4 if (ea, eb) == (2, 0.0) else 2.0 * ea + (2.0 * eb + 1.0) / np.e + 1.0)


def composite_rays_float64(n_step, idx, weights_sum, depth, image, sigmas, rgbs, ts, T_thresh, alpha_mode, exp_ulps=2, rel=1e-5):
    """One composite_rays call (raymarching.cu:842-924) in float64 on the call's own float32 inputs, for the alive rays `idx` (ids into the per-ray state), with the
    forward-error bound of a float32 run of it.  -> acc f64 [n, 5] (r, g, b, weights_sum, depth afterwards), stays (the ray was not ended), t (the last sample's t),
    near (1 - weights_sum came within a relative `rel` of T_thresh at some sample the ray looked at: its end may differ in float32), bound f64 [n, 5].
    The bound, first order in u = 2^-24, for inputs with 0 <= alpha <= 1 and 0 <= weights_sum <= 1.  Per sample k = 0, 1, ... of the call: |d alpha| <= A u
    (alpha_error_constant).  T = fl(1 - ws): |dT| <= |dws| + u.  w = fl(alpha T): |dw| <= A u T + alpha (|dws| + u) + u w.  ws' = fl(ws + w) = (1 - alpha) ws + alpha
    in exact arithmetic, so an error of ws enters ws' with the factor 1 - alpha <= 1: |dws'| <= |dws| + A u T + alpha u + u w + u ws' <= |dws| + (A + 3) u, i.e.
    |dws_k| <= k (A + 3) u =: E_k before sample k (the state the call starts from is shared, so E_0 = 0).  A sum acc' = fl(acc + fl(w v)) (v = t: depth, v = a
    colour channel): |d acc'| <= |d acc| + |v| |dw| + u |w v| + u |acc'|.  Summed over the samples the ray used, with u' = u / (1 - 8 n u) for the higher orders:
      bound_ws = n (A + 3) u',   bound_v = u' sum_k [ |v_k| (A T_k + alpha_k (E_k / u + 1) + w_k) + |w_k v_k| + |acc_k'| ],  evaluated on the float64 values."""
    idx = np.asarray(idx, np.int64); n = idx.shape[0]
    im = np.asarray(image, np.float64).reshape(-1, 3)
    acc = np.stack([im[idx, 0], im[idx, 1], im[idx, 2], np.asarray(weights_sum, np.float64)[idx], np.asarray(depth, np.float64)[idx]], 1)
    sig = np.asarray(sigmas, np.float64).reshape(n, n_step); rgb = np.asarray(rgbs, np.float64).reshape(n, n_step, 3); ts = np.asarray(ts, np.float64).reshape(n, n_step, 2)
    A = alpha_error_constant(alpha_mode, exp_ulps)
    u1 = U / (1.0 - 8.0 * n_step * U)
    going = np.ones(n, bool); step = np.zeros(n, np.int64); near = np.zeros(n, bool); t = np.zeros(n); used = np.zeros(n)
    bound = np.zeros((n, 5))
    with np.errstate(all="ignore"):
        for k in range(n_step):
            going &= ts[:, k, 0] != 0
            T = 1.0 - acc[:, 3]
            near |= going & (np.abs(T - T_thresh) <= rel * T_thresh)
            alpha = sig[:, k] if alpha_mode else 1.0 - np.exp(-sig[:, k] * ts[:, k, 1])
            w = np.where(going, alpha * T, 0.0)
            dw = np.where(going, A * T + alpha * (used * (A + 3.0) + 1.0) + w, 0.0)      # |dw| / u
            v = np.stack([rgb[:, k, 0], rgb[:, k, 1], rgb[:, k, 2], np.ones(n), ts[:, k, 0]], 1)
            acc += w[:, None] * v
            t = np.where(going, ts[:, k, 0], t)
            bound += np.where(going[:, None], u1 * (np.abs(v) * dw[:, None] + np.abs(w[:, None] * v) + np.abs(acc)), 0.0)
            used += going
            going &= ~(T < T_thresh)
            step += going
    bound[:, 3] = used * (A + 3.0) * u1
    return acc, step >= n_step, t, near, bound


def composite_rays_sets(n_step=16):
    """Stand-alone composite_rays inputs cut from the compositing sets: every ray of train_composite_inputs with at least n_step samples gives its first n_step (both
    alpha modes), and the three constant-sigma rays 50 of theirs (the third has 7: the rest of its slots are ts = 0 rows, as the marcher leaves them).  Every seventh
    ray of the random sets gets ts = 0 rows from some slot on.  The per-ray state starts from non-zero sums; rays_alive is a permutation into a larger state.
    -> [(name, alpha_mode, n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image)]"""
    out = []
    for name, am, (sig, rgb, ts, rays, M), ns in (("random-0", 0, train_composite_inputs(False), n_step), ("random-1", 1, train_composite_inputs(True), n_step),
                                                  ("constant", 0, constant_sigma_rays(), 50)):
        rng = np.random.default_rng(91 + am)
        off, cnt, ok = _spans(rays, M)
        pick = np.nonzero(ok & ((cnt >= ns) | (name == "constant")))[0]
        n = pick.shape[0]
        s2 = np.zeros((n, ns), np.float32); c2 = np.zeros((n, ns, 3), np.float32); t2 = np.zeros((n, ns, 2), np.float32)
        for i, r in enumerate(pick):
            m = min(ns, int(cnt[r]))
            s2[i, :m] = sig[off[r]:off[r] + m]; c2[i, :m] = rgb[off[r]:off[r] + m]; t2[i, :m] = ts[off[r]:off[r] + m]
            if name != "constant" and i % 7 == 3:
                t2[i, int(rng.integers(0, ns)):] = 0
        N = n + 5
        alive = rng.permutation(N)[:n].astype(np.int32)
        state = (rng.uniform(0.1, 0.5, N).astype(np.float32), rng.uniform(0, 0.3, N).astype(np.float32), rng.uniform(0, 1, N).astype(np.float32),
                 rng.uniform(0, 1, (N, 3)).astype(np.float32))
        out.append((name, am, n, ns, alive, state[0], s2.reshape(-1), c2.reshape(-1, 3), t2.reshape(-1, 2), state[1], state[2], state[3]))
    return out


def composite_error_bound(sigmas, ts, rays, alpha_mode, values=None, exp_ulps=2):
    """Forward-error bound of the float32 compositing against exact arithmetic on the same inputs, per ray, for sum_k w_k v_k (v = 1: weights_sum; v = t: depth; v = a
    colour channel), first order in u = 2^-24 with the higher orders folded into u' = u / (1 - 8 n u).  Derivation, per sample k (0-based) of a ray of n samples:
      x = fl(sigma dt): relative u.  e = mrf_exp(-x): within 2 ulp = 4 u relative of exp(-x), and exp(-x) moves by x u relative when x does: |de| <= (4 e + x e) u
      <= 4.37 u (e <= 1, x e^-x <= 1/e).  alpha = fl(1 - e): |d alpha| <= 4.37 u + u alpha <= 5.4 u =: A u  (alpha mode: alpha is an input, A = 0).
      q = fl(1 - alpha): |dq| <= (A + 1) u.  T_k = the product of k such factors, each <= 1, one rounding per product: |dT_k| <= k (A + 2) u.
      w = fl(alpha T): |dw_k| <= A u T_k + alpha_k k (A + 2) u + u w_k.
      term = fl(w v): |d term| <= |v| |dw_k| + u |w v|;  the n sequential additions: gamma_n sum |w v| <= n u sum |w v|.
    Total: u' * sum_k [ |v_k| (A T_k + (A + 2) k alpha_k + w_k) + |w_k v_k| ] + n u' sum_k |w_k v_k|, evaluated on the float64 values.
    exp_ulps: the exponential's error.  A number K: within K ulp = 2 K u relative everywhere, so |de| <= (2 K e + x e) u <= (2 K + 1/e) u and A = 2 K + 1/e + 1
    (K = 2: 5.37, kept as today's 5.4).  A pair (a, b): an error that may grow with the argument, within (a + b x) ulp at exp(-x) — an exponential formed as
    exp2(x log2 e) carries the rounding of the product, an absolute x log2(e) u in the exponent, into a relative error proportional to x —
    |de| <= (2 a + (2 b + 1) x) e^-x u <= (2 a + (2 b + 1) / e) u, since e^-x <= 1 and x e^-x <= 1/e: A = 2 a + (2 b + 1) / e + 1."""
    sig = np.asarray(sigmas, np.float64); ts = np.asarray(ts, np.float64).reshape(-1, 2)
    M = sig.shape[0]
    offset, count, ok = _spans(rays, M)
    A = alpha_error_constant(alpha_mode, exp_ulps)
    out = np.zeros(len(count))
    for n in np.nonzero(ok)[0]:
        sl = slice(int(offset[n]), int(offset[n] + count[n]))
        alpha = sig[sl] if alpha_mode else 1.0 - np.exp(-sig[sl] * ts[sl, 1])
        Tex = np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]])
        w = alpha * Tex
        v = np.ones(w.shape) if values is None else np.abs(np.asarray(values, np.float64)[sl])
        k = np.arange(w.shape[0], dtype=np.float64)
        nn = float(w.shape[0])
        u1 = U / (1.0 - 8.0 * nn * U)
        out[n] = u1 * np.sum(v * (A * Tex + (A + 2.0) * k * alpha + w) + w * v) + nn * u1 * np.sum(w * v)
    return out


def transmittance_near_threshold(sigmas, ts, rays, T_thresh, alpha_mode, rel=1e-5):
    """Per ray: does the float64 transmittance after some sample, up to and including the one that ends the ray, come within a relative `rel` of T_thresh?  Such a
    ray may use one sample more or fewer in float32 than in exact arithmetic, whichever exponential is used; every other ray uses the same number."""
    sig = np.asarray(sigmas, np.float64); ts = np.asarray(ts, np.float64).reshape(-1, 2)
    offset, count, ok = _spans(rays, sig.shape[0])
    near = np.zeros(len(count), bool)
    with np.errstate(all="ignore"):
        for n in np.nonzero(ok)[0]:
            sl = slice(int(offset[n]), int(offset[n] + count[n]))
            alpha = sig[sl] if alpha_mode else 1.0 - np.exp(-sig[sl] * ts[sl, 1])
            Tin = np.cumprod(1.0 - alpha)
            cut = np.nonzero(Tin < T_thresh)[0]
            Tin = Tin[:cut[0] + 1] if cut.size else Tin
            near[n] = bool((np.abs(Tin - T_thresh) <= rel * T_thresh).any())
    return near


def train_composite_inputs(alpha_mode):
    """512 rays, M just under 20 000: lengths 0, 1, 2, 63, 64, 65 and the cap 1024, rays cut by T_thresh at the first step, in the middle and never, one ray with
    offset + n > M, sigma = 0 and sigma = +inf samples."""
    rng = np.random.default_rng(77 + int(alpha_mode))
    counts = np.concatenate([[0, 1, 2, 63, 64, 65, 1024], rng.integers(1, 70, 504), [40]])
    assert counts.shape[0] == 512
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts[:-1].sum()) + 7
    assert M <= 20000
    dt = rng.uniform(0.002, 0.02, M)
    alpha = rng.uniform(0.0, 0.6, M)
    alpha[offs[6]:offs[6] + 1024] = rng.uniform(0, 0.004, 1024)               # the cap-length ray is never cut: 0.996^1024 > 1e-2
    alpha[offs[5]:offs[5] + 65] = 0.0; alpha[offs[5] + 30] = 0.99999            # cut in the middle
    alpha[offs[4]] = 0.99999                                                   # cut at the first step
    alpha[offs[3]:offs[3] + 63] = 0.01                                        # never cut
    sig = alpha.copy() if alpha_mode else -np.log1p(-alpha) / dt
    sig[offs[10] + 1] = 0.0
    if not alpha_mode:
        sig[offs[11]] = np.inf
    ts = np.stack([0.5 + np.cumsum(dt) * 0.01, dt], 1)
    rgb = rng.uniform(0, 1, (M, 3))
    rays = np.stack([offs, counts], 1).astype(np.int32)
    return sig.astype(np.float32), rgb.astype(np.float32), ts.astype(np.float32), rays, M


def constant_sigma_rays():
    """The three rays of tests/test_raymarch_host.py::test_compositing_constant_sigma_closed_form as one input set -> sigmas, rgbs, ts, rays, M."""
    sets = [(3.0, 0.01, 50), (40.0, 0.004, 200), (0.5, 0.02, 7)]
    sig = np.concatenate([np.full(n, s, np.float32) for s, dt, n in sets])
    ts = np.concatenate([np.stack([0.5 + dt * np.arange(1, n + 1), np.full(n, dt)], 1) for s, dt, n in sets]).astype(np.float32)
    counts = np.array([n for _, _, n in sets])
    rays = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1).astype(np.int32)
    M = int(counts.sum())
    rgb = np.random.default_rng(12).uniform(0, 1, (M, 3)).astype(np.float32)
    return sig, rgb, ts, rays, M


# ---------------------------------------------------------------------------------------------------------------- the occupancy grid
def cascade_scales(Cn, H, bound):
    """Per cascade (bound_c - half_cell, half_cell, 2 half_cell) as the reference's Python forms them: doubles, rounded to fp32 where they meet a tensor."""
    out = []
    for c in range(Cn):
        b = min(2.0 ** c, float(bound)); h = b / H
        out.append((F(b - h), F(h), F(h * 2)))
    return out


def lattice(H):
    """The lattice coordinate 2 i / (H - 1) - 1 of every Morton index -> f32 [H^3, 3]."""
    c = morton3D_invert(np.arange(H ** 3, dtype=np.int32)).astype(np.float32)
    return (F(2) * c) / F(H - 1) - F(1)


def mark_untrained(grid, H, bound, poses, intrinsics, aabb, min_near, cam_near_far=None):
    """-> the boolean [C, H^3] set of cells that become -1."""
    grid = np.asarray(grid, np.float32)
    Cn = grid.shape[0]
    P = np.asarray(poses, np.float32); K = np.asarray(intrinsics, np.float32).reshape(-1, 4); a = np.asarray(aabb, np.float32)
    B = P.shape[0]
    lat = lattice(H)
    mark = np.zeros((Cn, H ** 3), bool)
    for cas, (scale, hgs, hgs2) in enumerate(cascade_scales(Cn, H, bound)):
        w = lat * scale
        in_box = ((w >= a[:3] - hgs) & (w <= a[3:] + hgs)).all(1)
        seen = np.zeros(H ** 3, bool)
        for b in range(B):
            q = w - P[b, :3, 3]
            cam = [(q[:, 0] * P[b, 0, j] + q[:, 1] * P[b, 1, j]) + q[:, 2] * P[b, 2, j] for j in range(3)]
            cz = -cam[2]
            k = K[b if K.shape[0] == B and B > 1 else 0]
            nr = F(min_near) if cam_near_far is None else np.asarray(cam_near_far, np.float32)[b, 0]
            seen |= (cz > nr) & (np.abs(cam[0]) < (k[2] / k[0]) * cz + hgs2) & (np.abs(cam[1]) < (k[3] / k[1]) * cz + hgs2)
        mark[cas] = ~(in_box & seen)
    return mark


# ---------------------------------------------------------------------------------------------------------------- shared inputs of the host and the device tests
GRID_KINDS = ("random", "full", "empty", "single")
GRID_SHAPES = ((16, 1, 1.0), (16, 3, 4.0), (32, 1, 1.0), (32, 3, 4.0))      # (H, cascades, bound)
MARCH_PARAMS = [dict(dt_gamma=g, perturb=p, contract=c, max_steps=m) for g in (0.0, 1.0 / 256.0) for p in (False, True) for c in (False, True) for m in (64, 1024)]
TRIP_CAP = 10 ** 5
N_HOSTILE = 3


def grid_bits(kind, H, Cn, seed=7):
    """A bitfield u8 [C * H^3 / 8]: about 10 % random occupancy, full, empty, or one cell of cascade 0 (the cell of the point (0.3, 0.05, -0.2))."""
    cells = Cn * H ** 3
    if kind == "random":
        occ = np.random.default_rng(seed + H + Cn).random(cells) < 0.1
    elif kind == "full":
        occ = np.ones(cells, bool)
    elif kind == "empty":
        occ = np.zeros(cells, bool)
    else:
        occ = np.zeros(cells, bool)
        occ[single_cell_index(H)] = True
    return packbits(occ.astype(np.float32), 0.5)


def single_cell_coords(H):
    return [int(0.5 * (v + 1.0) * H) for v in (0.3, 0.05, -0.2)]


def single_cell_index(H):
    return int(morton3D(np.array([single_cell_coords(H)], np.int32))[0])


def make_rays(N, bound, H, seed=3, hostile=True):
    """N rays around the cube [-bound, bound]^3 -> rays_o, rays_d, nears, fars (near_far_from_aabb above, min_near 0.2), noises.  From N >= 16 the first rows are
    special: a ray that misses the box, rays ALONG cell faces of cascade 0 (axis-parallel, the origin's other coordinates on cell boundaries), rays aimed at the cell
    of grid_bits('single'), a ray from inside, and — with `hostile` — the three rays the termination guards exist for: a zero direction, a NaN near and an origin at
    1e7 with a finite far (rows 0 .. N_HOSTILE - 1)."""
    rng = np.random.default_rng(seed + N)
    b = float(bound)
    o = rng.normal(size=(N, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.2 * b, 2.5 * b, size=(N, 1))
    tgt = rng.uniform(-0.9 * b, 0.9 * b, size=(N, 3))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    special = N >= 16
    if special:
        cell = (np.array(single_cell_coords(H)) + 0.5) / H * 2.0 - 1.0
        o[3] = [-2.0 * b, 3.0 * b, 0.0]; d[3] = [0.0, 1.0, 0.0]                                 # misses
        o[4] = [-2.0 * b, 2.0 / H, -4.0 / H]; d[4] = [1.0, 0.0, 0.0]                               # along the faces y = 2 / H, z = -4 / H
        o[5] = [0.0, 2.0 * b, 0.0]; d[5] = [0.0, -1.0, -0.0]                                       # along x = 0, z = 0, with a negative zero
        o[6] = [cell[0], cell[1], 2.0 * b]; d[6] = [0.0, 0.0, -1.0]                                # through the single cell, axis-parallel
        o[7] = [2.0 * b, 2.0 * b, 2.0 * b]; v = cell - o[7]; d[7] = v / np.linalg.norm(v)          # through it, diagonal
        o[8] = [0.1, -0.2, 0.05]                                                                   # from inside
        for k in range(9, 12):                                                                     # a zero component on each axis
            d[k, k - 9] = 0.0
    nears, fars = near_far_from_aabb(o, d, [-b, -b, -b, b, b, b], 0.2)
    if special and hostile:
        d[0] = 0.0                                                                                 # zero direction (its near / far are NaN or inf as well)
        nears[1] = np.nan                                                                          # NaN near
        o[2] = [1e7, 0.0, 0.0]; d[2] = [-1.0, 0.0, 0.0]                                            # far away: t is absorbed at once
        n2, f2 = near_far_from_aabb(o[2:3], d[2:3], [-b, -b, -b, b, b, b], 0.2)
        nears[2], fars[2] = n2[0], f2[0]
    noises = rng.random(N).astype(np.float32)
    return o, d, nears.astype(np.float32), fars.astype(np.float32), noises


@functools.lru_cache(maxsize=None)
def march_train_case(kind, shape_i, param_i, N, hostile=True):
    """One march_rays_train case, computed once per process and shared by the host and the device tests: the inputs and the restatement's outputs."""
    H, Cn, bound = GRID_SHAPES[shape_i]
    P = MARCH_PARAMS[param_i]
    bits = grid_bits(kind, H, Cn)
    o, d, nears, fars, noises = make_rays(N, bound, H, hostile=hostile)
    if not P["perturb"]:
        noises = np.zeros_like(noises)
    xyzs, dirs, ts, rays, trips = march_rays_train(o, d, bound, P["contract"], bits, Cn, H, nears, fars, noises, P["dt_gamma"], P["max_steps"], max_trips=TRIP_CAP)
    case = dict(H=H, C=Cn, bound=bound, bits=bits, o=o, d=d, nears=nears, fars=fars, noises=noises, xyzs=xyzs, dirs=dirs, ts=ts, rays=rays, trips=trips, **P)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ---------------------------------------------------------------------------------------------------------------- tests/golden/ref_raymarch.npz
def golden_cases():
    """The march_rays_train cases recorded from the reference's kernels: every grid and shape, the parameter sets with max_steps = 64, 65 rays, none hostile."""
    return [(k, s, p) for k in range(len(GRID_KINDS)) for s in range(len(GRID_SHAPES)) for p in range(len(MARCH_PARAMS)) if MARCH_PARAMS[p]["max_steps"] == 64]


def near_far_inputs():
    """The 4096 rays of tests/test_gpu_raymarch.py::test_near_far_bit_equal: zero components, -0.0, a miss, origins inside -> rays_o, rays_d, aabb."""
    N = 4096
    rng = np.random.default_rng(2)
    o = rng.uniform(-3, 3, size=(N, 3)).astype(np.float32)
    o[:1024] = rng.uniform(-0.9, 0.9, size=(1024, 3))
    d = rng.normal(size=(N, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(3):
        d[100 + k::97, k] = 0.0
    d[7, 1] = -0.0; d[8] = [-0.0, 0.0, 1.0]
    o[9] = [5, 5, 5]; d[9] = [1, 0, 0]
    return o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32)


def digest(a):
    """SHA-256 of an array's bytes, every NaN first made the same quiet NaN -> u8 [32]."""
    import hashlib
    a = np.ascontiguousarray(a).copy()
    if a.dtype == np.float32:
        a[np.isnan(a)] = np.float32(np.nan)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the inference loop's shared inputs
def sigma_of(xyzs):
    """A fixed function of position: a soft ball that turns opaque fast.  numpy float32 here; tests/test_gpu_raymarch.py applies the same operations in torch."""
    r2 = (xyzs[:, 0] * xyzs[:, 0] + xyzs[:, 1] * xyzs[:, 1]) + xyzs[:, 2] * xyzs[:, 2]
    return np.maximum(F(0.49) - r2, F(0)) * F(800.0)


INFER_COLOUR = np.array([0.9, 0.5, 0.2], np.float32)


@functools.lru_cache(maxsize=None)
def infer_case(N=1024, H=16, max_steps=256, T_thresh=1e-2, hostile=True):
    """The loop of nerf/renderer.py:784-828 on the host, computed once per process: a ball of occupied cells (centres within 0.85) around sigma_of's smaller ball,
    make_rays' rays WITH the hostile ones (unless hostile=False), constant colours.  -> the inputs and, per round, what went into march_rays (n_alive, n_step, rays_alive, rays_t) and what
    came out of it and of composite_rays (xyzs, dirs, ts, loop passes, rays_alive and rays_t afterwards), then the final weights_sum, depth, image."""
    cells = np.stack(np.meshgrid(*[np.arange(H)] * 3, indexing="ij"), -1).reshape(-1, 3)
    occ = np.zeros(H ** 3, np.float32)
    occ[morton3D(cells)] = (np.linalg.norm((cells + 0.5) / H * 2 - 1, axis=1) < 0.85).astype(np.float32)
    bits = packbits(occ, 0.5)
    o, d, nears, fars, _ = make_rays(N, 1.0, H, seed=40, hostile=hostile)
    ws, dp, im = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    rounds = []
    rays_alive, rays_t, step = np.arange(N, dtype=np.int32), nears.copy(), 0
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts, trips = march_rays(n_alive, n_step, rays_alive, rays_t, o, d, 1.0, False, bits, 1, H, nears, fars, np.zeros(n_alive, np.float32), 0.0, max_steps,
                                           TRIP_CAP)
        after, t_after, ws, dp, im = composite_rays(n_alive, n_step, rays_alive, rays_t, sigma_of(xyzs), np.tile(INFER_COLOUR, (n_alive * n_step, 1)), ts, ws, dp, im,
                                                    T_thresh, False)
        rounds.append(dict(n_alive=n_alive, n_step=n_step, rays_alive=rays_alive, rays_t=rays_t, xyzs=xyzs, dirs=dirs, ts=ts, trips=trips, alive_after=after,
                           t_after=t_after))
        rays_alive, rays_t = after[after >= 0], t_after
        step += n_step
    case = dict(N=N, H=H, max_steps=max_steps, T_thresh=T_thresh, bits=bits, o=o, d=d, nears=nears, fars=fars, rounds=rounds, weights_sum=ws, depth=dp, image=im)
    for v in list(case.values()) + [x for r in rounds for x in r.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case
