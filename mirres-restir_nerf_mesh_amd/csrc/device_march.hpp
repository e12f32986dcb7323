// device_march.hpp — the per-ray code of the stage-0 ray-marching operators (raymarch.hip; torch-ngp raymarching/src/raymarching.cu): the occupancy-cell lookup, one
// iteration of the grid-accelerated march (raymarching.cu:396-465 / :759-827), and one compositing step forward (:541-568), backward (:651-693) and for
// inference (:874-908).  It is plain C++: the kernels include it as device code, a host compiler includes it as it stands (RM_FN then is `static inline`), and with
// -ffp-contract=off both give the same bits — tests/test_raymarch_host.py builds it for the host and holds it against the numpy restatement.
//
// FIXED arithmetic (DESIGN.md sections 3 and 5.13): fp32, every operation rounded on its own, IEEE division incl. the reciprocals, and each expression under the
// promotion rules of the reference's own C++: the cell index 0.5 * (c * mip_rbound + 1) * H is a DOUBLE product of a float sum, rounded to float where clamp() takes
// it and then truncated; mip_from_dt's dt * H * 0.5 is a float product times a double 0.5, rounded to float.  frexpf / scalbnf are exact.  The compositing
// exponential is mrf_exp (include/mirres_fmath.h) where the reference has the __expf intrinsic.
//
// Termination (the reference's loops can spin): a ray with a zero or non-finite direction or a NaN near / far takes no step (rm_ray_ok); the voxel-skipping
// do-while also ends at t >= far (t is not written after the outer loop, so no output changes) and when t + dt == t (absorption at large t), which ends the ray.
// RmMarch::trips counts the passes of both loops; a ray stops when it reaches RmMarch::max_trips (the kernels pass RM_NO_CAP: 2^32 - 1 passes of >= dt_min each are
// never needed below the absorption point).
#pragma once
#include <math.h>
#include <stdint.h>
#include "mirres_fmath.h"

#if defined(__HIPCC__)
#define RM_FN __host__ __device__ __forceinline__
#else
#define RM_FN static inline
#endif
#define RM_NO_CAP 0xffffffffu
#define RM_SQRT3 1.7320508075688772f

RM_FN float rm_clamp(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }                 // raymarching.cu:34-36: a NaN x gives lo
RM_FN float rm_sign(float x) { return copysignf(1.0f, x); }                                           // :30-32

RM_FN uint32_t rm_expand_bits(uint32_t v) {                                                             // :56-63
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
RM_FN uint32_t rm_morton3D(uint32_t x, uint32_t y, uint32_t z) { return rm_expand_bits(x) | (rm_expand_bits(y) << 1) | (rm_expand_bits(z) << 2); }   // :65-71
RM_FN uint32_t rm_morton3D_invert(uint32_t x) {                                                         // :73-81
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

RM_FN int rm_mip_from_pos(float x, float y, float z, float max_cascade) {                               // :42-47
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0, (float)e));
}
RM_FN int rm_mip_from_dt(float dt, float H, float max_cascade) {                                        // :49-54
    const float mx = (float)((double)(dt * H) * 0.5);
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0, (float)e));
}

// what is constant over a launch (raymarching.cu:375-386 / :742-751)
struct RmGrid {
    const uint8_t* bits;        // density_bitfield [C * H^3 / 8]
    uint32_t C, H;
    float bound, dt_gamma, dt_min, dt_max, rH;
    int contract;
};
RM_FN RmGrid rm_grid(const uint8_t* bits, uint32_t C, uint32_t H, float bound, int contract, float dt_gamma, uint32_t max_steps) {
    RmGrid g;
    g.bits = bits; g.C = C; g.H = H; g.bound = bound; g.contract = contract; g.dt_gamma = dt_gamma;
    g.dt_min = 2 * RM_SQRT3 / (float)max_steps;
    g.dt_max = 2 * RM_SQRT3 * bound / (float)H;
    g.rH = 1 / (float)H;
    return g;
}

// one ray on its way
struct RmMarch {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz, far;
    float t;
    uint32_t step, trips, max_trips;
    int done;                   // absorbed (t + dt == t in the skipping loop) or out of trips: the ray takes no further step
};
// a ray that may march at all: a direction with a finite, non-zero length and ordered near / far
RM_FN bool rm_ray_ok(float dx, float dy, float dz, float near, float far) {
    const float m = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
    return dx == dx && dy == dy && dz == dz && m > 0.0f && m < mrf_inf() && near == near && far == far;
}
// eps: 0 for march_rays_train's 1 / d (:377), 1e-10f for march_rays' 1 / (d + 1e-10f) (:744)
RM_FN RmMarch rm_march_begin(const RmGrid& g, float ox, float oy, float oz, float dx, float dy, float dz, float near, float far, float t_start, float noise, float eps,
                             uint32_t max_trips) {
    RmMarch m;
    m.ox = ox; m.oy = oy; m.oz = oz; m.dx = dx; m.dy = dy; m.dz = dz;
    m.rdx = 1 / (dx + eps); m.rdy = 1 / (dy + eps); m.rdz = 1 / (dz + eps);
    m.far = far;
    float t = t_start;
    t += rm_clamp(t * g.dt_gamma, g.dt_min, g.dt_max) * noise;                                          // :389-391 / :755-756
    m.t = t;
    m.step = 0; m.trips = 0; m.max_trips = max_trips;
    m.done = rm_ray_ok(dx, dy, dz, near, far) ? 0 : 1;
    return m;
}
RM_FN bool rm_march_live(const RmMarch& m, uint32_t num_steps) { return !m.done && m.t < m.far && m.step < num_steps; }

// the occupancy cell of a (clamped, possibly contracted) point at a level: its integer coordinates and its bit (:421-427)
RM_FN bool rm_cell(const RmGrid& g, int level, float mip_rbound, float cx, float cy, float cz, int& nx, int& ny, int& nz) {
    const float top = (float)(g.H - 1);
    nx = (int)rm_clamp((float)(0.5 * (cx * mip_rbound + 1) * g.H), 0.0f, top);
    ny = (int)rm_clamp((float)(0.5 * (cy * mip_rbound + 1) * g.H), 0.0f, top);
    nz = (int)rm_clamp((float)(0.5 * (cz * mip_rbound + 1) * g.H), 0.0f, top);
    const uint64_t index = (uint64_t)level * ((uint64_t)g.H * g.H * g.H) + rm_morton3D((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);
    return (g.bits[index / 8] & (1u << (index % 8))) != 0;
}

// One pass of the outer loop (:396-465).  True: a sample was taken — out = {cx, cy, cz, t after the step, dt} and m.step advanced; false: the ray skipped to the
// next cell (or stopped: m.done).
RM_FN bool rm_march_iter(const RmGrid& g, RmMarch& m, float out[5]) {
    m.trips++;
    if (m.trips >= m.max_trips) { m.done = 1; return false; }
    const float t = m.t;
    const float x = rm_clamp(m.ox + t * m.dx, -g.bound, g.bound);
    const float y = rm_clamp(m.oy + t * m.dy, -g.bound, g.bound);
    const float z = rm_clamp(m.oz + t * m.dz, -g.bound, g.bound);
    float dt = rm_clamp(t * g.dt_gamma, g.dt_min, g.dt_max);
    const int la = rm_mip_from_pos(x, y, z, (float)g.C), lb = rm_mip_from_dt(dt, (float)g.H, (float)g.C);
    const int level = la > lb ? la : lb;
    const float mip_bound = fminf(scalbnf(1.0f, level), g.bound);
    const float mip_rbound = 1 / mip_bound;
    float cx = x, cy = y, cz = z;
    const float mag = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    const bool outer = g.contract && mag > 1;
    if (outer) {                                                                                        // L-inf contraction (:413-419)
        const float s = (2 - 1 / mag) / mag;
        cx *= s; cy *= s; cz *= s;
    }
    int nx, ny, nz;
    const bool occ = rm_cell(g, level, mip_rbound, cx, cy, cz, nx, ny, nz);
    if (occ || outer) {
        m.step++;
        m.t = t + dt;
        out[0] = cx; out[1] = cy; out[2] = cz; out[3] = m.t; out[4] = dt;
        return true;
    }
    const float tx = (((nx + 0.5f + 0.5f * rm_sign(m.dx)) * g.rH * 2 - 1) * mip_bound - cx) * m.rdx;
    const float ty = (((ny + 0.5f + 0.5f * rm_sign(m.dy)) * g.rH * 2 - 1) * mip_bound - cy) * m.rdy;
    const float tz = (((nz + 0.5f + 0.5f * rm_sign(m.dz)) * g.rH * 2 - 1) * mip_bound - cz) * m.rdz;
    const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    float ts = t;
    do {
        dt = rm_clamp(ts * g.dt_gamma, g.dt_min, g.dt_max);
        const float tn = ts + dt;
        if (tn == ts) { m.done = 1; break; }                                                            // absorbed: the reference spins here for ever
        ts = tn;
        m.trips++;
        if (m.trips >= m.max_trips) { m.done = 1; break; }
    } while (ts < tt && ts < m.far);
    m.t = ts;
    return false;
}

// ---- compositing.  alpha of a sample (:543): sigma itself in alpha mode, else 1 - exp(-sigma * dt)
RM_FN float rm_alpha(float sigma, float dt, int alpha_mode) { return alpha_mode ? sigma : (1.0f - mrf_exp(-sigma * dt)); }

struct RmComp { float T, r, g, b, ws, d; };
RM_FN RmComp rm_comp_begin() { RmComp c; c.T = 1.0f; c.r = 0; c.g = 0; c.b = 0; c.ws = 0; c.d = 0; return c; }

// one sample of composite_rays_train's forward (:543-554) -> its weight; the caller stops the ray when c.T < T_thresh afterwards (:557)
RM_FN float rm_comp_fwd(RmComp& c, float sigma, float t, float dt, float cr, float cg, float cb, int alpha_mode) {
    const float alpha = rm_alpha(sigma, dt, alpha_mode);
    const float weight = alpha * c.T;
    c.r += weight * cr;
    c.g += weight * cg;
    c.b += weight * cb;
    c.ws += weight;
    c.d += weight * t;
    c.T *= 1.0f - alpha;
    return weight;
}

// the ray's forward results and cotangents as the backward reads them (:648, :666-677); gws is grad_weights_sum of the ray, gw the sample's grad_weights
struct RmCompFinal { float r, g, b, ws, d; float gr, gg, gb, gws, gd; };
// one sample of the backward (:653-678) -> grad_sigma; grad_rgb[3] written
RM_FN float rm_comp_bwd(RmComp& c, const RmCompFinal& f, float sigma, float t, float dt, float cr, float cg, float cb, float gw, int alpha_mode, float grad_rgb[3]) {
    const float alpha = rm_alpha(sigma, dt, alpha_mode);
    const float weight = alpha * c.T;
    c.r += weight * cr;
    c.g += weight * cg;
    c.b += weight * cb;
    c.ws += weight;
    c.d += weight * t;
    c.T *= 1.0f - alpha;
    grad_rgb[0] = f.gr * weight;
    grad_rgb[1] = f.gg * weight;
    grad_rgb[2] = f.gb * weight;
    const float grad_scale = alpha_mode ? (1.0f / (1.0f - alpha)) : dt;
    return grad_scale * (f.gr * (c.T * cr - (f.r - c.r)) + f.gg * (c.T * cg - (f.g - c.g)) + f.gb * (c.T * cb - (f.b - c.b)) + (f.gws + gw) * (c.T - (f.ws - c.ws)) +
                         f.gd * (c.T * t - (f.d - c.d)));
}

// one sample of composite_rays (inference, :879-896): the transmittance is 1 - weight_sum, and T (the value BEFORE the sample) decides the stop (:901)
struct RmInfer { float r, g, b, ws, d; };
RM_FN float rm_comp_infer(RmInfer& c, float sigma, float t, float dt, float cr, float cg, float cb, int alpha_mode) {
    const float alpha = rm_alpha(sigma, dt, alpha_mode);
    const float T = 1 - c.ws;
    const float weight = alpha * T;
    c.ws += weight;
    c.d += weight * t;
    c.r += weight * cr;
    c.g += weight * cg;
    c.b += weight * cb;
    return T;
}
