// radiance_pos.hip — the position adjoint of mirres_radiance_points (radiance.hip): from the cotangents of sigma and rgb to d / d pos, what the reference's stage 1
// asks of self.rgb(xyzs, dirs) under --enable_offset_nerf_grad (nerf/renderer.py:1046-1052: xyzs[mask] is not detached), carried there by the grid encoder's dy_dx
// (gridencoder/src/gridencoder.cu:198-243, 343-368) and divided by 2 bound (gridencoder/grid.py:156).  The parameters' gradients are radiance_bwd.hip's; the
// direction gets none (in stage 1 it comes from the camera, not from the mesh).
// One thread per point, no atomics, nothing taped: the forward is recomputed with the shared device functions (dn_encode and the cell primitives under it, rd_sh, the chains of rd_sigma_net and
// rd_color_net on the weights rd_stage_weights put into LDS) and the cotangent goes back under mirres_radiance_points_bwd's rules:
//   colour net   d_pre = grad_rgb * (rgb (1 - rgb)); a ReLU passes the cotangent where its output is > 0; every adjoint sum is an fmaf chain from 0 over the layer's
//                outputs ascending (the chains of k_radiance_points_bwd); the first layer's d_in[16..30] is d_h16[1..15];
//   sigma        d_h16[0] = grad_sigma * mrf_exp(clamp(h16[0], -15, 15));  d_feat = W0^T (relu'(h1) W1^T d_h16);
//   encoder      per level l ascending and axis a: dy_dx[a][ch] = sum over the four corner pairs that differ in a alone (pairs ascending: bit 0 of the pair is the lower
//                of the two other axes) of w * (table[right][ch] - table[left][ch]), w = (scale_l * w_lower) * w_upper with the forward's fractions, cell and entry
//                indices; grad_u[a] = grad_u[a] + d_feat[2 l + ch] * dy_dx[a][ch], channels ascending; grad_pos[a] = grad_u[a] / (2 bound).  Every operation of
//                this part rounds on its own: no FMA (-ffp-contract=off).  The eight corners of a level are gathered once (they are the four pairs of every axis).
// A point out of bounds or not finite has constant (zero) features: exactly 0, 0, 0.
// What a ReLU let through is kept as one bit per neuron (three 64-bit words) instead of the activations; the registers' peak is the 64 cotangents of a hidden layer
// beside the 16 of h16.  Every register array is indexed by compile-time constants only; loops over a layer's 64 neurons that read LDS stay rolled (radiance_bwd.hip).
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"
#include "device_radiance.hpp"

namespace mr {

__global__ void __launch_bounds__(DN_BLOCK) k_radiance_points_bwd_pos(mirres_radiance_t N, const float* __restrict__ pos, const float* __restrict__ dirs, long long n,
                                                                      float bound, const float* __restrict__ grad_sigma, const float* __restrict__ grad_rgb,
                                                                      float* __restrict__ grad_pos) {
    __shared__ __attribute__((aligned(16))) float sw[RD_LDS_WORDS];
    rd_stage_weights(N, sw);
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= n) return;                                              // no barrier below
    const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
    float dh16[RD_H16];
    uint64_t m1 = 0;                                                 // sigma_net's hidden layer: bit o = h1[o] > 0
    {
        uint64_t c0m = 0, c1m = 0;                                   // the colour net's layers 0 and 1 likewise
        float in[RD_IN], h0;
        {
            float feat[DN_FEAT], h16[RD_H16];
            if (!dn_encode(N.grid, x, y, z, bound, feat)) {
                grad_pos[3 * i] = 0.f; grad_pos[3 * i + 1] = 0.f; grad_pos[3 * i + 2] = 0.f;
                return;
            }
            // rd_sigma_net's chains, keeping which neurons passed
#pragma unroll
            for (int j = 0; j < RD_H16; j++) h16[j] = 0.f;
#pragma unroll 2
            for (int o = 0; o < DN_HIDDEN; o++) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < DN_FEAT; k++) acc = fmaf(feat[k], sw[RD_LDS_W0 + o * DN_FEAT + k], acc);
                const float h1 = fmaxf(acc, 0.f);
                m1 |= (uint64_t)(h1 > 0.f) << o;
#pragma unroll
                for (int j = 0; j < RD_H16; j++) h16[j] = fmaf(h1, sw[RD_LDS_W1 + o * RD_H16 + j], h16[j]);
            }
            h0 = h16[0];
#pragma unroll
            for (int k = 0; k < RD_GEO; k++) in[RD_SH + k] = h16[1 + k];
        }
        rd_sh(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], in);
        float d1[RD_HIDDEN];                                         // first a0, then d_a1pre
        {   // rd_color_net's chains
#pragma unroll
            for (int o = 0; o < RD_HIDDEN; o++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < RD_IN; k++) s = fmaf(in[k], sw[RD_LDS_C0 + o * RD_IN_PAD + k], s);
                d1[o] = rd_relu(s);
                c0m |= (uint64_t)!(d1[o] <= 0.f) << o;
            }
            float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll 2
            for (int o = 0; o < RD_HIDDEN; o++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < RD_HIDDEN; k++) s = fmaf(d1[k], sw[RD_LDS_C1 + o * RD_HIDDEN + k], s);
                const float h = rd_relu(s);
                c1m |= (uint64_t)!(h <= 0.f) << o;
                r = fmaf(h, sw[RD_LDS_C2 + 4 * o + 0], r);
                g = fmaf(h, sw[RD_LDS_C2 + 4 * o + 1], g);
                b = fmaf(h, sw[RD_LDS_C2 + 4 * o + 2], b);
            }
            const float rgb[3] = {mrf_sigmoid(r), mrf_sigmoid(g), mrf_sigmoid(b)};
            float dout[3];
#pragma unroll
            for (int c = 0; c < 3; c++) dout[c] = grad_rgb[3 * i + c] * (rgb[c] * (1.0f - rgb[c]));
            // d_a1pre = relu'(a1) C2^T d_out
#pragma unroll
            for (int o = 0; o < RD_HIDDEN; o++) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) s = fmaf(dout[c], sw[RD_LDS_C2 + 4 * o + c], s);
                d1[o] = ((c1m >> o) & 1) ? s : 0.f;
            }
        }
        // per neuron k of layer 0: d_a0[k] = C1[:, k] . d_a1pre (o ascending), through its ReLU, then into d_geo = rows 16..30 of C0^T d_a0pre (k ascending)
#pragma unroll
        for (int j = 0; j < RD_H16; j++) dh16[j] = 0.f;
#pragma unroll 2
        for (int k = 0; k < RD_HIDDEN; k++) {
            float s = 0.f;
#pragma unroll
            for (int o = 0; o < RD_HIDDEN; o++) s = fmaf(sw[RD_LDS_C1 + o * RD_HIDDEN + k], d1[o], s);
            s = ((c0m >> k) & 1) ? s : 0.f;
#pragma unroll
            for (int j = 0; j < RD_GEO; j++) dh16[1 + j] = fmaf(sw[RD_LDS_C0 + k * RD_IN_PAD + RD_SH + j], s, dh16[1 + j]);
        }
        dh16[0] = grad_sigma ? grad_sigma[i] * mrf_exp(fminf(fmaxf(h0, -15.0f), 15.0f)) : 0.f;
    }
    // d_feat = W0^T (relu'(h1) W1^T d_h16), o ascending
    float dfeat[DN_FEAT];
#pragma unroll
    for (int k = 0; k < DN_FEAT; k++) dfeat[k] = 0.f;
#pragma unroll 2
    for (int o = 0; o < DN_HIDDEN; o++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RD_H16; k++) s = fmaf(sw[RD_LDS_W1 + o * RD_H16 + k], dh16[k], s);
        s = ((m1 >> o) & 1) ? s : 0.f;
#pragma unroll
        for (int k = 0; k < DN_FEAT; k++) dfeat[k] = fmaf(sw[RD_LDS_W0 + o * DN_FEAT + k], s, dfeat[k]);
    }
    // the encoder's input gradient over the forward's cell, fractions and entries (device_density.hpp's primitives; the point is in bounds)
    float u[3];
    dn_unit(x, y, z, bound, u);
    float gu[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < DN_LEVELS; l++) {
        if (l >= N.grid.num_levels) continue;
        const DnLevel V = dn_level(N.grid, l);
        float f[3], o[3]; uint32_t c[3];
        dn_cell(V, u, c, f, o);
        float2 v[8];
        dn_gather((const float2*)N.grid.table, V, c, v);
        const float g0 = dfeat[2 * l], g1 = dfeat[2 * l + 1];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;      // the two other axes, ascending
            float r0 = 0.f, r1 = 0.f;
#pragma unroll
            for (int pr = 0; pr < 4; pr++) {
                float w = V.scale;
                w = w * ((pr & 1) ? f[lo] : o[lo]);
                w = w * ((pr & 2) ? f[hi] : o[hi]);
                const int left = ((pr & 1) << lo) | (((pr >> 1) & 1) << hi), right = left | (1 << a);
                r0 = r0 + w * (v[right].x - v[left].x);
                r1 = r1 + w * (v[right].y - v[left].y);
            }
            gu[a] = gu[a] + g0 * r0;
            gu[a] = gu[a] + g1 * r1;
        }
    }
    const float den = 2.0f * bound;
    grad_pos[3 * i] = gu[0] / den; grad_pos[3 * i + 1] = gu[1] / den; grad_pos[3 * i + 2] = gu[2] / den;
}

}  // namespace mr
using namespace mr;

extern "C" int mirres_radiance_points_bwd_pos(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, const float* grad_sigma,
                                              const float* grad_rgb, float* grad_pos, void* stream) {
    if (!net) { set_error("mirres_radiance_points_bwd_pos: net is NULL"); return MIRRES_E_ARG; }
    if (!dn_net_ok(&net->grid, "mirres_radiance_points_bwd_pos")) return MIRRES_E_ARG;
    if (!net->w1 || !net->c0 || !net->c1 || !net->c2) { set_error("mirres_radiance_points_bwd_pos: net has a NULL w1 / c0 / c1 / c2"); return MIRRES_E_ARG; }
    if (n < 0 || n > (1LL << 38) || (n > 0 && (!pos || !dirs || !grad_rgb || !grad_pos)) || !(bound > 0.f) || !(bound < 3.0e38f)) {
        set_error("mirres_radiance_points_bwd_pos: bad argument (n %lld, bound %g, pos / dirs / grad_rgb / grad_pos %s)", n, (double)bound,
                  (pos && dirs && grad_rgb && grad_pos) ? "given" : "NULL");
        return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    k_radiance_points_bwd_pos<<<grid_for((size_t)n, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(*net, pos, dirs, n, bound, grad_sigma, grad_rgb, grad_pos);
    MR_LAUNCH_CHECK("radiance_points_bwd_pos");
    return MIRRES_OK;
}
