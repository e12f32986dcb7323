// device_radiance.hpp — the stage-0 radiance network's device code past the position encoder (NeRFNetwork.forward, nerf/network.py:146-174): all 16 outputs of
// sigma_net, the degree-4 spherical-harmonics direction encoder (shencoder/src/shencoder.cu:43-68 after SHEncoder.forward's normalisation, sphere_harmonics.py:82)
// and the bias-free colour net 31 -> 64 -> 64 -> 3 with mrf_sigmoid.  The position encoder is dn_encode of device_density.hpp, unchanged.
// The arithmetic is fixed: DESIGN.md section 5.14 and the note at the top of radiance.hip.
#pragma once
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"

namespace mr {

#define RD_SH 16                                     // degree 4: 16 outputs
#define RD_GEO 15                                    // geo_feat: outputs 1 .. 15 of sigma_net
#define RD_H16 (1 + RD_GEO)
#define RD_IN (RD_SH + RD_GEO)                       // the colour net's input, [sh, geo_feat] as torch.cat orders it (network.py:165)
#define RD_IN_PAD 32                                 // a row of C0 in LDS: 31 weights and one pad word that no chain reads
#define RD_HIDDEN 64
// LDS words: W0 [64][32], W1 transposed [64][16], C0 [64][32 padded], C1 [64][64], C2 transposed [64][4 padded]
#define RD_LDS_W0 0
#define RD_LDS_W1 (RD_LDS_W0 + DN_HIDDEN * DN_FEAT)
#define RD_LDS_C0 (RD_LDS_W1 + DN_HIDDEN * RD_H16)
#define RD_LDS_C1 (RD_LDS_C0 + RD_HIDDEN * RD_IN_PAD)
#define RD_LDS_C2 (RD_LDS_C1 + RD_HIDDEN * RD_HIDDEN)
#define RD_LDS_WORDS (RD_LDS_C2 + RD_HIDDEN * 4)

// torch's ReLU: a NaN stays a NaN (fmaxf would turn it into 0), so a NaN direction reaches rgb as the reference's does
MR_DEV float rd_relu(float a) { return a < 0.f ? 0.f : a; }

// The 16 real spherical harmonics of degree < 4 of the direction (dx, dy, dz), which need not be a unit vector.  No FMA anywhere: every product, sum and difference
// rounds on its own (-ffp-contract=off), the square root and the divisions are the IEEE operations.  A zero or non-finite direction gives NaN (0 / 0), as the
// reference's does.
MR_DEV void rd_sh(float dx, float dy, float dz, float out[RD_SH]) {
    const float s = (dx * dx + dy * dy) + dz * dz;
    const float n = sqrtf(s);
    const float x = dx / n, y = dy / n, z = dz / n;
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    out[0] = 0.28209479177387814f;
    out[1] = -0.48860251190291987f * y;
    out[2] = 0.48860251190291987f * z;
    out[3] = -0.48860251190291987f * x;
    out[4] = 1.0925484305920792f * xy;
    out[5] = -1.0925484305920792f * yz;
    out[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    out[7] = -1.0925484305920792f * xz;
    out[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    out[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    out[10] = 2.8906114426405538f * xy * z;
    out[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    out[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    out[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    out[14] = 1.4453057213202769f * z * (x2 - y2);
    out[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}

// all five weight matrices into LDS, once per block
MR_DEV void rd_stage_weights(const mirres_radiance_t& N, float* sw) {
    for (int i = threadIdx.x; i < DN_HIDDEN * DN_FEAT; i += DN_BLOCK) sw[RD_LDS_W0 + i] = N.grid.w0[i];
    for (int i = threadIdx.x; i < DN_HIDDEN * RD_H16; i += DN_BLOCK) sw[RD_LDS_W1 + i] = N.w1[(i % RD_H16) * DN_HIDDEN + i / RD_H16];       // [o][j] <- W1[j][o]
    for (int i = threadIdx.x; i < RD_HIDDEN * RD_IN_PAD; i += DN_BLOCK) {
        const int o = i / RD_IN_PAD, k = i % RD_IN_PAD;
        sw[RD_LDS_C0 + i] = k < RD_IN ? N.c0[o * RD_IN + k] : 0.f;
    }
    for (int i = threadIdx.x; i < RD_HIDDEN * RD_HIDDEN; i += DN_BLOCK) sw[RD_LDS_C1 + i] = N.c1[i];
    for (int i = threadIdx.x; i < RD_HIDDEN * 4; i += DN_BLOCK) sw[RD_LDS_C2 + i] = (i % 4) < 3 ? N.c2[(i % 4) * RD_HIDDEN + i / 4] : 0.f;  // [o][c] <- C2[c][o]
    __syncthreads();
}

// h16 = W1 . relu(W0 . feat): every output a k-ascending fmaf chain from 0; h1 feeds the 16 accumulators as it is produced.  h16[0] has dn_head's bits.
MR_DEV void rd_sigma_net(const float* sw, const float feat[DN_FEAT], float h16[RD_H16]) {
#pragma unroll
    for (int j = 0; j < RD_H16; j++) h16[j] = 0.f;
#pragma unroll 2
    for (int o = 0; o < DN_HIDDEN; o++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DN_FEAT; k++) acc = fmaf(feat[k], sw[RD_LDS_W0 + o * DN_FEAT + k], acc);
        const float h1 = fmaxf(acc, 0.f);
#pragma unroll
        for (int j = 0; j < RD_H16; j++) h16[j] = fmaf(h1, sw[RD_LDS_W1 + o * RD_H16 + j], h16[j]);
    }
}

// rgb = mrf_sigmoid(C2 . relu(C1 . relu(C0 . in))); only the first layer's 64 outputs live together, the second layer's feed the three chains as they are produced
MR_DEV void rd_color_net(const float* sw, const float in[RD_IN], float rgb[3]) {
    float a[RD_HIDDEN];
#pragma unroll
    for (int o = 0; o < RD_HIDDEN; o++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < RD_IN; k++) acc = fmaf(in[k], sw[RD_LDS_C0 + o * RD_IN_PAD + k], acc);
        a[o] = rd_relu(acc);
    }
    float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll 2
    for (int o = 0; o < RD_HIDDEN; o++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < RD_HIDDEN; k++) acc = fmaf(a[k], sw[RD_LDS_C1 + o * RD_HIDDEN + k], acc);
        const float h = rd_relu(acc);
        r = fmaf(h, sw[RD_LDS_C2 + 4 * o + 0], r);
        g = fmaf(h, sw[RD_LDS_C2 + 4 * o + 1], g);
        b = fmaf(h, sw[RD_LDS_C2 + 4 * o + 2], b);
    }
    rgb[0] = mrf_sigmoid(r); rgb[1] = mrf_sigmoid(g); rgb[2] = mrf_sigmoid(b);
}

}  // namespace mr
