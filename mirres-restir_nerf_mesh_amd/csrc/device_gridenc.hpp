// device_gridenc.hpp — torch-ngp's GridEncoder as an operator of its own (gridencoder/src/gridencoder.cu: kernel_grid :87-244, kernel_grid_backward :247-339,
// kernel_input_backward :343-368), restated for D in {2, 3} and C in {1, 2, 4, 8} channels with gridtype, align_corners, interpolation and max_level at run time.
// The arithmetic is FIXED and is that of device_density.hpp's cell primitives (dn_unit, dn_cell, dn_corner, dn_weight) wherever the two
// overlap, so that for D = 3, C = 2, hash, align_corners False, linear the features have dn_encode's bits and the input gradient k_radiance_points_bwd_pos'
// (radiance_pos.hip).  The two stay separate implementations: the switches here are run-time values, and each is the other's check (tests/test_gpu_gridenc.py):
//   u[d] = (x[d] + bound) / (2.0f * bound); in bounds: every u[d] >= 0 && u[d] <= 1 (NaN: outside);
//   per level: p = u[d] * scale; p = p + (align_corners ? 0.0f : 0.5f); cell = floorf(p); f = p - cell;
//              smoothstep: s = (f * f) * (3.0f - 2.0f * f), ds = (6.0f * f) * (1.0f - f); linear: s = f, ds = 1;
//   corners idx ascending: w = 1; for d ascending: w = w * (bit d of idx ? s[d] : 1.0f - s[d]); r[ch] = r[ch] + w * table[entry][ch];
//   entry = get_grid_index (gridencoder.cu:66-84) in uint32 arithmetic (gn_strides of grid_layout.hpp, gn_index below).
// Every operation rounds once (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "grid_layout.hpp"

namespace mr {

#define GN_BLOCK 256
#define GN_LEVELS MIRRES_DENSITY_MAX_LEVELS

// what a level needs besides the point: wave-uniform
struct GnLevel {
    float scale, half;           // half: 0.0f with align_corners, else 0.5f
    uint32_t hs, stride[3];
    bool hash, smooth;
    size_t first;                // first entry of the level in the table
};

GN_HD GnLevel gn_level(const mirres_gridenc_t& G, int D, int l) {
    GnLevel V;
    V.scale = G.scale[l];
    V.half = G.align_corners ? 0.0f : 0.5f;
    V.hs = (uint32_t)(G.offsets[l + 1] - G.offsets[l]);
    const uint32_t res = (uint32_t)G.resolution[l];
    const uint32_t last = gn_strides(D, G.align_corners ? res : res + 1u, V.hs, V.stride);
    V.hash = G.gridtype == 0 && last > V.hs;
    V.smooth = G.interpolation == 1;
    V.first = (size_t)G.offsets[l];
    return V;
}

template <int D>
MR_DEV uint32_t gn_index(const GnLevel& V, const uint32_t c[D]) {
    uint32_t index;
    if (V.hash) {
        index = c[0] * 1u ^ c[1] * 2654435761u;
        if (D == 3) index ^= c[2] * 805459861u;
    } else {
        index = c[0] * V.stride[0] + c[1] * V.stride[1];
        if (D == 3) index += c[2] * V.stride[2];
    }
    return index % V.hs;                                             // < hs: inside the level
}

// u of one point; false when it is out of bounds
template <int D>
MR_DEV bool gn_unit(const float* __restrict__ pos, long long i, float bound, float u[D]) {
    const float den = 2.0f * bound;
    bool in = true;
#pragma unroll
    for (int d = 0; d < D; d++) {
        u[d] = (pos[D * i + d] + bound) / den;
        in = in && (u[d] >= 0.f && u[d] <= 1.f);
    }
    return in;
}

// the cell, the interpolation weights s (o = 1 - s) and their derivative ds of one point on one level
template <int D>
MR_DEV void gn_cell(const GnLevel& V, const float u[D], uint32_t c[D], float s[D], float o[D], float ds[D]) {
#pragma unroll
    for (int d = 0; d < D; d++) {
        float p = u[d] * V.scale;
        p = p + V.half;
        const float cell = floorf(p);
        const float f = p - cell;
        c[d] = (uint32_t)cell;
        if (V.smooth) {
            s[d] = (f * f) * (3.0f - 2.0f * f);
            ds[d] = (6.0f * f) * (1.0f - f);
        } else {
            s[d] = f;
            ds[d] = 1.0f;
        }
        o[d] = 1.0f - s[d];
    }
}

template <int D>
MR_DEV uint32_t gn_corner(const GnLevel& V, const uint32_t c[D], int idx) {
    uint32_t cc[D];
#pragma unroll
    for (int d = 0; d < D; d++) cc[d] = c[d] + ((idx >> d) & 1);
    return gn_index<D>(V, cc);
}

template <int D>
MR_DEV float gn_weight(const float s[D], const float o[D], int idx) {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < D; d++) w = w * (((idx >> d) & 1) ? s[d] : o[d]);
    return w;
}

// one entry's C channels, by the widest load its alignment allows (an entry is C * 4 bytes and starts at a multiple of that)
template <int C>
MR_DEV void gn_load(const float* __restrict__ p, float v[C]) {
    if (C == 1) { v[0] = p[0]; }
    else if (C == 2) { const float2 t = *(const float2*)p; v[0] = t.x; v[1] = t.y; }
    else {
#pragma unroll
        for (int k = 0; k < C; k += 4) { const float4 t = *(const float4*)(p + k); v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w; }
    }
}

template <int C>
MR_DEV void gn_store(float* __restrict__ p, const float v[C]) {
    if (C == 1) { p[0] = v[0]; }
    else if (C == 2) { *(float2*)p = make_float2(v[0], v[1]); }
    else {
#pragma unroll
        for (int k = 0; k < C; k += 4) *(float4*)(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

}  // namespace mr
