// device_density.hpp — the stage-0 density network's device code (torch-ngp GridEncoder forward + the bias-free sigma_net head + mrf_exp), shared by the query kernels
// (density.hip) and the density grid's update (raymarch.hip k_grid_update): one definition, so a cell's sigma has the bits DensityField.density gives its point.
// The arithmetic is fixed: DESIGN.md section 5.11 and the note at the top of density.hip.
#pragma once
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"

namespace mr {

#define DN_BLOCK 256
#define DN_LEVELS MIRRES_DENSITY_MAX_LEVELS
#define DN_FEAT (2 * DN_LEVELS)
#define DN_HIDDEN 64

// get_grid_index (gridencoder.cu:66-84) for D = 3, align_corners False.  The stride loop's outcome depends on the level alone, so the host has decided it
// (mirres_density_layout: `hashed`): a level whose final stride exceeds hashmap_size takes the hash, every other level went through all three axes.
MR_DEV uint32_t dn_index(uint32_t x, uint32_t y, uint32_t z, uint32_t s1, uint32_t hs, bool hashed) {
    uint32_t index = hashed ? (x * 1u) ^ (y * 2654435761u) ^ (z * 805459861u) : x + y * s1 + z * (s1 * s1);
    if (index >= hs) index %= hs;                                  // index % hashmap_size; the division only where it changes the value
    return index;
}

// features of one point; false (and 32 zeros) when a coordinate is out of bounds: u < 0, u > 1 or not finite (gridencoder.cu:110-135; NaN counts as outside)
MR_DEV bool dn_encode(const mirres_density_t& N, float x, float y, float z, float bound, float feat[DN_FEAT]) {
    const float den = 2.0f * bound;
    const float u[3] = {(x + bound) / den, (y + bound) / den, (z + bound) / den};
#pragma unroll
    for (int i = 0; i < DN_FEAT; i++) feat[i] = 0.f;
    if (!(u[0] >= 0.f && u[0] <= 1.f && u[1] >= 0.f && u[1] <= 1.f && u[2] >= 0.f && u[2] <= 1.f)) return false;
    const float2* __restrict__ table = (const float2*)N.table;
#pragma unroll
    for (int l = 0; l < DN_LEVELS; l++) {
        if (l >= N.num_levels) continue;
        const float scale = N.scale[l];
        const uint32_t s1 = (uint32_t)N.resolution[l] + 1u, hs = (uint32_t)(N.offsets[l + 1] - N.offsets[l]);
        const bool hashed = N.hashed[l] != 0;
        const float2* __restrict__ g = table + (size_t)N.offsets[l];
        float f[3], o[3]; uint32_t c[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            float p = u[d] * scale;
            p = p + 0.5f;
            const float cell = floorf(p);
            f[d] = p - cell; o[d] = 1.0f - f[d];
            c[d] = (uint32_t)cell;
        }
        float2 v[8];
#pragma unroll
        for (int idx = 0; idx < 8; idx++)
            v[idx] = g[dn_index(c[0] + (idx & 1), c[1] + ((idx >> 1) & 1), c[2] + ((idx >> 2) & 1), s1, hs, hashed)];
        float r0 = 0.f, r1 = 0.f;
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            float w = 1.0f;
            w = w * ((idx & 1) ? f[0] : o[0]);
            w = w * ((idx & 2) ? f[1] : o[1]);
            w = w * ((idx & 4) ? f[2] : o[2]);
            r0 = r0 + w * v[idx].x;
            r1 = r1 + w * v[idx].y;
        }
        feat[2 * l] = r0; feat[2 * l + 1] = r1;
    }
    return true;
}

// sigma = exp(W1[0, :] . relu(W0 . feat)); sw0 [64][32], sw1 [64] in LDS
MR_DEV float dn_head(const float* sw0, const float* sw1, const float feat[DN_FEAT]) {
    float h = 0.f;
#pragma unroll 2
    for (int o = 0; o < DN_HIDDEN; o++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DN_FEAT; k++) acc = fmaf(feat[k], sw0[o * DN_FEAT + k], acc);
        h = fmaf(fmaxf(acc, 0.f), sw1[o], h);
    }
    return mrf_exp(h);
}

MR_DEV void dn_stage_weights(const mirres_density_t& N, float* sw0, float* sw1) {
    for (int i = threadIdx.x; i < DN_HIDDEN * DN_FEAT; i += DN_BLOCK) sw0[i] = N.w0[i];
    if (threadIdx.x < DN_HIDDEN) sw1[threadIdx.x] = N.w1[threadIdx.x];
    __syncthreads();
}

// what every entry that takes a net checks before a launch; need = 1: an entry that reads the table and the levels alone (w0 and w1 may be NULL), 0: the levels alone
static bool dn_net_ok(const mirres_density_t* N, const char* who, int need = 2) {
    if (!N) { set_error("%s: net is NULL", who); return false; }
    if (N->num_levels < 1 || N->num_levels > DN_LEVELS) { set_error("%s: num_levels %d outside [1, %d]", who, N->num_levels, DN_LEVELS); return false; }
    if (need >= 2 && (!N->table || !N->w0 || !N->w1)) { set_error("%s: net has a NULL table / w0 / w1", who); return false; }
    if (need >= 1 && !N->table) { set_error("%s: net has a NULL table", who); return false; }
    if (N->offsets[0] < 0) { set_error("%s: negative level offset", who); return false; }
    for (int l = 0; l < N->num_levels; l++) {
        if (N->offsets[l + 1] <= N->offsets[l] || N->resolution[l] < 1 || N->resolution[l] > (1 << 24) || !(N->scale[l] >= 0.f) || !(N->scale[l] <= 16777216.f)) {
            set_error("%s: bad level %d (offsets %d .. %d, resolution %d, scale %g): fill the table with mirres_density_layout", who, l, N->offsets[l], N->offsets[l + 1],
                      N->resolution[l], (double)N->scale[l]);
            return false;
        }
        // a dense level's index x + y s + z s^2 must stay inside 32 bits (it does whenever the final stride s^3 <= hashmap_size)
        const unsigned long long s1 = (unsigned long long)N->resolution[l] + 1ull, hs = (unsigned long long)(N->offsets[l + 1] - N->offsets[l]);
        if (!N->hashed[l] && s1 * s1 * s1 > hs) { set_error("%s: level %d is marked dense but (resolution + 1)^3 exceeds its %llu entries", who, l, hs); return false; }
    }
    return true;
}

}  // namespace mr
