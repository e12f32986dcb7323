// device_density.hpp — the stage-0 density network's device code (torch-ngp GridEncoder forward + the bias-free sigma_net head + mrf_exp), shared by the query kernels
// (density.hip), the density grid's update (raymarch.hip k_grid_update) and the radiance network (radiance*.hip), so a cell's sigma has the bits DensityField.density
// gives its point.  The hash-grid CELL of the reference's configuration (D = 3, C = 2, hash, align_corners False, linear) is written here ONCE, as dn_unit, dn_cell,
// dn_corner, dn_weight and dn_gather over one DnLevel: every fused kernel that needs a point's cell — dn_encode below, the table scatter and the position adjoint of the
// training step (radiance_bwd.hip, radiance_pos.hip), the total-variation term (grid_tv.hip) — calls them.  The arithmetic is fixed: DESIGN.md section 5.11 and the note
// at the top of density.hip.
#pragma once
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_scan.hpp"
#include "grid_layout.hpp"

namespace mr {

#define DN_BLOCK 256
#define DN_LEVELS MIRRES_DENSITY_MAX_LEVELS
#define DN_FEAT (2 * DN_LEVELS)
#define DN_HIDDEN 64

// what a level needs besides the point: wave-uniform
struct DnLevel {
    float scale;
    uint32_t s1, hs;             // resolution + 1 and the level's entries (hashmap_size)
    bool hashed;
    int first;                   // first entry of the level in the table; widened where it is used (as a size_t field it costs k_tv_points two VGPRs)
};

MR_DEV DnLevel dn_level(const mirres_density_t& N, int l) {
    return {N.scale[l], (uint32_t)N.resolution[l] + 1u, (uint32_t)(N.offsets[l + 1] - N.offsets[l]), N.hashed[l] != 0, N.offsets[l]};
}

// u of one point; false when a coordinate is out of bounds: u < 0, u > 1 or not finite (gridencoder.cu:110-135; NaN counts as outside)
MR_DEV bool dn_unit(float x, float y, float z, float bound, float u[3]) {
    const float den = 2.0f * bound;
    u[0] = (x + bound) / den; u[1] = (y + bound) / den; u[2] = (z + bound) / den;
    return u[0] >= 0.f && u[0] <= 1.f && u[1] >= 0.f && u[1] <= 1.f && u[2] >= 0.f && u[2] <= 1.f;
}

// the cell c (corner 0 of the interpolation), the fractions f and o = 1 - f of one point on one level
MR_DEV void dn_cell(const DnLevel& V, const float u[3], uint32_t c[3], float f[3], float o[3]) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float p = u[d] * V.scale;
        p = p + 0.5f;
        const float cell = floorf(p);
        f[d] = p - cell; o[d] = 1.0f - f[d];
        c[d] = (uint32_t)cell;
    }
}

// get_grid_index (gridencoder.cu:66-84) for D = 3, align_corners False.  The stride loop's outcome depends on the level alone, so the host has decided it
// (mirres_density_layout: `hashed`): a level whose final stride exceeds hashmap_size takes the hash, every other level went through all three axes.
MR_DEV uint32_t dn_index(uint32_t x, uint32_t y, uint32_t z, uint32_t s1, uint32_t hs, bool hashed) {
    uint32_t index = hashed ? (x * 1u) ^ (y * 2654435761u) ^ (z * 805459861u) : x + y * s1 + z * (s1 * s1);
    if (index >= hs) index %= hs;                                  // index % hashmap_size; the division only where it changes the value
    return index;
}

// the entry of corner idx = 0..7 of cell c (bit d of idx: +1 on axis d); < hs: inside the level
MR_DEV uint32_t dn_corner(const DnLevel& V, const uint32_t c[3], int idx) {
    return dn_index(c[0] + (idx & 1), c[1] + ((idx >> 1) & 1), c[2] + ((idx >> 2) & 1), V.s1, V.hs, V.hashed);
}

// the interpolation weight of corner idx
MR_DEV float dn_weight(const float f[3], const float o[3], int idx) {
    float w = 1.0f;
    w = w * ((idx & 1) ? f[0] : o[0]);
    w = w * ((idx & 2) ? f[1] : o[1]);
    w = w * ((idx & 4) ? f[2] : o[2]);
    return w;
}

// the eight corner entries of cell c, all loads issued before any is used
MR_DEV void dn_gather(const float2* __restrict__ table, const DnLevel& V, const uint32_t c[3], float2 v[8]) {
    const float2* __restrict__ g = table + (size_t)V.first;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) v[idx] = g[dn_corner(V, c, idx)];
}

// grad[e] += (v0, v1) for the lanes that are ok, by lane PAIRS: the even lane issues channel 0 and the odd lane channel 1 of the same entry — first the even lane's
// entry, then the odd lane's — so one entry is one memory request.  g: the level's part of the table's gradient.  EVERY lane of the wave must arrive (the shuffles
// read the partner lane); a lane that is not ok adds nothing, and its e is not used.
MR_DEV void dn_pair_add(float* g, uint32_t e, bool ok, float v0, float v1) {
    const int odd = lane_id() & 1;
    const uint32_t pe = (uint32_t)__shfl_xor((int)e, 1, 64);
    const int pok = __shfl_xor(ok ? 1 : 0, 1, 64);
    const float px = __shfl_xor(odd ? v0 : v1, 1, 64);             // the even lane receives the odd lane's channel 0, the odd lane the even lane's channel 1
    if (odd ? pok : (int)ok) atomicAdd(g + 2 * (size_t)(odd ? pe : e) + odd, odd ? px : v0);        // the even lane's entry
    if (odd ? (int)ok : pok) atomicAdd(g + 2 * (size_t)(odd ? e : pe) + odd, odd ? v1 : px);        // the odd lane's entry
}

// features of one point; false (and 32 zeros) when the point is out of bounds (dn_unit)
MR_DEV bool dn_encode(const mirres_density_t& N, float x, float y, float z, float bound, float feat[DN_FEAT]) {
#pragma unroll
    for (int i = 0; i < DN_FEAT; i++) feat[i] = 0.f;
    float u[3];
    if (!dn_unit(x, y, z, bound, u)) return false;
#pragma unroll
    for (int l = 0; l < DN_LEVELS; l++) {
        if (l >= N.num_levels) continue;
        const DnLevel V = dn_level(N, l);
        float f[3], o[3]; uint32_t c[3];
        dn_cell(V, u, c, f, o);
        float2 v[8];
        dn_gather((const float2*)N.table, V, c, v);
        float r0 = 0.f, r1 = 0.f;
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float w = dn_weight(f, o, idx);
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
    if (!grid_levels_ok(who, "mirres_density_layout", N->num_levels, N->offsets, N->resolution, N->scale)) return false;
    for (int l = 0; l < N->num_levels; l++) {
        // a dense level's index x + y s + z s^2 must stay inside 32 bits (it does whenever the final stride s^3 <= hashmap_size < 2^31; s <= 2048 keeps s^3 exact here)
        const unsigned long long s1 = (unsigned long long)N->resolution[l] + 1ull, hs = (unsigned long long)(N->offsets[l + 1] - N->offsets[l]);
        if (!N->hashed[l] && (s1 > 2048ull || s1 * s1 * s1 > hs)) { set_error("%s: level %d is marked dense but (resolution + 1)^3 exceeds its %llu entries", who, l, hs); return false; }
    }
    return true;
}

}  // namespace mr
