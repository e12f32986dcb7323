// grid_layout.hpp — the level table of torch-ngp's GridEncoder on the host: GridEncoder.__init__ (gridencoder/grid.py:104-135) with the kernel's per-level quantities
// (gridencoder.cu:137-139), and the range checks of a filled table.  One definition behind mirres_density_layout (density.hip: D = 3, hash, align_corners False) and
// mirres_gridenc_layout (gridenc.hip), which are argument checks plus a call, and behind dn_net_ok and gn_ok.  get_grid_index's stride loop (gn_strides) is defined
// here because the table's `hashed` flag is its outcome; device_gridenc.hpp's gn_level is its one device caller (the fused kernels, which include this file through
// device_density.hpp, never call it).
#pragma once
#include <math.h>
#include <stdint.h>
#include "engine.hpp"

namespace mr {

#define GN_HD __host__ __device__ __forceinline__

// get_grid_index's stride loop (gridencoder.cu:68-75), which depends on the level alone: stride[d] = the factor of axis d, 0 for an axis the loop no longer reaches
// (stride > hashmap_size: that axis adds nothing to the index).  Returns the final stride; uint32 arithmetic as in the reference, wrap-around included.
// Written without an early exit (once s > hs it stays so, because s no longer changes), so that the three strides stay in registers: a loop with a data-dependent
// exit indexes the array dynamically, and the compiler then moves it to LDS.
GN_HD uint32_t gn_strides(int D, uint32_t factor, uint32_t hs, uint32_t stride[3]) {
    uint32_t s = 1;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const bool on = d < D && s <= hs;
        stride[d] = on ? s : 0u;
        s = on ? s * factor : s;
    }
    return s;
}

// Fills offsets[0 .. MAX_LEVELS], resolution, hashed and scale (the levels past num_levels: zeros, their offsets the total) and returns the number of entries, or
// MIRRES_E_ARG with the error set.  The caller has checked its arguments: D in {2, 3}, 1 <= num_levels <= MAX_LEVELS, per_level_scale > 0, 1 <= base_resolution,
// log2_hashmap_size <= 26.  `hash`: gridtype 'hash' (a tiled grid never hashes).
// `wrap`: the ONE place where the two entries differ.  true (mirres_gridenc_layout): `hashed` is the outcome of gn_strides, the reference's uint32 loop, whose product
// can wrap below the level's size (resolution + 1 = 65537: 65537^2 = 2^32 + 131073), after which the reference, and gridenc.hip with it, index the level densely with
// wrapped strides.  false (mirres_density_layout): the product is taken without wrapping and such a level is hashed, because dn_index does not restate wrapped strides.
static long long grid_layout(const char* who, int D, bool align_corners, bool hash, bool wrap, int num_levels, double per_level_scale, int base_resolution, int log2_hashmap_size,
                             int* offsets, int* resolution, int* hashed, float* scale) {
    const float S = (float)log2(per_level_scale);                   // the `const float S` gridencoder.cu's kernels receive (grid.py:38)
    const long long max_params = 1LL << log2_hashmap_size;
    long long offset = 0;
    for (int l = 0; l < MIRRES_DENSITY_MAX_LEVELS; l++) { offsets[l + 1] = 0; resolution[l] = 0; hashed[l] = 0; scale[l] = 0.f; }
    offsets[0] = 0;
    for (int l = 0; l < num_levels; l++) {
        // grid.py:128-130: min(max_params, side^D) from the Python-side resolution, rounded up to a multiple of 8.  The product saturates just above max_params after
        // every axis, so it is exact below the clamp and cannot overflow above it: side^3 itself passes 2^63 from a resolution of 2^21
        const double res = ceil((double)base_resolution * pow(per_level_scale, (double)l));
        const long long side = res >= (double)max_params ? max_params + 1 : (long long)res + (align_corners ? 0 : 1);
        long long params = 1;
        for (int d = 0; d < D; d++) { params *= side; if (params > max_params) params = max_params + 1; }
        if (params > max_params) params = max_params;
        params = (params + 7) / 8 * 8;
        offsets[l] = (int)offset;
        offset += params;
        // not reachable through either entry today: 16 levels of at most 2^26 entries are 2^30; kept for a caller with other limits, whose offsets would not fit an int
        if (offset > 0x7FFFFFFFLL) { set_error("%s: %lld entries do not fit the 32-bit offsets of the reference's table", who, offset); return MIRRES_E_ARG; }
        // gridencoder.cu:138-139 with exp2f correctly rounded: t = float(l) * S, e = float(exp2(double(t))), scale = e * float(H) - 1.0f, each step rounded to fp32
        const float t = (float)l * S;
        const float e = (float)exp2((double)t);
        const float sc = e * (float)base_resolution - 1.0f;
        if (params < 8 || !(sc >= 0.f) || !(sc <= 16777216.f)) {
            set_error("%s: level %d has scale %g and %lld entries (a scale in [0, 2^24] and at least one entry are needed)", who, l, (double)sc, params);
            return MIRRES_E_ARG;
        }
        scale[l] = sc;
        resolution[l] = (int)ceilf(sc) + 1;
        // gridencoder.cu:68-81: the hash replaces the index when the stride loop's final stride exceeds the level's size
        uint32_t stride[3];
        const uint32_t factor = (uint32_t)resolution[l] + (align_corners ? 0u : 1u);
        unsigned long long last = 1;                                  // < 2^31 * 2^25 before the loop stops: exact
        for (int d = 0; d < D && last <= (unsigned long long)params; d++) last *= factor;
        if (wrap) last = gn_strides(D, factor, (uint32_t)params, stride);
        hashed[l] = hash && last > (unsigned long long)params ? 1 : 0;
    }
    for (int l = num_levels; l <= MIRRES_DENSITY_MAX_LEVELS; l++) offsets[l] = (int)offset;
    return offset;
}

// the range checks of the levels of a filled table, whichever struct holds it; `fill`: the entry that fills one
static bool grid_levels_ok(const char* who, const char* fill, int num_levels, const int* offsets, const int* resolution, const float* scale) {
    for (int l = 0; l < num_levels; l++) {
        if (offsets[l + 1] <= offsets[l] || resolution[l] < 1 || resolution[l] > (1 << 24) + 1 || !(scale[l] >= 0.f) || !(scale[l] <= 16777216.f)) {
            set_error("%s: bad level %d (offsets %d .. %d, resolution %d, scale %g): fill the table with %s", who, l, offsets[l], offsets[l + 1], resolution[l],
                      (double)scale[l], fill);
            return false;
        }
    }
    return true;
}

}  // namespace mr
