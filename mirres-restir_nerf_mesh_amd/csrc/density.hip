// density.hip — the stage-0 density network on the device: what NeRFRenderer.export_stage0 (nerf/renderer.py:516-539) asks of self.density() (nerf/network.py) when
// --mcubes_reso differs from the density grid's size.  One fused query per point:
//   torch-ngp GridEncoder forward (gridencoder/src/gridencoder.cu:87-196; gridtype 'hash', align_corners False, linear interpolation, D = 3, C = 2, fp32 table)
//   -> sigma_net, bias-free 32 -> 64 (ReLU) -> row 0 of the 64 -> 16 layer -> trunc_exp's forward, a plain exp (activation.py:8-10), here mrf_exp.
//   mirres_density_layout   the level table of GridEncoder.__init__ (gridencoder/grid.py:104-135) and the kernel's per-level quantities (gridencoder.cu:137-139);
//   mirres_density_points   sigma (and optionally the 32 features) of n points;
//   mirres_density_volume   sigma on the lattice xs x ys x zs (z fastest), optionally masked by the nearest cell of the density grid (renderer.py:532-541).
// The encoder's arithmetic is FIXED so that numpy float32 restates it bit for bit: u = (x + bound) / (2 bound) by IEEE division,
// p = u * scale, p = p + 0.5f, cell = floorf(p), f = p - cell; the eight corners in order idx = 0..7 (bit d of idx: +1 on axis d), w = 1 * (1 - f_d or f_d) for
// d = 0, 1, 2, r = r + w * g — every operation rounded on its own (the library is built with -ffp-contract=off).  The head is a k-ascending fmaf chain from 0 per
// neuron, like matnet.hip's mlp_point.  One thread per point; W0 and row 0 of W1 are staged in LDS and read at wave-uniform addresses (broadcast).
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

template <bool FEAT>
__global__ void __launch_bounds__(DN_BLOCK) k_density_points(mirres_density_t N, const float* __restrict__ pos, long long n, float bound, float* __restrict__ sigma,
                                                             float* __restrict__ feat_out) {
    __shared__ __attribute__((aligned(16))) float sw0[DN_HIDDEN * DN_FEAT];
    __shared__ float sw1[DN_HIDDEN];
    dn_stage_weights(N, sw0, sw1);
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float feat[DN_FEAT];
    const bool in = dn_encode(N, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], bound, feat);
    if (FEAT) {
#pragma unroll
        for (int k = 0; k < DN_FEAT; k += 4) *(float4*)(feat_out + DN_FEAT * i + k) = make_float4(feat[k], feat[k + 1], feat[k + 2], feat[k + 3]);
    }
    sigma[i] = in ? dn_head(sw0, sw1, feat) : 1.0f;               // all-zero features: h = 0, exp(0) = 1
}

// F.interpolate(mode='nearest'): source index = min(floor(dst * (float)(in / out)), in - 1), per axis — mirres_mc_mask_nearest's rule (mcubes.hip)
MR_DEV int dn_nearest(int dst, int n_out, int S) { return min((int)floorf((float)dst * ((float)S / (float)n_out)), S - 1); }

__global__ void __launch_bounds__(DN_BLOCK) k_density_volume(mirres_density_t N, const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                                                             int nx, int ny, int nz, float bound, const float* __restrict__ gvol, int S, float thresh,
                                                             float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float sw0[DN_HIDDEN * DN_FEAT];
    __shared__ float sw1[DN_HIDDEN];
    dn_stage_weights(N, sw0, sw1);
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= (long long)nx * ny * nz) return;
    const int iz = (int)(i % nz), iy = (int)((i / nz) % ny), ix = (int)(i / ((long long)ny * nz));
    if (gvol) {                                                     // sigmas * mask, then nan_to_num(., 0) (renderer.py:539-541): a cleared cell is 0 whatever sigma would be
        const float gv = gvol[((long long)dn_nearest(ix, nx, S) * S + dn_nearest(iy, ny, S)) * S + dn_nearest(iz, nz, S)];
        if (!(gv > thresh)) { out[i] = 0.f; return; }
    }
    float feat[DN_FEAT];
    const bool in = dn_encode(N, xs[ix], ys[iy], zs[iz], bound, feat);
    out[i] = in ? dn_head(sw0, sw1, feat) : 1.0f;
}

static bool dn_net_ok(const mirres_density_t* N, const char* who) {
    if (!N) { set_error("%s: net is NULL", who); return false; }
    if (N->num_levels < 1 || N->num_levels > DN_LEVELS) { set_error("%s: num_levels %d outside [1, %d]", who, N->num_levels, DN_LEVELS); return false; }
    if (!N->table || !N->w0 || !N->w1) { set_error("%s: net has a NULL table / w0 / w1", who); return false; }
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
using namespace mr;

extern "C" long long mirres_density_layout(int num_levels, int base_resolution, double desired_resolution, int log2_hashmap_size, mirres_density_t* net) {
    if (!net || num_levels < 1 || num_levels > DN_LEVELS || base_resolution < 1 || base_resolution > 65536 || !(desired_resolution >= base_resolution) ||
        !(desired_resolution <= 16777216.0) || log2_hashmap_size < 3 || log2_hashmap_size > 26) {
        set_error("mirres_density_layout: bad argument (num_levels %d in [1, %d], base_resolution %d, desired_resolution %g >= base, log2_hashmap_size %d in [3, 26])",
                  num_levels, DN_LEVELS, base_resolution, desired_resolution, log2_hashmap_size);
        return MIRRES_E_ARG;
    }
    // grid.py:108: per_level_scale in double; grid.py:128-130: the level's size from the Python-side resolution
    const double pls = num_levels > 1 ? exp2(log2(desired_resolution / (double)base_resolution) / (double)(num_levels - 1)) : 1.0;
    const float S = (float)log2(pls);                               // the `const float S` gridencoder.cu's kernel receives
    const long long max_params = 1LL << log2_hashmap_size;
    long long offset = 0;
    net->num_levels = num_levels;
    for (int l = 0; l < DN_LEVELS; l++) { net->offsets[l + 1] = 0; net->resolution[l] = 0; net->hashed[l] = 0; net->scale[l] = 0.f; }
    for (int l = 0; l < num_levels; l++) {
        const long long res = (long long)ceil((double)base_resolution * pow(pls, (double)l));
        long long params = (res + 1) * (res + 1) * (res + 1);
        if (params > max_params) params = max_params;
        params = (params + 7) / 8 * 8;
        net->offsets[l] = (int)offset;
        offset += params;
        if (offset > 0x7FFFFFFFLL) { set_error("mirres_density_layout: %lld entries do not fit the 32-bit offsets of the reference's table", offset); return MIRRES_E_ARG; }
        // gridencoder.cu:138-139 with exp2f correctly rounded: t = float(l) * S, e = float(exp2(double(t))), scale = e * float(H) - 1.0f, each step rounded to fp32
        const float t = (float)l * S;
        const float e = (float)exp2((double)t);
        const float scale = e * (float)base_resolution - 1.0f;
        net->scale[l] = scale;
        net->resolution[l] = (int)ceilf(scale) + 1;
        // gridencoder.cu:68-81: stride *= resolution + 1 while stride <= hashmap_size, at most three times; the hash replaces the index when the final stride exceeds it
        unsigned long long stride = 1;
        for (int d = 0; d < 3 && stride <= (unsigned long long)params; d++) stride *= (unsigned long long)net->resolution[l] + 1ull;
        net->hashed[l] = stride > (unsigned long long)params ? 1 : 0;
    }
    net->offsets[num_levels] = (int)offset;
    for (int l = num_levels + 1; l <= DN_LEVELS; l++) net->offsets[l] = (int)offset;
    return offset;
}

extern "C" int mirres_density_points(const mirres_density_t* net, const float* pos, long long n, float bound, float* sigma_out, float* feat_out, void* stream) {
    if (!dn_net_ok(net, "mirres_density_points")) return MIRRES_E_ARG;
    if (n < 0 || n > (1LL << 38) || (n > 0 && (!pos || !sigma_out)) || !(bound > 0.f) || !(bound < 3.0e38f)) {
        set_error("mirres_density_points: bad argument (n %lld, bound %g, pos / sigma_out %s)", n, (double)bound, (pos && sigma_out) ? "given" : "NULL"); return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    if (feat_out) k_density_points<true><<<grid_for((size_t)n, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(*net, pos, n, bound, sigma_out, feat_out);
    else k_density_points<false><<<grid_for((size_t)n, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(*net, pos, n, bound, sigma_out, nullptr);
    MR_LAUNCH_CHECK("density_points");
    return MIRRES_OK;
}

extern "C" int mirres_density_volume(const mirres_density_t* net, const float* xs, int nx, const float* ys, int ny, const float* zs, int nz, float bound,
                                     const float* grid_vol, int S, float thresh, float* out, void* stream) {
    if (!dn_net_ok(net, "mirres_density_volume")) return MIRRES_E_ARG;
    if (nx < 1 || ny < 1 || nz < 1 || nx > 65536 || ny > 65536 || nz > 65536 || (long long)nx * ny * nz > (1LL << 38) || !xs || !ys || !zs || !out || !(bound > 0.f) ||
        !(bound < 3.0e38f)) {
        set_error("mirres_density_volume: bad argument (lattice %d x %d x %d, bound %g, NULL axes or output)", nx, ny, nz, (double)bound); return MIRRES_E_ARG;
    }
    if (grid_vol && (S < 1 || S > 1290 || thresh != thresh)) { set_error("mirres_density_volume: bad mask (a cubic grid of S %d in [1, 1290], thresh %g)", S, (double)thresh); return MIRRES_E_ARG; }
    k_density_volume<<<grid_for((size_t)nx * ny * nz, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(*net, xs, ys, zs, nx, ny, nz, bound, grid_vol, S, thresh, out);
    MR_LAUNCH_CHECK("density_volume");
    return MIRRES_OK;
}
