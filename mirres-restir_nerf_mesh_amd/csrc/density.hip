// density.hip — the stage-0 density network on the device: what NeRFRenderer.export_stage0 (nerf/renderer.py:516-539) asks of self.density() (nerf/network.py) when
// --mcubes_reso differs from the density grid's size.  One fused query per point:
//   torch-ngp GridEncoder forward (gridencoder/src/gridencoder.cu:87-196; gridtype 'hash', align_corners False, linear interpolation, D = 3, C = 2, fp32 table)
//   -> sigma_net, bias-free 32 -> 64 (ReLU) -> row 0 of the 64 -> 16 layer -> trunc_exp's forward, a plain exp (activation.py:8-10), here mrf_exp.
//   mirres_density_layout   the level table of GridEncoder.__init__ (gridencoder/grid.py:104-135) and the kernel's per-level quantities (gridencoder.cu:137-139):
//                           grid_layout.hpp's routine, which mirres_gridenc_layout calls too;
//   mirres_density_points   sigma (and optionally the 32 features) of n points;
//   mirres_density_volume   sigma on the lattice xs x ys x zs (z fastest), optionally masked by the nearest cell of the density grid (renderer.py:532-541).
// The encoder's arithmetic is FIXED so that numpy float32 restates it bit for bit: u = (x + bound) / (2 bound) by IEEE division,
// p = u * scale, p = p + 0.5f, cell = floorf(p), f = p - cell; the eight corners in order idx = 0..7 (bit d of idx: +1 on axis d), w = 1 * (1 - f_d or f_d) for
// d = 0, 1, 2, r = r + w * g — every operation rounded on its own (the library is built with -ffp-contract=off).  The head is a k-ascending fmaf chain from 0 per
// neuron, like matnet.hip's mlp_point.  One thread per point; W0 and row 0 of W1 are staged in LDS and read at wave-uniform addresses (broadcast).
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"

namespace mr {

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

}  // namespace mr
using namespace mr;

extern "C" long long mirres_density_layout(int num_levels, int base_resolution, double desired_resolution, int log2_hashmap_size, mirres_density_t* net) {
    if (!net || num_levels < 1 || num_levels > DN_LEVELS || base_resolution < 1 || base_resolution > 65536 || !(desired_resolution >= base_resolution) ||
        !(desired_resolution <= 16777216.0) || log2_hashmap_size < 3 || log2_hashmap_size > 26) {
        set_error("mirres_density_layout: bad argument (num_levels %d in [1, %d], base_resolution %d, desired_resolution %g >= base, log2_hashmap_size %d in [3, 26])",
                  num_levels, DN_LEVELS, base_resolution, desired_resolution, log2_hashmap_size);
        return MIRRES_E_ARG;
    }
    // grid.py:108: per_level_scale in double
    const double pls = num_levels > 1 ? exp2(log2(desired_resolution / (double)base_resolution) / (double)(num_levels - 1)) : 1.0;
    net->num_levels = num_levels;
    return grid_layout("mirres_density_layout", 3, false, true, false, num_levels, pls, base_resolution, log2_hashmap_size, net->offsets, net->resolution, net->hashed,
                       net->scale);
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
