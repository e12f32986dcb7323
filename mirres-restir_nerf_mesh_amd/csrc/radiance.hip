// radiance.hip — the stage-0 radiance network on the device: NeRFNetwork.forward(x, d) (nerf/network.py:146-174), what NeRFRenderer.render's inference loop asks per
// sample (nerf/renderer.py:802-806).  One fused query per point:
//   dn_encode (device_density.hpp, the bits of DensityField.encode) -> sigma_net 32 -> 64 (ReLU) -> 16: sigma = mrf_exp(h16[0]), geo_feat = h16[1..15]
//   -> SH direction encoder, degree 4 (shencoder/src/shencoder.cu:43-68 after the normalisation of sphere_harmonics.py:82)
//   -> color_net [sh, geo_feat] 31 -> 64 (ReLU) -> 64 (ReLU) -> 3 -> mrf_sigmoid.
//   mirres_radiance_points   sigma (optional), rgb and optionally h16 and sh of n points;
//   mirres_sh_encode         the direction encoder alone.
// The direction encoder's arithmetic is FIXED so that numpy float32 restates it bit for bit: s = (dx dx + dy dy) + dz dz, n = sqrtf(s),
// x, y, z = dx / n, dy / n, dz / n by IEEE division, the six monomials xy, xz, yz, x2, y2, z2, then the reference's sixteen expressions left to right with its literals
// rounded to fp32 — every operation rounded on its own, no FMA (the library is built with -ffp-contract=off).  Every layer's output is a k-ascending fmaf chain from
// 0.  One thread per point; the five weight matrices (37 KiB with the pads) are staged in LDS once per block and read at wave-uniform addresses (broadcast).
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"
#include "device_radiance.hpp"

namespace mr {

__global__ void __launch_bounds__(DN_BLOCK) k_radiance_points(mirres_radiance_t N, const float* __restrict__ pos, const float* __restrict__ dirs, long long n, float bound,
                                                              float* __restrict__ sigma, float* __restrict__ rgb, float* __restrict__ h16_out, float* __restrict__ sh_out) {
    __shared__ __attribute__((aligned(16))) float sw[RD_LDS_WORDS];
    rd_stage_weights(N, sw);
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float in[RD_IN];
    {
        float feat[DN_FEAT], h16[RD_H16];
        const bool inside = dn_encode(N.grid, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], bound, feat);
        rd_sigma_net(sw, feat, h16);
        if (sigma) sigma[i] = inside ? mrf_exp(h16[0]) : 1.0f;       // mirres_density_points' value: all-zero features are h = 0, exp(0) = 1
        if (h16_out) {
#pragma unroll
            for (int k = 0; k < RD_H16; k += 4) *(float4*)(h16_out + RD_H16 * i + k) = make_float4(h16[k], h16[k + 1], h16[k + 2], h16[k + 3]);
        }
#pragma unroll
        for (int k = 0; k < RD_GEO; k++) in[RD_SH + k] = h16[1 + k];
    }
    rd_sh(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], in);
    if (sh_out) {
#pragma unroll
        for (int k = 0; k < RD_SH; k += 4) *(float4*)(sh_out + RD_SH * i + k) = make_float4(in[k], in[k + 1], in[k + 2], in[k + 3]);
    }
    float c[3];
    rd_color_net(sw, in, c);
    rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2];
}

__global__ void __launch_bounds__(DN_BLOCK) k_sh_encode(const float* __restrict__ dirs, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float sh[RD_SH];
    rd_sh(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], sh);
#pragma unroll
    for (int k = 0; k < RD_SH; k += 4) *(float4*)(out + RD_SH * i + k) = make_float4(sh[k], sh[k + 1], sh[k + 2], sh[k + 3]);
}

}  // namespace mr
using namespace mr;

extern "C" int mirres_radiance_points(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, float* sigma_out, float* rgb_out,
                                      float* h16_out, float* sh_out, void* stream) {
    if (!net) { set_error("mirres_radiance_points: net is NULL"); return MIRRES_E_ARG; }
    if (!dn_net_ok(&net->grid, "mirres_radiance_points")) return MIRRES_E_ARG;
    if (!net->w1 || !net->c0 || !net->c1 || !net->c2) { set_error("mirres_radiance_points: net has a NULL w1 / c0 / c1 / c2"); return MIRRES_E_ARG; }
    if (n < 0 || n > (1LL << 38) || (n > 0 && (!pos || !dirs || !rgb_out)) || !(bound > 0.f) || !(bound < 3.0e38f)) {
        set_error("mirres_radiance_points: bad argument (n %lld, bound %g, pos / dirs / rgb_out %s)", n, (double)bound, (pos && dirs && rgb_out) ? "given" : "NULL");
        return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    k_radiance_points<<<grid_for((size_t)n, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(*net, pos, dirs, n, bound, sigma_out, rgb_out, h16_out, sh_out);
    MR_LAUNCH_CHECK("radiance_points");
    return MIRRES_OK;
}

extern "C" int mirres_sh_encode(const float* dirs, long long n, float* out, void* stream) {
    if (n < 0 || n > (1LL << 38) || (n > 0 && (!dirs || !out))) {
        set_error("mirres_sh_encode: bad argument (n %lld, dirs / out %s)", n, (dirs && out) ? "given" : "NULL"); return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    k_sh_encode<<<grid_for((size_t)n, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(dirs, n, out);
    MR_LAUNCH_CHECK("sh_encode");
    return MIRRES_OK;
}
