// Host build of csrc/device_march.hpp for tests/test_raymarch_host.py: the loops of raymarch.hip's kernels around the header's per-ray functions, one ray after the
// other, with the iteration cap the device launches do not have.  Compiled by the test with the library's compiler in host-only mode and -ffp-contract=off.
#include <stdint.h>
#include "device_march.hpp"

extern "C" {

// the marcher of k_rm_march_train / k_rm_march: out f32[N, cap, 5] (cx, cy, cz, t, dt), steps / trips i64[N], t_end f32[N]
void rmh_march(long long N, const float* o, const float* d, const uint8_t* bits, float bound, int contract, float dt_gamma, int max_steps, int C, int H,
               const float* near, const float* far, const float* t_start, const float* noises, const long long* num_steps, float eps, unsigned max_trips, long long cap,
               float* out, long long* steps, long long* trips, float* t_end) {
    const RmGrid g = rm_grid(bits, (uint32_t)C, (uint32_t)H, bound, contract, dt_gamma, (uint32_t)max_steps);
    for (long long n = 0; n < N; n++) {
        RmMarch m = rm_march_begin(g, o[3 * n], o[3 * n + 1], o[3 * n + 2], d[3 * n], d[3 * n + 1], d[3 * n + 2], near[n], far[n], t_start[n], noises[n], eps, max_trips);
        float* w = out + n * cap * 5;
        while (rm_march_live(m, (uint32_t)num_steps[n])) {
            float s[5];
            if (rm_march_iter(g, m, s)) {
                for (int k = 0; k < 5; k++) w[k] = s[k];
                w += 5;
            }
        }
        steps[n] = m.step; trips[n] = m.trips; t_end[n] = m.t;
    }
}

static bool span_ok(const int32_t* rays, long long n, long long M, long long& offset, uint32_t& count) {
    offset = (long long)(uint32_t)rays[2 * n];
    count = (uint32_t)rays[2 * n + 1];
    return count != 0 && offset + (long long)count <= M;
}

void rmh_composite_train_fwd(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, long long M, long long N, float T_thresh, int alpha_mode,
                             float* weights, float* weights_sum, float* depth, float* image) {
    for (long long n = 0; n < N; n++) {
        long long p; uint32_t num_steps;
        RmComp c = rm_comp_begin();
        if (span_ok(rays, n, M, p, num_steps)) {
            for (uint32_t step = 0; step < num_steps; step++, p++) {
                weights[p] = rm_comp_fwd(c, sigmas[p], ts[2 * p], ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], alpha_mode);
                if (c.T < T_thresh) break;
            }
        }
        weights_sum[n] = c.ws; depth[n] = c.d; image[3 * n] = c.r; image[3 * n + 1] = c.g; image[3 * n + 2] = c.b;
    }
}

void rmh_composite_train_bwd(const float* gw, const float* gws, const float* gd, const float* gi, const float* sigmas, const float* rgbs, const float* ts,
                             const int32_t* rays, const float* weights_sum, const float* depth, const float* image, long long M, long long N, float T_thresh,
                             int alpha_mode, float* grad_sigmas, float* grad_rgbs) {
    for (long long n = 0; n < N; n++) {
        long long p; uint32_t num_steps;
        if (!span_ok(rays, n, M, p, num_steps)) continue;
        RmCompFinal f;
        f.r = image[3 * n]; f.g = image[3 * n + 1]; f.b = image[3 * n + 2]; f.ws = weights_sum[n]; f.d = depth[n];
        f.gr = gi[3 * n]; f.gg = gi[3 * n + 1]; f.gb = gi[3 * n + 2]; f.gws = gws[n]; f.gd = gd[n];
        RmComp c = rm_comp_begin();
        for (uint32_t step = 0; step < num_steps; step++, p++) {
            grad_sigmas[p] = rm_comp_bwd(c, f, sigmas[p], ts[2 * p], ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], gw[p], alpha_mode, grad_rgbs + 3 * p);
            if (c.T < T_thresh) break;
        }
    }
}

void rmh_composite(long long n_alive, int n_step, long long N, float T_thresh, int alpha_mode, int32_t* rays_alive, float* rays_t, const float* sigmas, const float* rgbs,
                   const float* ts, float* weights_sum, float* depth, float* image) {
    for (long long n = 0; n < n_alive; n++) {
        const long long index = rays_alive[n];
        if (index < 0 || index >= N) { rays_alive[n] = -1; continue; }
        RmInfer c;
        c.d = depth[index]; c.r = image[3 * index]; c.g = image[3 * index + 1]; c.b = image[3 * index + 2]; c.ws = weights_sum[index];
        float t = 0.f;
        long long p = n * (long long)n_step;
        int step = 0;
        for (; step < n_step; step++, p++) {
            if (ts[2 * p] == 0) break;
            t = ts[2 * p];
            const float T = rm_comp_infer(c, sigmas[p], t, ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], alpha_mode);
            if (T < T_thresh) break;
        }
        if (step < n_step) rays_alive[n] = -1;
        else rays_t[index] = t;
        weights_sum[index] = c.ws; depth[index] = c.d; image[3 * index] = c.r; image[3 * index + 1] = c.g; image[3 * index + 2] = c.b;
    }
}

}  // extern "C"
