// ORACLE — test infrastructure only (never linked or loaded by the product).
// oracle/_ref/libref_raymarch.so = the REFERENCE'S OWN ray-marching operators, raymarching/src/raymarching.cu, compiled by hipcc for gfx950 from where the file lies in
// the reference tree (oracle/Makefile, target `ref`) — nothing of it is copied into this repository.  The headers it includes resolve to oracle/ref_shim/: the HIP
// runtime for cuda*.h, an empty ATen context header, and a torch/torch.h that stands in for the at:: names its host wrappers mention (a Tensor there is a device
// pointer; the floating dispatch runs with scalar_t = float).  This file adds the entries: each takes device pointers, calls the reference's own host wrapper
// (which launches on the null stream and checks nothing), synchronises and returns the HIP error code, so a caller can stop at the first fault.
// sph_from_ray (:163-209) is not built on the product side and has no entry.
// tests/test_gpu_ref_raymarch.py holds csrc/raymarch.hip and tests/raymarch_refs.py to what these kernels compute.
#include REF_RAYMARCH_CU

namespace {
at::Tensor T(const void* p) { return at::Tensor(p); }
at::optional<at::Tensor> opt(const void* p) { return p ? at::optional<at::Tensor>(at::Tensor(p)) : at::optional<at::Tensor>(); }
int finish() {
    const hipError_t launch = hipGetLastError();
    const hipError_t sync = hipDeviceSynchronize();
    return (int)(sync != hipSuccess ? sync : launch);
}
// the compositors' exponential (:543, :653, :879) on its own: the same intrinsic under the same compiler and flags
__global__ void k_ref_fast_exp(const float* __restrict__ x, float* __restrict__ y, const uint32_t n) {
    const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < n) y[i] = __expf(x[i]);
}
}  // namespace

#define REF_NONEMPTY(n) if ((n) == 0) return (int)hipErrorInvalidValue      /* the reference would launch an empty grid */

extern "C" int ref_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near, float* nears, float* fars) {
    REF_NONEMPTY(N);
    near_far_from_aabb(T(rays_o), T(rays_d), T(aabb), N, min_near, T(nears), T(fars));
    return finish();
}
extern "C" int ref_morton3D(const int* coords, uint32_t N, int* indices) {
    REF_NONEMPTY(N);
    morton3D(T(coords), N, T(indices));
    return finish();
}
extern "C" int ref_morton3D_invert(const int* indices, uint32_t N, int* coords) {
    REF_NONEMPTY(N);
    morton3D_invert(T(indices), N, T(coords));
    return finish();
}
// grid f32 [N * 8] -> bitfield u8 [N]
extern "C" int ref_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield) {
    REF_NONEMPTY(N);
    packbits(T(grid), N, density_thresh, T(bitfield));
    return finish();
}
// rays i32 [N, 2] -> res i32 [M]; the caller guarantees that every span lies in [0, M) (the kernel does not look at M)
extern "C" int ref_flatten_rays(const int* rays, uint32_t N, uint32_t M, int* res) {
    REF_NONEMPTY(N);
    flatten_rays(T(rays), N, M, T(res));
    return finish();
}
// xyzs == NULL: the counting pass (rays and counter[0] written); else the writing pass, which reads rays.  counter: two ints, zeroed by the caller before pass one.
extern "C" int ref_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, int contract, float dt_gamma, uint32_t max_steps,
                                    uint32_t N, uint32_t C, uint32_t H, const float* nears, const float* fars, float* xyzs, float* dirs, float* ts, int* rays,
                                    int* counter, const float* noises) {
    REF_NONEMPTY(N);
    if ((xyzs == nullptr) != (dirs == nullptr) || (xyzs == nullptr) != (ts == nullptr)) return (int)hipErrorInvalidValue;
    march_rays_train(T(rays_o), T(rays_d), T(grid), bound, contract != 0, dt_gamma, max_steps, N, C, H, T(nears), T(fars), opt(xyzs), opt(dirs), opt(ts), T(rays),
                     T(counter), T(noises));
    return finish();
}
extern "C" int ref_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* ts, const int* rays, uint32_t M, uint32_t N, float T_thresh,
                                                int alpha_mode, float* weights, float* weights_sum, float* depth, float* image) {
    REF_NONEMPTY(N);
    composite_rays_train_forward(T(sigmas), T(rgbs), T(ts), T(rays), M, N, T_thresh, alpha_mode != 0, T(weights), T(weights_sum), T(depth), T(image));
    return finish();
}
extern "C" int ref_composite_rays_train_backward(const float* grad_weights, const float* grad_weights_sum, const float* grad_depth, const float* grad_image,
                                                 const float* sigmas, const float* rgbs, const float* ts, const int* rays, const float* weights_sum,
                                                 const float* depth, const float* image, uint32_t M, uint32_t N, float T_thresh, int alpha_mode, float* grad_sigmas,
                                                 float* grad_rgbs) {
    REF_NONEMPTY(N);
    composite_rays_train_backward(T(grad_weights), T(grad_weights_sum), T(grad_depth), T(grad_image), T(sigmas), T(rgbs), T(ts), T(rays), T(weights_sum), T(depth),
                                  T(image), M, N, T_thresh, alpha_mode != 0, T(grad_sigmas), T(grad_rgbs));
    return finish();
}
// xyzs, dirs f32 [n_alive * n_step, 3], ts [n_alive * n_step, 2]: zeroed by the caller, as the reference's Python does
extern "C" int ref_march_rays(uint32_t n_alive, uint32_t n_step, const int* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d, float bound,
                              int contract, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                              float* xyzs, float* dirs, float* ts, const float* noises) {
    REF_NONEMPTY(n_alive);
    march_rays(n_alive, n_step, T(rays_alive), T(rays_t), T(rays_o), T(rays_d), bound, contract != 0, dt_gamma, max_steps, C, H, T(grid), T(nears), T(fars), T(xyzs),
               T(dirs), T(ts), T(noises));
    return finish();
}
extern "C" int ref_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int alpha_mode, int* rays_alive, float* rays_t, const float* sigmas,
                                  const float* rgbs, const float* ts, float* weights_sum, float* depth, float* image) {
    REF_NONEMPTY(n_alive);
    composite_rays(n_alive, n_step, T_thresh, alpha_mode != 0, T(rays_alive), T(rays_t), T(sigmas), T(rgbs), T(ts), T(weights_sum), T(depth), T(image));
    return finish();
}
extern "C" int ref_fast_exp(const float* x, float* y, uint32_t n) {
    REF_NONEMPTY(n);
    k_ref_fast_exp<<<(n + 127) / 128, 128>>>(x, y, n);
    return finish();
}
