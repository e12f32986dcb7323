// ORACLE — test infrastructure only (never linked or loaded by the product).
// oracle/_ref/libref_normal.so = the REFERENCE'S OWN shading-normal kernels, nerf/renderutils/c_src/normal.cu (PrepareShadingNormalFwdKernel :95-123,
// PrepareShadingNormalBwdKernel :125-179) with the headers they include (common.h, vec3f.h, vec4f.h, tensor.h, normal.h), compiled by hipcc for gfx950 from where
// the sources lie — nothing of them is copied into this repository (oracle/Makefile: target _ref/libref_normal.so). The recipe's flags: -D__CUDACC__ selects the
// device halves of the reference's own #if blocks, -include hip/hip_runtime.h stands where nvcc pre-includes cuda_runtime.h, -Iref_shim resolves <cuda.h> to the
// HIP runtime, and -ffp-contract=off fixes the arithmetic without contraction, as the product's build does (a compiler flag, as nvcc's -fmad=false is).
// What this file adds is the launch. The host half of the reference's launcher (c_src/torch_bindings.cpp:93-194) needs ATen, so the kernel arguments are filled
// below the way that code fills them: fp32 tensors [n, h, w, 3] contiguous, each with its own sizes (a size of 1 broadcasts on fetch), gridSize = the
// element-wise maximum of the inputs' sizes, gradients written full-size and contiguous. The block shape is this file's own (fixed 8 x 8), not that launcher's.
// The kernels run on the GPU: tests/test_gpu_bilateral.py holds csrc/normal.hip to them.
#include REF_NORMAL_CU
#include <cstring>

namespace {
// shape[k] = (n, h, w) of input k, in the order pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm
void fill(Tensor& t, const float* val, float* grad, const int* shape, dim3 g) {
    std::memset(&t, 0, sizeof(t));
    t.val = const_cast<float*>(val); t.d_val = grad; t.fp16 = false;
    t.dims[0] = shape[0]; t.dims[1] = shape[1]; t.dims[2] = shape[2]; t.dims[3] = 3;
    t.strides[0] = shape[1] * shape[2] * 3; t.strides[1] = shape[2] * 3; t.strides[2] = 3; t.strides[3] = 1;
    t._dims[0] = (int)g.z; t._dims[1] = (int)g.y; t._dims[2] = (int)g.x; t._dims[3] = 3;
}
dim3 extent(const int* shapes) {
    dim3 g(0, 0, 0);
    for (int k = 0; k < 6; k++) {
        const unsigned n = shapes[3 * k], h = shapes[3 * k + 1], w = shapes[3 * k + 2];
        g.x = w > g.x ? w : g.x; g.y = h > g.y ? h : g.y; g.z = n > g.z ? n : g.z;
    }
    return g;
}
// 8 x 8 x 1 thread blocks, one thread per pixel, as ref_denoise_driver.hip launches: both kernels work on one element per thread and return early out of
// range (normal.cu:98-102, 128-132), so the block shape cannot change a bit of the output.
dim3 launch_grid(dim3 g) { return dim3((g.x + 7) / 8, (g.y + 7) / 8, g.z); }
}  // namespace

// six inputs f32[shape k, 3] -> out f32[N, H, W, 3], (N, H, W) = the maximum over the inputs   (torch_bindings.cpp:123-163)
extern "C" int ref_shading_normal_fwd(const float* const in[6], const int* shapes, int two_sided_shading, int opengl, float* out, void* stream) {
    const dim3 g = extent(shapes);
    if (g.x == 0 || g.y == 0 || g.z == 0) return -1;
    PrepareShadingNormalKernelParams p;
    std::memset(&p, 0, sizeof(p));
    Tensor* t[6] = {&p.pos, &p.view_pos, &p.perturbed_nrm, &p.smooth_nrm, &p.smooth_tng, &p.geom_nrm};
    for (int k = 0; k < 6; k++) fill(*t[k], in[k], nullptr, shapes + 3 * k, g);
    const int full[3] = {(int)g.z, (int)g.y, (int)g.x};
    fill(p.out, out, nullptr, full, g);
    p.gridSize = g; p.two_sided_shading = two_sided_shading != 0; p.opengl = opengl != 0;
    PrepareShadingNormalFwdKernel<<<launch_grid(g), dim3(8, 8, 1), 0, (hipStream_t)stream>>>(p);
    return (int)hipGetLastError();
}
// + dout f32[N, H, W, 3] -> six gradients f32[N, H, W, 3] each (full size: the caller sums the broadcast ones, ops.py)   (torch_bindings.cpp:165-194)
extern "C" int ref_shading_normal_bwd(const float* const in[6], const int* shapes, int two_sided_shading, int opengl, const float* dout, float* const grads[6], void* stream) {
    const dim3 g = extent(shapes);
    if (g.x == 0 || g.y == 0 || g.z == 0) return -1;
    PrepareShadingNormalKernelParams p;
    std::memset(&p, 0, sizeof(p));
    Tensor* t[6] = {&p.pos, &p.view_pos, &p.perturbed_nrm, &p.smooth_nrm, &p.smooth_tng, &p.geom_nrm};
    for (int k = 0; k < 6; k++) fill(*t[k], in[k], grads[k], shapes + 3 * k, g);
    const int full[3] = {(int)g.z, (int)g.y, (int)g.x};
    fill(p.out, dout, nullptr, full, g);
    p.gridSize = g; p.two_sided_shading = two_sided_shading != 0; p.opengl = opengl != 0;
    PrepareShadingNormalBwdKernel<<<launch_grid(g), dim3(8, 8, 1), 0, (hipStream_t)stream>>>(p);
    return (int)hipGetLastError();
}
