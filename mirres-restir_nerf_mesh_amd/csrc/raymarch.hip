// raymarch.hip — the stage-0 ray-marching operators (torch-ngp raymarching/src/raymarching.cu) and the upkeep of the occupancy grid they read
// (nerf/renderer.py:1438-1595), fp32 only (the reference's wrappers cast to float):
//   mirres_rm_near_far, _morton3d, _morton3d_invert, _packbits, _flatten_rays         the helpers (:92-145, :214-260, :268-289, :303-319)
//   mirres_rm_march_train_count / _scan / _write                                        march_rays_train (:338-475) in three launches: steps per ray, the exclusive
//                                                                                       prefix sum of the counts in ray order, the samples — no atomic counter, so
//                                                                                       rays[:, 0] is the same in every run
//   mirres_rm_composite_train_fwd / _bwd                                                composite_rays_train (:501-578, :605-694)
//   mirres_rm_march, mirres_rm_composite                                                the inference pair (:713-828, :842-924)
//   mirres_rm_grid_mark_untrained, mirres_rm_grid_update                                mark_untrained_grid and update_extra_state's grid pass, one launch each
// The per-ray arithmetic lives in device_march.hpp (fixed, restated by tests/raymarch_refs.py), the density query in device_density.hpp.
// One lane per ray (or cell), 64-bit element indices, no scratch.  Compositing reads a ray's samples at a per-lane stride: see DESIGN.md section 5.13 for its bound.
#include <math.h>
#include <float.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_scan.hpp"
#include "device_density.hpp"
#include "device_march.hpp"

namespace mr {

#define RM_BLOCK 128
#define RM_EW_BLOCK 256
#define RM_SCAN_BLOCK 1024
typedef long long i64;

MR_DEV i64 rm_tid(int block) { return (i64)blockIdx.x * block + threadIdx.x; }

__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_near_far(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ aabb, i64 N,
                                                             float min_near, float* __restrict__ nears, float* __restrict__ fars) {
    const i64 n = rm_tid(RM_EW_BLOCK);
    if (n >= N) return;
    const float ox = rays_o[3 * n], oy = rays_o[3 * n + 1], oz = rays_o[3 * n + 2];
    const float rdx = 1 / rays_d[3 * n], rdy = 1 / rays_d[3 * n + 1], rdz = 1 / rays_d[3 * n + 2];
    float near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx;
    if (near > far) { const float c = near; near = far; far = c; }
    float near_y = (aabb[1] - oy) * rdy, far_y = (aabb[4] - oy) * rdy;
    if (near_y > far_y) { const float c = near_y; near_y = far_y; far_y = c; }
    if (near > far_y || near_y > far) { nears[n] = fars[n] = FLT_MAX; return; }
    if (near_y > near) near = near_y;
    if (far_y < far) far = far_y;
    float near_z = (aabb[2] - oz) * rdz, far_z = (aabb[5] - oz) * rdz;
    if (near_z > far_z) { const float c = near_z; near_z = far_z; far_z = c; }
    if (near > far_z || near_z > far) { nears[n] = fars[n] = FLT_MAX; return; }
    if (near_z > near) near = near_z;
    if (far_z < far) far = far_z;
    if (near < min_near) near = min_near;
    nears[n] = near;
    fars[n] = far;
}

__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_morton3D(const int32_t* __restrict__ coords, i64 N, int32_t* __restrict__ indices) {
    const i64 n = rm_tid(RM_EW_BLOCK);
    if (n >= N) return;
    indices[n] = (int32_t)rm_morton3D((uint32_t)coords[3 * n], (uint32_t)coords[3 * n + 1], (uint32_t)coords[3 * n + 2]);
}

__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_morton3D_invert(const int32_t* __restrict__ indices, i64 N, int32_t* __restrict__ coords) {
    const i64 n = rm_tid(RM_EW_BLOCK);
    if (n >= N) return;
    const int32_t ind = indices[n];                                  // `ind >> k` on the signed value, as the reference has it
    coords[3 * n] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 0));
    coords[3 * n + 1] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 1));
    coords[3 * n + 2] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 2));
}

__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_packbits(const float* __restrict__ grid, i64 N, float thresh, uint8_t* __restrict__ bitfield) {
    const i64 n = rm_tid(RM_EW_BLOCK);
    if (n >= N) return;
    const float4 a = *(const float4*)(grid + 8 * n), b = *(const float4*)(grid + 8 * n + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) bits |= (v[i] > thresh) ? (1u << i) : 0u;
    bitfield[n] = (uint8_t)bits;
}

// a ray's samples [offset, offset + count) inside [0, M)?  offset and count are read as the reference reads them (uint32 of the int32)
MR_DEV bool rm_span_ok(const int32_t* rays, i64 n, i64 M, i64& offset, uint32_t& count) {
    offset = (i64)(uint32_t)rays[2 * n];
    count = (uint32_t)rays[2 * n + 1];
    return count != 0 && offset + (i64)count <= M;
}

__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_flatten_rays(const int32_t* __restrict__ rays, i64 N, i64 M, int32_t* __restrict__ res) {
    const i64 n = rm_tid(RM_EW_BLOCK);
    if (n >= N) return;
    i64 offset; uint32_t count;
    if (!rm_span_ok(rays, n, M, offset, count)) return;            // the reference writes past M here
    for (uint32_t i = 0; i < count; i++) res[offset + i] = (int32_t)n;
}

// WRITE false: the first pass (steps of every ray -> rays[n, 1]); true: the second (rays[n] = {offset, steps} -> the samples)
template <bool WRITE>
__global__ void __launch_bounds__(RM_BLOCK) k_rm_march_train(const float* __restrict__ rays_o, const float* __restrict__ rays_d, RmGrid g, uint32_t max_steps, i64 N,
                                                             const float* __restrict__ nears, const float* __restrict__ fars, const float* __restrict__ noises,
                                                             int32_t* __restrict__ rays, i64 M, float* __restrict__ xyzs, float* __restrict__ dirs,
                                                             float* __restrict__ ts) {
    const i64 n = rm_tid(RM_BLOCK);
    if (n >= N) return;
    uint32_t num_steps = max_steps;
    i64 p = 0;
    if (WRITE) {
        if (!rm_span_ok(rays, n, M, p, num_steps)) return;
    }
    const float near = nears[n], far = fars[n];
    RmMarch m = rm_march_begin(g, rays_o[3 * n], rays_o[3 * n + 1], rays_o[3 * n + 2], rays_d[3 * n], rays_d[3 * n + 1], rays_d[3 * n + 2], near, far, near, noises[n],
                               0.0f, RM_NO_CAP);
    while (rm_march_live(m, num_steps)) {
        float s[5];
        if (rm_march_iter(g, m, s) && WRITE) {
            xyzs[3 * p] = s[0]; xyzs[3 * p + 1] = s[1]; xyzs[3 * p + 2] = s[2];
            dirs[3 * p] = m.dx; dirs[3 * p + 1] = m.dy; dirs[3 * p + 2] = m.dz;
            ts[2 * p] = s[3]; ts[2 * p + 1] = s[4];
            p++;
        }
    }
    if (!WRITE) { rays[2 * n] = 0; rays[2 * n + 1] = (int32_t)m.step; }
}

// rays[n, 0] = sum of rays[k, 1] over k < n, total[0] = the sum over all rays: one workgroup, every thread a contiguous run of rays, the runs' sums
// through block_excl_scan (device_scan.hpp) in 64 bits
__global__ void __launch_bounds__(RM_SCAN_BLOCK) k_rm_scan(int32_t* __restrict__ rays, i64 N, i64* __restrict__ total) {
    __shared__ unsigned long long part[RM_SCAN_BLOCK / 64];
    const i64 run = (N + RM_SCAN_BLOCK - 1) / RM_SCAN_BLOCK;
    const i64 a = min((i64)threadIdx.x * run, N), b = min(a + run, N);
    i64 s = 0;
    for (i64 k = a; k < b; k++) s += (i64)(uint32_t)rays[2 * k + 1];
    unsigned long long all;                                          // exclusive scan of the runs' sums (none negative: counts are read as uint32)
    i64 base = (i64)block_excl_scan<RM_SCAN_BLOCK>((unsigned long long)s, part, all);
    for (i64 k = a; k < b; k++) {
        rays[2 * k] = (int32_t)(base > 0x7fffffffLL ? 0x7fffffffLL : base);      // beyond 2^31 - 1 samples the caller refuses (total says so); never a wrapped offset
        base += (i64)(uint32_t)rays[2 * k + 1];
    }
    if (threadIdx.x == 0) total[0] = (i64)all;
}

__global__ void __launch_bounds__(RM_BLOCK) k_rm_composite_train_fwd(const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ ts,
                                                                     const int32_t* __restrict__ rays, i64 M, i64 N, float T_thresh, int alpha_mode,
                                                                     float* __restrict__ weights, float* __restrict__ weights_sum, float* __restrict__ depth,
                                                                     float* __restrict__ image) {
    const i64 n = rm_tid(RM_BLOCK);
    if (n >= N) return;
    i64 p; uint32_t num_steps;
    RmComp c = rm_comp_begin();
    if (rm_span_ok(rays, n, M, p, num_steps)) {
        for (uint32_t step = 0; step < num_steps; step++, p++) {
            weights[p] = rm_comp_fwd(c, sigmas[p], ts[2 * p], ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], alpha_mode);
            if (c.T < T_thresh) break;
        }
    }
    weights_sum[n] = c.ws;
    depth[n] = c.d;
    image[3 * n] = c.r; image[3 * n + 1] = c.g; image[3 * n + 2] = c.b;
}

__global__ void __launch_bounds__(RM_BLOCK) k_rm_composite_train_bwd(const float* __restrict__ grad_weights, const float* __restrict__ grad_weights_sum,
                                                                     const float* __restrict__ grad_depth, const float* __restrict__ grad_image,
                                                                     const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ ts,
                                                                     const int32_t* __restrict__ rays, const float* __restrict__ weights_sum,
                                                                     const float* __restrict__ depth, const float* __restrict__ image, i64 M, i64 N, float T_thresh,
                                                                     int alpha_mode, float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs) {
    const i64 n = rm_tid(RM_BLOCK);
    if (n >= N) return;
    i64 p; uint32_t num_steps;
    if (!rm_span_ok(rays, n, M, p, num_steps)) return;
    RmCompFinal f;
    f.r = image[3 * n]; f.g = image[3 * n + 1]; f.b = image[3 * n + 2]; f.ws = weights_sum[n]; f.d = depth[n];
    f.gr = grad_image[3 * n]; f.gg = grad_image[3 * n + 1]; f.gb = grad_image[3 * n + 2]; f.gws = grad_weights_sum[n]; f.gd = grad_depth[n];
    RmComp c = rm_comp_begin();
    for (uint32_t step = 0; step < num_steps; step++, p++) {
        float gc[3];
        grad_sigmas[p] = rm_comp_bwd(c, f, sigmas[p], ts[2 * p], ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], grad_weights[p], alpha_mode, gc);
        grad_rgbs[3 * p] = gc[0]; grad_rgbs[3 * p + 1] = gc[1]; grad_rgbs[3 * p + 2] = gc[2];
        if (c.T < T_thresh) break;
    }
}

__global__ void __launch_bounds__(RM_BLOCK) k_rm_march(i64 n_alive, uint32_t n_step, const int32_t* __restrict__ rays_alive, const float* __restrict__ rays_t,
                                                       const float* __restrict__ rays_o, const float* __restrict__ rays_d, i64 N, RmGrid g,
                                                       const float* __restrict__ nears, const float* __restrict__ fars, float* __restrict__ xyzs,
                                                       float* __restrict__ dirs, float* __restrict__ ts, const float* __restrict__ noises) {
    const i64 n = rm_tid(RM_BLOCK);
    if (n >= n_alive) return;
    const i64 index = rays_alive[n];
    if (index < 0 || index >= N) return;                            // not a ray: its samples stay zero, which composite_rays reads as terminated
    RmMarch m = rm_march_begin(g, rays_o[3 * index], rays_o[3 * index + 1], rays_o[3 * index + 2], rays_d[3 * index], rays_d[3 * index + 1], rays_d[3 * index + 2],
                               nears[index], fars[index], rays_t[index], noises[n], 1e-10f, RM_NO_CAP);
    i64 p = n * (i64)n_step;
    while (rm_march_live(m, n_step)) {
        float s[5];
        if (rm_march_iter(g, m, s)) {
            xyzs[3 * p] = s[0]; xyzs[3 * p + 1] = s[1]; xyzs[3 * p + 2] = s[2];
            dirs[3 * p] = m.dx; dirs[3 * p + 1] = m.dy; dirs[3 * p + 2] = m.dz;
            ts[2 * p] = s[3]; ts[2 * p + 1] = s[4];
            p++;
        }
    }
}

__global__ void __launch_bounds__(RM_BLOCK) k_rm_composite(i64 n_alive, uint32_t n_step, i64 N, float T_thresh, int alpha_mode, int32_t* __restrict__ rays_alive,
                                                           float* __restrict__ rays_t, const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                           const float* __restrict__ ts, float* __restrict__ weights_sum, float* __restrict__ depth,
                                                           float* __restrict__ image) {
    const i64 n = rm_tid(RM_BLOCK);
    if (n >= n_alive) return;
    const i64 index = rays_alive[n];
    if (index < 0 || index >= N) { rays_alive[n] = -1; return; }
    RmInfer c;
    c.d = depth[index]; c.r = image[3 * index]; c.g = image[3 * index + 1]; c.b = image[3 * index + 2]; c.ws = weights_sum[index];
    float t = 0.f;
    i64 p = n * (i64)n_step;
    uint32_t step = 0;
    for (; step < n_step; step++, p++) {
        if (ts[2 * p] == 0) break;                                  // the marcher wrote no sample here (:877)
        t = ts[2 * p];
        const float T = rm_comp_infer(c, sigmas[p], t, ts[2 * p + 1], rgbs[3 * p], rgbs[3 * p + 1], rgbs[3 * p + 2], alpha_mode);
        if (T < T_thresh) break;
    }
    if (step < n_step) rays_alive[n] = -1;
    else rays_t[index] = t;
    weights_sum[index] = c.ws;
    depth[index] = c.d;
    image[3 * index] = c.r; image[3 * index + 1] = c.g; image[3 * index + 2] = c.b;
}

// ---- the occupancy grid.  Per cascade, computed by the host as the reference's Python does (doubles rounded to fp32 where they meet a tensor)
struct RmCascades { float scale[MIRRES_RM_MAX_CASCADES], hgs[MIRRES_RM_MAX_CASCADES], hgs2[MIRRES_RM_MAX_CASCADES]; };

// the lattice point of cell (Morton index i) on one axis: 2 * coord / (H - 1) - 1 (renderer.py:1474, :1554)
MR_DEV float rm_lattice(uint32_t coord, float hm1) { return (2.0f * (float)coord) / hm1 - 1.0f; }

// mark_untrained_grid (renderer.py:1438-1524): one lane per (cascade, cell), the cameras in a loop; cells no camera sees or outside aabb_train +- half a cell -> -1
__global__ void __launch_bounds__(RM_EW_BLOCK) k_rm_grid_mark(float* __restrict__ grid, int C, uint32_t H, RmCascades cs, const float* __restrict__ poses,
                                                              const float* __restrict__ intrinsics, int per_cam_intrinsics, const float* __restrict__ cam_near, int B,
                                                              float min_near, const float* __restrict__ aabb) {
    const i64 H3 = (i64)H * H * H;
    const i64 i = rm_tid(RM_EW_BLOCK);
    if (i >= H3 * C) return;
    const int cas = (int)(i / H3);
    const uint32_t mi = (uint32_t)(i % H3);
    const float hm1 = (float)(H - 1), scale = cs.scale[cas], hgs = cs.hgs[cas], hgs2 = cs.hgs2[cas];
    const float x = rm_lattice(rm_morton3D_invert(mi), hm1) * scale, y = rm_lattice(rm_morton3D_invert(mi >> 1), hm1) * scale,
                z = rm_lattice(rm_morton3D_invert(mi >> 2), hm1) * scale;
    const bool in_box = x >= aabb[0] - hgs && y >= aabb[1] - hgs && z >= aabb[2] - hgs && x <= aabb[3] + hgs && y <= aabb[4] + hgs && z <= aabb[5] + hgs;
    bool seen = false;
    for (int b = 0; b < B && in_box && !seen; b++) {
        const float* P = poses + 16 * (i64)b;
        const float px = x - P[3], py = y - P[7], pz = z - P[11];
        const float cx = (px * P[0] + py * P[4]) + pz * P[8];
        const float cy = (px * P[1] + py * P[5]) + pz * P[9];
        const float cz = -((px * P[2] + py * P[6]) + pz * P[10]);
        const float* K = intrinsics + (per_cam_intrinsics ? 4 * (i64)b : 0);
        const float cx_div_fx = K[2] / K[0], cy_div_fy = K[3] / K[1];
        const float nr = cam_near ? cam_near[2 * (i64)b] : min_near;
        seen = cz > nr && fabsf(cx) < cx_div_fx * cz + hgs2 && fabsf(cy) < cy_div_fy * cz + hgs2;
    }
    if (!(in_box && seen)) grid[i] = -1.0f;
}

// update_extra_state's grid pass (renderer.py:1540-1577, the non-trainable grid): every cell of every cascade in one launch — the jittered lattice point, the density
// network at it (device_density.hpp, the code DensityField.density runs) and max(grid * decay, sigma) where both are >= 0.  A cell at -1 is left without a query.
__global__ void __launch_bounds__(DN_BLOCK) k_rm_grid_update(mirres_density_t net, float field_bound, float* __restrict__ grid, int C, uint32_t H, RmCascades cs,
                                                             const float* __restrict__ noise, float decay) {
    __shared__ __attribute__((aligned(16))) float sw0[DN_HIDDEN * DN_FEAT];
    __shared__ float sw1[DN_HIDDEN];
    dn_stage_weights(net, sw0, sw1);
    const i64 H3 = (i64)H * H * H;
    const i64 i = rm_tid(DN_BLOCK);
    if (i >= H3 * C) return;
    const float gv = grid[i];
    if (!(gv >= 0.f)) return;
    const int cas = (int)(i / H3);
    const uint32_t mi = (uint32_t)(i % H3);
    const float hm1 = (float)(H - 1), scale = cs.scale[cas], hgs = cs.hgs[cas];
    float p[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float v = rm_lattice(rm_morton3D_invert(mi >> d), hm1) * scale;
        const float j = (noise[3 * i + d] * 2.0f - 1.0f) * hgs;
        p[d] = v + j;
    }
    float feat[DN_FEAT];
    const bool in = dn_encode(net, p[0], p[1], p[2], field_bound, feat);
    const float sigma = in ? dn_head(sw0, sw1, feat) : 1.0f;
    if (sigma >= 0.f) grid[i] = fmaxf(gv * decay, sigma);
}

// `what` names the buffer that goes with the grid's shape: the bitfield for the marchers, the density grid for its upkeep
static bool rm_grid_ok(const char* who, int C, int H, float bound, const void* buf, const char* what) {
    if (C < 1 || C > MIRRES_RM_MAX_CASCADES || H < 2 || H > 1024 || (H & (H - 1)) || !(bound > 0.f) || !(bound < 3.0e38f) || !buf) {
        set_error("%s: bad grid (cascades %d in [1, %d], H %d a power of two in [2, 1024], bound %g, %s %s)", who, C, MIRRES_RM_MAX_CASCADES, H, (double)bound, what,
                  buf ? "given" : "NULL");
        return false;
    }
    return true;
}
// one launch covers a count: one lane per element in blocks of 128 or 256, and at most 2^31 lanes (below HIP's 2^32 threads per launch, and beyond every int32 ray
// or point index of the interface)
#define RM_MAX_COUNT (1LL << 31)
static bool rm_count_ok(const char* who, const char* what, long long n) {
    if (n < 0 || n > RM_MAX_COUNT) { set_error("%s: %s %lld outside [0, 2^31]", who, what, n); return false; }
    return true;
}
static RmCascades rm_cascades(int C, int H, float bound) {
    RmCascades cs;
    for (int c = 0; c < MIRRES_RM_MAX_CASCADES; c++) {
        const double b = fmin(exp2((double)c), (double)bound), h = b / (double)H;     // renderer.py:1478-1479 in Python's doubles
        cs.scale[c] = (float)(b - h); cs.hgs[c] = (float)h; cs.hgs2[c] = (float)(h * 2.0);
    }
    return cs;
}

}  // namespace mr
using namespace mr;

#define RM_NEED(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return MIRRES_E_ARG; } } while (0)
#define RM_LAUNCH(kernel, n, block, ...) kernel<<<grid_for((size_t)(n), block), block, 0, (hipStream_t)stream>>>(__VA_ARGS__)

extern "C" int mirres_rm_near_far(const float* rays_o, const float* rays_d, const float* aabb, long long N, float min_near, float* nears, float* fars, void* stream) {
    if (!rm_count_ok("mirres_rm_near_far", "N", N)) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    RM_NEED(rays_o && rays_d && aabb && nears && fars, "mirres_rm_near_far: NULL argument");
    RM_LAUNCH(k_rm_near_far, N, RM_EW_BLOCK, rays_o, rays_d, aabb, N, min_near, nears, fars);
    MR_LAUNCH_CHECK("rm_near_far");
    return MIRRES_OK;
}

extern "C" int mirres_rm_morton3d(const int32_t* coords, long long N, int32_t* indices, void* stream) {
    if (!rm_count_ok("mirres_rm_morton3d", "N", N)) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    RM_NEED(coords && indices, "mirres_rm_morton3d: NULL argument");
    RM_LAUNCH(k_rm_morton3D, N, RM_EW_BLOCK, coords, N, indices);
    MR_LAUNCH_CHECK("rm_morton3D");
    return MIRRES_OK;
}

extern "C" int mirres_rm_morton3d_invert(const int32_t* indices, long long N, int32_t* coords, void* stream) {
    if (!rm_count_ok("mirres_rm_morton3d_invert", "N", N)) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    RM_NEED(coords && indices, "mirres_rm_morton3d_invert: NULL argument");
    RM_LAUNCH(k_rm_morton3D_invert, N, RM_EW_BLOCK, indices, N, coords);
    MR_LAUNCH_CHECK("rm_morton3D_invert");
    return MIRRES_OK;
}

extern "C" int mirres_rm_packbits(const float* grid, long long N, float thresh, uint8_t* bitfield, void* stream) {
    if (!rm_count_ok("mirres_rm_packbits", "N", N)) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    RM_NEED(grid && bitfield && ((uintptr_t)grid & 15) == 0, "mirres_rm_packbits: NULL or misaligned argument (the grid is read 16 bytes at a time)");
    RM_LAUNCH(k_rm_packbits, N, RM_EW_BLOCK, grid, N, thresh, bitfield);
    MR_LAUNCH_CHECK("rm_packbits");
    return MIRRES_OK;
}

extern "C" int mirres_rm_flatten_rays(const int32_t* rays, long long N, long long M, int32_t* res, void* stream) {
    if (!rm_count_ok("mirres_rm_flatten_rays", "N", N) || !rm_count_ok("mirres_rm_flatten_rays", "M", M)) return MIRRES_E_ARG;
    if (N == 0 || M == 0) return MIRRES_OK;
    RM_NEED(rays && res && N <= 0x7fffffffLL, "mirres_rm_flatten_rays: NULL argument or more than 2^31 - 1 rays");
    RM_LAUNCH(k_rm_flatten_rays, N, RM_EW_BLOCK, rays, N, M, res);
    MR_LAUNCH_CHECK("rm_flatten_rays");
    return MIRRES_OK;
}

static int rm_march_args(const char* who, const void* o, const void* d, const void* nears, const void* fars, const void* noises, float dt_gamma, int max_steps) {
    RM_NEED(o && d && nears && fars && noises, "%s: NULL argument", who);
    RM_NEED(max_steps >= 1 && dt_gamma >= 0.f && dt_gamma < 3.0e38f, "%s: max_steps %d (>= 1), dt_gamma %g (finite, >= 0)", who, max_steps, (double)dt_gamma);
    return MIRRES_OK;
}

extern "C" int mirres_rm_march_train_count(const float* rays_o, const float* rays_d, const uint8_t* bitfield, float bound, int contract, float dt_gamma, int max_steps,
                                           long long N, int C, int H, const float* nears, const float* fars, const float* noises, int32_t* rays, void* stream) {
    if (!rm_count_ok("mirres_rm_march_train_count", "N", N) || !rm_grid_ok("mirres_rm_march_train_count", C, H, bound, bitfield, "bitfield")) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    if (int rc = rm_march_args("mirres_rm_march_train_count", rays_o, rays_d, nears, fars, noises, dt_gamma, max_steps)) return rc;
    RM_NEED(rays, "mirres_rm_march_train_count: rays is NULL");
    const RmGrid g = rm_grid(bitfield, (uint32_t)C, (uint32_t)H, bound, contract, dt_gamma, (uint32_t)max_steps);
    RM_LAUNCH(k_rm_march_train<false>, N, RM_BLOCK, rays_o, rays_d, g, (uint32_t)max_steps, N, nears, fars, noises, rays, 0, nullptr, nullptr, nullptr);
    MR_LAUNCH_CHECK("rm_march_train_count");
    return MIRRES_OK;
}

extern "C" int mirres_rm_march_train_scan(int32_t* rays, long long N, long long* total, void* stream) {
    if (!rm_count_ok("mirres_rm_march_train_scan", "N", N)) return MIRRES_E_ARG;
    RM_NEED(total && (rays || N == 0), "mirres_rm_march_train_scan: NULL argument");
    k_rm_scan<<<1, RM_SCAN_BLOCK, 0, (hipStream_t)stream>>>(rays, N, total);
    MR_LAUNCH_CHECK("rm_march_train_scan");
    return MIRRES_OK;
}

extern "C" int mirres_rm_march_train_write(const float* rays_o, const float* rays_d, const uint8_t* bitfield, float bound, int contract, float dt_gamma, int max_steps,
                                           long long N, int C, int H, const float* nears, const float* fars, const float* noises, const int32_t* rays, long long M,
                                           float* xyzs, float* dirs, float* ts, void* stream) {
    if (!rm_count_ok("mirres_rm_march_train_write", "N", N) || !rm_grid_ok("mirres_rm_march_train_write", C, H, bound, bitfield, "bitfield")) return MIRRES_E_ARG;
    RM_NEED(M >= 0 && M <= 0x7fffffffLL, "mirres_rm_march_train_write: M %lld outside [0, 2^31 - 1] (the offsets in rays are int32)", M);
    if (N == 0 || M == 0) return MIRRES_OK;
    if (int rc = rm_march_args("mirres_rm_march_train_write", rays_o, rays_d, nears, fars, noises, dt_gamma, max_steps)) return rc;
    RM_NEED(rays && xyzs && dirs && ts, "mirres_rm_march_train_write: NULL argument");
    const RmGrid g = rm_grid(bitfield, (uint32_t)C, (uint32_t)H, bound, contract, dt_gamma, (uint32_t)max_steps);
    RM_LAUNCH(k_rm_march_train<true>, N, RM_BLOCK, rays_o, rays_d, g, (uint32_t)max_steps, N, nears, fars, noises, (int32_t*)rays, M, xyzs, dirs, ts);
    MR_LAUNCH_CHECK("rm_march_train_write");
    return MIRRES_OK;
}

extern "C" int mirres_rm_composite_train_fwd(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, long long M, long long N, float T_thresh,
                                             int alpha_mode, float* weights, float* weights_sum, float* depth, float* image, void* stream) {
    if (!rm_count_ok("mirres_rm_composite_train_fwd", "N", N) || !rm_count_ok("mirres_rm_composite_train_fwd", "M", M)) return MIRRES_E_ARG;
    if (N == 0) return MIRRES_OK;
    RM_NEED(rays && weights_sum && depth && image && (M == 0 || (sigmas && rgbs && ts && weights)), "mirres_rm_composite_train_fwd: NULL argument");
    RM_LAUNCH(k_rm_composite_train_fwd, N, RM_BLOCK, sigmas, rgbs, ts, rays, M, N, T_thresh, alpha_mode, weights, weights_sum, depth, image);
    MR_LAUNCH_CHECK("rm_composite_train_fwd");
    return MIRRES_OK;
}

extern "C" int mirres_rm_composite_train_bwd(const float* grad_weights, const float* grad_weights_sum, const float* grad_depth, const float* grad_image,
                                             const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, const float* weights_sum, const float* depth,
                                             const float* image, long long M, long long N, float T_thresh, int alpha_mode, float* grad_sigmas, float* grad_rgbs,
                                             void* stream) {
    if (!rm_count_ok("mirres_rm_composite_train_bwd", "N", N) || !rm_count_ok("mirres_rm_composite_train_bwd", "M", M)) return MIRRES_E_ARG;
    if (N == 0 || M == 0) return MIRRES_OK;
    RM_NEED(grad_weights && grad_weights_sum && grad_depth && grad_image && sigmas && rgbs && ts && rays && weights_sum && depth && image && grad_sigmas && grad_rgbs,
            "mirres_rm_composite_train_bwd: NULL argument");
    RM_LAUNCH(k_rm_composite_train_bwd, N, RM_BLOCK, grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, M, N,
              T_thresh, alpha_mode, grad_sigmas, grad_rgbs);
    MR_LAUNCH_CHECK("rm_composite_train_bwd");
    return MIRRES_OK;
}

extern "C" int mirres_rm_march(long long n_alive, int n_step, const int32_t* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d, long long N,
                               float bound, int contract, float dt_gamma, int max_steps, int C, int H, const uint8_t* bitfield, const float* nears, const float* fars,
                               float* xyzs, float* dirs, float* ts, const float* noises, void* stream) {
    if (!rm_count_ok("mirres_rm_march", "n_alive", n_alive) || !rm_count_ok("mirres_rm_march", "N", N) || !rm_grid_ok("mirres_rm_march", C, H, bound, bitfield, "bitfield"))
        return MIRRES_E_ARG;
    RM_NEED(n_step >= 1 && n_step <= 65536, "mirres_rm_march: n_step %d outside [1, 65536]", n_step);
    if (n_alive == 0) return MIRRES_OK;
    if (int rc = rm_march_args("mirres_rm_march", rays_o, rays_d, nears, fars, noises, dt_gamma, max_steps)) return rc;
    RM_NEED(rays_alive && rays_t && xyzs && dirs && ts, "mirres_rm_march: NULL argument");
    const RmGrid g = rm_grid(bitfield, (uint32_t)C, (uint32_t)H, bound, contract, dt_gamma, (uint32_t)max_steps);
    RM_LAUNCH(k_rm_march, n_alive, RM_BLOCK, n_alive, (uint32_t)n_step, rays_alive, rays_t, rays_o, rays_d, N, g, nears, fars, xyzs, dirs, ts, noises);
    MR_LAUNCH_CHECK("rm_march");
    return MIRRES_OK;
}

extern "C" int mirres_rm_composite(long long n_alive, int n_step, long long N, float T_thresh, int alpha_mode, int32_t* rays_alive, float* rays_t, const float* sigmas,
                                   const float* rgbs, const float* ts, float* weights_sum, float* depth, float* image, void* stream) {
    if (!rm_count_ok("mirres_rm_composite", "n_alive", n_alive) || !rm_count_ok("mirres_rm_composite", "N", N)) return MIRRES_E_ARG;
    RM_NEED(n_step >= 1 && n_step <= 65536, "mirres_rm_composite: n_step %d outside [1, 65536]", n_step);
    if (n_alive == 0) return MIRRES_OK;
    RM_NEED(rays_alive && rays_t && sigmas && rgbs && ts && weights_sum && depth && image, "mirres_rm_composite: NULL argument");
    RM_LAUNCH(k_rm_composite, n_alive, RM_BLOCK, n_alive, (uint32_t)n_step, N, T_thresh, alpha_mode, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image);
    MR_LAUNCH_CHECK("rm_composite");
    return MIRRES_OK;
}

extern "C" int mirres_rm_grid_mark_untrained(float* grid, int C, int H, float bound, const float* poses, int B, const float* intrinsics, int per_cam_intrinsics,
                                             const float* cam_near_far, float min_near, const float* aabb, void* stream) {
    if (!rm_grid_ok("mirres_rm_grid_mark_untrained", C, H, bound, grid, "density grid")) return MIRRES_E_ARG;
    RM_NEED(B >= 0 && B <= (1 << 24) && aabb && (B == 0 || (poses && intrinsics)), "mirres_rm_grid_mark_untrained: %d cameras, or a NULL argument", B);
    const long long cells = (long long)C * H * H * H;
    RM_LAUNCH(k_rm_grid_mark, cells, RM_EW_BLOCK, grid, C, (uint32_t)H, rm_cascades(C, H, bound), poses, intrinsics, per_cam_intrinsics, cam_near_far, B, min_near, aabb);
    MR_LAUNCH_CHECK("rm_grid_mark_untrained");
    return MIRRES_OK;
}

extern "C" int mirres_rm_grid_update(const mirres_density_t* net, float field_bound, float* grid, int C, int H, float bound, const float* noise, float decay,
                                     void* stream) {
    if (!dn_net_ok(net, "mirres_rm_grid_update") || !rm_grid_ok("mirres_rm_grid_update", C, H, bound, grid, "density grid")) return MIRRES_E_ARG;
    RM_NEED(noise && field_bound > 0.f && field_bound < 3.0e38f && decay == decay, "mirres_rm_grid_update: NULL noise, field bound %g or decay %g", (double)field_bound,
            (double)decay);
    const long long cells = (long long)C * H * H * H;
    RM_LAUNCH(k_rm_grid_update, cells, DN_BLOCK, *net, field_bound, grid, C, (uint32_t)H, rm_cascades(C, H, bound), noise, decay);
    MR_LAUNCH_CHECK("rm_grid_update");
    return MIRRES_OK;
}
