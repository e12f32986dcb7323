// device_grid.hpp — the material field's device code (multi-resolution hash grid with tcnn HashGrid semantics + the bias-free 32-32-32-6 MLP), shared by the forward
// kernels (matnet.hip) and the backward's forward recompute, position gradient and gradient scatter (backward.hip): one definition, so the recompute reproduces the
// forward's bits. What both sides call: normalise_pos (point -> unit cube), level_cell / corner_indices / corner_weight (cell, table entries and trilinear weights of
// one level), interpolate_cell over weighted_half2 (the fp16 interpolation), dense_layer (one k-ascending fmaf-chain layer) and stage_weights; MatNetD / matd() are
// the field as every kernel receives it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <cmath>
#include "engine.hpp"
#include "device_math.hpp"

namespace mr {

// level table of MLPTexture3D's encoder (render_helper.py:64-76): 16 levels, base resolution 16, T = 2^19, per-level scale exp(ln(256)/15)
#define MR_LEVELS 16

struct GridLevels { float scale[MR_LEVELS]; uint32_t res[MR_LEVELS]; uint32_t size[MR_LEVELS]; uint32_t offset[MR_LEVELS]; };

static GridLevels host_levels(uint32_t* total) {
    GridLevels L;
    const float per_level_scale = 1.4472692012786865f;  // fp32(exp(log(4096/16)/15)), render_helper.py:64-76
    const float log2_pls = log2f(per_level_scale);
    uint32_t offset = 0;
    for (int i = 0; i < MR_LEVELS; i++) {
        float scale = exp2f(i * log2_pls) * 16 - 1.0f;
        uint32_t res = (uint32_t)ceilf(scale) + 1;
        uint64_t dense = (uint64_t)res * res * res;
        uint32_t params = dense > 0x7fffffffull ? 0x7fffffffu : (uint32_t)dense;
        params = (params + 7u) / 8u * 8u;
        if (params > (1u << 19)) params = 1u << 19;
        L.scale[i] = scale; L.res[i] = res; L.size[i] = params; L.offset[i] = offset;
        offset += params;
    }
    if (total) *total = offset;
    return L;
}

MR_DEV uint32_t grid_index(uint32_t size, uint32_t res, uint32_t px, uint32_t py, uint32_t pz) {
    uint32_t stride = 1, index = 0;
    if (stride <= size) { index += px * stride; stride *= res; }
    if (stride <= size) { index += py * stride; stride *= res; }
    if (stride <= size) { index += pz * stride; stride *= res; }
    if (size < stride) index = (px * 1u) ^ (py * 2654435761u) ^ (pz * 805459861u);
    return index % size;
}

// The cell of x (in [0,1]^3) on a level: pos = fmaf(scale, x, 0.5) (tcnn grid.h), pg = its integer part (corner 0 of the cell), p = its fraction.
MR_DEV void level_cell(float scale, const float x[3], uint32_t pg[3], float p[3]) {
#pragma unroll
    for (int d = 0; d < 3; d++) { float q = fmaf(scale, x[d], 0.5f); float fl = floorf(q); pg[d] = (uint32_t)(int)fl; p[d] = q - fl; }
}
// Trilinear weight of corner idx (bit d set: the far corner along d): the product over d, in ascending d, of corner_factor. The position gradient takes the
// product of two of the three factors.
MR_DEV float corner_factor(const float p[3], uint32_t idx, int d) { return (idx & (1u << d)) == 0 ? 1 - p[d] : p[d]; }
MR_DEV float corner_weight(const float p[3], uint32_t idx) {
    float w = 1.f;
#pragma unroll
    for (int d = 0; d < 3; d++) w *= corner_factor(p, idx, d);
    return w;
}
// (T)(weight * value) of tcnn's interpolation (grid.h): the fp32 product is ROUNDED TO fp32 and then to fp16. Left to itself the compiler turns
// fptrunc(fmul) into v_fma_mixlo_f16 — one rounding of the exact product — whenever it does not happen to pack the multiplication with a neighbour
// (round 2: -fno-vectorize changed 1 feature in ~10^4 by one fp16 ulp against tcnn's two-step rounding); the empty asm pins the two-step form in every build.
// Both features of a table entry at once: the two fp16 roundings in one v_cvt_pk_f16_f32 (round to nearest even, like v_cvt_f16_f32) and the two
// fp16 additions in one v_pk_add_f16 — packed fp16, written out so that the instruction count does not depend on what a vectoriser finds.
MR_DEV __half2 weighted_half2(float w, __half2 v) {
    float p0 = w * __low2float(v), p1 = w * __high2float(v);
    asm("" : "+v"(p0), "+v"(p1));
    return __floats2half2_rn(p0, p1);
}
// One level's two features: the eight corners' entries, weighted and summed in fp16 in corner order (tcnn's accumulation).
MR_DEV __half2 interpolate_cell(const float p[3], const __half2 v[8]) {
    __half2 r = __floats2half2_rn(0.f, 0.f);
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) r = __hadd2(r, weighted_half2(corner_weight(p, idx), v[idx]));
    return r;
}
// The eight table entries of a cell, tcnn's grid_index for every corner (dx, dy, dz) at once — same values as grid_index(size, res, px + dx, py + dy,
// pz + dz), without its per-corner multiplications and its u32 modulo (a ~30-instruction sequence, eight times per level: it was most of the
// encoder's instructions). The level kind is uniform, so the branch is scalar:
//   hashed (res^3 > size, size = 2^19): (px + dx) ^ (py + dy) * P1 ^ (pz + dz) * P2 with the products of the +1 corners formed by one addition
//     (u32 arithmetic wraps, (p + 1) * P = p * P + P), and `% size` = `& (size - 1)`;
//   dense: px + py * res + pz * res^2 plus the corner strides; an index can pass `size` only at the far faces (a corner coordinate equal to res),
//     where it stays below 2 * size (res + res^2 + res^3 < 2 res^3), so `% size` is one conditional subtraction — the modulo is kept behind a
//     branch no wave takes for points inside the unit cube.
MR_DEV bool hashed(uint32_t size, uint32_t res) { return (uint64_t)res * res * res > (uint64_t)size && (size & (size - 1u)) == 0u; }
MR_DEV void corner_indices(uint32_t size, uint32_t res, const uint32_t pg[3], uint32_t idx[8]) {
    const bool dense = (uint64_t)res * res * res <= (uint64_t)size;
    if (hashed(size, res)) {
        const uint32_t m = size - 1u;
        const uint32_t hx[2] = {pg[0], pg[0] + 1u};
        const uint32_t y0 = pg[1] * 2654435761u, z0 = pg[2] * 805459861u;
        const uint32_t hy[2] = {y0, y0 + 2654435761u}, hz[2] = {z0, z0 + 805459861u};
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) idx[c] = (hx[c & 1u] ^ hy[(c >> 1) & 1u] ^ hz[c >> 2]) & m;
    } else if (dense) {
        const uint32_t r2 = res * res, base = pg[0] + pg[1] * res + pg[2] * r2;
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            uint32_t i = base + (c & 1u) + ((c >> 1) & 1u) * res + (c >> 2) * r2;
            i = i >= size ? i - size : i;
            if (i >= size) i %= size;
            idx[c] = i;
        }
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) idx[c] = grid_index(size, res, pg[0] + (c & 1u), pg[1] + ((c >> 1) & 1u), pg[2] + (c >> 2));
    }
}
// The eight entries of a cell in four 8-byte gathers where the table allows it: the corners (dx = 0, 1) of one (dy, dz) are neighbours in memory
// on a dense level (indices i, i + 1) and, on a hashed level, whenever px is even ((px + 1) ^ h = (px ^ h) ^ 1: the two entries of one aligned pair).
// Elsewhere — odd px on a hashed level, the wrap at a dense level's far face — the second entry is fetched by its own (lane-masked) gather.
// Same entries, same values: the encoder's time goes into these gathers (one L1 tag look-up per distinct line per instruction), not into arithmetic.
struct __attribute__((packed, aligned(4))) GridPair { uint32_t x, y; };
MR_DEV __half2 as_half2(uint32_t u) { __half2 h; __builtin_memcpy(&h, &u, 4); return h; }
MR_DEV void gather_cell(const __half2* __restrict__ g, const uint32_t ci[8], bool hashed, __half2 v[8]) {
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        const uint32_t i0 = ci[c], i1 = ci[c + 1];
        if (hashed) {
            const uint2 pr = *reinterpret_cast<const uint2*>(g + (i0 & ~1u));
            const bool odd = (i0 & 1u) != 0u;
            v[c] = as_half2(odd ? pr.y : pr.x);
            uint32_t o = odd ? pr.x : pr.y;
            if ((i0 ^ i1) != 1u) o = *reinterpret_cast<const uint32_t*>(g + i1);
            v[c + 1] = as_half2(o);
        } else {
            const GridPair pr = *reinterpret_cast<const GridPair*>(g + i0);
            v[c] = as_half2(pr.x);
            uint32_t o = pr.y;
            if (i1 != i0 + 1u) o = *reinterpret_cast<const uint32_t*>(g + i1);
            v[c + 1] = as_half2(o);
        }
    }
}

// ---------------------------------------------------------------- the field as the kernels receive it
struct MatNetD { const __half2* grid; const float *w0, *w1, *w2; float aabb_min[3], aabb_max[3], mn[6], mx[6]; };
static MatNetD matd(const mirres_matnet_t* m) {
    MatNetD M; M.grid = reinterpret_cast<const __half2*>(m->grid_f16); M.w0 = m->w0; M.w1 = m->w1; M.w2 = m->w2;
    for (int i = 0; i < 3; i++) { M.aabb_min[i] = m->aabb_min[i]; M.aabb_max[i] = m->aabb_max[i]; }
    for (int i = 0; i < 6; i++) { M.mn[i] = m->out_min[i]; M.mx[i] = m->out_max[i]; }
    return M;
}
// point i in the field's box: xraw = (pos - aabb_min) / (aabb_max - aabb_min), x = xraw clamped to [0, 1] (torch.clamp: the backward gates the position
// gradient on xraw)
MR_DEV float unit_coord(const MatNetD& M, const float* __restrict__ pos, size_t i, int d) { return (pos[3 * i + d] - M.aabb_min[d]) / (M.aabb_max[d] - M.aabb_min[d]); }
MR_DEV void normalise_pos(const MatNetD& M, const float* __restrict__ pos, size_t i, float x[3], float xraw[3]) {
#pragma unroll
    for (int d = 0; d < 3; d++) { xraw[d] = unit_coord(M, pos, i, d); x[d] = fminf(fmaxf(xraw[d], 0.f), 1.f); }
}
MR_DEV void normalise_pos(const MatNetD& M, const float* __restrict__ pos, size_t i, float x[3]) { float xraw[3]; normalise_pos(M, pos, i, x, xraw); }
// weights staged once per block in LDS (row-major [o][k] as given: the lanes of a wave read the same word, a broadcast)
MR_DEV void stage_weights(const MatNetD& M, float* sw0, float* sw1, float* sw2) {
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) { sw0[i] = M.w0[i]; sw1[i] = M.w1[i]; }
    for (int i = threadIdx.x; i < 192; i += blockDim.x) sw2[i] = M.w2[i];
    __syncthreads();
}
// One bias-free layer of 32 inputs: out[o] = act(chain, o) with the chain acc = fmaf(in[k], w[o][k], acc) from 0 in ASCENDING k (torch.nn.Linear in fp32 written as
// a chain, and the order k_mlp_mfma's K = 2 steps reproduce). The backward's recompute calls this too: its ReLU masks are the forward's only because the order is.
// act is applied where the chain ends (ActRelu, ActNone, or the forward's sigmoid / range): with the output layer's sigmoids in a loop of their own the compiler
// hoists that layer's 192 weight loads and the per-lane forward kernels go from 75 to 200 registers. UNROLL outputs are unrolled together: the per-lane forward
// kernels take a hidden layer in fours (a full unroll: 218 registers), k_matnet_bwd whole (in fours: 300 B more scratch); profiles/matnet_shared_regs.txt.
struct ActRelu { MR_DEV float operator()(float a, int) const { return fmaxf(a, 0.f); } };
struct ActNone { MR_DEV float operator()(float a, int) const { return a; } };
template <int NO, int UNROLL = NO, class Act>
MR_DEV void dense_layer(const float* w, const float in[32], float out[NO], Act act) {
#pragma unroll UNROLL
    for (int o = 0; o < NO; o++) { float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 32; k++) acc = fmaf(in[k], w[o * 32 + k], acc);
        out[o] = act(acc, o); }
}
}  // namespace mr
