// gridenc.hip — torch-ngp's GridEncoder as a stand-alone operator (encoding.py's GridEncoder): any of D in {2, 3}, C in {1, 2, 4, 8}, 1 .. 16 levels, gridtype
// hash / tiled, align_corners, linear / smoothstep, max_level.  The fused kernels (density.hip, radiance*.hip) stay the fast path of the one configuration the
// reference's network uses; for that configuration the kernels here give the same bits (device_gridenc.hpp restates the arithmetic of device_density.hpp's cell primitives), so each checks the other.
// The level table behind mirres_gridenc_layout and the range checks of gn_ok are grid_layout.hpp's, shared with mirres_density_layout and dn_net_ok.
//   mirres_gridenc_layout    GridEncoder.__init__'s level table (gridencoder/grid.py:104-135) and the kernel's per-level quantities (gridencoder.cu:137-139);
//   mirres_grid_encode_fwd   kernel_grid (:87-196): one thread per (point, level), blockIdx.y the level as in the reference, so the blocks that run together gather
//                            from one level's slice of the table; out is [n, L * C] directly (no [L, n, C] and permute).  Measured against one thread per point
//                            with a loop over the levels (rolled, unrolled 2 / 4 / 16, or with 16-byte stores of two levels): 0.58 ms against 0.71 - 0.86 ms for
//                            2^20 points of the reference's configuration;
//   mirres_grid_encode_bwd   the table's gradient (kernel_grid_backward :247-339): C ADJACENT LANES per (point, level), lane ch adds channel ch of every corner, so one
//                            entry's C * 4 bytes (one 32-byte sector at most) travel as ONE atomic request; blockIdx.y is the level, so the
//                            blocks that run together scatter into one level's slice of the table.  The order of the adds is not fixed.
//                            The input's gradient (dy_dx :198-243 and kernel_input_backward :343-368, nothing taped: the cell is recomputed): one thread per
//                            point, no atomics, levels ascending then axes ascending, in mirres_radiance_points_bwd_pos' order; bit-reproducible.
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_gridenc.hpp"

namespace mr {

// the C features of one in-bounds point on one level: all corners gathered, then accumulated in corner order
template <int D, int C>
MR_DEV void gn_features(const mirres_gridenc_t& G, const float* __restrict__ table, const float u[D], int l, float r[C]) {
    const GnLevel V = gn_level(G, D, l);
    uint32_t c[D]; float s[D], o[D], ds[D];
    gn_cell<D>(V, u, c, s, o, ds);
    float v[1 << D][C];
#pragma unroll
    for (int idx = 0; idx < (1 << D); idx++) gn_load<C>(table + (V.first + gn_corner<D>(V, c, idx)) * C, v[idx]);
#pragma unroll
    for (int ch = 0; ch < C; ch++) r[ch] = 0.f;
#pragma unroll
    for (int idx = 0; idx < (1 << D); idx++) {
        const float w = gn_weight<D>(s, o, idx);
#pragma unroll
        for (int ch = 0; ch < C; ch++) r[ch] = r[ch] + w * v[idx][ch];
    }
}

template <int D, int C>
__global__ void __launch_bounds__(GN_BLOCK) k_grid_encode(mirres_gridenc_t G, const float* __restrict__ table, const float* __restrict__ pos, long long n, float bound,
                                                          int max_level, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * GN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float u[D];
    const bool in = gn_unit<D>(pos, i, bound, u);
    float* __restrict__ row = out + (size_t)i * (size_t)(G.num_levels * C);
    const int l = blockIdx.y;                                       // < num_levels: the launch's grid
    float r[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) r[ch] = 0.f;
    if (in && l < max_level) gn_features<D, C>(G, table, u, l, r);
    gn_store<C>(row + l * C, r);
}

// grad_table += : thread t serves channel t % C of point t / C on level blockIdx.y
template <int D, int C>
__global__ void __launch_bounds__(GN_BLOCK) k_grid_encode_bwd_table(mirres_gridenc_t G, const float* __restrict__ pos, long long n, float bound,
                                                                    const float* __restrict__ grad_out, float* __restrict__ grad_table) {
    const long long t = (long long)blockIdx.x * GN_BLOCK + threadIdx.x;
    const long long i = t / C;
    const int ch = (int)(t % C);
    if (i >= n) return;
    float u[D];
    if (!gn_unit<D>(pos, i, bound, u)) return;                      // scatters nothing
    const int l = blockIdx.y;                                       // < min(max_level, num_levels): the launch's grid
    const GnLevel V = gn_level(G, D, l);
    uint32_t c[D]; float s[D], o[D], ds[D];
    gn_cell<D>(V, u, c, s, o, ds);
    const float g = grad_out[(size_t)i * (size_t)(G.num_levels * C) + (size_t)(l * C + ch)];
    float* __restrict__ gt = grad_table + V.first * C + ch;
#pragma unroll
    for (int idx = 0; idx < (1 << D); idx++) {
        const float w = gn_weight<D>(s, o, idx);
        atomicAdd(gt + (size_t)gn_corner<D>(V, c, idx) * C, w * g);
    }
}

template <int D, int C>
__global__ void __launch_bounds__(GN_BLOCK) k_grid_encode_bwd_pos(mirres_gridenc_t G, const float* __restrict__ table, const float* __restrict__ pos, long long n,
                                                                  float bound, int max_level, const float* __restrict__ grad_out, float* __restrict__ grad_pos) {
    const long long i = (long long)blockIdx.x * GN_BLOCK + threadIdx.x;
    if (i >= n) return;
    float u[D], gu[D];
#pragma unroll
    for (int d = 0; d < D; d++) gu[d] = 0.f;
    if (!gn_unit<D>(pos, i, bound, u)) {                            // constant (zero) features
#pragma unroll
        for (int d = 0; d < D; d++) grad_pos[D * i + d] = 0.f;
        return;
    }
    const float* __restrict__ grow = grad_out + (size_t)i * (size_t)(G.num_levels * C);
    for (int l = 0; l < max_level; l++) {                           // max_level <= num_levels: the entry clamps it
        const GnLevel V = gn_level(G, D, l);
        uint32_t c[D]; float s[D], o[D], ds[D];
        gn_cell<D>(V, u, c, s, o, ds);
        float v[1 << D][C], g[C];
#pragma unroll
        for (int idx = 0; idx < (1 << D); idx++) gn_load<C>(table + (V.first + gn_corner<D>(V, c, idx)) * C, v[idx]);
        gn_load<C>(grow + l * C, g);
#pragma unroll
        for (int a = 0; a < D; a++) {
            float r[C];
#pragma unroll
            for (int ch = 0; ch < C; ch++) r[ch] = 0.f;
#pragma unroll
            for (int pr = 0; pr < (1 << (D - 1)); pr++) {           // the pairs of corners that differ in axis a alone; bit nd of pr: the nd-th other axis, ascending
                float w = V.scale;
                int left = 0;
#pragma unroll
                for (int nd = 0; nd < D - 1; nd++) {
                    const int d = nd >= a ? nd + 1 : nd;
                    const int bit = (pr >> nd) & 1;
                    w = w * (bit ? s[d] : o[d]);
                    left |= bit << d;
                }
                const int right = left | (1 << a);
#pragma unroll
                for (int ch = 0; ch < C; ch++) r[ch] = r[ch] + (w * (v[right][ch] - v[left][ch])) * ds[a];
            }
#pragma unroll
            for (int ch = 0; ch < C; ch++) gu[a] = gu[a] + g[ch] * r[ch];
        }
    }
    const float den = 2.0f * bound;
#pragma unroll
    for (int d = 0; d < D; d++) grad_pos[D * i + d] = gu[d] / den;
}

// what every entry that takes a layout checks before a launch
static bool gn_ok(const mirres_gridenc_t* G, const char* who) {
    if (!G) { set_error("%s: the layout is NULL", who); return false; }
    if (G->input_dim != 2 && G->input_dim != 3) { set_error("%s: input_dim %d, 2 or 3 are built", who, G->input_dim); return false; }
    if (G->level_dim != 1 && G->level_dim != 2 && G->level_dim != 4 && G->level_dim != 8) { set_error("%s: level_dim %d, 1, 2, 4 or 8 are built", who, G->level_dim); return false; }
    if (G->num_levels < 1 || G->num_levels > GN_LEVELS) { set_error("%s: num_levels %d outside [1, %d]", who, G->num_levels, GN_LEVELS); return false; }
    if ((G->gridtype != 0 && G->gridtype != 1) || (G->align_corners != 0 && G->align_corners != 1) || (G->interpolation != 0 && G->interpolation != 1)) {
        set_error("%s: gridtype %d (0 hash, 1 tiled), align_corners %d (0, 1), interpolation %d (0 linear, 1 smoothstep)", who, G->gridtype, G->align_corners, G->interpolation);
        return false;
    }
    if (G->offsets[0] != 0) { set_error("%s: the first level starts at entry %d, not 0", who, G->offsets[0]); return false; }
    if (!grid_levels_ok(who, "mirres_gridenc_layout", G->num_levels, G->offsets, G->resolution, G->scale)) return false;
    for (int l = 0; l < G->num_levels; l++) {
        const GnLevel V = gn_level(*G, G->input_dim, l);
        if ((G->hashed[l] != 0) != V.hash) { set_error("%s: level %d is marked %s but get_grid_index %s there", who, l, G->hashed[l] ? "hashed" : "not hashed", V.hash ? "hashes" : "does not hash"); return false; }
    }
    return true;
}

static bool gn_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int D, int C>
static void gn_launch_fwd(const mirres_gridenc_t& G, const float* table, const float* pos, long long n, float bound, int max_level, float* out, hipStream_t st) {
    k_grid_encode<D, C><<<dim3((unsigned)grid_for((size_t)n, GN_BLOCK), (unsigned)G.num_levels), GN_BLOCK, 0, st>>>(G, table, pos, n, bound, max_level, out);
}

template <int D, int C>
static void gn_launch_bwd(const mirres_gridenc_t& G, const float* table, const float* pos, long long n, float bound, int max_level, const float* grad_out, float* grad_table,
                          float* grad_pos, hipStream_t st) {
    if (grad_table && max_level > 0)
        k_grid_encode_bwd_table<D, C><<<dim3((unsigned)grid_for((size_t)n * C, GN_BLOCK), (unsigned)max_level), GN_BLOCK, 0, st>>>(G, pos, n, bound, grad_out, grad_table);
    if (grad_pos) k_grid_encode_bwd_pos<D, C><<<grid_for((size_t)n, GN_BLOCK), GN_BLOCK, 0, st>>>(G, table, pos, n, bound, max_level, grad_out, grad_pos);
}

#define GN_DISPATCH(G, CALL)                                                                                                             \
    do {                                                                                                                                 \
        const int key_ = (G)->input_dim * 16 + (G)->level_dim;                                                                           \
        switch (key_) {                                                                                                                  \
            case 2 * 16 + 1: { constexpr int D_ = 2, C_ = 1; CALL; } break;                                                              \
            case 2 * 16 + 2: { constexpr int D_ = 2, C_ = 2; CALL; } break;                                                              \
            case 2 * 16 + 4: { constexpr int D_ = 2, C_ = 4; CALL; } break;                                                              \
            case 2 * 16 + 8: { constexpr int D_ = 2, C_ = 8; CALL; } break;                                                              \
            case 3 * 16 + 1: { constexpr int D_ = 3, C_ = 1; CALL; } break;                                                              \
            case 3 * 16 + 2: { constexpr int D_ = 3, C_ = 2; CALL; } break;                                                              \
            case 3 * 16 + 4: { constexpr int D_ = 3, C_ = 4; CALL; } break;                                                              \
            default: { constexpr int D_ = 3, C_ = 8; CALL; } break;                                                                      \
        }                                                                                                                                \
    } while (0)

}  // namespace mr
using namespace mr;

extern "C" long long mirres_gridenc_layout(int input_dim, int level_dim, int num_levels, double per_level_scale, int base_resolution, int log2_hashmap_size, int gridtype,
                                           int align_corners, int interpolation, mirres_gridenc_t* g) {
    if (!g || (input_dim != 2 && input_dim != 3) || (level_dim != 1 && level_dim != 2 && level_dim != 4 && level_dim != 8) || num_levels < 1 || num_levels > GN_LEVELS ||
        !(per_level_scale > 0.0) || !(per_level_scale <= 16777216.0) || base_resolution < 1 || base_resolution > 65536 || log2_hashmap_size < 1 || log2_hashmap_size > 26 ||
        (gridtype != 0 && gridtype != 1) || (align_corners != 0 && align_corners != 1) || (interpolation != 0 && interpolation != 1)) {
        set_error("mirres_gridenc_layout: bad argument (input_dim %d in {2, 3}, level_dim %d in {1, 2, 4, 8}, num_levels %d in [1, %d], per_level_scale %g, base_resolution %d, "
                  "log2_hashmap_size %d in [1, 26], gridtype %d, align_corners %d, interpolation %d)", input_dim, level_dim, num_levels, GN_LEVELS, per_level_scale,
                  base_resolution, log2_hashmap_size, gridtype, align_corners, interpolation);
        return MIRRES_E_ARG;
    }
    g->input_dim = input_dim; g->level_dim = level_dim; g->num_levels = num_levels; g->gridtype = gridtype; g->align_corners = align_corners; g->interpolation = interpolation;
    return grid_layout("mirres_gridenc_layout", input_dim, align_corners != 0, gridtype == 0, true, num_levels, per_level_scale, base_resolution, log2_hashmap_size, g->offsets,
                       g->resolution, g->hashed, g->scale);
}

static bool gn_args_ok(const char* who, const mirres_gridenc_t* g, const float* table, const float* pos, long long n, float bound) {
    if (!gn_ok(g, who)) return false;
    if (n < 0 || n > (1LL << 31)) { set_error("%s: n %lld outside [0, 2^31]", who, n); return false; }
    if (!(bound > 0.f) || !(bound < 3.0e38f)) { set_error("%s: bound %g is not positive and finite", who, (double)bound); return false; }
    if (n > 0 && (!table || !pos)) { set_error("%s: table / pos is NULL", who); return false; }
    if (!gn_aligned(table)) { set_error("%s: the table must be 16-byte aligned", who); return false; }
    return true;
}

extern "C" int mirres_grid_encode_fwd(const mirres_gridenc_t* g, const float* table, const float* pos, long long n, float bound, int max_level, float* out, void* stream) {
    if (!gn_args_ok("mirres_grid_encode_fwd", g, table, pos, n, bound)) return MIRRES_E_ARG;
    if (max_level < 0) { set_error("mirres_grid_encode_fwd: max_level %d is negative", max_level); return MIRRES_E_ARG; }
    if ((n > 0 && !out) || !gn_aligned(out)) { set_error("mirres_grid_encode_fwd: out is %s", out ? "not 16-byte aligned" : "NULL"); return MIRRES_E_ARG; }
    if (n == 0) return MIRRES_OK;
    const int ml = max_level < g->num_levels ? max_level : g->num_levels;
    GN_DISPATCH(g, (gn_launch_fwd<D_, C_>(*g, table, pos, n, bound, ml, out, (hipStream_t)stream)));
    MR_LAUNCH_CHECK("grid_encode_fwd");
    return MIRRES_OK;
}

extern "C" int mirres_grid_encode_bwd(const mirres_gridenc_t* g, const float* table, const float* pos, long long n, float bound, int max_level, const float* grad_out,
                                      float* grad_table, float* grad_pos, void* stream) {
    if (!gn_args_ok("mirres_grid_encode_bwd", g, table, pos, n, bound)) return MIRRES_E_ARG;
    if (max_level < 0) { set_error("mirres_grid_encode_bwd: max_level %d is negative", max_level); return MIRRES_E_ARG; }
    if ((n > 0 && !grad_out) || !gn_aligned(grad_out) || !gn_aligned(grad_table)) {
        set_error("mirres_grid_encode_bwd: grad_out is %s, grad_table %s 16-byte aligned", grad_out ? "given" : "NULL", gn_aligned(grad_table) ? "is" : "is not");
        return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    const int ml = max_level < g->num_levels ? max_level : g->num_levels;
    GN_DISPATCH(g, (gn_launch_bwd<D_, C_>(*g, table, pos, n, bound, ml, grad_out, grad_table, grad_pos, (hipStream_t)stream)));
    MR_LAUNCH_CHECK("grid_encode_bwd");
    return MIRRES_OK;
}
