// grid_tv.hip — the in-place total-variation regulariser of the stage-0 hash grid: GridEncoder.grad_total_variation (gridencoder/grid.py:170-192) over
// kernel_grad_tv (gridencoder/src/gridencoder.cu:505-609), D = 3, C = 2, align_corners False, fp32 table.  Per sample point and level the reference takes the
// point's cell (corner 0 of the encoder's interpolation), its up to six axis neighbours, and adds w * sum(diff) / sqrt(sum(diff^2) + 1e-9) per channel to the
// cell's entry of the table's gradient with an fp32 atomic.  Every point of one cell adds the SAME number to the SAME address, and a trained scene's samples share
// their coarse cells (DESIGN.md section 5.15 measured what that costs a scatter).  So the work is split by what a level is (section 5.16):
//   DENSE levels (entry <-> cell one to one): count the points per cell with INTEGER atomics (exact in any order) into the workspace — levels whose (res + 1)^3
//     words fit 64 KB go through a block-private LDS histogram (k_tv_count_lds: the contention stays on chip, a block adds each cell it met once), the other
//     dense levels merge equal cells inside the wave with ballots before one global add per distinct cell (k_tv_points) — then one thread per entry with a
//     count computes the value ONCE and stores grad + (float)count * value (k_tv_apply).  No fp32 atomic: one fixed set of bits per multiset of points.
//   HASHED levels: fp32 atomics of the value (k_tv_points); the lanes of a wave that hold the same cell are merged first ((float)k * value, k <= 64), an entry's
//     two channels are issued by a lane pair as one request (dn_pair_add, as in radiance_bwd.hip's rb_scatter).  The order of the adds is not fixed.
// The term's arithmetic is FIXED and restated by tests/tv_refs.py: u and c are the encoder's (dn_unit, dn_cell of device_density.hpp); e = dn_index(c); for d = 0, 1, 2: the right neighbour (c[d] + 1, when
// c[d] < resolution), then the left (c[d] - 1, when c[d] > 0), per channel diff = t[e] - t[nb], res = res + diff, idelta = idelta + diff * diff;
// value = (w * res) * mr_rcp(mr_sqrt(idelta + 1e-9f)), w = weight / 6.0f — IEEE 1 / sqrt where the reference has the approximate rsqrtf.
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"
#include "device_scan.hpp"

namespace mr {

#define TV_BLOCK 256
#define TV_LDS_WORDS 16384                                         // 64 KB: level 0 (17^3 = 4913) and level 1 (24^3 = 13824) of the reference's layout
#define TV_LDS_BLOCKS 512                                          // k_tv_count_lds's grid per level: every block adds each cell it met once

enum { TV_HASHED = 0, TV_DENSE = 1, TV_DENSE_LDS = 2 };
struct TvPlan {
    int mode[DN_LEVELS];                                           // TV_*
    int base[DN_LEVELS];                                           // a dense level's first word in the workspace
    int bits[DN_LEVELS];                                           // the bits of the level's largest entry: how many ballots match two entries
    int lds[DN_LEVELS], n_lds;                                     // the levels k_tv_count_lds takes
    int dense[DN_LEVELS], n_dense;                                 // the levels k_tv_apply takes
};

// the term of cell c whose entry is e; hashed: V.hashed, as the constant the caller knows it to be.  A neighbour that is not taken is read at e (a valid address) and not added.
MR_DEV void tv_value(const float2* __restrict__ table, const DnLevel& V, bool hashed, const uint32_t c[3], uint32_t e, float w, float& v0, float& v1) {
    const float2* __restrict__ g = table + (size_t)V.first;
    const uint32_t s1 = V.s1, hs = V.hs, res = V.s1 - 1u;
    const bool take[6] = {c[0] < res, c[0] > 0u, c[1] < res, c[1] > 0u, c[2] < res, c[2] > 0u};
    const uint32_t nb[6] = {dn_index(c[0] + 1u, c[1], c[2], s1, hs, hashed), dn_index(c[0] - 1u, c[1], c[2], s1, hs, hashed), dn_index(c[0], c[1] + 1u, c[2], s1, hs, hashed),
                            dn_index(c[0], c[1] - 1u, c[2], s1, hs, hashed), dn_index(c[0], c[1], c[2] + 1u, s1, hs, hashed), dn_index(c[0], c[1], c[2] - 1u, s1, hs, hashed)};
    const float2 t = g[e];
    float2 q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = g[take[k] ? nb[k] : e];
    float r0 = 0.f, r1 = 0.f, i0 = 0.f, i1 = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (take[k]) {
            const float d0 = t.x - q[k].x, d1 = t.y - q[k].y;
            r0 = r0 + d0; i0 = i0 + d0 * d0;
            r1 = r1 + d1; i1 = i1 + d1 * d1;
        }
    }
    v0 = (w * r0) * mr_rcp(mr_sqrt(i0 + 1e-9f));
    v1 = (w * r1) * mr_rcp(mr_sqrt(i1 + 1e-9f));
}

// the lanes of the wave that are valid and hold the same key (< 2^bits) as this lane; every lane of the wave must arrive.  An integer use of wave_digit_rank's match.
MR_DEV uint64_t tv_match(uint32_t key, bool valid, int bits) {
    uint64_t m = __ballot(valid);
    for (int b = 0; b < bits; b++) { const bool bit = (key >> b) & 1u; const uint64_t bal = __ballot(bit); m &= bit ? bal : ~bal; }
    return m;
}

// pass 1 of a dense level that fits the LDS: a block-private histogram of the cells of this block's points, then one global integer add per cell it met
__global__ void __launch_bounds__(TV_BLOCK) k_tv_count_lds(mirres_density_t N, TvPlan P, const float* __restrict__ pos, long long n, float bound, uint32_t* __restrict__ ws) {
    __shared__ uint32_t hist[TV_LDS_WORDS];
    const int l = P.lds[blockIdx.y];
    const DnLevel V = dn_level(N, l);
    const uint32_t cells = V.s1 * V.s1 * V.s1;                                       // <= TV_LDS_WORDS: the host chose the level
    for (uint32_t k = threadIdx.x; k < cells; k += TV_BLOCK) hist[k] = 0u;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * TV_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TV_BLOCK) {
        float u[3], f[3], o[3]; uint32_t c[3];
        if (!dn_unit(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], bound, u)) continue;
        dn_cell(V, u, c, f, o);
        const uint32_t idx = c[0] + c[1] * V.s1 + c[2] * (V.s1 * V.s1);
        if (idx < cells) atomicAdd(&hist[idx], 1u);                                  // u in [0, 1]: c <= resolution - 1 on every axis, so the guard never fires
    }
    __syncthreads();
    uint32_t* const out = ws + P.base[l];
    for (uint32_t k = threadIdx.x; k < cells; k += TV_BLOCK) { const uint32_t v = hist[k]; if (v) atomicAdd(out + k, v); }
}

// one thread per point, blockIdx.y = level (the levels of k_tv_count_lds leave at once).  A dense level: the wave's equal cells add their number once.
// A hashed level: the value, merged over the wave's equal cells, by fp32 atomics.  No early return before the ballots and shuffles: every lane arrives.
__global__ void __launch_bounds__(TV_BLOCK) k_tv_points(mirres_density_t N, TvPlan P, const float* __restrict__ pos, long long n, float bound, float w,
                                                        float* __restrict__ grad, uint32_t* __restrict__ ws) {
    const int l = blockIdx.y;
    const int mode = P.mode[l];
    if (mode == TV_DENSE_LDS) return;                                                // block-uniform
    const long long i = (long long)blockIdx.x * TV_BLOCK + threadIdx.x;
    float u[3] = {0.f, 0.f, 0.f}, f[3], o[3];
    const bool valid = i < n && dn_unit(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], bound, u);
    const DnLevel V = dn_level(N, l);
    const bool hashed = mode == TV_HASHED;                                           // tv_plan's word for V.hashed
    uint32_t c[3];
#pragma unroll
    for (int d = 0; d < 3; d++) u[d] = valid ? u[d] : 0.f;                           // a lane that is not valid holds cell 0 and adds nothing
    dn_cell(V, u, c, f, o);
    const uint32_t e = dn_index(c[0], c[1], c[2], V.s1, V.hs, hashed);                                         // < hs: inside the level
    const int lane = lane_id();
    const uint64_t m = tv_match(e, valid, P.bits[l]);
    const int leader = valid ? __builtin_ctzll(m) : lane;
    if (!hashed) {
        if (valid && lane == leader) atomicAdd(ws + P.base[l] + e, (uint32_t)__popcll(m));
        return;
    }
    // two cells of a hashed level may share an entry: only the lanes that hold the leader's cell are merged into it, the others add their own term
    const bool same = valid && c[0] == (uint32_t)__shfl((int)c[0], leader, 64) && c[1] == (uint32_t)__shfl((int)c[1], leader, 64) && c[2] == (uint32_t)__shfl((int)c[2], leader, 64);
    const uint64_t merged = m & __ballot(same);
    const bool ok = valid && (lane == leader || !same);
    float v0 = 0.f, v1 = 0.f;
    if (ok) {
        tv_value((const float2*)N.table, V, true, c, e, w, v0, v1);
        const float k = lane == leader ? (float)__popcll(merged) : 1.0f;             // <= 64: exact; 1 * v = v
        v0 = k * v0; v1 = k * v1;
    }
    dn_pair_add(grad + 2 * (size_t)V.first, e, ok, v0, v1);
}

// pass 2 of the dense levels: one thread per entry, blockIdx.y = which dense level; an entry no point fell into is not touched
__global__ void __launch_bounds__(TV_BLOCK) k_tv_apply(mirres_density_t N, TvPlan P, float w, float* __restrict__ grad, const uint32_t* __restrict__ ws) {
    const int l = P.dense[blockIdx.y];
    const DnLevel V = dn_level(N, l);                                                // P.dense holds dense levels only: hashed is the constant false below
    const uint32_t s1 = V.s1;
    const uint32_t e = blockIdx.x * TV_BLOCK + threadIdx.x;
    if (e >= s1 * s1 * s1) return;                                                   // <= hs (dn_net_ok); the level's padding holds no cell
    const uint32_t count = ws[P.base[l] + e];
    if (!count) return;
    const uint32_t c[3] = {e % s1, (e / s1) % s1, e / (s1 * s1)};
    float v0, v1;
    tv_value((const float2*)N.table, V, false, c, e, w, v0, v1);
    float2* const g = (float2*)grad + (size_t)V.first + e;
    const float2 old = *g;
    const float k = (float)count;                                                    // rounds above 2^24 points in one cell
    *g = make_float2(old.x + k * v0, old.y + k * v1);
}

// the split of the levels; words = the workspace's u32 words (all entries of the dense levels, level after level)
static long long tv_plan(const mirres_density_t* N, TvPlan* P) {
    long long words = 0;
    P->n_lds = P->n_dense = 0;
    for (int l = 0; l < DN_LEVELS; l++) { P->mode[l] = TV_HASHED; P->base[l] = 0; P->bits[l] = 0; P->lds[l] = 0; P->dense[l] = 0; }
    for (int l = 0; l < N->num_levels; l++) {
        const unsigned long long s1 = (unsigned long long)N->resolution[l] + 1ull, hs = (unsigned long long)(N->offsets[l + 1] - N->offsets[l]);
        while (P->bits[l] < 32 && ((hs - 1ull) >> P->bits[l])) P->bits[l]++;
        if (N->hashed[l]) continue;
        P->base[l] = (int)words;
        words += (long long)hs;
        P->dense[P->n_dense++] = l;
        if (s1 * s1 * s1 <= (unsigned long long)TV_LDS_WORDS) { P->mode[l] = TV_DENSE_LDS; P->lds[P->n_lds++] = l; }
        else P->mode[l] = TV_DENSE;
    }
    return words;
}

}  // namespace mr
using namespace mr;

extern "C" long long mirres_grid_tv_workspace_bytes(const mirres_density_t* net) {
    if (!dn_net_ok(net, "mirres_grid_tv_workspace_bytes", 0)) return MIRRES_E_ARG;
    TvPlan P;
    const long long words = tv_plan(net, &P);
    return 4 * (words > 0 ? words : 1);
}

extern "C" int mirres_grid_tv_grad(const mirres_density_t* net, const float* pos, long long n, float bound, float weight, float* grad_table, void* workspace,
                                   long long workspace_bytes, void* stream) {
    const char* who = "mirres_grid_tv_grad";
    if (!dn_net_ok(net, who, 1)) return MIRRES_E_ARG;
    if (n < 0 || n > (1LL << 31)) { set_error("%s: n %lld outside [0, 2^31]", who, n); return MIRRES_E_ARG; }
    if (n > 0 && !pos) { set_error("%s: pos is NULL for %lld points", who, n); return MIRRES_E_ARG; }
    if (!grad_table) { set_error("%s: grad_table is NULL", who); return MIRRES_E_ARG; }
    if (!(weight >= 0.f) || !(weight < INFINITY)) { set_error("%s: weight %g is negative or not finite", who, (double)weight); return MIRRES_E_ARG; }
    if (!(bound > 0.f) || !(bound < 3.0e38f)) { set_error("%s: bound %g is not positive", who, (double)bound); return MIRRES_E_ARG; }
    TvPlan P;
    const long long words = tv_plan(net, &P), need = 4 * (words > 0 ? words : 1);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %s, %lld bytes given, mirres_grid_tv_workspace_bytes asks for %lld", who, workspace ? "too small" : "is NULL", workspace_bytes, need);
        return MIRRES_E_ARG;
    }
    if (n == 0 || weight == 0.f) return MIRRES_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* const ws = (uint32_t*)workspace;
    const float w = weight / 6.0f;
    const int blocks = grid_for((size_t)n, TV_BLOCK);
    if (words > 0) MR_HIP(hipMemsetAsync(ws, 0, (size_t)words * 4, s));
    if (P.n_lds > 0) {
        k_tv_count_lds<<<dim3(blocks < TV_LDS_BLOCKS ? blocks : TV_LDS_BLOCKS, P.n_lds), TV_BLOCK, 0, s>>>(*net, P, pos, n, bound, ws);
        MR_LAUNCH_CHECK("tv_count_lds");
    }
    if (P.n_lds < net->num_levels) {
        k_tv_points<<<dim3(blocks, net->num_levels), TV_BLOCK, 0, s>>>(*net, P, pos, n, bound, w, grad_table, ws);
        MR_LAUNCH_CHECK("tv_points");
    }
    if (P.n_dense > 0) {
        unsigned long long most = 0;
        for (int k = 0; k < P.n_dense; k++) { const unsigned long long s1 = (unsigned long long)net->resolution[P.dense[k]] + 1ull; if (s1 * s1 * s1 > most) most = s1 * s1 * s1; }
        k_tv_apply<<<dim3(grid_for((size_t)most, TV_BLOCK), P.n_dense), TV_BLOCK, 0, s>>>(*net, P, w, grad_table, ws);
        MR_LAUNCH_CHECK("tv_apply");
    }
    return MIRRES_OK;
}
