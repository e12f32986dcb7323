// radiance_bwd.hip — the adjoint of mirres_radiance_points (radiance.hip): from the cotangents of sigma and rgb to the gradients of the hash table and of the five
// weight matrices, what torch-ngp's training step asks of NeRFNetwork.forward (nerf/network.py:146-174).  Nothing is taped: the forward is recomputed from pos / dirs
// with the shared device functions (dn_encode, rd_sigma_net, rd_sh and the chains of rd_color_net); the scatter walks the same cells with dn_encode's primitives.
//   colour net   d_pre = grad_rgb * rgb (1 - rgb); a ReLU passes the cotangent where its output is > 0 (an output of exactly 0 passes nothing, as torch's
//                threshold_backward); the first layer's d_in[16..30] is d_geo_feat; the direction gets no gradient;
//   sigma        d_h16[0] = grad_sigma * mrf_exp(clamp(h16[0], -15, 15)) (trunc_exp's backward, activation.py:14-16), d_h16[1..15] = d_geo_feat;
//   position     no gradient (the reference asks for one under --sdf only).
// WEIGHT GRADIENTS (9344 values) are a GEMM with K = n and carry no atomics: a fixed grid of blocks, each looping over 256-point tiles.  Per tile every thread takes
// one point through the network and its adjoint; each layer's activation (64 rows in sA) and cotangent (32 rows at a time in sB: the 64-wide layers go in two halves)
// are staged in LDS as [row][point], and every thread adds the tile's 256 outer products of its own 37 matrix elements to register accumulators, points ascending.
// After the last tile a block writes its 9344 partial sums to workspace [blocks][9344]; k_radiance_bwd_reduce adds them in block order and adds the total to the
// caller's gradients: two runs on the same inputs and the same grid give the same bits.
// TABLE GRADIENT: fp32 atomics.  A corner's two channels are issued by a lane PAIR (even lane channel 0, odd lane channel 1 of the same entry: first the even lane's
// entry, then the odd lane's), so one entry is one memory request (README, round 6).  The order of the adds is not fixed: the last bits vary from run to run.
// Activations of a layer that is waiting for its turn are recomputed (layer 0 of the colour net, sigma_net's hidden layer) rather than kept: 31 persistent registers
// (sh, geo_feat) beside the accumulators.  The adjoint's loops over a layer's 64 neurons stay rolled, reading the cotangent back from this thread's column of sB: fully
// unrolled, their weight loads at compile-time addresses were scheduled hundreds at a time and spilled.  Every register array is indexed by compile-time constants
// only; -ffp-contract=off stays.
#include <math.h>
#include "engine.hpp"
#include "device_math.hpp"
#include "device_density.hpp"
#include "device_radiance.hpp"

namespace mr {

#define RB_TILE DN_BLOCK                             // points per tile = threads per block
#define RB_LD (RB_TILE + 4)                          // words per LDS row: consecutive rows start 4 banks apart (the 16 rows a wave's b128 reads meet tile the 64 banks), 16-byte aligned
#define RB_W0 0                                      // the layout of a partial and of the reduce kernel's index: [w0 64x32][w1 16x64][c0 64x31][c1 64x64][c2 3x64]
#define RB_W1 (RB_W0 + DN_HIDDEN * DN_FEAT)
#define RB_C0 (RB_W1 + RD_H16 * DN_HIDDEN)
#define RB_C1 (RB_C0 + RD_HIDDEN * RD_IN)
#define RB_C2 (RB_C1 + RD_HIDDEN * RD_HIDDEN)
#define RB_PARTIAL (RB_C2 + 3 * RD_HIDDEN)           // 9344
#define RB_DEFAULT_BLOCKS 1024

struct RbGrads { float* table; float* w0; float* w1; float* c0; float* c1; float* c2; };

// acc[i][j] += sum over the tile's points of sB[b0 + 16 i][p] * sA[a0 + 16 j][p], p ascending, four points per LDS read
template <int NB, int NA>
MR_DEV void rb_gemm(const float* sB, const float* sA, int b0, int a0, float (&acc)[NB][NA]) {
#pragma unroll 2
    for (int p = 0; p < RB_TILE; p += 4) {
        float4 b[NB], a[NA];
#pragma unroll
        for (int i = 0; i < NB; i++) b[i] = *(const float4*)(sB + (b0 + 16 * i) * RB_LD + p);
#pragma unroll
        for (int j = 0; j < NA; j++) a[j] = *(const float4*)(sA + (a0 + 16 * j) * RB_LD + p);
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int j = 0; j < NA; j++) {
                float s = acc[i][j];
                s = fmaf(b[i].x, a[j].x, s); s = fmaf(b[i].y, a[j].y, s); s = fmaf(b[i].z, a[j].z, s); s = fmaf(b[i].w, a[j].w, s);
                acc[i][j] = s;
            }
    }
}

// the table scatter of one point's d_feat, by lane pairs (dn_pair_add).  Every lane of the wave walks every level and corner, so that all reach the shuffles: a lane
// that is not ok runs on u = 0 (cell 0 of every level) and adds nothing
MR_DEV void rb_scatter(const mirres_density_t& N, float x, float y, float z, float bound, const float dfeat[DN_FEAT], bool ok, float* __restrict__ gtable) {
    float u[3];
    dn_unit(x, y, z, bound, u);
#pragma unroll
    for (int d = 0; d < 3; d++) u[d] = ok ? u[d] : 0.f;
#pragma unroll
    for (int l = 0; l < DN_LEVELS; l++) {
        if (l >= N.num_levels) continue;
        const DnLevel V = dn_level(N, l);
        float f[3], o[3]; uint32_t c[3];
        dn_cell(V, u, c, f, o);
        const float g0 = dfeat[2 * l], g1 = dfeat[2 * l + 1];
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float w = dn_weight(f, o, idx);
            dn_pair_add(gtable + 2 * (size_t)V.first, dn_corner(V, c, idx), ok, w * g0, w * g1);
        }
    }
}

__global__ void __launch_bounds__(DN_BLOCK) k_radiance_points_bwd(mirres_radiance_t N, const float* __restrict__ pos, const float* __restrict__ dirs, long long n, float bound,
                                                                  const float* __restrict__ grad_sigma, const float* __restrict__ grad_rgb, float* __restrict__ gtable,
                                                                  float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float sw[RD_LDS_WORDS];
    __shared__ __attribute__((aligned(16))) float sA[RD_HIDDEN * RB_LD];
    __shared__ __attribute__((aligned(16))) float sB[(RD_HIDDEN / 2) * RB_LD];
    rd_stage_weights(N, sw);
    const int t = threadIdx.x, kg = t & 15, og = t >> 4;
    float acc_c2[1][1] = {{0.f}}, acc_c1[2][2][4], acc_c0[2][2][2], acc_w1[1][4], acc_w0[2][2][2];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) acc_c1[h][i][j] = 0.f;
#pragma unroll
            for (int j = 0; j < 2; j++) { acc_c0[h][i][j] = 0.f; acc_w0[h][i][j] = 0.f; }
        }
#pragma unroll
    for (int j = 0; j < 4; j++) acc_w1[0][j] = 0.f;

    const long long tiles = (n + RB_TILE - 1) / RB_TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long i = tile * RB_TILE + t;
        const bool valid = i < n;
        // a lane past the end runs a harmless point with zero cotangents: every barrier below is reached by all threads
        const float x = valid ? pos[3 * i] : 0.f, y = valid ? pos[3 * i + 1] : 0.f, z = valid ? pos[3 * i + 2] : 0.f;
        float in[RD_IN], h0;
        bool inside;
        {
            float feat[DN_FEAT], h16[RD_H16];
            inside = dn_encode(N.grid, x, y, z, bound, feat);
            rd_sigma_net(sw, feat, h16);
            h0 = h16[0];
#pragma unroll
            for (int k = 0; k < RD_GEO; k++) in[RD_SH + k] = h16[1 + k];
        }
        rd_sh(valid ? dirs[3 * i] : 0.f, valid ? dirs[3 * i + 1] : 0.f, valid ? dirs[3 * i + 2] : 1.f, in);
        float dout[3];
        {   // colour net forward (rd_color_net's chains): layer 1's outputs go to sA as they are produced
            float a[RD_HIDDEN];
#pragma unroll
            for (int o = 0; o < RD_HIDDEN; o++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < RD_IN; k++) s = fmaf(in[k], sw[RD_LDS_C0 + o * RD_IN_PAD + k], s);
                a[o] = rd_relu(s);
            }
            float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll 2
            for (int o = 0; o < RD_HIDDEN; o++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < RD_HIDDEN; k++) s = fmaf(a[k], sw[RD_LDS_C1 + o * RD_HIDDEN + k], s);
                const float h = rd_relu(s);
                sA[o * RB_LD + t] = h;
                r = fmaf(h, sw[RD_LDS_C2 + 4 * o + 0], r);
                g = fmaf(h, sw[RD_LDS_C2 + 4 * o + 1], g);
                b = fmaf(h, sw[RD_LDS_C2 + 4 * o + 2], b);
            }
            const float rgb[3] = {mrf_sigmoid(r), mrf_sigmoid(g), mrf_sigmoid(b)};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dout[c] = valid ? grad_rgb[3 * i + c] * (rgb[c] * (1.0f - rgb[c])) : 0.f;
                sB[c * RB_LD + t] = dout[c];
            }
        }
        __syncthreads();
        if (t < 3 * RD_HIDDEN) rb_gemm<1, 1>(sB, sA, t >> 6, t & 63, acc_c2);                  // grad_c2[c][o] += d_out[c] a1[o]
        __syncthreads();

        // d_a1pre = relu'(a1) C2^T d_out; the upper half waits in registers while sB holds the lower one
        float hi[RD_HIDDEN / 2];
#pragma unroll
        for (int o = 0; o < RD_HIDDEN; o++) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 3; c++) s = fmaf(dout[c], sw[RD_LDS_C2 + 4 * o + c], s);
            s = sA[o * RB_LD + t] <= 0.f ? 0.f : s;
            if (o < RD_HIDDEN / 2) sB[o * RB_LD + t] = s; else hi[o - RD_HIDDEN / 2] = s;
        }
        // layer 0's outputs again, into sA over a1 (this thread's column only; every other thread is past the barrier above)
#pragma unroll 2
        for (int o = 0; o < RD_HIDDEN; o++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < RD_IN; k++) s = fmaf(in[k], sw[RD_LDS_C0 + o * RD_IN_PAD + k], s);
            sA[o * RB_LD + t] = rd_relu(s);
        }
        float d64[RD_HIDDEN];                                                                      // d_a0 = C1^T d_a1pre, accumulated as sB's halves pass
#pragma unroll
        for (int k = 0; k < RD_HIDDEN; k++) d64[k] = 0.f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h == 1) {
#pragma unroll
                for (int o = 0; o < RD_HIDDEN / 2; o++) sB[o * RB_LD + t] = hi[o];
            }
            __syncthreads();
            rb_gemm<2, 4>(sB, sA, og, kg, acc_c1[h]);                                             // grad_c1[32 h + og + 16 i][kg + 16 j] += d_a1pre a0
#pragma unroll 2
            for (int o = 0; o < RD_HIDDEN / 2; o++) {
                const float v = sB[o * RB_LD + t];
#pragma unroll
                for (int k = 0; k < RD_HIDDEN; k++) d64[k] = fmaf(sw[RD_LDS_C1 + (32 * h + o) * RD_HIDDEN + k], v, d64[k]);
            }
            __syncthreads();
        }
        // d_a0pre = relu'(a0) d_a0 -> sB in halves; sA's rows 0..31 <- the colour net's input (row 31: the pad column, zero); d_geo = rows 16..30 of C0^T d_a0pre,
        // accumulated from this thread's column of sB as the halves pass
#pragma unroll
        for (int o = 0; o < RD_HIDDEN; o++) d64[o] = sA[o * RB_LD + t] <= 0.f ? 0.f : d64[o];
#pragma unroll
        for (int k = 0; k < RD_IN; k++) sA[k * RB_LD + t] = in[k];
        sA[RD_IN * RB_LD + t] = 0.f;
        float dh16[RD_H16];
#pragma unroll
        for (int k = 0; k < RD_H16; k++) dh16[k] = 0.f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int o = 0; o < RD_HIDDEN / 2; o++) sB[o * RB_LD + t] = d64[32 * h + o];
            __syncthreads();
            rb_gemm<2, 2>(sB, sA, og, kg, acc_c0[h]);                                             // grad_c0[32 h + og + 16 i][kg + 16 j] += d_a0pre in (column 31 is dropped)
#pragma unroll 2
            for (int o = 0; o < RD_HIDDEN / 2; o++) {
                const float v = sB[o * RB_LD + t];
#pragma unroll
                for (int k = 0; k < RD_GEO; k++) dh16[1 + k] = fmaf(sw[RD_LDS_C0 + (32 * h + o) * RD_IN_PAD + RD_SH + k], v, dh16[1 + k]);
            }
            __syncthreads();
        }
        {
            const float e = mrf_exp(fminf(fmaxf(h0, -15.0f), 15.0f));
            dh16[0] = (valid && grad_sigma) ? grad_sigma[i] * e : 0.f;
        }
        // sigma_net: the encoder's features and the hidden layer again
        float feat[DN_FEAT];
        dn_encode(N.grid, x, y, z, bound, feat);
#pragma unroll 2
        for (int o = 0; o < DN_HIDDEN; o++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < DN_FEAT; k++) s = fmaf(feat[k], sw[RD_LDS_W0 + o * DN_FEAT + k], s);
            sA[o * RB_LD + t] = fmaxf(s, 0.f);
        }
#pragma unroll
        for (int k = 0; k < RD_H16; k++) sB[k * RB_LD + t] = dh16[k];
        __syncthreads();
        rb_gemm<1, 4>(sB, sA, og, kg, acc_w1);                                                    // grad_w1[og][kg + 16 j] += d_h16 h1
        __syncthreads();
        // d_h1pre = relu'(h1) W1^T d_h16: the lower half to sB, the upper half in place over h1's rows 32..63 of this thread's column, which no GEMM reads any more;
        // d_feat = W0^T d_h1pre; then sA's rows 0..31 <- the features
        float dfeat[DN_FEAT];
#pragma unroll
        for (int k = 0; k < DN_FEAT; k++) dfeat[k] = 0.f;
#pragma unroll 2
        for (int o = 0; o < DN_HIDDEN; o++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < RD_H16; k++) s = fmaf(sw[RD_LDS_W1 + o * RD_H16 + k], dh16[k], s);
            s = sA[o * RB_LD + t] > 0.f ? s : 0.f;
            if (o < DN_HIDDEN / 2) sB[o * RB_LD + t] = s; else sA[o * RB_LD + t] = s;
#pragma unroll
            for (int k = 0; k < DN_FEAT; k++) dfeat[k] = fmaf(sw[RD_LDS_W0 + o * DN_FEAT + k], s, dfeat[k]);
        }
#pragma unroll
        for (int k = 0; k < DN_FEAT; k++) sA[k * RB_LD + t] = feat[k];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h == 1) {
#pragma unroll 4
                for (int o = 0; o < DN_HIDDEN / 2; o++) sB[o * RB_LD + t] = sA[(DN_HIDDEN / 2 + o) * RB_LD + t];
            }
            __syncthreads();
            rb_gemm<2, 2>(sB, sA, og, kg, acc_w0[h]);                                             // grad_w0[32 h + og + 16 i][kg + 16 j] += d_h1pre feat
            __syncthreads();
        }
        rb_scatter(N.grid, x, y, z, bound, dfeat, valid && inside, gtable);
    }

    float* const P = partial + (size_t)blockIdx.x * RB_PARTIAL;
    if (t < 3 * RD_HIDDEN) P[RB_C2 + (t >> 6) * RD_HIDDEN + (t & 63)] = acc_c2[0][0];
#pragma unroll
    for (int j = 0; j < 4; j++) P[RB_W1 + og * DN_HIDDEN + kg + 16 * j] = acc_w1[0][j];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int o = 32 * h + og + 16 * i;
#pragma unroll
            for (int j = 0; j < 4; j++) P[RB_C1 + o * RD_HIDDEN + kg + 16 * j] = acc_c1[h][i][j];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int k = kg + 16 * j;
                P[RB_W0 + o * DN_FEAT + k] = acc_w0[h][i][j];
                if (k < RD_IN) P[RB_C0 + o * RD_IN + k] = acc_c0[h][i][j];
            }
        }
}

// out[e] += partial[0][e] + partial[1][e] + ... in block order
__global__ void __launch_bounds__(DN_BLOCK) k_radiance_bwd_reduce(const float* __restrict__ partial, int blocks, RbGrads G) {
    const int e = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (e >= RB_PARTIAL) return;
    float s = 0.f;
    for (int b = 0; b < blocks; b++) s = s + partial[(size_t)b * RB_PARTIAL + e];
    float* const out = e < RB_W1 ? G.w0 + (e - RB_W0) : e < RB_C0 ? G.w1 + (e - RB_W1) : e < RB_C1 ? G.c0 + (e - RB_C0) : e < RB_C2 ? G.c1 + (e - RB_C1) : G.c2 + (e - RB_C2);
    *out = *out + s;
}

static long long rb_blocks(long long n, int max_blocks) {
    const long long tiles = (n + RB_TILE - 1) / RB_TILE, cap = max_blocks > 0 ? max_blocks : RB_DEFAULT_BLOCKS;
    return tiles < cap ? tiles : cap;
}

}  // namespace mr
using namespace mr;

extern "C" long long mirres_radiance_bwd_workspace_bytes(long long n, int max_blocks) {
    if (n < 0 || n > (1LL << 38) || max_blocks < 0) { set_error("mirres_radiance_bwd_workspace_bytes: bad argument (n %lld, max_blocks %d)", n, max_blocks); return MIRRES_E_ARG; }
    return rb_blocks(n, max_blocks) * (long long)(RB_PARTIAL * sizeof(float));
}

extern "C" int mirres_radiance_points_bwd(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, const float* grad_sigma,
                                          const float* grad_rgb, float* grad_table, float* grad_w0, float* grad_w1, float* grad_c0, float* grad_c1, float* grad_c2,
                                          void* workspace, long long workspace_bytes, int max_blocks, void* stream) {
    if (!net) { set_error("mirres_radiance_points_bwd: net is NULL"); return MIRRES_E_ARG; }
    if (!dn_net_ok(&net->grid, "mirres_radiance_points_bwd")) return MIRRES_E_ARG;
    if (!net->w1 || !net->c0 || !net->c1 || !net->c2) { set_error("mirres_radiance_points_bwd: net has a NULL w1 / c0 / c1 / c2"); return MIRRES_E_ARG; }
    if (n < 0 || n > (1LL << 38) || max_blocks < 0 || (n > 0 && (!pos || !dirs || !grad_rgb)) || !(bound > 0.f) || !(bound < 3.0e38f)) {
        set_error("mirres_radiance_points_bwd: bad argument (n %lld, max_blocks %d, bound %g, pos / dirs / grad_rgb %s)", n, max_blocks, (double)bound,
                  (pos && dirs && grad_rgb) ? "given" : "NULL");
        return MIRRES_E_ARG;
    }
    if (n == 0) return MIRRES_OK;
    if (!grad_table || !grad_w0 || !grad_w1 || !grad_c0 || !grad_c1 || !grad_c2) {
        set_error("mirres_radiance_points_bwd: a gradient output is NULL (grad_table / grad_w0 / grad_w1 / grad_c0 / grad_c1 / grad_c2)"); return MIRRES_E_ARG;
    }
    const long long blocks = rb_blocks(n, max_blocks), need = blocks * (long long)(RB_PARTIAL * sizeof(float));
    if (!workspace || workspace_bytes < need) {
        set_error("mirres_radiance_points_bwd: workspace of %lld bytes, %lld are needed (mirres_radiance_bwd_workspace_bytes)", workspace ? workspace_bytes : 0LL, need);
        return MIRRES_E_ARG;
    }
    k_radiance_points_bwd<<<(int)blocks, DN_BLOCK, 0, (hipStream_t)stream>>>(*net, pos, dirs, n, bound, grad_sigma, grad_rgb, grad_table, (float*)workspace);
    MR_LAUNCH_CHECK("radiance_points_bwd");
    const RbGrads G = {grad_table, grad_w0, grad_w1, grad_c0, grad_c1, grad_c2};
    k_radiance_bwd_reduce<<<grid_for(RB_PARTIAL, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>((const float*)workspace, (int)blocks, G);
    MR_LAUNCH_CHECK("radiance_bwd_reduce");
    return MIRRES_OK;
}
