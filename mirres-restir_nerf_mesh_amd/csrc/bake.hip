// bake.hip — the texture bake of the stage-1 mesh export (nerf/renderer.py:319-462, `_export_obj`): what the reference gets from nvdiffrast in UV
// space (dr.rasterize on uv * 2 - 1, :357), numpy (sRGB quantisation, :395-398), sklearn's kd-tree over scipy's dilation / erosion (gutter inpaint,
// :400-414) and cv2.resize (SSAA downsample, :420-422).  Four entry points, every one deterministic (DESIGN.md §5 "Texture bake"):
//   mirres_uv_rasterize        exact integer coverage (vertices snapped to 1/256 texel, int64 edge functions, top-left fill rule, lowest triangle
//                              index wins) over balanced (triangle, 32-texel chunk) work items;
//   mirres_bake_quantise       clip, linear -> sRGB, x 255, truncate, into two interleaved RGB8 planes;
//   mirres_texture_inpaint     every gutter texel within L1 distance `radius` of the covered set copies its Euclidean-nearest covered texel: a column
//                              pass and a row pass over LDS tiles, exact inside the (2 radius + 1)^2 window;
//   mirres_texture_downsample  cv2's INTER_LINEAR at an integer factor.
#include "device_uvcover.hpp"

namespace mr {

#define BK_NONE 0x7F7F7F7F   // "no triangle" in the id channel (the byte pattern of the clearing memset); > any id < 2^24
#define BK_R 32              // inpaint window half-width the LDS tiles are sized for
#define BK_NODY 127          // column pass: no covered texel within the radius

// one work item = up to 32 consecutive texels (row-major) of one triangle's box: the triangle is the last one whose first item is <= the item
__global__ void __launch_bounds__(BK_BLOCK) k_uv_cover(const UvTri* __restrict__ tris, const unsigned long long* __restrict__ first, int T, int W,
                                                       int32_t* __restrict__ rast_id) {
    const unsigned long long total = first[T];
    const unsigned long long stride = (unsigned long long)gridDim.x * BK_BLOCK;
    for (unsigned long long k = (unsigned long long)blockIdx.x * BK_BLOCK + threadIdx.x; k < total; k += stride) {
        const int t = uv_item_triangle(first, T, k);
        const UvTri r = tris[t];
        const long long i0 = (long long)(k - first[t]) * BK_CHUNK, n = (long long)r.bw * r.bh;
        for (int j = 0; j < BK_CHUNK; j++) {
            const long long i = i0 + j;
            if (i >= n) break;
            const int c = r.c0 + (int)(i % r.bw), row = r.r0 + (int)(i / r.bw);
            long long w0, w1, w2;
            if (inside(r, (long long)c * BK_FIX + BK_FIX / 2, (long long)row * BK_FIX + BK_FIX / 2, w0, w1, w2))
                atomicMin(&rast_id[4 * ((size_t)row * W + c) + 3], t);
        }
    }
}

// the winner's barycentrics (weights of the ORIGINAL v0, v1, nvdiffrast's (u, v)) from its exact edge functions, triangle id + 1
__global__ void __launch_bounds__(BK_BLOCK) k_uv_resolve(const UvTri* __restrict__ tris, int W, int H, float* __restrict__ rast) {
    const size_t p = (size_t)blockIdx.x * BK_BLOCK + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int32_t id = reinterpret_cast<const int32_t*>(rast)[4 * p + 3];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (id != BK_NONE) {
        const UvTri r = tris[id];
        const int c = (int)(p % W), row = (int)(p / W);
        long long w0, w1, w2;
        inside(r, (long long)c * BK_FIX + BK_FIX / 2, (long long)row * BK_FIX + BK_FIX / 2, w0, w1, w2);
        const double A = (double)(w0 + w1 + w2);
        o.x = (float)((double)w0 / A);
        o.y = (float)((double)((r.flags & 1) ? w2 : w1) / A);
        o.w = (float)(id + 1);
    }
    reinterpret_cast<float4*>(rast)[p] = o;
}

// linear_to_srgb_np (nerf/utils.py:60) on clip(x, 0, 1), x 255, truncated (renderer.py:395-398); fp32 throughout, powf of the device library
MR_DEV uint8_t quant(float x) {
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float s = x < 0.0031308f ? 12.92f * x : 1.055f * powf(x, 0.41666f) - 0.055f;
    const int q = (int)(s * 255.f);
    return (uint8_t)min(max(q, 0), 255);
}
__global__ void __launch_bounds__(BK_BLOCK) k_quantise(const float* __restrict__ f6, const int32_t* __restrict__ index, int n, int WH,
                                                       uint8_t* __restrict__ out0, uint8_t* __restrict__ out1) {
    const int i = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int p = index[i];
    if (p < 0 || p >= WH) return;
    const float* f = f6 + 6 * (size_t)i;
    for (int c = 0; c < 3; c++) { out0[3 * (size_t)p + c] = quant(f[c]); out1[3 * (size_t)p + c] = quant(f[3 + c]); }
}

// column pass: per texel the signed row offset of the nearest covered texel in its own column within +-R (the upper one on a tie), or BK_NODY.
// Tile: 64 columns x 64 rows, the mask of rows [r0 - 32, r0 + 96) in LDS.
#define CP_W 64
#define CP_H 64
__global__ void __launch_bounds__(BK_BLOCK) k_inpaint_cols(int W, int H, int R, const uint8_t* __restrict__ mask, int8_t* __restrict__ dy_out) {
    __shared__ uint8_t m[CP_H + 2 * BK_R][CP_W];
    const int c0 = blockIdx.x * CP_W, r0 = blockIdx.y * CP_H;
    for (int i = threadIdx.x; i < (CP_H + 2 * BK_R) * CP_W; i += BK_BLOCK) {
        const int lr = i / CP_W, lc = i % CP_W, r = r0 - BK_R + lr, c = c0 + lc;
        m[lr][lc] = (r >= 0 && r < H && c < W) ? (mask[(size_t)r * W + c] != 0) : 0;
    }
    __syncthreads();
    const int lc = threadIdx.x % CP_W, c = c0 + lc;
    if (c >= W) return;
    for (int lr = threadIdx.x / CP_W; lr < CP_H; lr += BK_BLOCK / CP_W) {
        const int r = r0 + lr;
        if (r >= H) break;
        int best = BK_NODY;
        for (int d = 0; d <= R; d++) {
            if (m[lr + BK_R - d][lc]) { best = -d; break; }
            if (m[lr + BK_R + d][lc]) { best = d; break; }
        }
        dy_out[(size_t)r * W + c] = (int8_t)best;
    }
}

// row pass: minimise (dx^2 + dy(x+dx)^2, row, col) over |dx| <= R; the region is min(|dx| + |dy(x+dx)|) <= R (scipy's cross dilation, `radius`
// iterations).  Covered texels keep their bytes, region texels copy the winner's, the rest is 0.  Tile: 64 columns x 16 rows, dy of columns
// [c0 - 32, c0 + 96) in LDS.
#define RP_W 64
#define RP_H 16
__global__ void __launch_bounds__(BK_BLOCK) k_inpaint_rows(int W, int H, int R, const int8_t* __restrict__ dy_in, const uint8_t* __restrict__ in0,
                                                           const uint8_t* __restrict__ in1, uint8_t* __restrict__ out0, uint8_t* __restrict__ out1) {
    __shared__ int8_t s[RP_H][RP_W + 2 * BK_R];
    const int c0 = blockIdx.x * RP_W, r0 = blockIdx.y * RP_H;
    for (int i = threadIdx.x; i < RP_H * (RP_W + 2 * BK_R); i += BK_BLOCK) {
        const int lr = i / (RP_W + 2 * BK_R), lc = i % (RP_W + 2 * BK_R), r = r0 + lr, c = c0 - BK_R + lc;
        s[lr][lc] = (r < H && c >= 0 && c < W) ? dy_in[(size_t)r * W + c] : (int8_t)BK_NODY;
    }
    __syncthreads();
    const int lc = threadIdx.x % RP_W, c = c0 + lc;
    if (c >= W) return;
    for (int lr = threadIdx.x / RP_W; lr < RP_H; lr += BK_BLOCK / RP_W) {
        const int r = r0 + lr;
        if (r >= H) break;
        const size_t p = (size_t)r * W + c;
        size_t src = p;
        bool keep = s[lr][lc + BK_R] == 0;
        if (!keep) {
            int bd2 = 1 << 30, brow = 0, bcol = 0, bl1 = 1 << 30;
            for (int d = 0; d <= R; d++) {
                if (d * d > bd2 && (bl1 <= R || d > bl1)) break;     // no later column can improve the winner, nor the region test
                for (int side = 0; side < (d ? 2 : 1); side++) {
                    const int dx = side ? d : -d;
                    const int dy = s[lr][lc + BK_R + dx];
                    if (dy == BK_NODY) continue;
                    const int d2 = dx * dx + dy * dy, l1 = d + (dy < 0 ? -dy : dy), row = r + dy, col = c + dx;
                    bl1 = min(bl1, l1);
                    if (d2 < bd2 || (d2 == bd2 && (row < brow || (row == brow && col < bcol)))) { bd2 = d2; brow = row; bcol = col; }
                }
            }
            if (bl1 <= R) { keep = true; src = (size_t)brow * W + bcol; }
        }
        for (int k = 0; k < 3; k++) {
            out0[3 * p + k] = keep ? in0[3 * src + k] : (uint8_t)0;
            out1[3 * p + k] = keep ? in1[3 * src + k] : (uint8_t)0;
        }
    }
}

// cv2.resize(INTER_LINEAR) by an integer factor s: source taps at (d + 0.5) s - 0.5 per axis — one texel for odd s, the mean of the two middle ones for
// even s, rounded half up ((a + b + c + d + 2) >> 2, cv2's fixed-point rounding of the 0.5 / 0.5 weights and its INTER_AREA path at s = 2)
__global__ void __launch_bounds__(BK_BLOCK) k_downsample(int W, int H, int s, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const int w0 = W / s, h0 = H / s;
    const size_t i = (size_t)blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i >= (size_t)w0 * h0 * 3) return;
    const int ch = (int)(i % 3), x = (int)((i / 3) % w0), y = (int)(i / 3 / w0);
    const int xa = x * s + (s - 1) / 2, ya = y * s + (s - 1) / 2;
    if (s & 1) { out[i] = in[3 * ((size_t)ya * W + xa) + ch]; return; }
    const int a = in[3 * ((size_t)ya * W + xa) + ch], b = in[3 * ((size_t)ya * W + xa + 1) + ch];
    const int c = in[3 * ((size_t)(ya + 1) * W + xa) + ch], d = in[3 * ((size_t)(ya + 1) * W + xa + 1) + ch];
    out[i] = (uint8_t)((a + b + c + d + 2) >> 2);
}

}  // namespace mr

using namespace mr;

extern "C" long long mirres_uv_rasterize_scratch(int T) {
    if (T < 0 || T >= (1 << 24)) return -1;
    return (long long)uv_items_bytes(T);
}

extern "C" int mirres_uv_rasterize(const float* uv, int n_uv, const int32_t* ft, int T, int W, int H, float* rast, void* scratch, long long scratch_bytes, void* stream) {
    if (T < 0 || n_uv < 0 || W <= 0 || H <= 0 || W > 65536 || H > 65536 || (long long)W * H >= (1LL << 31) || !rast) {
        set_error("mirres_uv_rasterize: bad argument (T %d, n_uv %d, %d x %d)", T, n_uv, W, H); return MIRRES_E_ARG;
    }
    if (T >= (1 << 24)) { set_error("mirres_uv_rasterize: %d triangles: the id is stored in fp32 (exact below 2^24)", T); return MIRRES_E_ARG; }
    if (T > 0 && (!uv || !ft || n_uv == 0 || !scratch || scratch_bytes < mirres_uv_rasterize_scratch(T))) {
        set_error("mirres_uv_rasterize: missing input or scratch (%lld bytes given, %lld needed)", scratch_bytes, mirres_uv_rasterize_scratch(T)); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)W * H;
    MR_HIP(hipMemsetAsync(rast, 0x7F, n * 16, s));                       // id channel = BK_NONE everywhere
    if (T > 0) {
        UvTri* tris; unsigned long long* first;
        uv_items_enqueue(uv, n_uv, ft, T, W, H, scratch, tris, first, s);
        k_uv_cover<<<2048, BK_BLOCK, 0, s>>>(tris, first, T, W, reinterpret_cast<int32_t*>(rast));
        k_uv_resolve<<<grid_for(n, BK_BLOCK), BK_BLOCK, 0, s>>>(tris, W, H, rast);
    } else {
        MR_HIP(hipMemsetAsync(rast, 0, n * 16, s));
    }
    MR_LAUNCH_CHECK("uv_rasterize");
    return MIRRES_OK;
}

extern "C" int mirres_bake_quantise(const float* feats6, const int32_t* index, int n, int W, int H, uint8_t* out0, uint8_t* out1, void* stream) {
    if (n < 0 || W <= 0 || H <= 0 || (long long)W * H >= (1LL << 31) || !out0 || !out1 || (n > 0 && (!feats6 || !index))) {
        set_error("mirres_bake_quantise: bad argument"); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MR_HIP(hipMemsetAsync(out0, 0, (size_t)W * H * 3, s));
    MR_HIP(hipMemsetAsync(out1, 0, (size_t)W * H * 3, s));
    if (n > 0) k_quantise<<<grid_for(n, BK_BLOCK), BK_BLOCK, 0, s>>>(feats6, index, n, W * H, out0, out1);
    MR_LAUNCH_CHECK("bake_quantise");
    return MIRRES_OK;
}

extern "C" int mirres_texture_inpaint(int W, int H, int radius, const uint8_t* mask, const uint8_t* in0, const uint8_t* in1, int8_t* scratch_dy,
                                      uint8_t* out0, uint8_t* out1, void* stream) {
    if (W <= 0 || H <= 0 || (long long)W * H >= (1LL << 31) || radius < 0 || radius > BK_R || !mask || !in0 || !in1 || !scratch_dy || !out0 || !out1) {
        set_error("mirres_texture_inpaint: bad argument (radius %d, at most %d)", radius, BK_R); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    k_inpaint_cols<<<dim3((W + CP_W - 1) / CP_W, (H + CP_H - 1) / CP_H), BK_BLOCK, 0, s>>>(W, H, radius, mask, scratch_dy);
    k_inpaint_rows<<<dim3((W + RP_W - 1) / RP_W, (H + RP_H - 1) / RP_H), BK_BLOCK, 0, s>>>(W, H, radius, scratch_dy, in0, in1, out0, out1);
    MR_LAUNCH_CHECK("texture_inpaint");
    return MIRRES_OK;
}

extern "C" int mirres_texture_downsample(int W, int H, int ssaa, const uint8_t* in, uint8_t* out, void* stream) {
    if (W <= 0 || H <= 0 || (long long)W * H >= (1LL << 31) || ssaa < 1 || W % ssaa || H % ssaa || !in || !out) {
        set_error("mirres_texture_downsample: bad argument (%d x %d, ssaa %d)", W, H, ssaa); return MIRRES_E_ARG;
    }
    k_downsample<<<grid_for((size_t)(W / ssaa) * (H / ssaa) * 3, BK_BLOCK), BK_BLOCK, 0, (hipStream_t)stream>>>(W, H, ssaa, in, out);
    MR_LAUNCH_CHECK("texture_downsample");
    return MIRRES_OK;
}
