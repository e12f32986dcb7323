// bake.hip — the texture bake of the stage-1 mesh export (nerf/renderer.py:319-462, `_export_obj`): what the reference gets from nvdiffrast in UV
// space (dr.rasterize on uv * 2 - 1, :357), numpy (sRGB quantisation, :395-398), sklearn's kd-tree over scipy's dilation / erosion (gutter inpaint,
// :400-414) and cv2.resize (SSAA downsample, :420-422).  Four entry points, every one deterministic (DESIGN.md §5 "Texture bake"):
//   mirres_uv_rasterize        exact integer coverage (vertices snapped to 1/256 texel, int64 edge functions, top-left fill rule, lowest triangle
//                              index wins) over balanced (triangle, 32-texel chunk) work items;
//   mirres_bake_quantise       clip, linear -> sRGB, x 255, truncate, into two interleaved RGB8 planes;
//   mirres_texture_inpaint     every gutter texel within L1 distance `radius` of the covered set copies its Euclidean-nearest covered texel: a column
//                              pass and a row pass over LDS tiles, exact inside the (2 radius + 1)^2 window;
//   mirres_texture_downsample  cv2's INTER_LINEAR at an integer factor.
#include "engine.hpp"
#include "device_math.hpp"
#include "device_scan.hpp"

namespace mr {

#define BK_BLOCK 256
#define BK_CHUNK 32          // bounding-box texels per work item of the UV rasteriser
#define BK_FIX 256           // sub-texel steps of the snapped vertex coordinates
#define BK_FIX_MAX (1 << 28) // |snapped coordinate| bound: edge-function products stay below 2^59
#define BK_NONE 0x7F7F7F7F   // "no triangle" in the id channel (the byte pattern of the clearing memset); > any id < 2^24
#define BK_R 32              // inpaint window half-width the LDS tiles are sized for
#define BK_NODY 127          // column pass: no covered texel within the radius

// per triangle: snapped vertices oriented counter-clockwise (v1 and v2 swapped when the UV triangle is clockwise), flags, texel bounding box
struct UvTri {
    int32_t x[3], y[3];
    int32_t flags;           // bit 0: v1 / v2 swapped; bit 1: covers nothing (zero area, non-finite or out-of-range vertex)
    int32_t c0, r0, bw, bh;  // first texel column / row of the box and its size (bw * bh == 0 when empty)
    int32_t pad;
};

MR_DEV long long floordiv(long long a, long long b) { long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
MR_DEV int32_t snap(float u, int n) {
    // u * n * 256 is exact in double (24-bit significand times an integer <= 2^24), and so is + 0.5: round half up, reproducible on any host
    double x = floor((double)u * (double)n * (double)BK_FIX + 0.5);
    x = fmin(fmax(x, -(double)BK_FIX_MAX), (double)BK_FIX_MAX);
    return (int32_t)x;
}
// edge function of the directed edge a -> b at p: > 0 on its left (counter-clockwise interior)
MR_DEV long long edgef(long long ax, long long ay, long long bx, long long by, long long px, long long py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
// top-left rule on a counter-clockwise triangle: a centre on edge a -> b belongs to it when the edge goes up, or is horizontal and goes left.
// Two triangles on either side of an edge see it in opposite directions, so exactly one of them takes the centres on it.
MR_DEV bool owns(long long ax, long long ay, long long bx, long long by) { const long long dy = by - ay, dx = bx - ax; return dy > 0 || (dy == 0 && dx < 0); }
MR_DEV bool inside(const UvTri& t, long long px, long long py, long long& w0, long long& w1, long long& w2) {
    w0 = edgef(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
    w1 = edgef(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
    w2 = edgef(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
    const bool i0 = w0 > 0 || (w0 == 0 && owns(t.x[1], t.y[1], t.x[2], t.y[2]));
    const bool i1 = w1 > 0 || (w1 == 0 && owns(t.x[2], t.y[2], t.x[0], t.y[0]));
    const bool i2 = w2 > 0 || (w2 == 0 && owns(t.x[0], t.y[0], t.x[1], t.y[1]));
    return i0 && i1 && i2;
}

__global__ void __launch_bounds__(BK_BLOCK) k_uv_setup(const float* __restrict__ uv, int n_uv, const int32_t* __restrict__ ft, int T, int W, int H,
                                                       UvTri* __restrict__ tris, unsigned long long* __restrict__ chunks) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    UvTri r;
    r.flags = 0;
    for (int k = 0; k < 3; k++) {
        const int j = ft[3 * (size_t)t + k];
        float u = 0.f, v = 0.f;
        if (j < 0 || j >= n_uv) r.flags |= 2;
        else { u = uv[2 * (size_t)j]; v = uv[2 * (size_t)j + 1]; }
        if (!isfinite(u) || !isfinite(v)) { r.flags |= 2; u = 0.f; v = 0.f; }
        r.x[k] = snap(u, W); r.y[k] = snap(v, H);
    }
    const long long area = edgef(r.x[0], r.y[0], r.x[1], r.y[1], r.x[2], r.y[2]);
    if (area == 0) r.flags |= 2;
    if (area < 0) { int32_t a = r.x[1]; r.x[1] = r.x[2]; r.x[2] = a; a = r.y[1]; r.y[1] = r.y[2]; r.y[2] = a; r.flags |= 1; }
    // texel c's centre is at c * 256 + 128: the box holds the centres inside [min, max] of the snapped coordinates, clamped to the grid
    const long long xmin = min(r.x[0], min(r.x[1], r.x[2])), xmax = max(r.x[0], max(r.x[1], r.x[2]));
    const long long ymin = min(r.y[0], min(r.y[1], r.y[2])), ymax = max(r.y[0], max(r.y[1], r.y[2]));
    long long c0 = -floordiv(-(xmin - BK_FIX / 2), BK_FIX), c1 = floordiv(xmax - BK_FIX / 2, BK_FIX);
    long long r0 = -floordiv(-(ymin - BK_FIX / 2), BK_FIX), r1 = floordiv(ymax - BK_FIX / 2, BK_FIX);
    c0 = max(c0, 0LL); r0 = max(r0, 0LL); c1 = min(c1, (long long)W - 1); r1 = min(r1, (long long)H - 1);
    r.c0 = (int32_t)c0; r.r0 = (int32_t)r0;
    r.bw = (c1 >= c0 && !(r.flags & 2)) ? (int32_t)(c1 - c0 + 1) : 0;
    r.bh = (r1 >= r0 && r.bw > 0) ? (int32_t)(r1 - r0 + 1) : 0;
    if (r.bh == 0) r.bw = 0;
    r.pad = 0;
    tris[t] = r;
    chunks[t] = ((unsigned long long)r.bw * (unsigned long long)r.bh + BK_CHUNK - 1) / BK_CHUNK;
}

// exclusive scan of n u64 counts, in place, + the total in a[n]: 1024 per workgroup, the workgroup sums scanned by one workgroup, then added
// (inside a workgroup: block_excl_scan, device_scan.hpp)
#define BK_SCAN 1024
__global__ void __launch_bounds__(BK_BLOCK) k_scan_local(unsigned long long* __restrict__ a, int n, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[BK_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * BK_SCAN + 4 * threadIdx.x;
    unsigned long long v[4], s = 0;
    for (int k = 0; k < 4; k++) { v[k] = base + k < (size_t)n ? a[base + k] : 0ULL; s += v[k]; }
    unsigned long long total;
    unsigned long long run = block_excl_scan<BK_BLOCK>(s, sh, total);
    for (int k = 0; k < 4; k++) { if (base + k < (size_t)n) a[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(BK_BLOCK) k_scan_sums(unsigned long long* __restrict__ sums, int nb, unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long sh[BK_BLOCK / 64];
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += BK_BLOCK) {               // nb <= 2^14: at most 64 rounds
        const int i = b0 + threadIdx.x;
        const unsigned long long v = i < nb ? sums[i] : 0ULL;
        unsigned long long total;
        const unsigned long long ex = block_excl_scan<BK_BLOCK>(v, sh, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}
__global__ void __launch_bounds__(BK_BLOCK) k_scan_add(unsigned long long* __restrict__ a, int n, const unsigned long long* __restrict__ sums) {
    const size_t i = (size_t)blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i < (size_t)n) a[i] += sums[i / BK_SCAN];
}

// one work item = up to 32 consecutive texels (row-major) of one triangle's box: the triangle is the last one whose first item is <= the item
__global__ void __launch_bounds__(BK_BLOCK) k_uv_cover(const UvTri* __restrict__ tris, const unsigned long long* __restrict__ first, int T, int W,
                                                       int32_t* __restrict__ rast_id) {
    const unsigned long long total = first[T];
    const unsigned long long stride = (unsigned long long)gridDim.x * BK_BLOCK;
    for (unsigned long long k = (unsigned long long)blockIdx.x * BK_BLOCK + threadIdx.x; k < total; k += stride) {
        int lo = 0, hi = T;                                       // upper_bound(first[0..T), k) - 1; first[0] = 0 <= k
        for (int it = 0; it < 32 && hi - lo > 1; it++) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= k) lo = mid; else hi = mid;
        }
        const int t = lo;
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

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static int scan_blocks(int T) { return (T + BK_SCAN - 1) / BK_SCAN; }

}  // namespace mr

using namespace mr;

extern "C" long long mirres_uv_rasterize_scratch(int T) {
    if (T < 0 || T >= (1 << 24)) return -1;
    return (long long)(align256(sizeof(UvTri) * (size_t)T) + align256(8 * ((size_t)T + 1)) + align256(8 * (size_t)(scan_blocks(T) + 1)));
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
        UvTri* tris = reinterpret_cast<UvTri*>(scratch);
        unsigned long long* first = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(scratch) + align256(sizeof(UvTri) * (size_t)T));
        unsigned long long* sums = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(first) + align256(8 * ((size_t)T + 1)));
        const int nb = scan_blocks(T);
        k_uv_setup<<<grid_for(T, BK_BLOCK), BK_BLOCK, 0, s>>>(uv, n_uv, ft, T, W, H, tris, first);
        k_scan_local<<<nb, BK_BLOCK, 0, s>>>(first, T, sums);
        k_scan_sums<<<1, BK_BLOCK, 0, s>>>(sums, nb, first + T);
        k_scan_add<<<grid_for(T, BK_BLOCK), BK_BLOCK, 0, s>>>(first, T, sums);
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
