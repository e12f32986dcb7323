// device_uvcover.hpp — the exact UV coverage rule shared by the texture bake (bake.hip: mirres_uv_rasterize) and the chart atlas' overlap check
// (atlas.hip: mirres_atlas_verify): vertices snapped to 1/256 texel, int64 edge functions at the texel centres, top-left fill rule; and the balanced
// (triangle, 32-texel chunk) work items both walk (per-triangle set-up, the u64 exclusive scan of the chunk counts, the item -> triangle search).
// The kernels are `static`: each translation unit that includes this header gets its own copies (-fno-gpu-rdc).
#pragma once
#include "engine.hpp"
#include "device_math.hpp"
#include "device_scan.hpp"

namespace mr {

#define BK_BLOCK 256
#define BK_CHUNK 32          // bounding-box texels per work item of the UV rasteriser
#define BK_FIX 256           // sub-texel steps of the snapped vertex coordinates
#define BK_FIX_MAX (1 << 28) // |snapped coordinate| bound: edge-function products stay below 2^59

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

static __global__ void __launch_bounds__(BK_BLOCK) k_uv_setup(const float* __restrict__ uv, int n_uv, const int32_t* __restrict__ ft, int T, int W, int H,
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
static __global__ void __launch_bounds__(BK_BLOCK) k_scan_local(unsigned long long* __restrict__ a, int n, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[BK_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * BK_SCAN + 4 * threadIdx.x;
    unsigned long long v[4], s = 0;
    for (int k = 0; k < 4; k++) { v[k] = base + k < (size_t)n ? a[base + k] : 0ULL; s += v[k]; }
    unsigned long long total;
    unsigned long long run = block_excl_scan<BK_BLOCK>(s, sh, total);
    for (int k = 0; k < 4; k++) { if (base + k < (size_t)n) a[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
static __global__ void __launch_bounds__(BK_BLOCK) k_scan_sums(unsigned long long* __restrict__ sums, int nb, unsigned long long* __restrict__ total_out) {
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
static __global__ void __launch_bounds__(BK_BLOCK) k_scan_add(unsigned long long* __restrict__ a, int n, const unsigned long long* __restrict__ sums) {
    const size_t i = (size_t)blockIdx.x * BK_BLOCK + threadIdx.x;
    if (i < (size_t)n) a[i] += sums[i / BK_SCAN];
}

// the triangle of work item k: the last one whose first item is <= k (upper_bound(first[0..T), k) - 1; first[0] = 0 <= k)
MR_DEV int uv_item_triangle(const unsigned long long* __restrict__ first, int T, unsigned long long k) {
    int lo = 0, hi = T;
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static int scan_blocks(int T) { return (T + BK_SCAN - 1) / BK_SCAN; }
// scratch of the work-item set-up for T triangles: UvTri[T], first u64[T + 1], block sums u64[scan_blocks + 1]
static size_t uv_items_bytes(int T) { return align256(sizeof(UvTri) * (size_t)T) + align256(8 * ((size_t)T + 1)) + align256(8 * (size_t)(scan_blocks(T) + 1)); }
// tris / first (first[T] = the item total) of the T > 0 triangles of (uv, ft) on a W x H grid, enqueued on s
static void uv_items_enqueue(const float* uv, int n_uv, const int32_t* ft, int T, int W, int H, void* scratch, UvTri*& tris, unsigned long long*& first, hipStream_t s) {
    tris = reinterpret_cast<UvTri*>(scratch);
    first = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(scratch) + align256(sizeof(UvTri) * (size_t)T));
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(first) + align256(8 * ((size_t)T + 1)));
    const int nb = scan_blocks(T);
    k_uv_setup<<<grid_for(T, BK_BLOCK), BK_BLOCK, 0, s>>>(uv, n_uv, ft, T, W, H, tris, first);
    k_scan_local<<<nb, BK_BLOCK, 0, s>>>(first, T, sums);
    k_scan_sums<<<1, BK_BLOCK, 0, s>>>(sums, nb, first + T);
    k_scan_add<<<grid_for(T, BK_BLOCK), BK_BLOCK, 0, s>>>(first, T, sums);
}

}  // namespace mr
