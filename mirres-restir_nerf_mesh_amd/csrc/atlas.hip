// atlas.hip — the per-face, per-UV-vertex and per-texel work of the chart atlas of the stage-1 mesh export (export.chart_atlas; DESIGN.md §5.7 "Chart atlas"): where the
// reference calls xatlas (nerf/renderer.py:334-347), charts here are connected sets of faces that look along one coordinate axis, projected along it.
//   mirres_atlas_classify   face normal and bucket (the axis direction +x, -x, +y, -y, +z, -z the face looks along most), -1 for a degenerate face;
//   mirres_atlas_smooth     one Jacobi round of relabelling: a face takes the bucket most of its manifold neighbours and itself vote for;
//   mirres_atlas_bounds     per chart the min / max of its faces' projected coordinates (integer-mapped float atomicMin / atomicMax: order-free);
//   mirres_atlas_emit       the UV of every (chart, mesh vertex) pair from the chart's bounds, its rectangle's origin and the shared density;
//   mirres_atlas_verify     marks the bake-grid texel centres every triangle covers (the coverage rule of mirres_uv_rasterize, device_uvcover.hpp) and
//                           flags the charts that cover a centre another triangle covers too.
// Nothing here adds floating-point numbers atomically: equal inputs give equal bytes.  The sorts and uniques between the calls are the caller's.
#include "device_uvcover.hpp"

namespace mr {

#define AT_BLOCK 256

// bucket k = 2 axis + (negative direction); (U, V) of a bucket are the two other coordinates in the order that makes (U, V, d_k) right-handed
__device__ static const int8_t AT_U[6] = {1, 2, 2, 0, 0, 1};
__device__ static const int8_t AT_V[6] = {2, 1, 0, 2, 1, 0};

MR_DEV bool at_face_ok(const int32_t* __restrict__ tris, int f, int V, int& a, int& b, int& c) {
    a = tris[3 * (size_t)f]; b = tris[3 * (size_t)f + 1]; c = tris[3 * (size_t)f + 2];
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V && a != b && b != c && a != c;
}

__global__ void __launch_bounds__(AT_BLOCK) k_atlas_classify(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris, int T,
                                                             float* __restrict__ normal, int32_t* __restrict__ bucket) {
    const int f = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (f >= T) return;
    int ia, ib, ic;
    float n[3] = {0.f, 0.f, 0.f};
    int best = -1;
    if (at_face_ok(tris, f, V, ia, ib, ic)) {
        float p[3][3];
        bool finite = true;
        for (int k = 0; k < 3; k++) {
            p[0][k] = verts[3 * (size_t)ia + k]; p[1][k] = verts[3 * (size_t)ib + k]; p[2][k] = verts[3 * (size_t)ic + k];
            finite = finite && isfinite(p[0][k]) && isfinite(p[1][k]) && isfinite(p[2][k]);
        }
        const float e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const float e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        n[0] = e1y * e2z - e1z * e2y;                       // every product and difference rounded once (-ffp-contract=off)
        n[1] = e1z * e2x - e1x * e2z;
        n[2] = e1x * e2y - e1y * e2x;
        finite = finite && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
        if (finite && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f)) {
            float bv = 0.f;
            for (int k = 0; k < 6; k++) {                   // strictly larger: ties go to the lowest k
                const float val = (k & 1) ? -n[k >> 1] : n[k >> 1];
                if (val > bv) { bv = val; best = k; }
            }
        } else { n[0] = n[1] = n[2] = 0.f; }
    }
    normal[3 * (size_t)f] = n[0]; normal[3 * (size_t)f + 1] = n[1]; normal[3 * (size_t)f + 2] = n[2];
    bucket[f] = best;
}

__global__ void __launch_bounds__(AT_BLOCK) k_atlas_smooth(const float* __restrict__ normal, const int32_t* __restrict__ bucket_in, const int32_t* __restrict__ nbr,
                                                           int T, double cos2, int32_t* __restrict__ bucket_out) {
    const int f = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (f >= T) return;
    const int own = bucket_in[f];
    if (own < 0 || own >= 6) { bucket_out[f] = -1; return; }
    const double nx = normal[3 * (size_t)f], ny = normal[3 * (size_t)f + 1], nz = normal[3 * (size_t)f + 2];
    const double thr = cos2 * ((nx * nx + ny * ny) + nz * nz);        // fp64: the squares are exact, each sum and the product rounded once
    unsigned elig = 0;
    for (int k = 0; k < 6; k++) {
        const double c = k < 2 ? nx : (k < 4 ? ny : nz), val = (k & 1) ? -c : c;
        if (val > 0.0 && val * val >= thr) elig |= 1u << k;
    }
    // votes in half units, one byte per bucket: the own bucket 3 (one vote and a half), a manifold neighbour's 2
    unsigned long long votes = 0;
    if (elig >> own & 1) votes += 3ULL << (8 * own);
    for (int e = 0; e < 3; e++) {
        const int g = nbr[3 * (size_t)f + e];
        if (g < 0 || g >= T) continue;
        const int b = bucket_in[g];
        if (b >= 0 && b < 6 && (elig >> b & 1)) votes += 2ULL << (8 * b);
    }
    int best = -1; unsigned bv = 0;
    for (int k = 0; k < 6; k++) {
        const unsigned v = (unsigned)(votes >> (8 * k)) & 255u;
        if (v > bv) { bv = v; best = k; }
    }
    const unsigned vown = (unsigned)(votes >> (8 * own)) & 255u;
    bucket_out[f] = (best < 0 || vown == bv) ? own : best;
}

// order-preserving map of float bits to u32 (negative floats reversed below the positive ones; -0 < +0) and back
MR_DEV uint32_t at_enc(float x) { const uint32_t b = __float_as_uint(x); return (b >> 31) ? ~b : (b | 0x80000000u); }
MR_DEV float at_dec(uint32_t e) { return __uint_as_float((e >> 31) ? (e & 0x7FFFFFFFu) : ~e); }

__global__ void __launch_bounds__(AT_BLOCK) k_atlas_bounds_init(uint32_t* __restrict__ enc, int n_charts) {
    const int c = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (c >= n_charts) return;
    enc[4 * (size_t)c] = enc[4 * (size_t)c + 1] = 0xFFFFFFFFu; enc[4 * (size_t)c + 2] = enc[4 * (size_t)c + 3] = 0u;
}
__global__ void __launch_bounds__(AT_BLOCK) k_atlas_bounds(const float* __restrict__ verts, int V, const int32_t* __restrict__ tris, int T,
                                                           const int32_t* __restrict__ bucket, const int32_t* __restrict__ chart, int n_charts,
                                                           uint32_t* __restrict__ enc) {
    const int f = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (f >= T) return;
    const int c = chart[f], b = bucket[f];
    int idx[3];
    if (c < 0 || c >= n_charts || b < 0 || b >= 6 || !at_face_ok(tris, f, V, idx[0], idx[1], idx[2])) return;
    const int au = AT_U[b], av = AT_V[b];
    for (int k = 0; k < 3; k++) {
        const uint32_t u = at_enc(verts[3 * (size_t)idx[k] + au]), v = at_enc(verts[3 * (size_t)idx[k] + av]);
        atomicMin(&enc[4 * (size_t)c], u); atomicMin(&enc[4 * (size_t)c + 1], v);
        atomicMax(&enc[4 * (size_t)c + 2], u); atomicMax(&enc[4 * (size_t)c + 3], v);
    }
}
__global__ void __launch_bounds__(AT_BLOCK) k_atlas_bounds_decode(uint32_t* __restrict__ enc, int n) {
    const int i = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (i < n) enc[i] = __float_as_uint(at_dec(enc[i]));
}

__global__ void __launch_bounds__(AT_BLOCK) k_atlas_emit(const float* __restrict__ verts, int V, const int32_t* __restrict__ uv_chart, const int32_t* __restrict__ uv_vertex,
                                                         int n_uv, const int32_t* __restrict__ chart_bucket, const float* __restrict__ bounds,
                                                         const int32_t* __restrict__ origin, int n_charts, float s, int w0, int h0, float* __restrict__ vt) {
    const int i = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (i >= n_uv) return;
    const int c = uv_chart[i], m = uv_vertex[i];
    float u = __uint_as_float(0x7FC00000u), v = u;                      // NaN for a pair that names no chart or vertex: such a triangle covers nothing
    if (c >= 0 && c < n_charts && m >= 0 && m < V) {
        const int b = chart_bucket[c];
        if (b >= 0 && b < 6) {
            const float cu = verts[3 * (size_t)m + AT_U[b]], cv = verts[3 * (size_t)m + AT_V[b]];
            // (origin + 0.5) is exact; then one fp32 subtraction, multiplication and addition, and the division: the quotient of two floats rounded to
            // fp64 and then to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)
            const float du = (cu - bounds[4 * (size_t)c]) * s, dv = (cv - bounds[4 * (size_t)c + 1]) * s;
            const float tu = ((float)origin[2 * (size_t)c] + 0.5f) + du, tv = ((float)origin[2 * (size_t)c + 1] + 0.5f) + dv;
            u = (float)((double)tu / (double)w0); v = (float)((double)tv / (double)h0);
        }
    }
    vt[2 * (size_t)i] = u; vt[2 * (size_t)i + 1] = v;
}

// PASS 0: every covered centre sets its bit in `once`; a centre whose bit was set already (the returning atomicOr) sets its bit in `twice`.
// PASS 1: every triangle that covers a centre marked in `twice` flags its chart (slot n_charts for a face of no chart).
// Work items as in mirres_uv_rasterize: up to 32 consecutive texels of one triangle's box, whatever the triangle's size.
template <int PASS>
__global__ void __launch_bounds__(BK_BLOCK) k_atlas_cover(const UvTri* __restrict__ tris, const unsigned long long* __restrict__ first, int T, int W,
                                                          uint32_t* __restrict__ once, uint32_t* __restrict__ twice, const int32_t* __restrict__ face_chart,
                                                          int n_charts, uint8_t* __restrict__ flagged) {
    const unsigned long long total = first[T];
    const unsigned long long stride = (unsigned long long)gridDim.x * BK_BLOCK;
    for (unsigned long long k = (unsigned long long)blockIdx.x * BK_BLOCK + threadIdx.x; k < total; k += stride) {
        const int t = uv_item_triangle(first, T, k);
        const UvTri r = tris[t];
        const long long i0 = (long long)(k - first[t]) * BK_CHUNK, n = (long long)r.bw * r.bh;
        bool hit = false;
        for (int j = 0; j < BK_CHUNK; j++) {
            const long long i = i0 + j;
            if (i >= n) break;
            const int c = r.c0 + (int)(i % r.bw), row = r.r0 + (int)(i / r.bw);
            long long w0, w1, w2;
            if (!inside(r, (long long)c * BK_FIX + BK_FIX / 2, (long long)row * BK_FIX + BK_FIX / 2, w0, w1, w2)) continue;
            const size_t p = (size_t)row * W + c;
            const uint32_t bit = 1u << (p & 31);
            if (PASS == 0) { if (atomicOr(&once[p >> 5], bit) & bit) atomicOr(&twice[p >> 5], bit); }
            else hit = hit || (twice[p >> 5] & bit);
        }
        if (PASS == 1 && hit) {
            const int c = face_chart[t];
            flagged[(c >= 0 && c < n_charts) ? c : n_charts] = 1;
        }
    }
}

static size_t atlas_bitmap_bytes(int W, int H) { return align256(4 * (((size_t)W * H + 31) / 32)); }
static bool atlas_mesh_args_ok(int V, int T) { return V >= 0 && T >= 0 && T < (1 << 24); }

}  // namespace mr

using namespace mr;

extern "C" int mirres_atlas_classify(const float* verts, int V, const int32_t* tris, int T, float* normal, int32_t* bucket, void* stream) {
    if (!atlas_mesh_args_ok(V, T) || (T > 0 && (!tris || !normal || !bucket)) || (T > 0 && V > 0 && !verts)) {
        set_error("mirres_atlas_classify: bad argument (V %d, T %d; fewer than 2^24 faces)", V, T); return MIRRES_E_ARG;
    }
    if (T == 0) return MIRRES_OK;
    k_atlas_classify<<<grid_for((size_t)T, AT_BLOCK), AT_BLOCK, 0, (hipStream_t)stream>>>(verts, V, tris, T, normal, bucket);
    MR_LAUNCH_CHECK("atlas_classify");
    return MIRRES_OK;
}

extern "C" int mirres_atlas_smooth(const float* normal, const int32_t* bucket_in, const int32_t* nbr, int T, float cos_min, int32_t* bucket_out, void* stream) {
    if (T < 0 || T >= (1 << 24) || !(cos_min >= 0.f && cos_min <= 1.f) || (T > 0 && (!normal || !bucket_in || !nbr || !bucket_out)) || (T > 0 && bucket_in == bucket_out)) {
        set_error("mirres_atlas_smooth: bad argument (T %d, cos_min %g in [0, 1]; a round is not done in place)", T, (double)cos_min); return MIRRES_E_ARG;
    }
    if (T == 0) return MIRRES_OK;
    k_atlas_smooth<<<grid_for((size_t)T, AT_BLOCK), AT_BLOCK, 0, (hipStream_t)stream>>>(normal, bucket_in, nbr, T, (double)cos_min * (double)cos_min, bucket_out);
    MR_LAUNCH_CHECK("atlas_smooth");
    return MIRRES_OK;
}

extern "C" int mirres_atlas_bounds(const float* verts, int V, const int32_t* tris, int T, const int32_t* bucket, const int32_t* chart, int n_charts, float* bounds,
                                   void* stream) {
    if (!atlas_mesh_args_ok(V, T) || n_charts < 0 || n_charts > T || (n_charts > 0 && !bounds) || (T > 0 && (!tris || !bucket || !chart)) || (T > 0 && V > 0 && !verts)) {
        set_error("mirres_atlas_bounds: bad argument (V %d, T %d, %d charts)", V, T, n_charts); return MIRRES_E_ARG;
    }
    if (n_charts == 0) return MIRRES_OK;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* enc = reinterpret_cast<uint32_t*>(bounds);
    k_atlas_bounds_init<<<grid_for((size_t)n_charts, AT_BLOCK), AT_BLOCK, 0, s>>>(enc, n_charts);
    k_atlas_bounds<<<grid_for((size_t)T, AT_BLOCK), AT_BLOCK, 0, s>>>(verts, V, tris, T, bucket, chart, n_charts, enc);
    k_atlas_bounds_decode<<<grid_for(4 * (size_t)n_charts, AT_BLOCK), AT_BLOCK, 0, s>>>(enc, 4 * n_charts);
    MR_LAUNCH_CHECK("atlas_bounds");
    return MIRRES_OK;
}

extern "C" int mirres_atlas_emit(const float* verts, int V, const int32_t* uv_chart, const int32_t* uv_vertex, int n_uv, const int32_t* chart_bucket, const float* bounds,
                                 const int32_t* origin, int n_charts, float density, int w0, int h0, float* vt, void* stream) {
    if (V < 0 || n_uv < 0 || n_uv > 3 * ((1 << 24) - 1) || n_charts < 0 || n_charts >= (1 << 24) || w0 <= 0 || h0 <= 0 || w0 > 65536 || h0 > 65536 || !(density >= 0.f) ||
        !isfinite(density) || (n_uv > 0 && (!uv_chart || !uv_vertex || !vt)) || (n_uv > 0 && n_charts > 0 && (!chart_bucket || !bounds || !origin || !verts))) {
        set_error("mirres_atlas_emit: bad argument (V %d, %d UV vertices, %d charts, %d x %d, density %g)", V, n_uv, n_charts, w0, h0, (double)density); return MIRRES_E_ARG;
    }
    if (n_uv == 0) return MIRRES_OK;
    k_atlas_emit<<<grid_for((size_t)n_uv, AT_BLOCK), AT_BLOCK, 0, (hipStream_t)stream>>>(verts, V, uv_chart, uv_vertex, n_uv, chart_bucket, bounds, origin, n_charts, density,
                                                                                        w0, h0, vt);
    MR_LAUNCH_CHECK("atlas_emit");
    return MIRRES_OK;
}

extern "C" long long mirres_atlas_verify_scratch(int T, int W, int H) {
    if (T < 0 || T >= (1 << 24) || W <= 0 || H <= 0 || W > 65536 || H > 65536 || (long long)W * H >= (1LL << 31)) return -1;
    return (long long)(uv_items_bytes(T) + 2 * atlas_bitmap_bytes(W, H));
}

extern "C" int mirres_atlas_verify(const float* vt, int n_uv, const int32_t* ft, int T, const int32_t* face_chart, int n_charts, int W, int H, uint8_t* flagged,
                                   void* scratch, long long scratch_bytes, void* stream) {
    if (T < 0 || n_uv < 0 || n_charts < 0 || n_charts > T || W <= 0 || H <= 0 || W > 65536 || H > 65536 || (long long)W * H >= (1LL << 31) || !flagged) {
        set_error("mirres_atlas_verify: bad argument (T %d, n_uv %d, %d charts, %d x %d)", T, n_uv, n_charts, W, H); return MIRRES_E_ARG;
    }
    if (T >= (1 << 24)) { set_error("mirres_atlas_verify: %d triangles (fewer than 2^24, as mirres_uv_rasterize)", T); return MIRRES_E_ARG; }
    if (T > 0 && (!vt || !ft || !face_chart || n_uv == 0 || !scratch || scratch_bytes < mirres_atlas_verify_scratch(T, W, H))) {
        set_error("mirres_atlas_verify: missing input or scratch (%lld bytes given, %lld needed)", scratch_bytes, mirres_atlas_verify_scratch(T, W, H)); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MR_HIP(hipMemsetAsync(flagged, 0, (size_t)n_charts + 1, s));
    if (T == 0) return MIRRES_OK;
    UvTri* tris; unsigned long long* first;
    uv_items_enqueue(vt, n_uv, ft, T, W, H, scratch, tris, first, s);
    uint32_t* once = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(scratch) + uv_items_bytes(T));
    uint32_t* twice = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(once) + atlas_bitmap_bytes(W, H));
    MR_HIP(hipMemsetAsync(once, 0, 2 * atlas_bitmap_bytes(W, H), s));
    k_atlas_cover<0><<<2048, BK_BLOCK, 0, s>>>(tris, first, T, W, once, twice, face_chart, n_charts, flagged);
    k_atlas_cover<1><<<2048, BK_BLOCK, 0, s>>>(tris, first, T, W, once, twice, face_chart, n_charts, flagged);
    MR_LAUNCH_CHECK("atlas_verify");
    return MIRRES_OK;
}
