// texmat.hip — material lookup in the exported stage-1 textured mesh (nerf/renderer.py:390-398 writes it; a viewer reads it back): per hit the
// barycentrics of the point on its triangle, the UV of that point, four clamped taps of the cascade's 8-byte texel plane decoded through the
// 8-bit sRGB table, bilinear filtering.  The exact rule (every step one correctly rounded fp32 operation, -ffp-contract=off) is written in
// include/mirres.h above mirres_texmat_lookup and restated in numpy by tests/texmat_refs.py.
//
// One kernel serves both callers: rows of the public entry point (occ / prim / pos per row), and the live-slot list of mirres_render's batches,
// where a vertex's triangle is the one its continuation ray hit (ray_prim[slot_c[slot]], written by the closest-hit trace of the bounce).
// Per hit: three UV corners (24 B) + three vertices (36 B) + four 8-byte texels; the decode table sits in LDS.
#include "engine.hpp"
#include "device_math.hpp"

namespace mr {

#define MR_TM_BLOCK 256
#define MR_TM_CAS 8

struct TexMatD {
    const float* verts; const int32_t* tris; const float* vt; const int32_t* ft;
    int n_cas; int tri_end[MR_TM_CAS]; int W[MR_TM_CAS], H[MR_TM_CAS]; const uint2* tex[MR_TM_CAS];
    const float* decode; float rough_min;
};

MR_DEV float tm_dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
MR_DEV float tm_lerp(float a, float b, float f) { return a + f * (b - a); }
MR_DEV float tm_byte(const float* sdec, uint2 t, int k) { return sdec[((k < 4 ? t.x : t.y) >> (8 * (k & 3))) & 255u]; }

// kd rgb, roughness, metallic of point p on triangle `prim` (0 <= prim < T)
MR_DEV void texmat_eval(const TexMatD& D, const float* sdec, int prim, v3 p, float o[5]) {
    const int i0 = D.tris[3 * (size_t)prim], i1 = D.tris[3 * (size_t)prim + 1], i2 = D.tris[3 * (size_t)prim + 2];
    const v3 v0 = ld3(D.verts, i0), v1 = ld3(D.verts, i1), v2 = ld3(D.verts, i2);
    const v3 e1 = V3(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z), e2 = V3(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z), d = V3(p.x - v0.x, p.y - v0.y, p.z - v0.z);
    const float d00 = tm_dot(e1, e1), d01 = tm_dot(e1, e2), d11 = tm_dot(e2, e2), d20 = tm_dot(d, e1), d21 = tm_dot(d, e2);
    const float den = d00 * d11 - d01 * d01;
    const float b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den, b0 = (1.0f - b1) - b2;
    const int t0 = D.ft[3 * (size_t)prim], t1 = D.ft[3 * (size_t)prim + 1], t2 = D.ft[3 * (size_t)prim + 2];
    const float2 c0 = reinterpret_cast<const float2*>(D.vt)[t0], c1 = reinterpret_cast<const float2*>(D.vt)[t1], c2 = reinterpret_cast<const float2*>(D.vt)[t2];
    const float u = (b0 * c0.x + b1 * c1.x) + b2 * c2.x, v = (b0 * c0.y + b1 * c1.y) + b2 * c2.y;
    // the cascade: a loop over the (kernel-argument) table whose trip count is the same for every lane; selects, no indexed private array
    const uint2* tb = D.tex[0]; int W = D.W[0], H = D.H[0];
#pragma unroll
    for (int k = 1; k < MR_TM_CAS; k++)
        if (k < D.n_cas && prim >= D.tri_end[k - 1]) { tb = D.tex[k]; W = D.W[k]; H = D.H[k]; }
    const float x = fmaxf(fminf(u * (float)W - 0.5f, (float)W), -1.0f), y = fmaxf(fminf(v * (float)H - 0.5f, (float)H), -1.0f);
    const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    const int xi = (int)xf, yi = (int)yf;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1), ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const uint2 t00 = tb[(size_t)ya * W + xa], t10 = tb[(size_t)ya * W + xb], t01 = tb[(size_t)yb * W + xa], t11 = tb[(size_t)yb * W + xb];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const float a = tm_lerp(tm_byte(sdec, t00, k), tm_byte(sdec, t10, k), fx), b = tm_lerp(tm_byte(sdec, t01, k), tm_byte(sdec, t11, k), fx);
        o[k] = tm_lerp(a, b, fy);
    }
    o[3] = fminf(fmaxf(o[3], D.rough_min), 1.0f);
}

// LIST: mirres_render's live slots (grid-stride over a device-side count; prim = ray_prim[slot_c[slot]]); otherwise one thread per row.
template <bool LIST>
__global__ void __launch_bounds__(MR_TM_BLOCK) k_texmat(TexMatD D, int T, const float* __restrict__ occ, const int32_t* __restrict__ prim, const float* __restrict__ pos,
                                                        int n, float* __restrict__ kd, float* __restrict__ rm, int use_scale, float sx, float sy, float sz,
                                                        const int32_t* __restrict__ live, const uint32_t* __restrict__ live_count, const int32_t* __restrict__ slot_c) {
    __shared__ float sdec[256];
    sdec[threadIdx.x] = D.decode[threadIdx.x];
    __syncthreads();
    const int n_items = LIST ? (int)*live_count : n;
    for (int t0 = blockIdx.x * MR_TM_BLOCK; t0 < n_items; t0 += gridDim.x * MR_TM_BLOCK) {
        const int t = t0 + (int)threadIdx.x;
        if (t >= n_items) continue;
        const int i = LIST ? live[t] : t;
        if (!occ || occ[i] >= 0.5f) {
            int pr = -1;
            if (LIST) { const int sc = slot_c[i]; if (sc >= 0) pr = prim[sc]; } else pr = prim[i];
            if (pr >= 0 && pr < T) {
                float o[5];
                texmat_eval(D, sdec, pr, ld3(pos, i), o);
                if (use_scale) { o[0] = o[0] * sx; o[1] = o[1] * sy; o[2] = o[2] * sz; }
                kd[3 * (size_t)i] = o[0]; kd[3 * (size_t)i + 1] = o[1]; kd[3 * (size_t)i + 2] = o[2];
                rm[2 * (size_t)i] = o[3]; rm[2 * (size_t)i + 1] = o[4];
            }
        }
        if (use_scale) {  // torch.clamp(new_diffuse_map, 0, 1) over the whole map (renderer_restir.py:408); in LIST mode over the listed slots (nothing reads the others)
#pragma unroll
            for (int k = 0; k < 3; k++) kd[3 * (size_t)i + k] = fminf(fmaxf(kd[3 * (size_t)i + k], 0.f), 1.f);
        }
    }
}

// the triangle of every slot's next vertex for the stepwise ABI (mirres_path_t::new_prim): the prim its continuation ray hit, -1 where there is no vertex
__global__ void __launch_bounds__(MR_TM_BLOCK) k_slot_prim(int n, const int32_t* __restrict__ slot_c, const float* __restrict__ new_occ, const int32_t* __restrict__ ray_prim,
                                                           int32_t* __restrict__ out) {
    const int i = blockIdx.x * MR_TM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = slot_c[i];
    out[i] = (s >= 0 && new_occ[i] >= 0.5f) ? ray_prim[s] : -1;
}

static int texmat_dev(const mirres_texmat_t* t, TexMatD& D, int& T, const char* who) {
    if (!t || !t->verts || !t->tris || !t->vt || !t->ft || !t->decode || t->n_cas < 1 || t->n_cas > MR_TM_CAS) { set_error("%s: bad texture material", who); return MIRRES_E_ARG; }
    D.verts = t->verts; D.tris = t->tris; D.vt = t->vt; D.ft = t->ft; D.n_cas = t->n_cas; D.decode = t->decode; D.rough_min = t->rough_min;
    int prev = 0;
    for (int c = 0; c < MR_TM_CAS; c++) {
        if (c < t->n_cas) {
            if (!t->texels[c] || t->W[c] < 1 || t->H[c] < 1 || t->tri_end[c] < prev || (reinterpret_cast<uintptr_t>(t->texels[c]) & 7)) {
                set_error("%s: cascade %d: texels %p, %d x %d, tri_end %d", who, c, t->texels[c], t->W[c], t->H[c], t->tri_end[c]); return MIRRES_E_ARG;
            }
            prev = t->tri_end[c];
            D.tri_end[c] = t->tri_end[c]; D.W[c] = t->W[c]; D.H[c] = t->H[c]; D.tex[c] = reinterpret_cast<const uint2*>(t->texels[c]);
        } else { D.tri_end[c] = prev; D.W[c] = 1; D.H[c] = 1; D.tex[c] = D.tex[0]; }
    }
    T = prev;
    return 0;
}

// mirres_render: the lookup at the vertices of a bounce (live list, prims of the continuation rays)
int launch_texmat_live(const mirres_texmat_t* t, const float* occ, const float* pos, int nv, float* kd, float* rm, int use_scale, const float* scale3, const int32_t* live,
                       const uint32_t* live_count, const int32_t* slot_c, const int32_t* ray_prim, hipStream_t s) {
    TexMatD D; int T = 0;
    if (int rc = texmat_dev(t, D, T, "mirres_render")) return rc;
    const float sx = scale3 ? scale3[0] : 1.f, sy = scale3 ? scale3[1] : 1.f, sz = scale3 ? scale3[2] : 1.f;
    int g = grid_for(nv, MR_TM_BLOCK); if (g > 256 * 8) g = 256 * 8;
    k_texmat<true><<<g, MR_TM_BLOCK, 0, s>>>(D, T, occ, ray_prim, pos, nv, kd, rm, use_scale, sx, sy, sz, live, live_count, slot_c);
    MR_LAUNCH_CHECK("texmat_live");
    return 0;
}

int launch_slot_prim(int n, const int32_t* slot_c, const float* new_occ, const int32_t* ray_prim, int32_t* out, hipStream_t s) {
    k_slot_prim<<<grid_for(n, MR_TM_BLOCK), MR_TM_BLOCK, 0, s>>>(n, slot_c, new_occ, ray_prim, out);
    MR_LAUNCH_CHECK("slot_prim");
    return 0;
}

}  // namespace mr

using namespace mr;

extern "C" int mirres_texmat_lookup(const mirres_texmat_t* t, const float* occ, const int32_t* prim, const float* pos, int n, float* kd, float* rough_metal,
                                    int use_scale, const float* h_scale3, void* stream) {
    if (!prim || !pos || !kd || !rough_metal || n < 0) { set_error("mirres_texmat_lookup: bad argument"); return MIRRES_E_ARG; }
    TexMatD D; int T = 0;
    if (int rc = texmat_dev(t, D, T, "mirres_texmat_lookup")) return rc;
    if (n == 0) return MIRRES_OK;
    const float sx = h_scale3 ? h_scale3[0] : 1.f, sy = h_scale3 ? h_scale3[1] : 1.f, sz = h_scale3 ? h_scale3[2] : 1.f;
    k_texmat<false><<<grid_for(n, MR_TM_BLOCK), MR_TM_BLOCK, 0, (hipStream_t)stream>>>(D, T, occ, prim, pos, n, kd, rough_metal, use_scale, sx, sy, sz, nullptr, nullptr, nullptr);
    MR_LAUNCH_CHECK("texmat_lookup");
    return MIRRES_OK;
}

// development aid (not part of include/mirres.h): the lookup as mirres_render's batches run it (launch_texmat_live) on caller-given lists — live: int32 slots in
// [0, nv), live_count: uint32[1] on the DEVICE, slot_c: int32[nv] ray of every slot (or -1), ray_prim: int32 triangle of every ray; occ may be null.
extern "C" int mirres_debug_texmat_live(const mirres_texmat_t* t, const float* occ, const float* pos, int nv, float* kd, float* rough_metal, int use_scale,
                                        const float* h_scale3, const int32_t* live, const uint32_t* live_count, const int32_t* slot_c, const int32_t* ray_prim,
                                        void* stream) {
    if (!pos || !kd || !rough_metal || !live || !live_count || !slot_c || !ray_prim || nv <= 0) { set_error("mirres_debug_texmat_live: bad argument"); return MIRRES_E_ARG; }
    return launch_texmat_live(t, occ, pos, nv, kd, rough_metal, use_scale, h_scale3, live, live_count, slot_c, ray_prim, (hipStream_t)stream);
}
