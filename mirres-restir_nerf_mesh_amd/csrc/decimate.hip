// decimate.hip — quadric-error edge collapse for the stage-0 export (decimate_mesh, meshutils.py:64-97, called at nerf/renderer.py:566-567) on the device, with no
// mesh library behind it.  Garland & Heckbert 1997 in deterministic, round-parallel form; one round is
//   mirres_dec_vertex_flags   which vertices lie on a boundary edge / on an edge with more than two faces;
//   mirres_dec_quadrics       (first round only) one area-weighted plane quadric per face and one constraint per boundary edge, GATHERED per vertex;
//   mirres_dec_edge           k_dec_edge: placement, cost, validity and the 64-bit key of every edge;
//   mirres_dec_select         k_dec_claim / k_dec_select: an independent set of the cheapest candidates by atomicMin of the keys over their regions;
//   mirres_dec_apply          k_dec_apply_edges / k_dec_apply_faces: the selected collapses, then the faces through the vertex remap.
// The host (stage0.decimate_mesh) does the sorts between them: the edge list (sorted unique keys min << 32 | max, their multiplicity, the edge of every face
// corner), the vertex -> corner CSR (stable sort of the 3 T corners by vertex: a vertex's corners in ascending order 3 f + k) and the candidate cut.
// State: positions f32, one symmetric 4 x 4 quadric per vertex as 10 doubles (a00 a01 a02 a03 a11 a12 a13 a22 a23 a33), triangles i32.  All per-edge arithmetic is
// fp64 on the fp32 positions, every step one correctly rounded operation (the library is built with -ffp-contract=off), sums are gathers in CSR order: equal
// inputs give equal bytes.  The only atomics are integer min / or / add, which do not depend on their order.  The rings are walked through the CSR, nothing is
// kept in per-thread arrays: a vertex of high valence costs time (quadratic in the valence for the link condition), not correctness.
#include <float.h>
#include "engine.hpp"
#include "device_math.hpp"

namespace mr {

#define DEC_BLOCK 256
#define DEC_BOUNDARY_WEIGHT 1.0     // a boundary edge's constraint plane weighs this times its squared length (a face's plane weighs its area)
#define DEC_DET_REL 1e-9            // the 3 x 3 system counts as singular when |det| <= this * (largest |entry|)^3
#define DEC_FLIP_COS2 0.04          // a moved face keeps a normal within acos(0.2) of its old one: dot > 0 and dot^2 > 0.04 |N|^2 |N'|^2
#define DEC_F_MULT 1                // validity bits of k_dec_edge (mirres.h)
#define DEC_F_LINK 2
#define DEC_F_BOUNDARY 4
#define DEC_F_FLIP 8
#define DEC_F_FINITE 16
#define DEC_KEY_NONE 0x7FFFFFFFFFFFFFFFULL

struct D3 { double x, y, z; };
MR_DEV D3 d3_load(const float* __restrict__ p, int v) { D3 r; r.x = (double)p[3 * (long long)v]; r.y = (double)p[3 * (long long)v + 1]; r.z = (double)p[3 * (long long)v + 2]; return r; }
MR_DEV D3 d3_sub(D3 a, D3 b) { D3 r; r.x = a.x - b.x; r.y = a.y - b.y; r.z = a.z - b.z; return r; }
MR_DEV D3 d3_cross(D3 a, D3 b) { D3 r; r.x = a.y * b.z - a.z * b.y; r.y = a.z * b.x - a.x * b.z; r.z = a.x * b.y - a.y * b.x; return r; }
MR_DEV double d3_dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
MR_DEV D3 d3_pick(D3 a, D3 b, D3 c, int k) { return k == 0 ? a : (k == 1 ? b : c); }

// q += w * (u, d)(u, d)^T
MR_DEV void q_add_plane(double* q, D3 u, double d, double w) {
    q[0] += w * (u.x * u.x); q[1] += w * (u.x * u.y); q[2] += w * (u.x * u.z); q[3] += w * (u.x * d);
    q[4] += w * (u.y * u.y); q[5] += w * (u.y * u.z); q[6] += w * (u.y * d);
    q[7] += w * (u.z * u.z); q[8] += w * (u.z * d);
    q[9] += w * (d * d);
}

// (x, y, z, 1) Q (x, y, z, 1)^T, row by row: on a plane all of a vertex's faces share, every row sum is an exact zero
MR_DEV double q_eval(const double* q, double x, double y, double z) {
    const double r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
    const double r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6];
    const double r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8];
    const double r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9];
    return ((x * r0 + y * r1) + z * r2) + r3;
}

// bit 0: the vertex lies on an edge with exactly one face (a boundary vertex); bit 1: on an edge with more than two faces (left alone)
__global__ void __launch_bounds__(DEC_BLOCK) k_dec_vertex_flags(const unsigned long long* __restrict__ ekeys, const int32_t* __restrict__ emult, int E, int V, int32_t* __restrict__ vflag) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int m = emult[e];
    const int bit = m == 1 ? 1 : (m > 2 ? 2 : 0);
    if (!bit) return;
    const int a = (int)(ekeys[e] >> 32), b = (int)(ekeys[e] & 0xFFFFFFFFULL);
    if (a >= 0 && a < V) atomicOr(&vflag[a], bit);
    if (b >= 0 && b < V) atomicOr(&vflag[b], bit);
}

// one thread per vertex: its corners in CSR order; per corner (face f, position k) the face's plane, then the constraints of the face's two edges at the vertex
// (edge k = (v_k, v_k+1), then edge k + 2 = (v_k+2, v_k)) where the edge has no second face
__global__ void __launch_bounds__(DEC_BLOCK) k_dec_quadrics(const float* __restrict__ pos, int V, const int32_t* __restrict__ tris, const int32_t* __restrict__ vstart,
                                                            const int32_t* __restrict__ vcorner, const int32_t* __restrict__ corner_edge, const int32_t* __restrict__ emult,
                                                            double* __restrict__ quad) {
    const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (v >= V) return;
    double q[10];
    for (int j = 0; j < 10; j++) q[j] = 0.0;
    for (int i = vstart[v]; i < vstart[v + 1]; i++) {
        const int c = vcorner[i], f = c / 3, k = c - 3 * f;
        const D3 p0 = d3_load(pos, tris[3 * (long long)f]), p1 = d3_load(pos, tris[3 * (long long)f + 1]), p2 = d3_load(pos, tris[3 * (long long)f + 2]);
        const D3 n = d3_cross(d3_sub(p1, p0), d3_sub(p2, p0));
        const double l2 = d3_dot(n, n);
        if (!(l2 > 0.0)) continue;                                                   // a face without area has no plane: nothing, and no NaN
        const double l = sqrt(l2);
        D3 u; u.x = n.x / l; u.y = n.y / l; u.z = n.z / l;
        q_add_plane(q, u, -d3_dot(u, p0), 0.5 * l);
        for (int s = 0; s < 2; s++) {
            const int j = s == 0 ? k : (k + 2) % 3;
            if (emult[corner_edge[3 * (long long)f + j]] != 1) continue;
            const D3 pu = d3_pick(p0, p1, p2, j), pw = d3_pick(p0, p1, p2, (j + 1) % 3);
            const D3 ed = d3_sub(pw, pu);
            const D3 m = d3_cross(ed, u);                                            // the plane through the edge, perpendicular to the face
            const double m2 = d3_dot(m, m);
            if (!(m2 > 0.0)) continue;
            const double ml = sqrt(m2);
            D3 w; w.x = m.x / ml; w.y = m.y / ml; w.z = m.z / ml;
            q_add_plane(q, w, -d3_dot(w, pu), DEC_BOUNDARY_WEIGHT * d3_dot(ed, ed));
        }
    }
    for (int j = 0; j < 10; j++) quad[10 * (long long)v + j] = q[j];
}

MR_DEV bool tri_has(const int32_t* __restrict__ tris, int f, int x) {
    return tris[3 * (long long)f] == x || tris[3 * (long long)f + 1] == x || tris[3 * (long long)f + 2] == x;
}

// the faces around `moved` that do not contain `other`, with `moved` at the new position nv: false when one of them turns its normal too far or loses its area;
// dup is set when one of them contains both c0 and c1 (the vertices opposite the edge)
MR_DEV bool ring_keeps_normals(const float* __restrict__ pos, const int32_t* __restrict__ tris, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vcorner,
                               int moved, int other, D3 nv, int c0, int c1, bool& dup) {
    bool ok = true;
    for (int i = vstart[moved]; i < vstart[moved + 1]; i++) {
        const int f = vcorner[i] / 3;
        const int i0 = tris[3 * (long long)f], i1 = tris[3 * (long long)f + 1], i2 = tris[3 * (long long)f + 2];
        if (i0 == other || i1 == other || i2 == other) continue;
        const D3 p0 = d3_load(pos, i0), p1 = d3_load(pos, i1), p2 = d3_load(pos, i2);
        const D3 n = d3_cross(d3_sub(p1, p0), d3_sub(p2, p0));
        const D3 r0 = i0 == moved ? nv : p0, r1 = i1 == moved ? nv : p1, r2 = i2 == moved ? nv : p2;
        const D3 m = d3_cross(d3_sub(r1, r0), d3_sub(r2, r0));
        const double dt = d3_dot(n, m);
        if (!(dt > 0.0 && dt * dt > DEC_FLIP_COS2 * (d3_dot(n, n) * d3_dot(m, m)))) ok = false;
        if (c1 >= 0 && (i0 == c0 || i1 == c0 || i2 == c0) && (i0 == c1 || i1 == c1 || i2 == c1)) dup = true;
    }
    return ok;
}

// one thread per edge (a, b), a < b
__global__ void __launch_bounds__(DEC_BLOCK) k_dec_edge(const float* __restrict__ pos, const double* __restrict__ quad, int V, const int32_t* __restrict__ tris,
                                                        const int32_t* __restrict__ vstart, const int32_t* __restrict__ vcorner, const unsigned long long* __restrict__ ekeys,
                                                        const int32_t* __restrict__ emult, const int32_t* __restrict__ vflag, int E, int optimal,
                                                        double* __restrict__ cost_out, float* __restrict__ epos, int32_t* __restrict__ eflags, unsigned long long* __restrict__ keys) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int a = (int)(ekeys[e] >> 32), b = (int)(ekeys[e] & 0xFFFFFFFFULL), m = emult[e];
    if (a < 0 || b >= V || a >= b) {                                                 // a face with a repeated index gives the "edge" (a, a): never collapsed
        cost_out[e] = 0.0; epos[3 * (long long)e] = epos[3 * (long long)e + 1] = epos[3 * (long long)e + 2] = 0.f; eflags[e] = DEC_F_MULT; keys[e] = DEC_KEY_NONE;
        return;
    }
    int flags = 0;
    const int fa = vflag[a], fb = vflag[b];
    if (m < 1 || m > 2 || ((fa | fb) & 2)) flags |= DEC_F_MULT;
    if (m == 2 && (fa & 1) && (fb & 1)) flags |= DEC_F_BOUNDARY;
    double q[10];
    for (int j = 0; j < 10; j++) q[j] = quad[10 * (long long)a + j] + quad[10 * (long long)b + j];
    const D3 pa = d3_load(pos, a), pb = d3_load(pos, b);
    // placement
    float vx = 0.f, vy = 0.f, vz = 0.f; bool placed = false;
    if (optimal == 1) {
        const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[2] * q[4];
        const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
        const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
        const double s = fmax(fmax(fmax(fabs(q[0]), fabs(q[1])), fmax(fabs(q[2]), fabs(q[4]))), fmax(fabs(q[5]), fabs(q[7])));
        if (fabs(det) > DEC_DET_REL * ((s * s) * s)) {
            vx = (float)(-(((c00 * q[3] + c01 * q[6]) + c02 * q[8]) / det));
            vy = (float)(-(((c01 * q[3] + c11 * q[6]) + c12 * q[8]) / det));
            vz = (float)(-(((c02 * q[3] + c12 * q[6]) + c22 * q[8]) / det));
            placed = (vx - vx == 0.f) && (vy - vy == 0.f) && (vz - vz == 0.f);
        }
    }
    double cost;
    if (placed) {
        cost = q_eval(q, (double)vx, (double)vy, (double)vz);
    } else {                                                                         // p_a, p_b, their midpoint (optimal == 2: the end points only): the cheapest, ties in that order
        const float mx = (float)(0.5 * (pa.x + pb.x)), my = (float)(0.5 * (pa.y + pb.y)), mz = (float)(0.5 * (pa.z + pb.z));
        const double ca = q_eval(q, pa.x, pa.y, pa.z), cb = q_eval(q, pb.x, pb.y, pb.z), cm = q_eval(q, (double)mx, (double)my, (double)mz);
        cost = ca; vx = (float)pa.x; vy = (float)pa.y; vz = (float)pa.z;
        if (cb < cost) { cost = cb; vx = (float)pb.x; vy = (float)pb.y; vz = (float)pb.z; }
        if (optimal != 2 && cm < cost) { cost = cm; vx = mx; vy = my; vz = mz; }
    }
    cost = cost > 0.0 ? cost : (cost == cost ? 0.0 : cost);                          // max(cost, 0), a NaN kept for the finiteness bit
    const float cf = (float)cost;
    if (!(cf - cf == 0.f) || !((vx - vx == 0.f) && (vy - vy == 0.f) && (vz - vz == 0.f))) flags |= DEC_F_FINITE;
    // link condition: the vertices opposite the edge in its faces, then the distinct common neighbours of a and b
    int c0 = -1, c1 = -1;
    const int sa = vstart[a], ea = vstart[a + 1], sb = vstart[b], eb = vstart[b + 1];
    int ncommon = 0;
    for (int i = sa; i < ea; i++) {
        const int f = vcorner[i] / 3;
        const bool has_b = tri_has(tris, f, b);
        for (int k = 0; k < 3; k++) {
            const int x = tris[3 * (long long)f + k];
            if (x == a || x == b) continue;
            if (has_b) { if (c0 < 0) c0 = x; else if (c1 < 0 && x != c0) c1 = x; }
            bool seen = false;
            for (int kk = 0; kk < k; kk++) seen = seen || tris[3 * (long long)f + kk] == x;
            for (int j = sa; j < i && !seen; j++) seen = tri_has(tris, vcorner[j] / 3, x);
            if (seen) continue;
            bool adj = false;
            for (int j = sb; j < eb && !adj; j++) adj = tri_has(tris, vcorner[j] / 3, x);
            ncommon += adj ? 1 : 0;
        }
    }
    if (ncommon != m) flags |= DEC_F_LINK;
    // normals of the faces that stay, and the pair of faces (a, c0, c1), (b, c0, c1) that would coincide (the last collapse of a tetrahedron)
    D3 nv; nv.x = (double)vx; nv.y = (double)vy; nv.z = (double)vz;
    bool dup_a = false, dup_b = false;
    const bool keep_a = ring_keeps_normals(pos, tris, vstart, vcorner, a, b, nv, c0, c1, dup_a);
    const bool keep_b = ring_keeps_normals(pos, tris, vstart, vcorner, b, a, nv, c0, c1, dup_b);
    if (!(keep_a && keep_b)) flags |= DEC_F_FLIP;
    if (dup_a && dup_b) flags |= DEC_F_LINK;
    cost_out[e] = cost;
    epos[3 * (long long)e] = vx; epos[3 * (long long)e + 1] = vy; epos[3 * (long long)e + 2] = vz;
    eflags[e] = flags;
    // optimal == 2: equal costs are ordered by a bijective scramble of the edge id (e * 0x9E3779B1 mod 2^32; the host multiplies by the inverse).  The mesh of a 0 / 1
    // volume is flat almost everywhere, cost exactly 0: ordered by the id itself, which follows the grid, an edge is the cheapest of its region only where a flat
    // stretch begins, and a round collapses a few dozen edges of 10^5 candidates
    const unsigned low = optimal == 2 ? (unsigned)e * 0x9E3779B1u : (unsigned)e;
    keys[e] = flags ? DEC_KEY_NONE : (((unsigned long long)__float_as_uint(cf) << 32) | (unsigned long long)low);
}

// region of an edge: a, b and every vertex of a face around a or b.  mode 0: atomicMin of the key into vkey over the region; mode 1: true when all of them hold the key
MR_DEV bool region_walk(const int32_t* __restrict__ tris, int V, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vcorner, int a, int b,
                        unsigned long long key, unsigned long long* __restrict__ vkey, int mode) {
    bool all = true;
    for (int side = 0; side < 2; side++) {
        const int v = side ? b : a;
        for (int i = vstart[v]; i < vstart[v + 1]; i++) {
            const int f = vcorner[i] / 3;
            for (int k = 0; k < 3; k++) {
                const int w = tris[3 * (long long)f + k];
                if (w < 0 || w >= V) continue;
                if (mode == 0) atomicMin(&vkey[w], key);
                else all = all && vkey[w] == key;
            }
        }
    }
    return all;
}

__global__ void __launch_bounds__(DEC_BLOCK) k_dec_claim(const int32_t* __restrict__ tris, int V, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vcorner,
                                                         const unsigned long long* __restrict__ ekeys, int E, const unsigned long long* __restrict__ keys,
                                                         const int32_t* __restrict__ cand, int n_cand, unsigned long long* __restrict__ vkey) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= n_cand) return;
    const int e = cand[i];
    if (e < 0 || e >= E || keys[e] == DEC_KEY_NONE) return;
    const int a = (int)(ekeys[e] >> 32), b = (int)(ekeys[e] & 0xFFFFFFFFULL);
    if (a < 0 || a >= V || b < 0 || b >= V) return;
    region_walk(tris, V, vstart, vcorner, a, b, keys[e], vkey, 0);
}

__global__ void __launch_bounds__(DEC_BLOCK) k_dec_select(const int32_t* __restrict__ tris, int V, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vcorner,
                                                          const unsigned long long* __restrict__ ekeys, int E, const unsigned long long* __restrict__ keys,
                                                          const int32_t* __restrict__ cand, int n_cand, unsigned long long* __restrict__ vkey, uint8_t* __restrict__ sel,
                                                          int32_t* __restrict__ count) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= n_cand) return;
    const int e = cand[i];
    bool won = false;
    if (e >= 0 && e < E && keys[e] != DEC_KEY_NONE) {
        const int a = (int)(ekeys[e] >> 32), b = (int)(ekeys[e] & 0xFFFFFFFFULL);
        if (a >= 0 && a < V && b >= 0 && b < V) won = region_walk(tris, V, vstart, vcorner, a, b, keys[e], vkey, 1);
    }
    sel[i] = won ? 1 : 0;
    if (won) atomicAdd(count, 1);
}

__global__ void __launch_bounds__(DEC_BLOCK) k_dec_iota(int32_t* __restrict__ a, int n) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i < n) a[i] = i;
}

// the regions of the selected edges are pairwise disjoint: nobody else reads or writes a, b in this launch
__global__ void __launch_bounds__(DEC_BLOCK) k_dec_apply_edges(float* __restrict__ pos, double* __restrict__ quad, int V, const unsigned long long* __restrict__ ekeys, int E,
                                                               const float* __restrict__ epos, const int32_t* __restrict__ cand, const uint8_t* __restrict__ sel, int n_cand,
                                                               int32_t* __restrict__ remap) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= n_cand || !sel[i]) return;
    const int e = cand[i];
    if (e < 0 || e >= E) return;
    const int a = (int)(ekeys[e] >> 32), b = (int)(ekeys[e] & 0xFFFFFFFFULL);
    if (a < 0 || a >= V || b < 0 || b >= V || a == b) return;
    for (int k = 0; k < 3; k++) pos[3 * (long long)a + k] = epos[3 * (long long)e + k];
    for (int j = 0; j < 10; j++) quad[10 * (long long)a + j] = quad[10 * (long long)a + j] + quad[10 * (long long)b + j];
    remap[b] = a;
}

__global__ void __launch_bounds__(DEC_BLOCK) k_dec_apply_faces(int32_t* __restrict__ tris, int T, int V, const int32_t* __restrict__ remap, uint8_t* __restrict__ keep,
                                                               uint8_t* __restrict__ used) {
    const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (f >= T) return;
    int r[3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        const int v = tris[3 * (long long)f + k];
        ok = ok && v >= 0 && v < V;
        r[k] = ok ? remap[v] : 0;
    }
    ok = ok && r[0] != r[1] && r[1] != r[2] && r[0] != r[2];
    if (ok) for (int k = 0; k < 3; k++) { tris[3 * (long long)f + k] = r[k]; used[r[k]] = 1; }      // every writer stores the same value
    keep[f] = ok ? 1 : 0;
}

static bool dec_sizes_ok(int V, int T) { return V > 0 && T > 0 && T <= 0x7FFFFFFF / 3; }

}  // namespace mr

using namespace mr;

extern "C" int mirres_dec_vertex_flags(const unsigned long long* edge_keys, const int32_t* edge_mult, int E, int V, int32_t* vflag, void* stream) {
    if (E < 0 || V <= 0 || !vflag || (E > 0 && (!edge_keys || !edge_mult))) { set_error("mirres_dec_vertex_flags: bad argument (E %d, V %d)", E, V); return MIRRES_E_ARG; }
    hipStream_t s = (hipStream_t)stream;
    MR_HIP(hipMemsetAsync(vflag, 0, sizeof(int32_t) * (size_t)V, s));
    if (E > 0) k_dec_vertex_flags<<<grid_for((size_t)E, DEC_BLOCK), DEC_BLOCK, 0, s>>>(edge_keys, edge_mult, E, V, vflag);
    MR_LAUNCH_CHECK("dec_vertex_flags");
    return MIRRES_OK;
}

extern "C" int mirres_dec_quadrics(const float* verts, int V, const int32_t* tris, int T, const int32_t* vstart, const int32_t* vcorner, const int32_t* corner_edge,
                                   const int32_t* edge_mult, int E, double* quadrics, void* stream) {
    if (!dec_sizes_ok(V, T) || E <= 0 || !verts || !tris || !vstart || !vcorner || !corner_edge || !edge_mult || !quadrics) {
        set_error("mirres_dec_quadrics: bad argument (V %d, T %d, E %d)", V, T, E); return MIRRES_E_ARG;
    }
    k_dec_quadrics<<<grid_for((size_t)V, DEC_BLOCK), DEC_BLOCK, 0, (hipStream_t)stream>>>(verts, V, tris, vstart, vcorner, corner_edge, edge_mult, quadrics);
    MR_LAUNCH_CHECK("dec_quadrics");
    return MIRRES_OK;
}

extern "C" int mirres_dec_edge(const float* verts, const double* quadrics, int V, const int32_t* tris, int T, const int32_t* vstart, const int32_t* vcorner,
                               const unsigned long long* edge_keys, const int32_t* edge_mult, const int32_t* vflag, int E, int optimalplacement, double* cost,
                               float* position, int32_t* flags, unsigned long long* keys, void* stream) {
    if (!dec_sizes_ok(V, T) || E <= 0 || !verts || !quadrics || !tris || !vstart || !vcorner || !edge_keys || !edge_mult || !vflag || !cost || !position || !flags || !keys) {
        set_error("mirres_dec_edge: bad argument (V %d, T %d, E %d)", V, T, E); return MIRRES_E_ARG;
    }
    k_dec_edge<<<grid_for((size_t)E, DEC_BLOCK), DEC_BLOCK, 0, (hipStream_t)stream>>>(verts, quadrics, V, tris, vstart, vcorner, edge_keys, edge_mult, vflag, E,
                                                                                     optimalplacement == 2 ? 2 : (optimalplacement ? 1 : 0), cost, position, flags, keys);
    MR_LAUNCH_CHECK("dec_edge");
    return MIRRES_OK;
}

extern "C" int mirres_dec_select(const int32_t* tris, int T, int V, const int32_t* vstart, const int32_t* vcorner, const unsigned long long* edge_keys, int E,
                                 const unsigned long long* keys, const int32_t* cand, int n_cand, unsigned long long* vkey, uint8_t* selected, int32_t* d_count, void* stream) {
    if (!dec_sizes_ok(V, T) || E <= 0 || n_cand <= 0 || n_cand > E || !tris || !vstart || !vcorner || !edge_keys || !keys || !cand || !vkey || !selected || !d_count) {
        set_error("mirres_dec_select: bad argument (V %d, T %d, E %d, %d candidates)", V, T, E, n_cand); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MR_HIP(hipMemsetAsync(vkey, 0xFF, sizeof(unsigned long long) * (size_t)V, s));       // above every key
    MR_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
    const int g = grid_for((size_t)n_cand, DEC_BLOCK);
    k_dec_claim<<<g, DEC_BLOCK, 0, s>>>(tris, V, vstart, vcorner, edge_keys, E, keys, cand, n_cand, vkey);
    k_dec_select<<<g, DEC_BLOCK, 0, s>>>(tris, V, vstart, vcorner, edge_keys, E, keys, cand, n_cand, vkey, selected, d_count);
    MR_LAUNCH_CHECK("dec_select");
    return MIRRES_OK;
}

extern "C" int mirres_dec_apply(float* verts, double* quadrics, int V, int32_t* tris, int T, const unsigned long long* edge_keys, int E, const float* position,
                                const int32_t* cand, const uint8_t* selected, int n_cand, int32_t* remap, uint8_t* keep_face, uint8_t* used_vertex, const int32_t* d_count,
                                int* h_selected, void* stream) {
    if (!dec_sizes_ok(V, T) || E <= 0 || n_cand <= 0 || n_cand > E || !verts || !quadrics || !tris || !edge_keys || !position || !cand || !selected || !remap || !keep_face ||
        !used_vertex || !d_count || !h_selected) {
        set_error("mirres_dec_apply: bad argument (V %d, T %d, E %d, %d candidates)", V, T, E, n_cand); return MIRRES_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MR_HIP(hipMemsetAsync(used_vertex, 0, (size_t)V, s));
    k_dec_iota<<<grid_for((size_t)V, DEC_BLOCK), DEC_BLOCK, 0, s>>>(remap, V);
    k_dec_apply_edges<<<grid_for((size_t)n_cand, DEC_BLOCK), DEC_BLOCK, 0, s>>>(verts, quadrics, V, edge_keys, E, position, cand, selected, n_cand, remap);
    k_dec_apply_faces<<<grid_for((size_t)T, DEC_BLOCK), DEC_BLOCK, 0, s>>>(tris, T, V, remap, keep_face, used_vertex);
    MR_LAUNCH_CHECK("dec_apply");
    int32_t h = 0;
    MR_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, s));
    MR_HIP(hipStreamSynchronize(s));
    *h_selected = (int)h;
    return MIRRES_OK;
}
