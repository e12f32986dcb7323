/* mirres.h — C ABI of libmirres.so: the MI355X (gfx950) engine behind the reference's ReSTIR path-tracing
 * operator surface (brabbitdousha/MIRReS-ReSTIR_Nerf_mesh, nerf/renderer_restir.py + nerf/ScreenSpaceReSTIR/...).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name starts with h_; all tensors are contiguous
 *     row-major fp32 / int32 exactly as the reference's torch tensors;
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no host sync) unless stated;
 *   - return value: 0 = ok, negative = MIRRES_E_*; nothing is allocated inside a call except in *_create and on the first
 *     use (or growth) of a pool kept in the context / BVH object: mirres_render's batch pool, the closest-hit redo lists;
 *   - pixelIndex = y * fx + x;  reservoir = (light_data f32[N,3], light_pdf f32[N], M i32[N], weight f32[N]).
 * Each entry point cites the reference interface it replaces (file:line relative to the reference repo).
 */
#ifndef MIRRES_H
#define MIRRES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MIRRES_OK 0
#define MIRRES_E_ARG (-1)
#define MIRRES_E_HIP (-2)
#define MIRRES_E_STATE (-3)

typedef struct mirres_bvh mirres_bvh_t; /* owns the traversal layout + build workspace  */
typedef struct mirres_ctx mirres_ctx_t; /* owns per-frame-size ray queues + tables        */

/* ReSTIR constants: load_m_for_restir defines (renderer_restir.py:151-181) + in-shader #defines
 * (FinalShading.slang:7-9). max_bounce is a runtime parameter here (BASELINE config 5).                    */
typedef struct mirres_config {
    int light_tile_count;      /* 128  */
    int light_tile_size;       /* 1024 */
    int screen_tile_size;      /* 8    */
    int initial_light_samples; /* 32   */
    int initial_brdf_samples;  /* 1    */
    int max_history;           /* 20   */
    int neighbor_offset_count; /* 8192 */
    int neighbor_count;        /* 5    */
    float gather_radius;       /* 30   */
    int max_bounce;            /* 2    */
    float vis_near;            /* 0.01 */
} mirres_config_t;
void mirres_default_config(mirres_config_t* cfg);

const char* mirres_version(void);
const char* mirres_last_error(void);

/* ------------------------------------------------------------------ LBVH  (restirbvhWorker, renderer_restir.py:13-94) */
int mirres_bvh_create(mirres_bvh_t** out, int max_tris);
void mirres_bvh_destroy(mirres_bvh_t* bvh);
/* update_mesh + update_bvh (renderer_restir.py:25-94; kernels under nerf/bvhworkers). Writes the reference
 * node arrays LBVHNode_info i32[2T-1,3] / LBVHNode_aabb f32[2T-1,6] and the internal traversal layout.
 * sorted_codes i32[T,2] (code, elementIdx) may be NULL. No host synchronisation.                            */
int mirres_bvh_build(mirres_bvh_t* bvh, const float* vert, int V, const int32_t* tri, int T, int32_t* info, float* aabb,
                     int32_t* sorted_codes, void* stream);
/* Round 6. The private steering hierarchy of the shadow-ray / ordered closest-hit kernels (no reference counterpart: the reference traverses its LBVH as built; any
 * hierarchy over the same leaves gives the same answers) costs 0.2 ms (extended-Morton tree) + 0.9-1.4 ms (binned-SAH top) per build and pays for itself only on a long
 * frame: a caller that rebuilds every frame (render_stage1 does, nerf/renderer.py:975) builds with private_level = 1 and asks for the SAH top when the frame is long
 * enough (renderer_restir.py does: from ~1e8 pixel-samples). private_level: 0 = collapsed reference LBVH, 1 = extended-Morton tree, 2 = + SAH top, 3 = + the
 * lower levels rebuilt by sweep SAH inside every subtree of <= 256 leaves, -1 = MIRRES_PRIVATE_TREE / default 3 (what mirres_bvh_build does). mirres_bvh_upgrade
 * completes a level-1 build to level 3 (pass the arrays of the build call; a no-op on any other level). mirres_bvh_private_level reports which hierarchy stands
 * above the clusters, 0 / 1 / 2 (2 for a level-3 build, as before that level existed); mirres_bvh_tree_level reports the level of the last build, 0 .. 3.  */
int mirres_bvh_build_level(mirres_bvh_t* bvh, const float* vert, int V, const int32_t* tri, int T, int32_t* info, float* aabb,
                           int32_t* sorted_codes, int private_level, void* stream);
int mirres_bvh_upgrade(mirres_bvh_t* bvh, const float* vert, const int32_t* tri, const int32_t* info, const float* aabb, void* stream);
int mirres_bvh_private_level(mirres_bvh_t* bvh);
int mirres_bvh_tree_level(mirres_bvh_t* bvh);
/* bvh_hit / bvh_hit_with_normal (utils/helperDi.slang:197-274, 313-395) over a batch of rays.
 * rays f32[n,8] = (ox,oy,oz,t_min, dx,dy,dz,t_max). mode 0: any-hit (early exit; only `hit` is written),
 * mode 1: closest by exhaustion in the reference's traversal order (hit,t,pos,normal,prim written; NULL skips).
 * mode 2: closest, same outputs bit for bit, via the front-to-back 4-wide fast path + reference-order recomputation of the rays whose
 *         result could depend on the visiting order (t <= 0 hits, exact ties); may grow an internal n-entry buffer on first use.
 * mode 3: occlusion as a conventional ray tracer answers it — some triangle is hit IN FRONT of the origin (t > 0); only `hit` is written.
 *         This is what nerf/render_dump.py:batch_intersector (:8-27) asks of the external `intersector` (intersects_closest(...)[0]).
 * mode 4: closest hit as a conventional ray tracer answers it — the nearest triangle met at t_min < t <= t_max (outputs as mode 1; no counters). The
 *         reference has no such query (its bvh_hit accepts triangles behind the origin); mirres_rasterize casts its near-plane rays with it.
 * counters u32[n,4] (popped, entered-internal, leaves-tested, stack-overflow) may be NULL.                   */
int mirres_bvh_trace(mirres_bvh_t* bvh, const float* rays, int n, int mode, int32_t* hit, float* t, float* pos, float* normal,
                     int32_t* prim, uint32_t* counters, void* stream);

/* ------------------------------------------------------------------ context (load_m_for_restir, renderer_restir.py:148-228) */
int mirres_ctx_create(mirres_ctx_t** out, int fx, int fy, const mirres_config_t* cfg);
void mirres_ctx_destroy(mirres_ctx_t* ctx);
/* createNeighborOffsetTexture (make_sampleable.slang:186-205) / 127 -> f32[count,2]; ctx keeps a copy.      */
int mirres_neighbor_offsets(mirres_ctx_t* ctx, float* out, void* stream);
/* totals since the last reset (host; synchronises): u64[16] = rays_any, rays_closest, then (popped, entered, leaves) of the any-hit
 * kernel and (popped, entered, leaves) of the closest-hit kernel — the node counts only advance while instrument bit 0 is set —
 * [8] / [9] deepest private traversal stack seen by the shadow-ray / ordered closest-hit kernel (instrument bit 0), [10] rays the
 * ordered closest-hit kernel handed to the reference-order kernel (instrument bit 0), [11] private-stack overflows of the
 * shadow-ray kernel (always counted; provably 0, bvh_trace.hip MR_ANY_STACK), [12] shadow rays of the spatial pass that were
 * not traced because the merge cannot see their answer (light reservoir with luminance 0; instrument bit 0; they are
 * included in rays_any), [13..15] shadow-ray kernel, instrument bit 0: wave iterations, wave iterations that ran the leaf
 * branch, leaf records fetched (how often a wave pays for the leaf branch and for how many lanes: bench.py roofline.leaf_branch).
 * A private-stack overflow also sets a sticky flag that makes mirres_render / mirres_bvh_trace return MIRRES_E_STATE afterwards.   */
int mirres_ctx_stats(mirres_ctx_t* ctx, uint64_t* h_out, int reset);
/* instrument bit 0: traversal kernels count visited nodes into the stats (slower kernels); bit 1: every traversal launch is
 * bracketed by HIP events on its own stream so that mirres_ctx_trace_time can report per-kernel durations; bit 2 (with bit 0):
 * shadow rays are counted by the reference-order traversal (bvh_hit's own visits, helperDi.slang:197-274) instead of the
 * production kernel's. Instrumented frames run on one stream.                                                           */
int mirres_ctx_set_instrument(mirres_ctx_t* ctx, int on);
/* sums the event-timed traversal launches since the last call (host; synchronises): ms and launch counts for the any-hit
 * and the closest-hit kernel.                                                                                         */
int mirres_ctx_trace_time(mirres_ctx_t* ctx, double* h_ms_any, int* h_n_any, double* h_ms_closest, int* h_n_closest);

/* ------------------------------------------------------------------ environment light */
/* make_sampleable (GenerateLightTiles.py:4-29 + make_sampleable.slang:34-86). env_tex f32[Hc*Wc,3] is the
 * vertically flipped, flattened map (renderer_restir.py:305-311). Outputs pdf[Hc*Wc], cdf[Hc*(Wc+1)], mpdf[Hc], mcdf[Hc+1]. */
int mirres_env_make_sampleable(const float* env_tex, int Wc, int Hc, float* pdf, float* cdf, float* mpdf, float* mcdf, void* stream);
/* GenerateLightTiles (GenerateLightTiles.py:31-52, GenerateLightTiles.slang:16-62).                          */
int mirres_light_tiles(mirres_ctx_t* ctx, const float* env_tex, int Wc, int Hc, const float* pdf, const float* cdf, const float* mpdf,
                       const float* mcdf, uint32_t frameIndex, float* light_data, int32_t* light_uv, float* light_inv_pdf, void* stream);

typedef struct mirres_env { const float* tex; int Wc, Hc; const float *pdf, *cdf, *mpdf, *mcdf; } mirres_env_t;
typedef struct mirres_gbuf { const float *occ, *pos, *normal_depth, *brdf, *ray_dir; } mirres_gbuf_t; /* [N],[N,3],[N,4],[N,3],[N,3] */
typedef struct mirres_res { float* light_data; float* light_pdf; int32_t* M; float* weight; } mirres_res_t;

/* ------------------------------------------------------------------ reservoir passes */
/* restirbvhWorker.InitialResampling_ (renderer_restir.py:96-114; InitialResampling.slang:151-295)            */
int mirres_restir_initial(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const mirres_env_t* env, const mirres_gbuf_t* g, const mirres_res_t* res,
                          const float* light_data, const float* light_inv_pdf, uint32_t frameIndex, void* stream);
/* TemporalResampling (Resampling.py:26-45; TemporalResampling.slang:23-135). motion may be NULL (= zeros).   */
int mirres_restir_temporal(mirres_ctx_t* ctx, const mirres_env_t* env, const mirres_gbuf_t* g, const mirres_gbuf_t* prev_g,
                           const mirres_res_t* res, const mirres_res_t* prev_res, const float* motion, uint32_t frameIndex, void* stream);
/* restirbvhWorker.SpatialResampling_ (renderer_restir.py:116-131; SpatialResampling.slang:178-322)           */
int mirres_restir_spatial(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const mirres_env_t* env, const mirres_gbuf_t* g, const mirres_res_t* res,
                          const mirres_res_t* prev_res, const float* neighbor_offsets, uint32_t frameIndex, void* stream);
/* restirbvhWorker.EvaluateFinalSamples_get_vis (renderer_restir.py:133-146; EvaluateFinalSamples.slang:84-124) */
int mirres_restir_final_vis(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const float* pos, const mirres_res_t* res, float* vis_map, void* stream);
/* EvaluateFinalSamples_di.forward/backward (Resampling.py:94-143; EvaluateFinalSamples.slang:129-188)        */
int mirres_restir_eval_final(mirres_ctx_t* ctx, const mirres_env_t* env, const mirres_res_t* res, const float* vis_map, float* final_dir,
                             float* final_dist, float* final_Li, void* stream);
int mirres_restir_eval_final_bwd(mirres_ctx_t* ctx, const mirres_env_t* env, const mirres_res_t* res, const float* vis_map,
                                 const float* grad_final_Li, float* grad_env /*[Hc*Wc,3], accumulated*/, void* stream);

/* ------------------------------------------------------------------ shading / path tracing */
/* FinalShading.forward/backward (Resampling.py:145-214; FinalShading.slang:14-109)                           */
int mirres_final_shading(mirres_ctx_t* ctx, const mirres_env_t* env, const float* occ, const float* normal, const float* ray_dir,
                         const float* kd, const float* rough_metal, const float* final_dir, const float* final_dist, const float* final_Li,
                         float* color, float* diff_light, float* spec_light, void* stream);
int mirres_final_shading_bwd(mirres_ctx_t* ctx, const float* occ, const float* normal, const float* ray_dir, const float* kd,
                             const float* rough_metal, const float* final_dir, const float* final_dist, const float* final_Li,
                             const float* g_color, const float* g_diff, const float* g_spec, float* g_normal, float* g_kd,
                             float* g_rough_metal, float* g_final_Li, void* stream);
typedef struct mirres_path {
    const float *occ, *pos, *normal, *ray_dir, *kd, *rough_metal; /* vertex inputs                              */
    float* prd;                                                   /* f32[N,5] throughput rgb, specularBounce, stop */
    float *new_pos, *new_ray_d, *new_occ, *new_normal;            /* next-vertex outputs                        */
    int32_t* new_prim;   /* i32[N] or NULL (no write): the mesh triangle of the next vertex, -1 where new_occ = 0 (what a textured material looks up) */
} mirres_path_t;
/* process_new_dir_for_pt (Resampling.py:216-232; FinalShading.slang:113-265)                                  */
int mirres_pt_new_dir(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const mirres_path_t* p, uint32_t frameIndex, uint32_t bounce_count, void* stream);
/* indirect_one_hit_divided_no_grad (Resampling.py:254-273; FinalShading.slang:641-1009). When acc_* are non-NULL
 * the results are ADDED to them instead of overwriting color/diff/spec (fuses renderer_restir.py:420-422).     */
int mirres_pt_bounce(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const mirres_env_t* env, const mirres_path_t* p, uint32_t frameIndex,
                     uint32_t bounce_count, float* color, float* diff_color, float* spec_color, void* stream);

/* ------------------------------------------------------------------ denoiser */
/* EAWDenoise_run.forward / EAWDenoise_run_no_di (Denoising.py:10-60; EAWDenoise.slang:50-302)                 */
int mirres_eaw(int fx, int fy, int step_width, float c_phi, float n_phi, float p_phi, const float* occ, const float* color,
               const float* normal, const float* pos, float* out, void* stream);
/* process_normal_ao (EAWDenoise.slang:591-651, launched at nerf/renderer.py:1153-1158 when --lambda_extra_kd > 0): per foreground pixel the weight
 * clamp(50 (1 - mean over the 8 x 8 window's foreground pixels of clamp(n_q . n_p, 0, 1)), 0, 1) written to the three channels of out_ao f32[N,3];
 * background pixels get 0. ray_dir is an argument of the reference kernel that it never reads and is not taken here.                             */
int mirres_normal_ao(int fx, int fy, const float* occ, const float* normal, float* out_ao, void* stream);
/* EAWDenoise_run.backward (Denoising.py:30-48): grads w.r.t. colour, normal and position are ACCUMULATED.      */
int mirres_eaw_bwd(int fx, int fy, int step_width, float c_phi, float n_phi, float p_phi, const float* occ, const float* color,
                   const float* normal, const float* pos, const float* grad_out, float* g_color, float* g_normal, float* g_pos, void* stream);
/* The same adjoint computed as a gather (two passes, no atomics, deterministic; scratch4 f32[N,4] is overwritten). The three gradient buffers are
 * accumulated into like mirres_eaw_bwd's.                                                                                                      */
int mirres_eaw_bwd_gather(int fx, int fy, int step_width, float c_phi, float n_phi, float p_phi, const float* occ, const float* color, const float* normal,
                          const float* pos, const float* grad_out, float* scratch4, float* g_color, float* g_normal, float* g_pos, void* stream);

/* bilateral_denoiser (nerf/renderutils/ops.py:173-211; c_src/denoising.cu:14-130): the alternative denoiser of run_restir_di_with_pt
 * (--use_bi_de, renderer_restir.py:529-541). sigma = max(2 * factor, 1e-4); window radius 2 ceil(2.5 sigma) + 1. col f32[N,3],
 * nrm f32[N,3] (normalised inside: safe_normalize, ops.py:168), zdz f32[N,2] = (z, |dz|); out f32[N,4] = (sum w col, max(sum w, 1e-4)) —
 * the caller divides (ops.py:198). scratch f32[N,8] is overwritten.                                                              */
int mirres_bilateral(int fx, int fy, float sigma, const float* col, const float* nrm, const float* zdz, float* scratch, float* out4, void* stream);
/* _bilateral_denoiser_func.backward (ops.py:181-185): col_grad f32[N,3] from grad_out f32[N,4] (its 4th channel carries no gradient to col). */
int mirres_bilateral_bwd(int fx, int fy, float sigma, const float* nrm, const float* zdz, const float* grad_out4, float* scratch, float* col_grad,
                         void* stream);

/* dump_render (nerf/render_dump.py:84-133) = dump_render_run_mesh (:136-215) + GGX_specular (:32-65) + get_light_rgbs (:70-82) +
 * batch_intersector (:8-27): the reference's direct-lighting renderer without ReSTIR (`--use_brdf` alone, nerf/renderer.py:1131-1149;
 * BASELINE configs[0]). n surface points (pos, normal, albedo, roughness, fresnel, rays_d: f32[n,3] each; roughness / fresnel are the
 * 3-channel repeats of renderer.py:1134-1135), env_map f32[env_h,env_w,3], the fixed light set of generate_envir_map_dir
 * (nerf/render_helper.py:8-26): light_dirs f32[L,3], light_area_weight f32[L] (may be NULL when equal_areas != 0 — sample_method
 * 'stratifed_sample_equal_areas'). Occlusion = mode 3 of mirres_bvh_trace from pos + 0.001 dir for every light with clamped cosine > 1e-6.
 * light_rgbs f32[L,3] receives get_light_rgbs; out_rgb (clamped to [0,1] when clamp_rgb, as dump_render does), out_diff, out_spec f32[n,3].
 * Works through the points in chunks of <= 2^24 (point, light) pairs; the chunk's ray pool (40 B per pair) is kept in the BVH object.  */
int mirres_dump_render(mirres_bvh_t* bvh, int n, int L, const float* pos, const float* normal, const float* albedo, const float* roughness,
                       const float* fresnel, const float* rays_d, const float* env_map, int env_h, int env_w, const float* light_dirs,
                       const float* light_area_weight, int equal_areas, int clamp_rgb, float* light_rgbs, float* out_rgb, float* out_diff,
                       float* out_spec, void* stream);

/* The step in front of the path: what render_stage1 gets from nvdiffrast (an un-vendored dependency of the reference).
 * mirres_raster_raycast stands in for dr.rasterize (nerf/renderer.py:983): primary rays f32[n,8] (as mirres_bvh_trace) are cast through the BVH
 * (closest hit) and rast f32[n,4] receives nvdiffrast's raster record (u, v, t, triangle_id + 1), zeros where nothing is hit; vert f32[V,3] /
 * tri i32[T,3] are the arrays the BVH was built from. mirres_interpolate(_bwd) = dr.interpolate without attribute derivatives (:985, :996,
 * :998): out f32[n,C] = u a[i0] + v a[i1] + (1-u-v) a[i2] (0 where triangle_id = 0); the backward ACCUMULATES into g_attr f32[V,C] and writes
 * g_uv f32[n,2] (either may be NULL). dr.texture and dr.antialias are not provided.                                                      */
int mirres_raster_raycast(mirres_bvh_t* bvh, const float* rays, int n, const float* vert, const int32_t* tri, float* rast, void* stream);
/* dr.rasterize(glctx, pos_clip, tri, (H, W)) itself (nerf/renderer.py:983; with rast_db as :1074 hands it to dr.interpolate): h_mvp = HOST float[16],
 * row-major, clip = mvp * (world, 1) — the matrix behind pos_clip = pad(vertices) @ mvp^T (:981), a perspective projection; h_eye = HOST float[3], the
 * world-space point with x_c = y_c = w_c = 0 (the eye: every pixel's line passes through it).  Pixel (ix, iy) of the W x H
 * image looks along NDC ((2 ix + 1) / W - 1, (2 iy + 1) / H - 1); its world-space line is cast through the BVH (the world-space vert / tri it was built
 * from).  rast f32[H*W,4] = (u, v, z/w, triangle_id + 1) with perspective-correct barycentrics (weights of v0, v1) and the clip-space depth of the hit;
 * rast_db f32[H*W,4] = (du/dX, du/dY, dv/dX, dv/dY) per pixel, or NULL.  The ray starts on the near plane (what lies in front of it is clipped away and hides nothing); hits beyond the far plane give an empty record.   */
int mirres_rasterize(mirres_bvh_t* bvh, const float* vert, const int32_t* tri, const float* h_mvp, const float* h_eye, int W, int H,
                     float* rast, float* rast_db, void* stream);
int mirres_interpolate(const float* attr, int C, const float* rast, const int32_t* tri, int n, float* out, void* stream);
int mirres_interpolate_bwd(const float* attr, int C, const float* rast, const int32_t* tri, int n, const float* g_out, float* g_attr, float* g_uv, void* stream);
/* dr.texture(tex, uv, filter_mode='linear', boundary_mode='clamp') (nerf/renderer.py:1004, 1008: the jittered taps of the smoothness
 * regularisers): tex f32[H,W,C], uv f32[n,2] in [0,1] (texel centres at (i + 0.5) / W) -> out f32[n,C]; the backward ACCUMULATES into g_tex. */
int mirres_texture2d(const float* tex, int H, int W, int C, const float* uv, int n, float* out, void* stream);
int mirres_texture2d_bwd(int H, int W, int C, const float* uv, int n, const float* g_out, float* g_tex, void* stream);
/* Texture bake of the stage-1 mesh export (nerf/renderer.py:319-462 `_export_obj`, called per cascade by :464-476; Trainer.export_stage1,
 * nerf/utils.py:1271-1281), csrc/bake.hip.  H x W is the SSAA bake grid (h0 * ssaa, w0 * ssaa); texel (row r, col c) has its centre at UV
 * ((c + 0.5) / W, (r + 0.5) / H), the row growing with v (dr.rasterize on uv * 2 - 1 at (h, w), :357).  All four only enqueue work.
 *
 * mirres_uv_rasterize (:352-357): uv f32[n_uv,2], ft i32[T,3] (T < 2^24: the id is stored in fp32) -> rast f32[H*W,4] = (b0, b1, 0, triangle_id + 1),
 * zeros where nothing covers the centre — the record mirres_interpolate reads (:358-359).  Coverage is exact integer arithmetic: vertices snapped to
 * 1/256 texel (floor(u W 256 + 0.5)), int64 edge functions at the texel centres, a centre on an edge taken by one side (top-left rule), both windings,
 * zero-area / non-finite / out-of-range triangles cover nothing, the lowest triangle index wins where triangles overlap.  scratch = a device buffer
 * of mirres_uv_rasterize_scratch(T) bytes (-1 when T is out of range).                                                                        */
long long mirres_uv_rasterize_scratch(int T);
int mirres_uv_rasterize(const float* uv, int n_uv, const int32_t* ft, int T, int W, int H, float* rast, void* scratch, long long scratch_bytes, void* stream);
/* (:390-398) feats6 f32[n,6] of the covered texels index i32[n] (linear texel index) -> out0 / out1 u8[H*W*3] (channels 0-2 / 3-5): clip to
 * [0, 1], linear_to_srgb_np (nerf/utils.py:60, pow of the device library), x 255, truncated; 0 at every texel not listed.                     */
int mirres_bake_quantise(const float* feats6, const int32_t* index, int n, int W, int H, uint8_t* out0, uint8_t* out1, void* stream);
/* (:400-414) mask u8[H*W] (nonzero = covered), in0 / in1 u8[H*W*3] -> out0 / out1: covered texels keep their bytes; a texel within L1 distance
 * `radius` (<= 32) of the mask (binary_dilation, `radius` iterations, minus the mask) copies the bytes of its Euclidean-nearest covered texel —
 * what the kd-tree over the 3-texel band returns (that texel lies on the band); ties go to the smallest (d^2, row, col); everything else is 0.
 * scratch_dy = device i8[H*W].                                                                                                           */
int mirres_texture_inpaint(int W, int H, int radius, const uint8_t* mask, const uint8_t* in0, const uint8_t* in1, int8_t* scratch_dy,
                           uint8_t* out0, uint8_t* out1, void* stream);
/* (:420-422) cv2.resize(INTER_LINEAR) of in u8[H*W*3] to (W / ssaa) x (H / ssaa) (both divisible): odd ssaa the centre texel, even ssaa the mean of
 * the 2 x 2 centre texels rounded half up.                                                                                                */
int mirres_texture_downsample(int W, int H, int ssaa, const uint8_t* in, uint8_t* out, void* stream);
/* Chart atlas of the stage-1 mesh export (export.chart_atlas; csrc/atlas.hip; DESIGN.md section 5.7 "Chart atlas"): xatlas in the reference (nerf/renderer.py:334-347), here
 * charts of faces that look along one coordinate axis, projected along it.  verts f32[V,3], tris i32[T,3] (T < 2^24); all pointers are device memory (NULL allowed
 * where the count is 0); all calls only enqueue work; no floating-point number is added atomically: equal inputs give equal bytes.
 * Buckets: k = 0..5 = +x, -x, +y, -y, +z, -z; (U, V) of a bucket = the coordinates (y,z) (z,y) (z,x) (x,z) (x,y) (y,x): (U, V, d_k) is right-handed.
 *
 * mirres_atlas_classify: normal f32[T,3] = cross(v1 - v0, v2 - v0) in fp32, e1 = v1 - v0, e2 = v2 - v0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 * every difference and product rounded once; bucket i32[T] = the k with the largest n . d_k (the largest |component| with its sign), ties to the lowest k.
 * A face is DEGENERATE (bucket -1, normal 0) when an index is outside [0, V) or repeated, a vertex coordinate or a normal component is not finite, or n = 0.  */
int mirres_atlas_classify(const float* verts, int V, const int32_t* tris, int T, float* normal, int32_t* bucket, void* stream);
/* One Jacobi round of relabelling, bucket_in -> bucket_out (different buffers): nbr i32[T,3] = the face across edge (v_k, v_k+1) when exactly two face corners
 * carry that edge, else -1.  Bucket k is ELIGIBLE for a face when n . d_k > 0 and (n . d_k)^2 >= cos_min^2 ((nx^2 + ny^2) + nz^2), evaluated in fp64 on the
 * fp32 normal (squares exact, the two sums and the product rounded once); cos_min in [0, 1].  Votes: the face's own bucket 1.5, each neighbour's bucket 1
 * (a degenerate neighbour none), counted for eligible buckets only.  The face takes the bucket with the most votes; its own when that is among the tied or
 * when nothing received a vote, else the lowest tied k.  A degenerate face stays -1.                                                              */
int mirres_atlas_smooth(const float* normal, const int32_t* bucket_in, const int32_t* nbr, int T, float cos_min, int32_t* bucket_out, void* stream);
/* bounds f32[n_charts,4] = (min U, min V, max U, max V) over the three vertices of every face f with chart[f] in [0, n_charts) and a bucket in 0..5 (the projection
 * is bucket[f]'s: all faces of a chart hold one bucket), by atomicMin / atomicMax on the order-preserving integer image of the float (so -0 < +0); the
 * coordinates are selected, not computed.  A chart without such a face gets NaN.  Faces with chart -1 take no part.                               */
int mirres_atlas_bounds(const float* verts, int V, const int32_t* tris, int T, const int32_t* bucket, const int32_t* chart, int n_charts, float* bounds, void* stream);
/* vt f32[n_uv,2]: UV vertex i is mesh vertex uv_vertex[i] in chart c = uv_chart[i] (one per pair: a chart's interior edges share both UV vertices):
 * u = ((origin[c].x + 0.5) + (U - bounds[c].minU) * density) / w0, v likewise with V, minV, origin[c].y, h0 — in fp32: the subtraction, the multiplication,
 * the addition and the division each rounded once ((origin + 0.5) is exact).  origin i32[n_charts,2] = the chart rectangle's first export texel (column, row),
 * chart_bucket i32[n_charts]; the rectangle is ceil((max - min) * density) + 1 texels a side (the same fp32 subtraction and product), so the geometry sits
 * half a texel inside it.  A pair that names no chart or no vertex gets NaN (such a triangle covers nothing).                                      */
int mirres_atlas_emit(const float* verts, int V, const int32_t* uv_chart, const int32_t* uv_vertex, int n_uv, const int32_t* chart_bucket, const float* bounds,
                      const int32_t* origin, int n_charts, float density, int w0, int h0, float* vt, void* stream);
/* The overlap check on the W x H bake grid with the coverage rule of mirres_uv_rasterize (shared code: 1/256-texel snap, int64 edge functions, top-left rule),
 * over the same balanced (triangle, 32-texel chunk) work items.  Pass 1: every triangle marks the centres it covers, one bit per texel (atomicOr); a centre found
 * marked is recorded in a second bit plane.  Pass 2: flagged u8[n_charts + 1]: [c] = 1 when a triangle of chart c = face_chart[t] covers a centre covered more
 * than once, [n_charts] likewise for the triangles of no chart (face_chart -1); 0 otherwise.  Every chart that takes part in an overlap is flagged, whatever
 * the order the triangles ran in.  scratch: mirres_atlas_verify_scratch(T, W, H) device bytes (-1 when out of range; grid limits as mirres_uv_rasterize). */
long long mirres_atlas_verify_scratch(int T, int W, int H);
int mirres_atlas_verify(const float* vt, int n_uv, const int32_t* ft, int T, const int32_t* face_chart, int n_charts, int W, int H, uint8_t* flagged,
                        void* scratch, long long scratch_bytes, void* stream);
/* dr.antialias (nerf/renderer.py:1184-1206; nvdiffrast is un-vendored: the published algorithm, csrc/antialias.hip): color f32[H*W,C], rast f32[H*W,4]
 * (mirres_raster_raycast's record: .z orders the two triangles of a pixel pair by distance, .w = triangle id + 1), pos_clip f32[V,4] clip-space
 * vertex positions (pixel (i, j)'s centre is NDC ((2i + 1) / W - 1, (2j + 1) / H - 1)), tri i32[T,3], opp i32[T,3] the vertex across each edge
 * (v_k, v_k+1) in the neighbouring triangle or -1 (topology: depends on `tri` only).  out f32[H*W,C], written without atomics (deterministic).
 * _bwd: g_color f32[H*W,C] (overwritten) and / or g_pos f32[V,4] (ACCUMULATED with atomics; scaled by pos_gradient_boost); either may be NULL. */
int mirres_antialias(int W, int H, int C, const float* color, const float* rast, const float* pos_clip, const int32_t* tri, const int32_t* opp,
                     float* out, void* stream);
int mirres_antialias_bwd(int W, int H, int C, const float* color, const float* rast, const float* pos_clip, const int32_t* tri, const int32_t* opp,
                         const float* g_out, float* g_color, float* g_pos, float pos_gradient_boost, void* stream);

/* prepare_shading_normal (nerf/renderutils/ops.py:100-163; c_src/normal.cu): the shading normal render_stage1 hands to the path
 * (nerf/renderer.py:1013). All inputs f32[n,3] (broadcast inputs expanded by the caller); out f32[n,3]. The backward writes the six input
 * gradients (any may be NULL).                                                                                                   */
int mirres_prepare_shading_normal(long long n, const float* pos, const float* view_pos, const float* perturbed_nrm, const float* smooth_nrm,
                                  const float* smooth_tng, const float* geom_nrm, int two_sided_shading, int opengl, float* out, void* stream);
int mirres_prepare_shading_normal_bwd(long long n, const float* pos, const float* view_pos, const float* perturbed_nrm, const float* smooth_nrm,
                                      const float* smooth_tng, const float* geom_nrm, int two_sided_shading, int opengl, const float* dout,
                                      float* g_pos, float* g_view_pos, float* g_perturbed_nrm, float* g_smooth_nrm, float* g_smooth_tng,
                                      float* g_geom_nrm, void* stream);

/* ------------------------------------------------------------------ material field (MLPTexture3D, render_helper.py:53-124) */
typedef struct mirres_matnet {
    const uint16_t* grid_f16; /* fp16 hash-grid table, 6 299 960 x 2 entries (tcnn layout)                      */
    const float *w0, *w1, *w2; /* torch Linear weights [32,32],[32,32],[6,32], row-major [out,in]                */
    float aabb_min[3], aabb_max[3], out_min[6], out_max[6];
} mirres_matnet_t;
int mirres_matnet_grid_entries(void);                      /* 6 299 960                                        */
int mirres_matnet_pack_grid(const float* params_f32, uint16_t* grid_f16, int64_t n, void* stream);
/* MLPTexture3D.sample / sample_no_di: pos f32[n,3] -> out f32[n,6]; enc_out (fp16 bits [n,32]) may be NULL.     */
int mirres_matnet_fwd(const mirres_matnet_t* m, const float* pos, int n, float* out, uint16_t* enc_out, void* stream);
/* _MLP.forward on precomputed encodings (render_helper.py:43-44, 100-104): enc fp16 bits [n,32] -> out f32[n,6] (sigmoid + range applied).
 * The MFMA-tiled kernel (v_mfma_f32_32x32x2_f32, sixteen K = 2 steps per layer in ascending k: the fp32 fmaf chain of mirres_matnet_fwd, bit for bit). */
int mirres_matnet_mlp(const mirres_matnet_t* m, const uint16_t* enc, int n, float* out, void* stream);
/* renderer_restir.py:398-408 fused: evaluate where occ>=0.5 and scatter kd / (roughness, metallic) in place.    */
int mirres_matnet_scatter(const mirres_matnet_t* m, const float* occ, const float* pos, int n, float* kd, float* rough_metal,
                          int use_scale, const float* h_scale3, void* stream);
/* backward of sample(): grads to the fp32 master grid (atomic, accumulated), the MLP weights (accumulated) and, when g_pos != NULL,
 * the sample positions f32[n,3] (overwritten; tcnn's HashGrid input gradient x 1/(aabb_max-aabb_min), zero where the clamp to the
 * AABB is active - render_helper.py:93-98).                                                                       */
int mirres_matnet_bwd(const mirres_matnet_t* m, const float* pos, int n, const float* grad_out, float* g_params_f32, float* g_w0,
                      float* g_w1, float* g_w2, float* g_pos, void* stream);

/* ------------------------------------------------------------------ textured material (the exported stage-1 asset, nerf/renderer.py:390-398; csrc/texmat.hip)
 * The render mesh verts f32[V,3] / tris i32[T,3] (what the BVH was built from), per-corner UVs ft i32[T,3] into vt f32[Nt,2] in the reference's convention
 * (v = 1 - v' of the OBJ).  Cascade c owns the triangles [tri_end[c-1], tri_end[c]) (tri_end[-1] = 0, tri_end[n_cas-1] = T, n_cas <= 8) and the W[c] x H[c]
 * texel plane texels[c]: 8 bytes per texel, row-major, row 0 = smallest v, bytes (feat0 R, G, B, feat1 G, feat1 B, 0, 0, 0) = (kd.rgb, roughness, metallic)
 * as 8-bit sRGB.  decode f32[256] maps every byte to linear (q -> srgb_to_linear(q / 255)); decoded roughness is clamped to [rough_min, 1].
 * Lookup of a point p on triangle prim, every operation one correctly rounded fp32 operation in this order, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z:
 *   e1 = v1 - v0, e2 = v2 - v0, d = p - v0;  d00 = dot(e1,e1), d01 = dot(e1,e2), d11 = dot(e2,e2), d20 = dot(d,e1), d21 = dot(d,e2);
 *   den = d00 d11 - d01 d01;  b1 = (d11 d20 - d01 d21) / den;  b2 = (d00 d21 - d01 d20) / den;  b0 = (1 - b1) - b2;
 *   uv = (b0 uv0 + b1 uv1) + b2 uv2;  x = fmax(fmin(u W - 0.5, W), -1), y = fmax(fmin(v H - 0.5, H), -1) (a NaN becomes the bound);
 *   i = floor(x), fx = x - i; taps at columns clamp(i, 0, W-1) and clamp(i+1, 0, W-1), rows likewise (clamp to the edge);
 *   per channel, decoded taps t00, t10 (row j), t01, t11 (row j+1): a = t00 + fx (t10 - t00), b = t01 + fx (t11 - t01), out = a + fy (b - a).
 * mirres_texmat_lookup: occ f32[n] (NULL = all 1), prim i32[n], pos f32[n,3] -> kd f32[n,3], rough_metal f32[n,2] with the row rules of
 * mirres_matnet_scatter: only rows with occ >= 0.5 are written (kd scaled by h_scale3 when use_scale), and with use_scale the kd of EVERY row is
 * then clamped to [0, 1]; an occupied row whose prim lies outside [0, T) is the caller's error and is left unwritten.                        */
typedef struct mirres_texmat {
    const float* verts; const int32_t* tris;
    const float* vt; const int32_t* ft;
    int n_cas; int tri_end[8];
    int W[8], H[8]; const void* texels[8];
    const float* decode;
    float rough_min;
} mirres_texmat_t;
int mirres_texmat_lookup(const mirres_texmat_t* t, const float* occ, const int32_t* prim, const float* pos, int n, float* kd, float* rough_metal,
                         int use_scale, const float* h_scale3, void* stream);

/* ------------------------------------------------------------------ albedo evaluation (the reference's albedo_eval.py; csrc/albedo.hip)
 * The TensoIR protocol aligns the predicted albedo to the ground truth by one scale per channel before scoring it, and the same three numbers are the
 * --albedo_scale_x/y/z of the relighting commands.  pred f32[n,3] is a view's albedo, gt_rgba f32[n,4] its ground truth (diffuse-color.exr); a pixel is
 * masked in iff double(alpha) >= mask_thr (albedo_eval.py:94-95 clears the mask where alpha < thr).  scratch = a device buffer of
 * MIRRES_ALBEDO_SCRATCH_BYTES bytes (one per stream in use).  All three only enqueue work; results are the same bits on every run.
 *
 * mirres_albedo_compact (:93-111): appends the masked-in (pred, gt rgb) pairs of one view, in pixel order, to pool_pred / pool_gt f32[pool_cap,3].
 * state u64[3] (device, zeroed by the caller before the first view): [0] pairs in the pool (where the append starts; advanced by the kept count),
 * [1] kept pixels so far with a ground-truth channel > 1 (:98-100 raises on them; the caller reads it after each view), [2] set when the pool was too
 * small — pairs beyond pool_cap are dropped and [0] stops at pool_cap (the caller sizes the pool for [0] + n beforehand; the flag stays set until the
 * caller clears it).  Only KEPT pixels are tested against 1: the script takes the maximum over the whole image before masking (:98), so a file it
 * refuses for a value above 1 outside the mask is accepted here.
 * mirres_albedo_median (:116-118): out3 f64[3] = np.median(float64(gt) / float64(pred).clip(min=1e-6), axis=0) over the first `count` pairs, exactly
 * (fp64 division is correctly rounded; an even count gives (a + b) / 2 of the two middle values; one NaN ratio makes its channel NaN).  count <= 0 is
 * MIRRES_E_ARG: an empty pool has no median.  Both pools 16-byte aligned, count < 2^40.
 * mirres_albedo_score (:142-172): masked pixels pred * h_scale3 (host f64[3], NULL = 1) in fp64, unmasked pixels of both images 1, prediction clipped
 * to [0, 1]  ->  out_sums2 f64[2] = the sums over the n * 3 values of (gt - now)^2 and of (gt^(1/2.2) - now^(1/2.2))^2 (fixed summation order; the
 * script rounds the two gamma images to fp32 before that difference, this sum keeps fp64), and out_pred_u8 / out_gt_u8 u8[n,3] (either may be NULL) =
 * the gamma images x 255, truncated.                                                                                                              */
#define MIRRES_ALBEDO_SCRATCH_BYTES 32768
long long mirres_albedo_scratch_bytes(void);               /* MIRRES_ALBEDO_SCRATCH_BYTES of the library that is loaded: bindings size the buffer by this */
int mirres_albedo_compact(const float* pred, const float* gt_rgba, long long n, double mask_thr, float* pool_pred, float* pool_gt, long long pool_cap,
                          unsigned long long* state, void* scratch, void* stream);
int mirres_albedo_median(const float* pool_pred, const float* pool_gt, long long count, double* out3, void* scratch, void* stream);
int mirres_albedo_score(const float* pred, const float* gt_rgba, long long n, double mask_thr, const double* h_scale3, double* out_sums2,
                        uint8_t* out_pred_u8, uint8_t* out_gt_u8, void* scratch, void* stream);

/* ------------------------------------------------------------------ whole frame: run_restir_di_with_pt (renderer_restir.py:473-550) */
typedef struct mirres_render_args {
    int spp; uint32_t random_offset; /* np.random.randint(2**20) in the reference (renderer_restir.py:245)     */
    int use_scale; float scale[3];
    const float* env_map; int Wc, Hc; /* f32[Hc,Wc,3] as passed by the caller (not flipped)                     */
    float* occ;                       /* f32[N]   modified in place (renderer_restir.py:484-485)                */
    const float *normal, *depth, *kd, *rough_metal, *ray_dir, *pos;
    const mirres_matnet_t* mat;       /* NULL -> const_kd / const_rm at indirect hits                           */
    float const_kd[3], const_rm[2];
    int denoise_iter, step_width; float c_phi, n_phi, p_phi;
    float* outs[6];                   /* final_color, den_diffuse, den_spec, den_indirect, den_indirect_diff, den_indirect_spec */
    float* tape;                      /* f32[samples, N, 8] or NULL: per sample and pixel the final (spatially merged) reservoir and its visibility
                                         {light_data.xyz inv_pdf | M weight vis 0}, what mirres_render_bwd differentiates through        */
    const float* gb_depth;            /* f32[N,2] (z, |dz|) or NULL: non-NULL selects the bilateral denoiser with factor 2 (:529-541) instead of EAW */
    int spp_begin, spp_end;           /* multi-GPU spp sharding: render samples [spp_begin, spp_end) and skip the
                                         average/denoise/composite (raw sums are left in outs[0..5]); 0,0 = all  */
    /* Multi-GPU strip sharding (exact: bit-identical to one GPU for the rows a rank owns). The context is created for the rank's
     * LOCAL frame = its own rows plus up to 30 halo rows (the spatial gather radius) on either side; all per-pixel inputs cover the
     * local frame (which may extend below the image by rows the caller padded with background, occ = 0, so that strips of different
     * heights share a context size). strip_full_fy = height of the whole frame (0 = no strip sharding), strip_y_off = global row of local row 0,
     * [own_y0, own_y1) = the local rows this rank owns. Halo rows are only read (G-buffer, reservoirs); `halo` is called once per
     * sample, on the host while the frame is being enqueued, between temporal and spatial reuse: it must enqueue — on the same
     * stream — the exchange that fills the halo rows of `records` (packed reservoirs, f32[local pixels, 8]) with the neighbouring
     * ranks' own rows and sends this rank's border rows. Like a spp slice, a strip leaves raw sums in outs[0..5].                */
    int strip_full_fy, strip_y_off, own_y0, own_y1;
    int (*halo)(void* user, float* records, int sample, void* stream);
    void* halo_user;
    /* strip_overlap != 0 (round 4; needs `halo`): the spatial pass of every sample runs in two parts. `halo` is called with a SIDE stream (ordered after the
     * temporal pass) and must enqueue the exchange there; meanwhile the caller's stream does the spatial pass of the INTERIOR rows — the own rows at least
     * gather_radius away from a strip edge with a neighbouring rank, whose neighbours are all own rows — and only then waits for the exchange and does the border
     * rows. Same results bit for bit; the exchange leaves the per-sample critical chain at the price of three more launches per sample (and the next sample's
     * temporal merge is not fused into the resolve kernel). Strips too short to have interior rows fall back to the in-line exchange.                       */
    int strip_overlap;
    /* Native exchange (round 6): halo_comm = a communicator of mirres_comm_create, or NULL. When set, mirres_render issues the per-sample exchange itself — for each of
     * the halo_n (<= 2) neighbouring ranks halo_peer[k] one ncclSend of the local rows [halo_send0[k], halo_send1[k]) and one ncclRecv into the local rows
     * [halo_recv0[k], halo_recv1[k]) of the packed reservoirs, inside one ncclGroupStart / ncclGroupEnd on the chain's stream — and `halo` is not called: no Python on
     * the per-sample path (the callback costs 56-63 us of host time per sample in the median over RCCL, 240-330 us in the mean: profiles/r06_halo_host_cost*.txt).
     * halo_time_stride > 0: every halo_time_stride-th exchange is bracketed by events on the stream; mirres_ctx_halo_time sums them (the strip's own busy time =
     * its render time minus the time spent inside the exchanges, which is where a rank waits for its neighbours: dist.StripBalancer).                              */
    void* halo_comm;
    int halo_n, halo_peer[2], halo_send0[2], halo_send1[2], halo_recv0[2], halo_recv1[2];
    int halo_time_stride;
    /* tex != NULL: the material at every indirect hit is looked up in this textured mesh (mirres_texmat_lookup's rule, at the triangle the continuation
     * ray hit); the BVH must have been built from tex->verts / tex->tris.  NULL: mat / const_kd.  Setting both tex and mat is MIRRES_E_ARG.       */
    const mirres_texmat_t* tex;
} mirres_render_args_t;
int mirres_render(mirres_ctx_t* ctx, mirres_bvh_t* bvh, const mirres_render_args_t* a, void* stream);
/* The library's own RCCL communicator for the native halo exchange (no reference counterpart: /root/reference is single-GPU). librccl is dlopen-ed —
 * `librccl_path` (may be NULL / empty) is tried first, the copy already loaded into the process wins. mirres_comm_unique_id: ncclGetUniqueId into 128 bytes (rank 0; the
 * caller distributes them, e.g. with torch.distributed.broadcast); mirres_comm_create: ncclCommInitRank (collective over the `world` ranks, current device);
 * mirres_ctx_halo_time: blocks until the last recorded exchange has finished, returns the summed milliseconds of the bracketed exchanges of the last mirres_render on
 * this context and their number, and forgets them.                                                                                                    */
int mirres_comm_unique_id(const char* librccl_path, void* id128);
int mirres_comm_create(void** comm, const char* librccl_path, const void* id128, int world, int rank);
void mirres_comm_destroy(void* comm);
int mirres_ctx_halo_time(mirres_ctx_t* ctx, double* ms, int* exchanges);
/* Backward of the frame's DIRECT lighting sums w.r.t. what the reference differentiates (EvaluateFinalSamples_di.backward +
 * FinalShading.backward summed over the samples, Resampling.py:116-214): from the cotangents of the three direct sums (total colour,
 * diffuse light, specular light — f32[N,3] each) and the tape of the forward call (`samples` samples), gradients w.r.t. normal [N,3],
 * kd [N,3], (roughness, metallic) [N,2] (overwritten) and the environment texels f32[Hc*Wc,3] in the caller's (unflipped) layout
 * (accumulated). The indirect sums carry no gradient (process_path_tracing_divided_no_grad). `a` = the forward call's arguments.       */
int mirres_render_bwd(mirres_ctx_t* ctx, const mirres_render_args_t* a, int samples, const float* g_color, const float* g_diff,
                      const float* g_spec, float* g_normal, float* g_kd, float* g_rough_metal, float* g_env, void* stream);
/* Sizes the context's batch pool ahead of the first frame (no reference counterpart: load_m_for_restir allocates the reference's persistent buffers at
 * start-up, renderer_restir.py:189-217; here the K-sample pool — ~670 B per sample slot, 55 GB for 32 samples of a 1600 x 1600 frame — would otherwise
 * be allocated inside the first mirres_render of a frame size, a device synchronisation and a multi-GB hipMalloc + clear in the middle of the first
 * timed frame).  samples_per_batch = 0: the default batch (MIRRES_PT_BATCH, 32).  Returns the batch size actually reserved (smaller when the device
 * cannot spare the request) or a negative error code.                                                                                        */
int mirres_ctx_reserve(mirres_ctx_t* ctx, int samples_per_batch);
/* second half of run_restir_di_with_pt (:507-549) on already-summed accumulators (after an all-reduce).         */
int mirres_render_finish(mirres_ctx_t* ctx, const mirres_render_args_t* a, float* sums[6], void* stream);

/* Self-check of the arithmetic the shading kernels are built on (no reference counterpart: the reference relies on nvcc's IEEE division).
 * The shading translation units divide and take square roots with short instruction sequences (csrc/device_math.hpp, mr_div / mr_rcp /
 * mr_sqrt) that must return the bits of the IEEE-754 operations. This runs them against the compiler's correctly rounded `a / b`, `1 / b`
 * and `sqrtf` on the device: every significand pair (a, b) in [1, 2) x S, S = 2^log2_b significands spread over [1, 2) plus the last 256
 * (log2_b = 23: all 2^46 pairs, ~50 s on an MI355X), every reciprocal of [1, 2), and every square root of [1, 4).
 * out[0] = pairs tested, out[1..3] = mismatches of mr_div, mr_rcp, mr_sqrt (all must be 0). Blocks until done.                          */
int mirres_selfcheck_arith(int log2_b, unsigned long long out[4], void* stream);

/* The transcendental functions of the path on the device (no reference counterpart: the reference calls CUDA's math library in
 * utils/lightDi.slang:119-132,181-209,312-330, utils/brdf.slang:76-124, EAWDenoise.slang:50-302, res.slang:53-61; here they are the fixed
 * arithmetic of include/mirres_fmath.h, the same header the CPU oracle includes).  fn: 0 sin, 1 cos, 2 acos, 3 exp, 4 exp2, 5 pow5,
 * 6 x^8, 7 x^128, 8 sigmoid (one argument, `a`); 16 atan2(a, b); 17 b / a with the short division of the shading kernels (mr_div);
 * 18 the short square root (mr_sqrt).
 * mirres_fmath_eval: out[i] = fn(a[i], b[i]) for n device floats (b may be NULL for one-argument functions).
 * mirres_fmath_checksum: over the argument bit patterns first .. first + count - 1 (for fn >= 16 the second argument is a fixed hash of the
 * first), *out = sum of result_bits * (2 * argument_bits + 1) mod 2^64 with NaN results canonical — order-free, so the host can form the same
 * sum from the same header (oracle/fmath_check.cpp) and tests/test_gpu_fmath.py can compare device and host over all 2^32 arguments. Blocks. */
int mirres_fmath_eval(int fn, const float* a, const float* b, float* out, long long n, void* stream);
int mirres_fmath_checksum(int fn, unsigned int first, unsigned long long count, unsigned long long* out, void* stream);

/* ------------------------------------------------------------------ stage-0 mesh extraction (NeRFRenderer.export_stage0, nerf/renderer.py:498-570)
 * Marching cubes over a dense volume vol f32[nx][ny][nz] (every size >= 2, at most 2^31 - 1 points) — mcubes.marching_cubes(sigmas, density_thresh),
 * renderer.py:549-555 — as an indexed mesh: vertices f32[V,3] in index space (the caller maps them with v / (res - 1) * 2 - 1, :553) and triangles
 * i32[T,3].  Non-finite values count as torch.nan_to_num(., 0) makes them (:541); a corner is inside when value >= iso; triangles are wound so that the
 * normal points towards decreasing values (for --sdf the caller passes -vol and iso 0, :549).  Every crossed grid edge carries exactly ONE vertex, at
 * float(i) + clamp((iso - va) / (vb - va), 0, 1) along the edge (va at the lower grid point), numbered in (grid point, axis) order; triangles are numbered in
 * (cell, case table) order: equal inputs give equal bytes.  The 256 cases are generated (scripts/gen_mc_table.py; ambiguous faces SEPARATE their inside corners).
 * mirres_mc_count (renderer.py:549-555): classifies, scans, returns h_counts = {V, T}; BLOCKS until the counts are on the host.  `scratch`: mirres_mc_scratch_bytes
 * device bytes (2 per grid point + 8 per 256 points), handed unchanged to mirres_mc_emit (renderer.py:549-555) together with the same volume and iso; V = T = 0
 * (no crossing) is a success and launches nothing.                                                                                                  */
long long mirres_mc_scratch_bytes(int nx, int ny, int nz);
int mirres_mc_count(const float* vol, int nx, int ny, int nz, float iso, void* scratch, long long scratch_bytes, int* h_counts, void* stream);
int mirres_mc_emit(const float* vol, int nx, int ny, int nz, float iso, const void* scratch, float* verts, int V, int32_t* tris, int T, void* stream);
/* renderer.py:511-515: cascade 0 of density_grid (S^3 values in Morton order, raymarching.cu:73-81: x from bits 0, 3, 6, ..., y from >> 1, z from >> 2; S a power of two
 * <= 1024) -> vol f32[S][S][S].  renderer.py:532-539: vol f32[R][R][R] *= (grid_vol[S][S][S] upsampled by F.interpolate(mode='nearest') > thresh).          */
int mirres_mc_unpack_morton(const float* grid, int S, float* vol, void* stream);
int mirres_mc_mask_nearest(float* vol, int R, const float* grid_vol, int S, float thresh, void* stream);
/* renderer.py:653-655, the outer cascades (cas >= 1) of export_stage0: grid_vol f32[S][S][S] (S a power of two in [2, 1024]) resampled to R^3 (R in [1, 1024]; R < S,
 * R == S and non-integer ratios included) as F.interpolate(mode='trilinear', align_corners=False) does — per axis src = max(scale * (d + 0.5f) - 0.5f, 0) with
 * scale = (float)S / R, i0 = floor(src), i1 = min(i0 + 1, S - 1), l1 = src - i0, l0 = 1 - l1; the eight products summed w inside h inside t; every product and
 * sum one fp32 rounding, zero weights multiplied (a non-finite neighbour makes the value NaN) — then nan_to_num(., 0) and > thresh: occ_out f32[R][R][R] = 1.0f / 0.0f
 * (NaN -> 0, +inf -> 1).  value_out (NULL: not stored) f32[R][R][R] receives the interpolated value itself.                                                     */
int mirres_mc_occupancy_trilinear(const float* grid_vol, int S, int R, float thresh, float* occ_out, float* value_out, void* stream);
/* mark_unseen_triangles (renderer.py:1421-1427): seen[id - 1] = 1 for the triangle id (+ 1, fourth component) of every pixel of rast f32[n,4]; id 0 (background)
 * marks nothing — the reference's mask[-1] += 1 for background pixels is not reproduced.  seen u8[T] is the caller's, cleared by the caller. */
int mirres_mesh_mark_seen(const float* rast, long long n, int T, uint8_t* seen, void* stream);
/* One ring of apply_selection_dilatation (meshutils.py:113-114): a vertex is selected when a selected face uses it (vert_flags u8[V], scratch, cleared inside),
 * then face_out[f] = any of its vertices selected.  face_in and face_out (u8[T]) are different buffers.                                                       */
int mirres_mesh_dilate(const int32_t* tris, int T, int V, const uint8_t* face_in, uint8_t* vert_flags, uint8_t* face_out, void* stream);
/* remove_selected_verts (meshutils.py:159-181) as export_stage0 calls it (renderer.py:663, :676): keep_face[f] = 0 iff some vertex of face f is selected, else 1.
 * box = {xmn, ymn, zmn, xmx, ymx, zmx} (host doubles).  outside = 0 selects x <= xmx && x >= xmn && y ... (the closed box), outside = 1 selects
 * x <= xmn || x >= xmx || y ... (everything not strictly inside).  Coordinates are compared as doubles with the given doubles; a NaN coordinate is selected by
 * neither; a face with an index outside [0, V) is dropped.  The caller compacts with mirres_mesh_compact(keep_face).                                            */
int mirres_mesh_select_box(const float* verts, int V, const int32_t* tris, int T, const double* box, int outside, uint8_t* keep_face, void* stream);
/* meshing_remove_selected_faces + meshing_remove_unreferenced_vertices (meshutils.py:118-121, :195): keeps the faces with keep_face[f] != 0 and the vertices they
 * use, both in their old order, indices remapped.  out_verts f32[V,3] / out_tris i32[T,3] are sized for the input; h_counts = {V', T'}; BLOCKS.  `scratch`:
 * mirres_mesh_scratch_bytes(V, T) device bytes.                                                                                                               */
long long mirres_mesh_scratch_bytes(int V, int T);
int mirres_mesh_compact(const float* verts, int V, const int32_t* tris, int T, const uint8_t* keep_face, float* out_verts, int32_t* out_tris, void* scratch,
                        int* h_counts, void* stream);
/* Connected components over faces that share an EDGE (MeshLab's face-face topology behind meshing_remove_connected_component_by_*, meshutils.py:203-207):
 * sorted_keys u64[n_keys] = the undirected edge keys of all faces in ascending order, key_face i32[n_keys] = the face each belongs to; neighbours in the sorted
 * list with equal keys are joined.  label i32[T] = the smallest face index of the face's component.  Rounds of hooking (atomicMin) + pointer jumping, the host
 * re-launching while the device flag `changed_flag` (i32[1]) is set; max_rounds = 0 means the cap of 64, past which the call returns MIRRES_E_STATE. BLOCKS. */
int mirres_mesh_components(const unsigned long long* sorted_keys, const int32_t* key_face, long long n_keys, int T, int32_t* label, int32_t* changed_flag,
                           int max_rounds, int* h_rounds, void* stream);

/* --------------------------------------------------------------------------------------------------------------------------------------------
 * Quadric-error edge collapse (decimate.hip): decimate_mesh, meshutils.py:64-97, called by export_stage0 at nerf/renderer.py:566-567 — MeshLab's
 * meshing_decimation_quadric_edge_collapse(targetfacenum, optimalplacement) as deterministic rounds of independent collapses (Garland & Heckbert 1997; DESIGN.md
 * section 5.10).  One round is the five calls below in this order (mirres_dec_quadrics in the first round only) plus mirres_mesh_compact; the caller does the
 * sorts between them.  Shared inputs, all device memory, indices in range (the caller checks): verts f32[V,3]; tris i32[T,3]; quadrics f64[V,10], the symmetric
 * 4 x 4 matrix of a vertex as a00 a01 a02 a03 a11 a12 a13 a22 a23 a33; edge_keys u64[E] = the distinct undirected edge keys (min << 32 | max) of all face corners
 * in ascending order — an edge's position in this list is its id — and edge_mult i32[E] how many corners carry each; corner_edge i32[3T] = the edge id of
 * corner 3 f + k, the edge (v_k, v_k+1) of face f; vstart i32[V+1] / vcorner i32[3T] = the corners sorted by their vertex, STABLY (a vertex's corners ascend).
 * Nothing here is a floating-point atomic: equal inputs give equal bytes.
 * mirres_dec_vertex_flags (meshutils.py:64-97): vflag i32[V], bit 0 = on an edge with one face (boundary), bit 1 = on an edge with more than two faces.      */
int mirres_dec_vertex_flags(const unsigned long long* edge_keys, const int32_t* edge_mult, int E, int V, int32_t* vflag, void* stream);
/* mirres_dec_quadrics (meshutils.py:64-97): quadrics[v] = sum over v's corners in CSR order of the face's plane quadric (unit normal, weight = area; a face with
 * a zero cross product adds nothing) followed by, for the face's edges k and k + 2 at that corner where edge_mult == 1, the plane through the edge perpendicular
 * to the face, weight = 1.0 * squared edge length.  fp64 on the fp32 positions.                                                                            */
int mirres_dec_quadrics(const float* verts, int V, const int32_t* tris, int T, const int32_t* vstart, const int32_t* vcorner, const int32_t* corner_edge,
                        const int32_t* edge_mult, int E, double* quadrics, void* stream);
/* mirres_dec_edge (meshutils.py:64-97; optimalplacement as MeshLab's flag): per edge (a, b), Q = Q[a] + Q[b]; position f32[E,3] = the solution of the 3 x 3 system
 * by cofactors rounded to fp32 (optimalplacement == 1 and |det| > 1e-9 * max|entry|^3 and finite), else the cheapest of p_a, p_b, fp32(midpoint), ties in that order;
 * optimalplacement == 2: the cheaper of p_a, p_b only, as MeshLab collapses with optimalplacement off — every vertex of the result is one of the input's
 * (renderer.py:685, the outer meshes), and the low word of a key is the edge id times 0x9E3779B1 mod 2^32 (a bijection: equal costs, which a flat mesh has
 * everywhere, are then ordered without regard to position and a round finds an independent set of useful size; the caller multiplies by the inverse 0x0E8B2F51);
 * cost f64[E] = max(v^T Q v, 0) at that fp32 position; flags i32[E], 0 = valid: 1 multiplicity not 1 or 2, or an end point on an edge with more than two faces;
 * 2 link condition (distinct common neighbours != multiplicity, or both (a, c0, c1) and (b, c0, c1) are faces); 4 interior edge between two boundary vertices;
 * 8 a face around a or b (not both) would turn its normal by acos(0.2) or more or lose its area; 16 cost (as fp32) or position not finite.
 * keys u64[E] = (bits of (float)cost) << 32 | edge id for a valid edge, 0x7FFFFFFFFFFFFFFF otherwise.                                                       */
int mirres_dec_edge(const float* verts, const double* quadrics, int V, const int32_t* tris, int T, const int32_t* vstart, const int32_t* vcorner,
                    const unsigned long long* edge_keys, const int32_t* edge_mult, const int32_t* vflag, int E, int optimalplacement, double* cost,
                    float* position, int32_t* flags, unsigned long long* keys, void* stream);
/* mirres_dec_select (meshutils.py:64-97): cand i32[n_cand] edge ids (the caller's cut: the smallest valid keys).  Every candidate takes the 64-bit atomicMin of
 * its key into vkey u64[V] (scratch, set inside) over its region = a, b and every vertex of a face around a or b; selected u8[n_cand] = 1 where the whole region
 * still holds the candidate's key.  Selected regions are pairwise disjoint and the smallest candidate is always selected.  d_count i32[1] (device) = their number. */
int mirres_dec_select(const int32_t* tris, int T, int V, const int32_t* vstart, const int32_t* vcorner, const unsigned long long* edge_keys, int E,
                      const unsigned long long* keys, const int32_t* cand, int n_cand, unsigned long long* vkey, uint8_t* selected, int32_t* d_count, void* stream);
/* mirres_dec_apply (meshutils.py:64-97), IN PLACE: per selected edge verts[a] = position, quadrics[a] += quadrics[b] (one addition per component), remap[b] = a
 * (remap i32[V], scratch, identity otherwise); per face the indices go through remap; keep_face u8[T] = 0 for a face with a repeated index (its indices are left),
 * used_vertex u8[V] = 1 for the vertices of the kept faces.  The caller compacts with mirres_mesh_compact(keep_face) and the quadrics by used_vertex.
 * h_selected = the count mirres_dec_select left in d_count; BLOCKS until it is on the host.                                                                 */
int mirres_dec_apply(float* verts, double* quadrics, int V, int32_t* tris, int T, const unsigned long long* edge_keys, int E, const float* position,
                     const int32_t* cand, const uint8_t* selected, int n_cand, int32_t* remap, uint8_t* keep_face, uint8_t* used_vertex, const int32_t* d_count,
                     int* h_selected, void* stream);

/* --------------------------------------------------------------------------------------------------------------------------------------------
 * The stage-0 density network (density.hip): what NeRFRenderer.export_stage0 evaluates on its --mcubes_reso lattice (nerf/renderer.py:516-539) — self.density()
 * = torch-ngp's GridEncoder forward (gridencoder/src/gridencoder.cu:87-196: 'hash', align_corners False, linear, D = 3, C = 2) -> the bias-free sigma_net
 * 32 -> 64 (ReLU) -> 16, of which density needs output 0 only -> trunc_exp (activation.py:8-10: exp).  Table and weights fp32 (the reference runs this query under
 * fp16 autocast; DESIGN.md sections 5.11 and 8).  Feature 2 l + c is channel c of level l.  The encoder's operation order is fixed and restated in DESIGN.md section
 * 5.11; sigma is mrf_exp of a k-ascending fmaf chain per neuron.  A point with a coordinate outside [-bound, bound] (or not finite) has 32 zero features and sigma 1. */
#define MIRRES_DENSITY_MAX_LEVELS 16
typedef struct {
    int num_levels;                                   /* 1 .. 16 */
    int offsets[MIRRES_DENSITY_MAX_LEVELS + 1];       /* first table entry of every level, offsets[num_levels] = all entries (grid.py:124-135)                 */
    int resolution[MIRRES_DENSITY_MAX_LEVELS];        /* the KERNEL's resolution, ceil(scale) + 1 (gridencoder.cu:139)                                         */
    int hashed[MIRRES_DENSITY_MAX_LEVELS];            /* 1: get_grid_index's final stride exceeds the level's size, the index is the hash (gridencoder.cu:79)  */
    float scale[MIRRES_DENSITY_MAX_LEVELS];           /* gridencoder.cu:138, computed once on the host                                                         */
    const float* table;                               /* device f32 [entries, 2]: encoder.embeddings                                                           */
    const float* w0;                                  /* device f32 [64, 32]: sigma_net.0.weight                                                               */
    const float* w1;                                  /* device f32 [64]: row 0 of sigma_net.1.weight                                                          */
} mirres_density_t;
/* GridEncoder.__init__ (gridencoder/grid.py:104-135) and gridencoder.cu:137-139 on the host: fills num_levels, offsets, resolution, hashed and scale of `net` (the
 * pointers are left alone) and returns the number of table entries, or a negative error.  per_level_scale = exp2(log2(desired / base) / (L - 1)) in double; the level's
 * size = min(2^log2_hashmap_size, (ceil(base pls^l) + 1)^3) rounded up to a multiple of 8; scale[l] = float(exp2(double(float(l) * float(log2 pls)))) * float(base) - 1.0f,
 * the product and the difference rounded to fp32 — gridencoder.cu:138's expression with a correctly rounded exp2f.                                                  */
long long mirres_density_layout(int num_levels, int base_resolution, double desired_resolution, int log2_hashmap_size, mirres_density_t* net);
/* self.density(pts) (nerf/renderer.py:527-530, one chunk): pos f32[n,3] -> sigma_out f32[n] and, when feat_out is not NULL, the encoder's output f32[n,32].       */
int mirres_density_points(const mirres_density_t* net, const float* pos, long long n, float bound, float* sigma_out, float* feat_out, void* stream);
/* nerf/renderer.py:516-541 in one launch: out f32[nx][ny][nz] = sigma at (xs[i], ys[j], zs[k]) — the axes are read, never recomputed (renderer.py:518-520 builds them
 * with torch.linspace).  With grid_vol f32[S][S][S] (cubic; NULL: no mask) a lattice point whose nearest cell — F.interpolate(mode='nearest')'s index per axis, as in
 * mirres_mc_mask_nearest — does not pass > thresh is exactly 0 and costs no table read: sigmas * mask, then nan_to_num(., 0) (renderer.py:532-541).                  */
int mirres_density_volume(const mirres_density_t* net, const float* xs, int nx, const float* ys, int ny, const float* zs, int nz, float bound,
                          const float* grid_vol, int S, float thresh, float* out, void* stream);

/* --------------------------------------------------------------------------------------------------------------------------------------------
 * The stage-0 radiance network (radiance.hip): NeRFNetwork.forward(x, d) (nerf/network.py:146-174) in one fused query per sample point, fp32 throughout (the
 * reference: fp16 autocast, as for the density; DESIGN.md sections 5.14 and 8).  The position encoder and its bits are mirres_density_points'; sigma_net gives all
 * 16 outputs h16 = W1 . relu(W0 . feat), sigma = mrf_exp(h16[0]) with the bits mirres_density_points gives the same point, geo_feat = h16[1..15]; the direction goes
 * through the degree-4 spherical-harmonics encoder (shencoder/src/shencoder.cu:43-68 after SHEncoder.forward's normalisation; the arithmetic is fixed without FMA,
 * section 5.14); rgb = mrf_sigmoid(C2 . relu(C1 . relu(C0 . [sh, geo_feat]))), every layer bias-free and every output a k-ascending fmaf chain from 0.  A point out
 * of bounds (or not finite) has zero features: sigma 1, geo_feat 0, and its colour is still evaluated.  A zero or non-finite direction gives NaN sh and NaN rgb.  */
typedef struct {
    mirres_density_t grid;   /* levels, table, w0; grid.w1 = row 0 of w1 as today */
    const float* w1;         /* device f32 [16, 64]: sigma_net.1.weight            */
    const float* c0;         /* device f32 [64, 31]: color_net.0.weight            */
    const float* c1;         /* device f32 [64, 64]: color_net.1.weight            */
    const float* c2;         /* device f32 [3, 64]:  color_net.2.weight            */
} mirres_radiance_t;
/* pos, dirs f32[n,3] -> sigma_out f32[n] (NULL: NeRFNetwork.rgb, the colour alone), rgb_out f32[n,3] and, when not NULL, h16_out f32[n,16] (sigma_net's raw
 * outputs) and sh_out f32[n,16].  n in [0, 2^38]; n == 0 launches nothing.  h16_out and sh_out are written 16 bytes at a time: they must be 16-byte aligned
 * (as feat_out of mirres_density_points).                                                                                                                       */
int mirres_radiance_points(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, float* sigma_out, float* rgb_out,
                           float* h16_out, float* sh_out, void* stream);
/* the direction encoder alone: dirs f32[n,3] (any length; normalised inside) -> out f32[n,16], 16-byte aligned                                                  */
int mirres_sh_encode(const float* dirs, long long n, float* out, void* stream);
/* The adjoint of mirres_radiance_points (radiance_bwd.hip): pos, dirs f32[n,3], grad_sigma f32[n] (NULL: zeros), grad_rgb f32[n,3] -> the gradients of the six
 * parameters, all fp32 and all ACCUMULATED INTO (+=; the caller zeroes them): grad_table [entries,2], grad_w0 [64,32], grad_w1 [16,64], grad_c0 [64,31],
 * grad_c1 [64,64], grad_c2 [3,64].  The forward is recomputed from pos / dirs; nothing is taped.  d_pre = grad_rgb rgb (1 - rgb); a ReLU passes the cotangent where
 * its output is > 0; d_h16[0] = grad_sigma mrf_exp(clamp(h16[0], -15, 15)) (trunc_exp's backward, activation.py:14-16), d_h16[1..15] = the colour net's d_in[16..30].
 * A point out of bounds (or not finite) scatters nothing and adds 0 to grad_w0 / grad_w1; its colour path still reaches grad_c0/1/2.  Positions and directions get
 * no gradient.  The weight gradients carry no atomics: min(ceil(n / 256), max_blocks; 0: 1024) blocks write one partial each to workspace [blocks][9344] f32 and a
 * second kernel adds them in block order, so equal inputs and an equal max_blocks give equal bits.  The table gradient is scattered with fp32 atomics and varies in
 * its last bits from run to run.  workspace: device memory of at least mirres_radiance_bwd_workspace_bytes(n, max_blocks) bytes, 4-byte aligned; its contents need
 * not be kept.  n == 0 launches nothing and touches nothing.                                                                                                    */
long long mirres_radiance_bwd_workspace_bytes(long long n, int max_blocks);
int mirres_radiance_points_bwd(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, const float* grad_sigma,
                               const float* grad_rgb, float* grad_table, float* grad_w0, float* grad_w1, float* grad_c0, float* grad_c1, float* grad_c2,
                               void* workspace, long long workspace_bytes, int max_blocks, void* stream);
/* The POSITION adjoint of mirres_radiance_points (radiance_pos.hip), what --enable_offset_nerf_grad lets reach the vertices through self.rgb(xyzs, dirs)
 * (nerf/renderer.py:1046-1052): pos, dirs f32[n,3], grad_sigma f32[n] (NULL: zeros), grad_rgb f32[n,3] -> grad_pos f32[n,3], OVERWRITTEN.  One thread per point, no
 * atomics: equal inputs give equal bits.  The forward is recomputed; the cotangent goes back through the two MLPs under mirres_radiance_points_bwd's rules (d_pre,
 * ReLU, trunc_exp's backward as above; every adjoint sum an fmaf chain from 0 over the layer's outputs ascending) to d_feat[32].  Then the encoder's input
 * gradient, the reference's dy_dx (gridencoder/src/gridencoder.cu:198-243), in this FIXED order, every operation rounded on its own, no FMA, fp32:
 *   levels l ascending; f, 1 - f, the cell and the eight entries are the forward's (dense and hashed levels alike; each corner gathered once);
 *   axes a = 0, 1, 2; lo < hi the two other axes; r[ch] = 0; pairs p = 0 .. 3 ascending: w = scale_l; w = w * (p & 1 ? f[lo] : 1 - f[lo]);
 *   w = w * (p & 2 ? f[hi] : 1 - f[hi]); r[ch] = r[ch] + w * (table[right][ch] - table[left][ch]) for ch = 0, 1 (left / right: the pair's corners at a = 0 / 1);
 *   grad_u[a] = grad_u[a] + d_feat[2 l] * r[0]; grad_u[a] = grad_u[a] + d_feat[2 l + 1] * r[1];
 *   after the last level grad_pos[a] = grad_u[a] / (2 * bound) (gridencoder/grid.py:156), an IEEE division.
 * A point out of bounds (or not finite) has constant features: exactly 0, 0, 0.  On a cell face the derivative is the one-sided one of the cell the forward picks.
 * Directions get no gradient.  Refused before a device is touched: a NULL net or weight or a bad layout, n < 0 or n > 2^38, NULL pos / dirs / grad_rgb / grad_pos
 * with n > 0, a bound that is not positive and finite.  n == 0 launches nothing.                                                                                */
int mirres_radiance_points_bwd_pos(const mirres_radiance_t* net, const float* pos, const float* dirs, long long n, float bound, const float* grad_sigma,
                                   const float* grad_rgb, float* grad_pos, void* stream);
/* GridEncoder.grad_total_variation (gridencoder/grid.py:170-192) over kernel_grad_tv (gridencoder/src/gridencoder.cu:505-609), grid_tv.hip: the in-place
 * total-variation regulariser of the hash grid.  pos f32[n,3] in world coordinates, as for mirres_density_points; grad_table f32[entries,2] is ACCUMULATED into;
 * net->w0 and net->w1 are not read and may be NULL.  Per point and level: c = the encoder's corner 0 (floorf(u * scale + 0.5f) per axis), e = its entry; for
 * d = 0, 1, 2 first the right neighbour (c[d] + 1, when c[d] < resolution), then the left (c[d] - 1, when c[d] > 0), per channel diff = table[e] - table[nb],
 * res += diff, idelta += diff * diff; value = (w * res) * (1 / sqrt(idelta + 1e-9f)) with w = weight / 6.0f, every operation rounded on its own and 1 / sqrt by
 * IEEE (the reference: rsqrtf).  A point with a coordinate outside [-bound, bound] or not finite contributes to no level (the reference casts a NaN to an index).
 * DENSE levels (hashed[l] == 0) take no fp32 atomic: the points of every cell are counted with integer atomics in `workspace`, then every entry with a count gets
 * grad[e] = grad[e] + (float)count * value by one plain store — one fixed set of bits for a given multiset of points, whatever their order; (float)count rounds
 * above 2^24 points in one cell.  Entries without a point are not touched.  HASHED levels add value with fp32 atomics in no fixed order; the lanes of a wave that
 * hold one cell add (float)k * value once.  workspace: device memory of at least mirres_grid_tv_workspace_bytes(net) bytes (4 bytes per entry of the dense
 * levels), 4-byte aligned; its contents need not be initialised and it can be handed to the next call on the same stream.  Refused before a device is touched:
 * a NULL net or table or a bad layout, n < 0 or n > 2^31, NULL pos with n > 0, NULL grad_table, a negative or non-finite weight, a bound that is not positive,
 * a NULL or short workspace.  n == 0 or weight == 0 returns 0 and changes nothing.                                                                              */
long long mirres_grid_tv_workspace_bytes(const mirres_density_t* net);
int mirres_grid_tv_grad(const mirres_density_t* net, const float* pos, long long n, float bound, float weight, float* grad_table, void* workspace,
                        long long workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------------------------------------------------------------
 * torch-ngp's GridEncoder as an operator of its own (gridenc.hip; encoding.py's GridEncoder): what the fused entries above hold for one configuration, for any of
 * input_dim D in {2, 3}, level_dim C in {1, 2, 4, 8}, 1 .. 16 levels, gridtype hash / tiled, align_corners, linear / smoothstep interpolation.  fp32 only.  The table
 * is passed beside the layout: f32 [offsets[num_levels], C], 16-byte aligned.  The arithmetic is FIXED, every operation rounded on its own:
 *   u[d] = (x[d] + bound) / (2.0f * bound); a point is in bounds when every u[d] >= 0 && u[d] <= 1 (NaN: outside);
 *   per level: p = u[d] * scale; p = p + (align_corners ? 0.0f : 0.5f); cell = floorf(p); f = p - cell; smoothstep: s = (f * f) * (3.0f - 2.0f * f) with derivative
 *   (6.0f * f) * (1.0f - f); linear: s = f, derivative 1; corners idx ascending: w = 1; for d ascending w = w * (bit d of idx ? s[d] : 1.0f - s[d]);
 *   r[ch] = r[ch] + w * table[entry][ch]; entry = get_grid_index (gridencoder.cu:66-84) in uint32 arithmetic: the stride loop stops adding axes once the stride
 *   exceeds the level's size, the factor is align_corners ? resolution : resolution + 1, the hash (primes 1, 2654435761, 805459861) only for gridtype 0 with a final
 *   stride above the level's size, then % size.  At u = 1 with align_corners the index is one past the last row, wrapped by the modulo, as in the reference.
 * For D = 3, C = 2, hash, align_corners 0, linear the features have mirres_density_points' bits and grad_pos mirres_radiance_points_bwd_pos' encoder part's.        */
typedef struct {
    int input_dim;                                    /* D: 2 or 3                                                                                              */
    int level_dim;                                    /* C: 1, 2, 4 or 8                                                                                        */
    int num_levels;                                   /* 1 .. 16                                                                                                */
    int gridtype;                                     /* 0 hash, 1 tiled                                                                                        */
    int align_corners;                                /* 0 or 1                                                                                                 */
    int interpolation;                                /* 0 linear, 1 smoothstep                                                                                 */
    int offsets[MIRRES_DENSITY_MAX_LEVELS + 1];       /* as mirres_density_t                                                                                    */
    int resolution[MIRRES_DENSITY_MAX_LEVELS];        /* the KERNEL's resolution, ceil(scale) + 1                                                               */
    int hashed[MIRRES_DENSITY_MAX_LEVELS];            /* 1: the level's index is the hash (gridtype 0 and a final stride above the level's size)                */
    float scale[MIRRES_DENSITY_MAX_LEVELS];           /* gridencoder.cu:138, computed once on the host                                                          */
} mirres_gridenc_t;
/* GridEncoder.__init__ (gridencoder/grid.py:104-135) and gridencoder.cu:137-139 on the host, under mirres_density_layout's rules: per_level_scale in double,
 * S = float(log2 per_level_scale), a correctly rounded exp2f, the level's size = min(2^log2_hashmap_size, (r if align_corners else r + 1)^D) with r = ceil(base pls^l),
 * rounded up to a multiple of 8.  Fills every field of `g` and returns the number of table entries, or a negative error.  For D = 3, hash, align_corners 0 and
 * per_level_scale = exp2(log2(desired / base) / (L - 1)) it fills mirres_density_layout's numbers (one routine computes both), but for the `hashed` flag
 * of a level whose uint32 stride product wraps (its square or cube passes 2^32): indexed densely with wrapped strides here, as in the reference, hashed there.          */
long long mirres_gridenc_layout(int input_dim, int level_dim, int num_levels, double per_level_scale, int base_resolution, int log2_hashmap_size, int gridtype,
                                int align_corners, int interpolation, mirres_gridenc_t* g);
/* pos f32[n, D] -> out f32[n, L * C] (feature l * C + ch; 16-byte aligned), every element written: a point out of bounds and every level >= max_level give 0
 * (max_level above num_levels counts as num_levels).  One thread per (point, level), launched level-major.                                                        */
int mirres_grid_encode_fwd(const mirres_gridenc_t* g, const float* table, const float* pos, long long n, float bound, int max_level, float* out, void* stream);
/* The adjoint: grad_out f32[n, L * C] (16-byte aligned) -> grad_table f32[entries, C], ACCUMULATED INTO with fp32 atomics in no fixed order (NULL: not wanted), term
 * w * grad_out[l * C + ch] per corner, one entry's C channels by C adjacent lanes, launched level-major; grad_pos f32[n, D], OVERWRITTEN (NULL: not wanted): the
 * reference's dy_dx (gridencoder.cu:198-243) recomputed, one thread per point, no atomics, equal inputs give equal bits — levels l ascending, axes a ascending; the
 * pairs of corners that differ in a alone, ascending (bit k of the pair: the k-th other axis): w = scale_l; w = w * (s or 1 - s) per other axis ascending;
 * r[ch] = r[ch] + (w * (table[right][ch] - table[left][ch])) * derivative[a]; then for ch ascending g[a] = g[a] + grad_out[l * C + ch] * r[ch]; last
 * grad_pos[a] = g[a] / (2.0f * bound).  A point out of bounds scatters nothing and gets exactly 0; levels >= max_level carry no gradient.
 * Both entries refuse, before a device is touched: a NULL layout, a D, C, level count or switch outside the sets above, a layout mirres_gridenc_layout would not
 * have filled, n < 0 or n > 2^31, a NULL table / pos / out / grad_out with n > 0, a misaligned pointer, a negative max_level, a bound that is not positive and
 * finite.  n == 0 launches nothing.                                                                                                                              */
int mirres_grid_encode_bwd(const mirres_gridenc_t* g, const float* table, const float* pos, long long n, float bound, int max_level, const float* grad_out,
                           float* grad_table, float* grad_pos, void* stream);

/* --------------------------------------------------------------------------------------------------------------------------------------------
 * The stage-0 ray-marching operators (raymarch.hip): torch-ngp's raymarching module (raymarching/src/raymarching.cu), fp32 only, and the upkeep of the
 * occupancy grid the marchers read (nerf/renderer.py:1438-1595).  The arithmetic is FIXED (csrc/device_march.hpp): no contraction, IEEE
 * division, the reference's own C++ promotions, mrf_exp where the reference has __expf.  Deviations: march_rays_train hands out point offsets as the exclusive
 * prefix sum of the per-ray counts (no atomic counter); every marching loop terminates for every input (a ray with a zero / non-finite direction or a NaN near /
 * far takes no step; the voxel-skipping loop also ends at t >= far and when t + dt == t); a ray whose span leaves [0, M) and a rays_alive entry outside [0, N)
 * are skipped, never followed.  Counts are 64-bit and at most 2^31 per call (one launch); H is a power of two in [2, 1024]; at most MIRRES_RM_MAX_CASCADES cascades.                            */
#define MIRRES_RM_MAX_CASCADES 8
/* raymarching.cu:92-145 kernel_near_far_from_aabb: rays_o/d f32[N,3], aabb f32[6] -> nears, fars f32[N]; a miss gives FLT_MAX for both.                      */
int mirres_rm_near_far(const float* rays_o, const float* rays_d, const float* aabb, long long N, float min_near, float* nears, float* fars, void* stream);
/* :214-232 kernel_morton3D: coords i32[N,3] -> indices i32[N];  :235-260 kernel_morton3D_invert: the inverse.                                                */
int mirres_rm_morton3d(const int32_t* coords, long long N, int32_t* indices, void* stream);
int mirres_rm_morton3d_invert(const int32_t* indices, long long N, int32_t* coords, void* stream);
/* :268-300 kernel_packbits: grid f32[8 N] (16-byte aligned) -> bitfield u8[N], bit i of byte n = grid[8 n + i] > thresh.                                      */
int mirres_rm_packbits(const float* grid, long long N, float thresh, uint8_t* bitfield, void* stream);
/* :303-326 kernel_flatten_rays: rays i32[N,2] (offset, count) -> res i32[M], res[offset + i] = n.                                                             */
int mirres_rm_flatten_rays(const int32_t* rays, long long N, long long M, int32_t* res, void* stream);
/* :338-489 kernel_march_rays_train in three launches.  _count: the reference's first pass, rays[n,1] = steps of ray n (rays[n,0] = 0).  _scan: rays[n,0] = the
 * exclusive prefix sum of rays[:,1] in ray order (clamped at 2^31 - 1), total[0] (device, 64-bit) = M.  _write: the second pass, xyzs/dirs f32[M,3], ts f32[M,2].  */
int mirres_rm_march_train_count(const float* rays_o, const float* rays_d, const uint8_t* bitfield, float bound, int contract, float dt_gamma, int max_steps,
                                long long N, int C, int H, const float* nears, const float* fars, const float* noises, int32_t* rays, void* stream);
int mirres_rm_march_train_scan(int32_t* rays, long long N, long long* total, void* stream);
int mirres_rm_march_train_write(const float* rays_o, const float* rays_d, const uint8_t* bitfield, float bound, int contract, float dt_gamma, int max_steps,
                                long long N, int C, int H, const float* nears, const float* fars, const float* noises, const int32_t* rays, long long M,
                                float* xyzs, float* dirs, float* ts, void* stream);
/* :501-589 kernel_composite_rays_train_forward: weights f32[M] must arrive zeroed (samples behind an early stop are not written).                             */
int mirres_rm_composite_train_fwd(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, long long M, long long N, float T_thresh,
                                  int alpha_mode, float* weights, float* weights_sum, float* depth, float* image, void* stream);
/* :605-705 kernel_composite_rays_train_backward: grad_sigmas f32[M], grad_rgbs f32[M,3] must arrive zeroed.                                                   */
int mirres_rm_composite_train_bwd(const float* grad_weights, const float* grad_weights_sum, const float* grad_depth, const float* grad_image,
                                  const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, const float* weights_sum, const float* depth,
                                  const float* image, long long M, long long N, float T_thresh, int alpha_mode, float* grad_sigmas, float* grad_rgbs,
                                  void* stream);
/* :713-838 kernel_march_rays: the first n_alive entries of rays_alive name rays of the N; xyzs/dirs f32[n_alive n_step,3], ts f32[n_alive n_step,2] arrive zeroed. */
int mirres_rm_march(long long n_alive, int n_step, const int32_t* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d, long long N,
                    float bound, int contract, float dt_gamma, int max_steps, int C, int H, const uint8_t* bitfield, const float* nears, const float* fars,
                    float* xyzs, float* dirs, float* ts, const float* noises, void* stream);
/* :842-933 kernel_composite_rays: accumulates into weights_sum, depth f32[N], image f32[N,3]; a finished ray's rays_alive entry becomes -1.                   */
int mirres_rm_composite(long long n_alive, int n_step, long long N, float T_thresh, int alpha_mode, int32_t* rays_alive, float* rays_t, const float* sigmas,
                        const float* rgbs, const float* ts, float* weights_sum, float* depth, float* image, void* stream);
/* nerf/renderer.py:1438-1524 mark_untrained_grid in one launch: grid f32[C, H^3] (Morton order); poses f32[B,4,4] camera-to-world; intrinsics f32[4] or, with
 * per_cam_intrinsics, f32[B,4] (fx, fy, cx, cy); cam_near_far f32[B,2] or NULL (then min_near); aabb f32[6].  The camera-space point is ((x r0 + y r1) + z r2)
 * without FMA.  Cells no camera covers, or outside the box by more than half a cell, become -1; every other cell is left alone.                               */
int mirres_rm_grid_mark_untrained(float* grid, int C, int H, float bound, const float* poses, int B, const float* intrinsics, int per_cam_intrinsics,
                                  const float* cam_near_far, float min_near, const float* aabb, void* stream);
/* nerf/renderer.py:1540-1577 update_extra_state's grid pass (non-trainable grid) in one launch over all cascades: per cell, in Morton index order, the point
 * ((2 i / (H - 1) - 1) * (bound_c - half_cell)) + (2 noise - 1) * half_cell, each step rounded to fp32; sigma of `net` (evaluated with field_bound, the code of
 * mirres_density_points) at it; grid = max(grid * decay, sigma) where both are >= 0.  noise f32[C, H^3, 3].  A cell at -1 costs no query.                      */
int mirres_rm_grid_update(const mirres_density_t* net, float field_bound, float* grid, int C, int H, float bound, const float* noise, float decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRRES_H */
