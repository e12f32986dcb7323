"""Stage-0 mesh extraction (NeRFRenderer.export_stage0, nerf/renderer.py:498-570; csrc/mcubes.hip): from a stage-0 checkpoint's density grid, a dumped
sigma / SDF volume or a foreign mesh to the `<workspace>/mesh_stage0/mesh_0.ply` every stage-1 tool starts from, with no PyMCubes / pymeshlab / trimesh /
nvdiffrast behind it.

    v, t = marching_cubes(vol, iso)                        # mcubes.marching_cubes (:549-555): index-space vertices, welded, deterministic
    vol = unpack_density_grid(ck["model"]["density_grid"]) # :511-515, cascade 0, Morton order -> [S, S, S]
    unseen = mark_unseen_triangles(v, t, mvps, H, W)       # :1400-1434 on raster.rasterize
    v, t = remove_masked_trigs(v, t, unseen, dilation=5)   # meshutils.py:100-130
    v, t = clean_mesh(v, t, min_f=8, min_d=5)              # meshutils.py:183-225 (repair=True, remesh=False)
    v, t = decimate_mesh(v, t, 3e5)                        # meshutils.py:64-97 (:566-567): quadric edge collapse in deterministic rounds, csrc/decimate.hip
    field = DensityField.from_checkpoint(ck, bound=1.0)    # self.density (nerf/network.py:177-192): hash-grid encoder + sigma_net + exp, csrc/density.hip
    vol = field.volume(512, grid_vol, thresh)              # :516-541: the --mcubes_reso lattice, masked by the density grid
    export_stage0(save_path, ckpt=..., cameras=(mvps, H, W), resolution=512)
    occ = occupancy_volume(grid_vol, 256, thresh)          # :653-655: a cascade's grid, trilinear to env_reso^3, nan_to_num, > thresh -> 0 / 1
    v, t = remove_selected_verts(v, t, box, "inside")      # meshutils.py:159-181 (:663, :676)
    v, t = outer_shell(grid_vol, cas, bound, 256, thresh, aabb)                 # :642-676: one outer cascade up to (not including) cleaning
    export_outer_meshes(save_path, ckpt, bound=2)          # :632-698: mesh_1.ply ... for a checkpoint trained with bound > 1 (export_stage0(outer=True))
    rf = RadianceField.from_checkpoint(ck, bound=1.0)      # NeRFNetwork.forward (nerf/network.py:146-174): + SH direction encoder + colour net, csrc/radiance.hip
    sigma, rgb = rf.forward(x, d)                          # one fused query per point
    out = render_stage0(rf, DensityGrid.from_checkpoint(ck), rays_o, rays_d)     # :714-717, 778-839: the inference branch of render -> image, depth, weights_sum
    sigma, rgb = rf.forward_train(x, d)                    # the same bits, differentiable in rf.parameters(): csrc/radiance_bwd.hip recomputes and adjoins
    out = render_stage0_train(rf, grid, rays_o, rays_d)    # :735-773, 830-838: the training branch (march_rays_train, composite_rays_train)
    rf.grad_total_variation(1e-8, out["xyzs"])             # gridencoder/grid.py:170-192 after loss.backward(): the table's TV regulariser in place, csrc/grid_tv.hip

Deviations from the reference: background pixels mark no face (the reference's `mask[-1] += 1` marks the last one); vertices are merged
when their three coordinates are bit-identical (MeshLab's tolerance merge is not reproduced); non-manifold repair and remeshing are not built; decimation
collapses independent sets of edges round by round instead of one edge at a time from a global heap, without MeshLab's quality / normal / planar extras, and may
end one face below the target; the density network is evaluated in fp32 (the reference: fp16 autocast), unfused, and a NaN coordinate counts as out of bounds;
the outer cascades' vertices are fp32 from marching cubes on (the reference holds float64 until after decimation), and the --sdf / contracted outer mesh
(:575-629) is not built; the radiance network likewise runs in fp32, its direction encoder with a fixed operation order and no FMA,
and a zero or non-finite direction gives NaN as the reference's 0 / 0 does; training runs in fp32 without autocast or a gradient scaler, and the table's
gradient is summed by atomics in no fixed order.
Tensors live on the current device; every function returns device tensors (vertices f32 [V, 3], triangles i32 [T, 3])."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_ptr

__all__ = ["marching_cubes", "morton_indices", "unpack_density_grid", "select_iso", "mask_by_density_grid", "seen_faces", "mark_unseen_triangles", "dilate_selection",
           "compact_mesh", "remove_masked_trigs", "face_components", "clean_mesh", "decimate_round", "decimate_mesh", "index_to_world", "synthetic_volume", "DensityField", "DensityGrid", "density_layout",
           "synthetic_checkpoint", "export_stage0", "occupancy_volume", "remove_selected_verts", "outer_shell", "export_outer_meshes",
           "RadianceField", "render_stage0", "render_stage0_train", "synthetic_radiance_checkpoint", "synthetic_radiance_color"]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _verts(v):
    return torch.as_tensor(v).to(_dev(), torch.float32).reshape(-1, 3).contiguous()


def _tris(t):
    return torch.as_tensor(t).to(_dev(), torch.int32).reshape(-1, 3).contiguous()


def marching_cubes(vol, iso):
    """vol f32 [nx, ny, nz] (tensor or numpy), iso -> (vertices f32 [V, 3] in index space, triangles i32 [T, 3]); inside = vol >= iso, normals towards
    decreasing values, non-finite values as torch.nan_to_num(., 0).  V = T = 0 when nothing crosses."""
    vol = torch.as_tensor(vol).to(_dev(), torch.float32).contiguous()
    if vol.dim() != 3:
        raise ValueError("marching_cubes: expected a 3-D volume, got %s" % (tuple(vol.shape),))
    nx, ny, nz = (int(s) for s in vol.shape)
    L = lib()
    nbytes = int(L.mirres_mc_scratch_bytes(nx, ny, nz))
    if nbytes < 0:
        check(nbytes, "mirres_mc_scratch_bytes")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    counts = (C.c_int * 2)()
    check(L.mirres_mc_count(ptr(vol), nx, ny, nz, float(iso), ptr(scratch), nbytes, counts, stream_ptr()), "mirres_mc_count")
    V, T = int(counts[0]), int(counts[1])
    verts = torch.empty((V, 3), dtype=torch.float32, device=vol.device); tris = torch.empty((T, 3), dtype=torch.int32, device=vol.device)
    check(L.mirres_mc_emit(ptr(vol), nx, ny, nz, float(iso), ptr(scratch), ptr(verts) if V else None, V, ptr(tris) if T else None, T, stream_ptr()), "mirres_mc_emit")
    return verts, tris


def morton_indices(S):
    """i64 [S, S, S]: the Morton index of grid point (x, y, z) — x in bits 0, 3, 6, ..., y in bits 1, 4, ..., z in bits 2, 5, ... (raymarching.cu:73-81)."""
    S = int(S)
    if S < 2 or S & (S - 1) or S > 1024:
        raise ValueError("grid size %d is not a power of two in [2, 1024]" % S)
    a = np.arange(S, dtype=np.int64)
    s = np.zeros(S, np.int64)
    for b in range(10):
        s |= ((a >> b) & 1) << (3 * b)
    return s[:, None, None] | (s[None, :, None] << 1) | (s[None, None, :] << 2)


def unpack_density_grid(density_grid, cascade=0):
    """density_grid [cascade, S^3] (or [S^3]) in Morton order -> vol f32 [S, S, S] of one cascade on the device (nerf/renderer.py:511-515)."""
    g = torch.as_tensor(density_grid).to(_dev(), torch.float32)
    g = g.reshape(1, -1) if g.dim() == 1 else g
    n = int(g.shape[1]); S = int(round(n ** (1.0 / 3.0)))
    if S * S * S != n:
        raise ValueError("density_grid: %d values per cascade is not a cube" % n)
    row = g[int(cascade)].contiguous()
    vol = torch.empty((S, S, S), dtype=torch.float32, device=row.device)
    check(lib().mirres_mc_unpack_morton(ptr(row), S, ptr(vol), stream_ptr()), "mirres_mc_unpack_morton")
    return vol


def select_iso(mean_density, density_thresh=10.0):
    """nerf/renderer.py:506."""
    return min(float(mean_density), float(density_thresh))


def mask_by_density_grid(vol, grid_vol, thresh):
    """nerf/renderer.py:532-539: vol [R, R, R] * (F.interpolate(grid_vol [S, S, S], mode='nearest') > thresh); returns a new tensor."""
    out = torch.as_tensor(vol).to(_dev(), torch.float32).contiguous().clone(); g = torch.as_tensor(grid_vol).to(_dev(), torch.float32).contiguous()
    if out.dim() != 3 or len(set(out.shape)) != 1 or g.dim() != 3 or len(set(g.shape)) != 1:
        raise ValueError("mask_by_density_grid: cubic volumes expected, got %s and %s" % (tuple(out.shape), tuple(g.shape)))
    check(lib().mirres_mc_mask_nearest(ptr(out), int(out.shape[0]), ptr(g), int(g.shape[0]), float(thresh), stream_ptr()), "mirres_mc_mask_nearest")
    return out


def index_to_world(vertices, resolution):
    """nerf/renderer.py:553; `resolution` an int or one per axis."""
    r = torch.as_tensor(resolution, dtype=torch.float32, device=vertices.device)
    return (vertices / (r - 1.0) * 2 - 1).to(torch.float32)


def occupancy_volume(grid_vol, resolution, thresh, return_values=False):
    """nerf/renderer.py:653-655 in one launch: grid_vol [S, S, S] -> F.interpolate(., [R] * 3, mode='trilinear') -> nan_to_num(., 0) -> > thresh, as f32 [R, R, R]
    of 0 / 1 (what mcubes.marching_cubes(occ, 0.5) reads).  return_values: (occ, the interpolated values f32 [R, R, R])."""
    g = torch.as_tensor(grid_vol).to(_dev(), torch.float32).contiguous()
    if g.dim() != 3 or len(set(g.shape)) != 1:
        raise ValueError("occupancy_volume: a cubic grid_vol expected, got %s" % (tuple(g.shape),))
    R = int(resolution)
    if R < 1 or R > 1024:
        raise ValueError("occupancy_volume: resolution %d is not in [1, 1024]" % R)
    occ = torch.empty((R, R, R), dtype=torch.float32, device=g.device)
    val = torch.empty_like(occ) if return_values else None
    check(lib().mirres_mc_occupancy_trilinear(ptr(g), int(g.shape[0]), R, float(thresh), ptr(occ), ptr(val), stream_ptr()), "mirres_mc_occupancy_trilinear")
    return (occ, val) if return_values else occ


def _box6(box):
    b = [float(x) for x in np.asarray(box, np.float64).reshape(-1)]
    if len(b) != 6 or any(x != x for x in b):
        raise ValueError("a box is (xmn, ymn, zmn, xmx, ymx, zmx) without NaN, got %r" % (box,))
    return b


def remove_selected_verts(vertices, triangles, box, where="inside", log=None):
    """meshutils.py:159-181 with the two queries export_stage0 builds: box = (xmn, ymn, zmn, xmx, ymx, zmx); where = "inside" deletes every vertex with
    x <= xmx && x >= xmn && ... (the closed box, renderer.py:663), "outside" every vertex with x <= xmn || x >= xmx || ... (:676).  A face goes when it touches a
    deleted vertex; so do the vertices no face uses any more; order is kept."""
    if where not in ("inside", "outside"):
        raise ValueError("remove_selected_verts: where is 'inside' or 'outside', got %r" % (where,))
    b = _box6(box)
    v, t = _verts(vertices), _tris(triangles)
    V, T = int(v.shape[0]), int(t.shape[0])
    keep = torch.empty(T, dtype=torch.uint8, device=v.device)
    check(lib().mirres_mesh_select_box(ptr(v) if V else None, V, ptr(t) if T else None, T, (C.c_double * 6)(*b), 1 if where == "outside" else 0, ptr(keep) if T else None,
                                       stream_ptr()), "mirres_mesh_select_box")
    ov, ot = compact_mesh(v, t, keep)
    if log:
        log("[INFO] mesh remove verts: %s --> %s, %s --> %s" % (tuple(v.shape), tuple(ov.shape), tuple(t.shape), tuple(ot.shape)))
    return ov, ot


OUTER_CENTRE = 0.45                          # renderer.py:662: the part of an outer cascade's cube the cascades before it cover


def outer_shell(grid_vol, cas, bound, env_reso, thresh, aabb, log=None):
    """One outer cascade of export_stage0 (nerf/renderer.py:642-676) up to, not including, cleaning: grid_vol [S, S, S] is cascade `cas` (>= 1) of the density
    grid; occupancy at env_reso^3 (occupancy_volume), marching cubes at 0.5, vertices to [-1, 1], the closed centre box of +-0.45 removed, vertices scaled by
    bound_cas - half (bound_cas = min(2^cas, bound), half = bound_cas / env_reso), everything not strictly inside aabb (6 values, aabb_train) shrunk by half
    removed -> (vertices f32 [V, 3] in world space, triangles i32 [T, 3]); V = T = 0 when nothing is left."""
    cas, R = int(cas), int(env_reso)
    if cas < 1:
        raise ValueError("outer_shell: cascade %d is not an outer one" % cas)
    if R < 2 or R > 1024:
        raise ValueError("outer_shell: env_reso %d is not in [2, 1024]" % R)
    a = _box6(aabb)
    bound_cas = min(2.0 ** cas, float(bound)); half = bound_cas / R
    occ = occupancy_volume(grid_vol, R, thresh)
    v, t = marching_cubes(occ, 0.5)
    if log:
        log("[INFO] cascade %d: marching cubes at %s of the occupancy > %g: %d vertices, %d triangles" % (cas, "x".join([str(R)] * 3), thresh, v.shape[0], t.shape[0]))
    v = index_to_world(v, R)
    r = OUTER_CENTRE
    v, t = remove_selected_verts(v, t, (-r, -r, -r, r, r, r), "inside", log=log)
    if v.shape[0] == 0:
        return v, t
    v = (v * float(bound_cas - half)).to(torch.float32)
    return remove_selected_verts(v, t, [a[0] + half, a[1] + half, a[2] + half, a[3] - half, a[4] - half, a[5] - half], "outside", log=log)


@torch.no_grad()
def seen_faces(vertices, triangles, mvps, H, W):
    """u8 [T]: 1 for every face whose id appears in raster.rasterize's output of some view (mvps [B, 4, 4]); background marks nothing.  The BVH is built once."""
    from . import raster
    from .renderer_restir import restirbvhWorker
    v, t = _verts(vertices), _tris(triangles)
    T = int(t.shape[0])
    seen = torch.zeros(T, dtype=torch.uint8, device=v.device)
    if T == 0:
        return seen
    worker = restirbvhWorker(v, t); worker.update_mesh(v, t)
    ctx = raster.RasterizeContext(worker)
    vh = torch.nn.functional.pad(v, (0, 1), value=1.0)
    for mvp in mvps:
        mvp = torch.as_tensor(mvp).to(v.device, torch.float32)
        rast, _ = raster.rasterize(ctx, (vh @ mvp.t())[None], t, (int(H), int(W)), grad_db=False, mvp=mvp)
        rast = rast.reshape(-1, 4)
        check(lib().mirres_mesh_mark_seen(ptr(rast), int(rast.shape[0]), T, ptr(seen), stream_ptr()), "mirres_mesh_mark_seen")
    return seen


def mark_unseen_triangles(vertices, triangles, mvps, H, W, log=None):
    """nerf/renderer.py:1400-1434 -> bool [T], True = seen by no camera."""
    mask = seen_faces(vertices, triangles, mvps, H, W) == 0
    if log:
        log("[mark unseen trigs] %d from %d" % (int(mask.sum()), mask.shape[0]))
    return mask


def dilate_selection(triangles, n_vertices, selected, rings):
    """`rings` rings of MeshLab's apply_selection_dilatation on a face selection (u8 / bool [T]) -> u8 [T]."""
    t = _tris(triangles); T = int(t.shape[0]); V = int(n_vertices)
    a = torch.as_tensor(selected).to(t.device).ne(0).to(torch.uint8).contiguous()
    if a.shape[0] != T:
        raise ValueError("dilate_selection: %d flags for %d faces" % (a.shape[0], T))
    b = torch.empty_like(a); vf = torch.empty(max(V, 1), dtype=torch.uint8, device=t.device)
    for _ in range(int(rings)):
        check(lib().mirres_mesh_dilate(ptr(t), T, V, ptr(a), ptr(vf), ptr(b), stream_ptr()), "mirres_mesh_dilate")
        a, b = b, a
    return a


def compact_mesh(vertices, triangles, keep_face=None):
    """Keeps the faces with keep_face != 0 (None: all) and the vertices they use, in their old order."""
    v, t = _verts(vertices), _tris(triangles)
    V, T = int(v.shape[0]), int(t.shape[0])
    keep = torch.ones(T, dtype=torch.uint8, device=v.device) if keep_face is None else torch.as_tensor(keep_face).to(v.device).ne(0).to(torch.uint8).contiguous()
    if keep.shape[0] != T:
        raise ValueError("compact_mesh: %d flags for %d faces" % (keep.shape[0], T))
    if T and (int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError("compact_mesh: face index out of range")
    L = lib()
    nbytes = int(L.mirres_mesh_scratch_bytes(V, T))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    ov = torch.empty_like(v); ot = torch.empty_like(t)
    counts = (C.c_int * 2)()
    check(L.mirres_mesh_compact(ptr(v), V, ptr(t), T, ptr(keep), ptr(ov), ptr(ot), ptr(scratch), counts, stream_ptr()), "mirres_mesh_compact")
    return ov[: counts[0]].contiguous(), ot[: counts[1]].contiguous()


def remove_masked_trigs(vertices, triangles, mask, dilation=5, log=None):
    """meshutils.py:100-130: mask 0 = keep, 1 = remove; the kept selection is dilated `dilation` rings before its complement is deleted."""
    v, t = _verts(vertices), _tris(triangles)
    keep = dilate_selection(t, v.shape[0], torch.as_tensor(mask).to(v.device).eq(0), dilation)
    ov, ot = compact_mesh(v, t, keep)
    if log:
        log("[INFO] mesh mask trigs: %s --> %s, %s --> %s" % (tuple(v.shape), tuple(ov.shape), tuple(t.shape), tuple(ot.shape)))
    return ov, ot


def face_components(triangles, max_rounds=0):
    """(labels i32 [T], rounds): the smallest face index of every face's component, components joined across shared EDGES (not shared vertices).
    `max_rounds` (0: the library's cap of 64) bounds the hook / jump rounds; past it MirresError is raised."""
    t = _tris(triangles); T = int(t.shape[0])
    label = torch.empty(T, dtype=torch.int32, device=t.device)
    if T == 0:
        return label, 0
    t64 = t.to(torch.int64)
    a = t64.reshape(-1); b = t64[:, [1, 2, 0]].reshape(-1)                      # entry 3 f + k: edge (v_k, v_k+1) of face f
    keys, order = torch.sort((torch.minimum(a, b) << 32) | torch.maximum(a, b), stable=True)
    face = (order // 3).to(torch.int32).contiguous(); keys = keys.contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=t.device)
    rounds = C.c_int(0)
    check(lib().mirres_mesh_components(ptr(keys), ptr(face), int(keys.shape[0]), T, ptr(label), ptr(flag), int(max_rounds), C.byref(rounds), stream_ptr()), "mirres_mesh_components")
    return label, rounds.value


def _first_of_group(inverse, n_groups):
    idx = torch.arange(inverse.shape[0], device=inverse.device)
    return torch.full((n_groups,), inverse.shape[0], dtype=torch.int64, device=inverse.device).scatter_reduce(0, inverse, idx, "amin")


def clean_mesh(vertices, triangles, min_f=8, min_d=5, max_rounds=0, log=None):
    """meshutils.py:183-225 with repair=True, remesh=False, in the reference's order: unreferenced vertices, duplicate vertices (bit-identical coordinates, lowest
    index kept), duplicate faces (same vertex set, first kept) and null faces (a repeated index or an exactly zero cross product), components (shared edges)
    whose bounding-box diagonal is below min_d % of the mesh's, components with fewer than min_f faces.  Order is preserved throughout."""
    v0, t0 = _verts(vertices), _tris(triangles)
    v, t = compact_mesh(v0, t0)
    if v.shape[0]:
        uniq, inv = torch.unique(v.view(torch.int32), dim=0, return_inverse=True)
        rep = _first_of_group(inv, uniq.shape[0])[inv]
        t = rep[t.to(torch.int64)].to(torch.int32)
    if t.shape[0]:
        s = torch.sort(t, dim=1).values
        uniq, inv = torch.unique(s, dim=0, return_inverse=True)
        keep = _first_of_group(inv, uniq.shape[0])[inv] == torch.arange(t.shape[0], device=t.device)
        p = v[t.to(torch.int64)]
        cross = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
        null = (s[:, 0] == s[:, 1]) | (s[:, 1] == s[:, 2]) | (cross == 0).all(dim=1)
        v, t = compact_mesh(v, t, keep & ~null)
    else:
        v, t = compact_mesh(v, t)
    if t.shape[0] and (min_d > 0 or min_f > 0):
        label, _ = face_components(t, max_rounds)
        lab = label.to(torch.int64); T = t.shape[0]
        keep = torch.ones(T, dtype=torch.bool, device=t.device)
        if min_d > 0:
            p = v[t.to(torch.int64)].double()                                           # [T, 3, 3]
            lo = torch.full((T, 3), float("inf"), dtype=torch.float64, device=t.device).scatter_reduce(0, lab[:, None].expand(T, 3), p.amin(dim=1), "amin")
            hi = torch.full((T, 3), float("-inf"), dtype=torch.float64, device=t.device).scatter_reduce(0, lab[:, None].expand(T, 3), p.amax(dim=1), "amax")
            diag = (hi - lo).square().sum(dim=1).sqrt()                                   # per label (rows of non-labels hold inf - -inf)
            whole = (v.double().amax(dim=0) - v.double().amin(dim=0)).square().sum().sqrt()
            keep &= ~(diag[lab] < whole * (float(min_d) / 100.0))
        if min_f > 0:
            size = torch.zeros(T, dtype=torch.int64, device=t.device).index_add_(0, lab, torch.ones(T, dtype=torch.int64, device=t.device))
            keep &= size[lab] >= int(min_f)
        v, t = compact_mesh(v, t, keep)
    if log:
        log("[INFO] mesh cleaning: %s --> %s, %s --> %s" % (tuple(v0.shape), tuple(v.shape), tuple(t0.shape), tuple(t.shape)))
    return v, t

DEC_MAX_ROUNDS = 4096                        # decimate_mesh's cap on rounds (max_rounds = 0)
DEC_KEY_NONE = 0x7FFFFFFFFFFFFFFF            # the key of an edge that may not be collapsed
DEC_KEY_UNSCRAMBLE = pow(0x9E3779B1, -1, 1 << 32)      # endpoints_only: the inverse of the multiplier that scrambles the edge id in a key
DEC_FLAGS = {"multiplicity": 1, "link": 2, "boundary": 4, "flip": 8, "finite": 16}      # bits of decimate_round's per-edge flags (include/mirres.h)


def _dec_topology(t, V):
    """The sorts of one decimation round: the distinct undirected edges in key order with their multiplicity, every corner's edge, and the vertex -> corner CSR
    (stable sort: a vertex's corners 3 f + k ascend)."""
    t64 = t.to(torch.int64)
    a = t64.reshape(-1); b = t64[:, [1, 2, 0]].reshape(-1)                        # corner 3 f + k: edge (v_k, v_k+1) of face f
    ekeys, corner_edge, emult = torch.unique((torch.minimum(a, b) << 32) | torch.maximum(a, b), sorted=True, return_inverse=True, return_counts=True)
    vcorner = torch.sort(a, stable=True).indices.to(torch.int32).contiguous()
    vstart = torch.zeros(V + 1, dtype=torch.int32, device=t.device)
    vstart[1:] = torch.cumsum(torch.bincount(a, minlength=V), 0)
    return dict(ekeys=ekeys.contiguous(), emult=emult.to(torch.int32).contiguous(), corner_edge=corner_edge.to(torch.int32).contiguous(), vcorner=vcorner, vstart=vstart,
                E=int(ekeys.shape[0]))


def decimate_round(vertices, quadrics, triangles, target, optimalplacement=True, mark=None, endpoints_only=False):
    """One round of decimate_mesh on device tensors whose indices are in range (vertices f32 [V, 3], quadrics f64 [V, 10] or None before the first round, triangles
    i32 [T, 3], T > target) -> (vertices, quadrics, triangles, info); the inputs are left as they are.  info: the round's edge list and CSR (`ekeys`, `emult`,
    `corner_edge`, `vcorner`, `vstart`, `E`), `vflag`, the quadrics the round started from (`quadrics`), per edge `cost` f64, `position` f32 [E, 3], `flags` i32
    (DEC_FLAGS; 0 = valid) and `keys` i64, the candidates `cand` (edge ids, cheapest first), `sel` u8 per candidate, and `selected`, their number (0: nothing could
    be collapsed, the mesh comes back as it was).  `mark(name)` is called after each stage ("edges", "k_dec_edge", "select", "apply") for timing.
    endpoints_only (without optimalplacement): the midpoint is no candidate, the edge collapses onto the cheaper of its two end points."""
    L = lib(); s = stream_ptr
    mark = mark or (lambda name: None)
    v, t = vertices.clone(), triangles.clone()
    V, T = int(v.shape[0]), int(t.shape[0]); dev = v.device
    tp = _dec_topology(t, V); E = tp["E"]
    vflag = torch.empty(V, dtype=torch.int32, device=dev)
    check(L.mirres_dec_vertex_flags(ptr(tp["ekeys"]), ptr(tp["emult"]), E, V, ptr(vflag), s()), "mirres_dec_vertex_flags")
    if quadrics is None:
        q = torch.empty((V, 10), dtype=torch.float64, device=dev)
        check(L.mirres_dec_quadrics(ptr(v), V, ptr(t), T, ptr(tp["vstart"]), ptr(tp["vcorner"]), ptr(tp["corner_edge"]), ptr(tp["emult"]), E, ptr(q), s()), "mirres_dec_quadrics")
        q0 = q.clone()
    else:
        q0 = quadrics; q = quadrics.clone()
    mark("edges")
    cost = torch.empty(E, dtype=torch.float64, device=dev); pos = torch.empty((E, 3), dtype=torch.float32, device=dev)
    flags = torch.empty(E, dtype=torch.int32, device=dev); keys = torch.empty(E, dtype=torch.int64, device=dev)
    check(L.mirres_dec_edge(ptr(v), ptr(q), V, ptr(t), T, ptr(tp["vstart"]), ptr(tp["vcorner"]), ptr(tp["ekeys"]), ptr(tp["emult"]), ptr(vflag), E, 1 if optimalplacement else (2 if endpoints_only else 0),
                            ptr(cost), ptr(pos), ptr(flags), ptr(keys), s()), "mirres_dec_edge")
    mark("k_dec_edge")
    skeys = torch.sort(keys).values
    n_cand = min((T - int(target) + 1) // 2, int((skeys != DEC_KEY_NONE).sum()))      # only the cheapest ceil((T - target) / 2) valid edges stand this round
    info = dict(tp, vflag=vflag, quadrics=q0, cost=cost, position=pos, flags=flags, keys=keys, cand=skeys[:0].to(torch.int32), sel=torch.empty(0, dtype=torch.uint8, device=dev), selected=0)
    if n_cand <= 0:
        return v, q, t, info
    cand = skeys[:n_cand] & 0xFFFFFFFF
    if endpoints_only and not optimalplacement:
        cand = (cand * DEC_KEY_UNSCRAMBLE) & 0xFFFFFFFF                                 # the key's low word is the edge id times 0x9E3779B1 mod 2^32 in this mode
    cand = cand.to(torch.int32).contiguous()
    vkey = torch.empty(V, dtype=torch.int64, device=dev); sel = torch.empty(n_cand, dtype=torch.uint8, device=dev); cnt = torch.empty(1, dtype=torch.int32, device=dev)
    check(L.mirres_dec_select(ptr(t), T, V, ptr(tp["vstart"]), ptr(tp["vcorner"]), ptr(tp["ekeys"]), E, ptr(keys), ptr(cand), n_cand, ptr(vkey), ptr(sel), ptr(cnt), s()), "mirres_dec_select")
    mark("select")
    remap = torch.empty(V, dtype=torch.int32, device=dev); keep = torch.empty(T, dtype=torch.uint8, device=dev); used = torch.empty(V, dtype=torch.uint8, device=dev)
    h = C.c_int(0)
    check(L.mirres_dec_apply(ptr(v), ptr(q), V, ptr(t), T, ptr(tp["ekeys"]), E, ptr(pos), ptr(cand), ptr(sel), n_cand, ptr(remap), ptr(keep), ptr(used), ptr(cnt), C.byref(h), s()),
          "mirres_dec_apply")
    scratch = torch.empty(int(L.mirres_mesh_scratch_bytes(V, T)), dtype=torch.uint8, device=dev)
    ov = torch.empty_like(v); ot = torch.empty_like(t); counts = (C.c_int * 2)()
    check(L.mirres_mesh_compact(ptr(v), V, ptr(t), T, ptr(keep), ptr(ov), ptr(ot), ptr(scratch), counts, s()), "mirres_mesh_compact")
    q = q[used != 0].contiguous()                                                     # the vertices the kept faces use, in their old order: what the compaction keeps
    if q.shape[0] != counts[0]:
        raise _lib.MirresError("decimate_round: %d quadrics for %d compacted vertices" % (q.shape[0], counts[0]))
    mark("apply")
    info.update(cand=cand, sel=sel, selected=int(h.value), remap=remap, keep=keep)
    return ov[: counts[0]].contiguous(), q, ot[: counts[1]].contiguous(), info


def decimate_mesh(vertices, triangles, target, optimalplacement=True, max_rounds=0, log=None, endpoints_only=False):
    """decimate_mesh (meshutils.py:64-97; nerf/renderer.py:566-567) -> (vertices f32 [V', 3], triangles i32 [T', 3]) with target - 1 <= T' <= target: quadric-error
    edge collapse (Garland & Heckbert 1997) in rounds, every round collapsing an independent set of the cheapest valid edges (decimate_round; csrc/decimate.hip,
    DESIGN.md section 5.10).  Surviving vertices and faces keep their order; equal inputs give equal bytes.  `optimalplacement`: the new vertex minimises the summed
    quadric where the system can be solved, else (and always without it) it is the cheapest of the two end points and their midpoint; `endpoints_only` (without
    optimalplacement) leaves the midpoint out, as MeshLab does with optimalplacement off: the result's vertices are a subset of the input's.  target >= T (or T == 0)
    returns the input.  A round without a valid edge (stall) or `max_rounds` rounds (0: DEC_MAX_ROUNDS) end the run early with one [WARN] line."""
    v, t = _verts(vertices), _tris(triangles)
    V, T0 = int(v.shape[0]), int(t.shape[0]); target = int(target)
    if T0 == 0 or target >= T0:
        return v, t
    if target < 0:
        raise ValueError("decimate_mesh: target %d" % target)
    if not bool(torch.isfinite(v).all()):
        raise ValueError("decimate_mesh: non-finite vertex positions")
    if int(t.min()) < 0 or int(t.max()) >= V:
        raise ValueError("decimate_mesh: face index out of range")
    if T0 > 0x7FFFFFFF // 3:
        raise ValueError("decimate_mesh: %d faces do not fit 32-bit corner indices" % T0)
    cap = DEC_MAX_ROUNDS if int(max_rounds) <= 0 else min(int(max_rounds), DEC_MAX_ROUNDS)
    ov, ot, q, rounds, why = v, t, None, 0, None
    while ot.shape[0] > target:
        if rounds >= cap:
            why = "%d rounds done (max_rounds)" % rounds; break
        ov, q, ot, info = decimate_round(ov, q, ot, target, optimalplacement, endpoints_only=endpoints_only)
        if info["selected"] == 0:
            why = "no edge can be collapsed after %d rounds (stall)" % rounds; break
        rounds += 1
    if why:
        (log or print)("[WARN] mesh decimation stopped at %d faces, target %d: %s" % (ot.shape[0], target, why))
    if log:
        log("[INFO] mesh decimation: %s --> %s, %s --> %s" % (tuple(v.shape), tuple(ov.shape), tuple(t.shape), tuple(ot.shape)))
    return ov, ot


def synthetic_volume(resolution=64, sdf=False):
    """An analytic density (or signed distance) of a unit-free scene for smoke runs and timings: a ball with a dent (radius 0.6 at the default threshold) and a small floater far from it
    that cleaning removes.  Density = -40 * signed distance clipped at 0, so the default threshold 10 cuts it 0.25 inside the zero level."""
    r = int(resolution)
    ax = torch.linspace(-1, 1, r, device=_dev())
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = 0.2                                                                           # the ball sits off-centre: the floater's box stays well below 5 % of the mesh's
    d_ball = torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.85
    d_dent = 0.35 - torch.sqrt((x - c - 0.7) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    d_float = torch.sqrt((x + 0.9) ** 2 + (y + 0.9) ** 2 + (z + 0.9) ** 2) - 0.28
    sd = torch.minimum(torch.maximum(d_ball, d_dent), d_float)
    return sd.contiguous() if sdf else torch.clamp(-40.0 * sd, min=0.0).contiguous()


# the reference's hash-grid configuration (nerf/network.py:77 -> encoding.get_encoder -> GridEncoder defaults): 16 levels of 2 features, base 16, 2^19 entries,
# desired_resolution = 2048 * bound
DENSITY_LEVELS, DENSITY_BASE, DENSITY_LOG2_T, DENSITY_FINEST = 16, 16, 19, 2048


def density_layout(bound=1.0, num_levels=DENSITY_LEVELS, base_resolution=DENSITY_BASE, log2_hashmap_size=DENSITY_LOG2_T, desired_resolution=None):
    """GridEncoder.__init__'s level table (gridencoder/grid.py:104-135) and the kernel's per-level quantities (gridencoder.cu:137-139) -> (_lib.DensityNet with the
    levels filled in and no pointers, total entries).  desired_resolution defaults to 2048 * bound (nerf/network.py:77).  No device is touched."""
    net = _lib.DensityNet()
    desired = float(DENSITY_FINEST * float(bound) if desired_resolution is None else desired_resolution)
    total = int(lib().mirres_density_layout(int(num_levels), int(base_resolution), desired, int(log2_hashmap_size), C.byref(net)))
    if total < 0:
        check(total, "mirres_density_layout")
    return net, total


class DensityField:
    """The stage-0 density network on the device (csrc/density.hip): sigma = exp(sigma_net(encoder(x))[..., 0]) as NeRFNetwork.density computes it
    (nerf/network.py:177-192), table and weights in fp32.
    table f32 [entries, 2] (encoder.embeddings), w0 f32 [64, 32] (sigma_net.0.weight), w1 f32 [16, 64] or its row 0 [64] (sigma_net.1.weight)."""

    def __init__(self, table, w0, w1, bound=1.0, num_levels=DENSITY_LEVELS, base_resolution=DENSITY_BASE, log2_hashmap_size=DENSITY_LOG2_T, desired_resolution=None):
        self.bound = float(bound)
        if not (self.bound > 0 and np.isfinite(self.bound)):
            raise ValueError("DensityField: bound %r" % (bound,))
        self.net, self.entries = density_layout(self.bound, num_levels, base_resolution, log2_hashmap_size, desired_resolution)
        table, w0, w1 = torch.as_tensor(table), torch.as_tensor(w0), torch.as_tensor(w1)
        if table.dim() != 2 or tuple(table.shape) != (self.entries, 2):
            raise ValueError("DensityField: a table of %s, the layout of bound %g has [%d, 2] (a checkpoint trained with another --bound?)" % (tuple(table.shape), self.bound, self.entries))
        if tuple(w0.shape) != (64, 2 * DENSITY_LEVELS):
            raise ValueError("DensityField: sigma_net.0.weight of %s, expected [64, 32]" % (tuple(w0.shape),))
        if w1.dim() == 2:
            if w1.shape[0] < 1 or w1.shape[1] != 64:
                raise ValueError("DensityField: sigma_net.1.weight of %s, expected [16, 64]" % (tuple(w1.shape),))
            w1 = w1[0]
        if tuple(w1.shape) != (64,):
            raise ValueError("DensityField: row 0 of sigma_net.1.weight of %s, expected [64]" % (tuple(w1.shape),))
        dev = _dev()
        self.table = table.detach().to(dev, torch.float32).contiguous()
        self.w0 = w0.detach().to(dev, torch.float32).contiguous()
        self.w1 = w1.detach().to(dev, torch.float32).contiguous()
        self.net.table, self.net.w0, self.net.w1 = self.table.data_ptr(), self.w0.data_ptr(), self.w1.data_ptr()

    @staticmethod
    def _checked_model(ckpt, bound, layout):
        """What from_checkpoint refuses, before anything is copied -> (the model state dict, sigma_net.0.weight, sigma_net.1.weight)."""
        model = ckpt["model"] if "model" in ckpt else ckpt
        if any(k.startswith("encoder.encoder.") for k in model):
            raise NotImplementedError("this checkpoint's encoder is tiny-cuda-nn's (encoder.encoder.params, --tcnn): not supported, only torch-ngp's GridEncoder "
                                      "(encoder.embeddings / encoder.offsets) is")
        for k in ("encoder.embeddings", "encoder.offsets", "sigma_net.0.weight", "sigma_net.1.weight"):
            if k not in model:
                raise KeyError("checkpoint has no %s: not a stage-0 density network" % k)
        net, total = density_layout(bound, **layout)
        want = [int(net.offsets[i]) for i in range(net.num_levels + 1)]
        have = [int(o) for o in torch.as_tensor(model["encoder.offsets"]).reshape(-1).tolist()]
        if have != want:
            raise ValueError("the checkpoint's encoder.offsets (%d levels, %d entries) do not fit the hash-grid layout of --bound %g (%d levels, %d entries): "
                             "pass the --bound the checkpoint was trained with" % (len(have) - 1, have[-1] if have else 0, float(bound), net.num_levels, total))
        w0, w1 = torch.as_tensor(model["sigma_net.0.weight"]), torch.as_tensor(model["sigma_net.1.weight"])
        if tuple(w0.shape) != (64, 32) or tuple(w1.shape) != (16, 64):
            raise ValueError("sigma_net weights of %s and %s: the stage-0 density head is 32 -> 64 -> 16 without biases" % (tuple(w0.shape), tuple(w1.shape)))
        if any(k in model for k in ("sigma_net.0.bias", "sigma_net.1.bias")):
            raise ValueError("sigma_net has biases: the stage-0 density head is bias-free")
        return model, w0, w1

    @classmethod
    def from_checkpoint(cls, ckpt, bound=1.0, **layout):
        """A torch-ngp stage-0 checkpoint dict (or its `model` state dict): encoder.embeddings [N, 2], encoder.offsets [17], sigma_net.0.weight [64, 32],
        sigma_net.1.weight [16, 64].  per_level_scale is not stored in a checkpoint, so the layout is recomputed from `bound` and compared with the stored offsets."""
        model, w0, w1 = cls._checked_model(ckpt, bound, layout)
        return cls(model["encoder.embeddings"], w0, w1, bound=bound, **layout)

    def _points(self, x, want_feat):
        x = torch.as_tensor(x).to(_dev(), torch.float32)
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("DensityField: positions of %s, expected [n, 3]" % (tuple(x.shape),))
        x = x.contiguous(); n = int(x.shape[0])
        sigma = torch.empty(n, dtype=torch.float32, device=x.device)
        feat = torch.empty((n, 2 * DENSITY_LEVELS), dtype=torch.float32, device=x.device) if want_feat else None
        check(lib().mirres_density_points(C.byref(self.net), ptr(x) if n else None, n, self.bound, ptr(sigma) if n else None, ptr(feat) if (want_feat and n) else None,
                                          stream_ptr()), "mirres_density_points")
        return sigma, feat

    def encode(self, x):
        """x [n, 3] -> the encoder's output f32 [n, 32] (feature 2 l + c: channel c of level l); all zero for a point outside [-bound, bound]^3."""
        return self._points(x, True)[1]

    def density(self, x):
        """x [n, 3] -> sigma f32 [n]."""
        return self._points(x, False)[0]

    def volume(self, resolution, grid_vol=None, thresh=None):
        """sigma on the lattice torch.linspace(-1, 1, R) per axis (nerf/renderer.py:516-530; `resolution` one int or three) -> f32 [Rx, Ry, Rz].  With grid_vol
        [S, S, S] and thresh: lattice points whose nearest grid cell does not pass > thresh are exactly 0 and are not evaluated (:532-541)."""
        res = [int(resolution)] * 3 if np.ndim(resolution) == 0 else [int(r) for r in resolution]
        if len(res) != 3 or min(res) < 1:
            raise ValueError("DensityField.volume: resolution %r" % (resolution,))
        dev = _dev()
        axes = [torch.linspace(-1, 1, r).to(dev).contiguous() for r in res]      # built on the host and copied, as the reference does (:518-528)
        g, S = None, 0
        if grid_vol is not None:
            if thresh is None:
                raise ValueError("DensityField.volume: a grid_vol needs a thresh")
            g = torch.as_tensor(grid_vol).to(dev, torch.float32).contiguous()
            if g.dim() != 3 or len(set(g.shape)) != 1:
                raise ValueError("DensityField.volume: a cubic grid_vol expected, got %s" % (tuple(g.shape),))
            S = int(g.shape[0])
        out = torch.empty(res, dtype=torch.float32, device=dev)
        check(lib().mirres_density_volume(C.byref(self.net), ptr(axes[0]), res[0], ptr(axes[1]), res[1], ptr(axes[2]), res[2], self.bound, ptr(g), S,
                                          float(thresh) if g is not None else 0.0, ptr(out), stream_ptr()), "mirres_density_volume")
        return out

    @torch.no_grad()
    def grad_total_variation(self, weight=1e-7, inputs=None, grad=None, B=1000000, generator=None):
        """GridEncoder.grad_total_variation (gridencoder/grid.py:170-192; csrc/grid_tv.hip): adds the total-variation term of every level's cell under every
        point to the table's gradient, in place -> None.  To be called after loss.backward() and before optimizer.step().  inputs [..., 3]: world positions; None
        or empty: B points uniform in [-bound, bound]^3 (the reference's random branch; `generator`: a device generator for them).  grad: a contiguous fp32
        device tensor of the table's shape (default: self.table.grad).  The dense levels' sum has one fixed set of bits for a given set of points; the hashed
        levels are summed by fp32 atomics in no fixed order.  One workspace tensor is kept per field."""
        if grad is None:
            grad = self.table.grad
            if grad is None:
                raise ValueError("grad is None, should be called after loss.backward() and before optimizer.step()!")
        if not torch.is_tensor(grad):
            raise TypeError("grad_total_variation: grad must be a tensor, got %s" % type(grad).__name__)
        if grad.dtype != torch.float32 or grad.device != self.table.device:
            raise TypeError("grad_total_variation: grad must be fp32 on the table's device, got %s on %s" % (grad.dtype, grad.device))
        if tuple(grad.shape) != tuple(self.table.shape) or not grad.is_contiguous():
            raise ValueError("grad_total_variation: grad of %s%s, the table has %s" % (tuple(grad.shape), "" if grad.is_contiguous() else " (not contiguous)", tuple(self.table.shape)))
        weight = float(weight)
        dev = self.table.device
        if inputs is None or torch.as_tensor(inputs).numel() == 0:
            x = (torch.rand(int(B), 3, dtype=torch.float32, device=dev, generator=generator) * 2 - 1) * self.bound
        else:
            x = torch.as_tensor(inputs)
            if x.shape[-1] != 3:
                raise ValueError("grad_total_variation: inputs of %s, expected [..., 3]" % (tuple(x.shape),))
            x = x.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        n = int(x.shape[0])
        L = lib()
        nbytes = int(L.mirres_grid_tv_workspace_bytes(C.byref(self.net)))
        if nbytes < 0:
            check(nbytes, "mirres_grid_tv_workspace_bytes")
        ws = getattr(self, "_tv_workspace", None)
        if ws is None or ws.device != dev or ws.numel() * 4 < nbytes:
            ws = self._tv_workspace = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        check(L.mirres_grid_tv_grad(C.byref(self.net), ptr(x) if n else None, n, self.bound, weight, ptr(grad), ptr(ws), ws.numel() * 4, stream_ptr()), "mirres_grid_tv_grad")
        return None


class DensityGrid:
    """The occupancy grid the ray marchers read, and its upkeep (nerf/renderer.py:1438-1595; csrc/raymarch.hip): density_grid f32 [C, H^3] in Morton order,
    density_bitfield u8 [C * H^3 / 8], mean_density and iter_density, as NeRFRenderer keeps them for --cuda_ray.  C = cascade_of_bound(bound); cascade c covers
    [-min(2^c, bound), min(2^c, bound)]^3."""

    def __init__(self, bound=1.0, grid_size=128, density_thresh=10.0, min_near=0.2, density_grid=None, density_bitfield=None, aabb_train=None, mean_density=0.0,
                 sdf=False, trainable_density_grid=False):
        from . import checkpoint as CK
        if sdf:
            raise NotImplementedError("DensityGrid: the --sdf branch of update_extra_state (renderer.py:1567-1569) is not built")
        if trainable_density_grid:
            raise NotImplementedError("DensityGrid: --trainable_density_grid (renderer.py:1578-1586) is not built")
        self.bound = float(bound)
        H = int(grid_size)
        if not (self.bound > 0 and np.isfinite(self.bound)):
            raise ValueError("DensityGrid: bound %r" % (bound,))
        if H < 2 or H > 1024 or H & (H - 1):
            raise ValueError("DensityGrid: grid_size %d is not a power of two in [2, 1024]" % H)
        self.grid_size, self.cascade = H, int(CK.cascade_of_bound(self.bound))
        if self.cascade > 8:
            raise ValueError("DensityGrid: bound %g needs %d cascades, at most 8 are supported" % (self.bound, self.cascade))
        self.density_thresh, self.min_near = float(density_thresh), float(min_near)
        cells = self.cascade * H ** 3
        if density_grid is not None:
            g = torch.as_tensor(density_grid)
            if g.numel() != cells:
                raise ValueError("DensityGrid: a density_grid of %s, bound %g and grid_size %d have [%d, %d]" % (tuple(g.shape), self.bound, H, self.cascade, H ** 3))
        if density_bitfield is not None:
            b = torch.as_tensor(density_bitfield)
            if b.dtype != torch.uint8 or b.numel() != cells // 8:
                raise ValueError("DensityGrid: a density_bitfield of %s %s, expected uint8 [%d]" % (b.dtype, tuple(b.shape), cells // 8))
        if aabb_train is not None and torch.as_tensor(aabb_train).numel() != 6:
            raise ValueError("DensityGrid: aabb_train of %s, expected [6]" % (tuple(torch.as_tensor(aabb_train).shape),))
        dev = _dev()
        self.density_grid = (torch.zeros(self.cascade, H ** 3, dtype=torch.float32, device=dev) if density_grid is None
                             else g.detach().to(dev, torch.float32).reshape(self.cascade, H ** 3).contiguous().clone())
        self.density_bitfield = (torch.zeros(cells // 8, dtype=torch.uint8, device=dev) if density_bitfield is None else b.detach().to(dev).reshape(-1).contiguous().clone())
        b_ = self.bound
        self.aabb_train = (torch.tensor([-b_, -b_, -b_, b_, b_, b_], dtype=torch.float32, device=dev) if aabb_train is None
                           else torch.as_tensor(aabb_train).detach().to(dev, torch.float32).reshape(6).contiguous())
        self.mean_density, self.iter_density = float(mean_density), 0

    @classmethod
    def from_checkpoint(cls, ckpt, bound=1.0, **kw):
        """A stage-0 checkpoint dict (or its `model`): density_grid [C, H^3] and, when present, density_bitfield and aabb_train; mean_density from the top level."""
        model = ckpt["model"] if "model" in ckpt else ckpt
        if "density_grid" not in model:
            raise KeyError("checkpoint has no density_grid")
        g = torch.as_tensor(model["density_grid"])
        if g.dim() != 2:
            raise ValueError("the checkpoint's density_grid of %s is not [cascade, H^3]" % (tuple(g.shape),))
        H = int(round(g.shape[1] ** (1.0 / 3.0)))
        if H ** 3 != g.shape[1]:
            raise ValueError("density_grid: %d values per cascade is not a cube" % g.shape[1])
        return cls(bound=bound, grid_size=H, density_grid=g, density_bitfield=model.get("density_bitfield"), aabb_train=model.get("aabb_train"),
                   mean_density=float(ckpt.get("mean_density", 0.0)) if "model" in ckpt else 0.0, **kw)

    def mark_untrained(self, poses, intrinsics, aabb_train=None, min_near=None, cam_near_far=None):
        """mark_untrained_grid (renderer.py:1438-1524) in one kernel: poses [B, 4, 4] camera-to-world, intrinsics [4] or [B, 4] (fx, fy, cx, cy), cam_near_far [B, 2] or
        None (then min_near).  Cells no camera covers or outside aabb_train by more than half a cell become -1 -> how many cells are at -1 now marked."""
        dev = _dev()
        poses = torch.as_tensor(poses).detach().to(dev, torch.float32)
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
            raise ValueError("mark_untrained: poses of %s, expected [B, 4, 4]" % (tuple(poses.shape),))
        B = int(poses.shape[0])
        K = torch.as_tensor(intrinsics).detach().to(dev, torch.float32)
        if tuple(K.shape) not in ((4,), (1, 4), (B, 4)):
            raise ValueError("mark_untrained: intrinsics of %s, expected [4] or [%d, 4]" % (tuple(K.shape), B))
        per_cam = int(K.dim() == 2 and K.shape[0] == B and B > 1)
        nf = None
        if cam_near_far is not None:
            nf = torch.as_tensor(cam_near_far).detach().to(dev, torch.float32).contiguous()
            if tuple(nf.shape) != (B, 2):
                raise ValueError("mark_untrained: cam_near_far of %s, expected [%d, 2]" % (tuple(nf.shape), B))
        aabb = self.aabb_train if aabb_train is None else torch.as_tensor(aabb_train).detach().to(dev, torch.float32).reshape(-1).contiguous()
        if aabb.numel() != 6:
            raise ValueError("mark_untrained: aabb_train of %d values, expected 6" % aabb.numel())
        poses, K = poses.contiguous(), K.reshape(-1).contiguous()
        check(lib().mirres_rm_grid_mark_untrained(ptr(self.density_grid), self.cascade, self.grid_size, self.bound, ptr(poses) if B else None, B, ptr(K), per_cam,
                                                  ptr(nf), float(self.min_near if min_near is None else min_near), ptr(aabb), stream_ptr()), "mirres_rm_grid_mark_untrained")
        return int((self.density_grid == -1).sum().item())

    def update(self, field, decay=0.95, noise=None):
        """update_extra_state (renderer.py:1527-1595) for the non-trainable grid: one fused kernel over all cascades evaluates `field` (a DensityField) at every cell's
        jittered lattice point and writes max(grid * decay, sigma) where both are >= 0; then mean_density from torch, iter_density += 1, and the bitfield packed at
        min(mean_density, density_thresh).  noise f32 [C, H^3, 3] in [0, 1) (Morton order), or None for torch.rand."""
        from . import raymarching
        if not isinstance(field, DensityField):
            raise TypeError("DensityGrid.update: field must be a DensityField, got %s" % type(field).__name__)
        H, Cn = self.grid_size, self.cascade
        if noise is None:
            noise = torch.rand(Cn, H ** 3, 3, dtype=torch.float32, device=self.density_grid.device)
        else:
            noise = torch.as_tensor(noise)
            if tuple(noise.shape) != (Cn, H ** 3, 3):
                raise ValueError("DensityGrid.update: noise of %s, expected [%d, %d, 3]" % (tuple(noise.shape), Cn, H ** 3))
            noise = noise.detach().to(self.density_grid.device, torch.float32).contiguous()
        check(lib().mirres_rm_grid_update(C.byref(field.net), field.bound, ptr(self.density_grid), Cn, H, self.bound, ptr(noise), float(decay), stream_ptr()),
              "mirres_rm_grid_update")
        self.mean_density = torch.mean(self.density_grid.clamp(min=0)).item()      # -1 cells count as 0 (renderer.py:1588)
        self.iter_density += 1
        self.density_bitfield = raymarching.packbits(self.density_grid, min(self.mean_density, self.density_thresh), self.density_bitfield)
        return None


SH_DIM, GEO_FEAT_DIM, COLOR_HIDDEN = 16, 15, 64      # encoder_dir's outputs (degree 4), geo_feat, the colour net's width (nerf/network.py:68-72, 98)


class RadianceField(DensityField):
    """The stage-0 radiance network on the device (csrc/radiance.hip): NeRFNetwork.forward(x, d) (nerf/network.py:146-174) in one fused query per point, table and
    weights in fp32.  On top of DensityField's table and w0: w1 f32 [16, 64] (sigma_net.1.weight, all rows: row 0 is sigma, rows 1 .. 15 geo_feat), c0 f32 [64, 31]
    (color_net.0.weight, input [sh(16), geo_feat(15)]), c1 f32 [64, 64], c2 f32 [3, 64]; no biases.  encoder_dir (spherical harmonics, degree 4) has no
    parameters.  density, encode and volume are DensityField's, on the same table."""

    def __init__(self, table, w0, w1, c0, c1, c2, bound=1.0, **layout):
        w1, c0, c1, c2 = (torch.as_tensor(w) for w in (w1, c0, c1, c2))
        if tuple(w1.shape) != (1 + GEO_FEAT_DIM, 64):
            raise ValueError("RadianceField: sigma_net.1.weight of %s, expected [16, 64] (all rows: 1 .. 15 are geo_feat)" % (tuple(w1.shape),))
        for name, w, shape in (("color_net.0.weight", c0, (COLOR_HIDDEN, SH_DIM + GEO_FEAT_DIM)), ("color_net.1.weight", c1, (COLOR_HIDDEN, COLOR_HIDDEN)),
                               ("color_net.2.weight", c2, (3, COLOR_HIDDEN))):
            if tuple(w.shape) != shape:
                raise ValueError("RadianceField: %s of %s, expected %s" % (name, tuple(w.shape), list(shape)))
        super().__init__(table, w0, w1, bound=bound, **layout)
        dev = self.table.device
        self.w1_full, self.c0, self.c1, self.c2 = (w.detach().to(dev, torch.float32).contiguous() for w in (w1, c0, c1, c2))
        # DensityField kept a copy of row 0; here the density head reads row 0 of w1_full itself (the first 64 floats of a contiguous [16, 64]), so that density()
        # and DensityGrid.update follow an optimiser's in-place steps on w1_full
        self.w1 = self.w1_full[0]
        self.net.w1 = self.w1_full.data_ptr()
        self.bwd_max_blocks = 0                          # forward_train's backward: the grid of mirres_radiance_points_bwd (0: the library's default)
        self.rnet = _lib.RadianceNet()
        self.rnet.grid = self.net
        self.rnet.w1, self.rnet.c0, self.rnet.c1, self.rnet.c2 = self.w1_full.data_ptr(), self.c0.data_ptr(), self.c1.data_ptr(), self.c2.data_ptr()

    @classmethod
    def from_checkpoint(cls, ckpt, bound=1.0, **layout):
        """A torch-ngp stage-0 checkpoint dict (or its `model`): what DensityField.from_checkpoint reads and refuses, and color_net.{0,1,2}.weight of [64, 31],
        [64, 64] and [3, 64] without biases."""
        model, w0, w1 = cls._checked_model(ckpt, bound, layout)
        keys = ["color_net.%d.weight" % l for l in range(3)]
        for k in keys:
            if k not in model:
                raise KeyError("checkpoint has no %s: not a stage-0 radiance network" % k)
        c0, c1, c2 = (torch.as_tensor(model[k]) for k in keys)
        if tuple(c0.shape) != (64, 31) or tuple(c1.shape) != (64, 64) or tuple(c2.shape) != (3, 64):
            raise ValueError("color_net weights of %s, %s and %s: the stage-0 colour net is 31 -> 64 -> 64 -> 3 without biases" % (tuple(c0.shape), tuple(c1.shape), tuple(c2.shape)))
        if any(k.startswith("color_net.") and k.endswith(".bias") for k in model):
            raise ValueError("color_net has biases: the stage-0 colour net is bias-free")
        return cls(model["encoder.embeddings"], w0, w1, c0, c1, c2, bound=bound, **layout)

    @staticmethod
    def _n3(t, what):
        t = torch.as_tensor(t).to(_dev(), torch.float32)
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("RadianceField: %s of %s, expected [n, 3]" % (what, tuple(t.shape)))
        return t.contiguous()

    def _query(self, x, d, want_sigma=True, want_aux=False):
        """-> (sigma or None, rgb, h16 or None, sh or None): one launch."""
        x, d = self._n3(x, "positions"), self._n3(d, "directions")
        if x.shape[0] != d.shape[0]:
            raise ValueError("RadianceField: %d positions and %d directions" % (x.shape[0], d.shape[0]))
        n = int(x.shape[0])
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)
        sigma = new(n) if want_sigma else None
        rgb = new(n, 3)
        h16, sh = (new(n, 1 + GEO_FEAT_DIM), new(n, SH_DIM)) if want_aux else (None, None)
        p = (lambda t: ptr(t) if (t is not None and n) else None)
        check(lib().mirres_radiance_points(C.byref(self.rnet), p(x), p(d), n, self.bound, p(sigma), p(rgb), p(h16), p(sh), stream_ptr()), "mirres_radiance_points")
        return sigma, rgb, h16, sh

    def forward(self, x, d):
        """x [n, 3], d [n, 3] (any length; the encoder normalises) -> (sigma f32 [n], rgb f32 [n, 3]); sigma has DensityField.density's bits."""
        return self._query(x, d)[:2]

    def rgb(self, x, d):
        """NeRFNetwork.rgb: the colour alone, with forward's bits."""
        return self._query(x, d, want_sigma=False)[1]

    def sh(self, d):
        """d [n, 3] -> encoder_dir's output f32 [n, 16]; NaN for a zero or non-finite direction (the reference's 0 / 0)."""
        d = self._n3(d, "directions")
        n = int(d.shape[0])
        out = torch.empty((n, SH_DIM), dtype=torch.float32, device=d.device)
        check(lib().mirres_sh_encode(ptr(d) if n else None, n, ptr(out) if n else None, stream_ptr()), "mirres_sh_encode")
        return out

    PARAMETER_NAMES = ("table", "w0", "w1_full", "c0", "c1", "c2")

    def parameters(self):
        """The six trainable tensors (PARAMETER_NAMES: table, w0, w1_full, c0, c1, c2) as leaf tensors with requires_grad, for an optimiser.  They are the tensors the
        kernels read: in-place updates (optimizer.step()) are seen by every later query, density() and DensityGrid.update included; assigning a new tensor is not."""
        return [getattr(self, k).requires_grad_(True) for k in self.PARAMETER_NAMES]

    @classmethod
    def init_random(cls, bound=1.0, seed=0, **layout):
        """A freshly initialised network as the reference builds it: the table U(-1e-4, 1e-4) (gridencoder/grid.py reset_parameters), the five bias-free matrices
        nn.Linear's default U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), all from one host generator seeded with `seed`."""
        _, total = density_layout(bound, **layout)
        g = torch.Generator().manual_seed(int(seed))
        table = (torch.rand((total, 2), generator=g, dtype=torch.float32) * 2 - 1) * 1e-4
        lin = lambda o, i: (torch.rand((o, i), generator=g, dtype=torch.float32) * 2 - 1) / float(np.sqrt(i))
        return cls(table, lin(64, 2 * DENSITY_LEVELS), lin(1 + GEO_FEAT_DIM, 64), lin(COLOR_HIDDEN, SH_DIM + GEO_FEAT_DIM), lin(COLOR_HIDDEN, COLOR_HIDDEN),
                   lin(3, COLOR_HIDDEN), bound=bound, **layout)

    def backward_points(self, x, d, grad_sigma, grad_rgb, grads=None, max_blocks=None):
        """The adjoint of forward (csrc/radiance_bwd.hip), one mirres_radiance_points_bwd call: x, d [n, 3], grad_sigma [n] or None (zeros), grad_rgb [n, 3] ->
        the gradients of PARAMETER_NAMES, fp32.  grads: six tensors to ADD to (default: fresh zeros).  The weight gradients are bit-reproducible for one max_blocks
        (None: self.bwd_max_blocks); the table gradient is scattered with atomics and is not.  Positions and directions get no gradient."""
        x, d = self._n3(x, "positions"), self._n3(d, "directions")
        n = int(x.shape[0])
        grad_rgb = torch.as_tensor(grad_rgb).to(x.device, torch.float32).contiguous()
        if d.shape[0] != n or tuple(grad_rgb.shape) != (n, 3):
            raise ValueError("RadianceField: %d positions, %d directions and grad_rgb of %s" % (n, d.shape[0], tuple(grad_rgb.shape)))
        if grad_sigma is not None:
            grad_sigma = torch.as_tensor(grad_sigma).to(x.device, torch.float32).contiguous()
            if tuple(grad_sigma.shape) != (n,):
                raise ValueError("RadianceField: grad_sigma of %s for %d points" % (tuple(grad_sigma.shape), n))
        params = [getattr(self, k) for k in self.PARAMETER_NAMES]
        if grads is None:
            grads = [torch.zeros(w.shape, dtype=torch.float32, device=x.device) for w in params]
        for g, w, k in zip(grads, params, self.PARAMETER_NAMES):
            if g.shape != w.shape or g.dtype != torch.float32 or not g.is_contiguous() or g.device != w.device:
                raise ValueError("RadianceField: the gradient buffer of %s must be a contiguous fp32 %s on the field's device" % (k, tuple(w.shape)))
        mb = int(self.bwd_max_blocks if max_blocks is None else max_blocks)
        L = lib()
        nbytes = int(L.mirres_radiance_bwd_workspace_bytes(n, mb))
        if nbytes < 0:
            check(nbytes, "mirres_radiance_bwd_workspace_bytes")
        ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
        p = (lambda t: ptr(t) if (t is not None and n) else None)
        check(L.mirres_radiance_points_bwd(C.byref(self.rnet), p(x), p(d), n, self.bound, p(grad_sigma), p(grad_rgb), *(ptr(g) for g in grads), ptr(ws), nbytes, mb,
                                           stream_ptr()), "mirres_radiance_points_bwd")
        return grads

    def forward_train(self, x, d):
        """forward with gradients: (sigma [n], rgb [n, 3]) with forward's bits, differentiable in parameters() (not in x or d).  The forward is one
        mirres_radiance_points launch; nothing but x and d is kept, the backward recomputes (backward_points)."""
        return _RadianceTrain.apply(self, self._n3(x, "positions").detach(), self._n3(d, "directions").detach(), *[getattr(self, k) for k in self.PARAMETER_NAMES])

    def backward_pos(self, x, d, grad_sigma, grad_rgb):
        """The position adjoint of forward (csrc/radiance_pos.hip), one mirres_radiance_points_bwd_pos call: x, d [n, 3], grad_sigma [n] or None (zeros),
        grad_rgb [n, 3] -> d / dx f32 [n, 3]; exactly 0 for a point out of bounds.  No atomics: equal inputs give equal bits.  Directions get no gradient."""
        x, d = self._n3(x, "positions"), self._n3(d, "directions")
        n = int(x.shape[0])
        grad_rgb = torch.as_tensor(grad_rgb).to(x.device, torch.float32).contiguous()
        if d.shape[0] != n or tuple(grad_rgb.shape) != (n, 3):
            raise ValueError("RadianceField: %d positions, %d directions and grad_rgb of %s" % (n, d.shape[0], tuple(grad_rgb.shape)))
        if grad_sigma is not None:
            grad_sigma = torch.as_tensor(grad_sigma).to(x.device, torch.float32).contiguous()
            if tuple(grad_sigma.shape) != (n,):
                raise ValueError("RadianceField: grad_sigma of %s for %d points" % (tuple(grad_sigma.shape), n))
        out = torch.empty((n, 3), dtype=torch.float32, device=x.device)
        p = (lambda t: ptr(t) if (t is not None and n) else None)
        check(lib().mirres_radiance_points_bwd_pos(C.byref(self.rnet), p(x), p(d), n, self.bound, p(grad_sigma), p(grad_rgb), p(out), stream_ptr()),
              "mirres_radiance_points_bwd_pos")
        return out

    def rgb_train(self, x, d, pos_grad=False):
        """rgb with gradients, what stage 1 asks of self.rgb(xyzs, dirs) (nerf/renderer.py:1046-1052): rgb()'s bits from one mirres_radiance_points launch without
        sigma, differentiable in parameters() (backward_points with no grad_sigma) and, with pos_grad (--enable_offset_nerf_grad) and x.requires_grad, in x
        (backward_pos); otherwise x gets no gradient.  d never does."""
        x = self._n3(x, "positions")
        if not pos_grad:
            x = x.detach()
        return _RadianceRgbTrain.apply(self, x, self._n3(d, "directions").detach(), *[getattr(self, k) for k in self.PARAMETER_NAMES])


class _RadianceTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, x, d, *params):
        sigma, rgb = field._query(x, d)[:2]
        ctx.field = field
        ctx.save_for_backward(x, d)
        return sigma, rgb

    @staticmethod
    def backward(ctx, grad_sigma, grad_rgb):
        x, d = ctx.saved_tensors
        if grad_rgb is None:
            grad_rgb = torch.zeros((x.shape[0], 3), dtype=torch.float32, device=x.device)
        grads = ctx.field.backward_points(x, d, grad_sigma, grad_rgb)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


class _RadianceRgbTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, x, d, *params):
        rgb = field._query(x, d, want_sigma=False)[1]
        ctx.field = field
        ctx.save_for_backward(x, d)
        return rgb

    @staticmethod
    def backward(ctx, grad_rgb):
        x, d = ctx.saved_tensors
        grad_rgb = grad_rgb.contiguous()
        gp = (None,) * 6
        if any(ctx.needs_input_grad[3:]):
            grads = ctx.field.backward_points(x, d, None, grad_rgb)
            gp = tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))
        gx = ctx.field.backward_pos(x, d, None, grad_rgb) if ctx.needs_input_grad[1] else None
        return (None, gx, None) + gp


def _safe_normalize(x, eps=1e-20):
    """nerf/utils.py:43-44."""
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def _bg_color(bg_color, N):
    """None -> 1; a scalar, [3] or [N, 3] -> what broadcasts against image [N, 3] (a tensor stays where it is)."""
    if bg_color is None:
        return 1
    if isinstance(bg_color, (int, float)):
        return float(bg_color)
    bg = torch.as_tensor(bg_color)
    if bg.dim() == 0 or tuple(bg.shape) in ((3,), (N, 3)):
        return bg
    raise ValueError("render_stage0: bg_color of %s, expected a scalar, [3] or [%d, 3]" % (tuple(bg.shape), N))


@torch.no_grad()
def render_stage0(field, grid, rays_o, rays_d, bg_color=None, dt_gamma=0, max_steps=1024, T_thresh=1e-4, cam_near_far=None, perturb=False, min_near=None, aabb=None):
    """The INFERENCE branch of NeRFRenderer.render (nerf/renderer.py:714-717, 778-839) over the ray-marching operators -> {"image" [N, 3], "depth" [N],
    "weights_sum" [N]}: near_far_from_aabb (aabb: 6 values, default the grid's aabb_train; min_near: default the grid's), the optional cam_near_far [N, 2] clamp,
    then while step < max_steps with n_step = max(min(N // n_alive, 8), 1): march_rays (perturb on the first step only) -> safe_normalize(dirs) in torch as the
    reference writes it -> field.forward -> composite_rays -> compaction of rays_alive; last image + (1 - weights_sum) * bg_color (None: 1; a scalar, [3] or [N, 3]).
    field: a RadianceField; grid: a DensityGrid with its bitfield.  rays_o, rays_d [..., 3]; the outputs are flat.
    The training branch is render_stage0_train.  Not built: --sdf and individual_codes."""
    from . import raymarching as RM
    if not isinstance(field, RadianceField):
        raise TypeError("render_stage0: field must be a RadianceField, got %s" % type(field).__name__)
    if not isinstance(grid, DensityGrid):
        raise TypeError("render_stage0: grid must be a DensityGrid, got %s" % type(grid).__name__)
    max_steps = int(max_steps)
    if max_steps < 1:
        raise ValueError("render_stage0: max_steps %d" % max_steps)
    rays_o, rays_d = torch.as_tensor(rays_o), torch.as_tensor(rays_d)
    if rays_o.shape != rays_d.shape or rays_o.dim() < 1 or rays_o.shape[-1] != 3:
        raise ValueError("render_stage0: rays_o %s and rays_d %s, expected two [..., 3] of one shape" % (tuple(rays_o.shape), tuple(rays_d.shape)))
    N = int(rays_o.numel() // 3)
    if cam_near_far is not None:
        cam_near_far = torch.as_tensor(cam_near_far)
        if tuple(cam_near_far.shape) != (N, 2):
            raise ValueError("render_stage0: cam_near_far of %s, expected [%d, 2]" % (tuple(cam_near_far.shape), N))
    if aabb is not None and torch.as_tensor(aabb).numel() != 6:
        raise ValueError("render_stage0: aabb of %d values, expected 6" % torch.as_tensor(aabb).numel())
    bg = _bg_color(bg_color, N)
    dev = _dev()
    if torch.is_tensor(bg):
        bg = bg.to(dev, torch.float32)
    rays_o = rays_o.to(dev, torch.float32).contiguous().view(-1, 3)
    rays_d = rays_d.to(dev, torch.float32).contiguous().view(-1, 3)
    box = grid.aabb_train if aabb is None else torch.as_tensor(aabb).to(dev, torch.float32).reshape(6)
    nears, fars = RM.near_far_from_aabb(rays_o, rays_d, box, grid.min_near if min_near is None else float(min_near))
    if cam_near_far is not None:
        cam_near_far = cam_near_far.to(dev, torch.float32)
        nears = torch.maximum(nears, cam_near_far[:, 0])
        fars = torch.minimum(fars, cam_near_far[:, 1])
    weights_sum = torch.zeros(N, dtype=torch.float32, device=dev)
    depth = torch.zeros(N, dtype=torch.float32, device=dev)
    image = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    rays_alive = torch.arange(N, dtype=torch.int32, device=dev)
    rays_t = nears.clone()
    step = 0
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, ts = RM.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid.bound, False, grid.density_bitfield, grid.cascade, grid.grid_size,
                                       nears, fars, perturb if step == 0 else False, dt_gamma, max_steps)
        sigmas, rgbs = field.forward(xyzs, _safe_normalize(dirs))
        RM.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh, False)
        rays_alive = rays_alive[rays_alive >= 0]
        step += n_step
    image = image + (1 - weights_sum).unsqueeze(-1) * bg
    return {"image": image, "depth": depth, "weights_sum": weights_sum}


def render_stage0_train(field, grid, rays_o, rays_d, bg_color=None, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4, cam_near_far=None, noises=None):
    """The TRAINING branch of NeRFRenderer.render (nerf/renderer.py:735-773, 830-838) -> {"image" [N, 3], "depth" [N], "weights_sum" [N], "weights" [M],
    "num_points" M, "xyzs" [M, 3]}, differentiable in field.parameters(): near_far_from_aabb on the grid's aabb_train (min_near the grid's), the optional
    cam_near_far [N, 2] clamp, march_rays_train (perturb; noises [N] in [0, 1) or None for torch.rand), safe_normalize(dirs), field.forward_train,
    composite_rays_train, image + (1 - weights_sum) * bg_color (None: 1; a scalar, [3] or [N, 3]).  rays_o, rays_d [..., 3]; the outputs are flat."""
    from . import raymarching as RM
    if not isinstance(field, RadianceField):
        raise TypeError("render_stage0_train: field must be a RadianceField, got %s" % type(field).__name__)
    if not isinstance(grid, DensityGrid):
        raise TypeError("render_stage0_train: grid must be a DensityGrid, got %s" % type(grid).__name__)
    rays_o, rays_d = torch.as_tensor(rays_o), torch.as_tensor(rays_d)
    if rays_o.shape != rays_d.shape or rays_o.dim() < 1 or rays_o.shape[-1] != 3:
        raise ValueError("render_stage0_train: rays_o %s and rays_d %s, expected two [..., 3] of one shape" % (tuple(rays_o.shape), tuple(rays_d.shape)))
    N = int(rays_o.numel() // 3)
    bg = _bg_color(bg_color, N)
    dev = _dev()
    if torch.is_tensor(bg):
        bg = bg.to(dev, torch.float32)
    rays_o = rays_o.detach().to(dev, torch.float32).contiguous().view(-1, 3)
    rays_d = rays_d.detach().to(dev, torch.float32).contiguous().view(-1, 3)
    nears, fars = RM.near_far_from_aabb(rays_o, rays_d, grid.aabb_train, grid.min_near)
    if cam_near_far is not None:
        cam_near_far = torch.as_tensor(cam_near_far)
        if tuple(cam_near_far.shape) != (N, 2):
            raise ValueError("render_stage0_train: cam_near_far of %s, expected [%d, 2]" % (tuple(cam_near_far.shape), N))
        cam_near_far = cam_near_far.to(dev, torch.float32)
        nears = torch.maximum(nears, cam_near_far[:, 0])
        fars = torch.minimum(fars, cam_near_far[:, 1])
    xyzs, dirs, ts, rays = RM.march_rays_train(rays_o, rays_d, grid.bound, False, grid.density_bitfield, grid.cascade, grid.grid_size, nears, fars, perturb, dt_gamma,
                                               max_steps, noises)
    sigmas, rgbs = field.forward_train(xyzs, _safe_normalize(dirs))
    weights, weights_sum, depth, image = RM.composite_rays_train(sigmas, rgbs, ts, rays, T_thresh, False)
    image = image + (1 - weights_sum).unsqueeze(-1) * bg
    return {"image": image, "depth": depth, "weights_sum": weights_sum, "weights": weights, "num_points": int(xyzs.shape[0]), "xyzs": xyzs}


def _synthetic_outer_row(S, k, c, A):
    """Row k >= 1 of synthetic_checkpoint's density_grid in [x][y][z] order: the scene at the centres of cascade k's cells (world = normalised * 2^k)."""
    cc = (np.arange(S, dtype=np.float64) + 0.5) / S * 2.0 - 1.0
    x, y, z = (w * 2.0 ** k for w in np.meshgrid(cc, cc, cc, indexing="ij"))
    r = np.sqrt(x * x + y * y + z * z)
    row = np.exp(c * (A - r))                                                   # the ball
    solid = np.zeros(row.shape, bool)
    for j in range(1, k + 1):                                                   # cascade j's slab and dome, at its own scale
        u = 2.0 ** j
        solid |= (z > -0.85 * u) & (z < -0.6 * u) & (np.abs(x) < 0.85 * u) & (np.abs(y) < 0.85 * u)
        solid |= (r > 0.7 * u) & (r < 0.9 * u) & (z > 0.25 * u)
    row[solid] = np.exp(c * A)
    row[(x > 0.9 * 2.0 ** k) & (y > 0.9 * 2.0 ** k)] = -1.0                     # a column of cells no training step has updated (torch-ngp marks them -1)
    return row.astype(np.float32)


def synthetic_checkpoint(S=16, radius=0.6, cascades=1):
    """A stage-0 checkpoint dict (bound 1, the reference's hash-grid configuration) whose network encodes a ball, for tests and smoke runs: feature 0 of level 0
    holds 2 - |x| at the level's vertices (vertex i of an axis sits at u = (i - 0.5) / 15), every other table entry is 0, W0[0, 0] = c = 1.5, W1[0, 0] = 1 and all
    other weights are 0, so sigma = exp(1.5 * trilinear(2 - |x|)): it falls with the radius everywhere in the cube and passes mean_density = exp(1.5 * (2 - radius))
    (8.17 at the default, below the default density_thresh) at |x| = radius up to level 0's interpolation error (< 0.01).  density_grid [1, S^3] (Morton order)
    holds, per cell, the density a full cell diagonal nearer to the centre than the cell's own centre: an upper bound over the cell and its neighbours, as a trained
    grid's running maximum is, so masking by it removes nothing the iso level would keep.
    cascades = 2 or 3 (bound 2 or 4) adds `aabb_train` (+-bound) and rows 1 ... of density_grid: row k is cascade k's view of one scene in its normalised coordinates
    (world / 2^k), sampled at the cell centres — the ball (inside the 0.45 box of every outer cascade, so no outer mesh may show it), per cascade j <= k a ground slab
    (-0.85 < z / 2^j < -0.6, |x|, |y| < 0.85 * 2^j) and a dome (0.7 < |p| / 2^j < 0.9, z > 0.25 * 2^j) at exp(c * A), which lie between 0.55 and 0.9 of cascade j's
    cube and inside the 0.45 box of the cascades after it, and a corner column of untrained cells (-1).  The network still describes the ball in [-1, 1]^3 only."""
    S = int(S); c, A = 1.5, 2.0
    cascades = int(cascades)
    if cascades < 1 or cascades > 3:
        raise ValueError("synthetic_checkpoint: %d cascades (1, 2 or 3)" % cascades)
    net, total = density_layout(1.0)
    table = torch.zeros((total, 2), dtype=torch.float32)
    s1 = int(net.resolution[0]) + 1
    i = np.arange(s1, dtype=np.float64)
    ax = ((i - 0.5) / float(net.scale[0])) * 2.0 - 1.0
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    idx = (np.arange(s1)[:, None, None] + np.arange(s1)[None, :, None] * s1 + np.arange(s1)[None, None, :] * s1 * s1).reshape(-1)
    table[torch.from_numpy(idx), 0] = torch.from_numpy((A - np.sqrt(x * x + y * y + z * z)).reshape(-1).astype(np.float32))
    w0 = torch.zeros((64, 32), dtype=torch.float32); w0[0, 0] = c
    w1 = torch.zeros((16, 64), dtype=torch.float32); w1[0, 0] = 1.0
    cc = (np.arange(S, dtype=np.float64) + 0.5) / S * 2.0 - 1.0
    gx, gy, gz = np.meshgrid(cc, cc, cc, indexing="ij")
    r = np.maximum(np.sqrt(gx * gx + gy * gy + gz * gz) - np.sqrt(3.0) * 2.0 / S, 0.0)
    grid = np.zeros(S ** 3, np.float32)
    grid[morton_indices(S).reshape(-1)] = np.exp(c * (A - r)).reshape(-1).astype(np.float32)
    offsets = torch.tensor([int(net.offsets[k]) for k in range(net.num_levels + 1)], dtype=torch.int32)
    ck = {"mean_density": float(np.exp(c * (A - float(radius)))),
          "model": {"encoder.embeddings": table, "encoder.offsets": offsets, "sigma_net.0.weight": w0, "sigma_net.1.weight": w1,
                    "density_grid": torch.from_numpy(grid)[None]}}
    if cascades > 1:
        rows = [grid]
        for k in range(1, cascades):
            row = np.zeros(S ** 3, np.float32)
            row[morton_indices(S).reshape(-1)] = _synthetic_outer_row(S, k, c, A).reshape(-1)
            rows.append(row)
        b = float(2 ** (cascades - 1))
        ck["model"]["density_grid"] = torch.from_numpy(np.stack(rows, 0))
        ck["model"]["aabb_train"] = torch.tensor([-b, -b, -b, b, b, b], dtype=torch.float32)
    return ck


# synthetic_radiance_checkpoint's constants: the fp32 values of the reference's SH literals for l = 0 and l = 1, and the gains of the three channels
SYN_SH0, SYN_SH1 = float(np.float32(0.28209479177387814)), float(np.float32(0.48860251190291987))
SYN_KR, SYN_KG, SYN_KB, SYN_BIAS = 4.0, 4.0, 2.0, 4.0


def synthetic_radiance_color(d, feat0):
    """synthetic_radiance_checkpoint's closed form in float64 numpy: d [n, 3] directions of any non-zero length, feat0 [n] the encoder's feature 0 (level 0,
    channel 0: trilinear(2 - |x|)) at the positions -> rgb [n, 3]."""
    d = np.asarray(d, np.float64); f = np.asarray(feat0, np.float64)
    u = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    sig = lambda h: 1.0 / (1.0 + np.exp(-h))
    return np.stack([sig(SYN_KR * SYN_SH1 * u[:, 0]), sig(SYN_KG * SYN_SH1 * u[:, 2]), sig(SYN_KB * (1.5 * f - SYN_BIAS * SYN_SH0))], axis=1)


def synthetic_radiance_checkpoint(S=16, radius=0.6):
    """synthetic_checkpoint(S, radius) with a colour net whose output is a closed form, for tests and smoke runs.  Everything the density reads is
    synthetic_checkpoint's (table, sigma_net.0.weight, row 0 of sigma_net.1.weight, density_grid, mean_density): sigma is unchanged.  With u = d / |d| the unit view
    direction, F(x) = the encoder's feature 0 (trilinear(2 - |x|) on level 0), SH0 = fp32(0.28209479177387814) and SH1 = fp32(0.48860251190291987):
        r = sigmoid(4 * SH1 * u_x)                      direction alone: - 4 * sh[3], sh[3] = - SH1 * u_x
        g = sigmoid(4 * SH1 * u_z)                      direction alone: + 4 * sh[2], sh[2] = + SH1 * u_z
        b = sigmoid(2 * (1.5 * F(x) - 4 * SH0))         position alone, through geo_feat[14] = 1.5 * F(x) and the constant sh[0] = SH0 in the place of a bias
    (synthetic_radiance_color).  How: row 15 of sigma_net.1.weight is [1, 0, ...], so geo_feat[14] = relu(1.5 F) = 1.5 F (F > 0 in the cube) — input 16 + 14 = 30 of
    the colour net, which pins the [sh, geo_feat] order and the 1 + 14 offset; a value t passes both hidden ReLU layers as the pair relu(t), relu(-t) (neurons 0 / 1:
    t = sh[3]; 2 / 3: t = sh[2]; 4 / 5: t = geo_feat[14] - 4 sh[0]; color_net.1.weight is the identity on them) and color_net.2.weight recombines
    k * (relu(t) - relu(-t)) = k * t.  Every weight is a small integer: in fp32 the pre-activations of r and g are exact products of the encoder's sh."""
    ck = synthetic_checkpoint(S, radius)
    m = ck["model"]
    w1 = m["sigma_net.1.weight"].clone(); w1[15, 0] = 1.0
    c0 = torch.zeros((COLOR_HIDDEN, SH_DIM + GEO_FEAT_DIM), dtype=torch.float32)
    c0[0, 3], c0[1, 3] = 1.0, -1.0
    c0[2, 2], c0[3, 2] = 1.0, -1.0
    c0[4, 0], c0[4, SH_DIM + 14] = -SYN_BIAS, 1.0
    c0[5, 0], c0[5, SH_DIM + 14] = SYN_BIAS, -1.0
    c1 = torch.zeros((COLOR_HIDDEN, COLOR_HIDDEN), dtype=torch.float32)
    for k in range(6):
        c1[k, k] = 1.0
    c2 = torch.zeros((3, COLOR_HIDDEN), dtype=torch.float32)
    c2[0, 0], c2[0, 1] = -SYN_KR, SYN_KR
    c2[1, 2], c2[1, 3] = SYN_KG, -SYN_KG
    c2[2, 4], c2[2, 5] = SYN_KB, -SYN_KB
    m["sigma_net.1.weight"] = w1
    m["color_net.0.weight"], m["color_net.1.weight"], m["color_net.2.weight"] = c0, c1, c2
    return ck


def _outer_plan(save_path, ckpt, bound, env_reso, sdf, overwrite):
    """What export_outer_meshes checks before it touches the device -> (density_grid, aabb as 6 floats, the paths of mesh_1.ply ...)."""
    from . import checkpoint as CK
    if ckpt is None:
        raise ValueError("the outer meshes come from a checkpoint's density_grid: no ckpt given")
    if sdf:
        raise NotImplementedError("the --sdf outer mesh (contracted background, nerf/renderer.py:575-629) is not built")
    if not (float(bound) > 0 and np.isfinite(float(bound))):
        raise ValueError("bound %r" % (bound,))
    if int(env_reso) < 2 or int(env_reso) > 1024:
        raise ValueError("env_reso %d is not in [2, 1024]" % int(env_reso))
    model = ckpt["model"] if "model" in ckpt else ckpt
    if "mean_density" not in ckpt:
        raise KeyError("checkpoint has no top-level mean_density")
    grid = torch.as_tensor(model["density_grid"])
    rows = int(grid.shape[0]) if grid.dim() == 2 else 1
    want = CK.cascade_of_bound(float(bound))
    if rows != want:
        raise ValueError("the checkpoint's density_grid has %d cascades, --bound %g has %d: pass the --bound the checkpoint was trained with" % (rows, float(bound), want))
    if "aabb_train" in model:
        aabb = _box6(torch.as_tensor(model["aabb_train"]).detach().cpu().numpy())
    else:
        aabb = [-float(bound)] * 3 + [float(bound)] * 3
    paths = [os.path.join(save_path, "mesh_%d.ply" % cas) for cas in range(1, rows)]
    for f in paths:
        if os.path.exists(f) and not overwrite:
            raise FileExistsError("%s exists (pass overwrite to replace it)" % f)
    return grid, aabb, paths


def export_outer_meshes(save_path, ckpt, bound, env_reso=256, density_thresh=10.0, cameras=None, dilation=5, min_f=8, min_d=5, decimate_target=3e5, overwrite=False,
                        log=print, sdf=False):
    """The non-SDF outer meshes of NeRFRenderer.export_stage0 (nerf/renderer.py:632-698) -> the list of written paths, `mesh_{cas}.ply` for cas = 1 ... .
    ckpt: a stage-0 checkpoint whose density_grid has exactly checkpoint.cascade_of_bound(bound) rows; model["aabb_train"] when present, else +-bound, bounds the
    meshes.  Per cascade: outer_shell at env_reso with thresh = min(mean_density, density_thresh), clean_mesh(min_f, min_d), decimate_mesh to HALF of decimate_target
    (:635) with every edge collapsed onto one of its end points (optimalplacement=False as MeshLab reads it, :685: the vertices stay a subset of the shell's), and only
    then the visibility cull (cameras = (mvps, H, W), :692-694).
    A cascade whose mesh is empty after the centre is removed (:664), after cleaning (:681) or after the cull is skipped with one log line: no file is written.
    The cull casts rays through the BVH, whose box test passes no ray through a box of zero thickness: faces that lie exactly in an axis-aligned plane, of which the
    mesh of a 0 / 1 volume has many, count as unseen and stay only within `dilation` rings of a seen face.
    sdf = True is refused (the contracted outer mesh, :575-629, is not built)."""
    from . import checkpoint as CK
    grid, aabb, paths = _outer_plan(save_path, ckpt, bound, env_reso, sdf, overwrite)
    thresh = select_iso(ckpt["mean_density"], density_thresh)
    target = decimate_target // 2                                                 # :635, once: the inner mesh has been written with the full target
    written = []
    for cas, out in zip(range(1, len(paths) + 1), paths):
        v, t = outer_shell(unpack_density_grid(grid, cas), cas, bound, env_reso, thresh, aabb, log=log)
        if v.shape[0]:
            v, t = clean_mesh(v, t, min_f=min_f, min_d=min_d, log=log)
        if v.shape[0] == 0 or t.shape[0] == 0:
            log("[INFO] cascade %d: nothing outside the centre box is left, %s is not written" % (cas, os.path.basename(out)))
            continue
        if target > 0 and t.shape[0] > target:
            v, t = decimate_mesh(v, t, int(target), optimalplacement=False, endpoints_only=True, log=log)
        log("[INFO] exporting outer mesh at cas %d, v = %s, f = %s" % (cas, tuple(v.shape), tuple(t.shape)))
        if cameras is not None:
            mvps, H, W = cameras
            unseen = mark_unseen_triangles(v, t, mvps, H, W, log=log)
            v, t = remove_masked_trigs(v, t, unseen, dilation=dilation, log=log)
            if t.shape[0] == 0:
                log("[INFO] cascade %d: no camera sees the mesh, %s is not written" % (cas, os.path.basename(out)))
                continue
        os.makedirs(save_path, exist_ok=True)
        CK.write_ply(out, v.cpu().numpy(), t.cpu().numpy())
        log("[INFO] wrote %s: %d vertices, %d triangles" % (out, v.shape[0], t.shape[0]))
        written.append(out)
    return written


def export_stage0(save_path, ckpt=None, volume=None, iso=None, sdf=False, density_thresh=10.0, mesh=None, cameras=None, dilation=5, min_f=8, min_d=5,
                  decimate_target=3e5, optimalplacement=True, overwrite=False, log=print, resolution=None, bound=1.0, outer=False, env_reso=256):
    """NeRFRenderer.export_stage0 (nerf/renderer.py:498-570) -> path of the written mesh_0.ply.
    Exactly one geometry source, or a volume together with the checkpoint that masks it:
      ckpt    a stage-0 checkpoint dict (top-level `mean_density`, `model` -> `density_grid` [cascade, S^3]): cascade 0 at the grid's own resolution (:511-515),
              iso = min(mean_density, density_thresh) (:506); with `resolution` (the reference's --mcubes_reso) given and different from the grid's S, the
              checkpoint's density network (DensityField.from_checkpoint(ckpt, bound)) is evaluated on the resolution^3 lattice and masked by the grid (:516-541);
      volume  a dense [R, R, R] sigma volume (iso as for ckpt when one is given, else `iso` or density_thresh; with ckpt and not sdf it is masked by the grid,
              :532-539) or, with sdf, a signed distance extracted as (-volume, 0) (:549);
      mesh    (vertices, triangles) of a foreign mesh in world space: cull, clean and decimate only.
    Above decimate_target (> 0) triangles the cleaned mesh is decimated to it (:566-567, decimate_mesh).
    cameras = (mvps [B, 4, 4], H, W) switches the visibility cull on (:557-560).
    outer (needs ckpt, excludes sdf): after mesh_0.ply the outer cascades' meshes mesh_1.ply ... of a checkpoint trained with `bound` > 1 are written from its density
    grid at env_reso (export_outer_meshes, :632-698); a checkpoint of one cascade has none.  Its arguments are checked before anything is written."""
    from . import checkpoint as CK
    if outer:
        if ckpt is None:
            raise ValueError("export_stage0: outer needs a checkpoint (the outer meshes come from its density_grid)")
        _outer_plan(save_path, ckpt, bound, env_reso, sdf, overwrite)
    if mesh is not None and (ckpt is not None or volume is not None):
        raise ValueError("export_stage0: a mesh excludes a checkpoint and a volume")
    if mesh is None and ckpt is None and volume is None:
        raise ValueError("export_stage0: nothing to extract from (ckpt, volume or mesh)")
    if sdf and volume is None:
        raise ValueError("export_stage0: sdf needs a volume")
    if resolution is not None and (ckpt is None or volume is not None):
        raise ValueError("export_stage0: resolution queries a checkpoint's density network: it needs ckpt and excludes a volume and a mesh")
    out = os.path.join(save_path, "mesh_0.ply")
    if os.path.exists(out) and not overwrite:
        raise FileExistsError("%s exists (pass overwrite to replace it)" % out)
    if mesh is not None:
        v, t = _verts(mesh[0]), _tris(mesh[1])
    else:
        grid_vol = None
        if ckpt is not None:
            model = ckpt["model"] if "model" in ckpt else ckpt
            grid = torch.as_tensor(model["density_grid"])
            if grid.dim() == 2 and grid.shape[0] > 1:
                log("[INFO] checkpoint has %d cascades: %s" % (grid.shape[0], "cascade 0 first, the outer meshes follow" if outer else
                                                                 "exporting cascade 0 only, outer=True (--outer_meshes) writes the outer meshes (bound > 1)"))
            grid_vol = unpack_density_grid(grid, 0)
            if not sdf:
                if "mean_density" not in ckpt:
                    raise KeyError("checkpoint has no top-level mean_density")
                thresh = select_iso(ckpt["mean_density"], density_thresh)
        if volume is not None:
            vol = torch.as_tensor(volume).to(_dev(), torch.float32).contiguous()
            if sdf:
                vol, thresh = -vol, 0.0
            elif ckpt is not None:
                vol = mask_by_density_grid(vol, grid_vol, thresh)
            else:
                thresh = float(iso) if iso is not None else float(density_thresh)
        elif resolution is not None and int(resolution) != int(grid_vol.shape[0]):
            vol = DensityField.from_checkpoint(ckpt, bound).volume(int(resolution), grid_vol, thresh)
        else:
            vol = grid_vol
        if iso is not None and not sdf:
            thresh = float(iso)
        v, t = marching_cubes(vol, thresh)
        log("[INFO] marching cubes at %s, iso %g: %d vertices, %d triangles" % ("x".join(str(s) for s in vol.shape), thresh, v.shape[0], t.shape[0]))
        v = index_to_world(v, [int(s) for s in vol.shape])
    if cameras is not None and t.shape[0]:
        mvps, H, W = cameras
        unseen = mark_unseen_triangles(v, t, mvps, H, W, log=log)
        v, t = remove_masked_trigs(v, t, unseen, dilation=dilation, log=log)
    v, t = clean_mesh(v, t, min_f=min_f, min_d=min_d, log=log)
    if decimate_target > 0 and t.shape[0] > decimate_target:
        v, t = decimate_mesh(v, t, int(decimate_target), optimalplacement=optimalplacement, log=log)
    if t.shape[0] == 0:
        raise RuntimeError("export_stage0: the mesh is empty after cleaning")
    os.makedirs(save_path, exist_ok=True)
    CK.write_ply(out, v.cpu().numpy(), t.cpu().numpy())
    log("[INFO] wrote %s: %d vertices, %d triangles" % (out, v.shape[0], t.shape[0]))
    if outer:
        export_outer_meshes(save_path, ckpt, bound, env_reso=env_reso, density_thresh=density_thresh, cameras=cameras, dilation=dilation, min_f=min_f, min_d=min_d,
                            decimate_target=decimate_target, overwrite=overwrite, log=log)
    return out
