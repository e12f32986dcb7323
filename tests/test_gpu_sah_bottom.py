"""The sweep-SAH bottom of the private hierarchy (private level 3, bvh_build.hip k_sb_*): every maximal subtree of at most MR_SAH_BOTTOM = 256 leaves is rebuilt
top-down by exact sweep SAH. Levels 2 and 3 are built in ONE process through mirres_bvh_build_level and compared:

  structure (the binary hierarchy itself, mirres_debug_private_tree, and the 4-wide layout collapsed from it, test_gpu_layout.check_layout)
    - every internal node and every leaf slot is reachable from node 0 exactly once,
    - every node box is the exact fmin / fmax union of the leaf boxes below it, leaf entries carry the reference's own boxes,
    - unused 4-wide entries point at the null leaf,
    - the level-3 tree is never taller than the level-2 tree it was made from (the bound stated in bvh_build.hip: a rebuilt subtree is not taller than the
      one it replaces), hence within 40 + 14 + ceil(log2 T) binary levels, and the 4-wide layout has no more levels than the binary tree,
  answers
    - any-hit bits (mode 0) and closest-hit records (mode 2: hit, prim, t, pos, normal) of 4 096 seeded rays that start ON the triangles, half of them aimed at
      other triangles' centroids, are bit-equal between the two levels; no private-stack overflow is counted,
  the two routes to level 3
    - a level-1 build on a second handle followed by mirres_bvh_upgrade reports level 3 and gives the direct level-3 build's private tree and 4-wide layout, word
      for word once the node ids are taken out (canon_binary, canon_layout: the SAH top's ids come from device atomics; which child is left and which right does
      not); on "soup 1366" and "lego small" the SAH top must have rebuilt something on both routes (clusters >= 2, no failure).

Meshes: soups around the subtree limit (T = 8, 255, 256, 257, 513, 1366), 300 copies of one triangle (all centroids equal: the object-median rule), 300 triangles
with collinear centroids, the 68-triangle adversarial chain of test_gpu_layout.py, the small lego-like mesh.
CPU: the replay tool's (scripts/treelab) bottom rebuild on a 1 366-triangle soup — same reachability, same hit bits as the tool's first tree."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_RAYS = 4096


def _soup(T, seed=5):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (3 * T, 3)).astype(np.float32)
    v[1::3] = v[0::3] + rng.normal(0, 0.05, (T, 3)).astype(np.float32); v[2::3] = v[0::3] + rng.normal(0, 0.05, (T, 3)).astype(np.float32)
    return v, np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def _copies(T=300):
    one = np.array([[0.1, 0.2, 0.3], [0.6, 0.25, 0.3], [0.2, 0.7, 0.45]], np.float32)
    return np.tile(one, (T, 1)), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def _collinear(T=300):
    """Box centres on the line x = y = z = k / 256 (exact in fp32): triangle k spans [c - h, c + h]^3 with a power-of-two half size that varies with k."""
    v = np.zeros((T, 3, 3), np.float32)
    for k in range(T):
        c = np.float32(k) / np.float32(256.0); h = np.float32(2.0 ** -(3 + k % 4))
        v[k, 0] = (c - h, c - h, c - h); v[k, 1] = (c + h, c + h, c - h); v[k, 2] = (c - h, c + h, c + h)
    return v.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


CASES = ["soup 8", "soup 255", "soup 256", "soup 257", "soup 513", "soup 1366", "copies 300", "collinear 300", "chain 68", "lego small"]


def _mesh(name, scene_mod):
    kind, n = name.split()
    if kind == "soup":
        return _soup(int(n))
    if kind == "copies":
        return _copies(int(n))
    if kind == "collinear":
        return _collinear(int(n))
    if kind == "chain":
        from test_oracle_invariants import adversarial_chain_mesh
        return adversarial_chain_mesh(dups=40)[:2]
    v, t = scene_mod.make_mesh_clustered(target_tris=20000, seed=3)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)


def _rays(v, t, seed=11):
    rng = np.random.default_rng(seed)
    T = len(t)
    a, b, c = v[t[:, 0]].astype(np.float64), v[t[:, 1]].astype(np.float64), v[t[:, 2]].astype(np.float64)
    i = rng.integers(0, T, N_RAYS); j = rng.integers(0, T, N_RAYS)
    u = rng.uniform(0, 1, (N_RAYS, 2)); flip = u.sum(1) > 1; u[flip] = 1 - u[flip]
    o = a[i] + u[:, :1] * (b[i] - a[i]) + u[:, 1:] * (c[i] - a[i])
    d = rng.normal(0, 1, (N_RAYS, 3))
    aimed = np.arange(N_RAYS) % 2 == 0
    d[aimed] = ((a[j] + b[j] + c[j]) / 3.0 - o)[aimed]
    dead = np.abs(d).max(1) < 1e-6
    d[dead] = (1.0, 0.5, 0.25)
    r = np.zeros((N_RAYS, 8), np.float32); r[:, 0:3] = o; r[:, 4:7] = d; r[:, 7] = 1e7
    return r


def check_binary(info, aabb, T, ref_aabb):
    """The private binary hierarchy: reachability, exact unions. Returns its height (levels of internal nodes)."""
    LEAF = T - 1
    seen = np.zeros(2 * T - 1, np.int64); seen[0] = 1
    levels = [np.array([0], np.int64)]
    while True:
        kids = info[levels[-1], :2].astype(np.int64).ravel()
        assert np.all((kids > 0) & (kids < 2 * T - 1))
        np.add.at(seen, kids, 1)
        nxt = kids[kids < LEAF]
        if nxt.size == 0:
            break
        levels.append(nxt)
        assert len(levels) < 400
    assert np.all(seen == 1), "every node is reachable exactly once (missing %d, doubled %d)" % (int((seen == 0).sum()), int((seen > 1).sum()))
    slots = info[LEAF:, 2]
    assert np.array_equal(np.sort(slots), np.arange(T)), "leaf entries carry a permutation of the reference slots"
    assert np.array_equal(aabb[LEAF:], ref_aabb[LEAF + slots]), "leaf entries carry the reference's own leaf boxes"
    box = aabb.copy()
    for cur in reversed(levels):
        l, r = info[cur, 0], info[cur, 1]
        lo = np.minimum(box[l, 0:3], box[r, 0:3]); hi = np.maximum(box[l, 3:6], box[r, 3:6])
        assert np.array_equal(aabb[cur, 0:3], lo) and np.array_equal(aabb[cur, 3:6], hi), "a node box is not the union of the boxes below it"
    return len(levels)


INTERNAL = 0xffffffff      # canonical forms: "an internal node follows" (no leaf slot is this large)


def canon_binary(info, aabb, T):
    """The private binary hierarchy without its node ids (the SAH top hands them out through device atomics; left and right it decides itself): depth-first from
    node 0, left child first; an internal node gives INTERNAL and its six box words, a leaf its slot."""
    LEAF = T - 1
    left, right = info[:, 0].tolist(), info[:, 1].tolist()
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        if n < LEAF:
            stack.append(right[n]); stack.append(left[n])
        assert len(order) <= 2 * T - 1
    order = np.array(order, np.int64)
    words = np.zeros((len(order), 7), np.uint32)
    inner = order < LEAF
    words[inner, 0] = INTERNAL; words[inner, 1:] = np.ascontiguousarray(aabb, np.float32).view(np.uint32)[order[inner]]
    words[~inner, 0] = info[order[~inner], 2].astype(np.uint32)
    return words


def canon_layout(nodes, T):
    """The 4-wide layout without its node ids: depth-first from node 0 in `ref` order; a node gives org, the three steps, qlo, qhi, and per entry the leaf slot
    (T: the null leaf) or INTERNAL."""
    ref = nodes["ref"].astype(np.int64)
    steps = np.stack([nodes["step_x"], nodes["step_y"], nodes["step_z"]], 1)
    words = np.concatenate([nodes["org"].view(np.uint32), steps.view(np.uint32), nodes["qlo"], nodes["qhi"], np.where(ref >= 0, INTERNAL, ~ref).astype(np.uint32)], 1)
    kids = ref.tolist()
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        stack.extend(r for r in reversed(kids[n]) if r >= 0)
        assert len(order) <= T
    return words[order]


# cases left out of the "level 1 + upgrade == level 3" equality, with the reason (at most two; never "soup 1366" or "lego small")
UPGRADE_NOT_COMPARED = {}


class _Handle:
    def __init__(self, h, t):
        self.h, self.v_ind = h, t


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_level_3_is_a_valid_hierarchy_with_level_2s_answers(name, scene_mod):
    import torch
    from mirres_restir_nerf_mesh_amd._lib import lib, check
    from test_gpu_layout import check_layout, fetch_layout
    L = lib()
    L.mirres_debug_private_tree.argtypes = [C.c_void_p] * 3; L.mirres_debug_private_tree.restype = C.c_int
    L.mirres_debug_sah_bottom.argtypes = [C.c_void_p, C.c_void_p]; L.mirres_debug_sah_bottom.restype = C.c_int
    v, t = _mesh(name, scene_mod)
    T, V = len(t), len(v)
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    rays = torch.from_numpy(_rays(v, t)).cuda()
    L.mirres_debug_sah_state.argtypes = [C.c_void_p, C.c_void_p]; L.mirres_debug_sah_state.restype = C.c_int
    h, h2 = C.c_void_p(), C.c_void_p()
    check(L.mirres_bvh_create(C.byref(h), T), "mirres_bvh_create")
    try:
        got = {}
        for level in (2, 3):
            info = torch.empty((2 * T - 1, 3), dtype=torch.int32, device="cuda"); aabb = torch.empty((2 * T - 1, 6), device="cuda")
            check(L.mirres_bvh_build_level(h, dv.data_ptr(), V, dt.data_ptr(), T, info.data_ptr(), aabb.data_ptr(), None, level, None), "mirres_bvh_build_level")
            torch.cuda.synchronize()
            assert L.mirres_bvh_tree_level(h) == level and L.mirres_bvh_private_level(h) == 2
            r_info, r_aabb = info.cpu().numpy(), aabb.cpu().numpy()
            p_info = np.zeros((2 * T - 1, 3), np.int32); p_aabb = np.zeros((2 * T - 1, 6), np.float32)
            check(L.mirres_debug_private_tree(h, p_info.ctypes.data, p_aabb.ctypes.data), "mirres_debug_private_tree")
            height = check_binary(p_info, p_aabb, T, r_aabb)
            nodes, leaves, top = fetch_layout(_Handle(h, dt))
            st = check_layout(nodes, leaves, top, T, v, t, r_info, r_aabb)
            assert st["levels"] <= height
            n = N_RAYS
            out = {"height": height, "p_info": p_info, "tree": canon_binary(p_info, p_aabb, T), "layout": canon_layout(nodes, T)}
            hit = torch.zeros(n, dtype=torch.int32, device="cuda")
            check(L.mirres_bvh_trace(h, rays.data_ptr(), n, 0, hit.data_ptr(), None, None, None, None, None, None), "any-hit")
            torch.cuda.synchronize(); out["any"] = hit.cpu().numpy().copy()
            cnt = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
            check(L.mirres_bvh_trace(h, rays.data_ptr(), n, 0, hit.data_ptr(), None, None, None, None, cnt.data_ptr(), None), "any-hit, counted")
            torch.cuda.synchronize()
            assert np.array_equal(hit.cpu().numpy(), out["any"]) and int(cnt[:, 3].sum()) == 0, "no private-stack overflow"
            tt = torch.zeros(n, device="cuda"); pos = torch.zeros((n, 3), device="cuda"); nrm = torch.zeros((n, 3), device="cuda"); pr = torch.zeros(n, dtype=torch.int32, device="cuda")
            check(L.mirres_bvh_trace(h, rays.data_ptr(), n, 2, hit.data_ptr(), tt.data_ptr(), pos.data_ptr(), nrm.data_ptr(), pr.data_ptr(), None, None), "closest")
            torch.cuda.synchronize()
            out["closest"] = [x.cpu().numpy().copy().view(np.uint32) for x in (hit, pr, tt, pos, nrm)]
            if level == 3:
                sb = (C.c_uint32 * 4)()
                check(L.mirres_debug_sah_bottom(h, sb), "mirres_debug_sah_bottom")
                assert sb[0] >= 1 and sb[1] == 0 and sb[2] == 256, list(sb)
            got[level] = out
        assert got[3]["height"] <= got[2]["height"] <= 40 + 14 + int(np.ceil(np.log2(T)))
        if name in ("soup 255", "soup 256", "soup 257", "soup 513", "soup 1366", "lego small"):
            assert not np.array_equal(got[2]["p_info"], got[3]["p_info"]), "level 3 changed the hierarchy"
        assert np.array_equal(got[2]["any"], got[3]["any"])
        assert 0.1 < got[3]["any"].mean(), "a good share of the rays is occluded"
        for a, b in zip(got[2]["closest"], got[3]["closest"]):
            assert np.array_equal(a, b)
        assert got[3]["closest"][0].view(np.int32).mean() > 0.1
        # ---- the other route to level 3: a level-1 build on a handle of its own, then mirres_bvh_upgrade — the same tree and the same layout, node ids aside
        check(L.mirres_bvh_create(C.byref(h2), T), "mirres_bvh_create")
        info2 = torch.empty((2 * T - 1, 3), dtype=torch.int32, device="cuda"); aabb2 = torch.empty((2 * T - 1, 6), device="cuda")
        check(L.mirres_bvh_build_level(h2, dv.data_ptr(), V, dt.data_ptr(), T, info2.data_ptr(), aabb2.data_ptr(), None, 1, None), "mirres_bvh_build_level")
        assert L.mirres_bvh_tree_level(h2) == 1
        check(L.mirres_bvh_upgrade(h2, dv.data_ptr(), dt.data_ptr(), info2.data_ptr(), aabb2.data_ptr(), None), "mirres_bvh_upgrade")
        torch.cuda.synchronize()
        assert L.mirres_bvh_tree_level(h2) == 3
        u_info = np.zeros((2 * T - 1, 3), np.int32); u_aabb = np.zeros((2 * T - 1, 6), np.float32)
        check(L.mirres_debug_private_tree(h2, u_info.ctypes.data, u_aabb.ctypes.data), "mirres_debug_private_tree")
        u_nodes = fetch_layout(_Handle(h2, dt))[0]
        if name in ("soup 1366", "lego small"):                  # the top really rebuilt something on both routes: the equality is not about trees it never touched
            for hh in (h, h2):
                st = (C.c_uint32 * 8)()
                check(L.mirres_debug_sah_state(hh, st), "mirres_debug_sah_state")
                print("%s: SAH top clusters %d, fail %d" % (name, st[0], st[5]))
                assert st[0] >= 2 and st[5] == 0, list(st)
        if name not in UPGRADE_NOT_COMPARED:
            assert np.array_equal(canon_binary(u_info, u_aabb, T), got[3]["tree"]), "level 1 + upgrade: another private tree than the direct level-3 build"
            assert np.array_equal(canon_layout(u_nodes, T), got[3]["layout"]), "level 1 + upgrade: another 4-wide layout than the direct level-3 build"
    finally:
        torch.cuda.synchronize()
        L.mirres_bvh_destroy(h)
        if h2:
            L.mirres_bvh_destroy(h2)


def test_replay_tool_bottom_rebuild_keeps_every_leaf_and_every_hit_bit(tmp_path):
    """scripts/treelab on a 1 366-triangle soup: the tool checks every tree it builds (each leaf below the root exactly once) and compares the hit bits of every
    hierarchy with those of its first tree; here its rows for the bottom rebuild must be present, checked, and free of differences."""
    v, t = _soup(1366)
    exe = str(tmp_path / "treelab")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "treelab", "treelab.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    with open(tmp_path / "mesh.bin", "wb") as f:
        f.write(np.array([len(v), len(t)], np.int32).tobytes()); f.write(v.tobytes()); f.write(t.tobytes())
    r = _rays(v, t)
    with open(tmp_path / "rays.bin", "wb") as f:
        f.write(np.array([len(r)], np.int32).tobytes()); f.write(r.tobytes())
    p = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "rays.bin")], env=dict(os.environ, TL_ONLY="EMC"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l for l in p.stdout.splitlines() if "SAH bottom" in l and "greedy" in l]
    assert len(rows) >= 3, p.stdout
    assert "!!" not in p.stdout, p.stdout
    assert p.stdout.count("tree ok") >= len(rows) // 3
    hit = [float(l.split()[-1]) for l in rows]
    assert all(0.1 < x for x in hit)
