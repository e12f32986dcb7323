"""GPU: the shadow-ray kernel's per-wave pool of prepared rays (bvh_trace.hip, pool_fill / pool_get). The pool changes which lane walks which ray and where a ray
is set up, never a ray's answer: the production any-hit (mirres_bvh_trace mode 0) is compared hit for hit with the reference-order kernel (mode 1) on ray
counts around every edge of the chunk / sub-queue / pool arithmetic and on ray sets that leave the pool empty, nearly empty, or drained every iteration;
the pixel-pair source is checked through whole small frames against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]


@pytest.fixture(scope="module")
def world(oracle, scene_mod):
    """Icosphere of subdivision 3 over a 16 x 16 ground grid (1792 triangles) and a tracer for it: trace(rays, mode) -> hit[]."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mirres_restir_nerf_mesh_amd.renderer_restir import restirbvhWorker
    from mirres_restir_nerf_mesh_amd._lib import lib, check
    v, t = scene_mod.make_mesh(3, 16)
    w = restirbvhWorker(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()); w.update_mesh(w.vrt, w.v_ind)

    def trace(rays, mode):
        k = len(rays)
        dr = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).cuda()
        hit = torch.full((k,), -7, dtype=torch.int32, device="cuda")         # every slot must be written, also for rays that never enter the pool
        if mode == 0:
            check(lib().mirres_bvh_trace(w.h, dr.data_ptr(), k, 0, hit.data_ptr(), None, None, None, None, None, None), "any-hit")
        else:
            tt = torch.zeros(k, device="cuda"); pos = torch.zeros((k, 3), device="cuda"); nrm = torch.zeros((k, 3), device="cuda")
            pr = torch.zeros(k, dtype=torch.int32, device="cuda")
            check(lib().mirres_bvh_trace(w.h, dr.data_ptr(), k, 1, hit.data_ptr(), tt.data_ptr(), pos.data_ptr(), nrm.data_ptr(), pr.data_ptr(), None, None), "reference order")
        torch.cuda.synchronize()
        return hit.cpu().numpy()
    return trace


def _scene_rays(oracle, n, seed, tmin=0.0, tmax=1e7):
    """Origins inside the scene's box, directions all round: a mixture of occluded and free rays, every one of them inside the root box."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * 1.6 - 0.8).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[::17, 0] = 0.0                                                          # the zero-component fix-up of the reciprocals
    return oracle.make_rays(o, d, tmin, tmax)


def _miss_rays(oracle, n):
    """Rays that start far outside the scene and point away from it: the root box test fails, nothing is pooled."""
    o = np.tile(np.array([[40.0, 35.0, 50.0]], np.float32), (n, 1)) + np.arange(n, dtype=np.float32)[:, None] * 1e-3
    d = np.tile(np.array([[0.3, 0.2, 1.0]], np.float32), (n, 1))
    return oracle.make_rays(o, d)


def _agree(world, rays, what):
    got, ref = world(rays, 0), world(rays, 1)
    assert set(np.unique(got)) <= {0, 1}, what
    assert np.array_equal(got, ref), "%s: %d of %d rays differ from the reference order" % (what, int((got != ref).sum()), len(ref))
    return got


# 1 .. 129: below, at and above one wave; 32 * 64 -+ 1: one 64-ray chunk per sub-queue (MR_NQ = 32), a ray short and a ray over; 4097: a second chunk
# in one sub-queue; 70001: chunks longer than 64, sub-queues that end in a partial chunk, more waves than one per sub-queue
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 32 * 64 - 1, 32 * 64, 32 * 64 + 1, 4097, 70001])
def test_ray_counts_around_every_edge(world, oracle, n):
    rays = _scene_rays(oracle, n, seed=n)
    got = _agree(world, rays, "%d rays" % n)
    if n >= 2047:
        assert 0.05 < got.mean() < 0.95, "the fixture must mix occluded and free rays"


def test_all_rays_miss_the_root_box(world, oracle):
    got = _agree(world, _miss_rays(oracle, 4096), "root misses")
    assert not got.any()


def test_one_live_ray_among_root_misses(world, oracle):
    rays = _miss_rays(oracle, 4096)
    rays[1234] = oracle.make_rays(np.array([[0.01, 0.02, 3.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32))[0]    # straight down onto the sphere
    got = _agree(world, rays, "one live ray")
    assert got[1234] == 1 and got.sum() == 1


def test_live_and_missing_rays_alternate(world, oracle):
    """every other lane's ray enters the pool: the compaction ranks are the lane number halved"""
    n = 4097
    rays = _scene_rays(oracle, n, seed=11)
    rays[1::2] = _miss_rays(oracle, n)[1::2]
    got = _agree(world, rays, "alternating")
    assert not got[1::2].any() and 0.05 < got[0::2].mean() < 0.95


def test_every_ray_is_occluded_at_once(world, oracle):
    """rays from a shell around the sphere towards its centre: each ends at one of its first leaves, so lanes free up in every iteration and the pool is
    drained as fast as it is filled"""
    n = 4097
    rng = np.random.default_rng(5)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True); u[:, 2] = np.abs(u[:, 2]) + 0.2
    o = (1.5 * u + np.array([0.0, 0.0, 0.0])).astype(np.float32)
    rays = oracle.make_rays(o, (-u + 0.02 * rng.normal(size=(n, 3))).astype(np.float32))
    got = _agree(world, rays, "all occluded")
    assert got.mean() > 0.9


@pytest.mark.parametrize("kind", ["short", "negative", "mixed"])
def test_rays_with_their_own_interval(world, oracle, kind):
    """plain ray queues carry t_min / t_max in the pool entry: a short t_max, a negative t_min, and several intervals within one wave"""
    n = 4097
    rays = _scene_rays(oracle, n, seed=23)
    rng = np.random.default_rng(29)
    if kind == "short":
        rays[:, 3] = 0.0; rays[:, 7] = (0.02 + 0.3 * rng.random(n)).astype(np.float32)
    elif kind == "negative":
        rays[:, 3] = (-0.6 * rng.random(n)).astype(np.float32); rays[:, 7] = 1e7
    else:
        table = np.array([[0.0, 1e7], [0.0, 0.15], [-0.5, 1e7], [-0.3, 0.1], [0.4, 0.6], [0.0, 0.0]], np.float32)
        pick = table[rng.integers(0, len(table), n)]
        rays[:, 3] = pick[:, 0]; rays[:, 7] = pick[:, 1]
    got = _agree(world, rays, kind + " intervals")
    assert 0.02 < got.mean() < 0.98


def test_three_launches_give_the_same_hits(world, oracle):
    """which lane walks which ray differs from launch to launch (the chunks go to whichever wave asks first); the answers may not"""
    rays = _scene_rays(oracle, 70001, seed=70001)
    ref = world(rays, 1)
    for k in range(3):
        assert np.array_equal(world(rays, 0), ref), "launch %d" % k


def _frame_pair(oracle, scene_mod, fx, fy, spp, black=False, seed=31):
    import torch
    from util import SmallFrame
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    F = SmallFrame(oracle, scene_mod, fx=fx, fy=fy, subdiv=3, ground=16, env_hw=(8, 16))
    W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    env = np.zeros_like(F.env) if black else F.env
    outs, _, _ = RR.render_fused(get_ctx(F.fx, F.fy), W, None, False, (1, 1, 1), cu(env), cu(F.occ[:, None].copy()), cu(F.normal), cu(F.depth[:, None]), cu(F.kd), cu(F.rm),
                                 cu(F.ray_dir_raw), cu(F.pos), spp, 2, 2, 2.0, 0.1, 0.001, seed)
    ref = oracle.render(F.fx, F.fy, spp, seed, (F.info, F.aabb), F.vert, F.tri, env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=None)
    return F, [o.cpu().numpy() for o in outs], ref


@pytest.mark.parametrize("fx,fy", [(33, 17), (48, 40)])
def test_pixel_pair_frames_match_the_oracle(oracle, scene_mod, fx, fy):
    """the spatial pass's queue of pixel pairs (rays formed in the kernel) at sizes whose pair counts are multiples neither of 64 nor of the chunk: 3 samples,
    every output of the frame equal to the oracle's bit for bit, as in test_gpu_render.py"""
    from util import pixel_parity
    F, got, ref = _frame_pair(oracle, scene_mod, fx, fy, 3)
    for g, n in zip(got, NAMES):
        assert np.isfinite(g).all()
        pixel_parity(g, ref[n], "%d x %d frame / %s" % (fx, fy, n), tol=0.0)


def test_black_environment_frame_pools_nothing(oracle, scene_mod):
    """an all-zero environment: every light sample carries zero luminance, every spatial ray is dead and the pool never fills"""
    from util import pixel_parity
    F, got, ref = _frame_pair(oracle, scene_mod, 33, 17, 3, black=True)
    fg = F.occ > 0.5
    assert fg.any() and (~fg).any()
    for g, n in zip(got, NAMES):
        assert np.isfinite(g).all() and (g[fg] == 0).all(), n
        pixel_parity(g, ref[n], "black environment / " + n, tol=0.0)
    assert (got[0][~fg] == 1).all()
