"""GPU parity of the temporal and spatial reservoir passes where history, neighbours and G-buffer disagree (tests/reservoir_refs.py; the fixtures are proved on
the CPU by tests/test_reservoir_fixtures.py), through the reference-shaped Python surface, against the oracle on identical inputs.  M is compared exactly, the
floats BIT FOR BIT, and nothing stored on either side may be NaN or inf.

If GPU and oracle ever differ in a NaN-carrying lane (an infinite history weight makes 0 * inf and inf - inf), the reference's shader source decides which side
is right.  On these inputs they do not differ: both sides feed the NaN only into `rnd * weightSum < w` (false on both) and into the final weight, which store_ris
empties on both."""
import numpy as np
import pytest

import reservoir_refs as R
from util import pixel_parity, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("light_data", "light_pdf", "M", "weight")


class _Gpu:
    """One Hostile bundle on the device: the worker (mesh + BVH), the module handles of its frame size and the G-buffer tensors."""

    def __init__(self, oracle, scene_mod, fx, fy):
        import torch
        from mirres_restir_nerf_mesh_amd import renderer_restir as RR
        self.torch, self.RR = torch, RR
        self.X = X = R.Hostile(oracle, scene_mod, fx, fy)
        F = X.F
        self.W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda())
        self.W.update_mesh(self.W.vrt, self.W.v_ind)
        self.mods = RR.load_m_for_restir(F.fx, F.fy)
        cu = self.cu
        self.T = dict(occ=cu(F.occ[:, None]), pos=cu(F.pos), nd=cu(F.normal_depth), brdf=cu(F.brdf), rd=cu(F.ray_dir), tex=cu(F.tex), noff=cu(F.noff),
                      p_occ=cu(X.p_occ[:, None]), p_nd=cu(X.p_nd), p_brdf=cu(X.p_brdf), p_rd=cu(X.p_rd), motion=cu(X.motion), snd=cu(X.snd))
        self._other = {}

    def cu(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def res(self, r):
        return tuple(self.cu(a.reshape(self.X.F.N, -1)) for a in r)

    def module(self, **constants):
        """A module handle over a context with other ReSTIR constants (runtime configuration, as test_reservoir_passes_with_other_constants builds one)."""
        from mirres_restir_nerf_mesh_amd import _lib, _ops
        key = tuple(sorted(constants.items()))
        if key not in self._other:
            cfg = _lib.default_config()
            for k, v in constants.items():
                setattr(cfg, k, v)
            self._other[key] = _ops.Module("restir (%s)" % (constants,), _ops.Context(self.X.F.fx, self.X.F.fy, cfg))
        return self._other[key]


@pytest.fixture(scope="module")
def gpus(oracle, scene_mod):
    import torch
    assert torch.cuda.is_available()
    made = {}

    def get(fx=48, fy=40):
        if (fx, fy) not in made:
            made[(fx, fy)] = _Gpu(oracle, scene_mod, fx, fy)
        return made[(fx, fy)]
    return get


def _compare(gpu, ref, what):
    g = [r.detach().cpu().numpy().reshape(r.shape[0], -1).squeeze() for r in gpu]
    for a, b, nm in zip(g, ref, NAMES):
        print("%s / %s: %d of %d values differ" % (what, nm, int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum()), a.size))
    for a, nm in zip(g, NAMES):
        assert np.isfinite(a).all(), "%s: the GPU stored NaN or inf in %s" % (what, nm)
    for b, nm in zip(ref, NAMES):
        assert np.isfinite(b).all(), "%s: the oracle stored NaN or inf in %s" % (what, nm)
    assert np.array_equal(g[2], ref[2]), what + ": M"
    for k in (0, 1, 3):
        same_bits(g[k], ref[k], "%s reservoirs / %s" % (what, NAMES[k]))


def _temporal(G, motion, max_history):
    from mirres_restir_nerf_mesh_amd import Resampling as RS
    X, T, F = G.X, G.T, G.X.F
    m = G.mods[3] if max_history == 20 else G.module(max_history=max_history)
    cur, prev = G.res(X.cur), G.res(X.prev)
    RS.TemporalResampling(m, cur, prev, T["tex"], F.Wc, F.Hc, F.fx, F.fy, X.TEMPORAL_INDEX, T["occ"], T["nd"], T["brdf"], T["rd"],
                          T["p_occ"], T["p_nd"], T["p_brdf"], T["p_rd"], T["motion"] if motion else None)
    for a, b, nm in zip(prev, X.prev, NAMES):      # the history is read only (inf weights included)
        assert np.array_equal(a.cpu().numpy().reshape(b.shape), b), "temporal pass wrote its history / " + nm
    return cur


@pytest.mark.parametrize("max_history", [20, 7])
@pytest.mark.parametrize("motion", [True, False])
def test_temporal_on_a_hostile_history(gpus, motion, max_history):
    """k_temporal on a history that disagrees with the frame: a third of the history G-buffer from another view, depths to both sides of the 10 % threshold,
    motion vectors of up to three pixels and some beyond the frame, history reservoirs with M = 0, M = 500 (the cap binds: 20 and, on a second context, 7),
    weight 0, weight inf, and non-empty reservoirs on the background.  Every exit of temporal_history_pixel / k_temporal / temporal_merge decides for at least
    15 pixels (test_reservoir_fixtures.py); without motion vectors the history pixel is the pixel itself under another view's normal, ray direction and BRDF."""
    G = gpus()
    _compare(_temporal(G, motion, max_history), G.X.oracle_temporal(motion, max_history), "temporal, hostile history, %s motion vectors, cap %d" % ("with" if motion else "no", max_history))


@pytest.mark.parametrize("shape", [(7, 5), (130, 18)])
def test_temporal_on_frames_smaller_and_wider_than_a_tile(gpus, shape):
    """The same on 7 x 5 (smaller than any tile or block) and 130 x 18 (crosses one 128-pixel chunk boundary, no multiple of 8 or 16)."""
    G = gpus(*shape)
    _compare(_temporal(G, True, 20), G.X.oracle_temporal(True, 20), "temporal, hostile history, %d x %d" % shape)


@pytest.mark.parametrize("k", [5, 7])
def test_spatial_on_hostile_neighbours(gpus, k):
    """k_spatial_gen<5> / <8> and k_spatial_resolve<5> / <8> (five and seven neighbours) on a stale G-buffer: background pixels that carry a foreground
    neighbour's normal and depth and a non-empty reservoir (only the occupancy clause rejects them), foreground reservoirs with M = 0 (only the M clause
    rejects them), M = 500, weight 0 and weight inf among the accepted neighbours and on the canonical pixel."""
    G = gpus()
    X, T, F, torch = G.X, G.T, G.X.F, G.torch
    m = G.mods[4] if k == 5 else G.module(neighbor_count=k)
    out = (torch.full((F.N, 3), 7.0, device="cuda"), torch.full((F.N, 1), 7.0, device="cuda"), torch.full((F.N, 1), 7, dtype=torch.int32, device="cuda"),
           torch.full((F.N, 1), 7.0, device="cuda"))           # background pixels must be emptied, not left alone
    G.W.SpatialResampling_(m, T["pos"], out, G.res(X.sres), T["noff"], T["tex"], F.Wc, F.Hc, F.fx, F.fy, X.SPATIAL_INDEX, T["occ"], T["snd"], T["brdf"], T["rd"])
    _compare(out, X.oracle_spatial(k), "spatial, hostile neighbours, %d neighbours" % k)


# ------------------------------------------------------------------ the moved history pixel inside whole frames
@pytest.fixture(scope="module")
def thin(oracle, scene_mod):
    import torch
    from mirres_restir_nerf_mesh_amd import renderer_restir as RR
    T = R.ThinFrame(oracle, scene_mod)
    W = RR.restirbvhWorker(torch.from_numpy(T.vert).cuda(), torch.from_numpy(T.tri).cuda()); W.update_mesh(W.vrt, W.v_ind)
    refs = {}

    def reference(fx, fy):
        if (fx, fy) not in refs:
            refs[(fx, fy)] = oracle.render(fx, fy, R.THIN_SPP, R.THIN_OFFSET, (T.info, T.aabb), T.vert, T.tri, T.env, T.occ, T.normal, T.depth, T.kd, T.rm,
                                           T.ray_dir_raw, T.pos, mat=None)
        return refs[(fx, fy)]
    return T, W, RR, torch, reference


def _render(T, W, RR, torch, fx, fy):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mods = RR.load_m_for_restir(fx, fy)
    RR.set_random_offset(R.THIN_OFFSET)
    N = T.N
    z = lambda *s: torch.zeros(s, device="cuda")
    out = RR.run_restir_di_with_pt(False, 1.0, 1.0, 1.0, None, None, W, *mods[:8], *mods[8:17], cu(T.env), cu(T.occ[:, None].copy()), cu(T.normal), cu(T.depth[:, None]),
                                   cu(T.kd), cu(T.rm), cu(T.ray_dir_raw), cu(T.pos), z(N, 1), z(N, 4), z(N, 3), z(N, 3), fx, fy, R.THIN_SPP, 2, 2, 2.0, 0.1, 0.001)
    return [o.detach().cpu().numpy() for o in out]


@pytest.mark.parametrize("batch", [None, "1", "4"])
@pytest.mark.parametrize("shape", R.THIN_SHAPES)
def test_thin_frames_with_a_moved_history_pixel(thin, monkeypatch, shape, batch):
    """32768 surface pixels as a 16384 x 2 and as a 2 x 16384 frame, 6 samples, constant material: at coordinates of several thousand (float)x + u rounds up often
    enough that some 50 pixels over the frame's five temporal passes take their history from the right / lower neighbour and accept it
    (test_reservoir_fixtures.py asserts at least 20).  All six output buffers equal the oracle's bit for bit.
    MIRRES_PT_BATCH unset: one batch holds the six samples and every temporal merge is fused into the previous sample's k_spatial_resolve<5, true>, which
    recomputes the neighbour's spatial merge for a moved history pixel.  4: batches of 4 + 2 — the merge of sample 4, first of its batch, goes through k_temporal,
    the others are fused.  1: a batch of one never has a next sample to fuse with (fuse_next needs k + 1 < batch size), so every merge goes through k_temporal."""
    T, W, RR, torch, reference = thin
    fx, fy = shape
    if batch is None:
        monkeypatch.delenv("MIRRES_PT_BATCH", raising=False)
    else:
        monkeypatch.setenv("MIRRES_PT_BATCH", batch)
    ref = reference(fx, fy)
    got = _render(T, W, RR, torch, fx, fy)
    for g, n in zip(got, ("final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec")):
        assert np.isfinite(g).all()
        pixel_parity(g, ref[n], "thin frame %d x %d, batch %s / %s" % (fx, fy, batch, n), tol=0.0)
