"""The spatial pass with its neighbour acceptance made per batch (csrc/passes.hip k_spatial_accept, MIRRES_SPATIAL_PREGEN) against the generator inside the chain
(MIRRES_SPATIAL_PREGEN=0) and against the CPU oracle: all six output buffers, bit for bit.

k_spatial_accept makes three of the reference's four acceptance tests (in bounds, isValidNeighbor, neighbour is foreground) for the K samples of a batch at once;
the fourth, "neighbour reservoir M != 0", is made by the merge.  mirres_debug_spatial_pregen says whether a frame ran that way, and how many pairs each sample of its
first batch queued."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spatial_pregen_refs as P
from util import SmallFrame

pytestmark = pytest.mark.gpu

NAMES = ["final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"]
SPP, BATCH, SEED = 7, 3, 4242      # batches of 3, 3, 1: a first-of-batch temporal merge, fused merges, a ragged last batch; pass index 3 -> 4 after sample 0


def _pregen_report(ctx):
    """(ran, pairs of every sample of the first batch) of the context's last frame."""
    from mirres_restir_nerf_mesh_amd import _lib
    L = _lib.lib()
    L.mirres_debug_spatial_pregen.restype = C.c_int
    L.mirres_debug_spatial_pregen.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    ran, n = C.c_int(-1), C.c_int(-1); pairs = (C.c_uint32 * 64)()
    _lib.check(L.mirres_debug_spatial_pregen(ctx.h, C.byref(ran), C.byref(n), pairs), "mirres_debug_spatial_pregen")
    return ran.value, list(pairs[:n.value])


def _scaled_mlp(scene_mod, torch):      # the material field of tests/test_gpu_render.py's schedule tests
    from mirres_restir_nerf_mesh_amd.render_helper import MLPTexture3D
    mn, mx = scene_mod.material_min_max()
    mlp = MLPTexture3D(torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32), channels=6, min_max=(torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()), seed=3)
    with torch.no_grad():
        mlp.encoder.params.mul_(1e3)
    return mlp


def _oracle_mat(oracle, scene_mod, mlp, keep):
    """The oracle's restatement of the field `mlp` holds (same table, same weights)."""
    mn, mx = scene_mod.material_min_max()
    w = [mlp.net.net[i].weight.detach().cpu().numpy().copy() for i in (0, 2, 4)]
    return oracle.matnet_struct(keep, mlp.encoder.params.detach().cpu().numpy().copy(), w[0], w[1], w[2], (-1, -1, -1), (1, 1, 1), mn, mx)


class Scene:
    """One small frame on the device, its worker and its material field; frames are rendered with the knobs given."""

    def __init__(self, oracle, scene_mod, fx, fy, with_mlp=True):
        import torch
        from mirres_restir_nerf_mesh_amd import renderer_restir as RR
        self.torch, self.RR, self.oracle = torch, RR, oracle
        self.F = F = SmallFrame(oracle, scene_mod, fx=fx, fy=fy)
        self.W = RR.restirbvhWorker(torch.from_numpy(F.vert).cuda(), torch.from_numpy(F.tri).cuda()); self.W.update_mesh(self.W.vrt, self.W.v_ind)
        self.mlp = _scaled_mlp(scene_mod, torch) if with_mlp else None
        self.keep = oracle.Keep()
        self.mat = _oracle_mat(oracle, scene_mod, self.mlp, self.keep) if with_mlp else None
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.g = {"occ": cu(F.occ[:, None].copy()), "normal": cu(F.normal), "depth": cu(F.depth[:, None]), "kd": cu(F.kd), "rm": cu(F.rm), "ray_dir": cu(F.ray_dir_raw), "pos": cu(F.pos)}
        self.env = F.env

    def render(self, ctx, rm=None, spp=SPP, g=None, **kw):
        torch = self.torch; g = self.g if g is None else g
        e = torch.from_numpy(np.ascontiguousarray(self.env)).cuda()
        rm = g["rm"] if rm is None else torch.from_numpy(np.ascontiguousarray(rm)).cuda()
        outs, _, _ = self.RR.render_fused(ctx, self.W, self.mlp, False, (1, 1, 1), e, g["occ"].clone(), g["normal"], g["depth"], g["kd"], rm, g["ray_dir"], g["pos"],
                                          spp, 2, 2, 2.0, 0.1, 0.001, SEED, **kw)
        torch.cuda.synchronize()
        return [o.clone() for o in outs]

    def reference(self, rm=None, spp=SPP):
        F = self.F
        return self.oracle.render(F.fx, F.fy, spp, SEED, (F.info, F.aabb), F.vert, F.tri, self.env, F.occ, F.normal, F.depth, F.kd, F.rm if rm is None else rm,
                                  F.ray_dir_raw, F.pos, mat=self.mat)


def _knobs(setenv, pregen, streams=2, batch=BATCH, bands=None):
    for k, v in (("MIRRES_SPATIAL_PREGEN", pregen), ("MIRRES_STREAMS", streams), ("MIRRES_PT_BATCH", batch), ("MIRRES_BANDS", bands)):
        setenv(k, None if v is None else str(v))


def _setenv_of(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def _same_bits(got, ref, what):
    """torch.equal of the six buffers (`ref`: tensors, or the oracle's arrays)."""
    import torch
    for k, (a, b) in enumerate(zip(got, ref)):
        b = b if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(a.device)
        assert torch.equal(a, b), "%s: buffer %d (%s) differs in %d values" % (what, k, NAMES[k], int((a != b).sum()))


@pytest.fixture(scope="module", params=[(40, 32), (48, 144)], ids=["40x32", "48x144"])      # 40 is no multiple of the 16-pixel tile; 48 x 144: nine tiles high, the band test's shape
def scene(request, oracle, scene_mod):
    fx, fy = request.param
    S = Scene(oracle, scene_mod, fx, fy)
    S.ref = S.reference()
    S.pairs = P.geometric_pairs(oracle, S.F, BATCH, SEED)
    return S


@pytest.mark.parametrize("streams", [1, 2])
def test_acceptance_per_batch_renders_the_frame_of_the_generator_in_the_chain_and_of_the_oracle(scene, monkeypatch, streams):
    """Knob on against knob off in one process, and both against the oracle's render: 7 samples in batches of 3, 3, 1, the scaled material field, on one stream and on
    two.  The debug entry point says which frame took its acceptance from k_spatial_accept, and the pair counts of the first batch are the ones the three
    geometric clauses give on the CPU (tests/spatial_pregen_refs.py)."""
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    S = scene; ctx = get_ctx(S.F.fx, S.F.fy); setenv = _setenv_of(monkeypatch)
    _knobs(setenv, 0, streams)
    off = S.render(ctx)
    assert _pregen_report(ctx) == (0, [])
    _knobs(setenv, 1, streams)
    on = S.render(ctx)
    ran, pairs = _pregen_report(ctx)
    assert ran == 1 and pairs == S.pairs and min(pairs) > 0, (ran, pairs, S.pairs)
    for k, (a, b) in enumerate(zip(on, off)):
        assert S.torch.equal(a, b), "streams %d: buffer %d (%s) differs between MIRRES_SPATIAL_PREGEN=1 and =0 in %d values" % (streams, k, NAMES[k], int((a != b).sum()))
    _same_bits(on, [S.ref[n] for n in NAMES], "acceptance per batch against the oracle, %d stream(s)" % streams)
    _same_bits(off, [S.ref[n] for n in NAMES], "generator in the chain against the oracle, %d stream(s)" % streams)


def _moved_test_check(oracle, scene_mod, setenv):
    """A frame in which FOREGROUND reservoirs entering a spatial pass hold M == 0 (spatial_pregen_refs.hostile_roughness) and are geometrically accepted neighbours,
    in every sample: the one clause the merge now makes decides.  Knob on = knob off = oracle."""
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    S = Scene(oracle, scene_mod, 48, 144, with_mlp=False)
    rm = P.hostile_roughness(S.F)
    counts = P.m_zero_neighbours(oracle, S.F, rm, SPP, SEED)
    assert min(counts) >= 1, counts      # [17, 10, 12, 12, 18, 13, 15] on the default frame
    ref = S.reference(rm)
    ctx = get_ctx(S.F.fx, S.F.fy)
    frames = {}
    for pregen in (0, 1):
        _knobs(setenv, pregen)
        frames[pregen] = S.render(ctx, rm)
        assert _pregen_report(ctx)[0] == pregen
    _same_bits(frames[1], frames[0], "M == 0 neighbours: MIRRES_SPATIAL_PREGEN=1 against =0")
    _same_bits(frames[1], [ref[n] for n in NAMES], "M == 0 neighbours: acceptance per batch against the oracle")
    _same_bits(frames[0], [ref[n] for n in NAMES], "M == 0 neighbours: generator in the chain against the oracle")


def test_a_foreground_neighbour_with_an_empty_reservoir_is_passed_over_by_the_merge(oracle, scene_mod, monkeypatch):
    _moved_test_check(oracle, scene_mod, _setenv_of(monkeypatch))


def test_the_same_with_every_spatial_shadow_ray_traced():
    """MIRRES_SKIP_DEAD=0 (latched per process: a child process): the pair of an emptied neighbour then traces BOTH its rays, and still no answer reaches the frame."""
    env = dict(os.environ, MIRRES_SKIP_DEAD="0"); env.pop("MIRRES_PARITY_REPORT", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "moved-test"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("moved-test ok"), (r.stdout[-2000:], r.stderr[-2000:])


def test_a_strip_without_overlap_takes_its_acceptance_per_batch(oracle, scene_mod, monkeypatch):
    """Rank 0 of the two-rank split of a 48 x 96 image with the recorded halo (no strip_overlap): the acceptance reads the true G-buffer, halo rows included, and
    the exchanged reservoirs only in the merge.  Knob on = knob off, and the own rows are the whole frame's."""
    from mirres_restir_nerf_mesh_amd import dist as D, _lib, _ops
    S = Scene(oracle, scene_mod, 48, 96); fx, fy, spp = 48, 96, 4
    setenv = _setenv_of(monkeypatch)
    rec = {}
    def recorder(user, records, sample, stream):
        rec[sample] = D.device_view(records, (fy, fx, 8)).clone()
        return 0
    _knobs(setenv, 0)
    ref = S.render(_ops.Context(fx, fy), spp=spp, strip=(fy, 0, 0, fy), halo=_lib.HALO_FN(recorder))
    y0, y1, lo, hi = D.strip_rows(fy, 0, 2)
    plan = D.halo_plan(fy, fx, 0, 2)
    loc = {k: v[lo * fx:hi * fx].contiguous() for k, v in S.g.items()}
    def replay(user, records, sample, stream):
        view = D.device_view(records, (hi - lo, fx, 8))
        for peer, send, (ra, rb) in plan:
            view[ra:rb].copy_(rec[sample][lo + ra:lo + rb])
        return 0
    ctx = _ops.Context(fx, hi - lo)
    frames = {}
    for pregen in (0, 1):
        _knobs(setenv, pregen)
        frames[pregen] = S.render(ctx, spp=spp, g=loc, strip=(fy, lo, y0 - lo, y1 - lo), halo=_lib.HALO_FN(replay))
        assert _pregen_report(ctx)[0] == pregen
    for k, (a, b) in enumerate(zip(frames[1], frames[0])):
        assert S.torch.equal(a, b), "strip: buffer %d differs between MIRRES_SPATIAL_PREGEN=1 and =0" % k
        assert S.torch.equal(ref[k][y0 * fx:y1 * fx], a[(y0 - lo) * fx:(y1 - lo) * fx]), "strip: buffer %d differs from the whole frame's rows" % k
    # with strip_overlap the pass is cut into row-restricted launches: the generator stays in the chain, the frame is the same
    got = S.render(ctx, spp=spp, g=loc, strip=(fy, lo, y0 - lo, y1 - lo), halo=_lib.HALO_FN(replay), strip_overlap=True)
    assert _pregen_report(ctx)[0] == 0
    for k, (a, b) in enumerate(zip(got, frames[0])):
        assert S.torch.equal(a, b), "strip_overlap with the knob on: buffer %d differs" % k


def test_bands_and_the_counting_mode_keep_the_generator_in_the_chain(oracle, scene_mod, monkeypatch):
    """The fallbacks with the knob on: a band frame (MIRRES_BANDS=2) and a counting-mode frame run k_spatial_gen inside the chain and give the reference frame."""
    from mirres_restir_nerf_mesh_amd._ops import get_ctx
    S = Scene(oracle, scene_mod, 48, 144); ctx = get_ctx(48, 144); setenv = _setenv_of(monkeypatch)
    _knobs(setenv, 0)
    ref = S.render(ctx)
    _knobs(setenv, 1, bands=2)
    got = S.render(ctx)
    assert _pregen_report(ctx)[0] == 0
    for k, (a, b) in enumerate(zip(got, ref)):
        assert S.torch.equal(a, b), "band frame with the knob on: buffer %d differs" % k
    _knobs(setenv, 1)
    ctx.set_instrument(1); ctx.stats(reset=True)
    try:
        got = S.render(ctx)
        ran = _pregen_report(ctx)[0]
        st = ctx.stats(reset=True)
    finally:
        ctx.set_instrument(0)
    assert ran == 0 and st["rays_any"] > 0
    for k, (a, b) in enumerate(zip(got, ref)):
        assert S.torch.equal(a, b), "counting-mode frame with the knob on: buffer %d differs" % k


if __name__ == "__main__" and sys.argv[1:] == ["moved-test"]:      # the child process of test_the_same_with_every_spatial_shadow_ray_traced
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from oracle import oracle as O
    import mirres_restir_nerf_mesh_amd as M
    O.lib()
    def _setenv(k, v):
        if v is None: os.environ.pop(k, None)
        else: os.environ[k] = v
    _moved_test_check(O, M.scene, _setenv)
    print("moved-test ok")
