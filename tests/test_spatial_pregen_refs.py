"""CPU proof that the fixtures of tests/test_gpu_spatial_pregen.py test what they claim (oracle only, no GPU)."""
import os

import numpy as np

import reservoir_refs as R
import spatial_pregen_refs as P
from util import SmallFrame

DEFAULT_SEED = os.environ.get("MIRRES_TEST_SEED", "0") == "0"


def test_tiny_roughness_empties_foreground_reservoirs_that_are_accepted_neighbours(oracle, scene_mod):
    """In the 48 x 144 frame with spatial_pregen_refs.hostile_roughness, foreground pixels whose reservoir holds M == 0 are in-bounds, geometrically accepted
    neighbours of other foreground pixels in EVERY one of the seven samples ([17, 10, 12, 12, 18, 13, 15] on the default frame): "neighbour reservoir M != 0" decides
    alone there.  With the frame's own roughness it never does, and the oracle's frame stays finite."""
    F = SmallFrame(oracle, scene_mod, fx=48, fy=144)
    rm = P.hostile_roughness(F)
    counts = P.m_zero_neighbours(oracle, F, rm, 7, 4242)
    assert min(counts) >= (3 if DEFAULT_SEED else 1), counts
    assert sum(P.m_zero_neighbours(oracle, F, F.rm, 7, 4242)) == 0
    ref = oracle.render(F.fx, F.fy, 7, 4242, (F.info, F.aabb), F.vert, F.tri, F.env, F.occ, F.normal, F.depth, F.kd, rm, F.ray_dir_raw, F.pos, mat=None)
    assert all(np.isfinite(ref[n]).all() for n in ("final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"))


def test_geometric_pairs_are_the_accepted_pairs_of_full_reservoirs(oracle, scene_mod):
    """geometric_pairs counts what the spatial pass accepts when no reservoir is empty, and the pass index moves from 3 to 4 after sample 0."""
    F = SmallFrame(oracle, scene_mod, fx=40, fy=32)
    pairs = P.geometric_pairs(oracle, F, 3, 4242)
    assert len(pairs) == 3 and min(pairs) > 0
    c = R.classify_spatial(oracle, F.fx, F.fy, F.occ, F.normal_depth, np.ones(F.N, np.int32), np.ones(F.N, np.float32), F.noff, 4242 + 20 + 4)
    assert pairs[1] == int((c.cls == R.S_ACCEPTED).sum())
    c0 = R.classify_spatial(oracle, F.fx, F.fy, F.occ, F.normal_depth, np.ones(F.N, np.int32), np.ones(F.N, np.float32), F.noff, 4242 + 3)
    assert pairs[0] == int((c0.cls == R.S_ACCEPTED).sum())
    assert pairs[0] <= 5 * int((F.occ > 0.5).sum())
