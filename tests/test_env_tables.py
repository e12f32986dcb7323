"""CPU: the oracle's environment-light tables and light tiles (oracle/orc_light.hpp) on the hostile map catalogue of tests/envmap_refs.py, against the
float64 statements there — so that a misreading of make_sampleable.slang:62-86 or lightDi.slang:41-105 shared by oracle and kernel (which the GPU tests
compare bit for bit) fails here too.  Row and marginal sums, the 1e-4 fallback on both sides of the threshold, whole fallback rows, flat CDF runs, single
rows and columns, and an all-black map."""
import numpy as np
import pytest

import envmap_refs as E

CATALOGUE = E.catalogue()


@pytest.fixture(scope="module")
def frame(oracle, scene_mod):
    from util import SmallFrame
    return SmallFrame(oracle, scene_mod, fx=24, fy=20, subdiv=2, ground=4, env_hw=(16, 32))


def _oracle_frame(oracle, F, tex, H, W, tables):
    return oracle.make_frame(oracle.Keep(), F.fx, F.fy, F.occ, F.pos, F.normal_depth, F.brdf, F.ray_dir, (F.info, F.aabb), F.vert, F.tri, tex, W, H, tables)


@pytest.mark.parametrize("name", [n for n, _ in CATALOGUE])
def test_oracle_tables_and_tiles_match_float64(name, oracle, frame):
    env = dict(CATALOGUE)[name]
    H, W = env.shape[:2]
    tex = E.flip(env)
    tables = oracle.make_sampleable(tex, W, H)
    wts = oracle.env_weights(tex, W, H).reshape(H, W)
    E.check_weights(wts, env, name)
    R = E.check_tables(tables, wts, name)
    E.check_intent(name, env, R)
    ld, uv, p = oracle.light_tiles(_oracle_frame(oracle, frame, tex, H, W, tables), 3)
    E.check_tiles(tables, H, W, ld, uv, p, 3, name)


def test_the_catalogue_reaches_the_hostile_paths(oracle):
    """What the catalogue is for: heights past one 1024-entry chunk, widths on both sides of the 64-lane workgroup and of the chunk, whole fallback rows,
    flat CDF runs of positive pdf (zero-width intervals the search must skip)."""
    shapes = {env.shape[:2] for _, env in CATALOGUE}
    assert max(h for h, _ in shapes) > 1024 and {63, 64, 65, 1023, 1024, 1025} <= {w for _, w in shapes}
    fall = flat = 0
    for name, env in CATALOGUE:
        H, W = env.shape[:2]
        pdf, cdf, _, _ = oracle.make_sampleable(E.flip(env), W, H)
        fall += int(E.distribution64(oracle.env_weights(E.flip(env), W, H).reshape(H, W))["fallback"].sum())
        flat += int(((np.diff(cdf.reshape(H, W + 1), axis=1) == 0) & (pdf.reshape(H, W) > 0)).sum())
    assert fall > 100 and flat > 100, (fall, flat)


def test_oracle_tile_texels_follow_the_tables(oracle, frame):
    env = E.chi_square_map()
    H, W = env.shape[:2]
    tex = E.flip(env)
    tables = oracle.make_sampleable(tex, W, H)
    ld, uv, _ = oracle.light_tiles(_oracle_frame(oracle, frame, tex, H, W, tables), 11)
    E.check_texel_frequencies(tables, H, W, ld, uv)


def test_fallback_threshold_in_float64():
    """distribution64 itself: a row just below 1e-4 is uniform with its raw sum kept in the marginal, a row just above is normalised."""
    w = np.zeros((3, 4))
    w[0] = 0.99e-4 / 4; w[1] = 1.01e-4 / 4; w[2] = [1.0, 0.0, 3.0, 0.0]
    R = E.distribution64(w)
    assert R["fallback"].tolist() == [True, False, False]
    assert (R["pdf"][0] == 0.25).all() and (R["cdf"][0] == [0, 0.25, 0.5, 0.75, 1]).all()
    np.testing.assert_allclose(R["pdf"][1], 0.25) and np.testing.assert_allclose(R["pdf"][2], [0.25, 0, 0.75, 0])
    np.testing.assert_allclose(R["mpdf"], np.array([0.99e-4, 1.01e-4, 4.0]) / (4.0 + 2e-4))
    np.testing.assert_allclose(R["mcdf"], np.cumsum([0, 0.99e-4, 1.01e-4, 4.0]) / (4.0 + 2e-4))


def test_oracle_all_black_map(oracle, frame):
    """All black: every row falls back, the marginal divides 0 by 0 (NaN, as the reference's arithmetic gives), and the frame is finite and black: no
    light sample carries radiance, so no reservoir takes one.  tests/test_gpu_envmap.py pins the kernels to this."""
    F = frame
    env = np.zeros((16, 32, 3), np.float32)
    pdf, cdf, mpdf, mcdf = oracle.make_sampleable(E.flip(env), 32, 16)
    assert (pdf == np.float32(1 / 32)).all() and (cdf.reshape(16, 33)[:, :32] == (np.arange(32) / 32).astype(np.float32)).all()
    assert np.isnan(mpdf).all() and np.isnan(mcdf[:16]).all() and mcdf[16] == 1
    ref = oracle.render(F.fx, F.fy, 2, 7, (F.info, F.aabb), F.vert, F.tri, env, F.occ, F.normal, F.depth, F.kd, F.rm, F.ray_dir_raw, F.pos, mat=None)
    fg = F.occ > 0.5
    for k in ("final_color", "diffuse", "spec", "indirect", "indirect_diff", "indirect_spec"):
        assert np.isfinite(ref[k]).all() and (ref[k][fg] == 0).all(), k
    assert (ref["final_color"][~fg] == 1).all()
