"""The hostile reservoir fixtures (tests/reservoir_refs.py) do their job: every clause of the temporal and spatial passes decides for a countable set of pixels,
and the oracle agrees, pixel by pixel, with the plain restatement of who decides.  CPU only — the oracle alone.  tests/test_gpu_reservoir_hostile.py runs the HIP
passes on the same inputs."""
import os

import numpy as np
import pytest

import reservoir_refs as R
from util import SmallFrame

DEFAULT_SEED = os.environ.get("MIRRES_TEST_SEED", "0") == "0"      # the class counts are asserted for the default frame; a sweep value keeps everything else
MIN_CLASS = 15


@pytest.fixture(scope="module")
def fx(oracle, scene_mod):
    return R.Hostile(oracle, scene_mod)


def _count(name, n):
    print("%-40s %d" % (name, n))
    if DEFAULT_SEED:
        assert n >= MIN_CLASS, "%s: only %d pixels / candidates" % (name, n)


def _differs(a, b):
    """Per pixel: any of the four reservoir arrays differs in bits."""
    d = np.zeros(len(a[2]), bool)
    for x, y in zip(a, b):
        x = np.ascontiguousarray(x).reshape(len(d), -1); y = np.ascontiguousarray(y).reshape(len(d), -1)
        d |= (x.view(np.uint32) != y.view(np.uint32)).any(1)
    return d


def _finite(res, what):
    for a, nm in zip(res, ("light_data", "light_pdf", "M", "weight")):
        assert np.isfinite(a).all(), "%s: %s holds NaN or inf" % (what, nm)


def test_every_temporal_class_is_populated(fx):
    c = fx.temporal_classes(motion=True)
    for k, nm in R.T_NAMES.items():
        _count("temporal / " + nm, int((c.cls == k).sum()))
    for nm in ("moved", "other_context", "m_zero", "cap", "w_zero", "w_inf"):
        _count("temporal / accepted, " + nm, int(getattr(c, nm).sum()))
    _count("temporal / accepted at another pixel with another target context", int((c.moved & c.other_context).sum()))
    # without motion vectors the history pixel is the pixel itself, but a third of the history G-buffer belongs to another view
    c0 = fx.temporal_classes(motion=False)
    assert not c0.moved.any() and not (c0.cls == R.T_OUTSIDE).any()
    for k in (R.T_HIST_BG, R.T_NORMAL, R.T_DEPTH, R.T_ACCEPTED):
        _count("temporal, no motion / " + R.T_NAMES[k], int((c0.cls == k).sum()))
    for nm in ("other_context", "m_zero", "cap", "w_inf"):
        _count("temporal, no motion / accepted, " + nm, int(getattr(c0, nm).sum()))


@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("max_history", [20, 7])
def test_oracle_temporal_agrees_with_the_classification(fx, oracle, motion, max_history):
    F = fx.F
    c = fx.temporal_classes(motion, max_history)
    out = fx.oracle_temporal(motion, max_history)
    fg = F.occ > 0.5
    rejected = fg & ~c.accepted
    assert not _differs(out, fx.cur)[rejected | ~fg].any()            # a rejected pixel (and the background) keeps its input reservoir bit for bit
    _finite(out, "oracle.temporal on the hostile history")
    # an accepted pixel holds M_cur + min(M_history, M_cur * max_history) of the history pixel the classification names, unless store_ris emptied it
    a = np.flatnonzero(c.accepted)
    emptied = (out[2][a] == 0) & (out[3][a] == 0) & (out[0][a] == 0).all(1)
    want = fx.cur[2][a] + np.minimum(fx.prev[2][c.qi[a]], fx.cur[2][a] * max_history)
    assert np.array_equal(out[2][a][~emptied], want[~emptied])
    # an infinite history weight never survives: the reservoir is emptied (weight inf or NaN: store_ris) or nothing was selected (weight 0, no light sample)
    wi = c.w_inf[a]
    assert (wi | ~emptied).all()
    assert (emptied[wi] | ((out[3][a][wi] == 0) & (out[0][a][wi] == 0).all(1))).all()
    if DEFAULT_SEED:
        assert int((emptied & wi).sum()) >= MIN_CLASS
    if max_history == 20:
        benign = fx.oracle_temporal_benign()
        assert _differs(out, benign)[fg].mean() >= 0.25


def test_every_spatial_class_is_populated(fx):
    for k in (5, 7):
        c = fx.spatial_classes(k)
        for q, nm in R.S_NAMES.items():
            _count("spatial, %d neighbours / %s" % (k, nm), int((c.cls == q).sum()))
        _count("spatial, %d neighbours / accepted, weight 0" % k, int(c.w_zero.sum()))
        _count("spatial, %d neighbours / accepted, weight inf" % k, int(c.w_inf.sum()))
    # the point of the stale background: with the plain G-buffer (zero normals on the background) the geometry clause rejects those neighbours first
    plain = R.classify_spatial(fx.O, fx.F.fx, fx.F.fy, fx.F.occ, fx.F.normal_depth, fx.sres[2], fx.sres[3], fx.F.noff, fx.SPATIAL_INDEX, 5)
    assert not (plain.cls == R.S_BACKGROUND).any()


@pytest.mark.parametrize("k", [5, 7])
def test_oracle_spatial_agrees_with_the_classification(fx, oracle, k):
    F = fx.F
    c = fx.spatial_classes(k)
    out = fx.oracle_spatial(k)
    _finite(out, "oracle.spatial on the hostile neighbours")
    alone = fx.oracle_spatial(k, noff=R.outside_offsets())
    fg = F.occ > 0.5
    none_accepted = fg & ~(c.cls == R.S_ACCEPTED).any(1)
    assert none_accepted.sum() > 0 and (fg & ~none_accepted).sum() > 0
    assert not _differs(out, alone)[none_accepted].any()               # all candidates rejected: the output of the pass without neighbours
    assert _differs(out, alone)[fg & ~none_accepted].any()             # and accepted neighbours do reach the output
    assert (out[2][~fg] == 0).all() and (out[3][~fg] == 0).all()      # background pixels are emptied whatever their input reservoir held
    if k == 5:
        assert _differs(out, fx.oracle_spatial_benign())[fg].mean() >= 0.25


def test_thin_frames_move_the_history_pixel(oracle, scene_mod):
    """16384 x 2 and 2 x 16384: summed over the temporal passes of a 6-sample frame, at least 20 pixels take their history from the right / lower neighbour and
    accept it (the fused chain of k_spatial_resolve then recomputes that neighbour's spatial merge; k_temporal loads another pixel's reservoir)."""
    T = R.ThinFrame(oracle, scene_mod)
    assert (T.occ > 0.5).all()
    for fx_, fy_ in R.THIN_SHAPES:
        moved = T.moved_and_accepted(fx_, fy_, R.THIN_SPP, R.THIN_OFFSET)
        n = sum(len(m) for m in moved)
        print("thin frame %d x %d: moved and accepted per pass %s" % (fx_, fy_, [len(m) for m in moved]))
        if DEFAULT_SEED:
            assert n >= 20, "%d x %d: only %d moved history pixels" % (fx_, fy_, n)
