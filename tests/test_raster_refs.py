"""CPU: the conditions tests/test_gpu_raster_adjoints.py rests on, established by the references alone (tests/raster_refs.py, tests/util.py) — no HIP code runs here.

  * aa_analyse (decisions + margins) reproduces util.antialias_ref's pairs exactly, so the float64 blend the GPU tests compare with is the project's
    independent statement of dr.antialias, the one test_antialias_reference_statement_on_analytic_edges pins to closed-form answers;
  * no scene has a pair whose nearest decision is closer than 1e-3 px to flipping: the GPU tests exclude nothing and compare every element;
  * the scenes contain every case the kernel distinguishes, in numbers;
  * aa_torch's position gradient is the derivative of antialias_ref (central differences, per element);
  * the float32 evaluation of the same expression — the noise floor the GPU tolerances stand on.

Measured (this file prints the figures with -s):
    scene                 lowest margin [px]   blends  min of the 8 (axis, s, sign) counts  tri-vs-tri  boundary  fold  skipped w<=0  edges skipped opp w<=0
    seed7-24x20                0.0045           153            14                               48        140      13        0             0
    seed7-24x20-behind         0.0045           122            10                               50        109      13       62            24
    seed7-17x15                0.0027           106             9                               31         97       9        0             0
    seed7-17x15-behind         0.0027            88             6                               31         79       9       39            16
    seed22-24x20               0.0023           190            16                               35        174      16        0             0
    seed22-24x20-behind        0.0023           164            12                               31        148      16       43            27
    seed22-17x15               0.0017           124            10                               22        114      10        0             0
    seed22-17x15-behind        0.0017           110             8                               19        100      10       27            14
    seed7-16x16                0.0021           103             8                               30         95       8        0             0
    seed7-257x1                0.0192             6             -                                4          6       0        0             0
    fold 0.018 (10 fold blends), sliver 0.0625 (6 two-crossing pairs), shared interior edge 0.023, row 16x1 and column 1x16 0.0156.
    float32 noise: max |alpha32 - alpha64| 1.3e-6 .. 1.4e-5 on the random scenes (<= 2.5e-8 on the hand-made ones, whose coordinates are exact);
    position gradient max error 3.7e-7 .. 1.1e-5 of the largest element."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_refs as R
from util import antialias_ref, elementwise

KEYS = [k for k, _ in R.scene_specs()]
RANDOM_MAIN = [k for k in KEYS if k[0] == "random" and (k[2], k[3]) in R.SIZES]
MARGIN = 1e-3


def _inputs(sc, C=3, seed=7):
    rng = np.random.default_rng(seed)
    n = sc.H * sc.W
    color = (0.25 + 0.75 * rng.random((n, C))).astype(np.float32).astype(np.float64)
    gout = (rng.random((n, C)) - 0.5).astype(np.float32).astype(np.float64)
    return color, gout


@pytest.mark.parametrize("key", KEYS, ids=R.scene_id)
def test_analysis_reproduces_the_reference_statement_and_no_decision_is_marginal(key):
    sc = R.get_scene(key)
    color, _ = _inputs(sc)
    ref_out, pairs = antialias_ref(color, sc.rast, sc.pos, sc.tri, sc.opp, sc.H, sc.W)
    assert R.aa_pairs(sc.recs) == pairs                                   # same pairs, same edges, alpha bit for bit
    out, alpha = R.aa_torch(torch.from_numpy(color), torch.from_numpy(sc.pos), sc.recs, sc.H, sc.W)
    # the vectorised blend is the looped one; it projects with x * (1 / w) as the kernel does, antialias_ref with x / w: pixel coordinates up to 257 carry
    # 6e-14 of float64 rounding, the crossing amplifies it by 1 / |bo - ao| <= 500 (both end points keep the margin) -> 1e-11 at the very most
    assert np.abs(out.numpy() - ref_out).max() <= 1e-11
    assert np.abs(alpha.numpy() - np.array([p[2] for p in pairs if p[2] != 0])).max() <= 1e-11
    low = [r for r in sc.recs if r.margin < MARGIN]
    print("%s: %d pairs, %d blends, lowest margin %.4f px" % (sc.name, len(sc.recs), sum(r.blend for r in sc.recs), min(r.margin for r in sc.recs)))
    assert not low, "%s: %d pair(s) within %g px of another decision, e.g. pixels (%d, %d): %s — choose another seed" % (
        sc.name, len(low), MARGIN, low[0].lo, low[0].hi, low[0].label)
    # the inputs are what the kernel will read: fp32 values, ids within [0, T], vertex indices within [0, V), finite w != 0
    assert np.array_equal(sc.pos.astype(np.float32).astype(np.float64), sc.pos) and np.array_equal(sc.rast.astype(np.float32).astype(np.float64), sc.rast)
    ids = sc.rast[:, 3]
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 0 and ids.max() <= len(sc.tri)
    assert sc.tri.min() >= 0 and sc.tri.max() < len(sc.pos) and sc.opp.min() >= -1 and sc.opp.max() < len(sc.pos)
    assert np.isfinite(sc.pos).all() and (sc.pos[:, 3] != 0).all()
    if key[0] != "random":
        assert np.array_equal(sc.pos, sc.pos_exact)                       # hand-made coordinates are exact in fp32


@pytest.mark.parametrize("key", RANDOM_MAIN, ids=R.scene_id)
def test_random_scenes_contain_every_case_in_numbers(key):
    sc = R.get_scene(key)
    B = [r for r in sc.recs if r.blend]
    cat = Counter(r.category for r in B)
    counts = {(a, s, g): cat.get((a, s, g), 0) for a in (0, 1) for s in (1, -1) for g in ("alpha>0", "alpha<0")}
    tritri = sum(r.versus == "tri" for r in B); boundary = sum(r.sil == "boundary" for r in B); fold = sum(r.sil == "fold" for r in B)
    behind = sum(r.kind == "behind" for r in sc.recs); opp_behind = sum(r.n_opp_behind for r in sc.recs)
    print("%s: categories %s, tri-vs-tri %d, boundary %d, fold %d, skipped w<=0 %d, edges skipped opp w<=0 %d" % (sc.name, sorted(counts.items()), tritri, boundary, fold, behind, opp_behind))
    assert min(counts.values()) >= 3, counts
    assert tritri >= 15 and boundary >= 60, (tritri, boundary)
    if key[4]:
        assert behind >= 10 and opp_behind >= 10, (behind, opp_behind)
    else:
        assert behind == 0 and opp_behind == 0


def test_hand_made_scenes_supply_what_the_random_ones_lack():
    recs = {f.__name__: R.get_scene((f.__name__,)).recs for f in R.HAND_MADE}
    folds = sum(r.blend and r.sil == "fold" for rs in recs.values() for r in rs)
    twice = sum(r.blend and r.n_cross > 1 for rs in recs.values() for r in rs)
    assert folds >= 5 and twice >= 3, (folds, twice)
    assert sum(r.blend and r.sil == "fold" for r in recs["scene_fold"]) >= 5
    # the sliver: in every two-crossing pair the NEARER crossing decides, and it is the left long edge (vertices 0 -> 2 of the triangle)
    sl = [r for r in recs["scene_sliver"] if r.blend]
    assert len(sl) >= 3 and all(r.n_cross == 2 and {r.va, r.vb} == {0, 2} and -0.5 < r.alpha < -0.2 for r in sl)
    # the shared interior edge: pairs across it exist and none of them blends
    sh = recs["scene_shared_edge"]
    across = [r for r in sh if r.versus == "tri"]
    assert len(across) >= 5 and all(r.kind == "none" for r in across) and sum(r.blend for r in sh) >= 10
    # one-pixel frames: one axis only
    assert {r.axis for r in recs["scene_row"]} == {0} and {r.axis for r in recs["scene_column"]} == {1}
    assert sum(r.blend for r in recs["scene_row"]) >= 3 and sum(r.blend for r in recs["scene_column"]) >= 3


def test_position_gradient_is_the_derivative_of_the_reference_statement():
    """aa_torch's autograd gradient against central differences of util.antialias_ref in float64, element by element (x, y, w of every vertex; z does not
    enter), on the 17 x 15 scene of seed 7 with `behind`.
    Step h = 1e-6 in clip units: a vertex moves by at most h (W / 2) / w_min = 2e-5 px, fifty times less than the 1e-3 px margin, so no decision flips and
    the loss is a smooth (rational) function along the step.  The error of a central difference is h^2 |f'''| / 6 + u |L| / h.  Rounding: u = 1.1e-16,
    |L| <= sum |g| |out| < 400, so u |L| / h < 4.4e-8.  Truncation: alpha is a ratio of two expressions bilinear in the projected end points; each derivative with
    respect to a clip coordinate multiplies by at most K = (W / 2 w_min) / |bo - ao|_min, and |bo - ao| >= 2e-3 (both end points keep the 1e-3 margin from
    the line), w_min = 0.4: K <= 1.1e4 and h^2 K^2 / 6 <= 2e-5 RELATIVE to the element in the worst case — the bound: 2e-5 |f'| + 4.4e-8 absolute.
    (Measured: largest difference 2.9e-9 absolute at a gradient scale of 21: the edges of this scene are far from the worst case.)"""
    sc = R.get_scene(("random", 7, 15, 17, True))
    color, gout = _inputs(sc)
    pos = torch.tensor(sc.pos, requires_grad=True)
    out, _ = R.aa_torch(torch.from_numpy(color), pos, sc.recs, sc.H, sc.W)
    (out * torch.from_numpy(gout)).sum().backward()
    g = pos.grad.numpy()
    assert (g[:, 2] == 0).all()
    loss = lambda P: float((antialias_ref(color, sc.rast, P, sc.tri, sc.opp, sc.H, sc.W)[0] * gout).sum())
    h = 1e-6
    used = sorted({v for r in sc.recs if r.blend for v in (r.va, r.vb)})
    assert len(used) >= 20 and (np.abs(g[[v for v in range(len(g)) if v not in used]]) == 0).all()
    worst = 0.0
    for v in range(len(sc.pos)):
        for c in (0, 1, 3):
            if v not in used and c != 0:
                continue                                      # vertices no blended edge names: one component each is enough to see the zero
            d = np.zeros_like(sc.pos); d[v, c] = h
            fd = (loss(sc.pos + d) - loss(sc.pos - d)) / (2 * h)
            worst = max(worst, abs(fd - g[v, c]))
            assert abs(fd - g[v, c]) <= 2e-5 * abs(g[v, c]) + 4.4e-8, (v, c, fd, g[v, c])
    print("central differences vs autograd: largest difference %.2e (gradient scale %.2e)" % (worst, np.abs(g).max()))


@pytest.mark.parametrize("key", KEYS, ids=R.scene_id)
def test_float32_noise_floor(key):
    """The same restatement evaluated in torch float32 with the decisions held fixed, against float64: what fp32 arithmetic alone does to the blend weight and
    to the position gradient.  Measured: max |alpha32 - alpha64| 1.3e-6 .. 1.4e-5 on the random scenes (largest: seed 22, 17 x 15), <= 2.5e-8 on the hand-made
    ones; position gradient error at most 1.1e-5 of the largest element (seed 22, 17 x 15; 3.4e-6 and below elsewhere).
    Asserted: the weight error stays below 1e-4 — a tenth of the 1e-3 px margin (alpha is a length in pixels), so fp32 cannot flip a decision the analysis
    admitted, and the forward bound of the GPU test (4 x this scene's figure) stays below 4e-4 of a colour difference; the gradient passes util.elementwise at
    rtol 1e-4 / atol_scale 1e-5, ten times tighter than the defaults (1e-3 / 1e-4) the GPU test applies to the kernel."""
    sc = R.get_scene(key)
    noise = R.aa_alpha_noise(sc)
    color, gout = _inputs(sc)
    grads = []
    for dt in (torch.float64, torch.float32):
        pos = torch.tensor(sc.pos, dtype=dt, requires_grad=True)
        out, _ = R.aa_torch(torch.tensor(color, dtype=dt), pos, sc.recs, sc.H, sc.W)
        (out * torch.tensor(gout, dtype=dt)).sum().backward()
        grads.append(pos.grad)
    err = float((grads[1].double() - grads[0]).abs().max() / grads[0].abs().max())
    print("%s: max |alpha32 - alpha64| %.2e, position gradient error %.2e of the largest element" % (sc.name, noise, err))
    assert noise < 1e-4
    elementwise(grads[1], grads[0], "float32 restatement of the position gradient, " + sc.name, rtol=1e-4, atol_scale=1e-5)


def test_interpolate_and_texture_restatements_on_known_answers():
    """interpolate_torch: a record at a vertex returns that vertex's attribute, the empty record returns 0.  texture_torch: a texel centre returns the texel,
    the midpoint between two centres their mean, anything beyond the outermost centres the edge texel; on a 1 x 1 texture every coordinate returns the texel."""
    attr = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], dtype=torch.float64)
    tri = torch.tensor([[0, 1, 2]])
    rast = torch.tensor([[1.0, 0, 0, 1], [0, 1.0, 0, 1], [0, 0, 0, 1], [0.25, 0.25, 0, 1], [0.3, 0.3, 0.5, 0], [1.5, -0.5, 0, 1]], dtype=torch.float64)
    assert R.interpolate_torch(attr, rast, tri).tolist() == [[1, 10], [2, 20], [4, 40], [2.75, 27.5], [0, 0], [0.5, 5.0]]
    db = R.interpolate_db_torch(attr, rast, tri, torch.tensor([[1.0, 0, 0, 1.0]] * 6, dtype=torch.float64), [1])
    assert db.tolist() == [[-30.0, -20.0]] * 4 + [[0.0, 0.0]] + [[-30.0, -20.0]]
    tex = torch.arange(12, dtype=torch.float64).view(2, 3, 2)                                 # texel (j, i) = (6 j + 2 i, 6 j + 2 i + 1)
    uv = torch.tensor([[0.5 / 3, 0.25], [2.5 / 3, 0.75], [1.0 / 3, 0.25], [0.5, 0.5], [-1e30, -1e30], [1e30, 1e30], [0.0, 1.0]], dtype=torch.float64)
    assert torch.allclose(R.texture_torch(tex, uv), torch.tensor([[0.0, 1], [10, 11], [1, 2], [5, 6], [0, 1], [10, 11], [6, 7]], dtype=torch.float64), rtol=0, atol=1e-14)
    one = torch.tensor([[[3.0]]], dtype=torch.float64)
    assert R.texture_torch(one, uv).view(-1).tolist() == [3.0] * 7
    touched = R.texture_touched(torch.tensor([[0.5 / 3, 0.25]]), 2, 3)
    assert touched.tolist() == [[True, True, False], [True, True, False]]                      # a centre: itself and, within the slack, its lower / right neighbours
    assert R.texture_touched(torch.tensor([[0.55 / 3, 0.55 / 3]]), 3, 3).tolist() == [[True, True, False], [True, True, False], [False, False, False]]
