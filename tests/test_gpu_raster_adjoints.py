"""GPU: dr.antialias, dr.interpolate and dr.texture (csrc/antialias.hip, csrc/raster.hip, raster.py) against float64 restatements, element by element
(tests/raster_refs.py; the conditions on the inputs are asserted on the CPU by tests/test_raster_refs.py).

The raster record is an input of all three operators: it is built on the CPU in float64, rounded to fp32, and the identical fp32 arrays go to the kernel
and to the restatement.  No scene has a decision nearer than 1e-3 px to flipping, so nothing is excluded: every pixel, every colour-gradient element and
every position-gradient element is compared.  Tolerances: gradients and interpolated values with util.elementwise at its defaults (rtol 1e-3, atol 1e-4 of
the largest element, all elements) — for the antialias position gradient that is 9 to 250 times the float32 noise floor of the same expression
(test_raster_refs.py::test_float32_noise_floor); the antialiased image per pixel within 4 x that scene's float32 weight noise times the colour differences
it blends, plus 4 ulp.  Every test prints its largest error relative to its bound (-s).
Observed on the MI355X, largest error / bound: antialias forward 0.25, g_color 0.059, g_pos 0.024 (per category: 0.003); interpolate forward 6e-4, g_attr 3e-3,
g_uv 5e-4, out_db 5e-4; texture forward 1e-3, g_tex 4e-3."""
import functools
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_refs as R
from util import elementwise, same_bits

pytestmark = pytest.mark.gpu

KEYS = [k for k, _ in R.scene_specs()]
RTOL, ATOL_SCALE = 1e-3, 1e-4                     # util.elementwise's defaults, restated only to report error / bound and to find the offenders of a failure


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _ratio(got, want):
    """Largest error relative to util.elementwise's bound at its defaults, and the mask of elements beyond it."""
    got = got.detach().double().cpu().numpy(); want = want.detach().double().cpu().numpy()
    bound = RTOL * np.abs(want) + ATOL_SCALE * np.abs(want).max()
    err = np.abs(got - want)
    return float((err / bound).max()), err > bound


def _check(got, want, what, explain=None):
    ratio, bad = _ratio(got, want)
    print("%s: largest error %.3g of its bound" % (what, ratio))
    try:
        elementwise(got, want, what)
    except AssertionError as e:
        raise AssertionError(str(e) + ("\n" + explain(bad) if explain else "")) from None


def _by_category(sc, involved, bad_items, what):
    """Which kinds of pair the offending elements have in common: `involved(r)` = the items (pixels or vertices) blend r bears on."""
    bad_items = set(int(i) for i in bad_items)
    hit = Counter(); total = Counter()
    for r in sc.recs:
        if r.blend:
            total[r.label] += 1
            if bad_items & set(involved(r)):
                hit[r.label] += 1
    lines = ["%s: %d offending %s; pairs bearing on them, by category (offending / all of that category in the scene):" % (sc.name, len(bad_items), what)]
    lines += ["    %3d / %3d  %s" % (hit[k], total[k], k) for k in sorted(hit, key=lambda k: -hit[k] / total[k])]
    # one property at a time: a defect confined to one case shows as a property whose pairs all offend while the others' do not
    props = (("axis", lambda r: r.axis), ("s", lambda r: int(r.s)), ("sign of alpha", lambda r: "+" if r.alpha > 0 else "-"), ("silhouette", lambda r: r.sil),
             ("against", lambda r: r.versus), ("crossings", lambda r: min(r.n_cross, 2)))
    for name, f in props:
        h = Counter(); t = Counter()
        for r in sc.recs:
            if r.blend:
                t[f(r)] += 1; h[f(r)] += bool(bad_items & set(involved(r)))
        lines.append("    by %-13s %s" % (name + ":", ",  ".join("%s: %d / %d" % (k, h[k], t[k]) for k in sorted(t, key=str))))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------------- antialias

def _aa_inputs(sc, C):
    rng = np.random.default_rng(100 + C)
    n = sc.H * sc.W
    return (0.25 + 0.75 * rng.random((n, C))).astype(np.float32), (rng.random((n, C)) - 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _aa_reference(key, C, boost):
    """Float64: (out, g_color, g_pos, alpha) of one scene — computed once, shared, never modified."""
    sc = R.get_scene(key)
    color, gout = _aa_inputs(sc, C)
    col = torch.tensor(color, dtype=torch.float64, requires_grad=True); pos = torch.tensor(sc.pos, requires_grad=True)
    out, alpha = R.aa_torch(col, pos, sc.recs, sc.H, sc.W, pos_gradient_boost=boost)
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    return out.detach(), col.grad, pos.grad, alpha.detach()


def _aa_run(sc, color, gout, boost, want_color=True, want_pos=True):
    from mirres_restir_nerf_mesh_amd import raster
    H, W = sc.H, sc.W
    c = _dev(color).view(1, H, W, -1).requires_grad_(want_color); p = _dev(sc.pos).requires_grad_(want_pos)
    out = raster.antialias(c, _dev(sc.rast).view(1, H, W, 4), p[None], _dev(sc.tri, torch.int32), topology_hash=_dev(sc.opp, torch.int32), pos_gradient_boost=boost)
    out.backward(_dev(gout).view(1, H, W, -1))
    return out.detach().view(H * W, -1), (c.grad.view(H * W, -1) if want_color else None), (p.grad if want_pos else None)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("key", KEYS, ids=R.scene_id)
def test_antialias_forward_and_adjoints(key, C):
    sc = R.get_scene(key)
    n = sc.H * sc.W
    color, gout = _aa_inputs(sc, C)
    ref_out, ref_gc, ref_gp, _ = _aa_reference(key, C, 1.0)
    out, gc, gp = _aa_run(sc, color, gout, 1.0)
    recv = R.aa_receivers(sc.recs, n)
    blends = [r for r in sc.recs if r.blend]

    # forward, per pixel: delta * sum |c_other - c_p| over the pairs the pixel receives from + 4 ulp; delta = 4 x the float32 restatement's weight noise
    delta = 4.0 * R.aa_alpha_noise(sc)
    c64 = color.astype(np.float64)
    spread = np.zeros((n, C))
    for p in range(n):
        for r, other in recv[p]:
            spread[p] += np.abs(c64[other] - c64[p])
    want = ref_out.numpy()
    bound = delta * spread + 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(out.double().cpu().numpy() - want)
    print("%s C=%d forward: largest error %.3g of its bound (delta %.2e)" % (sc.name, C, float((err / bound).max()), delta))
    bad = np.nonzero((err > bound).any(1))[0]
    assert len(bad) == 0, "forward: max error %.3e, bound there %.3e\n%s" % (float(err.max()), float(bound.ravel()[np.argmax(err)]), _by_category(
        sc, lambda r: (r.p1,) if r.alpha > 0 else (r.p0,), bad, "pixels"))
    quiet = np.array([not recv[p] for p in range(n)])
    assert quiet.any() or n < 20
    same_bits(out.cpu().numpy()[quiet], color[quiet], "pixels that receive nothing")
    out2, gc2, _ = _aa_run(sc, color, gout, 1.0)
    same_bits(out2.cpu().numpy(), out.cpu().numpy(), "two runs of the forward"); same_bits(gc2.cpu().numpy(), gc.cpu().numpy(), "two runs of the colour gradient")

    # colour gradient, per element
    _check(gc, ref_gc, "%s C=%d g_color" % (sc.name, C), lambda bad: _by_category(sc, lambda r: (r.p0, r.p1), np.nonzero(bad.any(1))[0], "pixels"))

    # position gradient, per element, boost 1 and 3; z never enters; vertices no blended edge names get exactly 0
    named = sorted({v for r in blends for v in (r.va, r.vb)})
    unnamed = [v for v in range(len(sc.pos)) if v not in named]
    for boost in (1.0, 3.0):
        if boost != 1.0:
            _, gc_b, gp = _aa_run(sc, color, gout, boost)
            same_bits(gc_b.cpu().numpy(), gc.cpu().numpy(), "pos_gradient_boost must not touch the colour gradient")
        ref = _aa_reference(key, C, boost)[2]
        _check(gp, ref, "%s C=%d g_pos (boost %g)" % (sc.name, C, boost), lambda bad: _by_category(sc, lambda r: (r.va, r.vb), np.nonzero(bad.any(1))[0], "vertices"))
        assert float(gp[:, 2].abs().max()) == 0.0
        if unnamed:
            assert float(gp[unnamed].abs().max()) == 0.0
    assert torch.allclose(_aa_reference(key, C, 3.0)[2], 3.0 * ref_gp, rtol=1e-14, atol=0)              # the reference's own boost is a plain factor

    # one gradient at a time: the colour gradient is a gather (bit-equal); the position gradient is scattered with atomics, so it is held to the float64
    # reference again, not to the other run
    _, gc_only, none = _aa_run(sc, color, gout, 1.0, want_pos=False)
    assert none is None
    same_bits(gc_only.cpu().numpy(), gc.cpu().numpy(), "colour-only call vs joint call")
    _, none, gp_only = _aa_run(sc, color, gout, 1.0, want_color=False)
    assert none is None
    _check(gp_only, ref_gp, "%s C=%d g_pos, pos-only call" % (sc.name, C), lambda bad: _by_category(sc, lambda r: (r.va, r.vb), np.nonzero(bad.any(1))[0], "vertices"))
    assert float(gp_only[:, 2].abs().max()) == 0.0


CATEGORIES = [(axis, s, sign) for axis in (0, 1) for s in (1, -1) for sign in ("alpha>0", "alpha<0")]


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] != "random" or (k[2], k[3]) in R.SIZES], ids=R.scene_id)
def test_antialias_position_gradient_per_category(key):
    """A vertex of these meshes belongs to edges of every kind, so an offending element of the full position gradient does not say which kind of pair is
    wrong.  The operator is linear in g_out and a pair's position gradient reads g_out at its receiving pixel only; so for each of the 8 categories
    (axis, s, sign of alpha) g_out is zeroed everywhere but on the pixels that receive from pairs of that category ALONE: only pairs of the category
    contribute, the result is held to float64 per element with its own scale (a small category is not hidden under the largest one's absolute term), and a
    failure names the category — a sign or factor error confined to one case fails exactly the runs of that case."""
    sc = R.get_scene(key)
    n = sc.H * sc.W
    color, gout = _aa_inputs(sc, 3)
    recv = R.aa_receivers(sc.recs, n)
    failures = []; ran = 0
    for cat in CATEGORIES:
        mask = np.array([bool(recv[p]) and all(r.category == cat for r, _ in recv[p]) for p in range(n)])
        pairs = [r for p in np.nonzero(mask)[0] for r, _ in recv[p]]
        if not pairs:
            continue
        assert key[0] != "random" or len(pairs) >= 3, (cat, len(pairs))
        g = gout * mask[:, None]
        pos = torch.tensor(sc.pos, requires_grad=True)
        out, _ = R.aa_torch(torch.tensor(color, dtype=torch.float64), pos, sc.recs, sc.H, sc.W)
        (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
        _, _, gp = _aa_run(sc, color, g.astype(np.float32), 1.0, want_color=False)
        ran += 1
        what = "%s g_pos of the %d pairs with axis %d, s %+d, %s (%s)" % (sc.name, len(pairs), cat[0], cat[1], cat[2], ", ".join(
            "%d %s vs %s" % (c, k[0], "triangle" if k[1] == "tri" else "background") for k, c in sorted(Counter((r.sil, r.versus) for r in pairs).items())))
        try:
            _check(gp, pos.grad, what)
        except AssertionError as e:
            failures.append(str(e))
    assert ran >= (8 if key[0] == "random" else 1)
    assert not failures, "%d of %d categories differ:\n%s" % (len(failures), ran, "\n".join(failures))


# ---------------------------------------------------------------------------------------------------------------------------------------- interpolate

V_USED, V_ALL, T = 36, 40, 60                     # vertices 36..39 belong to no triangle: their gradient must stay exactly 0


def _interp_case(n, C, one_triangle=False):
    rng = np.random.default_rng(1000 * n + C)
    tri = np.stack([rng.permutation(V_USED)[:3] for _ in range(T)]).astype(np.int32)
    ids = np.ones(n) if one_triangle else rng.integers(1, T + 1, n).astype(np.float64)
    if not one_triangle and n > 1:
        ids[rng.random(n) < 0.3] = 0.0                                     # background rows, each with a non-zero g_out
        ids[0] = 1.0 + (n % T)
    rast = np.stack([rng.uniform(-0.5, 1.5, n), rng.uniform(-0.5, 1.5, n), rng.uniform(-1, 1, n), ids], 1).astype(np.float32)
    attr = rng.standard_normal((V_ALL, C)).astype(np.float32)
    gout = rng.standard_normal((n, C)).astype(np.float32)
    gout[gout == 0] = 1.0
    rast_db = rng.uniform(-2, 2, (n, 4)).astype(np.float32)
    return tri, rast, attr, gout, rast_db


def _interp_reference(tri, rast, attr, gout):
    a = torch.tensor(attr, dtype=torch.float64, requires_grad=True); r = torch.tensor(rast, dtype=torch.float64, requires_grad=True)
    out = R.interpolate_torch(a, r, torch.from_numpy(tri))
    (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    return out.detach(), a.grad, r.grad


def _interp_checks(n, C, one_triangle):
    from mirres_restir_nerf_mesh_amd import raster
    from mirres_restir_nerf_mesh_amd._lib import lib, check, stream_ptr
    tri, rast, attr, gout, rast_db = _interp_case(n, C, one_triangle)
    ref_out, ref_ga, ref_gr = _interp_reference(tri, rast, attr, gout)
    what = "interpolate n=%d C=%d%s" % (n, C, " (one triangle)" if one_triangle else "")
    bg = rast[:, 3] == 0
    assert one_triangle or n == 1 or (bg.any() and not bg.all())
    assert rast[:, 3].min() >= 0 and rast[:, 3].max() <= T and tri.min() >= 0 and tri.max() < V_ALL
    a = _dev(attr).requires_grad_(True); r = _dev(rast).requires_grad_(True); t = _dev(tri, torch.int32); g = _dev(gout)
    out = raster.interpolate(a, r, t)
    out.backward(g)
    _check(out, ref_out, what + " forward")
    assert float(out.detach()[_dev(bg, torch.bool)].abs().sum()) == 0.0
    _check(a.grad, ref_ga, what + " g_attr")
    assert float(a.grad[V_USED:].abs().max()) == 0.0
    _check(r.grad[:, 0:2], ref_gr[:, 0:2], what + " g_uv")
    assert float(r.grad[:, 2:4].abs().max()) == 0.0 and float(ref_gr[:, 2:4].abs().max()) == 0.0
    assert float(r.grad[_dev(bg, torch.bool)].abs().sum()) == 0.0
    # one pointer at a time, straight through the library
    ac, rc = a.detach().contiguous(), r.detach().contiguous()
    ga = torch.zeros_like(ac)
    check(lib().mirres_interpolate_bwd(ac.data_ptr(), C, rc.data_ptr(), t.data_ptr(), n, g.data_ptr(), ga.data_ptr(), None, stream_ptr()), "mirres_interpolate_bwd")
    _check(ga, ref_ga, what + " g_attr alone")
    assert float(ga[V_USED:].abs().max()) == 0.0
    guv = torch.full((n, 2), float("nan"), device="cuda")
    check(lib().mirres_interpolate_bwd(ac.data_ptr(), C, rc.data_ptr(), t.data_ptr(), n, g.data_ptr(), None, guv.data_ptr(), stream_ptr()), "mirres_interpolate_bwd")
    same_bits(guv.cpu().numpy(), r.grad[:, 0:2].cpu().numpy(), what + " g_uv alone vs joint")
    # image-space derivatives of selected attributes
    if C >= 3:
        sel = [0, 2]
        o2, db = raster.dr_interpolate(a.detach()[None], r.detach().view(1, 1, n, 4), t, rast_db=_dev(rast_db).view(1, 1, n, 4), diff_attrs=sel)
        assert o2.shape == (1, 1, n, C) and db.shape == (1, 1, n, 2 * len(sel))
        same_bits(o2.view(n, C).cpu().numpy(), out.detach().cpu().numpy(), what + " dr_interpolate's value")
        ref_db = R.interpolate_db_torch(torch.tensor(attr, dtype=torch.float64), torch.tensor(rast, dtype=torch.float64), torch.from_numpy(tri),
                                        torch.tensor(rast_db, dtype=torch.float64), sel)
        _check(db.view(n, -1), ref_db, what + " out_db")
        assert float(db.view(n, -1)[_dev(bg, torch.bool)].abs().sum()) == 0.0


@pytest.mark.parametrize("C", [1, 3, 5, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_interpolate_forward_and_adjoints(n, C):
    _interp_checks(n, C, False)


def test_interpolate_adjoint_with_every_pixel_on_one_triangle():
    """4096 pixels, one triangle: every atomic of the attribute gradient lands on the same 3 C addresses."""
    _interp_checks(4096, 5, True)


# ---------------------------------------------------------------------------------------------------------------------------------------- texture

def _texture_coords(H, W, which):
    rng = np.random.default_rng(10 * H + W)
    if which == "one texel":                       # every tap within texels (x0, x0 + 1) x (y0, y0 + 1)
        x0, y0 = max(0, min(5, W - 2)), max(0, min(3, H - 2))
        return np.stack([(x0 + 0.5 + rng.uniform(0.1, 0.9, 1500)) / W, (y0 + 0.5 + rng.uniform(0.1, 0.9, 1500)) / H], 1).astype(np.float32)
    out_x = np.concatenate([rng.uniform(-0.5, -1e-3, 200), rng.uniform(1.001, 1.5, 200), [1e30, -1e30, 1e30, -1e30]])
    out_y = np.concatenate([rng.uniform(1.001, 1.5, 200), rng.uniform(-0.5, -1e-3, 200), [1e30, -1e30, -1e30, 1e30]])
    outside = np.stack([out_x, out_y], 1)
    if which == "outside":                         # both coordinates beyond the outermost texel centres: corner texels only
        return outside.astype(np.float32)
    gx, gy = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    centres = np.stack([gx.ravel(), gy.ravel()], 1)
    bx, by = np.meshgrid(np.arange(W + 1) / W, np.arange(H + 1) / H)
    borders = np.stack([bx.ravel(), by.ravel()], 1)
    corners = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    mixed = np.stack([np.concatenate([out_x, rng.random(len(out_x))]), np.concatenate([rng.random(len(out_y)), out_y])], 1)   # one coordinate inside, one outside
    inside = rng.random((2000, 2))
    return np.concatenate([centres, borders, corners, outside, mixed, inside]).astype(np.float32)


@pytest.mark.parametrize("which", ["all", "one texel", "outside"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 3), (7, 1, 3), (13, 21, 5)], ids=lambda s: "%dx%dx%d" % s)
def test_texture_forward_and_adjoint(shape, which):
    from mirres_restir_nerf_mesh_amd import raster
    H, W, C = shape
    uv = _texture_coords(H, W, which)
    rng = np.random.default_rng(H * 100 + W)
    tex = rng.random((H, W, C)).astype(np.float32) + 0.5
    gout = rng.standard_normal((len(uv), C)).astype(np.float32)
    t64 = torch.tensor(tex, dtype=torch.float64, requires_grad=True)
    ref = R.texture_torch(t64, torch.tensor(uv, dtype=torch.float64))
    (ref * torch.tensor(gout, dtype=torch.float64)).sum().backward()
    t = _dev(tex).requires_grad_(True)
    out = raster.texture(t, _dev(uv))
    out.backward(_dev(gout))
    what = "texture %dx%dx%d, %s (%d taps)" % (H, W, C, which, len(uv))
    _check(out, ref.detach(), what + " forward")
    _check(t.grad, t64.grad, what + " g_tex")
    touched = R.texture_touched(torch.from_numpy(uv), H, W)
    if which != "all" and H * W > 4:
        assert not touched.all()
    assert float(t.grad[~touched.cuda()].abs().sum()) == 0.0 and float(t64.grad[~touched].abs().sum()) == 0.0
