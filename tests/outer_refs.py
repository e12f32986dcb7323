"""numpy restatements for the outer-cascade tests (csrc/mcubes.hip: mirres_mc_occupancy_trilinear, mirres_mesh_select_box; stage0.outer_shell): torch's
upsample_trilinear3d (align_corners=False) with one fp32 rounding per operation, its fp64 value with the rounding bound, remove_selected_verts' two box
predicates, and the chain of one outer cascade up to cleaning."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage0_refs as R      # noqa: E402

F = np.float32
SHAPES = [(4, 4), (4, 9), (8, 20), (16, 12), (16, 33), (16, 32)]        # (S, R): R == S, non-integer ratios up and down, an integer ratio
EPS = 2.0 ** -24                                                         # half an ulp of 1: the relative error of one fp32 rounding
OUTER_CENTRE = 0.45


def axis_weights(S, Rr):
    """(i0, i1, l0, l1) of one axis: src = max(scale * (d + 0.5) - 0.5, 0), scale = (float)S / R, every step one fp32 operation."""
    scale = F(S) / F(Rr)
    d = np.arange(Rr).astype(F)
    src = np.maximum(scale * (d + F(0.5)) - F(0.5), F(0))
    assert src.dtype == np.float32
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = src - i0.astype(F)
    l0 = F(1) - l1
    return i0, i1, l0.astype(F), l1.astype(F)


def _corners(vol, Rr):
    vol = np.asarray(vol, F)
    S = vol.shape[0]
    assert vol.shape == (S, S, S)
    i0, i1, l0, l1 = axis_weights(S, Rr)
    lx = (l0[:, None, None], l1[:, None, None]); ly = (l0[None, :, None], l1[None, :, None]); lz = (l0[None, None, :], l1[None, None, :])
    ix = (i0, i1)
    g = {(a, b, c): vol[np.ix_(ix[a], ix[b], ix[c])] for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    return g, lx, ly, lz


def trilinear_fp32(vol, Rr):
    """F.interpolate(vol[None, None], [R] * 3, mode='trilinear')[0, 0] in fp32: w inside h inside t, every product and every sum rounded once, zero weights
    multiplied (a non-finite neighbour makes the value NaN)."""
    g, lx, ly, lz = _corners(vol, Rr)
    with np.errstate(all="ignore"):
        a = {(i, j): lz[0] * g[(i, j, 0)] + lz[1] * g[(i, j, 1)] for i in (0, 1) for j in (0, 1)}
        b = {i: ly[0] * a[(i, 0)] + ly[1] * a[(i, 1)] for i in (0, 1)}
        v = lx[0] * b[0] + lx[1] * b[1]
    assert v.dtype == np.float32
    return v


def trilinear_fp64(vol, Rr):
    """(value, bound): the same sum with the same fp32 weights, products and sums in fp64, and 8 * 2^-24 * sum |w_i v_i| — every term passes through at most three
    nested products and four sums on its way to the result, at most seven roundings of relative size 2^-24 each (first order), rounded up to 8."""
    g, lx, ly, lz = _corners(vol, Rr)
    D = np.float64
    val = np.zeros((Rr, Rr, Rr), D); mag = np.zeros((Rr, Rr, Rr), D)
    with np.errstate(all="ignore"):
        for (a, b, c), gv in g.items():
            w = lx[a].astype(D) * ly[b].astype(D) * lz[c].astype(D)
            val = val + w * gv.astype(D); mag = mag + np.abs(w * gv.astype(D))
    return val, 8.0 * EPS * mag


def occupancy(vol, Rr, thresh):
    """(occ f32 of 0 / 1, value): renderer.py:653-655 on the fp32 restatement; nan_to_num(., 0) then > thresh."""
    v = trilinear_fp32(vol, Rr)
    c = np.nan_to_num(v, nan=0.0, posinf=R.FLT_MAX, neginf=-R.FLT_MAX).astype(F)
    return (c > F(thresh)).astype(F), v


def same_values(got, want):
    """Bit-equal where the value is a number; NaN where the restatement has NaN (the payload and sign of a NaN an invalid operation produces differ between
    processors and carry no meaning)."""
    got = np.asarray(got, F); want = np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def lognormal_grid(S, seed):
    return np.random.default_rng(seed).lognormal(mean=1.0, sigma=1.5, size=(S, S, S)).astype(F)


def thresh_between(vol, k=None):
    """A fp32 threshold strictly between two adjacent values of the grid (around the median by default)."""
    u = np.unique(np.asarray(vol, F)[np.isfinite(vol)])
    k = len(u) // 2 if k is None else k
    for j in list(range(k, len(u) - 1)) + list(range(k - 1, -1, -1)):
        t = F((np.float64(u[j]) + np.float64(u[j + 1])) / 2)
        if u[j] < t < u[j + 1]:
            return float(t)
    raise AssertionError("no fp32 number between two adjacent grid values")


def hostile_grid():
    """4^3: a NaN corner, +inf and -inf inside, untrained -1 cells, the rest log-normal."""
    vol = lognormal_grid(4, 77)
    vol[0, 0, 0] = np.nan; vol[2, 1, 3] = np.inf; vol[3, 3, 0] = -np.inf
    vol[1, 2, :] = -1.0; vol[3, 0, 2] = -1.0
    return vol


# ------------------------------------------------------------------------------------------------ box selection
def select_box(verts, box, outside):
    """bool [V]: remove_selected_verts' condition, coordinates compared as doubles.  box = (xmn, ymn, zmn, xmx, ymx, zmx)."""
    v = np.asarray(verts, F).reshape(-1, 3).astype(np.float64)
    lo = np.asarray(box, np.float64)[:3]; hi = np.asarray(box, np.float64)[3:]
    if outside:
        return ((v <= lo) | (v >= hi)).any(axis=1)
    return ((v <= hi) & (v >= lo)).all(axis=1)


def remove_selected(verts, tris, box, outside):
    """A face goes when it touches a selected vertex; the vertices no face uses go with it; order kept."""
    verts = np.asarray(verts, F).reshape(-1, 3); tris = np.asarray(tris, np.int32).reshape(-1, 3)
    sel = select_box(verts, box, outside)
    keep = ~sel[tris.astype(np.int64)].any(axis=1) if len(tris) else np.zeros(0, bool)
    return R.compact(verts, tris, keep)


# ------------------------------------------------------------------------------------------------ one outer cascade
def outer_boxes(cas, bound, env_reso, aabb):
    bound_cas = min(2.0 ** cas, float(bound)); half = bound_cas / env_reso
    a = [float(x) for x in np.asarray(aabb, np.float64)]
    r = OUTER_CENTRE
    return (-r, -r, -r, r, r, r), bound_cas - half, [a[0] + half, a[1] + half, a[2] + half, a[3] - half, a[4] - half, a[5] - half]


def outer_shell(grid_row, S, cas, bound, env_reso, thresh, aabb):
    """nerf/renderer.py:642-676 in numpy -> (vertices f32, triangles i32, the mesh before the first removal)."""
    vol = R.unpack_morton(grid_row, S)
    occ, _ = occupancy(vol, env_reso, thresh)
    v, t = R.marching_cubes(occ, 0.5)
    v = (v / F(env_reso - 1) * F(2) - F(1)).astype(F)
    raw = (v, t)
    centre, factor, shrunk = outer_boxes(cas, bound, env_reso, aabb)
    v, t = remove_selected(v, t, centre, False)
    if len(v) == 0:
        return v, t, raw
    v = (v * F(factor)).astype(F)
    v, t = remove_selected(v, t, shrunk, True)
    return v, t, raw
