"""Test infrastructure for prepare_shading_normal (csrc/normal.hip): a numpy float32 restatement of the BACKWARD in the operation order of
k_shading_normal_bwd (the forward's is oracle.prepare_shading_normal), the float64 torch formula both are held to, and the rows of the tests — benign ones and
the kinks of nerf/renderutils/c_src/normal.cu:40-44, 77-89 and vec3f.h:93-104.  Every fp32 operation below is one IEEE operation of the kernel (the build
contracts nothing), so kernel and restatement agree in every bit."""
import numpy as np

f = np.float32
THRESHOLD = f(0.1)
NAMES = ("pos", "view_pos", "perturbed_nrm", "smooth_nrm", "smooth_tng", "geom_nrm")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _len(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]


def _safe_normalize(v):
    l = _len(v)
    ok = l > 0
    return np.where(ok, v / np.where(ok, l, f(1)), f(0)).astype(f)


def _safe_normalize_bwd(v, g):
    """(g - n (n . g)) / |v| with n = v / |v|; 0 for a zero-length v."""
    l = _len(v)
    ok = l > 0
    ls = np.where(ok, l, f(1))
    n = v / ls
    return np.where(ok, (g - n * _dot(n, g)[..., None]) / ls, f(0)).astype(f)


def _fmax0(x):
    """fmaxf(x, 0.f) as the GPU evaluates it: +0 for -0 (its maximum orders -0 below +0) and for NaN."""
    return np.where(x > 0, x, f(0)).astype(f)


def backward32(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading, opengl, dout):
    """All inputs f32[..., 3] of one shape -> the six gradients in the order of NAMES, and `dp` (the bend's dot product, for the tests of the kinks)."""
    pos, view_pos, p, rn, rt, geom0, go = (np.ascontiguousarray(a, f) for a in (pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, dout))
    with np.errstate(all="ignore"):
        rv = view_pos - pos
        nrm, tng, view = _safe_normalize(rn), _safe_normalize(rt), _safe_normalize(rv)
        sgn = f(-1.0 if opengl else 1.0)
        px, py, pz = p[..., 0:1], p[..., 1:2], p[..., 2:3]
        rb = _cross(tng, nrm); bit = _safe_normalize(rb)
        rs = (tng * px + bit * (sgn * py)) + nrm * _fmax0(pz)
        sh0 = _safe_normalize(rs)
        flip = (_dot(view, geom0)[..., None] < 0) & bool(two_sided_shading)
        sh = np.where(flip, -sh0, sh0); geom = np.where(flip, -geom0, geom0)
        dp = _dot(view, sh)[..., None]
        t = np.fmin(_fmax0(dp / THRESHOLD), f(1))
        d_geom = go * (f(1) - t); d_sh = go * t
        d_t = _dot(go, sh - geom)[..., None]
        d_dp = np.where((dp < 0) | (dp > THRESHOLD), f(0), d_t / THRESHOLD)
        d_view = np.zeros_like(go) + sh * d_dp
        d_sh = d_sh + view * d_dp
        d_sh = np.where(flip, -d_sh, d_sh); d_geom = np.where(flip, -d_geom, d_geom)
        d_rs = _safe_normalize_bwd(rs, d_sh)
        pos_z = pz > 0
        d_tng = d_rs * px; d_bit = d_rs * (sgn * py); d_nrm = np.where(pos_z, d_rs * pz, f(0))
        d_p = np.stack([_dot(d_rs, tng), sgn * _dot(d_rs, bit), np.where(pos_z[..., 0], _dot(d_rs, nrm), f(0))], axis=-1)
        d_rb = _safe_normalize_bwd(rb, d_bit)
        d_tng = d_tng + _cross(nrm, d_rb); d_nrm = d_nrm + _cross(d_rb, tng)
        d_rv = _safe_normalize_bwd(rv, d_view)
        grads = (-d_rv, d_rv, d_p, _safe_normalize_bwd(rn, d_nrm), _safe_normalize_bwd(rt, d_tng), d_geom)
    return [np.ascontiguousarray(g, f) for g in grads], dp[..., 0].astype(f)


def formula64(pos, view, p, sn, st, gn, two_sided, opengl):
    """bsdf_prepare_shading_normal (ops.py:84-121) in torch, any dtype, for autograd in float64 (away from zero-length vectors)."""
    import torch
    nz = lambda v: v / v.norm(dim=-1, keepdim=True)
    nrm, tng, vv = nz(sn), nz(st), nz(view - pos)
    bit = nz(torch.cross(tng, nrm, dim=-1))
    sh = nz(tng * p[..., 0:1] + bit * ((-1.0 if opengl else 1.0) * p[..., 1:2]) + nrm * p[..., 2:3].clamp(min=0))
    flip = ((vv * gn).sum(-1, keepdim=True) < 0) & bool(two_sided)
    sh2, gn2 = torch.where(flip, -sh, sh), torch.where(flip, -gn, gn)
    t = ((vv * sh2).sum(-1, keepdim=True) / 0.1).clamp(0, 1)
    return gn2 * (1 - t) + sh2 * t


def gradients64(ins, two_sided, opengl, dout):
    """float64 autograd gradients of sum(dout * formula64(ins)) for fp32 inputs (any broadcastable shapes) -> list of float64 arrays in the inputs' own shapes."""
    import torch
    t = [torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in ins]
    (formula64(*t, two_sided, opengl) * torch.from_numpy(np.asarray(dout, np.float64))).sum().backward()
    return [a.grad.numpy() for a in t]


def benign_rows(n, seed=2):
    """n rows of N(0, 1) vectors, perturbed normals in the upper half space: no zero-length vector, no kink nearby (probability-wise)."""
    rng = np.random.default_rng(seed)
    ins = [rng.normal(size=(n, 3)).astype(f) for _ in range(6)]
    ins[2][:, 2] = np.abs(ins[2][:, 2]) + f(0.05)
    return ins


def _view_with_z(target):
    """A vector (a, b, 1) whose fp32 safe_normalize has z == target exactly (searched among the fp32 neighbours of (sqrt(99), 0, 1))."""
    a0 = f(np.sqrt(99.0))
    a = a0 + np.arange(-400, 401, dtype=np.float64) * float(np.spacing(a0))
    b = np.arange(0, 64, dtype=np.float64) * 1e-3
    A, Bg = np.meshgrid(a.astype(f), b.astype(f), indexing="ij")
    v = np.stack([A, Bg, np.ones_like(A)], axis=-1).astype(f)
    z = _safe_normalize(v)[..., 2]
    hit = np.argwhere(z == target)
    assert len(hit), "no fp32 vector normalises to z == %r" % target
    return v[hit[0][0], hit[0][1]]


KINKS = ("zero_nrm", "zero_tng", "zero_view", "parallel", "dp_zero", "dp_threshold", "dp_below_threshold", "dp_above_threshold", "dp_negative", "pz_zero",
         "pz_negative", "vg_zero", "vg_negative")


# what the conventions fix at each kink: (input, components) whose gradient is exactly zero / (input) whose gradient must be non-zero
KINK_ZERO = {"zero_nrm": [("smooth_nrm", (0, 1, 2))], "zero_tng": [("smooth_tng", (0, 1, 2))], "zero_view": [("pos", (0, 1, 2)), ("view_pos", (0, 1, 2))],
             "parallel": [("perturbed_nrm", (1,))], "dp_above_threshold": [("pos", (0, 1, 2)), ("view_pos", (0, 1, 2)), ("geom_nrm", (0, 1, 2))],
             "dp_negative": [(k, (0, 1, 2)) for k in ("pos", "view_pos", "perturbed_nrm", "smooth_nrm", "smooth_tng")],
             "pz_zero": [("perturbed_nrm", (2,))], "pz_negative": [("perturbed_nrm", (2,))]}
KINK_PASS = {"dp_zero": ["pos", "view_pos"], "dp_threshold": ["pos", "view_pos"], "dp_below_threshold": ["pos", "view_pos"], "pz_zero": ["smooth_tng"], "pz_negative": ["smooth_tng"]}


def check_kink_conventions(grads, where, who):
    """grads: six [n,3] arrays in the order of NAMES; where: {kind: row} of mixed_rows."""
    g = dict(zip(NAMES, grads))
    for kind, i in where.items():
        for name, comps in KINK_ZERO.get(kind, []):
            assert not g[name][i][list(comps)].any(), "%s: %s row, gradient of %s%r should be exactly zero, is %r" % (who, kind, name, comps, g[name][i])
        for name in KINK_PASS.get(kind, []):
            assert g[name][i].any() and np.isfinite(g[name][i]).all(), "%s: %s row, gradient of %s should pass, is %r" % (who, kind, name, g[name][i])


def kink_row(kind):
    """One row (six f32[3]) on a kink.  The frame of the dp rows: smooth normal +z, tangent +x, perturbed normal (0, 0, 1), so that the shading normal is exactly
    (0, 0, 1) and dp = the z of the normalised view vector; geom_nrm has a positive dot product with the view (no flip) and differs from the shading normal
    (so d_t != 0 and the clamp's convention shows in the view / position gradients)."""
    r = dict(pos=[0, 0, 0], view_pos=[1.0, 2.0, 3.0], perturbed_nrm=[0.2, -0.3, 0.9], smooth_nrm=[0.1, 0.2, 1.0], smooth_tng=[1.0, 0.1, -0.1], geom_nrm=[0.3, 0.1, 0.8])
    frame = dict(perturbed_nrm=[0, 0, 1.0], smooth_nrm=[0, 0, 2.0], smooth_tng=[3.0, 0, 0], geom_nrm=[0.6, 0.8, 0.5])
    one = f(1)
    if kind == "zero_nrm": r["smooth_nrm"] = [0, 0, 0]
    elif kind == "zero_tng": r["smooth_tng"] = [0, 0, 0]
    elif kind == "zero_view": r["pos"] = r["view_pos"]
    elif kind == "parallel": r["smooth_tng"] = [0.2, 0.4, 2.0]            # 2 x smooth_nrm: the same unit vector in every bit, cross product exactly 0
    elif kind == "dp_zero": r.update(frame); r["view_pos"] = [3.0, 4.0, 0.0]
    elif kind == "dp_threshold": r.update(frame); r["view_pos"] = _view_with_z(THRESHOLD)
    elif kind == "dp_below_threshold": r.update(frame); r["view_pos"] = _view_with_z(np.nextafter(THRESHOLD, f(0)))
    elif kind == "dp_above_threshold": r.update(frame); r["view_pos"] = _view_with_z(np.nextafter(THRESHOLD, one))
    elif kind == "dp_negative": r.update(frame); r["view_pos"] = [3.0, 4.0, -1.0]; r["geom_nrm"] = [0.6, 0.8, -0.1]
    elif kind == "pz_zero": r["perturbed_nrm"] = [0.2, -0.3, 0.0]; r["view_pos"] = [3.0, 1.0, 1.0]          # a view along the tangent, so that dp > 0
    elif kind == "pz_negative": r["perturbed_nrm"] = [0.2, -0.3, -0.4]; r["view_pos"] = [3.0, 1.0, 1.0]
    elif kind == "vg_zero": r.update(frame); r["view_pos"] = [1.0, 1.0, 0.3]; r["geom_nrm"] = [-0.7, 0.7, 0.0]     # view.x == view.y in every bit: -0.7 x + 0.7 x == 0
    elif kind == "vg_negative": r["geom_nrm"] = [-0.3, -0.1, -0.8]
    else: raise ValueError(kind)
    return [np.asarray(r[k], f) for k in ("pos", "view_pos", "perturbed_nrm", "smooth_nrm", "smooth_tng", "geom_nrm")]


def mixed_rows(n, seed=2):
    """benign_rows with the kink rows written over rows spread evenly (the last row included) as far as n allows -> (six f32[n,3], {kind: row index})."""
    ins = benign_rows(n, seed)
    where = {}
    if n >= len(KINKS):
        idx = np.unique(np.linspace(0, n - 1, len(KINKS)).astype(int))
        for kind, i in zip(KINKS, idx):
            for a, v in zip(ins, kink_row(kind)):
                a[i] = v
            where[kind] = int(i)
    return ins, where


WRAPPER_SHAPE = (2, 13, 17, 3)
WRAPPER_ATOL_SCALE = 1e-7          # util.elementwise's absolute term: about two fp32 ulp of the largest gradient element (sums that cancel have no relative accuracy)
WRAPPER_RTOL_MEASURED = 6.2e-6     # measured on the CPU (tests/test_normal_refs.py): wrapper_gradients32 against float64 autograd, the largest over the four flag pairs
WRAPPER_RTOL = 4 * WRAPPER_RTOL_MEASURED      # what the GPU is held to: a factor 4 for the different order of the 442-row sums


def wrapper_inputs(seed=11):
    """The autograd wrapper's case: full-size pos, perturbed_nrm, smooth_nrm, smooth_tng of WRAPPER_SHAPE, view_pos and geom_nrm of shape [1, 1, 1, 3] (their
    gradients are the sums over all 442 rows) -> (six arrays, dout)."""
    rng = np.random.default_rng(seed)
    mk = lambda: rng.normal(size=WRAPPER_SHAPE).astype(f)
    pos, pn, sn, st = mk(), mk(), mk(), mk()
    pos *= f(0.3)
    pn[..., 2] = np.abs(pn[..., 2]) + f(0.05)
    view = np.array([0.5, -2.0, 3.0], f).reshape(1, 1, 1, 3)
    gn = np.array([0.2, -0.5, 0.8], f).reshape(1, 1, 1, 3)
    return [pos, view, pn, sn, st, gn], mk()


def wrapper_gradients32(ins, two_sided, opengl, dout):
    """backward32 on the broadcast inputs, the broadcast ones summed back to their own shape in float32 (numpy's pairwise order)."""
    full = [np.ascontiguousarray(np.broadcast_to(a, WRAPPER_SHAPE)) for a in ins]
    g, _ = backward32(*full, two_sided, opengl, dout)
    return [x if a.shape == WRAPPER_SHAPE else x.reshape(-1, 3).sum(axis=0, dtype=f).reshape(a.shape) for x, a in zip(g, ins)]


def elementwise_rtol(got, want, atol_scale=WRAPPER_ATOL_SCALE):
    """The smallest rtol with which util.elementwise(got, want, rtol, atol_scale) passes."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    slack = np.abs(got - want) - atol_scale * float(np.abs(want).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(slack <= 0, 0.0, slack / np.abs(want))
    return float(r.max())
