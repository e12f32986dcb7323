"""Independent numpy restatements for the stand-alone grid encoder (csrc/gridenc.hip, encoding.GridEncoder); no import from the package.  torch-ngp's GridEncoder
(gridencoder/grid.py:104-135, gridencoder/src/gridencoder.cu:66-84, 87-244, 247-339) for input_dim D in {2, 3}, level_dim C, gridtype hash / tiled, align_corners,
linear / smoothstep, max_level:

    layout()        the level table and the kernels' per-level quantities;
    encode32()      the forward in float32 with exactly the operation order DESIGN.md section 5.18 fixes (every numpy float32 operation rounds once, no FMA);
    encode64()      the same interpolant in float64 from the same fp32 coordinates, in the cell the fp32 forward picks;
    input_grad32()  the input gradient in float32 in the fixed order (levels, axes, pairs, channels ascending);
    grads64()       the analytic gradients in float64 — the table's as a scatter, the input's as the derivative of the picked cell's polynomial — with, per
                    element, the sum of the absolute values of its terms and their number, for the Higham bounds below.

WHAT THE FLOAT64 GRADIENTS START FROM.  The fixed arithmetic defines, per point, level and axis, the cell, the interpolation factor s (f, or smoothstep's
(f f)(3 - 2 f)) and its derivative ds in float32; the forward tests hold those to the bit (they decide every feature).  The gradients are polynomials in s, ds, the
table and the cotangent; grads64() evaluates those polynomials in float64 FROM THE FLOAT32 s AND ds.  (From f instead, 1 - s would carry smoothstep's three roundings
as an absolute error, which no bound relative to the term covers when s is near 1.)

THE BOUNDS (Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1 and 4.2: k roundings on a term give a relative error <= gamma_k, and a sum of m
terms in ANY order adds m - 1), gamma_k = k u / (1 - k u), u = 2^-24:
    table entry e, channel ch:  a term is w * grad, w = 1 * (s or 1 - s) per axis: 1 - s rounds once, the D products at most D times, w * grad once, then the m terms
        into (e, ch) are summed by atomics in some order:  |g - g64| <= gamma_(m + D + 2) * sum |terms|              (table_k(m, D) = m + D + 2);
    input gradient, axis a:  a term is grad * (scale * prod (s or 1 - s) * (right - left) * ds) / (2 bound): 1 - s, right - left, D - 1 products for w, w * diff,
        * ds, the 2^(D-1) pair additions, grad * r, the L C additions into g[a], the division, and 2 * bound is exact:
        |g - g64| <= gamma_(D + 2^(D-1) + L C + 5) * sum |terms|                                                     (pos_k(D, L, C)).
Nothing here depends on what the code under test gives."""
import numpy as np

F32 = np.float32
U32 = np.uint32
U = 2.0 ** -24
PRIMES = (1, 2654435761, 805459861)


def gamma(k):
    return k * U / (1.0 - k * U)


def table_k(m, D):
    return m + D + 2


def pos_k(D, L, C):
    return D + 2 ** (D - 1) + L * C + 5


def per_level_scale(desired, base, num_levels):
    """grid.py:107-108."""
    return np.exp2(np.log2(desired / base) / (num_levels - 1))


def layout(D=3, C=2, num_levels=16, pls=2.0, base=16, log2_T=19, gridtype="hash", align=False, interp="linear"):
    pls = np.float64(pls)
    S = F32(np.log2(pls))
    offsets, scale, res, hashed, strides = [0], [], [], [], []
    for l in range(num_levels):
        r_py = int(np.ceil(base * pls ** l))
        params = min(2 ** log2_T, (r_py if align else r_py + 1) ** D)
        params = int(np.ceil(params / 8) * 8)
        offsets.append(offsets[-1] + params)
        t = F32(l) * S
        e = F32(np.exp2(np.float64(t)))
        sc = F32(F32(e * F32(base)) - F32(1.0))
        r = int(np.ceil(sc)) + 1
        factor = r if align else r + 1
        stride, st = 1, [0] * D
        for d in range(D):                                          # get_grid_index's loop, uint32
            if stride > params:
                break
            st[d] = stride
            stride = (stride * factor) & 0xFFFFFFFF
        scale.append(sc); res.append(r); strides.append(st)
        hashed.append(gridtype == "hash" and stride > params)
    return dict(D=D, C=C, num_levels=num_levels, offsets=np.array(offsets, np.int64), scale=np.array(scale, F32), resolution=np.array(res, np.int64),
                hashed=np.array(hashed, bool), strides=strides, total=offsets[-1], align=bool(align), smooth=(interp == "smoothstep"), gridtype=gridtype)


def grid_index(L, l, cc):
    """cc: D uint32 arrays -> entry inside level l (get_grid_index, gridencoder.cu:66-84)."""
    hs = U32(L["offsets"][l + 1] - L["offsets"][l])
    with np.errstate(over="ignore"):
        if L["hashed"][l]:
            idx = cc[0] * U32(PRIMES[0])
            for d in range(1, L["D"]):
                idx = idx ^ (cc[d] * U32(PRIMES[d]))
        else:
            idx = cc[0] * U32(L["strides"][l][0])
            for d in range(1, L["D"]):
                idx = idx + cc[d] * U32(L["strides"][l][d])
    return (idx % hs).astype(np.int64)


def unit32(L, pos, bound):
    pos = np.asarray(pos, F32).reshape(-1, L["D"])
    b = F32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + b) / F32(F32(2.0) * b)
        ok = ((u >= 0) & (u <= 1)).all(axis=1)
    return u, ok


def levels_run(L, max_level):
    return L["num_levels"] if max_level is None else max(0, min(int(max_level), L["num_levels"]))


def cells32(L, l, uu):
    """The fixed float32 arithmetic of one level: uu f32 [m, D] in [0, 1] -> cell u32 [m, D], f, s, o, ds f32 [m, D], idx i64 [m, 2^D] (entries in the whole table)."""
    D = L["D"]
    p = uu * L["scale"][l]
    p = p + (F32(0.0) if L["align"] else F32(0.5))
    cell = np.floor(p)
    f = p - cell
    if L["smooth"]:
        s = (f * f) * (F32(3.0) - F32(2.0) * f)
        ds = (F32(6.0) * f) * (F32(1.0) - f)
    else:
        s = f
        ds = np.ones_like(f)
    o = F32(1.0) - s
    c = cell.astype(U32)
    idx = np.zeros((len(uu), 1 << D), np.int64)
    for k in range(1 << D):
        idx[:, k] = grid_index(L, l, [c[:, d] + U32((k >> d) & 1) for d in range(D)]) + int(L["offsets"][l])
    return cell, f, s, o, ds, idx


def weights(s, o, dtype):
    """w [m, 2^D]: w = 1; for d ascending w = w * (bit d ? s[d] : o[d])."""
    m, D = s.shape
    w = np.ones((m, 1 << D), dtype)
    for k in range(1 << D):
        for d in range(D):
            w[:, k] = w[:, k] * (s[:, d] if (k >> d) & 1 else o[:, d])
    return w


def encode32(table, L, pos, bound, max_level=None):
    """pos f32 [n, D], table f32 [entries, C] -> f32 [n, L * C], bit for bit what csrc/gridenc.hip computes."""
    table = np.asarray(table, F32)
    C = L["C"]
    u, ok = unit32(L, pos, bound)
    out = np.zeros((len(u), L["num_levels"] * C), F32)
    uu = u[ok]
    for l in range(levels_run(L, max_level)):
        _, _, s, o, _, idx = cells32(L, l, uu)
        w = weights(s, o, F32)
        r = np.zeros((len(uu), C), F32)
        for k in range(idx.shape[1]):
            v = table[idx[:, k]]
            for ch in range(C):
                r[:, ch] = r[:, ch] + w[:, k] * v[:, ch]
        out[ok, l * C: (l + 1) * C] = r
    return out


def encode64(table, L, pos, bound, max_level=None):
    """The same interpolant in float64: u, p and f in float64 from the fp32 coordinates, in the cell (and for the points) the fp32 arithmetic picks."""
    table = np.asarray(table).astype(np.float64)
    C, D = L["C"], L["D"]
    u32_, ok = unit32(L, pos, bound)
    pos = np.asarray(pos, F32).reshape(-1, D).astype(np.float64)
    out = np.zeros((len(pos), L["num_levels"] * C), np.float64)
    uu = ((pos + float(bound)) / (2.0 * float(bound)))[ok]
    for l in range(levels_run(L, max_level)):
        cell, _, _, _, _, idx = cells32(L, l, u32_[ok])
        f = uu * float(L["scale"][l]) + (0.0 if L["align"] else 0.5) - cell.astype(np.float64)
        s = f * f * (3.0 - 2.0 * f) if L["smooth"] else f
        w = weights(s, 1.0 - s, np.float64)
        out[ok, l * C: (l + 1) * C] = (w[:, :, None] * table[idx]).sum(axis=1)
    return out


def encode_tolerance(L, l, M):
    """What encode32 and encode64 may differ by on level l, M the largest |entry|.  (1) the interpolation point: u = (x + b) / (2 b) rounds twice, u * scale once,
    + 0.5 once, all on non-negative values, so p moves by at most gamma_4 * (scale + 0.5) cells, and f = p - cell is exact; (2) the interpolant is multilinear in s
    with |d r / d s_d| <= 2 M (a difference of two convex combinations) and |d s / d f| <= 1.5 (smoothstep; 1 linear): D axes; (3) its own arithmetic: a factor s
    or 1 - s is within gamma_4 absolutely (three roundings for smoothstep's s, one for 1 - s), so a weight, a product of D factors in [0, 1] with D more
    roundings, within D * (gamma_4 + u) <= D * gamma_6 absolutely; w * v and the 2^D additions: gamma_(2^D + 1) relative to sum w |v| <= M."""
    D = L["D"]
    lip = 3.0 if L["smooth"] else 2.0
    return M * (D * lip * gamma(4) * (float(L["scale"][l]) + 0.5) + (1 << D) * D * gamma(6) + gamma((1 << D) + 1))


def pairs(D, a):
    """The corner pairs that differ in axis a alone, ascending: [(left, right, [(other axis, bit), ...])]."""
    out = []
    for pr in range(1 << (D - 1)):
        left, sel = 0, []
        for nd in range(D - 1):
            d = nd + 1 if nd >= a else nd
            bit = (pr >> nd) & 1
            left |= bit << d
            sel.append((d, bit))
        out.append((left, left | (1 << a), sel))
    return out


def input_grad32(table, L, pos, bound, grad_out, max_level=None):
    """grad_out f32 [n, L * C] -> grad_pos f32 [n, D] in the fixed order of mirres_grid_encode_bwd."""
    table = np.asarray(table, F32); grad_out = np.asarray(grad_out, F32)
    C, D = L["C"], L["D"]
    u, ok = unit32(L, pos, bound)
    uu = u[ok]; go = grad_out.reshape(len(u), -1)[ok]
    g = np.zeros((len(uu), D), F32)
    for l in range(levels_run(L, max_level)):
        _, _, s, o, ds, idx = cells32(L, l, uu)
        v = table[idx]                                              # [m, 2^D, C]
        for a in range(D):
            r = np.zeros((len(uu), C), F32)
            for left, right, sel in pairs(D, a):
                w = np.full(len(uu), L["scale"][l], F32)
                for d, bit in sel:
                    w = w * (s[:, d] if bit else o[:, d])
                for ch in range(C):
                    r[:, ch] = r[:, ch] + (w * (v[:, right, ch] - v[:, left, ch])) * ds[:, a]
            for ch in range(C):
                g[:, a] = g[:, a] + go[:, l * C + ch] * r[:, ch]
    out = np.zeros((len(u), D), F32)
    out[ok] = g / F32(F32(2.0) * F32(bound))
    return out


def grads64(table, L, pos, bound, grad_out, max_level=None):
    """-> dict(table=(g64 [entries, C], sum |terms| [entries, C], m [entries, C]), pos=(g64 [n, D], sum |terms| [n, D])), from the float32 s and ds (module docstring)."""
    t64 = np.asarray(table).astype(np.float64)
    C, D = L["C"], L["D"]
    u, ok = unit32(L, pos, bound)
    uu = u[ok]; go = np.asarray(grad_out).astype(np.float64).reshape(len(u), -1)[ok]
    gt = np.zeros_like(t64); tsum = np.zeros_like(t64); tcnt = np.zeros(t64.shape, np.int64)
    gp = np.zeros((len(uu), D)); psum = np.zeros((len(uu), D))
    den = 2.0 * float(bound)
    for l in range(levels_run(L, max_level)):
        _, _, s, o_unused, ds, idx = cells32(L, l, uu)
        s = s.astype(np.float64); ds = ds.astype(np.float64); o = 1.0 - s
        w = weights(s, o, np.float64)
        for ch in range(C):
            term = w * go[:, l * C + ch][:, None]
            np.add.at(gt[:, ch], idx, term)
            np.add.at(tsum[:, ch], idx, np.abs(term))
            np.add.at(tcnt[:, ch], idx, 1)
        v = t64[idx]
        sc = float(L["scale"][l])
        for a in range(D):
            for left, right, sel in pairs(D, a):
                wp = np.full(len(uu), sc)
                for d, bit in sel:
                    wp = wp * (s[:, d] if bit else o[:, d])
                for ch in range(C):
                    term = go[:, l * C + ch] * (wp * (v[:, right, ch] - v[:, left, ch]) * ds[:, a]) / den
                    gp[:, a] += term
                    psum[:, a] += np.abs(term)
    gpos = np.zeros((len(u), D)); gpsum = np.zeros((len(u), D))
    gpos[ok] = gp; gpsum[ok] = psum
    return dict(ok=ok, table=(gt, tsum, tcnt), pos=(gpos, gpsum))
