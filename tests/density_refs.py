"""Independent numpy restatements for the stage-0 density network (no import from the package): the hash-grid level layout of torch-ngp's GridEncoder
(gridencoder/grid.py:104-135, gridencoder/src/gridencoder.cu:66-84, 137-139), its forward in float32 with exactly the operation order DESIGN.md section 5.11 fixes
(every numpy float32 operation rounds once, there is no fused multiply-add), the same forward in float64, and the sigma head in float64 with the forward
error bound of an fp32 fmaf chain."""
import numpy as np

F32 = np.float32
U32 = np.uint32
P1, P2 = U32(2654435761), U32(805459861)


def layout(bound=1.0, num_levels=16, base=16, log2_T=19, desired=None):
    desired = 2048.0 * float(bound) if desired is None else float(desired)
    pls = np.exp2(np.log2(desired / base) / (num_levels - 1))
    S = F32(np.log2(pls))
    offsets, scale, res, hashed = [0], [], [], []
    for l in range(num_levels):
        r_py = int(np.ceil(base * pls ** l))
        params = min(2 ** log2_T, (r_py + 1) ** 3)
        params = int(np.ceil(params / 8) * 8)
        offsets.append(offsets[-1] + params)
        t = F32(l) * S
        e = F32(np.exp2(np.float64(t)))
        sc = F32(F32(e * F32(base)) - F32(1.0))
        r = int(np.ceil(sc)) + 1
        stride, d = 1, 0
        while d < 3 and stride <= params:
            stride *= r + 1; d += 1
        scale.append(sc); res.append(r); hashed.append(stride > params)
    return dict(num_levels=num_levels, offsets=np.array(offsets, np.int64), scale=np.array(scale, F32), resolution=np.array(res, np.int64),
                hashed=np.array(hashed, bool), total=offsets[-1])


def grid_index(L, l, x, y, z):
    """uint32 arrays -> entry inside level l (get_grid_index, gridencoder.cu:66-84)."""
    hs = U32(L["offsets"][l + 1] - L["offsets"][l]); s1 = U32(L["resolution"][l] + 1)
    with np.errstate(over="ignore"):
        if L["hashed"][l]:
            idx = x ^ (y * P1) ^ (z * P2)
        else:
            idx = x + y * s1 + z * U32(s1 * s1)
    return (idx % hs).astype(np.int64)


def in_bounds(u):
    with np.errstate(invalid="ignore"):
        return ((u >= 0) & (u <= 1)).all(axis=1)


def encode32(table, L, pos, bound):
    """pos f32 [n, 3], table f32 [entries, 2] -> f32 [n, 32], bit for bit what csrc/density.hip computes."""
    pos = np.asarray(pos, F32); table = np.asarray(table, F32)
    n = len(pos); b = F32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + b) / F32(F32(2.0) * b)
    ok = in_bounds(u)
    out = np.zeros((n, 32), F32)
    uu = u[ok]
    for l in range(L["num_levels"]):
        g = table[L["offsets"][l]: L["offsets"][l + 1]]
        p = uu * L["scale"][l]
        p = p + F32(0.5)
        cell = np.floor(p)
        f = p - cell
        o = F32(1.0) - f
        c = cell.astype(U32)
        r = np.zeros((len(uu), 2), F32)
        for idx in range(8):
            w = np.ones(len(uu), F32)
            cc = []
            for d in range(3):
                bit = (idx >> d) & 1
                w = w * (f[:, d] if bit else o[:, d])
                cc.append(c[:, d] + U32(bit))
            v = g[grid_index(L, l, *cc)]
            r[:, 0] = r[:, 0] + w * v[:, 0]
            r[:, 1] = r[:, 1] + w * v[:, 1]
        out[ok, 2 * l: 2 * l + 2] = r
    return out


def encode64(table, L, pos, bound):
    """The same interpolation in float64 from the same fp32 coordinates and scales."""
    pos = np.asarray(pos, F32).astype(np.float64); table = np.asarray(table).astype(np.float64)
    n = len(pos)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + float(bound)) / (2.0 * float(bound))
    ok = in_bounds(u)
    out = np.zeros((n, 32), np.float64)
    uu = u[ok]
    for l in range(L["num_levels"]):
        g = table[L["offsets"][l]: L["offsets"][l + 1]]
        p = uu * float(L["scale"][l]) + 0.5
        cell = np.floor(p)
        f = p - cell
        c = cell.astype(U32)
        r = np.zeros((len(uu), 2), np.float64)
        for idx in range(8):
            w = np.ones(len(uu)); cc = []
            for d in range(3):
                bit = (idx >> d) & 1
                w = w * (f[:, d] if bit else 1.0 - f[:, d])
                cc.append(c[:, d] + U32(bit))
            r += w[:, None] * g[grid_index(L, l, *cc)]
        out[ok, 2 * l: 2 * l + 2] = r
    return out


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def head64(feat, w0, w1row):
    """feat [n, 32] (any float type), w0 [64, 32], w1row [64] -> (h float64 [n], dh float64 [n]): h = w1row . relu(w0 . feat) in float64 and the bound on
    |h_fp32 - h| for an fp32 evaluation by one k-ascending fmaf chain per neuron (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a chain of n fused
    multiply-adds has forward error <= gamma_n * sum |a_k| |w_k|):
        layer 0: |d acc_o| <= gamma_32 * sum_k |a_k| |W0[o, k]|, and ReLU does not enlarge it;
        layer 1: |d h| <= sum_o |w1_o| |d acc_o| + gamma_64 * sum_o (|h1_o| + |d acc_o|) |w1_o|."""
    a = np.asarray(feat).astype(np.float64); w0 = np.asarray(w0).astype(np.float64); w1 = np.asarray(w1row).astype(np.float64)
    acc = a @ w0.T
    d0 = gamma(32) * (np.abs(a) @ np.abs(w0).T)
    h1 = np.maximum(acc, 0.0)
    h = h1 @ w1
    dh = d0 @ np.abs(w1) + gamma(64) * ((h1 + d0) @ np.abs(w1))
    return h, dh


def nearest_index(n_out, S):
    """F.interpolate(mode='nearest'): source index of every destination index, in float32 as ATen computes it."""
    sc = F32(S) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * sc).astype(np.int64), S - 1)
