"""Independent restatement of the stage-0 radiance network with the POSITION as a differentiable leaf, on the host (no import from the package), for the tests of
mirres_radiance_points_bwd_pos: radiance_bwd_refs.network with the trilinear weights built in torch from the position, u = (pos + bound) / (2 bound),
f = u * scale + 0.5 - cell, w = prod (f or 1 - f), so that autograd carries the cotangent through the encoder as the reference's dy_dx does
(gridencoder/src/gridencoder.cu:198-243) and through 1 / (2 bound) (gridencoder/grid.py:156).

THE CELL AND THE IN-BOUNDS DECISION ARE THE fp32 RULE'S FOR BOTH PRECISIONS (radiance_bwd_refs.corners decides the points in bounds the same way): cell =
floor(fp32(fp32(u32 * scale) + 0.5)).  The float64 truth at a point on a cell face is then the one-sided derivative of the cell the product picks (its f is 0 or 1
up to rounding, outside [0, 1) by a hair in float64: the trilinear form is a polynomial and extends), not that of a neighbouring cell the float64 floor might pick.
A point out of bounds has constant features: its gradient is exactly 0.

THE CRITERION is radiance_bwd_refs.criterion on the one tensor grad_pos [n, 3] (name "pos"): |g - g64| / max |g64| <= max(2 E_ref, floor[e]).  Element (i, a) is
   (1 / (2 bound)) * sum over levels l, channels ch, pairs p of  d_feat[i, 2 l + ch] * (scale_l * w_other[i, l, a, p]) * (table[right] - table[left])[ch]:
m = levels * 2 * 4 products (128 for 16 levels) for a point in bounds, 0 otherwise; a pair's difference is one term (its subtraction rounds relative to the
difference itself).  floor[e] = gamma_(m+1) * sum |terms| / max |g64| with the terms from the float64 network (abs_terms_pos).  Counting the eight corners apart
would double m and enlarge the sum: the pairs are the stricter reading.  Nothing here depends on what the code under test gives."""
import numpy as np
import torch

import density_refs as D
import radiance_bwd_refs as B
import radiance_refs as RR

PAIRS = {0: (1, 2), 1: (0, 2), 2: (0, 1)}                     # axis -> the two other axes, ascending


def cells(L, pos, bound):
    """-> ok bool [n], cell f32 [n, levels, 3] (0 for a point out of bounds): the fp32 rule (density_refs.encode32's arithmetic)."""
    pos = np.asarray(pos, np.float32)
    b = np.float32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + b) / np.float32(np.float32(2.0) * b)
    ok = D.in_bounds(u)
    cell = np.zeros((len(pos), L["num_levels"], 3), np.float32)
    for l in range(L["num_levels"]):
        p = u[ok] * np.float32(L["scale"][l])
        p = p + np.float32(0.5)
        cell[ok, l] = np.floor(p)
    return ok, cell


def network(params, L, pos, dirs, bound, dtype=torch.float64):
    """radiance_bwd_refs.network's dict plus `x` (the position leaf, [n, 3], requires_grad), `f` [n, levels, 3] and `cell`; the corner entries are idx [n, levels, 8]
    (corner k: bit d of k is axis d's offset, as in the forward)."""
    ok, cell = cells(L, pos, bound)
    n, nl = len(cell), L["num_levels"]
    idx = np.zeros((n, nl, 8), np.int64)
    c = cell.astype(np.uint32)
    for l in range(nl):
        for k in range(8):
            cc = [c[ok, l, d] + np.uint32((k >> d) & 1) for d in range(3)]
            idx[ok, l, k] = D.grid_index(L, l, *cc) + int(L["offsets"][l])
    p = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in params]
    table, w0, w1, c0, c1, c2 = p
    x = torch.tensor(np.nan_to_num(np.asarray(pos, np.float32), nan=0.0, posinf=0.0, neginf=0.0), dtype=dtype, requires_grad=True)
    okt = torch.from_numpy(ok)
    u = (x + dtype_of(dtype, bound)) / dtype_of(dtype, 2.0 * float(bound))
    scale = torch.tensor(np.asarray(L["scale"], np.float32), dtype=dtype)
    f = u[:, None, :] * scale[None, :, None] + 0.5 - torch.from_numpy(cell).to(dtype)                  # [n, levels, 3]
    o = 1.0 - f
    ws = []
    for k in range(8):
        w = torch.ones((n, nl), dtype=dtype)
        for d in range(3):
            w = w * (f[:, :, d] if (k >> d) & 1 else o[:, :, d])
        ws.append(w)
    w = torch.stack(ws, dim=2) * okt[:, None, None].to(dtype)                                           # a point out of bounds: zero features, constant
    g = table[torch.from_numpy(idx.reshape(-1))].reshape(n, nl, 8, 2)
    feat = (w[..., None] * g).sum(dim=2).reshape(n, 2 * nl)
    sh = torch.tensor(RR.sh64(dirs) if dtype == torch.float64 else RR.sh32(dirs), dtype=dtype)
    z1 = feat @ w0.T
    h16 = torch.relu(z1) @ w1.T
    sigma = B._TruncExp.apply(h16[:, 0])
    cin = torch.cat([sh, h16[:, 1:]], dim=1)
    z2 = cin @ c0.T
    z3 = torch.relu(z2) @ c1.T
    h3 = torch.relu(z3) @ c2.T
    rgb = torch.sigmoid(h3)
    return dict(p=p, x=x, ok=ok, idx=idx, f=f, cell=cell, w=w, feat=feat, z1=z1, h16=h16, cin=cin, z2=z2, z3=z3, h3=h3, sigma=sigma, rgb=rgb)


def dtype_of(dtype, v):
    return torch.tensor(float(v), dtype=dtype)


def loss(net, grad_sigma, grad_rgb):
    dtype = net["rgb"].dtype
    out = (torch.tensor(np.asarray(grad_rgb), dtype=dtype) * net["rgb"]).sum()
    if grad_sigma is not None:
        out = out + (torch.tensor(np.asarray(grad_sigma), dtype=dtype) * net["sigma"]).sum()
    return out


def grad_pos(params, L, pos, dirs, bound, grad_sigma, grad_rgb, dtype=torch.float64, with_terms=False):
    """d (sum(grad_sigma * sigma) + sum(grad_rgb * rgb)) / d pos, numpy [n, 3] in dtype's precision; with_terms: also {"pos": (sum |terms|, m)}."""
    net = network(params, L, pos, dirs, bound, dtype)
    gx, dfeat = torch.autograd.grad(loss(net, grad_sigma, grad_rgb), [net["x"], net["feat"]], allow_unused=True)
    gx = torch.zeros_like(net["x"]) if gx is None else gx
    if not with_terms:
        return gx.detach().numpy()
    dfeat = torch.zeros_like(net["feat"]) if dfeat is None else dfeat
    return gx.detach().numpy(), {"pos": abs_terms_pos(net, dfeat.detach().numpy(), L, bound)}


def abs_terms_pos(net, dfeat, L, bound):
    """Per element of grad_pos: (sum of the absolute values of its levels * 2 * 4 terms, their number), from the float64 network."""
    f = net["f"].detach().numpy().astype(np.float64)
    table = net["p"][0].detach().numpy().astype(np.float64)
    idx, ok = net["idx"], net["ok"]
    n, nl = idx.shape[0], idx.shape[1]
    v = table[idx.reshape(-1)].reshape(n, nl, 8, 2)
    d = np.abs(dfeat).reshape(n, nl, 2)
    tsum = np.zeros((n, 3))
    for a in range(3):
        lo, hi = PAIRS[a]
        for pr in range(4):
            blo, bhi = pr & 1, (pr >> 1) & 1
            w = np.abs(f[:, :, lo] if blo else 1.0 - f[:, :, lo]) * np.abs(f[:, :, hi] if bhi else 1.0 - f[:, :, hi])
            left = (blo << lo) | (bhi << hi)
            diff = np.abs(v[:, :, left | (1 << a), :] - v[:, :, left, :])                             # [n, levels, 2]
            tsum[:, a] += (d * diff * (w * np.asarray(L["scale"], np.float64)[None, :])[..., None]).sum(axis=(1, 2))
    tsum = tsum * ok[:, None] / (2.0 * float(bound))
    m = np.where(ok[:, None], nl * 2 * 4, 0) * np.ones((1, 3), np.int64)
    return tsum, m


def criterion(g, g64, g32, terms):
    return B.criterion("pos", g, g64, g32, terms)
