"""Independent restatement of the stage-0 radiance network as DIFFERENTIABLE torch on the host (no import from the package), for the backward's tests:
NeRFNetwork.forward (nerf/network.py:146-174) with the hash-grid encoder written as a gather on the table — the corner indices and trilinear weights of every level
from density_refs' arithmetic (grid_index, encode64 / encode32) — the five bias-free layers as radiance_refs.forward64 has them, trunc_exp with the reference's
backward (activation.py:14-16: grad * exp(clamp(x, -15, 15))) and the logistic output.  The direction encoder has no parameters: its output is a constant input here
(radiance_refs.sh64 / sh32).

    grads(...) in float64 is the truth g64; the SAME code in float32 is the yardstick: E_ref = max |g32 - g64| / max |g64| per tensor, what plain fp32 autograd
    loses on the same inputs.

THE CRITERION (criterion()): for every element e of a gradient tensor   |g[e] - g64[e]| / max |g64|  <=  max(2 * E_ref, floor[e]),   where floor[e] is the bound no
fp32 summation can beat: element e is a sum of m products (m = the number of points for a weight, the number of corner contributions for a table entry), each
product rounded once, added in SOME order: by Higham (Accuracy and Stability of Numerical Algorithms, section 4.2) any order has error <= gamma_(m+1) * sum |terms|,
gamma_k = k u / (1 - k u), u = 2^-24.  floor[e] = gamma_(m+1) * sum |terms of e| / max |g64|, with the terms taken from the float64 network (abs_terms()).  Where
max |g64| is 0 the product's tensor must be exactly 0.  Nothing here depends on what the code under test gives."""
import numpy as np
import torch

import density_refs as D
import radiance_refs as RR

U = 2.0 ** -24
NAMES = ("table", "w0", "w1", "c0", "c1", "c2")


def gamma(k):
    return k * U / (1.0 - k * U)


def corners(L, pos, bound, dtype=np.float64):
    """-> ok bool [n], idx i64 [n, levels, 8] (entries in the whole table; 0 for a point out of bounds), w dtype [n, levels, 8] (0 for a point out of bounds):
    encode64's arithmetic (dtype float64) or encode32's (float32), from the fp32 coordinates; in bounds by encode32's rule."""
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    b = np.float32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + b) / np.float32(np.float32(2.0) * b)
        # WHICH points are in bounds is the fp32 rule's decision for both precisions (u in fp32: one ulp above +bound rounds to u = 1 and is inside): a float64
        # network that called such a point outside would differ from every fp32 evaluation by that point's whole contribution
        ok = D.in_bounds(u)
        if dtype != np.float32:
            u = (pos.astype(np.float64) + float(bound)) / (2.0 * float(bound))
    nl = L["num_levels"]
    idx = np.zeros((n, nl, 8), np.int64); w = np.zeros((n, nl, 8), dtype)
    uu = u[ok]
    half, one = dtype(0.5), dtype(1.0)
    for l in range(nl):
        p = uu * dtype(L["scale"][l])
        p = p + half
        cell = np.floor(p)
        f = p - cell
        o = one - f
        c = cell.astype(np.uint32)
        for k in range(8):
            ww = np.ones(len(uu), dtype); cc = []
            for d in range(3):
                bit = (k >> d) & 1
                ww = ww * (f[:, d] if bit else o[:, d])
                cc.append(c[:, d] + np.uint32(bit))
            idx[ok, l, k] = D.grid_index(L, l, *cc) + int(L["offsets"][l])
            w[ok, l, k] = ww
    return ok, idx, w


class _TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


def network(params, L, pos, dirs, bound, dtype=torch.float64):
    """params: six arrays (NAMES) -> dict of torch tensors: the six leaf parameters `p` (requires_grad), the intermediates feat, z1 (sigma_net's hidden
    pre-activation), h16, cin, z2, z3 (the colour net's hidden pre-activations), h3, and the outputs sigma, rgb."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    ok, idx, w = corners(L, pos, bound, npd)
    p = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in params]
    table, w0, w1, c0, c1, c2 = p
    n, nl = idx.shape[0], idx.shape[1]
    g = table[torch.from_numpy(idx.reshape(-1))].reshape(n, nl, 8, 2)
    feat = (torch.from_numpy(w)[..., None] * g).sum(dim=2).reshape(n, 2 * nl)
    sh = torch.tensor(RR.sh64(dirs) if dtype == torch.float64 else RR.sh32(dirs), dtype=dtype)
    z1 = feat @ w0.T
    h16 = torch.relu(z1) @ w1.T
    sigma = _TruncExp.apply(h16[:, 0])
    cin = torch.cat([sh, h16[:, 1:]], dim=1)
    z2 = cin @ c0.T
    z3 = torch.relu(z2) @ c1.T
    h3 = torch.relu(z3) @ c2.T
    rgb = torch.sigmoid(h3)
    return dict(p=p, ok=ok, idx=idx, w=w, feat=feat, z1=z1, h16=h16, cin=cin, z2=z2, z3=z3, h3=h3, sigma=sigma, rgb=rgb)


def grads(params, L, pos, dirs, bound, grad_sigma, grad_rgb, dtype=torch.float64, with_terms=False):
    """The six gradients (numpy, dtype's precision) of sum(grad_sigma * sigma) + sum(grad_rgb * rgb); grad_sigma None: zeros.  with_terms: also abs_terms()."""
    net = network(params, L, pos, dirs, bound, dtype)
    loss = (torch.tensor(np.asarray(grad_rgb), dtype=dtype) * net["rgb"]).sum()
    if grad_sigma is not None:
        loss = loss + (torch.tensor(np.asarray(grad_sigma), dtype=dtype) * net["sigma"]).sum()
    inter = [net[k] for k in ("feat", "z1", "h16", "z2", "z3", "h3")]
    out = torch.autograd.grad(loss, net["p"] + inter, allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    g = [z(t, q).detach().numpy() for t, q in zip(out[:6], net["p"])]
    if not with_terms:
        return g
    cot = dict(zip(("feat", "z1", "h16", "z2", "z3", "h3"), (z(t, q).detach().numpy() for t, q in zip(out[6:], inter))))
    return g, abs_terms(net, cot)


def abs_terms(net, cot):
    """Per element of every gradient: (sum of the absolute values of its terms, the number of terms), from the float64 network and its cotangents."""
    a = lambda k: np.abs(net[k].detach().numpy())
    relu = lambda k: np.maximum(net[k].detach().numpy(), 0.0)
    n = net["feat"].shape[0]
    c = {k: np.abs(v) for k, v in cot.items()}
    full = lambda shape: np.full(shape, n, np.int64)
    terms = {"w0": (c["z1"].T @ a("feat"), full((64, 32))), "w1": (c["h16"].T @ relu("z1"), full((16, 64))), "c0": (c["z2"].T @ a("cin"), full((64, 31))),
             "c1": (c["z3"].T @ relu("z2"), full((64, 64))), "c2": (c["h3"].T @ relu("z3"), full((3, 64)))}
    idx, w = net["idx"], net["w"].astype(np.float64)
    entries = net["p"][0].shape[0]
    nl = idx.shape[1]
    dfeat = c["feat"].reshape(n, nl, 1, 2)
    contrib = (np.abs(w)[..., None] * dfeat)                                     # [n, levels, 8, 2]
    live = np.broadcast_to(net["ok"][:, None, None], idx.shape)
    tsum = np.zeros((entries, 2)); tcnt = np.zeros((entries, 2), np.int64)
    for ch in range(2):
        np.add.at(tsum[:, ch], idx[live], contrib[..., ch][live])
        np.add.at(tcnt[:, ch], idx[live], 1)
    terms["table"] = (tsum, tcnt)
    return terms


def measure(g, g64):
    """|g - g64| / max |g64| per element (inf where max |g64| is 0 and g is not)."""
    g = np.asarray(g, np.float64); g64 = np.asarray(g64, np.float64)
    top = np.abs(g64).max() if g64.size else 0.0
    d = np.abs(g - g64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / top) if top > 0 else np.where(d == 0, 0.0, np.inf)


def criterion(name, g, g64, g32, terms):
    """-> (worst ratio of an element's error to its allowance, E (the product's worst error), E_ref, the largest floor): the module docstring's criterion holds
    when the first value is <= 1."""
    top = np.abs(g64).max()
    if top == 0:
        bad = float(np.abs(np.asarray(g)).max()) if np.asarray(g).size else 0.0
        return (0.0 if bad == 0 else np.inf), bad, 0.0, 0.0
    e = measure(g, g64)
    e_ref = float(measure(g32, g64).max())
    tsum, m = terms[name]
    floor = gamma(m + 1) * tsum / top
    allow = np.maximum(2.0 * e_ref, floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(e == 0, 0.0, e / allow)
    return float(ratio.max()), float(e.max()), e_ref, float(floor.max())
