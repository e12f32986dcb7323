"""Independent numpy restatement of the hash grid's total-variation regulariser (no import from the package): GridEncoder.grad_total_variation
(gridencoder/grid.py:170-192) over kernel_grad_tv (gridencoder/src/gridencoder.cu:505-609) with the operation order DESIGN.md section 5.16 fixes.  Per point and
level: u = (x + bound) / (2 bound), c = floor(u * scale + 0.5) (the encoder's corner 0), e = grid_index(c); for d = 0, 1, 2 the right neighbour (c[d] + 1 when
c[d] < resolution), then the left (c[d] - 1 when c[d] > 0), per channel diff = t[e] - t[nb], res = res + diff, idelta = idelta + diff * diff;
w = weight / 6; value = (w * res) * (1 / sqrt(idelta + 1e-9)).  In float32 every numpy operation rounds once (no fused multiply-add), which is what the kernel
computes; in float64 the same expression from the same fp32 cells, table, weight and 1e-9f.
The terms are bit-determined; only the ORDER in which a hashed entry's terms are added is free.  So nothing here is measured: a dense entry is
grad0 + fp32(count) * value, a hashed entry with one term is fp32(grad0 + value), and a hashed entry with m >= 2 terms lies within gamma(m) * (|grad0| + sum |terms|)
of the float64 sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: m additions in any order, u = 2^-24 — merging k equal terms into
fp32(k) * value first is one more rounding on those terms in place of k - 1 additions, which the same bound covers for k >= 2)."""
import numpy as np

from density_refs import layout, grid_index, in_bounds, P1, P2  # noqa: F401  (re-exported for the tests)

F32 = np.float32
U32 = np.uint32
EPS = F32(1e-9)


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def cells(L, pos, bound):
    """pos f32 [n, 3] -> (keep bool [n], [per level: cell u32 [m, 3]]) for the m points inside [-bound, bound]^3; fp32 as the encoder computes them."""
    pos = np.asarray(pos, F32).reshape(-1, 3); b = F32(bound)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (pos + b) / F32(F32(2.0) * b)
    keep = in_bounds(u)
    uu = u[keep]
    out = []
    for l in range(L["num_levels"]):
        p = uu * L["scale"][l]
        p = p + F32(0.5)
        out.append(np.floor(p).astype(U32))
    return keep, out


def cell_values(table, L, l, c, weight, f64=False):
    """c u32 [m, 3] cells of level l -> (entry i64 [m] inside the level, value [m, 2], scale [m, 2]); scale = w * sum |diff| / sqrt(idelta + 1e-9), what the
    rounding errors of the fp32 evaluation are proportional to.  fp32 with the kernel's order, or float64."""
    T = np.float64 if f64 else F32
    g = np.asarray(table, F32)[L["offsets"][l]: L["offsets"][l + 1]].astype(T)
    res = U32(L["resolution"][l])
    c = np.asarray(c, U32).reshape(-1, 3)
    e = grid_index(L, l, c[:, 0], c[:, 1], c[:, 2])
    t = g[e]
    r = np.zeros((len(c), 2), T); idl = np.zeros((len(c), 2), T); a = np.zeros((len(c), 2), T)
    for d in range(3):
        for side in (1, -1):
            take = (c[:, d] < res) if side > 0 else (c[:, d] > 0)
            cc = c.copy()
            with np.errstate(over="ignore"):
                cc[:, d] = c[:, d] + U32(1) if side > 0 else c[:, d] - U32(1)
            nb = grid_index(L, l, cc[:, 0], cc[:, 1], cc[:, 2])
            diff = t - g[nb]
            r = np.where(take[:, None], r + diff, r)
            idl = np.where(take[:, None], idl + diff * diff, idl)
            a = np.where(take[:, None], a + np.abs(diff), a)
    w = T(F32(weight)) / T(6.0)
    inv = T(1.0) / np.sqrt(idl + T(EPS))
    return e, (w * r) * inv, (w * a) * inv


def point_terms(table, L, pos, bound, weight, f64=False):
    """-> [per level: (entry i64 [m] in the WHOLE table, value [m, 2])] over the m in-bounds points, in point order."""
    _, cs = cells(L, pos, bound)
    out = []
    for l, c in enumerate(cs):
        e, v, _ = cell_values(table, L, l, c, weight, f64)
        out.append((e + int(L["offsets"][l]), v))
    return out


def dense_levels(L):
    return [l for l in range(L["num_levels"]) if not L["hashed"][l]]


def hashed_levels(L):
    return [l for l in range(L["num_levels"]) if L["hashed"][l]]


def level_mask(L, levels):
    """bool [entries]: the entries of `levels`."""
    m = np.zeros(int(L["total"]), bool)
    for l in levels:
        m[L["offsets"][l]: L["offsets"][l + 1]] = True
    return m


def expected_dense(grad0, table, L, pos, bound, weight):
    """-> (grad f32 [entries, 2], touched bool [entries]): grad0 with grad0 + fp32(count) * value at every dense-level entry that holds `count` > 0 points, in fp32,
    every other entry (the hashed levels included) as it was."""
    g = np.array(grad0, F32, copy=True); touched = np.zeros(len(g), bool)
    _, cs = cells(L, pos, bound)
    for l in dense_levels(L):
        uc, count = np.unique(cs[l], axis=0, return_counts=True)
        if not len(uc):
            continue
        e, v, _ = cell_values(table, L, l, uc, weight)
        e = e + int(L["offsets"][l])
        assert len(np.unique(e)) == len(e), "a dense level's cells and entries are one to one"
        g[e] = g[e] + count.astype(F32)[:, None] * v
        touched[e] = True
    return g, touched


def expected_hashed(grad0, table, L, pos, bound, weight):
    """-> dict over the hashed-level entries that receive a term: entry i64 [k] (sorted), terms i64 [k] (how many), sum64 f64 [k, 2] (grad0 + the fp32 terms,
    added in float64), allow f64 [k, 2] = gamma(terms) * (|grad0| + sum |terms|), single f32 [k, 2] = fp32(grad0 + value) (meaningful where terms == 1)."""
    grad0 = np.asarray(grad0, F32)
    pt = point_terms(table, L, pos, bound, weight)
    hl = hashed_levels(L)
    ent = np.concatenate([pt[l][0] for l in hl] + [np.zeros(0, np.int64)])
    val = np.concatenate([pt[l][1] for l in hl] + [np.zeros((0, 2), F32)])
    entry, inv, terms = np.unique(ent, return_inverse=True, return_counts=True)
    s = np.zeros((len(entry), 2)); a = np.zeros((len(entry), 2)); last = np.zeros((len(entry), 2), F32)
    np.add.at(s, inv, val.astype(np.float64)); np.add.at(a, inv, np.abs(val).astype(np.float64))
    last[inv] = val
    g0 = grad0[entry]
    return dict(entry=entry, terms=terms, sum64=g0.astype(np.float64) + s, allow=np.array([gamma(int(m)) for m in terms])[:, None] * (np.abs(g0).astype(np.float64) + a),
                single=g0 + last)


def check(got, grad0, table, L, pos, bound, weight):
    """Every claim about one call at once: got f32 [entries, 2] after accumulating into grad0.  Returns the number of hashed entries with one term and with more."""
    got = np.asarray(got, F32); grad0 = np.asarray(grad0, F32)
    want, touched = expected_dense(grad0, table, L, pos, bound, weight)
    dm = level_mask(L, dense_levels(L))
    assert np.array_equal(got[dm].view(U32), want[dm].view(U32)), "dense levels: %d entries differ in their bits" % int((got[dm].view(U32) != want[dm].view(U32)).any(axis=1).sum())
    H = expected_hashed(grad0, table, L, pos, bound, weight)
    rest = ~dm
    rest[H["entry"]] = False
    assert np.array_equal(got[rest].view(U32), grad0[rest].view(U32)), "an entry no point reaches changed"
    one = H["terms"] == 1
    g = got[H["entry"]]
    assert np.array_equal(g[one].view(U32), H["single"][one].view(U32)), "a hashed entry with one term is not fp32(grad0 + value)"
    err = np.abs(g[~one].astype(np.float64) - H["sum64"][~one])
    assert (err <= H["allow"][~one]).all(), "hashed entries: worst error / allowance %g" % float((err / np.maximum(H["allow"][~one], 1e-300)).max())
    return int(one.sum()), int((~one).sum())
