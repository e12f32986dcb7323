"""GPU: the batched material lookup of mirres_render called directly (csrc/matnet.hip: live-slot list -> compacted list + position keys -> radix sort ->
fused gather + MFMA MLP -> scatter by slot; the no-live form k_active_list; csrc/texmat.hip: the live-list texture lookup), through development entry
points that hand back what a frame hides: the device count, the compacted list, the list the lookup kernel walked and its keys.

Every comparison is exact (uint32 views).  References: tests/matlookup_refs.py for keys and order (pinned on the CPU by tests/test_matlookup_refs.py),
the per-lane mirres_matnet_fwd for material values (bit-equal to the oracle in tests/test_gpu_matnet.py), the public mirres_matnet_scatter and
mirres_texmat_lookup for the no-live and the texture path (the latter held to numpy in tests/test_gpu_texmat.py)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matlookup_refs as R

pytestmark = pytest.mark.gpu

BOXES = {"cube": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "slab": ((-1.0, -2.0, -1.0), (1.0, 2.0, 3.0))}   # extents are powers of two: lo + k (hi - lo) / 256 is exact
SCALE = (1.7, 0.6, 2.5)
HIST_WORDS = 256 * 1024 + 256
LS_TILE, LS_GRID = 2048, 1024
vp = C.c_void_p


class _Field:
    pass


@pytest.fixture(scope="module")
def field(scene_mod):
    """Seeded weights and table on the device, one mirres_matnet_t per box, the entry points bound."""
    from mirres_restir_nerf_mesh_amd import _lib
    from mirres_restir_nerf_mesh_amd._lib import lib, check
    F = _Field()
    params, w0, w1, w2 = scene_mod.make_matnet_params(seed=3)
    mn, mx = scene_mod.material_min_max(me_max=0.7)
    dp = torch.from_numpy(params).cuda()
    F.g16 = torch.empty(params.size, dtype=torch.int16, device="cuda")
    check(lib().mirres_matnet_pack_grid(dp.data_ptr(), F.g16.data_ptr(), params.size, None), "pack")
    F.w = [torch.from_numpy(a).cuda() for a in (w0, w1, w2)]
    F.st = {}
    for name, (lo, hi) in BOXES.items():
        st = _lib.MatNet()
        st.grid_f16 = F.g16.data_ptr(); st.w0, st.w1, st.w2 = (a.data_ptr() for a in F.w)
        st.aabb_min[:] = lo; st.aabb_max[:] = hi; st.out_min[:] = mn.tolist(); st.out_max[:] = mx.tolist()
        F.st[name] = st
    F.hist = torch.zeros(HIST_WORDS, dtype=torch.int32, device="cuda")
    L = lib()
    PF = C.POINTER(C.c_float)
    L.mirres_debug_matnet_scatter_live.restype = C.c_int
    L.mirres_debug_matnet_scatter_live.argtypes = [_lib.PMAT, vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, C.c_int, C.c_int] + [vp] * 10
    L.mirres_debug_matnet_scatter_mfma_scaled.restype = C.c_int
    L.mirres_debug_matnet_scatter_mfma_scaled.argtypes = [_lib.PMAT, vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, vp]
    L.mirres_debug_texmat_live.restype = C.c_int
    L.mirres_debug_texmat_live.argtypes = [C.POINTER(_lib.TexMat), vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, vp, vp, vp]
    F.L = L; F.check = check
    torch.cuda.synchronize()
    return F


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what, rows=None):
    """Bit-for-bit equality of two arrays of rows; names the first row that differs (`rows`: the slot of every row)."""
    if len(got) == 0 and len(want) == 0:
        return
    g = _u32(got).reshape(len(got), -1); w = _u32(want).reshape(len(want), -1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.flatnonzero((g != w).any(1))
    r = int(bad[0])
    raise AssertionError("%s: %d of %d rows differ; first: row %d%s got %r, expected %r" % (
        what, len(bad), len(g), r, "" if rows is None else " (slot %d)" % int(rows[r]), np.asarray(got)[r].tolist(), np.asarray(want)[r].tolist()))


def _fill(rng, shape):
    """What the output maps hold beforehand: values on both sides of [0, 1] and NaNs (no -0, whose clamp has two right answers)."""
    a = (rng.standard_normal(shape) * 1.5 + 0.5).astype(np.float32)
    a[rng.random(shape) < 0.05] = np.nan
    a[a == 0] = np.float32(0.25)
    return a


def _clamp_scaled(x, use_scale):
    """kd of a listed slot: clamp(x * scale, 0, 1) in float32 under use_scale."""
    if not use_scale:
        return x
    return np.fmin(np.fmax((x * np.asarray(SCALE, np.float32)[None]).astype(np.float32), np.float32(0)), np.float32(1))


def _scale3(use_scale):
    return (C.c_float * 3)(*SCALE) if use_scale else None


def _fwd(F, box, pos):
    """mirres_matnet_fwd (the per-lane kernel) at every position: f32[n, 6]."""
    n = len(pos)
    dpos = torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda()
    out = torch.empty((n, 6), device="cuda")
    F.check(F.L.mirres_matnet_fwd(C.byref(F.st[box]), dpos.data_ptr(), n, out.data_ptr(), None, None), "fwd")
    return out.cpu().numpy()


def _points(rng, n, box, spread=1.0):
    """Uniform points of the box (spread > 1: beyond it too); every fourth one on the 256-lattice of the box, where each step of the key is exact."""
    lo, hi = (np.asarray(v, np.float64) for v in BOXES[box])
    p = (lo + hi) / 2 + (rng.random((n, 3)) * 2 - 1) * (hi - lo) / 2 * spread
    k = rng.integers(0, 257, (len(p[::4]), 3))
    p[::4] = lo + k * (hi - lo) / 256
    p32 = p.astype(np.float32)
    assert np.array_equal(p32[::4].astype(np.float64), p[::4])
    return p32


def _from_cells(q, box, frac=0.5, bits=8):
    lo, hi = (np.asarray(v, np.float64) for v in BOXES[box])
    return (lo + (np.asarray(q, np.float64) + frac) * (hi - lo) / (1 << bits)).astype(np.float32)


def _run_live(F, box, pos, occ, live, nl, kd_t, rm_t, sort, bits, use_scale):
    nv = len(occ)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    dpos, docc, dlive = d(pos, np.float32), d(occ, np.float32), d(live, np.int32)
    dnl = torch.tensor([nl], dtype=torch.int32, device="cuda")
    # scratch starts as zeros: an entry the sort failed to write is then a valid slot, and a wrong list is a failed comparison, never a wild store
    scr = [torch.zeros((nv,), dtype=torch.int32, device="cuda") for _ in range(4)]              # index, keys, keys2, sorted
    outs = [torch.zeros((nv,), dtype=torch.int32, device="cuda") for _ in range(3)]             # unsorted, walked, keys
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    res = []
    for rep in range(2):                                                                          # (f): the second call runs on the same buffers
        F.check(F.L.mirres_debug_matnet_scatter_live(C.byref(F.st[box]), docc.data_ptr(), dpos.data_ptr(), nv, kd_t.data_ptr(), rm_t.data_ptr(), int(use_scale),
                                                     _scale3(use_scale), dlive.data_ptr(), dnl.data_ptr(), int(sort), bits, scr[0].data_ptr(), scr[1].data_ptr(),
                                                     scr[2].data_ptr(), scr[3].data_ptr(), F.hist.data_ptr(), cnt.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                     outs[2].data_ptr(), None), "mirres_debug_matnet_scatter_live")
        torch.cuda.synchronize()
        res.append(dict(count=int(cnt.cpu().numpy().view(np.uint32)[0]), unsorted=outs[0].cpu().numpy(), walked=outs[1].cpu().numpy(),
                        keys=outs[2].cpu().numpy().view(np.uint32), kd=kd_t.cpu().numpy(), rm=rm_t.cpu().numpy()))
    return res


def _check_live(F, box, pos, occ, live, nl, sort=1, bits=8, use_scale=False, key_ref=None):
    """Checks (a) - (f) of one live-path case; returns the reference keys."""
    nv = len(occ)
    lo, hi = BOXES[box]
    live = np.asarray(live, np.int32)
    assert live.min() >= 0 and live.max() < nv and len(np.unique(live)) == len(live) <= nv and 0 <= nl <= len(live)
    rng = np.random.default_rng(nv + 7 * nl + bits)
    kd0, rm0 = _fill(rng, (nv, 3)), _fill(rng, (nv, 2))
    kd_t, rm_t = torch.from_numpy(kd0).cuda(), torch.from_numpy(rm0).cuda()
    first, second = _run_live(F, box, pos, occ, live, nl, kd_t, rm_t, sort, bits, use_scale)
    want_listed = live[:nl][occ[live[:nl]] >= 0.5]
    # (a)
    assert first["count"] == len(want_listed), "device count %d, %d live slots have occ >= 0.5" % (first["count"], len(want_listed))
    cnt = first["count"]
    # (b)
    uns = first["unsorted"][:cnt]
    if not np.array_equal(np.sort(uns), np.sort(want_listed)):
        lost = np.setdiff1d(want_listed, uns); extra = np.setdiff1d(uns, want_listed)
        raise AssertionError("compacted list: %d slots dropped (first %s), %d slots that should not be listed (first %s), %d entries repeat a slot" % (
            len(lost), lost[:1], len(extra), extra[:1], len(uns) - len(np.unique(uns))))
    # (c)
    walked = first["walked"][:cnt]
    if sort:
        if key_ref is None:
            key_ref = R.morton_key(pos, lo, hi, bits)
        assert cnt == 0 or (walked.min() >= 0 and walked.max() < nv), "the walked list holds something that is no slot"
        keys = first["keys"][:cnt]
        if not np.array_equal(keys, key_ref[walked]):
            i = int(np.flatnonzero(keys != key_ref[walked])[0])
            raise AssertionError("key of place %d (slot %d): device %#x, restatement %#x, position %r" % (i, walked[i], keys[i], key_ref[walked[i]], pos[walked[i]].tolist()))
        want_walk = R.expected_walk(uns, key_ref)
        if not np.array_equal(walked, want_walk):
            i = int(np.flatnonzero(walked != want_walk)[0])
            in_set = np.array_equal(np.sort(walked), np.sort(uns))
            raise AssertionError("walked list differs from the stable sort of the compacted list from place %d of %d (slot %d, expected %d); it %s the same set of slots" % (
                i, cnt, walked[i], want_walk[i], "is" if in_set else "is NOT"))
        assert (np.diff(keys.astype(np.int64)) >= 0).all(), "the keys of the walked list decrease somewhere"
    else:
        assert np.array_equal(walked, uns), "without the sort the lookup kernel walks the compacted list"
    # (d), (e)
    listed = np.zeros(nv, bool); listed[want_listed] = True
    slots = np.flatnonzero(listed)
    ref = _fwd(F, box, pos[slots]) if len(slots) else np.zeros((0, 6), np.float32)
    _same(first["kd"][slots], _clamp_scaled(ref[:, 0:3], use_scale), "kd of listed slots", slots)
    _same(first["rm"][slots], ref[:, 4:6], "rough_metal of listed slots", slots)
    others = np.flatnonzero(~listed)
    _same(first["kd"][others], kd0[others], "kd of slots that are not listed", others)
    _same(first["rm"][others], rm0[others], "rough_metal of slots that are not listed", others)
    # (f)
    assert second["count"] == cnt
    _same(second["kd"], first["kd"], "kd of a second call")
    _same(second["rm"], first["rm"], "rough_metal of a second call")
    return key_ref


def _count_case(rng, L, box, extra=53):
    """L listed slots among L + extra, the live list a random order of ALL slots of which the first L count: whatever lies behind the device count is occupied too."""
    nv = L + extra
    live = rng.permutation(nv).astype(np.int32)
    occ = np.where(rng.random(nv) < 0.5, 1.0, 0.0).astype(np.float32)
    occ[live[:L]] = 1.0
    occ[live[:L:5]] = 0.5                                          # the threshold itself counts
    return _points(rng, nv, box), occ, live, L


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1])
def test_live_listed_counts(field, L):
    """Ragged tiles of the lookup kernel (64-point waves, 256-point blocks), of the compaction (2048 entries per block) and of the sort (2048-key tiles)."""
    rng = np.random.default_rng(L)
    box = "cube" if L % 2 else "slab"
    pos, occ, live, nl = _count_case(rng, L, box)
    _check_live(field, box, pos, occ, live, nl, use_scale=L in (65, 257, 2049, 3 * 2048 + 1))


@pytest.mark.parametrize("how", ["zero_count", "none_occupied"])
def test_live_nothing_listed(field, how):
    rng = np.random.default_rng(5)
    nv = 5000
    pos = _points(rng, nv, "cube")
    live = rng.permutation(nv).astype(np.int32)
    if how == "zero_count":                                         # a long list of occupied slots behind a device count of zero
        _check_live(field, "cube", pos, np.ones(nv, np.float32), live, 0, use_scale=True)
    else:
        occ = np.where(rng.random(nv) < 0.5, np.float32(0.49999997), np.float32(0.0)).astype(np.float32)
        _check_live(field, "cube", pos, occ, live, nv, use_scale=True)


@pytest.mark.parametrize("shape", ["ascending", "descending", "random", "every_other_empty", "few_of_many"])
def test_live_list_shapes(field, shape):
    rng = np.random.default_rng(11)
    nv = 100000 if shape == "few_of_many" else 5003
    pos = _points(rng, nv, "slab")
    occ = np.ones(nv, np.float32)
    if shape == "ascending": live = np.arange(nv)
    elif shape == "descending": live = np.arange(nv)[::-1]
    elif shape == "random": live = rng.permutation(nv)
    elif shape == "every_other_empty":
        live = rng.permutation(nv)[:4000]
        occ[live[::2]] = 0.0
    else:
        live = np.sort(rng.permutation(nv)[:300])
        occ[live[::7]] = 0.25
    _check_live(field, "slab", pos, occ, np.ascontiguousarray(live, np.int32), len(live), use_scale=shape in ("every_other_empty", "few_of_many"))


@pytest.mark.parametrize("keys", ["identical", "two_alternating", "lowest_byte", "highest_byte", "boundaries", "outside", "nonfinite"])
def test_live_key_patterns(field, keys):
    rng = np.random.default_rng(13)
    box = "cube"
    lo, hi = (np.asarray(v, np.float32) for v in BOXES[box])
    n = 2 * 2048 + 1 if keys == "identical" else 5003
    if keys == "identical":                                          # one digit bucket in every pass, all 64 lanes of every ballot match
        pos = np.repeat(np.array([[0.3, -0.2, 0.7]], np.float32), n, 0)
    elif keys == "two_alternating":
        pos = np.where((np.arange(n) % 2 == 0)[:, None], np.array([[0.9, 0.9, -0.9]], np.float32), np.array([[-0.3, 0.1, 0.5]], np.float32)).astype(np.float32)
    elif keys == "lowest_byte":                                      # key bits 0 .. 7: x bits 0, 1; y and z bits 0 .. 2
        pos = _from_cells(np.stack([rng.integers(0, 4, n), rng.integers(0, 8, n), rng.integers(0, 8, n)], 1), box, frac=rng.random((n, 3)) * 0.9)
    elif keys == "highest_byte":                                     # key bits 16 .. 23: x and y bits 5 .. 7, z bits 6, 7 (points on cell corners: lattice points)
        pos = _from_cells(np.stack([32 * rng.integers(0, 8, n), 32 * rng.integers(0, 8, n), 64 * rng.integers(0, 4, n)], 1), box, frac=0.0)
    elif keys == "boundaries":                                       # exactly on the cell faces, the max faces of the box included
        pos = _from_cells(rng.integers(0, 257, (n, 3)), box, frac=0.0)
    elif keys == "outside":
        pos = _points(rng, n, box, spread=1.5)
        for a in range(3):
            pos[8 + 2 * a, a] = lo[a] - np.float32(1e-3); pos[9 + 2 * a, a] = hi[a] + np.float32(1e-3)
            pos[16 + 2 * a, a] = np.float32(-1e30); pos[17 + 2 * a, a] = np.float32(1e30)
            pos[24 + 2 * a, a] = np.nextafter(lo[a], np.float32(-9)); pos[25 + 2 * a, a] = np.nextafter(hi[a], np.float32(9))
    else:
        pos = _points(rng, n, box, spread=1.1)
        bad = rng.random((n, 3)) < 0.1
        pos[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        pos[:3] = [[np.nan] * 3, [np.inf] * 3, [-np.inf] * 3]
    key_ref = R.morton_key(pos, lo, hi, 8)
    if keys == "identical": assert len(np.unique(key_ref)) == 1
    if keys == "two_alternating": assert len(np.unique(key_ref)) == 2
    if keys == "lowest_byte": assert (key_ref < 256).all() and len(np.unique(key_ref)) == 256
    if keys == "highest_byte": assert (key_ref & 0xffff == 0).all() and len(np.unique(key_ref)) == 256
    occ = np.ones(n, np.float32)
    _check_live(field, box, pos, occ, rng.permutation(n).astype(np.int32), n, use_scale=keys == "nonfinite", key_ref=key_ref)


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("bits", [1, 3, 5, 8])
def test_live_bits_and_passes(field, bits, sort):
    """1, 3, 5, 8 bits per axis = one, two, two, three 8-bit passes: the sorted list ends in the scratch buffer, in the caller's index (twice; bits = 3: a second
    pass with one significant bit), in the scratch buffer."""
    rng = np.random.default_rng(17 + bits)
    box = "cube" if bits in (1, 5) else "slab"
    n = 5003
    pos = _points(rng, n, box, spread=1.05)
    occ = np.where(rng.random(n) < 0.9, 1.0, 0.0).astype(np.float32)
    _check_live(field, box, pos, occ, rng.permutation(n).astype(np.int32), n, sort=sort, bits=bits, use_scale=bits == 5)


@pytest.mark.parametrize("n,bits", [(LS_GRID * LS_TILE, 8), (LS_GRID * LS_TILE + 1, 8), (2 * LS_GRID * LS_TILE + 2049, 8), (2 * LS_GRID * LS_TILE + 2049, 5)])
def test_live_large_regimes(field, n, bits):
    """nv = nl = n, every slot live and occupied: exactly one sort tile per workgroup; two tiles per workgroup with the last workgroups empty; the compaction's
    second grid-stride iteration (more than 2048 x 2048 entries) with three tiles per workgroup.  Measured on an MI355X, host side included: 0.6 s, 0.5 s, 1.1 s, 1.1 s."""
    t0 = time.time()
    rng = np.random.default_rng(n % 1000 + bits)
    pos = _points(rng, n, "cube")
    live = np.arange(n, dtype=np.int32)
    _check_live(field, "cube", pos, np.ones(n, np.float32), live, n, bits=bits)
    print("large regime %d entries, %d bits: %.2f s" % (n, bits, time.time() - t0))


# ---------------------------------------------------------------- no live list: k_active_list
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097, 70001])
def test_no_live_path(field, n, offset, use_scale):
    """The whole-map form: 16 slots per thread by 16-byte loads when the map is 16-byte aligned and the run is whole, else one by one (offset = 1: a view that
    starts one float later).  Same list either way; kd / rough_metal equal to the public per-lane mirres_matnet_scatter on every row, the rows without a vertex
    included (their kd is clamped under use_scale); listed rows equal to mirres_matnet_fwd."""
    F = field
    rng = np.random.default_rng(n)
    box = "slab"
    pos = _points(rng, n, box, spread=1.1)
    occ = np.where(rng.random(n) < 0.6, 1.0, 0.0).astype(np.float32)
    occ[::9] = 0.5
    occ[2::9] = np.float32(0.49999997)
    kd0, rm0 = _fill(rng, (n, 3)), _fill(rng, (n, 2))
    buf = torch.zeros(n + 8, device="cuda")
    docc = buf[offset:offset + n]; docc.copy_(torch.from_numpy(occ))
    assert docc.data_ptr() % 16 == 4 * offset
    dpos = torch.from_numpy(pos).cuda()
    kd_a, rm_a, kd_b, rm_b = (torch.from_numpy(a).cuda() for a in (kd0, rm0, kd0, rm0))
    index = torch.full((n,), -7, dtype=torch.int32, device="cuda"); cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    st = C.byref(F.st[box])
    F.check(F.L.mirres_debug_matnet_scatter_mfma_scaled(st, docc.data_ptr(), dpos.data_ptr(), n, kd_a.data_ptr(), rm_a.data_ptr(), int(use_scale), _scale3(use_scale),
                                                        index.data_ptr(), cnt.data_ptr(), None), "mirres_debug_matnet_scatter_mfma_scaled")
    F.check(F.L.mirres_matnet_scatter(st, docc.data_ptr(), dpos.data_ptr(), n, kd_b.data_ptr(), rm_b.data_ptr(), int(use_scale), _scale3(use_scale), None), "mirres_matnet_scatter")
    torch.cuda.synchronize()
    slots = np.flatnonzero(occ >= 0.5)
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c == len(slots)
    assert np.array_equal(np.sort(index.cpu().numpy()[:c]), slots), "the list is not the set of rows with occ >= 0.5"
    kd, rm = kd_a.cpu().numpy(), rm_a.cpu().numpy()
    _same(kd, kd_b.cpu().numpy(), "kd against mirres_matnet_scatter")
    _same(rm, rm_b.cpu().numpy(), "rough_metal against mirres_matnet_scatter")
    ref = _fwd(F, box, pos[slots]) if len(slots) else np.zeros((0, 6), np.float32)
    _same(kd[slots], _clamp_scaled(ref[:, 0:3], use_scale), "kd of listed rows", slots)
    _same(rm[slots], ref[:, 4:6], "rough_metal of listed rows", slots)
    others = np.flatnonzero(occ < 0.5)
    _same(rm[others], rm0[others], "rough_metal of rows without a vertex", others)
    _same(kd[others], np.fmin(np.fmax(kd0[others], np.float32(0)), np.float32(1)) if use_scale else kd0[others], "kd of rows without a vertex", others)


# ---------------------------------------------------------------- the texture path: k_texmat<true>
@pytest.fixture(scope="module")
def tex_asset(scene_mod):
    import test_gpu_texmat as TT
    from mirres_restir_nerf_mesh_amd import export
    return TT._two_cascade_material(export, scene_mod, np.random.default_rng(4)), TT._hits


@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("nl,nv", [(0, 700), (1, 700), (255, 700), (256, 700), (257, 700), (2048 * 256 + 257, 2048 * 256 + 257)])
def test_texture_live_path(field, tex_asset, nl, nv, use_scale):
    """The live slots in random order; slot -> ray by a permutation with -1 entries; ray -> triangle with -1 and T among them; some live slots unoccupied.
    Reference: the public row kernel on the listed slots with prim = ray_prim[slot_c[slot]] (-1 where slot_c < 0)."""
    F = field
    m, hits = tex_asset
    T = int(m.tri_end[-1])
    rng = np.random.default_rng(nl + int(use_scale))
    prim, pos = hits(m, rng, nv)
    ray_of = rng.permutation(nv).astype(np.int32)                  # slot -> ray
    ray_prim = np.empty(nv, np.int32); ray_prim[ray_of] = prim
    bad = rng.random(nv) < 0.06
    ray_prim[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, T)
    slot_c = ray_of.copy(); slot_c[rng.random(nv) < 0.06] = -1
    occ = np.where(rng.random(nv) < 0.85, 1.0, 0.0).astype(np.float32); occ[::11] = 0.5
    live = rng.permutation(nv).astype(np.int32)                    # all slots; the first nl count
    if nl == 1:                                                     # the one live slot has a vertex on a valid triangle
        s = int(np.flatnonzero((occ >= 0.5) & (slot_c >= 0) & (ray_prim[np.maximum(slot_c, 0)] >= 0) & (ray_prim[np.maximum(slot_c, 0)] < T))[0])
        live[np.flatnonzero(live == s)[0]] = live[0]; live[0] = s
    kd0, rm0 = _fill(rng, (nv, 3)), _fill(rng, (nv, 2))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kd_t, rm_t = d(kd0), d(rm0)
    dnl = torch.tensor([nl], dtype=torch.int32, device="cuda")
    keep = [d(occ), d(pos.astype(np.float32)), d(live), d(slot_c), d(ray_prim)]
    t0 = time.time()
    F.check(F.L.mirres_debug_texmat_live(C.byref(m._struct()), keep[0].data_ptr(), keep[1].data_ptr(), nv, kd_t.data_ptr(), rm_t.data_ptr(), int(use_scale),
                                         _scale3(use_scale), keep[2].data_ptr(), dnl.data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), None), "mirres_debug_texmat_live")
    torch.cuda.synchronize()
    kd, rm = kd_t.cpu().numpy(), rm_t.cpu().numpy()
    ls = live[:nl]
    rows_prim = np.where(slot_c[ls] >= 0, ray_prim[np.maximum(slot_c[ls], 0)], -1).astype(np.int32)
    vertex = (occ[ls] >= 0.5) & (rows_prim >= 0) & (rows_prim < T)
    if nl:
        kd_r, rm_r = m.lookup(d(rows_prim), d(pos[ls].astype(np.float32)), occ=d(occ[ls]), kd=d(kd0[ls]), rough_metal=d(rm0[ls]), use_scale=use_scale, scale=SCALE)
        torch.cuda.synchronize()
        kd_r, rm_r = kd_r.cpu().numpy(), rm_r.cpu().numpy()
        assert vertex.any() and (nl < 255 or (~vertex).any())
        _same(kd[ls][vertex], kd_r[vertex], "kd of live slots with a vertex on a triangle", ls[vertex])
        _same(rm[ls][vertex], rm_r[vertex], "rough_metal of live slots with a vertex on a triangle", ls[vertex])
        assert np.isfinite(kd[ls][vertex]).all() and np.isfinite(rm[ls][vertex]).all()
        # live slots without a vertex (slot_c = -1, triangle < 0 or >= T, occ < 0.5): rough_metal untouched, kd clamped to [0, 1] under use_scale, else untouched
        nov = ls[~vertex]
        _same(rm[nov], rm0[nov], "rough_metal of live slots without a vertex", nov)
        _same(kd[nov], np.fmin(np.fmax(kd0[nov], np.float32(0)), np.float32(1)) if use_scale else kd0[nov], "kd of live slots without a vertex", nov)
        if use_scale:
            assert (kd[ls] >= 0).all() and (kd[ls] <= 1).all()
    rest = live[nl:]
    _same(kd[rest], kd0[rest], "kd of slots that are not live", rest)
    _same(rm[rest], rm0[rest], "rough_metal of slots that are not live", rest)
    if nv > 100000:
        print("texture live path, %d slots: %.2f s after the upload" % (nv, time.time() - t0))
