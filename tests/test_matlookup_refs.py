"""CPU: the numpy restatement of the material lookup's position key (tests/matlookup_refs.py) pinned by answers one can check by hand, so that
tests/test_gpu_matlookup.py compares the device's keys with something that is itself known."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matlookup_refs as R

BOXES = [((-1, -1, -1), (1, 1, 1)), ((-1, -2, -1), (1, 2, 3))]
BITS = [1, 3, 5, 8]


def _cell(lo, hi, bits):
    return (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / (1 << bits)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("box", BOXES)
def test_corners(box, bits):
    lo, hi = box
    ones = (1 << (3 * bits)) - 1
    assert R.morton_key([lo], lo, hi, bits).tolist() == [0]
    assert R.morton_key([hi], lo, hi, bits).tolist() == [ones]
    beyond = np.asarray(hi, np.float32) + np.float32(0.75)
    assert R.morton_key([beyond, beyond * 1e6], lo, hi, bits).tolist() == [ones, ones]
    below = np.asarray(lo, np.float32) - np.float32(0.75)
    assert R.morton_key([below, below * 1e6], lo, hi, bits).tolist() == [0, 0]
    assert R.morton_key([lo], lo, hi, bits).dtype == np.uint32


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("box", BOXES)
def test_one_step_per_axis(box, bits):
    """One cell along x, y, z from the min corner sets bits 2, 1, 0 of the lowest triple; one cell along all three sets 7."""
    lo, hi = box
    c = _cell(lo, hi, bits)
    for axis, want in ((0, 4), (1, 2), (2, 1)):
        p = np.asarray(lo, np.float64).copy(); p[axis] += c[axis]
        assert R.morton_key([p], lo, hi, bits).tolist() == [want], (axis, bits)
        p[axis] -= 0.25 * c[axis]                                   # still inside the first cell
        assert R.morton_key([p], lo, hi, bits).tolist() == [0]
    assert R.morton_key([np.asarray(lo) + c], lo, hi, bits).tolist() == [7]


def test_interleave_by_hand():
    """bits = 8, box (-1, 1): cell numbers (x, y, z) = (0b10000001, 0b00000010, 0b11111111) -> x at bits 2, 23; y at bit 4; z at bits 0, 3, .. 21."""
    lo, hi = BOXES[0]
    q = np.array([129, 2, 255])
    p = -1 + (q + 0.5) / 128
    want = (1 << 2) | (1 << 23) | (1 << 4) | sum(1 << (3 * b) for b in range(8))
    assert R.morton_key([p], lo, hi, 8).tolist() == [want]
    assert R.quantise([p], lo, hi, 8).tolist() == [q.tolist()]
    # bits = 1: one bit per axis, key = 4 x + 2 y + z of the octant
    pts = [[-0.5, -0.5, -0.5], [-0.5, -0.5, 0.5], [-0.5, 0.5, -0.5], [0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]]
    assert R.morton_key(pts, lo, hi, 1).tolist() == [0, 1, 2, 4, 7, 7]
    assert R.spread10(0x3ff) == 0x9249249 and R.spread10(0b101) == 0b1000001 and R.spread10(0x7ff) == 0x9249249


@pytest.mark.parametrize("bits", [1, 8])
@pytest.mark.parametrize("box", BOXES)
def test_each_axis_is_monotone(box, bits):
    lo, hi = box
    lo_a, hi_a = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    t = np.linspace(-0.1, 1.1, 1537)
    for axis in range(3):
        p = np.repeat(((lo_a + hi_a) / 2)[None], len(t), 0)
        p[:, axis] = lo_a[axis] + t * (hi_a[axis] - lo_a[axis])
        k = R.morton_key(p, lo, hi, bits).astype(np.int64)
        assert (np.diff(k) >= 0).all(), (axis, bits)
        q = R.quantise(p, lo, hi, bits)[:, axis]
        assert q[0] == 0 and q[-1] == (1 << bits) - 1 and len(np.unique(q)) == 1 << bits
        others = [a for a in range(3) if a != axis]
        assert (R.quantise(p, lo, hi, bits)[:, others] == R.quantise(p[:1], lo, hi, bits)[:, others]).all()


@pytest.mark.parametrize("bits", [1, 8])
def test_nan_and_inf(bits):
    lo, hi = BOXES[1]
    top = (1 << bits) - 1
    nan, inf = np.nan, np.inf
    q = R.quantise([[nan, nan, nan], [inf, -inf, inf], [-inf, inf, nan], [0.0, nan, 1.0]], lo, hi, bits)
    mid_x = (1 << bits) // 2
    z1 = int(np.trunc((1.0 + 1.0) / 4.0 * (1 << bits)))
    assert q.tolist() == [[0, 0, 0], [top, 0, top], [0, top, 0], [mid_x, 0, z1]]
    ones = (1 << (3 * bits)) - 1
    assert R.morton_key([[nan] * 3, [inf] * 3, [-inf] * 3], lo, hi, bits).tolist() == [0, ones, 0]


@pytest.mark.parametrize("bits", BITS)
def test_lattice_points_fall_on_cell_boundaries(bits):
    """Box (-1, 1): pos = -1 + k / 128 is exact in float32 and so is every step of the key's arithmetic: cell k >> (8 - bits), 255 for k = 256."""
    lo, hi = BOXES[0]
    k = np.arange(257)
    p = np.stack([-1 + k / 128, np.full(257, -1.0), np.full(257, -1.0)], 1).astype(np.float32)
    assert np.array_equal(p[:, 0].astype(np.float64), -1 + k / 128)
    assert R.quantise(p, lo, hi, bits)[:, 0].tolist() == np.minimum(k >> (8 - bits), (1 << bits) - 1).tolist()


def test_expected_walk_is_a_stable_sort():
    keys = np.array([5, 1, 5, 0, 1, 9, 5], np.uint32)               # key of every slot
    unsorted = np.array([6, 2, 0, 4, 1, 3])                         # slot 5 is not listed
    assert R.expected_walk(unsorted, keys).tolist() == [3, 4, 1, 6, 2, 0]
    assert R.expected_walk(np.array([], np.int32), keys).tolist() == []


def test_development_entry_points_refuse_bad_arguments():
    """No GPU call: the two development entry points of the lookup (bound ad hoc, not part of include/mirres.h) return an error before any launch."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from mirres_restir_nerf_mesh_amd import _lib
    L = _lib.lib()
    vp, PF = C.c_void_p, C.POINTER(C.c_float)
    L.mirres_debug_matnet_scatter_live.restype = C.c_int
    L.mirres_debug_matnet_scatter_live.argtypes = [_lib.PMAT, vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, C.c_int, C.c_int] + [vp] * 10
    L.mirres_debug_matnet_scatter_mfma_scaled.restype = C.c_int
    L.mirres_debug_matnet_scatter_mfma_scaled.argtypes = [_lib.PMAT, vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, vp]
    L.mirres_debug_texmat_live.restype = C.c_int
    L.mirres_debug_texmat_live.argtypes = [C.POINTER(_lib.TexMat), vp, vp, C.c_int, vp, vp, C.c_int, PF, vp, vp, vp, vp, vp]
    st = _lib.MatNet()
    p = 4096                                                          # stands for a pointer; nothing is launched
    full = [C.byref(st), p, p, 16, p, p, 0, None, p, p, 1, 8] + [p] * 9 + [None]
    for i in (0, 1, 2, 4, 5, 8, 9, 12, 13, 14, 15, 16, 17):          # every pointer the lookup itself needs
        a = list(full); a[i] = None
        assert L.mirres_debug_matnet_scatter_live(*a) < 0, i
        assert b"mirres_debug_matnet_scatter_live" in L.mirres_last_error()
    for nv, bits in ((0, 8), (-1, 8), (16, 0), (16, 9)):
        a = list(full); a[3] = nv; a[11] = bits
        assert L.mirres_debug_matnet_scatter_live(*a) < 0, (nv, bits)
    assert L.mirres_debug_matnet_scatter_mfma_scaled(C.byref(st), None, p, 16, p, p, 1, None, p, p, None) < 0
    assert L.mirres_debug_matnet_scatter_mfma_scaled(C.byref(st), p, p, 0, p, p, 1, None, p, p, None) < 0
    tm = _lib.TexMat()
    full = [C.byref(tm), None, p, 16, p, p, 0, None, p, p, p, p, None]
    for i in (2, 4, 5, 8, 9, 10, 11):
        a = list(full); a[i] = None
        assert L.mirres_debug_texmat_live(*a) < 0, i
    assert L.mirres_debug_texmat_live(*full) < 0 and b"bad texture material" in L.mirres_last_error()      # an empty mirres_texmat_t
