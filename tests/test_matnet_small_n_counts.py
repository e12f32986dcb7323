"""CPU: the floors of tests/test_gpu_adjoints.py's small-n cases are not vacuous — the float64 reference alone, on the same inputs, touches exactly the number of
table entries recorded next to each floor (SMALL_N). A change of make_matnet_params, of the level layout or of the inputs shows here, without a GPU."""
import numpy as np
import pytest

from test_gpu_adjoints import SMALL_N, small_n_points
from util import torch_material_field


@pytest.fixture(scope="module")
def field(oracle, scene_mod):
    params, w0, w1, w2 = scene_mod.make_matnet_params(seed=4)
    mn, mx = scene_mod.material_min_max(me_max=0.6)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    keep = oracle.Keep()
    om = oracle.matnet_struct(keep, params, w0, w1, w2, lo, hi, mn, mx)
    return keep, om, params, w0, w1, w2, mn, mx, lo, hi, oracle.to_f16_bits(params).view(np.float16).astype(np.float64)


@pytest.mark.parametrize("n", sorted(SMALL_N))
def test_float64_reference_touches_the_recorded_entries(n, oracle, field):
    import torch
    keep, om, params, w0, w1, w2, mn, mx, lo, hi, table = field
    pos, cot = small_n_points(n)
    P64 = torch.from_numpy(table).requires_grad_(True)
    x01 = np.clip((pos - np.float32(lo[0])) / np.float32(hi[0] - lo[0]), 0, 1).astype(np.float32)
    enc = torch.from_numpy(oracle.hashgrid_encode(om, x01).view(np.float16).astype(np.float64))
    ref = torch_material_field(oracle, params, *[torch.from_numpy(a.astype(np.float64)) for a in (w0, w1, w2)], lo, hi, mn, mx, torch.from_numpy(pos).double(),
                               table=P64, enc=enc)
    (ref * torch.from_numpy(cot).double()).sum().backward()
    floor, counted = SMALL_N[n]
    assert int((P64.grad != 0).sum()) == counted > floor
