"""The hash grid's total-variation regulariser on the device (csrc/grid_tv.hip) through the C ABI, stage0.DensityField.grad_total_variation, one whole training
step and scripts/train_stage0.py, against the numpy restatement of tests/tv_refs.py.  What is held, and where (tv_refs.check):
  dense levels, every entry      bits equal to grad0 + fp32(count) * value; an entry without a point keeps its bits;
  hashed entries with one term   bits equal to fp32(grad0 + value);
  every other hashed entry       |g - sum64| <= gamma(m) * (|grad0| + sum |terms|) for its m terms (the order of m additions is free, nothing else is).
Nothing is tuned to the device.  The layout is T = 14 (levels 0-1 dense, 2-15 hashed; a 2 MB table) with one T = 19 case (levels 0-4 dense); the gradient starts
non-zero.  Sizes 1, 63, 64, 65 (a wave and its neighbours: the ballots' merge), 255, 256, 257 (a block and its neighbours), 4096 (16 blocks).

The case "a cell whose neighbour collides with itself" cannot be built: test_no_cell_has_a_neighbour_on_its_own_entry says why and asserts it.

Measured on the MI355X when these tests were written: all pass; the script's run A (no new option) ends at a last-window loss of 9.71e-4,
run B (-O --lambda_tv 1e-8 --num_points 65536) at 4.95e-4 with 361 ... 562 rays per step."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tv_refs as TV          # noqa: E402

F32 = np.float32
U32 = np.uint32
WEIGHT = 1e-3


@pytest.fixture(scope="module")
def S0():
    from mirres_restir_nerf_mesh_amd import stage0
    return stage0


class Net:
    """One seeded table on the host (left unchanged by every test), its layout, a starting gradient, and the DensityField over it (w0 and w1 are not read)."""

    def __init__(self, S0, log2_T, seed, spread, bound=1.0, num_levels=16):
        self.bound = bound
        self.L = TV.layout(bound, num_levels=num_levels, log2_T=log2_T)
        rng = np.random.default_rng(seed)
        n = self.L["total"]
        if spread:                                                                      # magnitudes over five decades: the terms of one entry differ
            self.table = (rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-5, 0, size=(n, 2))).astype(F32)
        else:                                                                           # GridEncoder.reset_parameters, as RadianceField.init_random
            self.table = rng.uniform(-1e-4, 1e-4, size=(n, 2)).astype(F32)
        self.grad0 = (rng.normal(size=(n, 2)) * 1e-4).astype(F32)
        self.field = S0.DensityField(torch.from_numpy(self.table), torch.zeros(64, 32), torch.zeros(16, 64), bound=bound, log2_hashmap_size=log2_T, num_levels=num_levels)
        for a in (self.table, self.grad0):
            a.setflags(write=False)

    def run(self, pos, weight=WEIGHT):
        g = torch.tensor(self.grad0).cuda().clone()
        assert len(pos) > 0
        assert self.field.grad_total_variation(weight, torch.from_numpy(np.ascontiguousarray(pos, F32)).cuda(), grad=g) is None
        return g.cpu().numpy()

    def check(self, got, pos, weight=WEIGHT, grad0=None):
        return TV.check(got, self.grad0 if grad0 is None else grad0, self.table, self.L, pos, self.bound, weight)


@pytest.fixture(scope="module")
def nets(S0):
    out = {"init": Net(S0, 14, 201, False), "spread": Net(S0, 14, 202, True)}
    assert TV.dense_levels(out["init"].L) == [0, 1] and out["init"].L["total"] * 8 < 2.1e6
    return out


def _points(n, bound=1.0, seed=5):
    """Hostile points first (test_gpu_radiance.py's idea), random ones after: the corners, u = 0 and u = 1 on each axis, points on level 0's cell faces, one ulp
    outside +-bound on every axis and side (below -bound: u < 0, outside; above +bound: x + bound rounds to 2 bound, u = 1, inside), a NaN, +inf and -inf."""
    b = F32(bound)
    face = lambda k: F32((F32(k) - F32(0.5)) / F32(15.0) * F32(2.0) - F32(1.0)) * b
    sp = [[0.1, -0.3, 0.6], [-b, -b, -b], [b, b, b], [-b, 0.2, 0.3], [b, 0.2, 0.3], [0.2, -b, 0.3], [0.2, b, 0.3], [0.2, 0.3, -b], [0.2, 0.3, b],
          [face(1), face(8), face(15)], [face(7), face(7), face(7)]]
    for d in range(3):
        for side in (1, -1):
            p = [0.3, -0.2, 0.7]; p[d] = np.nextafter(F32(side) * b, F32(side) * F32(np.inf)); sp.append(p)
    sp += [[np.nan, 0.1, 0.2], [0.1, np.inf, 0.2], [0.1, 0.2, -np.inf], [3.0 * b, 0.0, 0.0]]
    rnd = np.random.default_rng(seed).uniform(-bound, bound, size=(max(n, 1), 3)).astype(F32)
    return np.concatenate([np.array(sp, F32), rnd])[:n]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4096])
@pytest.mark.parametrize("which", ["init", "spread"])
def test_every_entry_against_the_restatement(nets, which, n):
    net = nets[which]
    pos = _points(n)
    one, more = net.check(net.run(pos), pos)
    assert one + more > 0
    print("%s n %d: %d hashed entries with one term (bits), %d with more (allowance)" % (which, n, one, more))


def test_t19_five_dense_levels(S0):
    net = Net(S0, 19, 203, True)
    assert TV.dense_levels(net.L) == [0, 1, 2, 3, 4]
    pos = _points(4096, seed=6)
    got = net.run(pos)
    net.check(got, pos)
    perm = np.random.default_rng(0).permutation(len(pos))
    dm = TV.level_mask(net.L, TV.dense_levels(net.L))
    assert np.array_equal(_bits(net.run(pos[perm])[dm]), _bits(got[dm]))


def test_contention_one_coarse_cell_and_one_finest_cell(nets):
    net = nets["spread"]
    rng = np.random.default_rng(8)
    # 4096 points in level 0's cell (7, 7, 7): u * 15 in [6.6, 7.4] on every axis; the finer levels spread them
    u = rng.uniform(6.6 / 15, 7.4 / 15, size=(4096, 3))
    pos = (u * 2 - 1).astype(F32)
    _, cs = TV.cells(net.L, pos, 1.0)
    assert len(np.unique(cs[0], axis=0)) == 1 and len(np.unique(cs[15], axis=0)) > 1000
    net.check(net.run(pos), pos)
    # 4096 points in one cell of the finest level (and so of every level): an entry of every hashed level takes 4096 terms
    pos = (F32([0.31, -0.52, 0.13]) + rng.uniform(0, 2e-6, size=(4096, 3)).astype(F32)).astype(F32)
    _, cs = TV.cells(net.L, pos, 1.0)
    assert all(len(np.unique(c, axis=0)) == 1 for c in cs)
    got = net.run(pos)
    assert net.check(got, pos) == (0, 14)
    H = TV.expected_hashed(net.grad0, net.table, net.L, pos, 1.0, WEIGHT)
    assert (H["terms"] == 4096).all() and (np.abs(got[H["entry"]] - net.grad0[H["entry"]]) > 0).any()


def _pos_of_cells(L, l, c):
    """A point whose cell on level l is c (u = c / scale: u * scale + 0.5 sits in the middle of the cell's range)."""
    u = np.asarray(c, np.float64) / float(L["scale"][l])
    pos = (u * 2 - 1).astype(F32).reshape(-1, 3)
    _, cs = TV.cells(L, pos, 1.0)
    assert np.array_equal(cs[l], np.asarray(c, U32).reshape(-1, 3))
    return pos


def _all_cells(L, l):
    r = int(np.floor(float(L["scale"][l])))                                         # cells a point can reach: c <= scale
    a = np.arange(r + 1, dtype=U32)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def test_two_cells_of_a_hashed_level_that_share_an_entry(nets):
    """Searched on the host: level 2 has more cells than entries.  The two points sit in one wave, so the kernel's merge of equal ENTRIES must keep their cells apart."""
    net = nets["spread"]; L = net.L
    l = 2
    c = _all_cells(L, l)
    e = TV.grid_index(L, l, c[:, 0], c[:, 1], c[:, 2])
    order = np.argsort(e, kind="stable")
    k = np.nonzero(e[order][1:] == e[order][:-1])[0][0]
    a, b = c[order[k]], c[order[k + 1]]
    assert e[order[k]] == e[order[k + 1]] and not np.array_equal(a, b)
    pos = _pos_of_cells(L, l, np.stack([a, b]))
    got = net.run(pos)
    net.check(got, pos)
    entry = int(L["offsets"][l]) + int(e[order[k]])
    _, va, _ = TV.cell_values(net.table, L, l, a[None], WEIGHT); _, vb, _ = TV.cell_values(net.table, L, l, b[None], WEIGHT)
    H = TV.expected_hashed(net.grad0, net.table, L, pos, 1.0, WEIGHT)
    allow = H["allow"][list(H["entry"]).index(entry)]
    assert H["terms"][list(H["entry"]).index(entry)] == 2
    # both terms landed: leaving either out misses the result by more than the allowance
    for v in (va[0], vb[0]):
        assert (np.abs(v.astype(np.float64)) > 2 * allow).any()
        assert (np.abs(got[entry].astype(np.float64) - (net.grad0[entry].astype(np.float64) + v)) > allow).any()
    # the same two cells with 31 copies each: merged per cell, never across
    pos = np.repeat(pos, 31, axis=0)
    net.check(net.run(pos), pos)


def test_no_cell_has_a_neighbour_on_its_own_entry(nets):
    """The case "a cell whose neighbour collides with itself" (that neighbour's diff would be 0) does not exist, and the search says why: a level's size is a multiple
    of 8, so an entry keeps the parity of x ^ y * P1 ^ z * P2, and a step of one along any axis flips it (x +- 1 flips bit 0 of x; y * P1 and z * P2 move by an odd
    prime).  Searched on the host over every cell of the first four hashed levels, both sides of every axis; the dense levels are one to one.  What can happen —
    two NEIGHBOURS of a cell on one entry — is part of every case above (the restatement reads the same table)."""
    L = nets["spread"].L
    assert all(int(L["offsets"][l + 1] - L["offsets"][l]) % 8 == 0 for l in range(16)) and TV.P1 % 2 == 1 and TV.P2 % 2 == 1
    for l in TV.hashed_levels(L)[:4]:
        c = _all_cells(L, l)
        c = c[(c > 0).all(axis=1)]
        e = TV.grid_index(L, l, c[:, 0], c[:, 1], c[:, 2])
        for d in range(3):
            for side in (1, -1):
                cc = c.copy(); cc[:, d] = (cc[:, d].astype(np.int64) + side).astype(U32)
                nb = TV.grid_index(L, l, cc[:, 0], cc[:, 1], cc[:, 2])
                assert ((nb ^ e) & 1 == 1).all(), (l, d, side)


def test_bad_points_contribute_nothing(nets):
    net = nets["init"]
    pos = _points(600)
    keep, _ = TV.cells(net.L, pos, 1.0)
    assert 0 < (~keep).sum() < 10 and np.isnan(pos).any() and np.isinf(pos).any()
    got, clean = net.run(pos), net.run(pos[keep])
    dm = TV.level_mask(net.L, TV.dense_levels(net.L))
    assert np.array_equal(_bits(got[dm]), _bits(clean[dm]))
    net.check(got, pos[keep])                                                          # the allowance of the run without them
    only_bad = pos[~keep]
    assert np.array_equal(_bits(net.run(only_bad)), _bits(net.grad0))


def test_dense_levels_do_not_depend_on_order_or_run(nets):
    net = nets["spread"]
    pos = _points(4096, seed=9)
    pos[1000:1600] = pos[1000]                                                          # a crowded cell among the others
    dm = TV.level_mask(net.L, TV.dense_levels(net.L))
    a = net.run(pos)
    b = net.run(pos)
    c = net.run(pos[np.random.default_rng(1).permutation(len(pos))])
    assert np.array_equal(_bits(a[dm]), _bits(b[dm])) and np.array_equal(_bits(a[dm]), _bits(c[dm]))
    net.check(c, pos)


def test_nothing_to_do_leaves_the_gradient(nets):
    from mirres_restir_nerf_mesh_amd import _lib
    from mirres_restir_nerf_mesh_amd._lib import lib, ptr, stream_ptr
    net = nets["init"]; f = net.field
    g = torch.tensor(net.grad0).cuda().clone()
    x = torch.from_numpy(_points(64)).cuda()
    nbytes = int(lib().mirres_grid_tv_workspace_bytes(C.byref(f.net)))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    assert lib().mirres_grid_tv_grad(C.byref(f.net), None, 0, 1.0, WEIGHT, ptr(g), ptr(ws), nbytes, stream_ptr()) == 0
    assert lib().mirres_grid_tv_grad(C.byref(f.net), ptr(x), 64, 1.0, 0.0, ptr(g), ptr(ws), nbytes, stream_ptr()) == 0
    f.grad_total_variation(0.0, x, grad=g)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(net.grad0))
    # the workspace is handed from call to call uninitialised and dirty: the second call of a pair computes what the first did
    ws.fill_(-1)
    g2 = g.clone()
    assert lib().mirres_grid_tv_grad(C.byref(f.net), ptr(x), 64, 1.0, WEIGHT, ptr(g), ptr(ws), nbytes, stream_ptr()) == 0
    net.check(g.cpu().numpy(), _points(64))
    assert lib().mirres_grid_tv_grad(C.byref(f.net), ptr(x), 64, 1.0, WEIGHT, ptr(g2), ptr(ws), nbytes, stream_ptr()) == 0
    dm = TV.level_mask(net.L, TV.dense_levels(net.L))
    assert np.array_equal(_bits(g2.cpu().numpy()[dm]), _bits(g.cpu().numpy()[dm]))
    with pytest.raises(_lib.MirresError, match="mirres_grid_tv_grad"):
        f.grad_total_variation(-1.0, x, grad=g)


def test_four_levels(S0):
    net = Net(S0, 14, 204, True, num_levels=4)
    assert net.L["num_levels"] == 4 and len(TV.dense_levels(net.L)) >= 1
    pos = _points(257)
    net.check(net.run(pos), pos)


def test_python_method_bound_2(S0):
    """bound 2 with points on both sides of the unit box, split as scripts/train_stage0.py does (nerf/utils.py:1152-1158); grad= explicit and table.grad by default;
    the ValueError without a gradient; the random branch on the draws of a seeded generator."""
    net = Net(S0, 14, 205, True, bound=2.0)
    f = net.field
    pos = _points(700, bound=2.0, seed=3)
    x = torch.from_numpy(pos).cuda()
    inner = x.abs().amax(-1) <= 1                                                        # NaN rows compare False: they go with the outer points, and count nowhere
    assert 50 < int(inner.sum()) < 650
    g = torch.tensor(net.grad0).cuda().clone()
    f.grad_total_variation(1e-3, x[inner], grad=g)
    mid = g.cpu().numpy()
    net.check(mid, pos[inner.cpu().numpy()], 1e-3)
    f.grad_total_variation(1e-2, x[~inner], grad=g)
    net.check(g.cpu().numpy(), pos[~inner.cpu().numpy()], 1e-2, grad0=mid)
    # [..., 3] inputs are flattened
    g3 = torch.tensor(net.grad0).cuda().clone()
    f.grad_total_variation(1e-3, x[:600].reshape(20, 30, 3), grad=g3)
    net.check(g3.cpu().numpy(), pos[:600], 1e-3)
    # table.grad by default
    with pytest.raises(ValueError, match="grad is None, should be called after loss.backward"):
        f.grad_total_variation(1e-3, x)
    f.table.requires_grad_(True)
    f.table.grad = torch.tensor(net.grad0).cuda().clone()
    f.grad_total_variation(1e-3, x)
    net.check(f.table.grad.cpu().numpy(), pos, 1e-3)
    # the random branch: B points uniform in [-bound, bound]^3 from the generator
    f.table.grad = torch.tensor(net.grad0).cuda().clone()
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    f.grad_total_variation(1e-3, None, B=3000, generator=gen)
    gen.manual_seed(11)
    drawn = ((torch.rand(3000, 3, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1) * 2.0).cpu().numpy()
    assert np.abs(drawn).max() > 1.5
    net.check(f.table.grad.cpu().numpy(), drawn, 1e-3)
    f.table.grad = torch.tensor(net.grad0).cuda().clone()
    gen.manual_seed(11)
    f.grad_total_variation(1e-3, torch.zeros(0, 3), B=3000, generator=gen)             # empty inputs take the random branch too
    net.check(f.table.grad.cpu().numpy(), drawn, 1e-3)
    with pytest.raises(ValueError):
        f.grad_total_variation(1e-3, x, grad=torch.zeros(3, 2, device="cuda"))
    with pytest.raises(TypeError):
        f.grad_total_variation(1e-3, x, grad=torch.zeros(net.L["total"], 2))           # on the host


def test_one_whole_training_step(S0):
    """render_stage0_train -> backward -> grad_total_variation on the product's own sample points: table.grad = the gradient before the call + the terms."""
    from render_stage0 import orbit_poses
    from mirres_restir_nerf_mesh_amd import harness
    ck = S0.synthetic_radiance_checkpoint(S=32)
    field = S0.RadianceField.from_checkpoint(ck, bound=1.0)
    grid = S0.DensityGrid.from_checkpoint(ck, bound=1.0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    for _ in range(3):
        grid.update(field, noise=torch.rand(grid.cascade, grid.grid_size ** 3, 3, generator=gen, device="cuda"))
    o, d = harness.get_rays(torch.from_numpy(np.asarray(orbit_poses(1)[0], np.float32)).cuda(), (80.0, 80.0, 4.0, 4.0), 8, 8)
    params = field.parameters()
    out = S0.render_stage0_train(field, grid, o, d, bg_color=1.0, perturb=True, noises=torch.rand(64, generator=gen, device="cuda"))
    loss = ((out["image"] - torch.rand(64, 3, generator=gen, device="cuda")) ** 2).mean()
    loss.backward()
    assert out["num_points"] > 64 and tuple(out["xyzs"].shape) == (out["num_points"], 3)
    before = field.table.grad.clone().cpu().numpy()
    table = field.table.detach().cpu().numpy()
    field.grad_total_variation(1e-4, out["xyzs"])
    L = TV.layout(1.0)
    one, more = TV.check(field.table.grad.cpu().numpy(), before, table, L, out["xyzs"].cpu().numpy(), 1.0, 1e-4)
    print("whole step: %d samples, %d hashed entries with one term, %d with more" % (out["num_points"], one, more))
    assert one + more > 0 and np.abs(before).max() > 0


def _train(args, tmp):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_stage0.py"), "--synthetic", "--workspace", str(tmp), "--iters", "160", "--num_rays", "1024",
                        "--window", "20", "--views", "8", "--grid_size", "64"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("[RESULT] first-window")][0].split()
    return r.stdout, float(line[3]), float(line[6])


def test_train_script_with_the_reference_recipe(tmp_path):
    """Run A is the script as it was; run B adds -O --lambda_tv 1e-8 --num_points 65536.  B's last-window loss is at most twice A's: the factor the --synthetic test
    of test_gpu_radiance_bwd.py allows for run-to-run and batch differences; a regulariser of 1e-8 is not expected to move the loss."""
    out_a, first_a, last_a = _train([], tmp_path / "a")
    out_b, first_b, last_b = _train(["-O", "--lambda_tv", "1e-8", "--num_points", "65536"], tmp_path / "b")
    print("run A: first-window %.4e last-window %.4e\nrun B: first-window %.4e last-window %.4e" % (first_a, last_a, first_b, last_b))
    rays = [int(l.split(" rays,")[0].split()[-1]) for l in out_b.splitlines() if " rays," in l]
    print("run B ray counts per window:", rays)
    assert len(rays) == 8 and any(r != 1024 for r in rays), rays
    assert "mark_untrained" in out_b and "held-out PSNR" in out_b
    assert all(int(l.split(" rays,")[0].split()[-1]) == 1024 for l in out_a.splitlines() if " rays," in l)
    assert last_b < first_b
    assert last_b <= 2.0 * last_a, (last_a, last_b)
