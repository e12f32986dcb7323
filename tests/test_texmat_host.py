"""CPU: the stage-1 asset loader (export.load_stage1) against files written by the exporter's own writers (write_obj, meters.write_png), JPEG input, refusals,
and a self-check of the numpy lookup rule of tests/texmat_refs.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texmat_refs as R


@pytest.fixture(scope="module")
def EX():
    from mirres_restir_nerf_mesh_amd import export
    return export


def _asset(EX, path, sizes, seed=0, ext=".png"):
    """One cascade per (H, W) in `sizes`: a small random triangle mesh with random per-corner UVs and random textures."""
    from mirres_restir_nerf_mesh_amd import meters
    from PIL import Image
    rng = np.random.default_rng(seed)
    cas = []
    for c, (H, W) in enumerate(sizes):
        nv, nt, nf = 7 + 3 * c, 9 + 2 * c, 5 + c
        v = rng.uniform(-1, 1, (nv, 3)).astype(np.float32)
        vt = rng.uniform(0, 1, (nt, 2)).astype(np.float32)
        f = rng.integers(0, nv, (nf, 3)).astype(np.int32); ft = rng.integers(0, nt, (nf, 3)).astype(np.int32)
        t0 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8); t1 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        EX.write_obj(os.path.join(path, "mesh_%d.obj" % c), v, vt, f, ft, c)
        EX.write_mtl(os.path.join(path, "mesh_%d.mtl" % c), c)
        for k, t in ((0, t0), (1, t1)):
            if ext == ".png":
                meters.write_png(os.path.join(path, "feat%d_%d.png" % (k, c)), t)
            else:
                Image.fromarray(t).save(os.path.join(path, "feat%d_%d%s" % (k, c, ext)), quality=95)
        cas.append((v, vt, f, ft, t0, t1))
    return cas


@pytest.mark.parametrize("sizes", [[(24, 40)], [(24, 40), (16, 8)]])
def test_round_trip(EX, tmp_path, sizes):
    cas = _asset(EX, str(tmp_path), sizes)
    m = EX.load_stage1(str(tmp_path), device="cpu")
    assert m.n_cas == len(sizes)
    nv = nt = nf = 0
    for c, (v, vt, f, ft, t0, t1) in enumerate(cas):
        _, vt_file, _, _ = EX.read_obj(str(tmp_path / ("mesh_%d.obj" % c)))
        assert np.array_equal(m.verts[nv:nv + v.shape[0]].numpy(), v)
        assert np.array_equal(m.tris[nf:nf + f.shape[0]].numpy(), f + nv), "cascade offsets"
        assert np.array_equal(m.ft[nf:nf + f.shape[0]].numpy(), ft + nt)
        want_vt, want_ft = EX.uv_from_obj(str(tmp_path / ("mesh_%d.obj" % c)))
        assert np.array_equal(m.vt[nt:nt + vt.shape[0]].numpy(), want_vt) and np.array_equal(want_ft, ft)
        assert np.abs(want_vt - vt).max() <= 1e-7, "v flip: the file holds 1 - v"
        assert np.array_equal(vt_file[:, 1], np.float32(1) - vt[:, 1]) or np.abs(vt_file[:, 1] - (1 - vt[:, 1])).max() <= 1e-7
        pl = m.planes[c].numpy()
        assert pl.shape == sizes[c] + (8,)
        assert np.array_equal(pl, R.pack_planes(t0, t1))
        nv += v.shape[0]; nt += vt.shape[0]; nf += f.shape[0]
        assert m.tri_end[c] == nf
    st = m._struct()
    assert st.n_cas == len(sizes) and [st.W[c] for c in range(len(sizes))] == [s[1] for s in sizes]
    assert abs(st.rough_min - 0.08) < 1e-7
    assert np.abs(m.decode.numpy() - R.srgb_decode_table()).max() <= 1e-7 and m.decode[0] == 0 and m.decode[255] == 1


def test_jpeg_input(EX, tmp_path):
    from PIL import Image
    _asset(EX, str(tmp_path), [(32, 48)], seed=3, ext=".jpg")
    m = EX.load_stage1(str(tmp_path), device="cpu")
    t0 = np.asarray(Image.open(tmp_path / "feat0_0.jpg").convert("RGB")); t1 = np.asarray(Image.open(tmp_path / "feat1_0.jpg").convert("RGB"))
    assert np.array_equal(m.planes[0].numpy(), R.pack_planes(t0, t1))


def test_bad_inputs_are_refused(EX, tmp_path):
    with pytest.raises(FileNotFoundError):
        EX.load_stage1(str(tmp_path / "nothing"), device="cpu")
    d = tmp_path / "a"; d.mkdir(); _asset(EX, str(d), [(8, 8)])
    with pytest.raises(FileNotFoundError, match="mesh_1"):
        EX.load_stage1(str(d), cascades=2, device="cpu")
    os.remove(d / "feat1_0.png")
    with pytest.raises(FileNotFoundError, match="feat1_0"):
        EX.load_stage1(str(d), device="cpu")
    d = tmp_path / "b"; d.mkdir(); _asset(EX, str(d), [(8, 8)])
    from mirres_restir_nerf_mesh_amd import meters
    meters.write_png(str(d / "feat1_0.png"), np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(ValueError, match="one size"):
        EX.load_stage1(str(d), device="cpu")
    d = tmp_path / "c"; d.mkdir(); _asset(EX, str(d), [(8, 8)])
    txt = open(d / "mesh_0.obj").read().splitlines()
    txt = [("f " + " ".join(q.split("/")[0] for q in l.split()[1:])) if l.startswith("f ") else l for l in txt]
    open(d / "mesh_0.obj", "w").write("\n".join(txt) + "\n")
    with pytest.raises(ValueError, match="without texture coordinates"):
        EX.load_stage1(str(d), device="cpu")


def test_refs_texel_centre_returns_the_texel():
    """On the triangle (0,0,0) (1,0,0) (0,1,0) with uv = (x, y) the fp32 formula gives uv = (x, y) exactly; at a texel centre of a power-of-two plane the
    filter weights are exactly 0 and the lookup is the decoded texel itself, in both cascades."""
    rng = np.random.default_rng(1)
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    vt = np.array([[0, 0], [1, 0], [0, 1]], np.float32); ft = np.array([[0, 1, 2], [0, 1, 2]], np.int32)
    planes = [rng.integers(0, 256, (16, 32, 8), dtype=np.uint8), rng.integers(0, 256, (64, 8, 8), dtype=np.uint8)]
    decode = R.srgb_decode_table()
    for c, pl in enumerate(planes):
        H, W = pl.shape[:2]
        jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        u = ((ii + 0.5) / W).ravel().astype(np.float32); v = ((jj + 0.5) / H).ravel().astype(np.float32)
        keep = u + v <= 1
        pos = np.stack((u[keep], v[keep], np.zeros(keep.sum(), np.float32)), 1)
        prim = np.full(pos.shape[0], c, np.int64)
        out = R.sample(verts, tris, vt, ft, [1, 2], planes, decode, 0.0, prim, pos)
        want = decode[pl[jj.ravel()[keep], ii.ravel()[keep], :5]]
        assert np.array_equal(out, want)
