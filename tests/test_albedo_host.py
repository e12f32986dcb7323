"""Host side of the albedo evaluation (no GPU): the OpenEXR reader on the files the TensoIR ground truth comes in (ZIP / ZIPS, HALF / FLOAT; written
here with zlib and struct), the script-variant SSIM against the formulas of the reference's albedo_eval.py:18-63 stated in float64 numpy, the scale
file, and the argument handling of scripts/evaluate.py."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from mirres_restir_nerf_mesh_amd import albedo, meters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ZIPS, ZIP, PIZ = 0, 2, 3, 4


def _exr_pack(raw):
    """The format's ZIP coding of one chunk: byte de-interleave (even positions first), differences biased by 128, deflate."""
    t = np.frombuffer(raw, np.uint8)
    t = np.concatenate([t[0::2], t[1::2]]).astype(np.int64)
    d = t.copy(); d[1:] = (t[1:] - t[:-1] + 128 + 256) & 255
    return zlib.compress(d.astype(np.uint8).tobytes(), 6)


def _write_exr(path, img, names, types, compression, force_raw_chunk=None):
    """img [H, W, C] float32, channel k named names[k] with pixel type types[k] (1 HALF, 2 FLOAT).  Channels are stored in alphabetical order, per scan line."""
    h, w, c = img.shape
    order = sorted(range(c), key=lambda k: names[k])
    attr = lambda name, typ, data: name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data
    chlist = b"".join(names[k].encode() + b"\0" + struct.pack("<iBBBBii", types[k], 0, 0, 0, 0, 1, 1) for k in order) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    head = (struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", chlist) + attr("compression", "compression", bytes([compression]))
            + attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0")
            + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
            + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    lines = {NONE: 1, ZIPS: 1, ZIP: 16, PIZ: 32}[compression]
    chunks = []
    for y0 in range(0, h, lines):
        raw = b"".join(img[y, :, k].astype("<f2" if types[k] == 1 else "<f4").tobytes() for y in range(y0, min(h, y0 + lines)) for k in order)
        data = raw
        if compression in (ZIPS, ZIP) and force_raw_chunk != len(chunks):
            z = _exr_pack(raw)
            data = z if len(z) < len(raw) else raw               # the format stores a chunk that does not shrink as it is
        chunks.append(struct.pack("<ii", y0, len(data)) + data)
    at = len(head) + 8 * len(chunks)
    offs = []
    for ch in chunks:
        offs.append(at); at += len(ch)
    with open(path, "wb") as f:
        f.write(head + struct.pack("<%dQ" % len(offs), *offs) + b"".join(chunks))


def _image(rng, h, w, c, half):
    img = rng.random((h, w, c)).astype(np.float32)
    img[: h // 2, : w // 2] = 0.25                               # a flat region: the deflate stage has something to shrink
    img[0, 0] = [-0.0, 1.0, 3.5e-5, 60000.0][:c]
    return img.astype(np.float16).astype(np.float32) if half else img


@pytest.mark.parametrize("compression", [NONE, ZIPS, ZIP])
@pytest.mark.parametrize("half", [False, True])
def test_read_exr_zip_zips_half_float(tmp_path, compression, half):
    rng = np.random.default_rng(11 + compression)
    for h, w in ((37, 13), (16, 5), (1, 1), (50, 31)):           # odd widths, heights that are no multiple of the 16-line ZIP chunk
        img = _image(rng, h, w, 4, half)
        p = str(tmp_path / ("a_%d_%d.exr" % (h, w)))
        _write_exr(p, img, ["R", "G", "B", "A"], [1 if half else 2] * 4, compression)       # stored as A, B, G, R
        got = meters.read_exr(p)
        assert got.dtype == np.float32 and got.shape == img.shape
        assert np.array_equal(got.view(np.uint32), img.view(np.uint32))


def test_read_exr_mixed_types_grey_and_raw_chunks(tmp_path):
    rng = np.random.default_rng(3)
    img = _image(rng, 40, 9, 4, True)
    p = str(tmp_path / "mixed.exr")
    _write_exr(p, img, ["R", "G", "B", "A"], [1, 2, 1, 2], ZIP, force_raw_chunk=1)          # HALF and FLOAT channels in one file; the second chunk stored raw
    assert np.array_equal(meters.read_exr(p), img)
    noise = rng.random((20, 7, 3)).astype(np.float32)                                       # incompressible FLOAT noise: deflate may not shrink it
    _write_exr(p, noise, ["R", "G", "B"], [2, 2, 2], ZIPS)
    assert np.array_equal(meters.read_exr(p), noise)
    y = rng.random((18, 3, 1)).astype(np.float32)
    _write_exr(p, y, ["Y"], [2], ZIP)
    assert np.array_equal(meters.read_exr(p), y)


def test_read_exr_refuses_other_compressions_by_name(tmp_path):
    p = str(tmp_path / "piz.exr")
    _write_exr(p, np.zeros((4, 4, 3), np.float32), ["R", "G", "B"], [2, 2, 2], PIZ)
    with pytest.raises(ValueError, match="PIZ"):
        meters.read_exr(p)
    _write_exr(p, np.zeros((4, 4, 3), np.float32), ["R", "G", "B"], [0, 2, 2], NONE)        # a UINT channel
    with pytest.raises(ValueError, match="HALF nor FLOAT"):
        meters.read_exr(p)


def test_read_exr_still_reads_write_exr(tmp_path):
    rng = np.random.default_rng(4)
    for c in (1, 3, 4):
        img = rng.standard_normal((21, 10, c)).astype(np.float32)
        p = meters.write_exr(str(tmp_path / ("w%d.exr" % c)), img)
        assert np.array_equal(meters.read_exr(p), img)


# ------------------------------------------------------------------------------------------------ rgb_ssim (albedo_eval.py:18-63) in float64 numpy
def _valid_conv(z, f, axis):
    """scipy.signal.convolve2d(z, f, mode='valid') for a 1-D filter along `axis`: out[i] = sum_k f[k] z[i + K - 1 - k]."""
    K = f.size
    n = z.shape[axis] - K + 1
    out = np.zeros([n if a == axis else s for a, s in enumerate(z.shape)], np.float64)
    for k in range(K):
        sl = [slice(None)] * z.ndim
        sl[axis] = slice(K - 1 - k, K - 1 - k + n)
        out += f[k] * z[tuple(sl)]
    return out


def _rgb_ssim(x, y, max_val, taps=11, sigma=1.5, k1=0.01, k2=0.03):
    """The script's SSIM, formula by formula, in float64: Gaussian window (offsets -5 .. 5 for 11 taps) normalised to sum 1; local means, second moments
    and the cross moment by the separable VALID blur; variances max(0, E[x^2] - mu^2); covariance limited in magnitude to sqrt(var_x var_y), sign kept;
    SSIM map ((2 mu_x mu_y + c1) (2 cov + c2)) / ((mu_x^2 + mu_y^2 + c1) (var_x + var_y + c2)), mean over positions and channels."""
    half = taps // 2
    offs = np.arange(taps) - half + (2 * half - taps + 1) / 2
    win = np.exp(-0.5 * (offs / sigma) ** 2); win = win / win.sum()
    blur = lambda z: _valid_conv(_valid_conv(z, win, 0), win, 1)                              # [H, W, 3] -> [H - 10, W - 10, 3]
    mx, my = blur(x), blur(y)
    vx = np.maximum(0.0, blur(x * x) - mx * mx); vy = np.maximum(0.0, blur(y * y) - my * my)
    cxy = blur(x * y) - mx * my
    cxy = np.sign(cxy) * np.minimum(np.sqrt(vx * vy), np.abs(cxy))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return float(np.mean((2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))))


def test_script_ssim_against_its_float64_statement():
    rng = np.random.default_rng(21)
    a = rng.random((40, 33, 3)).astype(np.float32)
    pairs = [(a, np.clip(a + 0.08 * rng.standard_normal(a.shape), 0, 1).astype(np.float32)),
             (a, a.copy()),                                                                       # identical: 1
             (np.full((25, 30, 3), 0.37, np.float32), rng.random((25, 30, 3)).astype(np.float32)),   # a constant image: its variance clamps at 0
             (rng.random((30, 12, 3)).astype(np.float32), (1 - rng.random((30, 12, 3))).astype(np.float32))]
    for k, (x, y) in enumerate(pairs):
        want = _rgb_ssim(x.astype(np.float64), y.astype(np.float64), 1.0)
        got = float(meters.ssim_script(torch.from_numpy(x), torch.from_numpy(y), 1.0))
        print("pair %d: ssim_script %.9f, float64 statement %.9f" % (k, got, want))
        assert abs(got - want) < 2e-5
    assert abs(float(meters.ssim_script(torch.from_numpy(a), torch.from_numpy(a))) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        meters.ssim_script(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3))


# ------------------------------------------------------------------------------------------------ scale file, evaluate.py's arguments
def test_scale_file_round_trip_is_exact(tmp_path):
    rng = np.random.default_rng(8)
    for k in range(20):
        s = tuple(float(x) for x in np.exp(rng.uniform(-14, 14, 3)) * (1 + rng.random(3)))
        if k == 0:
            s = (0.1, 1.0 / 3.0, 5e-324)
        p = albedo.write_scale(str(tmp_path / "albedo_scale.json"), s, 12345678901, 0.9)
        d = albedo.read_scale(p)
        assert d["scale"] == s and d["n_pixels"] == 12345678901 and d["mask_thr"] == 0.9
    (tmp_path / "other.json").write_text("{}")
    with pytest.raises(ValueError):
        albedo.read_scale(str(tmp_path / "other.json"))


def test_scratch_size_of_the_library_is_the_header_s():
    """The bindings size the kernels' scratch buffer by the loaded library's own answer, and that answer is the header's #define."""
    import re
    from mirres_restir_nerf_mesh_amd import _lib
    src = open(os.path.join(ROOT, "include", "mirres.h")).read()
    (define,) = re.findall(r"#define\s+MIRRES_ALBEDO_SCRATCH_BYTES\s+(\d+)", src)
    assert int(_lib.lib().mirres_albedo_scratch_bytes()) == int(define) >= 3 * 264 * 8


def _evaluate_module():
    spec = importlib.util.spec_from_file_location("mirres_evaluate_script", os.path.join(ROOT, "scripts", "evaluate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_evaluate_scale_arguments(tmp_path, capsys):
    ev = _evaluate_module()
    s = (0.7123456789012345, 1.3, 0.9000000000000001)
    f = albedo.write_scale(str(tmp_path / "albedo_scale.json"), s, 10, 0.9)
    typed, _ = ev.parse_args(["--albedo_scale_x", repr(s[0]), "--albedo_scale_y", repr(s[1]), "--albedo_scale_z", repr(s[2])])
    filed, _ = ev.parse_args(["--albedo_scale_file", f, "--envmap_path", "sky.hdr"])
    tup = lambda a: (a.albedo_scale_x, a.albedo_scale_y, a.albedo_scale_z)
    assert tup(filed) == tup(typed) == s
    none, _ = ev.parse_args([])
    assert tup(none) == (1.0, 1.0, 1.0) and none.exposure is None
    for extra in (["--albedo_scale_x", "1.0"], ["--albedo_scale_z", "0.5"]):                 # even a typed 1.0 is a second source
        with pytest.raises(SystemExit):
            ev.parse_args(["--albedo_scale_file", f, "--envmap_path", "sky.hdr"] + extra)
        assert "albedo_scale_file" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                                          # the file without relighting would be read and ignored
        ev.parse_args(["--albedo_scale_file", f])
    assert "envmap_path" in capsys.readouterr().err
    hdr, _ = ev.parse_args(["--use_hdr", "--exposure", "-1.5"])
    assert hdr.exposure == -1.5
    off, _ = ev.parse_args(["--exposure", "3"])                                              # --exposure is read with --use_hdr only (nerf/renderer.py:1125)
    assert off.exposure is None
