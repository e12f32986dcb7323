"""torch-ngp's encoders as stand-alone modules on the HIP path: what `from encoding import get_encoder` yields in the reference (encoding.py:71-107;
nerf/network.py:77, 98), with its constructor arguments, attribute names and state_dict keys.

    encoder, dim = get_encoder("hashgrid", desired_resolution=2048 * bound)      # GridEncoder (gridencoder/grid.py:102-192) on csrc/gridenc.hip
    encoder_dir, dim = get_encoder("sh")                                         # SHEncoder (shencoder/sphere_harmonics.py:61-90) on mirres_sh_encode
    feat = encoder(x, bound=bound)                                               # [..., num_levels * level_dim], differentiable in encoder.embeddings and in x

GridEncoder: input_dim 2 or 3, level_dim 1, 2, 4 or 8, 1 .. 16 levels, gridtype 'hash' / 'tiled', align_corners, 'linear' / 'smoothstep'.  For the reference's own
configuration (3, 16 levels of 2, base 16, 2^19, hash, align_corners False, linear) the features have DensityField.encode's bits: the fused kernels of stage0 stay the
fast path and the two check each other.

Deviations from the reference: everything is fp32 — under autocast or with half tensors the modules compute and return fp32 (the reference
casts the table to half for even level_dim); the map to [0, 1] is done in the kernel by an IEEE division; the gradients are once differentiable; SH degrees above 4
and tiny-cuda-nn's encoders are not built; a direction never gets a gradient; FreqEncoder is plain torch."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check, ptr, stream_ptr

__all__ = ["GridEncoder", "SHEncoder", "FreqEncoder", "get_encoder", "gridenc_layout"]

GRIDTYPE_IDS = {"hash": 0, "tiled": 1}
INTERPOLATION_IDS = {"linear": 0, "smoothstep": 1}


def gridenc_layout(input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19, gridtype="hash", align_corners=False,
                   interpolation="linear"):
    """GridEncoder.__init__'s level table and the kernels' per-level quantities -> (_lib.GridEnc, total entries).  No device is touched."""
    if gridtype not in GRIDTYPE_IDS:
        raise KeyError("gridtype %r: 'hash' or 'tiled'" % (gridtype,))
    if interpolation not in INTERPOLATION_IDS:
        raise KeyError("interpolation %r: 'linear' or 'smoothstep'" % (interpolation,))
    g = _lib.GridEnc()
    total = int(lib().mirres_gridenc_layout(int(input_dim), int(level_dim), int(num_levels), float(per_level_scale), int(base_resolution), int(log2_hashmap_size),
                                            GRIDTYPE_IDS[gridtype], int(bool(align_corners)), INTERPOLATION_IDS[interpolation], C.byref(g)))
    if total < 0:
        check(total, "mirres_gridenc_layout")
    return g, total


def _f32_aligned(t, device=None):
    """A contiguous fp32 tensor whose storage starts at a multiple of 16 bytes (the kernels read and write entries with vector accesses)."""
    t = t.to(device=device, dtype=torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _grid_encode(torch.autograd.Function):
    """forward keeps inputs and embeddings alone; the backward recomputes the cells (nothing is taped).  inputs and embeddings are on one device (GridEncoder.forward
    refuses anything else), so every gradient comes back on the device of the tensor it belongs to."""

    @staticmethod
    def forward(ctx, inputs, embeddings, enc, bound, max_level):
        # inputs [B, D] in [-bound, bound], embeddings [entries, C] -> [B, L * C]
        x = _f32_aligned(inputs.detach())
        table = _f32_aligned(embeddings.detach())
        n = int(x.shape[0])
        out = torch.empty((n, enc.output_dim), dtype=torch.float32, device=table.device)
        with torch.cuda.device(table.device):
            check(lib().mirres_grid_encode_fwd(C.byref(enc._layout), ptr(table), ptr(x) if n else None, n, bound, max_level, ptr(out) if n else None, stream_ptr()),
                  "mirres_grid_encode_fwd")
        ctx.save_for_backward(x, embeddings)
        ctx.enc, ctx.bound, ctx.max_level = enc, bound, max_level
        ctx.in_dtype = inputs.dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, embeddings = ctx.saved_tensors
        enc = ctx.enc
        n = int(x.shape[0])
        table = _f32_aligned(embeddings.detach())
        grad = _f32_aligned(grad, table.device)
        grad_table = torch.zeros(table.shape, dtype=torch.float32, device=table.device) if ctx.needs_input_grad[1] else None
        grad_x = torch.empty((n, enc.input_dim), dtype=torch.float32, device=table.device) if ctx.needs_input_grad[0] else None
        if n and (grad_table is not None or grad_x is not None):
            with torch.cuda.device(table.device):
                check(lib().mirres_grid_encode_bwd(C.byref(enc._layout), ptr(table), ptr(x), n, ctx.bound, ctx.max_level, ptr(grad), ptr(grad_table), ptr(grad_x),
                                                   stream_ptr()), "mirres_grid_encode_bwd")
        if grad_x is not None:
            grad_x = grad_x.to(ctx.in_dtype)
        if grad_table is not None:
            grad_table = grad_table.to(embeddings.dtype)
        return grad_x, grad_table, None, None, None


class GridEncoder(nn.Module):
    """The multi-resolution grid encoder with the reference's interface (gridencoder/grid.py:102-192) on csrc/gridenc.hip: parameter `embeddings` f32
    [entries, level_dim], buffer `offsets` i32 [num_levels + 1]; a reference checkpoint's encoder.embeddings / encoder.offsets load with load_state_dict.  The level
    table comes from mirres_gridenc_layout; the kernels read that layout, never the `offsets` buffer, which is kept for the state dict and checked when one is loaded."""

    INIT_RANGE = 1e-4          # the table starts uniform in (-INIT_RANGE, INIT_RANGE), as the reference's

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=None, gridtype="hash",
                 align_corners=False, interpolation="linear"):
        super().__init__()
        if desired_resolution is not None and num_levels > 1:
            # the geometric progression from base_resolution that ends at desired_resolution on the last level, computed in numpy doubles as the reference does
            # (the layout's bits depend on it); with one level there is nothing to scale and per_level_scale keeps its argument
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))
        self._layout, entries = gridenc_layout(input_dim, num_levels, level_dim, per_level_scale, base_resolution, log2_hashmap_size, gridtype, align_corners, interpolation)
        self._offsets_host = tuple(int(self._layout.offsets[i]) for i in range(num_levels + 1))
        # the reference's attribute names: its network, trainer and checkpoint code read them
        self.input_dim, self.num_levels, self.level_dim = input_dim, num_levels, level_dim
        self.per_level_scale, self.base_resolution, self.log2_hashmap_size = per_level_scale, base_resolution, log2_hashmap_size
        self.gridtype, self.gridtype_id = gridtype, GRIDTYPE_IDS[gridtype]
        self.interpolation, self.interp_id = interpolation, INTERPOLATION_IDS[interpolation]
        self.align_corners = align_corners
        self.output_dim = num_levels * level_dim
        self.max_params = 1 << log2_hashmap_size
        self.n_params = entries * level_dim
        self.register_buffer("offsets", torch.tensor(self._offsets_host, dtype=torch.int32))
        self.embeddings = nn.Parameter(torch.empty(entries, level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.embeddings.uniform_(-self.INIT_RANGE, self.INIT_RANGE)

    def extra_repr(self):
        finest = self.base_resolution * float(self.per_level_scale) ** (self.num_levels - 1)
        return ("input_dim=%d, levels=%d x %d features, resolution %d .. %.0f (x%.4f per level), table=%s, %s, align_corners=%s, %s"
                % (self.input_dim, self.num_levels, self.level_dim, self.base_resolution, finest, float(self.per_level_scale), tuple(self.embeddings.shape), self.gridtype,
                   self.align_corners, self.interpolation))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A state dict whose offsets are another configuration's is refused here, once, instead of being compared on every forward."""
        got = state_dict.get(prefix + "offsets")
        if got is not None and tuple(int(o) for o in torch.as_tensor(got).reshape(-1).tolist()) != self._offsets_host:
            error_msgs.append("GridEncoder: the state dict's %soffsets (%d levels, %d entries) are not this encoder's layout (%d levels, %d entries): a checkpoint of "
                              "another configuration or --bound" % (prefix, got.numel() - 1, int(got.reshape(-1)[-1]) if got.numel() else 0, self.num_levels,
                                                                     self._offsets_host[-1]))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _check_table(self):
        """Shapes alone: nothing is read from the device (no synchronisation per forward; usable under graph capture)."""
        if tuple(self.embeddings.shape) != (self._offsets_host[-1], self.level_dim) or tuple(self.offsets.shape) != (self.num_levels + 1,):
            raise ValueError("GridEncoder: embeddings of %s and offsets of %s do not fit this encoder's layout ([%d, %d] and [%d])"
                             % (tuple(self.embeddings.shape), tuple(self.offsets.shape), self._offsets_host[-1], self.level_dim, self.num_levels + 1))

    def forward(self, inputs, bound=1, max_level=None):
        """inputs [..., input_dim] in [-bound, bound], on the embeddings' device -> f32 [..., num_levels * level_dim]; max_level: only the first max_level levels, the
        others 0.  A point out of bounds (or not finite) has zero features and a zero gradient.  The input's gradient is computed only when inputs.requires_grad."""
        if inputs.shape[-1] != self.input_dim:
            raise ValueError("GridEncoder: inputs of %s, the last dimension must be input_dim = %d" % (tuple(inputs.shape), self.input_dim))
        if not self.embeddings.is_cuda:
            raise _lib.MirresError("GridEncoder: the embeddings are on %s; the encoder runs on the GPU only (there is no CPU fallback)" % self.embeddings.device)
        if inputs.device != self.embeddings.device:
            raise ValueError("GridEncoder: inputs on %s, embeddings on %s: move the inputs to the encoder's device" % (inputs.device, self.embeddings.device))
        bound = float(bound)
        if not (bound > 0 and np.isfinite(bound)):
            raise ValueError("GridEncoder: bound %r" % (bound,))
        self._check_table()
        ml = self.num_levels if max_level is None else min(int(max_level), self.num_levels)
        if ml < 0:
            raise ValueError("GridEncoder: max_level %r is negative" % (max_level,))
        outputs = _grid_encode.apply(inputs.reshape(-1, self.input_dim), self.embeddings, self, bound, ml)
        return outputs.view(*inputs.shape[:-1], self.output_dim)

    @torch.no_grad()
    def grad_total_variation(self, weight=1e-7, inputs=None, bound=1, B=1000000):
        """GridEncoder.grad_total_variation (grid.py:170-192) through mirres_grid_tv_grad, as DensityField.grad_total_variation: adds the regulariser's gradient to
        self.embeddings.grad in place.  Built for input_dim 3, level_dim 2, 'hash', align_corners False (csrc/grid_tv.hip); any other configuration raises."""
        if self.input_dim != 3 or self.level_dim != 2 or self.gridtype != "hash" or self.align_corners:
            raise NotImplementedError("grad_total_variation is built for input_dim=3, level_dim=2, gridtype='hash', align_corners=False; this encoder has input_dim=%d, "
                                      "level_dim=%d, gridtype=%r, align_corners=%s" % (self.input_dim, self.level_dim, self.gridtype, self.align_corners))
        grad = self.embeddings.grad
        if grad is None:
            raise ValueError("grad is None, should be called after loss.backward() and before optimizer.step()!")
        if grad.dtype != torch.float32 or not grad.is_cuda or not grad.is_contiguous():
            raise TypeError("grad_total_variation: embeddings.grad must be a contiguous fp32 device tensor, got %s on %s" % (grad.dtype, grad.device))
        self._check_table()
        bound = float(bound)
        dev = grad.device
        if inputs is None or inputs.numel() == 0:
            x = (torch.rand(int(B), 3, dtype=torch.float32, device=dev) * 2 - 1) * bound      # the reference's random branch draws u in [0, 1]: the same points
        else:
            x = inputs.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        n = int(x.shape[0])
        net = _lib.DensityNet()
        net.num_levels = self.num_levels
        for i in range(self.num_levels + 1):
            net.offsets[i] = self._layout.offsets[i]
        for i in range(self.num_levels + 1, 17):
            net.offsets[i] = self._layout.offsets[self.num_levels]
        for i in range(self.num_levels):
            net.resolution[i], net.hashed[i], net.scale[i] = self._layout.resolution[i], self._layout.hashed[i], self._layout.scale[i]
        table = self.embeddings.detach()
        if table.dtype != torch.float32 or not table.is_contiguous() or table.device != dev:
            raise TypeError("grad_total_variation: the embeddings must be contiguous fp32 on the gradient's device")
        net.table = table.data_ptr()
        L = lib()
        with torch.cuda.device(dev):
            nbytes = int(L.mirres_grid_tv_workspace_bytes(C.byref(net)))
            if nbytes < 0:
                check(nbytes, "mirres_grid_tv_workspace_bytes")
            ws = getattr(self, "_tv_workspace", None)
            if ws is None or ws.device != dev or ws.numel() * 4 < nbytes:
                ws = self._tv_workspace = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
            check(L.mirres_grid_tv_grad(C.byref(net), ptr(x) if n else None, n, bound, float(weight), ptr(grad), ptr(ws), ws.numel() * 4, stream_ptr()),
                  "mirres_grid_tv_grad")
        return None


class SHEncoder(nn.Module):
    """shencoder.SHEncoder (shencoder/sphere_harmonics.py:61-90): the first degree^2 columns of mirres_sh_encode (csrc/radiance.hip), RadianceField.sh's bits.
    Degrees 1 .. 4; the direction is normalised inside the kernel (`size` scales it and so changes nothing but the rounding of that division)."""

    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = degree ** 2
        if self.input_dim != 3:
            raise ValueError("SHEncoder: input_dim %r; spherical harmonics take a 3-vector" % (input_dim,))
        if not (isinstance(degree, (int, np.integer)) and 1 <= degree <= 8):
            raise ValueError("SHEncoder: degree %r; the reference knows 1 .. 8, of which 1 .. 4 are built here" % (degree,))
        if degree > 4:
            raise NotImplementedError("SHEncoder: degree %d is not built on the HIP path; degrees 1 .. 4 are (the reference's network uses 4)" % degree)

    def extra_repr(self):
        return "degree=%d, output_dim=%d" % (self.degree, self.output_dim)

    def forward(self, inputs, size=1):
        if inputs.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("SHEncoder: the input requires grad; a direction never gets a gradient on this path (nothing in the reference differentiates one)")
        if inputs.shape[-1] != 3:
            raise ValueError("SHEncoder: inputs of %s, expected [..., 3]" % (tuple(inputs.shape),))
        if not inputs.is_cuda:
            raise _lib.MirresError("SHEncoder: the input is on %s; the encoder runs on the GPU only (there is no CPU fallback)" % inputs.device)
        d = inputs.detach().to(torch.float32)
        if size != 1:
            d = d / size
        d = d.reshape(-1, 3).contiguous()
        n = int(d.shape[0])
        out = torch.empty((n, 16), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            check(lib().mirres_sh_encode(ptr(d) if n else None, n, ptr(out) if n else None, stream_ptr()), "mirres_sh_encode")
        if self.output_dim != 16:
            out = out[:, :self.output_dim].contiguous()
        return out.reshape(*inputs.shape[:-1], self.output_dim)


class FreqEncoder(nn.Module):
    """The frequency (positional) encoding in plain torch, with freqencoder.FreqEncoder's interface and column order (freqencoder/freq.py:55-77): the input, then per
    octave k = 0 .. degree - 1 a block sin(2^k x) and a block cos(2^k x), each input_dim wide.  Nothing in the reference's network uses it."""

    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = input_dim * (1 + 2 * degree)

    def extra_repr(self):
        return "input_dim=%d, degree=%d, output_dim=%d" % (self.input_dim, self.degree, self.output_dim)

    def forward(self, inputs, **kwargs):
        x = inputs.to(torch.float32)
        octaves = [x * float(1 << k) for k in range(self.degree)]
        return torch.cat([x] + [fn(o) for o in octaves for fn in (torch.sin, torch.cos)], dim=-1)


def _identity(x, **kwargs):
    return x


def _make_grid(gridtype):
    return lambda a: GridEncoder(input_dim=a["input_dim"], num_levels=a["num_levels"], level_dim=a["level_dim"], base_resolution=a["base_resolution"],
                                 log2_hashmap_size=a["log2_hashmap_size"], desired_resolution=a["desired_resolution"], gridtype=gridtype,
                                 align_corners=a["align_corners"], interpolation=a["interpolation"])


# encoding name -> constructor from get_encoder's arguments.  'frequency_torch' (the reference's torch class with log sampling and the input included) has
# FreqEncoder's output, so both names give FreqEncoder.
_ENCODERS = {
    "frequency": lambda a: FreqEncoder(input_dim=a["input_dim"], degree=a["multires"]),
    "frequency_torch": lambda a: FreqEncoder(input_dim=a["input_dim"], degree=a["multires"]),
    "sh": lambda a: SHEncoder(input_dim=a["input_dim"], degree=a["degree"]),
    "hashgrid": _make_grid("hash"),
    "tiledgrid": _make_grid("tiled"),
}


def get_encoder(encoding, input_dim=3, output_dim=1, resolution=300, mode='bilinear', multires=6, degree=4, num_levels=16, level_dim=2, base_resolution=16,
                log2_hashmap_size=19, desired_resolution=2048, align_corners=False, interpolation='linear', **kwargs):
    """The reference's factory (encoding.py:71-107), same signature -> (encoder, output_dim).  output_dim, resolution and mode belong to a dense-grid encoder the
    reference does not have either and are ignored; multires is the frequency encoders' degree; 'None' is the identity; 'hashgrid_tcnn' is refused."""
    if encoding == "None":
        return _identity, input_dim
    if encoding == "hashgrid_tcnn":
        raise NotImplementedError("get_encoder('hashgrid_tcnn'): tiny-cuda-nn's encoder is not built on the HIP path; use 'hashgrid'")
    if encoding not in _ENCODERS:
        raise NotImplementedError("get_encoder: unknown encoding %r; built: 'None', %s" % (encoding, ", ".join(repr(k) for k in _ENCODERS)))
    encoder = _ENCODERS[encoding](dict(input_dim=input_dim, multires=multires, degree=degree, num_levels=num_levels, level_dim=level_dim, base_resolution=base_resolution,
                                       log2_hashmap_size=log2_hashmap_size, desired_resolution=desired_resolution, align_corners=align_corners,
                                       interpolation=interpolation))
    return encoder, encoder.output_dim
