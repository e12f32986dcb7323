"""Plain numpy restatements for the batched material lookup of mirres_render (csrc/matnet.hip: k_active_from_live's position key and the order the
radix sort k_ls_* must leave the slot list in).  Everything that feeds a comparison is float32, one correctly rounded operation per step, as the device
code is built (no fast-math, -ffp-contract=off, an IEEE division): the keys are expected to agree bit for bit."""
import numpy as np


def spread10(v):
    """The low 10 bits of v, two zero bits between neighbours: bit b -> bit 3 b."""
    v = np.asarray(v, np.uint32) & np.uint32(0x3ff)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def quantise(pos, aabb_min, aabb_max, bits):
    """Cell of every coordinate on the 2^bits grid of the box: u = (pos - min) / (max - min) in float32, q = trunc(clamp(u 2^bits, 0, 2^bits - 1)), NaN -> 0."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    lo = np.asarray(aabb_min, np.float32); hi = np.asarray(aabb_max, np.float32)
    with np.errstate(all="ignore"):
        u = ((pos - lo[None]) / (hi - lo)[None]).astype(np.float32)
        v = (u * np.float32(1 << bits)).astype(np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)                     # fmaxf(NaN, 0) = 0
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32((1 << bits) - 1))
    return np.trunc(v).astype(np.uint32)


def morton_key(pos, aabb_min, aabb_max, bits):
    """uint32 key of every point: the three cell numbers interleaved, x the most significant bit of each triple."""
    q = quantise(pos, aabb_min, aabb_max, bits)
    return (spread10(q[:, 0]) << np.uint32(2)) | (spread10(q[:, 1]) << np.uint32(1)) | spread10(q[:, 2])


def expected_walk(unsorted, keys):
    """The list a stable sort by key leaves: `unsorted` are slots, `keys` the key of every slot."""
    unsorted = np.asarray(unsorted)
    return unsorted[np.argsort(np.asarray(keys)[unsorted], kind="stable")]
