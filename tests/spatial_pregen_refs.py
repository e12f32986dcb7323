"""The direct-lighting chain of a frame replayed pass by pass on the CPU oracle, to say which neighbours the spatial passes of a frame meet.

tests/test_gpu_spatial_pregen.py needs a frame in which the clause "neighbour reservoir M != 0" of the spatial pass decides alone for FOREGROUND neighbours: the
engine makes the other three clauses once per batch (csrc/passes.hip k_spatial_accept) and this one inside the merge, and only such a frame can tell whether the
merge makes it.  No GPU here."""
import numpy as np

import reservoir_refs as R

RIS_PASSES = 20      # mTotalRISPasses: frame index of sample i = random_offset + 20 i; light tiles take pass 0, initial 2, temporal 3 (from sample 1 on), spatial the next


def hostile_roughness(F, rough=0.005, step=2):
    """F's (roughness, metallic) map with every `step`-th pixel's roughness below the 0.01 clamp (alpha^2 = 1e-4).  Where a BRDF candidate of such a pixel falls
    into the lobe's peak, its weight target / pdf is not finite, the reservoir's weight neither, and the initial pass stores the empty reservoir (M = 0) for a
    FOREGROUND pixel.  The frame's outputs stay finite.  (0.02 and above: no reservoir is emptied.)"""
    rm = F.rm.copy()
    rm[::step, 0] = np.float32(rough)
    return rm


def brdf_scalars(kd, rm):
    """The per-pixel BRDF scalars of restir_di_with_pt (:279-287) as util.SmallFrame derives them: luminance of kd, luminance of metallic, alpha^2."""
    k, m, r_ = kd, rm[:, 1], rm[:, 0]
    b0 = (k[:, 0] * np.float32(0.2126) + k[:, 1] * np.float32(0.7152)) + k[:, 2] * np.float32(0.0722)
    b1 = (m * np.float32(0.2126) + m * np.float32(0.7152)) + m * np.float32(0.0722)
    a = np.clip(r_, np.float32(0.01), np.float32(1.0))
    return np.stack([b0, b1, a * a], 1).astype(np.float32)


def geometric_pairs(O, F, samples, random_offset, neighbor_count=5):
    """Per sample of a whole frame: the number of (foreground pixel, candidate) pairs that pass the three clauses k_spatial_accept makes — in bounds, isValidNeighbor,
    neighbour is foreground — i.e. the pairs it must queue.  Sample 0 has no temporal pass: its spatial pass is pass 3, the others' pass 4."""
    ones = np.ones(F.N, np.int32)
    out = []
    for i in range(samples):
        c = R.classify_spatial(O, F.fx, F.fy, F.occ, F.normal_depth, ones, np.ones(F.N, np.float32), F.noff, random_offset + RIS_PASSES * i + (4 if i > 0 else 3), neighbor_count)
        out.append(int((c.cls == R.S_ACCEPTED).sum()))
    return out


def m_zero_neighbours(O, F, rm, spp, random_offset, neighbor_count=5):
    """Per sample of the frame F with the (roughness, metallic) map `rm`: the number of (foreground pixel, candidate) pairs whose candidate is in bounds, passes
    isValidNeighbor, is FOREGROUND and holds M == 0 in the reservoirs that enter the sample's spatial pass (the temporal output)."""
    brdf = brdf_scalars(F.kd, rm)
    frame = O.make_frame(F.keep, F.fx, F.fy, F.occ, F.pos, F.normal_depth, brdf, F.ray_dir, (F.info, F.aabb), F.vert, F.tri, F.tex, F.Wc, F.Hc, F.tables)
    counts, prev = [], None
    for i in range(spp):
        base = random_offset + RIS_PASSES * i
        tile_ld, _, tile_pdf = O.light_tiles(frame, base)
        cur = O.new_reservoirs(F.N)
        O.initial(frame, cur, tile_ld, tile_pdf, base + 2)
        p = 3
        if i > 0:
            O.temporal(frame, cur, prev, F.occ, F.normal_depth, brdf, F.ray_dir, base + 3)
            p = 4
        c = R.classify_spatial(O, F.fx, F.fy, F.occ, F.normal_depth, np.asarray(cur[2]).reshape(-1), np.asarray(cur[3]).reshape(-1), F.noff, base + p, neighbor_count)
        fg_nb = F.occ[np.maximum(c.nb, 0)] > 0.5
        counts.append(int(((c.cls == R.S_M_ZERO) & fg_nb).sum()))
        out = O.new_reservoirs(F.N)
        O.spatial(frame, out, cur, F.noff, base + p)
        prev = out
    return counts
