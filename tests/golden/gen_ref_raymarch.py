"""Writes tests/golden/ref_raymarch.npz: what the REFERENCE'S OWN kernels (oracle/_ref/libref_raymarch.so: raymarching/src/raymarching.cu of the reference tree, built
by oracle/Makefile `ref`) computed on a GPU for the shared inputs of tests/raymarch_refs.py — data that the reference's program wrote, recorded so that
tests/test_raymarch_host.py can hold the numpy restatement to it where neither a GPU nor the reference tree exists.  Per march_rays_train case of
raymarch_refs.golden_cases() (65 rays, none hostile, max_steps 64): the samples per ray and a SHA-256 of xyzs / dirs / ts taken in ray order; for near_far_from_aabb
on the 4096 rays of the device test: a SHA-256 of nears and of fars.

Run on a machine with the GPU, after build():   python tests/golden/gen_ref_raymarch.py [output.npz]
Every input passes the host gate of tests/test_gpu_ref_raymarch.py before it is launched."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import raymarch_refs as R      # noqa: E402
import test_gpu_ref_raymarch as G      # noqa: E402


def main(out):
    cases = R.golden_cases()
    counts = np.zeros((len(cases), 65), np.int32); sha = np.zeros((len(cases), 3, 32), np.uint8)
    for i, (k, s, p) in enumerate(cases):
        c = R.march_train_case(R.GRID_KINDS[k], s, p, 65, False)
        xyzs, dirs, ts, rays = G.ref_march_train(c)
        counts[i] = rays[:, 1]
        for j, a in enumerate((xyzs, dirs, ts)):
            sha[i, j] = R.digest(G.in_ray_order(a, rays))
    o, d, aabb = R.near_far_inputs()
    go, gd, ga = G.dev(o), G.dev(d), G.dev(aabb)
    rn, rf = G.zeros(o.shape[0]), G.zeros(o.shape[0])
    G.call("ref_near_far_from_aabb", G.p(go), G.p(gd), G.p(ga), o.shape[0], 0.2, G.p(rn), G.p(rf))
    np.savez_compressed(out, cases=np.array(cases, np.int32), counts=counts, sha=sha, near_far_sha=np.stack([R.digest(G.host(rn)), R.digest(G.host(rf))]))
    print("wrote %s: %d cases, %d samples" % (out, len(cases), counts.sum()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_raymarch.npz"))
