"""Timing of one ICP iteration (localrf_amd/alignment.py over csrc/lrf_align.inl and lrf_mesh_closest), split into its parts.

  target    a scene_mesh-like mesh -- scripts/mesh_probe.py's sphere before a wall fused into a --n^3 volume -- under its
            default MeshIndex
  cloud     --points surface samples of that mesh moved by the inverse of a small similarity (0.05 rad, scale 1.02, a shift
            of two voxels): what icp has to bring back
  parts     transform (lrf_align_transform), closest (MeshIndex.closest with closest=True and max_distance = 8 voxels),
            accumulate (lrf_align_plane, and lrf_align_pairs for metric="point"), read-back plus host solve; then one whole
            icp iteration and a whole run

  python scripts/align_probe.py [--n 192] [--reps 20] [--points 1000000]
Prints one line per part: the median of --reps runs after one warm-up, between device events; the read-back and solve by the
host clock, since it ends in the copy's synchronise."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import alignment, mesh, mesh_distance  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def say(line):
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000000)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    depth, rgb8, c2w = frames(16)
    vol = mesh.TsdfVolume((-1.7, -1.7, -4.7), voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    raw = vol.extract()
    index = mesh_distance.MeshIndex(raw)
    m1 = mesh_distance.sample_surface(raw, voxel)["counts"][0]
    spacing = voxel * math.sqrt(m1 / a.points) * 0.99
    s = mesh_distance.sample_surface(raw, spacing, max_points=1 << 28)
    on = s["points"][torch.randperm(s["counts"][0], device=DEV)[:a.points]].contiguous()
    axis = np.array((1.0, 2.0, -1.0)) / math.sqrt(6.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(0.05) * K + (1 - math.cos(0.05)) * (K @ K)
    centre = np.array([(l + h) / 2 for l, h in zip(*index.info["box"])])
    truth = alignment.similarity(1.02, R, centre - 1.02 * R @ centre + 2 * voxel * np.array((1.0, -1.0, 0.5)))
    cloud = alignment.transform_points(on, alignment.inverse(truth))
    reach = 8 * voxel
    say(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, mesh {raw['counts']}, cell {index.info['cell']:.5f}, "
        f"cloud {cloud.shape[0]} points, max_distance {reach:.5f}")
    T = np.eye(4)
    cur = torch.empty_like(cloud)
    lo, hi = index.info["box"]
    c = tuple(float(x) for x in centre)
    u = alignment._power_of_two_at_least(max(h - l for l, h in zip(lo, hi)) + 2 * reach)
    c0, h0 = alignment.pair_frame(tuple(l - reach for l in lo), tuple(x + reach for x in hi))
    alignment._transform_into(cloud, T, cur)
    near = index.closest(cur, reach, closest=True)
    keep = (near["distance"] <= reach).to(torch.uint8)
    words = alignment._plane_words(index, cur, near, c, u, reach)

    def back():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = alignment.solve_plane(alignment._add_words(words.cpu()), True)
        alignment.compose(alignment.plane_update(sol, c, u), T)
        return (time.perf_counter() - t0) * 1e3
    rows = [("transform (lrf_align_transform)", timed(lambda: alignment._transform_into(cloud, T, cur), a.reps)),
            ("closest (lrf_mesh_closest, closest=True)", timed(lambda: index.closest(cur, reach, closest=True), a.reps)),
            ("accumulate, plane (lrf_align_plane)", timed(lambda: alignment._plane_words(index, cur, near, c, u, reach), a.reps)),
            ("accumulate, point (lrf_align_pairs)", timed(lambda: alignment._pair_words(c0, h0, cur, near["closest"], keep), a.reps)),
            ("read-back + host solve (host clock)", float(np.median([back() for _ in range(a.reps)]))),
            ("icp, one iteration, plane (whole call)", timed(lambda: alignment.icp(cloud, index, iterations=1, max_distance=reach), a.reps)),
            ("icp, one iteration, point (whole call)", timed(lambda: alignment.icp(cloud, index, iterations=1, max_distance=reach, metric="point"), a.reps))]
    for name, ms in rows:
        say(f"{name:42s} {ms:9.3f} ms")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = alignment.icp(cloud, index, max_distance=reach)
    ms = (time.perf_counter() - t0) * 1e3
    (s1, R1, t1), (s0, R0, t0_) = alignment.decompose(out["T"]), alignment.decompose(truth)
    say(f"icp to the end: {out['iterations']} iterations ({out['reason']}), {ms:.1f} ms, count {out['count']}, rms {out['rms'] / voxel:.2e} voxels; "
        f"scale off by {abs(s1 - s0):.2e}, rotation by {np.abs(R1 - R0).max():.2e}, translation by {np.abs(t1 - t0_).max() / voxel:.2e} voxels")


if __name__ == "__main__":
    main()
