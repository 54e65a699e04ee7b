"""Timing of the mesh rasteriser (csrc/lrf_mesh_raster.inl) and the agreement figures of one synthetic scene.

  rasterize   frames/s at 360 x 640 of a scene_mesh-like mesh -- scripts/mesh_probe.py's sphere before a wall fused into a
              --n^3 volume -- from cameras INSIDE the scene (between the sphere and the wall, turning round), over a sweep of
              small_max: the largest pixel box a face's own lane walks; larger ones go to a wavefront
  agreement   depth_agreement of the rasterised mesh with the input depth at the integration poses, for the raw mesh and a few
              simplify_cell / smooth_iterations settings

  python scripts/raster_probe.py [--n 192] [--reps 5] [--frames 8]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import mesh, mesh_raster  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402

SWEEP = (0, 16, 64, 128, 256, 512, 1024, 4096, (1 << 31) - 1)


def inside_cameras(V):
    """V cameras at (0.9, 0.2, -3.9), between the sphere and the wall, turning about y through a full circle."""
    c2w = np.zeros((V, 3, 4), np.float32)
    for k in range(V):
        a = 2 * math.pi * k / V
        c2w[k, :, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
        c2w[k, :, 3] = (0.9, 0.2, -3.9)
    return torch.from_numpy(c2w).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    depth, rgb8, c2w = frames(16)
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    raw = vol.extract()
    print(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, mesh {raw['counts']}, frames {H} x {W}")
    centre = (W / 2, H / 2)
    for name, poses in (("inside", inside_cameras(a.frames)), ("outside", c2w[:a.frames])):
        V = poses.shape[0]
        ref = None
        for small_max in SWEEP:
            out = mesh_raster.rasterize(raw, poses, W, H, FOCAL, centre, small_max=small_max)
            ref = out if ref is None else ref
            assert torch.equal(out["depth"], ref["depth"]) and torch.equal(out["face"], ref["face"])
            ms = timed(lambda: mesh_raster.rasterize(raw, poses, W, H, FOCAL, centre, small_max=small_max), a.reps)
            print(f"rasterize {name:8s} small_max {small_max:10d}: {ms:9.3f} ms for {V} frames  ({V / ms * 1e3:8.1f} frames / s)")
        hit = float((ref["face"] >= 0).float().mean())
        print(f"rasterize {name:8s} pixels with a hit: {100 * hit:.1f} %")
    for label, m in (("raw", raw), ("simplify 2 voxels", mesh.simplify(raw, 2 * voxel, origin=origin)),
                     ("simplify 4 voxels", mesh.simplify(raw, 4 * voxel, origin=origin)),
                     ("smooth 10", mesh.smooth(raw, 10)), ("simplify 2 voxels + smooth 10", mesh.smooth(mesh.simplify(raw, 2 * voxel, origin=origin), 10))):
        ras = mesh_raster.rasterize(m, c2w, W, H, FOCAL, centre)
        g = mesh_raster.depth_agreement(ras["depth"], depth, rel_tols=(0.001, 0.01, 0.05))
        px = 16 * H * W
        print(f"agreement {label:30s} faces {m['counts'][1]:8d}: both {100 * g['both'] / px:5.1f} %, mesh only {100 * g['mesh_only'] / px:5.2f} %, "
              f"render only {100 * g['render_only'] / px:5.2f} %, within 0.1 / 1 / 5 % of the depth: "
              + " / ".join(f"{100 * w / max(g['both'], 1):.2f}" for w in g["within"]) + f" % of both, mean relative error {g['mean_rel_error']:.5f}")
    ms = timed(lambda: mesh_raster._agreement_counts(ras["depth"], depth, [0.01, 0.05], 0.0, math.inf, False), a.reps)
    print(f"depth_agreement, 16 frames: {ms:.3f} ms")


if __name__ == "__main__":
    main()
