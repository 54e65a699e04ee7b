"""Timing of the texture bake (csrc/lrf_mesh_texture.inl) on the probe scene of scripts/raster_probe.py: scripts/mesh_probe.py's
sphere before a wall fused into a --n^3 volume; the raw mesh and simplify at 2 and 4 voxels; patch 4 / 8 / 16 and both blends;
--frames frames of 360 x 640 per call.

  add       TextureBaker.add(rgb8, poses, ...) with mesh_depth=None: the rasterisation of the mesh at the poses, then the bake
  bake      the same with the rasterised depth passed in: lrf_mesh_texture_bake alone (one launch)
  finish    lrf_mesh_texture_resolve and its read-back

  python scripts/texture_probe.py [--n 192] [--reps 21] [--frames 8]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events (finish: a host clock
around the call, which ends in a read-back)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import mesh, mesh_raster, mesh_texture  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    n, V = a.n, a.frames
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    depth, rgb8, c2w = frames(16)
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    raw = vol.extract()
    print(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, mesh {raw['counts']}, {V} frames of {H} x {W} per call")
    centre = (W / 2, H / 2)
    poses, rgb = c2w[:V], rgb8[:V].contiguous()
    for label, m in (("raw", raw), ("simplify 2 voxels", mesh.simplify(raw, 2 * voxel, origin=origin)),
                     ("simplify 4 voxels", mesh.simplify(raw, 4 * voxel, origin=origin))):
        flat = {"vertices": m["vertices"], "faces": m["faces"], "rgb8": None}
        dm = mesh_raster.rasterize(flat, poses, W, H, FOCAL, centre, cull="back")["depth"]
        ms_r = timed(lambda: mesh_raster.rasterize(flat, poses, W, H, FOCAL, centre, cull="back"), a.reps)
        print(f"{label:18s} faces {m['counts'][1]:7d}: rasterize alone {ms_r:8.3f} ms")
        for patch in (4, 8, 16):
            for blend in ("mean", "best"):
                baker = mesh_texture.TextureBaker(m, patch=patch, blend=blend)
                texels = baker.Ht * baker.Wt
                ms_add = timed(lambda: baker.add(rgb, poses, FOCAL, centre), a.reps)
                ms_bake = timed(lambda: baker.add(rgb, poses, FOCAL, centre, dm), a.reps)
                t = []
                for _ in range(max(3, a.reps // 4)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = baker.finish()
                    t.append(1e3 * (time.perf_counter() - t0))
                info = out["info"]
                print(f"{label:18s} patch {patch:2d} {blend}: atlas {baker.Ht} x {baker.Wt} ({texels / 1e6:7.2f} M texels, state "
                      f"{16 * texels / 2 ** 20:7.1f} MiB), add {ms_add:8.3f} ms, bake {ms_bake:8.3f} ms "
                      f"({texels * V / ms_bake / 1e6:7.2f} G texel-frames / s), finish {float(np.median(t)):8.3f} ms, observed "
                      f"{100 * info['observed_texels'] / max(info['used_texels'], 1):5.1f} % of the used texels")
                del baker, out


if __name__ == "__main__":
    main()
