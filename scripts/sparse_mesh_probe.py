"""Timing of the block-sparse TSDF volume (csrc/lrf_tsdf_blocks.inl) beside the dense one, on the synthetic frames and the
256^3 lattice of scripts/mesh_probe.py (64 frames of 360 x 640, a camera circling a sphere in front of a wall), and on a
lattice the dense path refuses: the same box at 2048^3 virtual points.

  touch + allocate  SparseTsdfVolume.touch and .allocate on a fresh volume (six launches, one read-back)
  integrate         one call over the 64 frames, sparse and dense
  extract           capacities given, sparse and dense

  python scripts/sparse_mesh_probe.py [--n 256] [--big 2048] [--reps 5]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import mesh  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402

ORIGIN, EXTENT, V = (-1.7, -1.7, -4.7), 3.4, 64


def fresh_timed(make, fn, reps):
    """Median ms of fn(make()) over reps runs after one warm-up; make() is outside the timed window."""
    ms = []
    for r in range(reps + 1):
        obj = make()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(obj)
        b.record()
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def sparse_run(n, depth, rgb8, c2w, reps, dense):
    blocks = (n // 8,) * 3
    voxel = EXTENT / (n - 1)
    cen = (W / 2, H / 2)

    def make():
        return mesh.SparseTsdfVolume(ORIGIN, voxel, blocks, 3 * voxel, DEV)

    def touch_allocate(v):
        v.touch(depth, c2w, FOCAL, cen)
        v.allocate()
    print(f"--- {n}^3 virtual points, voxel {voxel:.5f}, trunc {3 * voxel:.5f}, {V} frames {H} x {W}")
    print(f"sparse touch + allocate: {fresh_timed(make, touch_allocate, reps):8.3f} ms")
    vol = make()
    touch_allocate(vol)
    dense_bytes = n ** 3 * 20
    print(f"sparse: {vol.n_blocks} of {blocks[0] ** 3} blocks stored, {vol.nbytes} bytes (dense: {dense_bytes} bytes, "
          f"{dense_bytes / vol.nbytes:.1f} x)")
    ms = timed(lambda: vol.integrate(depth, c2w, FOCAL, cen, rgb=rgb8), reps)
    print(f"sparse integrate {V} frames: {ms:8.3f} ms  ({V * vol.n_blocks * 512 / ms / 1e6:.1f} G voxel-frame pairs / s)")
    vol = make()
    touch_allocate(vol)
    vol.integrate(depth, c2w, FOCAL, cen, rgb=rgb8)
    nv, nf = vol.extract()["counts"]
    print(f"sparse mesh: {nv} vertices, {nf} faces")
    print(f"sparse extract, capacities given: {timed(lambda: vol.extract(max_vertices=nv, max_faces=nf), reps):8.3f} ms")
    if not dense:
        try:
            mesh.TsdfVolume(ORIGIN, voxel, (n, n, n), 3 * voxel, DEV)
        except ValueError as e:
            print(f"dense: refused ({e})")
        return
    ref = mesh.TsdfVolume(ORIGIN, voxel, (n, n, n), 3 * voxel, DEV)
    ms = timed(lambda: ref.integrate(depth, c2w, FOCAL, cen, rgb=rgb8), reps)
    print(f"dense integrate {V} frames: {ms:8.3f} ms  ({V * n ** 3 / ms / 1e6:.1f} G voxel-frame pairs / s)")
    ref = mesh.TsdfVolume(ORIGIN, voxel, (n, n, n), 3 * voxel, DEV)
    ref.integrate(depth, c2w, FOCAL, cen, rgb=rgb8)
    dv, df = ref.extract()["counts"]
    print(f"dense mesh: {dv} vertices, {df} faces")
    print(f"dense extract, capacities given: {timed(lambda: ref.extract(max_vertices=dv, max_faces=df), reps):8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--big", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.n % 8 or a.big % 8:
        raise SystemExit("--n and --big must be multiples of 8")
    print(f"device {torch.cuda.get_device_name(0)}")
    depth, rgb8, c2w = frames(V)
    sparse_run(a.n, depth, rgb8, c2w, a.reps, dense=True)
    if a.big:
        sparse_run(a.big, depth, rgb8, c2w, a.reps, dense=False)


if __name__ == "__main__":
    main()
