"""Counts and timing of the hole filling (csrc/lrf_mesh_fill.inl) on the mesh of mesh_probe.py's scene -- a 256^3 volume, 64
frames of 360 x 640 of a camera circling a sphere in front of a wall -- with the weights of --holes seeded 3 x 3 x 3 blocks of
lattice points on the surface zeroed, which punches that many holes into the extracted mesh beside its open outer border.

  holes       mesh.holes at max_edges 16, 64, 1024 and 4096: the bounds pass, the analysis, two read-backs
  fill_holes  mesh.fill_holes at the same values: holes, the output allocations, the fill, a third read-back
  analysis    lrf_mesh_holes alone at max_edges 64 and 4096, nothing read back

  python scripts/mesh_fill_probe.py [--n 256] [--holes 200] [--reps 5]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from localrf_amd import _native as N, mesh  # noqa: E402
from localrf_amd._checks import float_of_key  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def punch(vol, count, seed=0):
    """Zero the weights of `count` 3 x 3 x 3 blocks centred on seeded lattice points next to the surface."""
    near = ((vol.tsdf.abs() < 0.3) & (vol.weight > 0)).nonzero()
    pick = near[torch.randperm(near.shape[0], generator=torch.Generator().manual_seed(seed))[:count].to(DEV)]
    for d in range(27):
        z, y, x = pick[:, 0] + d // 9 - 1, pick[:, 1] + d // 3 % 3 - 1, pick[:, 2] + d % 3 - 1
        ok = (z >= 0) & (y >= 0) & (x >= 0) & (z < vol.dims[2]) & (y < vol.dims[1]) & (x < vol.dims[0])
        vol.weight[z[ok], y[ok], x[ok]] = 0.0


def analysis_stage(m, max_edges):
    """lrf_mesh_holes on the box of the mesh; nothing is read back."""
    v, f = m["vertices"], m["faces"]
    nv, nf = m["counts"]
    keys = torch.empty(7, dtype=torch.int32, device=DEV)
    N.launch("lrf_mesh_smooth_bounds", DEV, v.data_ptr(), nv, keys.data_ptr(), guard=True)
    keys = keys.tolist()
    lo = [float_of_key(k) for k in keys[:3]]
    a = N.LrfMeshHoles()
    a.vertices, a.rgb8, a.faces, a.Nv, a.Nf, a.max_edges = v.data_ptr(), None, f.data_ptr(), nv, nf, max_edges
    a.s = 36 - math.frexp(max(float_of_key(k) - l for k, l in zip(keys[3:6], lo)))[1]
    for k in range(3):
        a.lo[k] = lo[k]
    info = torch.empty(8, dtype=torch.int64, device=DEV)
    ws = N.workspace("lrf_mesh_holes", DEV, nv, nf)

    def run():
        N.launch("lrf_mesh_holes", DEV, C.byref(a), info.data_ptr(), ws.data_ptr(), guard=True)
    return run, ws.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--holes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    print(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, frames {H} x {W}, {a.holes} blocks zeroed")
    depth, rgb8, c2w = frames(64)
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    whole = mesh.holes(vol.extract(), 4096)
    punch(vol, a.holes)
    m = vol.extract()
    print(f"mesh: {m['counts'][0]} vertices, {m['counts'][1]} faces; before the blocks were zeroed: {whole}")
    for max_edges in (16, 64, 1024, 4096):
        h = mesh.holes(m, max_edges)
        filled = mesh.fill_holes(m, max_edges)
        print(f"max_edges {max_edges:4d}: {h}")
        print(f"  holes {timed(lambda: mesh.holes(m, max_edges), a.reps):8.3f} ms, fill_holes "
              f"{timed(lambda: mesh.fill_holes(m, max_edges), a.reps):8.3f} ms -> {filled['counts']}, a second fill adds "
              f"{mesh.fill_holes(filled, max_edges)['fill']['loops']} loops")
    for max_edges in (64, 4096):
        run, nbytes = analysis_stage(m, max_edges)
        print(f"lrf_mesh_holes alone, max_edges {max_edges:4d} (workspace {nbytes} bytes): {timed(run, a.reps):8.3f} ms")


if __name__ == "__main__":
    main()
