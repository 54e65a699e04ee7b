"""Counts and timing of the incidence lists and what is built on them (csrc/lrf_mesh_smooth.inl) on the mesh of
mesh_clean_probe.py -- a 256^3 volume, 64 frames of 360 x 640 of a camera circling a sphere in front of a wall -- and on its
simplification at 2 voxels.

  extract / filter / simplify   the stages this one follows: TsdfVolume.extract with the capacities given,
                                filter_components(min_fraction=0.1), simplify at 2 voxels
  incidence       lrf_mesh_incidence alone (six launches), nothing read back
  topology        mesh.topology as a whole (the lists, the edge kernel, one read-back)
  vertex_normals  mesh.vertex_normals as a whole (the lists, two kernels, one read-back)
  one step        lrf_mesh_smooth with iterations=2 minus iterations=1 at mu=0: one k_sm_step launch, nothing read back
  smooth          mesh.smooth with its defaults (10 iterations, two read-backs)

  python scripts/mesh_smooth_probe.py [--n 256] [--reps 5]
One line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from localrf_amd import _native as N, mesh  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def incidence_stage(m):
    nv, nf = m["counts"]
    info = torch.empty(8, dtype=torch.int64, device=DEV)
    ws = N.workspace("lrf_mesh_incidence", DEV, nv, nf)

    def run():
        N.launch("lrf_mesh_incidence", DEV, m["faces"].data_ptr(), nv, nf, info.data_ptr(), ws.data_ptr(), guard=True)
    return run, info, ws.numel()


def smooth_stage(m, iterations):
    """lrf_mesh_smooth at lam=0.5, mu=0 on the box of the mesh, into a fresh buffer; nothing is read back."""
    v, f = m["vertices"], m["faces"]
    nv, nf = m["counts"]
    lo, hi = v.amin(0).double().tolist(), v.amax(0).double().tolist()
    a = N.LrfMeshSmooth()
    a.vertices, a.faces, a.Nv, a.Nf, a.lam, a.mu = v.data_ptr(), f.data_ptr(), nv, nf, 0.5, 0.0
    a.s, a.iterations, a.pin_boundary = 36 - math.frexp(max(h - l for l, h in zip(lo, hi)))[1], iterations, 1
    for k in range(3):
        a.lo[k] = lo[k]
    vo = torch.empty_like(v)
    info = torch.empty(8, dtype=torch.int64, device=DEV)
    ws = N.workspace("lrf_mesh_smooth", DEV, nv, nf)

    def run():
        N.launch("lrf_mesh_smooth", DEV, C.byref(a), vo.data_ptr(), info.data_ptr(), ws.data_ptr(), guard=True)
    return run, ws.numel()


def measure(name, m, reps):
    nv, nf = m["counts"]
    t = mesh.topology(m)
    n = mesh.vertex_normals(m)
    print(f"{name}: {nv} vertices, {nf} faces; boundary edges {t['boundary_edges']}, non-manifold edges {t['nonmanifold_edges']}, "
          f"degenerate faces {t['degenerate_faces']}, boundary vertices {int(t['boundary_vertices'].sum())}, zero normals "
          f"{n['normal_info']['zero_normals']}")
    run, info, nbytes = incidence_stage(m)
    print(f"  incidence alone (workspace {nbytes} bytes): {timed(run, reps):8.3f} ms; entries {int(info[6])}")
    print(f"  topology as a whole:       {timed(lambda: mesh.topology(m), reps):8.3f} ms")
    print(f"  vertex_normals as a whole: {timed(lambda: mesh.vertex_normals(m), reps):8.3f} ms")
    one, _ = smooth_stage(m, 1)
    two, nbytes = smooth_stage(m, 2)
    t1, t2 = timed(one, reps), timed(two, reps)
    print(f"  lrf_mesh_smooth, 1 and 2 steps (workspace {nbytes} bytes): {t1:8.3f} ms, {t2:8.3f} ms; one step {t2 - t1:8.3f} ms")
    s = mesh.smooth(m)
    print(f"  smooth as a whole, 10 iterations: {timed(lambda: mesh.smooth(m), reps):8.3f} ms; {s['smooth']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    print(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, frames {H} x {W}")
    depth, rgb8, c2w = frames(64)
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    m = vol.extract()
    nv, nf = m["counts"]
    print(f"extract, capacities given: {timed(lambda: vol.extract(max_vertices=nv, max_faces=nf), a.reps):8.3f} ms")
    print(f"filter_components(min_fraction=0.1): {timed(lambda: mesh.filter_components(m, min_fraction=0.1), a.reps):8.3f} ms")
    print(f"simplify at 2 voxels: {timed(lambda: mesh.simplify(m, 2 * voxel, origin=vol.origin), a.reps):8.3f} ms")
    measure("extracted mesh", m, a.reps)
    measure("simplified at 2 voxels", mesh.simplify(m, 2 * voxel, origin=vol.origin), a.reps)


if __name__ == "__main__":
    main()
