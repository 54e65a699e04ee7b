"""Counts and timing of the mesh simplification (csrc/lrf_mesh_simplify.inl) on the mesh of mesh_clean_probe.py: a 256^3
volume, 64 frames of 360 x 640 of a camera circling a sphere in front of a wall, simplified on grids of 2, 4 and 8 voxels
anchored at the volume's origin, with the vertices placed at the mean and by the quadric.

  extract    TsdfVolume.extract with the capacities given, and filter_components(min_fraction=0.1): the stages it follows
  simplify   mesh.simplify as a whole: the bounds pass and its read-back, the allocations, the simplification, the counts' read-back
  stage      lrf_mesh_simplify alone (twelve launches) on the box of that bounds pass, without a read-back
  quadric    the same two measurements of placement="quadric": lrf_mesh_simplify_quadric alone is sixteen launches

  python scripts/mesh_simplify_probe.py [--n 256] [--reps 5]
Prints, per cell size, vertices and faces in and out, the degenerate and duplicate faces and the signed volume before and
after under both placements, and one line per measurement: the median of --reps runs after one warm-up, timed with device
events.  The two placements are measured in turn in the same process."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from localrf_amd import _native as N, mesh  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def signed_volume(m):
    """Sum of a . (b x c) / 6 over the faces, in float64: the enclosed volume of a closed mesh."""
    v = m["vertices"].double()
    a, b, c = (v[m["faces"][:, k].long()] for k in range(3))
    return float((a * torch.linalg.cross(b, c)).sum() / 6.0)


def simplify_stage(m, info, quadric=False):
    """The native simplification on the box of info, into fresh buffers; nothing is read back."""
    v, f, c = m["vertices"], m["faces"], m["rgb8"]
    nv, nf = m["counts"]
    lo, dims = info["box"]["lo"], info["box"]["dims"]
    entry = "lrf_mesh_simplify_quadric" if quadric else "lrf_mesh_simplify"
    vo, fo, co = torch.empty_like(v), torch.empty_like(f), torch.empty_like(c)
    counts = torch.empty(7 if quadric else 5, dtype=torch.int64, device=DEV)
    ws = N.workspace(entry, DEV, nv, nf, dims[0] * dims[1] * dims[2])
    q = N.LrfMeshSimplifyQuadric() if quadric else None
    a = q.mesh if quadric else N.LrfMeshSimplify()
    a.vertices, a.rgb8, a.faces, a.Nv, a.Nf, a.cell, a.dedupe = v.data_ptr(), c.data_ptr(), f.data_ptr(), nv, nf, info["cell"], 1
    for k in range(3):
        a.origin[k], a.lo[k], a.dims[k] = info["origin"][k], lo[k], dims[k]
    if quadric:
        q.regularize = info["regularize"]

    def run():
        N.launch(entry, DEV, C.byref(q if quadric else a), vo.data_ptr(), co.data_ptr(), fo.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                 guard=True)
    return run, counts, ws.numel()


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
    print(f"mesh: {nv} vertices, {nf} faces, signed volume {signed_volume(m):.6f}")
    print(f"extract, capacities given: {timed(lambda: vol.extract(max_vertices=nv, max_faces=nf), a.reps):8.3f} ms")
    print(f"filter_components(min_fraction=0.1): {timed(lambda: mesh.filter_components(m, min_fraction=0.1), a.reps):8.3f} ms")
    for k in (2, 4, 8):
        cell = k * voxel
        s = mesh.simplify(m, cell, origin=vol.origin)
        info = s["simplify"]
        print(f"cell {k} voxels: {nv} / {nf} -> {s['counts'][0]} vertices / {s['counts'][1]} faces; box {info['box']['dims']}, "
              f"occupied {info['occupied']}, degenerate {info['degenerate_faces']}, duplicate {info['duplicate_faces']}, "
              f"signed volume {signed_volume(s):.6f}")
        run, counts, nbytes = simplify_stage(m, info)
        print(f"  simplify as a whole: {timed(lambda: mesh.simplify(m, cell, origin=vol.origin), a.reps):8.3f} ms")
        print(f"  stage alone (workspace {nbytes} bytes): {timed(run, a.reps):8.3f} ms; counts {counts.tolist()}")
        assert counts.tolist()[:2] == list(s["counts"])
        sq = mesh.simplify(m, cell, origin=vol.origin, placement="quadric")
        iq = sq["simplify"]
        assert sq["counts"] == s["counts"] and torch.equal(sq["faces"], s["faces"])
        print(f"  quadric: at the mean {iq['fallback_clusters']}, clamped {iq['clamped_clusters']}, signed volume {signed_volume(sq):.6f}")
        run, counts, nbytes = simplify_stage(m, iq, quadric=True)
        print(f"  quadric, simplify as a whole: {timed(lambda: mesh.simplify(m, cell, origin=vol.origin, placement='quadric'), a.reps):8.3f} ms")
        print(f"  quadric, stage alone (workspace {nbytes} bytes): {timed(run, a.reps):8.3f} ms; counts {counts.tolist()}")
        assert counts.tolist()[:2] == list(sq["counts"])


if __name__ == "__main__":
    main()
