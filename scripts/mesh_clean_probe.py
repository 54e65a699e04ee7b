"""Rounds and timing of the mesh cleaning (csrc/lrf_mesh_clean.inl) on the mesh of mesh_probe.py's scene: a 256^3 volume, 64
frames of 360 x 640 of a camera circling a sphere in front of a wall.

  extract    TsdfVolume.extract with the capacities given: the stage the cleaning follows
  label      mesh.components: the rounds (each three launches and a 4-byte read-back), then the counts and their read-back
  filter     lrf_mesh_filter alone on those labels (three launches), without its read-back
  whole      mesh.filter_components(min_fraction=0.1): label + filter + the counts' read-back + the output allocations
  permuted   label on the same mesh under a random vertex permutation: the order extraction never produces

  python scripts/mesh_clean_probe.py [--n 256] [--reps 5]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from localrf_amd import _native as N, mesh  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402


def filter_stage(m, comp, threshold):
    """The native filter on the labels of comp, into fresh buffers; nothing is read back."""
    v, f, c = m["vertices"], m["faces"], m["rgb8"]
    nv, nf = m["counts"]
    vo, fo, co = torch.empty_like(v), torch.empty_like(f), torch.empty_like(c)
    counts = torch.empty(3, dtype=torch.int64, device=DEV)
    ws = N.workspace("lrf_mesh_filter", DEV, nv, nf)
    a = N.LrfMeshFilter()
    a.vertices, a.rgb8, a.faces, a.labels, a.faces_of = v.data_ptr(), c.data_ptr(), f.data_ptr(), comp["labels"].data_ptr(), comp["faces_of"].data_ptr()
    a.Nv, a.Nf = nv, nf

    def run():
        N.launch("lrf_mesh_filter", DEV, C.byref(a), threshold, vo.data_ptr(), co.data_ptr(), fo.data_ptr(), counts.data_ptr(),
                 ws.data_ptr(), guard=True)
    return run, counts


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
    comp = mesh.components(m["faces"], nv)
    sizes = comp["faces_of"][comp["faces_of"] > 0].sort(descending=True).values[:8].tolist()
    print(f"mesh: {nv} vertices, {nf} faces, {comp['n_components']} components ({comp['n_with_faces']} with faces), largest {sizes}")
    print(f"rounds: {comp['rounds']}")
    print(f"extract, capacities given: {timed(lambda: vol.extract(max_vertices=nv, max_faces=nf), a.reps):8.3f} ms")
    print(f"label ({comp['rounds']} rounds + counts): {timed(lambda: mesh.components(m['faces'], nv), a.reps):8.3f} ms")
    threshold = -(-comp["largest_faces"] // 10)
    run, counts = filter_stage(m, comp, threshold)
    print(f"filter stage, threshold {threshold}: {timed(run, a.reps):8.3f} ms")
    print(f"  kept vertices, faces, components: {counts.tolist()}")
    print(f"whole filter_components(min_fraction=0.1): {timed(lambda: mesh.filter_components(m, min_fraction=0.1), a.reps):8.3f} ms")
    p = torch.randperm(nv, generator=torch.Generator().manual_seed(0)).to(DEV)
    fp = p[m["faces"].long()].to(torch.int32).contiguous()
    cp = mesh.components(fp, nv)
    assert (cp["n_components"], cp["largest_faces"]) == (comp["n_components"], comp["largest_faces"])
    print(f"permuted vertices: rounds {cp['rounds']}, label {timed(lambda: mesh.components(fp, nv), a.reps):8.3f} ms")


if __name__ == "__main__":
    main()
