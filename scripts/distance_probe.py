"""Timing of the point-to-mesh distance (csrc/lrf_mesh_distance.inl) and the mesh_distance figures of one synthetic scene.

  index     MeshIndex of a scene_mesh-like mesh -- scripts/mesh_probe.py's sphere before a wall fused into a --n^3 volume --
            over a sweep of the cell around default_cell
  closest   the query for --points surface samples of the mesh itself (every answer is 0: the cheapest walk) and for as many
            points of the frames' back-projected depth inside the mesh's box (a scene_point_cloud's points: near the surface,
            not on it), those with max_distance = 8 voxels: a point at distance D walks about (2 D / cell)^3 cells, so a
            benchmark bounds D
  brute     for scale only: a PyTorch brute force (point-to-vertex distances, cdist + min) on a subsample that fits memory
  figures   mesh_distance of the raw mesh against simplify at 2 and 4 voxels and against smooth(10)

  python scripts/distance_probe.py [--n 192] [--reps 5] [--points 1000000]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events; a call that takes
more than two seconds is timed once, by the host clock around a synchronise, and marked so."""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import mesh, mesh_distance, pointcloud  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames, timed  # noqa: E402

FACTORS = (4.0, 2.0, 1.5, 1.0, 0.75, 0.5)


def measure(fn, reps):
    """-> (ms, note): the median of reps runs between device events, or one run by the host clock when that takes over 2 s."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = (time.perf_counter() - t0) * 1e3
    return (once, " (one run)") if once > 2000 else (timed(fn, reps), "")


def say(line):
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    depth, rgb8, c2w = frames(16)
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    raw = vol.extract()
    say(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, mesh {raw['counts']}")
    base = mesh_distance.MeshIndex(raw)
    info = base.info
    m1 = mesh_distance.sample_surface(raw, voxel)["counts"][0]                       # area / voxel^2: sizes the spacing for --points
    spacing = voxel * math.sqrt(m1 / a.points) * 0.99
    s = mesh_distance.sample_surface(raw, spacing, max_points=1 << 28)
    samples = s["points"][torch.randperm(s["counts"][0], device=DEV)[:a.points]].contiguous()
    cloud = pointcloud.backproject(depth, c2w, W, H, FOCAL, (W / 2, H / 2))[0]
    lo, hi = (torch.tensor(b, device=DEV) for b in info["box"])
    cloud = cloud[((cloud >= lo - 2 * voxel) & (cloud <= hi + 2 * voxel)).all(1)]    # the frames also see the wall beyond the volume
    cloud = cloud[torch.randperm(cloud.shape[0], device=DEV)[:a.points]].contiguous()
    reach = {"samples": math.inf, "cloud": 8 * voxel}
    say(f"default cell {info['cell']:.5f} ({info['cell'] / voxel:.2f} voxels), dims {info['dims']}, entries {info['entries']}, "
          f"{base.nbytes / 2 ** 20:.1f} MiB; samples {samples.shape[0]} of {s['counts'][0]} at spacing {spacing:.5f}, cloud {cloud.shape[0]}")
    ms, note = measure(lambda: mesh_distance.sample_surface(raw, spacing, max_points=1 << 28), a.reps)
    say(f"sample_surface, {s['counts'][0]} samples: {ms:9.3f} ms{note}")
    ref = {}
    for f in FACTORS:
        cell = info["cell"] * f
        try:
            index = mesh_distance.MeshIndex(raw, cell=cell, max_bytes=8 << 30)
        except ValueError as e:
            say(f"cell x {f:4.2f}: refused: {e}")
            continue
        t_build, note = measure(lambda: mesh_distance.MeshIndex(raw, cell=cell, max_bytes=8 << 30), a.reps)
        line = f"cell x {f:4.2f} = {cell:.5f}: dims {index.info['dims']}, entries {index.info['entries']:9d}, {index.nbytes / 2 ** 20:7.1f} MiB, build {t_build:8.3f} ms{note}"
        for name, pts in (("samples", samples), ("cloud", cloud)):
            out = index.closest(pts, reach[name])
            if name in ref:
                assert torch.equal(out["distance"].view(torch.int32), ref[name]["distance"].view(torch.int32)) and torch.equal(out["face"], ref[name]["face"])
            ref.setdefault(name, out)
            ms, note = measure(lambda: index.closest(pts, reach[name]), a.reps)
            line += f", closest {name} {ms:8.3f} ms{note} ({pts.shape[0] / ms / 1e3:7.1f} M points / s)"
        print(line)
    for name in ref:
        d = ref[name]["distance"]
        d = d[torch.isfinite(d)]
        say(f"{name}: {d.numel()} within reach, mean distance {float(d.mean()) / voxel:.5f} voxels, max {float(d.max()) / voxel:.4f} voxels")
    ms = timed(lambda: mesh_distance.distance_summary(ref["cloud"]["distance"], (voxel, 2 * voxel), voxel), a.reps)
    say(f"distance_summary, {cloud.shape[0]} values (with its read-back): {ms:9.3f} ms")
    sub = cloud[:4096]
    verts = raw["vertices"]
    ms = timed(lambda: torch.cdist(sub, verts).min(1), a.reps)
    say(f"for scale only: torch.cdist + min of {sub.shape[0]} points against the {verts.shape[0]} VERTICES (not the faces): {ms:9.3f} ms "
          f"({sub.shape[0] / ms / 1e3:7.3f} M points / s)")
    for label, m in (("simplify 2 voxels", mesh.simplify(raw, 2 * voxel, origin=origin)), ("simplify 4 voxels", mesh.simplify(raw, 4 * voxel, origin=origin)),
                     ("smooth 10", mesh.smooth(raw, 10))):
        r = mesh_distance.mesh_distance(raw, m, voxel, thresholds=(0.25 * voxel, voxel), max_distance=8 * voxel)
        ms = timed(lambda: mesh_distance.mesh_distance(raw, m, voxel, thresholds=(0.25 * voxel, voxel), max_distance=8 * voxel), max(1, a.reps // 2))
        say(f"mesh_distance raw vs {label:18s} faces {m['counts'][1]:8d}, samples {r['samples']}: chamfer {r['chamfer'] / voxel:.4f} voxels, hausdorff "
              f"{r['hausdorff'] / voxel:.4f} voxels, rms {r['a_to_b']['rms'] / voxel:.4f} / {r['b_to_a']['rms'] / voxel:.4f}, beyond "
              f"{r['a_to_b']['beyond']} / {r['b_to_a']['beyond']}, fscore at 0.25 / 1 voxel: " + " / ".join(f"{x:.4f}" for x in r["fscore"])
              + f"; {ms:9.3f} ms")


if __name__ == "__main__":
    main()
