"""Timing of the point-cloud index (csrc/lrf_cloud.inl) on a scene_point_cloud-like cloud: --points points of the back-projected
depth of scripts/mesh_probe.py's frames (a sphere before a wall, 16 views), shuffled.

  index     CloudIndex over a sweep of the cell around default_point_cell
  closest   the cloud's twin -- every point moved by a quarter of the median spacing in a random direction -- against the index,
            at every cell of the sweep: the answers are asserted equal across the sweep
  knn       k = 1 and k = 8 with exclude_self on the cloud itself; radius_count at 2 and 4 spacings; voxel_downsample at 2 spacings
  parent    the only route to the same answer before this index: mesh_distance.MeshIndex over the faces (i, i, i), queried with
            the same twin.  The two are timed ALTERNATELY, one run of each per repetition, in the same process, at the same cell
            and at each index's own default cell; the answers are asserted equal bit for bit

  python scripts/cloud_probe.py [--points 1000000] [--reps 7]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events, with the smallest and
largest run; a ratio is the parent's median over the new one's."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import cloud, mesh_distance, pointcloud  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames  # noqa: E402

FACTORS = (4.0, 2.0, 1.0, 0.5, 0.25)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """One warm-up of each, then reps rounds of one run of each in turn -> per function (median, min, max) in ms."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(once(fn))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def say(line):
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    depth, rgb8, c2w = frames(16)
    pts = pointcloud.backproject(depth, c2w, W, H, FOCAL, (W / 2, H / 2))[0]
    pts = pts[torch.isfinite(pts).all(1)]
    g = torch.Generator(device=DEV).manual_seed(1)
    pts = pts[torch.randperm(pts.shape[0], device=DEV, generator=g)[:a.points]].contiguous()
    M = pts.shape[0]
    base = cloud.CloudIndex(pts)
    spacing = cloud.nearest_spacing(base)
    s = spacing["median"]
    say(f"device {torch.cuda.get_device_name(0)}, cloud {M} points, box {base.info['box']}, nearest-neighbour spacing median {s:.6f} mean {spacing['mean']:.6f}")
    say(f"default_point_cell {base.info['cell']:.6f} ({base.info['cell'] / s:.2f} spacings), dims {base.info['dims']}, {base.nbytes / 2 ** 20:.1f} MiB")
    d = torch.randn(M, 3, device=DEV, generator=g)
    twin = (pts + 0.25 * s * d / d.norm(dim=1, keepdim=True)).contiguous()
    ref = None
    for f in FACTORS:
        cell = base.info["cell"] * f
        try:
            index = cloud.CloudIndex(pts, cell=cell, max_bytes=8 << 30)
        except ValueError as e:
            say(f"cell x {f:4.2f}: refused: {e}")
            continue
        out = index.closest(twin)
        if ref is not None:
            assert torch.equal(out["distance"].view(torch.int32), ref["distance"].view(torch.int32)) and torch.equal(out["index"], ref["index"])
        ref = out if ref is None else ref
        t_build, t_closest = alternate([lambda: cloud.CloudIndex(pts, cell=cell, max_bytes=8 << 30), lambda: index.closest(twin)], a.reps)
        say(f"cell x {f:4.2f} = {cell:.6f}: dims {index.info['dims']}, {index.nbytes / 2 ** 20:7.1f} MiB, build {fmt(t_build)}, closest twin {fmt(t_closest)} "
            f"({M / t_closest[0] / 1e3:7.1f} M points / s)")
    twins = float((ref["index"] == torch.arange(M, device=DEV, dtype=torch.int32)).float().mean())
    say(f"closest twin: {twins:.4f} of the answers are the twin, mean distance {float(ref['distance'].mean()) / s:.4f} spacings")
    for label, fn in (("knn k=1 exclude_self", lambda: base.knn(pts, 1, exclude_self=True)), ("knn k=8 exclude_self", lambda: base.knn(pts, 8, exclude_self=True)),
                      ("radius_count 2 spacings", lambda: base.radius_count(pts, 2 * s, exclude_self=True)),
                      ("radius_count 4 spacings", lambda: base.radius_count(pts, 4 * s, exclude_self=True)),
                      ("voxel_downsample 2 spacings", lambda: cloud.voxel_downsample(pts, 2 * s))):
        t = alternate([fn], a.reps)[0]
        say(f"{label:28s} {fmt(t)} ({M / t[0] / 1e3:7.1f} M points / s)")
    counts = base.radius_count(pts, 2 * s, exclude_self=True).float()
    say(f"radius_count 2 spacings: mean {float(counts.mean()):.2f} neighbours; voxel_downsample 2 spacings: {cloud.voxel_downsample(pts, 2 * s)['counts'][0]} clusters")
    faces = torch.arange(M, dtype=torch.int32, device=DEV)[:, None].expand(M, 3).contiguous()
    mesh = {"vertices": pts, "faces": faces, "rgb8": None, "counts": (M, M)}
    for label, cell in (("the cloud index's default cell", base.info["cell"]), ("the mesh index's default cell", None)):
        parent = mesh_distance.MeshIndex(mesh, cell=cell, max_bytes=8 << 30)
        new = base if cell is not None else cloud.CloudIndex(pts, cell=parent.info["cell"], max_bytes=8 << 30)
        old = parent.closest(twin, closest=True)
        got = new.closest(twin, closest=True)
        assert torch.equal(old["distance"].view(torch.int32), got["distance"].view(torch.int32)) and torch.equal(old["face"], got["index"])
        assert torch.equal(old["closest"].view(torch.int32), got["closest"].view(torch.int32))
        t_new, t_old = alternate([lambda: new.closest(twin, closest=True), lambda: parent.closest(twin, closest=True)], a.reps)
        b_new, b_old = alternate([lambda: cloud.CloudIndex(pts, cell=parent.info["cell"], max_bytes=8 << 30),
                                  lambda: mesh_distance.MeshIndex(mesh, cell=parent.info["cell"], max_bytes=8 << 30)], a.reps)
        say(f"at {label} {parent.info['cell']:.6f}: closest twin, cloud index {fmt(t_new)}, mesh index over (i, i, i) {fmt(t_old)}, ratio {t_old[0] / t_new[0]:.2f}; "
            f"build {fmt(b_new)} against {fmt(b_old)}, ratio {b_old[0] / b_new[0]:.2f}; index {new.nbytes / 2 ** 20:.1f} against {parent.nbytes / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
