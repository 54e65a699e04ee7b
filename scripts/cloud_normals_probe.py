"""Timing of point-cloud normals (csrc/lrf_cloud.inl item 9) and of one point-to-plane ICP iteration against a cloud
(csrc/lrf_align.inl item 4), on scripts/cloud_probe.py's cloud: --points points of the back-projected depth of
scripts/mesh_probe.py's frames (a sphere before a wall, 16 views), shuffled.

  normals   estimate_normals at 2 and 4 median spacings, order="input" against order="records", and radius_count at the same
            radius -- what the walk alone costs -- timed ALTERNATELY, one run of each per repetition, in the same process; the
            bytes of the two orders are asserted equal
  icp       one plane iteration against the cloud's index with its normals at 4 spacings, split into transform, closest
            (CloudIndex.closest with closest=True), accumulate (lrf_align_plane_cloud, and lrf_align_pairs for
            metric="point"), read-back plus host solve; then one whole icp iteration of either metric.  The source is
            --source points of the same cloud, every one moved by a quarter of the median spacing in a random direction and
            then by the inverse of a small rigid motion

  python scripts/cloud_normals_probe.py [--points 1000000] [--source 1000000] [--reps 7]
Prints one line per measurement: the median of --reps runs after one warm-up, between device events, with the smallest and
largest run; the read-back and solve by the host clock, since it ends in the copy's synchronise."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import alignment, cloud, pointcloud  # noqa: E402
from cloud_probe import alternate, fmt, say  # noqa: E402
from mesh_probe import DEV, FOCAL, H, W, frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--source", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    depth, rgb8, c2w = frames(16)
    pts = pointcloud.backproject(depth, c2w, W, H, FOCAL, (W / 2, H / 2))[0]
    pts = pts[torch.isfinite(pts).all(1)]
    g = torch.Generator(device=DEV).manual_seed(1)
    pts = pts[torch.randperm(pts.shape[0], device=DEV, generator=g)[:a.points]].contiguous()
    M = pts.shape[0]
    index = cloud.CloudIndex(pts)
    s = cloud.nearest_spacing(index)["median"]
    say(f"device {torch.cuda.get_device_name(0)}, cloud {M} points, spacing median {s:.6f}, cell {index.info['cell']:.6f} ({index.info['cell'] / s:.2f} spacings), "
        f"dims {index.info['dims']}")
    for k in (2.0, 4.0):
        r = k * s
        one, two = (cloud.estimate_normals(index, r, order=o) for o in cloud.NORMAL_ORDERS)
        assert all(torch.equal(one[key].view(torch.int32), two[key].view(torch.int32)) for key in ("normals", "eigenvalues", "count"))
        count = one["count"].float()
        t_in, t_rec, t_count = alternate([lambda: cloud.estimate_normals(index, r, order="input"), lambda: cloud.estimate_normals(index, r, order="records"),
                                          lambda: index.radius_count(pts, r)], a.reps)
        say(f"{k:.0f} spacings ({float(count.mean()):.2f} neighbours on average, {float((one['normals'] == 0).all(1).float().mean()):.4f} without a normal): "
            f"estimate_normals input order {fmt(t_in)} ({M / t_in[0] / 1e3:.1f} M points / s), record order {fmt(t_rec)} ({M / t_rec[0] / 1e3:.1f} M points / s), "
            f"ratio {t_in[0] / t_rec[0]:.2f}; radius_count {fmt(t_count)}")
    normals = cloud.estimate_normals(index, 4 * s)["normals"]
    n = min(a.source, M)
    d = torch.randn(n, 3, device=DEV, generator=g)
    on = (pts[:n] + 0.25 * s * d / d.norm(dim=1, keepdim=True)).contiguous()
    axis = np.array((1.0, 2.0, -1.0)) / math.sqrt(6.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(0.002) * K + (1 - math.cos(0.002)) * (K @ K)
    lo, hi = index.info["box"]
    centre = np.array([(l + h) / 2 for l, h in zip(lo, hi)])
    truth = alignment.similarity(1.0, R, centre - R @ centre + 2 * s * np.array((1.0, -1.0, 0.5)))
    src = alignment.transform_points(on, alignment.inverse(truth))
    reach = 16 * s
    T = np.eye(4)
    cur = torch.empty_like(src)
    c = tuple(float(x) for x in centre)
    u = alignment._power_of_two_at_least(max(h - l for l, h in zip(lo, hi)) + 2 * reach)
    c0, h0 = alignment.pair_frame(tuple(l - reach for l in lo), tuple(x + reach for x in hi))
    alignment._transform_into(src, T, cur)
    near = index.closest(cur, reach, closest=True)
    keep = (near["distance"] <= reach).to(torch.uint8)
    words = alignment._plane_words(index, cur, near, c, u, reach, normals)

    def back():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = alignment.solve_plane(alignment._add_words(words.cpu()), False)
        if sol["omega"] is not None:
            alignment.compose(alignment.plane_update(sol, c, u), T)
        return (time.perf_counter() - t0) * 1e3
    say(f"icp: source {n} points, max_distance {reach:.6f} (16 spacings)")
    rows = [("transform (lrf_align_transform)", lambda: alignment._transform_into(src, T, cur)),
            ("closest (lrf_cloud_closest, closest=True)", lambda: index.closest(cur, reach, closest=True)),
            ("accumulate, plane (lrf_align_plane_cloud)", lambda: alignment._plane_words(index, cur, near, c, u, reach, normals)),
            ("accumulate, point (lrf_align_pairs)", lambda: alignment._pair_words(c0, h0, cur, near["closest"], keep)),
            ("icp, one iteration, plane (whole call)", lambda: alignment.icp(src, index, iterations=1, max_distance=reach, scale=False, target_normals=normals)),
            ("icp, one iteration, point (whole call)", lambda: alignment.icp(src, index, iterations=1, max_distance=reach, scale=False, metric="point"))]
    for name, fn in rows:
        say(f"{name:44s} {fmt(alternate([fn], a.reps)[0])}")
    say(f"{'read-back + host solve (host clock)':44s} {float(np.median([back() for _ in range(a.reps)])):9.3f} ms")
    for metric, extra in (("plane", dict(target_normals=normals)), ("point", dict())):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = alignment.icp(src, index, max_distance=reach, scale=False, metric=metric, iterations=30, **extra)
        ms = (time.perf_counter() - t0) * 1e3
        (_, R1, t1), (_, R0, t0_) = alignment.decompose(out["T"]), alignment.decompose(truth)
        say(f"icp {metric} to the end: {out['iterations']} iterations ({out['reason']}), {ms:.1f} ms, count {out['count']}, rms {out['rms'] / s:.3f} spacings; "
            f"rotation off by {np.abs(R1 - R0).max():.2e}, translation by {np.abs(t1 - t0_).max() / s:.3f} spacings")


if __name__ == "__main__":
    main()
