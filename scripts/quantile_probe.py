"""Time of depth_quantiles.median_depth beside novel_views.render_poses and normals.render_normals, and of k_depth_quantiles
alone, on one MI355X over BASELINE configs[2] (bench.config3_scene: 4 blended 300^3 fields) at 640x360:

  render_poses / render_normals / median_depth / quartiles   the same N poses along the scene's frames, chunk 4096
  kernel alone   lrf_depth_quantiles_from_weights on 4096 x 512 weights, K = 1, q = 0.5: the crossing in the first 64-sample
                 step (the whole weight in sample 3) and never reached (all weights zero: every step is read)
Each variant runs 3 times untimed, then is timed `--reps` times between two HIP events, one run each; the median is reported.
Prints one JSON object; --out writes it as well.
Usage:  python scripts/quantile_probe.py [--poses 8] [--reps 5] [--out profiles/quantile_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available(), "quantile_probe needs the GPU"
    import bench
    from localrf_amd import _native as N
    from localrf_amd import depth_quantiles, normals, novel_views
    lt = bench.config3_scene(DEV)[0]
    W, H, n = 640, 360, args.poses
    c2w = lt.get_cam2world().detach()
    views = torch.linspace(0, c2w.shape[0] - 1, n).round().long().tolist()
    poses = c2w[views].contiguous()
    res = {"device": torch.cuda.get_device_name(0), "scene": "BASELINE configs[2]: 4 blended 300^3 fields (bench.config3_scene)",
           "W": W, "H": H, "poses": n, "reps": args.reps, "statistic": "median of reps single runs between HIP events"}
    cases = {"render_poses": lambda: novel_views.render_poses(lt, poses, W, H, frame_indices=views, encode=False),
             "render_normals": lambda: normals.render_normals(lt, poses, W, H, frame_indices=views),
             "median_depth": lambda: depth_quantiles.median_depth(lt, poses, W, H, frame_indices=views),
             "quartiles": lambda: depth_quantiles.render_depth_quantiles(lt, poses, W, H, (0.25, 0.5, 0.75), frame_indices=views)}
    for name, fn in cases.items():
        ms = event_ms(fn, args.reps)
        res[name] = {"ms_per_frame": ms / n, "frames_per_s": 1e3 * n / ms}
    res["median_over_poses"] = res["median_depth"]["ms_per_frame"] / res["render_poses"]["ms_per_frame"]
    res["median_over_normals"] = res["median_depth"]["ms_per_frame"] / res["render_normals"]["ms_per_frame"]
    med = cases["median_depth"]()
    exp = cases["render_poses"]()["depth"]
    res["pixels_without_median"] = int((med == 0).sum())
    res["mean_median_depth"], res["mean_expected_depth"] = float(med.mean()), float(exp.mean())
    R, S = 4096, 512
    z = torch.linspace(0.1, 6.0, S, device=DEV)
    rays = torch.randn(R, 6, device=DEV)
    depth = torch.empty(1, R, device=DEV)
    q = (C.c_float * 1)(0.5)
    kernel = {}
    for name, j in (("crossing_in_first_step", 3), ("never_reached", None)):
        w = torch.zeros(R, S, device=DEV)
        if j is not None:
            w[:, j] = 0.75
        ms = event_ms(lambda: N.launch("lrf_depth_quantiles_from_weights", torch.device(DEV), N.ptr(w), N.ptr(z), N.ptr(rays), R, S, q,
                                       1, N.ptr(depth), None), args.reps)
        kernel[name] = {"us": 1e3 * ms, "weight_bytes_read": 4 * R * (64 if j is not None else S)}
    res["kernel_alone"] = {"R": R, "S": S, "K": 1, **kernel}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
