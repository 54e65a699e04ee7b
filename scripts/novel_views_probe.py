"""Frames per second of novel-view rendering (localrf_amd.novel_views) on one GPU, on the 4 x 300^3 scene of BASELINE
configs[2] (bench.config3_scene), over a smooth camera path of N poses through the scene's 14 frames, at 640x360 and at
240x136 (where several frames per call matter):

  forward      bare per-frame LocalTensorfs.forward(ray_ids, [nearest], W, H, is_train=False, cam2world=pose[None]), no encoding
  render       (a) render_poses: device tensors, encoded (rgb8 / depth8), frames batched per lrf_scene_fwd call
  render_fpc1  render_poses with frames_per_call=1
  iter         (b) iter_pose_frames consumed to host numpy arrays
  host_loop    (c) the reference's shape: per-frame forward, .cpu(), the numpy visualize_depth index image and colour lookup,
               the rgb bytes in numpy
  encode_ms    encode_frames alone on one frame and on a batch of 16 (HIP events)
Each variant runs once untimed, then twice timed (host clock, ending in a device synchronise); the better run is kept.
Prints one JSON object; --out writes it as well.  --quick: 24 poses, one size (for a kernel trace).
Usage:  python scripts/novel_views_probe.py [--quick] [--out profiles/novel_views_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def path_poses(c2w, n):
    """n poses along the frames' poses: translations and rotation columns interpolated linearly, then re-orthonormalised."""
    c2w = c2w.detach().cpu().double()
    F = c2w.shape[0]
    s = torch.linspace(0, F - 1, n, dtype=torch.float64)
    i0 = s.floor().long().clamp(max=F - 2)
    w = (s - i0)[:, None, None]
    p = (1 - w) * c2w[i0] + w * c2w[i0 + 1]
    z = torch.nn.functional.normalize(p[:, :, 2], dim=-1)
    x = torch.nn.functional.normalize(torch.linalg.cross(p[:, :, 1], z, dim=-1), dim=-1)
    y = torch.linalg.cross(z, x, dim=-1)
    return torch.stack([x, y, z, p[:, :, 3]], -1).float().to(DEV)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def event_ms(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--poses", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available(), "novel_views_probe needs the GPU"
    import bench
    from localrf_amd import novel_views
    from localrf_amd.pose_plan import PosePlan
    from novel_views_cases import depth_idx_host, rgb8_host
    lt = bench.config3_scene(DEV)[0]
    n = 24 if args.quick else args.poses
    poses = path_poses(lt.get_cam2world(), n)
    views = novel_views.nearest_frames(lt, poses).tolist()
    tests = [3, 8]
    lut = novel_views.jet_lut()
    res = {"device": torch.cuda.get_device_name(0), "scene": "BASELINE configs[2]: 4 blended 300^3 fields (bench.config3_scene)",
           "poses": n, "sizes": []}
    for W, H in ((640, 360),) if args.quick else ((640, 360), (240, 136)):
        ray_ids = torch.arange(W * H, dtype=torch.int64, device=DEV)

        def forward():
            with torch.no_grad():
                for p, v in zip(poses, views):
                    lt(ray_ids, [v], W, H, is_train=False, cam2world=p[None], test_id=v in tests, chunk=4096, floater_thresh=0.5)

        def host_loop():
            with torch.no_grad():
                for p, v in zip(poses, views):
                    rgb, depth, _, _ = lt(ray_ids, [v], W, H, is_train=False, cam2world=p[None], test_id=v in tests, chunk=4096,
                                          floater_thresh=0.5)
                    rgb, depth = rgb.reshape(H, W, 3).cpu().numpy(), depth.reshape(H, W).cpu().numpy()
                    rgb8_host(rgb)
                    lut[depth_idx_host(depth, [0, 5])[0]]

        render = lambda fpc=None: novel_views.render_poses(lt, poses, W, H, test_frames=tests, floater_thresh=0.5,  # noqa: E731
                                                           frames_per_call=fpc)
        it = lambda: list(novel_views.iter_pose_frames(lt, poses, W, H, test_frames=tests, floater_thresh=0.5))  # noqa: E731
        row = {"W": W, "H": H}
        for name, fn in (("forward", forward), ("render", render), ("render_fpc1", lambda: render(1)), ("iter", it),
                         ("host_loop", host_loop)):
            dt = timed(fn)
            row[name] = {"s": dt, "frames_per_s": n / dt}
        row["calls"] = len(PosePlan(lt, poses, W, H, tests).groups)
        out = render()
        one = (out["rgb"][:1].contiguous(), out["depth"][:1].contiguous())
        many = (out["rgb"][:16].contiguous(), out["depth"][:16].contiguous())
        row["encode_ms"] = {"1_frame": event_ms(lambda: novel_views.encode_frames(*one)),
                            "16_frames": event_ms(lambda: novel_views.encode_frames(*many)),
                            "16_frames_auto_range": event_ms(lambda: novel_views.encode_frames(*many, minmax=None))}
        f = row["forward"]["frames_per_s"]
        row["ratios"] = {"render_over_forward": row["render"]["frames_per_s"] / f,
                         "iter_over_render": row["iter"]["frames_per_s"] / row["render"]["frames_per_s"],
                         "render_over_fpc1": row["render"]["frames_per_s"] / row["render_fpc1"]["frames_per_s"],
                         "render_over_host_loop": row["render"]["frames_per_s"] / row["host_loop"]["frames_per_s"]}
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
