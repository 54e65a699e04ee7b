"""Time of normals.render_normals beside novel_views.render_poses, and of lrf_density_gradient beside lrf_density_feature, on
one MI355X over BASELINE configs[2] (bench.config3_scene: 4 blended 300^3 fields) at 640x360:

  render_poses    colour and depth of N poses along the scene's frames, not encoded, chunk 4096 (as the renderer calls it)
  render_normals  the normal map and acc of the same poses, chunk 4096 and chunk 65536
  feature / gradient   TensorVMSplit.compute_densityfeature and density_gradient of P uniform points in [-1, 1]^3
Each variant runs 3 times untimed, then `--reps` times between two HIP events; the mean per run is reported.
Prints one JSON object; --out writes it as well.
Usage:  python scripts/normals_probe.py [--poses 8] [--reps 5] [--points 4194304] [--out profiles/normals_probe.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def event_ms(fn, reps):
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
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available(), "normals_probe needs the GPU"
    import bench
    from localrf_amd import normals, novel_views
    lt = bench.config3_scene(DEV)[0]
    W, H, n = 640, 360, args.poses
    c2w = lt.get_cam2world().detach()
    views = torch.linspace(0, c2w.shape[0] - 1, n).round().long().tolist()
    poses = c2w[views].contiguous()
    res = {"device": torch.cuda.get_device_name(0), "scene": "BASELINE configs[2]: 4 blended 300^3 fields (bench.config3_scene)",
           "W": W, "H": H, "poses": n, "reps": args.reps}
    cases = {"render_poses_chunk4096": lambda: novel_views.render_poses(lt, poses, W, H, frame_indices=views, encode=False),
             "render_normals_chunk4096": lambda: normals.render_normals(lt, poses, W, H, frame_indices=views),
             "render_normals_chunk65536": lambda: normals.render_normals(lt, poses, W, H, frame_indices=views, chunk=65536)}
    for name, fn in cases.items():
        ms = event_ms(fn, args.reps)
        res[name] = {"ms_per_frame": ms / n, "frames_per_s": 1e3 * n / ms}
    out = normals.render_normals(lt, poses, W, H, frame_indices=views)
    res["mean_acc"] = float(out["acc"].mean())
    res["mean_normal_length"] = float(out["normal"].norm(dim=-1).mean())
    res["normals_over_poses"] = res["render_normals_chunk4096"]["ms_per_frame"] / res["render_poses_chunk4096"]["ms_per_frame"]
    f = lt.tensorfs[0]
    u = torch.rand(args.points, 3, device=DEV) * 2 - 1
    feat_ms = event_ms(lambda: f.compute_densityfeature(u), args.reps)
    grad_ms = event_ms(lambda: f.density_gradient(u), args.reps)
    res["points"] = {"P": args.points, "density_feature_ms": feat_ms, "density_gradient_ms": grad_ms,
                     "gradient_over_feature": grad_ms / feat_ms, "gradient_Gpoints_per_s": args.points / grad_ms / 1e6}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
