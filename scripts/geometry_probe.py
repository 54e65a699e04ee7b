"""Timing of the test-view geometry diagnostics (csrc/lrf_select.inl, csrc/lrf_evalgeo.inl, localrf_amd.diagnostics) on
one GPU, one process.

  select     diagnostics.quantile(q = 0.9) and median of B = 4 rows of n = 2^10 .. 2^22 values: HIP events around 20
             back-to-back calls after 5 warm-up calls (each call allocates its small workspace from torch's cache)
  per_view   flow_comparison + depth_comparison of one view at 480x270 and 960x540 (seeded synthetic inputs), same timing
  views      test_view_evaluation (metrics + flow + depth images) against test_view_metrics on the same 8 views of
             480x270 of a seeded 4-field scene, host clock around each call (both end in a host sync)
Prints one JSON object; --out writes it to a file as well.
Usage:  python scripts/geometry_probe.py [--out profiles/geometry_probe.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def event_ms(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def synthetic_view(W, H, rng):
    HW = W * H
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return dict(depth=d((1.0 + 3.0 * rng.random(HW)).astype(np.float32)),
                dirs=d(np.concatenate([rng.uniform(-0.5, 0.5, (HW, 2)), -np.ones((HW, 1))], 1).astype(np.float32)),
                ij=d(np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.int64)),
                flows=[d((2.0 * rng.standard_normal((H, W, 2))).astype(np.float32)) for _ in range(2)],
                masks=[d((rng.random((H, W)) < 0.8).astype(np.float32)) for _ in range(2)],
                inv=d((0.2 + rng.random((H, W))).astype(np.float32)))


def build_scene(W, H):
    from localrf_amd import LocalTensorfs
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import FIELD_KW
    torch.manual_seed(0)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]]).to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        lt = LocalTensorfs(fov=85.6, n_init_frames=5, n_overlap=3, WH=(W, H), n_iters_per_frame=600, n_iters_reg=100,
                           lr_R_init=5e-3, lr_t_init=5e-4, lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
                           lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[], camera_prior=None, device=DEV,
                           lr_upsample_reset=True, aabb=aabb, gridSize=[128, 128, 128], **FIELD_KW)
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            for _ in range(3):
                lt.append_frame()
                with torch.no_grad():
                    lt.t_c2w[-1].add_((0.05 * torch.randn(3, generator=g)).to(DEV))
            lt.append_rf(3)
    return lt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from localrf_amd import diagnostics, metrics
    assert torch.cuda.is_available(), "geometry_probe needs the GPU"
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "select": [], "per_view": []}
    for e in range(10, 23, 2):
        n = 1 << e
        x = torch.from_numpy(rng.standard_normal((4, n)).astype(np.float32)).to(DEV)
        res["select"].append({"B": 4, "n": n, "quantile_ms": event_ms(lambda: diagnostics.quantile(x, 0.9)),
                              "median_ms": event_ms(lambda: diagnostics.median(x))})
    for W, H in ((480, 270), (960, 540)):
        v = synthetic_view(W, H, rng)
        c2w = torch.eye(3, 4, device=DEV)[None].repeat(8, 1, 1)
        c2w[:, 0, 3] = torch.arange(8, device=DEV) * 0.01
        focal, center = torch.tensor([0.9 * W], device=DEV), torch.tensor([W / 2, H / 2], device=DEV)
        fl = lambda: diagnostics.flow_comparison(v["depth"], v["dirs"], v["ij"], c2w, 3, focal, center, v["flows"][0], v["masks"][0],  # noqa: E731
                                                 v["flows"][1], v["masks"][1], W, H)
        dp = lambda: diagnostics.depth_comparison(v["depth"], v["inv"], W, H)  # noqa: E731
        fms, dms = event_ms(fl), event_ms(dp)
        res["per_view"].append({"W": W, "H": H, "flow_ms": fms, "depth_ms": dms, "total_ms": event_ms(lambda: (fl(), dp()))})
    W, H, n = 480, 270, 8
    lt = build_scene(W, H)
    views = list(range(3, 3 + n))
    gen = torch.Generator().manual_seed(2)
    gt = torch.rand(n, H, W, 3, generator=gen).to(DEV)
    ff, bf = [(2 * torch.randn(n, H, W, 2, generator=gen)).to(DEV) for _ in range(2)]
    fm, bm = [(torch.rand(n, H, W, generator=gen) < 0.8).float().to(DEV) for _ in range(2)]
    inv = (0.2 + torch.rand(n, H, W, generator=gen)).to(DEV)
    t_eval, t_metrics = [], []
    for _ in range(4):
        t0 = time.perf_counter()
        metrics.test_view_metrics(lt, gt, views, W, H)
        t1 = time.perf_counter()
        diagnostics.test_view_evaluation(lt, views, W, H, gt_rgbs=gt, fwd_flow=ff, fwd_mask=fm, bwd_flow=bf, bwd_mask=bm, invdepths=inv)
        t2 = time.perf_counter()
        t_metrics.append(1e3 * (t1 - t0))
        t_eval.append(1e3 * (t2 - t1))
    res["views"] = {"W": W, "H": H, "n_views": n, "test_view_metrics_ms": sorted(t_metrics[1:])[1],
                    "test_view_evaluation_ms": sorted(t_eval[1:])[1], "runs_ms": {"metrics": t_metrics, "evaluation": t_eval}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
