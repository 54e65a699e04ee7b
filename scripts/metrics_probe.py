"""Timing of the test-view metrics (csrc/lrf_metrics.inl, localrf_amd.metrics) on one GPU, one process.

  kernel     lrf_image_metrics (the kernel pair) at 960x540 and 1920x1080, B = 1 and 8: HIP events around 20 back-to-back
             launches after 5 warm-up launches, preallocated buffers (no allocation, no host work between launches)
  host       the reference's evaluation on this machine's host: the scipy.signal.convolve2d SSIM of utils/utils.py:232-287
             (restated here; 3 runs, median) for one frame pair of each size
  views      test_view_metrics over 20 views of 480x270 (train.py's vis_every size: W/2 x H/2) of a 4-field 300^3 scene,
             against render + .cpu() + host SSIM and fp32 MSE per view (renderer.py:65-77,158-163); the render alone is
             timed too, so the metrics' share of test_view_metrics is reported
Prints one JSON object; --out writes it to a file as well.
Usage:  python scripts/metrics_probe.py [--out profiles/metrics_probe.json]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scipy_ssim(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """The reference's evaluation SSIM as it runs there: numpy / scipy in fp64 on the host."""
    import scipy.signal
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    filt = np.exp(-0.5 * ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2)
    filt /= np.sum(filt)

    def blur(z):
        return np.stack([scipy.signal.convolve2d(scipy.signal.convolve2d(z[..., i], filt[:, None], mode="valid"),
                                                 filt[None, :], mode="valid") for i in range(z.shape[-1])], -1)
    mu0, mu1 = blur(img0), blur(img1)
    s00 = np.maximum(0.0, blur(img0 ** 2) - mu0 * mu0)
    s11 = np.maximum(0.0, blur(img1 ** 2) - mu1 * mu1)
    s01 = blur(img0 * img1) - mu0 * mu1
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return np.mean((2 * mu0 * mu1 + c1) * (2 * s01 + c2) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2)))


def kernel_ms(dev, B, H, W, warmup=5, iters=20):
    from localrf_amd import _native as N
    g = torch.Generator(device=dev).manual_seed(B * 7 + H)
    a = torch.rand(B, H, W, 3, device=dev, generator=g)
    b = (a + 0.05 * torch.randn(a.shape, device=dev, generator=g)).clamp(0, 1)
    m = N.LrfImageMetrics()
    m.img0, m.img1, m.B, m.H, m.W, m.filter_size = a.data_ptr(), b.data_ptr(), B, H, W, 11
    m.max_val, m.filter_sigma, m.k1, m.k2 = 1.0, 1.5, 0.01, 0.03
    lib = N.lib()
    ws = torch.empty(lib.lrf_image_metrics_workspace_bytes(B, H, W, 11), dtype=torch.uint8, device=dev)
    out = torch.empty(2, B, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        N.check(lib.lrf_image_metrics(C.byref(m), None, out[1].data_ptr(), out[0].data_ptr(), ws.data_ptr(), st), "lrf_image_metrics")
    for _ in range(warmup):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return {"B": B, "H": H, "W": W, "ms": ms, "ms_per_frame": ms / B,
            "read_GBps": 2 * B * H * W * 3 * 4 / (ms * 1e-3) / 1e9}


def host_ms(H, W, runs=3):
    rng = np.random.default_rng(H)
    a = rng.random((H, W, 3), dtype=np.float32)
    b = np.clip(a + 0.05 * rng.standard_normal(a.shape), 0, 1).astype(np.float32)
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        scipy_ssim(a, b, 1.0)
        t.append((time.perf_counter() - t0) * 1e3)
    return {"H": H, "W": W, "ms": statistics.median(t), "runs": runs}


def scene(dev, grid=300):
    """Four overlapping grid^3 fields over 14 frames (the construction of BASELINE.json configs[2])."""
    from localrf_amd import LocalTensorfs
    fkw = dict(density_n_comp=[8, 8, 8], appearance_n_comp=[24, 24, 24], app_dim=27, shadingMode="MLP_Fea_late_view",
               near_far=[0.1, 1e3], density_shift=-5, alphaMask_thres=1e-4, distance_scale=25, rayMarch_weight_thres=1e-3,
               pos_pe=0, view_pe=0, fea_pe=0, featureC=128, step_ratio=0.5, fea2denseAct="softplus")
    torch.manual_seed(33)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    with contextlib.redirect_stdout(io.StringIO()):
        lt = LocalTensorfs(fov=85.6, n_init_frames=5, n_overlap=3, WH=(960, 540), n_iters_per_frame=600, n_iters_reg=100,
                           lr_R_init=5e-3, lr_t_init=5e-4, lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02,
                           rf_lr_basis=1e-3, lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[],
                           camera_prior=None, device="cpu", lr_upsample_reset=True, aabb=aabb, gridSize=[grid] * 3, **fkw)
        g = torch.Generator().manual_seed(34)
        for _ in range(3):
            for _ in range(3):
                lt.append_frame()
                with torch.no_grad():
                    lt.t_c2w[-1].add_(0.05 * torch.randn(3, generator=g))
                    lt.r_c2w[-1].add_(0.05 * torch.randn(3, 2, generator=g))
            lt.append_rf(3)
    lt = lt.to(dev)
    lt.device = torch.device(dev)
    for f in lt.tensorfs:
        f.to(dev)
    return lt


def views_ms(dev, n_views=20, W=480, H=270):
    from localrf_amd import metrics
    lt = scene(dev)
    views = [i % len(lt.r_c2w) for i in range(n_views)]
    gt = torch.rand(n_views, H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    ray_ids = torch.arange(W * H, device=dev)

    def render_only():
        with torch.no_grad():
            for v in views:
                lt(ray_ids, [v], W, H, is_train=False, cam2world=None, test_id=True, chunk=4096)
        torch.cuda.synchronize()

    def on_device():
        metrics.test_view_metrics(lt, gt, views, W, H)

    gt_host = gt.cpu()

    def host_path():                                          # renderer.py:65-77,158-163
        out = {}
        with torch.no_grad():
            for i, v in enumerate(views):
                rgb = lt(ray_ids, [v], W, H, is_train=False, cam2world=None, test_id=True, chunk=4096)[0]
                rgb = rgb.reshape(H, W, 3).cpu()
                out[v] = (float(((gt_host[i] - rgb) ** 2).mean()), scipy_ssim(gt_host[i].numpy(), rgb.numpy(), 1.0))
        return out

    res = {}
    for name, fn, reps in (("render_only", render_only, 3), ("test_view_metrics", on_device, 3), ("render_cpu_host_ssim", host_path, 1)):
        fn()                                                  # warm-up
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = statistics.median(t)
    res["metrics_share_of_test_view_metrics"] = 1.0 - res["render_only_ms"] / res["test_view_metrics_ms"]
    res.update({"views": n_views, "W": W, "H": H, "fields": len(lt.tensorfs), "grid": 300})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-views", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    with contextlib.redirect_stdout(io.StringIO()):
        ge.build()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernel": [], "host_reference_ssim": []}
    for (H, W) in ((540, 960), (1080, 1920)):
        for B in (1, 8):
            res["kernel"].append(kernel_ms(dev, B, H, W))
        res["host_reference_ssim"].append(host_ms(H, W))
    if not args.skip_views:
        res["test_views"] = views_ms(dev)
    s = json.dumps(res)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
