"""Cost of the deterministic backward (LRF_FLAG_DETERMINISTIC) against the default mode, one JSON line:
  * forward + backward (lrf_render_fwd_train + lrf_render_bwd through autograd) of a random TensorVMSplit, 4096 rays, at 300^3
    (512 samples, BASELINE configs[1]) and 500^3 (the grid's default sample count);
  * the captured progressive loop of scripts/train_synth.py (the bench's progressive_loop workload, graph mode), ms per
    iteration at each grid size it reaches, with torch.use_deterministic_algorithms off / on.
Usage: python scripts/deterministic_probe.py [--steps 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FIELD_KW = dict(density_n_comp=[8, 8, 8], appearance_n_comp=[24, 24, 24], app_dim=27, shadingMode="MLP_Fea_late_view",
                near_far=[0.1, 1e3], density_shift=-5, alphaMask_thres=1e-4, distance_scale=25, rayMarch_weight_thres=1e-3,
                pos_pe=0, view_pe=0, fea_pe=0, featureC=128, step_ratio=0.5, fea2denseAct="softplus")


def fwd_bwd_ms(grid, n_samples, steps, dev):
    from localrf_amd import TensorVMSplit
    torch.manual_seed(0)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    f = TensorVMSplit(torch.device("cpu"), aabb, [grid] * 3, **FIELD_KW).to(dev)
    g = torch.Generator().manual_seed(1)
    rays = torch.cat([0.05 * torch.randn(4096, 3, generator=g), torch.randn(4096, 3, generator=g)], -1).to(dev)
    gr, gd = torch.randn(4096, 3, device=dev), torch.randn(4096, device=dev)
    out = {}
    for mode in ("default", "deterministic", "default_again"):
        f.deterministic = mode == "deterministic"

        def step():
            for p in f.parameters():
                p.grad = None
            rgb, depth = f(rays, white_bg=True, is_train=True, N_samples=n_samples)
            ((rgb * gr).sum() + (depth * gd).sum()).backward()
        for _ in range(3):
            step()
        best = None
        for _ in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                step()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / steps
            best = ms if best is None else min(best, ms)
        out[mode + "_ms"] = best
    out["ratio"] = out["deterministic_ms"] / min(out["default_ms"], out["default_again_ms"])
    del f
    torch.cuda.empty_cache()
    return out


def captured_loop(dev):
    import train_synth
    out = {}
    for mode in ("default", "deterministic"):
        was = torch.are_deterministic_algorithms_enabled()
        try:
            torch.use_deterministic_algorithms(mode == "deterministic")
            r = train_synth.run(frames=8, final=200, iters_per_frame=600, n_max_frames=6, max_iters=2400, dev=str(dev), graph=True)
        finally:
            torch.use_deterministic_algorithms(was)
        out[mode] = r["ms_per_iteration_by_resolution"]
    out["ratio"] = {k: out["deterministic"][k] / out["default"][k] for k in out["default"] if k in out["deterministic"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"fwd_bwd_300": fwd_bwd_ms(300, 1536, args.steps, dev), "fwd_bwd_500": fwd_bwd_ms(500, -1, args.steps, dev),
           "captured_loop": captured_loop(dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
