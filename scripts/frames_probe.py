"""Timing of the device frame store (csrc/lrf_frames.inl, localrf_amd.DeviceFrames) on one GPU, one process.

  gather     lrf_frames_gather for 16 views x 256 rays (4096) with all seven outputs, out of a 960x540 window of 10
             frames: HIP events around the replay of a captured graph of 50 back-to-back gathers (after a warm-up),
             so the number is GPU time per gather, without host launch cost
  frame      activate_frames per 960x540 frame (staging, one host->device copy, two flow decodes, the sharpness weight),
             wall time with a synchronise at the end, 10 frames; against the numpy restatement of the same preparation
             (decode_flow x 2 times flow_scale, grey, Laplacian, float32 .var(), times the mask: tests/frames_cases.py)
  train      scripts/train_synth.py captured (--graph), ms per iteration at 64^3 and at the final 300^3, with and without
             --frames-store (the render path is the same: the difference is the gather and the weighted loss)
Prints one JSON object; --out writes it to a file as well.
Usage:  python scripts/frames_probe.py [--out profiles/frames_probe.json] [--no-train]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import frames_cases as fc
    from localrf_amd import DeviceFrames
    dev = torch.device("cuda:0")
    H, W, F_ = 540, 960, 10
    host = [fc.make_frame(i, H, W, flow_scale=540 / 271) for i in range(F_)]
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H]}

    t0 = time.perf_counter()
    st = DeviceFrames(host.__getitem__, F_, F_, n_init_frames=0, device=dev)
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    times = []
    for _ in range(F_):
        t0 = time.perf_counter()
        st.activate_frames(1)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ref = []
    for d in host[:5]:
        t0 = time.perf_counter()
        fc.decode_flow_scaled(d["encoded_fwd_flow"], d["flow_scale"])
        fc.decode_flow_scaled(d["encoded_bwd_flow"], d["flow_scale"])
        v = fc.sharpness_numpy_f32(d["img"])
        _ = np.ones_like(d["img"][..., 0]) * v * d["mask"]
        ref.append(time.perf_counter() - t0)
    res["frame_prepare_ms"] = {"device_median": 1e3 * statistics.median(times[1:]), "device_first": 1e3 * times[0],
                               "numpy_restatement_median": 1e3 * statistics.median(ref), "store_init_ms": 1e3 * t_init}

    V, n = 16, 256
    g = torch.Generator().manual_seed(0)
    views = torch.randint(0, F_, (V,), generator=g).to(dev)
    rays = torch.randint(0, H * W, (V * n,), generator=g).to(dev)
    for _ in range(3):
        st.gather(views, rays)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(50):
            st.gather(views, rays)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(10):
        e0.record(); graph.replay(); e1.record()
        e1.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / 50)
    res["gather_4096_us"] = {"median": statistics.median(per), "min": min(per), "outputs": 7, "errors": st.errors()}
    del graph, st
    torch.cuda.empty_cache()

    if not args.no_train:
        import train_synth
        tr = {}
        for store in (False, True):
            out = train_synth.run(graph=True, final=300, frames_store=store)
            ms = out["ms_per_iteration_by_resolution"]
            tr["frames_store" if store else "default"] = {"ms_per_iteration_64": ms.get("64"), "ms_per_iteration_300": ms.get("300"),
                                                          "iterations": out["iterations"], "loss_last": out["loss_last"],
                                                          "store_errors": (out["frames_store"] or {}).get("errors")}
        res["train_synth_graph"] = tr
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
