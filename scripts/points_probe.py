"""Time of localrf_amd.pointcloud.fuse_points against the same computation as a PyTorch-ROCm op chain on the same GPU, for 64
frames of 360 x 640 on a synthetic consistent trajectory (an arc of cameras over a plane with a bump, 15 % floaters), with 0, 2
and 4 neighbours:

  fused    fuse_points(rgb8, depth, poses, focal, center, neighbours=..., rel_tol=0.02, min_consistent=min(2, n)): three
           launches and the read-back of the count
  kernels  the lrf_points_fuse call alone on preallocated buffers: the three launches, no read-back, no allocation
  chain    torch_chain below: the same arithmetic as eager torch ops (directions, world points, per offset the reprojection,
           rounding, gather and test, then boolean-mask compaction of xyz / rgb8 / src, whose nonzero reads the count back too)
Each variant runs 3 times untimed, then `--reps` times timed with HIP events, the variants interleaved (fused, kernels, chain,
fused, ...) so that clock and cache state are shared; the median is reported, with min and max.  bytes: the traffic the work
needs at least -- 4 B of depth per candidate, 4 B per candidate and neighbour gathered, 23 B (xyz, rgb8, src) per kept point.
Prints one JSON object; --out writes it as well.
Usage:  python scripts/points_probe.py [--frames 64] [--reps 15] [--out profiles/points_probe.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def trajectory(V, H, W, f, seed=0):
    """depth [V,H,W], rgb8, c2w [V,3,4]: cameras 0.05 apart in x, turned 0.01 rad about y per frame, over z = -4 - 0.3 sin x cos y."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = torch.arange(V, device=DEV, dtype=torch.float64) - (V - 1) / 2
    a = 0.01 * k
    c2w = torch.zeros(V, 3, 4, device=DEV, dtype=torch.float64)
    c2w[:, 0, 0], c2w[:, 0, 2], c2w[:, 1, 1], c2w[:, 2, 0], c2w[:, 2, 2] = a.cos(), a.sin(), 1.0, -a.sin(), a.cos()
    c2w[:, 0, 3] = 0.05 * k
    col = torch.arange(W, device=DEV, dtype=torch.float64)[None, :].expand(H, W)
    row = torch.arange(H, device=DEV, dtype=torch.float64)[:, None].expand(H, W)
    dirs = torch.stack([(col + 0.5 - W / 2) / f, -(row + 0.5 - H / 2) / f, -torch.ones_like(col)], -1)
    dw = torch.einsum("vrc,hwc->vhwr", c2w[:, :, :3], dirs)
    o = c2w[:, None, None, :, 3]
    t = (-4.0 - o[..., 2]) / dw[..., 2]
    for _ in range(8):                                                # fixed-point steps onto the bumpy surface
        p = o + t[..., None] * dw
        t = (-4.0 - 0.3 * torch.sin(p[..., 0]) * torch.cos(p[..., 1]) - o[..., 2]) / dw[..., 2]
    depth = t.float()
    floater = torch.rand(V, H, W, device=DEV, generator=g) < 0.15
    factor = torch.tensor([0.4, 0.55, 1.8], device=DEV)[torch.randint(0, 3, (V, H, W), device=DEV, generator=g)]
    depth = torch.where(floater, depth * factor, depth).contiguous()
    rgb8 = torch.randint(0, 256, (V, H, W, 3), device=DEV, dtype=torch.uint8, generator=g)
    return depth, rgb8, c2w.float().contiguous()


def torch_chain(depth, rgb8, c2w, f, cx, cy, neighbours, rel_tol, min_consistent):
    """fuse_points' arithmetic as eager torch ops (stride 1, no depth range) -> (xyz, rgb8, src)."""
    V, H, W = depth.shape
    col = torch.arange(W, device=DEV, dtype=torch.float32)[None, :]
    row = torch.arange(H, device=DEV, dtype=torch.float32)[:, None]
    x = ((col + 0.5 - cx) / f) * depth
    y = (-(row + 0.5 - cy) / f) * depth
    z = -depth
    M = c2w[:, None, None]
    pw = [((M[..., r, 0] * x + M[..., r, 1] * y) + M[..., r, 2] * z) + M[..., r, 3] for r in range(3)]
    keep = torch.isfinite(depth) & (depth > 0)
    if neighbours:
        passes = torch.zeros(V, H, W, dtype=torch.int32, device=DEV)
        in_range = torch.zeros(V, 1, 1, dtype=torch.int32, device=DEV)
        flat = depth.reshape(-1)
        for o in neighbours:
            lo, hi = max(0, -o), min(V, V - o)                       # frames v with v + o inside [0, V)
            if lo >= hi:
                continue
            Mn = c2w[lo + o:hi + o, None, None]
            d = [pw[r][lo:hi] - Mn[..., r, 3] for r in range(3)]
            q = [(Mn[..., 0, r] * d[0] + Mn[..., 1, r] * d[1]) + Mn[..., 2, r] * d[2] for r in range(3)]
            nz = -q[2]
            iu = torch.round(q[0] / nz * f + cx - 0.5)
            iw = torch.round(-q[1] / nz * f + cy - 0.5)
            ok = (nz > 0) & (iu >= 0) & (iu <= W - 1) & (iw >= 0) & (iw <= H - 1)
            n_idx = torch.arange(lo + o, hi + o, device=DEV)[:, None, None]
            idx = (n_idx * H + iw.clamp(0, H - 1).long()) * W + iu.clamp(0, W - 1).long()
            dn = flat[torch.where(ok, idx, torch.zeros_like(idx))]
            ok &= torch.isfinite(dn) & (dn > 0) & ((nz - dn).abs() <= rel_tol * dn)
            passes[lo:hi] += ok
            in_range[lo:hi] += 1
        keep &= passes >= in_range.clamp(max=min_consistent)
    xyz = torch.stack(pw, -1)[keep]
    src = keep.reshape(V, -1).nonzero().int()
    return xyz, rgb8[keep], src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available(), "points_probe needs the GPU"
    from localrf_amd import _native as N
    from localrf_amd import pointcloud
    V, H, W, f = args.frames, 360, 640, 500.0
    cx, cy = W / 2, H / 2
    depth, rgb8, c2w = trajectory(V, H, W, f)
    focal, center = torch.tensor([f], device=DEV), torch.tensor([cx, cy], device=DEV)
    lib = N.lib()
    P = V * H * W
    ws = torch.empty(lib.lrf_points_workspace_bytes(V, H, W, 1), dtype=torch.uint8, device=DEV)
    xyz, src = torch.empty(P, 3, device=DEV), torch.empty(P, 2, dtype=torch.int32, device=DEV)
    out8, count = torch.empty(P, 3, dtype=torch.uint8, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    res = {"device": torch.cuda.get_device_name(0), "frames": V, "H": H, "W": W, "reps": args.reps, "cases": []}
    for neigh in ((), (-1, 1), (-2, -1, 1, 2)):
        mc = min(2, len(neigh))
        a = N.LrfPointsFuse()
        a.depth, a.rgb8, a.cam2world, a.focal, a.center = depth.data_ptr(), rgb8.data_ptr(), c2w.data_ptr(), focal.data_ptr(), center.data_ptr()
        a.V, a.H, a.W, a.fov360, a.stride, a.d_min, a.d_max = V, H, W, 0, 1, 0.0, math.inf
        a.n_neigh, a.rel_tol, a.min_consistent = len(neigh), 0.02, mc
        for k, o in enumerate(neigh):
            a.neigh[k] = o
        st = torch.cuda.current_stream().cuda_stream

        def fused():
            return pointcloud.fuse_points(rgb8, depth, c2w, focal, center, neighbours=neigh, rel_tol=0.02, min_consistent=mc)

        def kernels():
            N.check(lib.lrf_points_fuse(C.byref(a), P, xyz.data_ptr(), out8.data_ptr(), src.data_ptr(), count.data_ptr(),
                                        ws.data_ptr(), st), "lrf_points_fuse")

        def chain():
            return torch_chain(depth, rgb8, c2w, f, cx, cy, neigh, 0.02, mc)
        variants = (("fused", fused), ("kernels", kernels), ("chain", chain))
        for _ in range(3):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        got, ref = fused(), chain()
        M = got["count"]
        same = ref[0].shape[0] == M and bool(torch.equal(ref[2], got["src"])) and bool(torch.equal(ref[1], got["rgb8"]))
        row = {"neighbours": list(neigh), "min_consistent": mc, "kept": M, "kept_share": M / P,
               "chain_gives_the_same_points": same,
               "chain_max_abs_xyz_diff": float((ref[0] - got["xyz"]).abs().max()) if same and M else None,
               "min_bytes": 4 * P * (1 + len(neigh)) + 23 * M}
        for name in times:
            t = sorted(times[name])
            row[name + "_ms"] = {"median": statistics.median(t), "min": t[0], "max": t[-1]}
            row[name + "_GBps"] = row["min_bytes"] / (statistics.median(t) * 1e-3) / 1e9
        row["chain_over_fused"] = row["chain_ms"]["median"] / row["fused_ms"]["median"]
        row["chain_over_kernels"] = row["chain_ms"]["median"] / row["kernels_ms"]["median"]
        res["cases"].append(row)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
