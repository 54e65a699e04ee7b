"""Median and quantile ray depth of a scene on the GPU (csrc/lrf_quantile.inl through lrf_render_depth_quantiles): the depth
a fusion wants, where novel_views.render_poses gives the expected depth the reference's losses want.

  render_depth_quantiles(local_tensorfs, poses, W, H, q=(0.5,), ...)  the depth maps [K,N,H,W] and acc [N,H,W] of every pose
  median_depth(local_tensorfs, poses, W, H, ...)                      q = 0.5 alone, [N,H,W]
  fusion_depth(local_tensorfs, poses, W, H, max_spread, ...)          what scene_point_cloud / scene_mesh fuse with depth="median"

A field's quantile depth is the distance at which the accumulated weight of the ray first reaches q, interpolated linearly in
accumulated weight inside the crossing sample's interval (TensorVMSplit.render_depth_quantiles); it lies on a surface the ray
met, where the expected depth of a ray that sees two surfaces lies in the empty space between them.  A scene's is
sum_k blend_w[v, k] d_k / sum_k blend_w[v, k] [found_k] over the active fields that reach q: a field without a crossing does
not drag the pixel towards zero, and a pixel no field crosses is exactly 0 -- "no depth" to fuse_points, backproject and
TsdfVolume.integrate.  Every function checks its arguments before its first launch.  CPU tensors raise NativeError: there is
no torch fallback.
"""
import math

import torch

from .pose_plan import PosePlan

MAX_QUANTILES = 4


def check_q(q):
    """q -> a tuple of 1..4 floats, each in (0, 1]; ValueError otherwise."""
    try:
        q = tuple(float(v) for v in q)
    except TypeError:
        q = (float(q),)
    if not 1 <= len(q) <= MAX_QUANTILES:
        raise ValueError(f"q must hold 1 to {MAX_QUANTILES} quantiles, got {len(q)}")
    if not all(0.0 < v <= 1.0 for v in q):
        raise ValueError(f"every q must lie in (0, 1], got {q}")
    return q


def render_depth_quantiles(local_tensorfs, poses, W, H, q=(0.5,), test_frames=(), frame_indices=None, start=0, floater_thresh=0,
                           chunk=4096):
    """The quantile depth maps of every pose: frame i at its pose through the blending weights of its nearest training frame,
    as novel_views.render_poses chooses it (poses, frame_indices and start mean what they mean there; test_frames is accepted
    for the same call shape and changes nothing, because exposure does not apply to a depth).  q: 1 to 4 quantiles in (0, 1],
    any order.  chunk bounds the rays of one field call, and with them the [chunk, S] sample weights the call keeps; the
    result does not depend on it, bit for bit.
    Returns {"depth": [K,N,H,W] fp32, "acc": [N,H,W] fp32} on the scene's device: depth = sum_k blend_w d_k / sum_k blend_w
    [found_k] where some field reaches q and exactly 0 elsewhere, acc = sum_k blend_w acc_k.  Raises ValueError before any
    launch for a frame whose nearest frame has no active field."""
    q = check_q(q)
    plan = PosePlan(local_tensorfs, poses, W, H, test_frames, frame_indices, start, None, chunk).on_device()
    n, W, H, dev, K = plan.n, plan.W, plan.H, plan.dev, len(q)
    depth = torch.empty(K, n, H, W, dtype=torch.float32, device=dev)
    acc = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        # per span of rays, the active fields add bw depth and bw [found] in the reference's field order into the span's own
        # [K, n] sums, which are divided and stored at the end of the span
        for i0, i1, active in plan.calls:
            d, a = depth[:, i0:i1].view(K, -1), acc[i0:i1].view(-1)
            for r0, r1, calls in plan.group_spans(i0, i1, active):
                dsum = torch.empty(K, r1 - r0, dtype=torch.float32, device=dev)
                wsum = torch.empty_like(dsum)
                for k, (f, z, flags, rays, bw) in enumerate(calls):
                    f._native_depth_quantiles(rays, z, flags, float(floater_thresh), q, blend_w=bw, per_view=W * H,
                                              out=(dsum, wsum, a[r0:r1]), accumulate=k > 0)
                d[:, r0:r1] = torch.where(wsum > 0, dsum / wsum, torch.zeros_like(dsum))
    return {"depth": depth, "acc": acc}


def median_depth(local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, floater_thresh=0, chunk=4096):
    """render_depth_quantiles with q = (0.5,): the median depth [N,H,W] of every pose."""
    return render_depth_quantiles(local_tensorfs, poses, W, H, (0.5,), test_frames, frame_indices, start, floater_thresh,
                                  chunk)["depth"][0]


def check_fusion_depth(who, depth, max_spread):
    """The depth= / max_spread= arguments of scene_point_cloud and scene_mesh -> max_spread as a float or None."""
    if depth not in ("expected", "median"):
        raise ValueError(f"{who}: depth must be 'expected' or 'median', got {depth!r}")
    if max_spread is None:
        return None
    if depth != "median":
        raise ValueError(f"{who}: max_spread needs depth='median'")
    max_spread = float(max_spread)
    if not (max_spread >= 0 and math.isfinite(max_spread)):
        raise ValueError(f"{who}: max_spread must be a finite number >= 0, got {max_spread}")
    return max_spread


def spread_filter(d25, d50, d75, max_spread):
    """d50 where all three quartile depths exist (> 0) and (d75 - d25) <= max_spread * d50, else 0."""
    keep = (d25 > 0) & (d50 > 0) & (d75 > 0) & ~((d75 - d25) > max_spread * d50)
    return torch.where(keep, d50, torch.zeros_like(d50))


def fusion_depth(local_tensorfs, poses, W, H, max_spread=None, **render):
    """The depth [N,H,W] scene_point_cloud and scene_mesh fuse with depth="median": median_depth, or with max_spread the
    median of q = (0.25, 0.5, 0.75) with the pixels zeroed whose interquartile range exceeds max_spread * median or that
    miss one of the three."""
    if max_spread is None:
        return median_depth(local_tensorfs, poses, W, H, **render)
    d = render_depth_quantiles(local_tensorfs, poses, W, H, (0.25, 0.5, 0.75), **render)["depth"]
    return spread_filter(d[0], d[1], d[2], max_spread)
