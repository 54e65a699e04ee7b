"""Test-view geometry diagnostics on the GPU: the flow and depth comparison images renderer.render(test=True) builds per
test view (renderer.py:79-124), and the exact device order statistics they rest on.

  quantile(x, q)               np.quantile(row, q) (method="linear") of every row of x [..., n], bit for bit
  median(x)                    torch.median(row) (the lower median) of every row
  flow_comparison(...)         (fwd_flow_cmp [3H, 2W], bwd_flow_cmp [3H, 2W]) of renderer.py:79-115
  depth_comparison(...)        depth_cmp [3H, W] of renderer.py:117-124
  test_view_evaluation(...)    renders each test view once and returns its metrics (metrics.test_view_metrics) and the
                               three comparison images, with one host sync at the end

The arithmetic is HIP (csrc/lrf_select.inl, csrc/lrf_evalgeo.inl, reached through lrf_select, lrf_flow_comparison and
lrf_depth_comparison).  Nothing synchronises with the host; CPU tensors raise NativeError, there is no torch fallback.
The depth comparison's mean absolute deviations are summed in fp64 and rounded once to fp32, where the reference takes an
fp32 torch mean: the images agree with the reference's to ~1e-6.  Every other value follows the reference's fp32 operations.
"""
import ctypes as C
import math

import torch

from . import _native as N
from ._native import NativeError
from .metrics import check_shapes, image_metrics

MAX_VIEWS = N.LRF_EVAL_MAX_VIEWS          # views per lrf_flow_comparison call; more are split into several calls
_MAX_ROWS = 65535


def _dev(t, name, dtype=torch.float32):
    N.require_gpu(t, name, "the diagnostics")
    return N.conform(t, dtype)


def _select(rows, lengths, mode, q):
    """rows: contiguous fp32 [B, stride] on the device; lengths: one shared length or B of them.  Returns fp32 [B]."""
    B, stride = rows.shape
    dev = rows.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    for b0 in range(0, B, _MAX_ROWS if len(lengths) == 1 else N.LRF_SELECT_MAX_ROWS):
        b1 = min(B, b0 + (_MAX_ROWS if len(lengths) == 1 else N.LRF_SELECT_MAX_ROWS))
        ln = lengths if len(lengths) == 1 else lengths[b0:b1]
        ws = N.workspace("lrf_select", dev, b1 - b0, max(ln))
        arr = (C.c_int64 * len(ln))(*ln)
        N.launch("lrf_select", dev, rows[b0].data_ptr(), stride, arr, len(ln), b1 - b0, mode, float(q), out[b0:b1].data_ptr(),
                 ws.data_ptr(), guard=True)
    return out


def _order_stat(x, mode, q):
    if isinstance(x, (list, tuple)):                        # ragged rows: 1-D device tensors of their own lengths
        if len(x) == 0:
            raise ValueError("no rows")
        rows = [_dev(t, "x").reshape(-1) for t in x]
        lengths = [int(t.numel()) for t in rows]
        if min(lengths) < 1:
            raise NativeError("lrf_select: a row is empty (n = 0)")
        if len(set(lengths)) == 1:
            return _order_stat(torch.stack(rows), mode, q)
        packed = torch.zeros(len(rows), max(lengths), dtype=torch.float32, device=rows[0].device)
        for i, t in enumerate(rows):
            packed[i, :lengths[i]].copy_(t)
        return _select(packed, lengths, mode, q)
    x = _dev(x, "x")
    if x.dim() == 0:
        x = x.reshape(1)
    n = int(x.shape[-1])
    if n < 1:
        raise NativeError("lrf_select: the rows are empty (n = 0)")
    if n >= 2 ** 31:
        raise NativeError(f"lrf_select: rows of {n} values (n must stay below 2^31)")
    lead = x.shape[:-1]
    rows = x.reshape(-1, n)
    if rows.shape[0] == 0:
        return torch.empty(lead, dtype=torch.float32, device=x.device)
    return _select(rows, [n], mode, q).reshape(lead)


def quantile(x, q):
    """np.quantile(row, q) (method="linear", as numpy computes it for float32: bit for bit) of every row of the device tensor
    x [..., n] (fp32; other dtypes are converted), over the last dimension, as an fp32 tensor of shape x.shape[:-1].  x may also
    be a list of 1-D device tensors of different lengths (one result each).  A row holding a NaN gives NaN; -0.0 and +0.0
    compare equal (a zero result is +0.0).  No host sync."""
    qf = float(q)
    if not 0.0 <= qf <= 1.0:
        raise ValueError(f"q must lie in [0, 1], got {q}")
    return _order_stat(x, N.LRF_SELECT_QUANTILE, qf)


def median(x):
    """torch.median(row) (the lower median, rank floor((n - 1) / 2)) of every row of x [..., n] or of a list of 1-D rows, as
    quantile() takes them.  NaN rows give NaN.  No host sync."""
    return _order_stat(x, N.LRF_SELECT_MEDIAN, 0.0)


def _views(t, V, shape, name, dtype=torch.float32):
    t = _dev(t, name, dtype)
    if t.numel() != V * math.prod(shape):
        raise ValueError(f"{name} must hold {V} x {list(shape)} values, got {tuple(t.shape)}")
    return t.reshape(V, *shape)


def _flow_batch(depth, dirs, ij, cam2world, idx, focal, center, fwd_flow, fwd_mask, bwd_flow, bwd_mask, W, H, raw):
    """Views stacked on a leading axis: depth [V,HW], dirs [V,HW,3], ij [V,HW,2], flows [V,H,W,2], masks [V,H,W]; idx: V ints."""
    V, HW = len(idx), W * H
    c2w = _dev(cam2world, "cam2world")
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (3, 4):
        raise ValueError(f"cam2world must be [F,3,4], got {tuple(c2w.shape)}")
    F = int(c2w.shape[0])
    for i in idx:
        if not 0 <= i < F:
            raise NativeError(f"lrf_flow_comparison: view index {i} lies outside [0, {F})")
    depth = _views(depth, V, (HW,), "depth_map")
    dirs = _views(dirs, V, (HW, 3), "directions")
    ij = _views(ij, V, (HW, 2), "ij", torch.int64)
    ins = [_views(t, V, s, n) for t, s, n in ((fwd_flow, (HW, 2), "fwd_flow"), (fwd_mask, (HW,), "fwd_mask"),
                                              (bwd_flow, (HW, 2), "bwd_flow"), (bwd_mask, (HW,), "bwd_mask"))]
    focal = _dev(torch.as_tensor(focal, device=depth.device), "focal").reshape(-1)
    center = _dev(torch.as_tensor(center, device=depth.device), "center").reshape(-1)
    dev = depth.device
    out = torch.empty(2, V, 3 * H, 2 * W, dtype=torch.float32, device=dev)
    rawt = torch.empty_like(out) if raw else None
    quant = torch.empty(V, 4, dtype=torch.float32, device=dev)
    for v0 in range(0, V, MAX_VIEWS):
        v1 = min(V, v0 + MAX_VIEWS)
        a = N.LrfFlowComparison()
        a.cam2world, a.depth, a.dirs, a.ij = c2w.data_ptr(), depth[v0].data_ptr(), dirs[v0].data_ptr(), ij[v0].data_ptr()
        a.fwd_flow, a.fwd_mask, a.bwd_flow, a.bwd_mask = [t[v0].data_ptr() for t in ins]
        a.focal, a.center = focal.data_ptr(), center.data_ptr()
        a.F, a.V, a.H, a.W = F, v1 - v0, H, W
        for k, i in enumerate(idx[v0:v1]):
            a.idx[k] = i
        ws = N.workspace("lrf_flow_comparison", dev, v1 - v0, H, W)
        N.launch("lrf_flow_comparison", dev, C.byref(a), out[0, v0].data_ptr(), out[1, v0].data_ptr(),
                 None if rawt is None else rawt[0, v0].data_ptr(), None if rawt is None else rawt[1, v0].data_ptr(),
                 quant[v0].data_ptr(), ws.data_ptr(), guard=True)
    return out, rawt, quant


def _frame(W, H):
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError(f"need W, H > 0, got {W} x {H}")
    return W, H


def flow_comparison(depth_map, directions, ij, cam2world, idx, focal, center, fwd_flow, fwd_mask, bwd_flow, bwd_mask, W, H,
                    return_raw=False):
    """renderer.py:79-115 for the view of absolute frame index idx: (fwd_flow_cmp, bwd_flow_cmp), each [3H, 2W] fp32 on the
    device, already clamped to [0, 1] (what the reference appends to fwd_flow_cmp_tb / bwd_flow_cmp_tb).
    depth_map [HW], directions [HW,3], ij [HW,2] as LocalTensorfs.forward returns them; cam2world [F,3,4]
    (local_tensorfs.get_cam2world()); focal = local_tensorfs.focal(W), center = local_tensorfs.center(W, H); flows [H,W,2] and
    masks [H,W] of the test dataset, already at W x H.  idx may also be a list of V indices with every per-view input stacked
    on a leading axis: the images are then [V, 3H, 2W].
    return_raw=True also returns the two images before the division and the clamp, and the four quantiles [4] ([V, 4]):
    forward x, forward y, backward x, backward y."""
    W, H = _frame(W, H)
    single = not isinstance(idx, (list, tuple))
    ids = [int(idx)] if single else [int(i) for i in idx]
    if len(ids) == 0:
        raise ValueError("no views")
    out, raw, quant = _flow_batch(depth_map, directions, ij, cam2world, ids, focal, center, fwd_flow, fwd_mask, bwd_flow,
                                  bwd_mask, W, H, return_raw)
    res = (out[0], out[1]) if not single else (out[0, 0], out[1, 0])
    if return_raw:
        res = res + ((raw[0], raw[1], quant) if not single else (raw[0, 0], raw[1, 0], quant[0]))
    return res


def depth_comparison(depth_map, invdepth, W, H, return_stats=False):
    """renderer.py:117-124: vstack([0.5 x^, 0.5 y^, (x^ - y^)^2]).clamp(0, 1) of compute_depth_loss(1 / depth.clamp(1e-6),
    invdepth), [3H, W] fp32 on the device.  depth_map [HW] (or [V, HW]), invdepth [H, W] (or [V, H, W]), already at W x H.
    return_stats=True also returns (median x, median y, mad x, mad y) [4] ([V, 4])."""
    W, H = _frame(W, H)
    d = _dev(depth_map, "depth_map")
    single = d.numel() == W * H
    V = 1 if single else d.numel() // (W * H)
    d = _views(d, V, (W * H,), "depth_map")
    inv = _views(invdepth, V, (W * H,), "invdepth")
    dev = d.device
    ws = N.workspace("lrf_depth_comparison", dev, V, H, W)
    out = torch.empty(V, 3 * H, W, dtype=torch.float32, device=dev)
    stats = torch.empty(V, 4, dtype=torch.float32, device=dev)
    N.launch("lrf_depth_comparison", dev, d.data_ptr(), inv.data_ptr(), V, H, W, out.data_ptr(), stats.data_ptr(), ws.data_ptr(),
             guard=True)
    if single:
        out, stats = out[0], stats[0]
    return (out, stats) if return_stats else out


def test_view_evaluation(local_tensorfs, view_ids, W, H, gt_rgbs=None, fwd_flow=None, fwd_mask=None, bwd_flow=None, bwd_mask=None,
                         invdepths=None, fbases=None, chunk=4096, floater_thresh=0, max_val=1.0, filter_size=11, filter_sigma=1.5,
                         k1=0.01, k2=0.03):
    """The test half of renderer.render(test=True) (renderer.py:55-167) on the device: every view of view_ids rendered once at
    W x H through local_tensorfs.forward (test_id=True, cam2world=None), then
      metrics      {fbase: {"mse", "ssim"}} against gt_rgbs [n,H,W,3] as metrics.test_view_metrics computes them ({} without gt_rgbs)
      fwd_flow_cmp / bwd_flow_cmp  lists of [3H, 2W] device images (renderer.py:79-115; poses from local_tensorfs.get_cam2world())
      depth_cmp    list of [3H, W] device images (renderer.py:117-124)
    The dataset inputs fwd_flow / bwd_flow [n,H,W,2], fwd_mask / bwd_mask [n,H,W], invdepths [n,H,W] are device tensors already
    at W x H (resizing stays the caller's job).  A group whose inputs are None is skipped (empty list), as the reference skips
    it when all_fwd_flow / all_invdepths is None.  One host sync, at the end (for the metrics)."""
    view_ids = [int(v) for v in (view_ids.tolist() if hasattr(view_ids, "tolist") else view_ids)]
    n = len(view_ids)
    W, H = _frame(W, H)
    fbases = list(view_ids) if fbases is None else list(fbases)
    if len(fbases) != n:
        raise ValueError(f"{len(fbases)} fbases for {n} views")
    flow_in = (fwd_flow, fwd_mask, bwd_flow, bwd_mask)
    do_flow = all(t is not None for t in flow_in)
    if not do_flow and any(t is not None for t in flow_in):
        raise ValueError("fwd_flow, fwd_mask, bwd_flow and bwd_mask go together")
    res = {"metrics": {}, "fwd_flow_cmp": [], "bwd_flow_cmp": [], "depth_cmp": []}
    if gt_rgbs is not None:
        if tuple(gt_rgbs.shape) != (n, H, W, 3):
            raise ValueError(f"gt_rgbs must be [{n},{H},{W},3], got {tuple(gt_rgbs.shape)}")
        check_shapes(gt_rgbs.shape[1:], (H, W, 3), filter_size)
        gt = _dev(gt_rgbs, "gt_rgbs")
    if do_flow:
        flow_in = [_views(t, n, s, nm) for t, s, nm in zip(flow_in, ((H * W, 2), (H * W,), (H * W, 2), (H * W,)),
                                                            ("fwd_flow", "fwd_mask", "bwd_flow", "bwd_mask"))]
    if invdepths is not None:
        invdepths = _views(invdepths, n, (H * W,), "invdepths")
    if n == 0:
        return res
    dev = torch.device(local_tensorfs.device)
    if dev.type != "cuda":
        raise NativeError(f"localrf_amd.diagnostics: the scene lives on {dev}; the diagnostics run only on an AMD GPU")
    ray_ids = torch.arange(W * H, dtype=torch.int64, device=dev)
    need_geo = do_flow or invdepths is not None
    if need_geo:
        depths = torch.empty(n, H * W, dtype=torch.float32, device=dev)
        dirs = torch.empty(n, H * W, 3, dtype=torch.float32, device=dev)
        ijs = torch.empty(n, H * W, 2, dtype=torch.int64, device=dev)
    scores = torch.empty(2, n, dtype=torch.float64, device=dev) if gt_rgbs is not None else None
    with torch.no_grad():
        for i, v in enumerate(view_ids):
            rgb, depth, d, ij = local_tensorfs(ray_ids, [v], W, H, is_train=False, cam2world=None, test_id=True, chunk=chunk,
                                               floater_thresh=floater_thresh)
            if scores is not None:
                mse, ssim = image_metrics(rgb.to(dev).reshape(1, H, W, 3), gt[i:i + 1], max_val, filter_size, filter_sigma, k1, k2)
                scores[0, i:i + 1].copy_(mse)
                scores[1, i:i + 1].copy_(ssim)
            if need_geo:
                depths[i].copy_(depth.reshape(-1))
                dirs[i].copy_(d.reshape(-1, 3))
                ijs[i].copy_(ij.reshape(-1, 2))
        if do_flow:
            cam2world = local_tensorfs.get_cam2world().detach()
            out, _, _ = _flow_batch(depths, dirs, ijs, cam2world, view_ids, local_tensorfs.focal(W), local_tensorfs.center(W, H),
                                    *flow_in, W, H, False)
            res["fwd_flow_cmp"], res["bwd_flow_cmp"] = list(out[0].unbind(0)), list(out[1].unbind(0))
        if invdepths is not None:
            cmp = depth_comparison(depths, invdepths, W, H) if n > 1 else depth_comparison(depths[0], invdepths[0], W, H)[None]
            res["depth_cmp"] = list(cmp.unbind(0))
    if scores is not None:
        host = scores.cpu()
        res["metrics"] = {fb: {"mse": float(host[0, i]), "ssim": float(host[1, i])} for i, fb in enumerate(fbases)}
    else:
        N.torch_stream(dev).synchronize()
    return res
