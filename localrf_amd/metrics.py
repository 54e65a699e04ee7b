"""Test-view image metrics on the GPU: the evaluation half of renderer.render(test=True) (renderer.py:155-167).

  rgb_ssim(img0, img1, max_val, ...)  utils/utils.py:232-287 with the reference's signature.  numpy [H,W,3] in: numpy out
                                      (numpy.float64, or the fp64 map), so `renderer.rgb_ssim = metrics.rgb_ssim` is a
                                      drop-in; device tensors [H,W,3] / [B,H,W,3] in: fp64 device tensors out, no sync
  image_metrics(rgb, gt, ...)         (mse [B], ssim [B]) fp64 device tensors for B frame pairs, one launch pair
  psnr(mses)                          train.py:567: -10 log10(mean(mses))
  test_view_metrics(lt, gt_rgbs, ...) renders each test view through LocalTensorfs.forward (renderer.py:65-77) and returns
                                      {fbase: {"mse", "ssim"}} as renderer.render does, with one host sync at the end

The arithmetic is the HIP kernel pair of csrc/lrf_metrics.inl (lrf_image_metrics), in fp64 as the reference's numpy /
scipy SSIM; images are read as fp32 (what the renderer's arrays are).  The MSE is summed in fp64 (the reference's is an
fp32 torch mean: the two agree to ~1e-7 relative).  No torch fallback: CPU tensors raise NativeError.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._native import NativeError

MAX_FILTER_SIZE = 31


def check_shapes(shape0, shape1, filter_size):
    """The filter size as an int, for two image shapes that go together; ValueError otherwise.  No launch."""
    if tuple(shape0) != tuple(shape1):
        raise ValueError(f"image shapes differ: {tuple(shape0)} vs {tuple(shape1)}")
    if len(shape0) not in (3, 4) or shape0[-1] != 3:
        raise ValueError(f"images must be [H,W,3] or [B,H,W,3], got {tuple(shape0)}")
    fs = int(filter_size)
    if fs != filter_size or not 1 <= fs <= MAX_FILTER_SIZE:
        raise ValueError(f"filter_size must be an integer in 1..{MAX_FILTER_SIZE}, got {filter_size}")
    H, W = int(shape0[-3]), int(shape0[-2])
    if H < fs or W < fs:
        raise ValueError(f"image {H}x{W} is smaller than filter_size {fs}: the valid SSIM map would be empty")
    return fs


def _images(t, name):
    N.require_gpu(t, name, "the metrics")
    return N.conform(t)


def _launch(img0, img1, max_val, fs, filter_sigma, k1, k2, want_map):
    """img0 / img1: contiguous fp32 [B,H,W,3] on one device.  Returns (mse [B], ssim [B], map or None), fp64."""
    B, H, W, _ = img0.shape
    dev = img0.device
    if img1.device != dev:
        raise ValueError(f"images on different devices: {img0.device} vs {img1.device}")
    a = N.LrfImageMetrics()
    a.img0, a.img1 = img0.data_ptr(), img1.data_ptr()
    a.B, a.H, a.W, a.filter_size = B, H, W, fs
    a.max_val, a.filter_sigma, a.k1, a.k2 = float(max_val), float(filter_sigma), float(k1), float(k2)
    ws = N.workspace("lrf_image_metrics", dev, B, H, W, fs)
    out = torch.empty(2, B, dtype=torch.float64, device=dev)
    smap = torch.empty(B, H - fs + 1, W - fs + 1, 3, dtype=torch.float64, device=dev) if want_map else None
    N.launch("lrf_image_metrics", dev, C.byref(a), None if smap is None else smap.data_ptr(), out[1].data_ptr(), out[0].data_ptr(),
             ws.data_ptr(), guard=True)
    return out[0], out[1], smap


def image_metrics(rgb, gt, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """Per-frame (mse [B], ssim [B]) of device images [B,H,W,3] (or [H,W,3]: B = 1) as fp64 device tensors, without a
    host sync.  ssim is rgb_ssim(gt[b], rgb[b], max_val, ...) (symmetric in its two images); mse is ((gt - rgb) ** 2).mean()."""
    fs = check_shapes(rgb.shape, gt.shape, filter_size)
    rgb, gt = _images(rgb, "rgb"), _images(gt, "gt")
    if rgb.dim() == 3:
        rgb, gt = rgb[None], gt[None]
    mse, ssim, _ = _launch(gt, rgb, max_val, fs, filter_sigma, k1, k2, False)
    return mse, ssim


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """utils/utils.py:rgb_ssim on the GPU.  numpy [H,W,3] inputs: the reference's return values (numpy.float64, or the fp64
    map [H-fs+1, W-fs+1, 3]).  Device tensors [H,W,3] or [B,H,W,3]: fp64 device tensors (a 0-d / [B] mean, or the
    map), no host sync."""
    host = not torch.is_tensor(img0) and not torch.is_tensor(img1)
    if host:
        img0, img1 = np.asarray(img0), np.asarray(img1)
        if img0.ndim != 3:
            raise ValueError(f"numpy images must be [H,W,3], got {img0.shape}")
    fs = check_shapes(img0.shape, img1.shape, filter_size)
    if host:
        if not torch.cuda.is_available():
            raise NativeError("localrf_amd.metrics.rgb_ssim: no AMD GPU visible; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        img0 = torch.from_numpy(np.ascontiguousarray(img0, dtype=np.float32)).to(dev)
        img1 = torch.from_numpy(np.ascontiguousarray(img1, dtype=np.float32)).to(dev)
    else:
        img0, img1 = _images(img0, "img0"), _images(img1, "img1")
    single = img0.dim() == 3
    if single:
        img0, img1 = img0[None], img1[None]
    _, ssim, smap = _launch(img0, img1, max_val, fs, filter_sigma, k1, k2, return_map)
    res = smap if return_map else ssim
    if single:
        res = res[0]
    if host:
        return res.cpu().numpy() if return_map else np.float64(res.item())
    return res


def psnr(mses):
    """train.py:567 (test/PSNR): -10 log10 of the mean of the per-view MSEs."""
    if torch.is_tensor(mses):
        mses = mses.detach().double().cpu().reshape(-1).tolist()
    m = np.asarray([float(v) for v in mses], dtype=np.float64)
    return float(-10.0 * np.log(m.mean()) / np.log(10.0))


def test_view_metrics(local_tensorfs, gt_rgbs, view_ids, W, H, fbases=None, chunk=4096, floater_thresh=0,
                      max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """The metrics of renderer.render(test=True) (renderer.py:55-167): every view of `view_ids` rendered at W x H through
    local_tensorfs.forward (test_id=True, cam2world=None, no tape), then MSE and SSIM against gt_rgbs [n,H,W,3] (device,
    already at W x H: resizing the dataset images stays the caller's job) on the device.  One host sync, at the end.
    Returns {fbase: {"mse": float, "ssim": float}}; fbases default to the view ids."""
    view_ids = [int(v) for v in (view_ids.tolist() if hasattr(view_ids, "tolist") else view_ids)]
    n = len(view_ids)
    fbases = list(view_ids) if fbases is None else list(fbases)
    if len(fbases) != n:
        raise ValueError(f"{len(fbases)} fbases for {n} views")
    if tuple(gt_rgbs.shape) != (n, H, W, 3):
        raise ValueError(f"gt_rgbs must be [{n},{H},{W},3], got {tuple(gt_rgbs.shape)}")
    fs = check_shapes(gt_rgbs.shape[1:], (H, W, 3), filter_size)
    gt = _images(gt_rgbs, "gt_rgbs")
    if n == 0:
        return {}
    dev = gt.device
    ray_ids = torch.arange(W * H, dtype=torch.int64, device=dev)
    out = torch.empty(2, n, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for i, v in enumerate(view_ids):
            rgb = local_tensorfs(ray_ids, [v], W, H, is_train=False, cam2world=None, test_id=True, chunk=chunk,
                                 floater_thresh=floater_thresh)[0]
            if not rgb.is_cuda:                         # a view no field covers: LocalTensorfs.forward's host placeholder
                rgb = rgb.to(dev)
            rgb = _images(rgb, "rendered rgb").reshape(1, H, W, 3)
            mse, ssim, _ = _launch(gt[i:i + 1], rgb, max_val, fs, filter_sigma, k1, k2, False)
            out[0, i:i + 1].copy_(mse)
            out[1, i:i + 1].copy_(ssim)
    host = out.cpu()
    return {fb: {"mse": float(host[0, i]), "ssim": float(host[1, i])} for i, fb in enumerate(fbases)}
