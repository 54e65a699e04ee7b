"""Novel camera poses rendered on the GPU, with the frames encoded on the device: the test=False branch of
renderer.render (renderer.py:43-77,130-148,172-174) that train.py:render_frames runs over the smoothed camera path and
--render_from_file over the poses of a transforms.json.

  nearest_frames(local_tensorfs, poses)     the training frame each pose borrows its blending weights from (renderer.py:47-53)
  visualize_depth(depth, minmax, cmap)      utils/utils.py:179-197 on the device: the colour-mapped depth as uint8 HWC bytes
  encode_frames(rgb, depth, ...)            the bytes of the frame files: rgb8 (cv2.imwrite(255 * rgb)) and depth8
  render_poses(local_tensorfs, poses, ...)  every pose rendered and encoded, device tensors out
  iter_pose_frames(...)                     the same frames as host numpy arrays, in order, for a video or image writer

The per-pixel encoding is HIP (csrc/lrf_encode.inl through lrf_encode_frames); the renders are lrf_scene_fwd, several
poses per call.  Every function checks its arguments before its first launch.  CPU tensors raise NativeError: there is no
torch fallback.  Cited lines are relative to the reference's localTensoRF directory.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .pose_plan import PosePlan, nearest_frames  # noqa: F401  (nearest_frames: part of this module's interface)

_ENC_MAX_PX = ((1 << 31) - 1) // 3           # lrf_encode_frames: 3 V H W < 2^31


def jet_lut():
    """[256, 3] uint8, BGR: the classic piecewise-linear jet (r = clip(1.5 - |4t - 3|), g = clip(1.5 - |4t - 2|),
    b = clip(1.5 - |4t - 1|), t = k / 255), rounded to bytes.  Its equality with OpenCV's COLORMAP_JET is not verified
    (OpenCV is not a dependency).  For the reference's exact bytes pass
    cv2.applyColorMap(np.arange(256, dtype=np.uint8)[:, None], cv2.COLORMAP_JET)[:, 0] as cmap."""
    t = np.arange(256, dtype=np.float64) / 255.0
    rgb = [np.clip(1.5 - np.abs(4.0 * t - c), 0.0, 1.0) for c in (3.0, 2.0, 1.0)]
    return np.rint(255.0 * np.stack(rgb[::-1], -1)).astype(np.uint8)


_lut_cache = {}


def _check_lut(cmap):
    """None, or a [256, 3] uint8 ndarray / tensor; raises on the host otherwise."""
    if cmap is None:
        return
    if isinstance(cmap, np.ndarray):
        ok = cmap.dtype == np.uint8 and cmap.shape == (256, 3)
    else:
        ok = torch.is_tensor(cmap) and cmap.dtype is torch.uint8 and tuple(cmap.shape) == (256, 3)
    if not ok:
        raise ValueError(f"cmap must be a [256, 3] uint8 table, got {getattr(cmap, 'dtype', type(cmap))} "
                         f"{tuple(getattr(cmap, 'shape', ()))}")


def _lut(cmap, dev):
    """The checked cmap (None: jet_lut()) as a contiguous device tensor."""
    if cmap is None:
        key = str(dev)
        if key not in _lut_cache:
            _lut_cache[key] = torch.from_numpy(jet_lut()).to(dev)
        return _lut_cache[key]
    if isinstance(cmap, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(cmap)).to(dev)
    return cmap.to(dev).contiguous()


def fixed_range(minmax):
    """(mi, ma) -> fp32 (mi, ma, D) as visualize_depth's `(x - mi) / (ma - mi + 1e-8)` rounds them in numpy 2.2: Python
    numbers are subtracted in fp64 and the divisor rounded once to fp32 (D = 5.0 for the renderer's [0, 5]); np.float32
    values (a range visualize_depth returned) are subtracted and offset in fp32.  Other numpy scalars count as Python floats."""
    if len(minmax) != 2:
        raise ValueError(f"minmax must be (mi, ma), got {minmax!r}")
    mi, ma = minmax
    if isinstance(mi, np.float32) and isinstance(ma, np.float32):
        D = np.float32(np.float32(ma - mi) + np.float32(1e-8))
    else:
        mi, ma = float(mi), float(ma)
        D = np.float32(ma - mi + 1e-8)
    return np.float32(mi), np.float32(ma), D


def _aligned(t):
    """Contiguous fp32; copied when the data does not start on 16 bytes (the kernel reads float4)."""
    t = N.conform(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _encode(rgb, depth, minmax, lut, want_idx, want_range):
    """rgb [V,H,W,3] or None, depth [V,H,W] on the device (already checked) -> (rgb8, depth8, idx, range [V,2])."""
    V, H, W = (int(s) for s in depth.shape)
    dev = depth.device
    fr = None if minmax is None else (C.c_float * 3)(*(float(v) for v in fixed_range(minmax)))
    rgb8 = None if rgb is None else torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    depth8 = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    idx = torch.empty(V, H, W, dtype=torch.uint8, device=dev) if want_idx else None
    rng = torch.empty(V, 2, dtype=torch.float32, device=dev) if want_range else None
    step = _ENC_MAX_PX // (H * W)
    step = V if step >= V else max(1, step // 4 * 4)          # split calls start on 16-byte boundaries
    ws = N.workspace("lrf_encode_frames", dev, min(V, step)) if minmax is None else None
    for v0 in range(0, V, step):
        v1 = min(V, v0 + step)
        p = lambda t: None if t is None else t[v0].data_ptr()  # noqa: E731
        N.launch("lrf_encode_frames", dev, p(rgb), depth[v0].data_ptr(), v1 - v0, H, W, lut.data_ptr(), fr, p(rgb8),
                 depth8[v0].data_ptr(), p(idx), p(rng), None if ws is None else ws.data_ptr(), guard=True)
    return rgb8, depth8, idx, rng


def _device_frames(t, name, trailing):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_floating_point():
        raise ValueError(f"{name} must hold floating-point values, got {t.dtype}")
    nd = 2 + len(trailing)
    if t.dim() < nd or tuple(t.shape[t.dim() - len(trailing):]) != tuple(trailing) or min(t.shape[:t.dim() - len(trailing)], default=1) < 1:
        raise ValueError(f"{name} must be [..., H, W{', 3' if trailing else ''}] with H, W > 0, got {tuple(t.shape)}")
    return t


def visualize_depth(depth, minmax=None, cmap=None, return_index=False):
    """utils/utils.py:179-197 on the device: depth [..., H, W] -> (uint8 [..., H, W, 3], [mi, ma]).  The bytes are what
    renderer.py:148 makes of the reference's result, (ToTensor(img) * 255).byte() permuted to HWC, i.e. the colour map's
    entries in its own (BGR) channel order.  cmap: a [256, 3] uint8 table (None: jet_lut(), see there).
    minmax=None takes each frame's range, mi = min(x[x > 0]), ma = max(x) of x = nan_to_num(depth), read back once; a frame
    without a positive depth raises ValueError (numpy's min of an empty array).  With several frames [mi, ma] becomes a
    list of one pair per frame.  return_index=True also returns the uint8 index image [..., H, W] given to the colour map."""
    d = _device_frames(depth, "depth", ())
    if minmax is not None:
        fixed_range(minmax)
    _check_lut(cmap)
    N.require_gpu(d, "depth", "the encoding")
    lut = _lut(cmap, d.device)
    lead, (H, W) = d.shape[:-2], d.shape[-2:]
    frames = _aligned(d.reshape(-1, H, W))
    _, img, idx, rng = _encode(None, frames, minmax, lut, return_index, minmax is None)
    if minmax is None:
        host = rng.cpu().numpy()
        empty = np.flatnonzero(np.isnan(host[:, 0]))
        if empty.size:
            raise ValueError(f"visualize_depth: frame {int(empty[0])} has no positive depth (min of an empty array)")
        ranges = [[np.float32(a), np.float32(b)] for a, b in host]
        out_range = ranges[0] if len(lead) == 0 else ranges
    else:
        out_range = list(minmax)
    img = img.reshape(*lead, H, W, 3)
    return (img, out_range, idx.reshape(*lead, H, W)) if return_index else (img, out_range)


def encode_frames(rgb, depth, minmax=(0, 5), cmap=None, return_index=False):
    """rgb [..., H, W, 3], depth [..., H, W] (device) -> (rgb8 [..., H, W, 3], depth8 [..., H, W, 3][, depth_idx [..., H, W]]),
    uint8 on the device, in one launch (two with minmax=None):
      rgb8   = clamp(rint(fp32(255 * rgb)), 0, 255), ties to even, NaN -> 0: the pixels cv2.imwrite(255 * rgb[..., ::-1])
               stores (renderer.py:173), in RGB order.  (cv2's cvRound sends values beyond the int32 range to 0; a
               rendered rgb lies in [0, 1].)
      depth8 = visualize_depth(depth, minmax, cmap) bytes; depth_idx its index image.
    minmax (0, 5) is renderer.py:130's [0, 5]; None is the per-frame automatic range (not read back here)."""
    r = _device_frames(rgb, "rgb", (3,))
    d = _device_frames(depth, "depth", ())
    if tuple(r.shape[:-1]) != tuple(d.shape):
        raise ValueError(f"rgb {tuple(r.shape)} and depth {tuple(d.shape)} must hold the same frames")
    if r.device != d.device:
        raise ValueError("rgb and depth must live on the same device")
    if minmax is not None:
        fixed_range(minmax)
    _check_lut(cmap)
    N.require_gpu(d, "depth", "the encoding")
    lut = _lut(cmap, d.device)
    lead, (H, W) = d.shape[:-2], d.shape[-2:]
    rgb8, depth8, idx, _ = _encode(_aligned(r.reshape(-1, H, W, 3)), _aligned(d.reshape(-1, H, W)), minmax, lut,
                                   return_index, False)
    out = (rgb8.reshape(*lead, H, W, 3), depth8.reshape(*lead, H, W, 3))
    return out + (idx.reshape(*lead, H, W),) if return_index else out


def _check_encoding(depth_minmax, cmap):
    if depth_minmax is not None:
        fixed_range(depth_minmax)
    _check_lut(cmap)


def render_poses(local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, floater_thresh=0, chunk=4096,
                 frames_per_call=None, depth_minmax=(0, 5), cmap=None, encode=True):
    """The test=False branch of renderer.render (renderer.py:43-77,130-148) on the device.  Frame i is rendered at its pose
    through the blending weights of its nearest training frame (nearest_frames, or frame_indices), with that frame's
    exposure, or -- when the nearest frame is in test_frames (the frame indices whose fbase the test split holds,
    renderer.py:47) -- the mean of its neighbours' (renderer.py:74, test_id).  The choice is made per frame.
    start reproduces the reference as it is: poses = poses[start:], the frames are range(start, len(poses)) of that shorter
    list, i.e. N - 2 start of them, and frame i uses pose poses[start + i] with frame_indices[start + i] -- which, when
    frame_indices is None, is the nearest frame of poses[2 start + i].
    Consecutive frames with the same active fields are rendered together, up to frames_per_call (None: no bound) per
    lrf_scene_fwd call and as many as the scene's max_untaped_workspace allows for the call's ray buffers; frames with
    different active sets are never merged.  The result does not depend on the grouping: it equals per-frame
    LocalTensorfs.forward(ray_ids, [nearest], W, H, is_train=False, cam2world=pose[None], test_id=..., floater_thresh=...)
    calls bit for bit.  chunk is the reference's args.batch_size (renderer.py:75).
    Returns a dict of device tensors: rgb [N,H,W,3] (rgb_maps_tb), depth [N,H,W] (the raw depth save_raw_depth writes),
    frame_indices [N] (int64), and with encode rgb8 / depth8 [N,H,W,3] uint8 (encode_frames with depth_minmax and cmap).
    Raises ValueError before any launch for a frame whose nearest frame has no active field."""
    if encode:
        _check_encoding(depth_minmax, cmap)
    plan = PosePlan(local_tensorfs, poses, W, H, test_frames, frame_indices, start, frames_per_call, chunk).on_device(exposure=True)
    n, W, H, dev = plan.n, plan.W, plan.H, plan.dev
    lut = _lut(cmap, dev) if encode else None
    rgb = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for i0, i1, active in plan.calls:
            r, d = plan.render_colour(i0, i1, active, floater_thresh)
            rgb[i0:i1].view(-1, 3).copy_(r)
            depth[i0:i1].view(-1).copy_(d)
    out = {"rgb": rgb, "depth": depth, "frame_indices": plan.vids}
    if encode and n:
        out["rgb8"], out["depth8"], _, _ = _encode(rgb, depth, depth_minmax, lut, False, False)
    elif encode:
        out["rgb8"] = torch.empty(0, H, W, 3, dtype=torch.uint8, device=dev)
        out["depth8"] = torch.empty(0, H, W, 3, dtype=torch.uint8, device=dev)
    return out


def iter_pose_frames(local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, floater_thresh=0, chunk=4096,
                     frames_per_call=None, depth_minmax=(0, 5), cmap=None, with_depth=False):
    """render_poses' frames on the host, in order: yields (i, rgb8 [H,W,3], depth8 [H,W,3]) uint8 numpy arrays, plus the raw
    depth [H,W] fp32 with with_depth=True -- what a video or image writer takes.  Each yielded array is the caller's own.
    A group of frames is rendered and encoded on the current stream; an event after it lets a side stream copy its bytes
    into one of two pinned host buffers without blocking, while the next group renders.  The host waits only on the copy
    event of the group whose frames it yields.  Closing the generator early synchronises both streams: nothing stays
    enqueued."""
    _check_encoding(depth_minmax, cmap)
    plan = PosePlan(local_tensorfs, poses, W, H, test_frames, frame_indices, start, frames_per_call, chunk).on_device(exposure=True)
    return _iter_frames(plan, _lut(cmap, plan.dev), floater_thresh, depth_minmax, with_depth)


def _iter_frames(plan, lut, floater_thresh, depth_minmax, with_depth):
    groups, W, H, dev = plan.calls, plan.W, plan.H, plan.dev
    if not groups:
        return
    vmax = max(i1 - i0 for i0, i1, _ in groups)
    names = ("rgb8", "depth8", "depth") if with_depth else ("rgb8", "depth8")
    shapes = {"rgb8": ((vmax, H, W, 3), torch.uint8), "depth8": ((vmax, H, W, 3), torch.uint8), "depth": ((vmax, H, W), torch.float32)}
    ring = [{k: torch.empty(*shapes[k][0], dtype=shapes[k][1], pin_memory=True) for k in names} for _ in range(2)]
    main = N.torch_stream(dev)
    side = torch.cuda.Stream(dev)
    pending = [None, None]                                      # per slot: (group, copy event, device tensors kept alive)

    def launch(k):
        i0, i1, active = groups[k]
        with torch.no_grad():
            r, d = plan.render_colour(i0, i1, active, floater_thresh)
            V = i1 - i0
            d = d.view(V, H, W)
            rgb8, depth8, _, _ = _encode(r.view(V, H, W, 3), d, depth_minmax, lut, False, False)
        rendered = torch.cuda.Event()
        rendered.record(main)
        side.wait_event(rendered)
        src = {"rgb8": rgb8, "depth8": depth8, "depth": d}
        slot = ring[k % 2]
        with torch.cuda.stream(side):
            for name in names:
                slot[name][:V].copy_(src[name], non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(side)
        pending[k % 2] = (k, copied, src)

    def drain(k):
        _, copied, _ = pending[k % 2]
        copied.synchronize()
        i0, i1, _ = groups[k]
        slot = ring[k % 2]
        host = {name: slot[name][:i1 - i0].numpy().copy() for name in names}
        pending[k % 2] = None                                   # the device tensors may go back to the allocator now
        return [(i0 + j,) + tuple(host[name][j] for name in names) for j in range(i1 - i0)]

    try:
        with torch.cuda.device(dev):
            launch(0)
            for k in range(1, len(groups) + 1):
                if k < len(groups):
                    launch(k)                                   # renders while group k - 1 copies
                for item in drain(k - 1):
                    yield item
    finally:
        side.synchronize()
        main.synchronize()
