"""Per-ray surface normals of a scene on the GPU: the third map of the renderer beside colour and depth, and the oriented
normals a point cloud needs for meshing (csrc/lrf_normals.inl through lrf_render_normals).

  render_normals(local_tensorfs, poses, W, H, ...)  the normal map [N,H,W,3] and acc [N,H,W] of every pose
  normal_colours(normal)                            0.5 N / max(|N|, 1e-8) + 0.5, the colour a normal map is drawn with
  encode_normals(normal)                            those colours as uint8 bytes (encode_frames' byte conversion)

A field's ray normal is N = sum over the samples its colour pass shades of w_i n_i, n_i = -grad g / max(|grad g|, 1e-8) with
g(x) = density_feature(u(contract(x))) (TensorVMSplit.render_normals); a scene's is sum_k blend_w[v, k] N_k over the active
fields, the blend lrf_scene_blend applies to depth.  Fields are translations of the world, so the orientation is the
world's.  Exposure does not apply.  N is not normalised: |N| <= acc, and a ray through empty space gives exactly (0, 0, 0).
Every function checks its arguments before its first launch.  CPU tensors raise NativeError: there is no torch fallback.
"""
import torch

from . import _native as N
from . import novel_views
from .scene_ops import scene_rays


def _group_spans(lt, poses, vids, i0, i1, active, W, H, chunk):
    """The per-field calls of frames i0..i1 (one active set), shared with depth_quantiles: yields (r0, r1, calls) per span of
    rays, calls = [(f, z, flags, rays [r1 - r0, 6], blend_w)] over the active fields in the reference's field order, blend_w
    being the field's weights from the span's first view on (per_view = H W).  A span holds whole views when chunk covers
    one, else part of a single view."""
    dev = lt.blending_weights.device
    V, HW = i1 - i0, W * H
    fields = [lt.tensorfs[rf] for rf in active]
    for f in fields:
        if f.device != dev:
            f.to(dev)
    pinhole = lt.fov != 360
    ray_ids = torch.arange(V * HW, dtype=torch.int64, device=dev)
    rays, _, _ = scene_rays(ray_ids, poses[i0:i1], lt._shifts(lt.world2rf, list(active)), lt.focal(W) if pinhole else None,
                            lt.center(W, H) if pinhole else None, HW, W, H, not pinhole)
    bw = lt.blending_weights[vids[i0:i1]].index_select(1, torch.tensor(active, dtype=torch.int64).to(dev, non_blocking=True))
    bw = N.conform(bw.t())                                          # [n_active, V]: a field's weights are one contiguous row
    plan = []
    for f in fields:
        z = f.z_schedule(False, -1, dev).detach().contiguous().float().view(-1)
        flags = f._flags(True) | (N.LRF_FLAG_PE_OFF if (f.fea_pe > 0 and not lt.is_refining) else 0)
        plan.append((f, z, flags))
    if chunk >= HW:                                                 # whole views per call
        step = (chunk // HW) * HW
        spans = [(r0, min(V * HW, r0 + step)) for r0 in range(0, V * HW, step)]
    else:                                                           # a call never crosses a view: one blend weight per call
        spans = [(v * HW + r0, v * HW + min(HW, r0 + chunk)) for v in range(V) for r0 in range(0, HW, chunk)]
    for r0, r1 in spans:
        yield r0, r1, [(f, z, flags, rays[k, r0:r1], bw[k, r0 // HW:]) for k, (f, z, flags) in enumerate(plan)]


def _render_group(lt, poses, vids, i0, i1, active, W, H, floater_thresh, chunk, normal, acc):
    """Frames i0..i1 (one active set): per chunk of rays, the active fields in the reference's field order, the first
    overwriting normal / acc and the others adding to them."""
    normal, acc = normal[i0:i1].view(-1, 3), acc[i0:i1].view(-1)
    for r0, r1, calls in _group_spans(lt, poses, vids, i0, i1, active, W, H, chunk):
        for k, (f, z, flags, rays, bw) in enumerate(calls):
            f._native_normals(rays, z, flags, floater_thresh, blend_w=bw, per_view=W * H, out=(normal[r0:r1], acc[r0:r1]),
                              accumulate=k > 0)


def render_normals(local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, floater_thresh=0, chunk=4096):
    """The normal map of every pose: frame i at its pose through the blending weights of its nearest training frame, as
    novel_views.render_poses chooses it (poses, frame_indices and start mean what they mean there; test_frames is accepted
    for the same call shape and changes nothing, because exposure does not apply to a normal).
    chunk bounds the rays of one field call, and with them the [chunk, S] sample weights the call keeps; the result does not
    depend on it, bit for bit.
    Returns {"normal": [N,H,W,3] fp32, "acc": [N,H,W] fp32} on the scene's device: normal = sum_k blend_w N_k, acc =
    sum_k blend_w acc_k, |normal| <= acc.  Raises ValueError before any launch for a frame whose nearest frame has no
    active field."""
    lt, poses, views, vids, _, groups, W, H, dev, _, _ = novel_views._prepare(
        local_tensorfs, poses, W, H, test_frames, frame_indices, start, None, chunk, None, None, False)
    n = len(views)
    normal = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)
    acc = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        for i0, i1, active in groups:
            _render_group(lt, poses, vids, i0, i1, active, W, H, float(floater_thresh), int(chunk), normal, acc)
    return {"normal": normal, "acc": acc}


def _check_normal(normal):
    if not torch.is_tensor(normal):
        raise TypeError("normal must be a torch tensor")
    if not normal.is_floating_point():
        raise ValueError(f"normal must hold floating-point values, got {normal.dtype}")
    if normal.dim() < 1 or normal.shape[-1] != 3:
        raise ValueError(f"normal must be [..., 3], got {tuple(normal.shape)}")


def unit_normals(normal):
    """N / max(|N|, 1e-8) of [..., 3] -> (unit [..., 3] fp32, length [...]); a zero-length row stays zero."""
    _check_normal(normal)
    n = normal.detach().float()
    length = torch.linalg.vector_norm(n, dim=-1)
    return n / length.clamp(min=1e-8)[..., None], length


def normal_colours(normal):
    """0.5 N / max(|N|, 1e-8) + 0.5 of [..., 3]: the colour a normal map is drawn with, 0.5 grey where the normal is zero."""
    return 0.5 * unit_normals(normal)[0] + 0.5


def encode_normals(normal):
    """normal [N,H,W,3] (device) -> [N,H,W,3] uint8: normal_colours through encode_frames' byte conversion
    (clamp(rint(255 x), 0, 255), ties to even), so a unit axis gives 255 / 128 / 0 and a zero-length normal 128, 128, 128."""
    _check_normal(normal)
    if normal.dim() < 3 or min(normal.shape[-3:-1]) < 1:
        raise ValueError(f"normal must be [..., H, W, 3] with H, W > 0, got {tuple(normal.shape)}")
    N.require_gpu(normal, "normal", "the encoding")
    unit, length = unit_normals(normal)
    return novel_views.encode_frames(0.5 * unit + 0.5, length)[0]   # (the lengths stand in for the depth the call also encodes)
