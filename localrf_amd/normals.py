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
from .pose_plan import PosePlan


def render_normals(local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, floater_thresh=0, chunk=4096):
    """The normal map of every pose: frame i at its pose through the blending weights of its nearest training frame, as
    novel_views.render_poses chooses it (poses, frame_indices and start mean what they mean there; test_frames is accepted
    for the same call shape and changes nothing, because exposure does not apply to a normal).
    chunk bounds the rays of one field call, and with them the [chunk, S] sample weights the call keeps; the result does not
    depend on it, bit for bit.
    Returns {"normal": [N,H,W,3] fp32, "acc": [N,H,W] fp32} on the scene's device: normal = sum_k blend_w N_k, acc =
    sum_k blend_w acc_k, |normal| <= acc.  Raises ValueError before any launch for a frame whose nearest frame has no
    active field."""
    plan = PosePlan(local_tensorfs, poses, W, H, test_frames, frame_indices, start, None, chunk).on_device()
    n, W, H, dev = plan.n, plan.W, plan.H, plan.dev
    normal = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)
    acc = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        # per span of rays, the active fields in the reference's field order: the first overwrites normal / acc, the others add
        for i0, i1, active in plan.calls:
            nrm, a = normal[i0:i1].view(-1, 3), acc[i0:i1].view(-1)
            for r0, r1, calls in plan.group_spans(i0, i1, active):
                for k, (f, z, flags, rays, bw) in enumerate(calls):
                    f._native_normals(rays, z, flags, float(floater_thresh), blend_w=bw, per_view=W * H,
                                      out=(nrm[r0:r1], a[r0:r1]), accumulate=k > 0)
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
