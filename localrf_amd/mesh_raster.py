"""A triangle mesh rasterised into camera poses on the GPU, and its depth compared with rendered depth (csrc/lrf_mesh_raster.inl
through lrf_mesh_rasterize and lrf_depth_agreement): the inverse of mesh.TsdfVolume.integrate, which closes the chain
field -> depth -> volume -> mesh -> depth -> agreement with the field.

  rasterize(mesh, poses, W, H, focal, center, ...)   depth, hit face, colour, barycentric weights and crossing counts per pixel
  depth_agreement(mesh_depth, depth, ...)            integer counts and the mean relative error of two depth maps
  scene_mesh_agreement(local_tensorfs, mesh, W, H)   the scene rendered in batches, the mesh rasterised at the same poses, the
                                                     agreement accumulated; nothing is kept per frame

A mesh is the dict of mesh.py.  Depth follows the convention of pointcloud.py and mesh.py: a multiple of the un-normalised
direction pixel_dir gives, whose z is -1, so TsdfVolume.integrate(rasterize(mesh, ...)["depth"], ...) consumes it unchanged; 0.0
means no surface, which backproject, fuse_points and integrate all drop.  Pinhole cameras only.  The same bytes on every run.
Every function checks its arguments on the host before its first launch.  CPU tensors raise NativeError: there is no torch
fallback.
"""
import ctypes as C
import math

import torch

from . import _native as N
from ._native import NativeError  # noqa: F401
from ._checks import INT32 as _INT32
from ._checks import (check_bytes, check_depth, check_flag, check_int, check_intrinsics, check_mesh, check_range, check_size, dev_f32,
                      mesh_on_device)
from .pointcloud import SceneFrames
from .pose_plan import check_poses

_CULL = {None: 0, "back": 1, "front": 2}
AGREEMENT_SCALE = 1 << 24                      # the fixed point of the relative-error sum
AGREEMENT_CLAMP = 16.0                         # a pixel's relative error enters the sum clamped to this
_MAX_FRAMES = 65535                            # frames per lrf_depth_agreement call


def _check_cull(cull):
    if not (cull is None or isinstance(cull, str)) or cull not in _CULL:
        raise ValueError(f"cull must be None, 'back' or 'front', got {cull!r}")
    return _CULL[cull]


def _check_small_max(small_max):
    return check_int("small_max", small_max, 0, _INT32, "None or an integer in [0, 2^31)", none_ok=True)


def frames_per_call(W, H, Nf, max_bytes):
    """How many frames one native call takes under max_bytes of workspace: 8 H W bytes of keys and 8 Nf of list per frame."""
    per_frame = 8 * H * W + 8 * Nf
    if per_frame + 8 > max_bytes:
        raise ValueError(f"one frame of {H} x {W} pixels and {Nf} faces takes a workspace of {per_frame + 8} bytes; max_bytes is "
                         f"{max_bytes}")
    return max(1, min((max_bytes - 8) // per_frame, _INT32 // max(H * W, Nf, 1)))


def rasterize(mesh, poses, W, H, focal, center, *, depth_range=(0.0, math.inf), cull=None, crossings=False, weights=False,
              max_bytes=1 << 30, small_max=None):
    """The mesh (the dict of mesh.py) seen from poses [V,3,4] camera-to-world by W x H pinhole cameras with focal (one value) and
    center (cx, cy) as pointcloud.fuse_points takes them (csrc/lrf_mesh_raster.inl states every rule).  Returns a dict of device
    tensors: depth [V,H,W] fp32, 0.0 where the pixel's ray hits no face; face [V,H,W] int32, the face hit, -1 for none; rgb8
    [V,H,W,3] uint8 when the mesh has rgb8 (the hit's vertex colours under its barycentric weights, rounded to nearest), else None;
    with weights=True weights [V,H,W,3] fp32, the barycentric weights of the hit (0 without one), so that a caller can interpolate
    any vertex attribute; with crossings=True crossings [V,H,W] int32, the faces of either orientation the ray crosses inside
    depth_range: even outside a closed mesh, odd inside; and info: the Python ints bad_index_faces (an index outside [0, Nv):
    never dereferenced), degenerate_faces (two equal indices) and nonfinite_faces (a coordinate that is not finite), all skipped.
    A hit is kept when its depth is finite, positive and inside depth_range; the nearest kept hit wins, and of equal depths the
    smallest face index.  cull="back" drops the faces seen from behind their winding's normal (for a TSDF mesh: from inside the
    surface), cull="front" those seen from the normal's side, None keeps both.  Coverage is decided by edge functions of exact
    sign with one symbolic tie-break for the whole image: a ray through a vertex or along an edge of a closed mesh hits exactly
    one of the faces that meet there.  Faces that straddle the camera plane need no clipping.
    The frames are rasterised frames_per_call(W, H, Nf, max_bytes) at a time (a workspace of 8 H W + 8 Nf bytes per frame; a
    single frame above max_bytes raises ValueError); the outputs stay resident.  One read-back: info.  small_max (None: the
    library's measured default) is the largest pixel box a face's own lane walks, larger ones go to a wavefront
    (lrf_debug_mesh_rasterize); the outputs do not depend on it."""
    v, f, c, Nv, Nf = check_mesh(mesh)
    poses = check_poses(poses)
    V = int(poses.shape[0])
    if V < 1:
        raise ValueError("rasterize: no pose to rasterise into")
    W, H = check_size(W, H)
    focal, center = check_intrinsics(focal, center, False)
    d_min, d_max = check_range(depth_range)
    cull = _check_cull(cull)
    crossings, weights = check_flag("crossings", crossings), check_flag("weights", weights)
    max_bytes = check_bytes(max_bytes)
    small_max = _check_small_max(small_max)
    per_call = frames_per_call(W, H, Nf, max_bytes)
    v, f, c, dev = mesh_on_device(v, f, c, "the mesh rasterisation")
    poses = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    fo, ce = dev_f32(focal, 1, dev), dev_f32(center, 2, dev)
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    rgb8 = None if c is None else torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    wts = torch.empty(V, H, W, 3, dtype=torch.float32, device=dev) if weights else None
    cross = torch.empty(V, H, W, dtype=torch.int32, device=dev) if crossings else None
    info = torch.empty(4, dtype=torch.int64, device=dev)
    spare = torch.empty(4, dtype=torch.int64, device=dev)           # the later batches count the same faces again
    ws = N.workspace("lrf_mesh_rasterize", dev, min(per_call, V), H, W, Nf)
    a = N.LrfMeshRaster()
    a.vertices, a.rgb8, a.faces = v.data_ptr() if Nf else None, None if c is None else (c.data_ptr() or None), f.data_ptr() if Nf else None
    a.focal, a.center = fo.data_ptr(), ce.data_ptr()
    a.Nv, a.Nf, a.H, a.W, a.cull, a.d_min, a.d_max = Nv, Nf, H, W, cull, d_min, d_max
    if c is not None and not a.rgb8:                                # a mesh without vertices still has its colour maps
        a.rgb8 = info.data_ptr()
    for i0 in range(0, V, per_call):
        i1 = min(V, i0 + per_call)
        a.cam2world, a.V = poses[i0:].data_ptr(), i1 - i0
        args = (C.byref(a), depth[i0:].data_ptr(), face[i0:].data_ptr(), None if rgb8 is None else rgb8[i0:].data_ptr(),
                None if wts is None else wts[i0:].data_ptr(), None if cross is None else cross[i0:].data_ptr(),
                (info if i0 == 0 else spare).data_ptr(), ws.data_ptr())
        if small_max is None:
            N.launch("lrf_mesh_rasterize", dev, *args, guard=True)
        else:
            N.launch("lrf_debug_mesh_rasterize", dev, *args, small_max, guard=True)
    words = [int(x) for x in info.tolist()]                         # the read-back (it also orders ws's release)
    return {"depth": depth, "face": face, "rgb8": rgb8, "weights": wts, "crossings": cross,
            "info": {"bad_index_faces": words[0], "degenerate_faces": words[1], "nonfinite_faces": words[2]}}


def _check_tols(rel_tols):
    try:
        tols = [float(t) for t in rel_tols]
    except (TypeError, ValueError):
        raise ValueError(f"rel_tols must be a sequence of numbers, got {rel_tols!r}") from None
    if len(tols) > N.LRF_AGREEMENT_MAX_TOLS:
        raise ValueError(f"at most {N.LRF_AGREEMENT_MAX_TOLS} rel_tols, got {len(tols)}")
    if not all(t >= 0 for t in tols):                               # NaN fails
        raise ValueError(f"every rel_tol must be >= 0, got {rel_tols!r}")
    return tols


def _check_maps(mesh_depth, depth):
    V, H, W = check_depth(depth)
    if not torch.is_tensor(mesh_depth):
        raise TypeError("mesh_depth must be a torch tensor")
    if not mesh_depth.is_floating_point() or tuple(mesh_depth.shape) != (V, H, W):
        raise ValueError(f"mesh_depth must be a floating-point tensor of shape {(V, H, W)} to go with depth, got {mesh_depth.dtype} "
                         f"{tuple(mesh_depth.shape)}")
    if mesh_depth.device != depth.device:
        raise ValueError("mesh_depth and depth must live on the same device")
    return V, H, W


def _agreement_counts(mesh_depth, depth, tols, d_min, d_max, error_map):
    """Checked arguments, device tensors -> (counts int64 [V,16] on the device, the error map or None); no read-back."""
    dev = depth.device
    V, H, W = (int(s) for s in depth.shape)
    a, b = N.conform(mesh_depth), N.conform(depth)
    counts = torch.empty(V, 16, dtype=torch.int64, device=dev)
    err = torch.empty(V, H, W, dtype=torch.float32, device=dev) if error_map else None
    tol = (C.c_float * max(len(tols), 1))(*tols)
    for i0 in range(0, V, _MAX_FRAMES):
        n = min(V, i0 + _MAX_FRAMES) - i0
        N.launch("lrf_depth_agreement", dev, a[i0:].data_ptr(), b[i0:].data_ptr(), n, H, W, tol, len(tols), d_min, d_max,
                 counts[i0:].data_ptr(), None if err is None else err[i0:].data_ptr(), guard=True)
    return counts, err


def _summary(total, tols, frames):
    """The 16 int64 words of one frame, or of a sum over frames, as the dict depth_agreement returns."""
    both = int(total[0])
    return {"both": both, "mesh_only": int(total[1]), "render_only": int(total[2]), "neither": int(total[3]),
            "within": tuple(int(total[8 + k]) for k in range(len(tols))), "rel_tols": tuple(tols), "error_sum": int(total[4]),
            "mean_rel_error": int(total[4]) / AGREEMENT_SCALE / both if both else math.nan, "frames": frames}


def depth_agreement(mesh_depth, depth, *, rel_tols=(0.01, 0.05), depth_range=(0.0, math.inf), error_map=False):
    """Two depth maps [V,H,W] on the device compared pixel by pixel in one kernel: mesh_depth (rasterize's) against depth (the
    render's).  A value is valid when finite, positive and inside depth_range.  Returns a dict of Python values over all frames:
    both, mesh_only, render_only and neither (the pixels valid in both maps, in one, in none: they add up to V H W); within, per
    tolerance of rel_tols (at most 8) the both-valid pixels with |mesh_depth - depth| <= tol * depth in fp32; error_sum, the
    int64 sum over the both-valid pixels of rint(min(|mesh_depth - depth| / depth, 16) * 2^24) (AGREEMENT_CLAMP,
    AGREEMENT_SCALE); mean_rel_error = error_sum / 2^24 / both (NaN without a both-valid pixel); rel_tols and frames = V; and
    per_frame: the same integers as numpy int64 arrays [V] (within: [V, len(rel_tols)]).  All integers: the same on every run.
    error_map=True adds "error_map" [V,H,W] fp32 on the device, |mesh_depth - depth| / depth unclamped and NaN where not both
    are valid; diagnostics.quantile takes exact medians of it.  One read-back: the counts."""
    V, H, W = _check_maps(mesh_depth, depth)
    tols = _check_tols(rel_tols)
    d_min, d_max = check_range(depth_range)
    error_map = check_flag("error_map", error_map)
    N.require_gpu(depth, "depth", "the depth agreement")
    counts, err = _agreement_counts(mesh_depth, depth, tols, d_min, d_max, error_map)
    words = counts.cpu().numpy()                                    # the read-back
    out = _summary(words.sum(0), tols, V)
    out["per_frame"] = {"both": words[:, 0].copy(), "mesh_only": words[:, 1].copy(), "render_only": words[:, 2].copy(),
                        "neither": words[:, 3].copy(), "error_sum": words[:, 4].copy(), "within": words[:, 8:8 + len(tols)].copy()}
    if error_map:
        out["error_map"] = err
    return out


_AGREE_KEYS = ("depth_range", "cull", "rel_tols", "frames_per_call", "small_max")


def scene_mesh_agreement(local_tensorfs, mesh, W, H, poses=None, depth="expected", max_spread=None, max_bytes=4 << 30, **options):
    """How well a mesh agrees with the scene it came from: the scene's frames rendered by novel_views.render_poses
    frames_per_call (default 8) at a time -- the same SceneFrames / PosePlan path as mesh.scene_mesh --, the mesh rasterised at
    the same poses with the scene's focal(W) and center(W, H), depth_agreement of the two accumulated on the device, and both
    maps dropped: nothing is kept per frame.  poses=None takes the scene's own get_cam2world(), each frame through itself;
    otherwise poses [N,3,4] as render_poses takes them.  depth="median" compares with the median depth of the same frames
    (depth_quantiles.fusion_depth) and max_spread (with "median" only) drops its uncertain pixels, as scene_mesh has them.
    options: rasterize's depth_range (it bounds both maps), cull and small_max, depth_agreement's rel_tols, frames_per_call, and
    render_poses' test_frames, frame_indices, floater_thresh, chunk.  A batch whose rasterisation workspace exceeds max_bytes
    raises ValueError before anything is rendered.  Pinhole scenes only.  Returns depth_agreement's dict without per_frame
    (frames = the number of poses) and with "info": rasterize's.  One read-back per batch (rasterize's info) and one at the end."""
    lt = local_tensorfs
    frames = SceneFrames("scene_mesh_agreement", lt, W, H, poses, depth, max_spread, options, _AGREE_KEYS, False)
    W, H, n, own = frames.W, frames.H, frames.n, frames.own
    v, f, c, Nv, Nf = check_mesh(mesh)
    if lt.fov == 360:
        raise ValueError("scene_mesh_agreement: the rasterisation needs a pinhole camera: there is no reprojection at 360 degrees")
    W, H = check_size(W, H)
    depth_range = own.get("depth_range", (0.0, math.inf))
    d_min, d_max = check_range(depth_range)
    _check_cull(own.get("cull"))
    _check_small_max(own.get("small_max"))
    tols = _check_tols(own.get("rel_tols", (0.01, 0.05)))
    frames.check_per_call("comparison")
    max_bytes = check_bytes(max_bytes)
    frames_per_call(W, H, Nf, max_bytes)                            # a single frame must fit; rasterize splits a batch further
    frames.on_device()
    flat = {"vertices": v, "faces": f, "rgb8": None}                # colours are not compared
    total, info = None, None
    for poses, _, dmap in frames.batches(depth, colour=False, encode=False):      # "median" never calls render_poses
        out = rasterize(flat, poses, W, H, frames.focal, frames.center, depth_range=depth_range, cull=own.get("cull"),
                        max_bytes=max_bytes, small_max=own.get("small_max"))
        info = out["info"] if info is None else info
        counts = _agreement_counts(out["depth"], dmap, tols, d_min, d_max, False)[0].sum(0)
        total = counts if total is None else total + counts
    result = _summary(total.tolist(), tols, n)                      # the read-back
    result["info"] = info
    return result
