"""The argument checks that more than one geometry module needs (pointcloud, mesh, mesh_raster, mesh_texture, mesh_distance,
cloud, alignment), the one place each where a mesh's and a point tensor's device is required to be a GPU, and the batcher of
the launches over points.  A check that a single module uses stays in that module.

  check_int, check_positive, check_interval, check_flag    one scalar each; bools, non-numbers and NaN are refused
  check_range, check_origin, check_bytes, check_size       depth_range, three finite values, max_bytes, an image's W and H
  check_mesh, check_faces, mesh_on_device                  the mesh dict of mesh.py: host checks, then the device
  check_points, points_on_device                           a [N,3] fp32 tensor: host checks, then the device
  check_max_distance, check_thresholds, check_unit         the arguments of the distance queries and of their summary
  chunks, POINTS_PER_CALL                                  (first item, count) of each launch over n points
  check_depth, check_frame_poses, check_intrinsics, check_rgb   the frame arguments; dev_f32 and rgb8_frames are their device half

Every check runs on the host and returns the value in the type the caller passes on; a refusal is a ValueError naming the
argument (TypeError for a value that is not a tensor or a mesh).  Callers keep the order type, then dtype and shape, then
their other arguments, then the device: mesh_on_device, points_on_device and the require_gpu calls come last.
"""
import math

import numpy as np
import torch

from . import _native as N
from . import novel_views
from .pose_plan import check_poses

INT32 = (1 << 31) - 1


def check_int(name, x, lo, hi=math.inf, wording=None, none_ok=False):
    """x as an int in [lo, hi]; `wording` states the bound in the refusal (default: an integer in [lo, hi])."""
    if x is None and none_ok:
        return None
    try:
        ok = not isinstance(x, (bool, np.bool_)) and int(x) == x and lo <= int(x) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be {wording or f'an integer in [{lo}, {hi}]'}, got {x!r}")
    return int(x)


def check_positive(name, x):
    try:
        ok = not isinstance(x, (bool, np.bool_)) and math.isfinite(float(x)) and float(x) > 0
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be a finite number > 0, got {x!r}")
    return float(x)


def check_interval(name, x, lo, hi, wording, open_lo=False):
    """x as a float in [lo, hi], or (lo, hi] with open_lo; `wording` states the interval in the refusal."""
    try:
        t = math.nan if isinstance(x, (bool, np.bool_)) else float(x)
    except (TypeError, ValueError):
        t = math.nan
    if not lo <= t <= hi or (open_lo and t == lo):                  # NaN fails
        raise ValueError(f"{name} must {wording}, got {x!r}")
    return t


def check_flag(name, x):
    if not isinstance(x, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {x!r}")
    return bool(x)


def check_choice(name, x, choices):
    """x as one of the strings `choices`."""
    if not isinstance(x, str) or x not in choices:
        raise ValueError(f"{name} must be one of {', '.join(repr(c) for c in choices)}, got {x!r}")
    return x


def check_range(depth_range):
    if len(depth_range) != 2:
        raise ValueError(f"depth_range must be (d_min, d_max), got {depth_range!r}")
    d_min, d_max = float(depth_range[0]), float(depth_range[1])
    if not d_min <= d_max:
        raise ValueError(f"depth_range needs d_min <= d_max, got {depth_range!r}")
    return d_min, d_max


def check_origin(origin):
    try:
        o = np.asarray(origin.detach().cpu() if torch.is_tensor(origin) else origin, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.size != 3 or not np.isfinite(o).all():
        raise ValueError(f"origin must hold 3 finite values, got {origin!r}")
    return tuple(float(x) for x in o)


def check_bytes(max_bytes):
    return check_int("max_bytes", max_bytes, 0, wording="an integer >= 0")


def check_size(W, H):
    try:
        ok = all(not isinstance(s, (bool, np.bool_)) and int(s) == s and int(s) >= 1 for s in (W, H))
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"need integers W, H > 0, got {W!r} x {H!r}")
    if int(W) * int(H) > INT32:
        raise ValueError(f"an image of {H} x {W} pixels; one rasterisation takes H W < 2^31")
    return int(W), int(H)


def check_faces(faces, n_vertices):
    """type, then dtype and shape -> (Nv, Nf); the device check is the caller's, after its other arguments."""
    if not torch.is_tensor(faces):
        raise TypeError("faces must be a torch tensor")
    if faces.dtype is not torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [Nf, 3] int32, got {faces.dtype} {tuple(faces.shape)}")
    Nv = check_int("n_vertices", n_vertices, 0, INT32, "an integer in [0, 2^31)")
    if faces.shape[0] > INT32:
        raise ValueError(f"faces holds {faces.shape[0]} rows; a mesh takes Nf < 2^31")
    if Nv == 0 and faces.shape[0]:
        raise ValueError(f"faces holds {faces.shape[0]} rows for a mesh without vertices")
    return Nv, int(faces.shape[0])


def check_mesh(mesh):
    """type, then dtype and shape -> (vertices, faces, rgb8 or None, Nv, Nf) as given; mesh_on_device is the device half."""
    if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
        raise TypeError("mesh must be a dict with vertices and faces, as extract_mesh returns it")
    v, f, c = mesh["vertices"], mesh["faces"], mesh.get("rgb8")
    for name, t in (("vertices", v), ("faces", f)) + ((("rgb8", c),) if c is not None else ()):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch tensor" + (" or None" if name == "rgb8" else ""))
    if v.dtype is not torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be [Nv, 3] float32, got {v.dtype} {tuple(v.shape)}")
    Nv, Nf = check_faces(f, int(v.shape[0]))
    if c is not None and (c.dtype is not torch.uint8 or tuple(c.shape) != (Nv, 3)):
        raise ValueError(f"rgb8 must be {(Nv, 3)} uint8 or None, got {c.dtype} {tuple(c.shape)}")
    return v, f, c, Nv, Nf


def mesh_on_device(v, f, c, feature):
    """The device half of check_mesh, after the call's other arguments: vertices, faces and (unless None: the feature does
    not read it) rgb8 on one GPU -> (vertices, faces, rgb8 or None, device), contiguous."""
    N.require_gpu(v, "vertices", feature)
    N.require_gpu(f, "faces", feature)
    if c is not None:
        N.require_gpu(c, "rgb8", feature)
    dev = v.device
    if f.device != dev or (c is not None and c.device != dev):
        raise ValueError(("vertices and faces" if c is None else "vertices, faces and rgb8") + " must live on the same device")
    return v.detach().contiguous(), f.detach().contiguous(), None if c is None else c.contiguous(), dev


def check_points(points):
    if not torch.is_tensor(points):
        raise TypeError("points must be a torch tensor")
    if points.dtype is not torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N, 3] float32, got {points.dtype} {tuple(points.shape)}")
    return int(points.shape[0])


def points_on_device(t, name, feature, dev=None, wording=None):
    """The device half of check_points, after the call's other arguments: t on a GPU (NativeError naming it) and, with dev -- an
    index's device or a first tensor's -- on that one (ValueError(wording): the callers' sentences differ) -> t detached and
    contiguous.  Also for what goes with the points (a viewpoint per point, normals, a keep mask, uint8 colours, which are
    not detached)."""
    N.require_gpu(t, name, feature)
    if dev is not None and t.device != dev:
        raise ValueError(wording)
    return t.contiguous() if t.dtype is torch.uint8 else t.detach().contiguous()


def check_max_distance(max_distance):
    try:
        ok = not isinstance(max_distance, (bool, np.bool_)) and float(max_distance) >= 0        # NaN fails
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"max_distance must be a number >= 0 or infinity, got {max_distance!r}")
    return float(max_distance)


def check_thresholds(thresholds):
    try:
        taus = [float(t) for t in thresholds if not isinstance(t, (bool, np.bool_))]
        ok = len(taus) == len(thresholds)
    except (TypeError, ValueError, OverflowError):
        taus, ok = [], False
    if not ok:
        raise ValueError(f"thresholds must be a sequence of numbers, got {thresholds!r}")
    if len(taus) > N.LRF_DISTANCE_MAX_THRESHOLDS:
        raise ValueError(f"at most {N.LRF_DISTANCE_MAX_THRESHOLDS} thresholds, got {len(taus)}")
    if not all(math.isfinite(t) and t > 0 for t in taus):
        raise ValueError(f"every threshold must be a finite number > 0, got {thresholds!r}")
    taus = [float(np.float32(t)) for t in taus]                     # the kernel compares in fp32
    if not all(math.isfinite(t) and t > 0 for t in taus):
        raise ValueError(f"every threshold must be finite and > 0 as float32, got {thresholds!r}")
    return taus


def check_unit(unit):
    unit = check_positive("unit", unit)
    if not (math.isfinite(float(np.float32(unit))) and float(np.float32(unit)) > 0):
        raise ValueError(f"unit must be finite and > 0 as float32, got {unit!r}")
    return unit


POINTS_PER_CALL = 1 << 30                      # what one launch over points takes; chunks reads it at each call


def chunks(n, per_call=None):
    """(i0, m) per launch over n items taken per_call (None: POINTS_PER_CALL) at a time: m items from item i0.  None for n = 0."""
    per_call = POINTS_PER_CALL if per_call is None else per_call
    for i0 in range(0, n, per_call):
        yield i0, min(per_call, n - i0)


def float_of_key(key):
    """The fp32 value of the bounds kernels' order-preserving integer, as a Python float."""
    bits = (key ^ ((key >> 31) & 0x7FFFFFFF)) & 0xFFFFFFFF
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def check_depth(depth):
    if not torch.is_tensor(depth):
        raise TypeError("depth must be a torch tensor")
    if not depth.is_floating_point():
        raise ValueError(f"depth must hold floating-point values, got {depth.dtype}")
    if depth.dim() != 3 or min(depth.shape) < 1:
        raise ValueError(f"depth must be [V, H, W] with V, H, W > 0, got {tuple(depth.shape)}")
    V, H, W = (int(s) for s in depth.shape)
    if V * H * W > INT32:
        raise ValueError(f"depth holds {V * H * W} pixels; one call takes V H W < 2^31")
    return V, H, W


def check_frame_poses(poses, V, what="depth frames"):
    poses = check_poses(poses)
    if poses.shape[0] != V:
        raise ValueError(f"{poses.shape[0]} poses for {V} {what}")
    return poses


def check_intrinsics(focal, center, fov360):
    """-> (focal, center) as given (tensors or numbers), shapes checked; None, None for 360."""
    if fov360:
        return None, None
    if focal is None or center is None:
        raise ValueError("a pinhole camera needs focal and center (or pass fov360=True)")
    nf = focal.numel() if torch.is_tensor(focal) else np.size(focal)
    nc = center.numel() if torch.is_tensor(center) else np.size(center)
    if nf != 1 or nc != 2:
        raise ValueError(f"focal must hold 1 value and center 2 (cx, cy), got {nf} and {nc}")
    return focal, center


def check_rgb(rgb, depth):
    """rgb (not None) against the checked depth [V,H,W] it colours: type, dtype, shape, then the same device."""
    if not torch.is_tensor(rgb):
        raise TypeError("rgb must be a torch tensor or None")
    if not (rgb.is_floating_point() or rgb.dtype is torch.uint8):
        raise ValueError(f"rgb must hold floating-point or uint8 values, got {rgb.dtype}")
    if tuple(rgb.shape) != tuple(depth.shape) + (3,):
        raise ValueError(f"rgb must be {tuple(depth.shape) + (3,)} to go with depth {tuple(depth.shape)}, got {tuple(rgb.shape)}")
    if rgb.device != depth.device:
        raise ValueError("rgb and depth must live on the same device")


def rgb8_frames(rgb, depth):
    """Checked rgb [V,H,W,3] as uint8 on the device: uint8 passes through, float is encoded as novel_views.encode_frames does
    (which takes the frames' depth along)."""
    if rgb.dtype is torch.uint8:
        return rgb.contiguous()
    return novel_views.encode_frames(rgb.detach(), depth.detach())[0]


def dev_f32(x, n, dev):
    t = x if torch.is_tensor(x) else torch.tensor(np.asarray(x, np.float32).reshape(n))
    return t.detach().reshape(n).to(device=dev, dtype=torch.float32).contiguous()
