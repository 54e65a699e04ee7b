"""Rendered depth fused into a coloured world-space point cloud on the GPU (csrc/lrf_points.inl through lrf_points_fuse).

  backproject(depth, poses, W, H, ...)          every pixel with a finite positive depth -> (xyz [M,3], src [M,2])
  fuse_points(rgb, depth, poses, focal, ...)    strided, depth-ranged, multi-view-consistent points with colours
  scene_point_cloud(local_tensorfs, W, H, ...)  novel_views.render_poses, then fuse_points with the scene's intrinsics
  write_ply(path, xyz, rgb8, normals, faces)    binary little-endian PLY from one device -> host copy

Conventions (the reference's): a rendered depth is sum w z / |d|, a multiple of the UN-normalised camera direction whose z
is -1 for a pinhole (tensorBase.py:615, utils/ray_utils.py:14-24); the camera point is direction * depth (utils/utils.py:15-48)
and the world point R (direction * depth) + t.  The points come out in (frame, row, column) order, the same list on every
run.  One output convention for the whole module: a point list with its source (frame, pixel id), never a dense image with
holes.  Every function checks its arguments on the host before its first launch.  CPU tensors raise NativeError: there is no
torch fallback.  Cited lines are relative to the reference's localTensoRF directory.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from . import depth_quantiles, normals as normal_maps, novel_views
from ._checks import INT32 as _INT32
from ._checks import check_depth, check_frame_poses, check_int, check_intrinsics, check_range, check_rgb, dev_f32, rgb8_frames
from .pose_plan import check_poses, nearest_frames

BYTES_PER_RESIDENT_PIXEL = 7                   # scene_point_cloud keeps depth (4 B) and rgb8 (3 B) of every frame
BYTES_PER_NORMAL_PIXEL = 16                    # and with normals=True the normal map (12 B) and its acc (4 B)


def _check_filter(stride, depth_range, neighbours, rel_tol, min_consistent, fov360, max_points):
    if int(stride) != stride or int(stride) < 1:
        raise ValueError(f"stride must be an integer >= 1, got {stride!r}")
    d_min, d_max = check_range(depth_range)
    neigh = [int(o) for o in neighbours]
    if any(int(o) != o for o in neighbours):
        raise ValueError(f"neighbours must be integer frame offsets, got {neighbours!r}")
    if len(neigh) > N.LRF_POINTS_MAX_NEIGH:
        raise ValueError(f"at most {N.LRF_POINTS_MAX_NEIGH} neighbours, got {len(neigh)}")
    if 0 in neigh:
        raise ValueError("a neighbours offset must not be 0 (a frame agrees with itself)")
    if len(set(neigh)) != len(neigh):
        raise ValueError(f"neighbours holds a repeated offset: {neigh}")
    if any(abs(o) > _INT32 for o in neigh):
        raise ValueError(f"neighbours offsets must fit int32, got {neigh}")
    if neigh and fov360:
        raise ValueError("the consistency test needs a pinhole camera: there is no reprojection at 360 degrees (train.py:386-387)")
    rel_tol = float(rel_tol)
    if not rel_tol >= 0:
        raise ValueError(f"rel_tol must be >= 0, got {rel_tol}")
    if int(min_consistent) != min_consistent or int(min_consistent) < 0:
        raise ValueError(f"min_consistent must be an integer >= 0, got {min_consistent!r}")
    if max_points is not None and (int(max_points) != max_points or int(max_points) < 0):
        raise ValueError(f"max_points must be None or an integer >= 0, got {max_points!r}")
    return int(stride), d_min, d_max, neigh, rel_tol, min(int(min_consistent), _INT32)


def _fuse(depth, rgb8, poses, focal, center, fov360, stride, d_min, d_max, neigh, rel_tol, min_consistent, max_points):
    """Checked arguments, device tensors -> (xyz, rgb8 or None, src, count).  The one read-back is count."""
    dev = depth.device
    V, H, W = (int(s) for s in depth.shape)
    depth = N.conform(depth)
    poses = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    f = c = None
    if not fov360:
        f, c = dev_f32(focal, 1, dev), dev_f32(center, 2, dev)
    n_cand = V * (-(-H // stride)) * (-(-W // stride))
    cap = n_cand if max_points is None else min(int(max_points), n_cand)
    rows = max(cap, 1)
    ws = N.workspace("lrf_points", dev, V, H, W, stride)
    xyz = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    src = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    out8 = None if rgb8 is None else torch.empty(rows, 3, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    a = N.LrfPointsFuse()
    a.depth, a.rgb8, a.cam2world = depth.data_ptr(), None if rgb8 is None else rgb8.data_ptr(), poses.data_ptr()
    a.focal, a.center = (None, None) if fov360 else (f.data_ptr(), c.data_ptr())
    a.V, a.H, a.W, a.fov360, a.stride = V, H, W, int(bool(fov360)), stride
    a.d_min, a.d_max = d_min, d_max
    a.n_neigh = len(neigh)
    for k, o in enumerate(neigh):
        a.neigh[k] = o
    a.rel_tol, a.min_consistent = rel_tol, min_consistent
    N.launch("lrf_points_fuse", dev, C.byref(a), cap, xyz.data_ptr(), None if out8 is None else out8.data_ptr(), src.data_ptr(),
             count.data_ptr(), ws.data_ptr(), guard=True)
    m = int(count.item())                                          # the ONE read-back (it also orders ws's release)
    if m > cap:
        raise ValueError(f"the fused cloud holds {m} points; max_points={max_points} does not fit them")
    return xyz[:m], None if out8 is None else out8[:m], src[:m], m


def backproject(depth, poses, W, H, focal=None, center=None, fov360=False):
    """depth [V,H,W] (device), poses [V,3,4] camera-to-world -> (xyz [M,3] fp32, src [M,2] int32 = (frame, pixel id j W + i)):
    the world point of every pixel with a finite positive depth, no other filter, in (frame, row, column) order.  focal (one
    value) and center (cx, cy) may be tensors or numbers; fov360=True takes the equirectangular directions instead."""
    V, Hd, Wd = check_depth(depth)
    if (int(H), int(W)) != (Hd, Wd):
        raise ValueError(f"depth is {Hd} x {Wd} (H x W) but H, W = {H}, {W}")
    poses = check_frame_poses(poses, V)
    focal, center = check_intrinsics(focal, center, fov360)
    N.require_gpu(depth, "depth", "the point fusion")
    xyz, _, src, _ = _fuse(depth, None, poses, focal, center, bool(fov360), 1, 0.0, math.inf, [], 0.0, 0, None)
    return xyz, src


def fuse_points(rgb, depth, poses, focal, center, *, fov360=False, stride=1, depth_range=(0.0, math.inf), neighbours=(),
                rel_tol=0.02, min_consistent=1, max_points=None):
    """V rendered frames -> ONE filtered, ordered, coloured point list, on the device.
    rgb [V,H,W,3]: float (encoded as novel_views.encode_frames does: clamp(rint(255 x), 0, 255), ties to even, NaN -> 0) or
    uint8, or None for no colours; depth [V,H,W]; poses [V,3,4] camera-to-world; focal / center as backproject takes them.
    Candidates are the pixels (i, j) with i % stride == 0 and j % stride == 0.  A candidate is kept when its depth is finite,
    positive and inside depth_range and, with neighbours (signed frame offsets, at most 8, pinhole only), when its world
    point reprojected into the frames v + o that exist agrees with the depth rendered there -- |z - dn| <= rel_tol * dn at
    the nearest pixel -- in at least min(min_consistent, offsets that stayed in range) of them.  An offset that leaves the
    trajectory counts neither for nor against, so the end frames are judged by the neighbours they have.
    The defaults rel_tol=0.02 and min_consistent=1 are conveniences, not measured optima: choose them for the scene.
    Returns a dict: xyz [M,3] fp32, rgb8 [M,3] uint8 (None without rgb), src [M,2] int32 (frame, pixel id j W + i) -- device
    tensors in (frame, row, column) order, views of buffers sized for max_points rows (None: for every candidate) -- and
    count = M, a Python int: the one read-back.  A result that does not fit max_points raises ValueError naming the true count."""
    V, H, W = check_depth(depth)
    if rgb is not None:
        check_rgb(rgb, depth)
    poses = check_frame_poses(poses, V)
    focal, center = check_intrinsics(focal, center, fov360)
    stride, d_min, d_max, neigh, rel_tol, min_consistent = _check_filter(stride, depth_range, neighbours, rel_tol, min_consistent,
                                                                         fov360, max_points)
    N.require_gpu(depth, "depth", "the point fusion")
    rgb8 = None if rgb is None else rgb8_frames(rgb, depth)
    xyz, out8, src, m = _fuse(depth, rgb8, poses, focal, center, bool(fov360), stride, d_min, d_max, neigh, rel_tol,
                              min_consistent, max_points)
    return {"xyz": xyz, "rgb8": out8, "src": src, "count": m}


_FUSE_KEYS = ("stride", "depth_range", "neighbours", "rel_tol", "min_consistent", "max_points")
_RENDER_KEYS = ("test_frames", "frame_indices", "floater_thresh", "chunk", "frames_per_call")   # the last: render_poses' alone


class SceneFrames:
    """What the scene functions (`who`: scene_point_cloud, scene_mesh, scene_mesh_agreement, scene_texture) share.
    Construction checks on the host, in this order: depth= / max_spread=, unknown options (TypeError), W and H, poses (None:
    the scene's own frames, each through itself) and the frame count n >= 1.  own: the caller's options; render: those every
    renderer takes; colour: render plus frames_per_call, which only render_poses takes, when the caller forwards it.
    cam2world() is the device half, for after the caller's own checks: it refuses a CPU scene and returns the poses [n, 3, 4].
    A caller that renders frames_per_call frames at a time and keeps none calls check_per_call(noun) among its host checks,
    on_device() after them and then loops over batches(), once per pass."""

    def __init__(self, who, local_tensorfs, W, H, poses, depth, max_spread, options, own_keys, forwards_frames_per_call):
        self.who = who
        self.max_spread = depth_quantiles.check_fusion_depth(who, depth, max_spread)
        unknown = sorted(set(options) - set(own_keys) - set(_RENDER_KEYS))
        if unknown:
            raise TypeError(f"{who}: unknown options {unknown}")
        self.W, self.H = int(W), int(H)
        if self.W <= 0 or self.H <= 0:
            raise ValueError(f"need W, H > 0, got {self.W} x {self.H}")
        self.lt = local_tensorfs
        self.own = {k: options[k] for k in own_keys if k in options}
        self.render = {k: options[k] for k in _RENDER_KEYS[:-1] if k in options}
        self.poses = None if poses is None else check_poses(poses)
        self.n = len(local_tensorfs.r_c2w) if poses is None else int(self.poses.shape[0])
        if poses is None:
            self.render.setdefault("frame_indices", list(range(self.n)))
        if self.n < 1:
            raise ValueError(f"{who}: no frame to render")
        self.colour = dict(self.render)
        if forwards_frames_per_call and "frames_per_call" in options:
            self.colour["frames_per_call"] = options["frames_per_call"]

    def cam2world(self):
        N.require_gpu(self.lt.blending_weights, "the scene", "rendering")
        if self.poses is None:
            with torch.no_grad():
                return self.lt.get_cam2world().detach()
        return self.poses

    def check_per_call(self, noun):
        """The caller's own frames_per_call option (default 8): an integer >= 1 whose frames one `noun` call can take."""
        per_call = check_int("frames_per_call", self.own.get("frames_per_call", 8), 1, wording="an integer >= 1")
        if per_call * self.H * self.W > _INT32:
            raise ValueError(f"{self.who}: {per_call} frames of {self.H} x {self.W} per call; one {noun} takes V H W < 2^31")
        self.per_call = per_call

    def on_device(self):
        """The device half of a batched caller: cam, the poses of cam2world(); fi, the training frame of every pose as a list
        (the frame_indices option, else nearest_frames: one read-back), at least n long; the scene's focal and center."""
        self.cam = self.cam2world()
        fi = self.render.pop("frame_indices", None)
        if fi is None:
            fi = nearest_frames(self.lt, self.cam)
        self.fi = fi.tolist() if hasattr(fi, "tolist") else list(fi)
        if len(self.fi) < self.n:
            raise ValueError(f"frame_indices holds {len(self.fi)} entries for {self.n} poses")
        self.focal, self.center = self.lt.focal(self.W), self.lt.center(self.W, self.H)
        return self

    def batches(self, depth=None, colour=True, encode=True):
        """One pass over the frames, per_call at a time -> (poses [V,3,4], out, dmap) per batch, nothing kept.  out is
        novel_views.render_poses' dict (with `encode` as given) when colour or the expected depth is wanted, else None: that
        render is skipped.  dmap [V,H,W] is what depth= selects: out["depth"] for "expected", depth_quantiles.fusion_depth
        (one more render) for "median", None for None.  Both renderers are looked up when a batch is rendered."""
        lt, W, H = self.lt, self.W, self.H
        for i0 in range(0, self.n, self.per_call):
            i1 = min(self.n, i0 + self.per_call)
            poses, fi = self.cam[i0:i1], self.fi[i0:i1]
            out = dmap = None
            if colour or depth == "expected":
                out = novel_views.render_poses(lt, poses, W, H, frame_indices=fi, encode=encode, **self.render)
                dmap = out["depth"] if depth == "expected" else None
            if depth == "median":
                dmap = depth_quantiles.fusion_depth(lt, poses, W, H, self.max_spread, frame_indices=fi, **self.render)
            yield poses, out, dmap


def scene_point_cloud(local_tensorfs, W, H, poses=None, max_bytes=4 << 30, normals=False, orient=False, depth="expected",
                      max_spread=None, **options):
    """A scene's point cloud: its frames rendered by novel_views.render_poses, then fuse_points with the scene's focal(W),
    center(W, H) and fov.  poses=None renders the scene's own get_cam2world(), each frame through itself (frame_indices =
    0..F-1); otherwise poses [N,3,4] as render_poses takes them.  options: fuse_points' stride, depth_range, neighbours,
    rel_tol, min_consistent, max_points and render_poses' test_frames, frame_indices, floater_thresh, chunk, frames_per_call.
    Every frame's depth and rgb8 stay resident, 7 bytes per pixel (the float colours are dropped once encoded); more than
    max_bytes of them raises ValueError before anything is rendered.  A sliding window over frames is not provided.
    normals=True adds cloud["normal"] [M,3]: the scene's normal map (normals.render_normals, same poses and render options,
    16 more resident bytes per pixel) gathered at cloud["src"] and scaled to unit length, a zero-length row left as zero.
    orient=True (with normals) flips a normal that faces away from its source camera, n . (x - t_cam) > 0.
    depth="median" fuses the median depth of the same frames (depth_quantiles.median_depth: one more render pass) instead of
    render_poses' expected depth, which lies in empty space where a ray sees two surfaces; the colours stay render_poses'.
    max_spread (with "median" only) also drops the pixels whose interquartile depth range (d75 - d25) exceeds max_spread times
    their median, or that miss one of the three quartiles.  Any other depth= raises ValueError."""
    if orient and not normals:
        raise ValueError("scene_point_cloud: orient=True needs normals=True")
    lt = local_tensorfs
    frames = SceneFrames("scene_point_cloud", lt, W, H, poses, depth, max_spread, options, _FUSE_KEYS, True)
    W, H, n, fuse = frames.W, frames.H, frames.n, frames.own
    fov360 = lt.fov == 360
    _check_filter(fuse.get("stride", 1), fuse.get("depth_range", (0.0, math.inf)), fuse.get("neighbours", ()),
                  fuse.get("rel_tol", 0.02), fuse.get("min_consistent", 1), fov360, fuse.get("max_points"))
    need = (BYTES_PER_RESIDENT_PIXEL + (BYTES_PER_NORMAL_PIXEL if normals else 0)) * n * H * W
    if need > int(max_bytes):
        raise ValueError(f"scene_point_cloud: {n} frames of {H} x {W} keep {need} bytes of depth and rgb8"
                         f"{' and normals' if normals else ''} resident; max_bytes is {int(max_bytes)}")
    if n * H * W > _INT32:
        raise ValueError(f"scene_point_cloud: {n * H * W} pixels; one fusion takes V H W < 2^31")
    poses = frames.cam2world()
    out = novel_views.render_poses(lt, poses, W, H, **frames.colour)
    dmap, rgb8 = out["depth"], out["rgb8"]
    del out                                                         # the float colours go back to the allocator
    if depth == "median":
        dmap = depth_quantiles.fusion_depth(lt, poses, W, H, frames.max_spread, **frames.render)
    cloud = fuse_points(rgb8, dmap, poses, None if fov360 else lt.focal(W), None if fov360 else lt.center(W, H), fov360=fov360,
                        **fuse)
    if normals:
        nrm = normal_maps.render_normals(lt, poses, W, H, **frames.render)["normal"]
        src = cloud["src"].long()
        unit = normal_maps.unit_normals(nrm.view(n, H * W, 3)[src[:, 0], src[:, 1]])[0]
        if orient:
            t_cam = poses[:, :, 3].to(device=nrm.device, dtype=torch.float32)[src[:, 0]]
            away = ((cloud["xyz"] - t_cam) * unit).sum(-1) > 0
            unit = torch.where(away[:, None], -unit, unit)
        cloud["normal"] = unit
    return cloud


def ply_header(n, colours, normals=False, faces=None):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(n)}",
             "property float x", "property float y", "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    if colours:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    if faces is not None:
        lines += [f"element face {int(faces)}", "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, xyz, rgb8=None, normals=None, faces=None):
    """Binary little-endian PLY (x y z float, nx ny nz float when normals are given, red green blue uchar when rgb8 is
    given) of xyz [M,3], normals [M,3] and rgb8 [M,3] uint8: tensors (one device -> host copy each) or numpy arrays.
    faces [F,3] (integers in [0, M), e.g. mesh.extract_mesh's) adds `element face F` with `property list uchar int
    vertex_indices`: records of one byte 3 and three little-endian int32.  Returns the number of vertices written."""
    def host(t, dtype, name):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must be [M, 3], got {a.shape}")
        if dtype == np.uint8 and a.dtype != np.uint8:
            raise ValueError(f"rgb8 must be uint8, got {a.dtype}")
        return np.ascontiguousarray(a, dtype=dtype)
    pts = host(xyz, np.float32, "xyz")
    cols = None if rgb8 is None else host(rgb8, np.uint8, "rgb8")
    if cols is not None and cols.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} points but {cols.shape[0]} colours")
    nrm = None if normals is None else host(normals, np.float32, "normals")
    if nrm is not None and nrm.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} points but {nrm.shape[0]} normals")
    tri = None
    if faces is not None:
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
            raise ValueError(f"faces must be [F, 3] integers, got {f.dtype} {f.shape}")
        if f.size and (int(f.min()) < 0 or int(f.max()) >= pts.shape[0]):
            raise ValueError(f"faces index vertices outside [0, {pts.shape[0]})")
        tri = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", 3)]))
        tri["n"], tri["v"] = 3, f
    if cols is None and nrm is None:
        rec = pts.astype("<f4")
    else:
        fields = [("p", "<f4", 3)] + ([("n", "<f4", 3)] if nrm is not None else []) + ([("c", "u1", 3)] if cols is not None else [])
        rec = np.empty(pts.shape[0], dtype=np.dtype(fields))
        rec["p"] = pts
        if nrm is not None:
            rec["n"] = nrm
        if cols is not None:
            rec["c"] = cols
    with open(path, "wb") as fh:
        fh.write(ply_header(pts.shape[0], cols is not None, nrm is not None, None if tri is None else tri.shape[0]))
        fh.write(rec.tobytes())
        if tri is not None:
            fh.write(tri.tobytes())
    return int(pts.shape[0])
