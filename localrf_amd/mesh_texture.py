"""A texture atlas baked for an extracted mesh from rendered frames on the GPU (csrc/lrf_mesh_texture.inl through
lrf_mesh_texture_bake and lrf_mesh_texture_resolve): the last link of field -> depth -> volume -> mesh -> textured mesh.

  atlas_layout(Nf, patch, cols) / face_uv(Nf, patch, cols)   the fixed-patch layout and the uv of every face corner
  TextureBaker(mesh, ...).add(rgb, poses, ...).finish()      frames folded into a per-texel state, then resolved to bytes
  scene_texture(local_tensorfs, mesh, W, H)                  the scene rendered in batches, the mesh rasterised at the same
                                                             poses, the frames baked; nothing is kept per frame
  sample_texture(raster_out, tex)                            the atlas looked up at rasterize(weights=True)'s hits (previews)
  write_obj(path, mesh, tex)                                 OBJ + MTL + PNG, standard library only

The layout is a uniform patch: every pair of faces gets patch x patch texels, whatever its area.  That is deliberate:
marching-tetrahedra faces are voxel-sized and simplify's faces are cell-sized, so one size fits the meshes this package makes;
per-face sizes, chart packing, seam levelling, exposure compensation and mip-safe gutters are out of scope.  A mesh is the dict
of mesh.py.  Depth follows mesh_raster.py's convention.  Pinhole cameras only.  The same bytes on every run and however the
frames are split over add() calls.  Every function checks its arguments on the host before its first launch, in the order mesh,
layout, frames, poses, intrinsics, options, device.  CPU tensors raise NativeError: there is no torch fallback.
"""
import ctypes as C
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _native as N
from ._native import NativeError  # noqa: F401
from . import mesh_raster
from ._checks import INT32 as _INT32
from ._checks import (check_bytes, check_flag, check_frame_poses, check_int, check_interval, check_intrinsics, check_mesh, check_range,
                      check_size, dev_f32, mesh_on_device, rgb8_frames)
from .pointcloud import SceneFrames

_BLEND = {"mean": 0, "best": 1}
INFO_KEYS = ("bad_index_faces", "degenerate_faces", "nonfinite_faces", "zero_area_faces", "used_texels", "observed_texels",
             "fallback_texels", "empty_texels")


def atlas_layout(Nf, patch=8, cols=None):
    """-> (rows, cols, Ht, Wt): faces 2c and 2c + 1 share cell c of patch x patch texels, cols cells per row (None:
    ceil(sqrt(n_cells)) by integer arithmetic, 1 for no face), rows = ceil(n_cells / cols), the atlas Ht = rows patch by
    Wt = cols patch.  Refuses 2^31 texels or more: one bake takes fewer."""
    Nf = check_int("Nf", Nf, 0, _INT32)
    P = check_int("patch", patch, 4, 64)
    cells = (Nf + 1) // 2
    if cols is None:
        cols = max(1, math.isqrt(cells - 1) + 1 if cells > 0 else 1)
    cols = check_int("cols", cols, 1, _INT32)
    rows = -(-cells // cols)
    if rows * cols * P * P > _INT32:
        raise ValueError(f"an atlas of {rows} x {cols} cells of {P} x {P} texels; one bake takes fewer than 2^31 texels")
    return rows, cols, rows * P, cols * P


def face_uv(Nf, patch=8, cols=None):
    """uv [Nf,3,2] fp32 (CPU) of every face corner: (px / Wt, 1 - py / Ht) formed in fp64 and rounded once, with the corners in
    atlas pixels, cell origin (X0, Y0), K = patch - 3: an even face (X0 + .5, Y0 + .5), (X0 + K + .5, Y0 + .5),
    (X0 + .5, Y0 + K + .5); an odd face (X0 + P - .5, Y0 + P - .5), (X0 + P - K - .5, Y0 + P - .5), (X0 + P - .5, Y0 + P - K - .5)."""
    rows, cols, Ht, Wt = atlas_layout(Nf, patch, cols)
    P, K = int(patch), int(patch) - 3
    f = np.arange(Nf, dtype=np.int64)
    c, odd = f // 2, (f % 2).astype(np.float64)
    X0, Y0 = ((c % cols) * P).astype(np.float64), ((c // cols) * P).astype(np.float64)
    sgn = 1.0 - 2.0 * odd
    ox, oy = X0 + 0.5 + odd * (P - 1), Y0 + 0.5 + odd * (P - 1)                                  # corner 0
    px = np.stack([ox, ox + sgn * K, ox], 1)
    py = np.stack([oy, oy, oy + sgn * K], 1)
    uv = np.stack([px / max(Wt, 1), 1.0 - py / max(Ht, 1)], -1)
    return torch.from_numpy(uv.astype(np.float32).reshape(Nf, 3, 2))


def _check_options(blend, vis_tol, min_cos, two_sided):
    if not isinstance(blend, str) or blend not in _BLEND:
        raise ValueError(f"blend must be 'mean' or 'best', got {blend!r}")
    try:
        vis_tol, min_cos = float(vis_tol), float(min_cos)
    except (TypeError, ValueError):
        raise ValueError(f"vis_tol and min_cos must be numbers, got {vis_tol!r} and {min_cos!r}") from None
    if not vis_tol >= 0:
        raise ValueError(f"vis_tol must be >= 0, got {vis_tol}")
    return _BLEND[blend], vis_tol, check_interval("min_cos", min_cos, 0.0, 1.0, "lie in [0, 1]"), check_flag("two_sided", two_sided)


def _check_fill(fill):
    try:
        vals = [int(x) for x in fill]
        ok = len(vals) == 3 and all(int(x) == x and 0 <= int(x) <= 255 and not isinstance(x, bool) for x in fill)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"fill must be three integers in [0, 255], got {fill!r}")
    return vals


class TextureBaker:
    """The per-texel state of one atlas for one mesh on the device: state [Ht,Wt,4] fp32 = (c_r, c_g, c_b, w), zero at creation.
    patch, cols: atlas_layout's.  blend="mean" averages the frames that see a texel under the weight cos^2 / distance^2 (head-on
    and close counts most); "best" keeps the one frame of largest weight, the earliest of equal ones.  A frame sees a texel
    when the texel projects into the image in front of the camera, the mesh's depth at its nearest pixel is within vis_tol
    (relative) of its own, and the cosine between the face normal and the direction to the camera is at least min_cos;
    two_sided=False also drops the frames behind the winding's normal.  The mesh is held, not copied; the constructor checks on
    the host only, the device is looked at by the first add(), finish() or state."""

    def __init__(self, mesh, patch=8, cols=None, blend="mean", vis_tol=0.02, min_cos=0.2, two_sided=False):
        v, f, c, Nv, Nf = check_mesh(mesh)
        self.rows, self.cols, self.Ht, self.Wt = atlas_layout(Nf, patch, cols)
        self.patch = int(patch)
        self.blend, self.vis_tol, self.min_cos, self.two_sided = _check_options(blend, vis_tol, min_cos, two_sided)
        self.Nv, self.Nf, self.frames = Nv, Nf, 0
        self._mesh, self._state, self.device = (v, f, c), None, None

    def _ready(self):
        """The device half of the construction, at the first add(), finish() or state: after every host check."""
        if self._state is not None:
            return
        self._v, self._f, self._c, self.device = mesh_on_device(*self._mesh, "the texture bake")
        self._state = torch.zeros(self.Ht, self.Wt, 4, dtype=torch.float32, device=self.device)

    @property
    def state(self):
        self._ready()
        return self._state

    def _args(self):
        a = N.LrfMeshTexture()
        a.vertices, a.faces = (self._v.data_ptr(), self._f.data_ptr()) if self.Nf else (None, None)
        a.rgb8 = None if self._c is None or not self.Nf else self._c.data_ptr()
        a.Nv, a.Nf, a.patch, a.cols, a.blend, a.two_sided = self.Nv, self.Nf, self.patch, self.cols, self.blend, int(self.two_sided)
        a.vis_tol, a.min_cos = self.vis_tol, self.min_cos
        return a

    def add(self, rgb, poses, focal, center, mesh_depth=None, depth_range=(0.0, math.inf), max_bytes=1 << 30):
        """Fold V frames into the state, in frame order: rgb [V,H,W,3] uint8, or float encoded as novel_views.encode_frames does
        (as TsdfVolume.integrate takes it), poses [V,3,4] camera-to-world, focal (one value) and center (cx, cy).  mesh_depth
        [V,H,W] is the mesh's own depth at those poses, the visibility test; None: rasterize(mesh, poses, ...)["depth"] inside
        depth_range, with cull="back" unless two_sided.  The frames go mesh_raster.frames_per_call(W, H, Nf, max_bytes) at a
        time; the state does not depend on the split.  No read-back beyond rasterize's own."""
        if not torch.is_tensor(rgb):
            raise TypeError("rgb must be a torch tensor")
        if not (rgb.is_floating_point() or rgb.dtype is torch.uint8):
            raise ValueError(f"rgb must hold floating-point or uint8 values, got {rgb.dtype}")
        if rgb.dim() != 4 or rgb.shape[3] != 3 or min(rgb.shape) < 1:
            raise ValueError(f"rgb must be [V, H, W, 3] with V, H, W > 0, got {tuple(rgb.shape)}")
        V, H, W = (int(s) for s in rgb.shape[:3])
        check_size(W, H)
        if mesh_depth is not None:
            if not torch.is_tensor(mesh_depth):
                raise TypeError("mesh_depth must be a torch tensor or None")
            if not mesh_depth.is_floating_point() or tuple(mesh_depth.shape) != (V, H, W):
                raise ValueError(f"mesh_depth must be a floating-point tensor of shape {(V, H, W)} to go with rgb, got "
                                 f"{mesh_depth.dtype} {tuple(mesh_depth.shape)}")
        poses = check_frame_poses(poses, V, "frames")
        focal, center = check_intrinsics(focal, center, False)
        depth_range = check_range(depth_range)
        max_bytes = check_bytes(max_bytes)
        per_call = mesh_raster.frames_per_call(W, H, self.Nf, max_bytes)
        self._ready()
        N.require_gpu(rgb, "rgb", "the texture bake")
        if mesh_depth is not None:
            N.require_gpu(mesh_depth, "mesh_depth", "the texture bake")
        dev = self.device
        if rgb.device != dev or (mesh_depth is not None and mesh_depth.device != dev):
            raise ValueError(f"rgb and mesh_depth must live on the mesh's device {dev}")
        poses = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
        fo, ce = dev_f32(focal, 1, dev), dev_f32(center, 2, dev)
        mesh = {"vertices": self._v, "faces": self._f, "rgb8": None}
        a = self._args()
        a.focal, a.center, a.H, a.W = fo.data_ptr(), ce.data_ptr(), H, W
        for i0 in range(0, V, per_call):
            i1 = min(V, i0 + per_call)
            if mesh_depth is None:
                dm = mesh_raster.rasterize(mesh, poses[i0:i1], W, H, fo, ce, depth_range=depth_range,
                                           cull=None if self.two_sided else "back", max_bytes=max_bytes)["depth"]
            else:
                dm = N.conform(mesh_depth[i0:i1])
            rgb8 = rgb8_frames(rgb[i0:i1], dm)
            if self.Nf:
                a.frames, a.mesh_depth, a.cam2world, a.V = rgb8.data_ptr(), dm.data_ptr(), poses[i0:].data_ptr(), i1 - i0
                N.launch("lrf_mesh_texture_bake", dev, C.byref(a), self.state.data_ptr(), guard=True)
        self.frames += V
        return self

    def finish(self, fill=(0, 0, 0)):
        """The state resolved -> {"atlas": [Ht,Wt,3] uint8, "mask": [Ht,Wt] uint8 (1 where a frame saw the texel), "uv":
        [Nf,3,2] fp32 (face_uv's, on the device), "info": Python ints under INFO_KEYS, "patch", "cols"}.  A texel no frame saw takes
        its face's vertex colours under its barycentric weights when the mesh has rgb8, else fill; a texel without a face takes
        fill.  The state is left as it is: more frames may follow.  One read-back: info."""
        fill = _check_fill(fill)
        self._ready()
        dev = self.device
        atlas = torch.empty(self.Ht, self.Wt, 3, dtype=torch.uint8, device=dev)
        mask = torch.empty(self.Ht, self.Wt, dtype=torch.uint8, device=dev)
        info = torch.zeros(8, dtype=torch.int64, device=dev)
        if self.Nf:
            N.launch("lrf_mesh_texture_resolve", dev, C.byref(self._args()), self.state.data_ptr(), (C.c_uint8 * 3)(*fill),
                     atlas.data_ptr(), mask.data_ptr(), info.data_ptr(), guard=True)
        words = [int(x) for x in info.tolist()]                     # the read-back
        return {"atlas": atlas, "mask": mask, "uv": face_uv(self.Nf, self.patch, self.cols).to(dev),
                "info": dict(zip(INFO_KEYS, words)), "patch": self.patch, "cols": self.cols}


_BAKE_KEYS = ("patch", "cols", "blend", "vis_tol", "min_cos", "two_sided")
_TEXTURE_KEYS = _BAKE_KEYS + ("depth_range", "frames_per_call", "fill")


def scene_texture(local_tensorfs, mesh, W, H, poses=None, max_bytes=4 << 30, **options):
    """A texture for a mesh of the scene it came from: the scene's frames rendered by novel_views.render_poses frames_per_call
    (default 8) at a time -- the SceneFrames / PosePlan path of mesh_raster.scene_mesh_agreement --, the mesh rasterised at the
    same poses with the scene's focal(W) and center(W, H), the encoded frames baked, and both maps dropped: nothing is kept per
    frame.  poses=None takes the scene's own get_cam2world(), each frame through itself.  options: TextureBaker's patch, cols,
    blend, vis_tol, min_cos and two_sided, add's depth_range, finish's fill, frames_per_call, and render_poses' test_frames,
    frame_indices, floater_thresh, chunk.  A batch whose rasterisation workspace exceeds max_bytes raises ValueError before
    anything is rendered.  Pinhole scenes only.  Returns finish()'s dict with "frames": the number of poses."""
    lt = local_tensorfs
    frames = SceneFrames("scene_texture", lt, W, H, poses, "expected", None, options, _TEXTURE_KEYS, False)
    W, H, own = frames.W, frames.H, frames.own
    v, f, c, Nv, Nf = check_mesh(mesh)
    atlas_layout(Nf, own.get("patch", 8), own.get("cols"))
    if lt.fov == 360:
        raise ValueError("scene_texture: the bake needs a pinhole camera: there is no reprojection at 360 degrees")
    W, H = check_size(W, H)
    _check_options(own.get("blend", "mean"), own.get("vis_tol", 0.02), own.get("min_cos", 0.2), own.get("two_sided", False))
    depth_range = own.get("depth_range", (0.0, math.inf))
    check_range(depth_range)
    fill = _check_fill(own.get("fill", (0, 0, 0)))
    frames.check_per_call("bake")
    max_bytes = check_bytes(max_bytes)
    mesh_raster.frames_per_call(W, H, Nf, max_bytes)                # a single frame must fit; add splits a batch further
    frames.on_device()
    baker = TextureBaker(mesh, **{k: own[k] for k in _BAKE_KEYS if k in own})
    for poses, out, _ in frames.batches():                          # only rgb8 is taken
        baker.add(out["rgb8"], poses, frames.focal, frames.center, depth_range=depth_range, max_bytes=max_bytes)
    out = baker.finish(fill)
    out["frames"] = frames.n
    return out


def sample_texture(raster_out, tex):
    """The atlas looked up at the hits of mesh_raster.rasterize(..., weights=True): raster_out's face [V,H,W] and weights
    [V,H,W,3], tex as finish() returns it -> rgb8 [V,H,W,3] uint8, 0 where no face was hit.  Each pixel takes its nearest texel:
    (a, b) = rint((w_1, w_2) (patch - 3)) inside its face's half.  Plain torch indexing for previews and round-trip tests: not a
    hot path, and no bit-exactness claim."""
    face, wts, atlas = raster_out["face"], raster_out.get("weights"), tex["atlas"]
    if wts is None:
        raise ValueError("sample_texture needs rasterize(..., weights=True)")
    P, cols = int(tex["patch"]), int(tex["cols"])
    K = P - 3
    hit = face >= 0
    f = face.clamp(min=0).long()
    a = torch.round(wts[..., 1] * K).long().clamp(0, P - 1)
    b = torch.round(wts[..., 2] * K).long().clamp(0, P - 1)
    odd = (f % 2) == 1
    a, b = torch.where(odd, P - 1 - a, a), torch.where(odd, P - 1 - b, b)
    c = f // 2
    x, y = (c % cols) * P + a, (c // cols) * P + b
    out = torch.zeros(*face.shape, 3, dtype=torch.uint8, device=atlas.device)
    if atlas.numel():
        y, x = y.clamp(max=atlas.shape[0] - 1), x.clamp(max=atlas.shape[1] - 1)
        out = torch.where(hit[..., None], atlas[y, x], out)
    return out


def _png(rgb):
    """uint8 [H,W,3] -> the bytes of an 8-bit RGB PNG (filter 0 on every row, one IDAT)."""
    H, W = int(rgb.shape[0]), int(rgb.shape[1])

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    rows = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(rgb, np.uint8).reshape(H, 3 * W)], 1)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def write_obj(path, mesh, tex):
    """The textured mesh as Wavefront OBJ: path (v, vt, f lines), beside it <stem>.mtl (one material, map_Kd) and <stem>.png (the
    atlas, written with zlib alone).  One vt per face corner, vt 3 f + k + 1 for corner k of face f, and f a/ta b/tb c/tc with
    1-based indices.  The mesh must hold at least one face (a PNG cannot be empty)."""
    v, f, _, Nv, Nf = check_mesh(mesh)
    atlas, uv = tex["atlas"], tex["uv"]
    if Nf < 1 or atlas.numel() == 0:
        raise ValueError("write_obj: the mesh holds no face")
    if tuple(uv.shape) != (Nf, 3, 2):
        raise ValueError(f"uv must be {(Nf, 3, 2)} to go with the mesh, got {tuple(uv.shape)}")
    v, f = v.detach().cpu().numpy(), f.detach().cpu().numpy().astype(np.int64)
    uv, atlas = uv.detach().cpu().numpy().astype(np.float64).reshape(-1, 2), atlas.detach().cpu().numpy()
    path = os.fspath(path)
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    with open(stem + ".png", "wb") as out:
        out.write(_png(atlas))
    with open(stem + ".mtl", "w") as out:
        out.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += [f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}" for p in v]
    lines += [f"vt {float(t[0])!r} {float(t[1])!r}" for t in uv]
    lines += [f"f {a + 1}/{3 * k + 1} {b + 1}/{3 * k + 2} {c + 1}/{3 * k + 3}" for k, (a, b, c) in enumerate(f.tolist())]
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")
