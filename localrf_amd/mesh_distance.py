"""Point-to-mesh distance on the GPU: the closest point of a triangle mesh for a batch of points, and what follows from it --
surface error, Chamfer distance, Hausdorff distance and F-score of two meshes or of a cloud against a mesh
(csrc/lrf_mesh_distance.inl through lrf_mesh_index_*, lrf_mesh_closest, lrf_mesh_sample_* and lrf_distance_summary).  It answers
in 3-D, whatever the cameras, what mesh_raster.depth_agreement answers in view space: how far simplify or smooth moved a surface,
how a scene_point_cloud and a scene_mesh agree, how a reconstruction scores against a reference.

  MeshIndex(mesh, cell=None)                     a uniform grid over the faces, built once
  MeshIndex.closest(points, max_distance)        distance, face and closest point per query point
  sample_surface(mesh, spacing)                  about area / spacing^2 points on the surface, independent of the face order
  distance_summary(distance, thresholds, unit)   integer counts and sums of a distance tensor
  cloud_to_mesh(points, mesh_or_index, ...)      closest + distance_summary
  mesh_distance(a, b, spacing, ...)              both directions: Chamfer, Hausdorff, precision / recall / F-score
  decode_bounds, cell_box, closest_query, finite_rows, near_summary, two_sided    what cloud.CloudIndex and cloud's figures share
  check_target, as_index                         a mesh dict or a MeshIndex as the target: host checks, then the build

A module of its own rather than part of mesh.py for the reason mesh_raster.py is one: it consumes meshes, it does not make them.
A mesh is the dict of mesh.py.  Unsigned distance.  The same bytes and the same integers on every run.  Every function checks
its arguments on the host before its first launch.  CPU tensors raise NativeError: there is no torch fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._native import NativeError  # noqa: F401
from ._checks import INT32 as _INT32
from ._checks import (check_bytes, check_flag, check_int, check_max_distance, check_mesh, check_points, check_positive, check_thresholds,
                      check_unit, chunks, float_of_key, mesh_on_device, points_on_device)

DISTANCE_SCALE = 1 << 24                       # the fixed point of the two sums
DISTANCE_CLAMP = 8.0                           # a distance enters the sums as min(d / unit, this)
MAX_FACE_SAMPLES = 1 << 21                     # samples one face may take


def _check_count(max_points):
    return check_int("max_points", max_points, 0, _INT32, "an integer in [0, 2^31)")


def default_cell(lo, hi, used_faces):
    """The cell edge MeshIndex takes for cell=None, a function of the box (lo, hi: three floats each) and the number of used
    faces alone: the longest box edge times 2 sqrt(2 / used_faces) -- twice the edge of a triangle when used_faces of them tile a
    square of that edge -- doubled until the cell box holds fewer than 2^31 cells; 1.0 for a box without extent."""
    longest = max(h - l for l, h in zip(lo, hi))
    if not longest > 0 or used_faces < 1:
        return 1.0
    cell = longest * 2.0 * math.sqrt(2.0 / used_faces)
    while math.prod(grid_dims(lo, hi, cell)) > _INT32:
        cell *= 2.0
    return cell


def grid_dims(lo, hi, cell):
    """The cells per axis of the box at this cell edge: floor((hi - lo) / cell) + 1 in fp64."""
    return tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))


def decode_bounds(host):
    """The 8 int64 words a bounds pass wrote, read back -> (its four counts, lo, hi): the box as Python floats."""
    counts, keys = host[:4].tolist(), host[4:7].view(torch.int32).tolist()
    return counts, tuple(float_of_key(k) for k in keys[:3]), tuple(float_of_key(k) for k in keys[3:6])


def cell_box(lo, hi, cell):
    """-> (dims, cells, the words that name the cell box in a refusal); ValueError for a box of 2^31 cells or more."""
    dims = grid_dims(lo, hi, cell)
    cells = dims[0] * dims[1] * dims[2]
    box = f"the cell box {dims[0]} x {dims[1]} x {dims[2]} of cell {cell} over {lo} .. {hi}"
    if cells > _INT32:
        raise ValueError(f"{box} holds {cells} cells; an index takes fewer than 2^31: a larger cell is needed")
    return dims, cells, box


def finite_rows(pts):
    """bool [N] on the device: the rows of pts [N,3] without a coordinate that is not finite."""
    return torch.isfinite(pts).all(1)


def closest_query(symbol, key, feature, dev, args, points, max_distance, closest):
    """closest() of MeshIndex (lrf_mesh_closest, "face") and of cloud.CloudIndex (lrf_cloud_closest, "index"): the checks, the
    device, and one launch per chunk.  args: the index's struct, None for an index that holds nothing -- then nothing is near,
    and nothing is launched."""
    n = check_points(points)
    max_distance = check_max_distance(max_distance)
    closest = check_flag("closest", closest)
    pts = points_on_device(points, "points", feature, dev, f"points live on {points.device}, the index on {dev}")
    out = {"distance": torch.empty(n, dtype=torch.float32, device=dev), key: torch.empty(n, dtype=torch.int32, device=dev)}
    if closest:
        out["closest"] = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if args is None:
        out["distance"].copy_(torch.where(finite_rows(pts), math.inf, math.nan))
        out[key].fill_(-1)
        if closest:
            out["closest"].fill_(math.nan)
        return out
    for i0, m in chunks(n):
        N.launch(symbol, dev, C.byref(args), pts[i0:].data_ptr(), m, max_distance, out["distance"][i0:].data_ptr(), out[key][i0:].data_ptr(),
                 out["closest"][i0:].data_ptr() if closest else None, guard=True)
    return out


class MeshIndex:
    """A uniform grid over the faces of a mesh (the dict of mesh.py), built once on the mesh's device and held
    (csrc/lrf_mesh_distance.inl states every rule).  Faces with an index outside [0, Nv) -- never dereferenced -- or a corner that
    is not finite are skipped and counted; zero-area faces stay, as the segments or points they are.  cell=None takes
    default_cell(box, used_faces).  Two read-backs: the bounds pass (the box of the used faces' corners and the three counts),
    then the number of (cell, face) entries, which sizes the list.  ValueError, naming the cell box and asking for a larger cell,
    for a cell box of 2^31 cells or more, a list of 2^31 entries or more, or an index of more than max_bytes.
    .info: cell, box (lo, hi), dims, entries, bad_index_faces, nonfinite_faces, used_faces as Python values; .nbytes: the
    index's own device memory.  The index holds the mesh's tensors, not copies: a mesh changed in place needs a new index."""

    def __init__(self, mesh, cell=None, max_bytes=1 << 30):
        v, f, _, Nv, Nf = check_mesh(mesh)
        if cell is not None:
            check_positive("cell", cell)
        check_bytes(max_bytes)
        v, f, _, dev = mesh_on_device(v, f, None, "the mesh index")
        self.vertices, self.faces, self.device, self.counts = v, f, dev, (Nv, Nf)
        self._grid = self._list = None
        self.info = {"cell": None if cell is None else float(cell), "box": None, "dims": (0, 0, 0), "entries": 0, "bad_index_faces": 0,
                     "nonfinite_faces": 0, "used_faces": 0}
        if Nf == 0 or Nv == 0:
            return
        out = torch.empty(8, dtype=torch.int64, device=dev)
        N.launch("lrf_mesh_index_bounds", dev, v.data_ptr(), f.data_ptr(), Nv, Nf, out.data_ptr(), guard=True)
        host = out.cpu()                                            # read-back one
        counts, lo, hi = decode_bounds(host)
        self.info.update(bad_index_faces=int(counts[0]), nonfinite_faces=int(counts[1]), used_faces=int(counts[2]))
        if counts[2] == 0:
            return
        cell = default_cell(lo, hi, int(counts[2])) if cell is None else float(cell)
        dims, cells, box = cell_box(lo, hi, cell)
        need = int(N.lib().lrf_mesh_index_workspace_bytes(cells))
        if need == 0:
            raise NativeError(f"lrf_mesh_index: refused shape {(cells,)}")
        if need > max_bytes:
            raise ValueError(f"{box} takes a grid of {need} bytes; max_bytes is {max_bytes}: a larger cell is needed")
        grid = torch.empty(need, dtype=torch.uint8, device=dev)
        a = N.LrfMeshIndex()
        a.vertices, a.faces, a.grid, a.list = v.data_ptr(), f.data_ptr(), grid.data_ptr(), None
        a.Nv, a.Nf, a.entries, a.cell = Nv, Nf, 0, cell
        for k in range(3):
            a.lo[k], a.dims[k] = lo[k], dims[k]
        total = torch.empty(1, dtype=torch.int64, device=dev)
        N.launch("lrf_mesh_index_build", dev, C.byref(a), total.data_ptr(), guard=True)
        entries = int(total.item())                                 # read-back two
        if entries > _INT32:
            raise ValueError(f"{box} lists {entries} (cell, face) entries; an index takes fewer than 2^31: a larger cell is needed")
        if need + 4 * entries > max_bytes:
            raise ValueError(f"{box} takes an index of {need + 4 * entries} bytes; max_bytes is {max_bytes}: a larger cell is needed")
        lst = torch.empty(max(entries, 1), dtype=torch.int32, device=dev)
        a.list, a.entries = lst.data_ptr(), entries
        N.launch("lrf_mesh_index_build", dev, C.byref(a), None, guard=True)
        self._grid, self._list, self._args = grid, lst, a
        self.info.update(cell=cell, box=(lo, hi), dims=dims, entries=entries)

    @property
    def nbytes(self):
        return 0 if self._grid is None else self._grid.numel() + 4 * self._list.numel()

    def closest(self, points, max_distance=math.inf, closest=False):
        """points [N,3] fp32 on the index's device -> {"distance": [N] fp32, "face": [N] int32[, "closest": [N,3] fp32]} on the
        device, no read-back.  distance is the unsigned distance to the nearest used face, face its index (the smallest among
        equally near faces) and closest the nearest point of that face.  Without a face within max_distance (or without any):
        +inf, -1, NaN.  For a point with a coordinate that is not finite: NaN, -1, NaN.  The result is a function of the mesh,
        the point and max_distance alone: it does not depend on cell, on how the points are batched or on the stream.  A point at
        distance D walks about (2 D / cell)^3 cells, empty or not: give clouds with far outliers a max_distance."""
        return closest_query("lrf_mesh_closest", "face", "the mesh distance", self.device, None if self._grid is None else self._args,
                             points, max_distance, closest)


def sample_surface(mesh, spacing, max_points=1 << 26):
    """About area / spacing^2 points on the surface of the mesh (the dict of mesh.py; csrc/lrf_mesh_distance.inl item 5): a face
    of area A takes floor(A / spacing^2 + u) samples, u a 32-bit fraction hashed from the bits of its corners, so the expected
    number is exactly A / spacing^2 and M = the total is area / spacing^2 up to a spread of about sqrt(faces / 6); the samples of
    a face follow a fixed low-discrepancy sequence seeded by the same hash.  Neither a face's index nor the corner it starts at
    enters: the set of samples does not depend on the order of the faces.  Skipped and counted as in MeshIndex: faces with a bad
    index or a corner that is not finite.  Returns {"points": [M,3] fp32, "face": [M] int32 (the face each sample lies on), in
    face order, "counts": (M,), "info": spacing, bad_index_faces, nonfinite_faces}.  One read-back, after the count; a total
    above max_points, or a single face above 2^21 samples, raises ValueError before anything is emitted."""
    v, f, _, Nv, Nf = check_mesh(mesh)
    spacing, max_points = check_positive("spacing", spacing), _check_count(max_points)
    v, f, _, dev = mesh_on_device(v, f, None, "the surface sampling")
    info = {"spacing": spacing, "bad_index_faces": 0, "nonfinite_faces": 0}
    if Nf == 0 or Nv == 0:
        return {"points": torch.empty(0, 3, dtype=torch.float32, device=dev), "face": torch.empty(0, dtype=torch.int32, device=dev),
                "counts": (0,), "info": info}
    offsets = torch.empty(Nf, dtype=torch.int32, device=dev)
    words = torch.empty(4, dtype=torch.int64, device=dev)
    N.launch("lrf_mesh_sample_count", dev, v.data_ptr(), f.data_ptr(), Nv, Nf, spacing, offsets.data_ptr(), words.data_ptr(), guard=True)
    total, bad, nonfinite, over = (int(x) for x in words.tolist())  # the read-back
    info.update(bad_index_faces=bad, nonfinite_faces=nonfinite)
    if over:
        raise ValueError(f"{over} faces take more than {MAX_FACE_SAMPLES} samples each at spacing {spacing}: a larger spacing is needed")
    if total > max_points:
        raise ValueError(f"spacing {spacing} gives {total} samples; max_points is {max_points}: a larger spacing is needed")
    pts = torch.empty(total, 3, dtype=torch.float32, device=dev)
    face = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        N.launch("lrf_mesh_sample_emit", dev, v.data_ptr(), f.data_ptr(), Nv, Nf, spacing, offsets.data_ptr(), total, pts.data_ptr(),
                 face.data_ptr(), guard=True)
    return {"points": pts, "face": face, "counts": (total,), "info": info}


def _check_distance(distance):
    if not torch.is_tensor(distance):
        raise TypeError("distance must be a torch tensor")
    if distance.dtype is not torch.float32:
        raise ValueError(f"distance must be float32, got {distance.dtype}")
    if distance.numel() > _INT32:
        raise ValueError(f"distance holds {distance.numel()} values; one summary takes fewer than 2^31")


def _summary_words(distance, taus, unit):
    """Checked arguments -> the 16 int64 words on the device; no read-back."""
    dev = distance.device
    d = distance.detach().contiguous().reshape(-1)
    words = torch.empty(16, dtype=torch.int64, device=dev)
    tau = (C.c_float * max(len(taus), 1))(*taus)
    N.launch("lrf_distance_summary", dev, d.data_ptr() if d.numel() else None, d.numel(), tau, len(taus), unit, words.data_ptr(), guard=True)
    return words


def _summary(words, taus, unit):
    finite = int(words[0])
    s1, s2 = int(words[3]), int(words[4])
    return {"finite": finite, "beyond": int(words[1]), "nan": int(words[2]),
            "within": tuple(int(words[8 + k]) for k in range(len(taus))), "sum": s1, "sum_sq": s2,
            "mean": s1 / DISTANCE_SCALE / finite * unit if finite else math.nan,
            "rms": math.sqrt(s2 / DISTANCE_SCALE / finite) * unit if finite else math.nan,
            "max": float(np.array([int(words[5])], np.uint32).view(np.float32)[0]) if finite else math.nan,
            "thresholds": tuple(taus), "unit": unit}


def distance_summary(distance, thresholds=(), unit=1.0):
    """A float32 distance tensor on the device (MeshIndex.closest's) summarised in one kernel.  Returns Python values: finite,
    beyond (infinite entries: no face within max_distance) and nan, which add up to the number of entries; within, per threshold
    (at most 8, each finite and > 0, compared in fp32) the finite entries <= it; sum, the int64 sum over the finite entries of
    rint(min(d / unit, 8) * 2^24), and sum_sq, that of rint(min(d / unit, 8)^2 * 2^24) (DISTANCE_CLAMP, DISTANCE_SCALE: 2^31
    entries cannot overflow either); mean = sum / 2^24 / finite * unit and rms = sqrt(sum_sq / 2^24 / finite) * unit, NaN
    without a finite entry; max, the largest finite entry (NaN without one); thresholds (as float32) and unit.  Choose unit so
    that distances stay below 8 units -- cloud_to_mesh takes max_distance -- or mean and rms saturate.  All integers: the same
    on every run.  One read-back.  diagnostics.quantile takes exact medians and other quantiles of the same tensor."""
    _check_distance(distance)
    taus = check_thresholds(thresholds)
    unit = check_unit(unit)
    N.require_gpu(distance, "distance", "the distance summary")
    return _summary(_summary_words(distance, taus, unit).tolist(), taus, unit)     # the read-back


def check_target(mesh_or_index, name="mesh_or_index"):
    """The host half of as_index, before the caller's other checks: a MeshIndex passes, a mesh dict goes through check_mesh."""
    if not isinstance(mesh_or_index, MeshIndex):
        if not isinstance(mesh_or_index, dict):
            raise TypeError(f"{name} must be a mesh dict or a MeshIndex")
        check_mesh(mesh_or_index)


def as_index(mesh_or_index, max_bytes):
    """The checked target as a MeshIndex, after the caller's other checks: built here (device check, launches) unless it is one."""
    return mesh_or_index if isinstance(mesh_or_index, MeshIndex) else MeshIndex(mesh_or_index, max_bytes=max_bytes)


def near_summary(index, key, points, taus, max_distance, unit):
    """What cloud_to_mesh and cloud.cloud_to_cloud share after their checks: the unit's default, index.closest and
    distance_summary's dict with "distance" and the index's `key` ("face", "index") carried along."""
    if unit is None:
        unit = max_distance if math.isfinite(max_distance) and max_distance > 0 else 1.0
    unit = check_unit(unit)
    near = index.closest(points, max_distance)
    out = _summary(_summary_words(near["distance"], taus, unit).tolist(), taus, unit)
    out.update({"distance": near["distance"], key: near[key]})
    return out


def cloud_to_mesh(points, mesh_or_index, thresholds=(), max_distance=math.inf, unit=None, max_bytes=1 << 30):
    """The distances of a point cloud [N,3] fp32 to a mesh (or to a MeshIndex built from it, which is not built again):
    MeshIndex.closest and distance_summary.  unit defaults to max_distance when that is finite and > 0, else 1.0.  Returns
    distance_summary's dict plus "distance" and "face" on the device.  With a reconstruction's cloud and a reference mesh,
    mean is the accuracy; with the reference's cloud and the reconstruction's mesh, the completeness."""
    check_target(mesh_or_index)
    check_points(points)
    taus, max_distance = check_thresholds(thresholds), check_max_distance(max_distance)
    if unit is not None:
        check_unit(unit)
    check_bytes(max_bytes)
    return near_summary(as_index(mesh_or_index, max_bytes), "face", points, taus, max_distance, unit)


def _ratio(a, b):
    return a / b if b else math.nan


def two_sided(ab, ba, taus):
    """The two one-sided summaries (distance_summary's dicts) of a compared with b -> the dict mesh_distance and
    cloud.cloud_distance return, formed on the host from the integer counts."""
    n_a, n_b = ab["finite"] + ab["beyond"], ba["finite"] + ba["beyond"]
    maxima = [s["max"] for s in (ab, ba) if s["finite"]]
    precision = tuple(_ratio(w, n_a) for w in ab["within"])
    recall = tuple(_ratio(w, n_b) for w in ba["within"])
    fscore = tuple(2 * p * r / (p + r) if p + r > 0 else math.nan for p, r in zip(precision, recall))
    return {"a_to_b": ab, "b_to_a": ba, "chamfer": ab["mean"] + ba["mean"], "hausdorff": max(maxima) if maxima else math.nan,
            "precision": precision, "recall": recall, "fscore": fscore, "thresholds": tuple(taus),
            "samples": (ab["finite"] + ab["beyond"] + ab["nan"], ba["finite"] + ba["beyond"] + ba["nan"])}


def mesh_distance(a, b, spacing, thresholds=(), max_distance=math.inf, max_bytes=1 << 30, max_points=1 << 26):
    """Two meshes compared through surface samples: sample_surface(a, spacing) queried against b, and b's samples against a.
    Returns a_to_b and b_to_a (distance_summary's dicts, unit as in cloud_to_mesh); chamfer, the sum of the two means; hausdorff,
    the larger of the two maxima over the finite entries (the sampled, one-sided-in-each-direction estimate: it approaches the
    true value from below as spacing shrinks); per threshold precision (the share of a's finite-or-beyond samples within it of
    b), recall (b's within it of a) and fscore = 2 p r / (p + r), formed on the host from the integer counts, NaN where
    undefined; and samples = (M_a, M_b).  With a the reconstruction and b the reference these are the figures of the
    reconstruction benchmarks.  The same integers on every run, and for every order of the faces of either mesh."""
    check_mesh(a)
    check_mesh(b)
    check_positive("spacing", spacing)
    taus = check_thresholds(thresholds)
    check_max_distance(max_distance)
    check_bytes(max_bytes)
    _check_count(max_points)

    def side(src, dst):
        r = cloud_to_mesh(sample_surface(src, spacing, max_points)["points"], dst, taus, max_distance, None, max_bytes)
        del r["distance"], r["face"]
        return r
    return two_sided(side(a, b), side(b, a), taus)
