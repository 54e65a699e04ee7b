"""Point clouds on the GPU: a neighbour index over a cloud -- the point-cloud counterpart of mesh_distance.MeshIndex -- and what
follows from it: the nearest point, the k nearest, the points within a radius, a cloud's own spacing, outlier removal, a voxel
grid, and the cloud-to-cloud figures of the reconstruction benchmarks, whose references are laser scans
(csrc/lrf_cloud.inl through lrf_cloud_index_*, lrf_cloud_closest, lrf_cloud_knn, lrf_cloud_radius_count, lrf_cloud_normals and
lrf_cloud_voxel*; the summary is mesh_distance's lrf_distance_summary).

  CloudIndex(points, cell=None)                    a uniform grid over the points, built once
  CloudIndex.closest(points, max_distance)         distance, index and the nearest point per query point
  CloudIndex.knn(points, k, max_distance)          the k nearest, ascending, k <= 8
  CloudIndex.radius_count(points, radius)          the cloud's points within radius of each query point
  CloudIndex.normals(points, radius, ...)          the cloud's normal, eigenvalues and neighbour count around each query point
  estimate_normals(points_or_index, radius, ...)   a cloud's own normals and surface variation: what a bare scan lacks
  voxel_downsample(points, cell, origin, rgb8)     one point per occupied cell: mean position, mean colour, count
  nearest_spacing(points_or_index)                 mean and exact median nearest-neighbour distance: the unit of every threshold
  remove_outliers(points, radius, min_neighbours)  the points with enough neighbours, in input order
  cloud_to_cloud(points, cloud_or_index, ...)      closest + distance_summary: cloud_to_mesh's twin
  cloud_distance(a, b, thresholds, voxel=...)      both directions: Chamfer, Hausdorff, precision / recall / F-score

The benchmarks' protocol: voxel_downsample both clouds (cloud_distance's voxel), align them (alignment.icp takes a CloudIndex
as its target: metric="point", or metric="plane" with estimate_normals' normals as target_normals), nearest-neighbour distances in both directions, precision, recall and F-score at a threshold.
A cloud is [M,3] fp32 on the device.  Exact minima with an index tie-break, integer counts and sums: the same bytes and the same
integers on every run, whatever the cell.  Every function checks its arguments on the host before its first launch.  CPU
tensors raise NativeError: there is no torch fallback.
"""
import ctypes as C
import math

import torch

from . import _native as N
from . import diagnostics
from ._native import NativeError  # noqa: F401
from ._checks import INT32 as _INT32
from ._checks import (check_bytes, check_choice, check_flag, check_int, check_max_distance, check_origin, check_points, check_positive,
                      check_thresholds, check_unit, chunks, points_on_device)
from .mesh_distance import cell_box, closest_query, decode_bounds, distance_summary, finite_rows, grid_dims, near_summary, two_sided

MAX_K = N.LRF_CLOUD_MAX_K
NORMAL_LATTICE = 1 << 15                       # lrf_cloud_normals: a neighbour's offset is at most this many lattice steps


def default_point_cell(lo, hi, used, max_bytes=1 << 30):
    """The cell edge CloudIndex takes for cell=None, a function of the box (lo, hi: three floats each), the number of used
    points and max_bytes alone: the longest box edge times 2 / sqrt(used) -- a surface cloud then holds about four points per
    occupied cell -- doubled until the grid has fewer than 2^31 cells and its start and end words (8 bytes a cell) take at most
    half of max_bytes; 1.0 for a box without extent."""
    longest = max(h - l for l, h in zip(lo, hi))
    if not longest > 0 or used < 1:
        return 1.0
    cell = longest * 2.0 / math.sqrt(used)
    while True:
        cells = math.prod(grid_dims(lo, hi, cell))
        if cells <= _INT32 and (8 * cells <= max_bytes // 2 or cells == 1):
            return cell
        cell *= 2.0


def _check_radius(radius):
    try:
        ok = not isinstance(radius, bool) and math.isfinite(float(radius)) and float(radius) >= 0
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"radius must be a finite number >= 0, got {radius!r}")
    return float(radius)


def normal_lattice(radius):
    """The lattice step of lrf_cloud_normals for a radius (finite, > 0): the smallest power of two h with radius / h <= 2^15.
    ValueError for a radius so small that h is no longer a float64 (below 2^-1058)."""
    m, e = math.frexp(radius)                                       # radius = m 2^e, 0.5 <= m < 1
    h = math.ldexp(1.0, e - 16 if m == 0.5 else e - 15)
    if not h > 0:
        raise ValueError(f"radius must be at least 2^-1058, got {radius!r}")
    return h


def _check_viewpoint(viewpoint, n):
    """None, three finite values or an [n,3] fp32 tensor -> None, a tuple of floats or the tensor."""
    if viewpoint is None:
        return None
    if torch.is_tensor(viewpoint) and viewpoint.dim() == 2:
        if viewpoint.dtype is not torch.float32 or tuple(viewpoint.shape) != (n, 3):
            raise ValueError(f"viewpoint must be None, 3 finite values or {(n, 3)} float32, got {viewpoint.dtype} {tuple(viewpoint.shape)}")
        return viewpoint
    try:
        return check_origin(viewpoint)
    except ValueError:
        raise ValueError(f"viewpoint must be None, 3 finite values or {(n, 3)} float32, got {viewpoint!r}") from None


def _check_colours(name, t, n, dtype, what):
    if t is None:
        return
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor or None")
    if t.dtype is not dtype or tuple(t.shape) != (n, 3):
        raise ValueError(f"{name} must be {(n, 3)} {what} or None, got {t.dtype} {tuple(t.shape)}")


class CloudIndex:
    """A uniform grid over the points of a cloud ([M,3] fp32 on the device), built once and held (csrc/lrf_cloud.inl states
    every rule).  A point with a coordinate that is not finite is skipped and counted, and no query returns it; duplicates stay.
    cell=None takes default_point_cell(box, used points, max_bytes).  One read-back: the bounds pass (the box of the used points
    and the two counts), which fixes the number of records.  ValueError, naming the cell box and asking for a larger cell, for a
    cell box of 2^31 cells or more or an index of more than max_bytes.
    .info: cell, box (lo, hi), dims, points (used) and nonfinite_points as Python values; .nbytes: the index's own device memory
    (the grid words and one 16-byte record -- x, y, z, index -- per used point, in cell order); .counts: (M,).  The index holds
    the cloud's tensor, not a copy: a cloud changed in place needs a new index.  No result depends on the cell."""

    def __init__(self, points, cell=None, max_bytes=1 << 30):
        M = check_points(points)
        if cell is not None:
            check_positive("cell", cell)
        max_bytes = check_bytes(max_bytes)
        if M > _INT32:
            raise ValueError(f"points holds {M} rows; a cloud index takes M < 2^31")
        pts = points_on_device(points, "points", "the cloud index")
        dev = pts.device
        self.points, self.device, self.counts = pts, dev, (M,)
        self._grid = self._records = self._args = None
        self.info = {"cell": None if cell is None else float(cell), "box": None, "dims": (0, 0, 0), "points": 0, "nonfinite_points": 0}
        if M == 0:
            return
        out = torch.empty(8, dtype=torch.int64, device=dev)
        N.launch("lrf_cloud_index_bounds", dev, pts.data_ptr(), M, out.data_ptr(), guard=True)
        host = out.cpu()                                            # the read-back
        counts, lo, hi = decode_bounds(host)
        used = int(counts[1])
        self.info.update(points=used, nonfinite_points=int(counts[0]))
        if used == 0:
            return
        cell = default_point_cell(lo, hi, used, max_bytes) if cell is None else float(cell)
        dims, cells, box = cell_box(lo, hi, cell)
        need = int(N.lib().lrf_cloud_index_workspace_bytes(cells))
        if need == 0:
            raise NativeError(f"lrf_cloud_index: refused shape {(cells,)}")
        if need + 16 * used > max_bytes:
            raise ValueError(f"{box} takes an index of {need + 16 * used} bytes; max_bytes is {max_bytes}: a larger cell is needed")
        grid = torch.empty(need, dtype=torch.uint8, device=dev)
        records = torch.empty(used, 4, dtype=torch.float32, device=dev)
        a = N.LrfCloudIndex()
        a.points, a.grid, a.records, a.M, a.entries, a.cell = pts.data_ptr(), grid.data_ptr(), records.data_ptr(), M, used, cell
        for k in range(3):
            a.lo[k], a.dims[k] = lo[k], dims[k]
        N.launch("lrf_cloud_index_build", dev, C.byref(a), guard=True)
        self._grid, self._records, self._args = grid, records, a
        self.info.update(cell=cell, box=(lo, hi), dims=dims)

    @property
    def nbytes(self):
        return 0 if self._grid is None else self._grid.numel() + 16 * self._records.shape[0]

    def _queries(self, points, exclude_self):
        n = check_points(points)
        exclude_self = check_flag("exclude_self", exclude_self)
        if exclude_self and n != self.counts[0]:
            raise ValueError(f"exclude_self pairs query i with cloud point i: {n} queries for a cloud of {self.counts[0]} points")
        return n, exclude_self

    def _on_device(self, t, name="points", verb="live"):
        return points_on_device(t, name, "the cloud queries", self.device, f"{name} {verb} on {t.device}, the index on {self.device}")

    def closest(self, points, max_distance=math.inf, closest=False):
        """points [N,3] fp32 on the index's device -> {"distance": [N] fp32, "index": [N] int32[, "closest": [N,3] fp32]} on the
        device, no read-back.  distance is the distance to the nearest used point of the cloud, index that point's row (the
        smallest among equally near points) and closest its own coordinates.  Without a point within max_distance (or without
        any): +inf, -1, NaN.  For a query with a coordinate that is not finite: NaN, -1, NaN.  The result is a function of the
        cloud, the query and max_distance alone: it does not depend on cell, on how the queries are batched or on the stream.
        A query at distance D walks about (2 D / cell)^3 cells, empty or not: give clouds with far outliers a max_distance."""
        return closest_query("lrf_cloud_closest", "index", "the cloud queries", self.device, None if self._grid is None else self._args,
                             points, max_distance, closest)

    def knn(self, points, k, max_distance=math.inf, exclude_self=False):
        """The k nearest used points of the cloud per query point, k in 1..8: {"distance": [N,k] fp32, "index": [N,k] int32},
        ascending in (distance, index); slots without a neighbour within max_distance hold +inf, -1, a query that is not finite
        NaN, -1.  exclude_self=True needs N == M and skips cloud point i for query i; a duplicate of it elsewhere still counts,
        at distance 0.  The walk stops on the k-th best: a query whose k-th neighbour lies at distance D walks about
        (2 D / cell)^3 cells, empty or not, so give clouds with far outliers a max_distance.  No read-back."""
        n, exclude_self = self._queries(points, exclude_self)
        k = check_int("k", k, 1, MAX_K)
        max_distance = check_max_distance(max_distance)
        pts, dev = self._on_device(points), self.device
        out = {"distance": torch.empty(n, k, dtype=torch.float32, device=dev), "index": torch.empty(n, k, dtype=torch.int32, device=dev)}
        if self._grid is None:
            out["distance"].copy_(torch.where(finite_rows(pts)[:, None], math.inf, math.nan).expand(n, k))
            out["index"].fill_(-1)
            return out
        for i0, m in chunks(n):
            N.launch("lrf_cloud_knn", dev, C.byref(self._args), pts[i0:].data_ptr(), m, k, max_distance, i0 if exclude_self else -1,
                     out["distance"][i0:].data_ptr(), out["index"][i0:].data_ptr(), guard=True)
        return out

    def radius_count(self, points, radius, exclude_self=False):
        """int32 [N] on the device: the used points of the cloud within radius of each query point, the boundary included
        (squared distance <= radius^2 in fp64); -1 for a query that is not finite.  radius is finite and >= 0; exclude_self as in
        knn.  A query walks about (2 radius / cell)^3 cells, empty or not.  No read-back."""
        n, exclude_self = self._queries(points, exclude_self)
        radius = _check_radius(radius)
        pts, dev = self._on_device(points), self.device
        out = torch.empty(n, dtype=torch.int32, device=dev)
        if self._grid is None:
            out.copy_(torch.where(finite_rows(pts), 0, -1))
            return out
        for i0, m in chunks(n):
            N.launch("lrf_cloud_radius_count", dev, C.byref(self._args), pts[i0:].data_ptr(), m, radius, i0 if exclude_self else -1,
                     out[i0:].data_ptr(), guard=True)
        return out

    def normals(self, points, radius, min_neighbours=6, viewpoint=None):
        """points [N,3] fp32 on the index's device -> {"normals": [N,3] fp32, "eigenvalues": [N,3] fp32, "count": int32 [N]} on the
        device, no read-back: per query point the normal of the cloud around it by principal component analysis.  The
        neighbourhood is radius_count's -- the used points within radius, the boundary and a point equal to the query included;
        its covariance is formed from integer sums on a lattice of 2^16 steps across the radius, so the result does not depend on
        cell, on the order of the cloud's points, on how the queries are batched or on the stream; its eigenvectors come from a
        fixed number of Jacobi sweeps in fp64 (csrc/lrf_cloud.inl item 9).  normals: the unit eigenvector to the smallest
        eigenvalue; eigenvalues: all three, ascending, in squared world units; count: the neighbours.  viewpoint: three finite
        values, or [N,3] fp32 on the index's device, one per query: each normal is turned towards its viewpoint; with None, or
        where the viewpoint lies exactly in the normal's plane, the component of largest magnitude is made positive.
        Fewer than min_neighbours (>= 3) neighbours, or neighbours that all coincide: normal (0, 0, 0) and the true count.  A
        query that is not finite: NaN, NaN, -1.  radius is finite and > 0, best given in units of nearest_spacing."""
        return self._normals(points, check_points(points), radius, min_neighbours, viewpoint)

    def _normals(self, points, n, radius, min_neighbours, viewpoint):
        """normals() for checked points, or with points=None for the cloud's own n = M points walked in record order."""
        radius = check_positive("radius", radius)
        h = normal_lattice(radius)
        min_neighbours = check_int("min_neighbours", min_neighbours, 3, _INT32, "an integer in [3, 2^31)")
        viewpoint = _check_viewpoint(viewpoint, n)
        dev = self.device
        pts = self._on_device(self.points if points is None else points)
        view, stride = None, 0
        if torch.is_tensor(viewpoint):
            view, stride = self._on_device(viewpoint, "viewpoint", "lives"), 3
        elif viewpoint is not None:
            view = torch.tensor(viewpoint, dtype=torch.float32).to(dev)
        out = {"normals": torch.empty(n, 3, dtype=torch.float32, device=dev), "eigenvalues": torch.empty(n, 3, dtype=torch.float32, device=dev),
               "count": torch.empty(n, dtype=torch.int32, device=dev)}
        if self._grid is None:                                      # no used point: no neighbour
            finite = finite_rows(pts)
            out["normals"].copy_(torch.where(finite, 0.0, math.nan)[:, None].expand(n, 3))
            out["eigenvalues"].copy_(out["normals"])
            out["count"].copy_(torch.where(finite, 0, -1))
            return out
        if points is None:
            N.launch("lrf_cloud_normals", dev, C.byref(self._args), None, n, radius, h, min_neighbours, None if view is None else view.data_ptr(),
                     stride, out["normals"].data_ptr(), out["eigenvalues"].data_ptr(), out["count"].data_ptr(), guard=True)
            return out
        for i0, m in chunks(n):
            N.launch("lrf_cloud_normals", dev, C.byref(self._args), pts[i0:].data_ptr(), m, radius, h, min_neighbours,
                     None if view is None else (view[i0:] if stride else view).data_ptr(), stride, out["normals"][i0:].data_ptr(),
                     out["eigenvalues"][i0:].data_ptr(), out["count"][i0:].data_ptr(), guard=True)
        return out


def voxel_downsample(points, cell, origin=(0.0, 0.0, 0.0), rgb8=None, max_bytes=1 << 30):
    """The cloud ([M,3] fp32, rgb8 [M,3] uint8 or None) reduced to one point per occupied cell of the grid of edge `cell`
    anchored at `origin`: the mean position and the rounded mean colour of the cell's points, by mesh.simplify's integer
    arithmetic (csrc/lrf_mesh_simplify.inl items 1-4).  Every occupied cell is emitted, in cell order (x fastest) -- simplify
    emits only what a face holds, so a mesh without faces gives it nothing.  A point that is not finite or lies 2^30 cells or
    more from origin is skipped and counted.  Returns {"points": [C,3], "rgb8": [C,3] (with rgb8), "count": int32 [C] (points per
    cluster), "cluster_of": int32 [M] (-1 for a bad point), "counts": (C,), "info": cell, origin, box (lo, dims), points (used),
    bad_points}.  The bytes of points, rgb8 and count do not depend on the order of the input.  Two read-backs: the bounds pass
    (a cell box of 2^31 cells or more, or a workspace above max_bytes, raises ValueError before anything is summed), then the
    number of clusters; the outputs are allocated at M rows and sliced."""
    M = check_points(points)
    cell = check_positive("cell", cell)
    origin = check_origin(origin)
    _check_colours("rgb8", rgb8, M, torch.uint8, "uint8")
    max_bytes = check_bytes(max_bytes)
    if M > _INT32:
        raise ValueError(f"points holds {M} rows; a voxel grid takes M < 2^31")
    pts = points_on_device(points, "points", "the voxel grid")
    dev = pts.device
    col = None if rgb8 is None else points_on_device(rgb8, "rgb8", "the voxel grid", dev, "points and rgb8 must live on the same device")
    info = {"cell": cell, "origin": origin, "box": {"lo": (0, 0, 0), "dims": (0, 0, 0)}, "points": 0, "bad_points": 0}
    out = {"points": pts[:0], "count": torch.empty(0, dtype=torch.int32, device=dev),
           "cluster_of": torch.full((M,), -1, dtype=torch.int32, device=dev), "counts": (0,), "info": info}
    if col is not None:
        out["rgb8"] = col[:0]
    if M == 0:
        return out
    o3 = (C.c_double * 3)(*origin)
    words = torch.empty(8, dtype=torch.int64, device=dev)
    N.launch("lrf_cloud_voxel_bounds", dev, pts.data_ptr(), M, o3, cell, words.data_ptr(), guard=True)
    host = words.cpu()                                              # read-back one
    bad, used = (int(x) for x in host[:2].tolist())
    info.update(points=used, bad_points=bad)
    if used == 0:
        return out
    ends = host[4:7].view(torch.int32).tolist()
    lo, dims = tuple(ends[:3]), tuple(h - l + 1 for l, h in zip(ends[:3], ends[3:6]))
    cells = dims[0] * dims[1] * dims[2]
    box = f"the cell box {dims[0]} x {dims[1]} x {dims[2]} from {lo}"
    if cells > _INT32:
        raise ValueError(f"{box} holds {cells} cells; a voxel grid takes fewer than 2^31: a larger cell is needed")
    need = int(N.lib().lrf_cloud_voxel_workspace_bytes(M, cells))
    if need == 0:
        raise NativeError(f"lrf_cloud_voxel: refused shape {(M, cells)}")
    if need > max_bytes:
        raise ValueError(f"{box} takes a workspace of {need} bytes; max_bytes is {max_bytes}: a larger cell is needed")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    po, no = torch.empty_like(pts), torch.empty(M, dtype=torch.int32, device=dev)
    co = None if col is None else torch.empty_like(col)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    a = N.LrfCloudVoxel()
    a.points, a.rgb8, a.M, a.cell = pts.data_ptr(), None if col is None else col.data_ptr(), M, cell
    for k in range(3):
        a.origin[k], a.lo[k], a.dims[k] = origin[k], lo[k], dims[k]
    N.launch("lrf_cloud_voxel", dev, C.byref(a), po.data_ptr(), None if co is None else co.data_ptr(), no.data_ptr(),
             out["cluster_of"].data_ptr(), counts.data_ptr(), ws.data_ptr(), guard=True)
    n = int(counts[2].item())                                       # read-back two (it also orders ws's release)
    info.update(box={"lo": lo, "dims": dims})
    out.update(points=po[:n], count=no[:n], counts=(n,))
    if co is not None:
        out["rgb8"] = co[:n]
    return out


def as_cloud_index(cloud_or_index, max_bytes, name="cloud_or_index"):
    """The target as a CloudIndex, after the caller's other checks: built here (its checks, the device, launches) unless it is one."""
    if isinstance(cloud_or_index, CloudIndex):
        return cloud_or_index
    if not torch.is_tensor(cloud_or_index):
        raise TypeError(f"{name} must be a [M, 3] float32 tensor or a CloudIndex")
    return CloudIndex(cloud_or_index, max_bytes=max_bytes)


def nearest_spacing(points_or_index, max_bytes=1 << 30):
    """A cloud's own spacing: the distance of every used point to its nearest other point (knn with k = 1 and exclude_self on
    the cloud itself; a duplicate is a neighbour at distance 0).  Returns {"mean": distance_summary's mean over the finite
    distances in units of the median, "median": diagnostics.median of them (exact, the lower median), "count": the finite
    distances}; NaN, NaN, 0 for a cloud with fewer than two used points.  Every threshold of this module is best chosen in
    these units."""
    check_bytes(max_bytes)
    index = as_cloud_index(points_or_index, max_bytes, "points_or_index")
    d = index.knn(index.points, 1, exclude_self=True)["distance"].reshape(-1)
    d = d[torch.isfinite(d)]
    if d.numel() == 0:
        return {"mean": math.nan, "median": math.nan, "count": 0}
    median = float(diagnostics.median(d))
    unit = median if math.isfinite(median) and median > 0 else 1.0
    s = distance_summary(d, (), check_unit(unit))
    return {"mean": s["mean"], "median": median, "count": s["finite"]}


NORMAL_ORDERS = ("input", "records")


def estimate_normals(points_or_index, radius, min_neighbours=6, viewpoint=None, max_bytes=1 << 30, order="records"):
    """A cloud's own normals: CloudIndex.normals of the cloud ([M,3] fp32 on the device, or a CloudIndex built from it, which is
    not built again) queried at its own points -> {"normals": [M,3], "eigenvalues": [M,3], "count": int32 [M], "variation": [M]}
    on the device, no read-back beyond the index's own.  variation is the surface variation l0 / (l0 + l1 + l2) of the ascending
    eigenvalues (torch, fp32): 0 on a plane, 1 / 3 where the neighbourhood has no direction, and 0 where the sum is 0.
    radius is best given in units of nearest_spacing: 3 to 4 medians is what the tests use -- at 3 spacings of a unit sphere of
    4099 points no normal is off by more than a degree.  viewpoint: None, three values, or [M,3] fp32 (the scanner's position per
    point); without one the signs follow the largest component and are not consistent across a surface.  A point with fewer
    than min_neighbours neighbours (itself included) has the normal (0, 0, 0), which alignment.icp counts as degenerate; a point
    that is not finite NaN and count -1.  These are the normals that write_ply(normals=...), remove_outliers(normals=...) and
    alignment.icp(target_normals=...) take.  order: "records", the default, walks the cloud in the order of the index's records,
    where the lanes of a wave share cells and cache lines; "input" queries the points as they lie in memory.  The bytes are the
    same; on a shuffled cloud of a million points "records" measured four times as fast (docs/CLOUD_FIGURES.md)."""
    if not isinstance(points_or_index, CloudIndex):
        if not torch.is_tensor(points_or_index):
            raise TypeError("points_or_index must be a [M, 3] float32 tensor or a CloudIndex")
        check_points(points_or_index)
    m = points_or_index.counts[0] if isinstance(points_or_index, CloudIndex) else int(points_or_index.shape[0])
    normal_lattice(check_positive("radius", radius))
    check_int("min_neighbours", min_neighbours, 3, _INT32, "an integer in [3, 2^31)")
    _check_viewpoint(viewpoint, m)
    check_bytes(max_bytes)
    check_choice("order", order, NORMAL_ORDERS)
    index = as_cloud_index(points_or_index, max_bytes, "points_or_index")
    out = index._normals(None if order == "records" else index.points, m, radius, min_neighbours, viewpoint)
    e = out["eigenvalues"]
    total = e.sum(1)
    out["variation"] = torch.where(total == 0, torch.zeros_like(total), e[:, 0] / total)
    return out


def remove_outliers(points, radius, min_neighbours, rgb8=None, normals=None, index=None):
    """Floater removal: keeps point i iff at least min_neighbours other points of the cloud lie within radius of it
    (radius_count with exclude_self; the boundary counts).  A point that is not finite goes.  Survivors stay in input order.
    index: a CloudIndex of these very points, which is then not built again.  Returns {"points", "rgb8" and "normals" where
    given, "keep": bool [M], "counts": (kept,)}.  One read-back: the number kept."""
    M = check_points(points)
    radius = _check_radius(radius)
    min_neighbours = check_int("min_neighbours", min_neighbours, 0, _INT32, "an integer in [0, 2^31)")
    _check_colours("rgb8", rgb8, M, torch.uint8, "uint8")
    _check_colours("normals", normals, M, torch.float32, "float32")
    if index is not None:
        if not isinstance(index, CloudIndex):
            raise TypeError("index must be a CloudIndex or None")
        if index.counts != (M,):
            raise ValueError(f"index was built over {index.counts[0]} points, points holds {M}")
    pts = points_on_device(points, "points", "the outlier removal")
    rows = {name: points_on_device(t, name, "the outlier removal", pts.device, f"points and {name} must live on the same device")
            for name, t in (("rgb8", rgb8), ("normals", normals)) if t is not None}
    index = CloudIndex(pts) if index is None else index
    keep = index.radius_count(pts, radius, exclude_self=True) >= max(min_neighbours, 0)
    out = {"points": pts[keep], "keep": keep}
    out.update({name: t[keep] for name, t in rows.items()})
    out["counts"] = (int(out["points"].shape[0]),)
    return out


def cloud_to_cloud(points, cloud_or_index, thresholds=(), max_distance=math.inf, unit=None, max_bytes=1 << 30):
    """The distances of a point cloud [N,3] fp32 to another cloud (or to a CloudIndex built from it, which is not built again):
    CloudIndex.closest and distance_summary; mesh_distance.cloud_to_mesh's twin.  unit defaults to max_distance when that is
    finite and > 0, else 1.0.  Returns distance_summary's dict plus "distance" and "index" on the device.  With a
    reconstruction's cloud and a reference scan, mean is the accuracy; the other way round, the completeness."""
    check_points(points)
    taus, max_distance = check_thresholds(thresholds), check_max_distance(max_distance)
    if unit is not None:
        check_unit(unit)
    check_bytes(max_bytes)
    return near_summary(as_cloud_index(cloud_or_index, max_bytes), "index", points, taus, max_distance, unit)


def cloud_distance(a, b, thresholds=(), max_distance=math.inf, voxel=None, max_bytes=1 << 30):
    """Two clouds compared point to point: a queried against b, and b against a.  With voxel (a cell edge) both first go through
    voxel_downsample(cloud, voxel), the benchmarks' protocol, which takes the density of either cloud out of the figures.
    Returns mesh_distance.mesh_distance's dict: a_to_b and b_to_a (distance_summary's dicts, unit as in cloud_to_cloud);
    chamfer, the sum of the two means; hausdorff, the larger of the two maxima over the finite entries; per threshold precision
    (the share of a's finite-or-beyond points within it of b), recall (b's within it of a) and fscore = 2 p r / (p + r), formed
    on the host from the integer counts, NaN where undefined; thresholds; and samples = (points of a, points of b) that were
    queried.  With a the reconstruction and b the reference scan these are the figures of the reconstruction benchmarks.  The
    same integers on every run, and with voxel for every order of the points of either cloud."""
    check_points(a)
    check_points(b)
    taus, max_distance = check_thresholds(thresholds), check_max_distance(max_distance)
    if voxel is not None:
        check_positive("voxel", voxel)
    check_bytes(max_bytes)
    if voxel is not None:
        a, b = (voxel_downsample(x, voxel, max_bytes=max_bytes)["points"] for x in (a, b))

    def side(src, dst):
        r = cloud_to_cloud(src, dst, taus, max_distance, None, max_bytes)
        del r["distance"], r["index"]
        return r
    return two_sided(side(a, b), side(b, a), taus)
