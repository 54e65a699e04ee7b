"""Rendered depth fused into a TSDF volume and a triangle mesh extracted from it on the GPU (csrc/lrf_mesh.inl through
lrf_tsdf_integrate and lrf_mesh_extract; csrc/lrf_tsdf_blocks.inl through lrf_tsdf_blocks_* and lrf_mesh_extract_blocks).

  TsdfVolume(origin, voxel, dims, trunc, device)   the three volume tensors; .integrate(frames) and .extract() -> mesh
  SparseTsdfVolume(origin, voxel, blocks, trunc, device)  the same lattice stored in 8 x 8 x 8 blocks where depth reaches:
                                                   .touch(frames), .allocate(), .integrate(frames), .extract(), .to_dense()
  extract_mesh(values, origin, voxel, level, ...)  marching tetrahedra of any [Nz,Ny,Nx] device tensor
  components(faces, n_vertices)                    connected-component labels and sizes of an indexed mesh (csrc/lrf_mesh_clean.inl)
  filter_components(mesh, min_faces, min_fraction) the mesh without its small components, order and bytes preserved
  simplify(mesh, cell, origin)                     the mesh with the vertices of every grid cell merged into one (csrc/lrf_mesh_simplify.inl),
                                                   at their mean or, placement="quadric", where the faces' plane quadric is smallest
  topology(mesh)                                   boundary and non-manifold edge counts, the boundary-vertex mask (csrc/lrf_mesh_smooth.inl)
  vertex_normals(mesh)                             the mesh with area-weighted unit normals per vertex
  smooth(mesh, iterations, lam, mu, boundary)      the mesh after Taubin lambda|mu smoothing of its vertices
  holes(mesh, max_edges)                           boundary edges, and the boundary loops that fill_holes would close (csrc/lrf_mesh_fill.inl)
  fill_holes(mesh, max_edges)                      the mesh with every simple boundary loop of up to max_edges edges closed by a fan
  scene_mesh(local_tensorfs, W, H, voxel=...)      novel_views.render_poses in batches, each integrated and dropped, then extract
  pointcloud.write_ply(path, vertices, rgb8, normals=normals, faces=faces) writes the result

A volume is a lattice of Nx x Ny x Nz points at origin + (ix, iy, iz) * voxel, x fastest in memory.  Depth follows the
convention of pointcloud.py: a multiple of the un-normalised camera direction whose z is -1, so the signed distance of a
lattice point along its pixel's ray is depth - z.  Pinhole cameras only.  A mesh is a dict: vertices [Nv,3] fp32, faces [Nf,3]
int32 (wound so that the normal points towards larger values: free space for a TSDF), rgb8 [Nv,3] uint8 or None, counts =
(Nv, Nf) Python ints.  The same bytes on every run.  Every function checks its arguments on the host before its first launch.
CPU tensors raise NativeError: there is no torch fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._native import NativeError
from . import pointcloud
from ._checks import INT32 as _INT32
from ._checks import (check_bytes, check_choice, check_depth, check_faces, check_flag, check_frame_poses, check_int, check_interval,
                      check_intrinsics, check_mesh, check_origin, check_positive, check_range, check_rgb, dev_f32, float_of_key,
                      mesh_on_device, rgb8_frames)
from .pointcloud import SceneFrames

BYTES_PER_VOXEL = 8                            # tsdf and weight
BYTES_PER_VOXEL_RGB = 12


def _check_lattice(origin, voxel, dims):
    origin = check_origin(origin)
    voxel = check_positive("voxel", float(voxel))
    if len(dims) != 3 or any(int(d) != d or int(d) < 1 for d in dims):
        raise ValueError(f"dims must be (Nx, Ny, Nz) integers >= 1, got {dims!r}")
    dims = tuple(int(d) for d in dims)
    if dims[0] * dims[1] * dims[2] > _INT32:
        raise ValueError(f"dims {dims} hold {dims[0] * dims[1] * dims[2]} lattice points; a volume takes Nx Ny Nz < 2^31")
    return origin, voxel, dims


def _check_extract(level, min_weight, max_vertices, max_faces):
    level, min_weight = float(level), float(min_weight)
    if math.isnan(level):
        raise ValueError("level must not be NaN")
    if not min_weight > 0:
        raise ValueError(f"min_weight must be > 0, got {min_weight}")
    for name, cap in (("max_vertices", max_vertices), ("max_faces", max_faces)):
        check_int(name, cap, 0, _INT32, "None or an integer in [0, 2^31)", none_ok=True)
    return level, min_weight


def _check_frames(colours, dev, depth, poses, focal, center, rgb, depth_range, what="TsdfVolume"):
    """The frame arguments of an integration into a volume on dev that keeps colours or not, checked on the host ->
    (depth, rgb8 or None, poses, focal, center as contiguous device tensors, (V, H, W), (d_min, d_max))."""
    V, H, W = check_depth(depth)
    if (rgb is not None) != colours:
        raise ValueError(f"rgb goes with a volume that keeps colours: pass rgb to a {what}(colours=True) and only to it")
    if rgb is not None:
        check_rgb(rgb, depth)
    poses = check_frame_poses(poses, V)
    focal, center = check_intrinsics(focal, center, False)
    d_min, d_max = check_range(depth_range)
    N.require_gpu(depth, "depth", "the TSDF integration")
    if depth.device != dev:
        raise ValueError(f"depth lives on {depth.device}, the volume on {dev}")
    rgb8 = None if rgb is None else rgb8_frames(rgb, depth)
    depth = N.conform(depth)
    poses = poses.detach().to(device=dev, dtype=torch.float32).contiguous()
    return depth, rgb8, poses, dev_f32(focal, 1, dev), dev_f32(center, 2, dev), (V, H, W), (d_min, d_max)


def _sized_extract(dev, colours, launch, max_vertices, max_faces):
    """The capacity protocol of both extractions.  launch(cap_v, cap_f, v, f, c, counts) enqueues one extraction into
    buffers of that many rows -> the mesh dict."""
    counts = torch.empty(2, dtype=torch.int64, device=dev)

    def run(cap_v, cap_f):
        v = torch.empty(max(cap_v, 1), 3, dtype=torch.float32, device=dev)
        f = torch.empty(max(cap_f, 1), 3, dtype=torch.int32, device=dev)
        c = torch.empty(max(cap_v, 1), 3, dtype=torch.uint8, device=dev) if colours else None
        launch(cap_v, cap_f, v, f, c, counts)
        nv, nf = (int(x) for x in counts.tolist())                  # the read-back (it also orders the workspace's release)
        return v, f, c, nv, nf

    if max_vertices is None or max_faces is None:                   # a counting call sizes the buffers: one more read-back
        _, _, _, nv, nf = run(0, 0)
        cap_v = nv if max_vertices is None else int(max_vertices)
        cap_f = nf if max_faces is None else int(max_faces)
        if nv > _INT32 or nf > _INT32:
            raise ValueError(f"the mesh holds {nv} vertices and {nf} faces; each count must stay below 2^31")
    else:
        cap_v, cap_f = int(max_vertices), int(max_faces)
    v, f, c, nv, nf = run(cap_v, cap_f)
    if nv > cap_v or nf > cap_f:
        err = ValueError(f"the mesh holds {nv} vertices and {nf} faces; max_vertices={max_vertices} and max_faces={max_faces} "
                         "do not fit them")
        err.partial = {"vertices": v[:min(nv, cap_v)], "faces": f[:min(nf, cap_f)], "rgb8": None if c is None else c[:min(nv, cap_v)],
                       "counts": (nv, nf)}                          # the rows inside capacity, as written
        raise err
    return {"vertices": v[:nv], "faces": f[:nf], "rgb8": None if c is None else c[:nv], "counts": (nv, nf)}


def _extract(value, weight, rgb, origin, voxel, dims, level, min_weight, max_vertices, max_faces):
    """Checked arguments, contiguous fp32 device tensors -> the mesh dict."""
    dev = value.device
    Nx, Ny, Nz = dims
    ws = N.workspace("lrf_mesh", dev, Nx, Ny, Nz)
    a = N.LrfMeshExtract()
    a.value, a.weight, a.rgb = value.data_ptr(), None if weight is None else weight.data_ptr(), None if rgb is None else rgb.data_ptr()
    a.Nx, a.Ny, a.Nz = Nx, Ny, Nz
    a.origin[0], a.origin[1], a.origin[2] = origin
    a.voxel, a.level, a.min_weight = voxel, level, min_weight

    def launch(cap_v, cap_f, v, f, c, counts):
        N.launch("lrf_mesh_extract", dev, C.byref(a), cap_v, cap_f, v.data_ptr(), None if c is None else c.data_ptr(),
                 f.data_ptr(), counts.data_ptr(), ws.data_ptr(), guard=True)

    return _sized_extract(dev, rgb is not None, launch, max_vertices, max_faces)


def extract_mesh(values, origin, voxel, level, weight=None, rgb=None, min_weight=1.0, max_vertices=None, max_faces=None):
    """Marching tetrahedra (the Kuhn split, six per cell: no ambiguous case, watertight by construction) of values
    [Nz,Ny,Nx] (device) on the lattice origin + (ix, iy, iz) * voxel at `level`.  A lattice point is inside when its value is
    < level; with weight [Nz,Ny,Nx] only cells whose eight corners have weight >= min_weight give faces; rgb [Nz,Ny,Nx,3] in
    [0, 1] gives vertex colours, interpolated like the positions and encoded as novel_views.encode_frames encodes.
    Vertices come in (z, y, x, edge) order and faces in (cell, tetrahedron, triangle) order.  With max_vertices and max_faces
    given, the buffers hold that many rows and the call costs one read-back; a mesh that does not fit raises ValueError naming
    both true counts (its .partial holds the rows inside capacity).  With either None a counting call sizes the buffers
    first: one more read-back.  Returns the mesh dict of the module docstring."""
    if not torch.is_tensor(values):
        raise TypeError("values must be a torch tensor")
    if not values.is_floating_point():
        raise ValueError(f"values must hold floating-point values, got {values.dtype}")
    if values.dim() != 3 or min(values.shape) < 1:
        raise ValueError(f"values must be [Nz, Ny, Nx] with Nz, Ny, Nx > 0, got {tuple(values.shape)}")
    Nz, Ny, Nx = (int(s) for s in values.shape)
    origin, voxel, dims = _check_lattice(origin, voxel, (Nx, Ny, Nz))
    for name, t, shape in (("weight", weight, (Nz, Ny, Nx)), ("rgb", rgb, (Nz, Ny, Nx, 3))):
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch tensor or None")
        if not t.is_floating_point() or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a floating-point tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        if t.device != values.device:
            raise ValueError(f"{name} and values must live on the same device")
    level, min_weight = _check_extract(level, min_weight, max_vertices, max_faces)
    N.require_gpu(values, "values", "the mesh extraction")
    return _extract(N.conform(values), None if weight is None else N.conform(weight), None if rgb is None else N.conform(rgb),
                    origin, voxel, dims, level, min_weight, max_vertices, max_faces)


def _check_rounds(max_rounds):
    return check_int("max_rounds", max_rounds, 1, wording="an integer >= 1")


def _check_min_faces(name, min_faces):
    return check_int(name, min_faces, 0, wording="an integer >= 0")


def _check_min_fraction(name, min_fraction):
    return check_interval(name, min_fraction, 0.0, 1.0, "lie in [0, 1]")


def _components(faces, Nv, Nf, max_rounds):
    """Checked arguments, faces a contiguous int32 device tensor -> the dict of components()."""
    dev = faces.device
    labels = torch.empty(Nv, dtype=torch.int32, device=dev)
    faces_of = torch.empty(Nv, dtype=torch.int32, device=dev)
    vertices_of = torch.empty(Nv, dtype=torch.int32, device=dev)
    if Nv == 0:
        return {"labels": labels, "faces_of": faces_of, "vertices_of": vertices_of, "n_components": 0, "n_with_faces": 0,
                "largest_faces": 0, "rounds": 0}
    fp = faces.data_ptr() if Nf else None
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    N.launch("lrf_mesh_components_init", dev, labels.data_ptr(), Nv, guard=True)
    rounds = 0
    while True:
        N.launch("lrf_mesh_components_round", dev, labels.data_ptr(), fp, Nv, Nf, changed.data_ptr(), guard=True)
        rounds += 1
        word = int(changed.item())                                  # the round's read-back: 4 bytes
        if word & 2:
            raise ValueError(f"faces holds an index outside [0, {Nv}): the mesh has {Nv} vertices")
        if not word & 1:
            break
        if rounds >= max_rounds:
            raise RuntimeError(f"components: the labels still changed in round {rounds}; max_rounds is {max_rounds}")
    summary = torch.empty(3, dtype=torch.int64, device=dev)
    N.launch("lrf_mesh_components_count", dev, labels.data_ptr(), fp, Nv, Nf, faces_of.data_ptr(), vertices_of.data_ptr(),
             summary.data_ptr(), guard=True)
    n_components, n_with_faces, largest = (int(x) for x in summary.tolist())     # the summary's read-back
    return {"labels": labels, "faces_of": faces_of, "vertices_of": vertices_of, "n_components": n_components,
            "n_with_faces": n_with_faces, "largest_faces": largest, "rounds": rounds}


def components(faces, n_vertices, max_rounds=64):
    """The connected components of the mesh whose faces [Nf,3] int32 (device) index n_vertices vertices.  Two vertices are
    connected when a face holds both; a vertex that no face holds is a component of its own with 0 faces.  Returns a dict:
    labels [Nv] int32 (the smallest vertex index of each vertex's component), faces_of and vertices_of [Nv] int32 (the
    component's face and vertex counts at its label, 0 elsewhere), all on the device, and the Python ints n_components,
    n_with_faces (components with at least one face), largest_faces (the face count of the largest) and rounds.
    Min-label hooking with atomicMin and a bounded walk (csrc/lrf_mesh_clean.inl): the host launches one round after the
    other and reads 4 bytes back after each; the first round whose hooking pass changes nothing ends the loop, and rounds
    counts it.  max_rounds guards against a loop that never ends -- it is not tuned -- and raises RuntimeError naming the
    count when it is reached.  A face index outside [0, n_vertices) is never dereferenced and raises ValueError.  One more
    read-back brings the three summary words.  The labels are a unique fixed point: the same bytes on every run."""
    Nv, Nf = check_faces(faces, n_vertices)
    max_rounds = _check_rounds(max_rounds)
    N.require_gpu(faces, "faces", "the component labelling")
    return _components(faces.detach().contiguous(), Nv, Nf, max_rounds)


def filter_components(mesh, min_faces=0, min_fraction=0.0, max_rounds=64):
    """The mesh (the dict of the module docstring) without its small connected components: a component is kept when it holds
    at least threshold = max(min_faces, ceil(min_fraction * largest_faces)) faces, largest_faces being the face count of the
    largest component.  min_fraction=1.0 keeps the largest component and every tie with it; min_faces=1 drops exactly the
    vertices that no face holds; with both 0 the result holds the input's bytes.  Kept vertices and faces keep their order,
    a kept vertex's new index is the number of kept vertices before it, rgb8 follows the vertices, and positions and colours
    are copied bit for bit: the output bytes are a fixed function of the input.  components() runs first (its read-backs);
    the threshold is computed on the host from its summary; the output buffers are allocated at the input's sizes and
    sliced once the filter's three counts come back: one more read-back.  An empty result is a mesh with shapes [0,3] and
    counts (0, 0).  Returns a new mesh dict -- every other entry of the input is carried over -- with "components": the
    Python ints of components() (n_components, n_with_faces, largest_faces, rounds), "threshold" and "kept", the number of
    kept components."""
    v, f, c, Nv, Nf = check_mesh(mesh)
    min_faces, min_fraction = _check_min_faces("min_faces", min_faces), _check_min_fraction("min_fraction", min_fraction)
    max_rounds = _check_rounds(max_rounds)
    v, f, c, dev = mesh_on_device(v, f, c, "the component filter")
    comp = _components(f, Nv, Nf, max_rounds)
    threshold = max(min_faces, int(math.ceil(min_fraction * comp["largest_faces"])))
    out = dict(mesh)
    info = {k: comp[k] for k in ("n_components", "n_with_faces", "largest_faces", "rounds")}
    info["threshold"] = threshold
    if Nv == 0:
        info["kept"] = 0
        out.update(vertices=v, faces=f, rgb8=c, counts=(0, 0), components=info)
        return out
    if threshold > _INT32:                                          # no component holds 2^31 faces
        threshold = _INT32
    vo, fo = torch.empty_like(v), torch.empty_like(f)
    co = None if c is None else torch.empty_like(c)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    ws = N.workspace("lrf_mesh_filter", dev, Nv, Nf)
    a = N.LrfMeshFilter()
    a.vertices, a.rgb8, a.faces = v.data_ptr(), None if c is None else c.data_ptr(), f.data_ptr() if Nf else None
    a.labels, a.faces_of = comp["labels"].data_ptr(), comp["faces_of"].data_ptr()
    a.Nv, a.Nf = Nv, Nf
    N.launch("lrf_mesh_filter", dev, C.byref(a), threshold, vo.data_ptr(), None if co is None else co.data_ptr(),
             fo.data_ptr() if Nf else None, counts.data_ptr(), ws.data_ptr(), guard=True)
    nv, nf, kept = (int(x) for x in counts.tolist())                # the read-back (it also orders the workspace's release)
    info["kept"] = kept
    out.update(vertices=vo[:nv], faces=fo[:nf], rgb8=None if co is None else co[:nv], counts=(nv, nf), components=info)
    return out


PLACEMENTS = ("mean", "quadric")


def simplify(mesh, cell, origin=(0.0, 0.0, 0.0), dedupe=True, max_bytes=1 << 30, *, placement="mean", regularize=2.0 ** -10):
    """The mesh (the dict of the module docstring) simplified by uniform vertex clustering (csrc/lrf_mesh_simplify.inl states
    every rule): the vertices that fall into one cell of the grid of edge `cell` anchored at `origin` become one vertex at
    their mean position and mean colour; every face index becomes its vertex's cluster; a face that has lost a corner is
    dropped; with dedupe, of the faces that have become equal (up to rotation; a mirrored face is another face) the one that
    came first stays.  Clusters are ordered by cell (x fastest), only those a surviving face holds are emitted, surviving
    faces keep their order, and each starts at its smallest index.  A mesh without faces gives the empty mesh.  Manifoldness
    is not preserved.  The output bytes are a fixed function of the input -- integer sums, fp64 operations rounded one by
    one, the smallest face index per key -- and do not depend on the order of the input's vertices.
    placement="quadric" changes the positions and nothing else: each emitted vertex goes where the summed plane quadric of
    the input faces that touch its cluster (weighted by squared area, faces that collapse included) is smallest, clamped to
    the cluster's closed cell.  A curved surface keeps its volume better and corners stay sharp where a cell holds one.
    regularize in (0, 1] pulls towards the mean with weight regularize * trace of the quadric; it decides the position inside
    a plane and along a crease.  A cluster without a usable quadric (no face with area, 2^21 or more contributions, a system
    that does not solve) keeps the mean.  The bytes do not depend on the order of vertices or faces either.  It is not an
    option of extract() or scene_mesh(): compose simplify(vol.extract(...), cell, origin=vol.origin, placement="quadric").
    Two read-backs: the 7 words of the bounds pass (a vertex that is not finite, or more than 2^30 cells from the origin,
    raises ValueError; so does a cell box of 2^31 cells or more, or one whose workspace exceeds max_bytes: a larger cell is
    needed), then the counts (a face index outside [0, Nv) is never dereferenced and raises ValueError); the output buffers
    are allocated at the input's sizes and sliced.  Returns a new mesh dict -- every other entry of the input is carried over
    -- with "simplify": the Python values cell, origin, box (lo, dims: the cell box of the input), occupied (cells that hold
    a vertex), degenerate_faces, duplicate_faces and placement; for "quadric" also regularize, fallback_clusters (emitted
    vertices left at the mean) and clamped_clusters (emitted vertices whose solution lay outside the cell)."""
    v, f, c, Nv, Nf = check_mesh(mesh)
    cell = check_positive("cell", cell)
    origin = check_origin(origin)
    dedupe = check_flag("dedupe", dedupe)
    max_bytes = check_bytes(max_bytes)
    placement = check_choice("placement", placement, PLACEMENTS)
    regularize = check_interval("regularize", regularize, 0.0, 1.0, "satisfy 0 < regularize <= 1", open_lo=True)
    quadric = placement == "quadric"
    entry = "lrf_mesh_simplify_quadric" if quadric else "lrf_mesh_simplify"
    v, f, c, dev = mesh_on_device(v, f, c, "the mesh simplification")
    out = dict(mesh)
    info = {"cell": cell, "origin": origin, "box": {"lo": (0, 0, 0), "dims": (0, 0, 0)}, "occupied": 0, "degenerate_faces": 0,
            "duplicate_faces": 0, "placement": placement}
    if quadric:
        info.update(regularize=regularize, fallback_clusters=0, clamped_clusters=0)
    if Nv == 0:
        out.update(vertices=v, faces=f, rgb8=c, counts=(0, 0), simplify=info)
        return out
    o3 = (C.c_double * 3)(*origin)
    words = torch.empty(7, dtype=torch.int32, device=dev)
    N.launch("lrf_mesh_simplify_bounds", dev, v.data_ptr(), Nv, o3, cell, words.data_ptr(), guard=True)
    words = words.tolist()                                          # read-back one
    if words[6]:
        raise ValueError(f"vertices holds a value that is not finite or lies 2^30 cells of {cell} or more from origin {origin}")
    lo, dims = tuple(words[:3]), tuple(h - l + 1 for l, h in zip(words[:3], words[3:6]))
    cells = dims[0] * dims[1] * dims[2]
    box = f"the cell box {dims[0]} x {dims[1]} x {dims[2]} from {lo}"
    if cells > _INT32:
        raise ValueError(f"{box} holds {cells} cells; a simplification takes fewer than 2^31: a larger cell is needed")
    need = int(getattr(N.lib(), entry + "_workspace_bytes")(Nv, Nf, cells))
    if need == 0:
        raise NativeError(f"{entry}: refused shape {(Nv, Nf, cells)}")
    if need > max_bytes:
        raise ValueError(f"{box} takes a workspace of {need} bytes; max_bytes is {max_bytes}: a larger cell is needed")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    vo, fo = torch.empty_like(v), torch.empty_like(f)
    co = None if c is None else torch.empty_like(c)
    counts = torch.empty(7 if quadric else 5, dtype=torch.int64, device=dev)
    q = N.LrfMeshSimplifyQuadric() if quadric else None
    a = q.mesh if quadric else N.LrfMeshSimplify()
    a.vertices, a.rgb8, a.faces = v.data_ptr(), None if c is None else c.data_ptr(), f.data_ptr() if Nf else None
    a.Nv, a.Nf, a.cell, a.dedupe = Nv, Nf, cell, int(dedupe)
    for k in range(3):
        a.origin[k], a.lo[k], a.dims[k] = origin[k], lo[k], dims[k]
    if quadric:
        q.regularize = regularize
    N.launch(entry, dev, C.byref(q if quadric else a), vo.data_ptr(), None if co is None else co.data_ptr(),
             fo.data_ptr() if Nf else None, counts.data_ptr(), ws.data_ptr(), guard=True)
    nv, nf, occupied, degenerate, duplicate, *placed = (int(x) for x in counts.tolist())    # read-back two (it also orders ws's release)
    if nf < 0:
        raise ValueError(f"faces holds an index outside [0, {Nv}): the mesh has {Nv} vertices")
    if nv < 0:
        raise ValueError(f"vertices changed between the bounds pass and the simplification: one lies outside {box}")
    info.update(box={"lo": lo, "dims": dims}, occupied=occupied, degenerate_faces=degenerate, duplicate_faces=duplicate)
    if quadric:
        info.update(fallback_clusters=placed[0], clamped_clusters=placed[1])
    out.update(vertices=vo[:nv], faces=fo[:nf], rgb8=None if co is None else co[:nv], counts=(nv, nf), simplify=info)
    return out


def _check_incidence_mesh(mesh):
    """check_mesh and the bound of the incidence lists -> (vertices, faces, Nv, Nf); rgb8 is not read."""
    v, f, _, Nv, Nf = check_mesh(mesh)
    if 3 * Nf > _INT32:
        raise ValueError(f"faces holds {Nf} rows; the incidence lists take 3 Nf < 2^31")
    return v, f, Nv, Nf


def _raise_flags(flags, Nv):
    """The flag word of csrc/lrf_mesh_smooth.inl after a call's read-back."""
    if flags & 1:
        raise ValueError(f"faces holds an index outside [0, {Nv}): the mesh has {Nv} vertices")
    if flags & 2:
        raise ValueError("a vertex is held by 2^20 faces or more: the int64 sums have no headroom for it")
    if flags & 4:
        raise ValueError("vertices holds a value that is not finite")
    if flags & 8:
        raise ValueError("the smoothing diverged: a coordinate left the fixed-point range (32 times the input's largest extent)")


def topology(mesh):
    """Boundary and non-manifold edges of the mesh (the dict of the module docstring; csrc/lrf_mesh_smooth.inl states every
    rule).  A face with two equal indices is degenerate: it is counted and takes part in nothing.  For each directed edge (a, b)
    of each other face f: opp = the directed edges (b, a) among those faces, same = the directed edges (a, b) in faces other
    than f.  Returns a dict of Python values -- boundary_edges (directed edges with opp == 0), nonmanifold_edges (same > 0 or
    opp > 1), degenerate_faces, closed (both edge counts are 0) -- and boundary_vertices: a device [Nv] uint8 mask, 1 at both
    ends of every edge with opp == 0.  Integer counts: the same values on every run.  One call, one read-back; a face index
    outside [0, Nv) is never dereferenced and raises ValueError, and so does a vertex held by 2^20 faces or more."""
    v, f, Nv, Nf = _check_incidence_mesh(mesh)
    v, f, _, dev = mesh_on_device(v, f, None, "the mesh topology")
    mask = torch.empty(Nv, dtype=torch.uint8, device=dev)
    if Nv == 0:
        return {"boundary_edges": 0, "nonmanifold_edges": 0, "degenerate_faces": 0, "closed": True, "boundary_vertices": mask}
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ws = N.workspace("lrf_mesh_incidence", dev, Nv, Nf)
    N.launch("lrf_mesh_topology", dev, f.data_ptr() if Nf else None, Nv, Nf, mask.data_ptr(), info.data_ptr(), ws.data_ptr(), guard=True)
    words = [int(x) for x in info.tolist()]                         # the read-back (it also orders ws's release)
    _raise_flags(words[0], Nv)
    return {"boundary_edges": words[2], "nonmanifold_edges": words[3], "degenerate_faces": words[1],
            "closed": words[2] == 0 and words[3] == 0, "boundary_vertices": mask}


def vertex_normals(mesh):
    """The mesh with "normals": [Nv,3] fp32 unit normals, area-weighted (csrc/lrf_mesh_smooth.inl states every rule).  The
    normal of face (a, b, c) is (v_b - v_a) x (v_c - v_a) in fp64; every face normal is rounded to fixed point at one shared
    exponent (41 bits for the largest component of the largest face), a vertex's normal is the int64 sum over the faces around
    it -- exact, so it does not depend on the order of the faces -- divided by its length in fp64 and rounded to fp32.  Faces
    keep extract_mesh's winding, so the normals of a TSDF mesh point towards free space.  A vertex whose sum is zero (one that
    no face holds among them) gets (0, 0, 0).  Degenerate faces (two equal indices) contribute nothing.  One call, one
    read-back; a face index outside [0, Nv), a vertex held by 2^20 faces or more and a vertex coordinate that is not finite raise
    ValueError.  Returns a new mesh dict -- every other entry of the input is carried over -- with "normals" and
    "normal_info": the Python ints zero_normals and degenerate_faces.  pointcloud.write_ply(path, vertices, rgb8,
    normals=mesh["normals"], faces=mesh["faces"]) writes them."""
    v, f, Nv, Nf = _check_incidence_mesh(mesh)
    v, f, _, dev = mesh_on_device(v, f, None, "the vertex normals")
    out = dict(mesh)
    normals = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    if Nv == 0:
        out.update(normals=normals, normal_info={"zero_normals": 0, "degenerate_faces": 0})
        return out
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ws = N.workspace("lrf_mesh_incidence", dev, Nv, Nf)
    N.launch("lrf_mesh_vertex_normals", dev, v.data_ptr(), f.data_ptr() if Nf else None, Nv, Nf, normals.data_ptr(), info.data_ptr(),
             ws.data_ptr(), guard=True)
    words = [int(x) for x in info.tolist()]                         # the read-back (it also orders ws's release)
    _raise_flags(words[0], Nv)
    out.update(normals=normals, normal_info={"zero_normals": words[4], "degenerate_faces": words[1]})
    return out


def smooth(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed"):
    """The mesh after `iterations` iterations of Taubin lambda|mu smoothing (csrc/lrf_mesh_smooth.inl states every rule): one
    iteration moves every vertex by lam times the way to the mean of its neighbours, then by mu (negative: back out, which keeps
    the shape from shrinking); mu == 0 skips the second step and gives plain Laplacian smoothing.  The neighbours of a vertex
    are the two other corners of every face around it, each face counted once: on a closed manifold every neighbour is
    counted twice and this is the uniform umbrella; along an open border the two border neighbours are counted once, so they
    weigh half.  Degenerate faces (two equal indices) take part in nothing.  boundary="fixed" pins the vertices of
    topology()'s boundary_vertices; "free" pins none.  Pinned vertices and vertices no face holds keep their bits; faces, rgb8
    and every other entry are carried over.  The means are exact: positions are rounded to fixed point (36 bits over the
    largest extent of the input's box, from its per-axis minimum) and summed in int64, and every fp64 operation around them is
    rounded on its own, so the output bytes are a fixed function of the input and do not depend on the order of the faces.
    Two read-backs: the 7 words of the bounds pass (a vertex that is not finite raises ValueError; a box of zero extent returns
    the input's bytes), then the counts and flags after all iterations, which one native call queues with no host
    synchronisation between them (a face index outside [0, Nv) is never dereferenced and raises ValueError; so do a vertex held
    by 2^20 faces or more and an iteration that leaves 32 times the input's extent).  Returns a new mesh dict with "smooth":
    iterations, lam, mu, boundary, pinned, boundary_edges, nonmanifold_edges, degenerate_faces."""
    v, f, Nv, Nf = _check_incidence_mesh(mesh)
    iterations = check_int("iterations", iterations, 0, 1000)
    lam = check_interval("lam", lam, 0.0, 1.0, "satisfy 0 < lam <= 1", open_lo=True)
    mu = check_interval("mu", mu, -1.0, 0.0, "satisfy -1 <= mu <= 0")
    if boundary not in ("fixed", "free"):
        raise ValueError(f"boundary must be 'fixed' or 'free', got {boundary!r}")
    v, f, _, dev = mesh_on_device(v, f, None, "the mesh smoothing")
    out = dict(mesh)
    info = {"iterations": iterations, "lam": lam, "mu": mu, "boundary": boundary, "pinned": 0,
            "boundary_edges": 0, "nonmanifold_edges": 0, "degenerate_faces": 0}
    if Nv == 0:
        out.update(vertices=v, smooth=info)
        return out
    keys = torch.empty(7, dtype=torch.int32, device=dev)
    N.launch("lrf_mesh_smooth_bounds", dev, v.data_ptr(), Nv, keys.data_ptr(), guard=True)
    keys = keys.tolist()                                            # read-back one
    if keys[6]:
        raise ValueError("vertices holds a value that is not finite")
    lo = [float_of_key(k) for k in keys[:3]]
    extent = max(float_of_key(k) - l for k, l in zip(keys[3:6], lo))
    a = N.LrfMeshSmooth()
    a.vertices, a.faces, a.Nv, a.Nf = v.data_ptr(), f.data_ptr() if Nf else None, Nv, Nf
    a.lam, a.mu, a.pin_boundary = lam, mu, int(boundary == "fixed")
    # a box of zero extent: nothing can move, the call copies the input's bytes (and still counts)
    a.s, a.iterations = (36 - math.frexp(extent)[1], iterations) if extent > 0.0 else (0, 0)
    for k in range(3):
        a.lo[k] = lo[k]
    vo = torch.empty_like(v)
    words = torch.empty(8, dtype=torch.int64, device=dev)
    ws = N.workspace("lrf_mesh_smooth", dev, Nv, Nf)
    N.launch("lrf_mesh_smooth", dev, C.byref(a), vo.data_ptr(), words.data_ptr(), ws.data_ptr(), guard=True)
    words = [int(x) for x in words.tolist()]                        # read-back two (it also orders ws's release)
    _raise_flags(words[0], Nv)
    info.update(pinned=words[5], boundary_edges=words[2], nonmanifold_edges=words[3], degenerate_faces=words[1])
    out.update(vertices=vo, smooth=info)
    return out


_HOLE_KEYS = ("boundary_edges", "nonmanifold_edges", "degenerate_faces", "loops", "loop_edges", "longest_loop", "open_edges")
MAX_HOLE_EDGES = 4096                          # HF_MAX_EDGES of csrc/lrf_mesh_fill.inl: the bound of the serial walk along a loop


def _check_max_edges(max_edges):
    return check_int("max_edges", max_edges, 3, MAX_HOLE_EDGES)


def _raise_fill_flags(flags, Nv):
    """The flag word of csrc/lrf_mesh_fill.inl after a call's read-back."""
    _raise_flags(flags & 7, Nv)
    if flags & 8:
        raise ValueError("vertices changed between the bounds pass and the hole analysis: a coordinate left the fixed-point range")
    if flags & 16:
        raise ValueError("the mesh changed between the hole analysis and the fill: the loops no longer fit the counted rows")


def _holes(v, c, f, Nv, Nf, max_edges, dev):
    """Checked arguments, Nv > 0: the bounds pass and lrf_mesh_holes, two read-backs -> (the dict of holes(), the filled-in
    LrfMeshHoles, the workspace)."""
    keys = torch.empty(7, dtype=torch.int32, device=dev)
    N.launch("lrf_mesh_smooth_bounds", dev, v.data_ptr(), Nv, keys.data_ptr(), guard=True)
    keys = keys.tolist()                                            # read-back one
    if keys[6]:
        raise ValueError("vertices holds a value that is not finite")
    lo = [float_of_key(k) for k in keys[:3]]
    extent = max(float_of_key(k) - l for k, l in zip(keys[3:6], lo))
    a = N.LrfMeshHoles()
    a.vertices, a.rgb8, a.faces = v.data_ptr(), None if c is None else c.data_ptr(), f.data_ptr() if Nf else None
    a.Nv, a.Nf, a.max_edges = Nv, Nf, max_edges
    a.s = 36 - math.frexp(extent)[1] if extent > 0.0 else 0
    for k in range(3):
        a.lo[k] = lo[k]
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ws = N.workspace("lrf_mesh_holes", dev, Nv, Nf)
    N.launch("lrf_mesh_holes", dev, C.byref(a), info.data_ptr(), ws.data_ptr(), guard=True)
    words = [int(x) for x in info.tolist()]                         # read-back two
    _raise_fill_flags(words[0], Nv)
    counts = {"boundary_edges": words[2], "nonmanifold_edges": words[3], "degenerate_faces": words[1], "loops": words[4],
              "loop_edges": words[5], "longest_loop": words[6], "open_edges": words[7]}
    if not extent > 0.0:                                            # a box of zero extent fills nothing
        counts.update(loops=0, loop_edges=0, longest_loop=0, open_edges=words[2])
    return counts, a, ws


def holes(mesh, max_edges=64):
    """The boundary of the mesh (the dict of the module docstring) and what fill_holes(mesh, max_edges) would close
    (csrc/lrf_mesh_fill.inl states every rule).  A boundary edge is a directed edge (a, b) of a face whose reverse no face holds
    (topology()'s opp == 0; degenerate faces take part in nothing).  A vertex is simple when exactly one boundary edge leaves it
    and exactly one enters it; following, from each boundary edge (a, b), the boundary edge that leaves b while b is simple
    splits the boundary into simple cycles and open chains.  A fillable loop is a cycle of 3 .. max_edges edges.  Returns a dict
    of Python ints: boundary_edges, nonmanifold_edges, degenerate_faces (as topology() counts them), loops (fillable loops),
    loop_edges (the boundary edges in them), longest_loop (the edges of the longest of them) and open_edges (boundary_edges -
    loop_edges: open chains, holes that touch in a vertex, rims through a non-manifold edge and loops above max_edges).
    max_edges lies in [3, 4096].  Two read-backs: the 7 words of smooth()'s bounds pass (a vertex that is not finite raises
    ValueError; in a box of zero extent nothing is fillable) and the 8 info words; a face index outside [0, Nv) is never
    dereferenced and raises ValueError, and so does a vertex held by 2^20 faces or more."""
    v, f, Nv, Nf = _check_incidence_mesh(mesh)
    max_edges = _check_max_edges(max_edges)
    v, f, _, dev = mesh_on_device(v, f, None, "the hole analysis")
    if Nv == 0:
        return dict.fromkeys(_HOLE_KEYS, 0)
    return _holes(v, None, f, Nv, Nf, max_edges, dev)[0]


def fill_holes(mesh, max_edges=64):
    """The mesh (the dict of the module docstring) with every fillable loop of holes(mesh, max_edges) closed
    (csrc/lrf_mesh_fill.inl states every rule).  The loops are ranked by their first boundary edge in face order; loop r adds
    vertex Nv + r at the mean of the loop's vertices -- exact: positions are rounded to smooth()'s fixed point and summed in
    int64, every fp64 operation around the sum rounded on its own -- with, where the mesh has rgb8, the rounded integer mean of
    their colours, and every boundary edge (a, b) of a fillable loop appends, in face order, the face (b, a, Nv + r), wound as
    the face that owns (a, b).  The input's vertices, colours and faces are the output's prefix, bit for bit, so the output
    bytes are a fixed function of the input; the set of new positions does not depend on the order of the input's faces.  Every
    edge of a filled loop is then shared by two faces, no new edge is non-manifold, and a second call with the same max_edges
    adds nothing.  A hole is closed by a fan, whatever its shape: no minimal-area triangulation, no refinement; holes that touch
    in a vertex, rims through a non-manifold edge and loops above max_edges (at most 4096) are left alone.
    holes() runs first (its two read-backs: a vertex that is not finite, a face index outside [0, Nv) and a vertex held by 2^20
    faces or more raise ValueError); then the buffers are allocated at Nv + loops and Nf + loop_edges rows and one native call
    fills them: a third read-back.  With nothing fillable that call is skipped and the result holds the input's tensors; an
    empty mesh returns itself.  Returns a new mesh dict -- every other entry of the input is carried over, except "normals",
    whose rows no longer match -- with "fill": the Python ints of holes() and added_vertices and added_faces."""
    v, f, Nv, Nf = _check_incidence_mesh(mesh)
    c = mesh.get("rgb8")
    max_edges = _check_max_edges(max_edges)
    v, f, c, dev = mesh_on_device(v, f, c, "the hole filling")
    out = dict(mesh)
    out.pop("normals", None)
    if Nv == 0:
        out["fill"] = dict(dict.fromkeys(_HOLE_KEYS, 0), added_vertices=0, added_faces=0)
        return out
    counts, a, ws = _holes(v, c, f, Nv, Nf, max_edges, dev)
    nv, nf = Nv + counts["loops"], Nf + counts["loop_edges"]
    out["fill"] = dict(counts, added_vertices=nv - Nv, added_faces=nf - Nf)
    if counts["loops"] == 0:
        return out
    if nv > _INT32 or 3 * nf > _INT32:
        raise ValueError(f"the filled mesh holds {nv} vertices and {nf} faces; a mesh takes Nv < 2^31 and 3 Nf < 2^31")
    vo = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    fo = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    co = None if c is None else torch.empty(nv, 3, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    N.launch("lrf_mesh_fill", dev, C.byref(a), vo.data_ptr(), None if co is None else co.data_ptr(), fo.data_ptr(), nv, nf,
             info.data_ptr(), ws.data_ptr(), guard=True)
    words = [int(x) for x in info.tolist()]                         # read-back three (it also orders ws's release)
    _raise_fill_flags(words[0] | (0 if (words[4], words[5]) == (nv - Nv, nf - Nf) else 16), Nv)
    out.update(vertices=vo, faces=fo, rgb8=co, counts=(nv, nf))
    return out


def _check_fill_option(name, max_edges):
    """0 (no fill), or the max_edges of fill_holes."""
    wording = f"0 or a max_edges value in [3, {MAX_HOLE_EDGES}]"
    n = check_int(name, max_edges, 0, MAX_HOLE_EDGES, wording)
    return n if n == 0 else check_int(name, n, 3, MAX_HOLE_EDGES, wording)


class _Chain:
    """The post-processing chain of an extracted mesh -- TsdfVolume.extract describes it -- and the only place that knows its
    options: their names, defaults and checks (OPTIONS, in the order in which a call with several bad values reports them),
    and the order in which they apply.  _Chain(mapping) reads its own keys from the mapping, checks them on the host and
    keeps them in .options, the keywords that both extract methods take."""
    OPTIONS = (("min_component_faces", 0, _check_min_faces),
               ("min_component_fraction", 0.0, _check_min_fraction),
               ("simplify_cell", None, lambda name, cell: None if cell is None else check_positive(name, cell)),
               ("smooth_iterations", 0, lambda name, n: check_int(name, n, 0, 1000)),
               ("normals", False, check_flag),
               ("fill_holes", 0, _check_fill_option))
    KEYS = tuple(name for name, _, _ in OPTIONS)

    def __init__(self, options):
        self.options = {name: check(name, options.get(name, default)) for name, default, check in self.OPTIONS}

    def apply(self, mesh, origin, empty=False):
        """The mesh itself with every option at its default -- nothing new is launched --, else filter_components of it, then
        fill_holes of that (the fill wants the manifold mesh at full resolution, and smooth then no longer pins the closed
        rims), then (the floaters having been judged at full resolution) simplify of that on the grid anchored at origin,
        then smooth of that with the defaults of smooth(), then vertex_normals of the smoothed positions.  empty: the mesh of
        a volume without blocks, which has nothing to filter, fill or simplify."""
        o = self.options
        if not empty:
            if not (o["min_component_faces"] == 0 and o["min_component_fraction"] == 0.0):
                mesh = filter_components(mesh, o["min_component_faces"], o["min_component_fraction"])
            if o["fill_holes"]:
                mesh = fill_holes(mesh, o["fill_holes"])
            if o["simplify_cell"] is not None:
                mesh = simplify(mesh, o["simplify_cell"], origin=origin)
        if o["smooth_iterations"]:
            mesh = smooth(mesh, o["smooth_iterations"])
        if o["normals"]:
            mesh = vertex_normals(mesh)
        return mesh


def _check_trunc_device(name, trunc, device):
    """The constructors' tail of checks -> (trunc, torch.device); the refusal names the class."""
    trunc_f = check_positive("trunc", trunc)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NativeError(f"localrf_amd.mesh: a {name} on {dev}; the integration can run only on an AMD GPU (HIP "
                          "kernels). There is no CPU fallback.")
    return trunc_f, dev


class TsdfVolume:
    """A truncated signed-distance volume on the device: tsdf [Nz,Ny,Nx] (starts at 1), weight [Nz,Ny,Nx] (starts at 0: the
    number of frames that saw the point) and, with colours, rgb [Nz,Ny,Nx,3] in [0, 1] (starts at 0).  dims = (Nx, Ny, Nz);
    trunc is the truncation distance in world units."""

    def __init__(self, origin, voxel, dims, trunc, device, colours=True):
        self.origin, self.voxel, self.dims = _check_lattice(origin, voxel, dims)
        self.trunc, dev = _check_trunc_device("TsdfVolume", trunc, device)
        Nx, Ny, Nz = self.dims
        self.tsdf = torch.ones(Nz, Ny, Nx, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(Nz, Ny, Nx, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(Nz, Ny, Nx, 3, dtype=torch.float32, device=dev) if colours else None

    @staticmethod
    def nbytes(dims, colours=True):
        return int(dims[0]) * int(dims[1]) * int(dims[2]) * (BYTES_PER_VOXEL + (BYTES_PER_VOXEL_RGB if colours else 0))

    def integrate(self, depth, poses, focal, center, rgb=None, depth_range=(0.0, math.inf)):
        """Fold V frames into the volume, in frame order: depth [V,H,W] (device), poses [V,3,4] camera-to-world, focal (one
        value) and center (cx, cy) as pointcloud.fuse_points takes them, rgb [V,H,W,3] float (encoded as encode_frames does) or
        uint8 -- required with colours, refused without.  Per lattice point and frame: the point is projected to its nearest
        pixel; with dn the depth there (finite, positive, inside depth_range), sdf = dn - z; the frame is skipped when
        sdf < -trunc (the point lies behind the surface by more than trunc), else s = min(1, sdf / trunc) enters the running
        means tsdf = (tsdf weight + s) / (weight + 1) and rgb, and weight += 1.  One launch, the volume read and written
        once; no read-back.  Calls add up: frames k..V on top of frames 0..k leave the bits of one call over 0..V."""
        dev = self.tsdf.device
        depth, rgb8, poses, f, c, (V, H, W), (d_min, d_max) = _check_frames(self.rgb is not None, dev, depth, poses, focal, center,
                                                                            rgb, depth_range)
        a = N.LrfTsdfVolume()
        a.tsdf, a.weight, a.rgb = self.tsdf.data_ptr(), self.weight.data_ptr(), None if self.rgb is None else self.rgb.data_ptr()
        a.Nx, a.Ny, a.Nz = self.dims
        a.origin[0], a.origin[1], a.origin[2] = self.origin
        a.voxel, a.trunc = self.voxel, self.trunc
        N.launch("lrf_tsdf_integrate", dev, C.byref(a), depth.data_ptr(), None if rgb8 is None else rgb8.data_ptr(),
                 poses.data_ptr(), f.data_ptr(), c.data_ptr(), V, H, W, d_min, d_max, guard=True)
        return self

    def extract(self, level=0.0, min_weight=1.0, max_vertices=None, max_faces=None, *, min_component_faces=0,
                min_component_fraction=0.0, simplify_cell=None, smooth_iterations=0, normals=False, fill_holes=0):
        """The mesh of the surface tsdf = level over the cells every corner of which at least min_weight frames saw:
        extract_mesh(self.tsdf, ..., weight=self.weight, rgb=self.rgb); see there for the capacities and the read-backs.
        The keyword-only options send that mesh through a chain of five steps, in this order, each skipped at its default:
        with min_component_faces or min_component_fraction above 0, filter_components(mesh, min_faces, min_fraction): its
        small connected components are gone.  With fill_holes (0, or a max_edges value), fill_holes(mesh, fill_holes): after
        the component filter and before simplify.  With simplify_cell (a cell edge in world units), simplify(mesh,
        simplify_cell, origin=self.origin): the grid is anchored at the volume's origin.  With smooth_iterations above 0,
        smooth(mesh, smooth_iterations), and with normals=True, vertex_normals(mesh): the normals of the smoothed surface.
        The defaults launch nothing new."""
        level, min_weight = _check_extract(level, min_weight, max_vertices, max_faces)
        chain = _Chain(dict(min_component_faces=min_component_faces, min_component_fraction=min_component_fraction,
                            simplify_cell=simplify_cell, smooth_iterations=smooth_iterations, normals=normals, fill_holes=fill_holes))
        return chain.apply(_extract(self.tsdf, self.weight, self.rgb, self.origin, self.voxel, self.dims, level, min_weight,
                                    max_vertices, max_faces), self.origin)


BLOCK = 8                                      # lattice points per block edge
BLOCK_POINTS = BLOCK ** 3
MAX_BLOCKS = (1 << 22) - 1                     # 512 n < 2^31


def _check_blocks(blocks):
    if len(blocks) != 3 or any(int(b) != b or int(b) < 1 for b in blocks):
        raise ValueError(f"blocks must be (Bx, By, Bz) integers >= 1, got {blocks!r}")
    blocks = tuple(int(b) for b in blocks)
    if any(BLOCK * b > _INT32 for b in blocks):
        raise ValueError(f"blocks {blocks}: an axis takes 8 B < 2^31 lattice points")
    if blocks[0] * blocks[1] * blocks[2] > _INT32:
        raise ValueError(f"blocks {blocks} make {blocks[0] * blocks[1] * blocks[2]} table entries; a grid takes Bx By Bz < 2^31")
    return blocks


class SparseTsdfVolume:
    """A TsdfVolume of dims 8 * blocks of which only the 8 x 8 x 8 blocks that some depth pixel's truncation band reaches are
    stored (csrc/lrf_tsdf_blocks.inl).  blocks = (Bx, By, Bz).  marks uint8 and table int32 [Bz,By,Bx] (-1, or the block's
    pool index), coords int32 [n,3] ((bx, by, bz) in pool order) and the pools tsdf, weight [n,8,8,8] and, with colours, rgb
    [n,8,8,8,3], x fastest.  touch() marks, allocate() gives the marked blocks their pool indices -- in (z, y, x) order after
    the blocks that exist, which keep index and contents --, integrate() updates the stored blocks only and leaves in each of
    their points the bits TsdfVolume.integrate leaves in the same lattice point, extract() meshes them.  A point in no block
    reads as (tsdf 1, weight 0): a missing block can leave a hole, never create or move a face.  No hash, no atomics: the
    same call sequence gives the same bytes."""

    def __init__(self, origin, voxel, blocks, trunc, device, colours=True):
        self.blocks = _check_blocks(blocks)
        self.dims = tuple(BLOCK * b for b in self.blocks)
        self.origin, self.voxel, _ = _check_lattice(origin, voxel, (1, 1, 1))
        self.trunc, dev = _check_trunc_device("SparseTsdfVolume", trunc, device)
        Bx, By, Bz = self.blocks
        self.colours = bool(colours)
        self.marks = torch.zeros(Bz, By, Bx, dtype=torch.uint8, device=dev)
        self.table = torch.full((Bz, By, Bx), -1, dtype=torch.int32, device=dev)
        self.n_blocks = 0
        self._coords = torch.zeros(1, 3, dtype=torch.int32, device=dev)
        self._tsdf = torch.ones(0, BLOCK, BLOCK, BLOCK, dtype=torch.float32, device=dev)
        self._weight = torch.zeros(0, BLOCK, BLOCK, BLOCK, dtype=torch.float32, device=dev)
        self._rgb = torch.zeros(0, BLOCK, BLOCK, BLOCK, 3, dtype=torch.float32, device=dev) if self.colours else None

    coords = property(lambda self: self._coords[:self.n_blocks])
    tsdf = property(lambda self: self._tsdf[:self.n_blocks])
    weight = property(lambda self: self._weight[:self.n_blocks])
    rgb = property(lambda self: None if self._rgb is None else self._rgb[:self.n_blocks])

    @staticmethod
    def bytes_for(blocks, n_blocks, colours=True):
        """marks and table of the grid, and coords and pools of n_blocks blocks."""
        per_block = 12 + BLOCK_POINTS * (BYTES_PER_VOXEL + (BYTES_PER_VOXEL_RGB if colours else 0))
        return int(blocks[0]) * int(blocks[1]) * int(blocks[2]) * 5 + int(n_blocks) * per_block

    @property
    def nbytes(self):
        return self.bytes_for(self.blocks, self.n_blocks, self.colours)

    def _args(self):
        a = N.LrfTsdfBlocks()
        a.marks, a.table, a.coords = self.marks.data_ptr(), self.table.data_ptr(), self._coords.data_ptr()
        a.tsdf, a.weight = self._tsdf.data_ptr() or None, self._weight.data_ptr() or None      # an empty pool has no address
        a.rgb = None if self._rgb is None else self._rgb.data_ptr() or None
        a.Bx, a.By, a.Bz = self.blocks
        a.n_blocks = self.n_blocks
        a.origin[0], a.origin[1], a.origin[2] = self.origin
        a.voxel, a.trunc = self.voxel, self.trunc
        return a

    def touch(self, depth, poses, focal, center, depth_range=(0.0, math.inf)):
        """Mark the blocks that the truncation bands of V frames reach; arguments as integrate takes them, without rgb.  Per
        pixel with a depth d that is finite, positive and inside depth_range: the world points a, b at depths max(d - trunc, 0)
        and d + trunc, the margin m = voxel + (d + trunc) / focal (half a pixel footprint and one voxel of slack), and every
        block that meets the box [min(a, b) - m, max(a, b) + m].  One launch, no read-back; marks add up over calls."""
        dev = self.table.device
        depth, _, poses, f, c, (V, H, W), (d_min, d_max) = _check_frames(False, dev, depth, poses, focal, center, None, depth_range)
        N.launch("lrf_tsdf_blocks_touch", dev, C.byref(self._args()), depth.data_ptr(), poses.data_ptr(), f.data_ptr(),
                 c.data_ptr(), V, H, W, d_min, d_max, guard=True)
        return self

    def allocate(self, max_bytes=None):
        """Give every marked block that has none a pool index -- the next ones, in block-linear (z, y, x) order -- and grow
        coords and the pools (new blocks: tsdf 1, weight 0, rgb 0).  A counting call (two launches), one read-back -- the
        number of new blocks, which is returned --, then, with new blocks only, the grown tensors and the assigning call (three
        launches).  A volume that would exceed max_bytes (nbytes with the new blocks) or 2^22 - 1 blocks raises ValueError
        and stays as it was."""
        dev = self.table.device
        limit = MAX_BLOCKS
        if max_bytes is not None:
            limit = min(limit, max(-1, (int(max_bytes) - self.bytes_for(self.blocks, 0, self.colours))
                                   // self.bytes_for((0, 0, 0), 1, self.colours)))
        if limit < self.n_blocks:
            raise ValueError(f"a volume of {self.n_blocks} blocks takes {self.nbytes} bytes; max_bytes is {int(max_bytes)}")
        ws = N.workspace("lrf_tsdf_blocks_assign", dev, *self.blocks)
        count = torch.empty(1, dtype=torch.int64, device=dev)

        def assign(max_blocks):
            N.launch("lrf_tsdf_blocks_assign", dev, C.byref(self._args()), max_blocks, self._coords.shape[0], count.data_ptr(),
                     ws.data_ptr(), guard=True)
        assign(self.n_blocks)                                       # a counting call: the table stays as it is
        new = int(count.item())                                     # the read-back (it also orders ws's release)
        n = self.n_blocks + new
        if n > MAX_BLOCKS:
            raise ValueError(f"the frames reach {n} blocks; a volume takes 512 n < 2^31 lattice points")
        if n > limit:
            raise ValueError(f"a volume of {n} blocks takes {self.bytes_for(self.blocks, n, self.colours)} bytes; max_bytes is "
                             f"{int(max_bytes)}")
        if new == 0:
            return 0

        def grown(old, fill):
            out = torch.full((n,) + tuple(old.shape[1:]), fill, dtype=old.dtype, device=dev)
            out[:self.n_blocks] = old[:self.n_blocks]
            return out
        # every allocation comes before the table changes: one that fails leaves the volume as it was
        coords = torch.zeros(n, 3, dtype=torch.int32, device=dev)
        tsdf, weight = grown(self._tsdf, 1.0), grown(self._weight, 0.0)
        rgb = None if self._rgb is None else grown(self._rgb, 0.0)
        old, self._coords = self._coords, coords                    # the pass below rewrites every row, the old ones too
        try:
            assign(n)
        except BaseException:
            self._coords = old
            raise
        self._tsdf, self._weight, self._rgb, self.n_blocks = tsdf, weight, rgb, n
        return new

    def integrate(self, depth, poses, focal, center, rgb=None, depth_range=(0.0, math.inf)):
        """TsdfVolume.integrate over the stored blocks: same arguments, same checks, same arithmetic per lattice point.  One
        launch of one workgroup per block, the pools read and written once; no read-back.  Blocks that are not stored see
        nothing: touch and allocate first.  With zero blocks nothing is launched."""
        dev = self.table.device
        depth, rgb8, poses, f, c, (V, H, W), (d_min, d_max) = _check_frames(self.colours, dev, depth, poses, focal, center, rgb,
                                                                            depth_range, "SparseTsdfVolume")
        if self.n_blocks:
            N.launch("lrf_tsdf_blocks_integrate", dev, C.byref(self._args()), depth.data_ptr(),
                     None if rgb8 is None else rgb8.data_ptr(), poses.data_ptr(), f.data_ptr(), c.data_ptr(), V, H, W, d_min, d_max,
                     guard=True)
        return self

    def extract(self, level=0.0, min_weight=1.0, max_vertices=None, max_faces=None, *, min_component_faces=0,
                min_component_fraction=0.0, simplify_cell=None, smooth_iterations=0, normals=False, fill_holes=0):
        """The mesh of the surface tsdf = level over the cells every corner of which is stored and was seen by at least
        min_weight frames.  Vertices come in pool order, then (z, y, x, edge) inside the block; faces in the pool order of
        the cell's lowest corner, then (z, y, x) inside the block, then (tetrahedron, triangle).  Capacities and read-backs as
        extract_mesh has them.  With zero blocks nothing is launched and the mesh is empty: of the chain only smooth and
        vertex_normals see it.  The keyword-only options, their checks and the chain's order as TsdfVolume.extract has them."""
        level, min_weight = _check_extract(level, min_weight, max_vertices, max_faces)
        chain = _Chain(dict(min_component_faces=min_component_faces, min_component_fraction=min_component_fraction,
                            simplify_cell=simplify_cell, smooth_iterations=smooth_iterations, normals=normals, fill_holes=fill_holes))
        dev = self.table.device
        if not self.n_blocks:
            empty = {"vertices": torch.empty(0, 3, dtype=torch.float32, device=dev), "faces": torch.empty(0, 3, dtype=torch.int32, device=dev),
                     "rgb8": torch.empty(0, 3, dtype=torch.uint8, device=dev) if self.colours else None, "counts": (0, 0)}
            return chain.apply(empty, self.origin, empty=True)
        ws = N.workspace("lrf_mesh_extract_blocks", dev, self.n_blocks)
        a = self._args()

        def launch(cap_v, cap_f, v, f, c, counts):
            N.launch("lrf_mesh_extract_blocks", dev, C.byref(a), level, min_weight, cap_v, cap_f, v.data_ptr(),
                     None if c is None else c.data_ptr(), f.data_ptr(), counts.data_ptr(), ws.data_ptr(), guard=True)

        return chain.apply(_sized_extract(dev, self.colours, launch, max_vertices, max_faces), self.origin)

    def to_dense(self):
        """(tsdf, weight, rgb or None, stored) as [8Bz,8By,8Bx] tensors of the virtual lattice (rgb [...,3]; stored: bool, the
        points of stored blocks); a point in no block holds (1, 0, 0).  For tests and debugging of small volumes."""
        Bx, By, Bz = self.blocks
        dev = self.table.device
        bx, by, bz = (self.coords[:, k].long() for k in range(3))

        def scatter(pool, fill, tail=()):
            out = torch.full((Bz, By, Bx, BLOCK, BLOCK, BLOCK) + tail, fill, dtype=pool.dtype, device=dev)
            out[bz, by, bx] = pool
            order = (0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(tail)))
            return out.permute(*order).reshape((BLOCK * Bz, BLOCK * By, BLOCK * Bx) + tail)
        stored = scatter(torch.ones(self.n_blocks, BLOCK, BLOCK, BLOCK, dtype=torch.bool, device=dev), False)
        return (scatter(self.tsdf, 1.0), scatter(self.weight, 0.0), None if self._rgb is None else scatter(self.rgb, 0.0, (3,)),
                stored)


_MESH_KEYS = ("depth_range", "level", "min_weight", "max_vertices", "max_faces", "colours", "frames_per_call") + _Chain.KEYS


def _lattice_of_box(lo, hi, voxel):
    lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
    if lo.size != 3 or hi.size != 3 or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or not (lo <= hi).all():
        raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)) with finite x0 <= x1, y0 <= y1, z0 <= z1, got {(lo, hi)!r}")
    dims = tuple(int(math.ceil((b - a) / voxel)) + 1 for a, b in zip(lo, hi))
    return tuple(float(v) for v in lo), dims


def scene_mesh(local_tensorfs, W, H, voxel, bounds=None, poses=None, trunc=None, max_bytes=4 << 30, depth="expected",
               max_spread=None, sparse=False, **options):
    """A scene's surface as a triangle mesh: its frames rendered by novel_views.render_poses frames_per_call (default 8) at
    a time, each batch integrated into one TsdfVolume and dropped -- only the volume stays resident, not the frames -- then
    TsdfVolume.extract.  poses=None renders the scene's own get_cam2world(), each frame through itself; otherwise poses
    [N,3,4] as render_poses takes them.  voxel is the lattice spacing in world units.  bounds = ((x0, y0, z0), (x1, y1, z1))
    is covered by ceil((x1 - x0) / voxel) + 1 points per axis from (x0, y0, z0); bounds=None renders every frame once more
    beforehand and takes the box of pointcloud.fuse_points over the depths inside depth_range, grown by trunc on every
    side: one more render pass and one more read-back of the box.  trunc=None means 3 * voxel: a convenience, not a measured
    optimum -- it should exceed the depth noise of the scene.  options: depth_range, level, min_weight, max_vertices,
    max_faces, colours (default True), frames_per_call, the keyword-only options of TsdfVolume.extract (min_component_faces,
    min_component_fraction, fill_holes, simplify_cell, smooth_iterations, normals: the chain of steps that the extracted mesh
    goes through, described there; the defaults skip every step) and render_poses' test_frames, frame_indices,
    floater_thresh, chunk.
    A volume above max_bytes raises ValueError before it is allocated and, with bounds given, before anything is rendered.
    depth="median" integrates the median depth of the same frames (depth_quantiles.median_depth: one more render pass per
    batch) instead of render_poses' expected depth, which carves a phantom sheet between two surfaces a ray sees; the colours
    stay render_poses'.  max_spread (with "median" only) also drops the pixels whose interquartile depth range (d75 - d25)
    exceeds max_spread times their median, or that miss one of the three quartiles.  Any other depth= raises ValueError.
    sparse=True fuses into a SparseTsdfVolume instead: the lattice of the box is rounded up to whole 8 x 8 x 8 blocks, one
    render pass touches the blocks the depths reach and allocates them, a second pass integrates every frame into every stored
    block (so that a stored point holds the bits of the dense volume), and bounds=None keeps its box pass in front of those
    two.  The 2^31-point limit of the dense lattice does not apply; max_bytes is checked against marks and table before anything
    is rendered (with bounds given) and against those plus the pools once the block count is known, before the pools are
    allocated.  The faces are those of the dense mesh whose cells lie in stored blocks, in SparseTsdfVolume.extract's order.
    Pinhole scenes only.  Returns the mesh dict of the module docstring with "volume": the TsdfVolume or SparseTsdfVolume."""
    lt = local_tensorfs
    frames = SceneFrames("scene_mesh", lt, W, H, poses, depth, max_spread, options, _MESH_KEYS, False)
    W, H, options = frames.W, frames.H, frames.own
    voxel = check_positive("voxel", float(voxel))
    trunc = check_positive("trunc", 3.0 * voxel if trunc is None else float(trunc))
    if lt.fov == 360:
        raise ValueError("scene_mesh: the integration needs a pinhole camera: there is no reprojection at 360 degrees")
    depth_range = options.get("depth_range", (0.0, math.inf))
    check_range(depth_range)
    level, min_weight = _check_extract(options.get("level", 0.0), options.get("min_weight", 1.0), options.get("max_vertices"),
                                       options.get("max_faces"))
    colours = bool(options.get("colours", True))
    chain = _Chain(options)
    frames.check_per_call("integration")

    def volume_for(lo, dims):                                       # -> origin and dims, or (sparse) blocks
        if sparse:
            blocks = _check_blocks(tuple(-(-d // BLOCK) for d in dims))
            need = SparseTsdfVolume.bytes_for(blocks, 0, colours)
            if need > int(max_bytes):
                raise ValueError(f"scene_mesh: the table of {blocks[0]} x {blocks[1]} x {blocks[2]} blocks takes {need} bytes; "
                                 f"max_bytes is {int(max_bytes)}")
            return lo, blocks
        _check_lattice(lo, voxel, dims)
        need = TsdfVolume.nbytes(dims, colours)
        if need > int(max_bytes):
            raise ValueError(f"scene_mesh: a volume of {dims[0]} x {dims[1]} x {dims[2]} points takes {need} bytes; max_bytes is "
                             f"{int(max_bytes)}")
        return lo, dims

    if bounds is not None:
        if len(bounds) != 2:
            raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)), got {bounds!r}")
        lo, shape = volume_for(*_lattice_of_box(bounds[0], bounds[1], voxel))
    frames.on_device()
    focal, center = frames.focal, frames.center

    def batches():                                                  # every pass renders again: no frame stays resident
        return frames.batches(depth, encode=colours)

    if bounds is None:
        box = None
        for p, _, dmap in batches():
            xyz = pointcloud.fuse_points(None, dmap, p, focal, center, depth_range=depth_range)["xyz"]
            if xyz.shape[0]:
                cur = torch.stack([xyz.amin(0), -xyz.amax(0)])
                box = cur if box is None else torch.minimum(box, cur)
        if box is None:
            raise ValueError("scene_mesh: no rendered depth lies inside depth_range; there is no box to cover")
        box = box.double().cpu().numpy()                            # the box's read-back
        lo, shape = volume_for(*_lattice_of_box(box[0] - trunc, -box[1] + trunc, voxel))
    if sparse:
        vol = SparseTsdfVolume(lo, voxel, shape, trunc, lt.blending_weights.device, colours=colours)
        for p, _, dmap in batches():
            vol.touch(dmap, p, focal, center, depth_range=depth_range)
        vol.allocate(max_bytes=max_bytes)
    else:
        vol = TsdfVolume(lo, voxel, shape, trunc, lt.blending_weights.device, colours=colours)
    for p, out, dmap in batches():
        vol.integrate(dmap, p, focal, center, rgb=out["rgb8"] if colours else None, depth_range=depth_range)
    mesh = vol.extract(level, min_weight, options.get("max_vertices"), options.get("max_faces"), **chain.options)
    mesh["volume"] = vol
    return mesh
