"""Shared pieces of the block-sparse TSDF tests: the numpy fp32 restatement of csrc/lrf_tsdf_blocks.inl (touch, assign, the
integration over stored blocks and the marching tetrahedra over the pools, same operation order as the kernels) and the
cases.  Everything is float32 arithmetic on float32 arrays; Python numbers only appear as weak scalars."""
import functools

import numpy as np

from mesh_cases import (CASE_E, CASE_N, TET_D, TET_LO, _shift, _shift_back, integrate_host, lattice, tet_corners)
from novel_views_cases import rgb8_host
from points_cases import pixel_dirs, random_case, trajectory_case, world_points

F32 = np.float32
BLOCK = 8


# ------------------------------------------------------------------------------------------------ the volume
def new_sparse(origin, voxel, blocks, trunc, colours=True):
    Bx, By, Bz = blocks
    return {"origin": tuple(origin), "voxel": voxel, "blocks": tuple(blocks), "trunc": trunc,
            "marks": np.zeros((Bz, By, Bx), np.uint8), "table": np.full((Bz, By, Bx), -1, np.int32),
            "coords": np.zeros((0, 3), np.int32), "tsdf": np.ones((0, 8, 8, 8), F32), "weight": np.zeros((0, 8, 8, 8), F32),
            "rgb": np.zeros((0, 8, 8, 8, 3), F32) if colours else None}


def dims_of(blocks):
    return tuple(BLOCK * b for b in blocks)


# ------------------------------------------------------------------------------------------------ touch
def touch_host(sv, depth, c2w, f, cx, cy, depth_range=(0.0, np.inf)):
    """k_blocks_touch on the host, in place on sv["marks"].  -> the largest number of blocks one pixel marked"""
    depth, c2w = np.asarray(depth, F32), np.asarray(c2w, F32)
    V, H, W = depth.shape
    Bx, By, Bz = sv["blocks"]
    lo_r, hi_r, tr, h = F32(depth_range[0]), F32(depth_range[1]), F32(sv["trunc"]), F32(sv["voxel"])
    o = np.asarray(sv["origin"], F32)
    fo = F32(f)
    dirs = pixel_dirs(H, W, f, cx, cy)
    with np.errstate(all="ignore"):
        ok = np.isfinite(depth) & (depth > 0) & (depth >= lo_r) & (depth <= hi_r)
        da = np.fmax(depth - tr, F32(0)).astype(F32)
        db = (depth + tr).astype(F32)
        pa, pb = world_points(da, c2w, dirs), world_points(db, c2w, dirs)
        m = (h + db / fo).astype(F32)
        bs = F32(8) * h
        first, last = [], []
        for k, B in enumerate((Bx, By, Bz)):
            l = (np.fmin(pa[..., k], pb[..., k]) - m).astype(F32)
            hh = (np.fmax(pa[..., k], pb[..., k]) + m).astype(F32)
            ok &= l <= hh
            fl = np.fmax(np.floor((l - o[k]) / bs), F32(0)).astype(F32)
            fh = np.fmin(np.floor((hh - o[k]) / bs), F32(B - 1)).astype(F32)
            ok &= fl <= fh
            first.append(np.where(ok, fl, 0).astype(np.int64))
            last.append(np.minimum(np.where(ok, fh, 0).astype(np.int64), B - 1))
    most = 0
    marks = sv["marks"]
    for v, j, i in zip(*np.nonzero(ok)):
        x0, x1, y0, y1, z0, z1 = first[0][v, j, i], last[0][v, j, i], first[1][v, j, i], last[1][v, j, i], first[2][v, j, i], last[2][v, j, i]
        marks[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 1
        most = max(most, int((x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1)))
    return most


# ------------------------------------------------------------------------------------------------ assign
def assign_host(sv, max_blocks=(1 << 22) - 1):
    """lrf_tsdf_blocks_assign and SparseTsdfVolume.allocate on the host: the marked blocks without an index get the next ones in
    block-linear (z, y, x) order; the pools grow (tsdf 1, weight 0, rgb 0).  -> the number of new blocks"""
    fresh = (sv["marks"] != 0) & (sv["table"] < 0)
    bz, by, bx = np.nonzero(fresh)                                  # C order: (z, y, x)
    n0, new = sv["coords"].shape[0], int(fresh.sum())
    if n0 + new > max_blocks:
        return new
    sv["table"][bz, by, bx] = n0 + np.arange(new, dtype=np.int32)
    sv["coords"] = np.concatenate([sv["coords"], np.stack([bx, by, bz], -1).astype(np.int32)])
    sv["tsdf"] = np.concatenate([sv["tsdf"], np.ones((new, 8, 8, 8), F32)])
    sv["weight"] = np.concatenate([sv["weight"], np.zeros((new, 8, 8, 8), F32)])
    if sv["rgb"] is not None:
        sv["rgb"] = np.concatenate([sv["rgb"], np.zeros((new, 8, 8, 8, 3), F32)])
    return new


# ------------------------------------------------------------------------------------------------ pools <-> lattice
def to_dense_host(sv):
    """-> dict(tsdf, weight, rgb, stored) over the virtual lattice [8Bz,8By,8Bx]; a point in no block holds (1, 0, 0)."""
    Bx, By, Bz = sv["blocks"]
    bx, by, bz = sv["coords"][:, 0], sv["coords"][:, 1], sv["coords"][:, 2]

    def scatter(pool, fill, tail=()):
        out = np.full((Bz, By, Bx, 8, 8, 8) + tail, fill, pool.dtype)
        out[bz, by, bx] = pool
        order = (0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(tail)))
        return np.ascontiguousarray(out.transpose(order)).reshape((8 * Bz, 8 * By, 8 * Bx) + tail)
    n = sv["coords"].shape[0]
    return {"tsdf": scatter(sv["tsdf"], 1.0), "weight": scatter(sv["weight"], 0.0),
            "rgb": None if sv["rgb"] is None else scatter(sv["rgb"], 0.0, (3,)), "stored": scatter(np.ones((n, 8, 8, 8), bool), False)}


def _gather(sv, dense, tail=()):
    Bx, By, Bz = sv["blocks"]
    order = (0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(tail)))
    cube = dense.reshape((Bz, 8, By, 8, Bx, 8) + tail).transpose(order)
    return np.ascontiguousarray(cube[sv["coords"][:, 2], sv["coords"][:, 1], sv["coords"][:, 0]])


def integrate_blocks_host(sv, depth, rgb8, c2w, f, cx, cy, depth_range=(0.0, np.inf)):
    """k_blocks_fuse on the host: k_tsdf_integrate's restatement on the virtual lattice, kept for the stored points only."""
    if not sv["coords"].shape[0]:
        return sv
    d = to_dense_host(sv)
    vol = {"tsdf": d["tsdf"], "weight": d["weight"], "rgb": d["rgb"]}
    integrate_host(vol, sv["origin"], sv["voxel"], sv["trunc"], depth, rgb8, c2w, f, cx, cy, depth_range=depth_range)
    sv["tsdf"], sv["weight"] = _gather(sv, vol["tsdf"]), _gather(sv, vol["weight"])
    if sv["rgb"] is not None:
        sv["rgb"] = _gather(sv, vol["rgb"], (3,))
    return sv


# ------------------------------------------------------------------------------------------------ extraction
def extract_blocks_host(sv, level=0.0, min_weight=1.0):
    """lrf_mesh_extract_blocks on the host: the marching tetrahedra of mesh_cases.extract_host on the virtual lattice with the
    points of no block at (tsdf 1, weight 0), vertices in pool order then (z, y, x, edge), faces in the pool order of the
    cell's lowest corner then (tetrahedron, triangle).  -> the mesh dict, with "cells" [Nf,3]: each face's cell (x, y, z)"""
    d = to_dense_host(sv)
    value, weight, rgb = d["tsdf"], d["weight"], d["rgb"]
    Nz, Ny, Nx = value.shape
    lev = F32(level)
    with np.errstate(invalid="ignore"):
        inside = value < lev
        okpt = weight >= F32(min_weight)
    assert not (okpt & ~d["stored"]).any()
    cell = okpt.copy()
    for c in range(1, 8):
        cell &= _shift(okpt, c, False)
    exist = np.zeros((Nz, Ny, Nx, 7), bool)
    for e in range(7):
        dd = e + 1
        free = ~dd & 7
        anyc = np.zeros(value.shape, bool)
        for s in range(8):
            if s & ~free:
                continue
            anyc |= _shift_back(cell, s, False)
        exist[..., e] = (inside != _shift(inside, dd, False)) & _shift(np.ones(value.shape, bool), dd, False) & anyc
    zz, yy, xx = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    blk = sv["table"].astype(np.int64)[zz >> 3, yy >> 3, xx >> 3]
    rank = blk * 512 + ((zz & 7) << 6 | (yy & 7) << 3 | (xx & 7))      # the pool index of a lattice point (< 0: in no block)
    iz, iy, ix, e = np.nonzero(exist)
    assert (blk[iz, iy, ix] >= 0).all()
    order = np.argsort(rank[iz, iy, ix] * 8 + e, kind="stable")
    iz, iy, ix, e = iz[order], iy[order], ix[order], e[order]
    vid = np.full(exist.shape, -1, np.int64)
    vid[iz, iy, ix, e] = np.arange(e.size)
    dd = e + 1
    pts = lattice(sv["origin"], sv["voxel"], (Nx + 1, Ny + 1, Nz + 1))
    pa = pts[iz, iy, ix]
    jz, jy, jx = iz + ((dd >> 2) & 1), iy + ((dd >> 1) & 1), ix + (dd & 1)
    pb = pts[jz, jy, jx]
    va, vb = value[iz, iy, ix], value[jz, jy, jx]
    with np.errstate(all="ignore"):
        t = ((lev - va) / (vb - va)).astype(F32)
        verts = (pa + t[:, None] * (pb - pa)).astype(F32).reshape(-1, 3)
        rgb8 = None
        if rgb is not None:
            ca, cb = rgb[iz, iy, ix], rgb[jz, jy, jx]
            rgb8 = rgb8_host((ca + t[:, None] * (cb - ca)).astype(F32)).reshape(-1, 3)
    bits = np.zeros(value.shape, np.int64)
    for c in range(8):
        bits |= _shift(inside, c, False).astype(np.int64) << c
    cz, cy_, cx_ = np.nonzero(cell)
    assert (blk[cz, cy_, cx_] >= 0).all()
    order = np.argsort(rank[cz, cy_, cx_], kind="stable")
    cz, cy_, cx_ = cz[order], cy_[order], cx_[order]
    cm = bits[cz, cy_, cx_]
    out = np.full((cm.size, 6, 2, 3), -1, np.int64)
    for tt in range(6):
        cs = tet_corners(tt)
        m = sum(((cm >> cs[k]) & 1) << k for k in range(4))
        for j in range(2):
            has = CASE_N[m] > j
            for k in range(3):
                ek = CASE_E[m, j, k]
                lo, dr = TET_LO[tt][ek], TET_D[tt][ek]
                oz, oy, ox = cz + ((lo >> 2) & 1), cy_ + ((lo >> 1) & 1), cx_ + (lo & 1)
                out[:, tt, j, k] = np.where(has, vid[oz, oy, ox, dr - 1], -1)
                assert (vid[oz, oy, ox, dr - 1][has] >= 0).all()
    faces = out.reshape(-1, 3)
    cells = np.repeat(np.stack([cx_, cy_, cz], -1), 12, axis=0)
    keep = faces[:, 0] >= 0
    return {"vertices": verts, "faces": faces[keep].astype(np.int32), "rgb8": rgb8, "cells": cells[keep],
            "counts": (int(verts.shape[0]), int(keep.sum()))}


def face_keys(mesh):
    """The faces as a set, each keyed by the nine words of its three vertex positions."""
    v = np.ascontiguousarray(np.asarray(mesh["vertices"], F32)).view(np.uint32)
    f = np.asarray(mesh["faces"], np.int64)
    return {tuple(row) for row in v[f].reshape(-1, 9).tolist()}


# ------------------------------------------------------------------------------------------------ cases
def lattice_for(blocks, voxel, centre, trunc_voxels=3.0):
    """(origin, voxel, trunc): the lattice of 8 * blocks points centred on `centre`."""
    dims = np.array(dims_of(blocks))
    origin = np.asarray(centre, np.float64) - (dims - 1) / 2 * voxel
    return tuple(float(v) for v in origin), float(voxel), trunc_voxels * float(voxel)


def spread_lattice(blocks, centre=(0.1, -0.05, -3.05), extent=1.7):
    """The lattice tests/test_gpu_mesh.py's _lattice_for gives dims = 8 * blocks."""
    dims = dims_of(blocks)
    return lattice_for(blocks, extent / max(max(dims) - 1, 1), centre)


@functools.lru_cache(maxsize=None)
def trajectory(clean):
    """trajectory_case() with its ray-cast depth (clean) or with the planted floaters."""
    c = dict(trajectory_case())
    if clean:
        c["depth"] = c["clean"]
    return c


@functools.lru_cache(maxsize=None)
def random_frames(V, H, W, inside=False):
    """random_case(1000 V + H, V, H, W); inside: the last frame stands inside the volumes, turned 2 rad about y."""
    c = random_case(1000 * V + H, V, H, W)
    if inside:
        a = 2.0
        c["c2w"][-1] = np.array([[np.cos(a), 0, np.sin(a), 0.0], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), -3.0]], F32)
    return c


def fuse_host(blocks, lat, case, depth_range=(0.0, np.inf), colours=True):
    """touch, assign and integrate on the host over all frames of the case -> (sv, most blocks one pixel marked)."""
    origin, voxel, trunc = lat
    sv = new_sparse(origin, voxel, blocks, trunc, colours)
    most = touch_host(sv, case["depth"], case["c2w"], case["f"], case["cx"], case["cy"], depth_range)
    assign_host(sv)
    integrate_blocks_host(sv, case["depth"], case["rgb8"] if colours else None, case["c2w"], case["f"], case["cx"], case["cy"],
                          depth_range)
    return sv, most
