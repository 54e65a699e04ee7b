"""Shared pieces of the mesh-simplification tests: the numpy restatement of csrc/lrf_mesh_simplify.inl by another algorithm --
float64 array arithmetic for the cells, np.unique for the clusters and for the duplicate keys, np.add.at for the integer sums;
no bit words, no scan, no table -- and the cases: the analytic meshes of tests/mesh_clean_cases.py at several cell sizes and
anchors, shifted and permuted, and hand-made meshes for the edges of the algorithm."""
import functools

import numpy as np

from mesh_cases import H_ANALYTIC
from mesh_clean_cases import (base_meshes, expected, fan, filter_host, permute_faces, permute_vertices, strip)

F32 = np.float32
Q_ONE = 4294967296.0                                                # 2^32


# ------------------------------------------------------------------------------------------------ the restatement
def cells_host(vertices, cell, origin):
    """Item 1 -> (i [Nv,3] int64, q [Nv,3] uint64, bad [Nv] bool)."""
    t = (vertices.astype(np.float64) - np.asarray(origin, np.float64)) / np.float64(cell)
    with np.errstate(invalid="ignore"):
        fl = np.floor(t)
        bad = ~(np.abs(fl) < 2.0 ** 30).all(1)
        fl = np.where(bad[:, None], 0.0, fl)
        q = ((np.where(bad[:, None], 0.0, t) - fl) * Q_ONE).astype(np.uint64)
    return fl.astype(np.int64), q, bad


def canonical(tri):
    """Rows of three distinct integers rotated so that the smallest comes first: the winding stays."""
    tri = np.asarray(tri).reshape(-1, 3)
    k = tri.argmin(1)
    rows = np.arange(tri.shape[0])
    return np.stack([tri[rows, k], tri[rows, (k + 1) % 3], tri[rows, (k + 2) % 3]], 1)


def simplify_host(mesh, cell, origin=(0.0, 0.0, 0.0), dedupe=True):
    """-> dict: vertices [n,3] fp32, rgb8 [n,3] uint8 or None, faces [m,3] int32, counts = (vertices out, faces out, occupied
    cells, degenerate faces, duplicate faces), box = (lo, dims), cells [n,3] int64 (the cell of every emitted vertex)."""
    v, f, c = mesh["vertices"], np.asarray(mesh["faces"], np.int64).reshape(-1, 3), mesh.get("rgb8")
    nv = v.shape[0]
    empty = {"vertices": np.zeros((0, 3), F32), "rgb8": None if c is None else np.zeros((0, 3), np.uint8),
             "faces": np.zeros((0, 3), np.int32)}
    if nv == 0:
        return dict(empty, counts=(0, 0, 0, 0, 0), box=((0, 0, 0), (0, 0, 0)), cells=np.zeros((0, 3), np.int64))
    i, q, bad = cells_host(v, cell, origin)
    assert not bad.any(), "a bad vertex: simplify raises"
    lo = i.min(0)
    dims = i.max(0) - lo + 1
    rel = i - lo
    linear = (rel[:, 2] * dims[1] + rel[:, 1]) * dims[0] + rel[:, 0]
    occupied, cluster_of = np.unique(linear, return_inverse=True)   # clusters in increasing linear cell index
    cluster_of = cluster_of.reshape(-1)
    nc = occupied.size
    box = (tuple(int(x) for x in lo), tuple(int(x) for x in dims))
    # faces
    g = cluster_of[f]
    degenerate = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    index = np.nonzero(~degenerate)[0]
    keys = canonical(g[index])
    if dedupe and keys.shape[0]:
        _, first = np.unique(keys, axis=0, return_index=True)       # the first occurrence: the smallest input face index
        first = np.sort(first)
        keys, n_dup = keys[first], index.size - first.size
    else:
        n_dup = 0
    used = np.unique(keys.reshape(-1))                              # emitted clusters, in cluster order
    faces = np.searchsorted(used, keys).astype(np.int32).reshape(-1, 3)
    # representatives
    S = np.zeros((nc, 3), np.uint64)
    np.add.at(S, cluster_of, q)
    n = np.bincount(cluster_of, minlength=nc)
    ci = np.stack([occupied % dims[0], occupied // dims[0] % dims[1], occupied // (dims[0] * dims[1])], 1) + lo
    mean = S.astype(np.float64) / n.astype(np.float64)[:, None]
    frac = mean * (1.0 / Q_ONE)
    t = ci.astype(np.float64) + frac
    x = t * np.float64(cell)
    pos = (np.asarray(origin, np.float64) + x).astype(F32)
    rgb = None
    if c is not None:
        C = np.zeros((nc, 3), np.int64)
        np.add.at(C, cluster_of, c.astype(np.int64))
        rgb = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)[used]
    return {"vertices": np.ascontiguousarray(pos[used]), "rgb8": rgb, "faces": faces,
            "counts": (int(used.size), int(faces.shape[0]), int(nc), int(degenerate.sum()), int(n_dup)), "box": box,
            "cells": ci[used]}


def face_keys(faces):
    """The canonical triples of the faces, as a sorted list of tuples."""
    return sorted(map(tuple, canonical(faces).tolist()))


# ------------------------------------------------------------------------------------------------ the meshes
SHIFT = np.array([1.5, 2.25, 1.125], F32)                           # exact in fp32; the unit cube becomes negative
STEPS = (2.0, 3.5, 9.0)                                             # cell edges in lattice steps
ANALYTIC = ("sphere", "torus", "blobs")


def _mesh(vertices, faces, seed, rgb=True):
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    rgb8 = np.random.default_rng(300 + seed).integers(0, 256, v.shape, dtype=np.uint8) if rgb else None
    return {"vertices": v, "faces": f, "rgb8": rgb8, "counts": (int(v.shape[0]), int(f.shape[0]))}


def shifted(mesh):
    return dict(mesh, vertices=(mesh["vertices"] - SHIFT).astype(F32))


@functools.lru_cache(maxsize=None)
def smallest_blob():
    """The smallest shell of the blobs (88 faces), as a mesh of its own."""
    m, comp = base_meshes()["blobs"], expected("blobs")
    out, kept = filter_host(m, dict(comp, faces_of=np.where(comp["faces_of"] == 88, 88, 0).astype(np.int32)), 88)
    assert kept == 1 and out["counts"][1] == 88
    return out


def lattice_points(seed=1, nv=400, nf=700):
    """Integer coordinates: with cell = 1 every vertex lies exactly on a cell boundary (q = 0)."""
    rng = np.random.default_rng(seed)
    return _mesh(rng.integers(-5, 6, (nv, 3)), rng.integers(0, nv, (nf, 3)), seed)


def fan_in_one_cell(nv=100000):
    """A fan over nv vertices that share the cell [0, 1)^3 (all of its faces degenerate), and one face from vertex 0 to two
    vertices in other cells, so that the big cluster is emitted: its sums run over nv vertices."""
    rng = np.random.default_rng(21)
    f = fan(nv)["faces"]
    v = np.concatenate([rng.random((nv, 3)) * 0.999, [[1.5, 0.25, 0.5], [0.25, 1.5, 0.5]]])
    return _mesh(v, np.concatenate([f, [[0, nv, nv + 1]]]), 21)


def copies(n=100000):
    """n copies of one triangle, cycling through its three rotations, and its mirror image twice among them."""
    v = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5]])
    rot = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])
    f = rot[np.arange(n) % 3]
    f = np.insert(f, [7, n - 1], [[2, 1, 0], [0, 2, 1]], axis=0)
    return _mesh(v, f, 22)


def sparse_box(n=3000):
    """n small triangles spread over a box of 128 x 128 x 80 unit cells: more than 2^20 cells, so the cells' ordered scan takes
    a second step.  The first two triangles pin the corners of the box."""
    rng = np.random.default_rng(23)
    size = np.array([128.0, 128.0, 80.0])
    base = rng.random((n, 1, 3)) * (size - 3.0)
    base[0], base[1] = 0.0, size - 3.0
    v = (base + rng.random((n, 3, 3)) * 2.999).reshape(-1, 3)
    return _mesh(v, np.arange(3 * n).reshape(n, 3), 23)


def _hand_made():
    tri = _mesh([[0.2, 0.3, 0.1], [1.4, 0.2, 0.3], [0.3, 1.6, -0.7]], [(0, 1, 2)], 31)
    inside = _mesh([[0.1, 0.2, 0.3], [0.8, 0.2, 0.4], [0.5, 0.9, 0.1], [0.4, 0.1, 0.9]], [(0, 1, 2), (1, 0, 3)], 32)
    out = {
        "alone": (smallest_blob(), H_ANALYTIC / 64, (0.0, 0.0, 0.0)),
        "lattice points": (lattice_points(), 1.0, (0.0, 0.0, 0.0)),
        "one triangle": (tri, 1.0, (0.0, 0.0, 0.0)),
        "one triangle in one cell": (tri, 8.0, (-4.0, -4.0, -4.0)),
        "one vertex": (_mesh([[0.3, -0.2, 7.0]], np.zeros((0, 3)), 33), 0.5, (0.0, 0.0, 0.0)),
        "two triangles in one cell": (inside, 1.0, (0.0, 0.0, 0.0)),
        "fan in one cell": (fan_in_one_cell(), 1.0, (0.0, 0.0, 0.0)),
        "copies": (copies(), 1.0, (0.0, 0.0, 0.0)),
        "strip": (strip(), 3.0, (0.0, 0.0, 0.0)),
        "sparse box": (sparse_box(), 1.0, (0.0, 0.0, 0.0)),
    }
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (mesh with rgb8, cell, origin), in a fixed order."""
    out = {}
    k = 0
    for name in ANALYTIC:
        for shift in (False, True):
            m = shifted(base_meshes()[name]) if shift else base_meshes()[name]
            lattice_origin = tuple(float(-x) for x in SHIFT) if shift else (0.0, 0.0, 0.0)
            origins = ((0.0, 0.0, 0.0), (0.1, -0.03, 0.017)) + ((lattice_origin,) if shift else ())
            for steps in STEPS:
                for origin in origins:
                    tag = f"{name}{' shifted' if shift else ''} / {steps:g} steps / origin {origin[0]:g}"
                    k += 1
                    out[tag] = (m, steps * H_ANALYTIC, origin)
                    out[tag + " / vertices permuted"] = (permute_vertices(m, 3000 + k), steps * H_ANALYTIC, origin)
                    out[tag + " / faces permuted"] = (permute_faces(m, 4000 + k), steps * H_ANALYTIC, origin)
    out.update(_hand_made())
    return out


def _names():
    out = []
    for name in ANALYTIC:
        for shift in (False, True):
            for steps in STEPS:
                for o in ("0", "0.1") + (("-1.5",) if shift else ()):
                    tag = f"{name}{' shifted' if shift else ''} / {steps:g} steps / origin {o}"
                    out += [tag, tag + " / vertices permuted", tag + " / faces permuted"]
    return tuple(out) + ("alone", "lattice points", "one triangle", "one triangle in one cell", "one vertex",
                         "two triangles in one cell", "fan in one cell", "copies", "strip", "sparse box")


CASE_NAMES = _names()
BIG = ("fan in one cell", "copies", "strip", "sparse box")


@functools.lru_cache(maxsize=None)
def expected_simplified(name, rgb=True, dedupe=True):
    """The restatement's result for cases()[name], computed once and shared."""
    m, cell, origin = cases()[name]
    return simplify_host(m if rgb else dict(m, rgb8=None), cell, origin, dedupe)
