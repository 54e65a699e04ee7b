"""Shared pieces of the mesh-cleaning tests: the numpy restatement of csrc/lrf_mesh_clean.inl -- min-index component labels by
a plain union-find, the per-component counts, the threshold and the ordered filter -- and the test meshes: marching-tetrahedra
meshes of analytic fields on the 24^3 lattice (mesh_cases.extract_host) and hand-made ones.  Integers only; vertices and
colours are moved, never recomputed."""
import functools
import math

import numpy as np

from mesh_cases import H_ANALYTIC, analytic_lattice, extract_host, sphere_field, torus_field

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def labels_host(faces, n_vertices):
    """labels[v] = the smallest vertex index of v's component: a plain union-find that always keeps the smaller root."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    return np.array([find(v) for v in range(n_vertices)], np.int32).reshape(n_vertices)


def labels_host_arrays(faces, n_vertices):
    """The same labels by whole-array steps (for meshes too large for the loop above): every face pulls the labels of its
    three vertices down to their minimum, then every label jumps to its label's label, until nothing moves.  Labels only
    decrease and stay inside the component, so the fixed point is the component's smallest index."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.arange(n_vertices, dtype=np.int64)
    while True:
        before = lab.copy()
        if f.shape[0]:
            m = lab[f].min(1)
            for k in range(3):
                np.minimum.at(lab, lab[f[:, k]], m)
                np.minimum.at(lab, f[:, k], m)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, before):
            return lab.astype(np.int32)


def labels_bfs(faces, n_vertices):
    """Brute force: a breadth-first search from every unvisited vertex in index order."""
    adj = [set() for _ in range(n_vertices)]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        adj[a].update((b, c)); adj[b].update((a, c)); adj[c].update((a, b))
    lab = [-1] * n_vertices
    for s in range(n_vertices):
        if lab[s] >= 0:
            continue
        lab[s] = s
        todo = [s]
        while todo:
            nxt = []
            for v in todo:
                for w in adj[v]:
                    if lab[w] < 0:
                        lab[w] = s
                        nxt.append(w)
            todo = nxt
    return np.array(lab, np.int32).reshape(n_vertices)


def counts_host(labels, faces, n_vertices):
    """-> faces_of, vertices_of ([Nv] int32, at the label, 0 elsewhere) and (n_components, n_with_faces, largest_faces)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    faces_of = np.bincount(labels[f[:, 0]], minlength=n_vertices).astype(np.int32)
    vertices_of = np.bincount(labels, minlength=n_vertices).astype(np.int32)
    roots = labels == np.arange(n_vertices)
    summary = (int(roots.sum()), int((faces_of[roots] > 0).sum()), int(faces_of.max()) if n_vertices else 0)
    return faces_of, vertices_of, summary


def components_host(mesh, big=False):
    nv = mesh["vertices"].shape[0]
    labels = (labels_host_arrays if big else labels_host)(mesh["faces"], nv)
    faces_of, vertices_of, (n, nw, largest) = counts_host(labels, mesh["faces"], nv)
    return {"labels": labels, "faces_of": faces_of, "vertices_of": vertices_of, "n_components": n, "n_with_faces": nw,
            "largest_faces": largest}


def threshold_host(min_faces, min_fraction, largest_faces):
    return max(int(min_faces), int(math.ceil(min_fraction * largest_faces)))


def filter_host(mesh, comp, threshold):
    """The ordered filter: components with faces_of >= threshold stay, kept vertices are renumbered by rank -> (mesh, kept)."""
    v, f, c = mesh["vertices"], mesh["faces"], mesh["rgb8"]
    keep_label = comp["faces_of"] >= threshold
    keep_v = keep_label[comp["labels"]]
    keep_f = keep_label[comp["labels"][f[:, 0]]] if f.shape[0] else np.zeros(0, bool)
    remap = (np.cumsum(keep_v) - 1).astype(np.int32)
    out = {"vertices": v[keep_v], "faces": remap[f[keep_f]].reshape(-1, 3).astype(np.int32), "rgb8": None if c is None else c[keep_v]}
    out["counts"] = (int(out["vertices"].shape[0]), int(out["faces"].shape[0]))
    kept = int((keep_label & (comp["labels"] == np.arange(v.shape[0]))).sum())
    return out, kept


# ------------------------------------------------------------------------------------------------ the meshes
BLOBS = (((0.50, 0.50, 0.50), 0.27), ((0.14, 0.15, 0.16), 0.09), ((0.86, 0.16, 0.85), 0.07), ((0.15, 0.86, 0.84), 0.055),
         ((0.85, 0.85, 0.15), 0.10), ((0.50, 0.91, 0.50), 0.045))
BLOB_FACES = (4200, 600, 476, 272, 144, 88)


def blobs_field():
    """The minimum of six sphere distances on the 24^3 lattice of the unit cube, fp32: six closed shells."""
    p = analytic_lattice()
    d = [np.sqrt(((p - np.array(c)) ** 2).sum(-1)) - r for c, r in BLOBS]
    return np.minimum.reduce(d).astype(F32)


def _mesh(fld, weight=None, seed=0):
    m = extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC, weight=weight)
    m["rgb8"] = np.random.default_rng(100 + seed).integers(0, 256, m["vertices"].shape, dtype=np.uint8)
    return m


def _made(vertices, faces, seed):
    nv = int(vertices)
    rng = np.random.default_rng(200 + seed)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    return {"vertices": rng.standard_normal((nv, 3)).astype(F32), "faces": f,
            "rgb8": rng.integers(0, 256, (nv, 3), dtype=np.uint8), "counts": (nv, int(f.shape[0]))}


def with_strays(mesh, at=(0, 1000, -1), seed=7):
    """The mesh with vertices that no face holds inserted before rows `at` (-1: appended)."""
    v, c, f = mesh["vertices"], mesh["rgb8"], mesh["faces"].astype(np.int64)
    nv = v.shape[0]
    pos = sorted(nv if a < 0 else min(a, nv) for a in at)
    rng = np.random.default_rng(seed)
    shift = np.searchsorted(np.array(pos), np.arange(nv), side="right")       # strays before each old vertex
    v2 = np.insert(v, pos, rng.standard_normal((len(pos), 3)).astype(F32), axis=0)
    c2 = np.insert(c, pos, rng.integers(0, 256, (len(pos), 3), dtype=np.uint8), axis=0)
    f2 = (f + shift[f]).astype(np.int32)
    return {"vertices": v2, "faces": f2, "rgb8": c2, "counts": (int(v2.shape[0]), int(f2.shape[0]))}


def fan(nv, seed=0):
    """Vertex 0 and the faces (0, i, i + 1): one component of nv - 2 faces."""
    i = np.arange(1, nv - 1, dtype=np.int32)
    return _made(nv, np.stack([np.zeros_like(i), i, i + 1], 1), seed)


def strip(n=20000):
    """A 2 x n strip in lattice order (vertex 2 i + j), both diagonal splits of every cell: 2 n vertices, 4 (n - 1) faces.  The
    first hooking pass leaves one parent chain through every vertex."""
    i = 2 * np.arange(n - 1, dtype=np.int32)
    a, b, c, d = i, i + 1, i + 2, i + 3
    return _made(2 * n, np.stack([np.stack(t, 1) for t in ((a, b, c), (b, d, c), (a, b, d), (a, d, c))], 1).reshape(-1, 3), 3)


def permute_vertices(mesh, seed):
    """Old vertex v becomes vertex p[v]; the faces keep their order."""
    nv = mesh["vertices"].shape[0]
    p = np.random.default_rng(seed).permutation(nv).astype(np.int32)
    inv = np.argsort(p)
    return {"vertices": mesh["vertices"][inv], "faces": p[mesh["faces"]].reshape(-1, 3).astype(np.int32),
            "rgb8": None if mesh["rgb8"] is None else mesh["rgb8"][inv], "counts": mesh["counts"]}


def permute_faces(mesh, seed):
    q = np.random.default_rng(seed).permutation(mesh["faces"].shape[0])
    return dict(mesh, faces=np.ascontiguousarray(mesh["faces"][q]))


@functools.lru_cache(maxsize=None)
def base_meshes():
    """name -> mesh, in a fixed order."""
    blobs = blobs_field()
    tie_w = np.ones_like(blobs)
    tie_w[:, :, 11:13] = 0                                          # the lattice columns x = 11, 12: the big shell falls in two
    noise_w = (np.random.default_rng(5).random(blobs.shape) >= 0.08).astype(F32)
    out = {
        "sphere": _mesh(sphere_field(), seed=1),
        "torus": _mesh(torus_field(), seed=2),
        "blobs": _mesh(blobs, seed=3),
        "blobs tie": _mesh(blobs, tie_w, seed=4),
        "blobs noise": _mesh(blobs, noise_w, seed=5),
        "one vertex": _made(1, np.zeros((0, 3), np.int32), 0),
        "one triangle": _made(3, [(0, 1, 2)], 1),
        "two triangles": _made(5, [(2, 3, 4), (0, 1, 2)], 2),
        "strip": strip(),
    }
    out["blobs strays"] = with_strays(out["blobs"])
    out["strip permuted"] = permute_vertices(out["strip"], 11)
    return out


@functools.lru_cache(maxsize=None)
def all_meshes():
    """Every base mesh, and each under a seeded vertex permutation and a seeded face permutation."""
    out = {}
    for k, (name, m) in enumerate(base_meshes().items()):
        out[name] = m
        out[name + " / vertices permuted"] = permute_vertices(m, 1000 + k)
        out[name + " / faces permuted"] = permute_faces(m, 2000 + k)
    return out


MESH_NAMES = tuple(n + s for n in ("sphere", "torus", "blobs", "blobs tie", "blobs noise", "one vertex", "one triangle",
                                   "two triangles", "strip", "blobs strays", "strip permuted")
                   for s in ("", " / vertices permuted", " / faces permuted"))
FANS = (3, 63, 64, 65, 255, 257, 1025)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's components of all_meshes()[name], computed once and shared."""
    return components_host(all_meshes()[name])
