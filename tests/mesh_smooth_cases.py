"""Shared pieces of the mesh-smoothing tests: the numpy restatement of csrc/lrf_mesh_smooth.inl by another algorithm -- np.unique
with counts on a Nv + b keys for the edges, np.add.at over face corners into int64 for the integer sums, float64 array arithmetic
in exactly the stated order; no incidence lists, no row scans -- and the cases: the analytic meshes of tests/mesh_clean_cases.py
plain, permuted and shifted, a simplified sphere, and hand-made meshes for the edges of the algorithm.

Which smoothing arguments run on which case (SMOOTH_FULL, SMOOTH_LIGHT, SMOOTH_FAN): every value of iterations (0, 1, 3, 10), of
(lam, mu) and of boundary, crossed, on the base meshes and the hand-made ones; three argument sets that still hold every (lam,
mu) and both boundary modes on the permuted and shifted copies, whose point is the order and the offset, not the arguments;
iterations=2 on the 100 000-vertex fan.  A trajectory is computed once and read at 1, 3 and 10 iterations."""
import functools

import numpy as np

from mesh_cases import H_ANALYTIC, SPHERE_C
from mesh_clean_cases import FANS, base_meshes, fan, permute_faces, permute_vertices
from mesh_simplify_cases import SHIFT, simplify_host

F32 = np.float32
E_NONE = -(1 << 31)
Q_LIMIT = 2.0 ** 41
FAR = np.array([1000.0, -2000.0, 500.0], F32)


# ------------------------------------------------------------------------------------------------ the restatement
def valid_faces(mesh):
    """-> (the faces without the degenerate ones [n,3] int64, the number of degenerate faces)."""
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    nv = mesh["vertices"].shape[0]
    assert ((f >= 0) & (f < nv)).all(), "a bad face index: every call raises"
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    return f[~degenerate], int(degenerate.sum())


def topology_host(mesh):
    """Item 2 -> dict: boundary_edges, nonmanifold_edges, degenerate_faces, closed, boundary_vertices [Nv] uint8."""
    f, degenerate = valid_faces(mesh)
    nv = mesh["vertices"].shape[0]
    a, b = f.reshape(-1), f[:, (1, 2, 0)].reshape(-1)
    mask = np.zeros(nv, np.uint8)
    if a.size == 0:
        return {"boundary_edges": 0, "nonmanifold_edges": 0, "degenerate_faces": degenerate, "closed": True, "boundary_vertices": mask}
    keys, counts = np.unique(a * nv + b, return_counts=True)

    def count_of(k):
        at = np.minimum(np.searchsorted(keys, k), keys.size - 1)
        return np.where(keys[at] == k, counts[at], 0)
    same, opp = count_of(a * nv + b) - 1, count_of(b * nv + a)
    boundary, nonmanifold = opp == 0, (same > 0) | (opp > 1)
    mask[a[boundary]] = 1
    mask[b[boundary]] = 1
    nb, nn = int(boundary.sum()), int(nonmanifold.sum())
    return {"boundary_edges": nb, "nonmanifold_edges": nn, "degenerate_faces": degenerate, "closed": nb == 0 and nn == 0,
            "boundary_vertices": mask}


def normals_host(mesh):
    """Item 3 -> dict: S [Nv,3] int64, E, normals [Nv,3] fp32, zero_normals, degenerate_faces."""
    f, degenerate = valid_faces(mesh)
    v = mesh["vertices"].astype(np.float64)
    nv = v.shape[0]
    pa, pb, pc = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = pb - pa, pc - pa
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).reshape(-1, 3)
    S = np.zeros((nv, 3), np.int64)
    E = E_NONE
    if (n != 0).any():
        E = int(np.frexp(n[n != 0])[1].max()) - 1                   # ilogb
        q = np.rint(np.ldexp(n, 40 - E)).astype(np.int64)
        assert (np.abs(q) <= 1 << 41).all()
        for k in range(3):
            np.add.at(S, f[:, k], q)
    Nd = S.astype(np.float64)
    length = np.sqrt((Nd[:, 0] * Nd[:, 0] + Nd[:, 1] * Nd[:, 1]) + Nd[:, 2] * Nd[:, 2])
    zero = length == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(zero[:, None], 0.0, Nd / length[:, None]).astype(F32)
    return {"S": S, "E": E, "normals": unit, "zero_normals": int(zero.sum()), "degenerate_faces": degenerate}


def smooth_host(mesh, iterations, lam=0.5, mu=-0.53, boundary="fixed"):
    """Item 4 -> dict: vertices {k: [Nv,3] fp32 after k iterations, for every k of `iterations` (an int or a tuple)}, and the
    info counts pinned, boundary_edges, nonmanifold_edges, degenerate_faces."""
    wanted = (iterations,) if isinstance(iterations, int) else tuple(iterations)
    f, degenerate = valid_faces(mesh)
    topo = topology_host(mesh)
    x = np.ascontiguousarray(mesh["vertices"], F32).copy()
    nv = x.shape[0]
    pinned = topo["boundary_vertices"].astype(bool) if boundary == "fixed" else np.zeros(nv, bool)
    out = {"vertices": {}, "pinned": int(pinned.sum()), "boundary_edges": topo["boundary_edges"],
           "nonmanifold_edges": topo["nonmanifold_edges"], "degenerate_faces": degenerate}
    if nv == 0:
        out["vertices"] = {k: x for k in wanted}
        return out
    lo = (x.min(0) + F32(0.0)).astype(np.float64)                   # -0 becomes +0
    extent = float((x.max(0).astype(np.float64) - lo).max())
    assert np.isfinite(x).all()
    if extent == 0.0:
        out["vertices"] = {k: x for k in wanted}
        return out
    s = 36 - int(np.frexp(extent)[1])
    n = 2 * np.bincount(f.reshape(-1), minlength=nv)
    moves = (n > 0) & ~pinned
    nd = np.where(moves, n, 1).astype(np.float64)[:, None]
    if 0 in wanted:
        out["vertices"][0] = x.copy()
    for it in range(1, max(wanted) + 1):
        for factor in (lam, mu):
            if factor == 0.0:
                continue
            x64 = x.astype(np.float64)
            t = np.ldexp(x64 - lo, s)
            assert (np.abs(t) < Q_LIMIT).all(), "diverged: smooth raises"
            q = np.rint(t).astype(np.int64)
            S = np.zeros((nv, 3), np.int64)
            for k in range(3):
                for other in ((k + 1) % 3, (k + 2) % 3):
                    np.add.at(S, f[:, k], q[f[:, other]])
            m = S.astype(np.float64) / nd
            p = lo + np.ldexp(m, -s)
            d = p - x64
            fd = np.float64(factor) * d
            x = np.where(moves[:, None], (x64 + fd).astype(F32), x)
        if it in wanted:
            out["vertices"][it] = x.copy()
    return out


# ------------------------------------------------------------------------------------------------ the meshes
def _mesh(vertices, faces):
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return {"vertices": v, "faces": f, "rgb8": None, "counts": (int(v.shape[0]), int(f.shape[0]))}


def moved(mesh, by):
    return dict(mesh, vertices=(mesh["vertices"] - np.asarray(by, F32)).astype(F32))


def noisy_sphere():
    """The 24^3 sphere with every vertex moved along its radius by a seeded uniform amount of up to half a lattice step."""
    m = base_meshes()["sphere"]
    d = m["vertices"].astype(np.float64) - np.array(SPHERE_C)
    r = np.sqrt((d * d).sum(1, keepdims=True))
    step = np.random.default_rng(41).uniform(-0.5, 0.5, r.shape) * H_ANALYTIC
    return dict(m, vertices=(np.array(SPHERE_C) + d * (1.0 + step / r)).astype(F32))


ANALYTIC = ("sphere", "torus", "blobs", "blobs tie", "blobs strays", "strip")
TETRAHEDRON = ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)])
BIG_FAN = 100000


def _hand_made():
    rng = np.random.default_rng(42)
    out = {
        "one vertex": _mesh([[0.3, -0.2, 7.0]], np.zeros((0, 3))),
        "one triangle": _mesh([[0.2, 0.3, 0.1], [1.4, 0.2, 0.3], [0.3, 1.6, -0.7]], [(0, 1, 2)]),
        "two triangles on one edge": _mesh([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, 0.2], [1.0, 1.1, -0.3]], [(0, 1, 2), (2, 1, 3)]),
        "tetrahedron": _mesh(*TETRAHEDRON),
        "three triangles on one edge": _mesh([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.1, 0.5], [-0.6, 0.9, 0.4], [-0.5, -0.8, 0.6]],
                                             [(0, 1, 2), (0, 1, 3), (0, 1, 4)]),
        "a degenerate face": _mesh(rng.standard_normal((5, 3)), [(0, 1, 2), (0, 0, 1), (2, 1, 3), (3, 4, 3), (1, 4, 3)]),
        "one point": _mesh(np.full((6, 3), [0.25, -1.5, 3.0]), [(0, 1, 2), (2, 1, 3), (3, 4, 5)]),
        "sphere noisy": noisy_sphere(),
    }
    simple = simplify_host(base_meshes()["sphere"], 3.5 * H_ANALYTIC)
    out["sphere simplified"] = _mesh(simple["vertices"], simple["faces"])
    for n in FANS + (BIG_FAN,):
        out[f"fan {n}"] = dict(fan(n, seed=n % 97), rgb8=None)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> mesh, in a fixed order."""
    out = {}
    for k, name in enumerate(ANALYTIC):
        m = base_meshes()[name]
        out[name] = m
        out[name + " / vertices permuted"] = permute_vertices(m, 5000 + k)
        out[name + " / faces permuted"] = permute_faces(m, 6000 + k)
        out[name + " / shifted"] = moved(m, SHIFT)
        out[name + " / far"] = moved(m, -FAR)
    out.update(_hand_made())
    return out


CASE_NAMES = tuple(n + s for n in ANALYTIC for s in ("", " / vertices permuted", " / faces permuted", " / shifted", " / far")) + (
    "one vertex", "one triangle", "two triangles on one edge", "tetrahedron", "three triangles on one edge", "a degenerate face",
    "one point", "sphere noisy", "sphere simplified") + tuple(f"fan {n}" for n in FANS + (BIG_FAN,))
PARAMS = ((0.5, -0.53), (1.0, 0.0), (0.33, -0.34))
ITERATIONS = (0, 1, 3, 10)
SMOOTH_FULL = tuple((it, lam, mu, b) for lam, mu in PARAMS for b in ("fixed", "free") for it in ITERATIONS)
SMOOTH_LIGHT = ((3, 0.5, -0.53, "fixed"), (1, 1.0, 0.0, "free"), (1, 0.33, -0.34, "free"))
SMOOTH_FAN = ((2, 0.5, -0.53, "fixed"), (2, 0.5, -0.53, "free"))


def smooth_arguments(name):
    """The (iterations, lam, mu, boundary) sets that run on case `name` (see the module docstring)."""
    if name == f"fan {BIG_FAN}":
        return SMOOTH_FAN
    return SMOOTH_LIGHT if " / " in name or name == "strip" else SMOOTH_FULL


@functools.lru_cache(maxsize=None)
def expected_topology(name):
    return topology_host(cases()[name])


@functools.lru_cache(maxsize=None)
def expected_normals(name):
    return normals_host(cases()[name])


@functools.lru_cache(maxsize=None)
def _trajectory(name, lam, mu, boundary):
    its = tuple(sorted({a[0] for a in smooth_arguments(name) if a[1:] == (lam, mu, boundary)}))
    return smooth_host(cases()[name], its, lam, mu, boundary)


def expected_smooth(name, iterations, lam, mu, boundary):
    """The restatement's smooth of cases()[name] -> (vertices [Nv,3] fp32, the info counts), computed once per trajectory."""
    r = _trajectory(name, lam, mu, boundary)
    return r["vertices"][iterations], {k: r[k] for k in ("pinned", "boundary_edges", "nonmanifold_edges", "degenerate_faces")}
