"""Shared pieces of the quadric-placement tests: the numpy restatement of rules a-d of csrc/lrf_mesh_simplify.inl on top of
mesh_simplify_cases.cells_host / simplify_host -- float64 array arithmetic (every ufunc rounds once, nothing is fused),
np.maximum.at for the exponents, np.add.at for the integer sums; no bit words, no scans, no runs -- and the cases: the
analytic meshes of mesh_simplify_cases at every cell and anchor, shifted and permuted, and hand-made meshes for the edges of
the rules."""
import functools

import numpy as np

from mesh_clean_cases import fan
from mesh_simplify_cases import ANALYTIC, CASE_NAMES as MEAN_CASE_NAMES, F32, Q_ONE, _mesh, cases as mean_cases, cells_host, simplify_host

REGULARIZE = 2.0 ** -10
CAP = 1 << 21
BITS = 40
NONE = np.iinfo(np.int32).min


# ------------------------------------------------------------------------------------------------ the restatement
def contributions(i, q, faces, cluster_of):
    """Rule a -> (cluster [K], coefficients [K,9], g [K]) of every contribution, skipped ones included."""
    out = []
    g3 = cluster_of[faces]
    speaks = (np.ones(faces.shape[0], bool), g3[:, 1] != g3[:, 0], (g3[:, 2] != g3[:, 0]) & (g3[:, 2] != g3[:, 1]))
    for j in range(3):
        rows = np.nonzero(speaks[j])[0]
        at = faces[rows]
        ic = i[at[:, j]]
        u = [(i[at[:, c]] - ic).astype(np.float64) + q[at[:, c]].astype(np.float64) * (1.0 / Q_ONE) for c in range(3)]
        a, b = u[1] - u[0], u[2] - u[0]
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        d = -((nx * u[0][:, 0] + ny * u[0][:, 1]) + nz * u[0][:, 2])
        md = -d
        coef = np.stack([nx * nx, ny * ny, nz * nz, nx * ny, nx * nz, ny * nz, md * nx, md * ny, md * nz], 1)
        g = np.maximum(np.maximum(coef[:, 0], coef[:, 1]), np.maximum(coef[:, 2], d * d))
        out.append((g3[rows, j], coef, g))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def sums(cl, coef, g, nc):
    """Rule b -> (Q [nc,9] int64, m [nc], E [nc])."""
    ok = (g > 0) & np.isfinite(g)
    cl, coef, g = cl[ok], coef[ok], g[ok]
    E = np.full(nc, NONE, np.int64)
    np.maximum.at(E, cl, np.frexp(g)[1].astype(np.int64) - 1)       # ilogb
    scaled = np.rint(np.ldexp(coef, (BITS - E[cl])[:, None].astype(np.int64))).astype(np.int64)
    assert (np.abs(scaled) <= 1 << (BITS + 1)).all()
    Q = np.zeros((nc, 9), np.int64)
    np.add.at(Q, cl, scaled)
    return Q, np.bincount(cl, minlength=nc), E


def solve(Q, m, mu, regularize):
    """Rule c -> (x [nc,3] clamped, mean [nc] bool: the cluster keeps the mean, clamped [nc] bool)."""
    A = Q.astype(np.float64)
    with np.errstate(all="ignore"):
        tr = (A[:, 0] + A[:, 1]) + A[:, 2]
        lam = regularize * tr
        M00, M11, M22, M01, M02, M12 = A[:, 0] + lam, A[:, 1] + lam, A[:, 2] + lam, A[:, 3], A[:, 4], A[:, 5]
        r = [A[:, 6 + k] + lam * mu[:, k] for k in range(3)]
        c00, c01, c02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
        c11, c12, c22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        x = np.stack([((c00 * r[0] + c01 * r[1]) + c02 * r[2]) / det,
                      ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) / det,
                      ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det], 1)
        mean = (m == 0) | (m >= CAP) | ~(tr > 0) | ~(det > 0) | ~np.isfinite(x).all(1)
        clamped = ~mean & ((x < 0) | (x > 1)).any(1)
    return np.minimum(np.maximum(x, 0.0), 1.0), mean, clamped


@functools.lru_cache(maxsize=None)
def _clusters(name, regularize):
    """Rules a-c for every cluster of cases()[name] (they do not depend on rgb8 or dedupe), keyed by cell."""
    mesh, cell, origin = cases()[name]
    v, f = mesh["vertices"], np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    i, q, bad = cells_host(v, cell, origin)
    assert not bad.any()
    cell_of, cluster_of = np.unique(i, axis=0, return_inverse=True)  # any numbering of the clusters serves
    cluster_of = cluster_of.reshape(-1)
    nc = cell_of.shape[0]
    S = np.zeros((nc, 3), np.uint64)
    np.add.at(S, cluster_of, q)
    n = np.bincount(cluster_of, minlength=nc)
    mu = (S.astype(np.float64) / n.astype(np.float64)[:, None]) * (1.0 / Q_ONE)
    Q, m, E = sums(*contributions(i, q, f, cluster_of), nc)
    x, mean, clamped = solve(Q, m, mu, regularize)
    index = {tuple(c): k for k, c in enumerate(cell_of.tolist())}
    return {"index": index, "x": x, "mean": mean, "clamped": clamped, "m": m, "E": E, "Q": Q}


@functools.lru_cache(maxsize=None)
def expected_quadric(name, rgb=True, dedupe=True, regularize=REGULARIZE):
    """The restatement's result for cases()[name]: simplify_host's dict with rule d's vertices, counts of seven (the five,
    clusters left at the mean, clusters clamped) and, per emitted vertex, mean_placed and contributions."""
    mesh, cell, origin = cases()[name]
    base = simplify_host(mesh if rgb else dict(mesh, rgb8=None), cell, origin, dedupe)
    if base["counts"][0] == 0:
        return dict(base, counts=base["counts"] + (0, 0), mean_vertices=base["vertices"], mean_placed=np.zeros(0, bool),
                    contributions=np.zeros(0, np.int64))
    c = _clusters(name, regularize)
    k = np.array([c["index"][tuple(t)] for t in base["cells"].tolist()])
    t = base["cells"].astype(np.float64) + c["x"][k]
    xx = t * np.float64(cell)
    pos = (np.asarray(origin, np.float64) + xx).astype(F32)
    pos = np.where(c["mean"][k][:, None], base["vertices"], pos)
    return dict(base, vertices=np.ascontiguousarray(pos), mean_vertices=base["vertices"], mean_placed=c["mean"][k],
                contributions=c["m"][k], counts=base["counts"] + (int(c["mean"][k].sum()), int(c["clamped"][k].sum())))


def signed_volume(vertices, faces):
    """Sum of a . (b x c) / 6 over the faces, in float64."""
    v = vertices.astype(np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------ the meshes
CUBE_LO, CUBE_HI, CUBE_N = 0.3, 3.7, 17                              # cell 1: the corner cells hold one corner each


def cube(n=CUBE_N, lo=CUBE_LO, hi=CUBE_HI):
    """The surface of [lo, hi]^3, every side split into n x n squares of two triangles, welded, wound outwards."""
    pts, tris = [], []
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    for axis in range(3):
        for side in (0, n):
            def at(da, db):
                p = np.zeros((a.size, 3), np.int64)
                p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side, a + da, b + db
                return p
            quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]          # counter-clockwise seen from +axis
            if side == 0:
                quad = quad[::-1]
            for t in ((0, 1, 2), (0, 2, 3)):
                tris.append(np.stack([quad[k] for k in t], 1))
    tris = np.concatenate(tris).reshape(-1, 3)                       # lattice triples of every corner of every face
    pts, inverse = np.unique(tris, axis=0, return_inverse=True)
    return _mesh(lo + pts * ((hi - lo) / n), inverse.reshape(-1, 3), 41)


PLANE = (0.37, 0.2, 0.3)                                             # z = 0.37 x + 0.2 y + 0.3


def planar_patch():
    """Six vertices of one plane inside the cell [0, 1)^3 with four faces among them, and one face of the same plane that
    reaches two other cells, so that the cluster is emitted."""
    xy = np.array([[0.1, 0.1], [0.8, 0.15], [0.5, 0.5], [0.2, 0.85], [0.7, 0.8], [0.9, 0.45], [1.6, 0.3], [0.4, 1.7]])
    z = PLANE[0] * xy[:, 0] + PLANE[1] * xy[:, 1] + PLANE[2]
    return _mesh(np.concatenate([xy, z[:, None]], 1), [(0, 1, 2), (0, 2, 3), (2, 4, 3), (1, 5, 2), (5, 6, 7)], 42)


def zero_area():
    """Every face lies on the line x = y = z (coordinates exact in fp32): no face has area, three clusters are emitted."""
    t = np.array([0.125, 0.5, 0.75, 1.25, 1.5, 2.25, 2.875])
    return _mesh(np.stack([t, t, t], 1), [(0, 1, 2), (0, 3, 5), (1, 4, 6), (3, 4, 0), (5, 6, 2)], 43)


def repeated_indices():
    """The one-triangle mesh of three cells with faces that name a vertex twice or three times among the ordinary ones."""
    v = [[0.2, 0.3, 0.1], [1.4, 0.2, 0.3], [0.3, 1.6, 0.7], [0.6, 0.7, 0.2], [1.2, 0.6, 0.9], [0.7, 1.3, 0.4]]
    return _mesh(v, [(0, 0, 1), (0, 1, 2), (3, 4, 4), (5, 5, 5), (3, 4, 5), (2, 1, 2), (0, 3, 1)], 44)


def spanning_face(n=300):
    """One face across hundreds of unit cells beside lattice-sized faces that share its corner clusters and a few others."""
    rng = np.random.default_rng(45)
    big = np.array([[0.3, 0.4, 0.2], [300.6, 0.2, 0.7], [0.5, 250.3, 0.1]])
    base = np.concatenate([np.repeat(np.floor(big), n // 3, 0), rng.integers(0, 6, (n - 3 * (n // 3), 3)).astype(np.float64)])
    small = (base[:, None, :] + rng.random((n, 3, 3)) * 1.9).reshape(-1, 3)
    return _mesh(np.concatenate([big, small]), np.concatenate([[[0, 1, 2]], 3 + np.arange(3 * n).reshape(n, 3)]), 45)


def capped_fan(faces=CAP + 3):
    """A fan of `faces` faces with area inside the cell [0, 1)^3 and one face to two other cells: the cluster's count reaches
    the cap of rule b."""
    nv = faces + 2
    rng = np.random.default_rng(46)
    v = np.concatenate([rng.random((nv, 3), dtype=np.float32) * F32(0.999), np.array([[1.5, 0.25, 0.5], [0.25, 1.5, 0.5]], F32)])
    return _mesh(v, np.concatenate([fan(nv)["faces"], [[0, nv, nv + 1]]]), 46, rgb=False)


ANALYTIC_NAMES = tuple(n for n in MEAN_CASE_NAMES if n.split(" ")[0] in ANALYTIC)
FROM_MEAN = ("lattice points", "one triangle", "one triangle in one cell", "one vertex", "two triangles in one cell", "fan in one cell")
HAND_MADE = ("cube", "planar patch", "zero area", "repeated indices", "spanning face")
CASE_NAMES = ANALYTIC_NAMES + FROM_MEAN + HAND_MADE                  # "capped fan" stands apart: one test each side
CAPPED = "capped fan"


@functools.lru_cache(maxsize=None)
def _made(name):
    return {"cube": cube, "planar patch": planar_patch, "zero area": zero_area, "repeated indices": repeated_indices,
            "spanning face": spanning_face, CAPPED: capped_fan}[name]()


class _Cases:
    """name -> (mesh with rgb8, cell, origin); the hand-made meshes are built when first asked for."""
    def __getitem__(self, name):
        if name in HAND_MADE or name == CAPPED:
            return _made(name), 1.0, (0.0, 0.0, 0.0)
        return mean_cases()[name]


def cases():
    return _Cases()
