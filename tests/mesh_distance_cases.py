"""Cases and numpy restatements for the point-to-mesh distance (csrc/lrf_mesh_distance.inl, localrf_amd/mesh_distance.py):

  pair_host          item 2, the point-triangle pair, in numpy array arithmetic in the .inl's operation order
  closest_host       the search restated by another algorithm: a brute-force minimum over every (point, face) pair, no grid
  grid_search_host   the .inl's own walk (shells, stopping rule) in pure Python over a matrix of pair results
  exact_pair         the pair in exact rational arithmetic (fractions.Fraction)
  sample_host        item 5 with np.repeat / integer arrays
  summary_host       item 6 with Python integers
  mesh_distance_host mesh_distance from the restatements

Everything is generated from seeds; nothing is read from disk."""
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

from mesh_clean_cases import base_meshes, fan, permute_faces, permute_vertices
from mesh_raster_cases import octa_sphere

F32, F64, U32 = np.float32, np.float64, np.uint32
SLACK = 1.0 - 2.0 ** -20
SCALE, CLAMP = 1 << 24, 8.0
FACE_SAMPLES = 1 << 21
QUERY_SIZES = (0, 1, 63, 64, 65, 1025)


# ------------------------------------------------------------------------------------------------ item 1
def used_faces(mesh):
    """-> (kind [Nf]: 0 used, 1 an index outside [0, Nv), 2 a corner not finite; corners [Nf,3,3] fp32, zeros where not used)."""
    v, f = np.asarray(mesh["vertices"], F32).reshape(-1, 3), np.asarray(mesh["faces"]).reshape(-1, 3).astype(np.int64)
    kind = np.zeros(f.shape[0], np.int64)
    bad = ((f < 0) | (f >= v.shape[0])).any(1)
    kind[bad] = 1
    x = np.zeros((f.shape[0], 3, 3), F32)
    x[~bad] = v[f[~bad]]
    nonfinite = ~bad & ~np.isfinite(x).all((1, 2))
    kind[nonfinite] = 2
    x[kind != 0] = 0
    return kind, x


# ------------------------------------------------------------------------------------------------ item 2
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _seg(X, e, xp):
    ee, pe = _dot(e, e), _dot(xp, e)
    pos = ee > 0
    t = np.where(pos, pe / np.where(pos, ee, 1.0), 0.0)
    t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
    te = t[..., None] * e
    r = xp - te
    return _dot(r, r), X + te


def pair_host(p, x):
    """p [...,3] and x [...,3,3] fp32 (broadcast against each other) -> d2 [...] fp64, q [...,3] fp64 (the closest point before its
    rounding to fp32), term [...] (0, 1, 2: the segment ab, bc, ca; 3: the plane)."""
    P = np.asarray(p, F32).astype(F64)
    x = np.asarray(x, F32).astype(F64)
    A, B, C = x[..., 0, :], x[..., 1, :], x[..., 2, :]
    ab, bc, ca, ac = B - A, C - B, A - C, C - A
    ap, bp, cp = P - A, P - B, P - C
    d2, q = _seg(A, ab, ap)
    term = np.zeros(d2.shape, np.int64)
    for k, (X, e, xp) in enumerate(((B, bc, bp), (C, ca, cp)), 1):
        dk, qk = _seg(X, e, xp)
        less = dk < d2
        d2, q, term = np.where(less, dk, d2), np.where(less[..., None], qk, q), np.where(less, k, term)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    inside = (nn > 0) & (_dot(_cross(ab, ap), n) >= 0) & (_dot(_cross(bc, bp), n) >= 0) & (_dot(_cross(ca, cp), n) >= 0)
    dn = _dot(ap, n)
    safe = np.where(nn > 0, nn, 1.0)
    d_pl = (dn * dn) / safe
    less = inside & (d_pl < d2)
    s = dn / safe
    q_pl = P - s[..., None] * n
    return np.where(less, d_pl, d2), np.where(less[..., None], q_pl, q), np.where(less, 3, term)


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """(kind, d2 [N,F] fp64 with +inf at the faces not used) of a case: every (point, face) pair, no grid."""
    c = cases()[name]
    kind, x = used_faces(c["mesh"])
    p = c["points"]
    d2 = np.full((p.shape[0], x.shape[0]), np.inf)
    use = np.nonzero(kind == 0)[0]
    with np.errstate(all="ignore"):
        for i0 in range(0, p.shape[0], 16):
            if use.size:
                d2[i0:i0 + 16, use] = pair_host(p[i0:i0 + 16, None, :], x[None, use])[0]
    d2.setflags(write=False)
    return kind, d2


def closest_from_pairs(c, kind, d2, max_distance):
    """The brute-force minimum: ties to the smallest face index, cut at max_distance."""
    p = c["points"]
    n = p.shape[0]
    finite = np.isfinite(p).all(1) if n else np.zeros(0, bool)
    md = float(max_distance)
    if d2.shape[1]:
        face = d2.argmin(1)                                                      # the first of equal minima: the smallest index
        best = d2[np.arange(n), face]
    else:
        face, best = np.zeros(n, np.int64), np.full(n, np.inf)
    hit = finite & np.isfinite(best) & ~(best > md * md)
    with np.errstate(all="ignore"):
        distance = np.where(finite, np.where(hit, np.sqrt(best), np.inf), np.nan).astype(F32)
    closest = np.full((n, 3), np.nan, F32)
    if hit.any():
        _, x = used_faces(c["mesh"])
        with np.errstate(all="ignore"):
            closest[hit] = pair_host(p[hit], x[face[hit]])[1].astype(F32)
    return {"distance": distance, "face": np.where(hit, face, -1).astype(np.int32), "closest": closest, "d2": np.where(hit, best, np.inf)}


@functools.lru_cache(maxsize=None)
def expected(name, max_distance=None):
    c = cases()[name]
    kind, d2 = _pairs(name)
    out = closest_from_pairs(c, kind, d2, c["max_distance"] if max_distance is None else max_distance)
    out["info"] = {"bad_index_faces": int((kind == 1).sum()), "nonfinite_faces": int((kind == 2).sum()), "used_faces": int((kind == 0).sum())}
    return out


# ------------------------------------------------------------------------------------------------ items 3 and 4
def box_host(mesh):
    kind, x = used_faces(mesh)
    if not (kind == 0).any():
        return None
    pts = x[kind == 0].reshape(-1, 3).astype(F64) + 0.0
    return tuple(float(a) for a in pts.min(0)), tuple(float(a) for a in pts.max(0))


def dims_host(lo, hi, cell):
    return tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))


def default_cell_host(lo, hi, used):
    longest = max(h - l for l, h in zip(lo, hi))
    if not longest > 0 or used < 1:
        return 1.0
    cell = longest * 2.0 * math.sqrt(2.0 / used)
    while math.prod(dims_host(lo, hi, cell)) > (1 << 31) - 1:
        cell *= 2.0
    return cell


def cell_host(x, lo, cell, dim):
    t = math.floor((float(x) - lo) / cell)
    return min(max(t, 0), dim - 1)


def grid_host(mesh, cell):
    """-> (lo, dims, {cell index: [faces]}) as k_md_fill lists them (the order inside a list is free)."""
    kind, x = used_faces(mesh)
    lo, hi = box_host(mesh)
    dims = dims_host(lo, hi, cell)
    lists = {}
    for f in np.nonzero(kind == 0)[0]:
        c0 = [cell_host(x[f, :, k].min(), lo[k], cell, dims[k]) for k in range(3)]
        c1 = [cell_host(x[f, :, k].max(), lo[k], cell, dims[k]) for k in range(3)]
        for z in range(c0[2], c1[2] + 1):
            for y in range(c0[1], c1[1] + 1):
                for i in range(c0[0], c1[0] + 1):
                    lists.setdefault((z * dims[1] + y) * dims[0] + i, []).append(int(f))
    return lo, dims, lists


def grid_search_host(mesh, points, cell, max_distance, d2):
    """The .inl's walk for every finite point: -> (best d2 [N], face [N], shells walked [N]); d2 [N,F]: the pair results."""
    lo, dims, lists = grid_host(mesh, cell)
    n = points.shape[0]
    best_out, face_out, shells = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        p = points[i]
        if not np.isfinite(p).all():
            continue
        c = [cell_host(p[k], lo[k], cell, dims[k]) for k in range(3)]
        rmax = max(max(c[k], dims[k] - 1 - c[k]) for k in range(3))
        best, bf, r = math.inf, None, 0
        while True:
            for z in range(max(c[2] - r, 0), min(c[2] + r, dims[2] - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, dims[1] - 1) + 1):
                    if abs(z - c[2]) == r or abs(y - c[1]) == r:
                        xs = range(max(c[0] - r, 0), min(c[0] + r, dims[0] - 1) + 1)
                    else:
                        xs = [x for x in (c[0] - r, c[0] + r) if 0 <= x <= dims[0] - 1]
                    for x in xs:
                        for f in lists.get((z * dims[1] + y) * dims[0] + x, ()):
                            d = d2[i, f]
                            if d < best or (d == best and f < bf):
                                best, bf = d, f
            bound = (float(r) * cell) * SLACK
            if best < bound * bound or r >= rmax or bound > max_distance:
                break
            r += 1
        shells[i] = r
        if bf is not None and not best > max_distance * max_distance:
            best_out[i], face_out[i] = best, bf
    return best_out, face_out, shells


# ------------------------------------------------------------------------------------------------ exact arithmetic
def exact_pair(p, x):
    """p [3], x [3,3] fp32 -> the exact squared distance of the point to the triangle (a segment or a point when it has no area)
    as a Fraction."""
    P = [Fraction(float(v)) for v in p]
    A, B, C = ([Fraction(float(v)) for v in row] for row in x)

    def sub(a, b):
        return [a[k] - b[k] for k in range(3)]

    def dot(a, b):
        return sum(a[k] * b[k] for k in range(3))

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def seg(X, Y):
        e, xp = sub(Y, X), sub(P, X)
        ee = dot(e, e)
        t = min(max(dot(xp, e) / ee, 0), 1) if ee > 0 else Fraction(0)
        r = [xp[k] - t * e[k] for k in range(3)]
        return dot(r, r)

    best = min(seg(A, B), seg(B, C), seg(C, A))
    n = cross(sub(B, A), sub(C, A))
    nn = dot(n, n)
    if nn > 0 and all(dot(cross(sub(Y, X), sub(P, X)), n) >= 0 for X, Y in ((A, B), (B, C), (C, A))):
        dn = dot(sub(P, A), n)
        best = min(best, dn * dn / nn)
    return best


def exact_error(p, x, d2):
    """|sqrt(d2) - d_exact| / L with L the largest absolute coordinate difference between the point and the corners; the fp64
    result before any fp32 rounding.  The exact root is taken at 60 digits."""
    getcontext().prec = 60
    e = exact_pair(p, x)
    root = (Decimal(e.numerator) / Decimal(e.denominator)).sqrt()
    L = float(np.abs(np.asarray(x, F64) - np.asarray(p, F64)).max())
    if L == 0:
        return 0.0 if d2 == 0 else math.inf
    return float(abs(Decimal(math.sqrt(d2)) - root) / Decimal(L))


@functools.lru_cache(maxsize=None)
def exact_cases(n=160):
    """kind -> (p [n,3], x [n,3,3]) fp32: random, sliver, zero-area (segment), single-point, near-surface and on-surface."""
    rng = np.random.default_rng(77)
    out = {}
    x = rng.standard_normal((n, 3, 3)).astype(F32)
    out["random"] = (rng.standard_normal((n, 3)).astype(F32) * 2, x)
    s = x.copy()
    s[:, 2] = (s[:, 0] + (s[:, 1] - s[:, 0]) * rng.random((n, 1)).astype(F32) + rng.standard_normal((n, 3)).astype(F32) * 1e-5).astype(F32)
    ps = rng.standard_normal((n, 3)).astype(F32)
    ns = np.cross(s[:, 1].astype(F64) - s[:, 0], s[:, 2].astype(F64) - s[:, 0])
    ns /= np.maximum(np.linalg.norm(ns, axis=1, keepdims=True), 1e-300)
    inside = (rng.dirichlet((1, 1, 1), n)[:, :, None] * s.astype(F64)).sum(1) + ns * rng.standard_normal((n, 1)) * 1e-3
    ps[1::2] = inside[1::2].astype(F32)                                                 # every other point over the sliver itself
    out["sliver"] = (ps, s)
    z = np.round(rng.standard_normal((n, 3, 3)) * 64).astype(F32) / 64                 # short mantissas: the third corner is exact
    t = rng.integers(-8, 17, (n, 1)).astype(F32) / 8
    z[:, 2] = z[:, 0] + (z[:, 1] - z[:, 0]) * t
    z[::4, 1] = z[::4, 0]                                                               # two equal corners
    out["zero-area"] = (rng.standard_normal((n, 3)).astype(F32) * 3, z)
    pt = rng.standard_normal((n, 1, 3)).astype(F32).repeat(3, 1)
    out["single-point"] = (rng.standard_normal((n, 3)).astype(F32), pt)
    w = rng.dirichlet((1, 1, 1), n)
    on = (w[:, :, None] * x.astype(F64)).sum(1)
    nrm = np.cross(x[:, 1].astype(F64) - x[:, 0], x[:, 2].astype(F64) - x[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    out["near-surface"] = ((on + nrm * rng.standard_normal((n, 1)) * 1e-4).astype(F32), x)
    onp = on.astype(F32)
    onp[::3] = x[::3, 1]                                                                # on a vertex
    onp[1::3] = ((x[1::3, 0].astype(F64) + x[1::3, 2]) / 2).astype(F32)                 # on an edge (up to its rounding)
    out["on-surface"] = (onp, x)
    return out


# ------------------------------------------------------------------------------------------------ item 5
def _mix(x):
    x = x.astype(U32)
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def _hash3(a, b, c):
    return _mix(_mix(_mix(a.astype(U32) + U32(0x9e3779b9)) ^ b) ^ c)


def sample_faces_host(x, spacing):
    """Used faces' corners x [F,3,3] fp32 -> (A, ab, ac [F,3] fp64 of the rotated corners, H [F] uint32, count [F] int64 with -1
    where a face takes more than 2^21 samples)."""
    b = np.ascontiguousarray(x, F32).view(U32).astype(np.int64)
    first = np.zeros(x.shape[0], np.int64)
    cur = b[:, 0].copy()
    for k in (1, 2):
        cand = b[:, k]
        less = np.where(cand[:, 0] != cur[:, 0], cand[:, 0] < cur[:, 0],
                        np.where(cand[:, 1] != cur[:, 1], cand[:, 1] < cur[:, 1], cand[:, 2] < cur[:, 2]))
        first[less] = k
        cur[less] = cand[less]
    order = (first[:, None] + np.arange(3)[None]) % 3
    rb = np.take_along_axis(b, order[:, :, None], 1).astype(U32)
    rx = np.take_along_axis(np.asarray(x, F32), order[:, :, None], 1).astype(F64)
    with np.errstate(over="ignore"):
        H = _hash3(*(_hash3(rb[:, k, 0], rb[:, k, 1], rb[:, k, 2]) for k in range(3)))
    A = rx[:, 0]
    ab, ac = rx[:, 1] - A, rx[:, 2] - A
    n = _cross(ab, ac)
    area = 0.5 * np.sqrt(_dot(n, n))
    y = np.floor(area / (float(spacing) * float(spacing)) + H.astype(F64) * 2.0 ** -32)
    count = np.where(y <= FACE_SAMPLES, y, -1).astype(np.int64)
    return A, ab, ac, H, count


def sample_host(mesh, spacing):
    """-> {"points" [M,3] fp32, "face" [M] int32, "counts": (M,), "info", "per_face" [Nf] int64}"""
    kind, x = used_faces(mesh)
    use = np.nonzero(kind == 0)[0]
    per_face = np.zeros(kind.shape[0], np.int64)
    info = {"spacing": float(spacing), "bad_index_faces": int((kind == 1).sum()), "nonfinite_faces": int((kind == 2).sum())}
    if not use.size:
        return {"points": np.zeros((0, 3), F32), "face": np.zeros(0, np.int32), "counts": (0,), "info": info, "per_face": per_face}
    A, ab, ac, H, count = sample_faces_host(x[use], spacing)
    assert (count >= 0).all(), "a face takes more than 2^21 samples"
    per_face[use] = count
    row = np.repeat(np.arange(use.size), count)
    k = np.arange(row.size) - np.repeat(np.cumsum(count) - count, count)
    with np.errstate(over="ignore"):
        su, sv = _mix(H ^ U32(0x68bc21eb))[row], _mix(H ^ U32(0x02e5be93))[row]
        U = su + (k + 1).astype(U32) * U32(0xC13FA9A9)
        V = sv + (k + 1).astype(U32) * U32(0x91E10DA5)
    u, v = U.astype(F64) * 2.0 ** -32, V.astype(F64) * 2.0 ** -32
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)
    pts = ((A[row] + u[:, None] * ab[row]) + v[:, None] * ac[row]).astype(F32)
    return {"points": pts, "face": use[row].astype(np.int32), "counts": (int(row.size),), "info": info, "per_face": per_face}


# ------------------------------------------------------------------------------------------------ item 6
def summary_host(d, thresholds=(), unit=1.0):
    d = np.asarray(d, F32).reshape(-1)
    taus = [float(F32(t)) for t in thresholds]
    fin = np.isfinite(d)
    df = d[fin]
    with np.errstate(all="ignore"):
        x = np.minimum(df / F32(unit), F32(CLAMP)).astype(F64)
    s1 = sum(int(v) for v in np.rint(x * float(SCALE)))
    s2 = sum(int(v) for v in np.rint((x * x) * float(SCALE)))
    pos = df[df >= 0]
    top = int((pos.view(U32) & U32(0x7FFFFFFF)).max()) if pos.size else 0
    n = int(fin.sum())
    return {"finite": n, "beyond": int(np.isinf(d).sum()), "nan": int(np.isnan(d).sum()),
            "within": tuple(int((df <= F32(t)).sum()) for t in taus), "sum": s1, "sum_sq": s2,
            "mean": s1 / SCALE / n * unit if n else math.nan, "rms": math.sqrt(s2 / SCALE / n) * unit if n else math.nan,
            "max": float(np.array([top], U32).view(F32)[0]) if n else math.nan, "thresholds": tuple(taus), "unit": unit}


def summary_inputs(seed, n):
    """Distances around 0.3 with planted NaN, infinities, zeros, negatives, values beyond the clamp and exact thresholds."""
    rng = np.random.default_rng(seed)
    d = (rng.random(n) ** 2 * 0.9).astype(F32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-30, 3e38, 50.0, 0.25, 0.5], F32)
    k = rng.permutation(n)[:max(1, n // 5)] if n else np.zeros(0, np.int64)
    d[k] = specials[rng.integers(0, specials.size, k.size)]
    return d


SUMMARY_SIZES = (0, 1, 63, 2048, 2049, 40001)
SUMMARY_TAUS = (0.01, 0.25, 0.5, 2.0)


def mesh_distance_host(a, b, spacing, thresholds=(), max_distance=math.inf):
    """mesh_distance from sample_host, the brute force and summary_host."""
    sides = []
    for src, dst in ((a, b), (b, a)):
        s = sample_host(src, spacing)
        kind, x = used_faces(dst)
        use = np.nonzero(kind == 0)[0]
        d2 = np.full((s["points"].shape[0], x.shape[0]), np.inf)
        with np.errstate(all="ignore"):
            for i0 in range(0, s["points"].shape[0], 64):
                if use.size:
                    d2[i0:i0 + 64, use] = pair_host(s["points"][i0:i0 + 64, None, :], x[None, use])[0]
        near = closest_from_pairs({"points": s["points"], "mesh": dst}, kind, d2, max_distance)
        unit = max_distance if math.isfinite(max_distance) and max_distance > 0 else 1.0
        sides.append(summary_host(near["distance"], thresholds, unit))
    ab, ba = sides
    n_a, n_b = ab["finite"] + ab["beyond"], ba["finite"] + ba["beyond"]
    maxima = [s["max"] for s in sides if s["finite"]]
    precision = tuple(w / n_a if n_a else math.nan for w in ab["within"])
    recall = tuple(w / n_b if n_b else math.nan for w in ba["within"])
    fscore = tuple(2 * p * r / (p + r) if p + r > 0 else math.nan for p, r in zip(precision, recall))
    return {"a_to_b": ab, "b_to_a": ba, "chamfer": ab["mean"] + ba["mean"], "hausdorff": max(maxima) if maxima else math.nan,
            "precision": precision, "recall": recall, "fscore": fscore, "thresholds": ab["thresholds"],
            "samples": (ab["finite"] + ab["beyond"] + ab["nan"], ba["finite"] + ba["beyond"] + ba["nan"])}


# ------------------------------------------------------------------------------------------------ the cases
def _mesh(vertices, faces):
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    return {"vertices": v, "faces": f, "rgb8": None, "counts": (int(v.shape[0]), int(f.shape[0]))}


def mean_edge(mesh):
    kind, x = used_faces(mesh)
    x = x[kind == 0].astype(F64)
    return float(np.linalg.norm(x - np.roll(x, 1, 1), axis=2).mean())


def queries(mesh, n, seed, cell=None):
    """n query points for the mesh: on vertices, on edges (up to their rounding), near the surface on both sides, inside the box,
    far outside it on every side, and on cell borders of the grid at `cell` (default: the default cell)."""
    rng = np.random.default_rng(seed)
    kind, x = used_faces(mesh)
    x = x[kind == 0].astype(F64)
    if not x.shape[0]:
        return (rng.standard_normal((n, 3)) * 2).astype(F32)
    lo, hi = (np.array(b) for b in box_host(mesh))
    ext = max(float((hi - lo).max()), 1e-3)
    cell = default_cell_host(tuple(lo), tuple(hi), x.shape[0]) if cell is None else cell
    out = []
    sides = [np.array(s) for s in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1))]
    for i in range(n):
        f = x[rng.integers(x.shape[0])]
        k = i % 8
        if k == 0:
            p = f[rng.integers(3)]
        elif k == 1:
            p = (f[0] + f[1]) / 2 if i % 16 == 1 else f[1] + (f[2] - f[1]) * rng.random()
        elif k in (2, 3):
            w = rng.dirichlet((1, 1, 1))
            nrm = np.cross(f[1] - f[0], f[2] - f[0])
            nrm = nrm / max(np.linalg.norm(nrm), 1e-30)
            p = w @ f + nrm * rng.standard_normal() * ext * (0.002 if k == 2 else 0.05)
        elif k == 4:
            p = lo + (hi - lo) * rng.random(3)
        elif k == 5:
            p = (lo + hi) / 2 + sides[(i // 8) % 8] * ext * (0.6 + 3 * rng.random()) + rng.standard_normal(3) * ext * 0.1
        elif k == 6:
            p = lo + np.floor((hi - lo) * rng.random(3) / cell) * cell                   # on cell borders, all three axes
        else:
            p = lo + (hi - lo) * rng.random(3)
            a = rng.integers(3)
            p[a] = lo[a] + math.floor((hi[a] - lo[a]) * rng.random() / cell) * cell      # on one border
        out.append(p)
    return np.asarray(out, F64).reshape(-1, 3).astype(F32)


def _case(mesh, points, cells=(None,), max_distance=math.inf, host_cell=None):
    """cells: the cell sizes the GPU tests build the index at (None: the default); host_cell: the one the pure-Python walk uses
    (None: the default cell)."""
    return {"mesh": mesh, "points": np.ascontiguousarray(points, F32).reshape(-1, 3), "cells": tuple(cells), "max_distance": max_distance,
            "host_cell": host_cell}


TRIANGLE = _mesh([(0.1, -0.2, 0.3), (1.3, 0.1, -0.2), (0.4, 1.1, 0.5)], [(0, 1, 2)])


def planar(n=8):
    """n x n quads in the plane z = 0.25, two faces each: a grid one cell thick."""
    g = np.arange(n + 1, dtype=F64) / n
    v = np.stack([np.tile(g, n + 1), np.repeat(g, n + 1), np.full((n + 1) ** 2, 0.25)], 1)
    i = (np.arange(n)[None, :] + (n + 1) * np.arange(n)[:, None]).reshape(-1)
    return _mesh(v, np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)]))


def slabs():
    """Face 0 in the plane z = -1, face 1 in z = 0, both over [0, 4]^2, with cell 0.5 (exact in binary): distances are exact
    multiples of the cell, and z = -0.5 is equally far from both."""
    return _mesh([(0, 0, -1), (4, 0, -1), (0, 4, -1), (0, 0, 0), (4, 0, 0), (0, 4, 0)], [(0, 1, 2), (3, 4, 5)])


def slab_points():
    z = [0.5 * k for k in range(-8, 9)] + [0.25, -0.25, -0.75, 1e-3]
    return [(1.25, 1.0, t) for t in z] + [(1.0 + 0.5 * k, 0.5, -0.5) for k in range(4)] + [(-0.5 * k, -0.5 * k, 0.0) for k in range(1, 5)]


def spanning():
    """A planar patch of small faces and, last, one face across the whole box: it is listed in every cell."""
    m = planar(6)
    v = np.concatenate([m["vertices"], np.array([(0, 0, 0), (1, 0, 0.5), (0, 1, 0.5), (1, 1, 0)], F32)])
    nv = m["vertices"].shape[0]
    return _mesh(v, np.concatenate([m["faces"], [(nv, nv + 1, nv + 2)], [(nv + 3, nv + 2, nv + 1)]]))


def zero_area():
    """Segments (collinear corners; two equal corners; two equal indices), points (three equal corners or indices) and one
    ordinary face."""
    v = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0.5, 1, 0), (0.5, 1, 0), (0.5, 1, 0), (0, 0, 1), (0, 0.75, 1), (-1, -1, -1), (1, 0.5, 2), (1.5, 0.25, 2),
         (1.25, 1.5, 2.5)]
    return _mesh(v, [(0, 1, 2), (0, 2, 1), (3, 4, 5), (6, 7, 7), (6, 6, 7), (8, 8, 8), (9, 10, 11), (2, 0, 1)])


def bad_faces():
    """Used faces between faces with indices outside [0, Nv) and faces with NaN or infinite corners."""
    m = octa_sphere(1)
    v = np.concatenate([m["vertices"], np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)], F32)])
    nv = m["vertices"].shape[0]
    f = m["faces"].astype(np.int64)
    extra = np.array([(0, 1, nv + 3), (-1, 2, 3), (1 << 30, 0, 1), (0, 1, nv), (nv + 1, 2, 3), (4, nv + 2, 5), (0, -5, nv)], np.int64)
    f = np.concatenate([extra[:3], f[:10], extra[3:5], f[10:], extra[5:]])
    return _mesh(v, f)


def special_points():
    p = queries(octa_sphere(1), 24, 5).copy()
    p[3, 0], p[7, 1], p[11, 2], p[12] = np.nan, np.inf, -np.inf, np.nan
    return p


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    octa = {k: v for k, v in octa_sphere().items()}
    edge = mean_edge(octa)
    out["no faces"] = _case(_mesh(TRIANGLE["vertices"], np.zeros((0, 3))), queries(TRIANGLE, 5, 1))
    for n in QUERY_SIZES:
        out[f"one triangle N={n}"] = _case(TRIANGLE, queries(TRIANGLE, n, 10 + n), cells=(None, 10.0, 0.11), host_cell=0.11 if n <= 65 else None)
    two = _mesh(TRIANGLE["vertices"], [(0, 1, 2), (0, 1, 2)])
    out["two coincident faces"] = _case(two, queries(two, 65, 2), cells=(None, 0.3))
    rot = _mesh(TRIANGLE["vertices"], [(1, 2, 0), (0, 1, 2)])
    out["two coincident faces, rotated corners"] = _case(rot, queries(rot, 65, 3))
    for k, (name, m) in enumerate(base_meshes().items()):
        big = m["faces"].shape[0] > 20000                                               # random corners: every face spans the box
        box = box_host(m)
        coarse = None if not big else max(h - l for l, h in zip(*box)) / 3
        host_cell = coarse if big or m["faces"].shape[0] < 1000 else max(h - l for l, h in zip(*box)) / 8
        out[f"base {name}"] = _case(m, queries(m, 17 if big else 65, 30 + k, coarse), cells=(coarse,), host_cell=host_cell)
    out["octa 512 N=1025"] = _case(octa, queries(octa, 1025, 4), cells=(None, 0.25 * edge, 10 * edge), host_cell=10 * edge)
    out["octa 512 default cell"] = _case(octa, queries(octa, 65, 6))
    out["octa 512 max_distance 0.05"] = _case(octa, queries(octa, 130, 7), cells=(None, 10 * edge), max_distance=0.05)
    small = octa_sphere(1)
    out["octa 32 cell a tenth of the edge"] = _case(small, queries(small, 65, 8, 0.1 * mean_edge(small)), cells=(0.1 * mean_edge(small),),
                                                    max_distance=0.5, host_cell=0.1 * mean_edge(small))
    out["octa faces permuted"] = _case(permute_faces(octa, 41), out["octa 512 default cell"]["points"])
    out["octa vertices permuted"] = _case(permute_vertices(dict(octa, rgb8=None), 42), out["octa 512 default cell"]["points"])
    out["grid of 1 x 1 x 1"] = _case(small, queries(small, 65, 9), cells=(100.0,), host_cell=100.0)
    out["planar, one cell thick"] = _case(planar(), queries(planar(), 65, 12), cells=(None, 0.05))
    out["one face spans every cell"] = _case(spanning(), queries(spanning(), 65, 13, 0.125), cells=(0.125, None), host_cell=0.125)
    f70 = fan(70, seed=3)
    out["fan: 68 faces in one cell"] = _case(f70, queries(f70, 65, 14), cells=(100.0, None), host_cell=100.0)
    for md in (math.inf, 0.5, 0.0):
        out[f"slabs at multiples of the cell, max_distance {md}"] = _case(slabs(), slab_points(), cells=(0.5, 0.25, None), max_distance=md,
                                                                          host_cell=0.5)
    out["zero-area faces"] = _case(zero_area(), queries(zero_area(), 65, 15), cells=(None, 0.4))
    out["bad faces, special points"] = _case(bad_faces(), special_points(), cells=(None, 0.3))
    nv = bad_faces()["vertices"].shape[0]
    only_bad = _mesh(bad_faces()["vertices"], [(0, 1, 99), (nv - 3, 0, 1)])
    out["no used face"] = _case(only_bad, special_points())
    return out


CASE_NAMES = tuple(cases())
SAMPLE_CASES = {"octa 512 at 0.05": (lambda: octa_sphere(), 0.05), "octa 512 at 0.2": (lambda: octa_sphere(), 0.2),
                "one triangle at 0.03": (lambda: TRIANGLE, 0.03), "one triangle at 5": (lambda: TRIANGLE, 5.0),
                "zero-area at 0.1": (zero_area, 0.1), "bad faces at 0.07": (bad_faces, 0.07), "planar at 0.02": (planar, 0.02),
                "base sphere at 0.02": (lambda: base_meshes()["sphere"], 0.02), "spanning at 0.04": (spanning, 0.04)}
