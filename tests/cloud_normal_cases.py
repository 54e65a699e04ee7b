"""Shared pieces of the point-cloud normal tests: the restatements of csrc/lrf_cloud.inl item 9 and csrc/lrf_align.inl item 4 in
numpy and Python integers, independent of the package, and the cases.

  lattice_h             the lattice step the host passes: the smallest power of two with radius / h <= 2^15
  neighbours_host       the brute force over all pairs in item 2's operation order: d2 <= radius radius
  moments_host          the ten lattice sums of a neighbourhood as Python integers
  covariance_host       the covariance in fp64, operation by operation (np.float64(int) is the int64 -> double conversion)
  jacobi_host           the cyclic Jacobi, operation by operation in fp64 scalars (a Python float is an IEEE double and every
                        Python operation is rounded on its own)
  normals_host          all of item 9: normal, eigenvalues, count, with the sign rules
  plane_cloud_host      item 4 of lrf_align.inl: the 48 words for given points, closest, index, distance and normals
  icp_plane_cloud_host  the plane iteration against a cloud with the restatements in place of the kernels

Everything is generated from seeds; nothing is read from disk."""
import functools
import math

import numpy as np

from align_cases import PLANE_SCALE, _cross, _dot, apply, sim_inverse, transform_host, truth
from cloud_cases import closest_host, planted, random_cloud

F32, F64 = np.float32, np.float64
SWEEPS = 6                                                          # CL_JACOBI_SWEEPS of csrc/lrf_cloud.inl
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                           # (p, q, the remaining index), the order of a sweep
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ item 9, restated
def lattice_h(radius):
    m, e = math.frexp(float(radius))                                # radius = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, e - 16 if m == 0.5 else e - 15)


def neighbours_host(queries, cloud, radius):
    """bool [N,M]: d2 <= radius radius with d2 = (d0 d0 + d1 d1) + d2 d2, d_k = (double)p_k - (double)q_k; the column of a cloud
    point that is not finite is False, the row of such a query is garbage (the callers mask it)."""
    q, c = np.asarray(queries, F32).astype(F64), np.asarray(cloud, F32).astype(F64)
    used = np.isfinite(c).all(1)
    r2 = F64(radius) * F64(radius)
    out = np.zeros((q.shape[0], c.shape[0]), bool)
    with np.errstate(all="ignore"):
        for i0 in range(0, q.shape[0], 512):
            d = q[i0:i0 + 512, None, :] - c[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            out[i0:i0 + 512] = (d2 <= r2) & used[None, :]
    return out


def moments_host(query, near, h):
    """The ten sums over the neighbours `near` [n,3] of one query, as Python integers: n, sum t_k, sum t_i t_j for i <= j in the
    order (0,0), (0,1), (0,2), (1,1), (1,2), (2,2), with t_k = rint(((double)q_k - (double)p_k) / h), q the neighbour."""
    with np.errstate(all="ignore"):
        t = np.rint((np.asarray(near, F32).astype(F64) - np.asarray(query, F32).astype(F64)) / F64(h))
    t = [[int(x) for x in row] for row in t.tolist()]
    assert all(abs(x) <= 1 << 15 for row in t for x in row)
    s = [sum(row[k] for row in t) for k in range(3)]
    S = [sum(row[i] * row[j] for row in t) for i in range(3) for j in range(i, 3)]
    return len(t), s, S


def covariance_host(n, s, S):
    """-> (C00, C01, C02, C11, C12, C22) in fp64: mean_k = (double)s_k / (double)n, C_ij = (double)S_ij / (double)n - mean_i mean_j."""
    nd = float(F64(n))
    mean = [float(F64(x)) / nd for x in s]
    at = iter(S)
    return tuple(float(F64(next(at))) / nd - mean[i] * mean[j] for i in range(3) for j in range(i, 3))


def jacobi_host(C, sweeps=SWEEPS, record=None):
    """The fixed number of sweeps over (0,1), (0,2), (1,2) -> (the three diagonal entries, V as three rows).  record: a list
    that receives, after every sweep, the largest |off-diagonal entry|."""
    a = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(sweeps):
        for p, q, r in PAIRS:
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            a[p][q] = a[q][p] = 0.0
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq
                v[k][q] = s * vkp + c * vkq
        if record is not None:
            record.append(max(abs(a[0][1]), abs(a[0][2]), abs(a[1][2])))
    return [a[0][0], a[1][1], a[2][2]], v


def sweeps_needed(C, limit=40):
    """The first number of sweeps after which every off-diagonal entry is 0 or below 2^-52 trace in magnitude."""
    trace = (C[0] + C[3]) + C[5]
    off = []
    jacobi_host(C, limit, off)
    if max(abs(C[1]), abs(C[2]), abs(C[4])) == 0.0:
        return 0
    for k, x in enumerate(off):
        if x == 0.0 or x < EPS * trace:
            return k + 1
    return limit + 1


def oriented_host(n, p, view):
    """The sign rules on the fp64 column n for the query p (fp32) and the viewpoint view (fp32 [3] or None) -> the column as it
    is written (before the narrowing)."""
    dot = 0.0
    if view is not None:
        with np.errstate(all="ignore"):
            d = [float(F64(F32(view[k])) - F64(F32(p[k]))) for k in range(3)]
            dot = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]
    if dot < 0.0:
        flip = True
    elif dot > 0.0:
        flip = False
    else:                                                           # exactly 0 (or NaN: a viewpoint that is not finite)
        k = 0
        if abs(n[1]) > abs(n[k]):
            k = 1
        if abs(n[2]) > abs(n[k]):
            k = 2
        flip = n[k] < 0.0
    return [-x for x in n] if flip else list(n)


def normals_host(queries, cloud, radius, min_neighbours=6, viewpoint=None, sweeps=SWEEPS):
    """All of item 9 -> normals [N,3] fp32, eigenvalues [N,3] fp32, count [N] int32, and what the host tests look at: cov (the
    six fp64 entries in lattice units, None without a neighbour), lattice (the three diagonal entries ascending and the
    oriented fp64 column, in lattice units), needed (sweeps_needed).  viewpoint: None, three values or [N,3]."""
    q, c = np.ascontiguousarray(queries, F32), np.ascontiguousarray(cloud, F32)
    N = q.shape[0]
    h = lattice_h(radius)
    near = neighbours_host(q, c, radius)
    finite = np.isfinite(q).all(1)
    view = None if viewpoint is None else np.asarray(viewpoint, F32)
    out = {"normals": np.zeros((N, 3), F32), "eigenvalues": np.zeros((N, 3), F32), "count": np.zeros(N, np.int32), "cov": [None] * N,
           "lattice": [None] * N, "needed": [0] * N, "h": h}
    for i in range(N):
        if not finite[i]:
            out["normals"][i], out["eigenvalues"][i], out["count"][i] = np.nan, np.nan, -1
            continue
        n, s, S = moments_host(q[i], c[near[i]], h) if near[i].any() else (0, [0] * 3, [0] * 6)
        out["count"][i] = n
        if n == 0:
            continue
        C = covariance_host(n, s, S)
        trace = (C[0] + C[3]) + C[5]
        lam, v = jacobi_host(C, sweeps)
        k = 0
        if lam[1] < lam[k]:
            k = 1
        if lam[2] < lam[k]:
            k = 2
        col = [v[0][k], v[1][k], v[2][k]]
        e = list(lam)                                               # three compare-and-swaps: ascending, equal entries keep their order
        if e[1] < e[0]:
            e[0], e[1] = e[1], e[0]
        if e[2] < e[1]:
            e[1], e[2] = e[2], e[1]
        if e[1] < e[0]:
            e[0], e[1] = e[1], e[0]
        with np.errstate(all="ignore"):
            out["eigenvalues"][i] = [F32(F64(x) * (F64(h) * F64(h))) for x in e]
        col = oriented_host(col, q[i], None if view is None else (view if view.ndim == 1 else view[i]))
        if n >= min_neighbours and trace != 0.0:
            out["normals"][i] = [F32(x) for x in col]
        out["cov"][i], out["lattice"][i], out["needed"][i] = C, (e, col), sweeps_needed(C)
    return out


# ------------------------------------------------------------------------------------------------ lrf_align.inl item 4, restated
def plane_cloud_host(points, closest, index, distance, normals, c, u, gate):
    """-> the 48 words as Python integers (align_cases.plane_host with the unit normal stored for index_i as the plane)."""
    p, q = np.asarray(points, F32).reshape(-1, 3), np.asarray(closest, F32).reshape(-1, 3)
    index, d = np.asarray(index).astype(np.int64), np.asarray(distance, F32)
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    M = nrm.shape[0]
    ok = (index >= 0) & (index < M)
    safe = np.where(ok, index, 0)
    matched = ok & np.isfinite(d)
    with np.errstate(all="ignore"):
        gated = matched & (d > F32(gate))
        n = nrm[safe].astype(F64) if M else np.zeros((p.shape[0], 3))
        nn = _dot(n, n)
        flat = matched & ~gated & (~np.isfinite(nrm[safe]).all(1) | (nn == 0))
        pt, qt = (p.astype(F64) - np.asarray(c, F64)) / float(u), (q.astype(F64) - np.asarray(c, F64)) / float(u)
        inside = (np.abs(pt) <= 1).all(1) & (np.abs(qt) <= 1).all(1)
        far = matched & ~gated & ~flat & ~inside
        use = matched & ~gated & ~flat & inside
        m = n[use] / np.sqrt(nn[use])[:, None]
        pt, qt = pt[use], qt[use]
        r = _dot(m, pt - qt)
        J = np.concatenate([_cross(pt, m), m, _dot(pt, m)[:, None]], 1)

        def total(v):
            return sum(int(t) for t in np.rint(v * PLANE_SCALE))
        w = [0] * 48
        w[:5] = int(use.sum()), int((~matched).sum()), int(gated.sum()), int(flat.sum()), int(far.sum())
        w[6] = total(r * r)
        at = 14
        for k in range(7):
            w[7 + k] = total(J[:, k] * r)
            for l in range(k, 7):
                w[at] = total(J[:, k] * J[:, l])
                at += 1
    return w


@functools.lru_cache(maxsize=None)
def plane_cloud_case():
    """The scan with the restatement's normals, two of them spoilt (a zero row, a row with a NaN) under points that pass the
    gate, and a cloud with a far point and a NaN point (unmatched), points beyond the gate and points beyond the frame
    -> (scan, normals, cloud, c, u, max_distance, gate, the brute force's closest / index / distance for the cloud)."""
    B, c, u, max_distance, gate = scan(), (-0.95, 0.0, 0.0), 2.0, 0.3, 0.04
    cloud = np.concatenate([scan_source(0, True), np.array([(9, 9, 9), (np.nan, 0, 0)], F32)])
    near = closest_host(cloud, B, max_distance)
    normals = scan_normals()["normals"].copy()
    with np.errstate(all="ignore"):
        ok = np.isfinite(near["distance"]) & (near["distance"] <= F32(gate)) & (np.abs((cloud.astype(F64) - c) / u) <= 1).all(1)
    spoilt = np.unique(near["index"][ok])[:2]
    assert spoilt.shape == (2,)
    normals[spoilt[0]], normals[spoilt[1], 1] = 0.0, np.nan
    return B, normals, cloud, c, u, max_distance, gate, near


def _power_of_two_at_least(x):
    m, e = math.frexp(x)
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def cloud_frame(target, cloud):
    """icp's frame for max_distance = inf: (the centre of the target's box, u the smallest power of two that covers the box of
    the target and of the cloud with half its longest edge around it)."""
    t, s = np.asarray(target, F32).astype(F64), np.asarray(cloud, F32).astype(F64)
    c = tuple((float(l) + float(h)) / 2.0 for l, h in zip(t.min(0), t.max(0)))
    lo, hi = np.minimum(t.min(0), s.min(0)), np.maximum(t.max(0), s.max(0))
    pad = 0.5 * float((hi - lo).max())
    return c, _power_of_two_at_least(float(((hi + pad) - (lo - pad)).max()))


def icp_plane_cloud_host(cloud, target, normals, scale, iterations=20, tol=1e-7):
    """alignment.icp(metric="plane", target_normals=...) against a CloudIndex with the restatements in place of the kernels
    -> (T, history of steps)."""
    from localrf_amd import alignment
    T = np.eye(4)
    c, u = cloud_frame(target, transform_host(T[:3], cloud))
    steps = []
    for _ in range(iterations):
        cur = transform_host(T[:3], cloud)
        near = closest_host(cur, target, math.inf)
        sol = alignment.solve_plane(plane_cloud_host(cur, near["closest"], near["index"], near["distance"], normals, c, u, F32(np.inf)), scale)
        assert sol["omega"] is not None, sol
        T = alignment.compose(alignment.plane_update(sol, c, u), T)
        hit = near["index"] >= 0
        c = tuple(float(v) for v in near["closest"][hit].astype(F64).sum(0) / hit.sum())
        steps.append(max(float(np.linalg.norm(sol["omega"])), abs(sol["sigma"]), float(np.linalg.norm(sol["tau"]))))
        if steps[-1] < tol:
            break
    return T, steps


# ------------------------------------------------------------------------------------------------ the cases
def fibonacci(n=4099):
    """n unit directions in fp64: z_i = 1 - (2 i + 1) / n, the azimuth advancing by the golden angle."""
    i = np.arange(n, dtype=F64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def sphere_spacing(n=4099):
    return math.sqrt(4.0 * math.pi / n)


@functools.lru_cache(maxsize=None)
def sphere():
    return np.ascontiguousarray(fibonacci().astype(F32))


def plane_lattice():
    """9 x 9 points at z = 0.5 with step 0.125: every coordinate a multiple of the lattice step of radius 0.3 (2^-16)."""
    g = np.arange(9, dtype=F32) * F32(0.125)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, np.full_like(x, 0.5)], -1).reshape(-1, 3), F32)


def _case(cloud, queries=None, radius=0.5, min_neighbours=6, viewpoint=None):
    cloud = np.ascontiguousarray(cloud, F32)
    own = queries is None
    return {"cloud": cloud, "queries": cloud if own else np.ascontiguousarray(queries, F32), "own": own, "radius": float(radius),
            "min_neighbours": int(min_neighbours), "viewpoint": viewpoint}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> cloud [M,3], queries [N,3] (own: they are the cloud), radius, min_neighbours, viewpoint (None, 3 floats or [N,3])."""
    out = {}
    for m in (0, 1, 2, 3, 64, 65):
        out[f"random M={m}"] = _case(random_cloud(m, 110 + m), random_cloud(65, 120 + m, 1.1), radius=0.75)
    out["random M=65 on itself"] = _case(random_cloud(65, 130), radius=0.75, viewpoint=(0.25, -3.0, 0.5))
    s = sphere()
    r3 = 3.0 * sphere_spacing()
    out["sphere, viewpoint inside"] = _case(s, radius=r3, viewpoint=(0.0, 0.0, 0.0))
    out["sphere, viewpoints outside"] = _case(s, radius=r3, viewpoint=np.ascontiguousarray(s * F32(2.0)))
    rng = np.random.default_rng(7200)
    off = (s[rng.permutation(4099)[:65]].astype(F64) * rng.uniform(0.97, 1.03, (65, 1)) + rng.normal(0, 0.01, (65, 3))).astype(F32)
    out["sphere, queries off the cloud"] = _case(s, off, radius=r3)
    lat = plane_lattice()
    out["planar lattice"] = _case(lat, radius=0.3)
    out["planar lattice, min_neighbours at a corner's 8"] = _case(lat, radius=0.3, min_neighbours=8)
    out["planar lattice, min_neighbours above a corner's 8"] = _case(lat, radius=0.3, min_neighbours=9)
    out["planar lattice, viewpoint below"] = _case(lat, radius=0.3, viewpoint=(0.5, 0.25, -2.0))
    out["planar lattice, viewpoint in the plane"] = _case(lat, radius=0.3, viewpoint=(3.0, 1.0, 0.5))
    line = np.zeros((64, 3), F32)
    line[:, 0] = np.random.default_rng(7201).uniform(-2.0, 2.0, 64)
    out["line"] = _case(line, radius=0.5, min_neighbours=3)
    same = np.tile(np.array([[1.5, 2.5, -0.5]], F32), (70, 1))
    out["70 identical points"] = _case(same, np.concatenate([same[:3], random_cloud(30, 140, 0.5) + same[:1]]), radius=0.75)
    cloud, q = planted()
    out["planted distance"] = _case(cloud, q, radius=1.25, min_neighbours=3)
    bad = random_cloud(65, 150)
    bad[[0, 7, 33], [0, 1, 2]] = np.nan
    bad[[12, 64], [1, 0]] = np.inf
    bad[40, 2] = -np.inf
    out["cloud entries that are not finite"] = _case(bad, radius=0.75)
    qbad = random_cloud(64, 151)
    qbad[[1, 5], [0, 2]] = np.nan
    qbad[9, 1] = np.inf
    qbad[63] = -np.inf
    out["queries that are not finite"] = _case(random_cloud(65, 152), qbad, radius=0.75)
    out["coordinates near 1e30"] = _case(random_cloud(65, 153, 1e30), random_cloud(64, 154, 1.1e30), radius=1.2e30)
    out["no finite point"] = _case(np.full((5, 3), np.nan, F32), qbad[:12], radius=0.75)
    return out


CASE_NAMES = tuple(f"random M={m}" for m in (0, 1, 2, 3, 64, 65)) + (
    "random M=65 on itself", "sphere, viewpoint inside", "sphere, viewpoints outside", "sphere, queries off the cloud", "planar lattice",
    "planar lattice, min_neighbours at a corner's 8", "planar lattice, min_neighbours above a corner's 8", "planar lattice, viewpoint below",
    "planar lattice, viewpoint in the plane", "line", "70 identical points", "planted distance", "cloud entries that are not finite",
    "queries that are not finite", "coordinates near 1e30", "no finite point")


@functools.lru_cache(maxsize=None)
def expected(name):
    """normals_host for cases()[name], computed once and shared."""
    c = cases()[name]
    return normals_host(c["queries"], c["cloud"], c["radius"], c["min_neighbours"], c["viewpoint"])


# ------------------------------------------------------------------------------------------------ the registration
def surface(d):
    """align_cases.blob's radius function 1 + 0.35 x + 0.25 y^2 - 0.2 z x + 0.3 max(z, 0)^2 + 0.15 x y z of unit directions d
    [n,3] fp64, axes scaled by (1, 0.8, 0.6) -> points [n,3] fp64."""
    x, y, z = d.T
    r = 1 + 0.35 * x + 0.25 * y * y - 0.2 * z * x + 0.3 * np.maximum(z, 0) ** 2 + 0.15 * x * y * z
    return r[:, None] * d * (1.0, 0.8, 0.6)


@functools.lru_cache(maxsize=None)
def scan():
    """Target B: the surface at the 4099 Fibonacci directions, fp32."""
    return np.ascontiguousarray(surface(fibonacci()).astype(F32))


@functools.lru_cache(maxsize=None)
def scan_source_points():
    d = np.random.default_rng(3).standard_normal((1500, 3))
    p = surface(d / np.linalg.norm(d, axis=1, keepdims=True))
    p.setflags(write=False)
    return p


def scan_source(k, free):
    """1500 other points of the same surface moved by the inverse of align_cases.truth(k, free), fp32."""
    return np.ascontiguousarray(apply(sim_inverse(truth(k, free)), scan_source_points()).astype(F32))


SCAN_RUNS = tuple((k, free) for k in range(3) for free in (True, False))


@functools.lru_cache(maxsize=None)
def scan_spacing():
    """The lower median of the scan's nearest-neighbour distances, the (float) of the fp64 root, as nearest_spacing gives it."""
    B = scan().astype(F64)
    best = np.full(B.shape[0], np.inf)
    for i0 in range(0, B.shape[0], 512):
        d = B[i0:i0 + 512, None, :] - B[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2[np.arange(d2.shape[0]), np.arange(i0, i0 + d2.shape[0])] = np.inf
        best[i0:i0 + 512] = d2.min(1)
    nn = np.sort(np.sqrt(best).astype(F32))
    return float(nn[(nn.size - 1) // 2])


@functools.lru_cache(maxsize=None)
def scan_normals():
    """normals_host of the scan on itself at 4 median spacings."""
    B = scan()
    return normals_host(B, B, 4.0 * scan_spacing())
