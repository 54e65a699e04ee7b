"""Shared pieces of the point-cloud tests: the numpy restatements of csrc/lrf_cloud.inl by other algorithms -- a brute force over
all pairs in fp64 in the .inl's operation order with argmin / a stable sort / a comparison for the three queries, the grid walk
in pure Python over a dict of cells for the stopping rule, np.unique and np.add.at for the voxel grid (the cell of a point is
tests/mesh_simplify_cases.py's cells_host, imported, not copied) -- and the cases, the smallest at which each rule can go wrong."""
import functools
import math

import numpy as np

from mesh_distance_cases import dims_host
from mesh_simplify_cases import Q_ONE, cells_host

F32 = np.float32
QUERY_SIZES = (0, 1, 63, 64, 65, 1025)
CLOUD_SIZES = (0, 1, 64, 65, 4099)
KS = (1, 2, 3, 8)
SLACK = 1.0 - 2.0 ** -20
NONE = np.iinfo(np.int32).max


# ------------------------------------------------------------------------------------------------ the restatements
def used_host(cloud):
    return np.isfinite(cloud).all(1)


def pairs_host(queries, cloud):
    """d2 [N,M] fp64: (d0 d0 + d1 d1) + d2 d2 with d_k = (double)p_k - (double)q_k, every operation rounded on its own; +inf in
    the column of a cloud point that is not used.  Rows of queries that are not finite hold garbage; the callers mask them."""
    with np.errstate(all="ignore"):
        d = queries.astype(np.float64)[:, None, :] - cloud.astype(np.float64)[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[:, ~used_host(cloud)] = np.inf
    return d2


def _without_self(d2):
    d2 = d2.copy()
    assert d2.shape[0] == d2.shape[1]
    d2[np.arange(d2.shape[0]), np.arange(d2.shape[0])] = np.inf
    return d2


def closest_host(queries, cloud, max_distance, d2=None):
    """-> distance [N] fp32, index [N] int32, closest [N,3] fp32, d2 [N] fp64 (the winner's; +inf without one)."""
    n, m = queries.shape[0], cloud.shape[0]
    d2 = pairs_host(queries, cloud) if d2 is None else d2
    finite = np.isfinite(queries).all(1)
    if m:
        idx = d2.argmin(1)                                          # the first minimum: the smallest index among equal d2
        best = d2[np.arange(n), idx]
    else:
        idx, best = np.zeros(n, np.int64), np.full(n, np.inf)
    hit = finite & np.isfinite(best) & ~(best > np.float64(max_distance) * np.float64(max_distance))
    distance = np.where(hit, np.sqrt(np.where(hit, best, 0.0)), np.inf).astype(F32)
    distance[~finite] = np.nan
    closest = np.full((n, 3), np.nan, F32)
    if m:
        closest[hit] = cloud[idx[hit]]
    return {"distance": distance, "index": np.where(hit, idx, -1).astype(np.int32), "closest": closest,
            "d2": np.where(hit, best, np.inf)}


def knn_host(queries, cloud, k, max_distance, exclude_self=False, d2=None):
    """-> distance [N,k] fp32, index [N,k] int32, ascending in (d2, index): a stable sort of each row."""
    n, m = queries.shape[0], cloud.shape[0]
    d2 = pairs_host(queries, cloud) if d2 is None else d2
    if exclude_self:
        d2 = _without_self(d2)
    finite = np.isfinite(queries).all(1)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    best = np.take_along_axis(d2, order, 1)
    if m < k:
        order = np.concatenate([order, np.zeros((n, k - m), np.int64)], 1)
        best = np.concatenate([best, np.full((n, k - m), np.inf)], 1)
    hit = finite[:, None] & np.isfinite(best) & ~(best > np.float64(max_distance) * np.float64(max_distance))
    distance = np.where(hit, np.sqrt(np.where(hit, best, 0.0)), np.inf).astype(F32)
    distance[~finite] = np.nan
    return {"distance": distance, "index": np.where(hit, order, -1).astype(np.int32)}


def radius_count_host(queries, cloud, radius, exclude_self=False, d2=None):
    d2 = pairs_host(queries, cloud) if d2 is None else d2
    if exclude_self:
        d2 = _without_self(d2)
    count = (d2 <= np.float64(radius) * np.float64(radius)).sum(1).astype(np.int32)
    count[~np.isfinite(queries).all(1)] = -1
    return count


def box_host(cloud):
    """(lo, hi) of the used points as tuples of Python floats (-0 counts as +0); None without a used point."""
    u = cloud[used_host(cloud)]
    if not u.shape[0]:
        return None
    return tuple(float(x) + 0.0 for x in u.min(0)), tuple(float(x) + 0.0 for x in u.max(0))


def default_point_cell_host(lo, hi, used, max_bytes=1 << 30):
    longest = max(h - l for l, h in zip(lo, hi))
    if not longest > 0 or used < 1:
        return 1.0
    cell = longest * 2.0 / math.sqrt(used)
    while True:
        cells = math.prod(dims_host(lo, hi, cell))
        if cells < 1 << 31 and (8 * cells <= max_bytes // 2 or cells == 1):
            return cell
        cell *= 2.0


def cell_sweep(cloud):
    """(None, default / 4, default x 4, one cell for the whole box), and the default itself; () without a used point."""
    box = box_host(cloud)
    if box is None:
        return (None,), None
    lo, hi = box
    default = default_point_cell_host(lo, hi, int(used_host(cloud).sum()))
    longest = max(h - l for l, h in zip(lo, hi))
    whole = 2.0 * longest if longest > 0 else 3.0
    assert dims_host(lo, hi, whole) == (1, 1, 1)
    return (None, default / 4.0, default * 4.0, whole), default


def _cell_of(x, lo, cell, dims):
    with np.errstate(all="ignore"):
        t = np.floor((x.astype(np.float64) - np.asarray(lo, np.float64)) / np.float64(cell))
    return np.clip(np.where(np.isnan(t), 0.0, t), 0, np.asarray(dims) - 1).astype(np.int64)


def grid_host(cloud, cell):
    """-> (lo, dims, {(cx, cy, cz): indices of the used points of that cell})."""
    lo, hi = box_host(cloud)
    dims = dims_host(lo, hi, cell)
    use = np.nonzero(used_host(cloud))[0]
    c = _cell_of(cloud[use], lo, cell, dims)
    cells = {}
    for i, key in zip(use.tolist(), map(tuple, c.tolist())):
        cells.setdefault(key, []).append(i)
    return lo, dims, {k: np.array(v) for k, v in cells.items()}


def grid_walk_host(queries, cloud, cell, limit, d2, mode, k=1, exclude_self=False):
    """The .inl's shells and stopping rule in pure Python for the finite queries, over the brute force's d2 rows.
    mode "closest" -> (best d2 [N], index [N]); "knn" -> (d2 [N,k], index [N,k]); "count" -> counts [N] (limit = the radius);
    and the shells walked per query.  Unvisited points stay unknown to the walk: what it returns is what the kernel would."""
    lo, dims, cells = grid_host(cloud, cell)
    n = queries.shape[0]
    out_d = np.full((n, k), np.inf)
    out_i = np.full((n, k), NONE, np.int64)
    counts = np.zeros(n, np.int64)
    shells = np.zeros(n, np.int64)
    r2 = np.float64(limit) * np.float64(limit)
    for q in np.nonzero(np.isfinite(queries).all(1))[0].tolist():
        c = _cell_of(queries[q], lo, cell, dims).tolist()
        rmax = max(max(c[a], dims[a] - 1 - c[a]) for a in range(3))
        found = []                                                  # (d2, index) of every point met
        r = 0
        while True:
            box = [(max(c[a] - r, 0), min(c[a] + r, dims[a] - 1)) for a in range(3)]
            for z in range(box[2][0], box[2][1] + 1):
                for y in range(box[1][0], box[1][1] + 1):
                    on_shell = abs(z - c[2]) == r or abs(y - c[1]) == r
                    xs = range(box[0][0], box[0][1] + 1) if on_shell else [x for x in (c[0] - r, c[0] + r) if 0 <= x <= dims[0] - 1]
                    for x in xs:
                        for i in cells.get((x, y, z), ()):
                            if not (exclude_self and i == q):
                                found.append((float(d2[q, i]), int(i)))
            found.sort()
            bound = (float(r) * cell) * SLACK
            deciding = found[k - 1][0] if mode != "count" and len(found) >= k else math.inf
            if deciding < bound * bound or r >= rmax or bound > limit:
                break
            r += 1
        shells[q] = r
        for j, (e, i) in enumerate(found[:k]):
            out_d[q, j], out_i[q, j] = e, i
        counts[q] = sum(e <= r2 for e, _ in found)
    if mode == "count":
        return counts, shells
    return out_d, out_i, shells


def voxel_host(points, cell, origin=(0.0, 0.0, 0.0), rgb8=None):
    """The voxel rule -> points [C,3] fp32, rgb8 [C,3] uint8 or None, count [C] int32, cluster_of [M] int32, box (lo, dims), bad."""
    m = points.shape[0]
    i, q, bad = cells_host(points, cell, origin) if m else (np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint64), np.zeros(0, bool))
    good = ~bad
    cluster_of = np.full(m, -1, np.int32)
    if not good.any():
        return {"points": np.zeros((0, 3), F32), "rgb8": None if rgb8 is None else np.zeros((0, 3), np.uint8), "count": np.zeros(0, np.int32),
                "cluster_of": cluster_of, "box": ((0, 0, 0), (0, 0, 0)), "bad": int(bad.sum())}
    lo = i[good].min(0)
    dims = i[good].max(0) - lo + 1
    rel = i[good] - lo
    linear = (rel[:, 2] * dims[1] + rel[:, 1]) * dims[0] + rel[:, 0]
    occupied, inv = np.unique(linear, return_inverse=True)
    inv = inv.reshape(-1)
    cluster_of[good] = inv
    nc = occupied.size
    S = np.zeros((nc, 3), np.uint64)
    np.add.at(S, inv, q[good])
    n = np.bincount(inv, minlength=nc)
    ci = np.stack([occupied % dims[0], occupied // dims[0] % dims[1], occupied // (dims[0] * dims[1])], 1) + lo
    mean = S.astype(np.float64) / n.astype(np.float64)[:, None]
    frac = mean * (1.0 / Q_ONE)
    t = ci.astype(np.float64) + frac
    x = t * np.float64(cell)
    pos = (np.asarray(origin, np.float64) + x).astype(F32)
    rgb = None
    if rgb8 is not None:
        C = np.zeros((nc, 3), np.int64)
        np.add.at(C, inv, rgb8[good].astype(np.int64))
        rgb = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    return {"points": pos, "rgb8": rgb, "count": n.astype(np.int32), "cluster_of": cluster_of,
            "box": (tuple(int(v) for v in lo), tuple(int(v) for v in dims)), "bad": int(bad.sum())}


def summary_counts_host(distance, taus):
    """The integer words of distance_summary that cloud_distance's ratios are formed from: finite, beyond, nan, within."""
    d = np.asarray(distance, F32)
    fin = np.isfinite(d)
    return {"finite": int(fin.sum()), "beyond": int(np.isinf(d).sum()), "nan": int(np.isnan(d).sum()),
            "within": tuple(int((d[fin] <= F32(t)).sum()) for t in taus)}


# ------------------------------------------------------------------------------------------------ the cases
def _rng(seed):
    return np.random.default_rng(7000 + seed)


def random_cloud(m, seed, scale=1.0):
    return (_rng(seed).uniform(-1.0, 1.0, (m, 3)) * scale).astype(F32)


def lattice():
    """A 5 x 5 x 5 lattice queried at its cell centres (8 equally near points), face centres (4), edge midpoints (2) and corners
    (the points themselves)."""
    g = np.arange(5, dtype=F32)
    cloud = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    h = np.arange(4, dtype=F32) + F32(0.5)
    centres = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    faces = np.stack(np.meshgrid(h, h, g, indexing="ij"), -1).reshape(-1, 3)
    edges = np.stack(np.meshgrid(h, g, g, indexing="ij"), -1).reshape(-1, 3)[:, [1, 0, 2]]
    return np.ascontiguousarray(cloud), np.ascontiguousarray(np.concatenate([centres, faces, edges, cloud]), dtype=F32)


def triplicates():
    base = random_cloud(65, 1)
    return np.ascontiguousarray(np.concatenate([base, base, base])[_rng(2).permutation(195)])


@functools.lru_cache(maxsize=None)
def sphere():
    """4099 seeded points on the unit sphere; 1025 queries: on it (cloud points and jittered ones), inside it (at 0.8 to 0.95 of
    the radius, one at the centre) and outside the box.  Queried with max_distance 0.3, so that no lane walks far."""
    rng = _rng(3)
    v = rng.standard_normal((4099, 3))
    cloud = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    w = rng.standard_normal((1025, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    q = np.concatenate([cloud[:200], cloud[200:400] + rng.normal(0, 0.01, (200, 3)), w[:300] * rng.uniform(0.8, 0.95, (300, 1)),
                        w[300:624] * rng.uniform(1.05, 1.9, (324, 1)), np.zeros((1, 3))]).astype(F32)
    q = q[rng.permutation(1025)]
    assert q.shape == (1025, 3) and (np.abs(q).max(1) > 1.0).sum() > 50
    return cloud, np.ascontiguousarray(q)


def planted():
    """One point at the origin and 69 far ones; queries at exactly 1.25 from the origin ((0.75, 1, 0): d2 = 1.5625, exact), one
    ulp-ish further, and nearer.  max_distance = radius = 1.25: the boundary is inclusive for the hit and for the count."""
    far = random_cloud(69, 4) + F32(12.0)
    cloud = np.concatenate([np.zeros((1, 3), F32), far])
    q = np.array([(0.75, 1.0, 0.0), (0.75, 1.0, 2.0 ** -10), (0.75, -1.0, 0.0), (0.5, 0.5, 0.5), (-1.25, 0.0, 0.0), (0.0, 1.25, 2.0 ** -12)], F32)
    return np.ascontiguousarray(cloud), q


def _case(cloud, queries, max_distance=math.inf, radius=0.5, self_queries=False, walk=None):
    return {"cloud": np.ascontiguousarray(cloud, F32), "queries": np.ascontiguousarray(queries, F32), "max_distance": float(max_distance),
            "radius": float(radius), "self": self_queries, "walk": walk}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> cloud [M,3], queries [N,3], max_distance, radius, self (queries are the cloud: exclude_self runs too) and walk
    (how many queries the pure-Python grid walk takes; None: all)."""
    out = {}
    for m in CLOUD_SIZES[:4]:
        out[f"random M={m} N=65"] = _case(random_cloud(m, 10 + m), random_cloud(65, 20 + m, 1.2))
    for n in QUERY_SIZES[:4]:
        out[f"random M=65 N={n}"] = _case(random_cloud(65, 30), random_cloud(n, 40 + n, 1.2))
    cloud, q = lattice()
    out["lattice"] = _case(cloud, q, radius=1.0)
    out["lattice on itself"] = _case(cloud, cloud, radius=1.0, self_queries=True)
    t = triplicates()
    out["triplicates"] = _case(t, np.concatenate([random_cloud(64, 5), t[:30]]), radius=0.25)
    out["triplicates on themselves"] = _case(t, t, radius=0.25, self_queries=True)
    line = np.zeros((64, 3), F32)
    line[:, 0] = _rng(6).uniform(-2.0, 2.0, 64)
    out["line"] = _case(line, random_cloud(65, 7, 2.0) * np.array([1.0, 0.2, 0.2], F32))
    out["a single point"] = _case(np.array([[0.3, -0.2, 7.0]], F32), random_cloud(63, 8) + np.array([0.3, -0.2, 7.0], F32), radius=1.0)
    same = np.tile(np.array([[1.5, 2.5, -0.5]], F32), (70, 1))
    out["70 identical points"] = _case(same, np.concatenate([same[:3], random_cloud(61, 9) + same[:1]]), radius=0.75)
    out["70 identical points on themselves"] = _case(same, same, radius=0.0, self_queries=True)
    cloud, q = sphere()
    out["sphere"] = _case(cloud, q, max_distance=0.3, radius=0.1, walk=65)
    bad = random_cloud(65, 11)
    bad[[0, 7, 33], [0, 1, 2]] = np.nan
    bad[[12, 64], [1, 0]] = np.inf
    bad[40, 2] = -np.inf
    out["cloud entries that are not finite"] = _case(bad, np.concatenate([random_cloud(60, 12), random_cloud(65, 11)[[0, 7, 12, 40, 64]]]))
    qbad = random_cloud(64, 13)
    qbad[[1, 5], [0, 2]] = np.nan
    qbad[9, 1] = np.inf
    qbad[63] = -np.inf
    out["queries that are not finite"] = _case(random_cloud(65, 14), qbad)
    out["coordinates near 1e30"] = _case(random_cloud(65, 15, 1e30), random_cloud(64, 16, 1.2e30), radius=5e29)
    cloud, q = planted()
    out["planted distance"] = _case(cloud, q, max_distance=1.25, radius=1.25)
    out["no finite point"] = _case(np.full((5, 3), np.nan, F32), qbad[:12])
    return out


CASE_NAMES = tuple(f"random M={m} N=65" for m in CLOUD_SIZES[:4]) + tuple(f"random M=65 N={n}" for n in QUERY_SIZES[:4]) + (
    "lattice", "lattice on itself", "triplicates", "triplicates on themselves", "line", "a single point", "70 identical points",
    "70 identical points on themselves", "sphere", "cloud entries that are not finite", "queries that are not finite",
    "coordinates near 1e30", "planted distance", "no finite point")


@functools.lru_cache(maxsize=None)
def pairs(name):
    c = cases()[name]
    return pairs_host(c["queries"], c["cloud"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The brute force's results for cases()[name], computed once and shared: closest, knn[k], count, and with self knn_self[k]
    and count_self; info (points, nonfinite_points)."""
    c, d2 = cases()[name], pairs(name)
    q, cloud = c["queries"], c["cloud"]
    out = {"closest": closest_host(q, cloud, c["max_distance"], d2), "knn": {k: knn_host(q, cloud, k, c["max_distance"], False, d2) for k in KS},
           "count": radius_count_host(q, cloud, c["radius"], False, d2),
           "info": {"points": int(used_host(cloud).sum()), "nonfinite_points": int((~used_host(cloud)).sum())}}
    if c["self"]:
        out["knn_self"] = {k: knn_host(q, cloud, k, c["max_distance"], True, d2) for k in KS}
        out["count_self"] = radius_count_host(q, cloud, c["radius"], True, d2)
    return out


# ------------------------------------------------------------------------------------------------ voxel grid, outliers, ICP
def voxel_cases():
    """name -> (points, rgb8, cell, origin)."""
    rng = _rng(50)
    cloud, _ = sphere()
    col = rng.integers(0, 256, (4099, 3), dtype=np.uint8)
    bad = cloud[:200].copy()
    bad[[3, 50], [0, 2]] = np.nan
    bad[120, 1] = np.inf
    bad[7] = (3e9, 0.0, 0.0)                                        # 2^30 cells of 0.25 and more from the origin
    lat = rng.integers(-5, 6, (400, 3)).astype(F32)                 # with cell = 1 every point lies on a cell boundary
    return {"sphere at 0.11": (cloud, col, 0.11, (0.0, 0.0, 0.0)), "sphere at 0.07, anchored": (cloud, None, 0.07, (0.1, -0.03, 0.017)),
            "one cell": (cloud[:65], col[:65], 8.0, (-4.0, -4.0, -4.0)), "a single point": (cloud[:1], col[:1], 0.5, (0.0, 0.0, 0.0)),
            "bad points": (bad, col[:200], 0.25, (0.0, 0.0, 0.0)), "lattice points": (lat, col[:400], 1.0, (0.0, 0.0, 0.0)),
            "no good point": (np.full((4, 3), np.nan, F32), col[:4], 1.0, (0.0, 0.0, 0.0))}


@functools.lru_cache(maxsize=None)
def surface_with_floaters():
    """A bumpy sheet of 48 x 48 points (spacing 1/48) and two floater clusters of 3 and 5 points well off it.  With radius =
    2.5 spacings every sheet point has at least 8 others within reach (a corner: the 3 x 3 block around it and more)."""
    g = (np.arange(48) + 0.5) / 48
    x, y = np.meshgrid(g, g, indexing="ij")
    sheet = np.stack([x, y, 0.05 * np.sin(5 * x) * np.cos(4 * y)], -1).reshape(-1, 3)
    rng = _rng(60)
    f1 = np.array([0.3, 0.3, 0.6]) + rng.normal(0, 0.004, (3, 3))
    f2 = np.array([0.8, 0.2, -0.5]) + rng.normal(0, 0.004, (5, 3))
    pts = np.concatenate([sheet, f1, f2])
    order = rng.permutation(pts.shape[0])
    floater = np.concatenate([np.zeros(sheet.shape[0], bool), np.ones(8, bool)])[order]
    return np.ascontiguousarray(pts[order], dtype=F32), floater, 2.5 / 48


@functools.lru_cache(maxsize=None)
def icp_case():
    """Target B: a bumpy, jittered sheet of 24 x 24 points; source A = B moved by a planted rigid motion that moves no point by
    more than a quarter of B's smallest nearest-neighbour distance (asserted here, in fp64 on the host): the first
    correspondences are then the twins.  -> (A, B, T planted (A = T B), smallest nearest-neighbour distance, largest move)."""
    rng = _rng(70)
    g = (np.arange(24) + 0.5) / 24
    x, y = np.meshgrid(g, g, indexing="ij")
    B = np.stack([x, y, 0.15 * np.sin(4 * x) * np.cos(3 * y) + 0.1 * x * x], -1).reshape(-1, 3)
    B = (B + rng.uniform(-0.2, 0.2, B.shape) / 24).astype(F32)
    d2 = pairs_host(B, B)
    np.fill_diagonal(d2, np.inf)
    nn = float(np.sqrt(d2.min()))
    w = np.array([0.002, -0.0015, 0.0025])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (math.sin(th) / th) * K + ((1 - math.cos(th)) / th ** 2) * (K @ K)
    c = B.astype(np.float64).mean(0)
    t = c - R @ c + np.array([0.0008, -0.0005, 0.001])
    A = (B.astype(np.float64) @ R.T + t).astype(F32)
    move = float(np.linalg.norm(A.astype(np.float64) - B.astype(np.float64), axis=1).max())
    assert move <= 0.25 * nn, (move, nn)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return A, B, T, nn, move
