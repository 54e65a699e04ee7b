"""Cases and numpy restatements for the registration (csrc/lrf_align.inl, localrf_amd/alignment.py):

  transform_host   item 1, the fp64 expression rounded once to fp32
  pairs_host       item 2, the 24 words as Python integers
  plane_host       item 3, the 48 words as Python integers, from closest / face / distance as lrf_mesh_closest writes them
  closest_host     the brute force of mesh_distance_cases (pair_host over every face)
  umeyama_host     the similarity of corresponding pairs in plain fp64 numpy: another route than the integer moments
  icp_plane_host   the plane iteration with closest_host, plane_host and the module's host solves

Everything is generated from seeds; nothing is read from disk."""
import functools
import math

import numpy as np

from mesh_distance_cases import _cross, _dot, closest_from_pairs, pair_host, used_faces
from mesh_raster_cases import octa_sphere

F32, F64 = np.float32, np.float64
PAIR_SIZES = (1, 63, 64, 65, 1025, 1 << 20)
TRANSFORM_SIZES = (1, 63, 64, 65, 1025)
AXIS = (2.0, -1.0, 1.0)
# (rotation in rad about AXIS, scale, shift s with t = (s, -s, s / 2), max_distance)
PERTURBATIONS = ((0.10, 1.05, 0.05, math.inf), (0.2, 1.1, 0.1, math.inf), (0.35, 0.9, 0.15, math.inf), (0.2, 1.1, 0.1, 0.15))
ICP_RUNS = tuple((k, free) for k in range(len(PERTURBATIONS)) for free in (True, False))
ICP_BAR = 1e-5
PLANE_SCALE = 2.0 ** 36


def rot(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def sim(angle, scale, shift, axis=AXIS, t=None):
    T = np.eye(4)
    T[:3, :3] = scale * rot(axis, angle)
    T[:3, 3] = (shift, -shift, shift / 2) if t is None else t
    return T


def sim_inverse(T):
    B = np.linalg.inv(T[:3, :3])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = B, -B @ T[:3, 3]
    return out


def apply(T, p):
    return np.asarray(p, F64) @ T[:3, :3].T + T[:3, 3]


def truth(k, free):
    """The similarity run (k, free) has to recover: perturbation k, with scale 1 when the scale is not free."""
    angle, scale, shift, _ = PERTURBATIONS[k]
    return sim(angle, scale if free else 1.0, shift)


def parts(T):
    """(scale, rotation, translation) of a similarity, without the module under test."""
    s = np.linalg.det(T[:3, :3]) ** (1 / 3)
    return s, T[:3, :3] / s, T[:3, 3]


def deviation(T, want):
    """The largest difference in scale, any rotation entry and any translation component."""
    (s, R, t), (s0, R0, t0) = parts(T), parts(want)
    return max(abs(s - s0), float(np.abs(R - R0).max()), float(np.abs(t - t0).max()))


@functools.lru_cache(maxsize=None)
def blob():
    """octa_sphere(3) around its box centre with the radius 1 + 0.35 x + 0.25 y^2 - 0.2 z x + 0.3 max(z, 0)^2 + 0.15 x y z of the
    unit direction, axes scaled by (1, 0.8, 0.6): 512 faces, no symmetry."""
    m = octa_sphere(3)
    v = m["vertices"].astype(F64)
    d = v - (v.min(0) + v.max(0)) / 2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d.T
    r = 1 + 0.35 * x + 0.25 * y * y - 0.2 * z * x + 0.3 * np.maximum(z, 0) ** 2 + 0.15 * x * y * z
    out = {"vertices": np.ascontiguousarray((r[:, None] * d * (1.0, 0.8, 0.6)).astype(F32)), "faces": np.ascontiguousarray(m["faces"], np.int32),
           "rgb8": None, "counts": m["counts"]}
    assert out["faces"].shape[0] == 512
    return out


@functools.lru_cache(maxsize=None)
def blob_points(n=1500):
    """n points on the blob's surface in fp64: face by integers, weights by dirichlet((1, 1, 1)), from default_rng(3)."""
    rng = np.random.default_rng(3)
    m = blob()
    f = rng.integers(0, m["faces"].shape[0], n)
    w = rng.dirichlet((1, 1, 1), n)
    p = (w[:, :, None] * m["vertices"][m["faces"][f]].astype(F64)).sum(1)
    p.setflags(write=False)
    return p


def source_cloud(T):
    """The blob's points moved by the inverse of T, rounded to fp32: what T has to bring back."""
    return np.ascontiguousarray(apply(sim_inverse(T), blob_points()).astype(F32))


# ------------------------------------------------------------------------------------------------ item 1
def transform_host(T, p):
    T, p = np.asarray(T, F64).reshape(-1)[:12], np.asarray(p, F32).astype(F64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3] for k in range(3)], 1).astype(F32)


# ------------------------------------------------------------------------------------------------ item 2
def pairs_host(c, h, a, b, keep=None):
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    n = a.shape[0]
    x = np.concatenate([a, b], 1)
    kept = np.ones(n, bool) if keep is None else np.asarray(keep).astype(bool)
    finite = np.isfinite(x).all(1)
    with np.errstate(all="ignore"):
        r = np.rint((x.astype(F64) - np.tile(np.asarray(c, F64), 2)) / float(h))
        inside = (np.abs(r) < 2.0 ** 20).all(1)
    use = kept & finite & inside
    w = [0] * 24
    w[0], w[1], w[2], w[3] = int(use.sum()), int((kept & finite & ~inside).sum()), int((~kept).sum()), int((kept & ~finite).sum())
    q = r[use].astype(np.int64)
    qa, qb = q[:, :3], q[:, 3:]
    for j in range(3):
        w[4 + j], w[7 + j] = int(qa[:, j].sum()), int(qb[:, j].sum())
        for l in range(3):
            w[10 + 3 * j + l] = int((qa[:, j] * qb[:, l]).sum())
    w[19], w[20] = int((qa * qa).sum()), int((qb * qb).sum())
    return w


def add_words(*chunks):
    return [sum(col) for col in zip(*chunks)]


def pair_inputs(seed, n, c=(0.25, -0.5, 1.0), h=2.0 ** -18):
    """n pairs around c within the lattice's reach, b a moved copy of a, with planted NaN, infinities, values just inside and just
    outside 2^20 steps (rint of +-(2^20 - 1), +-(2^20 - 0.5), +-2^20 and beyond) and a keep mask that drops about a seventh."""
    rng = np.random.default_rng(seed)
    c = np.asarray(c, F64)
    a = (c + rng.uniform(-1.5, 1.5, (n, 3))).astype(F32)
    b = (c + apply(sim(0.3, 1.2, 0.1), a.astype(F64) - c)).astype(F32)
    edge = [s * (2.0 ** 20 + d) * h for s in (1, -1) for d in (-1.0, -0.75, -0.5, -0.25, 0.0, 0.5, 4.0)]
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38] + edge, F64)
    k = rng.permutation(n)[:max(1, n // 6)]
    which, col, val = rng.integers(0, 2, k.size), rng.integers(0, 3, k.size), special[np.arange(k.size) % special.size]
    for i, wch, cl, v in zip(k, which, col, val):
        (a if wch else b)[i, cl] = F32(c[cl] + v) if np.isfinite(v) and abs(v) < 1e30 else F32(v)
    keep = (rng.random(n) > 1 / 7).astype(np.uint8)
    keep[k[:special.size:2]] = 1                                                    # every other planted value is surely seen
    return a, b, keep, tuple(c), h


# ------------------------------------------------------------------------------------------------ item 3
def plane_host(mesh, points, closest, face, distance, c, u, gate):
    """-> the 48 words as Python integers."""
    p, q = np.asarray(points, F32).reshape(-1, 3), np.asarray(closest, F32).reshape(-1, 3)
    face, d = np.asarray(face).astype(np.int64), np.asarray(distance, F32)
    kind, x = used_faces(mesh)
    nf = kind.shape[0]
    ok_face = (face >= 0) & (face < nf)
    safe = np.where(ok_face, face, 0)
    matched = ok_face & np.isfinite(d) & (kind[safe] == 0)
    with np.errstate(all="ignore"):
        gated = matched & (d > F32(gate))
        X = x[safe].astype(F64)
        n = _cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        nn = _dot(n, n)
        flat = matched & ~gated & (nn == 0)
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


def closest_host(mesh, points, max_distance=math.inf):
    """The brute force over every (point, face) pair -> distance, face, closest as lrf_mesh_closest writes them."""
    kind, x = used_faces(mesh)
    p = np.asarray(points, F32).reshape(-1, 3)
    use = np.nonzero(kind == 0)[0]
    d2 = np.full((p.shape[0], x.shape[0]), np.inf)
    with np.errstate(all="ignore"):
        for i0 in range(0, p.shape[0], 256):
            d2[i0:i0 + 256, use] = pair_host(p[i0:i0 + 256, None, :], x[None, use])[0]
    return closest_from_pairs({"points": p, "mesh": mesh}, kind, d2, max_distance)


# ------------------------------------------------------------------------------------------------ the fit by another route
def umeyama_host(a, b, scale=True):
    """The least-squares similarity of the pairs in plain fp64 numpy (no lattice, no integer moments)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    ma, mb = a.mean(0), b.mean(0)
    H = (b - mb).T @ (a - ma) / a.shape[0]
    U, D, Vt = np.linalg.svd(H)
    S = np.array([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / ((a - ma) ** 2).sum(1).mean()) if scale else 1.0
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, mb - s * R @ ma
    return T


def trajectory(V=30, seed=9):
    """V camera-to-world matrices on a loop of radius 0.4 with random orientations, fp32."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 1.7 * math.pi, V)
    centres = np.stack([0.4 * np.cos(a), 0.3 * np.sin(a), 0.1 * a / math.pi + 0.05 * rng.standard_normal(V)], 1)
    poses = np.zeros((V, 3, 4), F32)
    for i in range(V):
        poses[i, :, :3] = rot(rng.standard_normal(3), rng.uniform(0, 3))
        poses[i, :, 3] = centres[i]
    return poses


def move_poses(poses, T):
    s, R, t = parts(T)
    out = np.zeros_like(poses)
    out[:, :, :3] = R @ poses[:, :, :3].astype(F64)
    out[:, :, 3] = apply(T, poses[:, :, 3])
    return out.astype(F32)


# ------------------------------------------------------------------------------------------------ the plane iteration on the host
def box_frame(mesh, cloud, max_distance):
    """icp's frame: (centre of the mesh's box, u)."""
    kind, x = used_faces(mesh)
    pts = x[kind == 0].reshape(-1, 3).astype(F64)
    lo, hi = pts.min(0), pts.max(0)
    c = tuple(float(v) for v in (lo + hi) / 2)
    if math.isfinite(max_distance):
        pad = max_distance
    else:
        cl = np.asarray(cloud, F32).astype(F64)
        lo, hi = np.minimum(lo, cl.min(0)), np.maximum(hi, cl.max(0))
        pad = 0.5 * float((hi - lo).max())
    edge = float((hi - lo).max()) + 2 * pad
    return c, 2.0 ** math.ceil(math.log2(edge))


def icp_plane_host(cloud, mesh, scale, max_distance, iterations=10, tol=1e-7):
    """alignment.icp(metric="plane") with the restatements in place of the kernels: -> (T, history of steps)."""
    from localrf_amd import alignment
    T = np.eye(4)
    c, u = box_frame(mesh, cloud, max_distance)
    steps = []
    for _ in range(iterations):
        cur = transform_host(T[:3], cloud)
        near = closest_host(mesh, cur, max_distance)
        sol = alignment.solve_plane(plane_host(mesh, cur, near["closest"], near["face"], near["distance"], c, u, F32(max_distance)), scale)
        assert sol["omega"] is not None, sol
        T = alignment.compose(alignment.plane_update(sol, c, u), T)
        hit = near["face"] >= 0
        c = tuple(float(v) for v in near["closest"][hit].astype(F64).sum(0) / hit.sum())
        steps.append(max(float(np.linalg.norm(sol["omega"])), abs(sol["sigma"]), float(np.linalg.norm(sol["tau"]))))
        if steps[-1] < tol:
            break
    return T, steps
