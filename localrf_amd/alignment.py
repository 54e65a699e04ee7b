"""Registration on the GPU: the similarity that brings a point cloud, a trajectory or a mesh from its own gauge into another's
(csrc/lrf_align.inl through lrf_align_transform, lrf_align_pairs, lrf_align_plane and lrf_align_plane_cloud, over
mesh_distance.MeshIndex.closest and cloud.CloudIndex.closest).
A localrf scene lives in a gauge of its own -- poses are self-calibrated; origin, orientation and scale are arbitrary -- so
mesh_distance's figures against a reference scan, another pipeline's mesh or a second training run mean something only after
the two have been registered: a similarity from the trajectories (fit_pairs, trajectory_error), then ICP (icp, align_meshes).

  similarity / decompose / compose / inverse     4 x 4 float64 transforms on the host
  transform_points(points, T)                    T applied to device points
  transform_mesh(mesh, T)                        a mesh dict moved: vertices by T, normals by its rotation
  fit_pairs(a, b, keep, scale)                   the least-squares similarity of corresponding pairs, from exact integer moments
  trajectory_error(poses_est, poses_gt, scale)   absolute trajectory error after similarity alignment
  icp(points, mesh_or_index, ...)                point-to-plane (or point-to-point) ICP against a mesh, or against a cloud (a
                                                 cloud.CloudIndex; point-to-plane with the cloud's normals as target_normals)
  align_meshes(a, b, spacing, ...)               sample_surface + icp + transform_mesh

A transform is a numpy float64 [4,4] matrix T whose upper-left block is s R with det R = +1, applied as p' = s R p + t.  The
device sums are integers: the same T bytes on every run and for every order of the points.  Every function checks its arguments
on the host before its first launch.  CPU tensors raise NativeError: there is no torch fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from ._native import NativeError  # noqa: F401
from ._checks import (check_choice, check_flag, check_int, check_interval, check_max_distance, check_mesh, check_points, check_positive,
                      chunks, mesh_on_device, points_on_device)
from .cloud import CloudIndex
from .mesh_distance import as_index, check_target, sample_surface

PAIRS_PER_CALL = 1 << 20                       # lrf_align_pairs and lrf_align_plane: no word can overflow below this
PAIR_RANGE = 1 << 20                           # integer coordinates of fit_pairs stay below this in magnitude
PLANE_SCALE = 1 << 36                          # the fixed point of lrf_align_plane's sums
ROTATION_TOL = 1e-9                            # decompose: max |R^T R - I| of the block divided by its scale
RANK_TOL = 1e-10                               # fit_pairs: second singular value of the covariance against the first
CONDITION_MAX = 1e12                           # icp: condition number of the normal equations
MIN_MATCHES = 7


# ------------------------------------------------------------------------------------------------ host helpers
def _matrix(T, name="T"):
    try:
        M = np.array(T.detach().cpu().numpy() if torch.is_tensor(T) else T, dtype=np.float64)
    except (TypeError, ValueError):
        M = np.zeros(0)
    if M.shape != (4, 4) or not np.isfinite(M).all() or not np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError(f"{name} must be a finite 4 x 4 matrix with the last row (0, 0, 0, 1), got {T!r}")
    return M


def _build(s, R, t):
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = t
    return T


def decompose(T):
    """T -> (scale, rotation [3,3], translation [3]).  ValueError unless the upper-left block B is a positive multiple of a
    proper rotation: det B > 0 and, with s = det(B)^(1/3), max |(B / s)^T (B / s) - I| <= 1e-9 (ROTATION_TOL)."""
    M = _matrix(T)
    B = M[:3, :3]
    d = float(np.linalg.det(B))
    s = d ** (1.0 / 3.0) if d > 0 else math.nan
    if not s > 0 or not np.abs((B / s).T @ (B / s) - np.eye(3)).max() <= ROTATION_TOL:
        raise ValueError(f"T's upper-left block must be a positive multiple of a proper rotation (within {ROTATION_TOL}), got {B!r}")
    return s, B / s, M[:3, 3].copy()


def similarity(scale, rotation, translation):
    """The transform p' = scale rotation p + translation.  rotation: a proper rotation [3,3] (decompose's tolerance)."""
    s = check_positive("scale", scale)
    try:
        R = np.array(rotation, dtype=np.float64)
        t = np.array(translation, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        R, t = np.zeros(0), np.zeros(0)
    if R.shape != (3, 3) or not np.isfinite(R).all() or not np.linalg.det(R) > 0 or not np.abs(R.T @ R - np.eye(3)).max() <= ROTATION_TOL:
        raise ValueError(f"rotation must be a proper 3 x 3 rotation (within {ROTATION_TOL}), got {rotation!r}")
    if t.shape != (3,) or not np.isfinite(t).all():
        raise ValueError(f"translation must hold 3 finite values, got {translation!r}")
    return _build(s, R, t)


def compose(T2, T1):
    """The transform that applies T1, then T2."""
    M = _matrix(T2, "T2") @ _matrix(T1, "T1")
    M[3] = (0.0, 0.0, 0.0, 1.0)
    return M


def inverse(T):
    """The inverse similarity: (1 / s, R^T, -R^T t / s)."""
    s, R, t = decompose(T)
    return _build(1.0 / s, R.T, -(R.T @ t) / s)


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def _power_of_two_at_least(x):
    """The smallest power of two >= x (x > 0 and finite; 1.0 otherwise)."""
    if not (x > 0 and math.isfinite(x)):
        return 1.0
    m, e = math.frexp(x)                                            # x = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def pair_frame(lo, hi):
    """The frame of lrf_align_pairs for the box (lo, hi): c its centre, h the smallest power of two with half_extent / h <=
    2^20 - 2 (so that the rounded coordinates stay below 2^20 in magnitude)."""
    c = tuple((float(l) + float(h)) / 2.0 for l, h in zip(lo, hi))
    half = max((float(h) - float(l)) / 2.0 for l, h in zip(lo, hi))
    return c, _power_of_two_at_least(half / (PAIR_RANGE - 2))


def solve_pairs(words, c, h, scale=True):
    """The closed form of fit_pairs from lrf_align_pairs' words (24 integers; chunks already added) in the frame (c, h).  The
    centred moments are formed exactly in Python integers and only then divided."""
    w = [int(x) for x in words]
    n = w[0]
    info = {"count": n, "out_of_range": w[1], "masked": w[2], "nonfinite": w[3]}
    if n < 3:
        raise ValueError(f"a similarity needs at least 3 kept pairs, got {n} ({info})")
    Sa, Sb, M = w[4:7], w[7:10], [w[10 + 3 * i:13 + 3 * i] for i in range(3)]
    n2 = n * n
    cov = np.array([[(n * M[i][j] - Sa[i] * Sb[j]) / n2 for j in range(3)] for i in range(3)])      # cov(a_i, b_j), units h^2
    va, vb = (n * w[19] - sum(x * x for x in Sa)) / n2, (n * w[20] - sum(x * x for x in Sb)) / n2
    U, D, Vt = np.linalg.svd(cov.T)                                 # sum (b - mean_b)(a - mean_a)^T / n
    if not va > 0 or not D[1] > RANK_TOL * D[0]:
        raise ValueError(f"the pairs' covariance has rank below 2 (singular values {D.tolist()}): no rotation is determined")
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0])
    R = U @ np.diag(S) @ Vt
    tr = float((D * S).sum())
    s = tr / va if scale else 1.0
    mean_a = np.array([c[k] + h * (Sa[k] / n) for k in range(3)])
    mean_b = np.array([c[k] + h * (Sb[k] / n) for k in range(3)])
    e2 = vb + s * s * va - 2.0 * s * tr
    return dict(info, T=_build(s, R, mean_b - s * (R @ mean_a)), scale=s, rms=h * math.sqrt(max(e2, 0.0)))


def pairs_rms(words, h):
    """The root mean square distance of the summed pairs as they are, from the same words: exact integers, one division."""
    w = [int(x) for x in words]
    return h * math.sqrt(max(w[19] - 2 * (w[10] + w[14] + w[18]) + w[20], 0) / w[0]) if w[0] else math.nan


def solve_plane(words, scale=True):
    """One point-to-plane step from lrf_align_plane's words (48 integers; chunks already added) -> omega [3], tau [3] (in
    units of u), sigma, rms (in units of u), count and cond; omega None when fewer than 7 points matched or the system's
    condition number exceeds 1e12 (CONDITION_MAX).  scale=False solves the 6 x 6 system without sigma's row and column."""
    w = [int(x) for x in words]
    n = w[0]
    out = {"omega": None, "tau": None, "sigma": 0.0, "count": n, "cond": math.inf, "rms": math.sqrt(w[6] / PLANE_SCALE / n) if n else math.nan,
           "unmatched": w[1], "gated": w[2], "degenerate": w[3], "out_of_range": w[4]}
    if n < MIN_MATCHES:
        return out
    A, at = np.zeros((7, 7)), 14
    for k in range(7):
        for l in range(k, 7):
            A[k, l] = A[l, k] = w[at] / PLANE_SCALE
            at += 1
    g = np.array([w[7 + k] / PLANE_SCALE for k in range(7)])
    k = 7 if scale else 6
    A, g = A[:k, :k], g[:k]
    try:
        with np.errstate(all="ignore"):
            cond = float(np.linalg.cond(A))
            x = np.linalg.solve(A, -g) if cond <= CONDITION_MAX else None
    except np.linalg.LinAlgError:
        cond, x = math.inf, None
    out["cond"] = cond if math.isfinite(cond) else math.inf
    if x is None or not np.isfinite(x).all():
        return out
    out.update(omega=x[:3], tau=x[3:6], sigma=float(x[6]) if scale else 0.0)
    return out


def plane_update(sol, c, u):
    """solve_plane's step as a transform: p' = c + (1 + sigma) exp(omega) (p - c) + u tau."""
    c = np.asarray(c, np.float64)
    s, R = 1.0 + sol["sigma"], _rodrigues(sol["omega"])
    return _build(s, R, c - s * (R @ c) + u * sol["tau"])


# ------------------------------------------------------------------------------------------------ device halves
def _transform_into(pts, T, out):
    t = (C.c_double * 12)(*T[:3].reshape(-1).tolist())
    for i0, m in chunks(pts.shape[0]):
        N.launch("lrf_align_transform", pts.device, t, pts[i0:].data_ptr(), m, out[i0:].data_ptr(), guard=True)
    return out


def transform_points(points, T):
    """points [N,3] fp32 on the device -> T applied, a new [N,3] fp32 tensor: each coordinate ((T0 x + T1 y) + T2 z) + T3 in
    fp64, rounded once to fp32 (csrc/lrf_align.inl item 1).  No read-back."""
    check_points(points)
    M = _matrix(T)
    pts = points_on_device(points, "points", "the alignment")
    return _transform_into(pts, M, torch.empty_like(pts))


def transform_mesh(mesh, T):
    """The mesh dict of mesh.py moved by T: a new dict with new vertices; normals, where the mesh has them, rotated by T's
    rotation alone (neither scaled nor shifted); faces, colours and every other entry are the input's own tensors."""
    v, f, _, Nv, Nf = check_mesh(mesh)
    M = _matrix(T)
    _, R, _ = decompose(M)
    normals = mesh.get("normals")
    if normals is not None:
        check_points(normals)
        if normals.shape[0] != Nv:
            raise ValueError(f"normals must be {(Nv, 3)} float32, got {tuple(normals.shape)}")
    v, _, _, dev = mesh_on_device(v, f, None, "the alignment")
    out = dict(mesh)
    out["vertices"] = _transform_into(v, M, torch.empty_like(v))
    if normals is not None:
        nrm = points_on_device(normals, "normals", "the alignment")
        out["normals"] = _transform_into(nrm, _build(1.0, R, np.zeros(3)), torch.empty_like(nrm))
    return out


def _finite_box(*clouds):
    """The box of the finite coordinates of the clouds ([N,3] each, N > 0): (lo, hi) as Python floats, +-inf without one.  One
    read-back."""
    rows = []
    for x in clouds:
        fin = torch.isfinite(x)
        rows += [torch.where(fin, x, math.inf).amin(0), -torch.where(fin, x, -math.inf).amax(0)]
    lo_hi = torch.stack(rows).reshape(-1, 2, 3).amin(0).cpu().tolist()
    return tuple(lo_hi[0]), tuple(-h for h in lo_hi[1])


def _chunk_words(n, width, dev, launch):
    """One launch(i0, m, row) per PAIRS_PER_CALL of n > 0 items, which fills row, the data pointer of its `width` words (the
    entry points zero them themselves) -> int64 [chunks, width] on the device; no read-back."""
    spans = list(chunks(n, PAIRS_PER_CALL))
    words = torch.empty(len(spans), width, dtype=torch.int64, device=dev)
    for j, (i0, m) in enumerate(spans):
        launch(i0, m, words[j].data_ptr())
    return words


def _pair_words(c, h, a, b, keep):
    """Checked, contiguous device arguments -> int64 [chunks, 24] on the device; no read-back."""
    fr = N.LrfAlignFrame()
    fr.h = h
    for k in range(3):
        fr.c[k] = c[k]

    def launch(i0, m, row):
        N.launch("lrf_align_pairs", a.device, C.byref(fr), a[i0:].data_ptr(), b[i0:].data_ptr(), None if keep is None else keep[i0:].data_ptr(),
                 m, row, guard=True)
    return _chunk_words(a.shape[0], 24, a.device, launch)


def _plane_words(index, pts, near, c, u, gate, normals=None):
    """Checked, contiguous device arguments -> int64 [chunks, 48] on the device; no read-back.  Against a MeshIndex the plane of a
    point is its closest face's (lrf_align_plane); against a CloudIndex, with normals = its target_normals, the one through its
    closest cloud point with that point's normal (lrf_align_plane_cloud)."""
    if normals is None:
        p, symbol, key = N.LrfAlignPlane(), "lrf_align_plane", "face"
        p.vertices, p.faces, (p.Nv, p.Nf) = index.vertices.data_ptr(), index.faces.data_ptr(), index.counts
    else:
        p, symbol, key = N.LrfAlignPlaneCloud(), "lrf_align_plane_cloud", "index"
        p.normals, p.M = normals.data_ptr(), index.counts[0]
    p.u, p.gate = u, gate
    for k in range(3):
        p.c[k] = c[k]

    def launch(i0, m, row):
        p.N = m
        p.points, p.closest, p.distance = pts[i0:].data_ptr(), near["closest"][i0:].data_ptr(), near["distance"][i0:].data_ptr()
        setattr(p, key, near[key][i0:].data_ptr())
        N.launch(symbol, pts.device, C.byref(p), row, guard=True)
    return _chunk_words(pts.shape[0], 48, pts.device, launch)


def _add_words(host):
    """int64 [chunks, W] read back -> W Python integers: exact for any number of chunks."""
    return [sum(col) for col in zip(*host.tolist())]


def _check_keep(keep, n):
    if keep is None:
        return
    if not torch.is_tensor(keep):
        raise TypeError("keep must be a torch tensor or None")
    if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (n,):
        raise ValueError(f"keep must be {(n,)} bool or uint8, got {keep.dtype} {tuple(keep.shape)}")


def fit_pairs(a, b, keep=None, scale=True):
    """The similarity that maps a onto b in the least-squares sense: a, b [N,3] fp32 on one device, row i of a corresponding to
    row i of b; keep [N] bool or uint8 (None: every pair).  The coordinates are rounded onto a lattice of 2^21 steps over the box
    of the finite coordinates of both sets (pair_frame), their first and second moments are summed as integers on the device
    (csrc/lrf_align.inl item 2; chunks of 2^20 pairs added as Python integers: exact for any N), centred exactly, and the
    rotation is R = U diag(1, 1, det(U V^T)) V^T of the 3 x 3 covariance's SVD, the scale tr(D S) / var_a (1 with scale=False) and
    t = mean_b - s R mean_a.  Returns T, scale, rms (the residual after the fit, from the moments, in world units), count, and
    the pairs left out: out_of_range, masked, nonfinite.  ValueError for fewer than 3 kept pairs or a covariance of rank below
    2 (second singular value <= 1e-10 of the first).  Two read-backs: the box, then the words."""
    n = check_points(a)
    if check_points(b) != n:
        raise ValueError(f"a and b must hold the same number of points, got {n} and {b.shape[0]}")
    _check_keep(keep, n)
    scale = check_flag("scale", scale)
    a, b = points_on_device(a, "a", "the alignment"), points_on_device(b, "b", "the alignment")
    keep = None if keep is None else points_on_device(keep, "keep", "the alignment").to(torch.uint8)
    if b.device != a.device or (keep is not None and keep.device != a.device):
        raise ValueError("a, b and keep must live on the same device")
    if n < 3:
        raise ValueError(f"a similarity needs at least 3 kept pairs, got {n}")
    lo, hi = _finite_box(a, b)                                      # read-back one
    c, h = pair_frame(lo, hi) if all(math.isfinite(x) for x in lo + hi) else ((0.0, 0.0, 0.0), 1.0)
    return solve_pairs(_add_words(_pair_words(c, h, a, b, keep).cpu()), c, h, scale)      # read-back two


def _check_pose_stack(name, poses):
    if not torch.is_tensor(poses):
        raise TypeError(f"{name} must be a torch tensor")
    if not poses.is_floating_point() or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"{name} must be [V, 3, 4] floating point camera-to-world matrices, got {poses.dtype} {tuple(poses.shape)}")
    return int(poses.shape[0])


def trajectory_error(poses_est, poses_gt, scale=True):
    """The absolute trajectory error of poses_est against poses_gt ([V,3,4] camera-to-world matrices on one device) after the
    similarity (scale=False: the rigid motion) that fit_pairs finds between the camera centres.  Returns T (est -> gt),
    ate_rmse, ate_mean, ate_max over the V centres after alignment (fp64 torch on the device) and count, the pairs that entered
    the fit.  Three read-backs: fit_pairs' two, then the three figures."""
    V = _check_pose_stack("poses_est", poses_est)
    if _check_pose_stack("poses_gt", poses_gt) != V:
        raise ValueError(f"{V} estimated poses for {poses_gt.shape[0]} ground-truth ones")
    scale = check_flag("scale", scale)
    N.require_gpu(poses_est, "poses_est", "the alignment")
    N.require_gpu(poses_gt, "poses_gt", "the alignment")
    ce = poses_est.detach()[:, :, 3].to(torch.float32).contiguous()
    cg = poses_gt.detach()[:, :, 3].to(torch.float32).contiguous()
    fit = fit_pairs(ce, cg, None, scale)
    T = torch.from_numpy(fit["T"]).to(ce.device)
    d = (ce.double() @ T[:3, :3].T + T[:3, 3] - cg.double()).norm(dim=1)
    rmse, mean, top = torch.stack([d.square().mean().sqrt(), d.mean(), d.max()]).cpu().tolist()
    return {"T": fit["T"], "ate_rmse": rmse, "ate_mean": mean, "ate_max": top, "count": fit["count"]}


def _check_icp_options(init=None, scale=True, metric="plane", iterations=20, max_distance=math.inf, tol=1e-7):
    if init is not None:
        decompose(init)
    check_flag("scale", scale)
    check_choice("metric", metric, ("plane", "point"))
    check_int("iterations", iterations, 1, 10000)
    check_max_distance(max_distance)
    check_interval("tol", tol, 0.0, 1.0, "lie in [0, 1]")


def _plane_iteration(index, cur, near, c, u, gate, scale, normals=None):
    """One accumulation and solve of metric="plane" -> (rms, count, the points left out, the step's transform or None, its size,
    the next frame centre).  normals: the target_normals of a CloudIndex.  One read-back: the words and the fp64 sum of the
    closest points in one tensor."""
    words = _plane_words(index, cur, near, c, u, gate, normals)
    q = near["closest"].double()
    qsum = torch.where(torch.isfinite(q), q, 0.0).sum(0)
    host = torch.cat([words.reshape(-1), qsum.view(torch.int64)]).cpu()                         # the read-back
    sol = solve_plane(_add_words(host[:-3].reshape(-1, 48)), scale)
    left = {k: sol[k] for k in ("unmatched", "gated", "degenerate", "out_of_range", "cond")}
    matched = cur.shape[0] - sol["unmatched"]
    nxt = tuple(float(x) / matched for x in host[-3:].view(torch.float64).tolist()) if matched else c
    if sol["omega"] is None or not 1.0 + sol["sigma"] > 0:
        return sol["rms"] * u, sol["count"], left, None, math.nan, nxt
    step = max(float(np.linalg.norm(sol["omega"])), abs(sol["sigma"]), float(np.linalg.norm(sol["tau"])))
    return sol["rms"] * u, sol["count"], left, plane_update(sol, c, u), step, nxt


def _point_iteration(cur, near, c0, h, u, max_distance, scale):
    """One accumulation and solve of metric="point" -> (rms, count, the pairs left out, the step's transform or None, its size:
    the largest of the rotation's sine, |s - 1| and the shift of the frame's centre in units of u).  One read-back."""
    keep = (near["distance"] <= max_distance).to(torch.uint8)
    w = _add_words(_pair_words(c0, h, cur, near["closest"], keep).cpu())                        # the read-back
    rms, left = pairs_rms(w, h), {"out_of_range": w[1], "masked": w[2], "nonfinite": w[3]}
    try:
        step_T = solve_pairs(w, c0, h, scale)["T"] if w[0] >= MIN_MATCHES else None
    except ValueError:                                              # rank below 2
        step_T = None
    if step_T is None:
        return rms, w[0], left, None, math.nan
    s_d, R_d, _ = decompose(step_T)
    mid = np.array(c0)
    step = max(float(np.linalg.norm([R_d[2, 1] - R_d[1, 2], R_d[0, 2] - R_d[2, 0], R_d[1, 0] - R_d[0, 1]])) / 2.0, abs(s_d - 1.0),
               float(np.linalg.norm(step_T[:3, :3] @ mid + step_T[:3, 3] - mid)) / u)
    return rms, w[0], left, step_T, step


def _check_target_normals(target_normals, target, metric):
    """target_normals (not None) against icp's target and metric: host checks only."""
    if not isinstance(target, CloudIndex):
        raise ValueError("target_normals go with a CloudIndex as the target: a mesh's planes are its faces")
    if metric != "plane":
        raise ValueError('target_normals are the planes of metric="plane"; metric="point" takes none')
    if not torch.is_tensor(target_normals):
        raise ValueError("target_normals must be a torch tensor or None")
    m = target.counts[0]
    if target_normals.dtype is not torch.float32 or tuple(target_normals.shape) != (m, 3):
        raise ValueError(f"target_normals must be {(m, 3)} float32, one row per point of the CloudIndex, got {target_normals.dtype} "
                         f"{tuple(target_normals.shape)}")
    if target_normals.device != target.device:
        raise ValueError(f"target_normals live on {target_normals.device}, the index on {target.device}")


def icp(points, mesh_or_index, init=None, scale=True, metric="plane", iterations=20, max_distance=math.inf, tol=1e-7, target_normals=None):
    """Iterative closest point of a cloud ([N,3] fp32 on the device) against a mesh (or a MeshIndex built from it, which is not
    built again): the similarity T (scale=False: the rigid motion), starting from init, that brings the cloud onto the surface.

    ICP refines; it does not search.  It needs a rough initial alignment -- closer than the features it should lock onto are
    wide -- and fit_pairs on the two trajectories (trajectory_error's T) gives one.  Correspondences are one-sided, from the
    cloud to the mesh: with a free scale a cloud that covers only part of the target can shrink onto it, so scale=False is the
    safe choice for partial overlap.

    Each iteration transforms the ORIGINAL points by the composed T (nothing drifts), queries MeshIndex.closest(closest=True,
    max_distance), accumulates once per 2^20 points, reads back once, solves on the host and composes.
    metric="plane" (csrc/lrf_align.inl item 3): the 7 x 7 normal equations of the linearised point-to-plane residual in the
    frame (c, u) -- c the mean of the previous iteration's matched closest points (first: the centre of the index's box), u the
    smallest power of two that covers the index's box inflated by max_distance, or, when that is infinite, the box of the
    index and of the initially transformed cloud inflated by half its longest edge -- solved by np.linalg.solve (6 x 6 without
    the scale), applied as p' = c + (1 + sigma) exp(omega) (p - c) + u tau.  metric="point": lrf_align_pairs over (point,
    closest point) with keep = distance <= max_distance, and fit_pairs' closed form; it slides slowly along smooth surfaces,
    which is why "plane" is the default.
    Stops with converged=True, reason="tolerance" when the step's largest of |omega|, |sigma| and |tau| (in units of u) is
    below tol; with converged=False, reason="degenerate" when fewer than 7 points match or the system's condition number
    exceeds 1e12 (a plane as the target, a direction the cloud can slide along); else reason="iterations".
    Returns T, iterations (steps applied), converged, reason, rms and count (of the last accumulation: the point-to-plane or
    point-to-point residual before its step, in world units) and history: per iteration rms, count, step and the points left
    out.  One read-back before the loop when max_distance is infinite, one per iteration.

    The target may also be a cloud.CloudIndex -- a laser scan, another run's scene_point_cloud: the loop is the same and the
    closest point is the nearest point of the cloud.  A cloud has no planes of its own: metric="plane" with a CloudIndex needs
    target_normals ([M,3] fp32 on the index's device, one row per point of the cloud; csrc/lrf_align.inl item 4), the plane of a
    point then being the one through its nearest cloud point with that point's normal; a point whose nearest cloud point has the
    normal (0, 0, 0) or one that is not finite is left out and counted as degenerate.  Without them it raises ValueError, and
    metric="point" needs none -- but when the points are not the scan's own sample, the nearest sample lies up to half a spacing
    off along the surface and point-to-point does not get below that.  The recipe for a scan:

        scan = cloud.CloudIndex(scan_points)
        normals = cloud.estimate_normals(scan, 3 * cloud.nearest_spacing(scan)["median"])["normals"]
        T = alignment.icp(points, scan, target_normals=normals, scale=False)["T"]

    target_normals with a mesh as the target, with metric="point", or of another shape, dtype or device raise ValueError."""
    to_cloud = isinstance(mesh_or_index, CloudIndex)
    if not to_cloud:
        check_target(mesh_or_index)                                 # the target's type, a mesh dict's tensors
    check_points(points)
    _check_icp_options(init, scale, metric, iterations, max_distance, tol)
    if target_normals is not None:
        _check_target_normals(target_normals, mesh_or_index, metric)
    elif to_cloud and metric == "plane":
        raise ValueError('a cloud has no planes: metric="plane" needs a mesh or a MeshIndex as the target; '
                         'pass metric="point" to align against a CloudIndex')
    index = mesh_or_index if to_cloud else as_index(mesh_or_index, 1 << 30)     # a mesh dict: the device, then the index build
    T = np.eye(4) if init is None else _matrix(init)
    max_distance, tol = check_max_distance(max_distance), float(tol)
    pts = points_on_device(points, "points", "the alignment", index.device, f"points live on {points.device}, the index on {index.device}")
    out = {"T": T, "iterations": 0, "converged": False, "reason": "degenerate", "rms": math.nan, "count": 0, "history": []}
    if pts.shape[0] < MIN_MATCHES or index.info["box"] is None:
        return out
    normals = None if target_normals is None else target_normals.detach().contiguous()
    cur = torch.empty_like(pts)
    lo, hi = index.info["box"]
    if math.isfinite(max_distance):
        pad = max_distance
    else:
        blo, bhi = _finite_box(_transform_into(pts, T, cur))        # the read-back before the loop
        if all(math.isfinite(x) for x in blo + bhi):
            lo, hi = tuple(min(x, y) for x, y in zip(lo, blo)), tuple(max(x, y) for x, y in zip(hi, bhi))
        pad = 0.5 * max(h - l for l, h in zip(lo, hi))
    lo, hi = tuple(l - pad for l in lo), tuple(h + pad for h in hi)
    u = _power_of_two_at_least(max(h - l for l, h in zip(lo, hi)))
    c0, h = pair_frame(lo, hi)
    c = tuple((l + r) / 2.0 for l, r in zip(*index.info["box"]))
    gate = float(np.float32(max_distance))
    for _ in range(iterations):
        _transform_into(pts, T, cur)
        near = index.closest(cur, max_distance, closest=True)
        if metric == "plane":
            rms, count, left, step_T, step, c = _plane_iteration(index, cur, near, c, u, gate, scale, normals)
        else:
            rms, count, left, step_T, step = _point_iteration(cur, near, c0, h, u, max_distance, scale)
        out.update(rms=rms, count=count)
        out["history"].append(dict(left, rms=rms, count=count, step=step))
        if step_T is None:
            return out
        T = compose(step_T, T)
        out.update(T=T, iterations=out["iterations"] + 1)
        if step < tol:
            out.update(converged=True, reason="tolerance")
            return out
    out["reason"] = "iterations"
    return out


def align_meshes(a, b, spacing, **icp_options):
    """Mesh a registered onto mesh b (a mesh dict or a MeshIndex): sample_surface(a, spacing), icp of the samples against b
    with icp_options (init, scale, metric, iterations, max_distance, tol), and a moved by the result.  Returns icp's dict plus
    "mesh": transform_mesh(a, T).  The recipe for scoring a reconstruction in another gauge against a reference:

        T0 = alignment.trajectory_error(poses_est, poses_ref)["T"]
        aligned = alignment.align_meshes(mesh, reference, spacing, init=T0, scale=False)["mesh"]
        figures = mesh_distance.mesh_distance(aligned, reference, spacing, thresholds)"""
    check_mesh(a)
    check_target(b, "b")
    check_positive("spacing", spacing)
    unknown = set(icp_options) - {"init", "scale", "metric", "iterations", "max_distance", "tol"}
    if unknown:
        raise TypeError(f"align_meshes got unexpected icp options {sorted(unknown)}")
    _check_icp_options(**icp_options)
    samples = sample_surface(a, spacing)
    out = icp(samples["points"], b, **icp_options)
    out["mesh"] = transform_mesh(a, out["T"])
    return out
