"""Shared pieces of the mesh-rasteriser tests: the numpy restatement of csrc/lrf_mesh_raster.inl (same operation order: fp32
camera points and shears, fp64 edge functions rounded one by one, the symbolic tie-break, the 64-bit key minimum), its pixel
box, an independent fp64 Moeller-Trumbore ray caster, the restatement of the depth agreement, and the cases."""
import functools
import math

import numpy as np

from mesh_clean_cases import fan
from points_cases import pixel_dirs, rigid_poses

F32 = np.float32
SMALL_MAX = 256                                # RS_SMALL_MAX of csrc/lrf_mesh_raster.inl
CULL = {None: 0, "back": 1, "front": 2}
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
AG_SCALE, AG_CLAMP = 1 << 24, 16.0


# ------------------------------------------------------------------------------------------------ the restatement
def to_camera(p, M):
    """World points p [...,3] fp32 into the camera M [3,4]: d = p - t, q = (c0 dx + c1 dy) + c2 dz per column (to_camera of
    csrc/lrf_points.inl) -> [...,3] fp32."""
    p, M = np.asarray(p, F32), np.asarray(M, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[..., 0] - M[0, 3], p[..., 1] - M[1, 3], p[..., 2] - M[2, 3]
        q = [(M[0, c] * dx + M[1, c] * dy) + M[2, c] * dz for c in range(3)]
    return np.stack(q, -1).astype(F32)


def face_kinds(mesh):
    """Per face 0: valid, 1: an index outside [0, Nv), 2: two equal indices, 3: a coordinate that is not finite."""
    v, f = np.asarray(mesh["vertices"], F32), np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    nv = v.shape[0]
    kind = np.zeros(f.shape[0], np.int64)
    bad = ((f < 0) | (f >= nv)).any(1)
    kind[bad] = 1
    kind[~bad & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))] = 2
    ok = kind == 0
    kind[np.nonzero(ok)[0][~np.isfinite(v[f[ok]]).all((1, 2))]] = 3
    return kind


def _sign(U, axb, ayb, axc, ayc):
    tie = np.where(ayb > ayc, 1, np.where(ayb < ayc, -1, np.where(axc > axb, 1, np.where(axc < axb, -1, 0))))
    return np.where(U > 0, 1, np.where(U < 0, -1, tie)).astype(np.int8)


def cover_host(q, x, y):
    """Camera-space corners q [F,3,3] fp32 against the rays (x [W], y [H], -1) -> (covered [F,H,W] bool, s [F,H,W] int8, U
    three [F,H,W] fp64)."""
    with np.errstate(all="ignore"):
        ax = (q[:, :, 0, None] + q[:, :, 2, None] * x[None, None, :]).astype(F32)            # [F,3,W]
        ay = (q[:, :, 1, None] + q[:, :, 2, None] * y[None, None, :]).astype(F32)            # [F,3,H]
        AX = [ax[:, k, None, :].astype(np.float64) for k in range(3)]
        AY = [ay[:, k, :, None].astype(np.float64) for k in range(3)]
        U = [AX[1] * AY[2] - AY[1] * AX[2], AX[2] * AY[0] - AY[2] * AX[0], AX[0] * AY[1] - AY[0] * AX[1]]
        fx = [ax[:, k, None, :] for k in range(3)]
        fy = [ay[:, k, :, None] for k in range(3)]
        s0 = _sign(U[0], fx[1], fy[1], fx[2], fy[2])
        s1 = _sign(U[1], fx[2], fy[2], fx[0], fy[0])
        s2 = _sign(U[2], fx[0], fy[0], fx[1], fy[1])
    return (s0 != 0) & (s0 == s1) & (s0 == s2), s0, U


def depth_host(q, U):
    with np.errstate(all="ignore"):
        n = [(-q[:, k, 2]).astype(np.float64)[:, None, None] for k in range(3)]
        t = ((U[0] * n[0] + U[1] * n[1]) + U[2] * n[2]) / ((U[0] + U[1]) + U[2])
        return t.astype(F32)


def _lo(a, n):
    with np.errstate(all="ignore"):
        a = np.floor(F32(a)) - F32(1)
    return (int(a) if a < n else n) if a > 0 else 0


def _hi(b, n):
    with np.errstate(all="ignore"):
        b = np.ceil(F32(b)) + F32(1)
    return (int(b) if b >= 0 else -1) if b < n - 1 else n - 1


def box_host(q, f, cx, cy, W, H):
    """rs_box: camera-space corners q [3,3] -> (i0, i1, j0, j1) or None when the face is skipped or the box is empty."""
    f, cx, cy = F32(f), F32(cx), F32(cy)
    nz = -np.asarray(q, F32)[:, 2]
    if (nz <= 0).all():
        return None
    box = [0, W - 1, 0, H - 1]
    if (nz > 0).all():
        with np.errstate(all="ignore"):
            u = q[:, 0] / nz * f + cx - F32(0.5)
            w = -q[:, 1] / nz * f + cy - F32(0.5)
        if not (np.isnan(u).any() or np.isnan(w).any()):
            box = [_lo(u.min(), W), _hi(u.max(), W), _lo(w.min(), H), _hi(w.max(), H)]
    return tuple(box) if box[0] <= box[1] and box[2] <= box[3] else None


def rasterize_host(mesh, c2w, W, H, f, cx, cy, depth_range=(0.0, np.inf), cull=None, chunk=128):
    """lrf_mesh_rasterize on the host, every (pixel, face) pair, no boxes -> dict(depth, face, rgb8 or None, weights, crossings,
    info)."""
    v, faces = np.asarray(mesh["vertices"], F32), np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    c2w = np.asarray(c2w, F32)
    V = c2w.shape[0]
    kind = face_kinds(mesh)
    valid = np.nonzero(kind == 0)[0]
    dirs = pixel_dirs(H, W, f, cx, cy)
    x, y = np.ascontiguousarray(dirs[0, :, 0]), np.ascontiguousarray(dirs[:, 0, 1])
    lo, hi = F32(depth_range[0]), F32(depth_range[1])
    keys = np.full((V, H, W), EMPTY, np.uint64)
    crossings = np.zeros((V, H, W), np.int32)
    for fr in range(V):
        for c0 in range(0, valid.size, chunk):
            ids = valid[c0:c0 + chunk]
            q = to_camera(v[faces[ids]], c2w[fr])                                             # [F,3,3]
            ids = ids[~(q[:, :, 2] >= 0).all(1)]                                              # all nz <= 0: skipped
            if not ids.size:
                continue
            q = to_camera(v[faces[ids]], c2w[fr])
            cov, s, U = cover_host(q, x, y)
            t = depth_host(q, U)
            with np.errstate(invalid="ignore"):
                keep = cov & np.isfinite(t) & (t > 0) & (t >= lo) & (t <= hi)
            crossings[fr] += keep.sum(0).astype(np.int32)
            if CULL[cull] == 1:
                keep &= s > 0
            elif CULL[cull] == 2:
                keep &= s < 0
            key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)[:, None, None]
            keys[fr] = np.minimum(keys[fr], np.where(keep, key, EMPTY).min(0))
    hit = keys != EMPTY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    weights = np.zeros((V, H, W, 3), F32)
    rgb8 = None if mesh.get("rgb8") is None else np.zeros((V, H, W, 3), np.uint8)
    for fr in range(V):
        jj, ii = np.nonzero(hit[fr])
        if not jj.size:
            continue
        fid = face[fr, jj, ii].astype(np.int64)
        q = to_camera(v[faces[fid]], c2w[fr])                                                 # [P,3,3]
        with np.errstate(all="ignore"):
            ax = (q[:, :, 0] + q[:, :, 2] * x[ii][:, None]).astype(F32).astype(np.float64)
            ay = (q[:, :, 1] + q[:, :, 2] * y[jj][:, None]).astype(F32).astype(np.float64)
            U = [ax[:, 1] * ay[:, 2] - ay[:, 1] * ax[:, 2], ax[:, 2] * ay[:, 0] - ay[:, 2] * ax[:, 0],
                 ax[:, 0] * ay[:, 1] - ay[:, 0] * ax[:, 1]]
            D = (U[0] + U[1]) + U[2]
            w = [U[k] / D for k in range(3)]
        weights[fr, jj, ii] = np.stack(w, -1).astype(F32)
        if rgb8 is not None:
            col = np.asarray(mesh["rgb8"], np.uint8)[faces[fid]].astype(np.float64)           # [P,3 corners,3 channels]
            m = np.rint((w[0][:, None] * col[:, 0] + w[1][:, None] * col[:, 1]) + w[2][:, None] * col[:, 2])
            rgb8[fr, jj, ii] = np.clip(m, 0, 255).astype(np.uint8)
    info = {"bad_index_faces": int((kind == 1).sum()), "degenerate_faces": int((kind == 2).sum()),
            "nonfinite_faces": int((kind == 3).sum())}
    return {"depth": depth, "face": face, "rgb8": rgb8, "weights": weights, "crossings": crossings, "info": info}


def moller_trumbore(mesh, M, W, H, f, cx, cy):
    """An independent fp64 ray caster over every (pixel, face) pair of one camera M [3,4]: rays from the camera position along
    R (x, y, -1).  -> (t [F,H,W] the ray parameter of the face's plane, b [F,H,W,3] the barycentric weights there)."""
    v = np.asarray(mesh["vertices"], np.float64)
    fc = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    M = np.asarray(M, np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(col + 0.5 - float(cx)) / float(f), -(row + 0.5 - float(cy)) / float(f), -np.ones_like(col)], -1) @ M[:, :3].T
    o = M[:, 3]
    v0, e1, e2 = v[fc[:, 0]], v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]]
    with np.errstate(all="ignore"):
        pv = np.cross(d[None], e2[:, None, None])                                             # [F,H,W,3]
        det = (e1[:, None, None] * pv).sum(-1)
        tv = o - v0                                                                           # [F,3]
        u = (tv[:, None, None] * pv).sum(-1) / det
        qv = np.cross(tv, e1)                                                                 # [F,3]
        w = (d[None] * qv[:, None, None]).sum(-1) / det
        t = (e2 * qv).sum(-1)[:, None, None] / det
    return t, np.stack([1.0 - u - w, u, w], -1)


def agreement_host(a, b, tols, depth_range=(0.0, np.inf)):
    """k_depth_agreement -> int64 [V,16]: both, first only, second only, neither, the fixed-point error sum, 0 0 0, within[8];
    and the error map."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    lo, hi = F32(depth_range[0]), F32(depth_range[1])
    with np.errstate(all="ignore"):
        va = np.isfinite(a) & (a > 0) & (a >= lo) & (a <= hi)
        vb = np.isfinite(b) & (b > 0) & (b >= lo) & (b <= hi)
        both = va & vb
        diff = np.abs(a - b).astype(F32)
        rel = (diff / b).astype(F32)
        fixed = np.rint(np.minimum(rel, F32(AG_CLAMP)).astype(np.float64) * float(AG_SCALE))
        out = np.zeros((a.shape[0], 16), np.int64)
        ax = (1, 2)
        out[:, 0], out[:, 1], out[:, 2] = both.sum(ax), (va & ~vb).sum(ax), (~va & vb).sum(ax)
        out[:, 3] = (~va & ~vb).sum(ax)
        out[:, 4] = np.where(both, fixed, 0).astype(np.int64).sum(ax)
        for k, tol in enumerate(tols):
            out[:, 8 + k] = (both & (diff <= (F32(tol) * b).astype(F32))).sum(ax)
    return out, np.where(both, rel, F32(np.nan)).astype(F32)


# ------------------------------------------------------------------------------------------------ the meshes and cameras
def _mesh(vertices, faces, seed=0, colours=True):
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    c = np.random.default_rng(300 + seed).integers(0, 256, v.shape, dtype=np.uint8) if colours else None
    return {"vertices": v, "faces": f, "rgb8": c, "counts": (int(v.shape[0]), int(f.shape[0]))}


def look(eye, R=None):
    """[3,4] fp32: a camera at eye whose frame is R (identity: it looks down -z with y up)."""
    M = np.zeros((3, 4), np.float64)
    M[:, :3] = np.eye(3) if R is None else R
    M[:, 3] = eye
    return M.astype(F32)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


SPHERE_C, SPHERE_R = (0.5, 0.25, -2.0), 0.5


@functools.lru_cache(maxsize=None)
def octa_sphere(levels=3):
    """The octahedron subdivided `levels` times onto the sphere (8 * 4^levels faces, wound outwards), closed and manifold, with
    its symmetric vertices exactly on the planes through the centre."""
    verts = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nxt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = np.array(verts[a]) + np.array(verts[b])
                verts.append(tuple(p / np.sqrt((p * p).sum())))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = nxt
    u = np.array(verts, np.float64)
    f = np.array(faces, np.int64)
    n = np.cross(u[f[:, 1]] - u[f[:, 0]], u[f[:, 2]] - u[f[:, 0]])
    assert ((n * u[f].mean(1)).sum(1) > 0).all()
    return _mesh(np.array(SPHERE_C) + SPHERE_R * u, f, seed=1)


# frames of the "sphere" case and what the parity test may say of each: outside (even), inside (odd, every pixel hit) or surface
SPHERE_FRAMES = ("outside", "inside", "surface", "outside rotated", "inside rotated")
SPHERE_KIND = ("outside", "inside", "surface", "outside", "inside")
SPHERE_NONDEGENERATE = (0, 1, 3, 4)


def sphere_cameras():
    c = np.array(SPHERE_C)
    on = octa_sphere()["vertices"][37].astype(np.float64)                                     # the camera sits on a vertex
    Ro, Ri = rot((0.3, 1.0, 0.2), 0.35), rot((1.0, -0.4, 0.6), 2.1)
    return np.stack([look(c + (0.0, 0.0, 1.7)), look(c + SPHERE_R * np.array((0.13, -0.07, 0.21))), look(on, rot((0, 1, 0), 0.4)),
                     look(c + Ro @ np.array((0.05, -0.03, 1.9)), Ro), look(c + SPHERE_R * np.array((-0.2, 0.3, 0.1)), Ri)])


def _case(mesh, c2w, W, H, f, cx=None, cy=None, depth_range=(0.0, np.inf), cull=None):
    c2w = np.asarray(c2w, F32).reshape(-1, 3, 4)
    return {"mesh": mesh, "c2w": c2w, "W": W, "H": H, "f": F32(f), "cx": F32(W / 2 if cx is None else cx),
            "cy": F32(H / 2 if cy is None else cy), "depth_range": depth_range, "cull": cull}


TRIANGLE = _mesh([(-0.6, -0.5, -2.0), (0.7, -0.4, -2.0), (0.1, 0.8, -2.0)], [(0, 1, 2)], seed=2)      # its normal is +z
QUAD_V = [(-0.8, -0.55, -3.0), (0.9, -0.6, -3.1), (0.85, 0.7, -2.9), (-0.75, 0.6, -3.2)]
# pixel extents (u, w) of faces whose boxes hold 64, 65 and SMALL_MAX pixels (257 is prime: no box inside an image holds it, so
# the threshold itself is crossed at 64 | 65 through lrf_debug_mesh_rasterize)
BOX_FACE = {64: ((10.3, 14.7), (20.3, 24.7)), 65: ((10.3, 11.7), (20.3, 29.7)), 256: ((10.3, 22.7), (20.3, 32.7))}


def _pixel_triangle(W, H, f, u, w, z=-2.0):
    """A triangle at depth -z whose corners project to the pixel coordinates (u0, w0), (u1, w0), (u0, w1)."""
    def pt(uu, ww):
        return ((uu + 0.5 - W / 2) / f * -z, -(ww + 0.5 - H / 2) / f * -z, z)
    return _mesh([pt(u[0], w[0]), pt(u[1], w[0]), pt(u[0], w[1])], [(0, 1, 2)], seed=3)


def _bad_faces():
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.uniform(-1, 1, (9, 2)), rng.uniform(-3.0, -2.0, (9, 1))], 1).astype(F32)
    v[7] = (np.nan, 0.0, -2.0)
    v[8] = (0.0, np.inf, -2.0)
    faces = [(0, 1, 2), (3, 3, 4), (0, 9, 1), (2, 3, 4), (-1, 0, 1), (4, 5, 4), (5, 6, 7), (0, 5, 6), (8, 1, 2), (1, 2, 1 << 30)]
    return _mesh(v, faces, seed=4)


@functools.lru_cache(maxsize=None)
def cases():
    origin = look((0.0, 0.0, 0.0))
    out = {}
    out["empty 5x7"] = _case(_mesh(np.zeros((0, 3)), np.zeros((0, 3)), colours=False), origin, 5, 7, 6.0)
    out["vertices without faces 5x7"] = _case(_mesh(TRIANGLE["vertices"], np.zeros((0, 3)), seed=2), origin, 5, 7, 6.0)
    out["triangle 1x1"] = _case(TRIANGLE, origin, 1, 1, 1.0)
    for cull in (None, "back", "front"):
        out[f"triangle from its normal's side 5x7 cull {cull}"] = _case(TRIANGLE, origin, 5, 7, 6.0, cull=cull)
        out[f"triangle from behind 5x7 cull {cull}"] = _case(TRIANGLE, look((0.0, 0.0, -4.0), rot((0, 1, 0), math.pi)), 5, 7, 6.0, cull=cull)
    out["quad diagonal 02"] = _case(_mesh(QUAD_V, [(0, 1, 2), (0, 2, 3)], seed=5), origin, 64, 48, 70.0)
    out["quad diagonal 13"] = _case(_mesh(QUAD_V, [(0, 1, 3), (1, 2, 3)], seed=5), origin, 64, 48, 70.0)
    poses3 = rigid_poses(np.random.default_rng(21), 3, angle=0.3, shift=0.4)
    poses3[:, 2, 3] += 4.0
    out["fan 130x70 V3"] = _case(fan(40, seed=9), poses3, 130, 70, 60.0, cx=65.25, cy=34.75)
    co = _mesh([(-1, -1, -3), (1, -1, -3), (0, 1, -3), (-1.2, 0.9, -3.5), (1.1, 1.0, -2.5)], [(3, 4, 0), (0, 1, 2), (0, 1, 2), (1, 2, 0)],
               seed=6)
    out["coincident faces"] = _case(co, origin, 64, 48, 50.0)
    out["bad faces"] = _case(_bad_faces(), origin, 64, 48, 40.0)
    out["behind the camera"] = _case(_mesh([(-1, -1, 2), (1, -1, 2.5), (0, 1, 3)], [(0, 1, 2)], seed=7), origin, 5, 7, 6.0)
    out["straddling the camera plane"] = _case(_mesh([(-0.5, -0.4, -2.0), (0.6, -0.3, -1.5), (0.2, 0.3, 1.0), (-0.3, 0.2, 0.5)],
                                                     [(0, 1, 2), (0, 2, 3)], seed=8), origin, 64, 48, 40.0)
    out["larger than the image"] = _case(_mesh([(-50, -40, -2.0), (60, -45, -3.0), (5, 70, -2.5)], [(0, 1, 2)], seed=9), origin, 64, 48, 50.0)
    for n, (u, w) in BOX_FACE.items():
        out[f"box of {n} pixels"] = _case(_pixel_triangle(64, 48, 50.0, u, w), origin, 64, 48, 50.0)
    cams = sphere_cameras()
    out["sphere 64x48 V5"] = _case(octa_sphere(), cams, 64, 48, 30.0)
    out["sphere depth range"] = _case(octa_sphere(), cams[[0, 3]], 64, 48, 30.0, depth_range=(1.45, 2.1))
    out["sphere cull back"] = _case(octa_sphere(), cams[[0, 1]], 64, 48, 30.0, cull="back")
    out["sphere ties"] = _case(octa_sphere(), look(SPHERE_C), 64, 48, 20.0, cx=32.5, cy=24.5)
    return out


CASE_NAMES = tuple(cases())


@functools.lru_cache(maxsize=None)
def expected(name):
    c = cases()[name]
    return rasterize_host(c["mesh"], c["c2w"], c["W"], c["H"], c["f"], c["cx"], c["cy"], c["depth_range"], c["cull"])


def agreement_maps(seed, V, H, W):
    """Two depth maps around 3 with planted NaN, infinities, zeros, negatives, exact equalities and values beyond the range."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.5, 6.0, (V, H, W)).astype(F32)
    a = (b * rng.choice(np.array([1.0, 1.0, 1.004, 0.97, 1.2, 40.0, 1e-3], F32), (V, H, W))).astype(F32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-30, 3e38, 50.0], F32)
    for m in (a, b):
        flat = m.reshape(-1)
        k = rng.permutation(flat.size)[:max(1, flat.size // 6)]
        flat[k] = specials[rng.integers(0, specials.size, k.size)]
    return a, b


AGREEMENT_SHAPES = ((1, 1, 1), (1, 7, 5), (3, 48, 64), (3, 70, 130))
AGREEMENT_TOLS = (0.0, 0.01, 0.05, 0.5)
