"""Shared pieces of the texture-bake tests: the numpy restatement of csrc/lrf_mesh_texture.inl (same operation order: fp32
weights, points, projection, visibility and bilinear taps, fp64 normals and facing rounded one by one, frames folded in frame
order), an independent fp64 implementation (4 x 4 matrices, normalised vectors with sqrt) that also marks the texels sitting on
a decision, analytic frames, and the cases.  mesh_depth comes from mesh_raster_cases' restatement of the rasteriser."""
import functools
import math

import numpy as np

from mesh_raster_cases import (TRIANGLE, _bad_faces, _mesh, cases as raster_cases, face_kinds, look, octa_sphere, rasterize_host,
                               rot, sphere_cameras, to_camera)

F32, F64 = np.float32, np.float64
BLEND = {"mean": 0, "best": 1}
INFO_KEYS = ("bad_index_faces", "degenerate_faces", "nonfinite_faces", "zero_area_faces", "used_texels", "observed_texels",
             "fallback_texels", "empty_texels")
# the analytic frames: channel k of pixel (i, j) of frame v is 127.5 + AMP sin(WX i + 0.7 k + 0.9 v) cos(WY j + 0.3 k); its
# gradient is at most AMP hypot(WX, WY) levels per pixel of distance
AMP, WX, WY = 60.0, 0.11, 0.13
G_LEVELS = AMP * math.hypot(WX, WY)


# ------------------------------------------------------------------------------------------------ the layout
def layout_host(Nf, P, cols=None):
    cells = (Nf + 1) // 2
    if cols is None:
        cols = 1
        while cols * cols < cells:
            cols += 1
    rows = (cells + cols - 1) // cols
    return rows, cols, rows * P, cols * P


def texels_host(Nf, P, cols):
    """Per texel of the atlas [Ht,Wt]: its face (Nf where empty) and (a, b) inside the face's half."""
    rows, cols, Ht, Wt = layout_host(Nf, P, cols)
    y, x = np.meshgrid(np.arange(Ht, dtype=np.int64), np.arange(Wt, dtype=np.int64), indexing="ij")
    c, a, b = (y // P) * cols + x // P, x % P, y % P
    odd = a + b > P - 1
    a, b = np.where(odd, P - 1 - a, a), np.where(odd, P - 1 - b, b)
    return np.minimum(2 * c + odd, Nf), a, b


def weights_host(a, b, P):
    K = F32(P - 3)
    beta, gamma = a.astype(F32) / K, b.astype(F32) / K
    return (F32(1) - beta) - gamma, beta, gamma


def uv_host(Nf, P, cols=None):
    rows, cols, Ht, Wt = layout_host(Nf, P, cols)
    K = P - 3
    uv = np.zeros((Nf, 3, 2), F64)
    for f in range(Nf):
        c = f // 2
        X0, Y0 = (c % cols) * P, (c // cols) * P
        if f % 2 == 0:
            px = [(X0 + .5, Y0 + .5), (X0 + K + .5, Y0 + .5), (X0 + .5, Y0 + K + .5)]
        else:
            px = [(X0 + P - .5, Y0 + P - .5), (X0 + P - K - .5, Y0 + P - .5), (X0 + P - .5, Y0 + P - K - .5)]
        uv[f] = [(x / Wt, 1.0 - y / Ht) for x, y in px]
    return uv.astype(F32)


# ------------------------------------------------------------------------------------------------ the restatement
def faces_host(mesh):
    """-> kind [Nf] (face_kinds' 0..3, 4: a zero normal), corners [Nf,3,3] fp32 (0 where not read), n [Nf,3] and nn [Nf] fp64."""
    v, f = np.asarray(mesh["vertices"], F32), np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    kind = face_kinds(mesh)
    p = np.zeros((f.shape[0], 3, 3), F32)
    p[kind != 1] = v[f[kind != 1]]
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1].astype(F64) - p[:, 0].astype(F64), p[:, 2].astype(F64) - p[:, 0].astype(F64)
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    kind = np.where((kind == 0) & (nn == 0), 4, kind)
    return kind, p, n, nn


def bake_host(mesh, P, cols, frames, mesh_depth, c2w, f, cx, cy, blend="mean", vis_tol=0.02, min_cos=0.2, two_sided=False, state=None):
    """k_tx_bake -> state [Ht,Wt,4] fp32 (a copy when `state` is given: the frames go on top of it)."""
    Nf = np.asarray(mesh["faces"]).reshape(-1, 3).shape[0]
    rows, cols, Ht, Wt = layout_host(Nf, P, cols)
    state = np.zeros((Ht, Wt, 4), F32) if state is None else np.array(state, F32)
    if Nf == 0:
        return state
    face, a, b = texels_host(Nf, P, cols)
    kind, p, n, nn = faces_host(mesh)
    fz = np.minimum(face, Nf - 1)
    live = (face < Nf) & (kind[fz] == 0)
    alpha, beta, gamma = weights_host(a, b, P)
    c2w, frames, mesh_depth = np.asarray(c2w, F32).reshape(-1, 3, 4), np.asarray(frames, np.uint8), np.asarray(mesh_depth, F32)
    V, H, W = mesh_depth.shape
    f, cx, cy, vt = F32(f), F32(cx), F32(cy), F32(vis_tol)
    mc = F64(F32(min_cos))
    mc2 = mc * mc
    with np.errstate(all="ignore"):
        pc = p[fz]                                                                                # [Ht,Wt,3,3]
        pw = ((alpha[..., None] * pc[:, :, 0] + beta[..., None] * pc[:, :, 1]) + gamma[..., None] * pc[:, :, 2]).astype(F32)
        nf_, nnf = n[fz], nn[fz]
        for v in range(V):
            M = c2w[v]
            q = to_camera(pw, M)
            nz = -q[..., 2]
            ok = live & (nz > 0)
            u = (q[..., 0] / nz * f + cx - F32(0.5)).astype(F32)
            w = (-q[..., 1] / nz * f + cy - F32(0.5)).astype(F32)
            ru, rw = np.rint(u), np.rint(w)
            ok &= (ru >= 0) & (ru < W) & (rw >= 0) & (rw < H)
            d = M[:, 3].astype(F64) - pw.astype(F64)
            s = (nf_[..., 0] * d[..., 0] + nf_[..., 1] * d[..., 1]) + nf_[..., 2] * d[..., 2]
            dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            ok &= (True if two_sided else (s > 0)) & ~(s * s < mc2 * (nnf * dd))
            iu, iw = np.where(ok, ru, 0).astype(np.int64), np.where(ok, rw, 0).astype(np.int64)
            dm = mesh_depth[v][iw, iu]
            ok &= np.isfinite(dm) & (dm > 0) & (np.abs(nz - dm).astype(F32) <= (vt * dm).astype(F32))
            wt = ((s * s) / (nnf * (dd * dd))).astype(F32)
            ok &= np.isfinite(wt) & (wt > 0)
            xf, yf = np.floor(u), np.floor(w)
            fx, fy = (u - xf).astype(F32), (w - yf).astype(F32)
            x0, y0 = np.where(ok, xf, 0).astype(np.int64), np.where(ok, yf, 0).astype(np.int64)
            xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
            ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
            img = frames[v].astype(F32)
            c00, c10, c01, c11 = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]
            top = (c00 + fx[..., None] * (c10 - c00)).astype(F32)
            bot = (c01 + fx[..., None] * (c11 - c01)).astype(F32)
            col = (top + fy[..., None] * (bot - top)).astype(F32)
            if BLEND[blend] == 0:
                new = np.concatenate([state[..., :3] + wt[..., None] * col, (state[..., 3] + wt)[..., None]], -1).astype(F32)
            else:
                ok &= wt > state[..., 3]
                new = np.concatenate([col, wt[..., None]], -1).astype(F32)
            state = np.where(ok[..., None], new, state)
    return state


def _byte(x):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.rint(x.astype(F32)), F32(0)), F32(255))


def resolve_host(mesh, P, cols, state, blend="mean", fill=(0, 0, 0)):
    """k_tx_resolve -> dict(atlas [Ht,Wt,3] uint8, mask [Ht,Wt] uint8, info)."""
    Nf = np.asarray(mesh["faces"]).reshape(-1, 3).shape[0]
    rows, cols, Ht, Wt = layout_host(Nf, P, cols)
    atlas = np.empty((Ht, Wt, 3), np.uint8)
    atlas[:] = np.asarray(fill, np.uint8)
    info = dict.fromkeys(INFO_KEYS, 0)
    if Nf == 0:
        return {"atlas": atlas, "mask": np.zeros((Ht, Wt), np.uint8), "info": info}
    face, a, b = texels_host(Nf, P, cols)
    kind = faces_host(mesh)[0]
    fz = np.minimum(face, Nf - 1)
    used = face < Nf
    state = np.asarray(state, F32)
    sw = state[..., 3]
    observed = used & (sw > 0)
    with np.errstate(all="ignore"):
        col = _byte(state[..., :3] / sw[..., None]) if BLEND[blend] == 0 else _byte(state[..., :3])
    atlas[observed] = col[observed].astype(np.uint8)
    fallback = used & ~observed & (kind[fz] != 1) & (mesh.get("rgb8") is not None)
    if fallback.any():
        alpha, beta, gamma = weights_host(a, b, P)
        w = [np.clip(t.astype(F64), 0.0, 1.0) for t in (alpha, beta, gamma)]
        tot = (w[0] + w[1]) + w[2]
        w = [t / tot for t in w]
        idx = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)[fz[fallback]]
        c = np.asarray(mesh["rgb8"], np.uint8)[idx].astype(F64)                                   # [T,3 corners,3 channels]
        ww = [t[fallback][:, None] for t in w]
        m = np.rint((ww[0] * c[:, 0] + ww[1] * c[:, 1]) + ww[2] * c[:, 2])
        atlas[fallback] = np.clip(m, 0, 255).astype(np.uint8)
    for k, key in ((1, "bad_index_faces"), (2, "degenerate_faces"), (3, "nonfinite_faces"), (4, "zero_area_faces")):
        info[key] = int((kind == k).sum())
    info.update(used_texels=int(used.sum()), observed_texels=int(observed.sum()), fallback_texels=int(fallback.sum()),
                empty_texels=int((~used).sum()))
    return {"atlas": atlas, "mask": observed.astype(np.uint8), "info": info}


# ------------------------------------------------------------------------------------------------ an independent fp64 baker
def bake_fp64(mesh, P, cols, frames, mesh_depth, c2w, f, cx, cy, blend="mean", vis_tol=0.02, min_cos=0.2, two_sided=False,
              fill=(0, 0, 0)):
    """Items 1 to 5 in fp64 with 4 x 4 matrices and unit vectors -> (atlas uint8, mask, decision [Ht,Wt] bool): a texel sits on a
    decision when in some frame its visibility is within 1e-4 (relative) of vis_tol, its cosine within 1e-6 of min_cos (or of 0
    when one-sided), its pixel coordinate within 1e-4 of a tie or of the image border, its camera depth within 1e-6 of 0, or,
    under "best", its two largest weights within 1e-6 (relative) of each other without being equal
    (a repeated pose gives equal weights on both sides, and both keep the earliest frame)."""
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    Nf = faces.shape[0]
    rows, cols, Ht, Wt = layout_host(Nf, P, cols)
    atlas = np.empty((Ht, Wt, 3), np.uint8)
    atlas[:] = np.asarray(fill, np.uint8)
    if Nf == 0:
        return atlas, np.zeros((Ht, Wt), bool), np.zeros((Ht, Wt), bool)
    face, a, b = texels_host(Nf, P, cols)
    kind = faces_host(mesh)[0]
    fz = np.minimum(face, Nf - 1)
    used = face < Nf
    live = used & (kind[fz] == 0)
    K = float(P - 3)
    bary = np.stack([1.0 - (a + b) / K, a / K, b / K], -1)                                        # [Ht,Wt,3]
    vtx = np.asarray(mesh["vertices"], F64)
    mesh_depth = np.asarray(mesh_depth, F64)
    V, H, W = mesh_depth.shape
    f, cx, cy = float(f), float(cx), float(cy)
    with np.errstate(all="ignore"):
        corners = np.where((kind != 1)[:, None, None], vtx[np.clip(faces, 0, vtx.shape[0] - 1)], 0.0)[fz]
        pt = np.einsum("hwk,hwkc->hwc", bary, corners)
        nrm = np.cross(corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0])
        nrm = nrm / np.sqrt((nrm * nrm).sum(-1))[..., None]
        decision = np.zeros((Ht, Wt), bool)
        sw, sc = np.zeros((Ht, Wt)), np.zeros((Ht, Wt, 3))
        second = np.zeros((Ht, Wt))
        for v in range(V):
            M = np.eye(4)
            M[:3] = np.asarray(c2w, F64).reshape(-1, 3, 4)[v]
            pc = np.concatenate([pt, np.ones((Ht, Wt, 1))], -1) @ np.linalg.inv(M).T
            z = -pc[..., 2]
            u, w = pc[..., 0] / z * f + cx - 0.5, -pc[..., 1] / z * f + cy - 0.5
            ok = live & (z > 0)
            edge = live & (np.abs(z) <= 1e-6)
            for t, n in ((u, W), (w, H)):
                near = (np.abs(np.abs(t - np.floor(t)) - 0.5) <= 1e-4) | (np.abs(t + 0.5) <= 1e-4) | (np.abs(t - (n - 0.5)) <= 1e-4)
                edge |= ok & near
            iu, iw = np.rint(u), np.rint(w)
            ok &= (iu >= 0) & (iu < W) & (iw >= 0) & (iw < H)
            to_cam = M[:3, 3] - pt
            dist = np.sqrt((to_cam * to_cam).sum(-1))
            cos = (nrm * to_cam).sum(-1) / dist
            edge |= ok & (np.abs(np.abs(cos) - min_cos) <= 1e-6)
            if two_sided:
                cos = np.abs(cos)
            else:
                edge |= ok & (np.abs(cos) <= 1e-6)
            ok &= (cos > 0) & (cos >= min_cos)
            dm = mesh_depth[v][np.where(ok, iw, 0).astype(np.int64), np.where(ok, iu, 0).astype(np.int64)]
            good = np.isfinite(dm) & (dm > 0)
            rel = np.abs(z - dm) / dm
            edge |= ok & good & (np.abs(rel - vis_tol) <= 1e-4 * vis_tol)
            ok &= good & (rel <= vis_tol)
            wt = cos * cos / (dist * dist)
            x0, y0 = np.floor(u), np.floor(w)
            fx, fy = (u - x0)[..., None], (w - y0)[..., None]
            x0, y0 = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
            xa, xb, ya, yb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
            img = np.asarray(frames[v], F64)
            col = (1 - fy) * ((1 - fx) * img[ya, xa] + fx * img[ya, xb]) + fy * ((1 - fx) * img[yb, xa] + fx * img[yb, xb])
            decision |= edge
            if BLEND[blend] == 0:
                sw, sc = np.where(ok, sw + wt, sw), np.where(ok[..., None], sc + wt[..., None] * col, sc)
            else:
                wv = np.where(ok, wt, 0.0)
                second = np.where(wv > sw, sw, np.maximum(second, wv))
                better = ok & (wv > sw)
                sw, sc = np.where(better, wv, sw), np.where(better[..., None], col, sc)
        if BLEND[blend] == 1:
            decision |= (sw > 0) & (sw != second) & (sw - second <= 1e-6 * sw)   # equal weights (a repeated pose): the earliest, here too
        observed = used & (sw > 0)
        mean = sc / sw[..., None] if BLEND[blend] == 0 else sc
        atlas[observed] = np.clip(np.rint(mean[observed]), 0, 255).astype(np.uint8)
        if mesh.get("rgb8") is not None:
            fb = used & ~observed & (kind[fz] != 1)
            wgt = np.clip(bary[fb], 0.0, 1.0)
            wgt = wgt / wgt.sum(-1, keepdims=True)
            c = np.asarray(mesh["rgb8"], F64)[faces[fz[fb]]]
            atlas[fb] = np.clip(np.rint(np.einsum("tk,tkc->tc", wgt, c)), 0, 255).astype(np.uint8)
    return atlas, observed, decision


# ------------------------------------------------------------------------------------------------ frames, meshes, cameras
def analytic_frames(V, H, W, first=0):
    v, j, i, k = np.meshgrid(np.arange(first, first + V), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    c = 127.5 + AMP * np.sin(WX * i + 0.7 * k + 0.9 * v) * np.cos(WY * j + 0.3 * k)
    return np.rint(c).astype(np.uint8)


def _join(*meshes):
    v, f, c, base = [], [], [], 0
    for m in meshes:
        v.append(m["vertices"]), f.append(m["faces"] + base), c.append(m["rgb8"])
        base += m["vertices"].shape[0]
    out = _mesh(np.concatenate(v), np.concatenate(f), colours=False)
    out["rgb8"] = np.concatenate(c)
    return out


WALL_Z, WALL_NX, WALL_NY = -3.0, 6, 5


@functools.lru_cache(maxsize=None)
def wall_scene():
    """The octahedron sphere of mesh_raster_cases in front of a wall z = WALL_Z of WALL_NX x WALL_NY quads whose normal is +z."""
    xs, ys = np.linspace(-1.0, 2.0, WALL_NX + 1), np.linspace(-1.0, 1.5, WALL_NY + 1)
    v = [(x, y, WALL_Z) for y in ys for x in xs]
    f = []
    for j in range(WALL_NY):
        for i in range(WALL_NX):
            k = j * (WALL_NX + 1) + i
            f += [(k, k + 1, k + WALL_NX + 2), (k, k + WALL_NX + 2, k + WALL_NX + 1)]
    return _join(octa_sphere(), _mesh(v, f, seed=12))


WALL_CAMERAS = np.stack([look((0.5, 0.25, 0.0)), look((-0.6, 0.25, 0.0)), look((1.4, 0.6, -0.2))])
ROUND_TRIP = {"sphere": ("sphere P8 mean", (0, 3)), "wall": ("wall P8 mean", (0, 1, 2))}


def _tilted(cos, scale=0.3):
    """TRIANGLE shrunk about its centroid and turned about the x axis until its normal makes acos(cos) with the +z axis."""
    v = TRIANGLE["vertices"].astype(F64)
    c = v.mean(0)
    out = dict(TRIANGLE)
    out["vertices"] = (c + (scale * (v - c)) @ rot((1, 0, 0), math.acos(cos)).T).astype(F32)
    return out


def _case(mesh, c2w, W, H, f, P=8, cols=None, blend="mean", two_sided=False, vis_tol=0.02, min_cos=0.2, fill=(0, 0, 0), cx=None, cy=None):
    c2w = np.asarray(c2w, F32).reshape(-1, 3, 4)
    return {"mesh": mesh, "c2w": c2w, "W": W, "H": H, "f": F32(f), "cx": F32(W / 2 + 0.137 if cx is None else cx),
            "cy": F32(H / 2 - 0.211 if cy is None else cy), "P": P, "cols": cols, "blend": blend, "two_sided": two_sided,
            "vis_tol": vis_tol, "min_cos": min_cos, "fill": fill}


@functools.lru_cache(maxsize=None)
def cases():
    origin, behind = look((0.0, 0.0, 0.0)), look((0.0, 0.0, -4.0), rot((0, 1, 0), math.pi))
    away = look((0.0, 0.0, 0.0), rot((0, 1, 0), math.pi))                                         # the mesh is behind this camera
    tri = TRIANGLE
    quad = _mesh([(-0.8, -0.55, -3.0), (0.9, -0.6, -3.1), (0.85, 0.7, -2.9), (-0.75, 0.6, -3.2)], [(0, 1, 2), (0, 2, 3)], seed=5)
    three = _mesh(np.concatenate([quad["vertices"], [(1.6, 0.1, -3.0)]]), [(0, 1, 2), (0, 2, 3), (1, 4, 2)], seed=6)
    far = _mesh(np.concatenate([tri["vertices"], [(40.0, 0.0, -2.0), (41.0, 0.0, -2.0), (40.0, 1.0, -2.0)]]), [(0, 1, 2), (3, 4, 5)], seed=7)
    plain = dict(far, rgb8=None)
    fan_case = raster_cases()["fan 130x70 V3"]
    cams = sphere_cameras()
    out = {}
    out["empty 5x7 P4"] = _case(_mesh(np.zeros((0, 3)), np.zeros((0, 3)), colours=False), origin, 5, 7, 6.0, P=4)
    out["Nf 1 1x1 P4"] = _case(tri, origin, 1, 1, 1.0, P=4)
    out["Nf 2 5x7 P5 cols 1 V2"] = _case(quad, [origin, look((0.2, -0.1, 0.3))], 5, 7, 6.0, P=5, cols=1)
    for blend in ("mean", "best"):
        out[f"Nf 3 5x7 P8 V3 {blend}"] = _case(three, [origin, look((0.2, -0.1, 0.3)), look((-0.3, 0.1, -0.2))], 5, 7, 6.0, blend=blend)
        out[f"fan P5 cols 4 V3 {blend}"] = _case(fan_case["mesh"], fan_case["c2w"], 64, 48, 30.0, P=5, cols=4, blend=blend, two_sided=True)
        out[f"wall P8 {blend}"] = _case(wall_scene(), WALL_CAMERAS, 64, 48, 30.0, blend=blend)
    out["sphere P8 mean"] = _case(octa_sphere(), cams, 64, 48, 30.0)
    out["sphere P16 cols 7 best two-sided"] = _case(octa_sphere(), cams[[1, 3]], 64, 48, 30.0, P=16, cols=7, blend="best", two_sided=True)
    for two in (False, True):
        out[f"triangle from behind two_sided {two}"] = _case(tri, behind, 64, 48, 40.0, P=8, two_sided=two)
    out["a frame behind the camera"] = _case(tri, [away, origin], 64, 48, 40.0, P=8)
    out["outside every image, vertex colours"] = _case(far, origin, 64, 48, 40.0, P=8, fill=(9, 200, 77))
    out["outside every image, fill"] = _case(plain, origin, 64, 48, 40.0, P=8, fill=(9, 200, 77))
    out["bad faces"] = _case(_bad_faces(), origin, 64, 48, 40.0, P=4, cols=3, two_sided=True)
    out["grazing above min_cos"] = _case(_tilted(0.25), origin, 64, 48, 40.0, P=8, vis_tol=0.1)
    out["grazing below min_cos"] = _case(_tilted(0.15), origin, 64, 48, 40.0, P=8, vis_tol=0.1)
    out["equal weights under best"] = _case(quad, [origin, origin, look((0.0, 0.0, 0.5))], 5, 7, 6.0, P=5, blend="best")
    return out


CASE_NAMES = tuple(cases())


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (frames uint8 [V,H,W,3], mesh_depth [V,H,W] fp32: the restated rasteriser, cull "back" unless two_sided)."""
    c = cases()[name]
    V = c["c2w"].shape[0]
    ras = rasterize_host(c["mesh"], c["c2w"], c["W"], c["H"], c["f"], c["cx"], c["cy"], cull=None if c["two_sided"] else "back")
    return analytic_frames(V, c["H"], c["W"]), ras["depth"]


def bake_case(name, frame_ids=None, state=None):
    c = cases()[name]
    frames, depth = inputs(name)
    ids = list(range(c["c2w"].shape[0])) if frame_ids is None else list(frame_ids)
    return bake_host(c["mesh"], c["P"], c["cols"], frames[ids], depth[ids], c["c2w"][ids], c["f"], c["cx"], c["cy"], c["blend"],
                     c["vis_tol"], c["min_cos"], c["two_sided"], state)


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> dict(state, atlas, mask, uv, info): the restatement over all frames of the case."""
    c = cases()[name]
    state = bake_case(name)
    out = resolve_host(c["mesh"], c["P"], c["cols"], state, c["blend"], c["fill"])
    out["state"] = state
    out["uv"] = uv_host(np.asarray(c["mesh"]["faces"]).reshape(-1, 3).shape[0], c["P"], c["cols"])
    return out
