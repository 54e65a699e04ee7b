"""Shared pieces of the point-cloud tests: the numpy fp32 restatement of csrc/lrf_points.inl (same operation order, np.rint)
and the case builders.  Everything here is float32 arithmetic on float32 arrays; Python numbers only appear as weak scalars."""
import numpy as np

F32 = np.float32
OFFSETS4 = (-2, -1, 1, 2)


# ------------------------------------------------------------------------------------------------ restatement
def pixel_dirs(H, W, f, cx, cy):
    """[H,W,3]: ids2pixel + get_ray_directions_lean as pixel_dir (csrc/lrf_scene.inl) orders it."""
    f, cx, cy = F32(f), F32(cx), F32(cy)
    col = np.broadcast_to(np.arange(W, dtype=F32)[None, :], (H, W))
    row = np.broadcast_to(np.arange(H, dtype=F32)[:, None], (H, W))
    x = (col + F32(0.5) - cx) / f
    y = -(row + F32(0.5) - cy) / f
    return np.stack([x, y, np.full((H, W), -1, F32)], -1).astype(F32)


def pixel_dirs_360(H, W):
    """[H,W,3]: get_ray_directions_360 as pixel_dir orders it.  numpy's cos / sin need not round as the device's do, so this
    is compared with a tolerance only; the bit-for-bit tests take the 360 directions from lrf_scene_rays."""
    pi = F32(3.14159265358979323846)
    col = np.broadcast_to(np.arange(W, dtype=F32)[None, :], (H, W))
    row = np.broadcast_to(np.arange(H, dtype=F32)[:, None], (H, W))
    phi = (row + F32(0.5)) * pi / F32(H) - pi / F32(2)
    th = (col + F32(0.5)) * F32(2) * pi / F32(W) + pi
    return np.stack([np.cos(phi) * np.sin(th), np.sin(phi), np.cos(phi) * np.cos(th)], -1).astype(F32)


def world_points(depth, c2w, dirs):
    """depth [...,H,W] of ONE frame or [V,H,W] with c2w [V,3,4] -> pw [V,H,W,3]: pc = dir * d, pw = ((r0 x + r1 y) + r2 z) + t."""
    depth = np.asarray(depth, F32)
    M = np.asarray(c2w, F32)[:, None, None]                      # [V,1,1,3,4]
    with np.errstate(all="ignore"):
        x, y, z = dirs[..., 0] * depth, dirs[..., 1] * depth, dirs[..., 2] * depth
        out = [((M[..., r, 0] * x + M[..., r, 1] * y) + M[..., r, 2] * z) + M[..., r, 3] for r in range(3)]
    return np.stack(out, -1).astype(F32)


def reproject(pw, Mn, f, cx, cy):
    """World points pw [...,3] into the camera Mn [3,4]: (nz, u, w) with q = R^T (pw - t) as (c0 dx + c1 dy) + c2 dz, nz = -q.z,
    u = q.x / nz * f + cx - 0.5, w = -q.y / nz * f + cy - 0.5 (pts2px without its clip)."""
    f, cx, cy = F32(f), F32(cx), F32(cy)
    Mn = np.asarray(Mn, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = pw[..., 0] - Mn[0, 3], pw[..., 1] - Mn[1, 3], pw[..., 2] - Mn[2, 3]
        qx = (Mn[0, 0] * dx + Mn[1, 0] * dy) + Mn[2, 0] * dz
        qy = (Mn[0, 1] * dx + Mn[1, 1] * dy) + Mn[2, 1] * dz
        qz = (Mn[0, 2] * dx + Mn[1, 2] * dy) + Mn[2, 2] * dz
        nz = -qz
        u = qx / nz * f + cx - F32(0.5)
        w = -qy / nz * f + cy - F32(0.5)
    return nz.astype(F32), u.astype(F32), w.astype(F32)


def _finite_pos(d):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def keep_mask(depth, c2w, f, cx, cy, fov360=False, stride=1, depth_range=(0.0, np.inf), neighbours=(), rel_tol=0.02,
              min_consistent=1, dirs=None):
    """-> (keep [V,Hs,Ws] bool, pw [V,Hs,Ws,3]) over the candidates (pixels at multiples of stride)."""
    depth = np.asarray(depth, F32)
    c2w = np.asarray(c2w, F32)
    V, H, W = depth.shape
    if dirs is None:
        dirs = pixel_dirs_360(H, W) if fov360 else pixel_dirs(H, W, f, cx, cy)
    s = int(stride)
    d = depth[:, ::s, ::s]
    lo, hi, tol = F32(depth_range[0]), F32(depth_range[1]), F32(rel_tol)
    with np.errstate(invalid="ignore"):
        keep = _finite_pos(d) & (d >= lo) & (d <= hi)
    pw = world_points(d, c2w, dirs[::s, ::s])
    if not len(neighbours):
        return keep, pw
    assert not fov360
    for v in range(V):
        in_range = 0
        passes = np.zeros(d.shape[1:], np.int64)
        for o in neighbours:
            n = v + int(o)
            if not 0 <= n < V:
                continue
            in_range += 1
            nz, u, w = reproject(pw[v], c2w[n], f, cx, cy)
            with np.errstate(invalid="ignore"):
                ru, rw = np.rint(u), np.rint(w)
                ok = (nz > 0) & (ru >= 0) & (ru < F32(2147483648.0)) & (rw >= 0) & (rw < F32(2147483648.0))
            iu = np.where(ok, ru, 0).astype(np.int64)
            iw = np.where(ok, rw, 0).astype(np.int64)
            ok &= (iu < W) & (iw < H)
            dn = depth[n][np.where(ok, iw, 0), np.where(ok, iu, 0)]
            ok &= _finite_pos(dn)
            with np.errstate(all="ignore"):
                ok &= np.abs(nz - dn) <= tol * dn
            passes += ok
        keep[v] &= passes >= min(int(min_consistent), in_range)
    return keep, pw


def fuse_host(depth, rgb8, c2w, f, cx, cy, **kw):
    """The whole of lrf_points_fuse on the host -> dict(count, xyz [M,3] fp32, rgb8 [M,3] uint8 or None, src [M,2] int32), in
    (frame, row, column) order."""
    depth = np.asarray(depth, F32)
    V, H, W = depth.shape
    s = int(kw.get("stride", 1))
    keep, pw = keep_mask(depth, c2w, f, cx, cy, **kw)
    v, js, is_ = np.nonzero(keep)                                 # C order: frame, row, column
    pix = js * s * W + is_ * s
    out = {"count": int(keep.sum()), "xyz": pw[keep].astype(F32), "src": np.stack([v, pix], -1).astype(np.int32), "rgb8": None}
    if rgb8 is not None:
        out["rgb8"] = np.asarray(rgb8, np.uint8)[v, js * s, is_ * s]
    return out


# ------------------------------------------------------------------------------------------------ cases
def rigid_poses(rng, V, angle=0.2, shift=0.5):
    """[V,3,4] fp32: random axis-angle rotations of up to `angle` rad (Rodrigues in fp64) and translations within `shift`."""
    out = np.zeros((V, 3, 4), np.float64)
    for v in range(V):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        t = rng.uniform(-angle, angle)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        out[v, :, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
        out[v, :, 3] = rng.uniform(-shift, shift, 3)
    return out.astype(F32)


def random_case(seed, V, H, W, smooth=True, angle=0.05, shift=0.1):
    """Case (a): depths with planted NaN, +-inf, 0, negative and out-of-range values, random rigid poses, random colours.
    smooth: a slowly varying surface around depth 3 (so that neighbouring frames agree in places); else uniform noise."""
    rng = np.random.default_rng(seed)
    if smooth:
        jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        depth = np.stack([3.0 + 0.4 * np.sin(0.11 * ii + 0.3 * v) * np.cos(0.07 * jj) + 0.03 * rng.normal(size=(H, W))
                          for v in range(V)]).astype(F32)
    else:
        depth = rng.uniform(0.2, 6.0, (V, H, W)).astype(F32)
    flat = depth.reshape(-1)
    k = rng.permutation(flat.size)[:max(1, flat.size // 8)] if flat.size > 1 else np.array([], np.int64)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-3, 50.0, 1e30, 1e-40], F32)
    flat[k] = specials[rng.integers(0, specials.size, k.size)]
    rgb8 = rng.integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    f = F32(0.9 * W)
    return {"depth": depth, "rgb8": rgb8, "c2w": rigid_poses(rng, V, angle, shift), "f": f, "cx": F32(W / 2 + 0.25),
            "cy": F32(H / 2 - 0.25), "depth_range": (0.05, 20.0)}


def trajectory_case(seed=7):
    """Case (b): 7 cameras of 48 x 64 pixels (focal 60, centre at the image centre) on a gentle arc -- 0.15 apart in x, turned
    0.04 rad about y per frame -- looking down -z at the plane z = -4 with a sphere of radius 0.6 at (0.2, 0, -3) in front of it.
    Depth by exact ray casting in fp64 as a multiple of the un-normalised direction, rounded to fp32; 15 % of the pixels are
    then replaced by floaters at 0.4 / 0.55 / 1.8 times their depth.  -> dict with depth, clean (the ray-cast depth), floater
    [V,H,W] bool, c2w, f, cx, cy, rgb8."""
    V, H, W = 7, 48, 64
    f, cx, cy = 60.0, W / 2.0, H / 2.0
    rng = np.random.default_rng(seed)
    c2w = np.zeros((V, 3, 4), np.float64)
    for k in range(V):
        a = 0.04 * (k - 3)
        c2w[k, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[k, :, 3] = [0.15 * (k - 3), 0.0, 0.0]
    c2w = c2w.astype(F32)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dirs = np.stack([(col + 0.5 - cx) / f, -(row + 0.5 - cy) / f, -np.ones_like(col)], -1)
    centre, radius = np.array([0.2, 0.0, -3.0]), 0.6
    clean = np.zeros((V, H, W), np.float64)
    for k in range(V):
        M = c2w[k].astype(np.float64)
        dw = dirs @ M[:, :3].T
        o = M[:, 3]
        t_plane = (-4.0 - o[2]) / dw[..., 2]
        oc = o - centre
        A = (dw * dw).sum(-1)
        B = 2.0 * (dw * oc).sum(-1)
        Cc = (oc * oc).sum() - radius * radius
        disc = B * B - 4 * A * Cc
        with np.errstate(invalid="ignore"):
            t_sph = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        t_sph = np.where(t_sph > 0, t_sph, np.inf)
        clean[k] = np.minimum(t_plane, t_sph)
    clean = clean.astype(F32)
    floater = rng.random((V, H, W)) < 0.15
    factor = np.array([0.4, 0.55, 1.8], F32)[rng.integers(0, 3, (V, H, W))]
    depth = np.where(floater, clean * factor, clean).astype(F32)
    rgb8 = rng.integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    return {"depth": depth, "clean": clean, "floater": floater, "c2w": c2w, "f": F32(f), "cx": F32(cx), "cy": F32(cy),
            "rgb8": rgb8}


def trajectory_shares(case, neighbours=OFFSETS4, rel_tol=0.02, min_consistent=2, all_offsets=True):
    """(kept share of all candidates, kept share of the untouched pixels whose reprojections fall inside the neighbours,
    rejected share of the planted floaters) of case (b), from the restatement alone.  all_offsets: only pixels of the frames
    that have every offset's neighbour (four reprojections); else also the end frames' pixels, judged by the reprojections
    into the neighbours they have."""
    depth, c2w, f, cx, cy = case["depth"], case["c2w"], case["f"], case["cx"], case["cy"]
    V, H, W = depth.shape
    keep, pw = keep_mask(depth, c2w, f, cx, cy, neighbours=neighbours, rel_tol=rel_tol, min_consistent=min_consistent)
    inside_all = np.zeros((V, H, W), bool)
    for v in range(V):
        if all_offsets and not all(0 <= v + o < V for o in neighbours):
            continue
        ok = np.ones((H, W), bool)
        for o in neighbours:
            if not 0 <= v + o < V:
                continue
            nz, u, w = reproject(pw[v], c2w[v + o], f, cx, cy)
            ru, rw = np.rint(u), np.rint(w)
            ok &= (nz > 0) & (ru >= 0) & (ru <= W - 1) & (rw >= 0) & (rw <= H - 1)
        inside_all[v] = ok
    untouched = ~case["floater"] & inside_all
    return (float(keep.mean()), float(keep[untouched].mean()), float(1.0 - keep[case["floater"]].mean()))
