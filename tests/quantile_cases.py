"""Shared pieces of the depth-quantile tests.

  restate(w, z, rays, q)        numpy fp32 restatement of csrc/lrf_quantile.inl in the kernel's operation order (scan="tree"),
                                or the same arithmetic with a sequential fp32 prefix sum (scan="sequential"): the yardstick
  oracle64(w, z, rays, q)       the definition in fp64 on the GIVEN fp32 weights: sequential np.cumsum in float64, the same
                                crossing rule; flags the (quantile, ray) pairs whose crossing index can legitimately differ
                                (some fp64 C_i within FLAG_C of q) or whose t is ill-conditioned (w_{i*} < FLAG_W)
  compare(label, w, z, rays, q, depth, index)   an implementation against the oracle: the cap, the index, the bound
  composite / synthetic / adversarial   weight sets
  oracle_weights(f, rays, ...)  the weights of a field on the CPU from the pieces of oracle/vm_render_torch.py
"""
import numpy as np
import torch

from oracle import vm_render_torch as O

FLAG_C = 1e-5
FLAG_W = 1e-4
MAX_FLAGGED = 0.02
F32 = np.float32


def ray_norm32(rays):
    """|d| as the kernel forms it: sqrt((dx dx + dy dy) + dz dz), every operation rounded to fp32."""
    d = np.asarray(rays, F32)[:, 3:6]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=F32)


def tree_scan32(w):
    """C [R,S] fp32 as k_depth_quantiles sums it: per 64-sample step an inclusive Hillis-Steele scan over the lanes (zeros
    beyond S), plus the carry: lane 63 of the step before."""
    w = np.asarray(w, F32)
    R, S = w.shape
    C = np.empty((R, S), F32)
    carry = np.zeros(R, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, S, 64):
            n = min(64, S - k0)
            p = np.zeros((R, 64), F32)
            p[:, :n] = w[:, k0:k0 + n]
            d = 1
            while d < 64:
                nxt = p.copy()
                nxt[:, d:] = p[:, d:] + p[:, :-d]
                p = nxt
                d *= 2
            c = carry[:, None] + p
            C[:, k0:k0 + n] = c[:, :n]
            carry = c[:, 63].copy()
    return C


def _finish(C, w, z, dn, q, dtype):
    """The crossing and the interpolation on a given prefix sum, in dtype.  -> (depth [R], index [R] int32)."""
    R, S = C.shape
    q = dtype(q)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        hit = C >= q
        found = hit.any(1)
        i = hit.argmax(1)
        rows = np.arange(R)
        prev = np.where(i > 0, C[rows, np.maximum(i - 1, 0)], dtype(0))
        t = np.minimum(np.maximum((q - prev) / w[rows, i], dtype(0)), dtype(1))
        z0, z1 = z[i], z[np.minimum(i + 1, S - 1)]
        depth = (z0 + t * (z1 - z0)) / dn
    depth = np.where(found, depth, dtype(0)).astype(dtype)
    return depth, np.where(found, i, -1).astype(np.int32)


def restate(w, z, rays, q, scan="tree"):
    """-> (depth [K,R] fp32, index [K,R] int32), bit for bit what the kernel stores (scan="tree")."""
    w, z = np.ascontiguousarray(w, F32), np.asarray(z, F32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        C = tree_scan32(w) if scan == "tree" else np.cumsum(w, axis=1, dtype=F32)
    dn = ray_norm32(rays)
    out = [_finish(C, w, z, dn, F32(qk), F32) for qk in q]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def oracle64(w, z, rays, q):
    """-> (depth [K,R] fp64, index [K,R] int32, flagged [K,R] bool) of the given fp32 weights; q as the fp32 value the
    kernel receives."""
    w64, z64 = np.asarray(w, F32).astype(np.float64), np.asarray(z, F32).reshape(-1).astype(np.float64)
    d = np.asarray(rays, F32)[:, 3:6].astype(np.float64)
    dn = np.sqrt((d * d).sum(1))
    with np.errstate(invalid="ignore"):
        C = np.cumsum(w64, axis=1)
    depth, index, flagged = [], [], []
    rows = np.arange(w64.shape[0])
    for qk in q:
        qk = float(F32(qk))
        dk, ik = _finish(C, w64, z64, dn, qk, np.float64)
        with np.errstate(invalid="ignore"):
            near = (np.abs(C - qk) < FLAG_C).any(1)
            thin = (ik >= 0) & (w64[rows, np.maximum(ik, 0)] < FLAG_W)
        depth.append(dk), index.append(ik), flagged.append(near | thin)
    return np.stack(depth), np.stack(index), np.stack(flagged)


def bound(e, z, rays):
    """[R]: max(4 e, 1e-6 max z / dn) -- the same fp32 arithmetic in another summation order (e: sequential fp32 against
    fp64), and never below an ulp-scale share of the largest depth the ray can return."""
    return np.maximum(4.0 * e, 1e-6 * float(np.max(z)) / ray_norm32(rays).astype(np.float64))


def compare(label, w, z, rays, q, depth, index):
    """depth / index [K,R] of an implementation against the fp64 oracle on the same weights; prints the figures, asserts the
    cap, the index and the bound.  -> flagged count."""
    d64, i64, flagged = oracle64(w, z, rays, q)
    dseq, _ = restate(w, z, rays, q, scan="sequential")
    keep = ~flagged
    n_flag, n = int(flagged.sum()), flagged.size
    e = float(np.abs(dseq.astype(np.float64) - d64)[keep].max()) if keep.any() else 0.0
    bnd = np.broadcast_to(bound(e, z, rays)[None], d64.shape)
    err = np.abs(depth.astype(np.float64) - d64)
    worst = float(err[keep].max()) if keep.any() else 0.0
    print(f"{label}: R {w.shape[0]} S {w.shape[1]} K {len(q)} flagged {n_flag} of {n}, found {int((i64 >= 0).sum())}, e = {e:.3e}, "
          f"error {worst:.3e}, bound min {float(bnd.min()):.3e} max {float(bnd.max()):.3e}")
    assert n_flag <= MAX_FLAGGED * n, (n_flag, n)
    assert np.array_equal(index[keep], i64[keep])
    assert (err[keep] <= bnd[keep]).all(), float((err - bnd)[keep].max())
    return n_flag


def composite(alpha):
    """alpha [R,S] -> w = alpha T, T the exclusive product of (1 - alpha), in fp32 (the forced last sample: alpha = 1)."""
    alpha = np.asarray(alpha, F32).copy()
    alpha[:, -1] = 1
    T = np.cumprod(np.concatenate([np.ones_like(alpha[:, :1]), F32(1) - alpha], 1), axis=1, dtype=F32)
    return (alpha * T[:, :-1]).astype(F32)


def synthetic(R, S, seed):
    """Random alphas composited: per ray a density scale between "crosses in its first samples" and "never before the forced
    last sample", so crossings land everywhere in the schedule.  -> (w [R,S], z [S], rays [R,6])."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2.5, 0.0, (R, 1))
    alpha = (rng.random((R, S)) ** 2 * scale).astype(F32)
    alpha[rng.random((R, S)) < 0.3] = 0                                 # empty stretches
    z = np.sort(rng.uniform(0.1, 6.0, S)).astype(F32)
    rays = np.concatenate([0.2 * rng.normal(size=(R, 3)), rng.normal(size=(R, 3))], 1).astype(F32)
    return composite(alpha), z, rays


def adversarial(S):
    """Rows that force the crossing of q = 0.5 where the scan can go wrong -> (w [n,S], labels).  Expectations for q = 0.5:
    "at j": the whole weight 0.75 in sample j -> index j; "tie j": 0.25 in samples j - 1 and j (or 0.5 in sample 0) -> C_j ==
    0.5 exactly in any summation order -> index j; "zero" and "sub" (acc = 0.3) -> (0, -1); "nan j": a NaN at j before 0.75
    at j + 1 -> (0, -1); "late nan": 0.75 at 0 then NaN -> index 0 for q <= 0.75, (0, -1) above."""
    spots = sorted({j for j in (0, 63, 64, S - 1) if j < S})
    rows, labels = [], []
    for j in spots:
        r = np.zeros(S, F32)
        r[j] = 0.75
        rows.append(r), labels.append(("at", j))
        r = np.zeros(S, F32)
        if j == 0:
            r[0] = 0.5
        else:
            r[j - 1] = r[j] = 0.25
        rows.append(r), labels.append(("tie", j))
        if j + 1 < S:
            r = np.zeros(S, F32)
            r[j], r[j + 1] = np.nan, 0.75
            rows.append(r), labels.append(("nan", j))
    rows.append(np.zeros(S, F32)), labels.append(("zero", -1))
    r = np.zeros(S, F32)
    r[S // 2] = 0.3
    rows.append(r), labels.append(("sub", -1))
    r = np.zeros(S, F32)
    r[0], r[1] = 0.75, np.nan
    rows.append(r), labels.append(("late nan", 0))
    return np.stack(rows), labels


def oracle_weights(f, rays, N_samples=-1, floater_thresh=0.0):
    """The per-sample weights of field f (no alpha mask) on the CPU in fp32, from the pieces of oracle/vm_render_torch.py in
    render_field's order (:118-146) -> (w [R,S], z [S]) numpy."""
    from normals_cases import field_dict
    fld = field_dict(f, torch.float32)
    n = N_samples if N_samples > 0 else f.nSamples
    z = O.z_schedule(n).float()
    rays = rays.detach().cpu().float()
    o, d = rays[:, :3], rays[:, 3:6]
    dh = d / torch.norm(d, dim=-1, keepdim=True)
    x = o[:, None, :] + dh[:, None, :] * z[..., None]
    m = x.abs().amax(dim=-1, keepdim=True).clamp(min=1e-6)
    x = torch.where(m <= 1, x, ((2 * m - 1) / (m ** 2)) * x)
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
    aabb = fld["aabb"]
    u = (x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1
    df = O.density_feature(fld, u.reshape(-1, 3)).view(x.shape[:2])
    sigma = torch.nn.functional.softplus(df + float(f.density_shift)) if f.fea2denseAct == "softplus" else torch.relu(df)
    sigma[:, -1] = 0
    alpha = 1.0 - torch.exp(-sigma * dists * float(f.distance_scale))
    w = O.alpha2weights(alpha)
    if floater_thresh > 0:
        k = torch.arange(alpha.shape[1])[None]
        idx = (w * k).sum(-1, keepdim=True)
        alpha[k < idx * floater_thresh] = 0
        w = O.alpha2weights(alpha)
    return w.numpy().astype(F32), z.view(-1).numpy().astype(F32)


FIELD_CASES = ("softplus", "relu", "alpha_mask", "floater", "three_steps", "one_ray")


def case_field(case, device):
    """The field, rays, floater threshold and sample count of a case of the normals tests (tests/test_gpu_normals.py);
    alpha_mask's mask is left to the caller: building it needs the GPU."""
    from normals_cases import field, test_rays
    rays = test_rays(200, 31)
    over = {"fea2denseAct": "relu"} if case in ("relu", "three_steps") else {"alphaMask_thres": 1e-3} if case == "alpha_mask" else {}
    f = field(device, 11, **over)
    if case == "three_steps":
        with torch.no_grad():
            for p in f.density_plane:
                p.mul_(5.0)
        f.layout.invalidate()
    if case == "one_ray":
        rays = rays[17:18]
    return f, rays, 0.5 if case == "floater" else 0.0, 420 if case == "three_steps" else -1
