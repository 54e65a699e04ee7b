"""Shared host restatements for the geometry-diagnostics tests: numpy's linear quantile of a float32 array written out
from numpy 2.2's source, and renderer.py:79-124 written out in torch / numpy on the CPU, plus the golden's views."""
import numpy as np
import torch

from util import load_golden


def np_quantile_f32(a, q):
    """np.quantile(a, q) of a float32 array, method="linear", step by step as numpy/lib/_function_base_impl.py forms it:
    q rounded to float32 (quantile() casts a Python float to the array's dtype); _compute_virtual_index (n - 1) * q in
    float32; _get_indexes: floor, and for v >= n - 1 both neighbours become the last element with prev = -1; _get_gamma
    v - prev, rounded back to float32; _lerp a + d t, or b - d (1 - t) where t >= 0.5, in float32 and unfused; a NaN
    anywhere gives NaN."""
    a = np.asarray(a, np.float32).reshape(-1)
    n = a.size
    q32 = np.float32(q)
    if np.isnan(a).any():
        return np.float32(np.nan)
    v = np.float32(np.float32(n - 1) * q32)
    if v >= np.float32(n - 1):
        lo = hi = n - 1
        prev = -1.0
    else:
        prev = float(np.floor(v))
        lo = int(prev)
        hi = lo + 1
    t = np.float32(np.float64(v) - prev)
    part = np.partition(a, (lo, hi)) if hi != lo else np.partition(a, lo)
    x0, x1 = part[lo], part[hi]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(x1 - x0)
        if t >= np.float32(0.5):
            return np.float32(x1 - np.float32(d * np.float32(np.float32(1.0) - t)))
        return np.float32(x0 + np.float32(d * t))


def golden_views():
    """(shared, [per-view dicts]) of tests/golden/eval_geometry.npz."""
    g = load_golden("eval_geometry")
    views = []
    for k in range(int(g["views"])):
        p = f"v{k}."
        views.append({key[len(p):]: val for key, val in g.items() if key.startswith(p)})
    return g, views


def pred_flow_host(cam2world, idx, depth, dirs, ij, focal, center, offset):
    """utils.py:15-48 in torch on the CPU, the reference's operations: cam2cam = inverse_pose(c2w[clamp(idx + offset)]) . c2w[idx],
    bmm, pts2px.  Returns [HW, 2] float32 numpy."""
    c2w = torch.as_tensor(np.asarray(cam2world, np.float32))
    ids = torch.tensor([int(idx)])
    nb = torch.clamp(ids + offset, 0, len(c2w) - 1)
    pose = c2w[nb]
    inv = torch.zeros_like(pose)
    inv[:, :3, :3] = pose[:, :3, :3].transpose(1, 2)
    inv[:, :3, 3] = -torch.bmm(inv[:, :3, :3].clone(), pose[:, :3, 3:])[..., 0]
    cc = torch.zeros_like(inv)
    cc[:, :3, :3] = torch.bmm(inv[:, :3, :3], c2w[ids, :3, :3])
    cc[:, :3, 3] = torch.bmm(inv[:, :3, :3], c2w[ids, :3, 3:])[..., 0] + inv[:, :3, 3]
    pts = torch.as_tensor(dirs)[None] * torch.as_tensor(depth)[None, ..., None]
    new = torch.bmm(cc[:, :3, :3], pts.transpose(1, 2)).transpose(1, 2) + cc[:, None, :3, 3]
    new[..., 1] = -new[..., 1]
    new[..., 2] = -new[..., 2]
    new[..., 2] = torch.clip(new[..., 2], min=1e-6)
    f = float(np.float32(focal))
    c = torch.as_tensor(np.asarray(center, np.float32))
    px = torch.stack([new[..., 0] / new[..., 2] * f + c[0] - 0.5, new[..., 1] / new[..., 2] * f + c[1] - 0.5], -1)
    return (px - torch.as_tensor(np.asarray(ij)).float())[0].numpy()


def flow_images_host(pred, flow, mask, W, H, quantile=None):
    """renderer.py:91-104 for one direction: (image [3H, 2W] after clamp, raw image, the two quantiles)."""
    quantile = quantile or (lambda a: np.quantile(a, 0.9))
    pred = pred.reshape(H, W, 2)
    flow = np.asarray(flow, np.float32).reshape(H, W, 2)
    mask = np.asarray(mask, np.float32).reshape(H, W)
    halves, raws, qs = [], [], []
    for c in range(2):
        cmp = np.vstack([pred[..., c], flow[..., c]])
        raw = np.vstack([cmp, np.abs(pred[..., c] - flow[..., c]) * mask / W])
        qv = quantile(cmp)
        cmp = cmp / qv
        err = np.abs(pred[..., c] - flow[..., c]) * mask / W
        halves.append(np.vstack([cmp, err]))
        raws.append(raw)
        qs.append(np.float32(qv))
    img = torch.from_numpy(np.hstack(halves)).clamp(0, 1).numpy()
    return img, np.hstack(raws), qs


def depth_image_host(depth, invdepth, W, H):
    """renderer.py:117-124 with compute_depth_loss (utils.py:50-59), in fp32 torch; the MADs as fp64 means rounded to fp32."""
    x = 1 / torch.as_tensor(np.asarray(depth, np.float32))[None].clamp(1e-6)
    y = torch.as_tensor(np.asarray(invdepth, np.float32)).reshape(1, -1)

    def norm(z):
        t = torch.median(z, dim=-1, keepdim=True).values
        s = torch.abs(z - t).double().mean(dim=-1, keepdim=True).float()
        return (z - t) / s, t, s
    xn, tx, sx = norm(x)
    yn, ty, sy = norm(y)
    img = torch.vstack([0.5 * xn[0].reshape(H, W), 0.5 * yn[0].reshape(H, W), ((xn - yn) ** 2)[0].reshape(H, W)]).clamp(0, 1)
    return img.numpy(), np.array([tx.item(), ty.item(), sx.item(), sy.item()], np.float32)
