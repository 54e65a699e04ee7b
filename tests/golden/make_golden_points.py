"""Generate tests/golden/points.npz: camera points, world points and reprojected pixel coordinates of 5 frames of 24 x 32
pixels from the reference's own get_ray_directions_lean (utils/ray_utils.py:14-24), inverse_pose, get_cam2cams and
get_pred_flow / pts2px (utils/utils.py:15-48).  Runs only where the reference tree is present (make_golden.import_reference);
the file it writes is what travels.
Usage:  python tests/golden/make_golden_points.py

Stored: depth [V,H,W], c2w [V,3,4], focal, center [2]; dirs [HW,3]; cam_pts [V,HW,3] = directions * depth; world_pts [V,HW,3]
= R pts + t, formed as get_pred_flow forms its points (bmm, then + t); per offset o in (-2, -1, 1, 2): "px{o}" [V,HW,2], the
pixel coordinates get_pred_flow(pts, ij = 0, get_cam2cams(c2w, indices, o)) returns, and "valid{o}" [V], whether v + o stayed
inside the trajectory (get_cam2cams clamps the index; the clamped rows are recorded but not valid).  Every point of the scene
lies in front of every camera, so pts2px's clip at 1e-6 never acts.
The same functions are also run in fp64 on the same fp32 inputs; noise_world and noise_px are the largest differences
between the reference's fp32 results and that fp64 evaluation: the measured rounding noise of the formulas, from which the
test's bars derive.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

V, H, W = 5, 24, 32
OFFSETS = (-2, -1, 1, 2)


def scene():
    rng = np.random.default_rng(11)
    c2w = np.zeros((V, 3, 4))
    for k in range(V):
        a, b = 0.05 * (k - 2), 0.02 * (k - 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        c2w[k, :, :3] = Ry @ Rx
        c2w[k, :, 3] = [0.2 * (k - 2), 0.03 * k, 0.05 * np.sin(k)]
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([3.0 + 0.6 * np.sin(0.2 * ii + k) * np.cos(0.15 * jj) + 0.05 * rng.normal(size=(H, W)) for k in range(V)])
    return depth.astype(np.float32), c2w.astype(np.float32), np.float32(30.0), np.array([W / 2 + 0.3, H / 2 - 0.2], np.float32)


def run(depth, c2w, focal, center, fns):
    get_dirs, get_cam2cams, get_pred_flow = fns
    ids = torch.arange(H * W)
    i, j = ids % W, ids // W
    dirs = get_dirs(i, j, focal, center)                              # [HW,3]
    pts = dirs[None] * depth.reshape(V, -1, 1)                        # utils.py: pts = directions * depth
    world = torch.transpose(torch.bmm(c2w[:, :3, :3], torch.transpose(pts, 1, 2)), 1, 2) + c2w[:, None, :3, 3]
    out = {"dirs": dirs, "cam_pts": pts, "world_pts": world}
    indices = torch.arange(V)
    ij0 = torch.zeros(V, H * W, 2)
    for o in OFFSETS:
        cam2cams = get_cam2cams(c2w, indices, o)
        out[f"px{o}"] = get_pred_flow(pts.clone(), ij0, cam2cams, focal, center)
    return out


def main():
    make_golden.import_reference()
    from utils.ray_utils import get_ray_directions_lean
    from utils.utils import get_cam2cams, get_pred_flow
    fns = (get_ray_directions_lean, get_cam2cams, get_pred_flow)
    depth, c2w, focal, center = scene()
    t = torch.from_numpy
    with torch.no_grad():
        r32 = run(t(depth), t(c2w), torch.tensor(focal), t(center), fns)
        # get_ray_directions_lean casts the pixel indices to fp32 (i.float()), which keeps its quotient in fp32 whatever the
        # intrinsics' type: the fp64 run evaluates the same expression on fp64 indices instead
        def dirs64(i, j, focal, center):
            i, j = i.double() + 0.5, j.double() + 0.5
            return torch.stack([(i - center[0]) / focal, -(j - center[1]) / focal, -torch.ones_like(i)], -1)
        r64 = run(t(depth).double(), t(c2w).double(), torch.tensor(focal).double(), t(center).double(), (dirs64,) + fns[1:])
    rec = {"depth": depth, "c2w": c2w, "focal": focal, "center": center, "offsets": np.array(OFFSETS, np.int64)}
    for k, v in r32.items():
        assert v.dtype == torch.float32, (k, v.dtype)
        rec[k] = v.numpy()
    assert all(v.dtype == torch.float64 for v in r64.values())
    valid = {o: np.array([0 <= v + o < V for v in range(V)]) for o in OFFSETS}
    for o in OFFSETS:
        rec[f"valid{o}"] = valid[o]
    rec["noise_world"] = np.float64(np.abs(r32["world_pts"].double() - r64["world_pts"]).max())
    rec["noise_px"] = np.float64(max(np.abs(r32[f"px{o}"].double() - r64[f"px{o}"]).numpy()[valid[o]].max() for o in OFFSETS))
    rec["meta"] = np.array(f"reference get_ray_directions_lean, get_cam2cams, get_pred_flow; numpy {np.__version__}; "
                           f"torch {torch.__version__}")
    print("noise_world", rec["noise_world"], "noise_px", rec["noise_px"], "max |world|", float(np.abs(rec["world_pts"]).max()))
    path = os.path.join(HERE, "points.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
