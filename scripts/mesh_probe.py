"""Timing of the TSDF fusion and the mesh extraction (csrc/lrf_mesh.inl) on synthetic frames: a 256^3 volume, 360 x 640 frames
of a camera circling a sphere in front of a wall.

  integrate  TsdfVolume.integrate for 16 and 64 frames in one call (one launch, no read-back)
  extract    TsdfVolume.extract with the capacities given (three launches, one read-back) and with None (a counting call first)
  torch      ONE frame of the same integration written as torch ops: the baseline a kernel-free implementation starts from

  python scripts/mesh_probe.py [--n 256] [--reps 5]
Prints one line per measurement: the median of --reps runs after one warm-up, timed with device events."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localrf_amd import mesh  # noqa: E402

DEV = "cuda:0"
H, W, FOCAL = 360, 640, 500.0


def frames(V):
    """V cameras on an arc around (0, 0, -3), looking at a sphere of radius 0.8 in front of the wall z = -4.5."""
    c2w = np.zeros((V, 3, 4), np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dirs = np.stack([(col + 0.5 - W / 2) / FOCAL, -(row + 0.5 - H / 2) / FOCAL, -np.ones_like(col)], -1)
    depth = np.zeros((V, H, W), np.float32)
    for k in range(V):
        a = 0.6 * (k / max(V - 1, 1) - 0.5)
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        o = np.array([0.0, 0.0, -3.0]) + R @ np.array([0.0, 0.0, 3.0])
        c2w[k, :, :3], c2w[k, :, 3] = R, o
        dw = dirs @ R.T
        oc = o - np.array([0.0, 0.0, -3.0])
        A, B, Cc = (dw * dw).sum(-1), 2 * (dw * oc).sum(-1), (oc * oc).sum() - 0.64
        disc = B * B - 4 * A * Cc
        t_s = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        t_w = (-4.5 - o[2]) / dw[..., 2]
        depth[k] = np.minimum(np.where(t_s > 0, t_s, np.inf), np.where(t_w > 0, t_w, np.inf))
    rgb8 = np.random.default_rng(0).integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    return torch.from_numpy(depth).to(DEV), torch.from_numpy(rgb8).to(DEV), torch.from_numpy(c2w.astype(np.float32)).to(DEV)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def torch_frame(vol, pts, depth, rgb8, c2w):
    """One frame of k_tsdf_integrate as torch ops (same formulas; every op reads and writes a volume-sized tensor)."""
    R, t = c2w[:, :3], c2w[:, 3]
    q = (pts - t) @ R
    nz = -q[..., 2]
    iu = torch.round(q[..., 0] / nz * FOCAL + W / 2 - 0.5).long()
    iw = torch.round(-q[..., 1] / nz * FOCAL + H / 2 - 0.5).long()
    ok = (nz > 0) & (iu >= 0) & (iu < W) & (iw >= 0) & (iw < H)
    iu, iw = iu.clamp(0, W - 1), iw.clamp(0, H - 1)
    dn = depth[iw, iu]
    sdf = dn - nz
    ok &= torch.isfinite(dn) & (dn > 0) & (sdf >= -vol.trunc)
    s = (sdf / vol.trunc).clamp(max=1.0)
    w1 = vol.weight + 1
    vol.tsdf.copy_(torch.where(ok, (vol.tsdf * vol.weight + s) / w1, vol.tsdf))
    c = rgb8[iw, iu].float() / 255
    vol.rgb.copy_(torch.where(ok[..., None], (vol.rgb * vol.weight[..., None] + c) / w1[..., None], vol.rgb))
    vol.weight.copy_(torch.where(ok, w1, vol.weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.n
    voxel = 3.4 / (n - 1)
    origin = (-1.7, -1.7, -4.7)
    print(f"device {torch.cuda.get_device_name(0)}, volume {n}^3, voxel {voxel:.5f}, trunc {3 * voxel:.5f}, frames {H} x {W}")
    vol = None
    for V in (16, 64):
        depth, rgb8, c2w = frames(V)
        vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
        ms = timed(lambda: vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8), a.reps)
        pairs = V * n ** 3
        print(f"integrate {V:3d} frames: {ms:8.3f} ms  ({pairs / ms / 1e6:.1f} G voxel-frame pairs / s)")
    vol = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    vol.integrate(depth, c2w, FOCAL, (W / 2, H / 2), rgb=rgb8)
    m = vol.extract()
    nv, nf = m["counts"]
    print(f"mesh: {nv} vertices, {nf} faces")
    print(f"extract, capacities given: {timed(lambda: vol.extract(max_vertices=nv, max_faces=nf), a.reps):8.3f} ms")
    print(f"extract, counting call first: {timed(lambda: vol.extract(), a.reps):8.3f} ms")
    ref = mesh.TsdfVolume(origin, voxel, (n, n, n), 3 * voxel, DEV)
    ax = [torch.arange(n, device=DEV, dtype=torch.float32) * voxel + o for o in origin]
    pts = torch.stack(torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")[::-1], -1)
    ms = timed(lambda: torch_frame(ref, pts, depth[0], rgb8[0], c2w[0]), a.reps)
    print(f"torch ops, ONE frame: {ms:8.3f} ms  ({n ** 3 / ms / 1e6:.2f} G voxel-frame pairs / s)")


if __name__ == "__main__":
    main()
