"""numpy restatements of the dataset arithmetic localrf_amd.frames reproduces, and frame data built from integer arithmetic
(no fixtures: the reference's utils / dataLoader modules import cv2, which the tests do not need).

  reference_sample     dataLoader/localrf_dataset.py:273-313 (sample), over concatenated all_X arrays
  decode_flow_scaled   utils/utils.py:67-71 (decode_flow) times flow_scale (localrf_dataset.py:193-194)
  grey_u8, laplacian   localrf_dataset.py:229-233: cv2.cvtColor((img * 255).astype(np.uint8), RGB2GRAY) and
                       cv2.Laplacian(., CV_32F) (ksize 1, BORDER_REFLECT_101), from OpenCV's documented constants
  sharpness_exact      the kernel's variance: exact integer moments, (N S2 - S1^2) / N^2 in fp64, rounded to fp32
"""
import random

import numpy as np


def reference_sample(test_mask, bounds, n_px, all_x, batch_size, is_refining, optimize_poses, n_views=16):
    """localrf_dataset.py:273-313 with its all_X arrays passed in ({name: [n_active * n_px, c]})."""
    active_test_mask = test_mask[bounds[0]:bounds[1]]
    test_ratio = active_test_mask.mean()
    if optimize_poses:
        train_test_poses = test_ratio > random.uniform(0, 1)
    else:
        train_test_poses = False
    inclusion_mask = active_test_mask if train_test_poses else 1 - active_test_mask
    sample_map = np.arange(bounds[0], bounds[1], dtype=np.int64)[inclusion_mask == 1]
    raw_samples = np.random.randint(0, inclusion_mask.sum(), n_views, dtype=np.int64)
    if not is_refining and inclusion_mask.sum() > 4:
        raw_samples[:2] = inclusion_mask.sum() - 1
        raw_samples[2:4] = inclusion_mask.sum() - 2
        raw_samples[4] = inclusion_mask.sum() - 3
        raw_samples[5] = inclusion_mask.sum() - 4
    view_ids = sample_map[raw_samples]
    idx = np.random.randint(0, n_px, batch_size, dtype=np.int64)
    idx = idx.reshape(n_views, -1)
    idx = idx + view_ids[..., None] * n_px
    idx = idx.reshape(-1)
    idx_sample = idx - bounds[0] * n_px
    out = {k: v[idx_sample] for k, v in all_x.items()}
    out.update(idx=idx, view_ids=view_ids, train_test_poses=train_test_poses)
    return out


def mask_of_fbases(fbases, test_frame_every):
    """localrf_dataset.py:81-90."""
    m = []
    for idx, fb in enumerate(fbases):
        index = int(fb) if fb.isnumeric() else idx
        m.append(1 if test_frame_every > 0 and index % test_frame_every == 0 else 0)
    return np.array(m)


def decode_flow_scaled(encoded, flow_scale):
    flow = encoded[..., :2].astype(np.float32)
    flow -= 2 ** 15
    flow /= 2 ** 8
    mask = (encoded[..., 2] > 2 ** 15).astype(np.float32)
    return flow * flow_scale, mask


def grey_u8(img):
    """OpenCV's COLOR_RGB2GRAY for 8-bit input: (4899 R + 9617 G + 1868 B + 8192) >> 14 (its documented fixed point)."""
    u = (img * np.float32(255)).astype(np.uint8).astype(np.int64)
    return (4899 * u[..., 0] + 9617 * u[..., 1] + 1868 * u[..., 2] + 8192) >> 14


def laplacian(g):
    """cv2.Laplacian(g, cv2.CV_32F), ksize 1: [[0,1,0],[1,-4,1],[0,1,0]], BORDER_REFLECT_101 (numpy's 'reflect')."""
    p = g
    for axis in (0, 1):
        n = g.shape[axis]
        p = np.take(p, [1 if n > 1 else 0] + list(range(n)) + [n - 2 if n > 1 else 0], axis=axis)
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * p[1:-1, 1:-1]


def sharpness_exact(img):
    lap = laplacian(grey_u8(img)).astype(np.int64)
    n = lap.size
    s1, s2 = int(lap.sum()), int((lap * lap).sum())
    return np.float32(np.float64(n * s2 - s1 * s1) / (np.float64(n) * np.float64(n)))


def sharpness_numpy_f32(img):
    """What the reference computes: the float32 Laplacian's .var()."""
    return laplacian(grey_u8(img)).astype(np.float32).var()


def make_frame(i, H, W, flow=True, depth=True, mask=True, encoded=True, flow_scale=1.0):
    """Frame i of a synthetic sequence from integer arithmetic: 8-bit colours k / 255, inverse depths, encoded flows that hit
    0, 32768, 32769 and 65535, validity channels on both sides of 2^15, a motion mask with holes."""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    k = (x * 37 + y * 91 + i * 53) % 256
    rgb = np.stack([k, (k * 7 + 11 * y) % 256, (k * 13 + 5 * x + i) % 256], -1)
    d = {"img": (rgb.astype(np.float32) / np.float32(255)).astype(np.float32)}
    if depth:
        d["invdepth"] = ((x + 3 * y + i) % 97 + 1).astype(np.float32) / np.float32(64)
    if flow:
        vals = np.array([0, 32768, 32769, 65535, 32767, 1, 40000, 25000], dtype=np.int64)
        e = np.stack([vals[(x + y + i) % 8], vals[(x * 3 + y + 2 * i) % 8], vals[(x * 5 + 7 * y + i) % 8]], -1).astype(np.uint16)
        e2 = np.stack([vals[(x * 2 + y + i) % 8], vals[(x + 5 * y) % 8], vals[(3 * x + y + i + 1) % 8]], -1).astype(np.uint16)
        if encoded:
            d.update(encoded_fwd_flow=e, encoded_bwd_flow=e2, flow_scale=flow_scale)
        else:
            f, m = decode_flow_scaled(e, flow_scale)
            b, n = decode_flow_scaled(e2, flow_scale)
            d.update(fwd_flow=f, fwd_mask=m, bwd_flow=b, bwd_mask=n)
    if mask:
        d["mask"] = ((x * 11 + y * 17 + i) % 9) != 0
    return d


def reference_all_x(frames):
    """concatenate_append of read_meta (localrf_dataset.py:225-263) for already-read frames: the all_X arrays."""
    out = {"rgbs": [], "loss_weights": [], "invdepths": [], "fwd_flow": [], "fwd_mask": [], "bwd_flow": [], "bwd_mask": []}
    for d in frames:
        img = d["img"]
        lap = np.ones_like(img[..., 0]) * sharpness_exact(img)
        out["loss_weights"].append((lap if d.get("mask") is None else lap * d["mask"]).reshape(-1, 1))
        out["rgbs"].append(img.reshape(-1, 3))
        if "invdepth" in d:
            out["invdepths"].append(d["invdepth"].reshape(-1, 1))
        if "encoded_fwd_flow" in d:
            f, m = decode_flow_scaled(d["encoded_fwd_flow"], d["flow_scale"])
            b, n = decode_flow_scaled(d["encoded_bwd_flow"], d["flow_scale"])
        elif "fwd_flow" in d:
            f, m, b, n = d["fwd_flow"], d["fwd_mask"], d["bwd_flow"], d["bwd_mask"]
        else:
            continue
        out["fwd_flow"].append(f.reshape(-1, 2)); out["fwd_mask"].append(m.reshape(-1, 1))
        out["bwd_flow"].append(b.reshape(-1, 2)); out["bwd_mask"].append(n.reshape(-1, 1))
    return {k: np.concatenate(v, 0) for k, v in out.items() if v}
