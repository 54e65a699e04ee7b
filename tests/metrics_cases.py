"""The image pairs of tests/golden/eval_metrics.npz, regenerated bit for bit instead of stored.

Every image is fp32 k * 2^-16 with integer k < 2^16, so it is exact; k comes from integer arithmetic only (a splitmix64
hash for the noise, triangle waves for the smooth images), never from numpy's random streams or transcendental functions,
so any numpy on any host produces the same bytes.  The golden records a SHA-256 of each image and the tests check it.
"""
import hashlib

import numpy as np

Q = np.float32(2.0 ** -16)


def _hash_u16(n, seed):
    z = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) % 2 ** 64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return (z >> np.uint64(48)).astype(np.int64)                      # uniform integers in [0, 65536)


def _img(k):
    return (np.clip(k, 0, 65535).astype(np.float32) * Q).astype(np.float32)


def uniform(h, w, seed):
    return _img(_hash_u16(h * w * 3, seed).reshape(h, w, 3))


def noise(h, w, seed, amp):
    """Roughly Gaussian integer noise: four uniforms summed and centred, scaled by amp / 65536 (spread ~ 0.58 amp)."""
    s = sum(_hash_u16(h * w * 3, seed * 4 + j) for j in range(4)) - 2 * 65535
    return ((s * amp) // 65536).reshape(h, w, 3)


def smooth_k(h, w):
    """A smooth three-channel pattern of triangle waves, integer-valued in [8000, 56000]."""
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    ch = []
    for c, (a, b, p) in enumerate(((3, 2, 97), (1, 4, 131), (5, 1, 71))):
        t = (a * y + b * x + 17 * c) % (2 * p)
        ch.append(8000 + (48000 * np.abs(t - p)) // p)
    return np.stack(ch, -1)


def cases():
    """[(name, img0, img1, rgb_ssim keyword arguments, map rows to record: None, or a row step)]"""
    out = []
    out.append(("random_37x53", uniform(37, 53, 1), uniform(37, 53, 2), {}, None))
    a = uniform(61, 90, 3)
    out.append(("random_61x90", a, _img(np.round(a / Q).astype(np.int64) + noise(61, 90, 4, 13000)), {}, None))
    sk = smooth_k(128, 160)
    smooth, noisy = _img(sk), _img(sk + noise(128, 160, 5, 3300))
    out.append(("smooth_noise_128x160_map", smooth, noisy, {}, 3))
    out.append(("identical_45x40", a[:45, :40].copy(), a[:45, :40].copy(), {}, None))
    c0 = np.full((33, 29, 3), 0.25, np.float32)
    c1 = np.full((33, 29, 3), 0.75, np.float32)
    out.append(("constant_33x29", c0, c1, {}, 1))
    out.append(("constant_same_20x24", c0[:20, :24].copy(), c0[:20, :24].copy(), {}, None))
    a, b = uniform(40, 50, 6), uniform(40, 50, 7)
    out.append(("fs7_40x50", a, b, {"filter_size": 7}, 1))
    out.append(("fs8_even_40x50", a, b, {"filter_size": 8}, 1))
    out.append(("fs31_70x64", noisy[:70, :64].copy(), smooth[:70, :64].copy(), {"filter_size": 31}, None))
    out.append(("sigma0.8_50x66", noisy[:50, :66].copy(), smooth[:50, :66].copy(), {"filter_sigma": 0.8}, None))
    a8 = np.round(smooth * 255).astype(np.float32)
    b8 = np.round(noisy * 255).astype(np.float32)
    out.append(("maxval255_128x160", a8, b8, {"max_val": 255.0}, None))
    a, b = uniform(30, 34, 8), uniform(30, 34, 9)
    a[12, 20, 1] = np.nan
    out.append(("nan_30x34", a, b, {}, 1))
    return out


def digest(img):
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()
