"""Generate tests/golden/eval_metrics.npz: the reference's own test-view metrics (renderer.py:162-163) on fixed image
pairs -- utils.utils.rgb_ssim (scipy, fp64) and the renderer's fp32 torch MSE.  Runs only where the reference tree is
present (make_golden.import_reference); the file it writes is what travels.
Usage:  python tests/golden/make_golden_metrics.py

The images are not stored: tests/metrics_cases.py regenerates them bit for bit from integer arithmetic.  Case k is
stored as  k.digest0, k.digest1 (SHA-256 of the fp32 images' bytes), k.args (max_val, filter_size, filter_sigma, k1,
k2), k.ssim (fp64 scalar), k.mse32 (the fp32 torch value), k.mse64 (fp64 numpy) and, when recorded, k.map (the fp64
map's rows k.map_rows).  `names` lists the cases in order.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from metrics_cases import cases, digest  # noqa: E402


def main():
    make_golden.import_reference()
    from utils.utils import rgb_ssim                    # the reference's own function (scipy.signal.convolve2d, fp64)
    rec = {"names": []}
    for name, a, b, kw, map_step in cases():
        args = dict(max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03)
        args.update(kw)
        gt, rgb = torch.from_numpy(a), torch.from_numpy(b)          # renderer.py:158-163: rgb_ssim(gt, rgb, 1)
        ssim = rgb_ssim(gt.numpy(), rgb.numpy(), args["max_val"], args["filter_size"], args["filter_sigma"],
                        args["k1"], args["k2"])
        rec["names"].append(name)
        rec[name + ".digest0"], rec[name + ".digest1"] = np.array(digest(a)), np.array(digest(b))
        rec[name + ".args"] = np.array([args["max_val"], args["filter_size"], args["filter_sigma"], args["k1"], args["k2"]])
        rec[name + ".ssim"] = np.float64(ssim)
        if map_step is not None:                         # every map_step-th row: the full 118 x 150 map is 425 KB of fp64
            m = rgb_ssim(gt.numpy(), rgb.numpy(), args["max_val"], args["filter_size"], args["filter_sigma"],
                         args["k1"], args["k2"], return_map=True)
            rows = np.arange(0, m.shape[0], map_step)
            rec[name + ".map_rows"], rec[name + ".map"] = rows, np.ascontiguousarray(m[rows])
        rec[name + ".mse32"] = np.float32(((gt - rgb) ** 2).mean().item())
        rec[name + ".mse64"] = np.float64(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
        print(f"{name:28s} ssim={float(ssim):.15f} mse={float(rec[name + '.mse32']):.6e}")
    rec["names"] = np.array(rec["names"])
    rec["meta"] = np.array(f"reference utils.utils.rgb_ssim; numpy {np.__version__}; torch {torch.__version__}")
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **rec)


if __name__ == "__main__":
    main()
