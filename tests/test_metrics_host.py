"""Test-view metrics (localrf_amd.metrics, lrf_image_metrics) without a GPU: a float64 restatement of the reference's
rgb_ssim (utils/utils.py:232-287) pinned to the reference-recorded goldens, the exported symbols, and the refusals that
happen before anything reaches the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, metrics
from util import load_golden


def ssim_host(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """rgb_ssim restated in numpy float64: the separable blur written out as shifted sums (convolve2d(mode="valid") with
    filt[:, None], then filt[None, :]); the squares and the product of the fp32 images formed in fp32, as numpy does."""
    img0, img1 = np.asarray(img0), np.asarray(img1)
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    filt = np.exp(-0.5 * ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2)
    filt /= np.sum(filt)
    fs = filter_size

    def blur(z):
        z = z.astype(np.float64)
        oh, ow = z.shape[0] - fs + 1, z.shape[1] - fs + 1
        t = sum(filt[fs - 1 - k] * z[k:k + oh] for k in range(fs))
        return sum(filt[fs - 1 - k] * t[:, k:k + ow] for k in range(fs))

    mu0, mu1 = blur(img0), blur(img1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0.0, blur(img0 * img0) - mu00)
    s11 = np.maximum(0.0, blur(img1 * img1) - mu11)
    s01 = blur(img0 * img1) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    m = (2 * mu01 + c1) * (2 * s01 + c2) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return m if return_map else np.mean(m)


def golden_cases():
    """[(name, img0, img1, rgb_ssim keyword arguments, golden)]: the golden's recorded values with the images
    tests/metrics_cases.py regenerates (checked byte for byte against the golden's digests)."""
    from metrics_cases import cases, digest
    g = load_golden("eval_metrics")
    out = []
    for name, a, b, _, _ in cases():
        assert digest(a) == str(g[name + ".digest0"]) and digest(b) == str(g[name + ".digest1"]), name
        mv, fs, sig, k1, k2 = [float(v) for v in g[name + ".args"]]
        out.append((name, a, b, dict(max_val=mv, filter_size=int(fs), filter_sigma=sig, k1=k1, k2=k2), g))
    assert [n for n, *_ in out] == [str(n) for n in g["names"]]
    return out


def recorded_map(g, name, m):
    """The rows of map m the golden recorded for case `name`."""
    return m[..., g[name + ".map_rows"], :, :]


def test_golden_covers_the_cases_the_issue_lists():
    cs = golden_cases()
    g = cs[0][4]
    args = {n: a for n, _, _, a, _ in cs}
    assert len(cs) >= 10
    assert {7, 8, 11, 31} <= {a["filter_size"] for a in args.values()}
    assert any(a["filter_sigma"] == 0.8 for a in args.values()) and any(a["max_val"] == 255 for a in args.values())
    assert any(np.isnan(g[n + ".ssim"]) for n in args)
    assert sum((n + ".map") in g for n in args) >= 3
    assert all(a.dtype == np.float32 and b.dtype == np.float32 for _, a, b, _, _ in cs)
    assert ("smooth_noise_128x160_map", (128, 160, 3)) in [(n, a.shape) for n, a, *_ in cs]


@pytest.mark.parametrize("case", [n for n, *_ in golden_cases()])
def test_host_restatement_reproduces_reference_golden(case):
    _, a, b, kw, g = next(c for c in golden_cases() if c[0] == case)
    want = float(g[case + ".ssim"])
    got = float(ssim_host(a, b, **kw))
    if np.isnan(want):
        assert np.isnan(got)
    else:
        assert abs(got - want) <= 1e-12, (got, want)
    if case + ".map" in g:
        m = recorded_map(g, case, ssim_host(a, b, return_map=True, **kw))
        ref = g[case + ".map"]
        assert m.shape == ref.shape
        assert (np.isnan(m) == np.isnan(ref)).all()
        ok = ~np.isnan(ref)
        assert np.abs(m[ok] - ref[ok]).max() <= 1e-12
    mse64 = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    assert np.array_equal(mse64, g[case + ".mse64"], equal_nan=True)
    mse32 = ((torch.from_numpy(a) - torch.from_numpy(b)) ** 2).mean().item()
    assert np.array_equal(np.float32(mse32), g[case + ".mse32"], equal_nan=True)


def test_library_exports_image_metrics(built_lib):
    assert hasattr(built_lib, "lrf_image_metrics") and hasattr(built_lib, "lrf_image_metrics_workspace_bytes")
    ws = built_lib.lrf_image_metrics_workspace_bytes
    one = ws(1, 540, 960, 11)
    assert one > 0 and ws(8, 540, 960, 11) == 8 * one
    assert ws(1, 540, 960, 32) == 0 and ws(1, 540, 960, 0) == 0       # filter_size outside 1..31
    assert ws(1, 10, 960, 11) == 0 and ws(1, 540, 10, 11) == 0         # H or W below filter_size
    assert ws(0, 540, 960, 11) == 0


def test_c_abi_refuses_bad_arguments_before_any_launch(built_lib):
    from localrf_amd import _native as N

    def call(**kw):
        a = N.LrfImageMetrics()
        a.B, a.H, a.W, a.filter_size = kw.get("B", 1), kw.get("H", 64), kw.get("W", 64), kw.get("fs", 11)
        a.max_val, a.filter_sigma, a.k1, a.k2 = 1.0, kw.get("sigma", 1.5), 0.01, 0.03
        # null device pointers: every shape refusal comes first, so nothing can reach a kernel
        rc = built_lib.lrf_image_metrics(C.byref(a), None, None, None, None, None)
        return rc, built_lib.lrf_last_error().decode()

    for kw, word in (({"fs": 32}, "filter_size"), ({"fs": 0}, "filter_size"), ({"H": 10}, "at least filter_size"),
                     ({"W": 10}, "at least filter_size"), ({"B": 0}, "B"), ({"sigma": 0.0}, "filter_sigma"),
                     ({}, "null argument")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_python_refuses_cpu_tensors_large_filters_and_small_images():
    x = torch.rand(2, 32, 40, 3)
    with pytest.raises(NativeError):
        metrics.image_metrics(x, x.clone())
    with pytest.raises(NativeError):
        metrics.rgb_ssim(x[0], x[0].clone(), 1.0)
    a = np.random.default_rng(0).random((40, 40, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="filter_size"):
        metrics.rgb_ssim(a, a, 1.0, filter_size=33)
    with pytest.raises(ValueError, match="smaller than filter_size"):
        metrics.rgb_ssim(a[:9], a[:9], 1.0)
    with pytest.raises(ValueError, match="smaller than filter_size"):
        metrics.image_metrics(x[:, :8], x[:, :8])
    with pytest.raises(ValueError, match="differ"):
        metrics.rgb_ssim(a, a[:, :39], 1.0)


def test_psnr_is_the_train_py_expression():
    mses = [0.01, 0.02, 0.005]
    assert metrics.psnr(mses) == -10.0 * np.log(np.array(mses).mean()) / np.log(10.0)
    assert metrics.psnr(torch.tensor(mses, dtype=torch.float64)) == metrics.psnr(mses)
