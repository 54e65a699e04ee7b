"""Geometry diagnostics (localrf_amd.diagnostics, lrf_select / lrf_flow_comparison / lrf_depth_comparison) without a GPU:
numpy's float32 linear quantile restated from its source and pinned bit for bit against np.quantile, the diagnostics
restated on the host and pinned against the reference's recorded images (tests/golden/eval_geometry.npz), the exported
symbols, and the refusals that happen before anything reaches the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, diagnostics
from localrf_amd import _native as N
from geometry_cases import depth_image_host, flow_images_host, golden_views, np_quantile_f32, pred_flow_host

QS = [0.0, 0.5, 0.8, 0.9, 1.0]


def _same(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def _arrays(rng):
    """(name, float32 array): n = 1, 2, 3, odd and even sizes up to ~1e6, duplicates, +-inf, mixed magnitudes."""
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 100, 101, 255, 256, 1000, 1001, 4095, 4096, 65537]
    for n in sizes:
        for kind in range(12):
            a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4)).astype(np.float32)
            if kind % 4 == 1:
                a = rng.integers(-3, 4, n).astype(np.float32)            # many duplicates
            elif kind % 4 == 2:
                a[rng.integers(0, n, max(1, n // 7))] = np.inf
                a[rng.integers(0, n, max(1, n // 9))] = -np.inf
            elif kind % 4 == 3:
                a = np.abs(a)
            yield f"n{n}.k{kind}", a
    for n in (524288, 1000001):
        yield f"n{n}", rng.standard_normal(n).astype(np.float32)


def test_quantile_restatement_equals_numpy_bit_for_bit():
    rng = np.random.default_rng(2024)
    count = 0
    for name, a in _arrays(rng):
        for q in QS:
            with np.errstate(invalid="ignore"):
                want = np.quantile(a, q)
            assert want.dtype == np.float32
            got = np_quantile_f32(a, q)
            assert _same(got, want), (name, q, got, want)
            count += 1
    assert count >= 1000, count


def test_quantile_restatement_special_rows():
    for q in QS:
        for a in ([np.nan], [1.0, np.nan, 2.0], [np.inf], [-np.inf, np.inf], [1.0, np.inf], [0.0, 0.0, 0.0], [5.0], [2.0, 7.0]):
            a = np.asarray(a, np.float32)
            with np.errstate(invalid="ignore"):
                want = np.quantile(a, q)
            assert _same(np_quantile_f32(a, q), want), (a, q)
    assert np.isnan(np_quantile_f32(np.array([1, 2, np.nan], np.float32), 0.5))
    z = np_quantile_f32(np.zeros(9, np.float32), 0.9)
    assert z.view(np.uint32) == 0                                      # an all-+0 row gives +0


def test_numpy_gamma_is_rounded_to_float32():
    """The finding that motivates the restatement: for n = 3, q = 0.9 numpy's gamma is 0.79999995."""
    v = np.float32(np.float32(2) * np.float32(0.9))
    assert np.float32(v - np.float32(1)) == np.float32(0.79999995)
    a = np.array([0.0, 1.0, 3.0], np.float32)
    assert _same(np_quantile_f32(a, 0.9), np.quantile(a, 0.9))


def test_golden_holds_three_views_with_the_last_frame():
    g, views = golden_views()
    F = g["cam2world"].shape[0]
    assert len(views) == 3 and int(views[-1]["idx"]) == F - 1
    W, H = int(g["W"]), int(g["H"])
    for v in views:
        assert v["fwd_cmp"].shape == (3 * H, 2 * W) and v["depth_cmp"].shape == (3 * H, W)


def test_flow_restatement_reproduces_the_reference_images():
    g, views = golden_views()
    W, H = int(g["W"]), int(g["H"])
    for v in views:
        for offset, key in ((1, "fwd"), (-1, "bwd")):
            pred = pred_flow_host(g["cam2world"], v["idx"], v["depth"], v["dirs"], v["ij"], g["focal"], g["center"], offset)
            img, _, _ = flow_images_host(pred, v[key + "_flow"], v[key + "_mask"], W, H)
            np.testing.assert_array_equal(img, v[key + "_cmp"])           # numpy's own quantile: exact
            img2, _, _ = flow_images_host(pred, v[key + "_flow"], v[key + "_mask"], W, H, lambda a: np_quantile_f32(a, 0.9))
            np.testing.assert_array_equal(img2, v[key + "_cmp"])


def test_depth_restatement_reproduces_the_reference_image():
    g, views = golden_views()
    W, H = int(g["W"]), int(g["H"])
    for v in views:
        img, _ = depth_image_host(v["depth"], v["invdepth"], W, H)
        assert np.abs(img - v["depth_cmp"]).max() <= 1e-6


def test_new_symbols_are_exported():
    lib = N.lib()
    for name in ("lrf_select", "lrf_select_workspace_bytes", "lrf_flow_comparison", "lrf_flow_comparison_workspace_bytes",
                 "lrf_depth_comparison", "lrf_depth_comparison_workspace_bytes"):
        assert hasattr(lib, name)
    assert lib.lrf_abi_version() == 7


def test_workspace_sizes_refuse_bad_shapes():
    lib = N.lib()
    assert lib.lrf_select_workspace_bytes(4, 1 << 22) > 0
    assert lib.lrf_select_workspace_bytes(0, 10) == 0
    assert lib.lrf_select_workspace_bytes(65536, 10) == 0
    assert lib.lrf_select_workspace_bytes(1, 0) == 0
    assert lib.lrf_select_workspace_bytes(1, 1 << 31) == 0
    assert lib.lrf_select_workspace_bytes(1, (1 << 31) - 1) > 0
    assert lib.lrf_flow_comparison_workspace_bytes(3, 270, 480) > 0
    assert lib.lrf_flow_comparison_workspace_bytes(0, 270, 480) == 0
    assert lib.lrf_flow_comparison_workspace_bytes(N.LRF_EVAL_MAX_VIEWS + 1, 270, 480) == 0
    assert lib.lrf_flow_comparison_workspace_bytes(1, 0, 480) == 0
    assert lib.lrf_flow_comparison_workspace_bytes(1, 1 << 16, 1 << 16) == 0
    assert lib.lrf_depth_comparison_workspace_bytes(3, 270, 480) > 0
    assert lib.lrf_depth_comparison_workspace_bytes(0, 270, 480) == 0
    assert lib.lrf_depth_comparison_workspace_bytes(1, 48, -1) == 0


def test_c_abi_refuses_before_launch():
    """Refused calls return an error before touching the (bogus, never dereferenced) device pointers."""
    lib = N.lib()
    bogus = C.c_void_p(16)
    one = (C.c_int64 * 1)(0)
    assert lib.lrf_select(bogus, 0, one, 1, 1, N.LRF_SELECT_MEDIAN, 0.0, bogus, bogus, None) != 0
    assert b"1 <= n < 2^31" in lib.lrf_last_error()
    big = (C.c_int64 * 1)(1 << 31)
    assert lib.lrf_select(bogus, 0, big, 1, 1, N.LRF_SELECT_MEDIAN, 0.0, bogus, bogus, None) != 0
    ok = (C.c_int64 * 1)(8)
    assert lib.lrf_select(bogus, 8, ok, 1, 1, N.LRF_SELECT_QUANTILE, 1.5, bogus, bogus, None) != 0
    assert lib.lrf_select(None, 8, ok, 1, 1, N.LRF_SELECT_MEDIAN, 0.0, bogus, bogus, None) != 0
    a = N.LrfFlowComparison()
    for f in ("cam2world", "depth", "dirs", "ij", "fwd_flow", "fwd_mask", "bwd_flow", "bwd_mask", "focal", "center"):
        setattr(a, f, 16)
    a.F, a.V, a.H, a.W = 5, 2, 4, 4
    a.idx[0], a.idx[1] = 0, 5
    assert lib.lrf_flow_comparison(C.byref(a), bogus, bogus, None, None, bogus, bogus, None) != 0
    assert b"outside [0, F)" in lib.lrf_last_error()
    assert lib.lrf_depth_comparison(bogus, None, 1, 4, 4, bogus, bogus, bogus, None) != 0


def test_python_refuses_cpu_tensors_and_bad_arguments():
    with pytest.raises(NativeError):
        diagnostics.quantile(torch.zeros(4, 5), 0.9)
    with pytest.raises(NativeError):
        diagnostics.median(torch.zeros(5))
    with pytest.raises(ValueError):
        diagnostics.quantile(torch.zeros(5), 1.5)
    g, views = golden_views()
    v = views[0]
    W, H = int(g["W"]), int(g["H"])
    t = {k: torch.from_numpy(np.asarray(x)) for k, x in v.items()}
    with pytest.raises(NativeError):
        diagnostics.flow_comparison(t["depth"], t["dirs"], t["ij"], torch.from_numpy(g["cam2world"]), int(v["idx"]), g["focal"],
                                    torch.from_numpy(g["center"]), t["fwd_flow"], t["fwd_mask"], t["bwd_flow"], t["bwd_mask"], W, H)
    with pytest.raises(NativeError):
        diagnostics.depth_comparison(t["depth"], t["invdepth"], W, H)
