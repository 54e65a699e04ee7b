"""Test-view metrics on the MI355X (csrc/lrf_metrics.inl through localrf_amd.metrics): every golden case of the
reference's rgb_ssim and fp32 MSE (tests/golden/eval_metrics.npz), bit-reproducibility and independence of the batch,
the numpy drop-in, and test_view_metrics end to end on a blended LocalTensorfs against the reference-style host path."""
import numpy as np
import pytest
import torch

from localrf_amd import metrics
from test_metrics_host import golden_cases, recorded_map, ssim_host
from util import FIELD_KW, load_golden, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [n for n, *_ in golden_cases()]


def _case(case):
    return next(c for c in golden_cases() if c[0] == case)


def _close_or_nan(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    if ok.any():
        err = float(np.abs(got[ok] - want[ok]).max())
        assert err <= tol, err
    return got


@pytest.mark.parametrize("case", CASES)
def test_metrics_vs_reference_golden(case):
    _, a, b, kw, g = _case(case)
    a, b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    mse, ssim = metrics.image_metrics(b, a, **kw)               # (rgb, gt): renderer.py:162-163
    assert mse.dtype == torch.float64 and ssim.shape == (1,)
    _close_or_nan(ssim.cpu().numpy()[0], g[case + ".ssim"], 1e-9)
    want32, want64 = float(g[case + ".mse32"]), float(g[case + ".mse64"])
    got = float(mse.cpu()[0])
    if np.isnan(want64):
        assert np.isnan(got)
    else:
        assert abs(got - want32) <= 1e-6 * abs(want32) + 1e-12
        assert abs(got - want64) <= 1e-12 * abs(want64) + 1e-15
    if case + ".map" in g:
        m = metrics.rgb_ssim(a, b, return_map=True, **kw)
        assert m.dtype == torch.float64
        _close_or_nan(recorded_map(g, case, m.cpu().numpy()), g[case + ".map"], 1e-8)


def test_numpy_drop_in_returns_float64_equal_to_the_device_call():
    _, a, b, _, g = _case("smooth_noise_128x160_map")
    got = metrics.rgb_ssim(a, b, 1)                              # renderer.py:163 with rgb_ssim swapped
    assert type(got) is np.float64
    dev = metrics.rgb_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 1)
    assert dev.dim() == 0 and got == float(dev.cpu())
    m = metrics.rgb_ssim(a, b, 1, return_map=True)
    assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (118, 150, 3)
    dev_map = metrics.rgb_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 1, return_map=True)
    assert np.array_equal(m, dev_map.cpu().numpy())
    _close_or_nan(recorded_map(g, "smooth_noise_128x160_map", m), g["smooth_noise_128x160_map.map"], 1e-8)


def test_bit_reproducible_and_independent_of_the_batch():
    gen = torch.Generator().manual_seed(7)
    H, W = 203, 317                                              # neither a multiple of the tile
    base = torch.rand(H, W, 3, generator=gen)
    gt = torch.stack([base * s + o for s, o in ((1.0, 0.0), (0.5, 0.2), (0.9, 0.05), (0.3, 0.6), (0.7, 0.1))], 0)
    rgb = (gt + 0.08 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    gt, rgb = gt.to(DEV).contiguous(), rgb.to(DEV).contiguous()
    m1, s1 = metrics.image_metrics(rgb, gt)
    m2, s2 = metrics.image_metrics(rgb, gt)
    assert torch.equal(m1, m2) and torch.equal(s1, s2)
    map5 = metrics.rgb_ssim(gt, rgb, 1.0, return_map=True)
    for i in range(5):
        mi, si = metrics.image_metrics(rgb[i], gt[i])
        assert torch.equal(mi, m1[i:i + 1]) and torch.equal(si, s1[i:i + 1]), i
        assert torch.equal(metrics.rgb_ssim(gt[i], rgb[i], 1.0, return_map=True), map5[i])
    assert len(set(s1.tolist())) == 5                            # five different frames
    # and they are the reference's values (host restatement, pinned to the goldens)
    for i in (0, 3):
        want = ssim_host(gt[i].cpu().numpy(), rgb[i].cpu().numpy(), 1.0)
        assert abs(float(s1[i]) - want) <= 1e-9


def test_full_size_frame_pair_vs_host_restatement():
    gen = torch.Generator().manual_seed(11)
    gt = torch.rand(540, 960, 3, generator=gen)
    rgb = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    mse, ssim = metrics.image_metrics(rgb.to(DEV), gt.to(DEV))
    want = ssim_host(gt.numpy(), rgb.numpy(), 1.0)
    assert abs(float(ssim[0]) - want) <= 1e-9
    want_mse = np.mean((gt.double() - rgb.double()).numpy() ** 2)
    assert abs(float(mse[0]) - want_mse) <= 1e-12 * want_mse


def _scene():
    """The blended 4-field scene of tests/golden/local_4fields.npz, as test_gpu_parity builds it."""
    from localrf_amd import LocalTensorfs
    g = load_golden("local_4fields")
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]]).to(DEV)
    lt = quiet(LocalTensorfs, fov=85.6, n_init_frames=5, n_overlap=3, WH=(32, 24),
               n_iters_per_frame=600, n_iters_reg=100, lr_R_init=5e-3, lr_t_init=5e-4,
               lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
               lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[],
               camera_prior=None, device=DEV, lr_upsample_reset=True,
               aabb=aabb, gridSize=[16, 16, 16], **FIELD_KW)
    ref = {k[3:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items() if k.startswith("lt.")}
    quiet(lt.load, ref)
    lt = lt.to(DEV)
    for f in lt.tensorfs:
        f.to(DEV)
    return lt


def test_test_view_metrics_matches_the_reference_style_host_path():
    lt = _scene()
    W, H = 32, 24
    views = [5, 6, 8]                                            # each blends two fields (0+1, 0+1, 1+2)
    bw = lt.blending_weights.detach().cpu()
    assert all(int((bw[v] > 0).sum()) == 2 for v in views)
    gen = torch.Generator().manual_seed(3)
    gt = torch.rand(len(views), H, W, 3, generator=gen)
    fbases = [f"{v:06d}" for v in views]
    got = metrics.test_view_metrics(lt, gt.to(DEV), views, W, H, fbases=fbases)
    assert list(got) == fbases
    ray_ids = torch.arange(W * H, device=DEV)
    for i, v in enumerate(views):                                # renderer.py:65-77,158-163
        with torch.no_grad():
            rgb_map = lt(ray_ids, torch.tensor([v]).to(DEV), W, H, is_train=False, cam2world=None, test_id=True,
                         chunk=4096)[0]
        rgb_map = rgb_map.reshape(H, W, 3).cpu()
        mse = ((gt[i] - rgb_map) ** 2).mean()
        ssim = ssim_host(gt[i].numpy(), rgb_map.numpy(), 1)
        assert abs(got[fbases[i]]["ssim"] - ssim) <= 1e-9, (v, got[fbases[i]]["ssim"], ssim)
        assert abs(got[fbases[i]]["mse"] - float(mse)) <= 1e-6 * float(mse)
    ps = metrics.psnr([m["mse"] for m in got.values()])
    assert np.isfinite(ps) and ps > 0
