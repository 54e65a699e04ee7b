"""Geometry diagnostics on the MI355X (csrc/lrf_select.inl and csrc/lrf_evalgeo.inl through localrf_amd.diagnostics): exact
quantiles and medians against np.quantile / torch.median bit for bit, reproducibility and graph capture, the flow and depth
comparison images against the reference's recorded ones (tests/golden/eval_geometry.npz) and the host restatement, and
test_view_evaluation end to end."""
import numpy as np
import pytest
import torch

from localrf_amd import NativeError, diagnostics, metrics
from geometry_cases import depth_image_host, flow_images_host, golden_views, pred_flow_host
from test_gpu_metrics import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QS = [0.0, 0.5, 0.8, 0.9, 1.0]


def _bits(a):
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _rows(rng):
    out = []
    for n in (1, 2, 3, 4, 5, 16, 17, 1000, 1001, 4096, 4097, 65537, 262143):
        for kind in range(4):
            a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4)).astype(np.float32)
            if kind == 1:
                a = rng.integers(-3, 4, n).astype(np.float32)
            elif kind == 2:
                a[rng.integers(0, n, max(1, n // 7))] = np.inf
                a[rng.integers(0, n, max(1, n // 9))] = -np.inf
            elif kind == 3 and n > 2:
                a[rng.integers(0, n)] = np.nan
            out.append(a)
    out.append(np.zeros(9, np.float32))
    out.append(np.full(5, np.inf, np.float32))
    return out


def _want_quantile(a, q):
    with np.errstate(invalid="ignore"):
        return np.quantile(a, q)


def test_quantile_and_median_match_numpy_and_torch_bit_for_bit():
    rng = np.random.default_rng(7)
    for a in _rows(rng):
        x = torch.from_numpy(a).to(DEV)
        for q in QS:
            got = diagnostics.quantile(x, q).cpu().numpy()
            assert _bits(got) == _bits(_want_quantile(a, q)), (a.size, q, got, _want_quantile(a, q))
        med = diagnostics.median(x).cpu().numpy()
        assert _bits(med) == _bits(torch.median(torch.from_numpy(a)).numpy()), (a.size, med)


def test_large_row_and_ragged_batch():
    rng = np.random.default_rng(8)
    a = rng.standard_normal(4194304 + 3).astype(np.float32)
    x = torch.from_numpy(a).to(DEV)
    for q in (0.5, 0.9):
        assert _bits(diagnostics.quantile(x, q).cpu().numpy()) == _bits(np.quantile(a, q))
    assert _bits(diagnostics.median(x).cpu().numpy()) == _bits(torch.median(torch.from_numpy(a)).numpy())
    sizes = [1, 2, 3, 1000, 70001, 4099]
    rows = [(rng.standard_normal(n) * 3).astype(np.float32) for n in sizes]
    rows[3][:500] = 2.0                                               # duplicates across the rank
    got_q = diagnostics.quantile([torch.from_numpy(r).to(DEV) for r in rows], 0.9).cpu().numpy()
    got_m = diagnostics.median([torch.from_numpy(r).to(DEV) for r in rows]).cpu().numpy()
    for i, r in enumerate(rows):
        assert _bits(got_q[i]) == _bits(np.quantile(r, 0.9)), sizes[i]
        assert _bits(got_m[i]) == _bits(torch.median(torch.from_numpy(r)).numpy()), sizes[i]
    batch = torch.from_numpy(np.stack([rng.standard_normal(3001).astype(np.float32) for _ in range(6)])).to(DEV)
    got = diagnostics.quantile(batch, 0.8).cpu().numpy()
    want = [np.quantile(r, 0.8) for r in batch.cpu().numpy()]
    assert (_bits(got) == _bits(np.array(want, np.float32))).all()


def test_select_is_reproducible_and_capturable():
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((4, 300001)).astype(np.float32)).to(DEV)
    a = diagnostics.quantile(x, 0.9).clone()
    b = diagnostics.quantile(x, 0.9).clone()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        diagnostics.quantile(x, 0.9)                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = diagnostics.quantile(x, 0.9)
        med = diagnostics.median(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), a.view(torch.int32))
    x.copy_(torch.from_numpy(rng.standard_normal((4, 300001)).astype(np.float32)).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    xs = x.cpu().numpy()
    assert (_bits(out.cpu().numpy()) == _bits(np.array([np.quantile(r, 0.9) for r in xs], np.float32))).all()
    assert torch.equal(med.cpu(), torch.median(x.cpu(), dim=-1).values)


def _golden_inputs(v, g):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for k, x in v.items() if isinstance(x, np.ndarray) and x.ndim > 0}
    return t, torch.from_numpy(g["cam2world"]).to(DEV), torch.tensor([float(g["focal"])], device=DEV), torch.from_numpy(g["center"]).to(DEV)


def test_flow_and_depth_comparison_against_the_reference_golden():
    g, views = golden_views()
    W, H = int(g["W"]), int(g["H"])
    for v in views:
        t, c2w, focal, center = _golden_inputs(v, g)
        fwd, bwd, fraw, braw, quant = diagnostics.flow_comparison(t["depth"], t["dirs"], t["ij"].long(), c2w, int(v["idx"]), focal,
                                                                  center, t["fwd_flow"], t["fwd_mask"], t["bwd_flow"], t["bwd_mask"],
                                                                  W, H, return_raw=True)
        assert np.abs(fwd.cpu().numpy() - v["fwd_cmp"]).max() <= 1e-5
        assert np.abs(bwd.cpu().numpy() - v["bwd_cmp"]).max() <= 1e-5
        q = quant.cpu().numpy()
        for k, raw in enumerate((fraw.cpu().numpy(), fraw.cpu().numpy(), braw.cpu().numpy(), braw.cpu().numpy())):
            half = raw[:2 * H, (k % 2) * W:(k % 2 + 1) * W]
            assert _bits(q[k]) == _bits(np.quantile(half, 0.9)), k
        d, stats = diagnostics.depth_comparison(t["depth"], t["invdepth"], W, H, return_stats=True)
        assert np.abs(d.cpu().numpy() - v["depth_cmp"]).max() <= 1e-5
        _, want = depth_image_host(v["depth"], v["invdepth"], W, H)
        st = stats.cpu().numpy()
        assert _bits(st[:2]).tolist() == _bits(want[:2]).tolist()       # medians exact
        assert np.allclose(st[2:], want[2:], rtol=1e-6, atol=0)


@pytest.mark.parametrize("W,H", [(480, 270), (960, 540)])
def test_flow_comparison_full_size_vs_host(W, H):
    g, views = golden_views()
    rng = np.random.default_rng(W)
    HW = W * H
    depth = (1.0 + 3.0 * rng.random(HW)).astype(np.float32)
    dirs = np.concatenate([rng.uniform(-0.5, 0.5, (HW, 2)), -np.ones((HW, 1))], 1).astype(np.float32)
    ij = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.int64)
    c2w = g["cam2world"]
    idx = 5
    focal, center = np.float32(0.9 * W), np.array([W / 2, H / 2], np.float32)
    flows = [(2.0 * rng.standard_normal((H, W, 2))).astype(np.float32) for _ in range(2)]
    masks = [(rng.random((H, W)) < 0.8).astype(np.float32) for _ in range(2)]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    fwd, bwd = diagnostics.flow_comparison(d(depth), d(dirs), d(ij), d(c2w), idx, d(focal.reshape(1)), d(center), d(flows[0]),
                                           d(masks[0]), d(flows[1]), d(masks[1]), W, H)
    for got, off, k in ((fwd, 1, 0), (bwd, -1, 1)):
        pred = pred_flow_host(c2w, idx, depth, dirs, ij, focal, center, off)
        want, _, _ = flow_images_host(pred, flows[k], masks[k], W, H)
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-5


def test_test_view_evaluation_end_to_end():
    lt = _scene()
    W, H = 32, 24
    views = [5, 6, lt.get_cam2world().shape[0] - 1]
    n = len(views)
    gen = torch.Generator().manual_seed(5)
    gt = torch.rand(n, H, W, 3, generator=gen).to(DEV)
    fwd_flow, bwd_flow = [(2 * torch.randn(n, H, W, 2, generator=gen)).to(DEV) for _ in range(2)]
    fwd_mask, bwd_mask = [(torch.rand(n, H, W, generator=gen) < 0.8).float().to(DEV) for _ in range(2)]
    inv = (0.2 + torch.rand(n, H, W, generator=gen)).to(DEV)
    fb = [f"{v:06d}" for v in views]
    res = diagnostics.test_view_evaluation(lt, views, W, H, gt_rgbs=gt, fwd_flow=fwd_flow, fwd_mask=fwd_mask, bwd_flow=bwd_flow,
                                           bwd_mask=bwd_mask, invdepths=inv, fbases=fb)
    assert res["metrics"] == metrics.test_view_metrics(lt, gt, views, W, H, fbases=fb)
    ray_ids = torch.arange(W * H, device=DEV)
    c2w = lt.get_cam2world().detach()
    for i, v in enumerate(views):
        with torch.no_grad():
            _, depth, dirs, ij = lt(ray_ids, [v], W, H, is_train=False, cam2world=None, test_id=True, chunk=4096)
        f, b = diagnostics.flow_comparison(depth, dirs, ij, c2w, v, lt.focal(W), lt.center(W, H), fwd_flow[i], fwd_mask[i],
                                           bwd_flow[i], bwd_mask[i], W, H)
        dc = diagnostics.depth_comparison(depth, inv[i], W, H)
        assert torch.equal(res["fwd_flow_cmp"][i], f) and torch.equal(res["bwd_flow_cmp"][i], b)
        assert torch.equal(res["depth_cmp"][i], dc)
        assert res["fwd_flow_cmp"][i].shape == (3 * H, 2 * W) and dc.shape == (3 * H, W)
    part = diagnostics.test_view_evaluation(lt, views, W, H, invdepths=inv)
    assert part["metrics"] == {} and part["fwd_flow_cmp"] == [] and part["bwd_flow_cmp"] == [] and len(part["depth_cmp"]) == n
    part = diagnostics.test_view_evaluation(lt, views, W, H, fwd_flow=fwd_flow, fwd_mask=fwd_mask, bwd_flow=bwd_flow, bwd_mask=bwd_mask)
    assert part["depth_cmp"] == [] and len(part["fwd_flow_cmp"]) == n


def test_refusals_raise_before_any_launch():
    g, views = golden_views()
    v = views[0]
    W, H = int(g["W"]), int(g["H"])
    t, c2w, focal, center = _golden_inputs(v, g)
    with pytest.raises(NativeError):
        diagnostics.flow_comparison(t["depth"], t["dirs"], t["ij"].long(), c2w, c2w.shape[0], focal, center, t["fwd_flow"],
                                    t["fwd_mask"], t["bwd_flow"], t["bwd_mask"], W, H)
    with pytest.raises(NativeError):
        diagnostics.flow_comparison(t["depth"], t["dirs"], t["ij"].long(), c2w, -1, focal, center, t["fwd_flow"],
                                    t["fwd_mask"], t["bwd_flow"], t["bwd_mask"], W, H)
    with pytest.raises(NativeError):
        diagnostics.quantile(torch.empty(3, 0, device=DEV), 0.5)
    with pytest.raises(NativeError):
        diagnostics.median([torch.ones(3, device=DEV), torch.empty(0, device=DEV)])
    with pytest.raises(NativeError):
        diagnostics.depth_comparison(t["depth"].cpu(), t["invdepth"], W, H)
