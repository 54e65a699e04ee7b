"""The device frame store on the MI355X (localrf_amd.DeviceFrames, csrc/lrf_frames.inl) against numpy restatements of
LocalRFDataset (tests/frames_cases.py, with the reference's line numbers): the gather bit for bit against
`self.all_X[idx_sample]`, the flow decode, the sharpness weight, the losses fed from the store, and train_synth through it."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_cases as fc  # noqa: E402
from localrf_amd import DeviceFrames, losses  # noqa: E402
from localrf_amd import _native as N  # noqa: E402
from localrf_amd.frames import KEYS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _store(H, W, num, capacity, n_init, **kw):
    cache = {}

    def reader(i):
        cache[i] = fc.make_frame(i, H, W, **kw)
        return cache[i]
    return DeviceFrames(reader, num, capacity, n_init_frames=n_init, device=DEV), cache


def _check_sample(st, cache, seed, is_refining, optimize_poses, batch=16 * 24):
    lo, hi = st.active_frames_bounds
    all_x = fc.reference_all_x([cache[i] for i in range(lo, hi)])
    random.seed(seed); np.random.seed(seed)
    ref = fc.reference_sample(st.test_mask, (lo, hi), st.n_px_per_frame, all_x, batch, is_refining, optimize_poses)
    random.seed(seed); np.random.seed(seed)
    got = st.sample(batch, is_refining, optimize_poses)
    assert bool(got["train_test_poses"]) == bool(ref["train_test_poses"])
    assert torch.equal(got["view_ids"].cpu(), torch.from_numpy(ref["view_ids"]))
    assert torch.equal(got["idx"].cpu(), torch.from_numpy(ref["idx"]))
    for k in KEYS:
        if k in all_x:
            assert torch.equal(got[k].cpu(), torch.from_numpy(np.ascontiguousarray(all_x[k]).astype(np.float32)[ref["idx"] - lo * st.n_px_per_frame])), k
        else:
            assert got[k] is None, k
    # the per-view pixel ids CapturedIteration stages give the same rows
    V = ref["view_ids"].shape[0]
    pix = torch.from_numpy(ref["idx"].reshape(V, -1) - ref["view_ids"][:, None] * st.n_px_per_frame).to(DEV)
    rows = st.gather(got["view_ids"], pix, want=st.available())
    for k in st.available():
        assert torch.equal(rows[k], got[k]), k
    return ref


@pytest.mark.parametrize("encoded", [True, False])
def test_gather_matches_reference_indexing_through_a_moving_window(built_lib, encoded):
    H, W = 23, 31
    st, cache = _store(H, W, num=40, capacity=9, n_init=7, encoded=encoded, flow_scale=540 / 271)
    for seed, refining, poses in ((0, False, True), (1, True, True), (2, False, False), (3, True, False)):
        _check_sample(st, cache, seed, refining, poses)
    st.activate_frames(2)                                       # [0, 9): full
    with pytest.raises(ValueError, match="capacity"):
        st.activate_frames(1)
    assert st.active_frames_bounds == [0, 9]
    st.deactivate_frames(5)
    st.activate_frames(4)                                       # frames 9..12 take the slots of 0..3: the slots wrap
    assert st.active_frames_bounds == [5, 13]
    assert list(st._slot_host[9:13]) == [0, 1, 2, 3]
    for seed in range(4, 10):
        _check_sample(st, cache, seed, seed % 2 == 0, True)
    st.deactivate_frames(11)
    st.activate_frames(6)
    for seed in range(10, 14):
        _check_sample(st, cache, seed, False, True)
    assert st.errors() == 0


def test_subset_outputs_and_stores_without_depth_or_flow(built_lib):
    st, cache = _store(8, 9, num=5, capacity=5, n_init=5, flow=False, depth=False, mask=False)
    assert st.available() == ("rgbs", "loss_weights")
    ref = _check_sample(st, cache, 7, True, False, batch=16 * 4)
    with pytest.raises(ValueError, match="holds no"):
        st.gather(torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), want=("fwd_flow",))
    st2, cache2 = _store(8, 9, num=5, capacity=5, n_init=5)
    v = torch.tensor([1, 4], dtype=torch.int64, device=DEV)
    ids = torch.arange(6, dtype=torch.int64, device=DEV) * 7
    only = st2.gather(v, ids, want=("fwd_mask",))
    full = st2.gather(v, ids)
    assert list(only) == ["fwd_mask"] and torch.equal(only["fwd_mask"], full["fwd_mask"])
    assert ref["view_ids"].shape == (16,)


def test_out_of_window_views_give_nan_rows_and_the_status_bit(built_lib):
    st, cache = _store(10, 12, num=12, capacity=6, n_init=6)
    st.deactivate_frames(2)
    n = 5
    good = st.gather(torch.tensor([3, 4, 5], dtype=torch.int64, device=DEV), torch.arange(3 * n, dtype=torch.int64, device=DEV))
    assert st.errors() == 0
    for bad_view in (1, 9, -1, 12, 1 << 40):                      # deactivated, never activated, negative, >= num_images
        v = torch.tensor([3, bad_view, 5], dtype=torch.int64, device=DEV)
        rows = st.gather(v, torch.arange(3 * n, dtype=torch.int64, device=DEV))
        for k in KEYS:
            r, g = rows[k].reshape(3, n, -1), good[k].reshape(3, n, -1)
            assert torch.isnan(r[1]).all(), (bad_view, k)
            assert torch.equal(r[0], g[0]) and torch.equal(r[2], g[2]), (bad_view, k)
        assert st.errors(clear=True) == N.LRF_FRAMES_ERR_NOT_RESIDENT, bad_view
    assert st.errors() == 0


def test_gather_under_capture_follows_the_window(built_lib):
    """A captured gather reads the live slot table: after the window moves, the replay gives the new frames' rows."""
    st, cache = _store(6, 7, num=10, capacity=4, n_init=4)
    v = torch.tensor([2, 3], dtype=torch.int64, device=DEV)
    ids = torch.arange(8, dtype=torch.int64, device=DEV) * 5
    st.gather(v, ids)                                           # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = st.gather(v, ids)
    g.replay()
    first = {k: t.clone() for k, t in out.items()}
    st.deactivate_frames(2)
    st.activate_frames(2)                                       # frames 4, 5 into the slots of 0, 1
    v.copy_(torch.tensor([4, 5], dtype=torch.int64, device=DEV))
    g.replay()
    ref = st.gather(v, ids)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
    assert not torch.equal(out["rgbs"], first["rgbs"])
    assert st.errors() == 0


def test_decode_flow_is_bit_identical(built_lib):
    H, W = 13, 17
    for scale in (1.0, 540 / 271, 0.5, 1 / 3):
        st, cache = _store(H, W, num=3, capacity=3, n_init=3, flow_scale=scale)
        for i in range(3):
            s = int(st._slot_host[i])
            e = cache[i]["encoded_fwd_flow"]
            assert {0, 32768, 32769, 65535} <= set(np.unique(e).tolist())
            f, m = fc.decode_flow_scaled(e, scale)
            b, n = fc.decode_flow_scaled(cache[i]["encoded_bwd_flow"], scale)
            assert np.array_equal(st.fwd_flow[s].cpu().numpy(), f.reshape(-1, 2))
            assert np.array_equal(st.fwd_mask[s].cpu().numpy(), m.reshape(-1))
            assert np.array_equal(st.bwd_flow[s].cpu().numpy(), b.reshape(-1, 2))
            assert np.array_equal(st.bwd_mask[s].cpu().numpy(), n.reshape(-1))


@pytest.mark.parametrize("H,W,mask", [(37, 53, True), (37, 53, False), (1, 9, False), (8, 1, True), (2, 2, False),
                                      (61, 3, True), (135, 241, False)])
def test_sharpness_weight_matches_the_reference_variance(built_lib, H, W, mask):
    st, cache = _store(H, W, num=3, capacity=3, n_init=3, mask=mask, flow=False)
    st2, _ = _store(H, W, num=3, capacity=3, n_init=3, mask=mask, flow=False)
    for i in range(3):
        s = int(st._slot_host[i])
        img = cache[i]["img"]
        exact, f32 = fc.sharpness_exact(img), fc.sharpness_numpy_f32(img)
        got = st.loss_weight[s].cpu().numpy()
        want = np.full(H * W, exact, np.float32) * (cache[i]["mask"].reshape(-1) if mask else 1)
        assert np.array_equal(got, want), (i, got[:4], exact)
        assert abs(float(exact) - float(f32)) <= 2e-6 * max(abs(float(f32)), 1e-30)
        assert np.array_equal(got, st2.loss_weight[s].cpu().numpy())            # bit-identical on a second upload
        if mask:
            assert (got == 0).any() and (got > 0).any()


def test_photometric_and_flow_losses_with_dataset_weights_and_masks(built_lib):
    """photometric_loss with the gathered loss weights = train.py:369-371; flow_loss with the gathered dataset masks = the
    torch chain of train.py:385-412 (oracle/vm_render_torch.flow_loss) with those masks, and differs from the position-only
    masks of losses.batch_gather when the dataset masks hold zeros."""
    from oracle import vm_render_torch as ot
    H, W, F_ = 48, 64, 8
    st, cache = _store(H, W, num=F_, capacity=F_, n_init=F_, flow_scale=0.05)
    random.seed(5); np.random.seed(5)
    b = st.sample(16 * 64, True, False)
    V, n = 16, 64
    gen = torch.Generator().manual_seed(9)
    rgb_map = torch.rand(V * n, 3, generator=gen).to(DEV)
    lw = b["loss_weights"]
    assert (lw == 0).any() and (lw > 0).any()
    got = losses.photometric_loss(rgb_map, b["rgbs"], lw)
    ref = (0.25 * (torch.abs(rgb_map - b["rgbs"]) * lw) / lw.mean()).mean()
    assert abs(float(got) - float(ref)) <= 1e-6 * abs(float(ref)), (float(got), float(ref))

    start = 0
    r6 = torch.eye(3)[:, :2][None].repeat(F_, 1, 1) + 0.02 * torch.randn(F_, 3, 2, generator=gen)
    b1 = torch.nn.functional.normalize(r6[..., 0], dim=-1)
    b2 = torch.nn.functional.normalize(r6[..., 1] - (b1 * r6[..., 1]).sum(-1, keepdim=True) * b1, dim=-1)
    c2w = torch.cat([torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -1), 0.05 * torch.randn(F_, 3, 1, generator=gen)], -1).to(DEV)
    pix = (b["idx"] % (H * W)).reshape(V, n)
    ij = torch.stack([pix % W, pix // W], -1)
    focal, center = torch.tensor([60.0], device=DEV), torch.tensor([W * 0.5, H * 0.5], device=DEV)
    dirs = torch.stack([(ij[..., 0] + 0.5 - center[0]) / focal, -(ij[..., 1] + 0.5 - center[1]) / focal, -torch.ones(V, n, device=DEV)], -1)
    depth = (0.5 + 3 * torch.rand(V, n, generator=gen)).to(DEV)
    views = b["view_ids"]
    fm, bm = b["fwd_mask"].reshape(V, n), b["bwd_mask"].reshape(V, n)
    assert (fm == 0).any() and (bm == 0).any()
    ff, bf = b["fwd_flow"].reshape(V, n, 2), b["bwd_flow"].reshape(V, n, 2)
    hip = losses.flow_loss(depth, dirs, ij, c2w, views, start, ff, fm, bf, bm, focal, center)
    aten, _ = ot.flow_loss(depth, dirs, ij, c2w, views, start, ff, fm, bf, bm, focal, center)
    assert abs(float(hip) - float(aten)) <= 1e-5 * abs(float(aten)), (float(hip), float(aten))
    pos = losses.batch_gather(views, pix, fwd_flow=st.fwd_flow[:F_].contiguous(), bwd_flow=st.bwd_flow[:F_].contiguous())
    by_position = losses.flow_loss(depth, dirs, ij, c2w, views, start, ff, pos["fwd_mask"], bf, pos["bwd_mask"], focal, center)
    assert abs(float(by_position) - float(hip)) > 1e-3 * abs(float(hip)), (float(by_position), float(hip))


def _train_synth():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_synth
    return train_synth


def test_train_synth_through_the_store_captured_and_eager(built_lib):
    train_synth = _train_synth()
    kw = dict(frames=9, final=80, iters_per_frame=30, n_max_frames=5, dev=DEV, geo_every=5, record_all=True, frames_store=True)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        g1 = train_synth.run(graph=True, max_iters=150, **kw)
        g2 = train_synth.run(graph=True, max_iters=150, **kw)
    finally:
        torch.use_deterministic_algorithms(was)
    a, b = np.array(g1["all_losses"]), np.array(g2["all_losses"])
    assert a.shape == b.shape and len(a) > 100 and np.array_equal(a, b)
    assert g1["frames_store"]["errors"] == 0 and g1["geometric_losses"]["iterations_with_them"] > 0
    eager = train_synth.run(graph=False, **kw)
    graph = train_synth.run(graph=True, **kw)
    assert graph["iterations"] == eager["iterations"] and graph["events"] == eager["events"], (graph["events"], eager["events"])
    print("train_synth through the store: events", eager["events"], "window", eager["frames_store"]["bounds"])
    assert eager["frames_store"]["bounds"][1] == 9 and graph["frames_store"]["bounds"] == eager["frames_store"]["bounds"]
    a, b = np.array(eager["all_losses"]), np.array(graph["all_losses"])
    assert a.shape == b.shape and np.isfinite(b).all()
    assert np.abs(a[:10] - b[:10]).max() <= 2e-5 * np.abs(a[:10]).max(), (a[:10], b[:10])
    assert np.abs(a[:25] - b[:25]).max() <= 5e-3 * np.abs(a[:25]).max(), np.abs(a[:25] - b[:25]).max()
    assert np.abs(a[:60] - b[:60]).max() <= 5e-2 * np.abs(a[:60]).max(), np.abs(a[:60] - b[:60]).max()
    assert abs(a[-20:].mean() - b[-20:].mean()) <= 0.25 * a[-20:].mean(), (a[-20:].mean(), b[-20:].mean())
    st = graph["graph"]
    assert st["replays"] >= 0.6 * graph["iterations"], st
    assert eager["frames_store"]["errors"] == 0 and graph["frames_store"]["errors"] == 0
    plain = train_synth.run(graph=False, **{**kw, "frames_store": False})
    assert not np.array_equal(np.array(plain["all_losses"]), a)                    # the weights and masks do reach the loss
