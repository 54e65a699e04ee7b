"""Novel-view rendering on the MI355X (csrc/lrf_encode.inl through localrf_amd.novel_views): the encode kernel against the
numpy restatement bit for bit, render_poses against the reference's own render(test=False) (tests/golden/novel_views.npz),
bit-identity of the batched renders with per-frame LocalTensorfs.forward calls, and iter_pose_frames."""
import numpy as np
import pytest
import torch

from localrf_amd import novel_views
from localrf_amd.pose_plan import PosePlan
from novel_views_cases import depth_idx_host, edge_depths, edge_rgbs, gap_case, golden, rgb8_host, scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _host_idx(depth, minmax):
    """depth_idx_host per frame; a frame without a positive depth (automatic range) maps to zeros, mi = NaN."""
    out, rng = [], []
    for f in depth:
        try:
            idx, r = depth_idx_host(f, minmax)
        except ValueError:
            idx, r = np.zeros(f.shape, np.uint8), (np.float32(np.nan), np.float32(np.nan_to_num(f).max()))
        out.append(idx)
        rng.append(r)
    return np.stack(out), np.array(rng, np.float32)


@pytest.mark.parametrize("V,H,W", [(3, 17, 23), (2, 360, 640), (700, 1, 3), (5, 2, 2)])
def test_encode_kernel_equals_the_restatement_bit_for_bit(V, H, W):
    rng = np.random.default_rng(V * 1000 + H)
    rgb = edge_rgbs(rng, V, H, W)
    depth = edge_depths(rng, V, H, W)
    if H * W <= 4:
        depth[1] = -np.abs(depth[1])                             # a frame without a positive depth
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    r, d = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
    want_rgb8 = rgb8_host(rgb)
    for minmax in ([0, 5], (0.5, 4.25), None):
        want_idx, want_rng = _host_idx(depth, minmax)
        rgb8, depth8, idx = novel_views.encode_frames(r, d, minmax=minmax, cmap=lut, return_index=True)
        again = novel_views.encode_frames(r, d, minmax=minmax, cmap=torch.from_numpy(lut).to(DEV), return_index=True)
        assert np.array_equal(rgb8.cpu().numpy(), want_rgb8)
        assert np.array_equal(idx.cpu().numpy(), want_idx), minmax
        assert np.array_equal(depth8.cpu().numpy(), lut[want_idx])
        assert all(torch.equal(a, b) for a, b in zip((rgb8, depth8, idx), again))
        if minmax is None:
            _, _, _, got_rng = novel_views._encode(None, d, None, torch.from_numpy(lut).to(DEV), False, True)
            got = got_rng.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want_rng))
            ok = ~np.isnan(want_rng)
            want_rng = want_rng + np.float32(0)                 # -0.0 -> +0.0: the kernel reads -0.0 as +0.0
            assert np.array_equal(got[ok].view(np.uint32), want_rng[ok].view(np.uint32))
    want_idx, want_rng = _host_idx(depth, None)
    empty = np.flatnonzero(np.isnan(want_rng[:, 0]))
    if empty.size == 0:
        img, mm, idx = novel_views.visualize_depth(d, None, cmap=lut, return_index=True)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(img.cpu().numpy(), lut[want_idx])
        assert np.array_equal(np.array(mm, np.float32), want_rng)
    else:
        with pytest.raises(ValueError, match=f"frame {empty[0]} has no positive depth"):
            novel_views.visualize_depth(d, None)


def test_visualize_depth_equals_the_reference_index_images():
    g = golden()
    for s in (0, 2):
        depth = torch.from_numpy(g[f"s{s}.depth"]).to(DEV)
        lut = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
        img, mm, idx = novel_views.visualize_depth(depth, [0, 5], cmap=lut, return_index=True)
        assert np.array_equal(idx.cpu().numpy(), g[f"s{s}.idx_fixed"]) and mm == [0, 5]
        assert np.array_equal(img.cpu().numpy(), np.repeat(g[f"s{s}.idx_fixed"][..., None], 3, axis=-1))
        for v in range(depth.shape[0]):                          # one frame at a time: [mi, ma] as the reference returns it
            img, mm, idx = novel_views.visualize_depth(depth[v], None, return_index=True)
            assert np.array_equal(idx.cpu().numpy(), g[f"s{s}.idx_auto"][v])
            assert np.array_equal(np.array(mm, np.float32), g[f"s{s}.range_auto"][v])
            assert np.array_equal(img.cpu().numpy(), novel_views.jet_lut()[g[f"s{s}.idx_auto"][v]])


def _near_boundary(x, tol):
    """Pixels whose value x lies within tol of a rounding / truncation boundary (x - boundary, boundaries at k + 0.5)."""
    return np.abs(x - np.floor(x) - 0.5) <= tol


def test_render_poses_against_the_reference():
    lt, g = scene(DEV)
    poses = torch.from_numpy(g["poses"]).to(DEV)
    W, H = int(g["W"]), int(g["H"])
    tests = g["test_frames"].tolist()
    for s in (0, 2):
        out = novel_views.render_poses(lt, poses, W, H, test_frames=tests, start=s, floater_thresh=0.5)
        assert out["frame_indices"].tolist() == g[f"s{s}.frame_indices"].tolist()
        rgb, depth = out["rgb"].cpu().numpy(), out["depth"].cpu().numpy()
        assert np.abs(rgb - g[f"s{s}.rgb"]).max() <= 1e-4
        assert np.abs(depth - g[f"s{s}.depth"]).max() <= 1e-4
        rgb8 = out["rgb8"].cpu().numpy()
        assert np.array_equal(rgb8, rgb8_host(rgb))               # our floats, encoded exactly
        ref8 = rgb8_host(g[f"s{s}.rgb"]).astype(int)
        diff = np.abs(rgb8.astype(int) - ref8)
        assert diff.max() <= 1
        assert _near_boundary(np.float32(255) * g[f"s{s}.rgb"], 1e-4 * 255)[diff > 0].all()
        _, _, idx = novel_views.visualize_depth(out["depth"], [0, 5], return_index=True)
        idx = idx.cpu().numpy()
        want, _ = _host_idx(depth, [0, 5])
        assert np.array_equal(idx, want)
        assert np.array_equal(out["depth8"].cpu().numpy(), novel_views.jet_lut()[want])
        ref = g[f"s{s}.idx_fixed"].astype(int)
        diff = np.abs(idx.astype(int) - ref)
        assert diff.max() <= 1
        scaled = np.float32(255) * np.clip(g[f"s{s}.depth"] / np.float32(5), 0, 1)
        assert _near_boundary(scaled + np.float32(0.5), 1e-4 * 255)[diff > 0].all()   # truncation: boundaries at integers


def _per_frame_forward(lt, poses, views, tests, W, H):
    ray_ids = torch.arange(W * H, dtype=torch.int64, device=DEV)
    rgbs, depths = [], []
    with torch.no_grad():
        for p, v in zip(poses, views):
            rgb, depth, _, _ = lt(ray_ids, torch.tensor([v], device=DEV), W, H, is_train=False, cam2world=p[None],
                                  test_id=v in tests, chunk=4096, floater_thresh=0.5)
            rgbs.append(rgb.reshape(H, W, 3))
            depths.append(depth.reshape(H, W))
    return torch.stack(rgbs), torch.stack(depths)


def test_batched_renders_are_bit_identical_to_per_frame_forward_calls():
    lt, g = scene(DEV)
    poses = torch.from_numpy(g["poses"]).to(DEV)
    W, H = int(g["W"]), int(g["H"])
    tests = g["test_frames"].tolist()
    outs = [novel_views.render_poses(lt, poses, W, H, test_frames=tests, floater_thresh=0.5, frames_per_call=f)
            for f in (1, 3, None)]
    views = outs[0]["frame_indices"].tolist()
    groups = PosePlan(lt, poses, W, H, tests, None, 0, None).groups
    assert any(i1 - i0 > 3 for i0, i1, _ in groups)                       # batching happens
    assert len({a for _, _, a in groups}) >= 3                            # mixed active sets
    assert any(len({views[i] in tests for i in range(i0, i1)}) == 2 for i0, i1, _ in groups)   # mixed test_id in a group
    for o in outs[1:]:
        for k in ("rgb", "depth", "rgb8", "depth8", "frame_indices"):
            assert torch.equal(o[k], outs[0][k]), k
    rgb, depth = _per_frame_forward(lt, poses, views, tests, W, H)
    assert torch.equal(rgb, outs[0]["rgb"]) and torch.equal(depth, outs[0]["depth"])
    # a larger frame, so the scene forward runs in several chunks, and the start quirk with caller frame indices
    W2, H2 = 160, 120
    fi = [(3 * i) % len(lt.r_c2w) for i in range(poses.shape[0])]
    a = novel_views.render_poses(lt, poses[:9], W2, H2, test_frames=tests, frame_indices=fi, start=1, floater_thresh=0.5,
                                 frames_per_call=2)
    b = novel_views.render_poses(lt, poses[:9], W2, H2, test_frames=tests, frame_indices=fi, start=1, floater_thresh=0.5)
    assert a["frame_indices"].tolist() == fi[1:8]
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["depth8"], b["depth8"])
    rgb, depth = _per_frame_forward(lt, poses[1:8], fi[1:8], tests, W2, H2)
    assert torch.equal(rgb, a["rgb"]) and torch.equal(depth, a["depth"])


def test_an_active_set_with_a_gap_renders_what_per_frame_forward_calls_render():
    """Active fields that are not adjacent: the blend-weight columns are gathered, not sliced."""
    lt, poses, views, W, H, tests = gap_case(DEV)
    out = novel_views.render_poses(lt, poses, W, H, test_frames=tests, frame_indices=views, floater_thresh=0.5, chunk=W * H * 3)
    assert [a for _, _, a in PosePlan(lt, poses, W, H, tests, views).groups] == [(0, 2), (1, 3), (0, 2)]
    rgb, depth = _per_frame_forward(lt, poses, views, tests, W, H)
    assert torch.equal(rgb, out["rgb"]) and torch.equal(depth, out["depth"])
    assert float(out["rgb"].std()) > 1e-3 and float(out["depth"].std()) > 1e-3
    small = novel_views.render_poses(lt, poses, W, H, test_frames=tests, frame_indices=views, floater_thresh=0.5, chunk=7)
    for k in ("rgb", "depth", "rgb8", "depth8"):
        assert torch.equal(small[k], out[k]), k


def test_normal_and_quantile_maps_compute_no_exposure(monkeypatch):
    """Exposure does not apply to a normal or a depth: with lr_exposure_init > 0 neither map may even compute one."""
    from localrf_amd import depth_quantiles, normals
    lt, g = scene(DEV)
    assert lt.lr_exposure_init > 0
    poses = torch.from_numpy(g["poses"][:2]).to(DEV)

    def forbidden(*a, **k):
        raise AssertionError("an exposure was computed for a map that has none")
    monkeypatch.setattr(lt, "_exposure_for", forbidden)
    tests = g["test_frames"].tolist()
    assert normals.render_normals(lt, poses, 12, 8, test_frames=tests)["normal"].shape == (2, 8, 12, 3)
    assert depth_quantiles.render_depth_quantiles(lt, poses, 12, 8, test_frames=tests)["depth"].shape == (1, 2, 8, 12)
    with pytest.raises(AssertionError, match="exposure"):
        novel_views.render_poses(lt, poses, 12, 8, test_frames=tests)


def test_iter_pose_frames_yields_the_encoded_frames_in_order():
    lt, g = scene(DEV)
    poses = torch.from_numpy(g["poses"]).to(DEV)
    W, H = int(g["W"]), int(g["H"])
    tests = g["test_frames"].tolist()
    out = novel_views.render_poses(lt, poses, W, H, test_frames=tests, floater_thresh=0.5)
    for fpc in (None, 2):
        items = list(novel_views.iter_pose_frames(lt, poses, W, H, test_frames=tests, floater_thresh=0.5, frames_per_call=fpc,
                                                  with_depth=True))
        assert [it[0] for it in items] == list(range(poses.shape[0]))
        for i, rgb8, depth8, depth in items:
            assert isinstance(rgb8, np.ndarray) and rgb8.shape == (H, W, 3) and rgb8.dtype == np.uint8
            assert np.array_equal(rgb8, out["rgb8"][i].cpu().numpy())
            assert np.array_equal(depth8, out["depth8"][i].cpu().numpy())
            assert np.array_equal(depth, out["depth"][i].cpu().numpy())
    gen = novel_views.iter_pose_frames(lt, poses, W, H, test_frames=tests, floater_thresh=0.5, frames_per_call=1)
    first = next(gen)
    assert first[0] == 0 and np.array_equal(first[1], out["rgb8"][0].cpu().numpy()) and len(first) == 3
    gen.close()
    assert torch.cuda.current_stream().query()                            # nothing left enqueued
