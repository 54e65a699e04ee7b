"""Point-cloud fusion on the MI355X (csrc/lrf_points.inl through localrf_amd.pointcloud): the kernels against the numpy
restatement of tests/points_cases.py bit for bit, capacity handling, reproducibility, a non-default stream, backproject against
the rays of lrf_scene_rays, and scene_point_cloud against fuse_points over render_poses' tensors.

360 degrees: the directions hold cos / sin, which numpy and the device's math library need not round alike, so the
restatement takes them from lrf_scene_rays (the same pixel_dir device function) and everything after them -- scaling,
rotation, translation, filtering, compaction -- is compared bit for bit; numpy's own directions are compared with a bar."""
import numpy as np
import pytest
import torch

from localrf_amd import novel_views, pointcloud, scene_ops
from novel_views_cases import rgb8_host, scene
from points_cases import OFFSETS4, fuse_host, pixel_dirs, pixel_dirs_360, random_case, trajectory_case, world_points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dirs_360_device(H, W):
    ids = torch.arange(H * W, dtype=torch.int64, device=DEV)
    eye = torch.eye(4, device=DEV)[None, :3].contiguous()
    _, dirs, _ = scene_ops.scene_rays(ids, eye, torch.zeros(1, 3, device=DEV), None, None, H * W, W, H, fov360=True)
    return dirs.reshape(H, W, 3).cpu().numpy()


def _fuse_device(case, with_rgb=True, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    fov360 = kw.get("fov360", False)
    return pointcloud.fuse_points(t(case["rgb8"]) if with_rgb else None, t(case["depth"]), t(case["c2w"]),
                                  None if fov360 else float(case["f"]), None if fov360 else (float(case["cx"]), float(case["cy"])),
                                  **kw)


def _check(case, with_rgb=True, **kw):
    """fuse_points on the device against fuse_host: count, src, xyz (as uint32) and rgb8, all exact.  -> count"""
    V, H, W = case["depth"].shape
    host_kw = dict(kw)
    host_kw.pop("max_points", None)
    if kw.get("fov360"):
        host_kw["dirs"] = _dirs_360_device(H, W)
    want = fuse_host(case["depth"], case["rgb8"] if with_rgb else None, case["c2w"], case["f"], case["cx"], case["cy"], **host_kw)
    got = _fuse_device(case, with_rgb, **kw)
    print(f"{(V, H, W)} {kw}: count {got['count']} (host {want['count']})")
    assert got["count"] == want["count"]
    M = want["count"]
    assert tuple(got["xyz"].shape) == (M, 3) and tuple(got["src"].shape) == (M, 2)
    assert got["xyz"].dtype is torch.float32 and got["src"].dtype is torch.int32
    assert np.array_equal(got["src"].cpu().numpy(), want["src"])
    assert np.array_equal(got["xyz"].cpu().numpy().view(np.uint32), want["xyz"].view(np.uint32))
    if with_rgb:
        assert got["rgb8"].dtype is torch.uint8 and np.array_equal(got["rgb8"].cpu().numpy(), want["rgb8"])
    else:
        assert got["rgb8"] is None
    return M


@pytest.mark.parametrize("V,H,W", [(1, 1, 1), (3, 17, 23), (5, 24, 32), (7, 48, 64), (2, 360, 640), (300, 2, 3)])
def test_kernels_equal_the_restatement_bit_for_bit(V, H, W):
    if (V, H, W) == (7, 48, 64):
        case = trajectory_case()                                        # case (b)
        rng = (0.0, np.inf)
    else:
        case = random_case(100 * V + H, V, H, W, smooth=True)
        rng = case["depth_range"]
    assert case["depth"].shape == (V, H, W)
    eight = (-4, -3, -2, -1, 1, 2, 3, V + 5)                            # one offset larger than V
    counts = [_check(case),
              _check(case, with_rgb=False, stride=2, depth_range=rng),
              _check(case, stride=3, neighbours=(1,), rel_tol=0.05),
              _check(case, neighbours=OFFSETS4, rel_tol=0.02, min_consistent=2),
              _check(case, stride=2, neighbours=OFFSETS4, rel_tol=0.05, min_consistent=4, depth_range=rng),
              _check(case, neighbours=eight, rel_tol=0.1, min_consistent=3),
              _check(case, stride=3, neighbours=(V + 1, -V - 7), min_consistent=2),   # every offset leaves the trajectory
              _check(case, fov360=True),
              _check(case, with_rgb=False, fov360=True, stride=2, depth_range=rng)]
    if V * H * W > 100:
        assert counts[3] < counts[0] and len(set(counts)) > 4          # the filters bite, and differently
    if V >= 5 and H * W > 100:
        assert 0 < counts[3] and 0 < counts[5]                          # and do not reject everything
    rough = _check(random_case(7 * V + W, V, H, W, smooth=False, angle=0.6, shift=1.0), neighbours=(-1, 1, 2), rel_tol=0.3)
    assert rough >= 0


def test_directions_360_of_numpy_and_device_agree_closely():
    """The angles are the same fp32 values on both sides (IEEE multiply, divide, add).  Each library's cos / sin lies within
    about 2 ulp of the exact value (ulp = 6e-8 below 1), so two libraries differ by up to 4 ulp per factor and a product of two
    factors by about 8 ulp plus its own rounding: 5e-7.  The bar is twice that."""
    for H, W in ((17, 23), (360, 640)):
        e = float(np.abs(_dirs_360_device(H, W) - pixel_dirs_360(H, W)).max())
        print(f"360 directions {H} x {W}: max diff {e:.3e}")
        assert e <= 1e-6


def test_zero_points_all_points_and_capacity():
    case = random_case(3, 3, 17, 23)
    none = dict(case, depth=-np.abs(np.nan_to_num(case["depth"], posinf=1.0, neginf=1.0)) - 1)
    got = _fuse_device(none)
    assert got["count"] == 0 and tuple(got["xyz"].shape) == (0, 3) and tuple(got["rgb8"].shape) == (0, 3)
    assert _check(none, neighbours=(1, -1)) == 0
    every = dict(case, depth=np.abs(np.nan_to_num(case["depth"], posinf=1.0, neginf=1.0)) + 1)
    assert _check(every) == 3 * 17 * 23
    assert _check(every, stride=2) == 3 * 9 * 12
    M = _check(case, neighbours=(1,), rel_tol=0.05)
    assert 0 < M < 3 * 17 * 23
    with pytest.raises(ValueError, match=f"holds {M} points"):
        _fuse_device(case, neighbours=(1,), rel_tol=0.05, max_points=M - 1)
    assert _check(case, neighbours=(1,), rel_tol=0.05, max_points=M) == M
    assert _check(case, neighbours=(1,), rel_tol=0.05, max_points=10 ** 9) == M
    with pytest.raises(ValueError, match=f"holds {M} points"):
        _fuse_device(case, neighbours=(1,), rel_tol=0.05, max_points=0)


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    case = trajectory_case()
    kw = dict(neighbours=OFFSETS4, rel_tol=0.02, min_consistent=2, stride=1)
    a, b = _fuse_device(case, **kw), _fuse_device(case, **kw)
    assert a["count"] == b["count"] and a["count"] > 0
    for k in ("xyz", "rgb8", "src"):
        assert torch.equal(a[k], b[k]), k
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    rgb, depth, c2w = t(case["rgb8"]), t(case["depth"]), t(case["c2w"])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = pointcloud.fuse_points(rgb, depth, c2w, float(case["f"]), (float(case["cx"]), float(case["cy"])), **kw)
    side.synchronize()
    assert c["count"] == a["count"]
    for k in ("xyz", "rgb8", "src"):
        assert torch.equal(a[k], c[k]), k


def test_float_colours_are_encoded_as_encode_frames_does():
    case = random_case(9, 3, 17, 23)
    rng = np.random.default_rng(1)
    rgb = rng.uniform(-0.1, 1.1, (3, 17, 23, 3)).astype(np.float32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    got = pointcloud.fuse_points(t(rgb), t(case["depth"]), t(case["c2w"]), torch.tensor([float(case["f"])], device=DEV),
                                 torch.tensor([float(case["cx"]), float(case["cy"])], device=DEV), stride=2)
    want = fuse_host(case["depth"], rgb8_host(rgb), case["c2w"], case["f"], case["cx"], case["cy"], stride=2)
    assert got["count"] == want["count"] and np.array_equal(got["rgb8"].cpu().numpy(), want["rgb8"])
    assert np.array_equal(got["xyz"].cpu().numpy().view(np.uint32), want["xyz"].view(np.uint32))


@pytest.mark.parametrize("fov360", [False, True])
def test_backproject_against_scene_rays(fov360):
    """xyz = R (dir d) + t against rays_o + rays_d d with rays_d = R dir: a different association, so not bit-exact.  The bar
    is 4 x the largest difference the two associations show in numpy fp32 on the same inputs, relative to the largest
    coordinate (2.8e-7 for the pinhole case, 6.1e-7 at 360 degrees with numpy's own directions), computed here on the host,
    never from the kernel's output."""
    V, H, W = 4, 30, 40
    case = random_case(21, V, H, W, angle=0.8, shift=2.0)
    with np.errstate(invalid="ignore"):
        depth = np.where(case["depth"] > 100, np.float32(2.0), case["depth"])     # no 1e30 points: they would set the scale
    c2w = case["c2w"]
    dirs = _dirs_360_device(H, W) if fov360 else pixel_dirs(H, W, case["f"], case["cx"], case["cy"])
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(depth) & (depth > 0)
    A = world_points(depth, c2w, dirs)
    R, tr = c2w[:, None, None, :, :3], c2w[:, None, None, :, 3]
    rd = np.stack([(R[..., r, 0] * dirs[..., 0] + R[..., r, 1] * dirs[..., 1]) + R[..., r, 2] * dirs[..., 2] for r in range(3)], -1)
    with np.errstate(all="ignore"):
        B = (tr + rd.astype(np.float32) * depth[..., None]).astype(np.float32)
    scale = float(np.abs(A[ok]).max())
    bar = 4 * float(np.abs(A[ok].astype(np.float64) - B[ok]).max()) / scale
    print(f"fov360={fov360}: association noise bar {bar:.3e} (relative), largest coordinate {scale:.3e}")
    assert 0 < bar < 1e-5
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    d_dev, c_dev = t(depth), t(c2w)
    focal = None if fov360 else torch.tensor([float(case["f"])], device=DEV)
    center = None if fov360 else torch.tensor([float(case["cx"]), float(case["cy"])], device=DEV)
    xyz, src = pointcloud.backproject(d_dev, c_dev, W, H, focal, center, fov360=fov360)
    assert xyz.shape[0] == int(ok.sum())
    v, pix = np.nonzero(ok.reshape(V, -1))
    assert np.array_equal(src.cpu().numpy(), np.stack([v, pix], -1).astype(np.int32))
    ids = torch.arange(V * H * W, dtype=torch.int64, device=DEV)
    rays, _, _ = scene_ops.scene_rays(ids, c_dev, torch.zeros(1, 3, device=DEV), focal, center, H * W, W, H, fov360=fov360,
                                      squeeze=True)
    ref = (rays[:, :3] + rays[:, 3:] * d_dev.reshape(-1, 1))[torch.from_numpy(ok.reshape(-1)).to(DEV)]
    err = float((xyz - ref).abs().max()) / scale
    print(f"fov360={fov360}: backproject vs rays_o + rays_d * depth: {err:.3e} (relative), bar {bar:.3e}")
    assert err <= bar


def test_scene_point_cloud_equals_fuse_points_over_render_poses(monkeypatch):
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    F = len(lt.r_c2w)
    kw = dict(stride=1, neighbours=(-1, 1), rel_tol=0.05, min_consistent=1, depth_range=(0.05, 50.0))
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    for poses, fi in ((None, list(range(F))), (torch.from_numpy(g["poses"]).to(DEV), None)):
        got = pointcloud.scene_point_cloud(lt, W, H, poses=poses, floater_thresh=0.5, **kw)
        p = own if poses is None else poses
        out = novel_views.render_poses(lt, p, W, H, frame_indices=fi, floater_thresh=0.5)
        want = pointcloud.fuse_points(out["rgb8"], out["depth"], p, lt.focal(W), lt.center(W, H), **kw)
        print(f"scene_point_cloud: {got['count']} of {p.shape[0] * H * W} pixels")
        assert got["count"] == want["count"] and 0 < got["count"] <= p.shape[0] * H * W
        for k in ("xyz", "rgb8", "src"):
            assert torch.equal(got[k], want[k]), k
        assert got["src"][:, 0].max().item() < p.shape[0]

    def forbidden(*a, **k):
        raise AssertionError("a launch path was reached before the max_bytes guard")
    monkeypatch.setattr(novel_views, "render_poses", forbidden)
    monkeypatch.setattr(pointcloud, "_fuse", forbidden)
    with pytest.raises(ValueError, match="max_bytes"):
        pointcloud.scene_point_cloud(lt, W, H, max_bytes=7 * F * H * W - 1, **kw)
