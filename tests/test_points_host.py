"""Point-cloud fusion without a GPU: the numpy restatement of csrc/lrf_points.inl against the reference's recorded camera
points, world points and reprojected pixels (tests/golden/points.npz), the conditions on the consistent synthetic trajectory,
argument refusals before any device work (Python and C ABI), the PLY writer, and the new symbols."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, pointcloud
from points_cases import (OFFSETS4, fuse_host, keep_mask, pixel_dirs, random_case, reproject, trajectory_case,
                          trajectory_shares, world_points)
from util import load_golden



def test_restatement_against_the_reference_points_and_pixels():
    """The bars are 4 x the largest difference between the reference's fp32 results and an fp64 evaluation of the same
    formulas, recorded with the golden (noise_world 2.7e-7, noise_px 4.6e-6 when recorded): the restatement and the reference
    are both fp32 evaluations of one expression in different summation orders, and the factor covers the independent
    roundings of each."""
    g = load_golden("points")
    depth, c2w, f, (cx, cy) = g["depth"], g["c2w"], g["focal"], g["center"]
    V, H, W = depth.shape
    dirs = pixel_dirs(H, W, f, cx, cy)
    assert np.array_equal(dirs.reshape(-1, 3).view(np.uint32), g["dirs"].view(np.uint32))      # the same expression: exact
    cam = (dirs[None] * depth[..., None]).astype(np.float32)
    assert np.array_equal(cam.reshape(V, -1, 3).view(np.uint32), g["cam_pts"].view(np.uint32))
    pw = world_points(depth, c2w, dirs)
    bar_w, bar_px = 4 * float(g["noise_world"]), 4 * float(g["noise_px"])
    assert 0 < bar_w < 1e-5 and 0 < bar_px < 1e-3
    e_w = float(np.abs(pw.reshape(V, -1, 3).astype(np.float64) - g["world_pts"]).max())
    print(f"world points: max diff {e_w:.3e}, bar {bar_w:.3e}")
    assert e_w <= bar_w
    worst = 0.0
    for o in g["offsets"].tolist():
        for v in np.flatnonzero(g[f"valid{o}"]):
            nz, u, w = reproject(pw[v], c2w[v + o], f, cx, cy)
            assert (nz > 1e-6).all()                                    # pts2px's clip never acted
            got = np.stack([u, w], -1).reshape(-1, 2).astype(np.float64)
            worst = max(worst, float(np.abs(got - g[f"px{o}"][v]).max()))
    print(f"reprojected pixels: max diff {worst:.3e}, bar {bar_px:.3e}")
    assert worst <= bar_px


def test_conditions_on_the_consistent_trajectory():
    """Case (b) with offsets (-2, -1, 1, 2), rel_tol 0.02, min_consistent 2, from the restatement alone."""
    case = trajectory_case()
    assert case["depth"].shape == (7, 48, 64)
    assert 0.13 < case["floater"].mean() < 0.17
    kept, kept_untouched, rejected_floaters = trajectory_shares(case)
    print(f"kept {kept:.4f}, untouched kept {kept_untouched:.4f}, floaters rejected {rejected_floaters:.4f}")
    assert 0.55 <= kept <= 0.85
    assert kept_untouched >= 0.80
    broad = trajectory_shares(case, all_offsets=False)[1]               # the end frames' pixels too, with the neighbours they have
    print(f"untouched kept, end frames included {broad:.4f}")
    assert broad >= 0.80
    assert rejected_floaters >= 0.95


def test_restatement_filters_and_order():
    c = random_case(5, 4, 9, 13)
    base = fuse_host(c["depth"], c["rgb8"], c["c2w"], c["f"], c["cx"], c["cy"])
    d = c["depth"]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d > 0)
    assert base["count"] == int(ok.sum()) and 0 < base["count"] < d.size
    key = base["src"][:, 0].astype(np.int64) * d[0].size + base["src"][:, 1]
    assert (np.diff(key) > 0).all()                                     # (frame, row, column) order
    v, pix = base["src"][:, 0], base["src"][:, 1]
    assert np.array_equal(base["rgb8"], c["rgb8"].reshape(4, -1, 3)[v, pix])
    ranged = fuse_host(c["depth"], None, c["c2w"], c["f"], c["cx"], c["cy"], depth_range=c["depth_range"])
    assert ranged["count"] < base["count"] and ranged["rgb8"] is None
    s2 = fuse_host(c["depth"], None, c["c2w"], c["f"], c["cx"], c["cy"], stride=2)
    col, row = s2["src"][:, 1] % 13, s2["src"][:, 1] // 13
    assert (col % 2 == 0).all() and (row % 2 == 0).all()
    # an offset that leaves the trajectory counts neither for nor against
    far = keep_mask(c["depth"], c["c2w"], c["f"], c["cx"], c["cy"], neighbours=(100, -100), min_consistent=2)[0]
    assert np.array_equal(far, ok)
    some = keep_mask(c["depth"], c["c2w"], c["f"], c["cx"], c["cy"], neighbours=(1, -1), rel_tol=0.05, min_consistent=1)[0]
    assert 0 < some.sum() < ok.sum()


def _valid_args():
    return dict(rgb=torch.zeros(2, 4, 5, 3), depth=torch.ones(2, 4, 5), poses=torch.eye(4)[None, :3].repeat(2, 1, 1),
                focal=4.0, center=(2.5, 2.0))


def test_python_refusals_before_any_device_work():
    def fuse(**over):
        a = _valid_args()
        a.update(over)
        rgb, depth, poses, focal, center = (a.pop(k) for k in ("rgb", "depth", "poses", "focal", "center"))
        return pointcloud.fuse_points(rgb, depth, poses, focal, center, **a)
    for bad, match in ((dict(depth=torch.ones(4, 5)), "depth"), (dict(depth=torch.ones(2, 4, 5).long()), "depth"),
                       (dict(depth=torch.ones(2, 0, 5), rgb=None), "depth"),
                       (dict(rgb=torch.zeros(2, 4, 5, 2)), "rgb"), (dict(rgb=torch.zeros(2, 4, 5, 3).long()), "rgb"),
                       (dict(poses=torch.zeros(3, 3, 4)), "poses"), (dict(poses=torch.zeros(2, 3, 3)), "poses"),
                       (dict(poses=torch.zeros(2, 3, 4).long()), "poses"),
                       (dict(focal=None), "focal"), (dict(center=(1.0, 2.0, 3.0)), "center"),
                       (dict(stride=0), "stride"), (dict(stride=1.5), "stride"),
                       (dict(depth_range=(2.0, 1.0)), "depth_range"), (dict(depth_range=(0.0, math.nan)), "depth_range"),
                       (dict(depth_range=(1.0,)), "depth_range"),
                       (dict(neighbours=(1, 0)), "neighbours"), (dict(neighbours=(1, 2, 1)), "neighbours"),
                       (dict(neighbours=tuple(range(1, 10))), "neighbours"), (dict(neighbours=(0.5,)), "neighbours"),
                       (dict(neighbours=(1,), fov360=True), "360"),
                       (dict(rel_tol=-0.1), "rel_tol"), (dict(rel_tol=math.nan), "rel_tol"),
                       (dict(min_consistent=-1), "min_consistent"), (dict(max_points=-1), "max_points")):
        with pytest.raises(ValueError, match=match):
            fuse(**bad)
    with pytest.raises(TypeError):
        fuse(depth=np.ones((2, 4, 5), np.float32))
    with pytest.raises(NativeError):                                    # valid arguments, CPU tensors: no fallback
        fuse()
    with pytest.raises(NativeError):
        fuse(rgb=None, fov360=True, focal=None, center=None)
    a = _valid_args()
    with pytest.raises(ValueError, match="H, W"):
        pointcloud.backproject(a["depth"], a["poses"], 4, 5, a["focal"], a["center"])
    with pytest.raises(ValueError, match="focal"):
        pointcloud.backproject(a["depth"], a["poses"], 5, 4)
    with pytest.raises(ValueError, match="poses"):
        pointcloud.backproject(a["depth"], a["poses"][:1], 5, 4, a["focal"], a["center"])
    with pytest.raises(NativeError):
        pointcloud.backproject(a["depth"], a["poses"], 5, 4, a["focal"], a["center"])
    with pytest.raises(NativeError):
        pointcloud.backproject(a["depth"], a["poses"], 5, 4, fov360=True)


def test_scene_point_cloud_refusals_on_a_cpu_scene():
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    F = len(lt.r_c2w)
    with pytest.raises(ValueError, match=f"{7 * F * H * W} bytes"):
        pointcloud.scene_point_cloud(lt, W, H, max_bytes=7 * F * H * W - 1)
    with pytest.raises(ValueError, match="bytes"):
        pointcloud.scene_point_cloud(lt, W, H, poses=torch.from_numpy(g["poses"]), max_bytes=1000)
    with pytest.raises(ValueError, match="W, H"):
        pointcloud.scene_point_cloud(lt, 0, H)
    with pytest.raises(ValueError, match="neighbours"):
        pointcloud.scene_point_cloud(lt, W, H, neighbours=(0,))
    with pytest.raises(TypeError, match="unknown"):
        pointcloud.scene_point_cloud(lt, W, H, strides=2)
    with pytest.raises(ValueError, match="poses"):
        pointcloud.scene_point_cloud(lt, W, H, poses=torch.zeros(3, 2, 4))
    with pytest.raises(NativeError):                                    # valid arguments, CPU scene
        pointcloud.scene_point_cloud(lt, W, H, max_bytes=7 * F * H * W)


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    for cols in (rgb, None):
        path = tmp_path / "cloud.ply"
        n = pointcloud.write_ply(str(path), torch.from_numpy(xyz), None if cols is None else torch.from_numpy(cols))
        assert n == 37
        raw = path.read_bytes()
        end = raw.index(b"end_header\n") + len(b"end_header\n")
        lines = raw[:end].decode("ascii").split("\n")
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == "element vertex 37"
        props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
        want = [["float", "x"], ["float", "y"], ["float", "z"]]
        if cols is not None:
            want += [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
        assert props == want
        dt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if cols is not None else []))
        assert len(raw) - end == 37 * dt.itemsize and dt.itemsize == (15 if cols is not None else 12)
        rec = np.frombuffer(raw[end:], dtype=dt)
        assert np.array_equal(rec["p"].view(np.uint32), xyz.view(np.uint32))
        if cols is not None:
            assert np.array_equal(rec["c"], rgb)
    assert pointcloud.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32)) == 0
    with pytest.raises(ValueError):
        pointcloud.write_ply(str(tmp_path / "bad.ply"), xyz[:, :2])
    with pytest.raises(ValueError):
        pointcloud.write_ply(str(tmp_path / "bad.ply"), xyz, rgb[:5])
    with pytest.raises(ValueError):
        pointcloud.write_ply(str(tmp_path / "bad.ply"), xyz, rgb.astype(np.float32))


def test_points_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, ("lrf_points_fuse", "lrf_points_workspace_bytes"))
    assert "#define LRF_POINTS_MAX_NEIGH 8" in header and N.LRF_POINTS_MAX_NEIGH == 8
    assert built_lib.lrf_abi_version() == 7
    ws = built_lib.lrf_points_workspace_bytes
    assert ws(0, 4, 5, 1) == 0 and ws(2, 0, 5, 1) == 0 and ws(2, 4, 5, 0) == 0 and ws(1 << 20, 1 << 10, 2, 1) == 0
    assert ws(1, 1, 1, 1) == 256                                         # one workgroup: 16 keep words + one count
    assert ws(64, 360, 640, 1) >= 64 * 360 * 640 // 8
    assert ws(64, 360, 640, 2) < ws(64, 360, 640, 1) // 3
    fake = C.c_void_p(FAKE)

    def fuse(capacity=10, xyz=fake, rgb8_out=fake, src=fake, count=fake, wsp=fake, **over):
        a = filled(N.LrfPointsFuse, dict(depth=FAKE, rgb8=FAKE, cam2world=FAKE, focal=FAKE, center=FAKE, V=2, H=4, W=5, fov360=0, stride=1,
                                         d_min=0.0, d_max=math.inf, n_neigh=2, rel_tol=0.02, min_consistent=1, neigh=(-1, 1)), **over)
        return refused(built_lib, built_lib.lrf_points_fuse(C.byref(a), capacity, xyz, rgb8_out, src, count, wsp, None))
    assert fuse(V=0) == "lrf_points_fuse: need V, H, W, stride >= 1 and V H W < 2^31"
    for bad in (dict(H=0), dict(W=-1), dict(stride=0), dict(V=1 << 20, H=1 << 10)):
        assert "need V, H, W, stride >= 1" in fuse(**bad)
    for bad in (dict(depth=None), dict(cam2world=None), dict(xyz=None), dict(src=None), dict(count=None), dict(wsp=None)):
        assert fuse(**bad) == "lrf_points_fuse: null argument", bad
    assert "go together" in fuse(rgb8=None) and "go together" in fuse(rgb8_out=None)
    assert "focal and center" in fuse(focal=None) and "focal and center" in fuse(center=None)
    assert "capacity" in fuse(capacity=-1)
    assert "d_min <= d_max" in fuse(d_min=2.0, d_max=1.0) and "d_min <= d_max" in fuse(d_min=math.nan)
    assert "n_neigh" in fuse(n_neigh=9) and "n_neigh" in fuse(n_neigh=-1)
    assert "pinhole" in fuse(fov360=1)
    assert "must not be 0" in fuse(neigh=(1, 0))
    assert "repeated" in fuse(n_neigh=3, neigh=(1, 2, 1))
    assert "rel_tol" in fuse(rel_tol=-1.0) and "rel_tol" in fuse(rel_tol=math.nan)
    assert "min_consistent" in fuse(min_consistent=-1)
    assert "4-byte aligned" in fuse(xyz=C.c_void_p(0x10002)) and "4-byte aligned" in fuse(depth=0x10001)
    assert "8-byte aligned" in fuse(count=C.c_void_p(0x10004)) and "8-byte aligned" in fuse(wsp=C.c_void_p(0x10004))
    assert refused(built_lib, built_lib.lrf_points_fuse(None, 0, fake, fake, fake, fake, fake, None)) == "lrf_points_fuse: null argument"


def test_points_kernels_use_no_scratch():
    """k_points_mark, k_points_scan and k_points_write as __graft_entry__.build() compiles them: no scratch, no spills, the
    divisions of the pixel mapping are full-precision ones, and the kernels multiply and add separately (contraction off)."""
    from isa_util import assert_no_scratch, device_asm
    found = assert_no_scratch(device_asm(), (r"k_points_mark", r"k_points_scan", r"k_points_write"), match="search", total=3, body_too=True)
    mark = dict(found)[[n for n, _ in found if "mark" in n][0]]
    assert "v_div_fixup_f32" in mark and "v_rndne_f32" in mark
