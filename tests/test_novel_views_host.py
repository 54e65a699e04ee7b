"""Novel-view rendering without a GPU: the numpy restatements of the frame encoding against the reference's recorded index
images (tests/golden/novel_views.npz) and its byte rules, the start / frame-index mapping of renderer.render(test=False)
on a CPU copy of the golden scene, argument refusals before any device work, and the new C ABI symbols."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, refused
from localrf_amd import NativeError, novel_views
from localrf_amd.pose_plan import PosePlan
from novel_views_cases import depth_idx_frames, depth_idx_host, edge_depths, edge_rgbs, golden, rgb8_host, scene



def test_depth_index_restatement_equals_the_reference_images():
    g = golden()
    for s in (0, 2):
        depth = g[f"s{s}.depth"]
        idx, _ = depth_idx_frames(depth, [0, 5])
        assert np.array_equal(idx, g[f"s{s}.idx_fixed"])
        idx, ranges = depth_idx_frames(depth, None)
        assert np.array_equal(idx, g[f"s{s}.idx_auto"])
        assert np.array_equal(ranges.view(np.uint32), g[f"s{s}.range_auto"].view(np.uint32))


def _visualize_depth_numpy(depth, minmax):
    """utils/utils.py:184-196 up to cv2.applyColorMap, line by line (numpy 2.2 promotion)."""
    x = np.nan_to_num(depth)
    if minmax is None:
        mi = np.min(x[x > 0])
        ma = np.max(x)
    else:
        mi, ma = minmax
    with np.errstate(invalid="ignore", over="ignore"):
        x = (x - mi) / (ma - mi + 1e-8)
        x = (255 * np.clip(x, 0, 1)).astype(np.uint8)
    return x


def test_depth_index_edge_cases():
    rng = np.random.default_rng(3)
    d = edge_depths(rng, 3, 17, 23)
    for minmax in ([0, 5], (0.5, 4.25), (-1, 7), None):
        for f in d:
            want = _visualize_depth_numpy(f, minmax)
            got, _ = depth_idx_host(f, minmax)
            assert np.array_equal(got, want), minmax
    mi, ma = np.float32(0.3), np.float32(4.7)                   # a range visualize_depth returned: fp32 arithmetic
    assert np.array_equal(depth_idx_host(d[0], None)[0], _visualize_depth_numpy(d[0], None))
    D = novel_views.fixed_range((mi, ma))[2]
    assert D == np.float32(ma - mi + 1e-8) and D.dtype == np.float32
    assert novel_views.fixed_range([0, 5]) == (np.float32(0), np.float32(5), np.float32(5))
    zeros = np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError):
        _visualize_depth_numpy(zeros, None)
    with pytest.raises(ValueError):
        depth_idx_host(zeros, None)
    assert not depth_idx_host(zeros, [0, 5])[0].any()
    special = np.array([[np.nan, np.inf, -np.inf, 5.0, 2.5, 0.0]], np.float32)
    assert depth_idx_host(special, [0, 5])[0].tolist() == [[0, 255, 0, 255, 127, 0]]
    assert depth_idx_host(special, None)[0].tolist() == _visualize_depth_numpy(special, None).tolist()


def test_rgb_byte_rule():
    rng = np.random.default_rng(4)
    x = edge_rgbs(rng, 2, 9, 11)
    got = rgb8_host(x)
    v = np.float32(255) * x
    with np.errstate(invalid="ignore"):
        want = np.clip(np.rint(v), 0, 255)
    want[np.isnan(v)] = 0
    assert np.array_equal(got, want.astype(np.uint8))
    # element by element: round half to even, as saturate_cast<uchar>(float) (cvRound) does for a rendered colour
    for a, b in zip(x.reshape(-1)[:2000], got.reshape(-1)[:2000]):
        y = float(np.float32(255) * a)
        assert b == (0 if y != y else min(255, max(0, round(y)))) if abs(y) < 2 ** 31 else b in (0, 255)
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    t = np.float32(255) * ties
    exact = t == np.arange(255, dtype=np.float32) + np.float32(0.5)
    assert exact.sum() > 100
    assert np.array_equal(rgb8_host(ties)[exact] % 2, np.zeros(int(exact.sum()), np.uint8))


def test_jet_table():
    lut = novel_views.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [128, 0, 0] and lut[255].tolist() == [0, 0, 128]      # BGR: dark blue .. dark red
    assert lut[:, 1].max() == 255 and lut[:, 0].max() == 255 and lut[:, 2].max() == 255


def test_start_and_frame_index_mapping_on_the_host():
    lt, g = scene("cpu")
    poses = torch.from_numpy(g["poses"])
    N = poses.shape[0]
    W, H = int(g["W"]), int(g["H"])
    tests = g["test_frames"].tolist()
    nearest = novel_views.nearest_frames(lt, poses)
    ref = np.array([int(torch.argmin(torch.norm(torch.stack(list(lt.t_c2w)) - p[None, :, 3], dim=-1))) for p in poses])
    assert nearest.tolist() == ref.tolist()
    assert nearest[N - 5].item() == 6                           # frame 7 duplicates frame 6's translation: first index
    for s in (0, 2):
        plan = PosePlan(lt, poses, W, H, tests, None, s, None)
        p, views, is_test, groups = plan.poses, plan.views, plan.is_test, plan.groups
        n = N - 2 * s
        assert views == g[f"s{s}.frame_indices"].tolist() and len(views) == n
        assert torch.equal(p, poses[s:s + n])                   # frame i: pose poses[start + i]
        assert views == novel_views.nearest_frames(lt, poses[s:])[s:s + n].tolist()   # frame_indices[start + i]
        assert is_test == [v in tests for v in views]
        flat = [i for i0, i1, _ in groups for i in range(i0, i1)]
        assert flat == list(range(n))
        bw = lt.blending_weights.detach()
        for i0, i1, active in groups:
            assert all(tuple(torch.nonzero(bw[views[i]])[:, 0].tolist()) == active for i in range(i0, i1))
        for fpc in (1, 3):
            gs = PosePlan(lt, poses, W, H, tests, None, s, fpc).groups
            assert max(i1 - i0 for i0, i1, _ in gs) <= fpc
            assert [i for i0, i1, _ in gs for i in range(i0, i1)] == list(range(n))
    fi = [i % len(lt.r_c2w) for i in range(N)]
    views = PosePlan(lt, poses, W, H, (), fi, 3, None).views
    assert views == fi[3:3 + N - 6]
    assert PosePlan(lt, poses[:3], W, H, (), None, 2, None).views == []          # start past the middle: no frame


def test_a_plan_on_a_cpu_scene_is_host_only(monkeypatch):
    """Construction launches nothing and works on a CPU scene; only the device half refuses it."""
    from localrf_amd import _native

    def forbidden(*a, **k):
        raise AssertionError("a native call was reached while planning")
    for name in ("launch", "call"):
        monkeypatch.setattr(_native, name, forbidden)
    lt, g = scene("cpu")
    poses = torch.from_numpy(g["poses"])
    W, H = int(g["W"]), int(g["H"])
    tests = g["test_frames"].tolist()
    plan = PosePlan(lt, poses, W, H, tests, chunk=100)
    assert (plan.lt, plan.W, plan.H, plan.chunk, plan.n) == (lt, W, H, 100, poses.shape[0])
    assert plan.views == g["s0.frame_indices"].tolist() and plan.is_test == [v in tests for v in plan.views]
    assert [i for i0, i1, _ in plan.groups for i in range(i0, i1)] == list(range(plan.n))
    assert torch.equal(plan.poses, poses[:, :3])
    for exposure in (False, True):
        with pytest.raises(NativeError, match="no CPU fallback") as e:
            plan.on_device(exposure=exposure)
        assert "cpu" in str(e.value)


def test_refusals_before_any_device_work():
    lt, g = scene("cpu")
    poses = torch.from_numpy(g["poses"])
    W, H = int(g["W"]), int(g["H"])
    with pytest.raises(ValueError, match="frames_per_call"):
        novel_views.render_poses(lt, poses, W, H, frames_per_call=0)
    with pytest.raises(ValueError, match="poses"):
        novel_views.render_poses(lt, poses[:, :2], W, H)
    with pytest.raises(ValueError, match="poses"):
        novel_views.render_poses(lt, poses.long(), W, H)
    with pytest.raises(ValueError, match="W, H"):
        novel_views.render_poses(lt, poses, 0, H)
    with pytest.raises(ValueError, match="start"):
        novel_views.render_poses(lt, poses, W, H, start=-1)
    with pytest.raises(ValueError, match="cmap"):
        novel_views.render_poses(lt, poses, W, H, cmap=np.zeros((256, 4), np.uint8))
    with pytest.raises(ValueError, match="cmap"):
        novel_views.render_poses(lt, poses, W, H, cmap=torch.zeros(256, 3))
    with pytest.raises(ValueError, match="frame_indices"):
        novel_views.render_poses(lt, poses, W, H, frame_indices=[0, 1])
    with pytest.raises(ValueError, match="outside"):
        novel_views.render_poses(lt, poses, W, H, frame_indices=[99] * poses.shape[0])
    with torch.no_grad():
        lt.blending_weights[5].zero_()                          # frame 5 without an active field
    fi = [0, 1, 5, 2]
    with pytest.raises(ValueError, match="frame 2: its nearest frame 5 has no active field"):
        novel_views.render_poses(lt, poses[:4], W, H, frame_indices=fi)
    with pytest.raises(ValueError, match="no active field"):
        list(novel_views.iter_pose_frames(lt, poses[:4], W, H, frame_indices=fi))
    with pytest.raises(NativeError):                            # valid arguments, CPU scene: no fallback
        novel_views.render_poses(lt, poses[:2], W, H, frame_indices=[0, 1])
    rgb, depth = torch.zeros(2, 4, 5, 3), torch.zeros(2, 4, 5)
    with pytest.raises(ValueError):
        novel_views.encode_frames(rgb, depth[:1])
    with pytest.raises(ValueError):
        novel_views.encode_frames(rgb[..., :2], depth)
    with pytest.raises(ValueError):
        novel_views.encode_frames(rgb.int(), depth)
    with pytest.raises(ValueError, match="cmap"):
        novel_views.encode_frames(rgb, depth, cmap=np.zeros((255, 3), np.uint8))
    with pytest.raises(ValueError, match="minmax"):
        novel_views.encode_frames(rgb, depth, minmax=(1, 2, 3))
    with pytest.raises(ValueError, match="cmap"):
        novel_views.visualize_depth(depth, cmap=np.zeros((256, 3), np.float32))
    with pytest.raises(NativeError):
        novel_views.encode_frames(rgb, depth)
    with pytest.raises(NativeError):
        novel_views.visualize_depth(depth)


def test_encode_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    declared_exported_bound(built_lib, ("lrf_encode_frames", "lrf_encode_frames_workspace_bytes"))
    assert built_lib.lrf_abi_version() == 7
    assert built_lib.lrf_encode_frames_workspace_bytes(3) == 3 * 64 * 8
    assert built_lib.lrf_encode_frames_workspace_bytes(0) == 0
    fake = C.c_void_p(FAKE)
    fr = (C.c_float * 3)(0.0, 5.0, 5.0)

    def enc(rgb=fake, depth=fake, V=2, H=4, W=5, lut=fake, fixed=fr, rgb8=fake, depth8=fake, idx=None, rng=None, ws=None):
        return refused(built_lib, built_lib.lrf_encode_frames(rgb, depth, V, H, W, lut, fixed, rgb8, depth8, idx, rng, ws, None))
    assert enc(V=0) == "lrf_encode_frames: need V >= 1, H, W > 0 and 3 V H W < 2^31"
    assert "need V >= 1" in enc(V=0) and "need V >= 1" in enc(H=0) and "need V >= 1" in enc(V=1 << 20, H=1 << 10)
    assert enc(depth=None) == "lrf_encode_frames: null argument"
    assert enc(lut=None) == "lrf_encode_frames: null argument"
    assert enc(rgb8=None) == "lrf_encode_frames: rgb and rgb8 go together"
    assert enc(fixed=None) == "lrf_encode_frames: the automatic range needs a workspace"
    assert "16-byte aligned" in enc(rgb=C.c_void_p(0x10004))
    assert "4-byte aligned" in enc(idx=C.c_void_p(0x10002))


def test_encode_kernels_use_no_scratch():
    """k_encode (both range modes) and k_encode_range, as __graft_entry__.build() compiles them: no scratch, no spills, and
    the division of the index image is a full-precision one (no v_rcp_f32 without the div_fixup that follows it)."""
    from isa_util import assert_no_scratch, device_asm, find
    assert_no_scratch(device_asm(), (r"k_encodeILb0E", r"k_encodeILb1E", r"k_encode_range"), match="search", total=3)
    for name, body in find(device_asm(), r"k_encodeILb[01]E"):
        assert "v_div_fixup_f32" in body and "scratch_" not in body, name
