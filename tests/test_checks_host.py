"""The shared argument checks of the geometry modules (localrf_amd/_checks.py), the frame batcher of pointcloud.SceneFrames
and the batcher of the launches over points, without a GPU: a table of accepted edge values and refused values per validator,
the batches of a CPU scene with the renderers replaced by recorders, the chunks of a launch over points with the launch replaced
by a recorder, and the order "other arguments, then the device" in one caller per module."""
import math

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, _checks, alignment, cloud, depth_quantiles, mesh, mesh_distance, mesh_raster, mesh_texture, novel_views
from localrf_amd.pointcloud import SceneFrames
from novel_views_cases import scene

INT32 = (1 << 31) - 1


class Unconvertible:
    def __int__(self):
        raise TypeError("no integer here")


JUNK = (True, np.True_, "3", None, math.nan, math.inf, -1, [1], Unconvertible())     # refused by every integer check
# (label, check of one value, the name the refusal carries, accepted -> returned, refused)
VALIDATORS = (
    ("integer in [0, 2^31)", lambda x: _checks.check_int("count", x, 0, INT32, "an integer in [0, 2^31)"), "count",
     ((0, 0), (INT32, INT32), (3.0, 3), (np.int64(5), 5), (np.float32(2.0), 2)), JUNK + (1.5, 2 ** 31)),
    ("None or an integer", lambda x: _checks.check_int("cap", x, 0, INT32, "None or an integer in [0, 2^31)", none_ok=True), "cap",
     ((None, None), (0, 0), (INT32, INT32)), tuple(x for x in JUNK if x is not None) + (1.5, 2 ** 31)),
    ("integer >= 1", lambda x: _checks.check_int("frames_per_call", x, 1, wording="an integer >= 1"), "frames_per_call",
     ((1, 1), (2 ** 31, 2 ** 31), (2 ** 40, 2 ** 40)), JUNK + (1.5, 0)),
    ("integer in [0, 1000]", lambda x: _checks.check_int("iterations", x, 0, 1000), "iterations",
     ((0, 0), (1000, 1000)), JUNK + (1.5, 1001, 2 ** 31)),
    ("max_bytes", _checks.check_bytes, "max_bytes", ((0, 0), (1 << 40, 1 << 40), (8.0, 8)), JUNK + (1.5,)),
    ("finite positive number", lambda x: _checks.check_positive("cell", x), "cell",
     ((1, 1.0), (1.5, 1.5), (5e-324, 5e-324), (2 ** 31, 2.0 ** 31), (np.float32(0.5), 0.5)),
     (True, np.True_, "x", None, math.nan, math.inf, -1, 0, 0.0, [1.0], Unconvertible())),
    ("number in [0, 1]", lambda x: _checks.check_interval("min_fraction", x, 0.0, 1.0, "lie in [0, 1]"), "min_fraction",
     ((0, 0.0), (1, 1.0), (0.5, 0.5), (np.float32(0.25), 0.25)),
     (True, np.True_, 1.5, "3", None, math.nan, math.inf, -1, 2 ** 31, [0.5], Unconvertible(), -1e-300, 1.0000000000000002)),
    ("number in (0, 1]", lambda x: _checks.check_interval("lam", x, 0.0, 1.0, "satisfy 0 < lam <= 1", open_lo=True), "lam",
     ((5e-324, 5e-324), (1, 1.0)), (True, np.True_, 1.5, "3", None, math.nan, math.inf, -1, 0, 0.0, -0.0, [0.5], Unconvertible())),
    ("number in [-1, 0]", lambda x: _checks.check_interval("mu", x, -1.0, 0.0, "satisfy -1 <= mu <= 0"), "mu",
     ((-1, -1.0), (0, 0.0), (-0.53, -0.53)), (True, np.True_, 1.5, "3", None, math.nan, -math.inf, -1.5, 5e-324, [0.0])),
    ("flag", lambda x: _checks.check_flag("dedupe", x), "dedupe",
     ((True, True), (False, False), (np.True_, True), (np.False_, False)), (1, 0, 1.5, "3", None, math.nan, [True], Unconvertible())),
    ("depth_range", _checks.check_range, "depth_range",
     (((0.0, math.inf), (0.0, math.inf)), ((1, 1), (1.0, 1.0)), ([0.5, 2], (0.5, 2.0)), ((-math.inf, 0), (-math.inf, 0.0))),
     ((2.0, 1.0), (math.nan, 1.0), (0.0, math.nan), (1.0,), (1.0, 2.0, 3.0), [])),
    ("origin", _checks.check_origin, "origin",
     (((0, 0, 0), (0.0, 0.0, 0.0)), (np.array([1.0, 2.0, 3.0], np.float32), (1.0, 2.0, 3.0)), (torch.tensor([[1.0], [2.0], [-3.0]]), (1.0, 2.0, -3.0))),
     ((0, 0), (0, 0, 0, 0), (0, math.nan, 0), (0, math.inf, 0), "3", None, True, 1.5, [Unconvertible()] * 3, Unconvertible(), ("a", "b", "c"))),
    ("image size", lambda wh: _checks.check_size(*wh), "W",
     (((1, 1), (1, 1)), ((8.0, 6), (8, 6)), ((INT32, 1), (INT32, 1))),
     ((0, 4), (4, 0), (True, 4), (np.True_, 4), (2.5, 4), ("3", 4), (None, 4), (math.nan, 4), (math.inf, 4), (-1, 4), (2 ** 31, 1),
      (1 << 16, 1 << 15), ([4], 4), (Unconvertible(), 4))),
    ("max_distance", _checks.check_max_distance, "max_distance",       # float() decides: a string that spells a number passes
     ((0, 0.0), (math.inf, math.inf), (np.float32(0.5), 0.5), (3, 3.0), (1.5, 1.5), ("3", 3.0)),
     (True, np.True_, math.nan, -1, -1e-300, -math.inf, "far", None, [1.0], Unconvertible())),
    ("thresholds", _checks.check_thresholds, "threshold",              # returned as float32 values: the kernel compares in fp32
     (((), []), ([], []), ((0.5, 1), [0.5, 1.0]), ((np.float32(0.5),), [0.5]), ((0.1,) * 8, [float(np.float32(0.1))] * 8),
      ((1e-45,), [float(np.float32(1e-45))])),
     ((0.1,) * 9, (True,), (np.True_,), (math.nan,), (math.inf,), (-1,), (0,), ("a",), "ab", 0.5, None, (0.1, None), (1e-50,), (1e39,),
      (5e-324,), (Unconvertible(),))),
    ("unit", _checks.check_unit, "unit",
     ((1, 1.0), (0.5, 0.5), (np.float32(0.5), 0.5), (1e-45, 1e-45), (3e38, 3e38)),
     (True, np.True_, math.nan, math.inf, -1, 0, "x", None, [1.0], Unconvertible(), 1e-50, 1e39, 5e-324)),
)


@pytest.mark.parametrize("label,check,name,accepted,refused", VALIDATORS, ids=[v[0] for v in VALIDATORS])
def test_validator_table(label, check, name, accepted, refused):
    for x, want in accepted:
        got = check(x)
        assert got == want and type(got) is type(want), (label, x, got)
    for x in refused:
        with pytest.raises(ValueError, match=name):
            check(x)


def _cpu_mesh(**over):
    m = {"vertices": torch.zeros(4, 3), "faces": torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32),
         "rgb8": torch.zeros(4, 3, dtype=torch.uint8), "counts": (4, 2)}
    m.update(over)
    return m


def test_mesh_and_frame_checks():
    v, f, c, Nv, Nf = _checks.check_mesh(_cpu_mesh())
    assert (Nv, Nf) == (4, 2) and c is not None
    assert _checks.check_mesh(_cpu_mesh(rgb8=None))[2] is None
    assert _checks.check_mesh({"vertices": torch.zeros(0, 3), "faces": torch.zeros(0, 3, dtype=torch.int32)})[3:] == (0, 0)
    for bad, name in (([torch.zeros(4, 3)], "mesh"), ({"vertices": torch.zeros(4, 3)}, "mesh"), (_cpu_mesh(vertices=np.zeros((4, 3))), "vertices"),
                      (_cpu_mesh(faces=[[0, 1, 2]]), "faces"), (_cpu_mesh(rgb8=np.zeros((4, 3), np.uint8)), "rgb8")):
        with pytest.raises(TypeError, match=name):
            _checks.check_mesh(bad)
    for bad, name in ((_cpu_mesh(vertices=torch.zeros(4, 3, dtype=torch.float64)), "vertices"), (_cpu_mesh(vertices=torch.zeros(4, 2)), "vertices"),
                      (_cpu_mesh(faces=torch.zeros(2, 3, dtype=torch.int64)), "faces"), (_cpu_mesh(faces=torch.zeros(2, 4, dtype=torch.int32)), "faces"),
                      (_cpu_mesh(rgb8=torch.zeros(4, 3)), "rgb8"), (_cpu_mesh(rgb8=torch.zeros(3, 3, dtype=torch.uint8)), "rgb8"),
                      (_cpu_mesh(vertices=torch.zeros(0, 3), rgb8=None), "without vertices")):
        with pytest.raises(ValueError, match=name):
            _checks.check_mesh(bad)
    faces = _cpu_mesh()["faces"]
    assert _checks.check_faces(faces, 4) == (4, 2) and _checks.check_faces(faces, INT32) == (INT32, 2)
    for bad in JUNK + (1.5, 2 ** 31):
        with pytest.raises(ValueError, match="n_vertices"):
            _checks.check_faces(faces, bad)

    depth = torch.ones(2, 4, 5)
    assert _checks.check_depth(depth) == (2, 4, 5)
    with pytest.raises(TypeError, match="depth"):
        _checks.check_depth(depth.numpy())
    for bad in (torch.ones(4, 5), torch.ones(2, 4, 5, dtype=torch.int32), torch.ones(0, 4, 5)):
        with pytest.raises(ValueError, match="depth"):
            _checks.check_depth(bad)
    assert tuple(_checks.check_frame_poses(torch.zeros(2, 4, 4), 2).shape) == (2, 3, 4)
    with pytest.raises(ValueError, match="3 poses for 2 depth frames"):
        _checks.check_frame_poses(torch.zeros(3, 3, 4), 2)
    with pytest.raises(ValueError, match="3 poses for 2 frames"):
        _checks.check_frame_poses(torch.zeros(3, 3, 4), 2, "frames")
    assert _checks.check_intrinsics(None, None, True) == (None, None) and _checks.check_intrinsics(5.0, (1.0, 2.0), False) == (5.0, (1.0, 2.0))
    for focal, center in ((None, (1.0, 2.0)), (5.0, None), (5.0, (1.0, 2.0, 3.0)), ((5.0, 5.0), (1.0, 2.0))):
        with pytest.raises(ValueError, match="focal"):
            _checks.check_intrinsics(focal, center, False)
    _checks.check_rgb(torch.zeros(2, 4, 5, 3), depth)
    _checks.check_rgb(torch.zeros(2, 4, 5, 3, dtype=torch.uint8), depth)
    with pytest.raises(TypeError, match="rgb"):
        _checks.check_rgb(np.zeros((2, 4, 5, 3), np.float32), depth)
    for bad in (torch.zeros(2, 4, 5, 3, dtype=torch.int32), torch.zeros(2, 4, 5, 2), torch.zeros(1, 4, 5, 3)):
        with pytest.raises(ValueError, match="rgb"):
            _checks.check_rgb(bad, depth)
    rgb8 = torch.arange(2 * 4 * 5 * 3, dtype=torch.uint8).view(2, 4, 5, 3)
    assert _checks.rgb8_frames(rgb8, depth) is rgb8                          # uint8 passes through; float would be encoded (HIP)
    assert _checks.float_of_key(0) == 0.0 and _checks.float_of_key(0x3F800000) == 1.0 and _checks.float_of_key(-1) == -0.0


def test_points_checks():
    assert _checks.check_points(torch.zeros(7, 3)) == 7 and _checks.check_points(torch.zeros(0, 3)) == 0
    assert _checks.check_points(torch.zeros(8, 6)[:, ::2]) == 8              # any strides: points_on_device makes it contiguous
    with pytest.raises(TypeError, match="points must be a torch tensor"):
        _checks.check_points(np.zeros((3, 3), np.float32))
    for bad in (torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 3, 3)):
        with pytest.raises(ValueError, match=r"points must be \[N, 3\] float32"):
            _checks.check_points(bad)


def test_chunks_cover_every_item_once(monkeypatch):
    assert _checks.POINTS_PER_CALL == 1 << 30 and list(_checks.chunks(7)) == [(0, 7)]
    for n in (0, 1, 4, 5, 6, 11):
        want = [(i0, min(5, n - i0)) for i0 in range(0, n, 5)]
        assert list(_checks.chunks(n, 5)) == want
        monkeypatch.setattr(_checks, "POINTS_PER_CALL", 5)                      # read at each call
        assert list(_checks.chunks(n)) == want
        monkeypatch.setattr(_checks, "POINTS_PER_CALL", 1 << 30)
    from localrf_amd import _native
    seen = []
    monkeypatch.setattr(_native, "launch", lambda name, dev, *args, guard=False: seen.append((name, dev, args)))
    monkeypatch.setattr(alignment, "PAIRS_PER_CALL", 5)
    for n in (1, 4, 5, 6, 11):
        a, b, keep = torch.zeros(n, 3), torch.ones(n, 3), torch.ones(n, dtype=torch.uint8)
        del seen[:]
        words = alignment._pair_words((0.0, 0.0, 0.0), 1.0, a, b, keep)
        spans = [(i0, min(5, n - i0)) for i0 in range(0, n, 5)]
        assert tuple(words.shape) == (len(spans), 24) and words.dtype is torch.int64 and len(seen) == len(spans)
        assert sum(args[4] for _, _, args in seen) == n
        for j, ((i0, m), (name, dev, args)) in enumerate(zip(spans, seen)):         # one launch per chunk, each into its own row
            assert name == "lrf_align_pairs" and dev == a.device
            assert args[1:] == (a[i0:].data_ptr(), b[i0:].data_ptr(), keep[i0:].data_ptr(), m, words[j].data_ptr())
        del seen[:]
        assert alignment._pair_words((0.0, 0.0, 0.0), 1.0, a, b, None).shape == (len(spans), 24) and all(args[3] is None for _, _, args in seen)
        near = {"closest": torch.zeros(n, 3), "distance": torch.zeros(n), "index": torch.zeros(n, dtype=torch.int32), "face": torch.zeros(n, dtype=torch.int32)}
        mesh_index = _StubMeshIndex()
        mesh_index.vertices, mesh_index.faces, mesh_index.counts = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), (4, 2)
        for index, normals, symbol, key in ((mesh_index, None, "lrf_align_plane", "face"), (_StubCloudIndex(), torch.zeros(8, 3), "lrf_align_plane_cloud", "index")):
            del seen[:]
            words = alignment._plane_words(index, a, near, (0.0, 0.0, 0.0), 2.0, math.inf, normals)
            assert tuple(words.shape) == (len(spans), 48) and [name for name, _, _ in seen] == [symbol] * len(spans)
            assert [args[1] for _, _, args in seen] == [words[j].data_ptr() for j in range(len(spans))]
            p = seen[-1][2][0]._obj                                                # one struct, refilled per chunk: the last chunk's
            i0, m = spans[-1]
            assert (p.N, p.points, p.closest, p.distance, getattr(p, key)) == (m, a[i0:].data_ptr(), near["closest"][i0:].data_ptr(),
                                                                               near["distance"][i0:].data_ptr(), near[key][i0:].data_ptr())
            assert (p.u, p.gate) == (2.0, math.inf)


class _StubMeshIndex(mesh_distance.MeshIndex):
    """A MeshIndex without a device and without a face: the checks of closest that come before the device check."""
    def __init__(self):
        self.device, self.counts, self._grid = torch.device("cpu"), (0, 0), None


class _StubCloudIndex(cloud.CloudIndex):
    def __init__(self, m=8):
        self.points, self.device, self.counts, self._grid = torch.zeros(m, 3), torch.device("cpu"), (m,), None


class _Recorder:
    def __init__(self, result):
        self.calls, self.result = [], result

    def __call__(self, lt, poses, W, H, *args, **kw):
        self.calls.append((poses, args, kw))
        return self.result(poses)


def test_scene_frames_batches_on_a_cpu_scene(monkeypatch):
    from localrf_amd import _native
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    monkeypatch.setattr(_native, "require_gpu", lambda *a, **k: None)          # the device step: the scene stays on the CPU
    renders = _Recorder(lambda p: {"depth": ("depth", p.shape[0]), "rgb8": ("rgb8", p.shape[0])})
    medians = _Recorder(lambda p: ("median", p.shape[0]))
    monkeypatch.setattr(novel_views, "render_poses", renders)
    monkeypatch.setattr(depth_quantiles, "fusion_depth", medians)
    poses = torch.from_numpy(g["poses"])
    n = int(poses.shape[0])
    assert n >= 3
    given = [(7 * i + 1) % len(lt.r_c2w) for i in range(n)]

    def frames_for(per_call, depth="expected", **options):
        fr = SceneFrames("caller", lt, W, H, poses, depth, 0.25 if depth == "median" else None,
                         dict(frames_per_call=per_call, floater_thresh=0.5, **options), ("frames_per_call",), False)
        fr.check_per_call("call")
        assert fr.per_call == per_call
        return fr.on_device()

    for per_call in (1, n - 1, n, n + 3):
        for fi in (given, None):
            fr = frames_for(per_call, "median", **({} if fi is None else {"frame_indices": torch.tensor(fi)}))
            want_fi = novel_views.nearest_frames(lt, poses).tolist() if fi is None else fi
            assert fr.fi == want_fi and torch.equal(fr.cam, poses[:, :3]) and fr.focal == lt.focal(W)
            for kw in (dict(depth="expected", colour=False, encode=False), dict(depth="median", colour=True, encode=True),
                       dict(depth="median", colour=False, encode=False), dict()):
                del renders.calls[:], medians.calls[:]
                got = list(fr.batches(**kw))
                sizes = [p.shape[0] for p, _, _ in got]
                assert all(s >= 1 for s in sizes) and sum(sizes) == n and sizes == [min(per_call, n - i0) for i0 in range(0, n, per_call)]
                rendered = kw.get("colour", True) or kw.get("depth") == "expected"
                assert len(renders.calls) == (len(got) if rendered else 0)      # "median" without colour never renders colour
                assert len(medians.calls) == (len(got) if kw.get("depth") == "median" else 0)
                i0 = 0
                for k, (p, out, dmap) in enumerate(got):
                    i1 = i0 + p.shape[0]
                    assert torch.equal(p, poses[i0:i1, :3])
                    for rec, extra in ((renders, {"encode": kw.get("encode", True)}), (medians, {})):
                        if rec.calls:
                            seen, args, opts = rec.calls[k]
                            assert torch.equal(seen, poses[i0:i1, :3]) and opts == dict(frame_indices=want_fi[i0:i1], floater_thresh=0.5, **extra)
                            assert args == ((0.25,) if rec is medians else ())
                    assert out == ({"depth": ("depth", i1 - i0), "rgb8": ("rgb8", i1 - i0)} if rendered else None)
                    assert dmap == {None: None, "expected": ("depth", i1 - i0), "median": ("median", i1 - i0)}[kw.get("depth")]
                    i0 = i1
    with pytest.raises(ValueError, match=f"frame_indices holds {n - 1} entries for {n} poses"):
        frames_for(2, frame_indices=given[:-1])
    for bad in (True, np.True_, 0, 1.5, "3", None):
        with pytest.raises(ValueError, match="frames_per_call"):
            frames_for(bad)
    fr = SceneFrames("caller", lt, 1 << 15, 1 << 15, poses, "expected", None, dict(frames_per_call=2), ("frames_per_call",), False)
    with pytest.raises(ValueError, match="caller: 2 frames of 32768 x 32768 per call; one bake takes V H W < 2\\^31"):
        fr.check_per_call("bake")
    fr = SceneFrames("caller", lt, W, H, poses, "expected", None, {}, ("frames_per_call",), False)
    fr.check_per_call("bake")
    assert fr.per_call == 8                                                 # the default
    for fn in (lambda **kw: mesh.scene_mesh(lt, W, H, voxel=0.1, **kw), lambda **kw: mesh_raster.scene_mesh_agreement(lt, _cpu_mesh(), W, H, **kw),
               lambda **kw: mesh_texture.scene_texture(lt, _cpu_mesh(), W, H, **kw)):
        for bad in (True, np.True_, 0, 2.5):
            del renders.calls[:]
            with pytest.raises(ValueError, match="frames_per_call must be an integer >= 1"):
                fn(frames_per_call=bad)
            assert not renders.calls and not medians.calls


def test_the_device_comes_after_the_other_arguments():
    m = _cpu_mesh()
    poses = torch.eye(4)[None, :3].repeat(2, 1, 1)
    baker = mesh_texture.TextureBaker(m)                                    # host checks only: the CPU mesh is accepted here
    rgb = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    for call, bad, name in ((lambda **kw: mesh.simplify(m, **{"cell": 0.5, **kw}), dict(cell=-1.0), "cell"),
                            (lambda **kw: mesh.simplify(m, 0.5, **kw), dict(max_bytes=-1), "max_bytes"),
                            (lambda **kw: mesh.smooth(m, **kw), dict(lam=0.0), "lam"),
                            (lambda **kw: mesh.filter_components(m, **kw), dict(min_fraction=math.nan), "min_fraction"),
                            (lambda **kw: mesh_raster.rasterize(m, poses, 8, 6, 5.0, (4.0, 3.0), **kw), dict(small_max=-1), "small_max"),
                            (lambda **kw: baker.add(rgb, poses, 5.0, (4.0, 3.0), **kw), dict(max_bytes=True), "max_bytes"),
                            (lambda **kw: mesh_distance.sample_surface(m, **{"spacing": 0.1, **kw}), dict(spacing=0.0), "spacing"),
                            (lambda **kw: mesh_distance.MeshIndex(m, **kw), dict(max_bytes=1.5), "max_bytes")):
        with pytest.raises(ValueError, match=name):
            call(**bad)
        with pytest.raises(NativeError, match="vertices"):
            call()
    with pytest.raises(NativeError, match="vertices"):
        _checks.mesh_on_device(m["vertices"], m["faces"], None, "the test")
    pts = torch.zeros(8, 3)
    for call, bad, name in ((lambda **kw: cloud.CloudIndex(pts, **kw), dict(max_bytes=1.5), "max_bytes"),
                            (lambda **kw: alignment.transform_points(pts, **{"T": np.eye(4), **kw}), dict(T=np.zeros((3, 3))), "T must be"),
                            (lambda **kw: _StubMeshIndex().closest(pts, **kw), dict(max_distance=-1.0), "max_distance"),
                            (lambda **kw: _StubCloudIndex().knn(pts, **{"k": 2, **kw}), dict(k=9), "k must be")):
        with pytest.raises(ValueError, match=name):
            call(**bad)
        with pytest.raises(NativeError, match="points lives on cpu"):
            call()
    with pytest.raises(NativeError, match="colours lives on cpu; the test can run only on an AMD GPU"):
        _checks.points_on_device(torch.zeros(8, 3, dtype=torch.uint8), "colours", "the test")
    with pytest.raises(TypeError, match="colours"):
        _checks.points_on_device(None, "colours", "the test")
    lt, g = scene("cpu")
    W, H = float(g["W"]) + 0.5, float(g["H"])                              # SceneFrames takes int(W) first, as render_poses does
    for fn in (mesh_raster.scene_mesh_agreement, mesh_texture.scene_texture):
        with pytest.raises(ValueError, match="frames_per_call"):
            fn(lt, m, W, H, frames_per_call=0)
        with pytest.raises(NativeError, match="the scene"):
            fn(lt, m, W, H)
