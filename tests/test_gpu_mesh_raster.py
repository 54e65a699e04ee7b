"""The mesh rasteriser and the depth agreement on the MI355X (csrc/lrf_mesh_raster.inl through localrf_amd.mesh_raster): every
case of tests/mesh_raster_cases.py against the numpy restatement bit for bit, both tiers and the default threshold, face
permutations, reproducibility, a non-default stream, frames in one call or several, parity on the device output, the round trip
through a TsdfVolume, and scene_mesh_agreement."""
import functools
import math

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, mesh, mesh_raster, novel_views, pointcloud
from localrf_amd.mesh_raster import depth_agreement, rasterize, scene_mesh_agreement
from mesh_raster_cases import (AGREEMENT_SHAPES, AGREEMENT_TOLS, BOX_FACE, CASE_NAMES, SPHERE_KIND, agreement_host, agreement_maps,
                               cases, expected)
from mesh_util import DEV, device_mesh, to_dev
from novel_views_cases import scene

pytestmark = pytest.mark.gpu
MAPS = ("depth", "face", "rgb8", "weights", "crossings")
ALL_LARGE, ALL_SMALL = 0, (1 << 31) - 1


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = cases()[name]
    return device_mesh(c["mesh"]), to_dev(c["c2w"])


def _run(name, mesh_=None, poses=None, **over):
    c = cases()[name]
    dm, c2w = _device_case(name)
    kw = dict(depth_range=c["depth_range"], cull=c["cull"], crossings=True, weights=True)
    kw.update(over)
    return rasterize(dm if mesh_ is None else mesh_, c2w if poses is None else poses, c["W"], c["H"], float(c["f"]),
                     (float(c["cx"]), float(c["cy"])), **kw)


def _host(out):
    return {k: None if out[k] is None else out[k].cpu().numpy() for k in MAPS}


def _bytes(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    for k in MAPS:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if got[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(_bytes(got[k]), _bytes(want[k])), (what, k, int((_bytes(got[k]) != _bytes(want[k])).sum()))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bit_for_bit_with_the_restatement_in_both_tiers(name):
    want = expected(name)
    first = None
    for small_max in (None, ALL_LARGE, ALL_SMALL):
        out = _run(name, small_max=small_max)
        got = _host(out)
        _same(got, want, (name, small_max))
        assert out["info"] == want["info"]
        first = got if first is None else first
        _same(got, first, (name, small_max, "tiers"))


@pytest.mark.parametrize("n", sorted(BOX_FACE))
def test_boxes_on_the_threshold(n):
    name = f"box of {n} pixels"
    for small_max in (n - 1, n, n + 1):                                    # the face changes tier between n - 1 and n
        _same(_host(_run(name, small_max=small_max)), expected(name), (name, small_max))


@pytest.mark.parametrize("name", ("sphere 64x48 V5", "coincident faces", "fan 130x70 V3", "sphere ties"))
def test_a_face_permutation_keeps_the_depth_bytes(name):
    c = cases()[name]
    base = _host(_run(name))
    nf = c["mesh"]["faces"].shape[0]
    p = np.random.default_rng(77).permutation(nf)                           # new face k is old face p[k]
    dm = device_mesh(dict(c["mesh"], faces=c["mesh"]["faces"][p]))
    got = _host(_run(name, mesh_=dm))
    for k in ("depth", "crossings"):
        assert np.array_equal(_bytes(got[k]), _bytes(base[k])), (name, k)
    hit = base["face"] >= 0
    assert np.array_equal(got["face"] >= 0, hit)
    e = expected(name)
    assert np.array_equal(_bytes(base["depth"]), _bytes(e["depth"]))
    mapped = p[got["face"][hit]]
    unique = _unique_winner(name, hit)                                      # a tie in depth between two faces is not unique
    assert unique.sum() > 0.9 * unique.size or name == "coincident faces"
    assert np.array_equal(mapped[unique], base["face"][hit][unique]), name
    assert np.array_equal(got["rgb8"][hit][unique], base["rgb8"][hit][unique])


def _unique_winner(name, hit):
    """Per hit pixel of the case: only one face is kept at the winning depth (the restatement, every pair)."""
    from mesh_raster_cases import cover_host, depth_host, face_kinds, to_camera
    from points_cases import pixel_dirs
    c, e = cases()[name], expected(name)
    v, f = c["mesh"]["vertices"], c["mesh"]["faces"].astype(np.int64)
    ids = np.nonzero(face_kinds(c["mesh"]) == 0)[0]
    d = pixel_dirs(c["H"], c["W"], c["f"], c["cx"], c["cy"])
    out = np.zeros(hit.shape, np.int64)
    for fr in range(c["c2w"].shape[0]):
        q = to_camera(v[f[ids]], c["c2w"][fr])
        cov, _, U = cover_host(q, np.ascontiguousarray(d[0, :, 0]), np.ascontiguousarray(d[:, 0, 1]))
        t = depth_host(q, U)
        out[fr] = (cov & (t == e["depth"][fr][None])).sum(0)
    return out[hit] == 1


def test_two_runs_a_side_stream_and_split_frames_give_the_same_bytes():
    for name in ("fan 130x70 V3", "sphere 64x48 V5"):
        c = cases()[name]
        base = _host(_run(name))
        _same(_host(_run(name)), base, (name, "again"))
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            out = _run(name)
        side.synchronize()
        _same(_host(out), base, (name, "side stream"))
        _, c2w = _device_case(name)
        V = c2w.shape[0]
        parts = [_host(_run(name, poses=c2w[i:i + 1])) for i in range(V)]
        joined = {k: None if base[k] is None else np.concatenate([p[k] for p in parts]) for k in MAPS}
        _same(joined, base, (name, "one frame per call"))
        nf = c["mesh"]["faces"].shape[0]
        one_frame = 8 * c["H"] * c["W"] + 8 * nf + 8
        assert mesh_raster.frames_per_call(c["W"], c["H"], nf, one_frame) == 1
        _same(_host(_run(name, max_bytes=one_frame)), base, (name, "batched under max_bytes"))
        plain = _run(name, crossings=False, weights=False)
        assert plain["weights"] is None and plain["crossings"] is None
        assert np.array_equal(_bytes(plain["depth"].cpu().numpy()), _bytes(base["depth"]))


def test_parity_on_the_device_output():
    out = _host(_run("sphere 64x48 V5"))
    for fr, kind in enumerate(SPHERE_KIND):
        cr, face = out["crossings"][fr], out["face"][fr]
        if kind == "outside":
            assert (cr % 2 == 0).all() and ((cr > 0) == (face >= 0)).all()
        elif kind == "inside":
            assert (cr % 2 == 1).all() and (face >= 0).all()
    ties = _host(_run("sphere ties"))
    assert (ties["crossings"] == 1).all() and (ties["face"] >= 0).all()


def test_refusals_on_the_device_and_a_mesh_without_colours():
    dm, c2w = _device_case("coincident faces")
    c = cases()["coincident faces"]
    args = (c["W"], c["H"], float(c["f"]), (float(c["cx"]), float(c["cy"])))
    with pytest.raises(NativeError, match="rgb8"):
        rasterize(dict(dm, rgb8=dm["rgb8"].cpu()), c2w, *args)
    out = rasterize(dict(dm, rgb8=None), c2w, *args)
    assert out["rgb8"] is None and out["weights"] is None and out["crossings"] is None
    assert np.array_equal(_bytes(out["depth"].cpu().numpy()), _bytes(expected("coincident faces")["depth"]))


@pytest.mark.parametrize("shape", AGREEMENT_SHAPES)
def test_depth_agreement_integers_equal_the_restatement(shape):
    a, b = agreement_maps(40 + shape[1], *shape)
    rng = (0.6, 30.0)
    words, err = agreement_host(a, b, AGREEMENT_TOLS, rng)
    got = depth_agreement(to_dev(a), to_dev(b), rel_tols=AGREEMENT_TOLS, depth_range=rng, error_map=True)
    pf = got["per_frame"]
    for k, col in (("both", 0), ("mesh_only", 1), ("render_only", 2), ("neither", 3), ("error_sum", 4)):
        assert np.array_equal(pf[k], words[:, col]), k
        assert got[k] == int(words[:, col].sum())
    assert np.array_equal(pf["within"], words[:, 8:8 + len(AGREEMENT_TOLS)])
    assert got["within"] == tuple(int(x) for x in words[:, 8:8 + len(AGREEMENT_TOLS)].sum(0)) and got["frames"] == shape[0]
    assert np.array_equal(_bytes(got["error_map"].cpu().numpy()), _bytes(err))
    if got["both"]:
        assert got["mean_rel_error"] == got["error_sum"] / (1 << 24) / got["both"]
    again = depth_agreement(to_dev(a), to_dev(b), rel_tols=AGREEMENT_TOLS, depth_range=rng)
    assert "error_map" not in again and again["error_sum"] == got["error_sum"] and again["within"] == got["within"]
    none = depth_agreement(to_dev(a), to_dev(b), rel_tols=())
    assert none["within"] == () and none["both"] + none["mesh_only"] + none["render_only"] + none["neither"] == a.size


# ------------------------------------------------------------------------------------------------ the round trip
RT_H, RT_W, RT_FOCAL, RT_N, RT_V = 48, 64, 50.0, 32, 8


def _wall_frames():
    """scripts/mesh_probe.py's scene at 48 x 64: cameras on an arc around (0, 0, -3), a sphere of radius 0.8 there, the wall
    z = -4.5 behind it; depth by exact ray casting in fp64."""
    V, H, W = RT_V, RT_H, RT_W
    c2w = np.zeros((V, 3, 4), np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dirs = np.stack([(col + 0.5 - W / 2) / RT_FOCAL, -(row + 0.5 - H / 2) / RT_FOCAL, -np.ones_like(col)], -1)
    depth = np.zeros((V, H, W), np.float32)
    for k in range(V):
        a = 0.6 * (k / (V - 1) - 0.5)
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        o = np.array([0.0, 0.0, -3.0]) + R @ np.array([0.0, 0.0, 3.0])
        c2w[k, :, :3], c2w[k, :, 3] = R, o
        dw = dirs @ R.T
        oc = o - np.array([0.0, 0.0, -3.0])
        A, B, Cc = (dw * dw).sum(-1), 2 * (dw * oc).sum(-1), (oc * oc).sum() - 0.64
        disc = B * B - 4 * A * Cc
        t_s = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        t_w = (-4.5 - o[2]) / dw[..., 2]
        depth[k] = np.minimum(np.where(t_s > 0, t_s, np.inf), np.where(t_w > 0, t_w, np.inf))
    return depth, c2w.astype(np.float32)


def test_round_trip_through_a_volume_stays_within_one_voxel():
    """integrate -> extract -> rasterize at the integration poses: at every pixel valid in both maps and more than two pixels
    from a depth discontinuity of the input (a step of more than one voxel between neighbouring pixels) the mesh's depth is
    within one voxel of the input: the trilinear zero crossing lies inside its cell."""
    depth, c2w = _wall_frames()
    voxel = 3.4 / (RT_N - 1)
    vol = mesh.TsdfVolume((-1.7, -1.7, -4.7), voxel, (RT_N,) * 3, 3 * voxel, DEV, colours=False)
    centre = (RT_W / 2, RT_H / 2)
    vol.integrate(to_dev(depth), to_dev(c2w), RT_FOCAL, centre)
    m = vol.extract()
    assert m["counts"][1] > 1000
    out = rasterize(m, to_dev(c2w), RT_W, RT_H, RT_FOCAL, centre, crossings=True)
    got = out["depth"].cpu().numpy()
    assert out["info"] == {"bad_index_faces": 0, "degenerate_faces": 0, "nonfinite_faces": 0}
    step = np.zeros(depth.shape, bool)
    for dj, di in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = depth[:, dj:, max(di, 0):RT_W + min(di, 0)]
        b = depth[:, :RT_H - dj, max(-di, 0):RT_W - max(di, 0)]
        jump = np.abs(a - b) > voxel
        step[:, dj:, max(di, 0):RT_W + min(di, 0)] |= jump
        step[:, :RT_H - dj, max(-di, 0):RT_W - max(di, 0)] |= jump
    near = np.zeros_like(step)
    for dj in range(-2, 3):
        for di in range(-2, 3):
            src = step[:, max(dj, 0):RT_H + min(dj, 0), max(di, 0):RT_W + min(di, 0)]
            near[:, max(-dj, 0):RT_H - max(dj, 0), max(-di, 0):RT_W - max(di, 0)] |= src
    both = (got > 0) & np.isfinite(depth) & (depth > 0)
    judged = both & ~near
    diff = np.abs(got - depth)
    print(f"round trip: mesh {m['counts']}, voxel {voxel:.4f}, both-valid {int(both.sum())}, judged {int(judged.sum())}, "
          f"largest difference {diff[judged].max() / voxel:.3f} voxels, mean {diff[judged].mean() / voxel:.3f} voxels")
    assert both.sum() > 0.25 * depth.size and judged.sum() > 0.25 * both.sum()   # the mesh fills part of the image; it is judged
    assert (diff[judged] <= voxel).all(), float(diff[judged].max() / voxel)


# ------------------------------------------------------------------------------------------------ the scene
def _scene_box(lt, W, H, own):
    out = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(len(lt.r_c2w))), floater_thresh=0.5)
    xyz = pointcloud.fuse_points(None, out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=(0.05, 50.0))["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 28
    return out, dict(voxel=voxel, bounds=(tuple(lo - 3 * voxel), tuple(hi + 3 * voxel)), floater_thresh=0.5, depth_range=(0.05, 50.0))


def test_scene_mesh_agreement_equals_rasterize_and_depth_agreement_over_render_poses():
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    rendered, kw = _scene_box(lt, W, H, own)
    rng, tols = kw["depth_range"], (0.01, 0.05, 0.2)
    for label, extra in (("raw", {}), ("simplify_cell = 2 voxels", {"simplify_cell": 2 * kw["voxel"]})):
        m = mesh.scene_mesh(lt, W, H, **extra, **kw)
        ras = rasterize(m, own, W, H, lt.focal(W), lt.center(W, H), depth_range=rng)
        want = depth_agreement(ras["depth"], rendered["depth"], rel_tols=tols, depth_range=rng)
        for per_call in (8, 3):
            got = scene_mesh_agreement(lt, m, W, H, floater_thresh=0.5, depth_range=rng, rel_tols=tols, frames_per_call=per_call)
            assert got["info"] == ras["info"] and got["frames"] == own.shape[0]
            for k in ("both", "mesh_only", "render_only", "neither", "within", "error_sum", "mean_rel_error", "rel_tols"):
                assert got[k] == want[k] or (k == "mean_rel_error" and math.isnan(got[k]) and math.isnan(want[k])), (label, k, got[k], want[k])
        assert "per_frame" not in got and got["both"] > 0
        print(f"scene_mesh_agreement, {label}: mesh {m['counts']}, both {got['both']}, mesh_only {got['mesh_only']}, render_only "
              f"{got['render_only']}, neither {got['neither']}, within {dict(zip(tols, got['within']))}, mean relative error "
              f"{got['mean_rel_error']:.5f}")
    median = scene_mesh_agreement(lt, m, W, H, depth="median", floater_thresh=0.5, depth_range=rng, rel_tols=tols)
    assert median["both"] + median["mesh_only"] + median["render_only"] + median["neither"] == own.shape[0] * H * W
