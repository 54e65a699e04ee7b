"""The texture bake on the MI355X (csrc/lrf_mesh_texture.inl through localrf_amd.mesh_texture): every case of
tests/mesh_texture_cases.py against the numpy restatement bit for bit, frames in one call or several, a side stream,
reproducibility, the rasterisation done inside add(), frame permutations under "best", float frames, scene_texture against its
parts, refusals on the device and the empty mesh."""
import functools

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, mesh, mesh_raster, novel_views, pointcloud
from localrf_amd.mesh_raster import rasterize
from localrf_amd.mesh_texture import INFO_KEYS, TextureBaker, sample_texture, scene_texture
from mesh_texture_cases import CASE_NAMES, cases, expected, inputs
from mesh_util import DEV, device_mesh, to_dev
from novel_views_cases import scene

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = cases()[name]
    m = c["mesh"]
    frames, depth = inputs(name)
    return device_mesh(m), to_dev(frames), to_dev(depth), to_dev(c["c2w"])


def _baker(name, **over):
    c = cases()[name]
    kw = dict(patch=c["P"], cols=c["cols"], blend=c["blend"], vis_tol=c["vis_tol"], min_cos=c["min_cos"], two_sided=c["two_sided"])
    kw.update(over)
    return TextureBaker(_device_case(name)[0], **kw)


def _add(baker, name, ids=None, depth=True, **kw):
    c = cases()[name]
    _, frames, dm, c2w = _device_case(name)
    ids = slice(None) if ids is None else ids
    return baker.add(frames[ids], c2w[ids], float(c["f"]), (float(c["cx"]), float(c["cy"])), dm[ids] if depth else None, **kw)


def _words(state):
    return np.ascontiguousarray(state.cpu().numpy()).view(np.uint32)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bit_for_bit_with_the_restatement(name):
    c, want = cases()[name], expected(name)
    baker = _add(_baker(name), name)
    assert np.array_equal(_words(baker.state), want["state"].view(np.uint32)), int((_words(baker.state) != want["state"].view(np.uint32)).sum())
    out = baker.finish(fill=c["fill"])
    for k in ("atlas", "mask"):
        got = out[k].cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == want[k].shape and np.array_equal(got, want[k]), (name, k)
    assert np.array_equal(out["uv"].cpu().numpy().view(np.uint32), want["uv"].view(np.uint32))
    assert out["info"] == want["info"] and tuple(out["info"]) == INFO_KEYS
    assert baker.frames == c["c2w"].shape[0] and (out["patch"], out["cols"]) == (c["P"], baker.cols)


@pytest.mark.parametrize("name", ("wall P8 mean", "wall P8 best", "sphere P8 mean", "fan P5 cols 4 V3 best"))
def test_split_frames_small_batches_a_side_stream_and_two_runs_give_the_same_bytes(name):
    c = cases()[name]
    V, nf = c["c2w"].shape[0], c["mesh"]["faces"].shape[0]
    base = _words(_add(_baker(name), name).state)
    assert np.array_equal(_words(_add(_baker(name), name).state), base), "again"
    one = _baker(name)
    for v in range(V):
        _add(one, name, slice(v, v + 1))
    assert np.array_equal(_words(one.state), base), "one frame per call"
    one_frame = 8 * c["H"] * c["W"] + 8 * nf + 8
    assert mesh_raster.frames_per_call(c["W"], c["H"], nf, one_frame) == 1
    assert np.array_equal(_words(_add(_baker(name), name, max_bytes=one_frame).state), base), "batched under max_bytes"
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = _add(_baker(name), name)
        atlas = on_side.finish()["atlas"]
    side.synchronize()
    assert np.array_equal(_words(on_side.state), base), "side stream"
    assert np.array_equal(atlas.cpu().numpy(), expected(name)["atlas"])


@pytest.mark.parametrize("name", ("wall P8 mean", "sphere P16 cols 7 best two-sided", "triangle from behind two_sided False"))
def test_rasterising_inside_add_equals_passing_the_depth(name):
    base = _words(_add(_baker(name), name).state)
    assert np.array_equal(_words(_add(_baker(name), name, depth=False).state), base)
    assert np.array_equal(_words(_add(_baker(name), name, depth=False, max_bytes=8 * 48 * 64 + 8 * 600 + 8).state), base)


def test_float_frames_are_encoded_as_encode_frames_does():
    name = "wall P8 mean"
    c = cases()[name]
    _, frames, dm, c2w = _device_case(name)
    got = _baker(name).add(frames.float() / 255.0, c2w, float(c["f"]), (float(c["cx"]), float(c["cy"])), dm)
    assert np.array_equal(_words(got.state), expected(name)["state"].view(np.uint32))


def test_a_frame_permutation_keeps_the_best_atlas_where_no_two_weights_tie():
    name = "wall P8 best"
    base = _add(_baker(name), name)
    perm = _baker(name)
    for v in (2, 0, 1):
        _add(perm, name, slice(v, v + 1))
    a, b = base.state.cpu().numpy(), perm.state.cpu().numpy()
    single = [_add(_baker(name), name, slice(v, v + 1)).state.cpu().numpy()[..., 3] for v in range(3)]
    w = np.sort(np.stack(single), 0)
    untied = w[2] != w[1]                                                  # the largest weight is held by one frame alone
    assert untied.sum() > 0.3 * untied.size and np.array_equal(a[untied].view(np.uint32), b[untied].view(np.uint32))
    assert np.array_equal(base.finish()["mask"].cpu().numpy(), perm.finish()["mask"].cpu().numpy())


def test_sample_texture_on_the_device_equals_the_host_lookup():
    name = "wall P8 mean"
    c = cases()[name]
    dm, _, _, c2w = _device_case(name)
    tex = _add(_baker(name), name).finish()
    ras = rasterize(dm, c2w, c["W"], c["H"], float(c["f"]), (float(c["cx"]), float(c["cy"])), cull="back", weights=True)
    got = sample_texture(ras, tex)
    host = sample_texture({"face": ras["face"].cpu(), "weights": ras["weights"].cpu()}, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in tex.items()})
    assert got.dtype is torch.uint8 and tuple(got.shape) == (3, c["H"], c["W"], 3) and np.array_equal(got.cpu().numpy(), host.numpy())
    assert not got[ras["face"] < 0].any() and got[ras["face"] >= 0].any()


def test_refusals_on_the_device_and_an_empty_mesh():
    name = "Nf 3 5x7 P8 V3 mean"
    c = cases()[name]
    dm, frames, depth, c2w = _device_case(name)
    args = (float(c["f"]), (float(c["cx"]), float(c["cy"])))
    with pytest.raises(NativeError, match="rgb8"):
        TextureBaker(dict(dm, rgb8=dm["rgb8"].cpu())).add(frames, c2w, *args, depth)
    with pytest.raises(NativeError, match="rgb"):
        TextureBaker(dm).add(frames.cpu(), c2w, *args, depth)
    with pytest.raises(NativeError, match="mesh_depth"):
        TextureBaker(dm).add(frames, c2w, *args, depth.cpu())
    empty = {"vertices": torch.zeros(0, 3, device=DEV), "faces": torch.zeros(0, 3, dtype=torch.int32, device=DEV), "rgb8": None}
    baker = TextureBaker(empty, patch=5)
    out = baker.add(frames, c2w, *args).finish(fill=(1, 2, 3))
    assert tuple(out["atlas"].shape) == (0, 5, 3) and tuple(out["mask"].shape) == (0, 5) and tuple(out["uv"].shape) == (0, 3, 2)
    assert tuple(baker.state.shape) == (0, 5, 4) and not any(out["info"].values())


def test_scene_texture_equals_render_rasterize_and_bake_over_the_same_tensors():
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    rendered = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(len(lt.r_c2w))), floater_thresh=0.5)
    xyz = pointcloud.fuse_points(None, rendered["depth"], own, lt.focal(W), lt.center(W, H), depth_range=(0.05, 50.0))["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 28
    m = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=(tuple(lo - 3 * voxel), tuple(hi + 3 * voxel)), floater_thresh=0.5,
                        depth_range=(0.05, 50.0), simplify_cell=2 * voxel)
    rng = (0.05, 50.0)
    for blend in ("mean", "best"):
        kw = dict(patch=5, blend=blend, vis_tol=0.05)
        ras = rasterize({"vertices": m["vertices"], "faces": m["faces"], "rgb8": None}, own, W, H, lt.focal(W), lt.center(W, H),
                        depth_range=rng, cull="back")
        baker = TextureBaker(m, **kw).add(rendered["rgb8"], own, lt.focal(W), lt.center(W, H), ras["depth"])
        want = baker.finish(fill=(7, 8, 9))
        for per_call in (8, 3):
            got = scene_texture(lt, m, W, H, floater_thresh=0.5, depth_range=rng, frames_per_call=per_call, fill=(7, 8, 9), **kw)
            assert got["frames"] == own.shape[0] and got["info"] == want["info"]
            for k in ("atlas", "mask", "uv"):
                assert torch.equal(got[k], want[k]), (blend, per_call, k)
        print(f"scene_texture, {blend}: mesh {m['counts']}, atlas {tuple(want['atlas'].shape)}, {want['info']}")
    assert want["info"]["observed_texels"] > 0
