"""TSDF fusion and mesh extraction on the MI355X (csrc/lrf_mesh.inl through localrf_amd.mesh): both kernels against the numpy
restatement of tests/mesh_cases.py bit for bit, chunked integration, reproducibility, a non-default stream, capacity handling
and scene_mesh against TsdfVolume.integrate + extract over render_poses' own tensors."""
import functools

import numpy as np
import pytest
import torch

from localrf_amd import mesh, novel_views, pointcloud
from mesh_cases import (H_ANALYTIC, closed_manifold_euler, extract_host, integrate_host, new_volume, sphere_field)
from mesh_util import DEV, blob_volumes, forbid_render, record_launches, same_device_mesh, same_mesh, to_dev
from novel_views_cases import scene
from points_cases import random_case, trajectory_case

pytestmark = pytest.mark.gpu
VOLUMES = [(1, 1, 1), (2, 2, 2), (3, 5, 4), (17, 23, 9), (33, 33, 33), (70, 3, 2)]
CENTRE = np.array([0.1, -0.05, -3.05])


@functools.lru_cache(maxsize=None)
def frame_cases():
    """(name, case, depth ranges): trajectory_case and random_case at V = 1, 3, 7, 17 x 23 and 48 x 64.  The last frame of the
    random cases with V >= 3 stands inside the volumes, turned 2 rad about y: some lattice points fall behind it."""
    out = [("trajectory", trajectory_case(), ((0.0, np.inf), (3.0, 3.9)))]
    for V in (1, 3, 7):
        for H, W in ((17, 23), (48, 64)):
            c = random_case(1000 * V + H, V, H, W)
            if V >= 3:
                a = 2.0
                c["c2w"][-1] = np.array([[np.cos(a), 0, np.sin(a), 0.0], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), -3.0]], np.float32)
            out.append((f"random V={V} {H}x{W}", c, (c["depth_range"], (2.8, 3.3))))
    return out


def _lattice_for(dims):
    voxel = 1.7 / max(max(dims) - 1, 1)
    origin = CENTRE - (np.array(dims) - 1) / 2 * voxel
    return tuple(float(v) for v in origin), float(voxel), 3 * float(voxel)


def _integrate_device(dims, case, rng, colours=True, split=None):
    origin, voxel, trunc = _lattice_for(dims)
    vol = mesh.TsdfVolume(origin, voxel, dims, trunc, DEV, colours=colours)
    d, r, p = to_dev(case["depth"]), to_dev(case["rgb8"]) if colours else None, to_dev(case["c2w"])
    f, c = float(case["f"]), (float(case["cx"]), float(case["cy"]))
    V = d.shape[0]
    for i0, i1 in ((0, V),) if split is None else ((0, split), (split, V)):
        vol.integrate(d[i0:i1], p[i0:i1], f, c, rgb=None if r is None else r[i0:i1], depth_range=rng)
    return vol


def _integrate_host(dims, case, rng, colours=True):
    origin, voxel, trunc = _lattice_for(dims)
    return integrate_host(new_volume(dims, colours), origin, voxel, trunc, case["depth"], case["rgb8"] if colours else None,
                          case["c2w"], case["f"], case["cx"], case["cy"], depth_range=rng)


def _same_volume(vol, want):
    for k in ("tsdf", "weight", "rgb"):
        got = getattr(vol, k)
        if want[k] is None:
            assert got is None
            continue
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k


def _extract_both(vol, host, **kw):
    origin, voxel, _ = _lattice_for(vol.dims)
    got = vol.extract(**kw)
    want = extract_host(host["tsdf"], origin, voxel, level=kw.get("level", 0.0), weight=host["weight"], rgb=host["rgb"],
                        min_weight=kw.get("min_weight", 1.0))
    same_mesh(got, want)
    return want["counts"]


@pytest.mark.parametrize("dims", VOLUMES)
def test_integrate_and_extract_equal_the_restatement_bit_for_bit(dims):
    seen = unseen = faces = 0
    for name, case, ranges in frame_cases():
        for k, rng in enumerate(ranges):
            colours = k == 0
            vol = _integrate_device(dims, case, rng, colours)
            want = _integrate_host(dims, case, rng, colours)
            _same_volume(vol, want)
            seen += int((want["weight"] > 0).sum())
            unseen += int((want["weight"] < case["depth"].shape[0]).sum())
            counts = [_extract_both(vol, want), _extract_both(vol, want, level=0.1, min_weight=2.0)]
            # without weights every cell counts: the unobserved ones too, at tsdf = 1
            origin, voxel, _ = _lattice_for(dims)
            bare = mesh.extract_mesh(vol.tsdf, origin, voxel, 0.1)
            same_mesh(bare, extract_host(want["tsdf"], origin, voxel, level=0.1))
            print(f"{dims} {name} range {rng}: seen {int((want['weight'] > 0).sum())}, meshes {counts} {bare['counts']}")
            faces += counts[0][1]
    if dims == (1, 1, 1):
        assert faces == 0                                               # no cell: no face, and no launch fault
    else:
        assert seen > 0 and unseen > 0                                  # frames see points, and the filters skip some
    if min(dims) >= 9:
        assert faces > 0


def test_extract_the_analytic_sphere_with_holes_levels_and_colours():
    fld = sphere_field()
    rng = np.random.default_rng(4)
    rgb = rng.uniform(-0.1, 1.1, fld.shape + (3,)).astype(np.float32)
    w = rng.integers(0, 4, fld.shape).astype(np.float32)
    w[:, :, :12] = 3
    o = (0.0, 0.0, 0.0)
    got = mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, 0.0)
    same_mesh(got, extract_host(fld, o, H_ANALYTIC))
    assert closed_manifold_euler({"vertices": got["vertices"].cpu().numpy(), "faces": got["faces"].cpu().numpy()}) == 2
    for level, mw in ((0.0, 1.0), (0.05, 2.0), (-0.02, 3.0)):
        got = mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, level, weight=to_dev(w), rgb=to_dev(rgb), min_weight=mw)
        want = extract_host(fld, o, H_ANALYTIC, level=level, weight=w, rgb=rgb, min_weight=mw)
        same_mesh(got, want)
        assert 0 < want["counts"][1]
    one = mesh.extract_mesh(torch.zeros(1, 1, 1, device=DEV), o, 1.0, 0.5)
    assert one["counts"] == (0, 0) and tuple(one["faces"].shape) == (0, 3)
    line = mesh.extract_mesh(to_dev(np.linspace(-1, 1, 300, dtype=np.float32).reshape(1, 1, 300)), o, 1.0, 0.0)
    assert line["counts"] == (0, 0)                                     # crossings, but no cell contains them


def test_chunked_integration_equals_one_shot():
    name, case, ranges = frame_cases()[-1]                              # V = 7, 48 x 64, with the turned frame
    for dims in ((17, 23, 9), (70, 3, 2)):
        whole = _integrate_device(dims, case, ranges[0])
        assert float(whole.weight.max()) > 1
        for k in (1, 3, 6):
            part = _integrate_device(dims, case, ranges[0], split=k)
            for a, b in ((whole.tsdf, part.tsdf), (whole.weight, part.weight), (whole.rgb, part.rgb)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (dims, k)


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    case = trajectory_case()
    dims = (33, 33, 33)
    a, b = _integrate_device(dims, case, (0.0, np.inf)), _integrate_device(dims, case, (0.0, np.inf))
    ma, mb = a.extract(), b.extract()
    assert ma["counts"] == mb["counts"] and ma["counts"][1] > 0
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = _integrate_device(dims, case, (0.0, np.inf))
        mc = c.extract()
    side.synchronize()
    for other, mo in ((b, mb), (c, mc)):
        for k in ("tsdf", "weight", "rgb"):
            assert torch.equal(getattr(a, k).view(torch.int32), getattr(other, k).view(torch.int32)), k
        assert mo["counts"] == ma["counts"]
        assert torch.equal(ma["vertices"].view(torch.int32), mo["vertices"].view(torch.int32))
        assert torch.equal(ma["faces"], mo["faces"]) and torch.equal(ma["rgb8"], mo["rgb8"])


def test_capacity_one_too_small_raises_with_the_true_counts():
    fld = sphere_field()
    o = (0.0, 0.0, 0.0)
    want = extract_host(fld, o, H_ANALYTIC)
    nv, nf = want["counts"]
    same_mesh(mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, 0.0, max_vertices=nv, max_faces=nf), want)
    same_mesh(mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, 0.0, max_vertices=nv + 100, max_faces=None), want)
    for cap_v, cap_f in ((nv - 1, nf), (nv, nf - 1), (5, 7), (0, 0)):
        with pytest.raises(ValueError, match=f"holds {nv} vertices and {nf} faces") as ei:
            mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, 0.0, max_vertices=cap_v, max_faces=cap_f)
        part = ei.value.partial                                         # the rows inside capacity are the mesh's first rows
        assert part["counts"] == (nv, nf)
        assert np.array_equal(part["vertices"].cpu().numpy().view(np.uint32), want["vertices"][:cap_v].view(np.uint32))
        assert np.array_equal(part["faces"].cpu().numpy(), want["faces"][:cap_f])


SCENE_RANGE = (0.05, 50.0)


@functools.lru_cache(maxsize=None)
def _scene_and_box():
    """scene(DEV), its own poses, render_poses of them, and the box of fuse_points over that depth with voxel = extent / 28."""
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    out = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(len(lt.r_c2w))), floater_thresh=0.5)
    xyz = pointcloud.fuse_points(None, out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=SCENE_RANGE)["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    return lt, g, W, H, own, out, lo, hi, float((hi - lo).max()) / 28


def test_scene_mesh_equals_integrate_and_extract_over_render_poses(monkeypatch):
    lt, g, W, H, own, out, lo, hi, voxel = _scene_and_box()
    rng = SCENE_RANGE
    got = mesh.scene_mesh(lt, W, H, voxel=voxel, floater_thresh=0.5, depth_range=rng, frames_per_call=2)
    vol = got["volume"]
    assert vol.trunc == 3 * voxel
    assert np.allclose(vol.origin, lo - vol.trunc, rtol=0, atol=1e-12)  # the box of fuse_points, grown by trunc
    top = np.array(vol.origin) + (np.array(vol.dims) - 1) * voxel
    assert (top >= hi + vol.trunc - 1e-9).all() and (top < hi + vol.trunc + voxel).all()
    ref = mesh.TsdfVolume(vol.origin, voxel, vol.dims, vol.trunc, DEV)
    ref.integrate(out["depth"], own, lt.focal(W), lt.center(W, H), rgb=out["rgb8"], depth_range=rng)
    for k in ("tsdf", "weight", "rgb"):
        assert torch.equal(getattr(vol, k).view(torch.int32), getattr(ref, k).view(torch.int32)), k
    want = ref.extract()
    print(f"scene_mesh: volume {vol.dims}, {got['counts']} vertices / faces")
    assert got["counts"] == want["counts"] and got["counts"][0] > 0 and got["counts"][1] > 0
    for k in ("vertices", "faces", "rgb8"):
        assert torch.equal(got[k], want[k]), k
    # explicit bounds and poses, no colours
    poses = torch.from_numpy(g["poses"]).to(DEV)
    box = (tuple(lo), tuple(hi))
    got = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=box, poses=poses, floater_thresh=0.5, colours=False, min_weight=2.0)
    out = novel_views.render_poses(lt, poses, W, H, floater_thresh=0.5)
    ref = mesh.TsdfVolume(got["volume"].origin, voxel, got["volume"].dims, 3 * voxel, DEV, colours=False)
    ref.integrate(out["depth"], poses, lt.focal(W), lt.center(W, H))
    want = ref.extract(min_weight=2.0)
    assert got["volume"].origin == tuple(lo) and got["rgb8"] is None and got["counts"] == want["counts"]
    assert torch.equal(got["vertices"], want["vertices"]) and torch.equal(got["faces"], want["faces"])
    forbid_render(monkeypatch)
    with pytest.raises(ValueError, match="max_bytes"):
        mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=box, max_bytes=1000)


@pytest.mark.parametrize("kind", [dict(depth="expected"), dict(sparse=True, depth="median")], ids=["dense expected", "sparse median"])
def test_scene_mesh_does_not_depend_on_frames_per_call(kind):
    """The same volume bits and mesh bytes whether the scene's 14 frames are rendered 1, 3 or (the default) 8 at a time."""
    lt, g, W, H, own, out, lo, hi, voxel = _scene_and_box()
    assert own.shape[0] % 3 and 8 < own.shape[0] < 16                   # batches of 1; of 3 and of 8, each with a shorter last one
    box = (tuple(lo - 3 * voxel), tuple(hi + 3 * voxel))
    want = None
    for extra in ({}, {"frames_per_call": 3}, {"frames_per_call": 1}):
        got = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=box, floater_thresh=0.5, depth_range=SCENE_RANGE, **kind, **extra)
        assert got["counts"][0] > 0 and got["counts"][1] > 0
        if want is None:
            want = got
            continue
        assert got["counts"] == want["counts"], extra
        for k in ("tsdf", "weight", "rgb"):
            assert torch.equal(getattr(got["volume"], k).view(torch.int32), getattr(want["volume"], k).view(torch.int32)), (extra, k)
        for k in ("vertices", "faces", "rgb8"):
            assert torch.equal(got[k], want[k]), (extra, k)
        if kind.get("sparse"):
            assert torch.equal(got["volume"].coords, want["volume"].coords) and torch.equal(got["volume"].table, want["volume"].table)


ROUND = "lrf_mesh_components_round"


def _launches_of(names, info):
    """The recorded symbol names with every run of component rounds as one entry.  How many rounds the labels take depends on
    the scheduling of the hooks (csrc/lrf_mesh_clean.inl), so two runs may differ in that number and in nothing else: each
    run's own count is checked against the rounds it reports."""
    assert names.count(ROUND) == info["rounds"]
    return [n for k, n in enumerate(names) if n != ROUND or names[k - 1] != ROUND]


@pytest.mark.parametrize("which", ("dense", "sparse"))
def test_every_chain_option_at_once_equals_the_five_calls_by_hand(which, monkeypatch):
    """extract with all six options on is filter_components, fill_holes, simplify at the volume's origin, smooth and
    vertex_normals of extract(), in that order: the same bytes from the same launches."""
    vol = blob_volumes()[which == "sparse"]
    cell = 2 * H_ANALYTIC
    names = record_launches(monkeypatch)
    got = vol.extract(min_component_faces=1, min_component_fraction=0.03, fill_holes=64, simplify_cell=cell, smooth_iterations=2,
                      normals=True)
    chain = list(names)
    del names[:]
    plain = vol.extract()
    kept = mesh.filter_components(plain, 1, 0.03)
    want = mesh.vertex_normals(mesh.smooth(mesh.simplify(mesh.fill_holes(kept, 64), cell, origin=vol.origin), 2))
    assert plain["counts"] == (2902, 5780) and kept["components"]["kept"] == 5 and kept["counts"][1] == 5780 - 88
    assert 0 < want["counts"][1] < kept["counts"][1] and want["simplify"]["occupied"] > 1
    print(f"{which}: {plain['counts']} -> {got['counts']}, {len(chain)} launches, rounds {got['components']['rounds']}")
    same_device_mesh(got, want)
    assert set(got) == set(want) == {"vertices", "faces", "rgb8", "counts", "components", "fill", "simplify", "smooth", "normals", "normal_info"}
    assert got["fill"] == want["fill"] and got["simplify"] == want["simplify"]
    assert got["components"] == dict(want["components"], rounds=got["components"]["rounds"])
    assert _launches_of(chain, got["components"]) == _launches_of(names, want["components"])


def test_a_sparse_volume_without_blocks_gives_the_empty_mesh_to_smooth_and_normals_only(monkeypatch):
    """smooth and vertex_normals of an empty mesh return before their first launch, so the chain launches nothing at all; the
    component filter and the fill, asked for as well, leave no entry in the result."""
    vol = mesh.SparseTsdfVolume((0.0, 0.0, 0.0), H_ANALYTIC, (3, 3, 3), 3 * H_ANALYTIC, DEV)
    names = record_launches(monkeypatch)
    got = vol.extract(smooth_iterations=2, normals=True, fill_holes=64, min_component_faces=5)
    assert names == []
    want = mesh.vertex_normals(mesh.smooth(vol.extract(), 2))
    assert names == []
    assert got["counts"] == (0, 0) and tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3)
    assert tuple(got["rgb8"].shape) == (0, 3) and tuple(got["normals"].shape) == (0, 3)
    assert set(got) == set(want) == {"vertices", "faces", "rgb8", "counts", "smooth", "normals", "normal_info"}
    same_device_mesh(got, want)
    assert got["smooth"]["iterations"] == 2 and got["normal_info"] == {"zero_normals": 0, "degenerate_faces": 0}
