"""Mesh simplification on the MI355X (csrc/lrf_mesh_simplify.inl through localrf_amd.mesh.simplify): every case of
tests/mesh_simplify_cases.py against the numpy restatement, bit for bit -- no tolerance anywhere --, permuted inputs,
reproducibility, a non-default stream, bad vertices and face indices, the workspace limit, and the extract options."""

import numpy as np
import pytest
import torch

from localrf_amd import _native, mesh, novel_views, pointcloud
from mesh_cases import H_ANALYTIC
from mesh_simplify_cases import CASE_NAMES, cases, expected_simplified
from mesh_util import DEV, blob_volumes, device_mesh, record_launches, same_device_mesh, to_dev
from novel_views_cases import scene

pytestmark = pytest.mark.gpu


def _same_as_host(got, want, cell, origin):
    """Counts, box, vertices (as uint32), faces and rgb8, all exact."""
    nv, nf, occupied, degenerate, duplicate = want["counts"]
    info = got["simplify"]
    print(f"  {got['counts']} of {occupied} cells, degenerate {info['degenerate_faces']}, duplicate {info['duplicate_faces']}, box {info['box']}")
    assert got["counts"] == (nv, nf)
    assert (info["occupied"], info["degenerate_faces"], info["duplicate_faces"]) == (occupied, degenerate, duplicate)
    assert all(type(info[k]) is int for k in ("occupied", "degenerate_faces", "duplicate_faces"))
    assert (info["box"]["lo"], info["box"]["dims"]) == want["box"] and info["cell"] == cell and info["origin"] == tuple(origin)
    assert tuple(got["vertices"].shape) == (nv, 3) and tuple(got["faces"].shape) == (nf, 3)
    assert got["vertices"].dtype is torch.float32 and got["faces"].dtype is torch.int32
    assert np.array_equal(got["vertices"].cpu().numpy().view(np.uint32), want["vertices"].view(np.uint32))
    assert np.array_equal(got["faces"].cpu().numpy(), want["faces"])
    if want["rgb8"] is None:
        assert got["rgb8"] is None
    else:
        assert got["rgb8"].dtype is torch.uint8 and tuple(got["rgb8"].shape) == (nv, 3)
        assert np.array_equal(got["rgb8"].cpu().numpy(), want["rgb8"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_simplify_equals_the_restatement_bit_for_bit(name):
    m, cell, origin = cases()[name]
    for rgb in (True, False):
        dm = device_mesh(m, rgb)
        for dedupe in (True, False):
            print(f"{name} rgb {rgb} dedupe {dedupe}: {m['counts']}")
            got = mesh.simplify(dm, cell, origin=origin, dedupe=dedupe)
            _same_as_host(got, expected_simplified(name, rgb, dedupe), cell, origin)
    assert got["vertices"].data_ptr() != dm["vertices"].data_ptr()      # a new mesh: the input is left alone
    assert np.array_equal(dm["faces"].cpu().numpy(), m["faces"]) and np.array_equal(dm["vertices"].cpu().numpy(), m["vertices"])
    assert set(got) == {"vertices", "faces", "rgb8", "counts", "simplify"}


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.endswith(" / vertices permuted")])
def test_permuted_inputs_give_identical_vertex_bytes(name):
    base = name.rsplit(" / ", 1)[0]
    m, cell, origin = cases()[base]
    want = mesh.simplify(device_mesh(m), cell, origin=origin)
    for other in (name, base + " / faces permuted"):
        got = mesh.simplify(device_mesh(cases()[other][0]), cell, origin=origin)
        assert got["counts"] == want["counts"] and got["simplify"] == want["simplify"]
        assert torch.equal(got["vertices"].view(torch.int32), want["vertices"].view(torch.int32))
        assert torch.equal(got["rgb8"], want["rgb8"])
        if other == name:
            assert torch.equal(got["faces"], want["faces"])


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    for name in ("strip", "blobs shifted / 2 steps / origin 0.1 / vertices permuted"):
        m, cell, origin = cases()[name]
        dm = device_mesh(m)
        runs = [mesh.simplify(dm, cell, origin=origin) for _ in range(2)]
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            runs.append(mesh.simplify(dm, cell, origin=origin))
        side.synchronize()
        assert 0 < runs[0]["counts"][1] < m["counts"][1]
        for r in runs[1:]:
            same_device_mesh(r, runs[0])
            assert r["simplify"] == runs[0]["simplify"]


def test_bad_vertices_raise_and_the_next_call_is_right():
    name = "blobs / 2 steps / origin 0"
    m, cell, origin = cases()[name]
    nv = m["counts"][0]
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for row, col in ((0, 0), (nv // 2, 1), (nv - 1, 2)):
            v = m["vertices"].copy()
            v[row, col] = bad
            with pytest.raises(ValueError, match="not finite or lies 2\\^30 cells"):
                mesh.simplify(dict(device_mesh(m), vertices=to_dev(v)), cell, origin=origin)
    _same_as_host(mesh.simplify(device_mesh(m), cell, origin=origin), expected_simplified(name), cell, origin)


def test_bad_face_indices_raise_and_the_next_call_is_right():
    name = "blobs / 2 steps / origin 0"
    m, cell, origin = cases()[name]
    nv, nf = m["counts"]
    for dedupe in (True, False):
        for bad in (nv, -1, (1 << 31) - 1, -(1 << 31)):
            for row, col in ((0, 0), (nf // 2, 1), (nf - 1, 2)):
                faces = m["faces"].copy()
                faces[row, col] = bad
                with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                    mesh.simplify(dict(device_mesh(m), faces=to_dev(faces)), cell, origin=origin, dedupe=dedupe)
    _same_as_host(mesh.simplify(device_mesh(m), cell, origin=origin), expected_simplified(name), cell, origin)


def test_a_box_above_max_bytes_raises_before_any_further_launch(monkeypatch):
    m, cell, origin = cases()["sparse box"]
    dm = device_mesh(m)
    seen = record_launches(monkeypatch)
    need = _native.lib().lrf_mesh_simplify_workspace_bytes(9000, 3000, 128 * 128 * 80)
    with pytest.raises(ValueError, match="128 x 128 x 80") as e:
        mesh.simplify(dm, cell, origin=origin, max_bytes=need - 1)
    assert str(need) in str(e.value) and "larger cell" in str(e.value) and seen == ["lrf_mesh_simplify_bounds"]
    with pytest.raises(ValueError, match="fewer than 2\\^31") as e:      # 2^33 cells: the box alone refuses
        mesh.simplify(dm, cell / 2048, origin=origin)
    assert "larger cell" in str(e.value) and seen == ["lrf_mesh_simplify_bounds"] * 2
    got = mesh.simplify(dm, cell, origin=origin, max_bytes=need)
    assert seen == ["lrf_mesh_simplify_bounds"] * 3 + ["lrf_mesh_simplify"]
    _same_as_host(got, expected_simplified("sparse box"), cell, origin)


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = {"vertices": torch.empty(0, 3, device=DEV), "faces": torch.empty(0, 3, dtype=torch.int32, device=DEV), "rgb8": None,
             "counts": (0, 0), "note": "kept"}
    got = mesh.simplify(empty, 0.5)
    assert got["counts"] == (0, 0) and tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3)
    assert got["note"] == "kept" and got["simplify"]["occupied"] == 0
    m = cases()["blobs / 2 steps / origin 0"][0]
    got = mesh.simplify(dict(device_mesh(m), faces=torch.empty(0, 3, dtype=torch.int32, device=DEV)), 2 * H_ANALYTIC)
    assert got["counts"] == (0, 0) and tuple(got["vertices"].shape) == (0, 3) and tuple(got["rgb8"].shape) == (0, 3)
    assert got["simplify"]["occupied"] == expected_simplified("blobs / 2 steps / origin 0")["counts"][2]


ORIGIN = (0.1, -0.2, 0.3)


@pytest.mark.parametrize("which", ("dense", "sparse"))
def test_extract_option_equals_simplify_of_extract(which):
    vol = blob_volumes(ORIGIN)[which == "sparse"]
    plain = vol.extract()
    assert set(plain) == {"vertices", "faces", "rgb8", "counts"} and plain["counts"] == (2902, 5780)
    assert set(vol.extract(simplify_cell=None)) == set(plain)           # the default: exactly today's dict
    for c in (2 * H_ANALYTIC, 3.5 * H_ANALYTIC):
        got = vol.extract(simplify_cell=c)
        want = mesh.simplify(plain, c, origin=vol.origin)
        same_device_mesh(got, want)
        assert got["simplify"] == want["simplify"] and got["simplify"]["origin"] == ORIGIN
        assert 0 < got["counts"][1] < plain["counts"][1]
        other = mesh.simplify(plain, c)                                 # another anchor, another mesh
        assert other["simplify"]["box"] != want["simplify"]["box"] or not torch.equal(other["vertices"], want["vertices"])
        # with the component filter: the filter runs first, at full resolution
        got = vol.extract(min_component_faces=601, simplify_cell=c)
        filtered = mesh.filter_components(plain, 601)
        want = mesh.simplify(filtered, c, origin=vol.origin)
        assert filtered["counts"][1] == 4200
        same_device_mesh(got, want)
        assert got["simplify"] == want["simplify"] and got["components"]["kept"] == 1
        wrong = mesh.filter_components(mesh.simplify(plain, c, origin=vol.origin), 601)
        assert wrong["counts"] != got["counts"]                         # simplifying first judges other components


def test_scene_mesh_option_writes_the_same_ply_twice(tmp_path):
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    out = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(len(lt.r_c2w))), floater_thresh=0.5)
    xyz = pointcloud.fuse_points(None, out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=(0.05, 50.0))["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 28
    kw = dict(voxel=voxel, bounds=(tuple(lo - 3 * voxel), tuple(hi + 3 * voxel)), floater_thresh=0.5, depth_range=(0.05, 50.0))
    plain = mesh.scene_mesh(lt, W, H, **kw)
    assert set(plain) == {"vertices", "faces", "rgb8", "counts", "volume"}
    files = []
    for _ in range(2):
        got = mesh.scene_mesh(lt, W, H, simplify_cell=3 * voxel, **kw)
        path = tmp_path / f"mesh{len(files)}.ply"
        pointcloud.write_ply(str(path), got["vertices"], got["rgb8"], faces=got["faces"])
        files.append(path.read_bytes())
    want = mesh.simplify(plain, 3 * voxel, origin=plain["volume"].origin)
    print(f"scene_mesh: {plain['counts']} -> {got['counts']}, {got['simplify']}")
    same_device_mesh(got, want)
    assert got["simplify"] == want["simplify"] and "volume" in got
    assert files[0] == files[1] and len(files[0]) > 200 and 0 < got["counts"][1] < plain["counts"][1]
