"""Mesh cleaning on the MI355X (csrc/lrf_mesh_clean.inl through localrf_amd.mesh): component labels, counts and the filtered
mesh against the numpy restatement of tests/mesh_clean_cases.py, all exact; the scan's block boundary, reproducibility, a
non-default stream, bad face indices and the extract options."""

import numpy as np
import pytest
import torch

from localrf_amd import mesh, novel_views, pointcloud
from mesh_clean_cases import (FANS, MESH_NAMES, all_meshes, components_host, expected, fan, filter_host,
                              threshold_host)
from mesh_util import DEV, blob_volumes, device_mesh, same_device_mesh, same_mesh, to_dev
from novel_views_cases import scene

pytestmark = pytest.mark.gpu
THRESHOLDS = (0, 1, 100, 601, 10 ** 6)
FRACTIONS = (0.1, 1.0)


def _same_components(got, want, nv):
    for k in ("labels", "faces_of", "vertices_of"):
        assert got[k].dtype is torch.int32 and tuple(got[k].shape) == (nv,) and got[k].device.type == "cuda"
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    for k in ("n_components", "n_with_faces", "largest_faces"):
        assert type(got[k]) is int and got[k] == want[k], (k, got[k], want[k])
    assert type(got["rounds"]) is int and 1 <= got["rounds"] <= 64


@pytest.mark.parametrize("name", MESH_NAMES)
def test_labels_and_counts_equal_the_restatement(name):
    m = all_meshes()[name]
    nv, nf = m["counts"]
    got = mesh.components(to_dev(m["faces"]), nv)
    print(f"{name}: {nv} vertices, {nf} faces, {got['n_components']} components, rounds {got['rounds']}")
    _same_components(got, expected(name), nv)


@pytest.mark.parametrize("nv", FANS)
def test_fans_across_a_wave_a_workgroup_and_a_keep_word_group(nv):
    """One fan, the fan beside strays and a second fan whose vertices straddle the boundary, and the same with the order
    reversed (every label then comes from the far end)."""
    f = fan(nv, seed=nv)
    two = np.concatenate([f["faces"], f["faces"][: max(1, (nv - 2) // 3)] + nv])
    rev = (nv - 1 - f["faces"]).astype(np.int32)
    for label, faces, n in (("fan", f["faces"], nv), ("fan and strays", f["faces"], nv + 70), ("two fans", two, 2 * nv),
                            ("reversed", rev, nv), ("reversed and strays", rev, nv + 1)):
        m = {"vertices": np.zeros((n, 3), np.float32), "faces": np.ascontiguousarray(faces, dtype=np.int32)}
        got = mesh.components(to_dev(m["faces"]), n)
        print(f"{label} Nv = {n}: {got['n_components']} components, rounds {got['rounds']}")
        _same_components(got, components_host(m), n)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_filter_equals_the_restatement_bit_for_bit(name):
    m, comp = all_meshes()[name], expected(name)
    once = {}
    for rgb in (True, False):
        dm = device_mesh(m, rgb)
        hm = m if rgb else dict(m, rgb8=None)
        for kw in [dict(min_faces=t) for t in THRESHOLDS] + [dict(min_fraction=q) for q in FRACTIONS] + [dict(min_faces=100, min_fraction=0.1)]:
            threshold = threshold_host(kw.get("min_faces", 0), kw.get("min_fraction", 0.0), comp["largest_faces"])
            want, kept = filter_host(hm, comp, threshold)
            got = mesh.filter_components(dm, **kw)
            same_mesh(got, want)
            info = got["components"]
            assert info["kept"] == kept and info["threshold"] == threshold, (kw, info)
            assert (info["n_components"], info["n_with_faces"], info["largest_faces"]) == (comp["n_components"], comp["n_with_faces"],
                                                                                         comp["largest_faces"])
            if rgb:
                once[tuple(kw.items())] = (got, kw)
            if threshold == 0:                                          # the input's bytes
                same_device_mesh(got, dm)
            if kw.get("min_faces") == 10 ** 6:
                assert got["counts"] == (0, 0) and tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3)
        print(f"{name} rgb {rgb}: rounds {info['rounds']}, largest {info['largest_faces']}")
    for got, kw in once.values():                                       # filtering twice equals filtering once
        again = mesh.filter_components(got, **kw)
        same_device_mesh(again, got)
        assert again["components"]["kept"] == again["components"]["n_components"]       # nothing is left to drop
    assert dm["vertices"].data_ptr() != got["vertices"].data_ptr()      # a new mesh: the input is left alone
    assert np.array_equal(dm["faces"].cpu().numpy(), m["faces"])


def test_a_fan_across_the_scan_block_boundary():
    """2^20 + 1 vertices make 1025 workgroup counts: k_points_scan takes a second step of 1024.  Strays among the fan's
    vertices make the ranks differ from the indices on both sides of the boundary."""
    nv = (1 << 20) + 1
    i = np.arange(1, nv - 1, dtype=np.int32)
    i = i[(i % 1000 != 0) & ((i + 1) % 1000 != 0)]                      # every 1000th vertex is in no face
    faces = np.stack([np.zeros_like(i), i, i + 1], 1)
    rng = np.random.default_rng(9)
    m = {"vertices": rng.standard_normal((nv, 3)).astype(np.float32), "faces": faces,
         "rgb8": rng.integers(0, 256, (nv, 3), dtype=np.uint8), "counts": (nv, int(faces.shape[0]))}
    comp = components_host(m, big=True)
    assert comp["n_components"] == 1 + (nv - 2) // 1000 and comp["largest_faces"] == faces.shape[0]
    dm = device_mesh(m)
    got = mesh.components(dm["faces"], nv)
    print(f"fan of 2^20 + 1: rounds {got['rounds']}")
    _same_components(got, comp, nv)
    for threshold in (0, 1):
        want, kept = filter_host(m, comp, threshold)
        out = mesh.filter_components(dm, min_faces=threshold)
        same_mesh(out, want)
        assert out["components"]["kept"] == kept
    assert out["counts"] == (nv - (nv - 2) // 1000, faces.shape[0])


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    m = all_meshes()["blobs noise / vertices permuted"]
    dm = device_mesh(m)
    runs = [(mesh.components(dm["faces"], m["counts"][0]), mesh.filter_components(dm, min_faces=100)) for _ in range(2)]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        runs.append((mesh.components(dm["faces"], m["counts"][0]), mesh.filter_components(dm, min_faces=100)))
    side.synchronize()
    (c0, f0) = runs[0]
    assert 0 < f0["counts"][1] < m["counts"][1]
    for c, f in runs[1:]:
        for k in ("labels", "faces_of", "vertices_of"):
            assert torch.equal(c[k], c0[k]), k
        assert all(c[k] == c0[k] for k in ("n_components", "n_with_faces", "largest_faces"))
        same_device_mesh(f, f0)
        assert f["components"]["kept"] == f0["components"]["kept"]
    same_mesh(f0, filter_host(m, expected("blobs noise / vertices permuted"), 100)[0])


def test_bad_face_indices_raise_and_the_next_call_is_right():
    m = all_meshes()["blobs"]
    nv = m["counts"][0]
    for bad in (nv, -1, (1 << 31) - 1, -(1 << 31)):
        for row, col in ((0, 0), (m["counts"][1] // 2, 1), (m["counts"][1] - 1, 2)):
            faces = m["faces"].copy()
            faces[row, col] = bad
            with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                mesh.components(to_dev(faces), nv)
            with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                mesh.filter_components(dict(device_mesh(m), faces=to_dev(faces)), min_faces=100)
    got = mesh.components(to_dev(m["faces"]), nv)
    _same_components(got, expected("blobs"), nv)
    same_mesh(mesh.filter_components(device_mesh(m), min_faces=100), filter_host(m, expected("blobs"), 100)[0])
    with pytest.raises(RuntimeError, match="max_rounds is 1"):          # the blobs need a changing round and a quiet one
        mesh.components(to_dev(m["faces"]), nv, max_rounds=1)


@pytest.mark.parametrize("which", ("dense", "sparse"))
def test_extract_options_equal_filter_components_of_extract(which):
    vol = blob_volumes()[which == "sparse"]
    plain = vol.extract()
    assert set(plain) == {"vertices", "faces", "rgb8", "counts"} and plain["counts"] == (2902, 5780)
    same_device_mesh(vol.extract(min_component_faces=0, min_component_fraction=0.0), plain)
    assert set(vol.extract(min_component_faces=0)) == set(plain)        # the defaults: exactly today's dict
    for kw in (dict(min_component_faces=100), dict(min_component_faces=601), dict(min_component_fraction=0.1),
               dict(min_component_fraction=1.0), dict(min_component_faces=10 ** 6), dict(min_component_faces=500, min_component_fraction=0.05)):
        got = vol.extract(**kw)
        want = mesh.filter_components(plain, kw.get("min_component_faces", 0), kw.get("min_component_fraction", 0.0))
        same_device_mesh(got, want)
        assert got["components"] == dict(want["components"], rounds=got["components"]["rounds"])
    assert vol.extract(min_component_faces=601)["counts"][1] == 4200 and vol.extract(min_component_fraction=1.0)["components"]["kept"] == 1


def test_scene_mesh_options_equal_scene_mesh_then_filter(tmp_path):
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
    same = mesh.scene_mesh(lt, W, H, min_component_faces=0, min_component_fraction=0.0, **kw)
    assert set(same) == set(plain)
    same_device_mesh(same, plain)
    comp = mesh.components(plain["faces"], plain["counts"][0])
    k = max(2, comp["largest_faces"] // 2)
    print(f"scene_mesh: {plain['counts']} vertices / faces, {comp['n_components']} components, largest {comp['largest_faces']}, "
          f"rounds {comp['rounds']}")
    files = []
    for opts in (dict(min_component_faces=k), dict(min_component_fraction=1.0)):
        got = mesh.scene_mesh(lt, W, H, **opts, **kw)
        want = mesh.filter_components(plain, opts.get("min_component_faces", 0), opts.get("min_component_fraction", 0.0))
        same_device_mesh(got, want)
        assert got["components"]["kept"] == want["components"]["kept"] and "volume" in got
        path = tmp_path / f"mesh{len(files)}.ply"
        pointcloud.write_ply(str(path), got["vertices"], got["rgb8"], faces=got["faces"])
        files.append(path.read_bytes())
        if got["counts"][0]:
            after = mesh.components(got["faces"], got["counts"][0])
            assert after["n_components"] == got["components"]["kept"] == after["n_with_faces"]
            assert int(after["faces_of"][after["labels"].unique().long()].min()) >= got["components"]["threshold"]
    # the written file holds only the kept shells, and the same bytes on a second run
    again = mesh.scene_mesh(lt, W, H, min_component_fraction=1.0, **kw)
    pointcloud.write_ply(str(tmp_path / "again.ply"), again["vertices"], again["rgb8"], faces=again["faces"])
    assert (tmp_path / "again.ply").read_bytes() == files[-1] and len(files[-1]) > 200
