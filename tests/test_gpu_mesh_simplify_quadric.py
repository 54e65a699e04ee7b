"""Quadric placement of the clustering simplifier on the MI355X (rules a-d of csrc/lrf_mesh_simplify.inl through
localrf_amd.mesh.simplify(placement="quadric")): every case of tests/mesh_simplify_quadric_cases.py against the numpy
restatement, bit for bit -- no tolerance anywhere --, the capped cluster, other regularisers, reproducibility, a non-default
stream, placement="mean" against the call without the keyword, and bad vertices and face indices."""

import numpy as np
import pytest
import torch

from localrf_amd import mesh
from mesh_simplify_quadric_cases import CAP, CAPPED, CASE_NAMES, REGULARIZE, cases, expected_quadric
from mesh_util import DEV, device_mesh, record_launches, same_device_mesh, to_dev

pytestmark = pytest.mark.gpu

MEAN_KEYS = {"cell", "origin", "box", "occupied", "degenerate_faces", "duplicate_faces", "placement"}
QUADRIC_KEYS = MEAN_KEYS | {"regularize", "fallback_clusters", "clamped_clusters"}


def _same_as_host(got, want, cell, origin, regularize=REGULARIZE):
    """All seven counts, the box, vertices (as uint32), faces and rgb8, all exact."""
    nv, nf, occupied, degenerate, duplicate, fallback, clamped = want["counts"]
    info = got["simplify"]
    print(f"  {got['counts']} of {occupied} cells, degenerate {info['degenerate_faces']}, duplicate {info['duplicate_faces']}, "
          f"at the mean {info['fallback_clusters']}, clamped {info['clamped_clusters']}, box {info['box']}")
    assert set(info) == QUADRIC_KEYS and info["placement"] == "quadric" and info["regularize"] == regularize
    assert got["counts"] == (nv, nf)
    counted = ("occupied", "degenerate_faces", "duplicate_faces", "fallback_clusters", "clamped_clusters")
    assert tuple(info[k] for k in counted) == (occupied, degenerate, duplicate, fallback, clamped)
    assert all(type(info[k]) is int for k in counted)
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
def test_quadric_placement_equals_the_restatement_bit_for_bit(name):
    m, cell, origin = cases()[name]
    for rgb in (True, False):
        dm = device_mesh(m, rgb)
        for dedupe in (True, False):
            print(f"{name} rgb {rgb} dedupe {dedupe}: {m['counts']}")
            got = mesh.simplify(dm, cell, origin=origin, dedupe=dedupe, placement="quadric")
            _same_as_host(got, expected_quadric(name, rgb, dedupe), cell, origin)
    assert got["vertices"].data_ptr() != dm["vertices"].data_ptr()      # a new mesh: the input is left alone
    assert np.array_equal(dm["faces"].cpu().numpy(), m["faces"]) and np.array_equal(dm["vertices"].cpu().numpy(), m["vertices"])
    assert set(got) == {"vertices", "faces", "rgb8", "counts", "simplify"}


def test_a_cluster_at_the_cap_takes_the_mean():
    m, cell, origin = cases()[CAPPED]
    assert m["counts"][1] == CAP + 4 and m["rgb8"] is None
    want = expected_quadric(CAPPED, False, True)
    assert want["counts"][5:] == (1, 0) and want["contributions"][0] >= CAP
    _same_as_host(mesh.simplify(device_mesh(m, False), cell, origin=origin, placement="quadric"), want, cell, origin)


@pytest.mark.parametrize("regularize", (1.0, 2.0 ** -4, 1e-3, 2.0 ** -30))
def test_other_regularisers(regularize):
    for name in ("cube", "blobs shifted / 3.5 steps / origin 0.1 / faces permuted", "spanning face"):
        m, cell, origin = cases()[name]
        got = mesh.simplify(device_mesh(m), cell, origin=origin, placement="quadric", regularize=regularize)
        _same_as_host(got, expected_quadric(name, True, True, regularize), cell, origin, regularize)


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    for name in ("spanning face", "blobs shifted / 2 steps / origin 0.1 / vertices permuted"):
        m, cell, origin = cases()[name]
        dm = device_mesh(m)
        runs = [mesh.simplify(dm, cell, origin=origin, placement="quadric") for _ in range(2)]
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            runs.append(mesh.simplify(dm, cell, origin=origin, placement="quadric"))
        side.synchronize()
        assert 0 < runs[0]["counts"][1] < m["counts"][1]
        for r in runs[1:]:
            same_device_mesh(r, runs[0])
            assert r["simplify"] == runs[0]["simplify"]


def test_mean_placement_is_the_call_without_the_keyword(monkeypatch):
    name = "torus / 3.5 steps / origin 0.1"
    m, cell, origin = cases()[name]
    dm = device_mesh(m)
    seen = record_launches(monkeypatch)
    plain = mesh.simplify(dm, cell, origin=origin)
    calls = list(seen)
    del seen[:]
    named = mesh.simplify(dm, cell, origin=origin, placement="mean", regularize=0.5)
    assert calls == seen == ["lrf_mesh_simplify_bounds", "lrf_mesh_simplify"]
    same_device_mesh(named, plain)
    assert named["simplify"] == plain["simplify"] and set(plain["simplify"]) == MEAN_KEYS and plain["simplify"]["placement"] == "mean"
    del seen[:]
    quadric = mesh.simplify(dm, cell, origin=origin, placement="quadric")
    assert seen == ["lrf_mesh_simplify_bounds", "lrf_mesh_simplify_quadric"]
    assert torch.equal(quadric["faces"], plain["faces"]) and torch.equal(quadric["rgb8"], plain["rgb8"])
    assert not torch.equal(quadric["vertices"], plain["vertices"])


def test_bad_vertices_and_face_indices_raise_and_the_next_call_is_right():
    name = "blobs / 2 steps / origin 0"
    m, cell, origin = cases()[name]
    nv, nf = m["counts"]
    for bad in (np.nan, np.inf, -1e30):
        for row, col in ((0, 0), (nv // 2, 1), (nv - 1, 2)):
            v = m["vertices"].copy()
            v[row, col] = bad
            with pytest.raises(ValueError, match="not finite or lies 2\\^30 cells"):
                mesh.simplify(dict(device_mesh(m), vertices=to_dev(v)), cell, origin=origin, placement="quadric")
    for dedupe in (True, False):
        for bad in (nv, -1, (1 << 31) - 1, -(1 << 31)):
            for row, col in ((0, 0), (nf // 2, 1), (nf - 1, 2)):
                faces = m["faces"].copy()
                faces[row, col] = bad
                with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                    mesh.simplify(dict(device_mesh(m), faces=to_dev(faces)), cell, origin=origin, dedupe=dedupe, placement="quadric")
    _same_as_host(mesh.simplify(device_mesh(m), cell, origin=origin, placement="quadric"), expected_quadric(name), cell, origin)


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = {"vertices": torch.empty(0, 3, device=DEV), "faces": torch.empty(0, 3, dtype=torch.int32, device=DEV), "rgb8": None,
             "counts": (0, 0), "note": "kept"}
    got = mesh.simplify(empty, 0.5, placement="quadric")
    assert got["counts"] == (0, 0) and got["note"] == "kept" and set(got["simplify"]) == QUADRIC_KEYS
    assert (got["simplify"]["fallback_clusters"], got["simplify"]["clamped_clusters"]) == (0, 0)
    m, cell, origin = cases()["blobs / 2 steps / origin 0"]
    got = mesh.simplify(dict(device_mesh(m), faces=torch.empty(0, 3, dtype=torch.int32, device=DEV)), cell, placement="quadric")
    assert got["counts"] == (0, 0) and tuple(got["vertices"].shape) == (0, 3) and tuple(got["rgb8"].shape) == (0, 3)
    assert got["simplify"]["occupied"] == expected_quadric("blobs / 2 steps / origin 0")["counts"][2]
    assert (got["simplify"]["fallback_clusters"], got["simplify"]["clamped_clusters"]) == (0, 0)
