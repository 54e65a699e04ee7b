"""Mesh cleaning without a GPU: the numpy restatement of csrc/lrf_mesh_clean.inl (tests/mesh_clean_cases.py) against a
brute-force search and the known component counts of the analytic meshes, what filtering leaves of closed shells, the stray
vertices at thresholds 0 and 1, argument refusals before any native call (Python and C ABI), the new symbols, and the new
kernels' scratch use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from mesh_cases import closed_manifold_euler
from mesh_clean_cases import (BLOB_FACES, MESH_NAMES, all_meshes, base_meshes, components_host, expected, fan, filter_host,
                              labels_bfs, labels_host, labels_host_arrays, threshold_host)
from mesh_util import DenseStub, cpu_mesh, forbid_native, forbid_render

SYMBOLS = ("lrf_mesh_components_init", "lrf_mesh_components_round", "lrf_mesh_components_count",
           "lrf_mesh_filter_workspace_bytes", "lrf_mesh_filter")


def _sizes(comp):
    return sorted(comp["faces_of"][comp["labels"] == np.arange(comp["labels"].size)].tolist(), reverse=True)


def test_restated_labels_equal_a_breadth_first_search():
    assert tuple(all_meshes()) == MESH_NAMES
    small = [n for n in MESH_NAMES if not n.startswith("strip")]
    assert len(small) == 27
    for name in small:
        m = all_meshes()[name]
        nv = m["vertices"].shape[0]
        want = labels_bfs(m["faces"], nv)
        assert np.array_equal(expected(name)["labels"], want), name
        assert np.array_equal(labels_host_arrays(m["faces"], nv), want), name
    for nv in (3, 64, 257):
        f = fan(nv)
        assert (labels_host(f["faces"], nv) == 0).all() and (labels_host_arrays(f["faces"], nv) == 0).all()
    for name in ("strip", "strip permuted"):                           # too long for the search: the two restatements agree
        m = all_meshes()[name]
        assert np.array_equal(expected(name)["labels"], labels_host_arrays(m["faces"], m["vertices"].shape[0]))


def test_component_counts_of_the_analytic_meshes():
    b = base_meshes()
    for name, counts, n, largest in (("sphere", (3624, 7244), 1, 7244), ("torus", (2736, 5472), 1, 5472),
                                     ("blobs", (2902, 5780), 6, 4200), ("strip", (40000, 79996), 1, 79996),
                                     ("strip permuted", (40000, 79996), 1, 79996), ("one vertex", (1, 0), 1, 0),
                                     ("one triangle", (3, 1), 1, 1), ("two triangles", (5, 2), 1, 2)):
        c = expected(name)
        assert b[name]["counts"] == counts and (c["n_components"], c["largest_faces"]) == (n, largest), name
        assert c["n_with_faces"] == (n if counts[1] else 0)
    assert _sizes(expected("blobs")) == list(BLOB_FACES)
    tie = _sizes(expected("blobs tie"))
    assert len(tie) == 6 and tie[:3] == [1592, 1592, 600]
    noise = _sizes(expected("blobs noise"))
    assert len(noise) == 13 and noise[-1] == 2
    for name in MESH_NAMES:                                         # a permutation moves the labels, not the sizes
        c, base = expected(name), expected(name.split(" / ")[0])
        assert _sizes(c) == _sizes(base), name
        assert int(c["faces_of"].sum()) == all_meshes()[name]["counts"][1] and int(c["vertices_of"].sum()) == c["labels"].size
        assert (c["labels"] <= np.arange(c["labels"].size)).all()


def test_filtering_the_blobs_leaves_closed_shells():
    for name in ("blobs", "blobs / vertices permuted", "blobs / faces permuted"):
        m, comp = all_meshes()[name], expected(name)
        assert closed_manifold_euler(m) == 12
        out, kept = filter_host(m, comp, 100)
        assert kept == 5 and out["counts"][1] == sum(BLOB_FACES[:5]) and closed_manifold_euler(out) == 10
        for k, threshold in enumerate(sorted(BLOB_FACES)):             # drops the k smallest shells
            out, kept = filter_host(m, comp, threshold)
            assert kept == 6 - k and closed_manifold_euler(out) == 2 * kept
            again = components_host(out)
            assert again["n_components"] == kept and _sizes(again) == list(BLOB_FACES[:kept])
        out, kept = filter_host(m, comp, BLOB_FACES[0] + 1)
        assert kept == 0 and out["counts"] == (0, 0) and out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3)
    tie = all_meshes()["blobs tie"]
    comp = expected("blobs tie")
    out, kept = filter_host(tie, comp, threshold_host(0, 1.0, comp["largest_faces"]))
    assert kept == 2 and out["counts"][1] == 2 * 1592                   # min_fraction = 1 keeps every tie with the largest
    assert threshold_host(601, 0.1, 4200) == 601 and threshold_host(3, 0.1, 4201) == 421 and threshold_host(0, 0.0, 9) == 0


def test_thresholds_0_and_1_on_stray_vertices():
    m, comp = all_meshes()["blobs strays"], expected("blobs strays")
    clean = all_meshes()["blobs"]
    assert comp["n_components"] == 9 and comp["n_with_faces"] == 6
    out, kept = filter_host(m, comp, 0)
    assert kept == 9
    for k in ("vertices", "faces", "rgb8"):
        assert out[k].tobytes() == m[k].tobytes(), k
    out, kept = filter_host(m, comp, 1)
    assert kept == 6 and out["counts"] == clean["counts"]
    for k in ("vertices", "faces", "rgb8"):                            # exactly the strays went
        assert out[k].tobytes() == clean[k].tobytes(), k


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    faces = cpu_mesh()["faces"]
    with pytest.raises(TypeError, match="faces"):
        mesh.components(faces.numpy(), 4)
    for f, nv, match in ((faces.long(), 4, "int32"), (faces[:, :2], 4, "int32"), (faces.reshape(-1), 4, "int32"),
                         (faces, -1, "n_vertices"), (faces, 2.5, "n_vertices"), (faces, 1 << 31, "n_vertices"), (faces, 0, "without")):
        with pytest.raises(ValueError, match=match):
            mesh.components(f, nv)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="max_rounds"):
            mesh.components(faces, 4, max_rounds=bad)
    with pytest.raises(NativeError):                                    # valid arguments, a CPU tensor: no fallback
        mesh.components(faces, 4)

    with pytest.raises(TypeError, match="mesh"):
        mesh.filter_components([torch.zeros(4, 3), faces])
    for key, bad in (("vertices", np.zeros((4, 3), np.float32)), ("faces", faces.numpy()), ("rgb8", np.zeros((4, 3), np.uint8))):
        with pytest.raises(TypeError, match=key):
            mesh.filter_components(dict(cpu_mesh(), **{key: bad}))
    for key, bad, match in (("vertices", torch.zeros(4, 3, dtype=torch.float64), "vertices"), ("vertices", torch.zeros(4, 2), "vertices"),
                            ("faces", faces.long(), "faces"), ("faces", faces.t().contiguous(), "faces"),
                            ("rgb8", torch.zeros(4, 3), "rgb8"), ("rgb8", torch.zeros(3, 3, dtype=torch.uint8), "rgb8")):
        with pytest.raises(ValueError, match=match):
            mesh.filter_components(dict(cpu_mesh(), **{key: bad}))
    for kw, match in ((dict(min_faces=-1), "min_faces"), (dict(min_faces=1.5), "min_faces"), (dict(min_faces=math.nan), "min_faces"),
                      (dict(min_faces=None), "min_faces"), (dict(min_fraction=-0.1), "min_fraction"),
                      (dict(min_fraction=1.01), "min_fraction"), (dict(min_fraction=math.nan), "min_fraction"),
                      (dict(max_rounds=0), "max_rounds")):
        with pytest.raises(ValueError, match=match):
            mesh.filter_components(cpu_mesh(), **kw)
    for rgb in (True, False):
        with pytest.raises(NativeError):
            mesh.filter_components(cpu_mesh(rgb), min_faces=1)
    # the extract options are checked with the other arguments, before the extraction
    for kw, match in ((dict(min_component_faces=-1), "min_component_faces"), (dict(min_component_fraction=2.0), "min_component_fraction"),
                      (dict(min_component_fraction=math.nan), "min_component_fraction")):
        with pytest.raises(ValueError, match=match):
            DenseStub(colours=False).extract(**kw)
    with pytest.raises(TypeError):
        DenseStub(colours=False).extract(0.0, 1.0, None, None, 5)                         # keyword-only
    assert "min_component_faces" in mesh._MESH_KEYS and "min_component_fraction" in mesh._MESH_KEYS


def test_scene_mesh_checks_the_component_options_before_it_renders(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    for kw, match in ((dict(min_component_faces=-2), "min_component_faces"), (dict(min_component_fraction=1.5), "min_component_fraction")):
        with pytest.raises(ValueError, match=match):
            mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, **kw)
    with pytest.raises(NativeError):                                    # accepted options, a CPU scene
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, min_component_faces=10, min_component_fraction=0.5)


def test_clean_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfMeshFilter" in header and C.sizeof(N.LrfMeshFilter) == 5 * 8 + 2 * 8
    assert built_lib.lrf_abi_version() == 7
    ws = built_lib.lrf_mesh_filter_workspace_bytes
    assert ws(0, 0) == 0 and ws(-1, 5) == 0 and ws(5, -1) == 0 and ws(1 << 31, 0) == 0 and ws(5, 1 << 31) == 0
    assert ws(1, 0) == 512 and ws(1024, 1024) == 512 and ws(1025, 3) == 1024 and ws(3, 1025) == 1024
    assert ws((1 << 31) - 1, (1 << 31) - 1) >= 2 * ((1 << 31) // 8 + (1 << 31) // 16)

    init = lambda parent=FAKE, Nv=5: refused(built_lib, built_lib.lrf_mesh_components_init(parent, Nv, None))  # noqa: E731
    assert "1 <= Nv < 2^31" in init(Nv=0) and "1 <= Nv < 2^31" in init(Nv=1 << 31) and "1 <= Nv < 2^31" in init(Nv=-4)
    assert init(parent=None) == "lrf_mesh_components_init: null argument" and "4-byte aligned" in init(parent=FAKE + 2)

    def rnd(parent=FAKE, faces=FAKE, Nv=5, Nf=3, changed=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_components_round(parent, faces, Nv, Nf, changed, None))
    for bad in (dict(Nv=0), dict(Nf=-1), dict(Nv=1 << 31), dict(Nf=1 << 31)):
        assert "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31" in rnd(**bad), bad
    for bad in (dict(parent=None), dict(faces=None), dict(changed=None)):
        assert rnd(**bad) == "lrf_mesh_components_round: null argument", bad
    for bad in (dict(parent=FAKE + 1), dict(faces=FAKE + 2), dict(changed=FAKE + 3)):
        assert "4-byte aligned" in rnd(**bad), bad

    def count(labels=FAKE, faces=FAKE, Nv=5, Nf=3, faces_of=FAKE, vertices_of=FAKE, summary=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_components_count(labels, faces, Nv, Nf, faces_of, vertices_of, summary, None))
    for bad in (dict(Nv=0), dict(Nf=-1), dict(Nv=1 << 31), dict(Nf=1 << 31)):
        assert "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31" in count(**bad), bad
    for bad in (dict(labels=None), dict(faces=None), dict(faces_of=None), dict(vertices_of=None), dict(summary=None)):
        assert count(**bad) == "lrf_mesh_components_count: null argument", bad
    for bad in (dict(labels=FAKE + 2), dict(faces=FAKE + 1), dict(faces_of=FAKE + 2), dict(vertices_of=FAKE + 2)):
        assert "4-byte aligned" in count(**bad), bad
    assert "8-byte aligned" in count(summary=FAKE + 4)

    def flt(threshold=1, vertices_out=FAKE, rgb8_out=FAKE, faces_out=FAKE, counts=FAKE, wsp=FAKE, **over):
        a = filled(N.LrfMeshFilter, dict(vertices=FAKE, rgb8=FAKE, faces=FAKE, labels=FAKE, faces_of=FAKE, Nv=5, Nf=3), **over)
        return refused(built_lib, built_lib.lrf_mesh_filter(C.byref(a), threshold, vertices_out, rgb8_out, faces_out, counts, wsp, None))
    for bad in (dict(Nv=0), dict(Nf=-1), dict(Nv=1 << 31), dict(Nf=1 << 31)):
        assert "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31" in flt(**bad), bad
    for bad in (dict(vertices=None), dict(faces=None), dict(labels=None), dict(faces_of=None), dict(vertices_out=None),
                dict(faces_out=None), dict(counts=None), dict(wsp=None)):
        assert flt(**bad) == "lrf_mesh_filter: null argument", bad
    assert "go together" in flt(rgb8=None) and "go together" in flt(rgb8_out=None)
    assert "threshold" in flt(threshold=-1)
    for bad in (dict(vertices=FAKE + 2), dict(faces=FAKE + 1), dict(labels=FAKE + 2), dict(faces_of=FAKE + 3), dict(vertices_out=FAKE + 2),
                dict(faces_out=FAKE + 2)):
        assert "4-byte aligned" in flt(**bad), bad
    assert "8-byte aligned" in flt(counts=FAKE + 4) and "8-byte aligned" in flt(wsp=FAKE + 4)
    assert built_lib.lrf_mesh_filter(None, 1, FAKE, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_clean_kernels_use_no_scratch():
    """The kernels of lrf_mesh_clean.inl as __graft_entry__.build() compiles them."""
    from isa_util import assert_no_scratch, device_asm
    names = ("k_cc_init", "k_cc_clear", "k_cc_hook", "k_cc_shorten", "k_cc_zero", "k_cc_count_faces", "k_cc_count_vertices",
             "k_cc_summary", "k_mesh_filter_mark", "k_mesh_filter_write")
    assert_no_scratch(device_asm(), names, match="search", total=len(names), body_too=True)
