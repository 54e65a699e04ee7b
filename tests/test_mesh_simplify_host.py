"""Mesh simplification without a GPU: properties of the numpy restatement of csrc/lrf_mesh_simplify.inl
(tests/mesh_simplify_cases.py) on every case, argument refusals before any native call (Python and C ABI), the new symbols,
the workspace size, and the new kernels' scratch use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from mesh_cases import H_ANALYTIC
from mesh_simplify_cases import (CASE_NAMES, canonical, cases, cells_host, expected_simplified, face_keys, simplify_host,
                                 smallest_blob)
from mesh_util import DenseStub, cpu_mesh, forbid_native, forbid_render

SYMBOLS = ("lrf_mesh_simplify_bounds", "lrf_mesh_simplify_workspace_bytes", "lrf_mesh_simplify")
KERNELS = ("k_ms_bounds_init", "k_ms_bounds", "k_ms_zero", "k_ms_mark", "k_ms_count_words", "k_ms_accumulate", "k_ms_faces_map",
           "k_ms_faces_insert", "k_ms_faces_keep", "k_ms_write", "k_ms_finish")


def test_case_names_are_fixed():
    assert tuple(cases()) == CASE_NAMES and len(CASE_NAMES) == 3 * (3 * 2 + 3 * 3) * 3 + 10


@pytest.mark.parametrize("name", CASE_NAMES)
def test_properties_of_the_restatement(name):
    m, cell, origin = cases()[name]
    for rgb in (True, False):
        for dedupe in (True, False):
            r = expected_simplified(name, rgb, dedupe)
            v, f = r["vertices"], r["faces"]
            nv, nf, occupied, degenerate, duplicate = r["counts"]
            assert v.dtype == np.float32 and v.shape == (nv, 3) and f.dtype == np.int32 and f.shape == (nf, 3)
            assert (r["rgb8"] is None) == (not rgb) and (not rgb or (r["rgb8"].dtype == np.uint8 and r["rgb8"].shape == (nv, 3)))
            # the three indices of a face are distinct, and the smallest comes first
            assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
            assert np.array_equal(canonical(f), f)
            keys = face_keys(f)
            if dedupe:
                assert len(set(keys)) == len(keys)
            else:
                assert duplicate == 0
            # every vertex is referenced
            assert np.array_equal(np.unique(f), np.arange(nv))
            # every vertex lies in its cell, to one fp32 ulp
            lo = np.asarray(origin, np.float64) + r["cells"].astype(np.float64) * cell
            ulp = np.spacing(np.maximum(np.abs(v), np.abs((lo + cell).astype(np.float32)))).astype(np.float64)
            assert (v >= lo - ulp).all() and (v <= lo + cell + ulp).all()
            # the counts add up
            assert m["counts"][1] == nf + degenerate + duplicate
            assert nv <= occupied <= min(m["counts"][0], int(np.prod(r["box"][1], dtype=np.int64)))
    on, off = expected_simplified(name, True, True), expected_simplified(name, True, False)
    assert on["counts"][1] + on["counts"][4] == off["counts"][1] and on["counts"][3] == off["counts"][3]
    assert set(face_keys(on["faces"])) == set(face_keys(off["faces"]))  # dedupe drops faces, never a vertex
    assert on["vertices"].tobytes() == off["vertices"].tobytes()


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.endswith(" permuted")])
def test_the_output_does_not_depend_on_the_input_order(name):
    base = name.rsplit(" / ", 1)[0]
    for rgb in (True, False):
        for dedupe in (True, False):
            a, b = expected_simplified(base, rgb, dedupe), expected_simplified(name, rgb, dedupe)
            assert a["counts"] == b["counts"] and a["box"] == b["box"]
            assert a["vertices"].view(np.uint32).tobytes() == b["vertices"].view(np.uint32).tobytes()
            assert not rgb or np.array_equal(a["rgb8"], b["rgb8"])
            assert face_keys(a["faces"]) == face_keys(b["faces"])      # as multisets
            if name.endswith("vertices permuted"):                     # the faces keep their order
                assert np.array_equal(a["faces"], b["faces"])


def test_alone_in_its_cell_returns_the_input_renumbered():
    m, cell, origin = cases()["alone"]
    assert cell == H_ANALYTIC / 64 and m is smallest_blob()
    r = expected_simplified("alone")
    nv, nf = m["counts"]
    assert r["counts"] == (nv, nf, nv, 0, 0)
    d = np.abs(m["vertices"].astype(np.float64)[:, None, :] - r["vertices"].astype(np.float64)[None, :, :]).max(-1)
    to = d.argmin(1)                                                    # input vertex -> output vertex
    assert np.array_equal(np.sort(to), np.arange(nv))
    # q drops less than 2^-32 of a cell, the fp64 operations lose far less than that again, then one fp32 rounding
    bound = cell * 2.0 ** -31 + np.spacing(np.abs(m["vertices"])).astype(np.float64)
    assert (np.abs(m["vertices"].astype(np.float64) - r["vertices"].astype(np.float64)[to]) <= bound).all()
    assert np.array_equal(canonical(to[m["faces"]]), r["faces"])
    assert np.array_equal(m["rgb8"], r["rgb8"][to])                    # a mean of one colour


def test_known_counts():
    assert expected_simplified("copies", True, True)["counts"] == (3, 2, 3, 0, 100000)
    assert expected_simplified("copies", True, False)["counts"] == (3, 100002, 3, 0, 0)
    assert np.array_equal(expected_simplified("copies")["faces"], [[0, 1, 2], [0, 2, 1]])
    assert expected_simplified("fan in one cell")["counts"] == (3, 1, 3, 99998, 0)
    for name in ("one vertex", "one triangle in one cell", "two triangles in one cell"):
        r = expected_simplified(name)
        assert r["counts"][:3] == (0, 0, 1) and r["vertices"].shape == (0, 3) and r["faces"].shape == (0, 3)
    assert int(np.prod(expected_simplified("sparse box")["box"][1])) == 128 * 128 * 80 > 1 << 20
    m, cell, origin = cases()["lattice points"]
    assert (cells_host(m["vertices"], cell, origin)[1] == 0).all()     # exactly on the boundaries
    bad = cells_host(np.array([[0, 0, np.nan], [np.inf, 0, 0], [1e30, 0, 0], [0, -1e30, 0], [1.0, 2.0, 3.0]], np.float32), 1.0, (0, 0, 0))[2]
    assert bad.tolist() == [True, True, True, True, False]


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    faces = cpu_mesh()["faces"]
    with pytest.raises(TypeError, match="mesh"):
        mesh.simplify([torch.zeros(4, 3), faces], 1.0)
    for key, bad in (("vertices", np.zeros((4, 3), np.float32)), ("faces", faces.numpy()), ("rgb8", np.zeros((4, 3), np.uint8))):
        with pytest.raises(TypeError, match=key):
            mesh.simplify(dict(cpu_mesh(), **{key: bad}), 1.0)
    for key, bad, match in (("vertices", torch.zeros(4, 3, dtype=torch.float64), "vertices"), ("vertices", torch.zeros(4, 2), "vertices"),
                            ("faces", faces.long(), "faces"), ("faces", faces.t().contiguous(), "faces"),
                            ("rgb8", torch.zeros(4, 3), "rgb8"), ("rgb8", torch.zeros(3, 3, dtype=torch.uint8), "rgb8")):
        with pytest.raises(ValueError, match=match):
            mesh.simplify(dict(cpu_mesh(), **{key: bad}), 1.0)
    for bad in (0, 0.0, -1.0, math.nan, math.inf, None, "wide", True):
        with pytest.raises(ValueError, match="cell"):
            mesh.simplify(cpu_mesh(), bad)
    for bad in ((0.0, 0.0), (0.0, 0.0, math.nan), (0.0, math.inf, 0.0), 1.0, None, "abc", (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="origin"):
            mesh.simplify(cpu_mesh(), 1.0, origin=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="dedupe"):
            mesh.simplify(cpu_mesh(), 1.0, dedupe=bad)
    for bad in (-1, 1.5, None, math.nan, True):
        with pytest.raises(ValueError, match="max_bytes"):
            mesh.simplify(cpu_mesh(), 1.0, max_bytes=bad)
    for rgb in (True, False):
        with pytest.raises(NativeError):                                # valid arguments, CPU tensors: no fallback
            mesh.simplify(cpu_mesh(rgb), 1.0, origin=(0.5, 0.25, -1.0), dedupe=False, max_bytes=1 << 20)
    # the extract option is checked with the other arguments, before the extraction
    sparse = mesh.SparseTsdfVolume.__new__(mesh.SparseTsdfVolume)
    for vol in (DenseStub(colours=False), sparse):
        for bad in (0, -0.5, math.nan, math.inf, "wide", True):
            with pytest.raises(ValueError, match="simplify_cell"):
                vol.extract(simplify_cell=bad)
        with pytest.raises(TypeError):
            vol.extract(0.0, 1.0, None, None, 0, 0.0, 0.5)              # keyword-only
    assert "simplify_cell" in mesh._MESH_KEYS


def test_scene_mesh_checks_simplify_cell_before_it_renders(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    for bad in (0, -2.0, math.nan, "wide"):
        with pytest.raises(ValueError, match="simplify_cell"):
            mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, simplify_cell=bad)
    with pytest.raises(NativeError):                                    # an accepted option, a CPU scene
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, simplify_cell=0.4)


def test_simplify_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfMeshSimplify" in header and C.sizeof(N.LrfMeshSimplify) == 3 * 8 + 2 * 8 + 4 * 8 + 6 * 4 + 2 * 4
    assert built_lib.lrf_abi_version() == 7
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)

    def bounds(vertices=FAKE, Nv=5, origin=o3, cell=1.0, out=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_simplify_bounds(vertices, Nv, origin, cell, out, None))
    for bad in (0, -4, 1 << 31):
        assert "1 <= Nv < 2^31" in bounds(Nv=bad)
    for bad in (dict(vertices=None), dict(origin=None), dict(out=None)):
        assert bounds(**bad) == "lrf_mesh_simplify_bounds: null argument", bad
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        assert "origin" in bounds(origin=(C.c_double * 3)(*bad))
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert "cell must be finite and > 0" in bounds(cell=bad)
    assert "4-byte aligned" in bounds(vertices=FAKE + 2) and "4-byte aligned" in bounds(out=FAKE + 1)

    def simp(vertices_out=FAKE, rgb8_out=FAKE, faces_out=FAKE, counts=FAKE, wsp=FAKE, **over):
        a = filled(N.LrfMeshSimplify, dict(vertices=FAKE, rgb8=FAKE, faces=FAKE, Nv=5, Nf=3, cell=1.0, dedupe=1, origin=(0.0, 0.0, 0.0),
                                           dims=(4, 4, 4), lo=(0, 0, 0)), **over)
        return refused(built_lib, built_lib.lrf_mesh_simplify(C.byref(a), vertices_out, rgb8_out, faces_out, counts, wsp, None))
    for bad in (dict(Nv=0), dict(Nf=-1), dict(Nv=1 << 31), dict(Nf=1 << 31)):
        assert "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31" in simp(**bad), bad
    for bad in (dict(vertices=None), dict(faces=None), dict(vertices_out=None), dict(faces_out=None), dict(counts=None), dict(wsp=None)):
        assert simp(**bad) == "lrf_mesh_simplify: null argument", bad
    assert "go together" in simp(rgb8=None) and "go together" in simp(rgb8_out=None)
    for bad in ((0, 4, 4), (4, -1, 4), (2048, 2048, 512), (1 << 30, 2, 1), (65536, 65536, 65536)):
        assert "1 <= cells < 2^31" in simp(dims=bad), bad
    assert "2^30" in simp(lo=(-(1 << 30), 0, 0)) and "2^30" in simp(lo=((1 << 30) - 3, 0, 0))
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0)):
        assert "origin" in simp(origin=bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert "cell must be finite and > 0" in simp(cell=bad)
    for bad in (dict(vertices=FAKE + 2), dict(faces=FAKE + 1), dict(vertices_out=FAKE + 2), dict(faces_out=FAKE + 2)):
        assert "4-byte aligned" in simp(**bad), bad
    assert "8-byte aligned" in simp(counts=FAKE + 4) and "8-byte aligned" in simp(wsp=FAKE + 4)
    assert built_lib.lrf_mesh_simplify(None, FAKE, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_workspace_bytes_refuses_and_grows(built_lib):
    ws = built_lib.lrf_mesh_simplify_workspace_bytes
    top = (1 << 31) - 1
    for bad in ((0, 0, 1), (-1, 5, 1), (5, -1, 1), (1 << 31, 0, 1), (5, 1 << 31, 1), (5, 5, 0), (5, 5, -3), (5, 5, 1 << 31)):
        assert ws(*bad) == 0, bad
    assert ws(1, 0, 1) > 0 and ws(1, 0, 1) % 256 == 0 and ws(top, top, top) > top
    steps = (1, 2, 63, 64, 65, 1000, 1024, 1025, 4097, 100000, (1 << 20) + 1, 1 << 24, top)
    for fixed in ((1, 0, 1), (1000, 2000, 4096), (1 << 20, 1 << 21, 1 << 22)):
        for axis in range(3):
            sizes = []
            for n in steps:
                shape = list(fixed)
                shape[axis] = n
                sizes.append(ws(*shape))
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], (fixed, axis, sizes)
    # a table of at least twice the faces, the accumulators of every vertex, a bit per cell
    assert ws(5, 1 << 20, 1) >= 4 * 2 * (1 << 20) and ws(1 << 20, 0, 1) >= 40 * (1 << 20) and ws(1, 0, 1 << 30) >= (1 << 30) // 8


def test_simplify_kernels_use_no_scratch():
    """The kernels of lrf_mesh_simplify.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
