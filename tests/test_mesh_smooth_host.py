"""Mesh topology, vertex normals and smoothing without a GPU: properties of the numpy restatement of csrc/lrf_mesh_smooth.inl
(tests/mesh_smooth_cases.py), argument refusals before any native call (Python and C ABI), the new symbols, the workspace
sizes, and the new kernels' scratch use."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from localrf_amd.mesh import smooth, topology, vertex_normals  # noqa: F401  (what every test here is about)
from mesh_cases import SPHERE_C
from mesh_smooth_cases import (ANALYTIC, BIG_FAN, CASE_NAMES, E_NONE, FAR, ITERATIONS, PARAMS, SHIFT, SMOOTH_FULL, cases,
                               expected_normals, expected_smooth, expected_topology, smooth_arguments, smooth_host)
from mesh_util import DenseStub, bits, cpu_mesh, forbid_native, forbid_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lrf_mesh_incidence_workspace_bytes", "lrf_mesh_incidence", "lrf_mesh_topology", "lrf_mesh_vertex_normals",
           "lrf_mesh_smooth_bounds", "lrf_mesh_smooth_workspace_bytes", "lrf_mesh_smooth")
KERNELS = ("k_sm_zero", "k_sm_count", "k_sm_rows", "k_sm_starts", "k_sm_fill", "k_sm_edges", "k_sm_pinned", "k_sm_exponent",
           "k_sm_normals", "k_sm_bounds", "k_sm_step", "k_sm_copy")


def test_case_names_and_arguments_are_fixed():
    assert tuple(cases()) == CASE_NAMES and len(CASE_NAMES) == 6 * 5 + 9 + 8
    assert len(SMOOTH_FULL) == 24 and {a[0] for a in SMOOTH_FULL} == set(ITERATIONS) and {a[1:3] for a in SMOOTH_FULL} == set(PARAMS)
    for name in CASE_NAMES:
        args = smooth_arguments(name)
        assert {a[3] for a in args} == {"fixed", "free"}
        assert name == f"fan {BIG_FAN}" or {a[1:3] for a in args} == set(PARAMS)
    assert smooth_arguments(f"fan {BIG_FAN}")[0][0] == 2 and smooth_arguments("sphere") is SMOOTH_FULL


def test_closed_and_open_meshes():
    for name in ("tetrahedron", "sphere", "torus", "blobs", "blobs strays", "sphere noisy"):
        t = expected_topology(name)
        assert t["closed"] is True and t["boundary_edges"] == 0 and t["nonmanifold_edges"] == 0 and not t["boundary_vertices"].any()
    tie, strip = expected_topology("blobs tie"), expected_topology("strip")
    assert not tie["closed"] and tie["boundary_edges"] > 0 and tie["nonmanifold_edges"] == 0
    assert tie["boundary_vertices"].sum() == tie["boundary_edges"]          # closed border loops: as many vertices as edges
    assert not strip["closed"] and strip["nonmanifold_edges"] > 0
    assert expected_topology("one vertex")["closed"] and expected_topology("one triangle")["boundary_edges"] == 3
    t = expected_topology("two triangles on one edge")
    assert (t["boundary_edges"], t["nonmanifold_edges"]) == (4, 0) and t["boundary_vertices"].all()
    t = expected_topology("three triangles on one edge")                    # (0, 1) three times, its reverse never
    assert (t["boundary_edges"], t["nonmanifold_edges"]) == (9, 3)
    t = expected_topology("a degenerate face")
    assert t["degenerate_faces"] == 2 and t["boundary_edges"] == 5
    for n in (3, 65, 1025):
        t = expected_topology(f"fan {n}")
        assert (t["boundary_edges"], t["nonmanifold_edges"]) == (n, 0) and t["boundary_vertices"].all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_properties_of_the_normals(name):
    m, r = cases()[name], expected_normals(name)
    nv = m["vertices"].shape[0]
    assert r["S"].shape == (nv, 3) and r["S"].dtype == np.int64 and r["normals"].shape == (nv, 3) and r["normals"].dtype == np.float32
    length = np.sqrt((r["normals"].astype(np.float64) ** 2).sum(1))
    zero = length == 0
    assert int(zero.sum()) == r["zero_normals"] and (np.abs(length[~zero] - 1.0) < 3e-7).all()
    referenced = np.zeros(nv, bool)
    referenced[np.asarray(m["faces"], np.int64).reshape(-1)] = True
    assert zero[~referenced].all()                                          # an unreferenced vertex has no normal
    assert r["E"] != E_NONE or not r["S"].any()
    assert (np.abs(r["S"]) <= (1 << 41) * (1 << 20)).all()


def test_sphere_normals_point_outwards_and_one_point_has_none():
    centre = np.array(SPHERE_C)
    for name, c in (("sphere", centre), ("sphere / shifted", centre - SHIFT.astype(np.float64)), ("sphere / far", centre + FAR.astype(np.float64))):
        m, r = cases()[name], expected_normals(name)
        d = m["vertices"].astype(np.float64) - c
        assert (np.abs(np.sqrt((d * d).sum(1)) - 0.35) < 0.01).all()
        assert ((r["normals"].astype(np.float64) * d).sum(1) > 0).all()
    r = expected_normals("one point")
    assert r["zero_normals"] == 6 and r["E"] == E_NONE and not r["S"].any() and not r["normals"].any()
    assert expected_normals("one vertex")["zero_normals"] == 1 and expected_normals("blobs strays")["zero_normals"] == 3


def test_smoothing_a_noisy_sphere():
    m = cases()["sphere noisy"]

    def radii(v):
        d = v.astype(np.float64) - np.array(SPHERE_C)
        return np.sqrt((d * d).sum(1))
    before = radii(m["vertices"])
    taubin = radii(expected_smooth("sphere noisy", 10, 0.5, -0.53, "fixed")[0])
    laplace = radii(expected_smooth("sphere noisy", 10, 1.0, 0.0, "fixed")[0])
    assert taubin.var() < before.var()
    assert laplace.mean() < before.mean()
    one_point = cases()["one point"]
    for it in ITERATIONS:                                                   # zero extent: the input's bytes
        assert np.array_equal(bits(expected_smooth("one point", it, 0.5, -0.53, "free")[0]), bits(one_point["vertices"]))


@pytest.mark.parametrize("name", ("blobs tie", "strip", "two triangles on one edge", "a degenerate face", "fan 65", "blobs strays"))
def test_fixed_leaves_the_boundary_and_unreferenced_vertices_bit_equal(name):
    m, mask = cases()[name], expected_topology(name)["boundary_vertices"].astype(bool)
    nv = m["vertices"].shape[0]
    referenced = np.zeros(nv, bool)
    f = np.asarray(m["faces"], np.int64).reshape(-1, 3)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    referenced[f.reshape(-1)] = True
    for it, lam, mu, b in smooth_arguments(name):
        got, info = expected_smooth(name, it, lam, mu, b)
        stay = ~referenced | (mask if b == "fixed" else False)
        assert np.array_equal(bits(got)[stay], bits(m["vertices"])[stay])
        assert info["pinned"] == (int(mask.sum()) if b == "fixed" else 0)
        if it and name == "blobs tie":
            assert (bits(got)[~stay] != bits(m["vertices"])[~stay]).any()
            if b == "free":
                assert (bits(got)[mask] != bits(m["vertices"])[mask]).any()


@pytest.mark.parametrize("name", ANALYTIC)
def test_a_vertex_permutation_permutes_the_rows_and_a_face_permutation_changes_nothing(name):
    k = ANALYTIC.index(name)
    base = cases()[name]
    nv = base["vertices"].shape[0]
    p = np.random.default_rng(5000 + k).permutation(nv)                     # old vertex v is vertex p[v]
    vp, fp = name + " / vertices permuted", name + " / faces permuted"
    assert np.array_equal(cases()[vp]["vertices"][p], base["vertices"])
    t0, n0 = expected_topology(name), expected_normals(name)
    for other, rows in ((vp, p), (fp, np.arange(nv))):
        t, n = expected_topology(other), expected_normals(other)
        assert {k_: v for k_, v in t.items() if k_ != "boundary_vertices"} == {k_: v for k_, v in t0.items() if k_ != "boundary_vertices"}
        assert np.array_equal(t["boundary_vertices"][rows], t0["boundary_vertices"])
        assert n["E"] == n0["E"] and np.array_equal(n["S"][rows], n0["S"]) and np.array_equal(bits(n["normals"])[rows], bits(n0["normals"]))
        for args in smooth_arguments(other):
            a, b = smooth_host(base, *args), expected_smooth(other, *args)
            assert np.array_equal(bits(b[0])[rows], bits(a["vertices"][args[0]]))
            assert b[1] == {k_: a[k_] for k_ in b[1]}


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    faces = cpu_mesh(rgb=False)["faces"]
    calls = (mesh.topology, mesh.vertex_normals, mesh.smooth)
    for fn in calls:
        with pytest.raises(TypeError, match="mesh"):
            fn([torch.zeros(4, 3), faces])
        for key, bad in (("vertices", np.zeros((4, 3), np.float32)), ("faces", faces.numpy())):
            with pytest.raises(TypeError, match=key):
                fn(dict(cpu_mesh(rgb=False), **{key: bad}))
        for key, bad in (("vertices", torch.zeros(4, 3, dtype=torch.float64)), ("vertices", torch.zeros(4, 2)), ("faces", faces.long()),
                         ("faces", faces.t().contiguous()), ("rgb8", torch.zeros(4, 3))):
            with pytest.raises(ValueError, match=key):
                fn(dict(cpu_mesh(rgb=False), **{key: bad}))
        with pytest.raises(NativeError):                                    # a valid mesh on the CPU: no fallback
            fn(cpu_mesh(rgb=False))
    for bad in (-1, 1001, 1.5, None, "ten", True, math.nan):
        with pytest.raises(ValueError, match="iterations"):
            mesh.smooth(cpu_mesh(rgb=False), iterations=bad)
    for bad in (0, 0.0, -0.5, 1.0001, math.nan, math.inf, None, "half", True):
        with pytest.raises(ValueError, match="lam"):
            mesh.smooth(cpu_mesh(rgb=False), lam=bad)
    for bad in (0.01, -1.0001, math.nan, -math.inf, None, "half", True):
        with pytest.raises(ValueError, match="mu"):
            mesh.smooth(cpu_mesh(rgb=False), mu=bad)
    for bad in ("pinned", None, 0, True, "Fixed"):
        with pytest.raises(ValueError, match="boundary"):
            mesh.smooth(cpu_mesh(rgb=False), boundary=bad)
    with pytest.raises(ValueError, match="vertices"):                        # dtype and shape come before the other arguments
        mesh.smooth(dict(cpu_mesh(rgb=False), vertices=torch.zeros(4, 2)), iterations=-1)
    with pytest.raises(ValueError, match="iterations"):                      # ... and those before the device
        mesh.smooth(cpu_mesh(rgb=False), iterations=-1)
    for args in (dict(iterations=0), dict(iterations=1000, lam=1.0, mu=-1.0, boundary="free"), dict(lam=1e-9, mu=0.0)):
        with pytest.raises(NativeError):
            mesh.smooth(cpu_mesh(rgb=False), **args)
    # the extract options are checked with the other arguments, before the extraction
    sparse = mesh.SparseTsdfVolume.__new__(mesh.SparseTsdfVolume)
    for vol in (DenseStub(colours=False), sparse):
        for bad in (-1, 1001, 2.5, "three", True, None):
            with pytest.raises(ValueError, match="smooth_iterations"):
                vol.extract(smooth_iterations=bad)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="normals"):
                vol.extract(normals=bad)
        with pytest.raises(TypeError):
            vol.extract(0.0, 1.0, None, None, 0, 0.0, None, 3)              # keyword-only
    assert "smooth_iterations" in mesh._MESH_KEYS and "normals" in mesh._MESH_KEYS


def test_scene_mesh_checks_the_options_before_it_renders(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    for bad in (-1, 1001, 0.5, "three"):
        with pytest.raises(ValueError, match="smooth_iterations"):
            mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, smooth_iterations=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="normals"):
            mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, normals=bad)
    with pytest.raises(NativeError):                                        # accepted options, a CPU scene
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, smooth_iterations=3, normals=True)


def test_smooth_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    debug = open(os.path.join(ROOT, "include", "lrf_debug.h")).read()
    assert "lrf_debug_mesh_vertex_normals(" in debug and "lrf_debug_mesh_vertex_normals" in N.SYMBOLS
    assert "typedef struct LrfMeshSmooth" in header and C.sizeof(N.LrfMeshSmooth) == 2 * 8 + 2 * 8 + 5 * 8 + 4 * 4
    assert built_lib.lrf_abi_version() == 7
    sizes = (dict(Nv=0), dict(Nv=-4), dict(Nv=1 << 31), dict(Nf=-1), dict(Nf=1 << 31), dict(Nf=(1 << 31) // 3 + 1))

    def incidence(faces=FAKE, Nv=5, Nf=3, info=FAKE, wsp=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_incidence(faces, Nv, Nf, info, wsp, None))

    def topology(faces=FAKE, Nv=5, Nf=3, boundary=FAKE, info=FAKE, wsp=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_topology(faces, Nv, Nf, boundary, info, wsp, None))

    def normals(vertices=FAKE, faces=FAKE, Nv=5, Nf=3, out=FAKE, info=FAKE, wsp=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_vertex_normals(vertices, faces, Nv, Nf, out, info, wsp, None))

    def debug_normals(vertices=FAKE, faces=FAKE, Nv=5, Nf=3, out=FAKE, S=FAKE, E=FAKE, info=FAKE, wsp=FAKE):
        return refused(built_lib, built_lib.lrf_debug_mesh_vertex_normals(vertices, faces, Nv, Nf, out, S, E, info, wsp, None))

    def smooth(vertices_out=FAKE + 0x1000, info=FAKE, wsp=FAKE, **over):
        a = filled(N.LrfMeshSmooth, dict(vertices=FAKE, faces=FAKE, Nv=5, Nf=3, lam=0.5, mu=-0.53, s=30, iterations=2, pin_boundary=1,
                                         lo=(0.0, 0.0, 0.0)), **over)
        return refused(built_lib, built_lib.lrf_mesh_smooth(C.byref(a), vertices_out, info, wsp, None))
    for fn in (incidence, topology, normals, debug_normals, smooth):
        for bad in sizes:
            assert "need 1 <= Nv < 2^31, 0 <= Nf and 3 Nf < 2^31" in fn(**bad), (fn.__name__, bad)
        for bad in (dict(faces=None), dict(info=None), dict(wsp=None)):
            assert fn(**bad).endswith(": null argument"), (fn.__name__, bad)
        assert "4-byte aligned" in fn(faces=FAKE + 2) and "8-byte aligned" in fn(info=FAKE + 4) and "8-byte aligned" in fn(wsp=FAKE + 4)
    assert topology(boundary=None).endswith(": null argument")
    for fn in (normals, debug_normals):
        assert fn(vertices=None).endswith(": null argument") and fn(out=None).endswith(": null argument")
        assert "4-byte aligned" in fn(vertices=FAKE + 2) and "4-byte aligned" in fn(out=FAKE + 1)
    assert debug_normals(S=None).endswith(": null argument") and debug_normals(E=None).endswith(": null argument")
    assert "8-byte aligned" in debug_normals(S=FAKE + 4) and "4-byte aligned" in debug_normals(E=FAKE + 2)
    assert smooth(vertices=None).endswith(": null argument") and smooth(vertices_out=None).endswith(": null argument")
    assert "4-byte aligned" in smooth(vertices=FAKE + 2) and "4-byte aligned" in smooth(vertices_out=FAKE + 0x1002)
    assert "must not be the input" in smooth(vertices_out=FAKE)
    for bad in (-1, 1001):
        assert "iterations" in smooth(iterations=bad)
    for bad in (0.0, -0.5, 1.5, math.nan, math.inf):
        assert "0 < lam <= 1" in smooth(lam=bad)
    for bad in (0.5, -1.5, math.nan, -math.inf):
        assert "-1 <= mu <= 0" in smooth(mu=bad)
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        assert "lo must hold 3 finite values" in smooth(lo=bad)
    for bad in (257, -257, 1 << 30):
        assert "s must lie" in smooth(s=bad)
    assert built_lib.lrf_mesh_smooth(None, FAKE, FAKE, FAKE, None) != 0

    def bounds(vertices=FAKE, Nv=5, out=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_smooth_bounds(vertices, Nv, out, None))
    for bad in (0, -4, 1 << 31):
        assert "1 <= Nv < 2^31" in bounds(Nv=bad)
    assert bounds(vertices=None).endswith(": null argument") and bounds(out=None).endswith(": null argument")
    assert "4-byte aligned" in bounds(vertices=FAKE + 2) and "4-byte aligned" in bounds(out=FAKE + 1)


def test_workspace_bytes_refuse_and_follow_the_formula(built_lib):
    lists, smooth = built_lib.lrf_mesh_incidence_workspace_bytes, built_lib.lrf_mesh_smooth_workspace_bytes
    top = (1 << 31) - 1
    for bad in ((0, 0), (-1, 5), (5, -1), (1 << 31, 0), (5, 1 << 31), (5, top), (5, top // 3 + 1)):
        assert lists(*bad) == 0 and smooth(*bad) == 0, bad

    def up(n):
        return (n + 255) // 256 * 256
    for nv in (1, 2, 255, 256, 257, 1000, 100000, (1 << 20) + 1, top):
        for nf in (0, 1, 3, 1000, 99998, 1 << 21, top // 3):
            want = up(8 + 4 * (nv + 1) + 4 * nv + 4 * ((nv + 255) // 256) + 12 * nf + nv)
            assert lists(nv, nf) == want, (nv, nf)
            assert smooth(nv, nf) == up(want + 12 * nv), (nv, nf)


def test_smooth_kernels_use_no_scratch():
    """The kernels of lrf_mesh_smooth.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
