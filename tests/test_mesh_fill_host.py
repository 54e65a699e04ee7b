"""Hole filling without a GPU: properties of the numpy restatement of csrc/lrf_mesh_fill.inl (tests/mesh_fill_cases.py), argument
refusals before any native call (Python and C ABI), the new symbols, the workspace sizes, and the new kernels' scratch use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from localrf_amd.mesh import fill_holes, holes  # noqa: F401  (what every test here is about)
from mesh_fill_cases import (CASE_NAMES, CLOSABLE, E2E_BLOCK, HOLE_KEYS, UNCHANGED, boundary_host, cases, e2e_mesh_host, expected, fill_host,
                             loops_host)
from mesh_smooth_cases import topology_host
from mesh_util import DenseStub, bits, cpu_mesh, forbid_native, forbid_render

SYMBOLS = ("lrf_mesh_holes_workspace_bytes", "lrf_mesh_holes", "lrf_mesh_fill")
KERNELS = ("k_hf_zero", "k_hf_edges", "k_hf_next", "k_hf_lead", "k_hf_members", "k_hf_loops", "k_hf_emit", "k_hf_bytes", "k_hf_info")


def test_case_names_are_fixed_and_say_what_they_are():
    assert tuple(cases()) == CASE_NAMES and len(CASE_NAMES) == 23
    assert CLOSABLE == tuple(n for n in CASE_NAMES if cases()[n][2])
    for name in CASE_NAMES:
        m, max_edges, _ = cases()[name]
        assert 3 <= max_edges <= 4096 and m["faces"].shape[0] <= 80000
        fill = expected(name)["fill"]
        assert set(fill) == set(HOLE_KEYS) | {"added_vertices", "added_faces"}
        assert (fill["loops"] == 0) == (name in UNCHANGED), name
        assert fill["open_edges"] == fill["boundary_edges"] - fill["loop_edges"]
        assert fill["added_vertices"] == fill["loops"] and fill["added_faces"] == fill["loop_edges"]
    want = {"tetrahedron minus one face": (1, 3, 3, 0), "sphere minus 20": (20, 60, 3, 0), "sphere minus 90": (90, 270, 3, 0),
            "sphere caps 3": (1, 3, 3, 4), "sphere caps 64": (1, 64, 64, 65), "sphere caps 65": (1, 65, 65, 66),
            "fan 3 / max_edges 3": (1, 3, 3, 0), "fan 65 / max_edges 65": (1, 65, 65, 0), "fan 65 / max_edges 4096": (1, 65, 65, 0),
            "fan 1025 / max_edges 1025": (1, 1025, 1025, 0), "fan 65 / max_edges 64": (0, 0, 0, 65),
            "fan 1025 / max_edges 1024": (0, 0, 0, 1025), "bow tie": (0, 0, 0, 6), "three triangles on one edge": (0, 0, 0, 9),
            "one point": (0, 0, 0, 7), "an unreferenced vertex": (1, 3, 3, 0), "sphere": (0, 0, 0, 0), "colour halves": (2, 7, 4, 0),
            "a degenerate face": (1, 5, 5, 0)}
    for name, counts in want.items():
        fill = expected(name)["fill"]
        assert (fill["loops"], fill["loop_edges"], fill["longest_loop"], fill["open_edges"]) == counts, name
    assert expected("sphere minus 90")["fill"]["boundary_edges"] > 256      # the ordered scan crosses workgroups
    assert expected("strip")["fill"]["open_edges"] == expected("strip")["fill"]["boundary_edges"] == 80000
    assert expected("a degenerate face")["fill"]["degenerate_faces"] == 2
    assert expected("three triangles on one edge")["fill"]["nonmanifold_edges"] == 3
    assert cases()["sphere minus 20 / no colours"][0]["rgb8"] is None and cases()["sphere minus 20"][0]["rgb8"] is not None


@pytest.mark.parametrize("name", CASE_NAMES)
def test_properties_of_the_restatement(name):
    m, max_edges, closable = cases()[name]
    r = expected(name)
    nv, nf = m["vertices"].shape[0], m["faces"].shape[0]
    fill = r["fill"]
    # the input is the output's prefix, bit for bit
    assert r["vertices"].shape == (nv + fill["loops"], 3) and r["faces"].shape == (nf + fill["loop_edges"], 3)
    assert np.array_equal(bits(r["vertices"][:nv]), bits(m["vertices"])) and np.array_equal(r["faces"][:nf], m["faces"])
    assert (r["rgb8"] is None) == (m["rgb8"] is None)
    if m["rgb8"] is not None:
        assert r["rgb8"].shape == (nv + fill["loops"], 3) and np.array_equal(r["rgb8"][:nv], m["rgb8"])
    if name in UNCHANGED:
        assert r["vertices"] is m["vertices"] and r["faces"] is m["faces"]
    # every edge of a filled loop has found its reverse, and no edge has become non-manifold
    before, after = topology_host(m), topology_host(r)
    assert after["boundary_edges"] == fill["open_edges"] and after["nonmanifold_edges"] == before["nonmanifold_edges"]
    assert after["degenerate_faces"] == before["degenerate_faces"] == fill["degenerate_faces"]
    assert after["closed"] is closable
    # every new face is wound as the face across its rim edge, and holds its loop's vertex
    new = r["faces"][nf:].astype(np.int64)
    if new.size:
        a, b, boundary, _, _ = boundary_host(m)
        rim = set(zip(a[boundary].tolist(), b[boundary].tolist()))
        assert all((q, p) in rim for p, q in new[:, :2].tolist()) and (new[:, 2] >= nv).all()
        assert set(new[:, 2].tolist()) == set(range(nv, nv + fill["loops"]))
        inside = r["vertices"][nv:].astype(np.float64)
        assert (inside >= m["vertices"].min(0) - 1e-6).all() and (inside <= m["vertices"].max(0) + 1e-6).all()
    # a second fill adds nothing
    again = fill_host(r, max_edges)
    assert again["fill"]["loops"] == 0 and again["vertices"] is r["vertices"] and again["faces"] is r["faces"]
    assert again["fill"]["boundary_edges"] == fill["open_edges"]


def test_the_colour_mean_rounds_a_half_upwards_and_a_mean_is_a_mean():
    r = expected("colour halves")
    assert r["rgb8"][7:].tolist() == [[1, 1, 255], [0, 1, 1]]
    m = cases()["colour halves"][0]
    assert np.allclose(r["vertices"][7], m["vertices"][:4].astype(np.float64).mean(0), atol=1e-7)
    assert np.allclose(r["vertices"][8], m["vertices"][4:].astype(np.float64).mean(0), atol=1e-7)
    for name in ("sphere minus 20 / far", "sphere minus 20 / shifted", "fan 1025 / max_edges 1025"):
        m, r = cases()[name][0], expected(name)
        nv, nf = m["counts"]
        for k in range(r["fill"]["loops"]):
            rim = r["faces"][nf:][r["faces"][nf:, 2] == nv + k][:, 0]
            mean = m["vertices"][rim].astype(np.float64).mean(0)
            scale = np.abs(m["vertices"]).max()
            assert np.abs(r["vertices"][nv + k] - mean).max() <= scale * 2.0 ** -22, (name, k)


@pytest.mark.parametrize("name", ("sphere minus 20", "sphere caps 64", "colour halves", "fan 65 / max_edges 65", "a degenerate face"))
def test_the_set_of_new_vertices_does_not_depend_on_the_order_of_the_faces(name):
    m, max_edges, _ = cases()[name]
    nv = m["vertices"].shape[0]

    def new_rows(r):
        v = bits(r["vertices"][nv:]).astype(np.int64)
        rows = np.concatenate([v, r["rgb8"][nv:].astype(np.int64)], 1) if r["rgb8"] is not None else v
        return sorted(map(tuple, rows.tolist()))
    want = expected(name)
    for seed in (1, 2, 3):
        rng = np.random.default_rng(9000 + seed)
        f = m["faces"][rng.permutation(m["faces"].shape[0])]
        turn = rng.integers(0, 3, f.shape[0])
        f = np.stack([f[np.arange(f.shape[0]), (turn + k) % 3] for k in range(3)], 1).astype(np.int32)
        got = fill_host(dict(m, faces=np.ascontiguousarray(f)), max_edges)
        assert got["fill"] == want["fill"] and new_rows(got) == new_rows(want)
        if name == "sphere minus 20":                                       # ... their order does
            assert not np.array_equal(bits(got["vertices"]), bits(want["vertices"]))


def test_the_punched_volume_leaves_one_simple_loop():
    m = e2e_mesh_host()
    assert E2E_BLOCK == (27, 15, 16) and not topology_host(m)["closed"]
    loops, counts = loops_host(m, 64)
    assert counts["loops"] == 1 and counts["open_edges"] == 0 and counts["nonmanifold_edges"] == 0 and 3 <= len(loops[0]) <= 64
    assert topology_host(fill_host(m, 64))["closed"] is True


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    faces = cpu_mesh(rgb=False)["faces"]
    for fn in (mesh.holes, mesh.fill_holes):
        with pytest.raises(TypeError, match="mesh"):
            fn([torch.zeros(4, 3), faces])
        for key, bad in (("vertices", np.zeros((4, 3), np.float32)), ("faces", faces.numpy())):
            with pytest.raises(TypeError, match=key):
                fn(dict(cpu_mesh(rgb=False), **{key: bad}))
        for key, bad in (("vertices", torch.zeros(4, 3, dtype=torch.float64)), ("vertices", torch.zeros(4, 2)), ("faces", faces.long()),
                         ("faces", faces.t().contiguous()), ("rgb8", torch.zeros(4, 3))):
            with pytest.raises(ValueError, match=key):
                fn(dict(cpu_mesh(rgb=False), **{key: bad}))
        for bad in (2, 0, -1, 4097, 1.5, None, "ten", True, math.nan):          # 2: what "fan 3" would need to stay open
            with pytest.raises(ValueError, match="max_edges"):
                fn(cpu_mesh(rgb=False), max_edges=bad)
        with pytest.raises(ValueError, match="vertices"):                      # dtype and shape come before the other arguments
            fn(dict(cpu_mesh(rgb=False), vertices=torch.zeros(4, 2)), max_edges=2)
        for ok in (3, 64, 4096):
            with pytest.raises(NativeError):                                    # a valid mesh on the CPU: no fallback
                fn(cpu_mesh(rgb=False), max_edges=ok)
        with pytest.raises(NativeError):
            fn(cpu_mesh(rgb=False))
    # the extract option is checked with the other arguments, before the extraction
    sparse = mesh.SparseTsdfVolume.__new__(mesh.SparseTsdfVolume)
    for vol in (DenseStub(colours=False), sparse):
        for bad in (-1, 1, 2, 4097, 2.5, "three", True, None):
            with pytest.raises(ValueError, match="fill_holes"):
                vol.extract(fill_holes=bad)
        with pytest.raises(TypeError):
            vol.extract(0.0, 1.0, None, None, 0, 0.0, None, 0, False, 64)       # keyword-only
    assert "fill_holes" in mesh._MESH_KEYS
    assert "holes(mesh, max_edges)" in mesh.__doc__ and "fill_holes(mesh, max_edges)" in mesh.__doc__


def test_scene_mesh_checks_the_option_before_it_renders(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    for bad in (-1, 2, 4097, 0.5, "three", True):
        with pytest.raises(ValueError, match="fill_holes"):
            mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, fill_holes=bad)
    with pytest.raises(NativeError):                                            # an accepted option, a CPU scene
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, fill_holes=64)


def test_fill_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    import __graft_entry__ as ge
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "lrf_mesh_fill.inl" in ge.HEADERS
    assert "typedef struct LrfMeshHoles" in header and C.sizeof(N.LrfMeshHoles) == 3 * 8 + 2 * 8 + 3 * 8 + 2 * 4
    assert N.SYMBOLS["lrf_mesh_holes"][1] == [C.POINTER(N.LrfMeshHoles), C.c_void_p, C.c_void_p, C.c_void_p]
    assert len(N.SYMBOLS["lrf_mesh_fill"][1]) == 9 and N.SYMBOLS["lrf_mesh_fill"][1][4:6] == [C.c_int64, C.c_int64]
    assert "int lrf_mesh_holes(const LrfMeshHoles* m, int64_t* info /* device [8] */, void* workspace, void* stream);" in header
    assert ("int lrf_mesh_fill(const LrfMeshHoles* m, float* vertices_out, uint8_t* rgb8_out /* nullable */, int32_t* faces_out, "
            "int64_t cap_v,") in header
    assert built_lib.lrf_abi_version() == 7

    def args(**over):
        return filled(N.LrfMeshHoles, dict(vertices=FAKE, rgb8=None, faces=FAKE, Nv=5, Nf=3, max_edges=64, s=30, lo=(0.0, 0.0, 0.0)), **over)

    def holes(info=FAKE, wsp=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_holes(C.byref(args(**over)), info, wsp, None))

    def fill(vertices_out=FAKE + 0x1000, rgb8_out=None, faces_out=FAKE + 0x2000, cap_v=6, cap_f=6, info=FAKE, wsp=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_fill(C.byref(args(**over)), vertices_out, rgb8_out, faces_out, cap_v, cap_f, info, wsp, None))
    for fn, who in ((holes, "lrf_mesh_holes: "), (fill, "lrf_mesh_fill: ")):
        for bad in (dict(Nv=0), dict(Nv=-4), dict(Nv=1 << 31), dict(Nf=-1), dict(Nf=1 << 31), dict(Nf=(1 << 31) // 3 + 1)):
            assert fn(**bad) == who + "need 1 <= Nv < 2^31, 0 <= Nf and 3 Nf < 2^31", bad
        for bad in (dict(faces=None), dict(info=None), dict(wsp=None), dict(vertices=None)):
            assert fn(**bad) == who + "null argument", bad
        assert "4-byte aligned" in fn(faces=FAKE + 2) and "4-byte aligned" in fn(vertices=FAKE + 1)
        assert "8-byte aligned" in fn(info=FAKE + 4) and "8-byte aligned" in fn(wsp=FAKE + 4)
        for bad in (2, 0, -1, 4097, 1 << 30):
            assert fn(max_edges=bad) == who + "max_edges must lie in [3, 4096]"
        for bad in (257, -257, 1 << 30):
            assert "s must lie in [-256, 256]" in fn(s=bad)
        for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
            assert "lo must hold 3 finite values" in fn(lo=bad)
    assert built_lib.lrf_mesh_holes(None, FAKE, FAKE, None) != 0 and built_lib.lrf_mesh_fill(None, FAKE, None, FAKE, 6, 6, FAKE, FAKE, None) != 0
    assert fill(vertices_out=None).endswith(": null argument") and fill(faces_out=None).endswith(": null argument")
    assert "4-byte aligned" in fill(vertices_out=FAKE + 0x1002) and "4-byte aligned" in fill(faces_out=FAKE + 0x2001)
    assert "go together" in fill(rgb8_out=FAKE + 0x3000) and "go together" in fill(rgb8=FAKE + 0x3000)
    for bad in (dict(cap_v=4), dict(cap_f=2), dict(cap_v=1 << 31), dict(cap_f=1 << 31), dict(cap_v=-1)):
        assert "need Nv <= cap_v < 2^31 and Nf <= cap_f < 2^31" in fill(**bad), bad
    assert "must not be its input" in fill(vertices_out=FAKE) and "must not be its input" in fill(faces_out=FAKE)
    assert "must not be its input" in fill(rgb8=FAKE + 0x3000, rgb8_out=FAKE + 0x3000)


def test_workspace_bytes_refuse_are_aligned_and_hold_the_lists(built_lib):
    size, lists = built_lib.lrf_mesh_holes_workspace_bytes, built_lib.lrf_mesh_incidence_workspace_bytes
    top = (1 << 31) - 1
    for bad in ((0, 0), (-1, 5), (5, -1), (1 << 31, 0), (5, 1 << 31), (5, top), (5, top // 3 + 1)):
        assert size(*bad) == 0, bad

    def up(n):
        return (n + 255) // 256 * 256
    for nv in (1, 2, 255, 256, 257, 1000, 100000, (1 << 20) + 1, top):
        for nf in (0, 1, 3, 341, 342, 1000, 99998, 1 << 21, top // 3):
            got = size(nv, nf)
            groups = max(1, (3 * nf + 1023) // 1024)
            want = lists(nv, nf) + 256 + 256 + 3 * up(4 * nv) + 2 * up(12 * nf) + up(groups * (2 * 16 * 8 + 2 * 16 * 4 + 2 * 4))
            assert got == want and got % 8 == 0, (nv, nf)


def test_fill_kernels_use_no_scratch():
    """The kernels of lrf_mesh_fill.inl, and k_sm_edges around the loop they share with it, as __graft_entry__.build() compiles
    them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS + ("k_sm_edges",), match="exact")
