"""Quadric placement of the clustering simplifier without a GPU: properties of the numpy restatement of rules a-d of
csrc/lrf_mesh_simplify.inl (tests/mesh_simplify_quadric_cases.py) on every case, the volume it keeps against mean placement,
argument refusals before any native call (Python and C ABI), the new symbols, the workspace size, and the new kernels'
scratch use."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from mesh_simplify_cases import expected_simplified, face_keys
from mesh_simplify_quadric_cases import (ANALYTIC_NAMES, CAP, CAPPED, CASE_NAMES, CUBE_HI, CUBE_LO, PLANE, REGULARIZE, cases,
                                         expected_quadric, signed_volume)
from mesh_util import cpu_mesh, forbid_native

SYMBOLS = ("lrf_mesh_simplify_quadric_workspace_bytes", "lrf_mesh_simplify_quadric")
KERNELS = ("k_ms_quadric_zero", "k_ms_quadric_exponent", "k_ms_quadric_accumulate", "k_ms_quadric_place")
# the rows of the issue's table: |signed volume out - signed volume in| must fall; the torus at 9 steps collapses to zero
# volume under both placements and is left out
VOLUME_ROWS = tuple((name, steps) for name in ("sphere", "torus", "blobs") for steps in ("2", "3.5", "9") if (name, steps) != ("torus", "9"))


def test_case_names_are_fixed():
    assert len(ANALYTIC_NAMES) == 3 * (3 * 2 + 3 * 3) * 3 and len(CASE_NAMES) == len(ANALYTIC_NAMES) + 6 + 5
    assert len(set(CASE_NAMES)) == len(CASE_NAMES) and CAPPED not in CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_properties_of_the_restatement(name):
    m, cell, origin = cases()[name]
    for rgb, dedupe in ((True, True), (False, False)):
        r = expected_quadric(name, rgb, dedupe)
        base = expected_simplified(name, rgb, dedupe) if name in ANALYTIC_NAMES else None
        v = r["vertices"]
        nv, nf, occupied, degenerate, duplicate, fallback, clamped = r["counts"]
        assert v.dtype == np.float32 and v.shape == (nv, 3) and 0 <= fallback <= nv and 0 <= clamped <= nv - fallback
        # every vertex lies in its closed cell, to one fp32 ulp
        lo = np.asarray(origin, np.float64) + r["cells"].astype(np.float64) * cell
        ulp = np.spacing(np.maximum(np.abs(v), np.abs((lo + cell).astype(np.float32)))).astype(np.float64)
        assert (v >= lo - ulp).all() and (v <= lo + cell + ulp).all()
        # a vertex left at the mean carries the mean's bits; the rule says which
        at_mean = r["mean_placed"]
        assert np.array_equal(v[at_mean].view(np.uint32), r["mean_vertices"][at_mean].view(np.uint32)) and int(at_mean.sum()) == fallback
        assert np.array_equal(at_mean, (r["contributions"] == 0) | (r["contributions"] >= CAP))    # no cluster failed to solve
        # everything but the positions is simplify_host's
        if base is not None:
            assert r["counts"][:5] == base["counts"] and r["box"] == base["box"] and np.array_equal(r["faces"], base["faces"])
            assert (r["rgb8"] is None) == (not rgb) and (not rgb or np.array_equal(r["rgb8"], base["rgb8"]))
            assert np.array_equal(r["mean_vertices"].view(np.uint32), base["vertices"].view(np.uint32))
    # the placement reads neither rgb8 nor dedupe
    on, off = expected_quadric(name, True, True), expected_quadric(name, True, False)
    assert on["vertices"].tobytes() == off["vertices"].tobytes() == expected_quadric(name, False, True)["vertices"].tobytes()


@pytest.mark.parametrize("name", [n for n in ANALYTIC_NAMES if n.endswith(" permuted")])
def test_the_output_does_not_depend_on_the_input_order(name):
    base = name.rsplit(" / ", 1)[0]
    a, b = expected_quadric(base), expected_quadric(name)
    assert a["counts"] == b["counts"] and a["box"] == b["box"]
    assert a["vertices"].view(np.uint32).tobytes() == b["vertices"].view(np.uint32).tobytes()
    assert face_keys(a["faces"]) == face_keys(b["faces"])
    assert a["vertices"].tobytes() != a["mean_vertices"].tobytes()      # and it is not the mean placement


def test_the_volume_error_falls_on_every_row_and_halves_at_two_steps():
    for name, steps in VOLUME_ROWS:
        tag = f"{name} / {steps} steps / origin 0"
        m = cases()[tag][0]
        r = expected_quadric(tag)
        want = signed_volume(m["vertices"], m["faces"])
        mean = abs(signed_volume(r["mean_vertices"], r["faces"]) - want)
        quadric = abs(signed_volume(r["vertices"], r["faces"]) - want)
        print(f"{tag}: |volume error| mean {mean:.5f} quadric {quadric:.5f} ratio {quadric / mean:.3f}")
        assert quadric < mean, (tag, mean, quadric)
        if steps == "2":
            assert quadric <= 0.5 * mean, (tag, mean, quadric)


def test_cube_corners_stay_sharper_than_under_mean_placement():
    r = expected_quadric("cube")
    assert r["counts"][:2] == (56, 108) and r["counts"][5] == 0
    seen = 0
    for corner in np.array(np.meshgrid(*[(CUBE_LO, CUBE_HI)] * 3, indexing="ij")).reshape(3, -1).T:
        row = np.nonzero((r["cells"] == np.floor(corner).astype(np.int64)).all(1))[0]
        assert row.size == 1
        q = np.abs(r["vertices"][row[0]].astype(np.float64) - corner).max()
        mean = np.abs(r["mean_vertices"][row[0]].astype(np.float64) - corner).max()
        print(f"corner {corner}: quadric {q:.5f} mean {mean:.5f}")
        # three planes meet in the corner: the regulariser alone moves the minimum, by about regularize * |corner - mean|
        assert q < mean and q < 8 * REGULARIZE * mean
        seen += 1
    assert seen == 8


def test_a_planar_patch_stays_in_its_plane():
    r = expected_quadric("planar patch")
    assert r["counts"] == (3, 1, 3, 4, 0, 0, 0)
    v = r["vertices"].astype(np.float64)
    off = np.abs(PLANE[0] * v[:, 0] + PLANE[1] * v[:, 1] + PLANE[2] - v[:, 2])
    assert (off < 1e-6).all(), off                                      # fp32 vertices of a plane with coefficients below 1
    # inside the plane the regulariser decides: the mean's projection, which for a vertex set of the plane is the mean
    assert np.abs(v - r["mean_vertices"].astype(np.float64)).max() < 1e-5


def test_zero_area_and_capped_clusters_take_the_mean_bit_for_bit():
    r = expected_quadric("zero area")
    assert r["counts"] == (3, 1, 3, 3, 1, 3, 0) and (r["contributions"] == 0).all()
    assert r["vertices"].tobytes() == r["mean_vertices"].tobytes()
    assert expected_quadric("repeated indices")["counts"][:5] == (3, 1, 3, 5, 1)
    r = expected_quadric(CAPPED, False, True)
    assert r["counts"] == (3, 1, 3, CAP + 3, 0, 1, 0) and r["contributions"].tolist() == [CAP + 4, 1, 1]
    assert r["mean_placed"].tolist() == [True, False, False]
    assert r["vertices"][0].tobytes() == r["mean_vertices"][0].tobytes()
    r = expected_quadric("fan in one cell")                              # 99 999 contributions: below the cap, solved
    assert r["contributions"].tolist() == [99999, 1, 1] and r["counts"][5] == 0


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    sig = inspect.signature(mesh.simplify).parameters
    assert [sig[k].kind for k in ("placement", "regularize")] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert sig["placement"].default == "mean" and sig["regularize"].default == 2.0 ** -10
    with pytest.raises(TypeError):
        mesh.simplify(cpu_mesh(), 1.0, (0.0, 0.0, 0.0), True, 1 << 30, "quadric")
    for bad in ("Quadric", "qem", "", None, 1, True, b"mean", ("mean",)):
        with pytest.raises(ValueError, match="placement"):
            mesh.simplify(cpu_mesh(), 1.0, placement=bad)
    for bad in (0, 0.0, -0.5, 1.5, math.nan, math.inf, None, "small", True):
        for placement in ("mean", "quadric"):
            with pytest.raises(ValueError, match="regularize"):
                mesh.simplify(cpu_mesh(), 1.0, placement=placement, regularize=bad)
    # the arguments before them are refused first, the device last
    with pytest.raises(TypeError, match="mesh"):
        mesh.simplify([], 1.0, placement="nowhere")
    with pytest.raises(ValueError, match="max_bytes"):
        mesh.simplify(cpu_mesh(), 1.0, max_bytes=-1, placement="nowhere")
    with pytest.raises(ValueError, match="placement"):
        mesh.simplify(cpu_mesh(), 1.0, placement="nowhere", regularize=0.0)
    for rgb in (True, False):
        for kw in (dict(placement="quadric"), dict(placement="quadric", regularize=1.0), dict(placement="mean", regularize=0.5)):
            with pytest.raises(NativeError):                            # valid arguments, CPU tensors: no fallback
                mesh.simplify(cpu_mesh(rgb), 1.0, origin=(0.5, 0.25, -1.0), dedupe=False, **kw)
    assert "placement" not in mesh._MESH_KEYS and "regularize" not in mesh._MESH_KEYS     # the chain is not touched


def test_quadric_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfMeshSimplifyQuadric" in header
    assert C.sizeof(N.LrfMeshSimplifyQuadric) == C.sizeof(N.LrfMeshSimplify) + 8 == 112
    assert N.LrfMeshSimplifyQuadric.mesh.offset == 0 and N.LrfMeshSimplifyQuadric.regularize.offset == 104
    assert built_lib.lrf_abi_version() == 7

    def simp(vertices_out=FAKE, rgb8_out=FAKE, faces_out=FAKE, counts=FAKE, wsp=FAKE, regularize=REGULARIZE, **over):
        q = N.LrfMeshSimplifyQuadric()
        q.regularize = regularize
        q.mesh = filled(N.LrfMeshSimplify, dict(vertices=FAKE, rgb8=FAKE, faces=FAKE, Nv=5, Nf=3, cell=1.0, dedupe=1, origin=(0.0, 0.0, 0.0),
                                                dims=(4, 4, 4), lo=(0, 0, 0)), **over)
        return refused(built_lib, built_lib.lrf_mesh_simplify_quadric(C.byref(q), vertices_out, rgb8_out, faces_out, counts, wsp, None))
    for bad in (dict(Nv=0), dict(Nf=-1), dict(Nv=1 << 31), dict(Nf=1 << 31)):
        assert "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31" in simp(**bad), bad
    for bad in (dict(vertices=None), dict(faces=None), dict(vertices_out=None), dict(faces_out=None), dict(counts=None), dict(wsp=None)):
        assert simp(**bad) == "lrf_mesh_simplify_quadric: null argument", bad
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
    for bad in (0.0, -0.0, -2.0 ** -10, 1.0000000000000002, 2.0, math.nan, math.inf, -math.inf):
        assert simp(regularize=bad) == "lrf_mesh_simplify_quadric: regularize must lie in (0, 1]", bad
    assert built_lib.lrf_mesh_simplify_quadric(None, FAKE, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_workspace_bytes_refuses_and_holds_the_sums(built_lib):
    ws, mean = built_lib.lrf_mesh_simplify_quadric_workspace_bytes, built_lib.lrf_mesh_simplify_workspace_bytes
    top = (1 << 31) - 1
    for bad in ((0, 0, 1), (-1, 5, 1), (5, -1, 1), (1 << 31, 0, 1), (5, 1 << 31, 1), (5, 5, 0), (5, 5, -3), (5, 5, 1 << 31)):
        assert ws(*bad) == 0, bad
    for shape in ((1, 0, 1), (5, 3, 64), (1000, 2000, 4096), (2902, 5780, 1728), (1 << 20, 1 << 21, 1 << 22), (top, top, top)):
        nv = shape[0]
        # the mean's workspace as one piece, then nine int64 sums, a count and an exponent per vertex, padded to 256 bytes
        assert ws(*shape) == (mean(*shape) + (9 * 8 + 4 + 4) * nv + 255) // 256 * 256 and ws(*shape) % 256 == 0, shape


def test_quadric_kernels_use_no_scratch():
    """The new kernels as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
