"""The point-to-mesh distance without a GPU: the numpy restatement of csrc/lrf_mesh_distance.inl (tests/mesh_distance_cases.py)
against exact rational arithmetic, the grid walk's termination argument against the brute force, the sampling's and the
summary's properties, argument refusals before any native call (Python and C ABI), the new symbols, the grid's size, and the
kernels' scratch use.

Measured with the committed restatement on the committed cases (160 per kind), |d - d_exact| / L with L the largest absolute
coordinate difference between the point and the corners, over the fp64 result before its fp32 rounding:
  random 1.19e-16, zero-area 2.27e-16, single-point 1.85e-16, near-surface 1.37e-16, on-surface 8.75e-17,
  sliver 3.74e-12 (half of those points lie over the sliver, where the plane term is taken: the cross product of two nearly
  parallel edges cancels, which leaves the normal's direction with a relative error of about 2^-53 / sin(angle); the distance is
  still right to well below one ulp of an fp32 coordinate).
Each kind's bar is four times its own figure: the bars guard the formulation, not one platform's last bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh_distance
from localrf_amd.mesh_distance import MeshIndex, cloud_to_mesh, distance_summary, sample_surface
from mesh_distance_cases import (CASE_NAMES, CLAMP, QUERY_SIZES, SAMPLE_CASES, SCALE, SUMMARY_SIZES, SUMMARY_TAUS, TRIANGLE, _pairs,
                                 box_host, cases, default_cell_host, dims_host, exact_cases, exact_error, exact_pair, expected,
                                 grid_host, grid_search_host, mean_edge, pair_host, sample_host, slabs, summary_host, summary_inputs,
                                 used_faces)
from mesh_clean_cases import permute_faces
from mesh_util import cpu_mesh, forbid_native

SYMBOLS = ("lrf_mesh_index_bounds", "lrf_mesh_index_workspace_bytes", "lrf_mesh_index_build", "lrf_mesh_closest", "lrf_mesh_sample_count",
           "lrf_mesh_sample_emit", "lrf_distance_summary")
KERNELS = ("k_md_bounds_init", "k_md_bounds", "k_md_zero", "k_md_fill", "k_md_closest", "k_md_sample_count", "k_md_sample_emit",
           "k_md_summary")
EXACT_MEASURED = {"random": 1.19e-16, "sliver": 3.74e-12, "zero-area": 2.27e-16, "single-point": 1.85e-16, "near-surface": 1.37e-16,
                  "on-surface": 8.75e-17}
EXACT_BAR = {k: 4 * v for k, v in EXACT_MEASURED.items()}


def test_the_cases_cover_what_they_should():
    cs = cases()
    assert {c["mesh"]["faces"].shape[0] for c in cs.values()} >= {0, 1, 2, 512}
    assert {cs[f"one triangle N={n}"]["points"].shape[0] for n in QUERY_SIZES} == set(QUERY_SIZES)
    edge = mean_edge(cs["octa 512 N=1025"]["mesh"])
    assert any(abs(c - 10 * edge) < 1e-12 for c in cs["octa 512 N=1025"]["cells"] if c)
    small = cs["octa 32 cell a tenth of the edge"]
    assert abs(small["cells"][0] - 0.1 * mean_edge(small["mesh"])) < 1e-12
    assert dims_host(*box_host(cs["grid of 1 x 1 x 1"]["mesh"]), 100.0) == (1, 1, 1)
    lo, hi = box_host(cs["planar, one cell thick"]["mesh"])
    assert dims_host(lo, hi, default_cell_host(lo, hi, 128))[2] == 1
    c = cs["one face spans every cell"]
    lo, dims, lists = grid_host(c["mesh"], 0.125)
    nf = c["mesh"]["faces"].shape[0]
    assert math.prod(dims) > 100 and all(nf - 2 in lists[i] or nf - 1 in lists[i] for i in range(math.prod(dims)))
    assert sum(nf - 2 in l for l in lists.values()) == math.prod(dims)
    c = cs["fan: 68 faces in one cell"]
    assert len(grid_host(c["mesh"], 100.0)[2][0]) == 68
    e = expected("bad faces, special points")
    assert e["info"] == {"bad_index_faces": 4, "nonfinite_faces": 3, "used_faces": 32} and np.isnan(e["distance"]).sum() == 4
    assert expected("no used face")["info"]["used_faces"] == 0


def test_exact_distances_at_multiples_of_the_cell_ties_and_cutoffs():
    e = expected("slabs at multiples of the cell, max_distance inf")
    p = cases()["slabs at multiples of the cell, max_distance inf"]["points"]
    col = np.nonzero((p[:, 0] == 1.25) & (p[:, 1] == 1.0))[0]
    z = p[col, 2].astype(np.float64)
    want = np.minimum(np.abs(z), np.abs(z + 1))
    assert np.array_equal(e["distance"][col], want.astype(np.float32))              # exact: multiples of the cell 0.5 among them
    assert {0.5, 1.0, 1.5, 2.0} <= set(e["distance"][col].tolist())
    assert np.array_equal(e["face"][col], np.where(np.abs(z + 1) <= np.abs(z), 0, 1))     # equally far (z = -0.5): the smaller index
    assert (e["face"][col][z == -0.5] == 0).all() and (z == -0.5).sum() == 1
    mid = expected("slabs at multiples of the cell, max_distance 0.5")
    assert ((mid["face"] >= 0) == (e["distance"] <= 0.5)).all() and (mid["face"] >= 0).sum() not in (0, p.shape[0])
    assert np.array_equal(mid["distance"][mid["face"] >= 0], e["distance"][mid["face"] >= 0])
    zero = expected("slabs at multiples of the cell, max_distance 0.0")
    assert ((zero["face"] >= 0) == (e["distance"] == 0)).all() and (zero["face"] >= 0).sum() == 2
    two = expected("two coincident faces")
    assert (two["face"] == 0).all()
    octa = expected("octa 512 N=1025")
    assert (octa["distance"] == 0).sum() >= 100                                     # the queries on vertices


@pytest.mark.parametrize("kind", tuple(EXACT_MEASURED))
def test_the_pair_against_exact_rational_arithmetic(kind):
    """|d - d_exact| / L of the restated pair function (the .inl's operation order) against fractions.Fraction; measured figures
    and bars: the module docstring.  Never NaN; a face without area gives the exact segment's or point's distance within the bar."""
    p, x = exact_cases()[kind]
    with np.errstate(all="ignore"):
        d2, q, term = pair_host(p, x)
    assert np.isfinite(d2).all() and np.isfinite(q).all() and (d2 >= 0).all()
    worst = max(exact_error(p[i], x[i], float(d2[i])) for i in range(p.shape[0]))
    print(f"{kind}: largest |d - d_exact| / L = {worst:.3e} (measured {EXACT_MEASURED[kind]:.3e}, bar {EXACT_BAR[kind]:.3e})")
    assert worst <= EXACT_BAR[kind]
    if kind in ("zero-area", "single-point"):
        assert (term < 3).all()                                                     # no plane term without a plane
    if kind == "sliver":
        assert (term == 3).sum() > 40
    on_face = np.abs(q.astype(np.float64) - p.astype(np.float64)).max(1)
    assert (np.sqrt(d2) <= on_face * math.sqrt(3) + 1e-12).all()                    # the closest point is that far away


def test_the_pair_is_exact_on_small_integers_and_degenerate_input():
    tri = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], np.float32)
    for p, want in (((1, 1, 3), 9), ((-3, -4, 0), 25), ((5, 0, 0), 1), ((2, 2, 0), 0), ((3, 3, 0), 2), ((1, -2, 0), 4), ((0, 0, 0), 0)):
        d2, q, term = pair_host(np.array(p, np.float32), tri)
        assert float(d2) == want == float(exact_pair(np.array(p, np.float32), tri)), p
    seg = np.array([(0, 0, 0), (2, 0, 0), (1, 0, 0)], np.float32)
    pt = np.zeros((3, 3), np.float32) + np.float32(1.5)
    for x in (seg, seg[[0, 0, 1]], pt):
        d2, q, term = pair_host(np.array((1, 2, 0), np.float32), x)
        assert float(d2) == float(exact_pair(np.array((1, 2, 0), np.float32), x)) and term < 3
    big = np.array([(3e38, 0, 0), (-3e38, 3e38, 0), (0, -3e38, 3e38)], np.float32)
    tiny = np.array([(1e-45, 0, 0), (0, 1e-45, 0), (0, 0, 1e-45)], np.float32)
    for x in (big, tiny):
        for p in ((3e38, 3e38, -3e38), (0, 0, 0), (1e-45, 1e-45, 0)):
            with np.errstate(all="ignore"):
                d2, q, term = pair_host(np.array(p, np.float32), x)
            assert np.isfinite(d2) and np.isfinite(q).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_grid_walk_equals_the_brute_force(name):
    """The .inl's shells and stopping rule in pure Python against the minimum over every pair: the termination argument."""
    c, e = cases()[name], expected(name)
    kind, d2 = _pairs(name)
    if not (kind == 0).any():
        assert (e["face"] == -1).all()
        return
    cell = c["host_cell"]
    if cell is None:
        cell = default_cell_host(*box_host(c["mesh"]), int((kind == 0).sum()))
    best, face, shells = grid_search_host(c["mesh"], c["points"], cell, c["max_distance"], d2)
    assert np.array_equal(face, e["face"]) and np.array_equal(best, e["d2"])
    if c["points"].shape[0] >= 63 and math.isinf(c["max_distance"]) and math.prod(dims_host(*box_host(c["mesh"]), cell)) > 27:
        assert shells.min() < shells.max()                                          # near queries stop early, far ones walk on


def test_the_result_does_not_depend_on_the_cell():
    name = "octa 512 default cell"
    c, e = cases()[name], expected(name)
    kind, d2 = _pairs(name)
    for cell in (0.07, 0.33, 5.0):
        best, face, _ = grid_search_host(c["mesh"], c["points"], cell, math.inf, d2)
        assert np.array_equal(face, e["face"]) and np.array_equal(best, e["d2"])


def test_a_face_permutation_maps_the_faces():
    a, b = expected("octa 512 default cell"), expected("octa faces permuted")
    assert np.array_equal(a["distance"], b["distance"])
    fa, fb = cases()["octa 512 default cell"]["mesh"]["faces"], cases()["octa faces permuted"]["mesh"]["faces"]
    kind, d2 = _pairs("octa 512 default cell")
    alone = (d2 == d2.min(1, keepdims=True)).sum(1) == 1
    assert alone.sum() > 20 and np.array_equal(fa[a["face"][alone]], fb[b["face"][alone]])
    c = expected("octa vertices permuted")
    assert np.array_equal(a["distance"], c["distance"]) and np.array_equal(a["face"], c["face"])


@pytest.mark.parametrize("name", tuple(SAMPLE_CASES))
def test_samples_lie_on_their_faces_and_their_number_follows_the_area(name):
    make, spacing = SAMPLE_CASES[name]
    mesh = make()
    s = sample_host(mesh, spacing)
    kind, x = used_faces(mesh)
    x64 = x.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(x64[:, 1] - x64[:, 0], x64[:, 2] - x64[:, 0]), axis=1)
    want = area / spacing ** 2
    assert (np.abs(s["per_face"] - want) < 1).all() and (s["per_face"][kind != 0] == 0).all()
    # a sum of independent roundings, each of variance at most 1/4: six standard deviations
    assert abs(s["counts"][0] - want.sum()) <= 6 * math.sqrt(max((kind == 0).sum(), 1) / 4) + 1
    assert s["points"].shape == (s["counts"][0], 3) and (np.diff(s["face"]) >= 0).all()
    if not s["counts"][0]:
        return
    with np.errstate(all="ignore"):
        d2 = pair_host(s["points"], x[s["face"]])[0]
    scale = float(np.abs(x[kind == 0]).max())
    assert np.sqrt(d2.max()) <= 2.0 ** -22 * scale
    if "octa" in name or "sphere" in name:                                          # well spread: every sizeable face is hit
        assert (s["per_face"][want >= 2] >= 1).all()


def test_the_sample_set_ignores_face_order_and_corner_rotation():
    make, spacing = SAMPLE_CASES["octa 512 at 0.05"]
    mesh = make()
    a = sample_host(mesh, spacing)
    rows = lambda s: sorted(map(bytes, np.ascontiguousarray(s["points"])))
    assert rows(a) == rows(sample_host(permute_faces(mesh, 5), spacing))
    rolled = dict(mesh, faces=np.concatenate([np.roll(mesh["faces"][:200], 1, 1), np.roll(mesh["faces"][200:], 2, 1)]))
    b = sample_host(rolled, spacing)
    assert np.array_equal(a["points"], b["points"]) and np.array_equal(a["face"], b["face"])
    mirrored = dict(mesh, faces=np.ascontiguousarray(mesh["faces"][:, ::-1]))      # another face: other samples, the same number law
    assert abs(sample_host(mirrored, spacing)["counts"][0] - a["counts"][0]) < 200
    assert len(set(rows(a))) > 0.99 * a["counts"][0]


@pytest.mark.parametrize("n", SUMMARY_SIZES)
def test_summary_identities(n):
    d = summary_inputs(50 + n, n)
    s = summary_host(d, SUMMARY_TAUS, 0.5)
    assert s["finite"] + s["beyond"] + s["nan"] == n
    assert all(a <= b for a, b in zip(s["within"], s["within"][1:])) and all(w <= s["finite"] for w in s["within"])
    fin = d[np.isfinite(d)]
    if fin.size:
        plain = np.minimum(fin.astype(np.float64) / 0.5, CLAMP)
        assert abs(s["mean"] - plain.mean() * 0.5) < 1e-6 and abs(s["rms"] - math.sqrt((plain ** 2).mean()) * 0.5) < 1e-5
        assert s["max"] == float(fin.max()) if (fin >= 0).any() else s["max"] == 0.0
    else:
        assert math.isnan(s["mean"]) and math.isnan(s["rms"]) and math.isnan(s["max"])


def test_the_sums_cannot_overflow():
    per_entry_1, per_entry_2 = int(CLAMP * SCALE), int(CLAMP * CLAMP * SCALE)
    assert (1 << 31) * per_entry_1 < 1 << 63 and (1 << 31) * per_entry_2 < 1 << 63
    assert mesh_distance.DISTANCE_SCALE == SCALE and mesh_distance.DISTANCE_CLAMP == CLAMP
    s = summary_host(np.full(10, 3e38, np.float32), (), 1e-30)
    assert s["sum"] == 10 * per_entry_1 and s["sum_sq"] == 10 * per_entry_2


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    with pytest.raises(TypeError, match="mesh"):
        MeshIndex([torch.zeros(4, 3)])
    for key, bad in (("vertices", torch.zeros(4, 3, dtype=torch.float64)), ("vertices", torch.zeros(4, 2)), ("faces", cpu_mesh(rgb=False)["faces"].long())):
        with pytest.raises(ValueError, match=key):
            MeshIndex(dict(cpu_mesh(rgb=False), **{key: bad}))
        with pytest.raises(ValueError, match=key):
            sample_surface(dict(cpu_mesh(rgb=False), **{key: bad}), 0.1)
        with pytest.raises(ValueError, match=key):
            mesh_distance.mesh_distance(cpu_mesh(rgb=False), dict(cpu_mesh(rgb=False), **{key: bad}), 0.1)
    for bad in (0, -1.0, math.nan, math.inf, True, "a"):
        with pytest.raises(ValueError, match="cell"):
            MeshIndex(cpu_mesh(rgb=False), cell=bad)
        with pytest.raises(ValueError, match="spacing"):
            sample_surface(cpu_mesh(rgb=False), bad)
        with pytest.raises(ValueError, match="spacing"):
            mesh_distance.mesh_distance(cpu_mesh(rgb=False), cpu_mesh(rgb=False), bad)
        with pytest.raises(ValueError, match="unit"):
            distance_summary(torch.zeros(3), unit=bad)
        with pytest.raises(ValueError, match="threshold"):
            distance_summary(torch.zeros(3), thresholds=(0.1, bad))
        with pytest.raises(ValueError, match="threshold"):
            cloud_to_mesh(torch.zeros(3, 3), cpu_mesh(rgb=False), thresholds=(bad,))
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="max_bytes"):
            MeshIndex(cpu_mesh(rgb=False), max_bytes=bad)
        with pytest.raises(ValueError, match="max_points"):
            sample_surface(cpu_mesh(rgb=False), 0.1, max_points=bad)
    with pytest.raises(ValueError, match="at most 8"):
        distance_summary(torch.zeros(3), thresholds=[0.1] * 9)
    with pytest.raises(ValueError, match="threshold"):
        distance_summary(torch.zeros(3), thresholds=0.5)
    with pytest.raises(TypeError, match="distance"):
        distance_summary(np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="float32"):
        distance_summary(torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError, match="points"):
        cloud_to_mesh(np.zeros((3, 3), np.float32), cpu_mesh(rgb=False))
    for bad in (torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="points"):
            cloud_to_mesh(bad, cpu_mesh(rgb=False))
    for bad in (-0.5, math.nan, True, "far"):
        with pytest.raises(ValueError, match="max_distance"):
            cloud_to_mesh(torch.zeros(3, 3), cpu_mesh(rgb=False), max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            mesh_distance.mesh_distance(cpu_mesh(rgb=False), cpu_mesh(rgb=False), 0.1, max_distance=bad)
    with pytest.raises(TypeError, match="mesh_or_index"):
        cloud_to_mesh(torch.zeros(3, 3), None)
    for call in (lambda: MeshIndex(cpu_mesh(rgb=False)), lambda: MeshIndex(cpu_mesh(rgb=False), cell=0.5), lambda: sample_surface(cpu_mesh(rgb=False), 0.1),
                 lambda: distance_summary(torch.zeros(3), (0.1, 0.2), 2.0), lambda: cloud_to_mesh(torch.zeros(3, 3), cpu_mesh(rgb=False), (0.1,), 1.0),
                 lambda: mesh_distance.mesh_distance(cpu_mesh(rgb=False), cpu_mesh(rgb=False), 0.1, (0.05,), math.inf)):
        with pytest.raises(NativeError):                                        # accepted arguments on the CPU: no fallback
            call()


def test_default_cell_is_a_function_of_box_and_faces():
    lo, hi = (0.0, -1.0, 2.0), (4.0, 1.0, 2.0)
    assert mesh_distance.default_cell(lo, hi, 800) == 4.0 * 2.0 * math.sqrt(2.0 / 800) == default_cell_host(lo, hi, 800)
    assert mesh_distance.default_cell(lo, lo, 5) == 1.0 and mesh_distance.grid_dims(lo, hi, 0.5) == (9, 5, 1) == dims_host(lo, hi, 0.5)
    cell = mesh_distance.default_cell((0.0,) * 3, (1.0,) * 3, (1 << 31) - 1)         # clamped: the cell box stays under 2^31
    assert math.prod(mesh_distance.grid_dims((0.0,) * 3, (1.0,) * 3, cell)) < 1 << 31
    assert math.prod(mesh_distance.grid_dims((0.0,) * 3, (1.0,) * 3, cell / 2)) >= 1 << 31


def test_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfMeshIndex" in header and C.sizeof(N.LrfMeshIndex) == 4 * 8 + 3 * 8 + 4 * 8 + 4 * 4
    assert "#define LRF_DISTANCE_MAX_THRESHOLDS 8" in header and N.LRF_DISTANCE_MAX_THRESHOLDS == 8
    assert built_lib.lrf_abi_version() == 7
    import __graft_entry__ as ge
    assert "lrf_mesh_distance.inl" in ge.HEADERS

    def index(**over):
        return filled(N.LrfMeshIndex, dict(vertices=FAKE, faces=FAKE, grid=FAKE, list=FAKE, Nv=5, Nf=3, entries=7, cell=0.5, lo=(0.0,) * 3,
                                           dims=(4,) * 3), **over)

    def build(total=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_index_build(C.byref(index(**over)), total, None))

    def closest(points=FAKE, n=9, md=math.inf, dist=FAKE, face=FAKE, cl=None, **over):
        return refused(built_lib, built_lib.lrf_mesh_closest(C.byref(index(**over)), points, n, md, dist, face, cl, None))
    for who, call in (("lrf_mesh_index_build", build), ("lrf_mesh_closest", closest)):
        for bad in (dict(Nv=0), dict(Nv=1 << 31), dict(Nf=0), dict(Nf=1 << 31)):
            assert call(**bad).startswith(who + ": need 1 <= Nv"), bad
        for bad in (dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(1 << 11, 1 << 10, 1 << 10))):
            assert "fewer than 2^31 cells" in call(**bad), bad
        for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf), dict(lo=(0.0, math.nan, 0.0)), dict(lo=(math.inf, 0.0, 0.0))):
            assert "finite cell" in call(**bad), bad
        for bad in (dict(vertices=None), dict(faces=None), dict(grid=None)):
            assert call(**bad).endswith(": null argument"), bad
        for bad in (dict(vertices=FAKE + 2), dict(faces=FAKE + 1), dict(list=FAKE + 2)):
            assert "4-byte aligned" in call(**bad), bad
        assert "8-byte aligned" in call(grid=FAKE + 4)
    assert "needs total" in build(total=None, list=None)
    assert "entries" in build(entries=-1) and "entries" in build(entries=1 << 31) and "8-byte aligned" in build(total=FAKE + 4)
    assert "entries" in closest(list=None) and "entries" in closest(entries=-1) and "entries" in closest(entries=1 << 31)
    assert "1 <= N" in closest(n=0) and "1 <= N" in closest(n=1 << 31)
    assert "max_distance" in closest(md=-1.0) and "max_distance" in closest(md=math.nan)
    for bad in (dict(points=None), dict(dist=None), dict(face=None)):
        assert closest(**bad).endswith(": null argument"), bad
    for bad in (dict(points=FAKE + 2), dict(dist=FAKE + 1), dict(face=FAKE + 3), dict(cl=FAKE + 2)):
        assert "4-byte aligned" in closest(**bad), bad
    assert built_lib.lrf_mesh_index_build(None, FAKE, None) != 0 and built_lib.lrf_mesh_closest(None, FAKE, 1, 1.0, FAKE, FAKE, None, None) != 0

    def bounds(v=FAKE, f=FAKE, nv=5, nf=3, out=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_index_bounds(v, f, nv, nf, out, None))

    def count(v=FAKE, f=FAKE, nv=5, nf=3, spacing=0.1, offsets=FAKE, info=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_sample_count(v, f, nv, nf, spacing, offsets, info, None))

    def emit(v=FAKE, f=FAKE, nv=5, nf=3, spacing=0.1, offsets=FAKE, m=4, pts=FAKE, face=FAKE):
        return refused(built_lib, built_lib.lrf_mesh_sample_emit(v, f, nv, nf, spacing, offsets, m, pts, face, None))
    for call in (bounds, count, emit):
        for bad in (dict(nv=0), dict(nv=1 << 31), dict(nf=-1), dict(nf=1 << 31)):
            assert "need 1 <= Nv" in call(**bad), bad
        for bad in (dict(v=None), dict(f=None)):
            assert call(**bad).endswith(": null argument"), bad
        assert "4-byte aligned" in call(v=FAKE + 2) and "4-byte aligned" in call(f=FAKE + 1)
    assert bounds(out=None).endswith(": null argument") and "8-byte aligned" in bounds(out=FAKE + 4)
    for call in (count, emit):
        assert "Nf >= 1" in call(nf=0)
        for bad in (0.0, -1.0, math.nan, math.inf):
            assert "spacing" in call(spacing=bad)
        assert call(offsets=None).endswith(": null argument") and "4-byte aligned" in call(offsets=FAKE + 2)
    assert count(info=None).endswith(": null argument") and "8-byte aligned" in count(info=FAKE + 4)
    assert "1 <= M" in emit(m=0) and "1 <= M" in emit(m=1 << 31)
    assert emit(pts=None).endswith(": null argument") and emit(face=None).endswith(": null argument") and "4-byte aligned" in emit(pts=FAKE + 1)

    def summary(d=FAKE, n=9, taus=(0.1, 0.2), k=None, unit=1.0, words=FAKE):
        arr = (C.c_float * 9)(*taus) if taus is not None else None
        return refused(built_lib, built_lib.lrf_distance_summary(d, n, arr, len(taus) if k is None else k, unit, words, None))
    assert "0 <= N" in summary(n=-1) and "0 <= N" in summary(n=1 << 31)
    assert "n_thresholds" in summary(k=-1) and "n_thresholds" in summary(k=9)
    for bad in (dict(d=None), dict(words=None), dict(taus=None, k=2)):
        assert summary(**bad).endswith(": null argument"), bad
    for bad in (0.0, -2.0, math.nan, math.inf):
        assert "unit" in summary(unit=bad) and "threshold" in summary(taus=(0.1, bad))
    assert "4-byte aligned" in summary(d=FAKE + 2) and "8-byte aligned" in summary(words=FAKE + 4)


def test_the_grid_bytes_refuse_and_follow_the_formula(built_lib):
    size = built_lib.lrf_mesh_index_workspace_bytes
    for bad in (0, -1, 1 << 31, 1 << 40):
        assert size(bad) == 0, bad
    for cells in (1, 2, 31, 32, 33, 4097, 1 << 20, (1 << 31) - 1):
        assert size(cells) == (8 * cells + 255) // 256 * 256


def test_distance_kernels_use_no_scratch():
    """The kernels of lrf_mesh_distance.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
