"""The point-to-mesh distance on the GPU against the restatements of tests/mesh_distance_cases.py: bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, _checks, mesh_distance
from localrf_amd import _native as N
from localrf_amd.mesh import simplify
from localrf_amd.mesh_distance import MeshIndex, cloud_to_mesh, distance_summary, sample_surface
from mesh_clean_cases import base_meshes
from mesh_distance_cases import (CASE_NAMES, SAMPLE_CASES, SUMMARY_SIZES, SUMMARY_TAUS, _pairs, box_host, cases, default_cell_host,
                                 dims_host, expected, mesh_distance_host, sample_host, summary_host, summary_inputs)
from mesh_raster_cases import octa_sphere
from mesh_util import DEV, bits, device_mesh, record_launches, same_bits

pytestmark = pytest.mark.gpu
U32 = np.uint32


def dev_mesh(m):
    return device_mesh(m, rgb=False)


def same(out, e, closest=True):
    assert np.array_equal(bits(out["distance"]), e["distance"].view(U32))
    assert np.array_equal(out["face"].cpu().numpy(), e["face"])
    if closest:
        assert np.array_equal(bits(out["closest"]), e["closest"].view(U32))


def equal_values(a, b):
    """Nested dicts and tuples of Python values, NaN equal to NaN."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(equal_values(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(equal_values(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b and type(a) is type(b)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_closest_equals_the_brute_force_at_every_cell(name):
    c, e = cases()[name], expected(name)
    mesh, pts = dev_mesh(c["mesh"]), torch.from_numpy(c["points"]).to(DEV)
    before = [t.clone() for t in (mesh["vertices"], mesh["faces"], pts)]
    for cell in c["cells"]:
        index = MeshIndex(mesh, cell=cell)
        assert {k: index.info[k] for k in e["info"]} == e["info"]
        assert all(type(v) in (int, float, tuple, type(None)) for v in index.info.values())
        if e["info"]["used_faces"]:
            lo, hi = box_host(c["mesh"])
            want = default_cell_host(lo, hi, e["info"]["used_faces"]) if cell is None else cell
            assert index.info["cell"] == want and index.info["box"] == (lo, hi) and index.info["dims"] == dims_host(lo, hi, want)
            assert index.nbytes == N.lib().lrf_mesh_index_workspace_bytes(math.prod(index.info["dims"])) + 4 * max(index.info["entries"], 1)
        else:
            assert index.nbytes == 0 and index.info["entries"] == 0
        out = index.closest(pts, c["max_distance"], closest=True)
        assert out["distance"].shape == (pts.shape[0],) and out["closest"].shape == (pts.shape[0], 3) and out["face"].dtype == torch.int32
        same(out, e)
        assert set(index.closest(pts, c["max_distance"])) == {"distance", "face"}
    for t, b in zip((mesh["vertices"], mesh["faces"], pts), before):                # the inputs are left untouched
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))


def test_the_same_bytes_for_every_run_stream_split_and_cell():
    name = "octa 512 N=1025"
    c, e = cases()[name], expected(name)
    mesh, pts = dev_mesh(c["mesh"]), torch.from_numpy(c["points"]).to(DEV)
    index = MeshIndex(mesh)
    first = index.closest(pts, closest=True)
    same(first, e)
    same(index.closest(pts, closest=True), e)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = index.closest(pts, closest=True)
    side.synchronize()
    same(out, e)
    parts = [index.closest(pts[a:b], closest=True) for a, b in ((0, 100), (100, 101), (101, 101), (101, 1025))]
    same({k: torch.cat([p[k] for p in parts]) for k in first}, e)
    for cell in (0.05, 0.6, 7.0):
        other = MeshIndex(mesh, cell=cell)
        assert other.info["dims"] != index.info["dims"]
        same(other.closest(pts, closest=True), e)
    again = MeshIndex(mesh)                                                         # the list's order is free, the answers are not
    assert again.info == index.info
    same(again.closest(pts, closest=True), e)


def test_a_face_permutation_leaves_the_distance_and_maps_the_face():
    a, b = cases()["octa 512 default cell"], cases()["octa faces permuted"]
    pts = torch.from_numpy(a["points"]).to(DEV)
    oa, ob = MeshIndex(dev_mesh(a["mesh"])).closest(pts), MeshIndex(dev_mesh(b["mesh"])).closest(pts)
    assert torch.equal(oa["distance"].view(torch.int32), ob["distance"].view(torch.int32))
    d2 = _pairs("octa 512 default cell")[1]
    alone = (d2 == d2.min(1, keepdims=True)).sum(1) == 1
    fa, fb = oa["face"].cpu().numpy()[alone], ob["face"].cpu().numpy()[alone]
    assert alone.sum() > 20 and np.array_equal(a["mesh"]["faces"][fa], b["mesh"]["faces"][fb])


def test_no_points_and_no_used_face(monkeypatch):
    index = MeshIndex(dev_mesh(cases()["octa 512 default cell"]["mesh"]))
    out = index.closest(torch.zeros(0, 3, device=DEV), closest=True)
    assert out["distance"].shape == (0,) and out["face"].shape == (0,) and out["closest"].shape == (0, 3)
    c, e = cases()["no used face"], expected("no used face")
    empty = MeshIndex(dev_mesh(c["mesh"]))
    launch = N.launch

    def no_query(name, *a, **k):
        assert name != "lrf_mesh_closest", "the query was launched for an index without a face"
        return launch(name, *a, **k)
    monkeypatch.setattr(N, "launch", no_query)
    same(empty.closest(torch.from_numpy(c["points"]).to(DEV), closest=True), e)


@pytest.mark.parametrize("name", tuple(SAMPLE_CASES))
def test_sample_surface_equals_the_restatement(name):
    make, spacing = SAMPLE_CASES[name]
    e = sample_host(make(), spacing)
    mesh = dev_mesh(make())
    out = sample_surface(mesh, spacing)
    assert out["counts"] == e["counts"] and out["info"] == e["info"]
    assert np.array_equal(bits(out["points"]), e["points"].view(U32)) and np.array_equal(out["face"].cpu().numpy(), e["face"])
    again = sample_surface(mesh, spacing)
    assert torch.equal(again["points"].view(torch.int32), out["points"].view(torch.int32)) and torch.equal(again["face"], out["face"])
    if e["counts"][0] > 1:
        with pytest.raises(ValueError, match="larger spacing"):
            sample_surface(mesh, spacing, max_points=e["counts"][0] - 1)
        assert sample_surface(mesh, spacing, max_points=e["counts"][0])["counts"] == e["counts"]


def test_sample_surface_of_nothing_and_of_too_much():
    none = sample_surface(dev_mesh(cases()["no faces"]["mesh"]), 0.1)
    assert none["counts"] == (0,) and none["points"].shape == (0, 3) and none["face"].shape == (0,)
    with pytest.raises(ValueError, match="larger spacing"):
        sample_surface(dev_mesh(octa_sphere()), 1e-5)                             # every face above 2^21 samples


@pytest.mark.parametrize("n", SUMMARY_SIZES)
def test_distance_summary_equals_the_restatement(n):
    d = summary_inputs(50 + n, n)
    for taus, unit in ((SUMMARY_TAUS, 0.5), ((), 1.0), ((0.3,) * 8, 1e-3)):
        out = distance_summary(torch.from_numpy(d).to(DEV), taus, unit)
        assert equal_values(out, summary_host(d, taus, unit)), (out, summary_host(d, taus, unit))
    two = distance_summary(torch.from_numpy(d).to(DEV).reshape(-1, 1)[:, 0], SUMMARY_TAUS, 0.5)
    assert equal_values(two, summary_host(d, SUMMARY_TAUS, 0.5))


@functools.lru_cache(maxsize=None)
def _pair_of_meshes():
    return {k: v for k, v in octa_sphere(2).items()}, {k: v for k, v in octa_sphere(3).items()}


@pytest.mark.parametrize("max_distance", (math.inf, 0.004))
def test_mesh_distance_equals_the_restatement(max_distance):
    a, b = _pair_of_meshes()
    taus = (0.002, 0.004, 0.02)
    e = mesh_distance_host(a, b, 0.045, taus, max_distance)
    out = mesh_distance.mesh_distance(dev_mesh(a), dev_mesh(b), 0.045, taus, max_distance)
    assert equal_values(out, e), (out, e)
    assert e["samples"][0] > 1000 and 0 < e["a_to_b"]["within"][0] < e["a_to_b"]["finite"]
    assert (e["a_to_b"]["beyond"] > 0) == math.isfinite(max_distance)
    from mesh_clean_cases import permute_faces
    assert equal_values(mesh_distance.mesh_distance(dev_mesh(permute_faces(a, 3)), dev_mesh(permute_faces(b, 4)), 0.045, taus, max_distance), e)
    pts = sample_surface(dev_mesh(a), 0.045)["points"]
    one = cloud_to_mesh(pts, MeshIndex(dev_mesh(b), cell=0.4), taus, max_distance)
    assert one["distance"].shape == (e["samples"][0],) and one["face"].dtype == torch.int32
    assert equal_values({k: v for k, v in one.items() if k not in ("distance", "face")}, e["a_to_b"])


@pytest.mark.parametrize("name", ("sphere", "torus"))
def test_a_mesh_is_at_distance_zero_from_itself_and_simplification_stays_within_a_cell_diagonal(name):
    m = base_meshes()[name]
    mesh = dev_mesh(m)
    scale = float(np.abs(m["vertices"]).max())
    own = mesh_distance.mesh_distance(mesh, mesh, 0.02)
    print(f"{name}: to itself, maxima {own['a_to_b']['max']:.3e} {own['b_to_a']['max']:.3e}, bar {2.0 ** -22 * scale:.3e}")
    assert own["a_to_b"]["max"] <= 2.0 ** -22 * scale and own["b_to_a"]["max"] <= 2.0 ** -22 * scale
    assert own["samples"][0] == own["samples"][1] > 500 and own["a_to_b"]["beyond"] == 0
    for cell in (2.0 / 23, 4.0 / 23):                                              # 2 and 4 voxels of the analytic lattice
        simple = simplify(mesh, cell)
        assert 0 < simple["counts"][1] < m["faces"].shape[0]
        r = mesh_distance.mesh_distance(mesh, simple, 0.02)
        print(f"{name}: simplify(cell={cell:.4f}) hausdorff {r['hausdorff']:.5f}, bar {math.sqrt(3) * cell:.5f}, chamfer {r['chamfer']:.5f}")
        assert 0 < r["hausdorff"] <= math.sqrt(3) * cell


def test_refusals():
    m = cases()["octa 512 default cell"]["mesh"]
    mesh = dev_mesh(m)
    cpu = {"vertices": mesh["vertices"].cpu(), "faces": mesh["faces"].cpu(), "rgb8": None, "counts": m["counts"]}
    pts = torch.zeros(4, 3, device=DEV)
    index = MeshIndex(mesh)
    for call in (lambda: MeshIndex(cpu), lambda: MeshIndex(dict(mesh, faces=cpu["faces"])), lambda: index.closest(pts.cpu()),
                 lambda: sample_surface(cpu, 0.1), lambda: sample_surface(dict(mesh, vertices=cpu["vertices"]), 0.1),
                 lambda: distance_summary(torch.zeros(4)), lambda: cloud_to_mesh(pts, cpu), lambda: cloud_to_mesh(pts.cpu(), mesh),
                 lambda: mesh_distance.mesh_distance(mesh, cpu, 0.1)):
        with pytest.raises(NativeError):
            call()
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="live on"):
            index.closest(pts.to("cuda:1"))
        with pytest.raises(ValueError, match="same device"):
            MeshIndex(dict(mesh, faces=mesh["faces"].to("cuda:1")))
    with pytest.raises(ValueError, match="cell box .* larger cell"):
        MeshIndex(mesh, cell=1e-4)                                                  # 20 000^3 cells
    with pytest.raises(ValueError, match="cell box .* max_bytes is 4096: a larger cell"):
        MeshIndex(mesh, cell=0.01, max_bytes=4096)                                  # the grid alone
    fits_grid = int(N.lib().lrf_mesh_index_workspace_bytes(math.prod(index.info["dims"])))
    with pytest.raises(ValueError, match="cell box .* larger cell"):
        MeshIndex(mesh, max_bytes=fits_grid + 4)                                    # the grid fits, the list does not
    assert MeshIndex(mesh, max_bytes=index.nbytes).info == index.info
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError, match="max_distance"):
            index.closest(pts, bad)
    with pytest.raises(ValueError, match="closest"):
        index.closest(pts, closest=1)


def test_chunks_give_the_bytes_of_one_call(monkeypatch):
    c = cases()["octa 512 default cell"]
    pts = torch.from_numpy(c["points"][:11].copy()).to(DEV)
    pts[6, 2] = math.nan
    index = MeshIndex(dev_mesh(c["mesh"]))
    names = record_launches(monkeypatch)
    whole = index.closest(pts, closest=True)
    assert names == ["lrf_mesh_closest"] and int((whole["face"] >= 0).sum()) == 10
    monkeypatch.setattr(_checks, "POINTS_PER_CALL", 5)
    del names[:]
    same_bits(index.closest(pts, closest=True), whole)                              # 5 + 5 + 1 points
    assert names == ["lrf_mesh_closest"] * 3
