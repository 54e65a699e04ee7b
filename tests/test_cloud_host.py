"""The point-cloud index without a GPU: the grid walk's stopping rule (tests/cloud_cases.py, pure Python) against the brute force
on every case, the properties the cases were made for, default_point_cell, argument refusals before any native call (Python and
C ABI), the new symbols and struct sizes, the workspace sizes, icp's new refusal, and the kernels' scratch use."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, alignment, cloud
from localrf_amd.cloud import CloudIndex, cloud_distance, cloud_to_cloud, nearest_spacing, remove_outliers, voxel_downsample
from cloud_cases import (CASE_NAMES, CLOUD_SIZES, NONE, QUERY_SIZES, box_host, cases, cell_sweep, default_point_cell_host, dims_host,
                         expected, grid_walk_host, icp_case, pairs, surface_with_floaters, used_host, voxel_cases, voxel_host)
from mesh_util import forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lrf_cloud_index_bounds", "lrf_cloud_index_workspace_bytes", "lrf_cloud_index_build", "lrf_cloud_closest", "lrf_cloud_knn",
           "lrf_cloud_radius_count", "lrf_cloud_voxel_bounds", "lrf_cloud_voxel_workspace_bytes", "lrf_cloud_voxel")
KERNELS = ("k_cl_bounds", "k_cl_fill", "k_cl_closest", "k_cl_knnILi1E", "k_cl_knnILi2E", "k_cl_knnILi4E", "k_cl_knnILi8E",
           "k_cl_radius_count", "k_cl_voxel_bounds", "k_cl_voxel_write")


def test_the_cases_cover_what_they_should():
    cs = cases()
    assert {c["cloud"].shape[0] for c in cs.values()} >= set(CLOUD_SIZES)
    assert {c["queries"].shape[0] for c in cs.values()} >= set(QUERY_SIZES)
    e = expected("lattice")
    d2 = pairs("lattice")
    ties = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert {1, 2, 4, 8} == set(ties.tolist())                                       # corners, edge midpoints, face and cell centres
    first = np.array([np.nonzero(row == row.min())[0][0] for row in d2])
    assert np.array_equal(e["closest"]["index"], first)
    eight = e["knn"][8]["index"][ties == 8]
    assert (np.diff(eight, axis=1) > 0).all()                                       # equal distances: ordered by index
    lo, hi = box_host(cs["line"]["cloud"])
    assert dims_host(lo, hi, default_point_cell_host(lo, hi, 64))[1:] == (1, 1)
    for name in ("a single point", "70 identical points"):
        lo, hi = box_host(cs[name]["cloud"])
        assert lo == hi and default_point_cell_host(lo, hi, cs[name]["cloud"].shape[0]) == 1.0
    bad = expected("cloud entries that are not finite")
    unused = np.nonzero(~used_host(cs["cloud entries that are not finite"]["cloud"]))[0]
    assert bad["info"] == {"points": 59, "nonfinite_points": 6} and not np.isin(bad["knn"][8]["index"], unused).any()
    q = expected("queries that are not finite")
    assert np.isnan(q["closest"]["distance"]).sum() == 4 and (q["count"] == -1).sum() == 4 and np.isnan(q["knn"][3]["distance"]).all(1).sum() == 4
    assert expected("no finite point")["info"]["points"] == 0 and (expected("no finite point")["closest"]["index"] == -1).all()
    big = expected("coordinates near 1e30")
    assert np.isfinite(big["closest"]["distance"]).all() and big["closest"]["distance"].min() > 1e27 and 0 < big["count"].max()
    one = expected("a single point")                                                # k > M: the slots past the cloud stay empty
    assert (one["knn"][8]["index"][:, 0] == 0).all() and (one["knn"][8]["index"][:, 1:] == -1).all() and np.isinf(one["knn"][8]["distance"][:, 1:]).all()
    s = cs["sphere"]
    assert s["cloud"].shape[0] == 4099 and math.isfinite(s["max_distance"])
    hit = expected("sphere")["closest"]["index"] >= 0
    assert 0 < hit.sum() < hit.size and (expected("sphere")["closest"]["distance"][hit] <= 0.3).all()


def test_boundaries_are_inclusive_and_self_is_one_record():
    e, c = expected("planted distance"), cases()["planted distance"]
    assert c["max_distance"] == c["radius"] == 1.25
    assert e["closest"]["distance"][0] == 1.25 and e["closest"]["index"][0] == 0 and e["count"][0] == 1      # exactly on the boundary
    assert np.isinf(e["closest"]["distance"][1]) and e["closest"]["index"][1] == -1 and e["count"][1] == 0   # just beyond it
    assert e["closest"]["distance"][4] == 1.25 and e["count"][4] == 1 and e["count"][5] == 0 and e["count"][3] == 1
    t, tc = expected("triplicates on themselves"), cases()["triplicates on themselves"]["cloud"]
    near = t["knn_self"][2]
    rows = np.arange(195)
    assert (near["distance"] == 0).all() and (near["index"] != rows[:, None]).all()                        # the two other copies, at 0
    assert (tc[near["index"][:, 0]] == tc).all() and (near["index"][:, 0] < near["index"][:, 1]).all()
    assert (t["knn"][1]["distance"] == 0).all() and (t["count"] - t["count_self"] == 1).all()
    same = expected("70 identical points on themselves")
    assert (same["count"] == 70).all() and (same["count_self"] == 69).all()                               # radius 0: d2 <= 0
    assert np.array_equal(same["knn_self"][1]["index"][:, 0], np.where(rows[:70] == 0, 1, 0))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_grid_walk_equals_the_brute_force(name):
    """The .inl's shells and stopping rule in pure Python against the brute force over every pair, for the three queries and
    with the self record skipped, at every cell of the sweep: the termination argument, checked on the CPU."""
    c, e, d2 = cases()[name], expected(name), pairs(name)
    cells, default = cell_sweep(c["cloud"])
    if default is None:
        assert (e["closest"]["index"] == -1).all() and (e["count"] <= 0).all()
        return
    n = c["queries"].shape[0] if c["walk"] is None else c["walk"]
    q, fin = c["queries"][:n], np.isfinite(c["queries"][:n]).all(1)
    reach = c["max_distance"] ** 2
    for cell in cells:
        cell = default if cell is None else cell
        if name == "sphere" and cell < default:
            q, fin = q[:16], fin[:16]                                               # 128^3 cells in pure Python: a few queries
        m = q.shape[0]
        best, idx, shells = grid_walk_host(q, c["cloud"], cell, c["max_distance"], d2, "closest")
        hit = fin & (idx[:, 0] != NONE) & ~(best[:, 0] > reach)
        assert np.array_equal(np.where(hit, idx[:, 0], -1), e["closest"]["index"][:m])
        assert np.array_equal(np.where(hit, best[:, 0], np.inf), e["closest"]["d2"][:m])
        for k in (3, 8):
            for self_ in (False, True) if c["self"] and m == c["cloud"].shape[0] else (False,):
                kd, ki, _ = grid_walk_host(q, c["cloud"], cell, c["max_distance"], d2, "knn", k, self_)
                hit = fin[:, None] & (ki != NONE) & ~(kd > reach)
                want = e["knn_self" if self_ else "knn"][k]
                assert np.array_equal(np.where(hit, ki, -1), want["index"][:m])
                assert np.array_equal(np.where(hit, np.sqrt(np.where(hit, kd, 0.0)), np.inf).astype(np.float32)[fin], want["distance"][:m][fin])
        for self_ in (False, True) if c["self"] and m == c["cloud"].shape[0] else (False,):
            counts, _ = grid_walk_host(q, c["cloud"], cell, c["radius"], d2, "count", 1, self_)
            assert np.array_equal(np.where(fin, counts, -1), (e["count_self"] if self_ else e["count"])[:m])
        if name == "lattice" and cell == default:
            assert shells.min() < shells.max()                                      # near queries stop early, others walk on


def test_default_point_cell_is_a_function_of_box_points_and_bytes():
    lo, hi = (0.0, -1.0, 2.0), (4.0, 1.0, 2.0)
    assert cloud.default_point_cell(lo, hi, 400) == 4.0 * 2.0 / 20.0 == default_point_cell_host(lo, hi, 400)
    assert cloud.default_point_cell(lo, lo, 5) == 1.0 and cloud.default_point_cell(lo, hi, 0) == 1.0
    unit = ((0.0,) * 3, (1.0,) * 3)
    cell = cloud.default_point_cell(*unit, 1 << 40)                                 # doubled: the grid stays under 2^31 cells ...
    cells = math.prod(dims_host(*unit, cell))
    assert cells < 1 << 31 and 8 * cells <= (1 << 30) // 2                          # ... and its words within half of max_bytes
    assert 8 * math.prod(dims_host(*unit, cell / 2)) > (1 << 30) // 2
    small = cloud.default_point_cell(*unit, 1 << 20, max_bytes=1 << 16)
    assert 8 * math.prod(dims_host(*unit, small)) <= 1 << 15 < 8 * math.prod(dims_host(*unit, small / 2))
    assert small == default_point_cell_host(*unit, 1 << 20, 1 << 16)
    assert cloud.default_point_cell(*unit, 1 << 20, max_bytes=0) > 1.0              # ends: one cell is always allowed


def test_the_voxel_rule_holds_its_properties():
    for name, (p, col, cell, origin) in voxel_cases().items():
        v = voxel_host(p, cell, origin, col)
        assert v["count"].sum() + v["bad"] == p.shape[0] and (v["cluster_of"] >= 0).sum() == v["count"].sum()
        assert v["points"].shape[0] == v["count"].shape[0] == len(set(v["cluster_of"][v["cluster_of"] >= 0].tolist()))
        if v["points"].shape[0]:
            perm = np.random.default_rng(1).permutation(p.shape[0])
            w = voxel_host(p[perm], cell, origin, None if col is None else col[perm])
            assert all(np.array_equal(v[k], w[k]) for k in ("points", "count")) and np.array_equal(v["cluster_of"][perm], w["cluster_of"])
            inside = np.abs(v["points"][v["cluster_of"][v["cluster_of"] >= 0]].astype(np.float64) - p[v["cluster_of"] >= 0]).max()
            assert inside <= cell * (1 + 1e-6)                                      # a point and its cluster's mean share a cell
    assert voxel_host(*[voxel_cases()["bad points"][k] for k in (0, 2, 3)])["bad"] == 4


def test_the_planted_cases_hold():
    pts, floater, radius = surface_with_floaters()
    assert floater.sum() == 8 and pts.shape[0] == 48 * 48 + 8
    A, B, T, nn, move = icp_case()
    assert 0 < move <= 0.25 * nn and A.shape == B.shape == (576, 3)


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    pts = torch.zeros(8, 3)
    with pytest.raises(TypeError, match="points"):
        CloudIndex(np.zeros((3, 3), np.float32))
    for bad in (torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64)):
        for call in (lambda: CloudIndex(bad), lambda: voxel_downsample(bad, 0.1), lambda: cloud_to_cloud(bad, pts), lambda: cloud_distance(pts, bad),
                     lambda: remove_outliers(bad, 0.1, 2)):
            with pytest.raises(ValueError, match=r"points must be \[N, 3\] float32"):
                call()
    for bad in (0, -1.0, math.nan, math.inf, True, "a"):
        with pytest.raises(ValueError, match="cell"):
            CloudIndex(pts, cell=bad)
        with pytest.raises(ValueError, match="cell"):
            voxel_downsample(pts, bad)
        with pytest.raises(ValueError, match="voxel"):
            cloud_distance(pts, pts, voxel=bad)
        with pytest.raises(ValueError, match="threshold"):
            cloud_to_cloud(pts, pts, thresholds=(0.1, bad))
        with pytest.raises(ValueError, match="unit"):
            cloud_to_cloud(pts, pts, unit=bad)
    for bad in (-1, 1.5, None, True):
        for call in (lambda: CloudIndex(pts, max_bytes=bad), lambda: voxel_downsample(pts, 0.1, max_bytes=bad),
                     lambda: cloud_to_cloud(pts, pts, max_bytes=bad), lambda: cloud_distance(pts, pts, max_bytes=bad), lambda: nearest_spacing(pts, bad)):
            with pytest.raises(ValueError, match="max_bytes"):
                call()
    for bad in (-0.5, math.nan, True, "far"):
        with pytest.raises(ValueError, match="max_distance"):
            cloud_to_cloud(pts, pts, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            cloud_distance(pts, pts, max_distance=bad)
    for bad in (-0.5, math.nan, math.inf, True, "r"):
        with pytest.raises(ValueError, match="radius"):
            remove_outliers(pts, bad, 2)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_neighbours"):
            remove_outliers(pts, 0.1, bad)
    with pytest.raises(ValueError, match="origin"):
        voxel_downsample(pts, 0.1, origin=(0.0, math.nan, 0.0))
    for key, bad in (("rgb8", torch.zeros(8, 3)), ("rgb8", torch.zeros(7, 3, dtype=torch.uint8)), ("normals", torch.zeros(8, 2))):
        with pytest.raises(ValueError, match=key):
            remove_outliers(pts, 0.1, 2, **{key: bad})
    with pytest.raises(ValueError, match="rgb8"):
        voxel_downsample(pts, 0.1, rgb8=torch.zeros(8, 3))
    with pytest.raises(TypeError, match="index"):
        remove_outliers(pts, 0.1, 2, index=pts)
    for call in (lambda: cloud_to_cloud(pts, None), lambda: nearest_spacing([pts])):
        with pytest.raises(TypeError, match="CloudIndex"):
            call()
    with pytest.raises(ValueError, match="at most 8"):
        cloud_distance(pts, pts, thresholds=[0.1] * 9)
    for call in (lambda: CloudIndex(pts), lambda: CloudIndex(pts, cell=0.5), lambda: voxel_downsample(pts, 0.1), lambda: nearest_spacing(pts),
                 lambda: voxel_downsample(pts, 0.1, rgb8=torch.zeros(8, 3, dtype=torch.uint8)), lambda: remove_outliers(pts, 0.1, 2),
                 lambda: cloud_to_cloud(pts, pts, (0.1,), 1.0), lambda: cloud_distance(pts, pts, (0.05,), math.inf, 0.1)):
        with pytest.raises(NativeError):                                        # accepted arguments on the CPU: no fallback
            call()


class _StubIndex(CloudIndex):
    """A CloudIndex without a device: the checks of the queries that come before the device check."""
    def __init__(self, m=8):
        self.points, self.device, self.counts, self._grid = torch.zeros(m, 3), torch.device("cpu"), (m,), None
        self.info = {"cell": None, "box": None, "dims": (0, 0, 0), "points": 0, "nonfinite_points": 0}


def test_query_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    index, pts = _StubIndex(), torch.zeros(8, 3)
    for bad in (0, 9, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="k must be"):
            index.knn(pts, bad)
    for bad in (-0.5, math.nan, True):
        with pytest.raises(ValueError, match="max_distance"):
            index.knn(pts, 2, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            index.closest(pts, bad)
    for bad in (-1.0, math.nan, math.inf, True):
        with pytest.raises(ValueError, match="radius"):
            index.radius_count(pts, bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="exclude_self"):
            index.knn(pts, 2, exclude_self=bad)
        with pytest.raises(ValueError, match="closest"):
            index.closest(pts, closest=bad)
    with pytest.raises(ValueError, match="7 queries for a cloud of 8"):
        index.knn(torch.zeros(7, 3), 1, exclude_self=True)
    with pytest.raises(ValueError, match="7 queries for a cloud of 8"):
        index.radius_count(torch.zeros(7, 3), 0.5, exclude_self=True)
    for call in (lambda: index.closest(pts), lambda: index.knn(pts, 8, exclude_self=True), lambda: index.radius_count(pts, 0.0)):
        with pytest.raises(NativeError):
            call()
    with pytest.raises(ValueError, match="built over 8 points"):
        remove_outliers(torch.zeros(5, 3), 0.1, 2, index=index)


def test_icp_refuses_planes_on_a_cloud_before_any_launch(monkeypatch):
    forbid_native(monkeypatch)
    index, pts = _StubIndex(), torch.zeros(8, 3)
    for metric in ("plane", None):
        with pytest.raises(ValueError, match='a cloud has no planes.*metric="point"'):
            alignment.icp(pts, index) if metric is None else alignment.icp(pts, index, metric=metric)
    with pytest.raises(ValueError, match="iterations"):                             # the other checks come first, as for a mesh
        alignment.icp(pts, index, metric="plane", iterations=0)
    with pytest.raises(ValueError, match="points"):
        alignment.icp(torch.zeros(8, 2), index, metric="point")
    with pytest.raises(NativeError):                                                # accepted: the device check is next
        alignment.icp(pts, index, metric="point")


def test_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfCloudIndex" in header and C.sizeof(N.LrfCloudIndex) == 3 * 8 + 2 * 8 + 4 * 8 + 4 * 4
    assert "typedef struct LrfCloudVoxel" in header and C.sizeof(N.LrfCloudVoxel) == 2 * 8 + 8 + 4 * 8 + 6 * 4
    assert "#define LRF_CLOUD_MAX_K 8" in header and N.LRF_CLOUD_MAX_K == 8 == cloud.MAX_K
    import __graft_entry__ as ge
    assert "lrf_cloud.inl" in ge.HEADERS
    src = open(os.path.join(ROOT, "localrf_amd", "csrc", "lrf_render.hip")).read()
    assert src.index('#include "lrf_align.inl"') < src.index('#include "lrf_cloud.inl"')

    def index(**over):
        return filled(N.LrfCloudIndex, dict(points=FAKE, grid=FAKE, records=FAKE, M=9, entries=7, cell=0.5, lo=(0.0,) * 3, dims=(4,) * 3), **over)

    def build(**over):
        return refused(built_lib, built_lib.lrf_cloud_index_build(C.byref(index(**over)), None))

    def closest(points=FAKE, n=9, md=math.inf, dist=FAKE, idx=FAKE, cl=None, **over):
        return refused(built_lib, built_lib.lrf_cloud_closest(C.byref(index(**over)), points, n, md, dist, idx, cl, None))

    def knn(points=FAKE, n=9, k=3, md=math.inf, first=-1, dist=FAKE, idx=FAKE, **over):
        return refused(built_lib, built_lib.lrf_cloud_knn(C.byref(index(**over)), points, n, k, md, first, dist, idx, None))

    def count(points=FAKE, n=9, radius=0.5, first=-1, out=FAKE, **over):
        return refused(built_lib, built_lib.lrf_cloud_radius_count(C.byref(index(**over)), points, n, radius, first, out, None))
    for who, call in (("lrf_cloud_index_build", build), ("lrf_cloud_closest", closest), ("lrf_cloud_knn", knn), ("lrf_cloud_radius_count", count)):
        for bad in (dict(M=0), dict(M=1 << 31)):
            assert call(**bad) == who + ": need 1 <= M < 2^31", bad
        for bad in (dict(entries=-1), dict(entries=10)):
            assert "entries <= M" in call(**bad), bad
        for bad in (dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(1 << 11, 1 << 10, 1 << 10))):
            assert "fewer than 2^31 cells" in call(**bad), bad
        for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf), dict(lo=(0.0, math.nan, 0.0)), dict(lo=(math.inf, 0.0, 0.0))):
            assert "finite cell" in call(**bad), bad
        for bad in (dict(points=None) if call is build else dict(records=None), dict(grid=None)):
            assert call(**bad).startswith(who) and ("null argument" in call(**bad) or "records" in call(**bad)), bad
        assert "8-byte aligned" in call(grid=FAKE + 4) and "16-byte aligned" in call(records=FAKE + 8) and "16-byte aligned" in call(records=FAKE + 4)
    assert "4-byte aligned" in build(points=FAKE + 2) and build(records=None).endswith(": null argument")
    assert built_lib.lrf_cloud_index_build(None, None) != 0 and built_lib.lrf_cloud_closest(None, FAKE, 1, 1.0, FAKE, FAKE, None, None) != 0
    for call in (closest, knn, count):
        assert "1 <= N" in call(n=0) and "1 <= N" in call(n=1 << 31)
        assert call(points=None).endswith(": null argument") and "4-byte aligned" in call(points=FAKE + 2)
        assert "records of a built index" in call(records=None)
    for call in (closest, knn):
        assert "max_distance" in call(md=-1.0) and "max_distance" in call(md=math.nan)
        assert call(dist=None).endswith(": null argument") and call(idx=None).endswith(": null argument")
        assert "4-byte aligned" in call(dist=FAKE + 1) and "4-byte aligned" in call(idx=FAKE + 3)
    assert "4-byte aligned" in closest(cl=FAKE + 2)
    for bad in (0, 9, -1):
        assert "k must lie in [1, LRF_CLOUD_MAX_K]" in knn(k=bad)
    for bad in (-1.0, math.nan, math.inf):
        assert "radius must be finite and >= 0" in count(radius=bad)
    for call in (knn, count):
        assert "self_first" in call(first=-2) and "self_first" in call(first=1) and "self_first" in call(first=5, n=5)
    assert count(out=None).endswith(": null argument") and "4-byte aligned" in count(out=FAKE + 2)

    def bounds(p=FAKE, m=5, out=FAKE):
        return refused(built_lib, built_lib.lrf_cloud_index_bounds(p, m, out, None))
    assert "1 <= M" in bounds(m=0) and "1 <= M" in bounds(m=1 << 31)
    assert bounds(p=None).endswith(": null argument") and bounds(out=None).endswith(": null argument")
    assert "4-byte aligned" in bounds(p=FAKE + 2) and "8-byte aligned" in bounds(out=FAKE + 4)

    def vbounds(p=FAKE, m=5, origin=(0.0, 0.0, 0.0), cell=0.5, out=FAKE):
        return refused(built_lib, built_lib.lrf_cloud_voxel_bounds(p, m, None if origin is None else (C.c_double * 3)(*origin), cell, out, None))
    assert "1 <= M" in vbounds(m=0) and "1 <= M" in vbounds(m=1 << 31)
    for bad in (dict(p=None), dict(origin=None), dict(out=None)):
        assert vbounds(**bad).endswith(": null argument"), bad
    assert "origin" in vbounds(origin=(0.0, math.inf, 0.0)) and "4-byte aligned" in vbounds(p=FAKE + 1) and "8-byte aligned" in vbounds(out=FAKE + 4)
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert "cell must be finite" in vbounds(cell=bad)

    def voxel(po=FAKE, co=None, no=FAKE, cl=FAKE, counts=FAKE, ws=FAKE, **over):
        a = filled(N.LrfCloudVoxel, dict(points=FAKE, rgb8=None, M=9, cell=0.5, origin=(0.0,) * 3, lo=(-2,) * 3, dims=(4,) * 3), **over)
        return refused(built_lib, built_lib.lrf_cloud_voxel(C.byref(a), po, co, no, cl, counts, ws, None))
    assert "1 <= M" in voxel(M=0) and "1 <= M" in voxel(M=1 << 31)
    for bad in (dict(points=None), dict(po=None), dict(no=None), dict(cl=None), dict(counts=None), dict(ws=None)):
        assert voxel(**bad).endswith(": null argument"), bad
    assert "go together" in voxel(rgb8=FAKE) and "go together" in voxel(co=FAKE)
    for bad in (dict(dims=(0, 4, 4)), dict(dims=(1 << 11, 1 << 10, 1 << 10))):
        assert "fewer than 2^31 cells" in voxel(**bad), bad
    assert "inside (-2^30, 2^30)" in voxel(lo=(-(1 << 30), 0, 0)) and "inside (-2^30, 2^30)" in voxel(lo=((1 << 30) - 3, 0, 0))
    assert "origin" in voxel(origin=(math.nan, 0.0, 0.0)) and "cell must be finite" in voxel(cell=0.0) and "cell must be finite" in voxel(cell=math.inf)
    assert "4-byte aligned" in voxel(points=FAKE + 2) and "4-byte aligned" in voxel(no=FAKE + 1) and "4-byte aligned" in voxel(cl=FAKE + 3)
    assert "8-byte aligned" in voxel(counts=FAKE + 4) and "8-byte aligned" in voxel(ws=FAKE + 4)
    assert built_lib.lrf_cloud_voxel(None, FAKE, None, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_the_workspace_bytes_refuse_and_follow_the_formula(built_lib):
    size = built_lib.lrf_cloud_index_workspace_bytes
    for bad in (0, -1, 1 << 31, 1 << 40):
        assert size(bad) == 0, bad
    for cells in (1, 2, 31, 32, 33, 4097, 1 << 20, (1 << 31) - 1):
        assert size(cells) == (8 + 8 * cells + 255) // 256 * 256
    vsize = built_lib.lrf_cloud_voxel_workspace_bytes
    for bad in ((0, 5), (1 << 31, 5), (5, 0), (5, 1 << 31)):
        assert vsize(*bad) == 0, bad
    for m, cells in ((1, 1), (65, 1000), (4099, 1 << 21)):
        words = ((cells + 63) // 64 + 15) // 16 * 16
        assert vsize(m, cells) == (8 + 8 * words + 24 * m + 16 * m + 4 * words + 4 * (words // 16) + 4 * m + 255) // 256 * 256


def test_cloud_kernels_use_no_scratch():
    """The kernels of lrf_cloud.inl as __graft_entry__.build() compiles them: the metadata only.  The K slots of k_cl_knn must
    stay registers: a runtime index into them would put them into scratch."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="prefix")
