"""The point-cloud index on the GPU against the restatements of tests/cloud_cases.py: bit for bit."""
import math

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, _checks, alignment
from localrf_amd import _native as N
from localrf_amd.cloud import (CloudIndex, cloud_distance, cloud_to_cloud, nearest_spacing, remove_outliers, voxel_downsample)
from localrf_amd.mesh import simplify
from localrf_amd.mesh_distance import MeshIndex
from cloud_cases import (CASE_NAMES, KS, box_host, cases, cell_sweep, closest_host, dims_host, expected, icp_case, pairs_host, radius_count_host,
                         random_cloud, sphere, summary_counts_host, surface_with_floaters, voxel_cases, voxel_host)
from mesh_clean_cases import base_meshes
from mesh_util import DEV, bits, device_mesh, record_launches, same_bits, to_dev

pytestmark = pytest.mark.gpu
U32 = np.uint32


def same_closest(out, e, closest=True):
    assert np.array_equal(bits(out["distance"]), e["distance"].view(U32))
    assert np.array_equal(out["index"].cpu().numpy(), e["index"])
    if closest:
        assert np.array_equal(bits(out["closest"]), e["closest"].view(U32))


def same_knn(out, e):
    assert out["distance"].shape == e["distance"].shape and out["index"].dtype is torch.int32
    assert np.array_equal(bits(out["distance"]), e["distance"].view(U32)) and np.array_equal(out["index"].cpu().numpy(), e["index"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_queries_equal_the_brute_force_at_every_cell(name):
    c, e = cases()[name], expected(name)
    cloud, pts = to_dev(c["cloud"]), to_dev(c["queries"])
    before = [t.clone() for t in (cloud, pts)]
    cells, default = cell_sweep(c["cloud"])
    n, m = pts.shape[0], cloud.shape[0]
    for cell in cells:
        index = CloudIndex(cloud, cell=cell)
        assert {k: index.info[k] for k in e["info"]} == e["info"] and index.counts == (m,) and index.device == cloud.device
        assert all(type(v) in (int, float, tuple, type(None)) for v in index.info.values())
        if default is not None:
            lo, hi = box_host(c["cloud"])
            want = default if cell is None else cell
            assert index.info["cell"] == want and index.info["box"] == (lo, hi) and index.info["dims"] == dims_host(lo, hi, want)
            assert index.nbytes == N.lib().lrf_cloud_index_workspace_bytes(math.prod(index.info["dims"])) + 16 * e["info"]["points"]
        else:
            assert index.nbytes == 0 and index.info["box"] is None
        out = index.closest(pts, c["max_distance"], closest=True)
        assert out["distance"].shape == (n,) and out["closest"].shape == (n, 3) and out["index"].dtype is torch.int32
        same_closest(out, e["closest"])
        assert set(index.closest(pts, c["max_distance"])) == {"distance", "index"}
        for k in KS:
            same_knn(index.knn(pts, k, c["max_distance"]), e["knn"][k])
        got = index.radius_count(pts, c["radius"])
        assert got.dtype is torch.int32 and np.array_equal(got.cpu().numpy(), e["count"])
        if c["self"]:
            for k in KS:
                same_knn(index.knn(pts, k, c["max_distance"], exclude_self=True), e["knn_self"][k])
            assert np.array_equal(index.radius_count(pts, c["radius"], exclude_self=True).cpu().numpy(), e["count_self"])
    for t, b in zip((cloud, pts), before):                                          # the inputs are left untouched
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))


def test_closest_equals_the_mesh_index_over_degenerate_faces():
    """faces[i] = (i, i, i): the parent's only route to the nearest point of a cloud.  Distance, index = face and closest are the
    same bits, and so are two point-to-point ICP runs, one against each index."""
    for name in ("lattice", "sphere", "triplicates", "cloud entries that are not finite", "coordinates near 1e30"):
        c = cases()[name]
        cloud, pts = to_dev(c["cloud"]), to_dev(c["queries"])
        m = cloud.shape[0]
        faces = torch.arange(m, dtype=torch.int32, device=DEV)[:, None].expand(m, 3).contiguous()
        mesh = MeshIndex({"vertices": cloud, "faces": faces, "rgb8": None, "counts": (m, m)})
        a, b = CloudIndex(cloud).closest(pts, c["max_distance"], closest=True), mesh.closest(pts, c["max_distance"], closest=True)
        assert torch.equal(a["distance"].view(torch.int32), b["distance"].view(torch.int32)) and torch.equal(a["index"], b["face"])
        assert torch.equal(a["closest"].view(torch.int32), b["closest"].view(torch.int32))
    A, B, _, _, _ = icp_case()
    src, tgt = to_dev(A), to_dev(B)
    m = tgt.shape[0]
    faces = torch.arange(m, dtype=torch.int32, device=DEV)[:, None].expand(m, 3).contiguous()
    one = alignment.icp(src, CloudIndex(tgt), metric="point", iterations=2)
    two = alignment.icp(src, MeshIndex({"vertices": tgt, "faces": faces, "rgb8": None, "counts": (m, m)}), metric="point", iterations=2)
    assert one["T"].tobytes() == two["T"].tobytes() and one["history"] == two["history"] and one["iterations"] == two["iterations"] >= 1


def test_the_same_bytes_for_every_run_stream_split_and_permutation():
    c, e = cases()["sphere"], expected("sphere")
    cloud, pts = to_dev(c["cloud"]), to_dev(c["queries"])
    index = CloudIndex(cloud)

    def run(ix, q):
        return ix.closest(q, c["max_distance"], closest=True), ix.knn(q, 8, c["max_distance"]), ix.radius_count(q, c["radius"])

    def check(r):
        same_closest(r[0], e["closest"])
        same_knn(r[1], e["knn"][8])
        assert np.array_equal(r[2].cpu().numpy(), e["count"])
    check(run(index, pts))
    check(run(index, pts))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = run(index, pts)
    side.synchronize()
    check(out)
    parts = [run(index, pts[a:b]) for a, b in ((0, 100), (100, 101), (101, 101), (101, 1025))]
    check(({k: torch.cat([p[0][k] for p in parts]) for k in parts[0][0]}, {k: torch.cat([p[1][k] for p in parts]) for k in parts[0][1]},
           torch.cat([p[2] for p in parts])))
    again = CloudIndex(cloud)                                                       # the records' order is free, the answers are not
    assert again.info == index.info
    check(run(again, pts))
    d2 = pairs_host(c["queries"], c["cloud"])                                       # tie-free: every minimum in reach stands alone
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 1)[e["closest"]["index"] >= 0].all()
    perm = np.random.default_rng(9).permutation(c["cloud"].shape[0])
    moved = CloudIndex(to_dev(c["cloud"][perm])).closest(pts, c["max_distance"], closest=True)
    assert np.array_equal(bits(moved["distance"]), e["closest"]["distance"].view(U32)) and np.array_equal(bits(moved["closest"]), e["closest"]["closest"].view(U32))
    mi = moved["index"].cpu().numpy()
    assert np.array_equal(np.where(mi >= 0, perm[np.maximum(mi, 0)], -1), e["closest"]["index"])


@pytest.mark.parametrize("name", tuple(voxel_cases()))
def test_voxel_downsample_equals_the_rule(name):
    p, col, cell, origin = voxel_cases()[name]
    e = voxel_host(p, cell, origin, col)
    out = voxel_downsample(to_dev(p), cell, origin, None if col is None else to_dev(col))
    n = e["points"].shape[0]
    assert out["counts"] == (n,) and out["points"].shape == (n, 3) and out["count"].dtype is torch.int32 and out["cluster_of"].dtype is torch.int32
    assert np.array_equal(bits(out["points"]), e["points"].view(U32)) and np.array_equal(out["count"].cpu().numpy(), e["count"])
    assert np.array_equal(out["cluster_of"].cpu().numpy(), e["cluster_of"])
    assert ("rgb8" in out) == (col is not None) and (col is None or np.array_equal(out["rgb8"].cpu().numpy(), e["rgb8"]))
    assert out["info"]["bad_points"] == e["bad"] and out["info"]["points"] == int(e["count"].sum()) == int(out["count"].sum())
    if n:
        assert (out["info"]["box"]["lo"], out["info"]["box"]["dims"]) == e["box"]
        perm = np.random.default_rng(2).permutation(p.shape[0])
        other = voxel_downsample(to_dev(p[perm]), cell, origin, None if col is None else to_dev(col[perm]))
        for k in ("points", "count") + (("rgb8",) if col is not None else ()):
            assert out[k].cpu().numpy().tobytes() == other[k].cpu().numpy().tobytes()
        assert np.array_equal(other["cluster_of"].cpu().numpy(), e["cluster_of"][perm])
        own = out["points"][out["cluster_of"].clamp(min=0).long()]                 # cluster_of is consistent with points
        good = (out["cluster_of"] >= 0).cpu().numpy()
        assert np.abs(own.cpu().numpy().astype(np.float64) - p)[good].max() <= cell * (1 + 1e-6)


def test_voxel_downsample_holds_the_vertices_of_simplify_and_refuses_a_huge_box():
    m = base_meshes()["sphere"]                                                     # a closed mesh: every vertex is in a face
    mesh = device_mesh(m, rgb=False)
    for cell, origin in ((2.0 / 23, (0.0, 0.0, 0.0)), (3.5 / 23, (0.1, -0.03, 0.017))):
        simple = simplify(mesh, cell, origin)
        vox = voxel_downsample(mesh["vertices"], cell, origin)
        rows = {r.tobytes(): i for i, r in enumerate(vox["points"].cpu().numpy())}
        at = [rows.get(r.tobytes(), -1) for r in simple["vertices"].cpu().numpy()]
        assert simple["counts"][0] > 10 and min(at) >= 0 and all(a < b for a, b in zip(at, at[1:]))      # a subsequence, bit for bit
        assert vox["counts"][0] == simple["simplify"]["occupied"]
    pts = to_dev(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], np.float32))
    with pytest.raises(ValueError, match="cell box .* larger cell"):
        voxel_downsample(pts, 1e-4)                                                 # 10 001^3 cells: refused before anything is summed
    with pytest.raises(ValueError, match="max_bytes is 64: a larger cell"):
        voxel_downsample(pts, 0.1, max_bytes=64)


def test_remove_outliers_keeps_the_brute_force_set():
    pts, floater, radius = surface_with_floaters()
    want = radius_count_host(pts, pts, radius, exclude_self=True) >= 6
    assert np.array_equal(want, ~floater)                                           # the floaters go, the surface stays
    dev = to_dev(pts)
    col = to_dev(np.random.default_rng(3).integers(0, 256, pts.shape, dtype=np.uint8))
    nrm = to_dev(np.random.default_rng(4).standard_normal(pts.shape).astype(np.float32))
    out = remove_outliers(dev, radius, 6, rgb8=col, normals=nrm)
    assert out["keep"].dtype is torch.bool and np.array_equal(out["keep"].cpu().numpy(), want) and out["counts"] == (int(want.sum()),)
    assert np.array_equal(bits(out["points"]), pts[want].view(U32))                 # in input order
    assert torch.equal(out["rgb8"], col[out["keep"]]) and torch.equal(out["normals"], nrm[out["keep"]])
    index = CloudIndex(dev, cell=0.3)
    again = remove_outliers(dev, radius, 6, index=index)
    assert torch.equal(again["keep"], out["keep"]) and set(again) == {"points", "keep", "counts"}
    assert remove_outliers(dev, radius, 0)["counts"] == (pts.shape[0],)
    spacing = nearest_spacing(index)
    d2 = pairs_host(pts, pts)
    np.fill_diagonal(d2, np.inf)
    nn = np.sqrt(d2.min(1)).astype(np.float32)
    assert spacing["median"] == float(np.sort(nn)[(nn.size - 1) // 2]) and spacing["count"] == nn.size
    assert spacing["mean"] == pytest.approx(float(nn.astype(np.float64).mean()), rel=1e-6)
    assert nearest_spacing(dev) == spacing


def test_cloud_distance_equals_the_restatement():
    cloud, _ = sphere()
    a = cloud[:2000]
    b = (cloud[1500:] * np.float32(1.01)).astype(np.float32)
    taus = (0.02, 0.05, 0.2)
    for max_distance in (math.inf, 0.1):
        out = cloud_distance(to_dev(a), to_dev(b), taus, max_distance)
        assert set(out) == {"a_to_b", "b_to_a", "chamfer", "hausdorff", "precision", "recall", "fscore", "thresholds", "samples"}
        for side, src, dst in (("a_to_b", a, b), ("b_to_a", b, a)):
            e = summary_counts_host(closest_host(src, dst, max_distance)["distance"], taus)
            assert {k: out[side][k] for k in e} == e
            assert (e["beyond"] > 0) == math.isfinite(max_distance) and 0 < e["within"][0] < e["within"][2] <= e["finite"]
        n_a, n_b = a.shape[0], b.shape[0]
        assert out["samples"] == (n_a, n_b)
        assert out["precision"] == tuple(w / n_a for w in out["a_to_b"]["within"]) and out["recall"] == tuple(w / n_b for w in out["b_to_a"]["within"])
        assert out["fscore"] == tuple(2 * p * r / (p + r) for p, r in zip(out["precision"], out["recall"]))
        assert out["chamfer"] == out["a_to_b"]["mean"] + out["b_to_a"]["mean"] and out["hausdorff"] == max(out["a_to_b"]["max"], out["b_to_a"]["max"])
    own = cloud_distance(to_dev(a), to_dev(a), taus)
    assert own["chamfer"] == 0.0 and own["hausdorff"] == 0.0 and own["fscore"] == (1.0, 1.0, 1.0) and own["a_to_b"]["sum"] == own["b_to_a"]["sum_sq"] == 0
    vox = cloud_distance(to_dev(a), to_dev(b), taus, voxel=0.08)
    va, vb = voxel_host(a, 0.08)["points"], voxel_host(b, 0.08)["points"]
    assert vox["samples"] == (va.shape[0], vb.shape[0]) and va.shape[0] < a.shape[0]
    assert vox["a_to_b"]["within"] == summary_counts_host(closest_host(va, vb, math.inf)["distance"], taus)["within"]
    perm = np.random.default_rng(5).permutation(a.shape[0])
    assert cloud_distance(to_dev(a[perm]), to_dev(b), taus, voxel=0.08) == vox
    one = cloud_to_cloud(to_dev(a), CloudIndex(to_dev(b), cell=0.4), taus, 0.1)
    assert one["distance"].shape == (2000,) and one["index"].dtype is torch.int32
    assert {k: v for k, v in one.items() if k not in ("distance", "index")} == cloud_distance(to_dev(a), to_dev(b), taus, 0.1)["a_to_b"]


def test_icp_against_a_cloud_finds_the_planted_motion():
    """A = T B with no point moved by more than a quarter of B's smallest nearest-neighbour distance: the first correspondences
    are the twins, for which fit_pairs(A, B) -- existing code -- is the reference.  Its residual is the fp32 rounding of A and the
    lattice of pair_frame; the bar is twice that rms plus one lattice step h."""
    A, B, T, nn, move = icp_case()
    src, tgt = to_dev(A), to_dev(B)
    index = CloudIndex(tgt)
    first = index.closest(src)
    assert np.array_equal(first["index"].cpu().numpy(), np.arange(B.shape[0]))      # the twins
    ref = alignment.fit_pairs(src, tgt, scale=False)
    out = alignment.icp(src, index, metric="point", scale=False)
    lo = np.minimum(index.info["box"][0], A.min(0)).tolist()                         # icp's frame for max_distance = inf: the box of
    hi = np.maximum(index.info["box"][1], A.max(0)).tolist()                         # the index and of the cloud, half its edge around it
    pad = 0.5 * max(b - a for a, b in zip(lo, hi))
    h = alignment.pair_frame(tuple(a - pad for a in lo), tuple(b + pad for b in hi))[1]
    print(f"icp to a cloud: rms {out['rms']:.3e} after {out['iterations']} steps ({out['reason']}); fit_pairs rms {ref['rms']:.3e}, h {h:.3e}, "
          f"bar {2 * ref['rms'] + h:.3e}; history {[x['rms'] for x in out['history']]}")
    assert out["converged"] is True and out["reason"] == "tolerance"
    assert out["rms"] <= 2 * ref["rms"] + h
    assert np.abs(out["T"] @ T - np.eye(4)).max() < 1e-5                            # T maps A back onto B
    assert alignment.icp(src, index, metric="point", scale=False)["T"].tobytes() == out["T"].tobytes()
    with pytest.raises(ValueError, match='a cloud has no planes.*metric="point"'):
        alignment.icp(src, index, metric="plane")


def test_empty_and_degenerate_clouds_launch_no_query(monkeypatch):
    full = CloudIndex(to_dev(random_cloud(65, 1)))
    out = full.closest(torch.zeros(0, 3, device=DEV), closest=True)
    assert out["distance"].shape == (0,) and out["index"].shape == (0,) and out["closest"].shape == (0, 3)
    assert full.knn(torch.zeros(0, 3, device=DEV), 3)["index"].shape == (0, 3) and full.radius_count(torch.zeros(0, 3, device=DEV), 1.0).shape == (0,)
    launch = N.launch

    def no_query(name, *a, **k):
        assert name not in ("lrf_cloud_closest", "lrf_cloud_knn", "lrf_cloud_radius_count"), "a query was launched for an index without a point"
        return launch(name, *a, **k)
    q = to_dev(cases()["queries that are not finite"]["queries"])
    fin = torch.isfinite(q).all(1).cpu().numpy()
    clouds = (torch.zeros(0, 3, device=DEV), to_dev(np.full((5, 3), np.nan, np.float32)))
    indices = [CloudIndex(c) for c in clouds]
    monkeypatch.setattr(N, "launch", no_query)
    for index in indices:
        assert index.nbytes == 0 and index.info["points"] == 0 and index.info["box"] is None
        out = index.closest(q, closest=True)
        d = out["distance"].cpu().numpy()
        assert np.isinf(d[fin]).all() and np.isnan(d[~fin]).all() and (out["index"] == -1).all() and torch.isnan(out["closest"]).all()
        near = index.knn(q, 3)
        assert near["distance"].shape == (64, 3) and np.isinf(near["distance"].cpu().numpy()[fin]).all() and (near["index"] == -1).all()
        assert np.array_equal(index.radius_count(q, 1.0).cpu().numpy(), np.where(fin, 0, -1))
    assert indices[1].info["nonfinite_points"] == 5
    monkeypatch.setattr(N, "launch", launch)
    assert voxel_downsample(clouds[0], 0.1)["counts"] == (0,)
    none = nearest_spacing(clouds[0])
    assert none["count"] == 0 and math.isnan(none["mean"]) and math.isnan(none["median"])
    one = nearest_spacing(to_dev(random_cloud(1, 2)))
    assert one["count"] == 0 and math.isnan(one["median"])


def test_refusals_on_the_device():
    cloud = to_dev(random_cloud(65, 1))
    pts = torch.zeros(4, 3, device=DEV)
    index = CloudIndex(cloud)
    for call in (lambda: CloudIndex(cloud.cpu()), lambda: index.closest(pts.cpu()), lambda: index.knn(pts.cpu(), 2), lambda: index.radius_count(pts.cpu(), 0.1),
                 lambda: voxel_downsample(cloud.cpu(), 0.1), lambda: cloud_to_cloud(pts.cpu(), index), lambda: remove_outliers(cloud.cpu(), 0.1, 2)):
        with pytest.raises(NativeError):
            call()
    with pytest.raises(ValueError, match="cell box .* larger cell"):
        CloudIndex(cloud, cell=1e-4)                                                # 20 000^3 cells
    with pytest.raises(ValueError, match="cell box .* max_bytes is 4096: a larger cell"):
        CloudIndex(cloud, cell=0.01, max_bytes=4096)
    assert CloudIndex(cloud, cell=index.info["cell"], max_bytes=index.nbytes).info == index.info
    with pytest.raises(ValueError, match="larger cell"):
        CloudIndex(cloud, cell=index.info["cell"], max_bytes=index.nbytes - 1)
    big = to_dev(sphere()[0])
    full = CloudIndex(big)
    small = CloudIndex(big, max_bytes=200000)                                       # the default cell grows until the grid's words fit half
    assert 8 * math.prod(full.info["dims"]) > 100000 >= 8 * math.prod(small.info["dims"])
    assert small.info["cell"] == 2 * full.info["cell"] and small.nbytes <= 200000
    assert torch.equal(small.closest(pts, 0.5)["index"], full.closest(pts, 0.5)["index"])


def test_chunks_give_the_bytes_of_one_call(monkeypatch):
    """Every query over points at 5 points per launch: 11 queries are two full chunks and a remainder.  exclude_self (the chunk's
    first query is cloud point i0) and the viewpoint per query (its rows start at i0) are what a wrong offset corrupts."""
    cloud = random_cloud(11, 80)
    cloud[4, 1], cloud[9] = np.nan, cloud[2]                                       # one point that is not finite, one duplicate pair
    pts, view = to_dev(cloud), to_dev(random_cloud(11, 81, 3.0))
    index = CloudIndex(pts)
    assert index.info["points"] == 10 and index.info["nonfinite_points"] == 1

    def run():
        return (index.closest(pts, closest=True), index.knn(pts, 3, exclude_self=True), index.radius_count(pts, 0.75, exclude_self=True),
                index.normals(pts, 1.5, 3, view), index.normals(pts, 1.5, 3, (0.5, -2.0, 1.0)))
    names = record_launches(monkeypatch)
    whole = run()
    assert names == ["lrf_cloud_closest", "lrf_cloud_knn", "lrf_cloud_radius_count", "lrf_cloud_normals", "lrf_cloud_normals"]
    assert int(whole[2].max()) >= 2 and int(whole[3]["count"].max()) >= 3 and whole[1]["distance"][9, 0] == 0  # neighbours, and the twin
    assert not torch.equal(whole[3]["normals"].view(torch.int32), whole[4]["normals"].view(torch.int32))      # the viewpoints matter
    monkeypatch.setattr(_checks, "POINTS_PER_CALL", 5)
    del names[:]
    parts = run()
    assert names == [n for name in ("lrf_cloud_closest", "lrf_cloud_knn", "lrf_cloud_radius_count", "lrf_cloud_normals", "lrf_cloud_normals")
                     for n in [name] * 3]
    for a, b in zip(whole, parts):
        same_bits(a, b)
