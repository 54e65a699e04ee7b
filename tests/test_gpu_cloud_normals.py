"""Point-cloud normals and point-to-plane ICP against a cloud on the GPU, against the restatements of
tests/cloud_normal_cases.py: normals, eigenvalues, counts and the 48 plane words bit for bit, then the registration of a cloud
onto a scan that is not its own sample.

The registration's figures on the host restatement (tests/test_cloud_normals_host.py prints them; the GPU loop must agree to
1e-9): deviation 2.8e-4 .. 3.4e-4 with a free scale and 4.8e-5 .. 5.0e-5 rigid after 5 to 7 steps; the issue's float64 prototype
found point-to-point after 30 iterations still at 6e-2 .. 1.8e-1."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from align_cases import deviation, truth
from cloud_cases import cell_sweep
from cloud_normal_cases import (CASE_NAMES, SCAN_RUNS, cases, expected, icp_plane_cloud_host, plane_cloud_case, plane_cloud_host, scan, scan_normals,
                                scan_source, scan_spacing)
from localrf_amd import alignment
from localrf_amd import _native as N
from localrf_amd.cloud import NORMAL_ORDERS, CloudIndex, estimate_normals, nearest_spacing
from mesh_util import DEV, bits, to_dev

pytestmark = pytest.mark.gpu
U32 = np.uint32


def same(out, e, rows=None):
    """A device result against the restatement (rows: the restatement's rows in the result's order), bit for bit."""
    rows = slice(None) if rows is None else rows
    n = e["count"][rows].shape[0]
    assert out["normals"].shape == (n, 3) and out["eigenvalues"].shape == (n, 3) and out["count"].shape == (n,)
    assert out["normals"].dtype is torch.float32 and out["eigenvalues"].dtype is torch.float32 and out["count"].dtype is torch.int32
    assert np.array_equal(out["count"].cpu().numpy(), e["count"][rows])
    assert np.array_equal(bits(out["eigenvalues"]), e["eigenvalues"][rows].view(U32))
    assert np.array_equal(bits(out["normals"]), e["normals"][rows].view(U32))


def view_of(c, rows=None):
    v = c["viewpoint"]
    if v is None or not isinstance(v, np.ndarray):
        return v
    return to_dev(v if rows is None else v[rows])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_normals_equal_the_restatement_at_every_cell(name):
    c, e = cases()[name], expected(name)
    cloud, pts = to_dev(c["cloud"]), to_dev(c["queries"])
    before = [t.clone() for t in (cloud, pts)]
    cells, _ = cell_sweep(c["cloud"])
    for cell in cells:
        index = CloudIndex(cloud, cell=cell)
        out = index.normals(pts, c["radius"], c["min_neighbours"], view_of(c))
        assert set(out) == {"normals", "eigenvalues", "count"}
        same(out, e)
        assert torch.equal(out["count"], index.radius_count(pts, c["radius"]))
        if c["own"]:
            for order in NORMAL_ORDERS:
                own = estimate_normals(index, c["radius"], c["min_neighbours"], view_of(c), order=order)
                same(own, e)
                lam = e["eigenvalues"].astype(np.float32)
                with np.errstate(all="ignore"):
                    total = lam.sum(1, dtype=np.float32)
                    want = np.where(total == 0, np.float32(0), lam[:, 0] / total)
                got = own["variation"].cpu().numpy()
                assert got.shape == want.shape and np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)
    for t, b in zip((cloud, pts), before):                                          # the inputs are left untouched
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))


def test_the_same_bytes_for_every_run_stream_split_permutation_and_order():
    c, e = cases()["sphere, viewpoints outside"], expected("sphere, viewpoints outside")
    cloud, view = to_dev(c["cloud"]), view_of(c)
    index = CloudIndex(cloud)
    m = cloud.shape[0]
    same(index.normals(cloud, c["radius"], viewpoint=view), e)
    same(index.normals(cloud, c["radius"], viewpoint=view), e)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = index.normals(cloud, c["radius"], viewpoint=view), estimate_normals(index, c["radius"], viewpoint=view, order="records")
    side.synchronize()
    same(out[0], e)
    same(out[1], e)
    parts = [index.normals(cloud[a:b], c["radius"], viewpoint=view[a:b]) for a, b in ((0, 100), (100, 101), (101, 101), (101, m))]
    same({k: torch.cat([p[k] for p in parts]) for k in parts[0]}, e)
    by_input, by_record = (estimate_normals(index, c["radius"], viewpoint=view, order=o) for o in NORMAL_ORDERS)
    for k in ("normals", "eigenvalues", "variation"):
        assert torch.equal(by_input[k].view(torch.int32), by_record[k].view(torch.int32))
    assert torch.equal(by_input["count"], by_record["count"])
    perm = np.random.default_rng(11).permutation(m)
    moved = CloudIndex(to_dev(c["cloud"][perm]))
    same(moved.normals(cloud, c["radius"], viewpoint=view), e)                      # the same queries over the permuted cloud
    for order in NORMAL_ORDERS:                                                     # the permuted cloud on itself: the permuted rows
        same(estimate_normals(moved, c["radius"], viewpoint=view_of(c, perm), order=order), e, perm)
    bad = cases()["cloud entries that are not finite"]                              # record order fills the rows without a record
    e_bad = expected("cloud entries that are not finite")
    assert (e_bad["count"] == -1).sum() == 6
    for order in NORMAL_ORDERS:
        same(estimate_normals(to_dev(bad["cloud"]), bad["radius"], order=order), e_bad)
    inside = expected("sphere, viewpoint inside")                                   # one viewpoint for all: the twin with the signs turned
    got = estimate_normals(index, c["radius"], viewpoint=(0.0, 0.0, 0.0))
    same(got, inside)
    radial = (inside["normals"].astype(np.float64) * c["cloud"]).sum(1)
    assert (radial < -0.99).all() and ((e["normals"].astype(np.float64) * c["cloud"]).sum(1) > 0.99).all()


# ------------------------------------------------------------------------------------------------ lrf_align_plane_cloud
def plane_cloud_words(index, normals, cur, near, c, u, gate):
    return alignment._add_words(alignment._plane_words(index, cur, near, c, u, gate, normals).cpu())


def test_plane_cloud_words_equal_the_restatement_for_every_order_and_run():
    B, normals, cloud, c, u, max_distance, gate, brute = plane_cloud_case()
    index = CloudIndex(to_dev(B))
    cur = to_dev(cloud)
    near = index.closest(cur, max_distance, closest=True)
    host = {k: v.cpu().numpy() for k, v in near.items()}
    assert all(np.array_equal(host[k].view(U32 if host[k].dtype == np.float32 else np.int32), brute[k].view(U32 if host[k].dtype == np.float32 else np.int32))
               for k in ("closest", "index", "distance"))
    want = plane_cloud_host(cloud, host["closest"], host["index"], host["distance"], normals, c, u, np.float32(gate))
    print("plane-cloud words 0..4 (summed, unmatched, gated, degenerate, out of range):", want[:5])
    assert min(want[:5]) > 0 and want[1] == 2 and want[3] >= 2 and sum(want[:5]) == cloud.shape[0] and want[5] == 0 and want[42:] == [0] * 6
    nrm = to_dev(normals)
    assert plane_cloud_words(index, nrm, cur, near, c, u, gate) == want
    assert plane_cloud_words(index, nrm, cur, near, c, u, gate) == want
    q = torch.from_numpy(np.random.default_rng(2).permutation(cloud.shape[0])).to(DEV)
    shuffled = {k: v[q].contiguous() for k, v in near.items()}
    assert plane_cloud_words(index, nrm, cur[q].contiguous(), shuffled, c, u, gate) == want
    open_gate = plane_cloud_host(cloud, host["closest"], host["index"], host["distance"], normals, c, u, np.float32(np.inf))
    assert open_gate[2] == 0 and plane_cloud_words(index, nrm, cur, near, c, u, math.inf) == open_gate
    longer = to_dev((normals.astype(np.float64) * 3.0).astype(np.float32))          # any length: the kernel normalises in fp64
    far = plane_cloud_host(cloud, host["closest"], host["index"], host["distance"], longer.cpu().numpy(), c, u, np.float32(gate))
    assert plane_cloud_words(index, longer, cur, near, c, u, gate) == far and far[:5] == want[:5]
    p = N.LrfAlignPlaneCloud()                                                      # an index past the cloud is unmatched, not read
    wild = near["index"].clone()
    wild[:3] = torch.tensor([B.shape[0], -2, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    host_wild = wild.cpu().numpy()
    words = torch.full((48,), -1, dtype=torch.int64, device=DEV)
    p.points, p.closest, p.index, p.distance, p.normals = cur.data_ptr(), near["closest"].data_ptr(), wild.data_ptr(), near["distance"].data_ptr(), nrm.data_ptr()
    p.N, p.M, p.u, p.gate = cloud.shape[0], B.shape[0], u, gate
    for k in range(3):
        p.c[k] = c[k]
    N.launch("lrf_align_plane_cloud", cur.device, C.byref(p), words.data_ptr(), guard=True)
    assert words.tolist() == plane_cloud_host(cloud, host["closest"], host_wild, host["distance"], normals, c, u, np.float32(gate))


# ------------------------------------------------------------------------------------------------ registration
@functools.lru_cache(maxsize=None)
def scan_on_device():
    """(the scan's index, its normals at 4 median spacings): the median and the normals are the restatement's, bit for bit."""
    index = CloudIndex(to_dev(scan()))
    median = nearest_spacing(index)["median"]
    assert median == scan_spacing()
    own = estimate_normals(index, 4.0 * median)
    same(own, scan_normals())
    assert int(own["count"].min()) >= 29
    return index, own["normals"]


@pytest.mark.parametrize("k,free", SCAN_RUNS)
def test_icp_plane_against_a_scan_recovers_the_similarity(k, free):
    """The source is no sample of the scan: point-to-point has a floor of about half a spacing along the surface, point-to-plane
    with the scan's own normals does not.  Bars: converged by tolerance within 20 iterations; the deviation within 1e-9 of the
    host loop's (the words are the same integers, the host solve sees another frame centre in the last bits); below 1e-3; at
    least 10 times below point-to-point's after 20 iterations."""
    index, normals = scan_on_device()
    want, cloud = truth(k, free), to_dev(scan_source(k, free))
    out = alignment.icp(cloud, index, scale=free, metric="plane", target_normals=normals, iterations=20)
    point = alignment.icp(cloud, index, scale=free, metric="point", iterations=20)
    T_host, steps = icp_plane_cloud_host(scan_source(k, free), scan(), scan_normals()["normals"], free)
    dev, dev_point, dev_host = deviation(out["T"], want), deviation(point["T"], want), deviation(T_host, want)
    print(f"perturbation {k}, scale {'free' if free else 'fixed'}: plane deviation {dev:.3e} after {out['iterations']} iterations ({out['reason']}), "
          f"host loop {dev_host:.3e} after {len(steps)}, point {dev_point:.3e} after {point['iterations']} ({point['reason']}), ratio {dev_point / dev:.0f}")
    assert out["converged"] is True and out["reason"] == "tolerance" and out["iterations"] == len(out["history"]) <= 20
    assert all(set(h) >= {"rms", "count", "step", "unmatched", "gated", "degenerate", "out_of_range", "cond"} for h in out["history"])
    assert out["count"] == 1500 and out["history"][-1]["degenerate"] == 0
    assert abs(dev - dev_host) <= 1e-9
    assert dev < 1e-3
    assert 10 * dev <= dev_point
    again = alignment.icp(cloud, index, scale=free, metric="plane", target_normals=normals, iterations=20)
    assert again["T"].tobytes() == out["T"].tobytes() and again["history"] == out["history"]


def test_icp_counts_points_without_a_normal_and_still_refuses_planes_without_normals():
    index, normals = scan_on_device()
    cloud = to_dev(scan_source(0, False))
    none = torch.zeros_like(normals)
    out = alignment.icp(cloud, index, scale=False, target_normals=none)
    assert out["converged"] is False and out["reason"] == "degenerate" and out["iterations"] == 0 and out["history"][0]["degenerate"] == 1500
    half = normals.clone()
    half[::2] = 0.0
    some = alignment.icp(cloud, index, scale=False, target_normals=half, iterations=3)
    assert 0 < some["history"][0]["degenerate"] < 1500 and some["history"][0]["degenerate"] + some["history"][0]["count"] == 1500
    with pytest.raises(ValueError, match='a cloud has no planes.*metric="point"'):
        alignment.icp(cloud, index)
    with pytest.raises(ValueError, match="target_normals"):
        alignment.icp(cloud, index, target_normals=normals.cpu())
    with pytest.raises(ValueError, match="target_normals"):
        alignment.icp(cloud, index, target_normals=normals[:-1])
