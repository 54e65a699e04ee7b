"""The registration on the GPU against the restatements of tests/align_cases.py: the three kernels bit for bit, then ICP, the
trajectory error and mesh alignment against known similarities.

Reached on the MI355X (bar ICP_BAR = 1e-5 in scale, every rotation entry and every translation component, iterations=10):
the eight blob runs of test_icp_plane_recovers_the_similarity ended 1.8e-9 .. 1.4e-8 from the truth, converged within 5 or 6
iterations -- the figures of the host restatement (tests/test_align_host.py), digit for digit.
test_align_meshes_brings_a_moved_simplified_mesh_back: Chamfer after alignment / Chamfer of the unmoved simplified mesh =
0.312 (sphere) and 0.601 (torus), bar 1.05: the free scale lets the inscribed simplified mesh grow onto the surface."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from align_cases import (ICP_BAR, ICP_RUNS, PAIR_SIZES, PERTURBATIONS, TRANSFORM_SIZES, add_words, apply, blob, deviation,
                         move_poses, pair_inputs, pairs_host, parts, plane_host, sim, sim_inverse, source_cloud, trajectory,
                         transform_host, truth, umeyama_host)
from localrf_amd import NativeError, _checks, alignment, cloud, mesh_distance
from localrf_amd import _native as N
from localrf_amd.mesh import simplify
from localrf_amd.mesh_distance import MeshIndex
from mesh_clean_cases import base_meshes
from cloud_normal_cases import plane_cloud_case, plane_cloud_host
from mesh_distance_cases import planar
from point_layer_cases import launch_lists
from mesh_util import DEV, bits, device_mesh, record_launches, same_bits, to_dev

pytestmark = pytest.mark.gpu
U32 = np.uint32
T_ANY = sim(0.7, 1.3, 0.0, axis=(0.3, -1.0, 0.5), t=(0.25, -1.5, 3.0))


@functools.lru_cache(maxsize=None)
def blob_index():
    return MeshIndex(device_mesh(blob(), rgb=False))


@pytest.mark.parametrize("n", TRANSFORM_SIZES)
def test_transform_equals_the_fp64_expression_and_works_in_place(n):
    p = (np.random.default_rng(n).standard_normal((n, 3)) * 3).astype(np.float32)
    want = transform_host(T_ANY[:3], p)
    dev = to_dev(p)
    out = alignment.transform_points(dev, T_ANY)
    assert out.shape == (n, 3) and out.data_ptr() != dev.data_ptr() and np.array_equal(bits(dev), p.view(U32))
    assert np.array_equal(bits(out), want.view(U32))
    t = (C.c_double * 12)(*T_ANY[:3].reshape(-1).tolist())
    N.launch("lrf_align_transform", dev.device, t, dev.data_ptr(), n, dev.data_ptr(), guard=True)
    assert np.array_equal(bits(dev), want.view(U32))
    assert alignment.transform_points(torch.zeros(0, 3, device=DEV), T_ANY).shape == (0, 3)


def pair_words(c, h, a, b, keep):
    fr = N.LrfAlignFrame()
    fr.h = h
    for k in range(3):
        fr.c[k] = c[k]
    words = torch.full((24,), -1, dtype=torch.int64, device=DEV)                    # the entry point zeroes them itself
    N.launch("lrf_align_pairs", words.device, C.byref(fr), a.data_ptr(), b.data_ptr(), None if keep is None else keep.data_ptr(),
             a.shape[0], words.data_ptr(), guard=True)
    return words.tolist()


@pytest.mark.parametrize("n", PAIR_SIZES)
def test_pair_words_equal_the_restatement_for_every_order(n):
    a, b, keep, c, h = pair_inputs(100 + n, n)
    want = pairs_host(c, h, a, b, keep)
    if n >= 63:
        assert min(want[:4]) > 0                                                # summed, out of range, masked and not finite
    assert pair_words(c, h, to_dev(a), to_dev(b), to_dev(keep)) == want
    assert pair_words(c, h, to_dev(a), to_dev(b), None) == pairs_host(c, h, a, b)
    q = np.random.default_rng(1).permutation(n)
    assert pair_words(c, h, to_dev(a[q]), to_dev(b[q]), to_dev(keep[q])) == want


def test_fit_pairs_adds_its_chunks_exactly():
    n = (1 << 20) + 5
    rng = np.random.default_rng(8)
    a = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    b = apply(T_ANY, a.astype(np.float64)).astype(np.float32)
    a[::1001, 1], b[5::2003, 0] = np.nan, np.inf
    keep = rng.random(n) > 0.1
    both = np.concatenate([a, b])
    both = np.where(np.isfinite(both), both, np.nan)
    c, h = alignment.pair_frame(np.nanmin(both, 0), np.nanmax(both, 0))
    cut = 1 << 20
    words = add_words(pairs_host(c, h, a[:cut], b[:cut], keep[:cut]), pairs_host(c, h, a[cut:], b[cut:], keep[cut:]))
    for free in (True, False):
        want = alignment.solve_pairs(words, c, h, free)
        got = alignment.fit_pairs(to_dev(a), to_dev(b), to_dev(keep), scale=free)
        assert got["T"].tobytes() == want["T"].tobytes() and {k: got[k] for k in want if k != "T"} == {k: want[k] for k in want if k != "T"}
    assert got["count"] + got["masked"] + got["nonfinite"] + got["out_of_range"] == n and got["nonfinite"] > 1000 and got["out_of_range"] == 0
    assert deviation(alignment.fit_pairs(to_dev(a), to_dev(b), to_dev(keep))["T"], T_ANY) < 1e-6
    with pytest.raises(ValueError, match="at least 3"):
        alignment.fit_pairs(to_dev(a[:5]), to_dev(b[:5]), torch.zeros(5, dtype=torch.bool, device=DEV))


def plane_case():
    """The blob plus a face without area, and a cloud with a point on that face, one far away, one NaN, points beyond the
    gate and points beyond the frame."""
    m = blob()
    nv = m["vertices"].shape[0]
    mesh = dict(m, vertices=np.concatenate([m["vertices"], np.array([(1.0, 2.0, 0), (1.2, 2.0, 0), (1.1, 2.0, 0)], np.float32)]),
                faces=np.concatenate([m["faces"], np.array([(nv, nv + 1, nv + 2)], np.int32)]))
    mesh["counts"] = (nv + 3, 513)
    cloud = np.concatenate([source_cloud(truth(0, True)), np.array([(1.1, 2.01, 0.0), (1.15, 1.99, 0.01), (9, 9, 9), (np.nan, 0, 0)], np.float32)])
    return mesh, cloud, (-0.95, 0.0, 0.0), 2.0, 0.3, 0.04


def plane_words(index, cur, near, c, u, gate):
    return alignment._add_words(alignment._plane_words(index, cur, near, c, u, gate).cpu())


def test_plane_words_equal_the_restatement_for_every_order_and_run():
    mesh, cloud, c, u, max_distance, gate = plane_case()
    index = MeshIndex(device_mesh(mesh, rgb=False))
    cur = to_dev(cloud)
    near = index.closest(cur, max_distance, closest=True)
    host = {k: v.cpu().numpy() for k, v in near.items()}
    want = plane_host(mesh, cloud, host["closest"], host["face"], host["distance"], c, u, np.float32(gate))
    print("plane words 0..4 (summed, unmatched, gated, degenerate, out of range):", want[:5])
    assert min(want[:5]) > 0 and want[3] == 2 and sum(want[:5]) == cloud.shape[0] and want[5] == 0 and want[42:] == [0] * 6
    got = plane_words(index, cur, near, c, u, gate)
    assert got == want
    assert plane_words(index, cur, near, c, u, gate) == want
    q = torch.from_numpy(np.random.default_rng(2).permutation(cloud.shape[0])).to(DEV)
    shuffled = {k: v[q].contiguous() for k, v in near.items()}
    assert plane_words(index, cur[q].contiguous(), shuffled, c, u, gate) == want
    open_gate = plane_host(mesh, cloud, host["closest"], host["face"], host["distance"], c, u, np.float32(np.inf))
    assert open_gate[2] == 0 and plane_words(index, cur, near, c, u, math.inf) == open_gate


@pytest.mark.parametrize("k,free", ICP_RUNS)
def test_icp_plane_recovers_the_similarity(k, free):
    want, cloud = truth(k, free), to_dev(source_cloud(truth(k, free)))
    out = alignment.icp(cloud, blob_index(), scale=free, iterations=10, max_distance=PERTURBATIONS[k][3])
    print(f"perturbation {k}, scale {'free' if free else 'fixed'}: deviation {deviation(out['T'], want):.3e} after {out['iterations']} "
          f"iterations ({out['reason']}), rms {out['rms']:.3e}, steps {[h['step'] for h in out['history']]}")
    assert deviation(out["T"], want) <= ICP_BAR
    assert out["converged"] is True and out["reason"] == "tolerance" and out["iterations"] == len(out["history"]) <= 10
    assert out["count"] > 1400 and all(set(h) >= {"rms", "count", "step"} for h in out["history"])
    if not free:
        assert parts(out["T"])[0] == pytest.approx(1.0, abs=1e-12)
    again = alignment.icp(cloud, blob_index(), scale=free, iterations=10, max_distance=PERTURBATIONS[k][3])
    assert again["T"].tobytes() == out["T"].tobytes() and again["history"] == out["history"]


def test_icp_point_descends():
    cloud = to_dev(source_cloud(truth(0, True)))
    out = alignment.icp(cloud, blob_index(), metric="point", iterations=10)
    rms = [h["rms"] for h in out["history"]]
    print("point-to-point rms per iteration:", rms, out["reason"])
    assert len(rms) >= 2 and all(b <= a + 1e-6 for a, b in zip(rms, rms[1:])) and rms[-1] < rms[0]
    assert all(h["count"] == 1500 for h in out["history"])
    mesh = device_mesh(blob(), rgb=False)
    assert alignment.icp(cloud, mesh, metric="point", iterations=2)["T"].tobytes() == alignment.icp(cloud, blob_index(), metric="point", iterations=2)["T"].tobytes()


def test_a_flat_target_is_reported_as_degenerate():
    rng = np.random.default_rng(4)
    cloud = np.concatenate([rng.uniform(0.1, 0.9, (500, 2)), 0.25 + 0.01 * rng.standard_normal((500, 1))], 1).astype(np.float32)
    for metric, free in (("plane", True), ("plane", False)):
        out = alignment.icp(to_dev(cloud), device_mesh(planar(), rgb=False), metric=metric, scale=free)
        assert out["converged"] is False and out["reason"] == "degenerate" and out["iterations"] == 0 and out["count"] == 500
        assert np.array_equal(out["T"], np.eye(4))
    few = alignment.icp(to_dev(cloud[:5]), blob_index())
    assert few["converged"] is False and few["reason"] == "degenerate"
    far = alignment.icp(to_dev(cloud + 50), blob_index(), max_distance=0.5)
    assert far["converged"] is False and far["reason"] == "degenerate" and far["count"] == 0


def test_trajectory_error_after_alignment():
    gt = trajectory()
    T = sim(0.6, 1.15, 0.0, axis=(1.0, 0.5, -2.0), t=(0.1, -0.1, 0.05))
    est = move_poses(gt, sim_inverse(T))
    out = alignment.trajectory_error(to_dev(est), to_dev(gt))
    print(f"trajectory: ate_rmse {out['ate_rmse']:.3e} mean {out['ate_mean']:.3e} max {out['ate_max']:.3e}, deviation {deviation(out['T'], T):.3e}")
    assert out["ate_rmse"] <= 1e-6 and out["ate_mean"] <= out["ate_rmse"] <= out["ate_max"] and out["count"] == 30
    assert deviation(out["T"], T) < 1e-5
    rigid = alignment.trajectory_error(to_dev(est), to_dev(gt), scale=False)
    assert parts(rigid["T"])[0] == pytest.approx(1.0, abs=1e-12) and rigid["ate_rmse"] > 1e-3
    moved = gt.copy()
    moved[11, :, 3] += np.array((0.06, -0.08, 0.0), np.float32)                      # one centre displaced by 0.1
    out = alignment.trajectory_error(to_dev(est), to_dev(moved))
    ref = umeyama_host(est[:, :, 3], moved[:, :, 3])                                 # the fit by another route
    d = np.linalg.norm(apply(ref, est[:, :, 3]) - moved[:, :, 3].astype(np.float64), axis=1)
    shift = np.linalg.norm(apply(ref, est[:, :, 3]) - gt[:, :, 3].astype(np.float64), axis=1).max()     # how far the fit itself moved
    print(f"displaced centre: ate_max {out['ate_max']:.6f}, restatement {d.max():.6f}, the fit's own shift {shift:.6f}")
    assert abs(out["ate_max"] - d.max()) <= 1e-6 and d.argmax() == 11
    assert abs(out["ate_max"] - 0.1) <= shift + 1e-6 and shift < 0.03
    assert abs(out["ate_rmse"] - math.sqrt((d * d).mean())) <= 1e-6


@pytest.mark.parametrize("name", ("sphere", "torus"))
def test_align_meshes_brings_a_moved_simplified_mesh_back(name):
    original = device_mesh(base_meshes()[name], rgb=False)
    # one cell size: 2 voxels of the analytic lattice, the finer of test_gpu_mesh_distance's two.  The coarser, 4 / 23 = 0.174, is
    # wider than the torus's tube radius 0.11: the 110 faces it leaves are no surface that a tube could be registered to
    simple = simplify(original, 2.0 / 23)
    assert 0 < simple["counts"][1] < original["counts"][1]
    base = mesh_distance.mesh_distance(simple, original, 0.02)["chamfer"]
    moved = alignment.transform_mesh(simple, sim_inverse(truth(0, True)))
    assert mesh_distance.mesh_distance(moved, original, 0.02)["chamfer"] > base
    out = alignment.align_meshes(moved, original, 0.02)
    after = mesh_distance.mesh_distance(out["mesh"], original, 0.02)["chamfer"]
    print(f"{name}: chamfer unmoved {base:.6f}, after alignment {after:.6f} (ratio {after / base:.4f}, bar 1.05), {out['iterations']} iterations "
          f"({out['reason']})")                                                     # both shapes are symmetric: T itself is not determined
    assert after <= 1.05 * base
    assert out["mesh"]["faces"] is moved["faces"] and out["mesh"]["counts"] == moved["counts"]
    index = MeshIndex(original)
    again = alignment.align_meshes(moved, index, 0.02)
    assert again["T"].tobytes() == out["T"].tobytes()


def test_transform_mesh_rotates_normals_and_shares_the_faces():
    m = blob()
    rng = np.random.default_rng(6)
    nrm = rng.standard_normal(m["vertices"].shape).astype(np.float32)
    mesh = device_mesh(m, rgb=False, normals=to_dev(nrm), note="kept")
    out = alignment.transform_mesh(mesh, T_ANY)
    s, R, t = parts(T_ANY)
    assert out["faces"] is mesh["faces"] and out["rgb8"] is None and out["note"] == "kept" and out["counts"] == mesh["counts"]
    assert out["vertices"].data_ptr() != mesh["vertices"].data_ptr() and np.array_equal(bits(mesh["vertices"]), m["vertices"].view(U32))
    assert np.array_equal(bits(out["vertices"]), transform_host(T_ANY[:3], m["vertices"]).view(U32))
    got = out["normals"].cpu().numpy().astype(np.float64)
    assert np.abs(got - nrm.astype(np.float64) @ R.T).max() < 1e-6                   # rotated: neither scaled (1.3) nor shifted
    assert np.abs(np.linalg.norm(got, axis=1) - np.linalg.norm(nrm.astype(np.float64), axis=1)).max() < 1e-6
    assert np.array_equal(bits(mesh["normals"]), nrm.view(U32))
    plain = alignment.transform_mesh(device_mesh(m, rgb=False), T_ANY)
    assert "normals" not in plain
    with pytest.raises(NativeError):
        alignment.transform_points(torch.zeros(3, 3), T_ANY)


def test_chunks_give_the_bytes_and_the_words_of_one_call(monkeypatch):
    """transform_points at 5 points per launch, and the plane words of both targets at 5 points per launch: 11 points are two full
    chunks and a remainder.  The words of the chunks, added, are the words of one call and the restatement's."""
    names = record_launches(monkeypatch)
    p = to_dev((np.random.default_rng(12).standard_normal((11, 3)) * 3).astype(np.float32))
    whole = alignment.transform_points(p, T_ANY)
    mesh, source, c, u, max_distance, gate = plane_case()
    B, normals, source_b, c_b, u_b, max_distance_b, gate_b, _ = plane_cloud_case()
    runs = []
    for index, src, nrm, frame in ((MeshIndex(device_mesh(mesh, rgb=False)), source[-11:], None, (c, u, max_distance, gate)),
                                   (cloud.CloudIndex(to_dev(B)), source_b[-11:], to_dev(normals), (c_b, u_b, max_distance_b, gate_b))):
        cur = to_dev(src)
        near = index.closest(cur, frame[2], closest=True)
        host = {k: v.cpu().numpy() for k, v in near.items()}
        want = (plane_host(mesh, src, host["closest"], host["face"], host["distance"], frame[0], frame[1], np.float32(frame[3])) if nrm is None else
                plane_cloud_host(src, host["closest"], host["index"], host["distance"], normals, frame[0], frame[1], np.float32(frame[3])))
        assert sum(want[:5]) == 11 and want[0] > 0 and want[1] > 0                  # summed and unmatched points among the eleven
        runs.append((index, cur, near, frame, nrm, want))
        del names[:]
        words = alignment._plane_words(index, cur, near, frame[0], frame[1], frame[3], nrm)
        assert tuple(words.shape) == (1, 48) and len(names) == 1 and alignment._add_words(words.cpu()) == want
    monkeypatch.setattr(_checks, "POINTS_PER_CALL", 5)
    monkeypatch.setattr(alignment, "PAIRS_PER_CALL", 5)
    del names[:]
    same_bits(alignment.transform_points(p, T_ANY), whole)
    assert names == ["lrf_align_transform"] * 3
    for index, cur, near, frame, nrm, want in runs:
        del names[:]
        words = alignment._plane_words(index, cur, near, frame[0], frame[1], frame[3], nrm)
        assert tuple(words.shape) == (3, 48) and names == ["lrf_align_plane" if nrm is None else "lrf_align_plane_cloud"] * 3
        assert alignment._add_words(words.cpu()) == want and words[2].tolist() != words[0].tolist()


def test_the_point_layer_launches_what_it_launched_before_its_helpers_were_shared():
    """tests/golden/point_layer_launches.json: per public call the (symbol, count) of every launch, recorded from the code before
    the refactor (tests/golden/make_golden_point_launches.py).  The same launches, in the same order, chunked the same way."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_layer_launches.json")) as f:
        want = json.load(f)
    got = launch_lists()
    assert set(got) == set(want) and len(want) == 21
    for call in want:
        assert got[call] == want[call], call
