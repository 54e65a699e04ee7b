"""The registration without a GPU: the new symbols, argument refusals before any native call (C ABI and Python), the host solves
of localrf_amd/alignment.py fed with the words of the numpy restatements (tests/align_cases.py), the overflow bounds of
csrc/lrf_align.inl, and the kernels' scratch use.

Measured with the committed restatements: fit_pairs' solve recovers (0.4 rad about (1, 2, 3), s = 1.07, t = (0.3, -0.2, 0.5))
from the 1500 blob points to 3.8e-8 (bar 1e-6); the plane solve iterated with the brute-force closest point reaches 1.8e-9 ..
1.4e-8 within 5 or 6 iterations on the eight blob runs (bar 1e-5, the GPU test's)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from align_cases import (ICP_BAR, ICP_RUNS, PERTURBATIONS, apply, blob, blob_points, deviation, icp_plane_host, pair_inputs, pairs_host,
                         parts, sim, source_cloud, truth, umeyama_host)
from localrf_amd import NativeError, alignment
from mesh_util import cpu_mesh, forbid_native

SYMBOLS = ("lrf_align_transform", "lrf_align_pairs", "lrf_align_plane")
KERNELS = ("k_al_transform", "k_al_pairs", "k_al_plane")
T_FIT = sim(0.4, 1.07, 0.0, axis=(1.0, 2.0, 3.0), t=(0.3, -0.2, 0.5))


def test_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfAlignFrame" in header and C.sizeof(N.LrfAlignFrame) == 4 * 8
    assert "typedef struct LrfAlignPlane" in header and C.sizeof(N.LrfAlignPlane) == 6 * 8 + 3 * 8 + 4 * 8 + 2 * 4
    assert built_lib.lrf_abi_version() == 7
    import __graft_entry__ as ge
    import localrf_amd
    assert "lrf_align.inl" in ge.HEADERS and "alignment" in localrf_amd.__all__ and "alignment." in localrf_amd.__doc__

    def transform(T=tuple(range(12)), points=FAKE, n=5, out=FAKE):
        arr = (C.c_double * 12)(*T) if T is not None else None
        return refused(built_lib, built_lib.lrf_align_transform(arr, points, n, out, None), "lrf_align_transform")
    assert "0 <= N" in transform(n=-1) and "0 <= N" in transform(n=1 << 31)
    for bad in (dict(T=None), dict(points=None), dict(out=None)):
        assert transform(**bad).endswith(": null argument"), bad
    assert "4-byte aligned" in transform(points=FAKE + 2) and "4-byte aligned" in transform(out=FAKE + 1)
    for bad in (math.nan, math.inf):
        assert "finite" in transform(T=(1.0,) * 11 + (bad,))

    def frame(**over):
        return filled(N.LrfAlignFrame, dict(c=(0.0, 0.0, 0.0), h=0.5), **over)

    def pairs(fr=True, a=FAKE, b=FAKE, keep=None, n=9, words=FAKE, **over):
        return refused(built_lib, built_lib.lrf_align_pairs(C.byref(frame(**over)) if fr else None, a, b, keep, n, words, None), "lrf_align_pairs")
    for bad in (dict(fr=False), dict(a=None), dict(b=None), dict(words=None)):
        assert pairs(**bad).endswith(": null argument"), bad
    assert "N <= 2^20" in pairs(n=-1) and "N <= 2^20" in pairs(n=(1 << 20) + 1)
    for bad in (0.0, -0.5, 0.75, 3.0, math.nan, math.inf):
        assert "power of two" in pairs(h=bad), bad
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        assert "c must be finite" in pairs(c=bad), bad
    assert "4-byte aligned" in pairs(a=FAKE + 2) and "4-byte aligned" in pairs(b=FAKE + 1) and "8-byte aligned" in pairs(words=FAKE + 4)

    def plane(p=True, words=FAKE, **over):
        a = filled(N.LrfAlignPlane, dict(vertices=FAKE, faces=FAKE, points=FAKE, closest=FAKE, face=FAKE, distance=FAKE, Nv=5, Nf=3, N=9,
                                         u=2.0, gate=math.inf), **over)
        return refused(built_lib, built_lib.lrf_align_plane(C.byref(a) if p else None, words, None), "lrf_align_plane")
    for bad in (dict(p=False), dict(words=None), dict(vertices=None), dict(faces=None), dict(points=None), dict(closest=None),
                dict(face=None), dict(distance=None)):
        assert plane(**bad).endswith(": null argument"), bad
    for bad in (dict(Nv=0), dict(Nv=1 << 31), dict(Nf=-1), dict(Nf=1 << 31)):
        assert "need 1 <= Nv" in plane(**bad), bad
    assert "Nf >= 1" in plane(Nf=0)
    assert "N <= 2^20" in plane(N=-1) and "N <= 2^20" in plane(N=(1 << 20) + 1)
    for bad in (0.0, -2.0, 1.5, math.nan, math.inf):
        assert "power of two" in plane(u=bad), bad
    assert "c must be finite" in plane(c=(0.0, math.nan, 0.0)) and "c must be finite" in plane(c=(math.inf, 0.0, 0.0))
    assert "gate" in plane(gate=-1.0) and "gate" in plane(gate=math.nan)
    for bad in (dict(vertices=FAKE + 2), dict(faces=FAKE + 1), dict(points=FAKE + 2), dict(closest=FAKE + 1), dict(face=FAKE + 3),
                dict(distance=FAKE + 2)):
        assert "4-byte aligned" in plane(**bad), bad
    assert "8-byte aligned" in plane(words=FAKE + 4)


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    eye, pts, mesh = np.eye(4), torch.zeros(8, 3), cpu_mesh(rgb=False)
    shear = np.eye(4)
    shear[0, 1] = 0.5
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    for bad in (0, -1.0, math.nan, True):
        with pytest.raises(ValueError, match="scale"):
            alignment.similarity(bad, np.eye(3), (0, 0, 0))
    with pytest.raises(ValueError, match="rotation"):
        alignment.similarity(1.0, mirror[:3, :3], (0, 0, 0))
    with pytest.raises(ValueError, match="translation"):
        alignment.similarity(1.0, np.eye(3), (0, math.inf, 0))
    for bad in (shear, mirror, np.zeros((4, 4)), np.eye(3), np.diag([1.0, 1.0, 1.0, 2.0]), "T"):
        for call in (alignment.decompose, alignment.inverse, lambda T: alignment.icp(pts, mesh, init=T), lambda T: alignment.transform_mesh(mesh, T)):
            with pytest.raises(ValueError, match="T"):
                call(bad)
    with pytest.raises(ValueError, match="T2"):
        alignment.compose(np.eye(3), eye)
    with pytest.raises(ValueError, match="T1"):
        alignment.compose(eye, np.full((4, 4), math.nan))
    with pytest.raises(TypeError, match="points"):
        alignment.transform_points(np.zeros((3, 3), np.float32), eye)
    with pytest.raises(ValueError, match="points"):
        alignment.transform_points(torch.zeros(3, 3, dtype=torch.float64), eye)
    with pytest.raises(ValueError, match="T"):
        alignment.transform_points(pts, np.eye(3))
    with pytest.raises(TypeError, match="mesh"):
        alignment.transform_mesh([pts], eye)
    with pytest.raises(ValueError, match="normals"):
        alignment.transform_mesh(dict(mesh, normals=torch.zeros(3, 3)), eye)
    with pytest.raises(ValueError, match="same number"):
        alignment.fit_pairs(pts, torch.zeros(7, 3))
    with pytest.raises(ValueError, match="points"):
        alignment.fit_pairs(pts, torch.zeros(8, 2))
    with pytest.raises(ValueError, match="keep"):
        alignment.fit_pairs(pts, pts, keep=torch.zeros(8))
    with pytest.raises(TypeError, match="keep"):
        alignment.fit_pairs(pts, pts, keep=[1] * 8)
    with pytest.raises(ValueError, match="scale"):
        alignment.fit_pairs(pts, pts, scale=1)
    with pytest.raises(TypeError, match="poses_est"):
        alignment.trajectory_error(np.zeros((4, 3, 4)), torch.zeros(4, 3, 4))
    with pytest.raises(ValueError, match="poses_gt"):
        alignment.trajectory_error(torch.zeros(4, 3, 4), torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match="4 estimated poses"):
        alignment.trajectory_error(torch.zeros(4, 3, 4), torch.zeros(5, 3, 4))
    with pytest.raises(ValueError, match="scale"):
        alignment.trajectory_error(torch.zeros(4, 3, 4), torch.zeros(4, 3, 4), scale="yes")
    for name, bad in (("metric", "planes"), ("iterations", 0), ("iterations", 2.5), ("max_distance", -1.0), ("max_distance", math.nan),
                      ("tol", -1e-3), ("tol", math.nan), ("scale", 0)):
        with pytest.raises(ValueError, match=name):
            alignment.icp(pts, mesh, **{name: bad})
        with pytest.raises(ValueError, match=name):
            alignment.align_meshes(mesh, mesh, 0.1, **{name: bad})
    with pytest.raises(ValueError, match="points"):
        alignment.icp(torch.zeros(8, 2), mesh)
    with pytest.raises(TypeError, match="mesh_or_index"):
        alignment.icp(pts, None)
    for bad in (0, -0.1, math.inf, "a"):
        with pytest.raises(ValueError, match="spacing"):
            alignment.align_meshes(mesh, mesh, bad)
    with pytest.raises(TypeError, match="unexpected"):
        alignment.align_meshes(mesh, mesh, 0.1, cell=0.5)
    with pytest.raises(TypeError, match="b must be"):
        alignment.align_meshes(mesh, None, 0.1)
    poses = torch.zeros(4, 3, 4)
    for call in (lambda: alignment.transform_points(pts, eye), lambda: alignment.transform_mesh(mesh, eye), lambda: alignment.fit_pairs(pts, pts),
                 lambda: alignment.fit_pairs(pts, pts, keep=torch.ones(8, dtype=torch.bool), scale=False),
                 lambda: alignment.trajectory_error(poses, poses), lambda: alignment.icp(pts, mesh), lambda: alignment.icp(pts, mesh, metric="point"),
                 lambda: alignment.align_meshes(mesh, mesh, 0.1)):
        with pytest.raises(NativeError):                                        # accepted arguments on the CPU: no fallback
            call()


def test_compose_inverse_and_decompose_round_trip():
    rng = np.random.default_rng(5)
    for _ in range(20):
        T = sim(rng.uniform(0, 3), rng.uniform(0.2, 5), 0.0, axis=rng.standard_normal(3), t=rng.standard_normal(3))
        s, R, t = alignment.decompose(T)
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
        assert np.abs(alignment.similarity(s, R, t) - T).max() < 1e-12
        assert np.abs(alignment.compose(alignment.inverse(T), T) - np.eye(4)).max() < 1e-12
        assert np.abs(alignment.compose(T, alignment.inverse(T)) - np.eye(4)).max() < 1e-12
        T2 = sim(rng.uniform(0, 3), rng.uniform(0.5, 2), 0.0, axis=rng.standard_normal(3), t=rng.standard_normal(3))
        p = rng.standard_normal((5, 3))
        assert np.abs(apply(alignment.compose(T2, T), p) - apply(T2, apply(T, p))).max() < 1e-12
        assert np.array_equal(alignment.compose(T2, T)[3], (0, 0, 0, 1))
        s12 = alignment.decompose(alignment.compose(T2, T))[0]
        assert abs(s12 - alignment.decompose(T2)[0] * s) < 1e-12 * s12
    assert alignment.pair_frame((-1.0, 0.0, 0.0), (1.0, 0.5, 0.25)) == ((0.0, 0.25, 0.125), 2.0 ** -19)
    c, h = alignment.pair_frame((0.0,) * 3, (2.0 ** 21 - 4,) * 3)               # half_extent / h = 2^20 - 2 exactly: h stays 1
    assert h == 1.0 and alignment.pair_frame((0.0,) * 3, (2.0 ** 21 - 3,) * 3)[1] == 2.0


def _fit_words(a, b, keep=None):
    both = np.concatenate([a, b])
    c, h = alignment.pair_frame(both.min(0), both.max(0))
    return pairs_host(c, h, a, b, keep), c, h


def test_the_pair_solve_recovers_a_known_similarity():
    a = blob_points().astype(np.float32)
    b = apply(T_FIT, a.astype(np.float64)).astype(np.float32)
    w, c, h = _fit_words(a, b)
    fit = alignment.solve_pairs(w, c, h, True)
    print(f"fit_pairs' solve: deviation {deviation(fit['T'], T_FIT):.3e} (bar 1e-6), rms {fit['rms']:.3e}, h {h:.3e}")
    assert deviation(fit["T"], T_FIT) <= 1e-6 and fit["count"] == 1500 and abs(fit["scale"] - 1.07) <= 1e-6
    assert fit["out_of_range"] == fit["masked"] == fit["nonfinite"] == 0 and fit["rms"] < 2 * h
    assert deviation(fit["T"], umeyama_host(a, b)) <= 1e-6
    rigid = alignment.solve_pairs(w, c, h, False)
    assert rigid["scale"] == 1.0 and alignment.decompose(rigid["T"])[0] == pytest.approx(1.0, abs=1e-15)
    assert deviation(rigid["T"], umeyama_host(a, b, scale=False)) <= 1e-6 and rigid["rms"] > 100 * fit["rms"]
    assert abs(alignment.pairs_rms(w, h) - np.sqrt(((a.astype(np.float64) - b) ** 2).sum(1).mean())) < 1e-6


def test_a_mirrored_target_still_gives_a_proper_rotation():
    a = blob_points().astype(np.float32)
    b = (apply(T_FIT, a.astype(np.float64)) * (1.0, 1.0, -1.0)).astype(np.float32)
    w, c, h = _fit_words(a, b)
    for free in (True, False):
        fit = alignment.solve_pairs(w, c, h, free)
        s, R, _ = parts(fit["T"])
        assert abs(np.linalg.det(R) - 1) < 1e-12 and s > 0
        assert deviation(fit["T"], umeyama_host(a, b, scale=free)) <= 1e-6
        alignment.decompose(fit["T"])


def test_the_pair_solve_refuses_too_few_pairs_and_rank_below_two():
    a, b, keep, c, h = pair_inputs(3, 65)
    assert pairs_host(c, h, a, b, keep)[1] > 0 and pairs_host(c, h, a, b, keep)[3] > 0
    alignment.solve_pairs(pairs_host(c, h, a, b, keep), c, h)
    with pytest.raises(ValueError, match="at least 3"):
        alignment.solve_pairs(pairs_host(c, h, a[:2], b[:2]), c, h)
    line = (np.linspace(-1, 1, 50)[:, None] * np.array((1.0, 2.0, -0.5))).astype(np.float32)
    w, c, h = _fit_words(line, line)
    with pytest.raises(ValueError, match="rank below 2"):
        alignment.solve_pairs(w, c, h)
    same = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="rank below 2"):
        alignment.solve_pairs(pairs_host((0, 0, 0), 1.0, same, same), (0, 0, 0), 1.0)


@pytest.mark.parametrize("k,free", ICP_RUNS)
def test_the_plane_solve_iterated_with_a_brute_force_closest_point(k, free):
    """alignment.solve_plane, plane_update and compose over the restated words: within ICP_BAR of the truth in scale, every
    rotation entry and every translation component after at most 10 iterations, converged by the step."""
    want = truth(k, free)
    T, steps = icp_plane_host(source_cloud(want), blob(), free, PERTURBATIONS[k][3])
    print(f"perturbation {k}, scale {'free' if free else 'fixed'}: deviation {deviation(T, want):.3e} after {len(steps)} iterations, steps {steps}")
    assert deviation(T, want) <= ICP_BAR and steps[-1] < 1e-7 and len(steps) <= 10


def test_the_plane_solve_reports_what_it_cannot_determine():
    w = [0] * 48
    w[0] = 6
    assert alignment.solve_plane(w)["omega"] is None
    w[0] = 100
    sol = alignment.solve_plane(w)                                              # a zero matrix
    assert sol["omega"] is None and sol["cond"] > 1e12
    for k in (0, 3, 6):                                                         # only three of seven directions are seen
        w[14 + 7 * k - k * (k - 1) // 2] = 1 << 40
    assert alignment.solve_plane(w)["omega"] is None and alignment.solve_plane(w, scale=False)["omega"] is None


def test_the_sums_cannot_overflow():
    top = (1 << 20) - 1
    assert (1 << 20) * top * top < 1 << 63 and (1 << 20) * 3 * top * top < 1 << 63
    j = 3 + math.sqrt(3)
    assert (1 << 20) * (j * j * 2.0 ** 36 + 1) < 2.0 ** 61 and alignment.PLANE_SCALE == 1 << 36 and alignment.PAIRS_PER_CALL == 1 << 20
    edge = np.float32(top * 0.5)
    a = np.full((4, 3), edge, np.float32)
    w = pairs_host((0, 0, 0), 0.5, a, -a)
    assert w[0] == 4 and w[19] == 4 * 3 * top * top and w[10] == -4 * top * top


def test_align_kernels_use_no_scratch():
    """The kernels of lrf_align.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
