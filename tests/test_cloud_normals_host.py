"""Point-cloud normals and the plane step against a cloud without a GPU: the Jacobi restatement of tests/cloud_normal_cases.py
against np.linalg.eigh on every case, the sweep constant, the properties the cases were made for, the accuracy on a sphere, the
host registration loop, argument refusals before any native call (Python and C ABI), the new symbols and struct size, and the
new kernels' scratch use."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from align_cases import deviation, truth
from cloud_normal_cases import (CASE_NAMES, EPS, SCAN_RUNS, SWEEPS, cases, expected, fibonacci, icp_plane_cloud_host, jacobi_host, lattice_h,
                                normals_host, plane_cloud_case, plane_cloud_host, scan, scan_normals, scan_source, scan_spacing, sphere_spacing)
from localrf_amd import NativeError, alignment, cloud
from localrf_amd.cloud import CloudIndex, estimate_normals
from mesh_util import cpu_mesh, forbid_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lrf_cloud_normals", "lrf_align_plane_cloud")
KERNELS = ("k_cl_normalsILb0E", "k_cl_normalsILb1E", "k_cl_normals_rest", "k_al_plane_cloud", "k_al_planeE")
SWEEPS_MEASURED = 4                                                 # the most any case needs; the constant is this plus 2


def _rows(name):
    e = expected(name)
    return [(i, e["cov"][i], e["lattice"][i], e["needed"][i]) for i in range(len(e["cov"])) if e["cov"][i] is not None]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_jacobi_restatement_agrees_with_eigh_and_the_sweeps_suffice(name):
    """Eigenvalues within 1e-12 trace of np.linalg.eigh's; the normal within 1e-9 of its eigenvector up to sign where the two
    smallest eigenvalues differ by more than 1e-6 trace; after SWEEPS sweeps every off-diagonal entry is 0 or below 2^-52
    trace, and no case needs more than SWEEPS - 2."""
    most = 0
    for i, cov, (lam, col), needed in _rows(name):
        A = np.array([[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]])
        trace = (cov[0] + cov[3]) + cov[5]
        w, v = np.linalg.eigh(A)
        assert np.abs(np.array(lam) - w).max() <= 1e-12 * trace, (name, i)
        if w[1] - w[0] > 1e-6 * trace:
            n = np.array(col)
            assert min(np.abs(n - v[:, 0]).max(), np.abs(n + v[:, 0]).max()) <= 1e-9, (name, i)
        off = []
        jacobi_host(cov, SWEEPS, off)
        assert off[-1] == 0.0 or off[-1] < EPS * trace, (name, i, off)
        most = max(most, needed)
    assert most <= SWEEPS_MEASURED == SWEEPS - 2
    src = open(os.path.join(ROOT, "localrf_amd", "csrc", "lrf_cloud.inl")).read()
    assert f"constexpr int CL_JACOBI_SWEEPS = {SWEEPS};" in src


def test_some_case_needs_the_measured_sweeps():
    assert max(max(expected(name)["needed"], default=0) for name in CASE_NAMES) == SWEEPS_MEASURED == max(scan_normals()["needed"])


def test_the_cases_cover_what_they_should():
    cs = cases()
    assert {c["cloud"].shape[0] for c in cs.values()} >= {0, 1, 2, 3, 64, 65, 4099}
    e = expected("planar lattice")
    assert (e["normals"] == np.array([0, 0, 1], np.float32)).all() and (e["eigenvalues"][:, 0] == 0).all() and (e["eigenvalues"][:, 1] > 0).all()
    assert e["count"].min() == 8 and e["count"].max() == 21 and (e["count"] == 8).sum() == 4
    at, above = expected("planar lattice, min_neighbours at a corner's 8"), expected("planar lattice, min_neighbours above a corner's 8")
    assert np.array_equal(at["normals"], e["normals"]) and ((above["normals"] == 0).all(1) == (e["count"] == 8)).all()
    assert np.array_equal(above["eigenvalues"], e["eigenvalues"]) and np.array_equal(above["count"], e["count"])
    assert (expected("planar lattice, viewpoint below")["normals"] == np.array([0, 0, -1], np.float32)).all()
    assert np.array_equal(expected("planar lattice, viewpoint in the plane")["normals"], e["normals"])         # a dot of exactly 0
    line = expected("line")
    assert (line["eigenvalues"][:, :2] == 0).all() and (line["eigenvalues"][:, 2] > 0).all() and (line["count"] >= 3).all()
    assert (np.abs(line["normals"]).sum(1) == 1).all() and (line["normals"][:, 0] == 0).all()
    same = expected("70 identical points")
    assert (same["normals"] == 0).all() and (same["eigenvalues"] == 0).all() and set(same["count"].tolist()) <= {0, 70} and (same["count"][:3] == 70).all()
    p = expected("planted distance")
    assert cs["planted distance"]["radius"] == 1.25 and p["count"].tolist() == [1, 0, 1, 1, 1, 0] and (p["normals"] == 0).all()
    bad = expected("cloud entries that are not finite")
    assert (bad["count"] == -1).sum() == 6 and np.isnan(bad["normals"][bad["count"] == -1]).all() and np.isnan(bad["eigenvalues"][bad["count"] == -1]).all()
    assert np.isfinite(bad["normals"][bad["count"] >= 0]).all()
    q = expected("queries that are not finite")
    assert (q["count"] == -1).sum() == 4 and np.isnan(q["normals"]).all(1).sum() == 4
    big = expected("coordinates near 1e30")
    assert (big["count"] >= 6).all() and np.isfinite(big["normals"]).all() and (np.abs(np.linalg.norm(big["normals"].astype(np.float64), axis=1) - 1) < 1e-6).all()
    none = expected("no finite point")
    assert set(none["count"].tolist()) == {0, -1}
    s = cs["sphere, viewpoint inside"]["cloud"].astype(np.float64)
    inward, outward = expected("sphere, viewpoint inside"), expected("sphere, viewpoints outside")
    assert ((inward["normals"] * s).sum(1) < -0.99).all() and ((outward["normals"] * s).sum(1) > 0.99).all()
    assert np.array_equal(inward["normals"], -outward["normals"]) and np.array_equal(inward["eigenvalues"], outward["eigenvalues"])
    off = expected("sphere, queries off the cloud")
    assert (off["count"] >= 6).all() and not (off["normals"] == 0).all(1).any()
    for name in CASE_NAMES:                                                          # a unit normal or none
        n = expected(name)["normals"].astype(np.float64)
        length = np.linalg.norm(n[np.isfinite(n).all(1)], axis=1)
        assert ((length == 0) | (np.abs(length - 1) < 1e-6)).all(), name
    assert lattice_h(0.3) == 2.0 ** -16 == lattice_h(0.5) and lattice_h(0.5000001) == 2.0 ** -15 and lattice_h(1.25) == 2.0 ** -14
    for r in (0.3, 0.5, 1.25, 1.2e30, 3e-5):
        assert r / lattice_h(r) <= 2 ** 15 < r / (lattice_h(r) / 2) and lattice_h(r) == cloud.normal_lattice(r)


def test_the_sums_cannot_overflow():
    top = 1 << 15
    assert ((1 << 31) - 1) * top * top < 1 << 61 and cloud.NORMAL_LATTICE == top
    assert (1 << 23) * top * top == 1 << 53                                          # below 2^23 neighbours every conversion is exact


@pytest.mark.parametrize("spacings,bar", ((3.0, 2.0),))
def test_normals_of_a_sphere_are_radial(spacings, bar):
    """4099 Fibonacci points on the unit sphere at a radius of 3 spacings (sqrt(4 pi / N)): the largest angle between a normal
    and the radial direction is at most 2 degrees (measured: 0.94)."""
    d = fibonacci()
    e = expected("sphere, viewpoint inside")
    assert cases()["sphere, viewpoint inside"]["radius"] == spacings * sphere_spacing()
    n = e["normals"].astype(np.float64)
    cos = np.abs((n * d).sum(1)) / np.linalg.norm(n, axis=1)
    angle = float(np.degrees(np.arccos(np.clip(cos, -1, 1))).max())
    print(f"largest angle to the radial direction at {spacings} spacings: {angle:.3f} degrees, neighbours {e['count'].min()} .. {e['count'].max()}")
    assert angle <= bar


def test_the_plane_cloud_case_hits_every_counter():
    B, normals, cloud_, c, u, max_distance, gate, near = plane_cloud_case()
    w = plane_cloud_host(cloud_, near["closest"], near["index"], near["distance"], normals, c, u, np.float32(gate))
    print("plane-cloud words 0..4 (summed, unmatched, gated, degenerate, out of range):", w[:5])
    assert min(w[:5]) > 0 and w[1] == 2 and w[3] >= 2 and sum(w[:5]) == cloud_.shape[0] and w[5] == 0 and w[42:] == [0] * 6
    assert (normals == 0).all(1).sum() == 1 and np.isnan(normals).any(1).sum() == 1
    perm = np.random.default_rng(3).permutation(cloud_.shape[0])
    assert plane_cloud_host(cloud_[perm], near["closest"][perm], near["index"][perm], near["distance"][perm], normals, c, u, np.float32(gate)) == w
    j = 3 + math.sqrt(3)
    assert (1 << 20) * (j * j * 2.0 ** 36 + 1) < 2.0 ** 61                           # item 3's bound, which item 4 inherits


@pytest.mark.parametrize("k,free", SCAN_RUNS)
def test_the_host_loop_registers_a_cloud_onto_a_scan(k, free):
    """alignment.solve_plane, plane_update and compose over the restated words of the plane step against a cloud, with the
    restated normals at 4 median spacings: below 1e-3 from the truth, converged by the step within 20 iterations.  Measured:
    2.8e-4 .. 3.4e-4 with a free scale, 4.8e-5 .. 5.0e-5 rigid, 5 to 7 steps."""
    nrm = scan_normals()
    assert abs(scan_spacing() - 0.0510) < 5e-4 and nrm["count"].min() >= 29 and not (nrm["normals"] == 0).all(1).any()
    T, steps = icp_plane_cloud_host(scan_source(k, free), scan(), nrm["normals"], free)
    print(f"perturbation {k}, scale {'free' if free else 'fixed'}: deviation {deviation(T, truth(k, free)):.3e} after {len(steps)} iterations, steps {steps}")
    assert deviation(T, truth(k, free)) < 1e-3 and steps[-1] < 1e-7 and len(steps) <= 20


class _StubIndex(CloudIndex):
    """A CloudIndex without a device: the checks that come before the device check."""
    def __init__(self, m=8):
        self.points, self.device, self.counts, self._grid = torch.zeros(m, 3), torch.device("cpu"), (m,), None
        self.info = {"cell": None, "box": None, "dims": (0, 0, 0), "points": 0, "nonfinite_points": 0}


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    index, pts = _StubIndex(), torch.zeros(8, 3)
    for call in (lambda **k: index.normals(pts, **k), lambda **k: estimate_normals(index, **k), lambda **k: estimate_normals(pts, **k)):
        for bad in (0, 0.0, -1.0, math.nan, math.inf, True, "r", None, 1e-320):
            with pytest.raises(ValueError, match="radius"):
                call(radius=bad)
        for bad in (2, 0, -1, 6.5, True, None, 1 << 31):
            with pytest.raises(ValueError, match="min_neighbours"):
                call(radius=0.1, min_neighbours=bad)
        for bad in ((0.0, 1.0), (0.0, math.nan, 0.0), "abc", torch.zeros(7, 3), torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 2), 1.0):
            with pytest.raises(ValueError, match="viewpoint"):
                call(radius=0.1, viewpoint=bad)
        for good in (dict(radius=0.1), dict(radius=0.1, min_neighbours=3, viewpoint=(0.0, 1.0, 2.0)), dict(radius=2.5, viewpoint=torch.zeros(8, 3)),
                     dict(radius=0.1, viewpoint=torch.zeros(3))):
            with pytest.raises(NativeError):                                    # accepted arguments on the CPU: no fallback
                call(**good)
    for bad in (torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64)):
        for call in (lambda: index.normals(bad, 0.1), lambda: estimate_normals(bad, 0.1)):
            with pytest.raises(ValueError, match=r"points must be \[N, 3\] float32"):
                call()
    with pytest.raises(TypeError, match="CloudIndex"):
        estimate_normals([pts], 0.1)
    for bad in ("cells", None, 1):
        with pytest.raises(ValueError, match="order"):
            estimate_normals(index, 0.1, order=bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match="max_bytes"):
            estimate_normals(pts, 0.1, max_bytes=bad)
    with pytest.raises(NativeError):
        estimate_normals(index, 0.1, order="records")


def test_icp_refusals_with_and_without_target_normals(monkeypatch):
    forbid_native(monkeypatch)
    index, pts, nrm = _StubIndex(), torch.zeros(8, 3), torch.zeros(8, 3)
    for kwargs in (dict(), dict(metric="plane"), dict(target_normals=None)):         # the old refusal, word for word
        with pytest.raises(ValueError, match='^a cloud has no planes: metric="plane" needs a mesh or a MeshIndex as the target; '
                                             'pass metric="point" to align against a CloudIndex$'):
            alignment.icp(pts, index, **kwargs)
    with pytest.raises(ValueError, match="iterations"):                             # the other checks come first
        alignment.icp(pts, index, iterations=0, target_normals=torch.zeros(7, 3))
    with pytest.raises(ValueError, match="points"):
        alignment.icp(torch.zeros(8, 2), index, target_normals=nrm)
    for bad in (torch.zeros(7, 3), torch.zeros(8, 2), torch.zeros(8, 3, dtype=torch.float64), torch.zeros(24), np.zeros((8, 3), np.float32), [0.0] * 24,
                torch.zeros(8, 3, device="meta")):
        with pytest.raises(ValueError, match="target_normals"):
            alignment.icp(pts, index, target_normals=bad)
    with pytest.raises(ValueError, match='target_normals.*metric="point" takes none'):
        alignment.icp(pts, index, metric="point", target_normals=nrm)
    for mesh in (cpu_mesh(rgb=False),):
        with pytest.raises(ValueError, match="target_normals go with a CloudIndex"):
            alignment.icp(pts, mesh, target_normals=nrm)
        with pytest.raises(ValueError, match="target_normals go with a CloudIndex"):
            alignment.icp(pts, mesh, metric="point", target_normals=nrm)
    with pytest.raises(NativeError):                                                # accepted: the device check is next
        alignment.icp(pts, index, target_normals=nrm)
    with pytest.raises(NativeError):
        alignment.icp(pts, index, metric="plane", scale=False, target_normals=nrm, iterations=3)


def test_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    import localrf_amd
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfAlignPlaneCloud" in header and C.sizeof(N.LrfAlignPlaneCloud) == 5 * 8 + 2 * 8 + 4 * 8 + 2 * 4
    assert built_lib.lrf_abi_version() == 7
    assert "estimate_normals" in localrf_amd.__doc__ and callable(cloud.estimate_normals) and callable(CloudIndex.normals)

    def index(**over):
        return filled(N.LrfCloudIndex, dict(points=FAKE, grid=FAKE, records=FAKE, M=9, entries=7, cell=0.5, lo=(0.0,) * 3, dims=(4,) * 3), **over)

    def normals(a=True, points=FAKE, n=9, radius=0.3, h=2.0 ** -16, least=6, view=None, stride=0, normal=FAKE, eig=FAKE, count=FAKE, **over):
        return refused(built_lib, built_lib.lrf_cloud_normals(C.byref(index(**over)) if a else None, points, n, radius, h, least, view, stride, normal, eig, count, None),
                       "lrf_cloud_normals")
    assert normals(a=False).endswith(": null argument") and "1 <= M" in normals(M=0) and "entries <= M" in normals(entries=10)
    assert "records of a built index" in normals(records=None) and "16-byte aligned" in normals(records=FAKE + 8) and normals(grid=None).endswith(": null argument")
    assert "0 <= N < 2^31" in normals(n=-1) and "0 <= N < 2^31" in normals(n=1 << 31)
    for bad in (0.0, -0.3, math.nan, math.inf):
        assert "radius must be finite and > 0" in normals(radius=bad), bad
    for bad in (0.0, -2.0 ** -16, 3e-5, math.nan, math.inf):
        assert "h must be a positive power of two" in normals(h=bad), bad
    for bad in (2.0 ** -17, 2.0 ** -15, 1.0):
        assert "the smallest power of two with radius / h <= 2^15" in normals(h=bad), bad
    assert "smallest power of two" in normals(radius=0.5, h=2.0 ** -15) and "smallest power of two" in normals(radius=0.5000001, h=2.0 ** -16)
    for bad in (2, 0, -1):
        assert "min_neighbours must be >= 3" in normals(least=bad), bad
    for bad in (1, 2, 4, -3, 12):
        assert "viewpoint_stride must be 0" in normals(view=FAKE, stride=bad), bad
    for bad in (dict(normal=None), dict(eig=None), dict(count=None)):
        assert normals(**bad).endswith(": null argument"), bad
    for bad in (dict(points=FAKE + 2), dict(view=FAKE + 1), dict(normal=FAKE + 2), dict(eig=FAKE + 3), dict(count=FAKE + 1)):
        assert "4-byte aligned" in normals(**bad), bad
    assert "need N == M" in normals(points=None, n=8) and "need N == M" in normals(points=None, n=0)

    def plane(p=True, words=FAKE, **over):
        a = filled(N.LrfAlignPlaneCloud, dict(points=FAKE, closest=FAKE, index=FAKE, distance=FAKE, normals=FAKE, N=9, M=5, u=2.0, gate=math.inf),
                   **over)
        return refused(built_lib, built_lib.lrf_align_plane_cloud(C.byref(a) if p else None, words, None), "lrf_align_plane_cloud")
    for bad in (dict(p=False), dict(words=None), dict(points=None), dict(closest=None), dict(index=None), dict(distance=None), dict(normals=None),
                dict(normals=None, N=0)):
        assert plane(**bad).endswith(": null argument"), bad
    for bad in (0, -1, 1 << 31):
        assert "need 1 <= M < 2^31" in plane(M=bad), bad
    assert "N <= 2^20" in plane(N=-1) and "N <= 2^20" in plane(N=(1 << 20) + 1)
    for bad in (0.0, -2.0, 1.5, math.nan, math.inf):
        assert "power of two" in plane(u=bad), bad
    assert "c must be finite" in plane(c=(0.0, math.nan, 0.0)) and "c must be finite" in plane(c=(math.inf, 0.0, 0.0))
    assert "gate" in plane(gate=-1.0) and "gate" in plane(gate=math.nan)
    for bad in (dict(points=FAKE + 2), dict(closest=FAKE + 1), dict(index=FAKE + 3), dict(distance=FAKE + 2), dict(normals=FAKE + 1)):
        assert "4-byte aligned" in plane(**bad), bad
    assert "8-byte aligned" in plane(words=FAKE + 4)


def test_the_new_kernels_use_no_scratch():
    """The new kernels, and k_al_plane beside its twin, as __graft_entry__.build() compiles them: the metadata only.  The ten
    sums, A and V of k_cl_normals must stay registers, and so must the 42 sums of k_al_plane_cloud."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="prefix")
