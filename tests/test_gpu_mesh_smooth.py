"""Mesh topology, vertex normals and Taubin smoothing on the MI355X (csrc/lrf_mesh_smooth.inl through localrf_amd.mesh):
every case of tests/mesh_smooth_cases.py against the numpy restatement -- counts, masks, the normals' integer sums and
smoothed vertices bit for bit, unit normals within one fp32 ulp --, reproducibility, a non-default stream, refusals, the
row-length limit, and the extract options."""
import functools

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, _native, mesh, novel_views, pointcloud
from localrf_amd.mesh import smooth, topology, vertex_normals  # noqa: F401  (what every test here is about)
from mesh_cases import H_ANALYTIC
from mesh_clean_cases import fan
from mesh_smooth_cases import (CASE_NAMES, cases, expected_normals, expected_smooth, expected_topology, smooth_arguments)
from mesh_util import DEV, bits, blob_volumes, device_mesh, same_device_mesh, to_dev
from novel_views_cases import scene

pytestmark = pytest.mark.gpu
COUNTS = ("boundary_edges", "nonmanifold_edges", "degenerate_faces")


@functools.lru_cache(maxsize=None)
def _case_mesh(name):
    return device_mesh(cases()[name], note="kept")


def _ordered(a):
    """fp32 -> int64 that orders as the floats do, -0 as +0: one step is one ulp."""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _debug_normals(dm):
    """lrf_debug_mesh_vertex_normals -> (S [Nv,3] int64, E, normals [Nv,3] fp32, info words), on the host."""
    nv, nf = dm["counts"]
    n = torch.empty(nv, 3, dtype=torch.float32, device=DEV)
    S = torch.empty(nv, 3, dtype=torch.int64, device=DEV)
    E = torch.empty(1, dtype=torch.int32, device=DEV)
    info = torch.empty(8, dtype=torch.int64, device=DEV)
    ws = _native.workspace("lrf_mesh_incidence", torch.device(DEV), nv, nf)
    _native.launch("lrf_debug_mesh_vertex_normals", torch.device(DEV), dm["vertices"].data_ptr(), dm["faces"].data_ptr() if nf else None,
                   nv, nf, n.data_ptr(), S.data_ptr(), E.data_ptr(), info.data_ptr(), ws.data_ptr(), guard=True)
    words = info.tolist()
    return S.cpu().numpy(), int(E.item()), n.cpu().numpy(), words


@pytest.mark.parametrize("name", CASE_NAMES)
def test_topology_equals_the_restatement(name):
    dm, want = _case_mesh(name), expected_topology(name)
    got = mesh.topology(dm)
    print(f"{name}: {dm['counts']} {[got[k] for k in COUNTS]} closed {got['closed']}")
    assert set(got) == set(COUNTS) | {"closed", "boundary_vertices"}
    for k in COUNTS:
        assert type(got[k]) is int and got[k] == want[k], k
    assert got["closed"] is want["closed"]
    mask = got["boundary_vertices"]
    assert mask.dtype is torch.uint8 and tuple(mask.shape) == (dm["counts"][0],)
    assert mask.cpu().numpy().tobytes() == want["boundary_vertices"].tobytes()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_vertex_normals_equal_the_restatement(name):
    dm, want = _case_mesh(name), expected_normals(name)
    S, E, debug_n, words = _debug_normals(dm)
    assert E == want["E"] and S.dtype == np.int64 and np.array_equal(S, want["S"])       # the integers: bit for bit
    got = mesh.vertex_normals(dm)
    n = got["normals"]
    assert n.dtype is torch.float32 and tuple(n.shape) == (dm["counts"][0], 3)
    assert got["normal_info"] == {"zero_normals": want["zero_normals"], "degenerate_faces": want["degenerate_faces"]}
    assert words[4] == want["zero_normals"] and words[1] == want["degenerate_faces"] and words[0] == 0
    assert np.array_equal(bits(n), debug_n.view(np.uint32))                              # both entry points, the same bytes
    steps = np.abs(_ordered(n.cpu().numpy()) - _ordered(want["normals"]))
    # one final rounding to fp32 of an fp64 quotient that may differ from numpy's in its last place: at most one step
    print(f"{name}: E {E}, components that differ from numpy at all: {int((steps > 0).sum())} of {steps.size}")
    assert steps.max(initial=0) <= 1
    assert set(got) == set(dm) | {"normals", "normal_info"} and got["note"] == "kept" and got["vertices"] is dm["vertices"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_smooth_equals_the_restatement_bit_for_bit(name):
    dm = _case_mesh(name)
    before = bits(dm["vertices"]).copy()
    for it, lam, mu, boundary in smooth_arguments(name):
        want_v, want_info = expected_smooth(name, it, lam, mu, boundary)
        got = mesh.smooth(dm, it, lam, mu, boundary)
        info = got["smooth"]
        assert info == dict(want_info, iterations=it, lam=lam, mu=mu, boundary=boundary), (it, lam, mu, boundary)
        assert all(type(info[k]) is int for k in COUNTS + ("pinned", "iterations"))
        assert got["vertices"].dtype is torch.float32 and tuple(got["vertices"].shape) == tuple(dm["vertices"].shape)
        assert np.array_equal(bits(got["vertices"]), want_v.view(np.uint32)), (it, lam, mu, boundary)
        assert got["faces"] is dm["faces"] and got["rgb8"] is dm["rgb8"] and got["note"] == "kept"
        assert got["vertices"].data_ptr() != dm["vertices"].data_ptr()
    assert np.array_equal(bits(dm["vertices"]), before)                                  # the input is left alone
    print(f"{name}: {dm['counts']} {len(smooth_arguments(name))} argument sets, pinned {info['pinned']}")


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    for name in ("blobs tie", "strip / vertices permuted", "fan 1025", "sphere noisy"):
        dm = _case_mesh(name)

        def run():
            t, n, s = mesh.topology(dm), mesh.vertex_normals(dm), mesh.smooth(dm, 3)
            return (t["boundary_vertices"].cpu().numpy().tobytes(), tuple(t[k] for k in COUNTS), bits(n["normals"]).tobytes(),
                    tuple(sorted(n["normal_info"].items())), bits(s["vertices"]).tobytes(), tuple(sorted(s["smooth"].items())))
        runs = [run(), run()]
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            runs.append(run())
        side.synchronize()
        assert runs[1] == runs[0] and runs[2] == runs[0]


def _all_right(name="blobs tie"):
    """The next valid call of each kind is right."""
    dm = _case_mesh(name)
    t, n, s = mesh.topology(dm), mesh.vertex_normals(dm), mesh.smooth(dm, 3)
    assert {k: t[k] for k in COUNTS} == {k: expected_topology(name)[k] for k in COUNTS}
    assert t["boundary_vertices"].cpu().numpy().tobytes() == expected_topology(name)["boundary_vertices"].tobytes()
    assert np.abs(_ordered(n["normals"].cpu().numpy()) - _ordered(expected_normals(name)["normals"])).max() <= 1
    assert np.array_equal(bits(s["vertices"]), expected_smooth(name, 3, 0.5, -0.53, "fixed")[0].view(np.uint32))


def test_bad_face_indices_raise_and_the_next_call_is_right():
    m = cases()["blobs tie"]
    nv, nf = m["vertices"].shape[0], m["faces"].shape[0]
    dm = _case_mesh("blobs tie")
    for bad in (nv, -1, (1 << 31) - 1, -(1 << 31)):
        for row, col in ((0, 0), (nf // 2, 1), (nf - 1, 2)):
            faces = m["faces"].copy()
            faces[row, col] = bad
            broken = dict(dm, faces=to_dev(faces))
            for fn in (mesh.topology, mesh.vertex_normals, mesh.smooth):
                with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                    fn(broken)
    _all_right()


def test_vertices_that_are_not_finite_raise_and_the_next_call_is_right():
    m = cases()["blobs tie"]
    nv = m["vertices"].shape[0]
    dm = _case_mesh("blobs tie")
    for bad in (np.nan, np.inf, -np.inf):
        for row, col in ((0, 0), (nv // 2, 1), (nv - 1, 2)):
            v = m["vertices"].copy()
            v[row, col] = bad
            broken = dict(dm, vertices=to_dev(v))
            for fn in (mesh.vertex_normals, mesh.smooth):
                with pytest.raises(ValueError, match="not finite"):
                    fn(broken)
    _all_right()


def test_cpu_tensors_raise_native_error():
    m = cases()["tetrahedron"]
    cpu = {"vertices": torch.from_numpy(m["vertices"]), "faces": torch.from_numpy(m["faces"]), "rgb8": None}
    for fn in (mesh.topology, mesh.vertex_normals, mesh.smooth):
        with pytest.raises(NativeError):
            fn(cpu)
        with pytest.raises(NativeError):
            fn(dict(_case_mesh("tetrahedron"), faces=cpu["faces"]))


def test_a_row_of_2_to_the_20_raises_and_one_entry_fewer_does_not():
    for nv, ok in (((1 << 20) + 1, True), ((1 << 20) + 2, False)):      # the hub of a fan holds nv - 2 faces
        m = fan(nv)
        dm = {"vertices": to_dev(m["vertices"]), "faces": to_dev(m["faces"]), "rgb8": None}
        if ok:
            t = mesh.topology(dm)
            assert (t["boundary_edges"], t["nonmanifold_edges"], t["degenerate_faces"]) == (nv, 0, 0) and bool(t["boundary_vertices"].all())
            assert mesh.vertex_normals(dm)["normal_info"]["zero_normals"] == 0
            assert mesh.smooth(dm, 1, boundary="free")["smooth"]["pinned"] == 0
        else:
            for fn in (mesh.topology, mesh.vertex_normals, mesh.smooth):
                with pytest.raises(ValueError, match="2\\^20 faces or more"):
                    fn(dm)
    _all_right("fan 65")


def test_an_iteration_that_leaves_the_fixed_point_range_raises():
    dm = _case_mesh("sphere noisy")
    with pytest.raises(ValueError, match="diverged"):                   # lam = 1, mu = -1 triples the sharpest mode every iteration
        mesh.smooth(dm, 300, 1.0, -1.0, "free")
    _all_right("sphere noisy")


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = {"vertices": torch.empty(0, 3, device=DEV), "faces": torch.empty(0, 3, dtype=torch.int32, device=DEV), "rgb8": None,
             "counts": (0, 0), "note": "kept"}
    t = mesh.topology(empty)
    assert t["closed"] is True and tuple(t["boundary_vertices"].shape) == (0,)
    n = mesh.vertex_normals(empty)
    assert tuple(n["normals"].shape) == (0, 3) and n["note"] == "kept" and n["normal_info"]["zero_normals"] == 0
    s = mesh.smooth(empty, 3)
    assert tuple(s["vertices"].shape) == (0, 3) and s["smooth"]["pinned"] == 0 and s["note"] == "kept"
    dm = dict(_case_mesh("blobs"), faces=torch.empty(0, 3, dtype=torch.int32, device=DEV))
    nv = dm["vertices"].shape[0]
    assert mesh.topology(dm)["closed"] is True
    n = mesh.vertex_normals(dm)
    assert n["normal_info"]["zero_normals"] == nv and not bool(n["normals"].any())
    assert np.array_equal(bits(mesh.smooth(dm, 3)["vertices"]), bits(dm["vertices"]))


ORIGIN = (0.1, -0.2, 0.3)


@pytest.mark.parametrize("which", ("dense", "sparse"))
def test_extract_options_equal_the_chain_of_calls(which):
    vol = blob_volumes(ORIGIN)[which == "sparse"]
    plain = vol.extract()
    assert set(plain) == {"vertices", "faces", "rgb8", "counts"} and plain["counts"] == (2902, 5780)
    assert set(vol.extract(smooth_iterations=0, normals=False)) == set(plain)           # the defaults: exactly today's dict
    t = mesh.topology(plain)                                                            # six closed shells: watertight
    assert t["closed"] is True and (t["boundary_edges"], t["nonmanifold_edges"], t["degenerate_faces"]) == (0, 0, 0)
    for filt in (0, 601):
        for cell in (None, 2 * H_ANALYTIC):
            got = vol.extract(min_component_faces=filt, simplify_cell=cell, smooth_iterations=3, normals=True)
            want = mesh.filter_components(plain, filt) if filt else plain
            want = mesh.simplify(want, cell, origin=vol.origin) if cell is not None else want
            moved = mesh.smooth(want, 3)
            want = mesh.vertex_normals(moved)
            same_device_mesh(got, want)
            assert got["smooth"]["iterations"] == 3 and got["counts"][1] > 0 and set(got) == set(want)
            if cell is None and not filt:                                               # the normals of the smoothed positions
                assert not torch.equal(got["normals"], mesh.vertex_normals(plain)["normals"])
    only = vol.extract(normals=True)
    same_device_mesh(only, mesh.vertex_normals(plain))
    assert "smooth" not in only and torch.equal(only["vertices"], plain["vertices"])
    only = vol.extract(smooth_iterations=3)
    same_device_mesh(only, mesh.smooth(plain, 3))
    assert "normals" not in only


def test_scene_mesh_options_write_the_same_ply_twice(tmp_path):
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    out = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(len(lt.r_c2w))), floater_thresh=0.5)
    xyz = pointcloud.fuse_points(None, out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=(0.05, 50.0))["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 28
    kw = dict(voxel=voxel, bounds=(tuple(lo - 3 * voxel), tuple(hi + 3 * voxel)), floater_thresh=0.5, depth_range=(0.05, 50.0))
    files = []
    for _ in range(2):
        got = mesh.scene_mesh(lt, W, H, smooth_iterations=3, normals=True, **kw)
        path = tmp_path / f"mesh{len(files)}.ply"
        pointcloud.write_ply(str(path), got["vertices"], got["rgb8"], normals=got["normals"], faces=got["faces"])
        files.append(path.read_bytes())
    plain = mesh.scene_mesh(lt, W, H, **kw)
    assert set(plain) == {"vertices", "faces", "rgb8", "counts", "volume"}
    want = mesh.vertex_normals(mesh.smooth(plain, 3))
    print(f"scene_mesh: {got['counts']}, {got['smooth']}, {got['normal_info']}")
    same_device_mesh(got, want)
    assert "volume" in got and files[0] == files[1] and len(files[0]) > 200 and got["counts"][1] > 0
    assert b"property float nx" in files[0][:400]
