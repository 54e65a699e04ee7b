"""Hole filling on the MI355X (csrc/lrf_mesh_fill.inl through localrf_amd.mesh): every case of tests/mesh_fill_cases.py against
the numpy restatement bit for bit -- vertices as uint32, colours, faces and every count --, reproducibility, what topology and
smooth say of the filled mesh, the capacity flag, refusals, and the extract option on a punched volume."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from localrf_amd import NativeError, _native, mesh
from localrf_amd._checks import float_of_key
from localrf_amd.mesh import fill_holes, holes  # noqa: F401  (what every test here is about)
from mesh_clean_cases import fan
from mesh_fill_cases import CASE_NAMES, CLOSABLE, E2E_H, E2E_N, HOLE_KEYS, UNCHANGED, cases, e2e_volume, expected
from mesh_util import DEV, bits, device_mesh, to_dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case_mesh(name):
    m = cases()[name][0]
    return device_mesh(m, note="kept", normals=torch.zeros(m["vertices"].shape[0], 3, device=DEV))


def _same_as_host(got, want):
    assert got["vertices"].dtype is torch.float32 and got["faces"].dtype is torch.int32
    assert np.array_equal(bits(got["vertices"]), np.ascontiguousarray(want["vertices"]).view(np.uint32))
    assert np.array_equal(got["faces"].cpu().numpy(), want["faces"])
    assert (got["rgb8"] is None) == (want["rgb8"] is None)
    if want["rgb8"] is not None:
        assert got["rgb8"].dtype is torch.uint8 and np.array_equal(got["rgb8"].cpu().numpy(), want["rgb8"])
    assert got["counts"] == (want["vertices"].shape[0], want["faces"].shape[0])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_holes_and_fill_equal_the_restatement_bit_for_bit(name):
    dm, max_edges, want = _case_mesh(name), cases()[name][1], expected(name)
    before = (bits(dm["vertices"]).copy(), dm["faces"].cpu().numpy().copy())
    h = mesh.holes(dm, max_edges)
    print(f"{name}: {dm['counts']} max_edges {max_edges} {h}")
    assert tuple(h) == HOLE_KEYS and all(type(h[k]) is int for k in h)
    assert h == {k: want["fill"][k] for k in HOLE_KEYS}
    got = mesh.fill_holes(dm, max_edges)
    assert got["fill"] == want["fill"] and all(type(v) is int for v in got["fill"].values())
    _same_as_host(got, want)
    assert set(got) == (set(dm) | {"fill"}) - {"normals"} and got["note"] == "kept"
    if name in UNCHANGED:                                                       # nothing fillable: the input's tensors
        assert got["vertices"] is dm["vertices"] and got["faces"] is dm["faces"] and got["rgb8"] is dm["rgb8"]
    else:
        assert got["vertices"].data_ptr() != dm["vertices"].data_ptr() and got["faces"].data_ptr() != dm["faces"].data_ptr()
    assert np.array_equal(bits(dm["vertices"]), before[0]) and np.array_equal(dm["faces"].cpu().numpy(), before[1])
    again = mesh.fill_holes(dm, max_edges)                                      # two runs, the same bytes
    _same_as_host(again, want)
    twice = mesh.fill_holes(got, max_edges)                                     # a second fill adds nothing
    assert twice["fill"]["loops"] == 0 and twice["fill"]["boundary_edges"] == want["fill"]["open_edges"]
    assert twice["vertices"] is got["vertices"] and twice["faces"] is got["faces"] and twice["counts"] == got["counts"]


@pytest.mark.parametrize("name", CLOSABLE)
def test_the_filled_mesh_is_closed_and_smooth_pins_nothing(name):
    dm, max_edges = _case_mesh(name), cases()[name][1]
    got = mesh.fill_holes(dm, max_edges)
    t = mesh.topology(got)
    assert t["closed"] is True and t["boundary_edges"] == 0 and not bool(t["boundary_vertices"].any())
    s = mesh.smooth(got, 1, boundary="fixed")
    assert s["smooth"]["pinned"] == 0 and s["smooth"]["boundary_edges"] == 0
    if got["fill"]["loops"]:
        assert mesh.topology(dm)["closed"] is False
        assert mesh.smooth(dm, 1, boundary="fixed")["smooth"]["pinned"] > 0


def test_a_side_stream_gives_the_same_bytes():
    for name in ("sphere minus 90", "sphere caps 65", "fan 1025 / max_edges 1025"):
        dm, max_edges, want = _case_mesh(name), cases()[name][1], expected(name)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            got = mesh.fill_holes(dm, max_edges)
        side.synchronize()
        _same_as_host(got, want)


def _native_fill(dm, max_edges, cap_v, cap_f, rows_v, rows_f):
    """lrf_mesh_fill into buffers of rows_v and rows_f rows filled with a pattern -> (vertices, faces, info words)."""
    dev = torch.device(DEV)
    nv, nf = dm["counts"]
    keys = torch.empty(7, dtype=torch.int32, device=dev)
    _native.launch("lrf_mesh_smooth_bounds", dev, dm["vertices"].data_ptr(), nv, keys.data_ptr(), guard=True)
    keys = keys.tolist()
    lo = [float_of_key(k) for k in keys[:3]]
    extent = max(float_of_key(k) - l for k, l in zip(keys[3:6], lo))
    a = _native.LrfMeshHoles()
    a.vertices, a.rgb8, a.faces, a.Nv, a.Nf, a.max_edges = dm["vertices"].data_ptr(), None, dm["faces"].data_ptr(), nv, nf, max_edges
    a.s = 36 - int(np.frexp(extent)[1])
    for k in range(3):
        a.lo[k] = lo[k]
    vo = torch.full((rows_v, 3), -7.0, dtype=torch.float32, device=dev)
    fo = torch.full((rows_f, 3), -7, dtype=torch.int32, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ws = _native.workspace("lrf_mesh_holes", dev, nv, nf)
    _native.launch("lrf_mesh_fill", dev, C.byref(a), vo.data_ptr(), None, fo.data_ptr(), cap_v, cap_f, info.data_ptr(), ws.data_ptr(), guard=True)
    return vo.cpu().numpy(), fo.cpu().numpy(), [int(x) for x in info.tolist()]


def test_a_capacity_one_short_sets_the_flag_and_writes_nothing_past_it():
    name = "sphere minus 20 / no colours"
    dm, max_edges, want = _case_mesh(name), cases()[name][1], expected(name)
    nv, nf = want["vertices"].shape[0], want["faces"].shape[0]
    v, f, words = _native_fill(dm, max_edges, nv, nf, nv + 2, nf + 2)           # the exact capacities: no flag, the rows beyond stay
    assert words[0] == 0 and words[4:6] == [20, 60]
    assert np.array_equal(v[:nv].view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(f[:nf], want["faces"])
    assert (v[nv:] == -7.0).all() and (f[nf:] == -7).all()
    v, f, words = _native_fill(dm, max_edges, nv, nf - 1, nv + 2, nf + 2)       # one face short
    assert words[0] == 16 and words[4:6] == [20, 60]
    assert np.array_equal(f[:nf - 1], want["faces"][:nf - 1]) and (f[nf - 1:] == -7).all() and (v[nv:] == -7.0).all()
    v, f, words = _native_fill(dm, max_edges, nv - 1, nf, nv + 2, nf + 2)       # one vertex short
    assert words[0] == 16
    assert np.array_equal(v[:nv - 1].view(np.uint32), want["vertices"][:nv - 1].view(np.uint32)) and (v[nv - 1:] == -7.0).all()
    assert (f[nf:] == -7).all()


def _all_right(name="sphere caps 64"):
    """The next valid call is right."""
    got = mesh.fill_holes(_case_mesh(name), cases()[name][1])
    assert got["fill"] == expected(name)["fill"]
    _same_as_host(got, expected(name))


def test_bad_face_indices_and_vertices_that_are_not_finite_raise_and_the_next_call_is_right():
    name = "sphere caps 64"
    m, dm = cases()[name][0], _case_mesh(name)
    nv, nf = m["vertices"].shape[0], m["faces"].shape[0]
    for bad in (nv, -1, (1 << 31) - 1, -(1 << 31)):
        for row, col in ((0, 0), (nf - 1, 2)):
            faces = m["faces"].copy()
            faces[row, col] = bad
            for fn in (mesh.holes, mesh.fill_holes):
                with pytest.raises(ValueError, match=f"outside \\[0, {nv}\\)"):
                    fn(dict(dm, faces=to_dev(faces)))
    for bad in (np.nan, np.inf, -np.inf):
        for row, col in ((0, 0), (nv - 1, 2)):
            v = m["vertices"].copy()
            v[row, col] = bad
            for fn in (mesh.holes, mesh.fill_holes):
                with pytest.raises(ValueError, match="not finite"):
                    fn(dict(dm, vertices=to_dev(v)))
    _all_right()


def test_cpu_tensors_raise_native_error_and_a_row_of_2_to_the_20_raises():
    m = cases()["tetrahedron minus one face"][0]
    cpu = {"vertices": torch.from_numpy(m["vertices"]), "faces": torch.from_numpy(m["faces"]), "rgb8": None}
    for fn in (mesh.holes, mesh.fill_holes):
        with pytest.raises(NativeError):
            fn(cpu)
        with pytest.raises(NativeError):
            fn(dict(_case_mesh("tetrahedron minus one face"), faces=cpu["faces"]))
    big = fan((1 << 20) + 2)                                                    # its hub holds 2^20 faces
    dm = {"vertices": to_dev(big["vertices"]), "faces": to_dev(big["faces"]), "rgb8": None}
    for fn in (mesh.holes, mesh.fill_holes):
        with pytest.raises(ValueError, match="2\\^20 faces or more"):
            fn(dm)
    _all_right("fan 65 / max_edges 65")


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = {"vertices": torch.empty(0, 3, device=DEV), "faces": torch.empty(0, 3, dtype=torch.int32, device=DEV), "rgb8": None,
             "counts": (0, 0), "note": "kept"}
    assert mesh.holes(empty) == dict.fromkeys(HOLE_KEYS, 0)
    got = mesh.fill_holes(empty)
    assert got["vertices"] is empty["vertices"] and got["faces"] is empty["faces"] and got["note"] == "kept" and got["counts"] == (0, 0)
    assert got["fill"] == dict(dict.fromkeys(HOLE_KEYS, 0), added_vertices=0, added_faces=0)
    dm = dict(_case_mesh("sphere"), faces=torch.empty(0, 3, dtype=torch.int32, device=DEV))
    assert mesh.holes(dm) == dict.fromkeys(HOLE_KEYS, 0)
    got = mesh.fill_holes(dm)
    assert got["fill"]["loops"] == 0 and got["vertices"] is dm["vertices"] and "normals" not in got


@functools.lru_cache(maxsize=None)
def _punched_volumes():
    fld, w = e2e_volume()
    rgb = np.random.default_rng(13).uniform(0.0, 1.0, fld.shape + (3,)).astype(np.float32)
    dense = mesh.TsdfVolume((0.0, 0.0, 0.0), E2E_H, (E2E_N,) * 3, 3 * E2E_H, DEV)
    dense.tsdf.copy_(to_dev(fld)); dense.weight.copy_(to_dev(w)); dense.rgb.copy_(to_dev(rgb))
    B = E2E_N // 8
    sparse = mesh.SparseTsdfVolume((0.0, 0.0, 0.0), E2E_H, (B, B, B), 3 * E2E_H, DEV, colours=False)
    sparse.marks.fill_(1)
    assert sparse.allocate() == B ** 3

    def pooled(a):
        return to_dev(np.ascontiguousarray(a.reshape(B, 8, B, 8, B, 8).transpose(0, 2, 4, 1, 3, 5).reshape(B ** 3, 8, 8, 8)))
    sparse.tsdf.copy_(pooled(fld)); sparse.weight.copy_(pooled(w))
    return dense, sparse


@pytest.mark.parametrize("which", ("dense", "sparse"))
def test_extract_fills_the_hole_a_block_of_unseen_points_leaves(which):
    vol = _punched_volumes()[which == "sparse"]
    plain = vol.extract()
    assert set(plain) == {"vertices", "faces", "rgb8", "counts"} and set(vol.extract(fill_holes=0)) == set(plain)
    t = mesh.topology(plain)
    assert t["closed"] is False and t["boundary_edges"] == 32 and t["nonmanifold_edges"] == 0
    got = vol.extract(fill_holes=64)
    print(f"{which}: {plain['counts']} -> {got['counts']} {got['fill']}")
    assert got["fill"]["loops"] == 1 and got["fill"]["loop_edges"] == 32 and got["fill"]["open_edges"] == 0
    assert got["counts"] == (plain["counts"][0] + 1, plain["counts"][1] + 32)
    assert mesh.topology(got)["closed"] is True
    want = mesh.fill_holes(plain, 64)
    assert torch.equal(got["vertices"].view(torch.int32), want["vertices"].view(torch.int32)) and torch.equal(got["faces"], want["faces"])
    assert (got["rgb8"] is None) == (which == "sparse") and (got["rgb8"] is None or torch.equal(got["rgb8"], want["rgb8"]))
    assert vol.extract(fill_holes=16)["fill"]["loops"] == 0                     # the rim is longer than 16 edges: left alone
    # the option sits between the component filter and simplify; smooth then moves the closed rim
    chain = vol.extract(min_component_faces=10, fill_holes=64, simplify_cell=2 * E2E_H, smooth_iterations=2, normals=True)
    by_hand = mesh.vertex_normals(mesh.smooth(mesh.simplify(mesh.fill_holes(mesh.filter_components(plain, 10), 64), 2 * E2E_H,
                                                            origin=vol.origin), 2))
    assert torch.equal(chain["vertices"].view(torch.int32), by_hand["vertices"].view(torch.int32))
    assert torch.equal(chain["faces"], by_hand["faces"]) and torch.equal(chain["normals"].view(torch.int32), by_hand["normals"].view(torch.int32))
    assert chain["fill"] == by_hand["fill"] and chain["fill"]["loops"] == 1
    assert vol.extract(fill_holes=64, smooth_iterations=1)["smooth"]["pinned"] == 0 and vol.extract(smooth_iterations=1)["smooth"]["pinned"] == 32
