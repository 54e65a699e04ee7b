"""TSDF fusion and mesh extraction without a GPU: the numpy restatement of csrc/lrf_mesh.inl (tests/mesh_cases.py) on analytic
fields -- closed manifolds with the right Euler characteristic, outward winding, the interpolation error bound, holes only
where weights are missing --, the restated integration on a plane it must recover, argument refusals before any device work
(Python and C ABI), the PLY writer's faces, and the new symbols."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh, pointcloud
from mesh_cases import (H_ANALYTIC, N_ANALYTIC, SPHERE_C, SPHERE_R, boundary_edges, closed_manifold_euler, extract_host,
                        integrate_host, new_volume, signed_volume, sphere_field, tet_case, tet_corners, torus_field)
from mesh_util import DenseStub, forbid_native, forbid_render



@pytest.fixture(scope="module")
def sphere():
    fld = sphere_field()
    return fld, extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC)


def test_case_tables_are_consistent():
    """Every tetrahedron of the split is positively oriented and a monotone path; a case and its complement give the same
    triangles reversed."""
    seen = set()
    for t in range(6):
        c = tet_corners(t)
        p = [np.array([(m >> k) & 1 for k in range(3)], float) for m in c]
        assert np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]])) > 0
        mid = sorted(c[1:3], key=lambda m: bin(m).count("1"))
        assert c[0] == 0 and c[3] == 7 and mid[0] & mid[1] == mid[0] and bin(mid[0]).count("1") == 1
        seen.add(tuple(mid))
    assert len(seen) == 6
    for m in range(16):
        a, b = tet_case(m), tet_case(15 - m)
        assert len(a) == len(b) == (0, 1, 2, 1, 0)[bin(m).count("1")]
        ea = {(tri[k], tri[(k + 1) % 3]) for tri in a for k in range(3)}
        eb = {(tri[(k + 1) % 3], tri[k]) for tri in b for k in range(3)}
        assert len(a) == 0 or len(ea & eb) >= 3                         # the outer edges run the other way


def test_sphere_is_a_closed_outward_manifold_within_the_interpolation_bound(sphere):
    fld, m = sphere
    assert fld.shape == (N_ANALYTIC,) * 3 and float(np.abs(fld).min()) > 1e-6     # no exact level hit
    assert closed_manifold_euler(m) == 2
    vol = signed_volume(m)
    print(f"sphere: {m['counts']} vertices / faces, signed volume {vol:.5f} (ball {4 / 3 * math.pi * SPHERE_R ** 3:.5f})")
    assert vol > 0
    h = H_ANALYTIC
    bar = 3 * h * h / (8 * (SPHERE_R - math.sqrt(3) * h)) + 1e-6
    err = float(np.abs(np.linalg.norm(m["vertices"].astype(np.float64) - np.array(SPHERE_C), axis=1) - SPHERE_R).max())
    print(f"sphere: max | |v - c| - r | = {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    # the surface stays two cells from the border
    assert m["vertices"].min() >= 2 * h and m["vertices"].max() <= 1 - 2 * h


def test_torus_has_euler_characteristic_zero():
    fld = torus_field()
    assert float(np.abs(fld).min()) > 1e-6
    m = extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC)
    assert closed_manifold_euler(m) == 0
    assert signed_volume(m) > 0
    assert m["vertices"].min() >= 2 * H_ANALYTIC and m["vertices"].max() <= 1 - 2 * H_ANALYTIC


def test_level_and_weightless_and_full_weight_agree(sphere):
    fld, m = sphere
    full = extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC, weight=np.ones_like(fld))
    assert np.array_equal(full["faces"], m["faces"]) and np.array_equal(full["vertices"].view(np.uint32), m["vertices"].view(np.uint32))
    shifted = extract_host(fld + np.float32(0.05), (0.0, 0.0, 0.0), H_ANALYTIC, level=0.05)
    assert shifted["counts"] == m["counts"] and closed_manifold_euler(shifted) == 2
    none = extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC, weight=np.zeros_like(fld))
    assert none["counts"] == (0, 0)
    one = extract_host(np.zeros((1, 1, 1), np.float32), (0.0, 0.0, 0.0), 1.0, level=0.5)
    assert one["counts"] == (0, 0)


def test_holes_appear_only_beside_the_unweighted_block(sphere):
    fld, m = sphere
    h = H_ANALYTIC
    w = np.ones_like(fld)
    z0, z1, y0, y1, x0, x1 = 10, 14, 9, 13, 18, 23                      # a block that the sphere's +x cap crosses
    w[z0:z1, y0:y1, x0:x1] = 0
    holed = extract_host(fld, (0.0, 0.0, 0.0), h, weight=w)
    assert 0 < holed["counts"][1] < m["counts"][1]
    b = boundary_edges(holed["faces"])
    assert len(b) > 0
    # cells adjacent to the block: those with a corner in it, grown by one cell; a boundary edge's ends lie in their hull
    lo = np.array([x0 - 2, y0 - 2, z0 - 2]) * h - 1e-6
    hi = np.array([x1 + 1, y1 + 1, z1 + 1]) * h + 1e-6
    ends = holed["vertices"][np.array(b).reshape(-1)]
    assert ((ends >= lo) & (ends <= hi)).all()
    # the rest is unchanged: every face of the holed mesh is a face of the full mesh, by position
    key = lambda mm: {tuple(mm["vertices"][f].view(np.uint32).reshape(-1).tolist()) for f in mm["faces"]}  # noqa: E731
    full, part = key(m), key(holed)
    assert part < full
    gone = np.array([np.frombuffer(np.array(k, np.uint32).tobytes(), np.float32) for k in full - part]).reshape(-1, 3)
    assert ((gone >= lo) & (gone <= hi)).all()                          # only faces beside the block went


def test_restated_integration_recovers_a_plane():
    """A camera at the origin looking down -z at the plane z = -2: depth is 2 everywhere (a multiple of the direction whose z
    is -1).  Seen voxels hold min(1, (z + 2) / trunc), the weight counts the frames, and the zero level is the plane."""
    Hh, Ww, f = 40, 40, 30.0
    c2w = np.tile(np.eye(4, dtype=np.float32)[None, :3], (3, 1, 1))
    c2w[1, 0, 3], c2w[2, 1, 3] = 0.05, -0.05
    depth = np.full((3, Hh, Ww), 2.0, np.float32)
    rgb8 = np.full((3, Hh, Ww, 3), 255, np.uint8)
    rgb8[..., 1] = 51
    origin, voxel, dims, trunc = (-0.4, -0.4, -2.35), 0.1, (9, 9, 7), 0.22
    vol = integrate_host(new_volume(dims), origin, voxel, trunc, depth, rgb8, c2w, f, Ww / 2, Hh / 2)
    z = (np.float32(origin[2]) + np.arange(7, dtype=np.float32) * np.float32(voxel)).astype(np.float64)
    seen = z + 2.0 >= -trunc - 1e-6
    assert (vol["weight"][seen] == 3).all() and (vol["weight"][~seen] == 0).all() and (vol["tsdf"][~seen] == 1).all()
    want = np.minimum(1.0, (z + 2.0) / trunc)
    assert np.abs(vol["tsdf"] - want[:, None, None])[seen].max() < 1e-5
    assert np.abs(vol["rgb"][seen] - np.array([1.0, 0.2, 1.0])).max() < 1e-6 and (vol["rgb"][~seen] == 0).all()
    m = extract_host(vol["tsdf"], origin, voxel, weight=vol["weight"], rgb=vol["rgb"])
    # a horizontal cut leaves 1, 1, 2, 2, 1, 1 triangles in the six tetrahedra of each of the 8 x 8 cells it crosses
    assert m["counts"][1] == 8 * 8 * 8 and np.abs(m["vertices"][:, 2] + 2.0).max() < 1e-5
    a, b, c = (m["vertices"][m["faces"][:, k]].astype(np.float64) for k in range(3))
    assert (np.cross(b - a, c - a)[:, 2] > 0).all()                     # towards the camera: free space
    assert (m["rgb8"] == np.array([255, 51, 255], np.uint8)).all()
    # incremental: frames 0..1 then 1..3
    two = integrate_host(new_volume(dims), origin, voxel, trunc, depth[:1], rgb8[:1], c2w[:1], f, Ww / 2, Hh / 2)
    integrate_host(two, origin, voxel, trunc, depth[1:], rgb8[1:], c2w[1:], f, Ww / 2, Hh / 2)
    assert all(np.array_equal(two[k].view(np.uint32), vol[k].view(np.uint32)) for k in ("tsdf", "weight", "rgb"))


def _frames():
    return dict(depth=torch.ones(2, 4, 5), poses=torch.eye(4)[None, :3].repeat(2, 1, 1), focal=4.0, center=(2.5, 2.0),
                rgb=torch.zeros(2, 4, 5, 3))


def test_python_refusals_before_any_device_work(monkeypatch):
    forbid_native(monkeypatch)
    V = mesh.TsdfVolume
    for bad, match in ((dict(origin=(0, 0)), "origin"), (dict(origin=(0, math.nan, 0)), "origin"), (dict(voxel=0), "voxel"),
                       (dict(voxel=-1.0), "voxel"), (dict(voxel=math.nan), "voxel"), (dict(dims=(3, 3)), "dims"),
                       (dict(dims=(3, 0, 3)), "dims"), (dict(dims=(3, 2.5, 3)), "dims"), (dict(dims=(2048, 2048, 512)), "2\\^31"),
                       (dict(trunc=0), "trunc"), (dict(trunc=math.nan), "trunc")):
        kw = dict(origin=(0, 0, 0), voxel=0.1, dims=(3, 3, 3), trunc=0.3, device="cuda:0")
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            V(**kw)
    with pytest.raises(NativeError):
        V((0, 0, 0), 0.1, (3, 3, 3), 0.3, "cpu")

    def integrate(vol=None, **over):
        a = _frames()
        a.update(over)
        return (vol or DenseStub()).integrate(a["depth"], a["poses"], a["focal"], a["center"], rgb=a["rgb"],
                                         **{k: v for k, v in a.items() if k == "depth_range"})
    for bad, match in ((dict(depth=torch.ones(4, 5)), "depth"), (dict(depth=torch.ones(2, 4, 5).long()), "depth"),
                       (dict(rgb=None), "colours"), (dict(rgb=torch.zeros(2, 4, 5, 2)), "rgb"),
                       (dict(rgb=torch.zeros(2, 4, 5, 3).long()), "rgb"), (dict(poses=torch.zeros(3, 3, 4)), "poses"),
                       (dict(focal=None), "focal"), (dict(center=(1.0, 2.0, 3.0)), "center"),
                       (dict(depth_range=(2.0, 1.0)), "depth_range"), (dict(depth_range=(0.0, math.nan)), "depth_range"),
                       (dict(depth_range=(1.0,)), "depth_range")):
        with pytest.raises(ValueError, match=match):
            integrate(**bad)
    with pytest.raises(ValueError, match="colours"):
        integrate(vol=DenseStub(colours=False))
    with pytest.raises(TypeError):
        integrate(depth=np.ones((2, 4, 5), np.float32))
    with pytest.raises(NativeError):                                    # valid arguments, CPU tensors: no fallback
        integrate()
    with pytest.raises(NativeError):
        integrate(vol=DenseStub(colours=False), rgb=None)
    for bad, match in ((dict(level=math.nan), "level"), (dict(min_weight=0), "min_weight"), (dict(min_weight=math.nan), "min_weight"),
                       (dict(max_vertices=-1), "max_vertices"), (dict(max_faces=1.5), "max_faces"), (dict(max_faces=1 << 31), "max_faces")):
        with pytest.raises(ValueError, match=match):
            DenseStub().extract(**bad)
    vals = torch.zeros(3, 4, 5)
    for args, kw, match in (((torch.zeros(4, 5), (0, 0, 0), 0.1, 0.0), {}, "values"), ((vals.long(), (0, 0, 0), 0.1, 0.0), {}, "values"),
                            ((vals, (0, 0), 0.1, 0.0), {}, "origin"), ((vals, (0, 0, 0), 0.0, 0.0), {}, "voxel"),
                            ((vals, (0, 0, 0), 0.1, math.nan), {}, "level"),
                            ((vals, (0, 0, 0), 0.1, 0.0), dict(weight=torch.zeros(3, 4, 4)), "weight"),
                            ((vals, (0, 0, 0), 0.1, 0.0), dict(rgb=torch.zeros(3, 4, 5)), "rgb"),
                            ((vals, (0, 0, 0), 0.1, 0.0), dict(weight=torch.zeros(3, 4, 5), min_weight=-1), "min_weight"),
                            ((vals, (0, 0, 0), 0.1, 0.0), dict(max_vertices=-2), "max_vertices")):
        with pytest.raises(ValueError, match=match):
            mesh.extract_mesh(*args, **kw)
    with pytest.raises(TypeError):
        mesh.extract_mesh(np.zeros((3, 4, 5), np.float32), (0, 0, 0), 0.1, 0.0)
    with pytest.raises(NativeError):
        mesh.extract_mesh(vals, (0, 0, 0), 0.1, 0.0)


def test_scene_mesh_refusals_on_a_cpu_scene(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    need = 21 * 21 * 21 * 20
    with pytest.raises(ValueError, match=f"{need} bytes"):
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"{21 ** 3 * 8} bytes"):
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, colours=False, max_bytes=100)
    for kw, match in ((dict(voxel=0.0), "voxel"), (dict(voxel=0.1, trunc=-1.0), "trunc"), (dict(voxel=0.1, bounds=((0, 0, 0),)), "bounds"),
                      (dict(voxel=0.1, bounds=((1, 0, 0), (0, 1, 1))), "bounds"), (dict(voxel=0.1, depth_range=(2, 1)), "depth_range"),
                      (dict(voxel=0.1, min_weight=0), "min_weight"), (dict(voxel=0.1, frames_per_call=0), "frames_per_call"),
                      (dict(voxel=1e-4, bounds=box), "2\\^31"), (dict(voxel=0.1, poses=torch.zeros(3, 2, 4)), "poses")):
        with pytest.raises(ValueError, match=match):
            mesh.scene_mesh(lt, W, H, **kw)
    with pytest.raises(ValueError, match="W, H"):
        mesh.scene_mesh(lt, 0, H, voxel=0.1)
    with pytest.raises(TypeError, match="unknown"):
        mesh.scene_mesh(lt, W, H, voxel=0.1, strides=2)
    fov = lt.fov
    lt.fov = 360
    with pytest.raises(ValueError, match="pinhole"):
        mesh.scene_mesh(lt, W, H, voxel=0.1)
    lt.fov = fov
    with pytest.raises(NativeError):                                    # valid arguments, CPU scene
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box)
    with pytest.raises(NativeError):
        mesh.scene_mesh(lt, W, H, voxel=0.1)


# the options of the post-processing chain in the order in which bad values are reported, one refused value each
CHAIN_BAD = (("min_component_faces", -1), ("min_component_fraction", 2.0), ("simplify_cell", 0), ("smooth_iterations", -1),
             ("normals", 1), ("fill_holes", 2))


def test_bad_chain_options_are_refused_in_one_order_at_every_entry_point(monkeypatch):
    """Of two bad options the one that comes first in CHAIN_BAD is named, a bad level wins over all of them, and both extract
    methods and scene_mesh say the same."""
    from novel_views_cases import scene
    forbid_native(monkeypatch)
    forbid_render(monkeypatch)
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    entries = (DenseStub().extract, mesh.SparseTsdfVolume.__new__(mesh.SparseTsdfVolume).extract,
               lambda **kw: mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, **kw))

    def refusals(**kw):
        said = []
        for entry in entries:
            with pytest.raises(ValueError) as e:
                entry(**kw)
            said.append(str(e.value))
        assert said[0] == said[1] == said[2], said
        return said[0]
    for i, (first, bad) in enumerate(CHAIN_BAD):
        assert first in refusals(**{first: bad})
        assert "level" in refusals(level=math.nan, **{first: bad})
        for second, worse in CHAIN_BAD[i + 1:]:
            said = refusals(**{first: bad, second: worse})
            assert first in said and second not in said, (first, second, said)
    assert "level" in refusals(level=math.nan, **dict(CHAIN_BAD))
    assert all(mesh._MESH_KEYS.count(name) == 1 for name, _ in CHAIN_BAD) and len(mesh._MESH_KEYS) == 7 + len(CHAIN_BAD)


def _read_ply(raw):
    """A small reader of what write_ply writes -> (vertex record array, faces [F,3] or None)."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elems, props = [], {}
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            elems.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[:1] == ["property"]:
            props[elems[-1][0]].append(w[1:])
    assert elems[0][0] == "vertex"
    kinds = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(p[1], kinds[p[0]]) for p in props["vertex"]])
    nv = elems[0][1]
    verts = np.frombuffer(raw[end:end + nv * vdt.itemsize], dtype=vdt)
    rest = raw[end + nv * vdt.itemsize:]
    if len(elems) == 1:
        assert rest == b""
        return verts, None
    assert elems[1][0] == "face" and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    fdt = np.dtype([("n", "u1"), ("v", "<i4", 3)])
    assert len(rest) == elems[1][1] * fdt.itemsize and fdt.itemsize == 13
    rec = np.frombuffer(rest, dtype=fdt)
    assert (rec["n"] == 3).all()
    return verts, rec["v"]


def test_write_ply_faces_round_trip(tmp_path, sphere):
    _, m = sphere
    rgb = np.random.default_rng(3).integers(0, 256, m["vertices"].shape, dtype=np.uint8)
    for cols in (rgb, None):
        path = tmp_path / "mesh.ply"
        n = pointcloud.write_ply(str(path), torch.from_numpy(m["vertices"]), None if cols is None else cols,
                                 faces=torch.from_numpy(m["faces"]))
        assert n == m["vertices"].shape[0]
        verts, faces = _read_ply(path.read_bytes())
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], -1).view(np.uint32), m["vertices"].view(np.uint32))
        assert np.array_equal(faces, m["faces"])
        if cols is not None:
            assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], -1), rgb)
    pointcloud.write_ply(str(tmp_path / "none.ply"), m["vertices"], faces=np.zeros((0, 3), np.int32))
    assert _read_ply((tmp_path / "none.ply").read_bytes())[1].shape == (0, 3)
    for bad in (m["faces"][:, :2], m["faces"].astype(np.float32), m["faces"] + m["vertices"].shape[0], -1 - m["faces"]):
        with pytest.raises(ValueError, match="faces"):
            pointcloud.write_ply(str(tmp_path / "bad.ply"), m["vertices"], faces=bad)
    # without faces the bytes are what they were: header and records as the point-cloud writer lays them out
    xyz = m["vertices"][:37]
    for cols, nrm in ((rgb[:37], None), (None, None), (rgb[:37], xyz)):
        pointcloud.write_ply(str(tmp_path / "cloud.ply"), xyz, cols, nrm)
        head = ["ply", "format binary_little_endian 1.0", "element vertex 37", "property float x", "property float y", "property float z"]
        head += ["property float nx", "property float ny", "property float nz"] if nrm is not None else []
        head += ["property uchar red", "property uchar green", "property uchar blue"] if cols is not None else []
        dt = np.dtype([("p", "<f4", 3)] + ([("n", "<f4", 3)] if nrm is not None else []) + ([("c", "u1", 3)] if cols is not None else []))
        rec = np.zeros(37, dt)
        rec["p"] = xyz
        if nrm is not None:
            rec["n"] = nrm
        if cols is not None:
            rec["c"] = cols
        assert (tmp_path / "cloud.ply").read_bytes() == ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + rec.tobytes()


def test_mesh_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, ("lrf_tsdf_integrate", "lrf_mesh_workspace_bytes", "lrf_mesh_extract"))
    assert "typedef struct LrfTsdfVolume" in header and "typedef struct LrfMeshExtract" in header
    assert C.sizeof(N.LrfTsdfVolume) == 3 * 8 + 3 * 4 + 5 * 4 and C.sizeof(N.LrfMeshExtract) == 3 * 8 + 3 * 4 + 6 * 4 + 4    # padded to 8
    assert built_lib.lrf_abi_version() == 7
    ws = built_lib.lrf_mesh_workspace_bytes
    assert ws(0, 4, 5) == 0 and ws(4, -1, 5) == 0 and ws(2048, 2048, 512) == 0 and ws(1 << 16, 1 << 16, 1) == 0
    assert ws(1, 1, 1) == 256 and ws(256, 256, 256) >= 4 * 256 ** 3 + 8 * 256 ** 3 // 256

    def integrate(depth=FAKE, rgb8=FAKE, c2w=FAKE, focal=FAKE, center=FAKE, V=2, H=4, W=5, d_min=0.0, d_max=math.inf, **over):
        a = filled(N.LrfTsdfVolume, dict(tsdf=FAKE, weight=FAKE, rgb=FAKE, Nx=3, Ny=4, Nz=5, voxel=0.1, trunc=0.3), **over)
        return refused(built_lib, built_lib.lrf_tsdf_integrate(C.byref(a), depth, rgb8, c2w, focal, center, V, H, W, d_min, d_max, None))
    for bad in (dict(Nx=0), dict(Ny=-1), dict(Nz=0), dict(Nx=2048, Ny=2048, Nz=512)):
        assert "need Nx, Ny, Nz >= 1 and Nx Ny Nz < 2^31" in integrate(**bad)
    for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(V=1 << 20, H=1 << 10, W=2)):
        assert "need V, H, W >= 1 and V H W < 2^31" in integrate(**bad)
    for bad in (dict(tsdf=None), dict(weight=None), dict(depth=None), dict(c2w=None), dict(focal=None), dict(center=None)):
        assert integrate(**bad) == "lrf_tsdf_integrate: null argument", bad
    assert "go together" in integrate(rgb=None) and "go together" in integrate(rgb8=None)
    assert "voxel" in integrate(voxel=0.0) and "voxel" in integrate(voxel=math.nan)
    assert "trunc" in integrate(trunc=0.0) and "trunc" in integrate(trunc=-1.0) and "trunc" in integrate(trunc=math.nan)
    assert "d_min <= d_max" in integrate(d_min=2.0, d_max=1.0) and "d_min <= d_max" in integrate(d_min=math.nan)
    assert "4-byte aligned" in integrate(tsdf=FAKE + 2) and "4-byte aligned" in integrate(depth=FAKE + 1)
    assert built_lib.lrf_tsdf_integrate(None, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 4, 5, 0.0, 1.0, None) != 0

    def extract(max_v=10, max_f=10, vertices=FAKE, rgb8_out=FAKE, faces=FAKE, counts=FAKE, wsp=FAKE, **over):
        a = filled(N.LrfMeshExtract, dict(value=FAKE, weight=FAKE, rgb=FAKE, Nx=3, Ny=4, Nz=5, voxel=0.1, level=0.0, min_weight=1.0), **over)
        return refused(built_lib, built_lib.lrf_mesh_extract(C.byref(a), max_v, max_f, vertices, rgb8_out, faces, counts, wsp, None))
    for bad in (dict(Nx=0), dict(Nz=-3), dict(Nx=2048, Ny=2048, Nz=512)):
        assert "need Nx, Ny, Nz >= 1 and Nx Ny Nz < 2^31" in extract(**bad)
    for bad in (dict(value=None), dict(vertices=None), dict(faces=None), dict(counts=None), dict(wsp=None)):
        assert extract(**bad) == "lrf_mesh_extract: null argument", bad
    assert "go together" in extract(rgb=None) and "go together" in extract(rgb8_out=None)
    assert "voxel" in extract(voxel=-0.1) and "level" in extract(level=math.nan)
    assert "min_weight" in extract(min_weight=0.0) and "min_weight" in extract(min_weight=math.nan)
    assert "[0, 2^31)" in extract(max_v=-1) and "[0, 2^31)" in extract(max_f=1 << 31)
    assert "4-byte aligned" in extract(vertices=FAKE + 2) and "4-byte aligned" in extract(wsp=FAKE + 1)
    assert "8-byte aligned" in extract(counts=FAKE + 4)
    assert built_lib.lrf_mesh_extract(None, 1, 1, FAKE, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_mesh_kernels_use_no_scratch_and_keep_the_pose_in_scalar_registers():
    """k_tsdf_integrate, k_mesh_count and k_mesh_emit as __graft_entry__.build() compiles them: no scratch; the frame loop reads
    the camera matrix with scalar loads, divides in full precision and rounds to nearest even."""
    import re
    from isa_util import assert_no_scratch, device_asm
    found = assert_no_scratch(device_asm(), (r"k_tsdf_integrate", r"k_mesh_count", r"k_mesh_emit"), match="search", total=3, body_too=True)
    integ = found[0][1]
    assert "v_div_fixup_f32" in integ and "v_rndne_f32" in integ
    assert re.search(r"s_load_dwordx(4|8)", integ)
