"""The block-sparse TSDF volume without a GPU: the numpy restatement of csrc/lrf_tsdf_blocks.inl (tests/sparse_mesh_cases.py)
-- the allocation rule covers every band point of the dense integration, the mesh over the stored blocks is the dense mesh
and a missing block only leaves a hole --, argument refusals before any device work (Python and C ABI), and the new symbols."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh
from mesh_cases import (H_ANALYTIC, closed_manifold_euler, extract_host, integrate_host, new_volume, sphere_field)
from mesh_util import SparseStub, forbid_native, forbid_render
from sparse_mesh_cases import (assign_host, dims_of, extract_blocks_host, face_keys, fuse_host, integrate_blocks_host, lattice_for,
                               new_sparse, random_frames, spread_lattice, to_dense_host, touch_host, trajectory)

NEW = ("lrf_tsdf_blocks_touch", "lrf_tsdf_blocks_assign_workspace_bytes", "lrf_tsdf_blocks_assign", "lrf_tsdf_blocks_integrate",
       "lrf_mesh_extract_blocks_workspace_bytes", "lrf_mesh_extract_blocks")


def _dense(blocks, lat, case, depth_range=(0.0, np.inf)):
    return integrate_host(new_volume(dims_of(blocks)), lat[0], lat[1], lat[2], case["depth"], case["rgb8"], case["c2w"], case["f"],
                          case["cx"], case["cy"], depth_range=depth_range)


def _check_properties(blocks, lat, case, depth_range=(0.0, np.inf)):
    """Property 1 (coverage) and property 2 (same mesh) of one case -> (blocks marked, band points, dense faces)."""
    sv, most = fuse_host(blocks, lat, case, depth_range)
    vol = _dense(blocks, lat, case, depth_range)
    d = to_dense_host(sv)
    band = (vol["weight"] > 0) & (vol["tsdf"] < 1)
    misses = int((band & ~d["stored"]).sum())
    print(f"{blocks} range {depth_range}: {int(sv['marks'].sum())} of {sv['marks'].size} blocks marked (at most {most} per pixel), "
          f"{int(band.sum())} band points, {misses} outside a marked block")
    assert misses == 0
    for k in ("tsdf", "weight", "rgb"):                                 # a stored point holds the dense bits
        assert np.array_equal(d[k][d["stored"]].view(np.uint32), vol[k][d["stored"]].view(np.uint32)), k
    dense = extract_host(vol["tsdf"], lat[0], lat[1], weight=vol["weight"], rgb=vol["rgb"])
    sparse = extract_blocks_host(sv)
    a, b = face_keys(dense), face_keys(sparse)
    assert len(a) == dense["counts"][1] and len(b) == sparse["counts"][1]
    print(f"    faces: dense {len(a)}, sparse {len(b)}, sparse only {len(b - a)}, dense only {len(a - b)}")
    assert not b - a and not a - b
    return int(sv["marks"].sum()), int(band.sum()), dense["counts"][1]


@pytest.mark.parametrize("clean,blocks,voxel,centre,want", [
    (True, (5, 4, 6), 0.06, (0.1, 0.0, -3.2), (86, 6842, 10248)),
    (False, (5, 4, 6), 0.06, (0.1, 0.0, -3.2), (106, 9209, 13884)),
    (True, (10, 8, 10), 0.04, (0.1, 0.0, -3.0), (240, 28888, 40888)),
    (False, (10, 8, 10), 0.04, (0.1, 0.0, -3.0), (530, 36685, 54906))])
def test_trajectory_blocks_band_points_and_faces(clean, blocks, voxel, centre, want):
    assert _check_properties(blocks, lattice_for(blocks, voxel, centre), trajectory(clean)) == want


@pytest.mark.parametrize("V,H,W", [(1, 17, 23), (3, 17, 23), (3, 48, 64)])
def test_random_frames_are_covered_and_give_the_dense_mesh(V, H, W):
    case = random_frames(V, H, W)
    for blocks in ((3, 3, 3), (2, 1, 2)):
        for rng in (case["depth_range"], (2.8, 3.3)):
            _check_properties(blocks, spread_lattice(blocks), case, rng)


def test_a_missing_block_only_leaves_a_hole():
    blocks, case = (5, 4, 6), trajectory(True)
    lat = lattice_for(blocks, 0.06, (0.1, 0.0, -3.2))
    full, _ = fuse_host(blocks, lat, case)
    whole = extract_blocks_host(full)
    # the stored block that holds the most face cells: the surface runs through it
    cells, n = np.unique(whole["cells"] >> 3, axis=0, return_counts=True)
    gone = tuple(int(v) for v in cells[n.argmax()])
    sv = new_sparse(lat[0], lat[1], blocks, lat[2])
    touch_host(sv, case["depth"], case["c2w"], case["f"], case["cx"], case["cy"])
    assert sv["marks"][gone[2], gone[1], gone[0]] == 1
    sv["marks"][gone[2], gone[1], gone[0]] = 0
    assign_host(sv)
    integrate_blocks_host(sv, case["depth"], case["rgb8"], case["c2w"], case["f"], case["cx"], case["cy"])
    assert sv["coords"].shape[0] == full["coords"].shape[0] - 1
    holed = extract_blocks_host(sv)
    # the faces that must go: those of cells with a corner in the missing block
    lo, hi = 8 * np.array(gone) - 1, 8 * np.array(gone) + 7
    touches = ((whole["cells"] >= lo) & (whole["cells"] <= hi)).all(1)
    assert 0 < touches.sum() < touches.size
    v = whole["vertices"].view(np.uint32)
    key = lambda rows: {tuple(r) for r in v[whole["faces"][rows]].reshape(-1, 9).tolist()}  # noqa: E731
    assert face_keys(holed) == key(~touches)
    assert not face_keys(holed) & key(touches) and holed["counts"][1] == int((~touches).sum())


def test_sphere_with_every_block_is_a_closed_manifold():
    fld = sphere_field()
    sv = new_sparse((0.0, 0.0, 0.0), H_ANALYTIC, (3, 3, 3), 3 * H_ANALYTIC, colours=False)
    sv["marks"][...] = 1
    assert assign_host(sv) == 27 and np.array_equal(sv["table"].reshape(-1), np.arange(27))
    sv["tsdf"] = np.ascontiguousarray(fld.reshape(3, 8, 3, 8, 3, 8).transpose(0, 2, 4, 1, 3, 5).reshape(27, 8, 8, 8))
    sv["weight"] = np.ones_like(sv["tsdf"])
    assert np.array_equal(to_dense_host(sv)["tsdf"], fld)
    m = extract_blocks_host(sv)
    assert closed_manifold_euler(m) == 2
    assert face_keys(m) == face_keys(extract_host(fld, (0.0, 0.0, 0.0), H_ANALYTIC))


def test_assignment_keeps_earlier_indices_and_refuses_past_the_limit():
    sv = new_sparse((0.0, 0.0, 0.0), 0.1, (3, 2, 2), 0.3)
    sv["marks"][1, 0, 2] = sv["marks"][0, 1, 1] = 1
    assert assign_host(sv) == 2
    assert sv["coords"].tolist() == [[1, 1, 0], [2, 0, 1]] and sv["table"][0, 1, 1] == 0 and sv["table"][1, 0, 2] == 1
    sv["marks"][0, 0, 0] = sv["marks"][1, 1, 2] = 1
    assert assign_host(sv) == 2                                          # appended in (z, y, x) order behind the first two
    assert sv["coords"].tolist() == [[1, 1, 0], [2, 0, 1], [0, 0, 0], [2, 1, 1]]
    sv["marks"][...] = 1
    before = sv["table"].copy()
    assert assign_host(sv, max_blocks=11) == 8 and np.array_equal(sv["table"], before)   # 12 blocks do not fit: nothing changes


# ------------------------------------------------------------------------------------------------ refusals
def _frames():
    return dict(depth=torch.ones(2, 4, 5), poses=torch.eye(4)[None, :3].repeat(2, 1, 1), focal=4.0, center=(2.5, 2.0),
                rgb=torch.zeros(2, 4, 5, 3))


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    V = mesh.SparseTsdfVolume
    for bad, match in ((dict(origin=(0, 0)), "origin"), (dict(origin=(0, math.nan, 0)), "origin"), (dict(voxel=0), "voxel"),
                       (dict(voxel=math.nan), "voxel"), (dict(blocks=(3, 3)), "blocks"), (dict(blocks=(3, 0, 3)), "blocks"),
                       (dict(blocks=(3, 2.5, 3)), "blocks"), (dict(blocks=(2048, 2048, 512)), "Bx By Bz < 2\\^31"),
                       (dict(blocks=(1 << 28, 1, 1)), "8 B < 2\\^31"), (dict(trunc=0), "trunc"), (dict(trunc=math.nan), "trunc")):
        kw = dict(origin=(0, 0, 0), voxel=0.1, blocks=(3, 3, 3), trunc=0.3, device="cuda:0")
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            V(**kw)
    with pytest.raises(NativeError):
        V((0, 0, 0), 0.1, (3, 3, 3), 0.3, "cpu")

    def call(method, vol=None, **over):
        a = _frames()
        a.update(over)
        kw = {k: v for k, v in a.items() if k == "depth_range"}
        if method == "integrate":
            kw["rgb"] = a["rgb"]
        return getattr(vol or SparseStub(), method)(a["depth"], a["poses"], a["focal"], a["center"], **kw)
    for method in ("touch", "integrate"):
        for bad, match in ((dict(depth=torch.ones(4, 5)), "depth"), (dict(depth=torch.ones(2, 4, 5).long()), "depth"),
                           (dict(poses=torch.zeros(3, 3, 4)), "poses"), (dict(focal=None), "focal"),
                           (dict(center=(1.0, 2.0, 3.0)), "center"), (dict(depth_range=(2.0, 1.0)), "depth_range"),
                           (dict(depth_range=(0.0, math.nan)), "depth_range"), (dict(depth_range=(1.0,)), "depth_range")):
            with pytest.raises(ValueError, match=match):
                call(method, **bad)
        with pytest.raises(TypeError):
            call(method, depth=np.ones((2, 4, 5), np.float32))
        with pytest.raises(NativeError):                                # valid arguments, CPU tensors: no fallback
            call(method)
    for bad, match in ((dict(rgb=None), "colours"), (dict(rgb=torch.zeros(2, 4, 5, 2)), "rgb"), (dict(rgb=torch.zeros(2, 4, 5, 3).long()), "rgb")):
        with pytest.raises(ValueError, match=match):
            call("integrate", **bad)
    with pytest.raises(ValueError, match="colours"):
        call("integrate", vol=SparseStub(colours=False))
    for bad, match in ((dict(level=math.nan), "level"), (dict(min_weight=0), "min_weight"), (dict(min_weight=math.nan), "min_weight"),
                       (dict(max_vertices=-1), "max_vertices"), (dict(max_faces=1.5), "max_faces"), (dict(max_faces=1 << 31), "max_faces")):
        with pytest.raises(ValueError, match=match):
            SparseStub().extract(**bad)
    with pytest.raises(ValueError, match="max_bytes is 39"):             # marks and table alone take 8 * 5 bytes
        SparseStub().allocate(max_bytes=39)
    empty = SparseStub().extract()                                             # zero blocks: no launch, an empty mesh
    assert empty["counts"] == (0, 0) and tuple(empty["vertices"].shape) == (0, 3) and tuple(empty["faces"].shape) == (0, 3)
    assert tuple(empty["rgb8"].shape) == (0, 3) and SparseStub(colours=False).extract()["rgb8"] is None
    assert SparseStub().nbytes == 40 and V.bytes_for((2, 2, 2), 3, True) == 40 + 3 * (12 + 512 * 20) and V.bytes_for((1, 1, 1), 1, False) == 5 + 12 + 4096


def test_scene_mesh_sparse_refusals_on_a_cpu_scene(monkeypatch):
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    need = 3 * 3 * 3 * 5                                                 # 21 points per axis: three blocks
    with pytest.raises(ValueError, match=f"{need} bytes"):
        mesh.scene_mesh(lt, W, H, voxel=0.1, bounds=box, sparse=True, max_bytes=need - 1)
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.scene_mesh(lt, W, H, voxel=1e-6, bounds=box, sparse=True)
    for kw, match in ((dict(voxel=0.0), "voxel"), (dict(voxel=0.1, trunc=-1.0), "trunc"), (dict(voxel=0.1, depth_range=(2, 1)), "depth_range"),
                      (dict(voxel=0.1, min_weight=0), "min_weight"), (dict(voxel=0.1, bounds=((1, 0, 0), (0, 1, 1))), "bounds")):
        with pytest.raises(ValueError, match=match):
            mesh.scene_mesh(lt, W, H, sparse=True, **kw)
    fov = lt.fov
    lt.fov = 360
    with pytest.raises(ValueError, match="pinhole"):
        mesh.scene_mesh(lt, W, H, voxel=0.1, sparse=True)
    lt.fov = fov
    with pytest.raises(ValueError, match="2\\^31"):                       # 2001 points per axis: dense refuses the lattice,
        mesh.scene_mesh(lt, W, H, voxel=1e-3, bounds=box)
    with pytest.raises(NativeError):                                    # sparse takes it and reaches the device check
        mesh.scene_mesh(lt, W, H, voxel=1e-3, bounds=box, sparse=True)


def test_block_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, NEW)
    assert "typedef struct LrfTsdfBlocks" in header
    assert C.sizeof(N.LrfTsdfBlocks) == 6 * 8 + 4 * 4 + 5 * 4 + 4        # padded to 8
    assert C.sizeof(N.LrfTsdfVolume) == 3 * 8 + 3 * 4 + 5 * 4 and C.sizeof(N.LrfMeshExtract) == 3 * 8 + 3 * 4 + 6 * 4 + 4
    assert built_lib.lrf_abi_version() == 7 and "#define LRF_ABI_VERSION 7" in header
    ws = built_lib.lrf_tsdf_blocks_assign_workspace_bytes
    assert ws(0, 4, 5) == 0 and ws(4, -1, 5) == 0 and ws(2048, 2048, 512) == 0 and ws(1 << 28, 1, 1) == 0 and ws(1 << 16, 1 << 16, 1) == 0
    assert ws(1, 1, 1) == 256 and ws(256, 256, 256) == 4 * 256 ** 3 // 256
    wm = built_lib.lrf_mesh_extract_blocks_workspace_bytes
    assert wm(-1) == 0 and wm(1 << 22) == 0 and wm(0) == 256 and wm(3) >= 3 * 512 * 4 + 2 * 6 * 4
    grid = "need Bx, By, Bz >= 1, 8 B < 2^31 per axis and Bx By Bz < 2^31"

    def volume(over):
        return filled(N.LrfTsdfBlocks, dict(marks=FAKE, table=FAKE, coords=FAKE, tsdf=FAKE, weight=FAKE, rgb=FAKE, Bx=3, By=4, Bz=5, n_blocks=2,
                                            voxel=0.1, trunc=0.3), **over)

    def touch(depth=FAKE, c2w=FAKE, focal=FAKE, center=FAKE, V=2, H=4, W=5, d_min=0.0, d_max=math.inf, **over):
        return refused(built_lib, built_lib.lrf_tsdf_blocks_touch(C.byref(volume(over)), depth, c2w, focal, center, V, H, W, d_min, d_max, None))

    def integrate(depth=FAKE, rgb8=FAKE, c2w=FAKE, focal=FAKE, center=FAKE, V=2, H=4, W=5, d_min=0.0, d_max=math.inf, **over):
        return refused(built_lib, built_lib.lrf_tsdf_blocks_integrate(C.byref(volume(over)), depth, rgb8, c2w, focal, center, V, H, W, d_min,
                                                                        d_max, None))

    def assign(max_blocks=10, cap=10, count=FAKE, wsp=FAKE, **over):
        return refused(built_lib, built_lib.lrf_tsdf_blocks_assign(C.byref(volume(over)), max_blocks, cap, count, wsp, None))

    def extract(level=0.0, min_weight=1.0, max_v=10, max_f=10, vertices=FAKE, rgb8_out=FAKE, faces=FAKE, counts=FAKE, wsp=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_extract_blocks(C.byref(volume(over)), level, min_weight, max_v, max_f, vertices, rgb8_out,
                                                                      faces, counts, wsp, None))
    for fn, name in ((touch, "lrf_tsdf_blocks_touch"), (integrate, "lrf_tsdf_blocks_integrate"), (assign, "lrf_tsdf_blocks_assign"),
                     (extract, "lrf_mesh_extract_blocks")):
        for bad in (dict(Bx=0), dict(By=-1), dict(Bz=0), dict(Bx=2048, By=2048, Bz=512), dict(Bx=1 << 28, By=1, Bz=1)):
            assert fn(**bad) == f"{name}: {grid}", bad
        for bad in (dict(n_blocks=-1), dict(n_blocks=1 << 22)):
            assert "512 n_blocks < 2^31" in fn(**bad)
        for bad in (dict(table=None), dict(coords=None)):
            assert fn(**bad) == f"{name}: null argument", bad
        assert "voxel" in fn(voxel=0.0) and "voxel" in fn(voxel=math.nan) and "voxel" in fn(voxel=-1.0)
        assert "trunc" in fn(trunc=0.0) and "trunc" in fn(trunc=-1.0) and "trunc" in fn(trunc=math.nan)
        assert "4-byte aligned" in fn(table=FAKE + 2) and "4-byte aligned" in fn(coords=FAKE + 1)
    for fn, name in ((touch, "lrf_tsdf_blocks_touch"), (integrate, "lrf_tsdf_blocks_integrate")):
        for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(V=1 << 20, H=1 << 10, W=2)):
            assert "need V, H, W >= 1 and V H W < 2^31" in fn(**bad)
        for bad in (dict(depth=None), dict(c2w=None), dict(focal=None), dict(center=None)):
            assert fn(**bad) == f"{name}: null argument", bad
        assert "d_min <= d_max" in fn(d_min=2.0, d_max=1.0) and "d_min <= d_max" in fn(d_min=math.nan)
        assert "4-byte aligned" in fn(depth=FAKE + 1) and "4-byte aligned" in fn(focal=FAKE + 2)
    assert touch(marks=None) == "lrf_tsdf_blocks_touch: null argument" and assign(marks=None) == "lrf_tsdf_blocks_assign: null argument"
    for fn, name in ((integrate, "lrf_tsdf_blocks_integrate"), (extract, "lrf_mesh_extract_blocks")):
        for bad in (dict(tsdf=None), dict(weight=None)):
            assert fn(**bad) == f"{name}: null argument", bad
        assert "4-byte aligned" in fn(tsdf=FAKE + 2) and "4-byte aligned" in fn(rgb=FAKE + 1)
    assert "go together" in integrate(rgb=None) and "go together" in integrate(rgb8=None)
    assert "go together" in extract(rgb=None) and "go together" in extract(rgb8_out=None)
    for bad in (dict(count=None), dict(wsp=None)):
        assert assign(**bad) == "lrf_tsdf_blocks_assign: null argument", bad
    assert "max_blocks" in assign(max_blocks=-1) and "max_blocks" in assign(max_blocks=1 << 22)
    assert "[0, 2^31)" in assign(cap=-1) and "[0, 2^31)" in assign(cap=1 << 31)
    assert "8-byte aligned" in assign(count=FAKE + 4) and "4-byte aligned" in assign(wsp=FAKE + 2)
    for bad in (dict(vertices=None), dict(faces=None), dict(counts=None), dict(wsp=None)):
        assert extract(**bad) == "lrf_mesh_extract_blocks: null argument", bad
    assert "level" in extract(level=math.nan) and "min_weight" in extract(min_weight=0.0) and "min_weight" in extract(min_weight=math.nan)
    assert "[0, 2^31)" in extract(max_v=-1) and "[0, 2^31)" in extract(max_f=1 << 31)
    assert "4-byte aligned" in extract(vertices=FAKE + 2) and "4-byte aligned" in extract(wsp=FAKE + 1)
    assert "8-byte aligned" in extract(counts=FAKE + 4)
    assert built_lib.lrf_tsdf_blocks_touch(None, FAKE, FAKE, FAKE, FAKE, 2, 4, 5, 0.0, 1.0, None) != 0
    assert built_lib.lrf_tsdf_blocks_assign(None, 1, 1, FAKE, FAKE, None) != 0
    assert built_lib.lrf_tsdf_blocks_integrate(None, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 4, 5, 0.0, 1.0, None) != 0
    assert built_lib.lrf_mesh_extract_blocks(None, 0.0, 1.0, 1, 1, FAKE, FAKE, FAKE, FAKE, FAKE, None) != 0


def test_block_kernels_use_no_scratch_and_keep_the_pose_in_scalar_registers():
    """The six new kernels as __graft_entry__.build() compiles them: no scratch; the integration's frame loop reads the camera
    matrix with scalar loads."""
    import re
    from isa_util import assert_no_scratch, device_asm
    found = assert_no_scratch(device_asm(), (r"k_blocks_touch", r"k_blocks_flag", r"k_blocks_assign", r"k_blocks_fuse", r"k_blocks_count",
                                             r"k_blocks_emit"), match="search", total=6, body_too=True)
    fuse = found[3][1]
    assert re.search(r"s_load_dwordx(4|8)", fuse)
