"""The block-sparse TSDF volume on the MI355X (csrc/lrf_tsdf_blocks.inl through localrf_amd.mesh.SparseTsdfVolume): touch, assign,
integrate and extract against the numpy restatement of tests/sparse_mesh_cases.py bit for bit and order included, the pools
against the device TsdfVolume under the block mask, incremental use, reproducibility, a side stream, capacity handling and
scene_mesh(sparse=True)."""

import numpy as np
import pytest
import torch

from localrf_amd import mesh, novel_views
from mesh_cases import H_ANALYTIC, closed_manifold_euler, sphere_field
from mesh_util import DEV, record_launches, same_mesh, to_dev
from novel_views_cases import scene
from sparse_mesh_cases import (assign_host, dims_of, extract_blocks_host, face_keys, integrate_blocks_host, lattice_for, new_sparse,
                               random_frames, spread_lattice, touch_host, trajectory)

pytestmark = pytest.mark.gpu
BIG = {(5, 4, 6): lattice_for((5, 4, 6), 0.06, (0.1, 0.0, -3.2)), (10, 8, 10): lattice_for((10, 8, 10), 0.04, (0.1, 0.0, -3.0))}


def _lat(blocks):
    return BIG.get(blocks) or spread_lattice(blocks)


def _frames_for(blocks):
    """(name, case, depth range, colours) per grid: clean and floater trajectories, random frames, a frame standing inside the
    volume, depth ranges that bite.  The four small grids take every case with and without colours.  The numpy restatement is
    what costs the time, so (5,4,6) takes the trajectories, the biting range and the inside frame with ONE colour setting each
    (clean, biting, inside: with; floaters, inside at the biting range: without) and leaves out the other random frames, and
    (10,8,10) takes the two trajectories only (clean with colours, floaters without): the random frames, the inside frame and
    the biting ranges run on the five smaller grids, whose kernels and code paths are the same."""
    big = blocks in BIG
    cases = [("clean", trajectory(True), (0.0, np.inf), (True,) if big else (True, False)),
             ("floaters", trajectory(False), (0.0, np.inf), (False,) if big else (True, False))]
    if blocks != (10, 8, 10):
        cases.append(("floaters, biting range", trajectory(False), (3.0, 3.9), (True,) if big else (True, False)))
        for V, H, W, inside in ((3, 17, 23, True),) if big else ((1, 17, 23, False), (3, 17, 23, True), (3, 48, 64, False)):
            c = random_frames(V, H, W, inside)
            cases.append((f"random V={V} {H}x{W}", c, c["depth_range"], (True,) if big else (True, False)))
            cases.append((f"random V={V} {H}x{W}, biting range", c, (2.8, 3.3), (False,) if big else (True, False)))
    return [(f"{name}, {'colours' if col else 'no colours'}", case, rng, col) for name, case, rng, cols in cases for col in cols]


def _args(case, colours, i0=0, i1=None):
    return dict(depth=case["depth"][i0:i1], c2w=case["c2w"][i0:i1], rgb8=case["rgb8"][i0:i1] if colours else None,
                f=case["f"], cx=case["cx"], cy=case["cy"])


def _touch(vol, a, rng):
    vol.touch(to_dev(a["depth"]), to_dev(a["c2w"]), float(a["f"]), (float(a["cx"]), float(a["cy"])), depth_range=rng)


def _integrate(vol, a, rng):
    vol.integrate(to_dev(a["depth"]), to_dev(a["c2w"]), float(a["f"]), (float(a["cx"]), float(a["cy"])),
                  rgb=None if a["rgb8"] is None else to_dev(a["rgb8"]), depth_range=rng)


def _fuse_device(blocks, case, rng, colours):
    origin, voxel, trunc = _lat(blocks)
    vol = mesh.SparseTsdfVolume(origin, voxel, blocks, trunc, DEV, colours=colours)
    a = _args(case, colours)
    _touch(vol, a, rng)
    vol.allocate()
    _integrate(vol, a, rng)
    return vol


def _same_state(vol, sv, pools=True):
    assert np.array_equal(vol.marks.cpu().numpy(), sv["marks"])
    assert np.array_equal(vol.table.cpu().numpy(), sv["table"])
    assert vol.n_blocks == sv["coords"].shape[0] and np.array_equal(vol.coords.cpu().numpy(), sv["coords"])
    if pools:
        for k in ("tsdf", "weight", "rgb"):
            got = getattr(vol, k)
            if sv[k] is None:
                assert got is None
                continue
            assert tuple(got.shape) == sv[k].shape and np.array_equal(got.cpu().numpy().view(np.uint32), sv[k].view(np.uint32)), k


def _keys(m):
    return face_keys({"vertices": m["vertices"].cpu().numpy(), "faces": m["faces"].cpu().numpy()})


def _dense_device(blocks, case, rng, colours, i0=0, i1=None):
    origin, voxel, trunc = _lat(blocks)
    ref = mesh.TsdfVolume(origin, voxel, dims_of(blocks), trunc, DEV, colours=colours)
    a = _args(case, colours, i0, i1)
    ref.integrate(to_dev(a["depth"]), to_dev(a["c2w"]), float(a["f"]), (float(a["cx"]), float(a["cy"])),
                  rgb=None if a["rgb8"] is None else to_dev(a["rgb8"]), depth_range=rng)
    return ref


def _pools_equal_dense(vol, ref, stored=None):
    """The stored points (or those of `stored`) hold the device TsdfVolume's bits."""
    t, w, c, mask = vol.to_dense()
    mask = mask if stored is None else stored
    for got, want in ((t, ref.tsdf), (w, ref.weight), (c, ref.rgb)):
        assert (got is None) == (want is None)
        if got is not None:
            assert torch.equal(got[mask].view(torch.int32), want[mask].view(torch.int32))
    return mask


@pytest.mark.parametrize("blocks", [(1, 1, 1), (2, 2, 2), (3, 2, 2), (5, 1, 1), (5, 4, 6), (10, 8, 10)])
def test_every_stage_equals_the_restatement_bit_for_bit(blocks):
    origin, voxel, trunc = _lat(blocks)
    stored = faces = 0
    for name, case, rng, colours in _frames_for(blocks):
        a = _args(case, colours)
        sv = new_sparse(origin, voxel, blocks, trunc, colours)
        vol = mesh.SparseTsdfVolume(origin, voxel, blocks, trunc, DEV, colours=colours)
        touch_host(sv, a["depth"], a["c2w"], a["f"], a["cx"], a["cy"], rng)
        _touch(vol, a, rng)
        assert np.array_equal(vol.marks.cpu().numpy(), sv["marks"]) and vol.n_blocks == 0
        assert vol.allocate() == assign_host(sv)
        _same_state(vol, sv)                                             # new blocks: tsdf 1, weight 0, rgb 0
        integrate_blocks_host(sv, a["depth"], a["rgb8"], a["c2w"], a["f"], a["cx"], a["cy"], rng)
        _integrate(vol, a, rng)
        _same_state(vol, sv)
        assert vol.nbytes == mesh.SparseTsdfVolume.bytes_for(blocks, vol.n_blocks, colours)
        ref = _dense_device(blocks, case, rng, colours)
        mask = _pools_equal_dense(vol, ref)
        band = (ref.weight > 0) & (ref.tsdf < 1)
        assert not bool((band & ~mask).any())                           # every band point of the dense volume is stored
        dense = _keys(ref.extract())
        for kw in (dict(),) if blocks == (10, 8, 10) else (dict(), dict(level=0.1, min_weight=2.0)):
            got, want = vol.extract(**kw), extract_blocks_host(sv, **kw)
            same_mesh(got, want)
            if not kw:
                assert _keys(got) <= dense
                faces += want["counts"][1]
                print(f"{blocks} {name}: {vol.n_blocks} of {sv['marks'].size} blocks, mesh {want['counts']}, dense faces {len(dense)}")
        stored += vol.n_blocks
    assert stored > 0
    if min(blocks) >= 4:
        assert faces > 0


def test_a_depth_range_that_excludes_everything_stores_nothing(monkeypatch):
    blocks, case = (3, 2, 2), trajectory(True)
    origin, voxel, trunc = _lat(blocks)
    launched = record_launches(monkeypatch)
    vol = mesh.SparseTsdfVolume(origin, voxel, blocks, trunc, DEV)
    a = _args(case, True)
    _touch(vol, a, (100.0, 200.0))
    assert vol.allocate() == 0 and vol.n_blocks == 0 and int(vol.marks.sum()) == 0 and int((vol.table != -1).sum()) == 0
    _integrate(vol, a, (100.0, 200.0))
    m = vol.extract()
    assert m["counts"] == (0, 0) and tuple(m["vertices"].shape) == (0, 3) and tuple(m["faces"].shape) == (0, 3)
    assert tuple(m["rgb8"].shape) == (0, 3) and tuple(vol.tsdf.shape) == (0, 8, 8, 8) and tuple(vol.coords.shape) == (0, 3)
    assert launched == ["lrf_tsdf_blocks_touch", "lrf_tsdf_blocks_assign"]
    t, w, c, mask = vol.to_dense()
    assert bool((t == 1).all()) and bool((w == 0).all()) and bool((c == 0).all()) and not bool(mask.any())


def test_the_analytic_sphere_equals_the_dense_mesh():
    fld = sphere_field()
    o, blocks = (0.0, 0.0, 0.0), (3, 3, 3)
    sv = new_sparse(o, H_ANALYTIC, blocks, 3 * H_ANALYTIC, colours=False)
    sv["marks"][...] = 1
    assign_host(sv)
    sv["tsdf"] = np.ascontiguousarray(fld.reshape(3, 8, 3, 8, 3, 8).transpose(0, 2, 4, 1, 3, 5).reshape(27, 8, 8, 8))
    sv["weight"] = np.ones_like(sv["tsdf"])
    vol = mesh.SparseTsdfVolume(o, H_ANALYTIC, blocks, 3 * H_ANALYTIC, DEV, colours=False)
    vol.marks.fill_(1)
    assert vol.allocate() == 27
    vol.tsdf.copy_(to_dev(sv["tsdf"]))
    vol.weight.fill_(1.0)
    assert torch.equal(vol.to_dense()[0], to_dev(fld))
    got = vol.extract()
    same_mesh(got, extract_blocks_host(sv))
    assert closed_manifold_euler({"vertices": got["vertices"].cpu().numpy(), "faces": got["faces"].cpu().numpy()}) == 2
    assert _keys(got) == _keys(mesh.extract_mesh(to_dev(fld), o, H_ANALYTIC, 0.0))
    # a plane through every block, seen by every frame: the sparse mesh of the trajectory's clean depth equals the dense one
    vol = _fuse_device((5, 4, 6), trajectory(True), (0.0, np.inf), True)
    assert _keys(vol.extract()) == _keys(_dense_device((5, 4, 6), trajectory(True), (0.0, np.inf), True).extract())


def test_incremental_use():
    blocks, case, rng, k = (5, 4, 6), trajectory(False), (0.0, np.inf), 3
    origin, voxel, trunc = _lat(blocks)
    whole = _fuse_device(blocks, case, rng, True)
    # A: touch all frames, allocate, integrate 0..k and k..V: the bytes of one call
    a = mesh.SparseTsdfVolume(origin, voxel, blocks, trunc, DEV)
    _touch(a, _args(case, True), rng)
    a.allocate()
    _integrate(a, _args(case, True, 0, k), rng)
    _integrate(a, _args(case, True, k, None), rng)
    assert torch.equal(a.table, whole.table) and torch.equal(a.coords, whole.coords)
    for name in ("tsdf", "weight", "rgb"):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(whole, name).view(torch.int32)), name
    # B: touch 0..k, allocate, integrate 0..k, touch k..V, allocate, integrate k..V
    b = mesh.SparseTsdfVolume(origin, voxel, blocks, trunc, DEV)
    sv = new_sparse(origin, voxel, blocks, trunc)
    news = []
    for i0, i1 in ((0, k), (k, None)):
        part = _args(case, True, i0, i1)
        _touch(b, part, rng)
        touch_host(sv, part["depth"], part["c2w"], part["f"], part["cx"], part["cy"], rng)
        first = b.coords.clone()
        news.append(b.allocate())
        assert news[-1] == assign_host(sv)
        assert torch.equal(b.coords[:first.shape[0]], first)            # the first blocks keep their indices
        _integrate(b, part, rng)
        integrate_blocks_host(sv, part["depth"], part["rgb8"], part["c2w"], part["f"], part["cx"], part["cy"], rng)
        _same_state(b, sv)
    n0 = news[0]
    assert n0 > 0 and news[1] > 0 and b.n_blocks == n0 + news[1]
    assert torch.equal(b.marks, whole.marks) and b.n_blocks == whole.n_blocks
    t, w, c, mask = b.to_dense()
    early = torch.zeros_like(mask)
    for bx, by, bz in b.coords[:n0].tolist():
        early[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = True
    _pools_equal_dense(b, _dense_device(blocks, case, rng, True), stored=early)             # the first blocks saw every frame
    _pools_equal_dense(b, _dense_device(blocks, case, rng, True, k, None), stored=mask & ~early)   # the appended ones frames k..V
    same_mesh(b.extract(), extract_blocks_host(sv))


def test_two_runs_are_equal_and_a_side_stream_gives_the_same():
    blocks, case, rng = (5, 4, 6), trajectory(False), (0.0, np.inf)
    a, b = _fuse_device(blocks, case, rng, True), _fuse_device(blocks, case, rng, True)
    ma, mb = a.extract(), b.extract()
    assert ma["counts"][1] > 0
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = _fuse_device(blocks, case, rng, True)
        mc = c.extract()
    side.synchronize()
    for other, mo in ((b, mb), (c, mc)):
        for k in ("marks", "table", "coords"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
        for k in ("tsdf", "weight", "rgb"):
            assert torch.equal(getattr(a, k).view(torch.int32), getattr(other, k).view(torch.int32)), k
        assert mo["counts"] == ma["counts"]
        assert torch.equal(ma["vertices"].view(torch.int32), mo["vertices"].view(torch.int32))
        assert torch.equal(ma["faces"], mo["faces"]) and torch.equal(ma["rgb8"], mo["rgb8"])


def test_capacity_one_too_small_raises_with_the_true_counts():
    vol = _fuse_device((5, 4, 6), trajectory(True), (0.0, np.inf), True)
    want = vol.extract()
    nv, nf = want["counts"]
    assert nv > 0 and nf > 0
    for caps in ((nv, nf), (nv + 100, None)):
        got = vol.extract(max_vertices=caps[0], max_faces=caps[1])
        assert got["counts"] == (nv, nf) and all(torch.equal(got[k], want[k]) for k in ("vertices", "faces", "rgb8"))
    for cap_v, cap_f in ((nv - 1, nf), (nv, nf - 1), (5, 7), (0, 0)):
        with pytest.raises(ValueError, match=f"holds {nv} vertices and {nf} faces") as ei:
            vol.extract(max_vertices=cap_v, max_faces=cap_f)
        part = ei.value.partial                                         # the rows inside capacity are the mesh's first rows
        assert part["counts"] == (nv, nf)
        assert torch.equal(part["vertices"], want["vertices"][:cap_v]) and torch.equal(part["faces"], want["faces"][:cap_f])
    # the pools of a volume that would pass max_bytes are not allocated, and the volume stays as it was
    origin, voxel, trunc = _lat((5, 4, 6))
    tight = mesh.SparseTsdfVolume(origin, voxel, (5, 4, 6), trunc, DEV)
    _touch(tight, _args(trajectory(True), True), (0.0, np.inf))
    need = mesh.SparseTsdfVolume.bytes_for((5, 4, 6), vol.n_blocks, True)
    with pytest.raises(ValueError, match=f"{vol.n_blocks} blocks takes {need} bytes"):
        tight.allocate(max_bytes=need - 1)
    assert tight.n_blocks == 0 and int((tight.table != -1).sum()) == 0
    assert tight.allocate(max_bytes=need) == vol.n_blocks and torch.equal(tight.table, vol.table)


def test_scene_mesh_sparse_equals_the_four_stages_over_render_poses():
    lt, g = scene(DEV)
    W, H = int(g["W"]), int(g["H"])
    F = len(lt.r_c2w)
    rng = (0.05, 50.0)
    with torch.no_grad():
        own = lt.get_cam2world().detach()
    out = novel_views.render_poses(lt, own, W, H, frame_indices=list(range(F)), floater_thresh=0.5)
    from localrf_amd import pointcloud
    xyz = pointcloud.fuse_points(None, out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=rng)["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 28
    got = mesh.scene_mesh(lt, W, H, voxel=voxel, floater_thresh=0.5, depth_range=rng, frames_per_call=2, sparse=True)
    vol = got["volume"]
    assert isinstance(vol, mesh.SparseTsdfVolume) and vol.trunc == 3 * voxel
    assert np.allclose(vol.origin, lo - vol.trunc, rtol=0, atol=1e-12)  # the box of fuse_points, grown by trunc
    top = np.array(vol.origin) + (np.array(vol.dims) - 1) * voxel
    assert (top >= hi + vol.trunc - 1e-9).all() and (top < hi + vol.trunc + 8 * voxel).all()   # rounded up to whole blocks
    ref = mesh.SparseTsdfVolume(vol.origin, voxel, vol.blocks, vol.trunc, DEV)
    ref.touch(out["depth"], own, lt.focal(W), lt.center(W, H), depth_range=rng)
    ref.allocate()
    ref.integrate(out["depth"], own, lt.focal(W), lt.center(W, H), rgb=out["rgb8"], depth_range=rng)
    for k in ("marks", "table", "coords"):
        assert torch.equal(getattr(vol, k), getattr(ref, k)), k
    for k in ("tsdf", "weight", "rgb"):
        assert torch.equal(getattr(vol, k).view(torch.int32), getattr(ref, k).view(torch.int32)), k
    want = ref.extract()
    print(f"scene_mesh sparse: {vol.blocks} blocks, {vol.n_blocks} stored, {got['counts']} vertices / faces")
    assert got["counts"] == want["counts"] and got["counts"][0] > 0 and got["counts"][1] > 0
    for k in ("vertices", "faces", "rgb8"):
        assert torch.equal(got[k], want[k]), k
    # bounds whose lattice is a whole number of blocks: the sparse faces are faces of the dense mesh
    box = (tuple(vol.origin), tuple(np.array(vol.origin) + (np.array(vol.dims) - 1) * voxel - 1e-9 * voxel))
    dense = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=box, floater_thresh=0.5, depth_range=rng)
    again = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=box, floater_thresh=0.5, depth_range=rng, sparse=True)
    assert dense["volume"].dims == again["volume"].dims == vol.dims
    assert again["counts"][1] > 0 and _keys(again) <= _keys(dense)
    assert torch.equal(again["vertices"], got["vertices"]) and torch.equal(again["faces"], got["faces"])
    # a virtual lattice above 2^31 points, nearly all of it air: dense refuses it, sparse returns the mesh under a max_bytes
    # that the table and the pools fit under
    mid = (lo + hi) / 2
    wide = (tuple(mid - 650 * voxel), tuple(mid + 650 * voxel))
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=wide, floater_thresh=0.5, depth_range=rng)
    big = mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=wide, floater_thresh=0.5, depth_range=rng, sparse=True, max_bytes=64 << 20)
    v = big["volume"]
    print(f"scene_mesh sparse, wide: {v.dims} points, {v.n_blocks} blocks, {v.nbytes} bytes, {big['counts']} vertices / faces")
    assert v.dims[0] * v.dims[1] * v.dims[2] > (1 << 31) and v.nbytes <= (64 << 20) and big["counts"][1] > 0
    with pytest.raises(ValueError, match="max_bytes"):                  # the table fits, the pools do not
        mesh.scene_mesh(lt, W, H, voxel=voxel, bounds=wide, floater_thresh=0.5, depth_range=rng, sparse=True,
                        max_bytes=mesh.SparseTsdfVolume.bytes_for(v.blocks, v.n_blocks, True) - 1)
