"""Depth quantiles on the GPU: the kernel alone against the numpy restatement of tests/quantile_cases.py bit for bit, the
field path against the restatement (bit for bit) and the fp64 oracle (the bound of test_quantile_host.py), the scene's blend,
and the two fusion entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import quantile_cases as Q
from localrf_amd import _native as N
from localrf_amd import depth_quantiles, mesh, novel_views, pointcloud
from normals_cases import field

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _from_weights(w, z, rays, q, want_index=True):
    """lrf_depth_quantiles_from_weights on numpy inputs -> (depth [K,R] fp32, index [K,R] int32) numpy."""
    wt, zt, rt = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (w, z, rays))
    R, S, K = wt.shape[0], wt.shape[1], len(q)
    depth = torch.full((K, R), -7.0, dtype=torch.float32, device=DEV)
    index = torch.full((K, R), -7, dtype=torch.int32, device=DEV) if want_index else None
    N.launch("lrf_depth_quantiles_from_weights", torch.device(DEV), N.ptr(wt), N.ptr(zt), N.ptr(rt), R, S, (C.c_float * K)(*q), K,
             N.ptr(depth), N.ptr(index))
    return depth.cpu().numpy(), None if index is None else index.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("S", [2, 63, 64, 65, 129, 4096])
@pytest.mark.parametrize("R", [1, 3, 200])
def test_kernel_alone_against_the_restatement(R, S, K):
    w, z, rays = Q.synthetic(R, S, seed=1000 + 7 * S + R)
    q = (0.5, 0.1, 0.9, 0.25)[:K]                                       # unsorted
    depth, index = _from_weights(w, z, rays, q)
    want_d, want_i = Q.restate(w, z, rays, q)
    assert np.array_equal(index, want_i)
    assert _same_bits(depth, want_d)
    assert (index >= 0).any()
    if K == 1:                                                          # the index is optional
        assert _same_bits(_from_weights(w, z, rays, q, want_index=False)[0], want_d)


@pytest.mark.parametrize("S", [2, 63, 64, 65, 129, 4096])
def test_kernel_alone_on_the_adversarial_rows(S):
    w, labels = Q.adversarial(S)
    _, z, rays = Q.synthetic(w.shape[0], S, seed=5)
    q = (0.9, 0.5)
    depth, index = _from_weights(w, z, rays, q)
    want_d, want_i = Q.restate(w, z, rays, q)
    assert np.array_equal(index, want_i) and _same_bits(depth, want_d)
    for r, (kind, j) in enumerate(labels):                              # and what the rows were built to give, for q = 0.5
        if kind in ("at", "tie"):
            assert index[1, r] == j and depth[1, r] > 0, (kind, j)
        elif kind == "late nan":
            assert index[1, r] == 0 and index[0, r] == -1 and depth[0, r] == 0
        else:
            assert index[1, r] == -1 and index[0, r] == -1 and depth[1, r] == 0 and not np.signbit(depth[1, r]), (kind, j)


@pytest.mark.parametrize("case", Q.FIELD_CASES)
def test_field_quantiles_against_restatement_and_oracle(case):
    f, rays, floater, n = Q.case_field(case, DEV)
    if case == "alpha_mask":
        f.updateAlphaMask((16, 16, 16))
        occ = float(f.alphaMask.alpha_volume.mean())
        assert 0.0 < occ < 1.0, occ                                     # the mask really culls
    rays = rays.to(DEV)
    q = (0.5, 0.25, 0.75)
    depth, acc, index = f.render_depth_quantiles(rays, q, N_samples=n, floater_thresh=floater, return_index=True)
    _, _, w, acc_w, z = f.render_weights(rays, N_samples=n, floater_thresh=floater)
    R = rays.shape[0]
    assert depth.shape == (3, R) and acc.shape == (R,) and index.shape == (3, R) and index.dtype is torch.int32
    assert torch.equal(acc.view(torch.int32), acc_w.view(torch.int32))  # bit for bit
    depth2, acc2 = f.render_depth_quantiles(rays, q, N_samples=n, floater_thresh=floater)
    assert torch.equal(depth.view(torch.int32), depth2.view(torch.int32)) and torch.equal(acc, acc2)    # two calls, the same bits
    wn, zn, rn = w.cpu().numpy(), z.view(-1).cpu().numpy(), rays.cpu().numpy()
    want_d, want_i = Q.restate(wn, zn, rn, q)
    assert np.array_equal(index.cpu().numpy(), want_i)
    assert _same_bits(depth.cpu().numpy(), want_d)
    Q.compare(case, wn, zn, rn, q, depth.cpu().numpy(), index.cpu().numpy())
    med, _ = f.render_depth_quantiles(rays, N_samples=n, floater_thresh=floater)    # the default: the median alone
    assert med.shape == (1, R) and torch.equal(med[0], depth[0])


def test_shapes_and_no_rays():
    f = field(DEV, 11)
    d, a = f.render_depth_quantiles(torch.zeros(0, 6, device=DEV), q=(0.5, 0.9))
    assert d.shape == (2, 0) and a.shape == (0,) and d.dtype is torch.float32
    with pytest.raises(ValueError, match=r"\[R, 6\]"):
        f.render_depth_quantiles(torch.zeros(4, 5, device=DEV))


def test_median_depth_sits_on_the_heaviest_sample_of_an_opaque_field():
    """A ray with one sample j of weight > 0.5 has C_{j-1} < 0.5 <= C_j whatever the rest holds: its median lies in the
    interval of sample j, where its expected depth is pulled towards the forced last sample."""
    f, rays, _, _ = Q.case_field("three_steps", DEV)                    # relu densities scaled until a ray ends within some twenty samples
    rays = rays.to(DEV)
    depth, acc, index = f.render_depth_quantiles(rays, return_index=True)
    _, _, w, _, z = f.render_weights(rays)
    z = z.view(-1)
    wmax, j = w.max(dim=1)
    sel = wmax > 0.5
    print(f"opaque field: {int(sel.sum())} of {rays.shape[0]} rays hold a sample of weight > 0.5")
    assert sel.any()
    dn = torch.linalg.vector_norm(rays[:, 3:6], dim=-1)
    lo, hi = z[j] / dn, z[(j + 1).clamp(max=z.shape[0] - 1)] / dn
    assert (index[0][sel].long() == j[sel]).all()
    assert ((depth[0] >= lo * (1 - 1e-6)) & (depth[0] <= hi * (1 + 1e-6)))[sel].all()


def _two_field_scene():
    """The two-field scene of the normals scene test: the golden scene's poses and blending weights over two fields of
    different grids (20x24x28 and 16^3)."""
    from novel_views_cases import scene
    lt, g = scene("cpu")
    f0 = field("cpu", 51)
    gen = torch.Generator().manual_seed(52)
    with torch.no_grad():
        for p in list(lt.tensorfs[1].density_plane) + list(lt.tensorfs[1].density_line):
            p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    lt.tensorfs[0] = f0
    lt = lt.to(DEV)
    lt.device = torch.device(DEV)
    for f in lt.tensorfs:
        f.to(DEV)
    return lt, g


SCENE_Q = (0.5, 1.0)                                                    # 1.0: the fp32 sum of a ray's weights may stop short of it


@pytest.fixture(scope="module")
def scene_case():
    lt, g = _two_field_scene()
    bw = lt._blending_host()
    both = [v for v in range(bw.shape[0]) if bw[v, 0] > 0 and bw[v, 1] > 0]
    assert both, "the scene has no frame blended from fields 0 and 1"
    W, H = 24, 16
    c2w = lt.get_cam2world().detach()
    views = [both[0], both[-1], both[0]]
    poses = c2w[views].clone()
    poses[2, :, 3] += 0.05                                              # a third, novel pose
    out = depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=SCENE_Q, frame_indices=views, chunk=W * H * 3)
    return lt, poses, views, W, H, out


def _assert_the_blend_of_the_fields(lt, poses, views, W, H, out, q):
    """-> the mask [K, 3, H W] of the pixels no field crosses."""
    from localrf_amd.scene_ops import scene_rays
    K = len(q)
    assert out["depth"].shape == (K, 3, H, W) and out["acc"].shape == (3, H, W)
    bw = lt.blending_weights.detach()
    dsum = torch.zeros(K, 3, H * W, device=DEV)
    wsum = torch.zeros(K, 3, H * W, device=DEV)
    want_a = torch.zeros(3, H * W, device=DEV)
    ids = torch.arange(H * W, dtype=torch.int64, device=DEV)
    overlapping = 0
    for i, v in enumerate(views):
        active = torch.nonzero(bw[v])[:, 0].tolist()
        overlapping += len(active) > 1
        with torch.no_grad():
            rays, _, _ = scene_rays(ids, poses[i:i + 1], lt._shifts(lt.world2rf, active), lt.focal(W), lt.center(W, H), H * W, W, H)
        for k, rf in enumerate(active):
            d_k, a_k, i_k = lt.tensorfs[rf].render_depth_quantiles(rays[k], q, return_index=True)
            found = (i_k >= 0).float()
            assert (d_k[i_k < 0] == 0).all()
            dsum[:, i] += bw[v, rf] * d_k
            wsum[:, i] += bw[v, rf] * found
            want_a[i] += bw[v, rf] * a_k
    assert overlapping >= 2
    want = torch.where(wsum > 0, dsum / wsum, torch.zeros_like(dsum))
    got = out["depth"].view(K, 3, -1)
    none = wsum == 0
    print(f"scene: pixels no field crosses: {none.sum(dim=(1, 2)).tolist()} of {3 * H * W} per quantile; max depth {float(want.max()):.3e}")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))   # exactly
    assert float((out["acc"].view(3, -1) - want_a).abs().max()) <= 1e-6
    assert (got[none] == 0).all() and (got[~none] > 0).all()              # a pixel no field crosses is exactly 0
    return none


def test_scene_quantiles_are_the_blend_of_the_fields(scene_case):
    lt, poses, views, W, H, out = scene_case
    none = _assert_the_blend_of_the_fields(lt, poses, views, W, H, out, SCENE_Q)
    assert none[1].any()
    med = depth_quantiles.median_depth(lt, poses, W, H, frame_indices=views)
    assert med.shape == (3, H, W) and torch.equal(med, out["depth"][0])


def test_scene_quantiles_over_an_active_set_with_a_gap():
    """Active fields that are not adjacent, (0, 2) and (1, 3): the same restatement at the same bounds, whatever the chunk."""
    from novel_views_cases import gap_case
    lt, poses, views, W, H, _ = gap_case(DEV)
    q = (0.25, 0.5)
    out = depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=q, frame_indices=views, chunk=W * H * 3)
    none = _assert_the_blend_of_the_fields(lt, poses, views, W, H, out, q)
    assert not none.all()
    small = depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=q, frame_indices=views, chunk=7)
    assert torch.equal(small["depth"].view(torch.int32), out["depth"].view(torch.int32)) and torch.equal(small["acc"], out["acc"])


@pytest.mark.parametrize("chunk", [7, 64])
def test_scene_quantiles_do_not_depend_on_the_chunk(scene_case, chunk):
    lt, poses, views, W, H, out = scene_case
    again = depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=SCENE_Q, frame_indices=views, chunk=chunk)
    assert torch.equal(again["depth"].view(torch.int32), out["depth"].view(torch.int32)) and torch.equal(again["acc"], out["acc"])


def _spread_expression(lt, poses, views, W, H, max_spread):
    d = depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=(0.25, 0.5, 0.75), frame_indices=views)["depth"]
    drop = ((d[2] - d[0]) > max_spread * d[1]) | (d[0] <= 0) | (d[1] <= 0) | (d[2] <= 0)
    return torch.where(drop, torch.zeros_like(d[1]), d[1]), drop, d


def test_point_cloud_from_median_depth(scene_case):
    lt, poses, views, W, H, _ = scene_case
    kw = dict(poses=poses, frame_indices=views, depth_range=(0.0, 1e4))
    plain = pointcloud.scene_point_cloud(lt, W, H, **kw)
    same = pointcloud.scene_point_cloud(lt, W, H, depth="expected", **kw)
    assert same["count"] == plain["count"] > 0
    for key in ("xyz", "rgb8", "src"):
        assert torch.equal(same[key], plain[key]), key                  # the default: today's bits
    rp = novel_views.render_poses(lt, poses, W, H, frame_indices=views)
    md = depth_quantiles.median_depth(lt, poses, W, H, frame_indices=views)
    fuse = dict(depth_range=(0.0, 1e4))
    want = pointcloud.fuse_points(rp["rgb8"], md, poses, lt.focal(W), lt.center(W, H), **fuse)
    got = pointcloud.scene_point_cloud(lt, W, H, depth="median", **kw)
    assert got["count"] == want["count"] > 0
    for key in ("xyz", "rgb8", "src"):
        assert torch.equal(got[key], want[key]), key
    assert not torch.equal(md, rp["depth"])
    _, _, d = _spread_expression(lt, poses, views, W, H, 0.0)
    ms = float(((d[2] - d[0]) / d[1]).flatten().nanmedian())               # a threshold that splits the pixels
    expr, drop, _ = _spread_expression(lt, poses, views, W, H, ms)
    assert drop.any() and not drop.all()
    want = pointcloud.fuse_points(rp["rgb8"], expr, poses, lt.focal(W), lt.center(W, H), **fuse)
    got = pointcloud.scene_point_cloud(lt, W, H, depth="median", max_spread=ms, **kw)
    print(f"max_spread {ms:.3f}: {int(drop.sum())} of {drop.numel()} pixels dropped, {got['count']} points")
    assert got["count"] == want["count"] == int((~drop & (expr <= 1e4)).sum())
    for key in ("xyz", "rgb8", "src"):
        assert torch.equal(got[key], want[key]), key
    kept = torch.zeros(3, H * W, dtype=torch.bool, device=DEV)
    kept[got["src"][:, 0].long(), got["src"][:, 1].long()] = True
    assert torch.equal(kept.view(3, H, W), ~drop & (expr <= 1e4))       # exactly the pixels the expression names


def test_mesh_from_median_depth(scene_case):
    lt, poses, views, W, H, _ = scene_case
    rng = (0.05, 1e4)
    rp = novel_views.render_poses(lt, poses, W, H, frame_indices=views)
    md = depth_quantiles.median_depth(lt, poses, W, H, frame_indices=views)
    xyz = pointcloud.fuse_points(None, md, poses, lt.focal(W), lt.center(W, H), depth_range=rng)["xyz"]
    lo, hi = xyz.amin(0).double().cpu().numpy(), xyz.amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 24
    kw = dict(voxel=voxel, bounds=(tuple(lo), tuple(hi)), poses=poses, frame_indices=views, depth_range=rng, frames_per_call=2)
    ms = 0.5
    expr, drop, _ = _spread_expression(lt, poses, views, W, H, ms)
    for depth, extra, src in (("expected", {}, rp["depth"]), ("median", {}, md), ("median", {"max_spread": ms}, expr)):
        got = mesh.scene_mesh(lt, W, H, depth=depth, **extra, **kw)
        vol = got["volume"]
        ref = mesh.TsdfVolume(vol.origin, voxel, vol.dims, vol.trunc, DEV)
        ref.integrate(src, poses, lt.focal(W), lt.center(W, H), rgb=rp["rgb8"], depth_range=rng)
        for k in ("tsdf", "weight", "rgb"):
            assert torch.equal(getattr(vol, k).view(torch.int32), getattr(ref, k).view(torch.int32)), (depth, extra, k)
        want = ref.extract()
        assert got["counts"] == want["counts"], (depth, extra)
        for k in ("vertices", "faces", "rgb8"):
            assert torch.equal(got[k], want[k]), (depth, extra, k)
        if depth == "expected":                                         # and the call without the argument: today's bits
            plain = mesh.scene_mesh(lt, W, H, **kw)
            assert plain["counts"] == got["counts"] and torch.equal(plain["vertices"], got["vertices"])
            assert torch.equal(plain["volume"].tsdf.view(torch.int32), vol.tsdf.view(torch.int32))
