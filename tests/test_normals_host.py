"""Normals without a GPU: the fp64 oracle against central differences, the exported symbols and their refusals, PLY files
with normals, the byte encoding's restatement, and the argument checks that come before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, refused
from localrf_amd import NativeError, normals, pointcloud
from normals_cases import (GRID, encode_normals_host, field, field_dict, flag_x, grad_x, density_of_x, sample_positions,
                           test_rays)



def test_fp64_oracle_agrees_with_central_differences():
    """autograd of density_feature(u(contract(x))) in fp64 against (g(x + h e) - g(x - h e)) / 2h, h = 1e-6, on the samples of
    256 rays x 32 distances that sit on no kink; the flagged ones stay a small share."""
    f = field("cpu", 3)
    fld = field_dict(f, torch.float64)
    z = torch.cat([torch.linspace(0.1, 1.1, 16), 1.0 / torch.linspace(1.0, 1e-3, 16) + 0.1])
    x = sample_positions(test_rays(256, 5), z, torch.float64).reshape(-1, 3)
    flagged, tie = flag_x(fld, x)
    assert int(flagged.sum()) <= 0.005 * x.shape[0], int(flagged.sum())
    g = grad_x(fld, x)
    h = 1e-6
    fd = torch.zeros_like(g)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        fd[:, a] = (density_of_x(fld, x + e) - density_of_x(fld, x - e)) / (2 * h)
    err = (g - fd).abs().max(-1).values
    print(f"flagged {int(flagged.sum())} of {x.shape[0]} (ties {int(tie.sum())}); max |autograd - central| unflagged "
          f"{float(err[~flagged].max()):.3e}; min |grad| {float(g.norm(dim=-1).min()):.3e}")
    assert (x.abs().amax(-1) > 1).any() and (x.abs().amax(-1) < 1).any()        # both sides of the contraction
    assert float(err[~flagged].max()) <= 1e-6


def test_normals_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    declared_exported_bound(built_lib, ("lrf_density_gradient", "lrf_normals_workspace_bytes", "lrf_render_normals"))
    assert built_lib.lrf_abi_version() == 7
    ws = built_lib.lrf_normals_workspace_bytes
    assert ws(0, 64) == 0 and ws(16, 1) == 0 and ws(16, 4097) == 0
    for R, S in ((1, 2), (200, 88), (4096, 512)):
        assert ws(R, S) >= built_lib.lrf_workspace_bytes(R, S) + 4 * R * S + 20 * R
        assert ws(R, S) <= built_lib.lrf_workspace_bytes(R, S) + 4 * R * S + 20 * R + 5 * 256
    fake = C.c_void_p(FAKE)
    fld = N.LrfField()
    fld.cache = FAKE
    fld.grid[:] = list(GRID)

    dg = built_lib.lrf_density_gradient
    assert refused(built_lib, dg(None, fake, 4, fake, None, None)) == "lrf_density_gradient: null argument"
    assert refused(built_lib, dg(C.byref(fld), None, 4, fake, None, None)) == "lrf_density_gradient: null argument"
    assert refused(built_lib, dg(C.byref(fld), fake, 4, None, None, None)) == "lrf_density_gradient: null argument"
    assert "0 <= P" in refused(built_lib, dg(C.byref(fld), fake, -1, fake, None, None))
    assert "4-byte aligned" in refused(built_lib, dg(C.byref(fld), fake, 4, C.c_void_p(0x10002), None, None))
    assert dg(C.byref(fld), fake, 0, fake, None, None) == 0              # no point: no launch

    def rn(f=C.byref(fld), rays=fake, z=fake, R=8, S=64, flags=1, bw=None, per_view=1, accumulate=0, out=fake, acc=None, wsp=fake):
        return refused(built_lib, built_lib.lrf_render_normals(f, rays, z, R, S, flags, 0.0, bw, per_view, accumulate, out, acc, wsp, None))
    for bad in (dict(f=None), dict(rays=None), dict(z=None), dict(out=None), dict(wsp=None)):
        assert rn(**bad) == "lrf_render_normals: null argument", bad
    for bad in (dict(R=0), dict(R=-3), dict(S=1), dict(S=4097)):
        assert "need R > 0 and 2 <= S <= 4096" in rn(**bad), bad
    assert "per_view" in rn(bw=fake, per_view=0)
    assert "accumulate" in rn(accumulate=2)
    assert "4-byte aligned" in rn(out=C.c_void_p(0x10002)) and "4-byte aligned" in rn(acc=C.c_void_p(0x10001))
    assert "256-byte aligned" in rn(wsp=C.c_void_p(0x10010))
    assert "unknown flag bits" in rn(flags=1 << 12)


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    return lines, [ln.split()[1:] for ln in lines if ln.startswith("property")], raw[end:], raw


def test_write_ply_with_normals(tmp_path):
    rng = np.random.default_rng(4)
    xyz = rng.normal(size=(41, 3)).astype(np.float32)
    nrm = rng.normal(size=(41, 3)).astype(np.float32)
    nrm[7] = 0.0
    rgb = rng.integers(0, 256, (41, 3), dtype=np.uint8)
    xyz_p = [["float", "x"], ["float", "y"], ["float", "z"]]
    nrm_p = [["float", "nx"], ["float", "ny"], ["float", "nz"]]
    rgb_p = [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    for cols in (rgb, None):
        path = str(tmp_path / "cloud.ply")
        n = pointcloud.write_ply(path, torch.from_numpy(xyz), None if cols is None else torch.from_numpy(cols),
                                 normals=torch.from_numpy(nrm))
        assert n == 41
        lines, props, payload, _ = _read_ply(path)
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 41"]
        assert props == xyz_p + nrm_p + (rgb_p if cols is not None else [])
        dt = np.dtype([("p", "<f4", 3), ("n", "<f4", 3)] + ([("c", "u1", 3)] if cols is not None else []))
        assert dt.itemsize == (27 if cols is not None else 24) and len(payload) == 41 * dt.itemsize
        rec = np.frombuffer(payload, dtype=dt)
        assert np.array_equal(rec["p"].view(np.uint32), xyz.view(np.uint32))
        assert np.array_equal(rec["n"].view(np.uint32), nrm.view(np.uint32))
        if cols is not None:
            assert np.array_equal(rec["c"], rgb)
    assert pointcloud.ply_header(3, True, normals=True).decode().count("property") == 9
    # without normals: today's bytes, spelled out
    for cols in (rgb, None):
        path = str(tmp_path / "plain.ply")
        pointcloud.write_ply(path, xyz, cols)
        head = ["ply", "format binary_little_endian 1.0", "element vertex 41", "property float x", "property float y",
                "property float z"] + (["property uchar red", "property uchar green", "property uchar blue"] if cols is not None else [])
        dt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if cols is not None else []))
        rec = np.empty(41, dtype=dt)
        rec["p"] = xyz
        if cols is not None:
            rec["c"] = rgb
        want = ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + rec.tobytes()
        assert open(path, "rb").read() == want
        assert pointcloud.ply_header(41, cols is not None) == pointcloud.ply_header(41, cols is not None, normals=False)
    with pytest.raises(ValueError, match="normals"):
        pointcloud.write_ply(str(tmp_path / "bad.ply"), xyz, rgb, normals=nrm[:5])
    with pytest.raises(ValueError, match="normals"):
        pointcloud.write_ply(str(tmp_path / "bad.ply"), xyz, normals=nrm[:, :2])


def test_normal_colours_match_the_numpy_restatement():
    """The float stage of encode_normals runs on any device; its bytes, formed by the numpy restatement of encode_frames'
    conversion, are pinned here on hand-computed cases: unit axes, a zero row, a tiny row under the 1e-8 clamp."""
    n = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, 0], [1, 1, 0], [1e-9, 0, 0], [-2, -2, -2]], np.float32)
    want = np.array([[255, 128, 128], [128, 0, 128], [128, 128, 255], [128, 128, 128], [218, 218, 128], [140, 128, 128],
                     [54, 54, 54]], np.uint8)
    assert np.array_equal(encode_normals_host(n), want)
    rng = np.random.default_rng(9)
    big = np.concatenate([n, rng.normal(size=(500, 3)).astype(np.float32) * np.float32(0.3)])
    cols = normals.normal_colours(torch.from_numpy(big)).numpy()
    from novel_views_cases import rgb8_host
    got, ref = rgb8_host(cols), encode_normals_host(big)
    # torch's and numpy's fp32 norms may differ in the last bit: a byte may move by one only where 255 x sits on a .5 tie
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1 and (got != ref).mean() < 0.01
    assert np.array_equal(got[:7], want)
    unit, length = normals.unit_normals(torch.from_numpy(n))
    assert torch.equal(unit[3], torch.zeros(3)) and float(length[0]) == 1.0


def test_refusals_before_any_launch():
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    F = len(lt.r_c2w)
    poses = torch.from_numpy(g["poses"])
    # CPU tensors
    f = field("cpu", 1)
    with pytest.raises(NativeError, match="no CPU fallback"):
        f.density_gradient(torch.zeros(4, 3))
    with pytest.raises(NativeError, match="no CPU fallback"):
        f.render_normals(torch.zeros(4, 6))
    with pytest.raises(TypeError):
        f.render_normals([[0.0] * 6])
    with pytest.raises(NativeError):
        normals.render_normals(lt, poses, W, H)
    with pytest.raises(NativeError, match="no CPU fallback"):
        normals.encode_normals(torch.zeros(1, 4, 5, 3))
    # wrong shapes
    with pytest.raises(ValueError, match="poses"):
        normals.render_normals(lt, torch.zeros(3, 2, 4), W, H)
    with pytest.raises(ValueError, match="W, H"):
        normals.render_normals(lt, poses, 0, H)
    with pytest.raises(ValueError, match="chunk"):
        normals.render_normals(lt, poses, W, H, chunk=0)
    with pytest.raises(ValueError, match=r"\[\.\.\., H, W, 3\]"):
        normals.encode_normals(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        normals.encode_normals(torch.zeros(1, 4, 5, 2))
    with pytest.raises(ValueError, match="floating-point"):
        normals.encode_normals(torch.zeros(1, 4, 5, 3, dtype=torch.int32))
    with pytest.raises(TypeError):
        normals.encode_normals(np.zeros((1, 4, 5, 3), np.float32))
    # the point cloud: normals keep 16 more bytes per pixel resident, counted before anything is rendered
    with pytest.raises(ValueError, match=f"{23 * F * H * W} bytes"):
        pointcloud.scene_point_cloud(lt, W, H, normals=True, max_bytes=23 * F * H * W - 1)
    with pytest.raises(ValueError, match=f"{23 * F * H * W} bytes"):
        pointcloud.scene_point_cloud(lt, W, H, normals=True, max_bytes=7 * F * H * W)     # enough without normals
    with pytest.raises(ValueError, match="orient"):
        pointcloud.scene_point_cloud(lt, W, H, orient=True)
    with pytest.raises(NativeError):                                     # valid arguments, CPU scene
        pointcloud.scene_point_cloud(lt, W, H, normals=True, max_bytes=23 * F * H * W)
