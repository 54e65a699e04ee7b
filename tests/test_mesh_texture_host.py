"""The texture bake without a GPU: the layout, properties of the numpy restatement of csrc/lrf_mesh_texture.inl
(tests/mesh_texture_cases.py) -- agreement with an independent fp64 baker, the round trip through the restated rasteriser --,
write_obj, argument refusals before any native call (Python and C ABI), the new symbols, the state size and the kernels'
scratch use.

Measured with the committed restatement.  Against the fp64 baker: no atlas byte differs by more than 1 level and no mask bit
differs outside the texels that sit on a decision, and at most 0.45 % of a case's used texels sit on one (sphere, patch 8; the
cap is 2 %).  The round trip (bar G (s + 1) + 2 levels with G = 10.22 levels per pixel): sphere, frames 0 and 3: s = 1.17 and
1.16 pixels, bars 24.2 and 24.0, largest difference 2 and 2 levels; wall, frames 0, 1, 2: s = 2.41, 2.41, 2.59, bars 36.9, 36.9,
38.6, largest difference 6, 6 and 7 levels.  The GPU equals the restatement bit for bit (tests/test_gpu_mesh_texture.py), so
these are its figures too."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError
from localrf_amd.mesh_texture import TextureBaker, atlas_layout, face_uv, sample_texture, scene_texture, write_obj
from mesh_raster_cases import SPHERE_C, SPHERE_R, rasterize_host
from mesh_texture_cases import (CASE_NAMES, G_LEVELS, ROUND_TRIP, WALL_CAMERAS, WALL_Z, bake_case, bake_fp64, cases, expected, inputs,
                                layout_host, resolve_host, texels_host, uv_host)
from mesh_util import cpu_mesh, forbid_native, forbid_render

SYMBOLS = ("lrf_mesh_texture_state_bytes", "lrf_mesh_texture_bake", "lrf_mesh_texture_resolve")
KERNELS = ("k_tx_bake", "k_tx_resolve")
FP64_LEVELS, FP64_EXCLUDED = 1, 0.02


def test_the_cases_cover_the_sizes_counts_and_options():
    cs = cases().values()
    nf = {np.asarray(c["mesh"]["faces"]).reshape(-1, 3).shape[0] for c in cs}
    assert {0, 1, 2, 3, 38, 512} <= nf
    assert {c["P"] for c in cs} >= {4, 5, 8, 16}
    assert {(c["W"], c["H"]) for c in cs} >= {(1, 1), (5, 7), (64, 48)}
    assert {c["c2w"].shape[0] for c in cs} >= {1, 2, 3, 5}
    assert {c["blend"] for c in cs} == {"mean", "best"} and {c["two_sided"] for c in cs} == {False, True}
    assert any(c["cols"] == 1 for c in cs) and any(c["cols"] is None for c in cs)
    c = cases()["fan P5 cols 4 V3 mean"]                                   # cols does not divide n_cells: an empty cell
    assert 19 % c["cols"] and expected("fan P5 cols 4 V3 mean")["info"]["empty_texels"] >= c["P"] ** 2


def test_layout_formulas_and_uv():
    for nf in (0, 1, 2, 3, 7, 8, 9, 38, 512, 5100, 302638):
        for P in (4, 5, 8, 16, 64):
            for cols in (None, 1, 3, 700):
                rows, cl, Ht, Wt = atlas_layout(nf, P, cols)
                assert (rows, cl, Ht, Wt) == layout_host(nf, P, cols)
                cells = (nf + 1) // 2
                assert rows * cl >= cells and (rows - 1) * cl < max(cells, 1) and Ht == rows * P and Wt == cl * P
                if cols is None and cells:
                    assert cl * cl >= cells > (cl - 1) * (cl - 1)
    assert atlas_layout(0) == (0, 1, 0, 8)
    for nf, P, cols in ((1, 4, None), (3, 8, None), (38, 5, 4), (512, 16, 7)):
        uv = face_uv(nf, P, cols)
        assert uv.dtype is torch.float32 and tuple(uv.shape) == (nf, 3, 2)
        assert np.array_equal(uv.numpy().view(np.uint32), uv_host(nf, P, cols).view(np.uint32))
        assert (uv.numpy() > 0).all() and (uv.numpy() < 1).all()
    for bad in (3, 65, 8.5, True, None):
        with pytest.raises(ValueError, match="patch"):
            atlas_layout(4, bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="cols"):
            atlas_layout(4, 8, bad)
    for bad in (-1, 1 << 31, 1.5):
        with pytest.raises(ValueError, match="Nf"):
            atlas_layout(bad)
    with pytest.raises(ValueError, match="2\\^31 texels"):
        atlas_layout(1 << 21, 64)


@pytest.mark.parametrize("P", range(4, 65))
def test_bilinear_neighbours_stay_in_the_half_and_uv_round_trips(P):
    K = P - 3
    face, a, b = texels_host(2, P, 1)                                      # one cell: faces 0 and 1
    for f in (0, 1):
        for bb in range(K + 1):
            for aa in range(K + 1 - bb):                                   # the texels of the triangle
                # a sample inside the triangle whose floor is (aa, bb) reads the four taps from there; with aa + bb = K the
                # sample lies on the hypotenuse at a texel centre, and the other three taps have weight zero
                for db in ((0, 1) if aa + bb < K else (0,)):
                    for da in ((0, 1) if aa + bb < K else (0,)):
                        x, y = (aa + da, bb + db) if f == 0 else (P - 1 - aa - da, P - 1 - bb - db)
                        assert face[y, x] == f and (a[y, x], b[y, x]) == (aa + da, bb + db)
    nf, cols = 7, 3                                                        # barycentric -> atlas pixel -> (a, b) -> barycentric
    uv = uv_host(nf, P, cols).astype(np.float64)
    rows, cols, Ht, Wt = layout_host(nf, P, cols)
    face, a, b = texels_host(nf, P, cols)
    for f in range(nf):
        px = np.stack([uv[f, :, 0] * Wt, (1.0 - uv[f, :, 1]) * Ht], -1)    # the corners in atlas pixels
        for bb in range(K + 1):
            for aa in range(K + 1 - bb):
                w = np.array([1.0 - (aa + bb) / K, aa / K, bb / K])
                x, y = w @ px
                xi, yi = int(math.floor(x + 1e-4)), int(math.floor(y + 1e-4))
                assert abs(x - xi - 0.5) < 1e-3 and abs(y - yi - 0.5) < 1e-3          # a texel centre
                assert face[yi, xi] == f and (a[yi, xi], b[yi, xi]) == (aa, bb)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_shapes_counts_and_empty_texels(name):
    c, e = cases()[name], expected(name)
    nf = np.asarray(c["mesh"]["faces"]).reshape(-1, 3).shape[0]
    rows, cols, Ht, Wt = layout_host(nf, c["P"], c["cols"])
    assert e["state"].shape == (Ht, Wt, 4) and e["atlas"].shape == (Ht, Wt, 3) and e["mask"].shape == (Ht, Wt)
    info = e["info"]
    assert info["used_texels"] + info["empty_texels"] == Ht * Wt and info["observed_texels"] == int(e["mask"].sum())
    assert info["observed_texels"] + info["fallback_texels"] <= info["used_texels"]
    face = texels_host(nf, c["P"], c["cols"])[0] if nf else np.zeros((0, Wt), np.int64)
    assert not e["state"][face >= nf].any() and (e["atlas"][face >= nf] == np.asarray(c["fill"], np.uint8)).all()
    assert ((e["state"][..., 3] > 0) == (e["mask"] == 1)).all() and np.isfinite(e["state"]).all()


def test_what_the_edge_cases_are_there_for():
    assert expected("triangle from behind two_sided False")["info"]["observed_texels"] == 0
    assert expected("triangle from behind two_sided True")["info"]["observed_texels"] > 5
    e = expected("a frame behind the camera")
    assert e["info"]["observed_texels"] > 5 and not bake_case("a frame behind the camera", [0]).any()
    assert np.array_equal(e["state"], bake_case("a frame behind the camera", [1]))
    with_c, without = expected("outside every image, vertex colours"), expected("outside every image, fill")
    face = texels_host(2, 8, None)[0]
    assert not with_c["mask"][face == 1].any() and with_c["info"]["fallback_texels"] > 30 and without["info"]["fallback_texels"] == 0
    assert (without["atlas"][(face == 1)] == np.array((9, 200, 77), np.uint8)).all()
    assert (with_c["atlas"][face == 1] != np.array((9, 200, 77), np.uint8)).any()
    assert np.array_equal(with_c["atlas"][with_c["mask"] == 1], without["atlas"][without["mask"] == 1])
    e = expected("bad faces")
    assert [e["info"][k] for k in ("bad_index_faces", "degenerate_faces", "nonfinite_faces")] == [3, 2, 2]
    assert expected("grazing above min_cos")["info"]["observed_texels"] > 5
    assert expected("grazing below min_cos")["info"]["observed_texels"] == 0
    both, first = bake_case("equal weights under best", [0, 1]), bake_case("equal weights under best", [0])
    assert first[..., 3].any() and np.array_equal(both, first)             # the earliest of two equal weights stays
    assert not np.array_equal(bake_case("equal weights under best", [1]), first)


def test_frames_split_over_calls_leave_the_same_state():
    for name in ("Nf 3 5x7 P8 V3 mean", "Nf 3 5x7 P8 V3 best", "wall P8 mean"):
        whole = expected(name)["state"]
        part = bake_case(name, [2], bake_case(name, [1], bake_case(name, [0])))
        assert np.array_equal(whole.view(np.uint32), part.view(np.uint32)), name


def test_occluded_wall_texels_take_colour_only_from_the_frames_that_see_them():
    """Wall texels whose segment to camera 0 passes within 0.8 R of the sphere's centre are hidden from it by the mesh (the
    512-face polyhedron contains the ball of 0.97 R): their state is that of the frames 1 and 2 alone."""
    for name in ("wall P8 mean", "wall P8 best"):
        c = cases()[name]
        mesh = c["mesh"]
        nf = mesh["faces"].shape[0]
        face, a, b = texels_host(nf, c["P"], c["cols"])
        K = c["P"] - 3.0
        corners = mesh["vertices"].astype(np.float64)[mesh["faces"][np.minimum(face, nf - 1)]]
        pt = np.einsum("hwk,hwkc->hwc", np.stack([1.0 - (a + b) / K, a / K, b / K], -1), corners)
        o = WALL_CAMERAS[0][:, 3].astype(np.float64)
        d = pt - o
        t = np.clip(((np.array(SPHERE_C) - o) * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
        gap = np.linalg.norm(o + t[..., None] * d - np.array(SPHERE_C), axis=-1)
        hidden = (face < nf) & (face >= 512) & (np.abs(pt[..., 2] - WALL_Z) < 1e-6) & (gap < 0.8 * SPHERE_R)
        all_frames, others, alone = expected(name)["state"], bake_case(name, [1, 2]), bake_case(name, [0])
        assert hidden.sum() > 100 and not alone[hidden].any()
        assert np.array_equal(all_frames[hidden], others[hidden]) and (others[hidden][:, 3] > 0).sum() > 50, name
        seen = (face >= 512) & (face < nf) & (alone[..., 3] > 0)
        assert seen.sum() > 1000 and not np.array_equal(all_frames[seen], others[seen])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_against_an_independent_fp64_baker(name):
    c, e = cases()[name], expected(name)
    frames, depth = inputs(name)
    atlas, observed, decision = bake_fp64(c["mesh"], c["P"], c["cols"], frames, depth, c["c2w"], c["f"], c["cx"], c["cy"], c["blend"],
                                          c["vis_tol"], c["min_cos"], c["two_sided"], c["fill"])
    used = e["info"]["used_texels"]
    if not used:
        assert atlas.shape == e["atlas"].shape
        return
    share = decision.sum() / used
    diff = np.abs(atlas.astype(np.int64) - e["atlas"].astype(np.int64)).max(-1)
    print(f"{name}: {int(decision.sum())} of {used} used texels on a decision ({share:.4%}); largest difference elsewhere "
          f"{int(diff[~decision].max())} levels, mask differences elsewhere {int((observed != (e['mask'] == 1))[~decision].sum())}")
    assert share <= FP64_EXCLUDED
    assert np.array_equal(observed[~decision], (e["mask"] == 1)[~decision])
    assert diff[~decision].max() <= FP64_LEVELS


@pytest.mark.parametrize("which", sorted(ROUND_TRIP))
def test_round_trip_through_the_rasteriser(which):
    """Per frame v: the frame baked alone, the mesh rasterised at its pose (the restatement, weights=True), the atlas sampled
    by sample_texture, and the result compared with the frame at the pixels the mesh hits and whose texel the frame observed (an
    unobserved texel holds no sample of the frame, so the bound says nothing of it).  The frames change by at most G levels per
    pixel of distance; a texel's footprint in the image is at most s = max over the hit faces of (|e1| + |e2|) / K pixels, e1
    and e2 the face's projected edges from corner 0; nearest texel plus nearest pixel move a sample by at most s + 1 pixels and
    the three roundings add 2 levels: the bar is G (s + 1) + 2."""
    name, frame_ids = ROUND_TRIP[which]
    c = cases()[name]
    frames, depth = inputs(name)
    mesh, K = c["mesh"], c["P"] - 3
    nf = mesh["faces"].shape[0]
    rows, cols, Ht, Wt = layout_host(nf, c["P"], c["cols"])
    for v in frame_ids:
        state = bake_case(name, [v])
        tex = resolve_host(mesh, c["P"], c["cols"], state, c["blend"], c["fill"])
        ras = rasterize_host(mesh, c["c2w"][v:v + 1], c["W"], c["H"], c["f"], c["cx"], c["cy"], cull="back")
        out = {"face": torch.from_numpy(ras["face"]), "weights": torch.from_numpy(ras["weights"])}
        got = sample_texture(out, {"atlas": torch.from_numpy(tex["atlas"]), "patch": c["P"], "cols": cols}).numpy()[0]
        seen = sample_texture(out, {"atlas": torch.from_numpy(np.repeat(tex["mask"][..., None], 3, -1)), "patch": c["P"], "cols": cols})
        hit = ras["face"][0] >= 0
        judged = hit & (seen.numpy()[0, ..., 0] == 1)
        M = np.eye(4)
        M[:3] = c["c2w"][v].astype(np.float64)
        ids = np.unique(ras["face"][0][hit])
        pc = np.concatenate([mesh["vertices"].astype(np.float64)[mesh["faces"][ids]], np.ones((ids.size, 3, 1))], -1) @ np.linalg.inv(M).T
        px = np.stack([pc[..., 0] / -pc[..., 2], -pc[..., 1] / -pc[..., 2]], -1) * float(c["f"])
        s = float(((np.linalg.norm(px[:, 1] - px[:, 0], axis=-1) + np.linalg.norm(px[:, 2] - px[:, 0], axis=-1)) / K).max())
        bar = G_LEVELS * (s + 1.0) + 2.0
        diff = np.abs(got.astype(np.int64) - frames[v].astype(np.int64)).max(-1)
        print(f"{which}, frame {v}: hit {int(hit.sum())} pixels, judged {int(judged.sum())}, s = {s:.3f} pixels, G = {G_LEVELS:.2f}, "
              f"bar {bar:.1f} levels, largest difference {int(diff[judged].max())}, mean {diff[judged].mean():.2f}")
        assert judged.sum() > 0.5 * hit.sum() > 50
        assert diff[judged].max() <= bar


def test_write_obj_parses_back(tmp_path):
    from PIL import Image
    c, e = cases()["fan P5 cols 4 V3 mean"], expected("fan P5 cols 4 V3 mean")
    mesh = {"vertices": torch.from_numpy(c["mesh"]["vertices"]), "faces": torch.from_numpy(c["mesh"]["faces"]), "rgb8": None}
    nv, nf = c["mesh"]["vertices"].shape[0], c["mesh"]["faces"].shape[0]
    tex = {"atlas": torch.from_numpy(e["atlas"]), "uv": face_uv(nf, c["P"], c["cols"])}
    path = tmp_path / "fan.obj"
    write_obj(path, mesh, tex)
    lines = path.read_text().splitlines()
    v = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")])
    vt = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("vt ")])
    f = np.array([[[int(x) for x in corner.split("/")] for corner in ln.split()[1:]] for ln in lines if ln.startswith("f ")])
    assert v.shape == (nv, 3) and vt.shape == (3 * nf, 2) and f.shape == (nf, 3, 2)
    assert np.array_equal(v.astype(np.float32), c["mesh"]["vertices"]) and np.array_equal(vt.astype(np.float32), uv_host(nf, c["P"], c["cols"]).reshape(-1, 2))
    assert (vt >= 0).all() and (vt <= 1).all()
    assert np.array_equal(f[..., 0] - 1, c["mesh"]["faces"]) and np.array_equal(f[..., 1].reshape(-1), np.arange(1, 3 * nf + 1))
    assert f.min() >= 1 and "mtllib fan.mtl" in lines and "usemtl fan" in lines
    assert "map_Kd fan.png" in (tmp_path / "fan.mtl").read_text()
    with Image.open(tmp_path / "fan.png") as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), e["atlas"])
    with pytest.raises(ValueError, match="no face"):
        write_obj(tmp_path / "none.obj", dict(mesh, faces=torch.zeros(0, 3, dtype=torch.int32)), tex)
    with pytest.raises(ValueError, match="uv"):
        write_obj(tmp_path / "bad.obj", mesh, dict(tex, uv=tex["uv"][:-1]))


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    with pytest.raises(TypeError, match="mesh"):
        TextureBaker([torch.zeros(4, 3)])
    for key, bad in (("vertices", torch.zeros(4, 2)), ("faces", cpu_mesh(rgb=False)["faces"].long()), ("rgb8", torch.zeros(4, 3))):
        with pytest.raises(ValueError, match=key):
            TextureBaker(dict(cpu_mesh(rgb=False), **{key: bad}))
    for key, bad in (("patch", 3), ("patch", 65), ("patch", 7.5), ("cols", 0), ("cols", 1.5), ("blend", "max"), ("blend", 1),
                     ("vis_tol", -0.1), ("vis_tol", math.nan), ("vis_tol", "x"), ("min_cos", 1.5), ("min_cos", -0.1),
                     ("min_cos", math.nan), ("two_sided", 1), ("two_sided", None)):
        with pytest.raises(ValueError, match=key):
            TextureBaker(cpu_mesh(rgb=False), **{key: bad})
    with pytest.raises(TypeError, match="mesh"):                           # the mesh is checked before the layout
        TextureBaker(None, patch=3)
    baker = TextureBaker(cpu_mesh(rgb=False), patch=5, cols=1, blend="best", two_sided=True)
    assert (baker.rows, baker.cols, baker.Ht, baker.Wt) == (1, 1, 5, 5)
    poses = torch.eye(4)[None, :3].repeat(2, 1, 1)
    ok = dict(rgb=torch.zeros(2, 6, 8, 3, dtype=torch.uint8), poses=poses, focal=5.0, center=(4.0, 3.0))

    def add(**over):
        kw = dict(ok, **over)
        return baker.add(kw.pop("rgb"), kw.pop("poses"), kw.pop("focal"), kw.pop("center"), **kw)
    with pytest.raises(TypeError, match="rgb"):
        add(rgb=np.zeros((2, 6, 8, 3), np.uint8))
    for bad in (torch.zeros(2, 6, 8, 3, dtype=torch.int32), torch.zeros(2, 6, 8, 4), torch.zeros(6, 8, 3), torch.zeros(0, 6, 8, 3)):
        with pytest.raises(ValueError, match="rgb"):
            add(rgb=bad)
    with pytest.raises(TypeError, match="mesh_depth"):
        add(mesh_depth=np.zeros((2, 6, 8), np.float32))
    for bad in (torch.zeros(2, 6, 7), torch.zeros(2, 6, 8, dtype=torch.int32), torch.zeros(1, 6, 8)):
        with pytest.raises(ValueError, match="mesh_depth"):
            add(mesh_depth=bad)
    for bad in (torch.zeros(2, 3, 3), torch.zeros(3, 4), torch.zeros(2, 3, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses"):
            add(poses=bad)
    with pytest.raises(ValueError, match="3 poses for 2 frames"):
        add(poses=torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="focal"):
        add(focal=None, center=None)
    with pytest.raises(ValueError, match="focal"):
        add(center=(1.0, 2.0, 3.0))
    for bad in ((2.0, 1.0), (math.nan, 1.0), (1.0,)):
        with pytest.raises(ValueError, match="depth_range"):
            add(depth_range=bad)
    for bad in (-1, 1.5, None, True, 100):
        with pytest.raises(ValueError, match="max_bytes"):
            add(max_bytes=bad)
    with pytest.raises(ValueError, match="poses"):                         # frames, then poses, then intrinsics
        add(poses=torch.zeros(2, 3, 3), focal=None)
    with pytest.raises(NativeError):                                       # a valid call on the CPU: no fallback
        add()
    with pytest.raises(NativeError):
        add(rgb=torch.zeros(2, 6, 8, 3), mesh_depth=torch.ones(2, 6, 8))
    for bad in ((0, 0), (0, 0, 256), (0, -1, 0), (0.5, 0, 0), 7, "abc"):
        with pytest.raises(ValueError, match="fill"):
            baker.finish(fill=bad)
    with pytest.raises(NativeError):
        baker.finish()
    with pytest.raises(NativeError):
        baker.state
    with pytest.raises(ValueError, match="weights=True"):
        sample_texture({"face": torch.zeros(1, 2, 2, dtype=torch.int32), "weights": None}, {"atlas": torch.zeros(4, 4, 3), "patch": 4, "cols": 1})


def test_scene_texture_checks_before_it_renders(monkeypatch):
    from localrf_amd import mesh_raster
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch, (mesh_raster, "rasterize"))
    m = cpu_mesh(rgb=False)
    with pytest.raises(TypeError, match="unknown options"):
        scene_texture(lt, m, W, H, voxel=0.1)
    with pytest.raises(TypeError, match="mesh"):
        scene_texture(lt, None, W, H)
    for key, bad, match in (("patch", 3, "patch"), ("cols", 0, "cols"), ("blend", "both", "blend"), ("vis_tol", -1.0, "vis_tol"),
                            ("min_cos", 2.0, "min_cos"), ("two_sided", 1, "two_sided"), ("depth_range", (2.0, 1.0), "depth_range"),
                            ("fill", (1, 2), "fill"), ("frames_per_call", 0, "frames_per_call"), ("max_bytes", -1, "max_bytes"),
                            ("max_bytes", 64, "max_bytes")):
        with pytest.raises(ValueError, match=match):
            scene_texture(lt, m, W, H, **{key: bad})
    fov = lt.fov
    try:
        lt.fov = 360
        with pytest.raises(ValueError, match="pinhole"):
            scene_texture(lt, m, W, H)
    finally:
        lt.fov = fov
    with pytest.raises(NativeError):                                       # accepted arguments, a CPU scene
        scene_texture(lt, m, W, H, patch=5, blend="best", fill=(1, 2, 3))


def test_texture_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    assert "typedef struct LrfMeshTexture" in header and C.sizeof(N.LrfMeshTexture) == 8 * 8 + 2 * 8 + 7 * 4 + 2 * 4 + 4
    assert built_lib.lrf_abi_version() == 7
    assert "mesh_texture" in __import__("localrf_amd").__all__
    fill = (C.c_uint8 * 3)(1, 2, 3)

    def args(**over):
        return filled(N.LrfMeshTexture, dict(vertices=FAKE, faces=FAKE, frames=FAKE, mesh_depth=FAKE, cam2world=FAKE, focal=FAKE, center=FAKE,
                                             Nv=5, Nf=3, patch=8, cols=2, blend=0, two_sided=0, V=2, H=6, W=8, vis_tol=0.02, min_cos=0.2), **over)

    def bake(state=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_texture_bake(C.byref(args(**over)), state, None))

    def resolve(state=FAKE, fill_=fill, atlas=FAKE, mask=FAKE, info=FAKE, **over):
        return refused(built_lib, built_lib.lrf_mesh_texture_resolve(C.byref(args(**over)), state, fill_, atlas, mask, info, None))
    for call, who in ((bake, "lrf_mesh_texture_bake"), (resolve, "lrf_mesh_texture_resolve")):
        for bad in (dict(patch=3), dict(patch=65), dict(Nf=-1), dict(Nv=-1), dict(Nv=1 << 31), dict(Nv=0), dict(Nf=1 << 22, patch=64),
                    dict(Nf=1 << 31)):
            assert call(**bad).startswith(who + ": need 4 <= patch <= 64"), bad
        assert "cols >= 1" in call(cols=0)
        for bad in (dict(vertices=None), dict(faces=None), dict(state=None)):
            assert call(**bad).endswith(": null argument"), bad
        for bad in (-1, 2):
            assert "blend" in call(blend=bad)
        for bad in (dict(vertices=FAKE + 2), dict(faces=FAKE + 1)):
            assert "4-byte aligned" in call(**bad), bad
        assert "16-byte aligned" in call(state=FAKE + 8)
    for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(V=1 << 15, H=1 << 8, W=1 << 8)):
        assert "need V, H, W >= 1" in bake(**bad), bad
    for bad in (dict(frames=None), dict(mesh_depth=None), dict(cam2world=None), dict(focal=None), dict(center=None)):
        assert bake(**bad).endswith(": null argument"), bad
    for bad in (-1, 2):
        assert "two_sided" in bake(two_sided=bad)
    for bad in (-0.5, math.nan):
        assert "vis_tol" in bake(vis_tol=bad)
    for bad in (-0.1, 1.5, math.nan):
        assert "min_cos" in bake(min_cos=bad)
    for bad in (dict(mesh_depth=FAKE + 2), dict(cam2world=FAKE + 1), dict(focal=FAKE + 2)):
        assert "4-byte aligned" in bake(**bad), bad
    for bad in (dict(fill_=None), dict(atlas=None), dict(mask=None), dict(info=None)):
        assert resolve(**bad).endswith(": null argument"), bad
    assert "8-byte aligned" in resolve(info=FAKE + 4)
    assert built_lib.lrf_mesh_texture_bake(None, FAKE, None) != 0 and built_lib.lrf_mesh_texture_resolve(None, FAKE, fill, FAKE, FAKE, FAKE, None) != 0
    assert built_lib.lrf_mesh_texture_bake(C.byref(args(Nf=0, Nv=0, vertices=None, faces=None)), None, None) == 0   # nothing to launch


def test_state_bytes_refuse_and_follow_the_formula(built_lib):
    size = built_lib.lrf_mesh_texture_state_bytes
    for bad in ((-1, 8, 0), (4, 3, 0), (4, 65, 0), (1 << 31, 4, 0), (1 << 22, 64, 0), (1 << 22, 64, 1)):
        assert size(*bad) == 0, bad
    assert size(0, 8, 0) == 0 and size(0, 8, 3) == 0                        # no face: no texel
    for nf, P, cols in ((1, 4, 0), (2, 5, 1), (3, 8, 0), (38, 5, 4), (512, 16, 7), (5100, 8, 0), (302638, 4, 0), (302638, 16, 0)):
        rows, cl, Ht, Wt = layout_host(nf, P, cols or None)
        assert size(nf, P, cols) == 16 * Ht * Wt, (nf, P, cols)
        assert atlas_layout(nf, P, cols or None) == (rows, cl, Ht, Wt)


def test_texture_kernels_use_no_scratch():
    """The kernels of lrf_mesh_texture.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
