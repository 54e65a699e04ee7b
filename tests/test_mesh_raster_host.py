"""The mesh rasteriser and the depth agreement without a GPU: properties of the numpy restatement of csrc/lrf_mesh_raster.inl
(tests/mesh_raster_cases.py) -- parity on closed meshes, agreement with an independent fp64 ray caster, the sign convention --,
argument refusals before any native call (Python and C ABI), the new symbols, the workspace size, and the kernels' scratch use.

Measured with the committed restatement on the non-degenerate sphere cameras: the largest relative depth difference from the
fp64 Moeller-Trumbore reference is 2.42e-7 (the bar below is four times that), with at most 0.065 % of an image excluded for a
barycentric weight within 1e-4 of zero."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, filled, refused
from localrf_amd import NativeError, mesh_raster
from localrf_amd.mesh_raster import depth_agreement, rasterize, scene_mesh_agreement
from mesh_raster_cases import (AGREEMENT_SHAPES, AGREEMENT_TOLS, AG_SCALE, BOX_FACE, CASE_NAMES, SMALL_MAX, SPHERE_KIND,
                               SPHERE_NONDEGENERATE, agreement_host, agreement_maps, box_host, cases, expected, moller_trumbore,
                               octa_sphere, to_camera)
from mesh_util import cpu_mesh, forbid_native, forbid_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lrf_mesh_rasterize_workspace_bytes", "lrf_mesh_rasterize", "lrf_depth_agreement")
KERNELS = ("k_rs_init", "k_rs_faces", "k_rs_large", "k_rs_resolve", "k_ag_zero", "k_depth_agreement")
MT_MEASURED, MT_BAR = 2.42e-7, 4 * 2.42e-7
MT_MARGIN, MT_EXCLUDED = 1e-4, 0.02


def test_the_cases_cover_the_sizes_and_frame_counts():
    sizes = {(c["W"], c["H"]) for c in cases().values()}
    assert {(1, 1), (5, 7), (64, 48), (130, 70)} <= sizes
    assert {c["c2w"].shape[0] for c in cases().values()} >= {1, 3}
    assert cases()["empty 5x7"]["mesh"]["faces"].shape == (0, 3)
    assert octa_sphere()["faces"].shape == (512, 3)
    assert SMALL_MAX in BOX_FACE and {64, 65} <= set(BOX_FACE)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_shapes_and_empty_pixels(name):
    c, e = cases()[name], expected(name)
    V, H, W = c["c2w"].shape[0], c["H"], c["W"]
    assert e["depth"].shape == (V, H, W) and e["depth"].dtype == np.float32 and e["face"].dtype == np.int32
    miss = e["face"] < 0
    assert (e["depth"][miss] == 0).all() and (e["depth"][~miss] > 0).all() and not e["weights"][miss].any()
    assert (e["crossings"][~miss] >= 1).all()
    w = e["weights"][~miss].astype(np.float64)
    assert (w >= 0).all() and (np.abs(w.sum(-1) - 1) < 1e-6).all()
    if c["cull"] is None:
        assert (e["crossings"][miss] == 0).all()


def test_closed_sphere_parity_and_no_hole_from_inside():
    e = expected("sphere 64x48 V5")
    for fr, kind in enumerate(SPHERE_KIND):
        cr, face = e["crossings"][fr], e["face"][fr]
        if kind == "outside":
            assert (cr % 2 == 0).all() and ((cr > 0) == (face >= 0)).all()
        elif kind == "inside":
            assert (cr % 2 == 1).all() and (face >= 0).all()
    ties = expected("sphere ties")                                          # rays through vertices and along edges
    assert (ties["crossings"] == 1).all() and (ties["face"] >= 0).all()


def test_the_tie_case_has_ties():
    c = cases()["sphere ties"]
    q = to_camera(c["mesh"]["vertices"], c["c2w"][0])
    assert (q[:, 0] == 0).sum() > 20 and (q[:, 1] == 0).sum() > 20
    from points_cases import pixel_dirs
    d = pixel_dirs(c["H"], c["W"], c["f"], c["cx"], c["cy"])
    assert (d[0, :, 0] == 0).sum() == 1 and (d[:, 0, 1] == 0).sum() == 1     # one column and one row of rays in those planes


def test_against_fp64_moller_trumbore():
    c, e = cases()["sphere 64x48 V5"], expected("sphere 64x48 V5")
    worst = 0.0
    for fr in SPHERE_NONDEGENERATE:
        t, b = moller_trumbore(c["mesh"], c["c2w"][fr], c["W"], c["H"], c["f"], c["cx"], c["cy"])
        front, least = t > 0, b.min(-1)
        safe = ~((np.abs(least) <= MT_MARGIN) & front).any(0)
        assert 1.0 - safe.mean() <= MT_EXCLUDED
        nearest = np.where(front & (least > 0), t, np.inf).min(0)
        covered = np.isfinite(nearest)
        depth = e["depth"][fr]
        assert ((depth > 0) == covered)[safe].all()
        m = safe & covered
        rel = np.abs(depth[m].astype(np.float64) - nearest[m]) / nearest[m]
        print(f"frame {fr}: excluded {1.0 - safe.mean():.5f}, largest relative depth difference {rel.max():.3e}")
        worst = max(worst, float(rel.max()))
    assert worst <= MT_BAR, (worst, MT_MEASURED)


def test_a_positive_sign_sees_the_normals_side():
    for where, seen in (("from its normal's side", True), ("from behind", False)):
        c = cases()[f"triangle {where} 5x7 cull None"]
        v = c["mesh"]["vertices"].astype(np.float64)
        n = np.cross(v[1] - v[0], v[2] - v[0])
        assert (float(n @ (c["c2w"][0][:, 3].astype(np.float64) - v[0])) > 0) is seen
        hits = {cull: int((expected(f"triangle {where} 5x7 cull {cull}")["face"] >= 0).sum()) for cull in (None, "back", "front")}
        assert hits[None] > 0 and hits["back" if seen else "front"] == hits[None] and hits["front" if seen else "back"] == 0
        for cull in ("back", "front"):                                      # crossings do not depend on cull
            assert np.array_equal(expected(f"triangle {where} 5x7 cull {cull}")["crossings"], expected(f"triangle {where} 5x7 cull None")["crossings"])
    inside = expected("sphere cull back")                                   # a TSDF-wound sphere: free space is outside
    assert (inside["face"][0] >= 0).sum() == (expected("sphere 64x48 V5")["face"][0] >= 0).sum() and (inside["face"][1] < 0).all()


def test_a_quad_is_the_same_pixels_along_either_diagonal():
    a, b = expected("quad diagonal 02"), expected("quad diagonal 13")
    assert np.array_equal(a["face"] >= 0, b["face"] >= 0) and (a["face"] >= 0).sum() > 500
    for e in (a, b):
        assert e["crossings"].max() == 1 and set(np.unique(e["face"])) == {-1, 0, 1}


def test_coincident_bad_behind_straddling_huge_and_range():
    e = expected("coincident faces")
    assert 2 not in e["face"] and (e["face"] == 1).sum() > 100              # faces 1 and 2 coincide: the smaller index wins
    e = expected("bad faces")
    assert e["info"] == {"bad_index_faces": 3, "degenerate_faces": 2, "nonfinite_faces": 2}
    assert set(np.unique(e["face"])) <= {-1, 0, 3, 7}
    assert (expected("behind the camera")["face"] < 0).all()
    e = expected("straddling the camera plane")
    assert (e["face"] >= 0).sum() > 100 and (e["depth"][e["face"] >= 0] > 0).all()
    assert (expected("larger than the image")["face"] == 0).all()
    c, e, full = cases()["sphere depth range"], expected("sphere depth range"), expected("sphere 64x48 V5")
    lo, hi = c["depth_range"]
    hit = e["face"] >= 0
    assert hit.any() and (e["depth"][hit] >= lo).all() and (e["depth"][hit] <= hi).all()
    near = full["depth"][[0, 3]]
    assert ((near > 0) & (near < lo)).any() and (e["crossings"] == 1).any()  # the front is cut away, the back shows


def test_the_box_cases_sit_on_the_threshold():
    for n in BOX_FACE:
        c = cases()[f"box of {n} pixels"]
        i0, i1, j0, j1 = box_host(to_camera(c["mesh"]["vertices"], c["c2w"][0]), c["f"], c["cx"], c["cy"], c["W"], c["H"])
        assert (i1 - i0 + 1) * (j1 - j0 + 1) == n
        jj, ii = np.nonzero(expected(f"box of {n} pixels")["face"][0] >= 0)
        assert jj.size and i0 < ii.min() and ii.max() < i1 and j0 < jj.min() and jj.max() < j1
    for name in CASE_NAMES:                                                 # every hit lies inside its face's box
        c, e = cases()[name], expected(name)
        for fr in range(c["c2w"].shape[0]):
            for f in np.unique(e["face"][fr]):
                if f < 0:
                    continue
                q = to_camera(c["mesh"]["vertices"][c["mesh"]["faces"][f]], c["c2w"][fr])
                i0, i1, j0, j1 = box_host(q, c["f"], c["cx"], c["cy"], c["W"], c["H"])
                jj, ii = np.nonzero(e["face"][fr] == f)
                assert i0 <= ii.min() and ii.max() <= i1 and j0 <= jj.min() and jj.max() <= j1, (name, fr, f)


@pytest.mark.parametrize("shape", AGREEMENT_SHAPES)
def test_agreement_restatement_against_plain_numpy(shape):
    a, b = agreement_maps(40 + shape[1], *shape)
    rng = (0.6, 30.0)
    words, err = agreement_host(a, b, AGREEMENT_TOLS, rng)
    with np.errstate(all="ignore"):
        def ok(d):
            return np.isfinite(d) & (d > 0) & (d >= np.float32(rng[0])) & (d <= np.float32(rng[1]))
        both = ok(a) & ok(b)
        assert np.array_equal(words[:, 0], both.sum((1, 2))) and words[:, :4].sum() == a.size
        rel = np.abs(a.astype(np.float64) - b) / b
        assert np.array_equal(np.isnan(err), ~both) and np.allclose(err[both], rel[both], rtol=3e-7)
        mean = words[:, 4].sum() / AG_SCALE / max(int(both.sum()), 1)
        assert abs(mean - np.minimum(rel[both], 16.0).mean() if both.any() else 0.0) < 1e-6
        for k, tol in enumerate(AGREEMENT_TOLS):
            plain = (both & (np.abs(a - b) <= np.float32(tol) * b)).sum((1, 2))
            assert np.array_equal(words[:, 8 + k], plain)
        assert not words[:, 5:8].any() and not words[:, 8 + len(AGREEMENT_TOLS):].any()
    assert (np.diff(words[:, 8:8 + len(AGREEMENT_TOLS)], axis=1) >= 0).all()


def test_python_refusals_before_any_native_call(monkeypatch):
    forbid_native(monkeypatch)
    poses = torch.eye(4)[None, :3].repeat(2, 1, 1)
    ok = dict(poses=poses, W=8, H=6, focal=5.0, center=(4.0, 3.0))

    def ras(mesh=None, **over):
        kw = dict(ok, **over)
        return rasterize(cpu_mesh(rgb=False) if mesh is None else mesh, kw.pop("poses"), kw.pop("W"), kw.pop("H"), kw.pop("focal"), kw.pop("center"), **kw)
    with pytest.raises(TypeError, match="mesh"):
        ras(mesh=[torch.zeros(4, 3)])
    for key, bad in (("vertices", torch.zeros(4, 3, dtype=torch.float64)), ("vertices", torch.zeros(4, 2)),
                     ("faces", cpu_mesh(rgb=False)["faces"].long()), ("rgb8", torch.zeros(4, 3))):
        with pytest.raises(ValueError, match=key):
            ras(mesh=dict(cpu_mesh(rgb=False), **{key: bad}))
    for bad in (torch.zeros(2, 3, 3), torch.zeros(3, 4), torch.zeros(2, 3, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses"):
            ras(poses=bad)
    with pytest.raises(ValueError, match="no pose"):
        ras(poses=torch.zeros(0, 3, 4))
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="W, H"):
            ras(W=bad)
    with pytest.raises(ValueError, match="focal"):                          # no intrinsics: a 360-degree request
        ras(focal=None, center=None)
    with pytest.raises(ValueError, match="focal"):
        ras(center=(1.0, 2.0, 3.0))
    for bad in ((2.0, 1.0), (math.nan, 1.0), (1.0,)):
        with pytest.raises(ValueError, match="depth_range"):
            ras(depth_range=bad)
    for bad in ("Back", "both", 1, True, 0):
        with pytest.raises(ValueError, match="cull"):
            ras(cull=bad)
    for key in ("crossings", "weights"):
        for bad in (1, None, "yes"):
            with pytest.raises(ValueError, match=key):
                ras(**{key: bad})
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="max_bytes"):
            ras(max_bytes=bad)
    with pytest.raises(ValueError, match="max_bytes"):                      # one frame does not fit
        ras(max_bytes=100)
    for bad in (-1, 1 << 31, 0.5):
        with pytest.raises(ValueError, match="small_max"):
            ras(small_max=bad)
    with pytest.raises(NativeError):                                        # a valid call on the CPU: no fallback
        ras()
    with pytest.raises(NativeError):
        ras(cull="front", crossings=True, weights=True, depth_range=(0.5, 0.5))

    d = torch.ones(2, 6, 8)
    with pytest.raises(TypeError, match="mesh_depth"):
        depth_agreement(d.numpy(), d)
    with pytest.raises(TypeError, match="depth"):
        depth_agreement(d, d.numpy())
    for bad in (torch.ones(2, 6, 7), torch.ones(6, 8), torch.ones(2, 6, 8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="mesh_depth"):
            depth_agreement(bad, d)
    with pytest.raises(ValueError, match="depth"):
        depth_agreement(d, torch.ones(2, 6, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="at most 8"):
        depth_agreement(d, d, rel_tols=[0.01] * 9)
    for bad in ((-0.1,), (math.nan,), 0.5, ("a",)):
        with pytest.raises(ValueError, match="rel_tol"):
            depth_agreement(d, d, rel_tols=bad)
    with pytest.raises(ValueError, match="depth_range"):
        depth_agreement(d, d, depth_range=(3.0, 1.0))
    with pytest.raises(ValueError, match="error_map"):
        depth_agreement(d, d, error_map=1)
    with pytest.raises(NativeError):
        depth_agreement(d, d, rel_tols=[0.01] * 8)


def test_scene_mesh_agreement_checks_before_it_renders(monkeypatch):
    from localrf_amd import depth_quantiles
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    forbid_render(monkeypatch, (depth_quantiles, "fusion_depth"), (mesh_raster, "rasterize"))
    m = cpu_mesh(rgb=False)
    with pytest.raises(ValueError, match="depth must be"):
        scene_mesh_agreement(lt, m, W, H, depth="mean")
    with pytest.raises(TypeError, match="unknown options"):
        scene_mesh_agreement(lt, m, W, H, voxel=0.1)
    with pytest.raises(TypeError, match="mesh"):
        scene_mesh_agreement(lt, None, W, H)
    for key, bad, match in (("cull", "both", "cull"), ("depth_range", (2.0, 1.0), "depth_range"), ("rel_tols", [0.1] * 9, "at most 8"),
                            ("frames_per_call", 0, "frames_per_call"), ("small_max", -1, "small_max"), ("max_bytes", -1, "max_bytes"),
                            ("max_bytes", 64, "max_bytes")):
        with pytest.raises(ValueError, match=match):
            scene_mesh_agreement(lt, m, W, H, **{key: bad})
    fov = lt.fov
    try:
        lt.fov = 360
        with pytest.raises(ValueError, match="pinhole"):
            scene_mesh_agreement(lt, m, W, H)
    finally:
        lt.fov = fov
    with pytest.raises(NativeError):                                        # accepted arguments, a CPU scene
        scene_mesh_agreement(lt, m, W, H, cull="back", rel_tols=(0.02,))


def test_raster_symbols_declared_exported_bound_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, SYMBOLS)
    debug = open(os.path.join(ROOT, "include", "lrf_debug.h")).read()
    assert "lrf_debug_mesh_rasterize(" in debug and "lrf_debug_mesh_rasterize" in N.SYMBOLS
    getattr(built_lib, "lrf_debug_mesh_rasterize")
    assert "typedef struct LrfMeshRaster" in header and C.sizeof(N.LrfMeshRaster) == 6 * 8 + 2 * 8 + 4 * 4 + 2 * 4
    assert "#define LRF_AGREEMENT_MAX_TOLS 8" in header and N.LRF_AGREEMENT_MAX_TOLS == 8
    assert built_lib.lrf_abi_version() == 7

    def ras(debug=False, small_max=64, depth=FAKE, face=FAKE, rgb8_out=None, weights=FAKE, crossings=FAKE, info=FAKE, wsp=FAKE, **over):
        a = filled(N.LrfMeshRaster, dict(vertices=FAKE, faces=FAKE, cam2world=FAKE, focal=FAKE, center=FAKE, Nv=5, Nf=3, V=2, H=6, W=8, cull=0,
                                         d_min=0.0, d_max=math.inf), **over)
        if debug:
            return refused(built_lib, built_lib.lrf_debug_mesh_rasterize(C.byref(a), depth, face, rgb8_out, weights, crossings, info, wsp, small_max, None))
        return refused(built_lib, built_lib.lrf_mesh_rasterize(C.byref(a), depth, face, rgb8_out, weights, crossings, info, wsp, None))
    for dbg in (False, True):
        who = "lrf_debug_mesh_rasterize" if dbg else "lrf_mesh_rasterize"
        for bad in (dict(V=0), dict(H=0), dict(W=-1), dict(V=1 << 15, H=1 << 8, W=1 << 8), dict(Nv=-1), dict(Nv=1 << 31), dict(Nf=-1),
                    dict(V=2, Nf=1 << 30), dict(Nv=0)):
            assert ras(dbg, **bad).startswith(who + ": need V, H, W >= 1"), bad
        for bad in (dict(cam2world=None), dict(focal=None), dict(center=None), dict(vertices=None), dict(faces=None)):
            assert ras(dbg, **bad).endswith(": null argument"), bad
        for bad in (dict(depth=None), dict(face=None), dict(info=None), dict(wsp=None)):
            assert ras(dbg, **bad).endswith(": null argument"), bad
        assert "go together" in ras(dbg, rgb8=FAKE) and "go together" in ras(dbg, rgb8_out=FAKE)
        for bad in (-1, 3):
            assert "cull" in ras(dbg, cull=bad)
        assert "d_min <= d_max" in ras(dbg, d_min=2.0, d_max=1.0) and "d_min <= d_max" in ras(dbg, d_min=math.nan)
        for bad in (dict(vertices=FAKE + 2), dict(depth=FAKE + 1), dict(weights=FAKE + 2), dict(crossings=FAKE + 3), dict(focal=FAKE + 2)):
            assert "4-byte aligned" in ras(dbg, **bad), bad
        assert "8-byte aligned" in ras(dbg, info=FAKE + 4) and "8-byte aligned" in ras(dbg, wsp=FAKE + 4)
    assert "small_max" in ras(True, small_max=-1)
    assert built_lib.lrf_mesh_rasterize(None, FAKE, FAKE, None, None, None, FAKE, FAKE, None) != 0

    def agree(a=FAKE, b=FAKE, V=2, H=6, W=8, tols=(0.01, 0.05), n=None, d_min=0.0, d_max=math.inf, counts=FAKE, emap=None):
        arr = (C.c_float * 9)(*tols) if tols is not None else None
        return refused(built_lib, built_lib.lrf_depth_agreement(a, b, V, H, W, arr, len(tols) if n is None else n, d_min, d_max, counts, emap, None))
    for bad in (dict(V=0), dict(V=65536, H=1, W=1), dict(H=0), dict(W=0), dict(V=1 << 10, H=1 << 11, W=1 << 10)):
        assert "need 1 <= V <= 65535" in agree(**bad), bad
    for bad in (-1, 9):
        assert "n_tols" in agree(n=bad)
    for bad in (dict(a=None), dict(b=None), dict(counts=None), dict(tols=None, n=2)):
        assert agree(**bad).endswith(": null argument"), bad
    assert "d_min <= d_max" in agree(d_min=1.0, d_max=0.5)
    for bad in ((-0.5,), (0.1, math.nan)):
        assert "tolerance" in agree(tols=bad)
    assert "4-byte aligned" in agree(a=FAKE + 2) and "4-byte aligned" in agree(emap=FAKE + 1) and "8-byte aligned" in agree(counts=FAKE + 4)


def test_workspace_bytes_refuse_and_follow_the_formula(built_lib):
    size = built_lib.lrf_mesh_rasterize_workspace_bytes
    for bad in ((0, 6, 8, 3), (2, 0, 8, 3), (2, 6, -1, 3), (2, 6, 8, -1), (1 << 15, 1 << 8, 1 << 8, 0), (2, 6, 8, 1 << 30), (1, 1, 1, 1 << 31)):
        assert size(*bad) == 0, bad
    for V, H, W, nf in ((1, 1, 1, 0), (1, 7, 5, 1), (3, 70, 130, 38), (8, 360, 640, 700000), (1, 1, 1, (1 << 31) - 1)):
        assert size(V, H, W, nf) == (8 * V * H * W + 8 * V * nf + 8 + 255) // 256 * 256
        if 8 * H * W + 8 * nf + 8 <= 1 << 30:
            assert mesh_raster.frames_per_call(W, H, nf, 1 << 30) >= 1
    assert mesh_raster.frames_per_call(8, 6, 10, 8 + 2 * (8 * 48 + 80)) == 2


def test_raster_kernels_use_no_scratch():
    """The kernels of lrf_mesh_raster.inl as __graft_entry__.build() compiles them: the metadata only."""
    from isa_util import assert_no_scratch, device_asm
    assert_no_scratch(device_asm(), KERNELS, match="exact")
