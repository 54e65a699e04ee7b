"""The cases of tests/scene_cases.py checked on the CPU: every case against the conditions tests/test_gpu_scene.py relies on
(bounded cancellation in every per-view sum, a clamp margin, a clamped share, no near-parallel 6D columns, tolerances under the
caps), the recorded table E32 against a fresh measurement, the float64 references against what the reference recorded and,
where it is on the machine, against the reference's own functions; LocalTensorfs.get_cam2world on a CPU scene.  No GPU."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

import scene_cases as K
from losses_cases import _not_stale
from util import FIELD_KW, load_golden, quiet

REFERENCE = os.environ.get("LOCALRF_REFERENCE", "/root/reference/localTensoRF")   # the project this one was modelled on


@pytest.mark.parametrize("family,name", [(f, n) for f, (names, _) in K.CHECKS.items() for n in names])
def test_case_meets_its_conditions_and_E32_is_current(family, name):
    bad, e32 = K.CHECKS[family][1](name)
    assert not bad, bad
    _not_stale(K.E32[f"{family}:{name}"], e32, f"{family}:{name}")


def test_every_case_has_a_seed_and_a_row():
    names = [n for names, _ in K.CHECKS.values() for n in names]
    assert set(K.SEEDS) == set(names) and len(set(names)) == len(names)
    assert set(K.E32) == {f"{f}:{n}" for f, (names, _) in K.CHECKS.items() for n in names}


REFUSED = (("rays", "stride-2/pinhole", 1, "cancellation"), ("blend", "train", 1, "clamp margin"))


@pytest.mark.parametrize("family,name,seed,what", REFUSED)
def test_a_seed_that_cancels_or_sits_on_the_clamp_is_refused(family, name, seed, what):
    """Seeds the search passed over, for the reason it passed them over: stride-2/pinhole seed 1 (two rays per view whose focal
    terms cancel to under 5 % of their size), blend train seed 1 (a blended colour within 1e-4 of the clamp)."""
    assert K.SEEDS[name] > seed
    bad, _ = K.CHECKS[family][1](name, seed)
    assert any(what in b for b in bad), bad


def test_the_cases_hold_their_edges():
    c = K.rays_case("train/pinhole")
    assert (c["V"], c["per_view"], c["n_rf"], c["W"], c["H"], c["squeeze"]) == (16, 256, 1, 640, 480, True)
    assert float(c["focal"]) == 500.0 and tuple(c["center"].tolist()) != (320.0, 240.0)
    assert int(c["ids"].max()) // (640 * 480) > 800 and int(c["ids"].min()) // (640 * 480) < 100      # spread over 900 frames
    f = K.rays_case("frame/pinhole")
    ij = K.rays_ref("frame/pinhole")["ij"]
    assert f["per_view"] == f["W"] * f["H"] and f["forward_only"] and ij[0].tolist() == [0, 0] and ij[-1].tolist() == [63, 47]
    b = K.rays_case("big_ids/360")
    assert int(b["ids"].min()) >= 2 ** 31 and int(b["ids"].max()) < 2 ** 33 and (b["W"], b["H"]) == (960, 540)
    assert K.rays_case("pose44/pinhole")["c2w"].shape == (3, 4, 4)
    assert np.array_equal(K.rays_ref("pose44/pinhole")["rays"], K.rays_run(dict(K.rays_case("pose44/pinhole"), c2w=K.rays_case(
        "pose44/pinhole")["c2w"][:, :3]), torch.float64)["rays"])
    t = K.blend_case("train")
    assert (t["V"], t["per_view"], t["n_rf"]) == (16, 256, 1) and bool((t["bw"] == 1).all()) and t["exposure"] is not None
    for name in ("boundary-none", "boundary-identity"):
        c, ref = K.blend_case(name), K.blend_ref(name)
        h = c["R"] // 2
        on = (ref["y"][:h] == 0) | (ref["y"][:h] == 1)
        assert 0.5 < on.mean() < 0.8                            # two thirds of the first half sit exactly on the clamp
        assert np.array_equal(ref["g_rgb_f"][0, :h], c["g_rgbs"][:h].double().numpy()) and not ref["g_rgb_f"][0, h:].any()
        assert ((ref["y"][h:] == -0.25) | (ref["y"][h:] == 1.25)).all()
    z = K.blend_case("zero_weight_view")
    lo, hi = z["zero_view"] * z["per_view"], (z["zero_view"] + 1) * z["per_view"]
    ref = K.blend_ref("zero_weight_view")
    assert not ref["g_rgb_f"][:, lo:hi].any() and not ref["g_depth_f"][:, lo:hi].any() and ref["g_rgb_f"][:, :lo].any()
    assert not K.blend_ref("no_depth_grad")["g_depth_f"].any() and "g_exposure" not in K.blend_ref("no_exposure")
    assert (K.blend_ref("no_exposure")["y"] > 1).any()
    for name, (n1, n2) in (("scaled-a", (1e-3, 1e3)), ("scaled-b", (1e3, 1e-3))):
        r = K.pose_case(name)["r"].double()
        assert np.allclose(r[..., 0].norm(dim=-1), n1, rtol=1e-6) and np.allclose(r[..., 1].norm(dim=-1), n2, rtol=1e-6)
    rep = K.pose_ref("repeat")
    assert np.allclose(rep["g_a1"][3], rep["slots_r"][[3, 64, 128], :, 0].sum(0), rtol=1e-14, atol=0)
    assert K.pose_case("quirk_repeat")["frames"] == [0, 0, 1] and K.pose_case("quirk_repeat")["quirk"]
    assert K.pose_case("prior33")["r"].shape == (4, 3, 3)


def test_float64_pose_reference_reproduces_the_recorded_sixd_to_mtx():
    """tests/golden/sixd_to_mtx.npz: matrices and gradients the reference's sixD_to_mtx gave in float32 for V in {1,2,3,4,7},
    over the view axis at V = 3.  The bars are the ones tests/test_gpu_training.py holds the kernel to against the same file."""
    g = load_golden("sixd_to_mtx")
    for V in (1, 2, 3, 4, 7):
        r = torch.from_numpy(g[f"r{V}"]).double().requires_grad_(True)
        m, _, _ = K.sixd_to_mtx(r, quirk=V == 3)
        (gr,) = torch.autograd.grad(m, r, torch.from_numpy(g[f"ct{V}"]).double())
        assert K.rel_err(m.detach().numpy(), g[f"m{V}"]) <= K.CAP_VALUE, V
        assert K.rel_err(gr.numpy(), g[f"g{V}"]) <= K.CAP_POSE_ROT, V
    m3 = K.sixd_to_mtx(torch.from_numpy(g["r3"]).double(), quirk=False)[0].numpy()
    assert np.abs(m3 - g["m3"]).max() > 1e-2                    # without the quirk: proper rotations, not the reference's


def _reference_module(path, name):
    """A module of the reference loaded from its file, with the third-party modules it imports and never calls on this path
    replaced by empty ones for the duration of the import."""
    stubs = {}
    for mod in ("kornia", "cv2", "torchvision", "torchvision.transforms", "plyfile", "skimage", "skimage.measure", "scipy",
                "scipy.signal", "scipy.interpolate", "matplotlib", "matplotlib.pyplot", "PIL", "PIL.Image"):
        try:
            importlib.import_module(mod)
        except Exception:
            stubs[mod] = types.ModuleType(mod)
    for k, m in stubs.items():
        m.__dict__.update(create_meshgrid=None, COLORMAP_JET=2, UnivariateSpline=None, use=lambda *a, **k: None, Image=None)
        if "." in k and k.split(".")[0] in stubs:
            setattr(stubs[k.split(".")[0]], k.split(".")[1], m)
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def test_float32_expressions_against_the_reference_functions():
    """The float64 references' expressions, evaluated in float32, against get_ray_directions_lean, get_ray_directions_360,
    get_rays_lean and sixD_to_mtx of the reference itself: the same operations in the same order, so the same bits."""
    if not os.path.isfile(os.path.join(REFERENCE, "utils", "ray_utils.py")):
        pytest.skip("the reference is not on this machine")
    ru = _reference_module(os.path.join(REFERENCE, "utils", "ray_utils.py"), "_reference_ray_utils")
    uu = _reference_module(os.path.join(REFERENCE, "utils", "utils.py"), "_reference_utils")
    with K.one_thread():
        for name in ("train/pinhole", "train/360", "big_ids/pinhole", "big_ids/360", "frame/pinhole", "stride-65/360"):
            c = K.rays_case(name)
            col, row = K.ids2pixel(c)
            want = (ru.get_ray_directions_360(col, row, c["W"], c["H"]) if c["fov360"]
                    else ru.get_ray_directions_lean(col, row, c["focal"], c["center"]))
            rays, dirs = K.rays_forward(c, torch.float32, c["c2w"], c["w2rf"], c["focal"], c["center"])
            assert torch.equal(dirs, want), name
            for k in range(c["n_rf"]):
                m = c["c2w"].clone()
                m[:, :3, 3] += c["w2rf"][k]
                o, d = ru.get_rays_lean(want, m.repeat_interleave(c["per_view"], dim=0))
                assert torch.equal(rays[k], torch.cat([o, d], -1)), (name, k)
        for name in ("sizes-1-0.3", "sizes-3q-0.3", "sizes-4-0.05", "sizes-65-0.3", "scaled-a", "scaled-b"):
            c = K.pose_case(name)
            r = c["r"][torch.tensor(c["frames"])][:, :, :2]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                 # the dim-less torch.cross is deprecated, which is the point
                want = uu.sixD_to_mtx(r)
            got = K.sixd_to_mtx(r, c["quirk"])[0]
            assert K.rel_err(got.numpy(), want.numpy()) <= K.FLOOR, name      # torch.norm against sqrt(sum of squares)
    q3 = K.pose_case("sizes-3-0.3")
    r = q3["r"][:, :, :2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert K.rel_err(K.sixd_to_mtx(r, True)[0].numpy(), uu.sixD_to_mtx(r).numpy()) <= K.FLOOR     # three views: the quirk is the reference
        assert K.rel_err(K.sixd_to_mtx(r, False)[0].numpy(), uu.sixD_to_mtx(r).numpy()) > 1e-2


def _cpu_scene(camera_prior=None):
    from localrf_amd import LocalTensorfs
    torch.manual_seed(7)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    lt = quiet(LocalTensorfs, fov=85.6, n_init_frames=6, n_overlap=3, WH=(32, 24), n_iters_per_frame=600, n_iters_reg=100,
               lr_R_init=5e-3, lr_t_init=5e-4, lr_i_init=1e-3, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
               lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[], camera_prior=camera_prior, device="cpu",
               lr_upsample_reset=True, aabb=aabb, gridSize=[12, 12, 10], **FIELD_KW)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for r, t in zip(lt.r_c2w, lt.t_c2w):
            r.add_(0.1 * torch.randn(r.shape, generator=g))
            t.add_(0.1 * torch.randn(3, generator=g))
    return lt


@pytest.mark.parametrize("prior", [False, True])
def test_get_cam2world_is_indexing_the_stacked_parameters(prior):
    """LocalTensorfs.get_cam2world on a CPU scene against torch.stack(params)[ids] through sixD_to_mtx (local_tensorfs.py:
    292-299): negative ids, repeated ids, three ids (the quirk, also with a repeated frame), starting_id, and the [3,3]
    parameters camera priors leave, of which columns 0 and 1 are read and column 2 gets a zero gradient."""
    from localrf_amd.rays import sixD_to_mtx
    cp = None
    if prior:
        rel = torch.eye(4)[None].repeat(8, 1, 1)
        rel[:, :3] = K._poses(8, torch.Generator().manual_seed(3))
        cp = {"transforms": {"fl_x": 30.0, "w": 44.0}, "rel_poses": rel}
    lt = _cpu_scene(cp)
    F = len(lt.r_c2w)
    assert F == 6 and tuple(lt.r_c2w[0].shape) == ((3, 3) if prior else (3, 2)) and lt.reference_cross
    R, T = torch.stack(list(lt.r_c2w))[:, :, :2], torch.stack(list(lt.t_c2w))

    def want(idx):
        return torch.cat([sixD_to_mtx(R[idx], True), T[idx][..., None]], -1)

    for ids in ([0], [5, 0, 3, 1], [-1, 2, -6, 2, 2], [4, 4, 1], [1, -5, 0], list(range(F))):
        idx = torch.tensor(ids)
        for arg in (ids, idx):
            got = lt.get_cam2world(arg)
            assert got.shape == (len(ids), 3, 4) and torch.equal(got, want(idx)), ids
        ref = K.sixd_to_mtx(R[idx].double(), quirk=len(ids) == 3)[0]
        assert K.rel_err(got[:, :, :3].detach().numpy(), ref.detach().numpy()) <= K.FLOOR, ids
    for start in (0, 2, 3, 5):                                  # starting_id = 3 leaves three frames: the quirk again
        assert torch.equal(lt.get_cam2world(starting_id=start), want(torch.arange(start, F))), start
    for p in lt.parameters():
        p.grad = None
    gout = torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(4))
    (lt.get_cam2world([-1, 2, -6, 2, 2]) * gout).sum().backward()
    leaf = R.detach().clone().requires_grad_(True)
    (sixD_to_mtx(leaf[torch.tensor([-1, 2, -6, 2, 2])], True) * gout[:, :, :3]).sum().backward()
    for f in range(F):
        g = lt.r_c2w[f].grad
        if f in (5, 2, 0):
            assert K.rel_err(g[:, :2].numpy(), leaf.grad[f].numpy()) <= K.FLOOR, f
            assert not prior or not g[:, 2].any()
        else:
            assert g is None or not g.any(), f
    assert torch.equal(lt.t_c2w[2].grad, gout[[1, 3, 4], :, 3].sum(0)) or K.rel_err(
        lt.t_c2w[2].grad.numpy(), gout[[1, 3, 4], :, 3].double().sum(0).numpy()) <= K.FLOOR


def test_tolerance_rule():
    """The three regimes: the floor, 4 e32, the cap of the quantity."""
    assert K.tolerance(0.0, "rays") == K.tolerance(1e-8, "g_focal") == K.FLOOR == 8 * 2.0 ** -24
    assert K.tolerance(1e-6, "rays") == K.tolerance(1e-6, "g_cam2world") == K.tolerance(1e-6, "g_a1") == 4e-6
    assert K.tolerance(1.0, "rays") == K.tolerance(1.0, "directions") == K.tolerance(1.0, "rgbs") == K.tolerance(1.0, "c2w") == 1e-5
    for q in ("g_cam2world", "g_world2rf", "g_focal", "g_center", "g_rgb_f", "g_depth_f", "g_exposure"):
        assert K.tolerance(1.0, q) == 2e-5
    assert K.tolerance(1.0, "g_a1") == K.tolerance(1.0, "g_a2") == 1e-5 and K.tolerance(1.0, "g_trans") == 1e-6
    assert K.tolerance(2e-7, "g_trans") == 8e-7


def test_the_three_summation_orders_differ_and_agree():
    """seq and k256 are other orders of the same terms: different bits from ATen's on a long sum, the same value in float64."""
    c, ref = K.rays_case("one_view/pinhole"), K.rays_ref("one_view/pinhole")
    r32 = {o: K.rays_run(c, torch.float32, o) for o in K.ORDERS}
    assert not np.array_equal(r32["seq"]["g_cam2world"], r32["k256"]["g_cam2world"])
    for o in K.ORDERS[1:]:
        r64 = K.rays_run(c, torch.float64, o)
        for q in K.RAYS_REDUCED:
            assert K.rel_err(r64[q], ref[q]) <= 1e-13, (o, q)
