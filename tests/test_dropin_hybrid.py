"""The drop-in surface (north_star: "so train.py drops it in unchanged"), as far as it can be exercised without a GPU,
against the reference's classes as recorded in tests/golden/dropin_reference_classes.npz (make_golden.py::case_dropin;
its seeded tensors are stored as digests of their bytes, so "equal" below is bit for bit):
this package's `LocalTensorfs` over its own `TensorVMSplit` -- INTEGRATION.md "Level 1" -- runs the lifecycle the
reference's scene class runs on a field and ends in the reference's state: construction from `tensorf_args`,
`append_frame`, `append_rf` (which parks the finished field with `.to("cpu")`, local_tensorfs.py:132), the device
shuffles of forward (:432-434,476-479), `get_optparam_groups` (group order is read by index, train.py:480,485),
`get_kwargs`, `save` -> `load`, and `forward` failing loudly (NativeError) where there is no GPU; every public member of
the reference's `TensorVMSplit` exists on the native class; seeded non-default colour networks have the reference's
state dict."""
import json

import pytest
import torch

from util import FIELD_KW, load_golden, quiet, tensor_digest

PE_CFGS = [dict(view_pe=2, fea_pe=2, featureC=64), dict(view_pe=6, fea_pe=0, featureC=128), dict(view_pe=0, fea_pe=6, featureC=256)]


@pytest.fixture(scope="module")
def ref():
    g = load_golden("dropin_reference_classes")
    g["keys"], g["digests"] = json.loads(str(g["keys"])), json.loads(str(g["digests"]))
    return g


def _scene(lt_cls, grid=(12, 12, 10)):     # x == y: the reference's load() swaps them (local_tensorfs.py:341)
    torch.manual_seed(7)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    return quiet(lt_cls, fov=85.6, n_init_frames=5, n_overlap=3, WH=(32, 24), n_iters_per_frame=600,
                 n_iters_reg=100, lr_R_init=5e-3, lr_t_init=5e-4, lr_i_init=1e-3, lr_exposure_init=1e-3, rf_lr_init=0.02,
                 rf_lr_basis=1e-3, lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[],
                 camera_prior=None, device="cpu", lr_upsample_reset=True, aabb=aabb, gridSize=list(grid), **FIELD_KW)


def test_scene_lifecycle_over_native_fields_ends_in_the_reference_state(ref, tmp_path):
    import localrf_amd
    from localrf_amd._native import NativeError
    lt = _scene(localrf_amd.LocalTensorfs)
    assert isinstance(lt.tensorfs[0], localrf_amd.TensorVMSplit)
    for _ in range(3):
        quiet(lt.append_frame)
    quiet(lt.append_rf, 3)                                  # parks field 0 with .to(torch.device("cpu")) (:132)
    assert len(lt.tensorfs) == 2 and tuple(lt.blending_weights.shape) == tuple(ref["scene_blend_shape"])
    assert lt.blending_weights.shape == (len(lt.r_c2w), 2)
    assert lt.tensorfs[0].device == torch.device("cpu")
    # the reference's LocalTensorfs after the same calls: every tensor of its state, bit for bit, and its kwargs
    sd = lt.state_dict()
    assert list(sd) == ref["keys"]["scene"]
    for k in sd:
        assert tensor_digest(sd[k]) == ref["digests"]["scene/" + k], k
    ka, kb = lt.get_kwargs(), json.loads(str(ref["scene_kwargs"]))
    assert set(ka) == set(kb) and all(str(ka[k]) == kb[k] for k in ka), (ka, kb)
    # the device shuffles of forward (:432-434, :476-479): .to() returns the module, keeps every attribute a forward reads
    f = lt.tensorfs[0]
    assert f.to(torch.device("cpu")) is f and f.to("cpu") is f
    for attr in ("aabb", "gridSize", "device", "alphaMask", "nSamples", "stepSize", "density_plane", "density_line",
                 "app_plane", "app_line", "basis_mat", "renderModule"):
        assert hasattr(f, attr), attr
    # optimiser groups: the order train.py:480,485 indexes, same tensors as the reference class yields
    torch.manual_seed(3)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    mine = quiet(localrf_amd.TensorVMSplit, "cpu", aabb, [12, 14, 10], **FIELD_KW)
    ga = mine.get_optparam_groups(0.02, 1e-3)
    assert len(ga) == len(ref["groups_lr"]) == 6
    for i, a in enumerate(ga):
        pa = list(a["params"])
        assert a["lr"] == float(ref["groups_lr"][i]) and len(pa) == int(ref["groups_n"][i])
        for j, p in enumerate(pa):                          # same seed -> same parameters, group by group
            assert tensor_digest(p) == ref["digests"][f"group{i}/{j}"], (i, j)
    assert list(mine.state_dict().keys()) == ref["keys"]["field"]
    ka, kb = mine.get_kwargs(), json.loads(str(ref["field_kwargs"]))
    assert set(ka) == set(kb) and all(str(ka[k]) == kb[k] for k in ka if k != "aabb")
    # save -> load: the checkpoint round trip over native fields
    path = str(tmp_path / "ckpt.th")
    lt.save(path)
    ckpt = torch.load(path, weights_only=False)
    kw = dict(ckpt["kwargs"])
    kw["device"] = "cpu"                                    # as train.py:182-191 rebuilds a scene from a checkpoint
    lt2 = quiet(localrf_amd.LocalTensorfs, **kw)
    quiet(lt2.load, ckpt["state_dict"])
    sd, sd2 = lt.state_dict(), lt2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    # the render path itself has no CPU fallback: loud, typed failure
    ray_ids = torch.randint(0, 32 * 24, (2 * 16,))
    with pytest.raises(NativeError):
        lt(ray_ids, torch.tensor([0, 1]), 32, 24, is_train=True)
    with pytest.raises(NativeError):
        lt.tensorfs[-1](torch.randn(8, 6))


def test_members_of_the_reference_class_exist_on_the_native_one(ref):
    """Every public attribute of the reference's TensorVMSplit (methods included) exists on the native class: live ones
    are implemented, dead ones (no caller in train.py / renderer.py / local_tensorfs.py) are real wrappers where that is
    two lines (compute_features, get_arange, save, init_render_func) and loud NotImplementedError stubs otherwise."""
    import localrf_amd
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    torch.manual_seed(5)
    mine = quiet(localrf_amd.TensorVMSplit, "cpu", aabb, [8, 8, 8], **FIELD_KW)
    assert len(ref["keys"]["members"]) > 50
    missing = [n for n in ref["keys"]["members"] if not hasattr(mine, n)]
    assert missing == [], missing
    theirs = torch.from_numpy(ref["get_arange_1"])
    assert mine.get_arange(1).shape == theirs.shape and torch.allclose(mine.get_arange(1), theirs, atol=1e-5)
    for call in (lambda: mine.sample_ray_ndc(torch.zeros(1, 3), torch.ones(1, 3)), lambda: mine.shrink(aabb),
                 lambda: mine.filtering_rays(torch.zeros(4, 6), torch.zeros(4, 3))):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.parametrize("cfg", PE_CFGS)
def test_nondefault_colour_network_has_the_reference_state_dict(ref, cfg):
    """opt.py:148-157 off their defaults: the native class builds the same parameter tensors (names, shapes, values under
    the same seed) as the reference's, so checkpoints interchange; the generic engine (csrc/lrf_generic.inl) renders them."""
    import localrf_amd
    i = PE_CFGS.index(cfg)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    kw = dict(FIELD_KW, **cfg)
    torch.manual_seed(9)
    mine = quiet(localrf_amd.TensorVMSplit, "cpu", aabb, [10, 12, 8], **kw)
    sd_m = mine.state_dict()
    assert list(sd_m) == ref["keys"][f"pe{i}"]
    for k in sd_m:
        assert tensor_digest(sd_m[k]) == ref["digests"][f"pe{i}/{k}"], k
    # the reference's checkpoint is, tensor for tensor, bit-identical to sd_m (digests above): it loads
    mine.load_state_dict({k: v.clone() for k, v in sd_m.items()})
    assert mine.get_kwargs()["view_pe"] == cfg["view_pe"] and mine.get_kwargs()["fea_pe"] == cfg["fea_pe"] and mine.get_kwargs()["featureC"] == cfg["featureC"]
