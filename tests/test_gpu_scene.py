"""The scene-end kernels of csrc/lrf_scene.inl (k_scene_rays / _bwd, k_scene_blend / _bwd, k_pose_assemble / _bwd) on the GPU at
the launch shapes and edge inputs of tests/scene_cases.py, held to its float64 references: training's 16 views x 256 rays with
one squeezed field, rays per view either side of the 64-lane and 256-thread strides, a full frame per view, pixel ids above
2^31, [V,4,4] poses, absent and non-contiguous incoming gradients, colours exactly on the clamp, a view without weight, 6D
columns far from unit length, frame lists either side of LRF_POSE_MAX with a frame named three times, the three-view quirk.

Tolerances: K.tolerance(K.E32[case][quantity], quantity) -- 4 x the error of the float32 CPU chain against float64 (for the
per-view sums: the largest of three summation orders), not below 8 roundings, not above the 1e-5 / 2e-5 / 1e-5 / 1e-6 of
tests/test_gpu_training.py; tests/test_scene_host.py keeps E32 current and checks the conditions under which zero clamp flips
can be demanded.  Every case runs twice and must return the same bits.  The direct calls of the entry points run on tensors
carved out of a sentinel pool (util.Pool), 16-byte aligned and one float past that.

Measured on an MI355X: docs/SCENE_KERNEL_FIGURES.md lists e32, tolerance and the kernels' error per case and quantity (the
tests print them).  The closest any quantity comes to its tolerance is 0.36 of it (`g_a1` of pose `sizes-63-0.3`: 2.1e-7 under
5.8e-7)."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_cases as K
from localrf_amd import _native as N
from localrf_amd import scene as scene_mod
from localrf_amd.scene_ops import pose_assemble, scene_blend, scene_rays
from util import FIELD_KW, PAD, Pool, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNWRITTEN = 0x7FD5A5A5                # a NaN no kernel computes: an output element still holding it was not written


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _report(tag, rows):
    """rows: (quantity, error, e32, tolerance).  Every figure is printed before anything is asserted."""
    for q, err, e32, tol in rows:
        print(f"[{tag}] {q:14s} e32 {e32:.2e}  tolerance {tol:.2e}  kernel {err:.2e}")
    over = [(q, err, tol) for q, err, e32, tol in rows if not err <= tol]
    assert not over, (tag, over)


def _rows(key, quantities, got, ref):
    e32 = K.E32[key]
    return [(q, K.rel_err(got[q].reshape(ref[q].shape), ref[q]), e32[q], K.tolerance(e32[q], q)) for q in quantities]


def _same_bits(a, b, tag):
    assert set(a) == set(b)
    for q in a:
        if a[q] is None or b[q] is None:
            assert a[q] is None and b[q] is None, (tag, q)
        else:
            assert a[q].shape == b[q].shape and np.array_equal(_bits(a[q]), _bits(b[q])), (tag, q, "bits differ")


def _leaf(t):
    return t.to(DEV).clone().requires_grad_(True)


def _grad(outs, leaves):
    gs = torch.autograd.grad([o for o, _ in outs], leaves, [g for _, g in outs], allow_unused=True)
    torch.cuda.synchronize()
    return [None if g is None else _host(g) for g in gs]


# ------------------------------------------------------------------------------------------------------------------ rays
def _run_rays(c, squeeze=None, c2w=None):
    """The case through scene_ops.scene_rays -> {quantity: array}; rays always as [n_rf,R,6].  The cotangents go in as
    grad_outputs, so an unused output reaches the backward as None (set_materialize_grads(False)) and a strided one strided."""
    squeeze = c["squeeze"] if squeeze is None else squeeze
    L = [_leaf(c["c2w"] if c2w is None else c2w), _leaf(c["w2rf"]), _leaf(c["focal"]), _leaf(c["center"])]
    rays, dirs, ij = scene_rays(c["ids"].to(DEV), *L, c["per_view"], c["W"], c["H"], fov360=c["fov360"], squeeze=squeeze)
    assert rays.shape == ((c["R"], 6) if squeeze else (c["n_rf"], c["R"], 6)) and not ij.requires_grad
    out = {"rays": _host(rays).reshape(c["n_rf"], c["R"], 6), "directions": _host(dirs), "ij": _host(ij)}
    if c["forward_only"]:
        return out
    g_rays = c["g_rays"].to(DEV)
    if c["strided"]:                                            # every other element of a twice as wide buffer
        wide = torch.full((c["n_rf"], c["R"], 12), float("nan"), device=DEV)
        wide[..., ::2] = g_rays
        g_rays = wide[..., ::2]
        assert not g_rays.is_contiguous()
    outs = ([(rays, g_rays[0] if squeeze else g_rays)] if c["use_rays"] else []) + ([(dirs, c["g_dirs"].to(DEV))] if c["use_dirs"] else [])
    g = _grad(outs, L)
    out.update(g_cam2world=g[0], g_world2rf=g[1], g_focal=g[2], g_center=g[3])
    return out


@pytest.mark.parametrize("name", K.RAYS_CASES)
def test_scene_rays_against_float64(name):
    """scene_rays and its backward against K.rays_ref: rays, directions and every gradient within the tolerance, ij exactly
    equal, 360 rays leave focal and centre without a gradient, two runs bit-identical.  train (squeeze=True): bit-identical to
    [0] of the unsqueezed call, gradients included.  pose44: bit-identical to passing [:, :3, :], the last row's gradient
    exactly zero.  dirs_only: cam2world and world2rf get exact zeros, the intrinsics their gradient.  no_dirs_grad: the
    reference differentiates the rays term alone."""
    c, ref = K.rays_case(name), K.rays_ref(name)
    a, b = _run_rays(c), _run_rays(c)
    _same_bits(a, b, name)
    assert np.array_equal(a["ij"], ref["ij"]) and a["ij"].dtype == np.int64
    kind = name.split("/")[0]
    if not c["forward_only"]:
        if c["fov360"]:
            assert a["g_focal"] is None and a["g_center"] is None
        if kind == "pose44":
            assert a["g_cam2world"].shape == (c["V"], 4, 4) and not a["g_cam2world"][:, 3].any()
            a["g_cam2world"] = a["g_cam2world"][:, :3]
            _same_bits(a, _run_rays(c, c2w=c["c2w"][:, :3, :]), name)
        if kind == "dirs_only":
            assert not a["g_cam2world"].any() and not a["g_world2rf"].any()
            assert c["fov360"] or (a["g_focal"].any() and a["g_center"].all())
        if c["squeeze"]:
            _same_bits(a, _run_rays(c, squeeze=False), name)
    for q in K.rays_quantities(c):
        assert np.isfinite(a[q]).all(), q
    _report(f"rays:{name}", _rows(f"rays:{name}", K.rays_quantities(c), a, ref))


# ------------------------------------------------------------------------------------------------------------------ blend
def _run_blend(c):
    L = [_leaf(c["rgb_f"]), _leaf(c["dep_f"])] + ([] if c["exposure"] is None else [_leaf(c["exposure"])])
    rgbs, depth = scene_blend(L[0], L[1], c["bw"].to(DEV), L[2] if len(L) == 3 else None, c["per_view"])
    g = _grad([(rgbs, c["g_rgbs"].to(DEV))] + ([(depth, c["g_depth"].to(DEV))] if c["use_depth"] else []), L)
    out = {"rgbs": _host(rgbs), "depth": _host(depth), "g_rgb_f": g[0], "g_depth_f": g[1]}
    if len(L) == 3:
        out["g_exposure"] = g[2]
    return out


@pytest.mark.parametrize("name", K.BLEND_CASES)
def test_scene_blend_against_float64(name):
    """scene_blend and its backward against K.blend_ref, zero clamp flips, two runs bit-identical.  boundary: where y is exactly
    0 or 1 the gradient of the colours is the incoming one bit for bit (ATen's clamp backward passes y >= 0 and y <= 1), at
    -0.25 and 1.25 it is exactly zero.  zero_weight_view: that view's per-field gradients are exactly zero.  no_depth_grad:
    the depth output is unused, the per-field depth gradient exactly zero.  no_exposure: no exposure, with a tape."""
    c, ref = K.blend_case(name), K.blend_ref(name)
    a, b = _run_blend(c), _run_blend(c)
    _same_bits(a, b, name)
    assert set(a) == set(K.blend_quantities(c))
    flips = K.clamp_flips(a["rgbs"], ref["rgbs"])
    print(f"[blend:{name}] clamp flips {flips}, clamped share {K.clamped(ref['y']).mean():.3f}")
    assert flips == 0
    if c["boundary"]:
        h = c["R"] // 2
        on = (ref["y"][:h] == 0) | (ref["y"][:h] == 1)
        assert on.any() and np.array_equal(_bits(a["g_rgb_f"][0, :h]), _bits(c["g_rgbs"][:h].numpy()))
        assert not a["g_rgb_f"][0, h:].any()
        assert np.array_equal(a["rgbs"], ref["rgbs"])
    if c["zero_view"] is not None:
        lo, hi = c["zero_view"] * c["per_view"], (c["zero_view"] + 1) * c["per_view"]
        assert not a["g_rgb_f"][:, lo:hi].any() and not a["g_depth_f"][:, lo:hi].any() and a["g_rgb_f"][:, :lo].any()
    if not c["use_depth"]:
        assert not a["g_depth_f"].any()
    _report(f"blend:{name}", _rows(f"blend:{name}", K.blend_quantities(c), a, ref))


# ------------------------------------------------------------------------------------------------------------------ pose
def _run_pose(c):
    """-> c2w, the per-FRAME gradients g_a1, g_a2, g_trans [F,3] (autograd adds up the slots that name a frame) and g_full
    [F,3,cols]."""
    rs, ts = [_leaf(r) for r in c["r"]], [_leaf(t) for t in c["t"]]
    r_list = [rs[f] if rs[f].shape[-1] == 2 else rs[f][:, :2] for f in c["frames"]]     # as LocalTensorfs.get_cam2world slices
    c2w = pose_assemble(r_list, [ts[f] for f in c["frames"]], cross_over_views=c["quirk"])
    g = _grad([(c2w, c["gout"].to(DEV))], rs + ts)
    gr, gt = np.stack(g[:c["F"]]), np.stack(g[c["F"]:])
    return {"c2w": _host(c2w), "g_a1": gr[..., 0], "g_a2": gr[..., 1], "g_trans": gt, "g_full": gr}


@pytest.mark.parametrize("name", K.POSE_CASES)
def test_pose_assemble_against_float64(name):
    """pose_assemble and its backward against K.pose_ref at V either side of LRF_POSE_MAX = 64 (one, two and three launches),
    both perturbation sizes, columns of norm 1e-3 and 1e3, the three-view quirk with and without a repeated frame; two runs
    bit-identical.  repeat: the gradient of the frame named in all three launches is the sum of its three slots' float64
    gradients.  prior33: column 2 of a [3,3] parameter's gradient is exactly zero."""
    c, ref = K.pose_case(name), K.pose_ref(name)
    a, b = _run_pose(c), _run_pose(c)
    _same_bits(a, b, name)
    assert N.LRF_POSE_MAX == 64
    full = a.pop("g_full")
    if name == "prior33":
        assert full.shape == (c["F"], 3, 3) and not full[:, :, 2].any() and full[:, :, :2].all()
    rows = _rows(f"pose:{name}", K.POSE_Q, a, ref)
    if name == "repeat":
        slots = ref["slots_r"][[3, 64, 128]]
        want = slots.sum(0)
        for k, q in ((0, "g_a1"), (1, "g_a2")):                 # frame 3 alone, on the scale of the whole tensor as the row above
            err = float(np.abs(a[q][3] - want[:, k]).max() / np.abs(ref[q]).max())
            rows.append((f"{q}[3]", err, K.E32["pose:repeat"][q], K.tolerance(K.E32["pose:repeat"][q], q)))
            assert all(np.abs(a[q][3] - s[:, k]).max() > 1e-2 * np.abs(want[:, k]).max() for s in slots)    # no single slot's
    _report(f"pose:{name}", rows)


# ------------------------------------------------------------------------------------------------------------------ direct calls
class _Carver:
    """Inputs and outputs of a direct call, carved out of one sentinel pool.  Float buffers start 16-byte aligned (mis = 0) or
    one float past that (mis = 1); int64 buffers are 16-byte aligned float views reinterpreted.  Outputs are pre-filled with
    UNWRITTEN."""

    def __init__(self, floats, mis):
        self.pool, self.mis, self.outs = Pool(floats), mis, {}

    def f32(self, t):
        return self.pool.take(_host(t).astype(np.float32), mis=self.mis)

    def i64(self, t):
        v = self.pool.take(np.zeros(2 * t.numel())).view(torch.int64)
        v.copy_(t.reshape(-1))
        return v.view(t.shape)

    def out(self, name, *shape, i64=False):
        v = self.pool.take(np.zeros(shape + ((2,) if i64 else ())), mis=0 if i64 else self.mis)
        v.view(torch.int32).fill_(UNWRITTEN)
        self.outs[name] = v.reshape(-1).view(torch.int64).view(shape) if i64 else v
        return self.outs[name]

    def check(self, tag, only=None):
        """Every element of every output written and no NaN in it, the bytes between the views untouched."""
        torch.cuda.synchronize()
        for name, v in self.outs.items():
            if only is None or name in only:
                assert not bool((v.view(torch.int32) == UNWRITTEN).any()), (tag, name, "an element was not written")
                assert v.dtype == torch.int64 or not bool(torch.isnan(v).any()), (tag, name, "NaN: a read past an input")
        assert self.pool.intact(), (tag, "a write outside the views")

    def untouched(self, tag):
        torch.cuda.synchronize()
        for name, v in self.outs.items():
            assert bool((v.view(torch.int32) == UNWRITTEN).all()), (tag, name, "written by a rejected call")
        assert self.pool.intact(), tag


def _room(*counts):
    return sum(int(k) + 2 * PAD + 8 for k in counts) + PAD


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


DIRECT = ("train", "stride-1", "stride-65", "stride-257")


def _carve_rays(c, mis):
    R, n_rf, V = c["R"], c["n_rf"], c["V"]
    P = _Carver(_room(2 * R, V * 12, n_rf * 3, 1, 2, n_rf * R * 6, R * 3, n_rf * R * 6, R * 3, 4 * R, V * 12, V * 3, V * n_rf * 3), mis)
    i = dict(ids=P.i64(c["ids"]), c2w=P.f32(c["c2w"]), w2rf=P.f32(c["w2rf"]), focal=P.f32(c["focal"]), center=P.f32(c["center"]),
             g_rays=P.f32(c["g_rays"]), g_dirs=P.f32(c["g_dirs"]))
    o = dict(rays=P.out("rays", n_rf, R, 6), directions=P.out("directions", R, 3), ij=P.out("ij", R, 2, i64=True))
    return P, i, o


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("name", [f"{k}/{p}" for k in DIRECT for p in K.PROJ])
def test_direct_rays_calls_in_a_sentinel_pool(name, mis):
    """lrf_scene_rays / lrf_scene_rays_bwd through N.launch with every buffer inside a sentinel pool: rays, directions, ij,
    g_cam2world, g_intr and g_world2rf fully written, no NaN picked up from beyond an input, nothing written between the
    views, the inputs as they were; every result bit-identical to the autograd seam's."""
    c = K.rays_case(name)
    R, n_rf, V, dev = c["R"], c["n_rf"], c["V"], torch.device(DEV)
    P, i, o = _carve_rays(c, mis)
    fo, ce = (None, None) if c["fov360"] else (i["focal"], i["center"])
    N.launch("lrf_scene_rays", dev, i["ids"].data_ptr(), R, c["per_view"], N.ptr(i["c2w"]), N.ptr(i["w2rf"]), n_rf, N.ptr(fo), N.ptr(ce),
             c["W"], c["H"], int(c["fov360"]), N.ptr(o["rays"]), N.ptr(o["directions"]), o["ij"].data_ptr())
    P.check((name, "fwd"))
    g_c2w, g_intr, g_w2rf = P.out("g_cam2world", V, 3, 4), P.out("g_intr", V, 3), P.out("g_world2rf", V, n_rf, 3)
    N.launch("lrf_scene_rays_bwd", dev, i["ids"].data_ptr(), R, c["per_view"], N.ptr(i["c2w"]), n_rf, N.ptr(fo), N.ptr(ce), c["W"], c["H"],
             int(c["fov360"]), N.ptr(i["g_rays"]), N.ptr(i["g_dirs"]), N.ptr(g_c2w), N.ptr(g_intr), N.ptr(g_w2rf))
    P.check((name, "bwd"))
    for k, t in i.items():
        assert torch.equal(t.cpu().reshape(-1), c[k].reshape(-1)), (k, "an input was changed")
    s = g_intr.clone().sum(0)                                   # the seam's own reductions over the views, on a tensor of its own
    got = {"rays": o["rays"], "directions": o["directions"], "ij": o["ij"], "g_cam2world": g_c2w, "g_world2rf": g_w2rf.clone().sum(0),
           "g_focal": None if c["fov360"] else s[0:1], "g_center": None if c["fov360"] else s[1:3]}
    _same_bits({k: None if v is None else _host(v) for k, v in got.items()}, _run_rays(c), name)


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("name", DIRECT)
def test_direct_blend_calls_in_a_sentinel_pool(name, mis):
    """lrf_scene_blend / lrf_scene_blend_bwd inside a sentinel pool: rgbs, depth, pre, g_rgb_f, g_depth_f and g_exposure fully
    written, nothing else touched, bit-identical to the autograd seam's."""
    c = K.blend_case(name)
    R, n_rf, V, dev = c["R"], c["n_rf"], c["V"], torch.device(DEV)
    P = _Carver(_room(n_rf * R * 3, n_rf * R, V * n_rf, V * 9, R * 3, R, R * 3, R, R * 3, n_rf * R * 3, n_rf * R, V * 9), mis)
    i = dict(rgb_f=P.f32(c["rgb_f"]), dep_f=P.f32(c["dep_f"]), bw=P.f32(c["bw"]), exposure=P.f32(c["exposure"]),
             g_rgbs=P.f32(c["g_rgbs"]), g_depth=P.f32(c["g_depth"]))
    rgbs, depth, pre = P.out("rgbs", R, 3), P.out("depth", R), P.out("pre", R, 3)
    N.launch("lrf_scene_blend", dev, N.ptr(i["rgb_f"]), N.ptr(i["dep_f"]), N.ptr(i["bw"]), N.ptr(i["exposure"]), R, c["per_view"], n_rf,
             N.ptr(rgbs), N.ptr(depth), N.ptr(pre))
    P.check((name, "fwd"))
    g_rgb_f, g_dep_f, g_ex = P.out("g_rgb_f", n_rf, R, 3), P.out("g_depth_f", n_rf, R), P.out("g_exposure", V, 3, 3)
    N.launch("lrf_scene_blend_bwd", dev, N.ptr(i["g_rgbs"]), N.ptr(i["g_depth"]), N.ptr(pre), N.ptr(i["bw"]), N.ptr(i["exposure"]), R,
             c["per_view"], n_rf, N.ptr(g_rgb_f), N.ptr(g_dep_f), N.ptr(g_ex))
    P.check((name, "bwd"))
    for k, t in i.items():
        assert torch.equal(t.cpu().reshape(-1), c[k].reshape(-1)), (k, "an input was changed")
    got = {"rgbs": rgbs, "depth": depth, "g_rgb_f": g_rgb_f, "g_depth_f": g_dep_f, "g_exposure": g_ex}
    _same_bits({k: _host(v) for k, v in got.items()}, _run_blend(c), name)


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("name", ["sizes-1-0.3", "sizes-64-0.3"])
def test_direct_pose_calls_in_a_sentinel_pool(name, mis):
    """lrf_pose_assemble / _bwd at V = 1 and V = LRF_POSE_MAX with every frame's parameters a buffer of its own inside a
    sentinel pool: cam2world, g_r6d and g_trans fully written, nothing else touched, bit-identical to the autograd seam's."""
    c = K.pose_case(name)
    V, dev = c["F"], torch.device(DEV)
    P = _Carver(_room(*([6] * V + [3] * V + [V * 12] * 2 + [V * 6, V * 3])), mis)
    rs, ts, gout = [P.f32(r) for r in c["r"]], [P.f32(t) for t in c["t"]], P.f32(c["gout"])
    c2w, g_r, g_t = P.out("cam2world", V, 3, 4), P.out("g_r6d", V, 3, 2), P.out("g_trans", V, 3)
    N.launch("lrf_pose_assemble", dev, _table(rs), _table(ts), V, 0, N.ptr(c2w))
    P.check((name, "fwd"), only={"cam2world"})
    N.launch("lrf_pose_assemble_bwd", dev, _table(rs), V, 0, N.ptr(gout), N.ptr(g_r), N.ptr(g_t))
    P.check((name, "bwd"))
    seam = _run_pose(c)
    got = {"c2w": _host(c2w), "g_a1": _host(g_r)[..., 0], "g_a2": _host(g_r)[..., 1], "g_trans": _host(g_t), "g_full": _host(g_r)}
    _same_bits(got, seam, name)


def test_rejected_arguments_launch_nothing():
    """R not a multiple of rays-per-view, rays-per-view 0, null pinhole intrinsics; V = 0, V = LRF_POSE_MAX + 1 and cross_views
    with V != 3 for the pose calls: each returns non-zero with a message, writes no output element and leaves the pool intact."""
    lib, st = N.lib(), _stream()
    c = K.rays_case("stride-65/pinhole")
    R, n_rf, V, pv = c["R"], c["n_rf"], c["V"], c["per_view"]
    P, i, o = _carve_rays(c, 0)
    g_c2w, g_intr, g_w2rf = P.out("g_cam2world", V, 3, 4), P.out("g_intr", V, 3), P.out("g_world2rf", V, n_rf, 3)
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(R_, pv_, fo, ce, fov=0):
        return lib.lrf_scene_rays(p(i["ids"]), R_, pv_, p(i["c2w"]), p(i["w2rf"]), n_rf, p(fo), p(ce), c["W"], c["H"], fov, p(o["rays"]),
                                  p(o["directions"]), p(o["ij"]), st)

    def bwd(R_, pv_, fo, ce, fov=0):
        return lib.lrf_scene_rays_bwd(p(i["ids"]), R_, pv_, p(i["c2w"]), n_rf, p(fo), p(ce), c["W"], c["H"], fov, p(i["g_rays"]), p(i["g_dirs"]),
                                      p(g_c2w), p(g_intr), p(g_w2rf), st)

    for call in (fwd, bwd):
        for args in ((R - 1, pv, i["focal"], i["center"]), (R, 0, i["focal"], i["center"]), (R, pv, None, i["center"]),
                     (R, pv, i["focal"], None), (R, pv, None, None), (R - 1, pv, None, None, 1), (R, 0, None, None, 1)):
            assert call(*args) != 0 and lib.lrf_last_error(), (call.__name__, args[:2])
    P.untouched("rays")

    b = K.blend_case("stride-65")
    R, n_rf, V, pv = b["R"], b["n_rf"], b["V"], b["per_view"]
    P = _Carver(_room(n_rf * R * 3, n_rf * R, V * n_rf, V * 9, R * 3, R, R * 3, R, R * 3, R * 3, n_rf * R * 3, n_rf * R, V * 9), 0)
    i = {k: P.f32(b[k]) for k in ("rgb_f", "dep_f", "bw", "exposure", "g_rgbs", "g_depth")}
    pre_in = P.f32(torch.rand(R, 3))
    outs = [P.out(k, *s) for k, s in (("rgbs", (R, 3)), ("depth", (R,)), ("pre", (R, 3)), ("g_rgb_f", (n_rf, R, 3)), ("g_depth_f", (n_rf, R)),
                                      ("g_exposure", (V, 3, 3)))]
    for R_, pv_ in ((R - 1, pv), (R, 0)):
        assert lib.lrf_scene_blend(p(i["rgb_f"]), p(i["dep_f"]), p(i["bw"]), p(i["exposure"]), R_, pv_, n_rf, p(outs[0]), p(outs[1]),
                                   p(outs[2]), st) != 0
        assert lib.lrf_scene_blend_bwd(p(i["g_rgbs"]), p(i["g_depth"]), p(pre_in), p(i["bw"]), p(i["exposure"]), R_, pv_, n_rf, p(outs[3]),
                                       p(outs[4]), p(outs[5]), st) != 0
    P.untouched("blend")

    n = N.LRF_POSE_MAX + 1
    q = K.pose_case("sizes-65-0.3")
    P = _Carver(_room(*([6] * n + [3] * n + [n * 12] * 2 + [n * 6, n * 3])), 0)
    rs, ts, gout = [P.f32(r) for r in q["r"]], [P.f32(t) for t in q["t"]], P.f32(q["gout"])
    c2w, g_r, g_t = P.out("cam2world", n, 3, 4), P.out("g_r6d", n, 3, 2), P.out("g_trans", n, 3)
    for V_, cross in ((0, 0), (n, 0), (2, 1), (4, 1), (1, 1), (N.LRF_POSE_MAX, 1)):
        assert lib.lrf_pose_assemble(_table(rs), _table(ts), V_, cross, p(c2w), st) != 0, (V_, cross)
        assert lib.lrf_pose_assemble_bwd(_table(rs), V_, cross, p(gout), p(g_r), p(g_t), st) != 0, (V_, cross)
    P.untouched("pose")
    with pytest.raises(ValueError):
        scene_rays(c["ids"].to(DEV)[:-1], c["c2w"].to(DEV), c["w2rf"].to(DEV), c["focal"].to(DEV), c["center"].to(DEV), pv, c["W"], c["H"])
    with pytest.raises(ValueError):
        pose_assemble([r.to(DEV) for r in q["r"][:4]], [t.to(DEV) for t in q["t"][:4]], cross_over_views=True)


# ------------------------------------------------------------------------------------------------------------------ LocalTensorfs
def _scene(grid=(20, 24, 28), seed=5):
    from localrf_amd import LocalTensorfs
    torch.manual_seed(seed)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]]).to(DEV)
    lt = quiet(LocalTensorfs, fov=85.6, n_init_frames=4, n_overlap=3, WH=(40, 30), n_iters_per_frame=600, n_iters_reg=100,
               lr_R_init=5e-3, lr_t_init=5e-4, lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
               lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[], camera_prior=None, device=DEV,
               lr_upsample_reset=True, aabb=aabb, gridSize=list(grid), **FIELD_KW)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in range(len(lt.r_c2w)):
            lt.t_c2w[i].add_(0.05 * torch.randn(3, generator=g).to(DEV))
            lt.r_c2w[i].add_(0.05 * torch.randn(3, 2, generator=g).to(DEV))
            lt.exposure[i].add_(0.05 * torch.randn(3, 3, generator=g).to(DEV))
        for p in lt.tensorfs[-1].density_plane:
            p.mul_(3.0)
    return lt


def test_three_view_batch_with_a_frame_drawn_twice(monkeypatch):
    """A training batch of three views [2, 2, 0] with reference_cross on, through LocalTensorfs: views are drawn with replacement,
    so the quirk meets a repeated frame.  The scene-level ends are held to the float64 chain on what the field's backward
    handed them: g_cam2world against K.rays_run on the captured ray gradient, the 6D and translation gradients against
    K.pose_run on the captured g_cam2world.  e32 is measured here, by the same functions on the same captured cotangents."""
    lt = _scene()
    assert lt.reference_cross
    seen = {}

    def spy(ray_ids, cam2world, shifts, focal, center, per_view, W, H, fov360=False, squeeze=False):
        rays, dirs, ij = scene_rays(ray_ids, cam2world, shifts, focal, center, per_view, W, H, fov360, squeeze=squeeze)
        seen.update(ids=ray_ids, c2w=cam2world.detach(), w2rf=shifts.detach(), focal=focal.detach(), center=center.detach(), per_view=per_view,
                    squeeze=squeeze, rays=rays.detach())
        rays.register_hook(lambda g: seen.update(g_rays=g.detach().clone()))
        cam2world.register_hook(lambda g: seen.update(g_c2w=g.detach().clone()))
        return rays, dirs, ij

    monkeypatch.setattr(scene_mod, "scene_rays", spy)
    gen = torch.Generator().manual_seed(11)
    frames, per = [2, 2, 0], 65
    ray_ids = torch.randint(0, lt.W * lt.H, (3 * per,), generator=gen).to(DEV)
    rgb, depth, _, _ = lt(ray_ids, torch.tensor(frames).to(DEV), lt.W, lt.H, is_train=True)
    ((rgb * (0.5 + torch.randn(3 * per, 3, generator=gen)).to(DEV)).sum() + (depth * torch.randn(3 * per, generator=gen).to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert seen["squeeze"] and seen["per_view"] == per and seen["c2w"].shape == (3, 3, 4)

    cpu = lambda t: t.detach().cpu()
    rc = dict(V=3, per_view=per, n_rf=1, R=3 * per, W=lt.W, H=lt.H, fov360=False, ids=cpu(ray_ids), c2w=cpu(seen["c2w"]), w2rf=cpu(seen["w2rf"]),
              focal=cpu(seen["focal"]).reshape(1), center=cpu(seen["center"]), g_rays=cpu(seen["g_rays"]).reshape(1, 3 * per, 6),
              g_dirs=None, use_rays=True, use_dirs=False, forward_only=False)
    ref = K.rays_run(rc, torch.float64)
    e_c2w = max(K.rel_err(K.rays_run(rc, torch.float32, o)["g_cam2world"], ref["g_cam2world"]) for o in K.ORDERS)
    e_rays = K.rel_err(K.rays_run(rc, torch.float32)["rays"], ref["rays"])
    rows = [("rays", K.rel_err(_host(seen["rays"]).reshape(1, -1, 6), ref["rays"]), e_rays, K.tolerance(e_rays, "rays")),
            ("g_cam2world", K.rel_err(_host(seen["g_c2w"]), ref["g_cam2world"]), e_c2w, K.tolerance(e_c2w, "g_cam2world"))]

    pc = dict(F=len(lt.r_c2w), frames=frames, quirk=True, r=torch.stack([cpu(r) for r in lt.r_c2w]), t=torch.stack([cpu(t) for t in lt.t_c2w]),
              gout=cpu(seen["g_c2w"]))
    pref, p32 = K.pose_run(pc, torch.float64), K.pose_run(pc, torch.float32)
    assert K.rel_err(_host(seen["c2w"]), pref["c2w"]) <= K.tolerance(K.rel_err(p32["c2w"], pref["c2w"]), "c2w")
    gr = np.stack([np.zeros((3, 2), np.float32) if r.grad is None else _host(r.grad) for r in lt.r_c2w])
    gt = np.stack([np.zeros(3, np.float32) if t.grad is None else _host(t.grad) for t in lt.t_c2w])
    for q, got in (("g_a1", gr[..., 0]), ("g_a2", gr[..., 1]), ("g_trans", gt)):
        e = K.rel_err(p32[q], pref[q])
        rows.append((q, K.rel_err(got, pref[q]), e, K.tolerance(e, q)))
    assert not gr[1].any() and not gr[3].any() and gr[2].any() and gr[0].any()       # frames 1 and 3 are not in the batch
    _report("scene:three_views_one_twice", rows)


@pytest.mark.parametrize("n_rays", [12, 10])
def test_no_valid_rf_returns_the_degenerate_tuple(n_rays, capsys):
    """An eval call whose supplied blending weights are all zero (local_tensorfs.py:420-422): ones for the colours and twice
    for the depth, directions and ij of the ray kernel for those ids -- also when n_rays is no multiple of n_views, which the
    reference never divides in this branch."""
    lt = _scene()
    gen = torch.Generator().manual_seed(12)
    ray_ids = torch.randint(0, 5 * lt.W * lt.H, (n_rays,), generator=gen).to(DEV)
    view_ids = torch.tensor([0, 2, 3]).to(DEV)
    with torch.no_grad():
        out = lt(ray_ids, view_ids, lt.W, lt.H, is_train=False, blending_weights=torch.zeros(3, len(lt.tensorfs), device=DEV))
        assert "No valid RF" in capsys.readouterr().out and len(out) == 5
        rgb, d1, d2, dirs, ij = out
        assert rgb.shape == (n_rays, 3) and bool((rgb == 1).all()) and rgb.dtype == torch.float32
        for d in (d1, d2):
            assert d.shape == (n_rays,) and d.dtype == torch.float32 and d.device == ray_ids.device and bool((d == 1).all())
        _, want_dirs, want_ij = scene_rays(ray_ids, lt.get_cam2world([0]), torch.zeros(1, 3, device=DEV), lt.focal(lt.W), lt.center(lt.W, lt.H),
                                           n_rays, lt.W, lt.H)
        assert torch.equal(dirs, want_dirs) and torch.equal(ij, want_ij)
    c = dict(ids=ray_ids.cpu(), W=lt.W, H=lt.H, fov360=False)
    ref = K.directions(c, torch.float64, lt.focal(lt.W).detach().cpu().double(), lt.center(lt.W, lt.H).detach().cpu().double())
    assert K.rel_err(_host(dirs), ref.numpy()) <= K.tolerance(0.0, "directions") and torch.equal(ij.cpu(), torch.stack(K.ids2pixel(c), -1))
