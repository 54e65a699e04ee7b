"""Shared pieces of the scene-end kernel tests (csrc/lrf_scene.inl): the cases, their float64 references in plain torch, and the
measured error of the float32 CPU evaluation of the same expressions, from which the GPU tolerances follow.

  rays_case(name) / rays_run(c, dtype)       ids -> (col, row) -> lean / 360 directions -> R d, t + shift per field; gradients of
                                             cam2world, world2rf, focal and center from autograd
  blend_case(name) / blend_run(c, dtype)     sum_k w rgb_k, sum_k w depth_k, bmm with the per-view exposure, clamp(0, 1)
  pose_case(name) / pose_run(c, dtype)       Gram-Schmidt, the cross product (over the VIEW axis for exactly three views with the
                                             quirk), cat with the translations
  *_check(name, seed)                        the conditions a seed has to meet -> (violations, e32)
  rel_err, tolerance, E32                    max|x - ref| / max|ref|; the tolerance rule; the recorded float32-CPU errors

Per-view sums.  The gradients of cam2world, world2rf, focal, center and exposure are sums over the rays of a view (and, for the
last four, over the views).  Their float32 error depends on the order of the sum, so e32 of such a quantity is the LARGEST error
of three float32 evaluations: ATen's own (autograd through the unexpanded leaves), a sequential sum, and 256 strided partial
sums added as four groups of 64 and then the four results -- the shape of the kernels' order (one 256-thread block per view,
a wave sum, four waves).  The terms of the last two are autograd's as well: the gradient with respect to the leaf repeated per
ray.  All three are arithmetic on the reference's terms, never on a kernel's output.

Nothing here touches a GPU or the HIP library.  Cited lines are relative to the reference's localTensoRF directory."""
import functools
import math

import numpy as np
import torch

from losses_cases import FLOOR, one_thread, rel_err  # noqa: F401  (re-exported: the tests read them from here)

CAP_VALUE, CAP_GRAD, CAP_POSE_ROT, CAP_POSE_TRANS = 1e-5, 2e-5, 1e-5, 1e-6     # what tests/test_gpu_training.py demands already
CANCEL = 0.05                           # a reduced output is at least this share of the largest sum of |terms|
MARGIN = 1e-4                           # no blended colour this close to 0 or 1 (outside `boundary`)
CLAMPED_SHARE = (0.02, 0.90)
STRIDES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
PROJ = ("pinhole", "360")
ORDERS = ("aten", "seq", "k256")

RAYS_REDUCED = ("g_cam2world", "g_world2rf", "g_focal", "g_center")
BLEND_Q = ("rgbs", "depth", "g_rgb_f", "g_depth_f", "g_exposure")
POSE_Q = ("c2w", "g_a1", "g_a2", "g_trans")

RAYS_CASES = ([f"{k}/{p}" for k in ["train"] + [f"stride-{n}" for n in STRIDES] + ["one_view", "frame", "big_ids"] for p in PROJ]
              + ["no_dirs_grad/pinhole"] + [f"{k}/{p}" for k in ("dirs_only", "pose44", "strided_grad") for p in PROJ])
BLEND_CASES = (["train"] + [f"stride-{n}" for n in STRIDES]
               + ["no_exposure", "no_depth_grad", "zero_weight_view", "boundary-none", "boundary-identity"])
POSE_SIZES = (1, 2, 3, 4, 63, 64, 65, 129)
POSE_CASES = ([f"sizes-{v}-{p}" for v in POSE_SIZES for p in (0.05, 0.3)] + [f"sizes-3q-{p}" for p in (0.05, 0.3)]
              + ["scaled-a", "scaled-b", "repeat", "quirk_repeat", "prior33"])

# Seeds found by the search of the *_check conditions on the CPU (first_seed): the first seed from 1 upwards that meets all of
# them.  A changed seed has to pass tests/test_scene_host.py.
SEEDS = {
    "train/pinhole": 1, "train/360": 1, "stride-1/pinhole": 1, "stride-1/360": 1, "stride-2/pinhole": 2, "stride-2/360": 1,
    "stride-63/pinhole": 1, "stride-63/360": 1, "stride-64/pinhole": 2, "stride-64/360": 1, "stride-65/pinhole": 1,
    "stride-65/360": 1, "stride-255/pinhole": 1, "stride-255/360": 1, "stride-256/pinhole": 1, "stride-256/360": 1,
    "stride-257/pinhole": 1, "stride-257/360": 1, "stride-1025/pinhole": 1, "stride-1025/360": 1, "one_view/pinhole": 1,
    "one_view/360": 1, "frame/pinhole": 1, "frame/360": 1, "big_ids/pinhole": 1, "big_ids/360": 1, "no_dirs_grad/pinhole":
    2, "dirs_only/pinhole": 2, "dirs_only/360": 1, "pose44/pinhole": 2, "pose44/360": 1, "strided_grad/pinhole": 2,
    "strided_grad/360": 1, "train": 4, "stride-1": 1, "stride-2": 1, "stride-63": 1, "stride-64": 1, "stride-65": 1,
    "stride-255": 1, "stride-256": 1, "stride-257": 1, "stride-1025": 1, "no_exposure": 1, "no_depth_grad": 1,
    "zero_weight_view": 1, "boundary-none": 1, "boundary-identity": 1, "sizes-1-0.05": 1, "sizes-1-0.3": 1, "sizes-2-0.05":
    1, "sizes-2-0.3": 1, "sizes-3-0.05": 1, "sizes-3-0.3": 1, "sizes-4-0.05": 1, "sizes-4-0.3": 1, "sizes-63-0.05": 1,
    "sizes-63-0.3": 1, "sizes-64-0.05": 1, "sizes-64-0.3": 1, "sizes-65-0.05": 1, "sizes-65-0.3": 1, "sizes-129-0.05": 1,
    "sizes-129-0.3": 1, "sizes-3q-0.05": 1, "sizes-3q-0.3": 1, "scaled-a": 1, "scaled-b": 1, "repeat": 1, "quirk_repeat": 1,
    "prior33": 1,
}


def cap_of(quantity):
    if quantity in ("g_a1", "g_a2"):
        return CAP_POSE_ROT
    if quantity == "g_trans":
        return CAP_POSE_TRANS
    return CAP_GRAD if quantity.startswith("g_") else CAP_VALUE


def tolerance(e32, quantity):
    """4 x the float32-CPU error, not below 8 roundings, not above what the project demands already."""
    return min(max(4.0 * e32, FLOOR), cap_of(quantity))


def _np(t):
    return t.detach().numpy().astype(np.float64)


def _seed(name, seed):
    return SEEDS[name] if seed is None else seed


def _grads(outs, leaves):
    """autograd.grad of the (output, cotangent) pairs that carry a tape; a leaf nothing depends on gets zeros."""
    outs = [(o, g) for o, g in outs if o.requires_grad]
    if not outs:
        return [torch.zeros_like(x) for x in leaves]
    gs = torch.autograd.grad([o for o, _ in outs], leaves, [g for _, g in outs], allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(gs, leaves)]


def _view_sum(terms, V, order):
    """terms [V * n, ...] -> [V, ...]: the sum over the n rays of each view in one of ORDERS[1:]."""
    x = terms.reshape((V, -1) + tuple(terms.shape[1:]))
    n = x.shape[1]
    if order == "seq":
        acc = torch.zeros_like(x[:, 0])
        for q in range(n):
            acc = acc + x[:, q]
        return acc
    steps = (n + 255) // 256                                    # thread t adds rays t, t + 256, ... in that order
    pad = torch.zeros((V, steps * 256) + tuple(x.shape[2:]), dtype=x.dtype)
    pad[:, :n] = x
    pad = pad.reshape((V, steps, 256) + tuple(x.shape[2:]))
    part = torch.zeros_like(pad[:, 0])
    for s in range(steps):
        part = part + pad[:, s]
    waves = part.reshape((V, 4, 64) + tuple(x.shape[2:])).sum(2)
    return ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]


def _seq(x):
    acc = torch.zeros_like(x[0])
    for v in range(x.shape[0]):
        acc = acc + x[v]
    return acc


def _poses(V, gen, rot=0.05, trans=0.2):
    r6 = torch.eye(3)[:, :2][None].repeat(V, 1, 1) + rot * torch.randn(V, 3, 2, generator=gen)
    b1 = torch.nn.functional.normalize(r6[..., 0], dim=-1)
    b2 = torch.nn.functional.normalize(r6[..., 1] - (b1 * r6[..., 1]).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.cat([torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=-1)], -1), trans * torch.randn(V, 3, 1, generator=gen)], -1)


# ------------------------------------------------------------------------------------------------------------------ rays
INTRINSICS = {(640, 480): (500.0, (288.0, 264.0)), (64, 48): (41.0, (30.5, 25.25)), (960, 540): (800.0, (470.25, 280.5))}


def _rays(seed, V, per_view, n_rf, WH=(64, 48), frames=7, lo=None, hi=None, **flags):
    gen = torch.Generator().manual_seed(seed)
    W, H = WH
    R = V * per_view
    lo, hi = (0, frames * W * H) if lo is None else (lo, hi)
    focal, center = INTRINSICS[WH]
    c = dict(V=V, per_view=per_view, n_rf=n_rf, W=W, H=H, ids=torch.randint(lo, hi, (R,), generator=gen, dtype=torch.int64),
             c2w=_poses(V, gen), w2rf=0.3 * torch.randn(n_rf, 3, generator=gen), focal=torch.tensor([focal]),
             center=torch.tensor(center), g_rays=0.7 + torch.randn(n_rf, R, 6, generator=gen),
             g_dirs=0.7 + torch.randn(R, 3, generator=gen), use_rays=True, use_dirs=True, squeeze=False, forward_only=False,
             strided=False, gen=gen)
    c.update(flags)
    return c


@functools.lru_cache(maxsize=None)
def rays_case(name, seed=None):
    """The inputs of a rays case as a dict of CPU tensors (float32 / int64).  The cotangents g_rays, g_dirs carry a mean of 0.7:
    the reduced gradients are then sums that do not cancel to nothing.  seed: another than SEEDS' (the seed search)."""
    kind, proj = name.split("/")
    seed = _seed(name, seed)
    if kind == "train":                                         # scripts/train_synth.py: 16 views x 256 rays, one field
        c = _rays(seed, 16, 256, 1, (640, 480), frames=900, squeeze=True)
    elif kind.startswith("stride-"):
        c = _rays(seed, 3, int(kind.split("-")[1]), 2)
    elif kind == "one_view":
        c = _rays(seed, 1, 4096, 4)
    elif kind == "frame":                                       # PosePlan's forward: a full frame per view, pixels in order
        c = _rays(seed, 3, 64 * 48, 2, forward_only=True)
        c["ids"] = (torch.arange(3)[:, None] * (64 * 48) + torch.arange(64 * 48)[None]).reshape(-1)
    elif kind == "big_ids":
        c = _rays(seed, 3, 100, 2, (960, 540), lo=2 ** 31, hi=2 ** 33)
    elif kind == "no_dirs_grad":
        c = _rays(seed, 3, 100, 2, use_dirs=False)
    elif kind == "dirs_only":
        c = _rays(seed, 3, 100, 2, use_rays=False)
    elif kind == "pose44":
        c = _rays(seed, 3, 100, 2)
        c["c2w"] = torch.cat([c["c2w"], torch.tensor([7.0, -3.0, 11.0, 5.0]).expand(3, 1, 4)], 1)   # a last row nobody may read
    elif kind == "strided_grad":
        c = _rays(seed, 3, 100, 2, strided=True)
    else:
        raise KeyError(name)
    c.pop("gen")
    c.update(name=name, fov360=proj == "360", R=c["V"] * c["per_view"])
    return c


def ids2pixel(c):
    """ids -> (col, row) (local_tensorfs.py:23-29)."""
    return c["ids"] % c["W"], (c["ids"] // c["W"]) % c["H"]


def directions(c, dtype, focal, center):
    """Lean and 360 directions (utils/ray_utils.py:14-37) in `dtype`; focal [1] or [R], center [2] or [R,2]."""
    col, row = ids2pixel(c)
    i, j = col.to(dtype) + 0.5, row.to(dtype) + 0.5
    if c["fov360"]:
        phi = j * math.pi / c["H"] - math.pi / 2.0
        theta = i * 2.0 * math.pi / c["W"] + math.pi
        return torch.stack([torch.cos(phi) * torch.sin(theta), torch.sin(phi), torch.cos(phi) * torch.cos(theta)], -1)
    return torch.stack([(i - center[..., 0]) / focal, -(j - center[..., 1]) / focal, -torch.ones_like(i)], -1)


def rays_forward(c, dtype, c2w, w2rf, focal, center, per_ray=False):
    """-> (rays [n_rf,R,6], directions [R,3]) (local_tensorfs.py:397-401,424-437,455-456).  per_ray: the leaves come repeated
    per ray (c2w [R,3,4], w2rf [n_rf,R,3], focal [R], center [R,2])."""
    dirs = directions(c, dtype, focal, center)
    M = c2w[:, :3, :]
    M = M if per_ray else M.repeat_interleave(c["per_view"], dim=0)
    d = torch.bmm(M[:, :, :3], dirs[..., None])[..., 0]
    rays = torch.stack([torch.cat([M[:, :, 3] + w2rf[k], d], -1) for k in range(c["n_rf"])], 0)
    return rays, dirs


def _rays_leaves(c, dtype, per_ray):
    n = c["per_view"]
    src = [c["c2w"], c["w2rf"], c["focal"], c["center"]]
    if per_ray:
        src = [c["c2w"].repeat_interleave(n, 0), c["w2rf"][:, None, :].repeat(1, c["R"], 1), c["focal"].repeat(c["R"]),
               c["center"][None].repeat(c["R"], 1)]
    return [t.to(dtype).clone().requires_grad_(True) for t in src]


def _rays_outs(c, dtype, rays, dirs):
    return ([(rays, c["g_rays"].to(dtype))] if c["use_rays"] else []) + ([(dirs, c["g_dirs"].to(dtype))] if c["use_dirs"] else [])


def rays_terms(c, dtype):
    """{reduced quantity: its per-ray terms} in `dtype`: autograd's gradient with respect to the leaves repeated per ray.
    g_cam2world [R,3,4], g_world2rf [R,n_rf,3], g_focal [R,1], g_center [R,2]."""
    with one_thread():
        L = _rays_leaves(c, dtype, True)
        rays, dirs = rays_forward(c, dtype, *L, per_ray=True)
        g = _grads(_rays_outs(c, dtype, rays, dirs), L)
    return {"g_cam2world": g[0][:, :3].detach(), "g_world2rf": g[1].permute(1, 0, 2).detach(), "g_focal": g[2][:, None].detach(),
            "g_center": g[3].detach()}


def rays_run(c, dtype, order="aten"):
    """The case on the CPU in `dtype` -> {quantity: float64 array}; ij as int64.  order: how the per-view sums of the reduced
    gradients are formed (ORDERS)."""
    with one_thread():
        L = _rays_leaves(c, dtype, False)
        rays, dirs = rays_forward(c, dtype, *L)
        out = {"rays": _np(rays), "directions": _np(dirs), "ij": torch.stack(ids2pixel(c), -1).numpy()}
        if c["forward_only"]:
            return out
        if order == "aten":
            g = _grads(_rays_outs(c, dtype, rays, dirs), L)
            red = {"g_cam2world": g[0][:, :3], "g_world2rf": g[1], "g_focal": g[2], "g_center": g[3]}
        else:
            red = {k: _view_sum(t, c["V"], order) for k, t in rays_terms(c, dtype).items()}
            red = {k: (v if k == "g_cam2world" else _seq(v)) for k, v in red.items()}
        for k in RAYS_REDUCED:
            if not (c["fov360"] and k in ("g_focal", "g_center")):
                out[k] = _np(red[k])
    return out


def rays_quantities(c):
    q = ["rays", "directions"]
    if not c["forward_only"]:
        q += ["g_cam2world", "g_world2rf"] + ([] if c["fov360"] else ["g_focal", "g_center"])
    return q


@functools.lru_cache(maxsize=None)
def rays_ref(name):
    return rays_run(rays_case(name), torch.float64)


def _cancellation(ref, terms64, V, keys, across):
    """Violations of: max|ref| >= CANCEL x the largest per-element sum of |terms| (float64)."""
    bad = []
    for k in keys:
        s = terms64[k].abs().reshape((V, -1) + tuple(terms64[k].shape[1:])).sum(1)
        s = float((s.sum(0) if k in across else s).max())
        if s > 0 and not float(np.abs(ref[k]).max()) >= CANCEL * s:
            bad.append(f"{k}: max|ref| {float(np.abs(ref[k]).max()):.3e} under {CANCEL} x the terms' {s:.3e} (cancellation)")
    return bad


def _e32(run, c, ref, quantities, reduced):
    runs = {o: run(c, torch.float32, o) for o in ORDERS}
    return {q: max(rel_err(runs[o][q], ref[q]) for o in (ORDERS if q in reduced else ORDERS[:1])) for q in quantities}


def _over_cap(e32):
    return [f"{q}: 4 e32 = {4 * e:.3e} over the cap {cap_of(q):.0e}" for q, e in e32.items() if not 4 * e <= cap_of(q)]


def rays_check(name, seed=None):
    """-> (violations, e32) of a rays case: bounded cancellation in every reduced gradient, 4 e32 under the caps."""
    c = rays_case(name, seed)
    ref = rays_ref(name) if seed is None else rays_run(c, torch.float64)
    q = rays_quantities(c)
    bad = []
    if not c["forward_only"]:
        bad += _cancellation(ref, rays_terms(c, torch.float64), c["V"], [k for k in RAYS_REDUCED if k in q],
                             ("g_world2rf", "g_focal", "g_center"))
    e32 = _e32(rays_run, c, ref, q, RAYS_REDUCED)
    return bad + _over_cap(e32), e32


# ------------------------------------------------------------------------------------------------------------------ blend
def _blend(seed, V, per_view, n_rf, ones=False, exposure=True, **flags):
    gen = torch.Generator().manual_seed(seed)
    R = V * per_view
    c = dict(V=V, per_view=per_view, n_rf=n_rf, R=R, rgb_f=torch.rand(n_rf, R, 3, generator=gen),
             dep_f=5 * torch.rand(n_rf, R, generator=gen), bw=torch.ones(V, n_rf) if ones else torch.rand(V, n_rf, generator=gen),
             exposure=(1.3 * torch.eye(3)[None] + 0.2 * torch.randn(V, 3, 3, generator=gen)) if exposure else None,
             g_rgbs=0.5 + torch.randn(R, 3, generator=gen), g_depth=0.5 + torch.randn(R, generator=gen), use_depth=True,
             zero_view=None, boundary=False, gen=gen)
    c.update(flags)
    return c


@functools.lru_cache(maxsize=None)
def blend_case(name, seed=None):
    seed = _seed(name, seed)
    if name == "train":
        c = _blend(seed, 16, 256, 1, ones=True)
    elif name.startswith("stride-"):
        c = _blend(seed, 3, int(name.split("-")[1]), 3)
    elif name == "no_exposure":                                 # three fields' weights add up to more than one: entries above 1
        c = _blend(seed, 3, 100, 3, exposure=False)
    elif name == "no_depth_grad":
        c = _blend(seed, 3, 100, 3, use_depth=False)
    elif name == "zero_weight_view":
        c = _blend(seed, 3, 100, 3, zero_view=1)
        c["bw"][1] = 0.0
    elif name.startswith("boundary"):
        # first half of the rays: colours from {0, 0.25, 1} exactly, y is exactly 0 or 1 on two thirds of the entries and the
        # gradient passes (ATen's clamp backward: y >= 0 and y <= 1); second half: -0.25 and 1.25, the gradient is exactly zero
        c = _blend(seed, 2, 96, 1, ones=True, exposure=False, boundary=True)
        g, R = c["gen"], c["R"]
        col = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (R, 3), generator=g)]
        col[R // 2:] = torch.tensor([-0.25, 1.25])[torch.randint(0, 2, (R - R // 2, 3), generator=g)]
        c["rgb_f"] = col[None]
        if name == "boundary-identity":
            c["exposure"] = torch.eye(3)[None].repeat(2, 1, 1)
    else:
        raise KeyError(name)
    c.pop("gen")
    c["name"] = name
    return c


def blend_forward(c, dtype, rgb_f, dep_f, expo, per_ray=False):
    """-> (rgbs [R,3], depth [R], y [R,3] before the clamp) (local_tensorfs.py:438-439,467-474,493-497)."""
    w = c["bw"].to(dtype).repeat_interleave(c["per_view"], dim=0)
    rgb, dep = torch.zeros_like(rgb_f[0]), torch.zeros_like(dep_f[0])
    for k in range(c["n_rf"]):
        rgb = rgb + rgb_f[k] * w[:, k][..., None]
        dep = dep + dep_f[k] * w[:, k]
    if expo is not None:
        E = expo if per_ray else expo.repeat_interleave(c["per_view"], dim=0)
        rgb = torch.bmm(E, rgb[..., None])[..., 0]
    return rgb.clamp(0, 1), dep, rgb


def _blend_leaves(c, dtype, per_ray):
    ex = c["exposure"]
    if ex is not None and per_ray:
        ex = ex.repeat_interleave(c["per_view"], 0)
    return [t.to(dtype).clone().requires_grad_(True) for t in (c["rgb_f"], c["dep_f"])] + (
        [] if ex is None else [ex.to(dtype).clone().requires_grad_(True)])


def _blend_grads(c, dtype, per_ray):
    L = _blend_leaves(c, dtype, per_ray)
    rgbs, dep, y = blend_forward(c, dtype, L[0], L[1], L[2] if len(L) == 3 else None, per_ray)
    g = _grads([(rgbs, c["g_rgbs"].to(dtype))] + ([(dep, c["g_depth"].to(dtype))] if c["use_depth"] else []), L)
    return rgbs, dep, y, g


def blend_terms(c, dtype):
    with one_thread():
        g = _blend_grads(c, dtype, True)[3]
    return {"g_exposure": g[2].detach()} if len(g) == 3 else {}


def blend_run(c, dtype, order="aten"):
    """-> {quantity: float64 array}; "y" is the colour before the clamp (not a quantity: the clamp margin reads it)."""
    with one_thread():
        rgbs, dep, y, g = _blend_grads(c, dtype, False)
        out = {"rgbs": _np(rgbs), "depth": _np(dep), "y": _np(y), "g_rgb_f": _np(g[0]), "g_depth_f": _np(g[1])}
        if len(g) == 3:
            out["g_exposure"] = _np(g[2] if order == "aten" else _view_sum(blend_terms(c, dtype)["g_exposure"], c["V"], order))
    return out


def blend_quantities(c):
    return [q for q in BLEND_Q if q != "g_exposure" or c["exposure"] is not None]


@functools.lru_cache(maxsize=None)
def blend_ref(name):
    return blend_run(blend_case(name), torch.float64)


def clamped(x):
    x = np.asarray(x)
    return (x <= 0) | (x >= 1)


def clamp_flips(a, b):
    """Entries clamped in one of two results and not in the other."""
    return int((clamped(a) != clamped(np.asarray(b).reshape(np.asarray(a).shape))).sum())


def blend_check(name, seed=None):
    """-> (violations, e32) of a blend case: the clamp margin, the clamped share, no clamp flip of the float32 chain, bounded
    cancellation in the exposure gradient, 4 e32 under the caps.  The rays of a view whose weights are all zero blend to
    exactly 0 in any precision and stay out of the margin (their gradients are exactly zero, which the GPU test demands)."""
    c = blend_case(name, seed)
    ref = blend_ref(name) if seed is None else blend_run(c, torch.float64)
    bad, y = [], ref["y"]
    if not c["boundary"]:
        keep = np.ones(c["R"], bool)
        if c["zero_view"] is not None:
            keep[c["zero_view"] * c["per_view"]:(c["zero_view"] + 1) * c["per_view"]] = False
        near = (np.minimum(np.abs(y), np.abs(y - 1)) < MARGIN)[keep]
        if near.any():
            bad.append(f"{int(near.sum())} blended colours within {MARGIN} of 0 or 1 (clamp margin)")
    share = float(clamped(y).mean())
    if c["exposure"] is not None and not c["boundary"] and not CLAMPED_SHARE[0] <= share <= CLAMPED_SHARE[1]:
        bad.append(f"clamped share {share:.3f} outside {CLAMPED_SHARE}")
    if c["exposure"] is not None:
        bad += _cancellation(ref, blend_terms(c, torch.float64), c["V"], ["g_exposure"], ())
    q = blend_quantities(c)
    r32 = blend_run(c, torch.float32)
    if clamp_flips(r32["rgbs"], ref["rgbs"]):
        bad.append(f"{clamp_flips(r32['rgbs'], ref['rgbs'])} clamp flips of the float32 chain")
    e32 = _e32(blend_run, c, ref, q, ("g_exposure",))
    return bad + _over_cap(e32), e32


# ------------------------------------------------------------------------------------------------------------------ pose
def _pose(seed, F, frames, perturb, quirk=False, cols=2):
    gen = torch.Generator().manual_seed(seed)
    r = torch.eye(3, cols)[None].repeat(F, 1, 1) + perturb * torch.randn(F, 3, cols, generator=gen)
    return dict(F=F, frames=list(frames), quirk=quirk, r=r, t=torch.randn(F, 3, generator=gen),
                gout=torch.randn(len(frames), 3, 4, generator=gen))


@functools.lru_cache(maxsize=None)
def pose_case(name, seed=None):
    """r [F,3,2] (prior33: [F,3,3]) and t [F,3] per-frame parameters, `frames` the list of frames that is assembled (a frame may
    appear more than once), gout [len(frames),3,4] the cotangent."""
    seed = _seed(name, seed)
    kind = name.split("-")[0]
    if kind == "sizes":
        v, p = name.split("-")[1:]
        V = int(v.rstrip("q"))
        c = _pose(seed, V, range(V), float(p), quirk=v.endswith("q"))
    elif kind == "scaled":                                      # the parameters are never normalised: |a1| = 1e-3, |a2| = 1e3 and
        c = _pose(seed, 4, range(4), 0.3)                       # the other way round
        s = (1e-3, 1e3) if name == "scaled-a" else (1e3, 1e-3)
        for k in (0, 1):
            c["r"][..., k] *= s[k] / c["r"][..., k].norm(dim=-1, keepdim=True)
    elif kind == "repeat":                                      # frame 3 at positions 3, 64 and 128: in all three launches
        c = _pose(seed, 127, list(range(64)) + [3] + list(range(64, 127)) + [3], 0.3)
        assert len(c["frames"]) == 129 and [i for i, f in enumerate(c["frames"]) if f == 3] == [3, 64, 128]
    elif kind == "quirk_repeat":
        c = _pose(seed, 2, [0, 0, 1], 0.3, quirk=True)
    elif kind == "prior33":                                     # camera priors: [3,3] parameters of which columns 0 and 1 are read
        c = _pose(seed, 4, range(4), 0.3, cols=3)
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def _cross(a, b, dim):
    a0, a1, a2 = a.unbind(dim)
    b0, b1, b2 = b.unbind(dim)
    return torch.stack([a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0], dim)


def sixd_to_mtx(r, quirk):
    """[V,3,2] -> [V,3,3] with columns (b1, b2, b3) (utils/utils.py:381-388) -> (matrix, |a1|, |u|).  quirk: the reference's
    torch.cross has no `dim` and runs over the first axis of size 3, the view axis of a stack of exactly three views."""
    a1, a2 = r[..., 0], r[..., 1]
    n1 = torch.sqrt((a1 * a1).sum(-1))
    b1 = a1 / n1[:, None]
    u = a2 - (b1 * a2).sum(-1)[:, None] * b1
    n2 = torch.sqrt((u * u).sum(-1))
    b2 = u / n2[:, None]
    assert not quirk or r.shape[0] == 3
    return torch.stack([b1, b2, _cross(b1, b2, 0 if quirk else -1)], -1), n1, n2


def pose_run(c, dtype):
    """-> {c2w [n,3,4]; g_a1, g_a2, g_trans [F,3]: the gradients per FRAME, the sum over the slots that name it; slots_r
    [n,3,2]: the gradients per slot}."""
    with one_thread():
        idx = torch.tensor(c["frames"])
        r = c["r"][idx][:, :, :2].to(dtype).clone().requires_grad_(True)
        t = c["t"][idx].to(dtype).clone().requires_grad_(True)
        m, n1, n2 = sixd_to_mtx(r, c["quirk"])
        c2w = torch.cat([m, t[..., None]], -1)
        gr, gt = torch.autograd.grad(c2w, [r, t], c["gout"].to(dtype))
        per_frame = lambda g: torch.zeros((c["F"],) + tuple(g.shape[1:]), dtype=dtype).index_add_(0, idx, g)
        fr = per_frame(gr)
    return {"c2w": _np(c2w), "g_a1": _np(fr[..., 0]), "g_a2": _np(fr[..., 1]), "g_trans": _np(per_frame(gt)), "slots_r": _np(gr),
            "norms": (_np(n1), _np(n2), _np(torch.sqrt((r[..., 1] ** 2).sum(-1))))}


@functools.lru_cache(maxsize=None)
def pose_ref(name):
    return pose_run(pose_case(name), torch.float64)


def pose_check(name, seed=None):
    """-> (violations, e32): both Gram-Schmidt norms above 1e-4 of the column norms (no near-parallel columns), 4 e32 under
    the caps."""
    c = pose_case(name, seed)
    ref = pose_ref(name) if seed is None else pose_run(c, torch.float64)
    n1, n2, a2 = ref["norms"]
    bad = [] if (n1 > 0).all() and (n2 > 1e-4 * a2).all() else ["near-parallel columns"]
    r32 = pose_run(c, torch.float32)
    e32 = {q: rel_err(r32[q], ref[q]) for q in POSE_Q}
    return bad + _over_cap(e32), e32


# ------------------------------------------------------------------------------------------------------------------ seeds, E32
CHECKS = {"rays": (RAYS_CASES, rays_check), "blend": (BLEND_CASES, blend_check), "pose": (POSE_CASES, pose_check)}


def first_seed(family, name, limit=2000):
    for seed in range(1, limit):
        bad, e32 = CHECKS[family][1](name, seed)
        if not bad:
            return seed, e32
    raise RuntimeError((family, name))


# E32["<family>:<case>"][quantity]: the float32 CPU chain's error against float64, max|x32 - x64| / max|x64|; for the reduced
# gradients the largest of the three summation orders.  tests/test_scene_host.py recomputes it.
E32 = {
    "rays:train/pinhole": {"rays": 1.02e-07, "directions": 2.96e-08, "g_cam2world": 5.26e-07, "g_world2rf": 1.20e-07,
        "g_focal": 9.20e-08, "g_center": 7.98e-08},
    "rays:train/360": {"rays": 8.74e-07, "directions": 8.72e-07, "g_cam2world": 5.28e-07, "g_world2rf": 1.20e-07},
    "rays:stride-1/pinhole": {"rays": 5.21e-08, "directions": 2.04e-08, "g_cam2world": 4.33e-08, "g_world2rf": 3.05e-08,
        "g_focal": 7.69e-08, "g_center": 8.36e-08},
    "rays:stride-1/360": {"rays": 8.33e-08, "directions": 9.04e-08, "g_cam2world": 1.39e-07, "g_world2rf": 3.05e-08},
    "rays:stride-2/pinhole": {"rays": 6.66e-08, "directions": 2.47e-08, "g_cam2world": 4.10e-08, "g_world2rf": 7.18e-08,
        "g_focal": 1.33e-07, "g_center": 1.59e-08},
    "rays:stride-2/360": {"rays": 1.86e-07, "directions": 1.73e-07, "g_cam2world": 5.46e-08, "g_world2rf": 4.36e-08},
    "rays:stride-63/pinhole": {"rays": 6.90e-08, "directions": 2.91e-08, "g_cam2world": 2.11e-07, "g_world2rf": 1.47e-07,
        "g_focal": 1.09e-07, "g_center": 3.12e-08},
    "rays:stride-63/360": {"rays": 5.30e-07, "directions": 5.30e-07, "g_cam2world": 2.21e-07, "g_world2rf": 1.47e-07},
    "rays:stride-64/pinhole": {"rays": 6.75e-08, "directions": 2.91e-08, "g_cam2world": 2.57e-07, "g_world2rf": 1.10e-07,
        "g_focal": 1.51e-07, "g_center": 1.60e-07},
    "rays:stride-64/360": {"rays": 4.99e-07, "directions": 5.30e-07, "g_cam2world": 1.99e-07, "g_world2rf": 8.54e-08},
    "rays:stride-65/pinhole": {"rays": 6.98e-08, "directions": 2.91e-08, "g_cam2world": 2.01e-07, "g_world2rf": 1.11e-07,
        "g_focal": 2.41e-07, "g_center": 7.24e-08},
    "rays:stride-65/360": {"rays": 3.71e-07, "directions": 5.30e-07, "g_cam2world": 1.28e-07, "g_world2rf": 1.11e-07},
    "rays:stride-255/pinhole": {"rays": 9.89e-08, "directions": 2.91e-08, "g_cam2world": 5.87e-07, "g_world2rf": 2.91e-07,
        "g_focal": 5.71e-08, "g_center": 1.97e-07},
    "rays:stride-255/360": {"rays": 5.93e-07, "directions": 6.15e-07, "g_cam2world": 5.87e-07, "g_world2rf": 2.91e-07},
    "rays:stride-256/pinhole": {"rays": 1.01e-07, "directions": 2.91e-08, "g_cam2world": 5.78e-07, "g_world2rf": 3.39e-07,
        "g_focal": 2.51e-07, "g_center": 1.19e-07},
    "rays:stride-256/360": {"rays": 5.95e-07, "directions": 6.15e-07, "g_cam2world": 4.21e-07, "g_world2rf": 3.39e-07},
    "rays:stride-257/pinhole": {"rays": 9.42e-08, "directions": 2.91e-08, "g_cam2world": 3.37e-07, "g_world2rf": 3.42e-07,
        "g_focal": 3.04e-07, "g_center": 1.44e-07},
    "rays:stride-257/360": {"rays": 6.18e-07, "directions": 6.15e-07, "g_cam2world": 3.47e-07, "g_world2rf": 3.42e-07},
    "rays:stride-1025/pinhole": {"rays": 9.13e-08, "directions": 2.91e-08, "g_cam2world": 1.36e-06, "g_world2rf": 5.39e-07,
        "g_focal": 1.04e-07, "g_center": 3.35e-07},
    "rays:stride-1025/360": {"rays": 6.42e-07, "directions": 6.15e-07, "g_cam2world": 1.37e-06, "g_world2rf": 5.39e-07},
    "rays:one_view/pinhole": {"rays": 9.25e-08, "directions": 2.91e-08, "g_cam2world": 1.31e-06, "g_world2rf": 2.04e-06,
        "g_focal": 1.11e-06, "g_center": 5.13e-07},
    "rays:one_view/360": {"rays": 6.32e-07, "directions": 6.15e-07, "g_cam2world": 1.31e-06, "g_world2rf": 2.04e-06},
    "rays:frame/pinhole": {"rays": 9.62e-08, "directions": 2.91e-08},
    "rays:frame/360": {"rays": 6.35e-07, "directions": 6.15e-07},
    "rays:big_ids/pinhole": {"rays": 8.02e-08, "directions": 2.86e-08, "g_cam2world": 1.85e-07, "g_world2rf": 1.05e-07,
        "g_focal": 1.35e-07, "g_center": 9.80e-08},
    "rays:big_ids/360": {"rays": 6.68e-07, "directions": 6.73e-07, "g_cam2world": 1.48e-07, "g_world2rf": 1.05e-07},
    "rays:no_dirs_grad/pinhole": {"rays": 8.87e-08, "directions": 2.91e-08, "g_cam2world": 2.34e-07, "g_world2rf": 1.02e-07,
        "g_focal": 1.02e-07, "g_center": 8.19e-08},
    "rays:dirs_only/pinhole": {"rays": 8.87e-08, "directions": 2.91e-08, "g_cam2world": 0.00e+00, "g_world2rf": 0.00e+00,
        "g_focal": 1.47e-07, "g_center": 8.63e-08},
    "rays:dirs_only/360": {"rays": 5.76e-07, "directions": 5.87e-07, "g_cam2world": 0.00e+00, "g_world2rf": 0.00e+00},
    "rays:pose44/pinhole": {"rays": 8.87e-08, "directions": 2.91e-08, "g_cam2world": 2.34e-07, "g_world2rf": 1.02e-07,
        "g_focal": 7.28e-08, "g_center": 1.19e-07},
    "rays:pose44/360": {"rays": 5.76e-07, "directions": 5.87e-07, "g_cam2world": 1.64e-07, "g_world2rf": 1.88e-07},
    "rays:strided_grad/pinhole": {"rays": 8.87e-08, "directions": 2.91e-08, "g_cam2world": 2.34e-07, "g_world2rf": 1.02e-07,
        "g_focal": 7.28e-08, "g_center": 1.19e-07},
    "rays:strided_grad/360": {"rays": 5.76e-07, "directions": 5.87e-07, "g_cam2world": 1.64e-07, "g_world2rf": 1.88e-07},
    "blend:train": {"rgbs": 1.17e-07, "depth": 0.00e+00, "g_rgb_f": 8.06e-08, "g_depth_f": 0.00e+00, "g_exposure":
        3.19e-07},
    "blend:stride-1": {"rgbs": 9.61e-09, "depth": 2.87e-08, "g_rgb_f": 5.07e-08, "g_depth_f": 2.60e-08, "g_exposure":
        2.41e-08},
    "blend:stride-2": {"rgbs": 8.86e-08, "depth": 2.14e-08, "g_rgb_f": 1.83e-08, "g_depth_f": 5.23e-08, "g_exposure":
        6.16e-08},
    "blend:stride-63": {"rgbs": 1.09e-07, "depth": 5.58e-08, "g_rgb_f": 7.90e-08, "g_depth_f": 5.21e-08, "g_exposure":
        1.55e-07},
    "blend:stride-64": {"rgbs": 1.93e-07, "depth": 6.39e-08, "g_rgb_f": 6.48e-08, "g_depth_f": 3.37e-08, "g_exposure":
        1.35e-07},
    "blend:stride-65": {"rgbs": 1.42e-07, "depth": 6.47e-08, "g_rgb_f": 4.40e-08, "g_depth_f": 3.36e-08, "g_exposure":
        1.44e-07},
    "blend:stride-255": {"rgbs": 1.89e-07, "depth": 5.83e-08, "g_rgb_f": 6.19e-08, "g_depth_f": 3.84e-08, "g_exposure":
        4.97e-07},
    "blend:stride-256": {"rgbs": 2.09e-07, "depth": 9.74e-08, "g_rgb_f": 1.05e-07, "g_depth_f": 3.89e-08, "g_exposure":
        3.31e-07},
    "blend:stride-257": {"rgbs": 2.09e-07, "depth": 8.75e-08, "g_rgb_f": 6.39e-08, "g_depth_f": 3.44e-08, "g_exposure":
        3.27e-07},
    "blend:stride-1025": {"rgbs": 2.00e-07, "depth": 8.51e-08, "g_rgb_f": 6.94e-08, "g_depth_f": 3.28e-08, "g_exposure":
        1.30e-06},
    "blend:no_exposure": {"rgbs": 8.38e-08, "depth": 7.95e-08, "g_rgb_f": 4.19e-08, "g_depth_f": 3.71e-08},
    "blend:no_depth_grad": {"rgbs": 1.16e-07, "depth": 7.95e-08, "g_rgb_f": 1.19e-07, "g_depth_f": 0.00e+00, "g_exposure":
        1.02e-07},
    "blend:zero_weight_view": {"rgbs": 1.16e-07, "depth": 7.95e-08, "g_rgb_f": 1.19e-07, "g_depth_f": 2.78e-08,
        "g_exposure": 1.02e-07},
    "blend:boundary-none": {"rgbs": 0.00e+00, "depth": 0.00e+00, "g_rgb_f": 0.00e+00, "g_depth_f": 0.00e+00},
    "blend:boundary-identity": {"rgbs": 0.00e+00, "depth": 0.00e+00, "g_rgb_f": 0.00e+00, "g_depth_f": 0.00e+00,
        "g_exposure": 2.44e-07},
    "pose:sizes-1-0.05": {"c2w": 9.56e-08, "g_a1": 2.88e-07, "g_a2": 1.33e-07, "g_trans": 0.00e+00},
    "pose:sizes-1-0.3": {"c2w": 2.85e-08, "g_a1": 3.05e-07, "g_a2": 3.71e-08, "g_trans": 0.00e+00},
    "pose:sizes-2-0.05": {"c2w": 1.46e-07, "g_a1": 1.92e-07, "g_a2": 2.43e-07, "g_trans": 0.00e+00},
    "pose:sizes-2-0.3": {"c2w": 4.34e-08, "g_a1": 1.78e-07, "g_a2": 2.29e-07, "g_trans": 0.00e+00},
    "pose:sizes-3-0.05": {"c2w": 3.56e-08, "g_a1": 9.31e-08, "g_a2": 1.33e-07, "g_trans": 0.00e+00},
    "pose:sizes-3-0.3": {"c2w": 3.16e-08, "g_a1": 4.87e-08, "g_a2": 1.41e-07, "g_trans": 0.00e+00},
    "pose:sizes-4-0.05": {"c2w": 2.05e-08, "g_a1": 1.10e-07, "g_a2": 1.07e-07, "g_trans": 0.00e+00},
    "pose:sizes-4-0.3": {"c2w": 2.39e-08, "g_a1": 2.22e-07, "g_a2": 8.88e-08, "g_trans": 0.00e+00},
    "pose:sizes-63-0.05": {"c2w": 4.15e-08, "g_a1": 2.23e-07, "g_a2": 1.90e-07, "g_trans": 0.00e+00},
    "pose:sizes-63-0.3": {"c2w": 6.12e-08, "g_a1": 1.44e-07, "g_a2": 1.20e-07, "g_trans": 0.00e+00},
    "pose:sizes-64-0.05": {"c2w": 4.29e-08, "g_a1": 1.48e-07, "g_a2": 2.12e-07, "g_trans": 0.00e+00},
    "pose:sizes-64-0.3": {"c2w": 6.33e-08, "g_a1": 1.90e-07, "g_a2": 1.95e-07, "g_trans": 0.00e+00},
    "pose:sizes-65-0.05": {"c2w": 4.65e-08, "g_a1": 1.88e-07, "g_a2": 1.75e-07, "g_trans": 0.00e+00},
    "pose:sizes-65-0.3": {"c2w": 6.87e-08, "g_a1": 2.84e-07, "g_a2": 1.89e-07, "g_trans": 0.00e+00},
    "pose:sizes-129-0.05": {"c2w": 5.74e-08, "g_a1": 1.08e-07, "g_a2": 1.35e-07, "g_trans": 0.00e+00},
    "pose:sizes-129-0.3": {"c2w": 7.16e-08, "g_a1": 5.73e-07, "g_a2": 1.47e-07, "g_trans": 0.00e+00},
    "pose:sizes-3q-0.05": {"c2w": 1.26e-08, "g_a1": 5.75e-08, "g_a2": 1.03e-07, "g_trans": 0.00e+00},
    "pose:sizes-3q-0.3": {"c2w": 4.77e-08, "g_a1": 1.89e-07, "g_a2": 9.92e-08, "g_trans": 0.00e+00},
    "pose:scaled-a": {"c2w": 3.38e-08, "g_a1": 1.72e-07, "g_a2": 6.16e-08, "g_trans": 0.00e+00},
    "pose:scaled-b": {"c2w": 1.68e-08, "g_a1": 4.42e-08, "g_a2": 7.13e-08, "g_trans": 0.00e+00},
    "pose:repeat": {"c2w": 5.24e-08, "g_a1": 1.97e-07, "g_a2": 1.24e-07, "g_trans": 1.43e-08},
    "pose:quirk_repeat": {"c2w": 5.78e-08, "g_a1": 9.09e-08, "g_a2": 8.50e-08, "g_trans": 3.09e-08},
    "pose:prior33": {"c2w": 4.18e-08, "g_a1": 2.46e-07, "g_a2": 1.11e-07, "g_trans": 0.00e+00},
}
