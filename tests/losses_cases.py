"""Shared pieces of the loss-kernel tests (csrc/lrf_losses.inl): the cases, their float64 references, and the measured error of
the float32 CPU evaluation of the same expressions, from which the GPU tolerances follow.

  geo_case(name)                      inputs of one geometric case (CPU tensors, deterministic from SEEDS)
  geo_run(case, dtype, form, frozen)  flow and depth loss through oracle/vm_render_torch.py in `dtype`, gradients from autograd
  geo_raw(case, dtype)                the unclipped per-ray arrays and the per-view thresholds
  photo_case / photo_run              the photometric loss (train.py:369-371)
  gather_case, rows_case / rows_run   inputs of lrf_batch_gather, lrf_rows_gather(_bwd) and the latter's float64 backward
  combine_case / combine_run          the loss assembly (train.py:425-437)
  rel_err, tolerance, E32             max|x - ref| / max|ref|; the tolerance rule; the recorded float32-CPU errors

Forms of a geometric case.  "mean": flow_loss and depth_loss each return their mean, differentiated separately.  "per_view": both
return their V per-view sums, which go through `combine` with the uniform weights of the training loop,
total = s (sum(flow sums) / ((W + H) / 2) / (V n) + 0.1 sum(depth sums) / (V n)), and the total is differentiated.

Nothing here touches a GPU or the HIP library.  Cited lines are relative to the reference's localTensoRF directory."""
import contextlib
import functools

import numpy as np
import torch

from oracle import vm_render_torch as ot

U = 2.0 ** -24                          # unit roundoff of float32
FLOOR = 8 * U                           # no tolerance below 8 roundings
CAP_VALUE, CAP_PHOTO, CAP_GRAD = 1e-5, 2e-6, 1e-4       # what tests/test_gpu_training.py demands already
W_IMG, H_IMG, FOCAL = 640, 480, 500.0
S_REG = float(np.float32(0.37))         # the schedule weight `combine` multiplies with, as the float32 the device scalar holds
W_FLOW, W_DEPTH = 1.0, 0.1
BEHIND = 1e6                            # px: a flow entry above this belongs to a ray reprojected behind the neighbour (zc = 1e-6)

POW2_SIZES = (2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096)
QUANTILES = (0.0, 0.5, 1.0)
GEO_CASES = (["dup_views", "one_frame", "two_frames", "shard"] + [f"pow2_edges-{n}" for n in POW2_SIZES]
             + ["single_ray", "masked", "depth_edges"] + [f"quantiles-{q}" for q in QUANTILES])
FORMS = ("mean", "per_view")
FLOW_Q = ("flow", "flow_arr", "flow_g_depth", "flow_g_dirs", "flow_g_c2w", "flow_g_focal", "flow_g_center")
DEPTH_Q = ("depth", "depth_arr", "depth_g_depth")
GRADS = {"flow_g_depth", "flow_g_dirs", "flow_g_c2w", "flow_g_focal", "flow_g_center", "depth_g_depth"}

# Seeds found by the search of geo_check's conditions on the CPU (the case holds its edges, clip margin, unique median, 4 e32
# under the caps, summation order): the first seed from 1 upwards that meets all of them.  A changed seed has to pass tests/test_losses_host.py.
SEEDS = {
    "dup_views": 1, "one_frame": 2, "two_frames": 1, "shard": 1, "single_ray": 1, "masked": 3, "depth_edges": 10, "quantiles": 37,
    "pow2_edges-2": 1, "pow2_edges-3": 2, "pow2_edges-63": 5, "pow2_edges-64": 1, "pow2_edges-65": 1, "pow2_edges-1023": 4,
    "pow2_edges-1024": 3, "pow2_edges-1025": 8, "pow2_edges-2049": 1, "pow2_edges-4095": 3, "pow2_edges-4096": 3,
}

PHOTO_SIZES = (1, 5, 341, 1023, 1024, 1025, 4096)
PHOTO_MODES = ("none", "w", "w_mean")
PHOTO_UP = 3.0
GATHER_SHAPES = ((3, 100, 77, 5), (16, 256, 640, 9))         # (V, n, HW, n_images)
ROWS_SHAPE = (70, 12, 30)                                     # (F, K, V)
COMBINE_CASES = ("eight-s", "eight-none", "single")
COMBINE_UP = 2.5


@contextlib.contextmanager
def one_thread():
    """The float32 CPU evaluations run on one thread: their summation order, and with it E32, is then a property of the torch
    build and not of the machine's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def rel_err(x, ref):
    """max|x - ref| / max|ref| (0 where both are all zero)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    d, m = float(np.abs(x - ref).max()), float(np.abs(ref).max())
    return 0.0 if d == 0.0 else d / m if m > 0 else float("inf")


def cap_of(quantity):
    return CAP_PHOTO if quantity.startswith("photo") else CAP_GRAD if (quantity in GRADS or "_g" in quantity) else CAP_VALUE


def tolerance(e32, quantity):
    """4 x the float32-CPU error (a different summation order: 1024 threads then 16 waves against ATen's tree), not below 8
    roundings, not above what the project demands already."""
    return min(max(4.0 * e32, FLOOR), cap_of(quantity))


def _not_stale(table, measured, key, floor=FLOOR):
    """The recorded and the measured error agree within 2 x.  Below floor / 4 an error does not enter the tolerance
    (max(4 e32, FLOOR)), and a single float32 result can be exact by chance: both are raised to that before comparing."""
    assert set(table) == set(measured), key
    lo = floor / 4
    for q in table:
        a, b = max(table[q], lo), max(measured[q], lo)
        assert a <= 2 * b and b <= 2 * a, (key, q, table[q], measured[q])


# ------------------------------------------------------------------------------------------------------- geometric cases
def _poses(F, gen, rot=0.05, trans=0.2):
    r6 = torch.eye(3)[:, :2][None].repeat(F, 1, 1) + rot * torch.randn(F, 3, 2, generator=gen)
    b1 = torch.nn.functional.normalize(r6[..., 0], dim=-1)
    b2 = torch.nn.functional.normalize(r6[..., 1] - (b1 * r6[..., 1]).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.cat([torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -1), trans * torch.randn(F, 3, 1, generator=gen)], -1)


def _sampled_views(gen, F, V):
    """V frame indices drawn with replacement and sorted, as scripts/train_synth.py's sampler draws a batch's views."""
    return torch.sort(torch.randint(0, F, (V,), generator=gen)).values


def _geo(seed, V, n, F, start, frames, q_flow=0.9, q_depth=0.8, flow=4.0):
    gen = torch.Generator().manual_seed(seed)
    frames = frames(gen) if callable(frames) else torch.as_tensor(frames, dtype=torch.int64)
    assert frames.shape == (V,) and int(frames.min()) >= 0 and int(frames.max()) < F
    col, row = torch.randint(0, W_IMG, (V, n), generator=gen), torch.randint(0, H_IMG, (V, n), generator=gen)
    focal, center = torch.tensor([FOCAL]), torch.tensor([W_IMG * 0.5, H_IMG * 0.5])
    dirs = torch.stack([(col + 0.5 - center[0]) / focal, -(row + 0.5 - center[1]) / focal, -torch.ones(V, n)], -1)
    return dict(V=V, n=n, F=F, start=start, frames=frames, view_ids=frames + start, c2w=_poses(F, gen), ij=torch.stack([col, row], -1),
                dirs=dirs, depth=0.5 + 5 * torch.rand(V, n, generator=gen), invdepths=0.1 + torch.rand(V, n, generator=gen),
                fwd_flow=flow * torch.randn(V, n, 2, generator=gen), bwd_flow=flow * torch.randn(V, n, 2, generator=gen),
                fwd_mask=(torch.rand(V, n, generator=gen) > 0.2).float(), bwd_mask=(torch.rand(V, n, generator=gen) > 0.2).float(),
                focal=focal, center=center, q_flow=q_flow, q_depth=q_depth, gen=gen)


def _rot_y(deg):
    a = np.deg2rad(deg)
    return torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def geo_case(name, seed=None):
    """The inputs of a geometric case as a dict of CPU tensors ([V,n,...] shaped, float32 / int64).  seed: another than SEEDS'
    (the seed search)."""
    kind = name.split("-")[0]
    seed = SEEDS[name if kind == "pow2_edges" else kind] if seed is None else seed
    if kind == "dup_views":
        c = _geo(seed, 16, 256, 5, 2, lambda g: _sampled_views(g, 5, 16))
    elif kind == "one_frame":
        # every cam2cam is the identity, the predicted flow is zero and the array is |target flow|: targets of 40 px, so that
        # the array's size stands against the float32 rounding of pixel coordinates up to 640 as it does in the other cases
        c = _geo(seed, 16, 64, 1, 0, [0] * 16, flow=40.0)
    elif kind == "two_frames":
        c = _geo(seed, 16, 64, 2, 0, lambda g: _sampled_views(g, 2, 16))
    elif kind == "shard":                                       # rank 3 of 8: views 6 and 7 of the sorted sixteen
        c = _geo(seed, 2, 256, 5, 2, lambda g: _sampled_views(g, 5, 16)[6:8])
    elif kind == "pow2_edges":                                  # frame 2: absolute id 3 = F - 1, not the last; frame 3: the last, id 4
        c = _geo(seed, 2, int(name.split("-")[1]), 4, 1, [2, 3])
    elif kind == "single_ray":
        c = _geo(seed, 2, 1, 4, 1, [2, 3])
    elif kind == "quantiles":
        q = float(name.split("-")[1])
        c = _geo(seed, 2, 100, 4, 0, [1, 3], q_flow=q, q_depth=q)
        c["fwd_mask"][:], c["bwd_mask"][:] = 1.0, 1.0          # no exact zeros: q = 0 keeps the smallest entry, not nothing
    elif kind == "masked":
        c = _geo(seed, 4, 128, 5, 0, [0, 1, 2, 4])
        g = c["gen"]
        for v, share in ((0, 1.0), (1, 0.95), (2, 0.85)):       # both masks zero on the same rays; view 3 keeps every ray
            off = torch.randperm(128, generator=g)[:int(round(share * 128))]
            for m in ("fwd_mask", "bwd_mask"):
                c[m][v] = 1.0
                c[m][v, off] = 0.0
        c["fwd_mask"][3] = 1.0
        c["bwd_mask"][3] = 1.0
    elif kind == "depth_edges":
        c = _geo(seed, 3, 200, 4, 0, [0, 1, 3])
        g = c["gen"]
        c["c2w"][2, :, :3] = _rot_y(60.0) @ c["c2w"][2, :, :3]  # frame 2, the forward neighbour of view 1, turned: rays at one
        for v in range(3):                                      # image edge reproject behind it
            p = torch.randperm(200, generator=g)
            c["depth"][v, p[:10]] = 1e-7                        # 5 % below the clamp
            c["depth"][v, p[10:13]] = float(np.float32(1e-6))   # exactly at it: the gradient passes (>=)
            c["depth"][v, p[13:19]] = -c["depth"][v, p[13:19]]  # negative
        c["invdepths"] = torch.round(c["invdepths"] * 0.5 * 255) / 255      # quantised: 128 levels for 200 rays, many equal values
    else:
        raise KeyError(name)
    c.pop("gen")
    c["name"] = name
    return c


def _depth(c, dtype):
    """The depth map in `dtype`.  An entry exactly at the clamp is at the clamp in either precision: float32(1e-6) in float32,
    where the literal 1e-6 of `clamp(1e-6)` rounds to it, and the double 1e-6 in float64 (2.5e-9 away), so that both pass the
    gradient there as the reference's float32 program does."""
    d = c["depth"].to(dtype).clone()
    if dtype == torch.float64:
        d = torch.where(c["depth"] == float(np.float32(1e-6)), torch.tensor(1e-6, dtype=dtype), d)
    return d


def _flow_kw(c, dtype):
    return dict(ij=c["ij"], view_ids=c["view_ids"], starting_frame_id=c["start"], fwd_flow=c["fwd_flow"].to(dtype),
                fwd_mask=c["fwd_mask"].to(dtype), bwd_flow=c["bwd_flow"].to(dtype), bwd_mask=c["bwd_mask"].to(dtype))


def per_view_coef(c):
    """The (a_k, b_k) of the flow and depth terms in `combine`, b_k as the float32 the ABI carries."""
    Vn = c["V"] * c["n"]
    return [(0.0, float(np.float32(W_FLOW / ((W_IMG + H_IMG) / 2) / Vn))), (0.0, float(np.float32(W_DEPTH / Vn)))]


def _np(t):
    return t.detach().numpy().astype(np.float64)


def geo_run(c, dtype, form="mean", frozen=False):
    """Flow and depth loss of case c through oracle/vm_render_torch.py on the CPU in `dtype` -> {quantity: float64 array}.
    The depth loss differentiates its own copy of the depth map, so that the two losses' depth gradients stay apart.  n = 1
    leaves the depth loss out (0 / 0).  frozen: focal and center carry no gradient."""
    with one_thread():
        leaf = lambda t, grad=True: t.to(dtype).clone().requires_grad_(grad)
        L = dict(depth_map=_depth(c, dtype).requires_grad_(True), directions=leaf(c["dirs"]), cam2world=leaf(c["c2w"]),
                 focal=leaf(c["focal"], not frozen), center=leaf(c["center"], not frozen))
        fl, farr = ot.flow_loss(**L, **_flow_kw(c, dtype), quantile=c["q_flow"])
        with_depth = c["n"] > 1
        if with_depth:
            d2 = _depth(c, dtype).requires_grad_(True)
            dl, darr = ot.depth_loss(d2, c["invdepths"].to(dtype), quantile=c["q_depth"])
        out = {"flow_arr": _np(farr)}
        if with_depth:
            out["depth_arr"] = _np(darr)
        wrt = [v for v in L.values() if v.requires_grad]
        if form == "mean":
            out["flow"] = _np(fl)
            gf = torch.autograd.grad(fl, wrt)
            if with_depth:
                out["depth"] = _np(dl)
                (gd,) = torch.autograd.grad(dl, [d2])
        else:
            (_, bf), (_, bd) = per_view_coef(c)
            fs = farr.sum(1)
            out["flow"] = _np(fs)
            total = fs.sum() * (bf * S_REG)
            if with_depth:
                ds = darr.sum(1)
                out["depth"] = _np(ds)
                total = total + ds.sum() * (bd * S_REG)
            out["total"] = _np(total)
            gf = torch.autograd.grad(total, wrt, retain_graph=with_depth)
            if with_depth:
                (gd,) = torch.autograd.grad(total, [d2])
        names = ["flow_g_depth", "flow_g_dirs", "flow_g_c2w"] + ([] if frozen else ["flow_g_focal", "flow_g_center"])
        for k, g in zip(names, gf):
            out[k] = _np(g)
        if with_depth:
            out["depth_g_depth"] = _np(gd)
    return out


def quantities(c, form):
    q = list(FLOW_Q) + (list(DEPTH_Q) if c["n"] > 1 else [])
    return q + (["total"] if form == "per_view" else [])


def geo_raw(c, dtype):
    """The arrays before clipping (the losses called with quantile 1: nothing lies above the maximum) and the per-view
    thresholds torch.quantile gives for them, in `dtype` -> {"flow": (raw [V,n], thr [V]), "depth": ...} as float64."""
    with one_thread(), torch.no_grad():
        out = {}
        _, raw = ot.flow_loss(_depth(c, dtype), c["dirs"].to(dtype), cam2world=c["c2w"].to(dtype), focal=c["focal"].to(dtype),
                              center=c["center"].to(dtype), **_flow_kw(c, dtype), quantile=1.0)
        out["flow"] = (_np(raw), _np(torch.quantile(raw, c["q_flow"], dim=1)))
        if c["n"] > 1:
            _, raw = ot.depth_loss(_depth(c, dtype), c["invdepths"].to(dtype), quantile=1.0)
            out["depth"] = (_np(raw), _np(torch.quantile(raw, c["q_depth"], dim=1)))
    return out


def one_frame_scale(c, ref):
    """With one frame every cam2cam is the identity and the flow loss does not depend on the depth: its depth gradient is a sum
    of three terms g_p[k] dir[k] that cancel, a relative error of which means nothing.  The size of those terms, per ray and in
    float64, is what that one quantity is normalised by: sum_k |g_p[k] dir[k]|, g_p = g_dirs / depth."""
    d = c["depth"].numpy().astype(np.float64)[..., None]
    return np.abs(ref["flow_g_dirs"] / d * c["dirs"].numpy().astype(np.float64)).sum(-1)


def geo_err(c, quantity, got, ref):
    """The error of `got` against the float64 result `ref[quantity]` in the form E32 records and the GPU test bounds."""
    got = np.asarray(got, np.float64).reshape(ref[quantity].shape)
    if c["name"] == "one_frame" and quantity == "flow_g_depth":
        scale = one_frame_scale(c, ref)
        diff = np.abs(got - ref[quantity])
        if (diff[scale == 0] != 0).any():
            return float("inf")
        return float((diff[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    return rel_err(got, ref[quantity])


@functools.lru_cache(maxsize=None)
def geo_ref(name, form):
    return geo_run(geo_case(name), torch.float64, form)


def clip_flips(a, b):
    return int(((np.asarray(a) == 0) != (np.asarray(b) == 0)).sum())


def _holds(c, raw64):
    """What the case is there for, checked on its inputs -> violations."""
    bad, kind, fr, F = [], c["name"].split("-")[0], c["frames"].tolist(), c["F"]
    if kind == "dup_views":                                     # F = 5, start = 2: frame 2 has the absolute id F - 1 and is not the last
        if not ({0, F - 1, F - 1 - c["start"]} <= set(fr) and max(fr.count(f) for f in fr) >= 3 and 0 < F - 1 - c["start"] < F - 1):
            bad.append(f"frames {fr}: first, last, a non-last one with absolute id F - 1 and one named three times wanted")
    if kind == "two_frames" and set(fr) != {0, 1}:
        bad.append(f"frames {fr}: both wanted")
    if kind == "masked":
        raw, thr = raw64["flow"]
        zeros = (raw == 0).sum(1).tolist()
        if not (zeros[0] == c["n"] and thr[1] == 0.0 and zeros[1] < c["n"] and thr[2] > 0 and zeros[2] > 0.8 * c["n"] and zeros[3] == 0):
            bad.append(f"zeros per view {zeros}, thresholds {thr.tolist()}")
    if kind == "depth_edges":
        raw, thr = raw64["flow"]
        if not ((raw[1] > BEHIND).any() and (thr < BEHIND).all()):
            bad.append("a ray behind the turned neighbour, and thresholds among ordinary pixel distances, wanted")
        if len(np.unique(c["invdepths"].numpy())) > 0.7 * c["n"]:
            bad.append("many equal inverse depths wanted")
    return bad


N_ORDERS = 4
PER_RAY = ("depth", "dirs", "ij", "invdepths", "fwd_flow", "bwd_flow", "fwd_mask", "bwd_mask", "flow_arr", "depth_arr", "flow_g_depth",
           "flow_g_dirs", "depth_g_depth")


def reordered(d, perm, c=None):
    """A case, or the results of one (c: whose), with the rays of every view taken in the order perm."""
    V, n = (c or d)["V"], (c or d)["n"]
    return {k: (v.reshape((V, n) + tuple(v.shape[2:] if v.ndim > 2 else ()))[:, perm if torch.is_tensor(v) else perm.numpy()]
                if k in PER_RAY and getattr(v, "ndim", 0) >= 2 else v) for k, v in d.items()}


def geo_check(name, seed=None):
    """The conditions a seed has to meet -> (violations, {form: e32}).  An empty list: the GPU test may demand zero clip flips
    and the median's index of this case, and its tolerances stay under the caps.

    Summation order.  E32 records ONE float32 evaluation.  Where a quantity is a sum whose terms cancel (the gradients of focal
    and center are sums of signed per-ray terms: thousands of +-g for the centre), the error of a float32 sum depends on the
    order of its terms by an order of magnitude, and one evaluation can come out far below what another order gives -- the
    kernels sum in yet another one.  So the chain is evaluated N_ORDERS more times with the rays of each view permuted (the
    losses do not depend on that order), and a seed is refused if any of them lies over HALF the tolerance its recorded e32
    gives: the recorded figure then stands for the orders, not for a lucky one.

    Clip margin, per loss and view: with d32 = max |arr32 - arr64| over the view, no entry of the float64 array lies within
    16 d32 of the view's float64 threshold.  Not counted: exact zeros (masked rays: zero in any precision, never above a
    threshold), and an entry the threshold EQUALS -- where q (n - 1) is an integer (q = 0, q = 1, 0.8 x 255, 0.8 x 4095)
    torch.quantile returns that element itself, `val > thr` is false for it in any precision, and the float32 rank is required
    to be the same integer.  In a view whose threshold is an ordinary pixel distance, flow entries above BEHIND px belong to
    rays reprojected behind the neighbour (zc clamped at 1e-6: 1e8 px and more); their float32 error of a few px is a relative
    1e-7 like everyone's but would, taken as the view's d32, put every ordinary entry inside the margin.  They stay out of d32
    and have to exceed the threshold a thousandfold in both precisions instead."""
    c = geo_case(name, seed)
    raw64, raw32 = geo_raw(c, torch.float64), geo_raw(c, torch.float32)
    bad = _holds(c, raw64)
    for loss, q in (("flow", c["q_flow"]), ("depth", c["q_depth"])):
        if loss not in raw64:
            continue
        rank64, rank32 = q * (c["n"] - 1), float(np.float32(q) * np.float32(c["n"] - 1))
        if (rank64 == int(rank64)) != (rank32 == int(rank32)) or int(rank64) != int(rank32):
            bad.append(f"{loss}: float32 rank {rank32!r} against {rank64!r}")
        for v in range(c["V"]):
            x64, x32, thr, thr32 = raw64[loss][0][v], raw32[loss][0][v], raw64[loss][1][v], raw32[loss][1][v]
            behind = (x64 > BEHIND) if (loss == "flow" and thr < BEHIND) else np.zeros_like(x64, bool)
            if behind.any() and not ((x64[behind] > 1e3 * thr).all() and (x32[behind] > 1e3 * thr32).all()):
                bad.append(f"{loss} view {v}: a ray behind the neighbour within 1000 x the threshold")
            if behind.all():
                continue
            d32 = float(np.abs(x32 - x64)[~behind].max())
            near = (np.abs(x64 - thr) <= 16 * d32) & ~behind & (x64 != 0) & (x64 != thr)
            if near.any():
                bad.append(f"{loss} view {v}: {int(near.sum())} entries within 16 d32 = {16 * d32:.3e} of the threshold {thr:.6e}")
    if c["n"] > 1:                                              # the median of 1 / clamp(depth): unique, the same element in float32
        d = c["depth"].numpy()
        x32, x64 = np.float32(1) / np.maximum(d, np.float32(1e-6)), 1.0 / np.maximum(d.astype(np.float64), float(np.float32(1e-6)))
        m = (c["n"] - 1) // 2
        for v in range(c["V"]):
            o32, o64 = np.argsort(x32[v], kind="stable"), np.argsort(x64[v], kind="stable")
            s = x32[v][o32]
            if (m > 0 and s[m - 1] == s[m]) or (m + 1 < c["n"] and s[m + 1] == s[m]) or o32[m] != o64[m]:
                bad.append(f"view {v}: the median of 1 / depth is tied or moves between float32 and float64")
    e32 = {}
    for form in FORMS:
        ref = geo_ref(name, form) if seed is None else geo_run(c, torch.float64, form)
        r32 = geo_run(c, torch.float32, form)
        for arr in ("flow_arr", "depth_arr"):
            if arr in ref and clip_flips(r32[arr], ref[arr]):
                bad.append(f"{form} {arr}: {clip_flips(r32[arr], ref[arr])} clip flips of the float32 chain")
        e32[form] = {k: geo_err(c, k, r32[k], ref) for k in quantities(c, form)}
        for k, e in e32[form].items():
            if not 4 * e <= cap_of(k):
                bad.append(f"{form} {k}: 4 e32 = {4 * e:.3e} over the cap {cap_of(k):.0e}")
        for order in range(N_ORDERS):                           # the same chain with the rays of every view in another order
            perm = torch.randperm(c["n"], generator=torch.Generator().manual_seed(1000 + order))
            rp = reordered(geo_run(reordered(c, perm), torch.float32, form), torch.argsort(perm), c)
            for k in quantities(c, form):
                e = geo_err(c, k, rp[k], ref)
                if not e <= tolerance(e32[form][k], k) / 2:
                    bad.append(f"{form} {k}: {e:.3e} with the rays in another order, over half the tolerance of e32 = {e32[form][k]:.3e}")
    return bad, e32


# ------------------------------------------------------------------------------------------------------- photometric loss
@functools.lru_cache(maxsize=None)
def photo_case(R):
    """rgb, target [R,3], weights [R,1], supplied mean; min(7, R // 2) rows have rgb == target exactly (seven of them wherever
    that leaves rows that differ)."""
    g = torch.Generator().manual_seed(500 + R)
    rgb, tgt = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    k = min(7, R // 2)
    tgt[:k] = rgb[:k]
    return dict(R=R, rgb=rgb, tgt=tgt, w=0.1 + 3 * torch.rand(R, 1, generator=g), wm=torch.tensor(1.7), equal=k)


def photo_args(p, mode):
    """(weights, weights_mean) of a mode: none; [R]; [R,1] with a supplied mean."""
    return {"none": (None, None), "w": (p["w"].reshape(-1), None), "w_mean": (p["w"], p["wm"])}[mode]


def photo_run(p, mode, dtype):
    with one_thread():
        rgb = p["rgb"].to(dtype).clone().requires_grad_(True)
        w, wm = photo_args(p, mode)
        w = torch.ones(p["R"], 1, dtype=dtype) if w is None else w.to(dtype).reshape(-1, 1)
        val = (0.25 * torch.abs(rgb - p["tgt"].to(dtype)) * w / (w.mean() if wm is None else wm.to(dtype))).mean()
        (g,) = torch.autograd.grad(val * PHOTO_UP, rgb)
    return {"photo": _np(val), "photo_g_rgb": _np(g)}


# ------------------------------------------------------------------------------------------------------- gathers
@functools.lru_cache(maxsize=None)
def gather_case(shape):
    V, n, HW, n_images = shape
    g = torch.Generator().manual_seed(700 + V)
    views = torch.randint(-n_images, n_images, (V,), generator=g)
    views[0], views[1], views[2] = 0, -1, n_images - 1          # first image; the last one named both ways
    pix = torch.randint(0, HW, (V, n), generator=g)
    pix[0, 0], pix[-1, -1], pix[1, 0], pix[0, -1] = 0, HW - 1, HW - 1, 0
    return dict(V=V, n=n, HW=HW, n_images=n_images, views=views, pix=pix, images=torch.rand(n_images, HW, 3, generator=g),
                fwd=torch.randn(n_images, HW, 2, generator=g), bwd=torch.randn(n_images, HW, 2, generator=g),
                inv=torch.rand(n_images, HW, generator=g))


@functools.lru_cache(maxsize=None)
def rows_case():
    F, K, V = ROWS_SHAPE
    g = torch.Generator().manual_seed(800)
    idx = torch.randint(-F, F, (V,), generator=g)
    idx[idx % F == 41] = 40                                     # frame 41: nobody names it
    idx[0], idx[1], idx[2], idx[3], idx[4] = 5, 5, 5 - F, F - 1, -1     # repeated, and the same frame named both ways
    return dict(F=F, K=K, V=V, idx=idx, src=torch.randn(F, K, generator=g), up=torch.randn(V, K, generator=g), unnamed=41)


def rows_run(r, dtype):
    with one_thread():
        g = torch.zeros(r["F"], r["K"], dtype=dtype).index_add_(0, r["idx"] % r["F"], r["up"].to(dtype))
    return {"rows_g_src": _np(g)}


# ------------------------------------------------------------------------------------------------------- combine
@functools.lru_cache(maxsize=None)
def combine_case(name):
    """(xs, coef, s): eight terms, scalars and length-16 vectors mixed, with and without s; a single scalar term."""
    g = torch.Generator().manual_seed(900)
    if name == "single":
        return [torch.randn((), generator=g)], [(float(np.float32(0.7)), float(np.float32(0.3)))], torch.tensor(S_REG)
    xs = [torch.randn(16 if k % 2 else (), generator=g) for k in range(8)]
    coef = [(float(np.float32(a)), float(np.float32(b))) for a, b in
            [(1.0, 0.0), (0.0, 1.0 / 560 / 4096), (1e-2, 0.0), (0.0, 0.1 / 4096), (0.5, 0.25), (0.0, 0.0), (-0.3, 0.0), (2.0, -1.0)]]
    return xs, coef, (torch.tensor(S_REG) if name == "eight-s" else None)


def combine_run(name, dtype):
    xs, coef, s = combine_case(name)
    with one_thread():
        ys = [x.to(dtype).clone().requires_grad_(True) for x in xs]
        sv = 0.0 if s is None else s.to(dtype)
        total = sum(y.sum() * (a + b * sv) for y, (a, b) in zip(ys, coef))
        gs = torch.autograd.grad(total * COMBINE_UP, ys)
    return {"combine": _np(total), "combine_g": np.concatenate([_np(g).reshape(-1) for g in gs])}


def other_e32():
    """{key: {quantity: float32-CPU error}} of the photometric, rows_gather and combine cases."""
    out = {}
    for R in PHOTO_SIZES:
        for mode in PHOTO_MODES:
            ref, r32 = photo_run(photo_case(R), mode, torch.float64), photo_run(photo_case(R), mode, torch.float32)
            out[f"photo-{R}-{mode}"] = {q: rel_err(r32[q], ref[q]) for q in ref}
    ref, r32 = rows_run(rows_case(), torch.float64), rows_run(rows_case(), torch.float32)
    out["rows"] = {q: rel_err(r32[q], ref[q]) for q in ref}
    for name in COMBINE_CASES:
        ref, r32 = combine_run(name, torch.float64), combine_run(name, torch.float32)
        out[f"combine-{name}"] = {q: rel_err(r32[q], ref[q]) for q in ref}
    return out


# E32[key][quantity]: the float32 CPU chain's error against float64, max|x32 - x64| / max|x64| (geo_err's form for one_frame's
# flow depth gradient); key = "<case>/<form>" for the geometric cases.  tests/test_losses_host.py recomputes it.
E32 = {
    "dup_views/mean": {"flow": 7.64e-08, "flow_arr": 2.84e-07, "flow_g_depth": 2.20e-07, "flow_g_dirs": 1.55e-07,
        "flow_g_c2w": 1.12e-07, "flow_g_focal": 4.20e-09, "flow_g_center": 0.00e+00, "depth": 3.79e-09, "depth_arr":
        3.54e-07, "depth_g_depth": 5.41e-07},
    "dup_views/per_view": {"flow": 7.77e-08, "flow_arr": 2.84e-07, "flow_g_depth": 3.45e-07, "flow_g_dirs": 2.09e-07,
        "flow_g_c2w": 1.59e-07, "flow_g_focal": 8.78e-08, "flow_g_center": 5.57e-08, "depth": 1.58e-07, "depth_arr":
        3.54e-07, "depth_g_depth": 5.06e-07, "total": 1.17e-08},
    "one_frame/mean": {"flow": 5.74e-08, "flow_arr": 6.50e-07, "flow_g_depth": 1.36e-07, "flow_g_dirs": 1.84e-07,
        "flow_g_c2w": 2.31e-07, "flow_g_focal": 7.69e-08, "flow_g_center": 0.00e+00, "depth": 9.80e-09, "depth_arr":
        2.65e-07, "depth_g_depth": 2.23e-07},
    "one_frame/per_view": {"flow": 1.42e-07, "flow_arr": 6.50e-07, "flow_g_depth": 1.17e-07, "flow_g_dirs": 1.99e-07,
        "flow_g_c2w": 1.73e-07, "flow_g_focal": 3.44e-08, "flow_g_center": 5.47e-07, "depth": 1.64e-07, "depth_arr":
        2.65e-07, "depth_g_depth": 2.18e-07, "total": 4.60e-08},
    "two_frames/mean": {"flow": 7.15e-08, "flow_arr": 5.55e-07, "flow_g_depth": 3.55e-07, "flow_g_dirs": 1.87e-07,
        "flow_g_c2w": 1.98e-07, "flow_g_focal": 4.22e-08, "flow_g_center": 0.00e+00, "depth": 2.64e-08, "depth_arr":
        2.81e-07, "depth_g_depth": 2.69e-07},
    "two_frames/per_view": {"flow": 1.57e-07, "flow_arr": 5.55e-07, "flow_g_depth": 2.48e-07, "flow_g_dirs": 1.73e-07,
        "flow_g_c2w": 1.97e-07, "flow_g_focal": 1.76e-08, "flow_g_center": 1.44e-07, "depth": 1.30e-07, "depth_arr":
        2.81e-07, "depth_g_depth": 3.06e-07, "total": 9.54e-09},
    "shard/mean": {"flow": 1.40e-08, "flow_arr": 4.11e-07, "flow_g_depth": 6.94e-07, "flow_g_dirs": 1.87e-07, "flow_g_c2w":
        2.07e-07, "flow_g_focal": 1.04e-07, "flow_g_center": 0.00e+00, "depth": 9.45e-08, "depth_arr": 7.27e-07,
        "depth_g_depth": 1.12e-06},
    "shard/per_view": {"flow": 4.26e-08, "flow_arr": 4.11e-07, "flow_g_depth": 2.88e-07, "flow_g_dirs": 2.13e-07,
        "flow_g_c2w": 7.98e-08, "flow_g_focal": 2.08e-07, "flow_g_center": 3.14e-08, "depth": 8.57e-08, "depth_arr":
        7.27e-07, "depth_g_depth": 8.79e-07, "total": 8.06e-09},
    "pow2_edges-2/mean": {"flow": 1.69e-07, "flow_arr": 1.81e-07, "flow_g_depth": 2.69e-07, "flow_g_dirs": 1.27e-07,
        "flow_g_c2w": 1.32e-07, "flow_g_focal": 2.58e-07, "flow_g_center": 0.00e+00, "depth": 0.00e+00, "depth_arr":
        0.00e+00, "depth_g_depth": 0.00e+00},
    "pow2_edges-2/per_view": {"flow": 1.81e-07, "flow_arr": 1.81e-07, "flow_g_depth": 4.07e-07, "flow_g_dirs": 1.30e-07,
        "flow_g_c2w": 1.15e-07, "flow_g_focal": 3.01e-07, "flow_g_center": 1.82e-08, "depth": 0.00e+00, "depth_arr":
        0.00e+00, "depth_g_depth": 0.00e+00, "total": 2.33e-07},
    "pow2_edges-3/mean": {"flow": 2.05e-08, "flow_arr": 1.38e-07, "flow_g_depth": 2.49e-07, "flow_g_dirs": 5.92e-08,
        "flow_g_c2w": 7.01e-08, "flow_g_focal": 8.21e-08, "flow_g_center": 2.98e-08, "depth": 4.60e-09, "depth_arr":
        4.54e-08, "depth_g_depth": 1.35e-07},
    "pow2_edges-3/per_view": {"flow": 1.07e-07, "flow_arr": 1.38e-07, "flow_g_depth": 7.79e-08, "flow_g_dirs": 1.19e-07,
        "flow_g_c2w": 1.03e-07, "flow_g_focal": 7.41e-08, "flow_g_center": 4.74e-08, "depth": 6.22e-08, "depth_arr":
        4.54e-08, "depth_g_depth": 1.43e-07, "total": 2.96e-08},
    "pow2_edges-63/mean": {"flow": 3.93e-08, "flow_arr": 4.96e-07, "flow_g_depth": 5.63e-07, "flow_g_dirs": 1.37e-07,
        "flow_g_c2w": 1.71e-07, "flow_g_focal": 1.30e-07, "flow_g_center": 4.47e-08, "depth": 7.17e-08, "depth_arr":
        2.06e-07, "depth_g_depth": 2.33e-07},
    "pow2_edges-63/per_view": {"flow": 9.38e-08, "flow_arr": 4.96e-07, "flow_g_depth": 4.04e-07, "flow_g_dirs": 1.27e-07,
        "flow_g_c2w": 1.01e-07, "flow_g_focal": 2.34e-07, "flow_g_center": 2.87e-08, "depth": 5.32e-08, "depth_arr":
        2.06e-07, "depth_g_depth": 2.28e-07, "total": 7.62e-08},
    "pow2_edges-64/mean": {"flow": 3.00e-08, "flow_arr": 6.51e-07, "flow_g_depth": 1.76e-07, "flow_g_dirs": 1.41e-07,
        "flow_g_c2w": 6.66e-08, "flow_g_focal": 4.06e-08, "flow_g_center": 0.00e+00, "depth": 6.63e-09, "depth_arr":
        4.12e-07, "depth_g_depth": 3.20e-07},
    "pow2_edges-64/per_view": {"flow": 4.33e-08, "flow_arr": 6.51e-07, "flow_g_depth": 2.78e-07, "flow_g_dirs": 1.88e-07,
        "flow_g_c2w": 1.81e-07, "flow_g_focal": 1.72e-08, "flow_g_center": 7.40e-09, "depth": 7.88e-08, "depth_arr":
        4.12e-07, "depth_g_depth": 3.42e-07, "total": 5.63e-08},
    "pow2_edges-65/mean": {"flow": 2.55e-08, "flow_arr": 7.42e-07, "flow_g_depth": 1.80e-07, "flow_g_dirs": 1.55e-07,
        "flow_g_c2w": 1.04e-07, "flow_g_focal": 3.52e-08, "flow_g_center": 5.43e-08, "depth": 4.95e-08, "depth_arr":
        3.50e-07, "depth_g_depth": 3.11e-07},
    "pow2_edges-65/per_view": {"flow": 4.25e-08, "flow_arr": 7.42e-07, "flow_g_depth": 4.22e-07, "flow_g_dirs": 1.38e-07,
        "flow_g_c2w": 1.73e-07, "flow_g_focal": 1.38e-08, "flow_g_center": 8.43e-08, "depth": 1.62e-07, "depth_arr":
        3.50e-07, "depth_g_depth": 2.47e-07, "total": 3.21e-08},
    "pow2_edges-1023/mean": {"flow": 4.54e-08, "flow_arr": 1.00e-06, "flow_g_depth": 1.05e-06, "flow_g_dirs": 1.44e-07,
        "flow_g_c2w": 1.56e-07, "flow_g_focal": 1.50e-08, "flow_g_center": 6.45e-08, "depth": 1.03e-07, "depth_arr":
        5.37e-07, "depth_g_depth": 1.28e-06},
    "pow2_edges-1023/per_view": {"flow": 8.69e-08, "flow_arr": 1.00e-06, "flow_g_depth": 8.65e-07, "flow_g_dirs": 1.67e-07,
        "flow_g_c2w": 2.26e-07, "flow_g_focal": 6.54e-09, "flow_g_center": 8.41e-08, "depth": 9.75e-08, "depth_arr":
        5.37e-07, "depth_g_depth": 1.20e-06, "total": 2.09e-08},
    "pow2_edges-1024/mean": {"flow": 3.42e-09, "flow_arr": 2.93e-07, "flow_g_depth": 4.72e-07, "flow_g_dirs": 1.69e-07,
        "flow_g_c2w": 3.00e-07, "flow_g_focal": 4.29e-08, "flow_g_center": 0.00e+00, "depth": 3.61e-08, "depth_arr":
        4.38e-07, "depth_g_depth": 7.10e-07},
    "pow2_edges-1024/per_view": {"flow": 5.94e-08, "flow_arr": 2.93e-07, "flow_g_depth": 4.55e-07, "flow_g_dirs": 1.89e-07,
        "flow_g_c2w": 1.48e-07, "flow_g_focal": 1.43e-08, "flow_g_center": 2.81e-07, "depth": 3.84e-08, "depth_arr":
        4.38e-07, "depth_g_depth": 5.98e-07, "total": 7.13e-08},
    "pow2_edges-1025/mean": {"flow": 4.23e-08, "flow_arr": 6.57e-07, "flow_g_depth": 2.55e-07, "flow_g_dirs": 2.05e-07,
        "flow_g_c2w": 2.05e-07, "flow_g_focal": 8.71e-08, "flow_g_center": 4.97e-08, "depth": 3.93e-08, "depth_arr":
        2.85e-07, "depth_g_depth": 7.69e-07},
    "pow2_edges-1025/per_view": {"flow": 4.55e-08, "flow_arr": 6.57e-07, "flow_g_depth": 3.36e-07, "flow_g_dirs": 2.00e-07,
        "flow_g_c2w": 1.05e-07, "flow_g_focal": 8.94e-08, "flow_g_center": 4.13e-08, "depth": 7.32e-08, "depth_arr":
        2.85e-07, "depth_g_depth": 8.37e-07, "total": 8.20e-08},
    "pow2_edges-2049/mean": {"flow": 1.24e-07, "flow_arr": 9.61e-07, "flow_g_depth": 2.66e-07, "flow_g_dirs": 2.20e-07,
        "flow_g_c2w": 3.19e-07, "flow_g_focal": 3.33e-09, "flow_g_center": 1.52e-07, "depth": 7.75e-08, "depth_arr":
        4.80e-07, "depth_g_depth": 8.66e-07},
    "pow2_edges-2049/per_view": {"flow": 9.16e-08, "flow_arr": 9.61e-07, "flow_g_depth": 2.86e-07, "flow_g_dirs": 2.22e-07,
        "flow_g_c2w": 1.32e-07, "flow_g_focal": 5.10e-09, "flow_g_center": 5.76e-08, "depth": 7.20e-08, "depth_arr":
        4.80e-07, "depth_g_depth": 9.13e-07, "total": 2.22e-08},
    "pow2_edges-4095/mean": {"flow": 4.05e-08, "flow_arr": 4.79e-07, "flow_g_depth": 5.14e-07, "flow_g_dirs": 2.11e-07,
        "flow_g_c2w": 8.42e-08, "flow_g_focal": 5.74e-08, "flow_g_center": 1.40e-07, "depth": 2.18e-08, "depth_arr":
        6.13e-07, "depth_g_depth": 8.75e-07},
    "pow2_edges-4095/per_view": {"flow": 3.79e-08, "flow_arr": 4.79e-07, "flow_g_depth": 4.12e-07, "flow_g_dirs": 2.08e-07,
        "flow_g_c2w": 1.62e-07, "flow_g_focal": 3.60e-08, "flow_g_center": 1.58e-08, "depth": 1.06e-07, "depth_arr":
        6.13e-07, "depth_g_depth": 9.96e-07, "total": 4.20e-08},
    "pow2_edges-4096/mean": {"flow": 3.75e-09, "flow_arr": 5.76e-07, "flow_g_depth": 6.53e-07, "flow_g_dirs": 3.38e-07,
        "flow_g_c2w": 8.68e-08, "flow_g_focal": 2.39e-08, "flow_g_center": 0.00e+00, "depth": 3.64e-08, "depth_arr":
        3.99e-07, "depth_g_depth": 7.09e-07},
    "pow2_edges-4096/per_view": {"flow": 7.48e-08, "flow_arr": 5.76e-07, "flow_g_depth": 5.82e-07, "flow_g_dirs": 3.27e-07,
        "flow_g_c2w": 1.82e-07, "flow_g_focal": 5.62e-08, "flow_g_center": 6.80e-09, "depth": 6.17e-08, "depth_arr":
        3.99e-07, "depth_g_depth": 6.96e-07, "total": 3.43e-08},
    "single_ray/mean": {"flow": 5.09e-09, "flow_arr": 9.36e-08, "flow_g_depth": 4.15e-07, "flow_g_dirs": 9.48e-08,
        "flow_g_c2w": 1.18e-07, "flow_g_focal": 6.44e-08, "flow_g_center": 0.00e+00},
    "single_ray/per_view": {"flow": 9.36e-08, "flow_arr": 9.36e-08, "flow_g_depth": 3.07e-07, "flow_g_dirs": 6.87e-08,
        "flow_g_c2w": 5.14e-08, "flow_g_focal": 4.41e-08, "flow_g_center": 1.82e-08, "total": 2.93e-08},
    "masked/mean": {"flow": 3.34e-08, "flow_arr": 2.92e-07, "flow_g_depth": 4.24e-07, "flow_g_dirs": 1.88e-07, "flow_g_c2w":
        1.69e-07, "flow_g_focal": 1.32e-07, "flow_g_center": 0.00e+00, "depth": 3.29e-08, "depth_arr": 4.18e-07,
        "depth_g_depth": 3.70e-07},
    "masked/per_view": {"flow": 1.10e-08, "flow_arr": 2.92e-07, "flow_g_depth": 5.49e-07, "flow_g_dirs": 1.86e-07,
        "flow_g_c2w": 1.45e-07, "flow_g_focal": 3.07e-08, "flow_g_center": 1.21e-07, "depth": 5.64e-08, "depth_arr":
        4.18e-07, "depth_g_depth": 4.83e-07, "total": 4.13e-08},
    "depth_edges/mean": {"flow": 1.21e-07, "flow_arr": 3.41e-07, "flow_g_depth": 1.15e-07, "flow_g_dirs": 4.52e-07,
        "flow_g_c2w": 4.72e-06, "flow_g_focal": 1.08e-08, "flow_g_center": 9.45e-08, "depth": 5.63e-08, "depth_arr":
        1.98e-07, "depth_g_depth": 1.53e-07},
    "depth_edges/per_view": {"flow": 1.17e-07, "flow_arr": 3.41e-07, "flow_g_depth": 6.00e-08, "flow_g_dirs": 5.92e-07,
        "flow_g_c2w": 7.27e-06, "flow_g_focal": 1.09e-07, "flow_g_center": 1.96e-07, "depth": 7.94e-08, "depth_arr":
        1.98e-07, "depth_g_depth": 3.65e-07, "total": 1.49e-07},
    "quantiles-0.0/mean": {"flow": 2.90e-07, "flow_arr": 2.88e-07, "flow_g_depth": 9.48e-07, "flow_g_dirs": 4.46e-08,
        "flow_g_c2w": 6.16e-08, "flow_g_focal": 1.72e-07, "flow_g_center": 2.24e-08, "depth": 2.12e-06, "depth_arr":
        1.18e-06, "depth_g_depth": 2.84e-06},
    "quantiles-0.0/per_view": {"flow": 2.88e-07, "flow_arr": 2.88e-07, "flow_g_depth": 1.08e-06, "flow_g_dirs": 6.54e-08,
        "flow_g_c2w": 5.67e-08, "flow_g_focal": 2.70e-07, "flow_g_center": 3.48e-08, "depth": 1.18e-06, "depth_arr":
        1.18e-06, "depth_g_depth": 2.82e-06, "total": 2.97e-07},
    "quantiles-0.5/mean": {"flow": 5.22e-08, "flow_arr": 2.57e-07, "flow_g_depth": 3.40e-07, "flow_g_dirs": 1.82e-07,
        "flow_g_c2w": 1.11e-07, "flow_g_focal": 9.35e-08, "flow_g_center": 6.41e-08, "depth": 1.43e-07, "depth_arr":
        5.66e-07, "depth_g_depth": 6.33e-07},
    "quantiles-0.5/per_view": {"flow": 1.16e-07, "flow_arr": 2.57e-07, "flow_g_depth": 8.61e-07, "flow_g_dirs": 1.64e-07,
        "flow_g_c2w": 2.14e-07, "flow_g_focal": 5.31e-08, "flow_g_center": 1.86e-08, "depth": 6.08e-08, "depth_arr":
        5.66e-07, "depth_g_depth": 6.52e-07, "total": 6.63e-08},
    "quantiles-1.0/mean": {"flow": 5.58e-08, "flow_arr": 1.11e-07, "flow_g_depth": 2.23e-07, "flow_g_dirs": 2.68e-07,
        "flow_g_c2w": 2.37e-07, "flow_g_focal": 1.58e-08, "flow_g_center": 1.02e-07, "depth": 6.38e-08, "depth_arr":
        1.47e-07, "depth_g_depth": 1.53e-07},
    "quantiles-1.0/per_view": {"flow": 1.45e-07, "flow_arr": 1.11e-07, "flow_g_depth": 8.70e-08, "flow_g_dirs": 1.51e-07,
        "flow_g_c2w": 1.54e-07, "flow_g_focal": 1.44e-08, "flow_g_center": 1.56e-07, "depth": 5.98e-08, "depth_arr":
        1.47e-07, "depth_g_depth": 2.33e-07, "total": 4.43e-08},
    "photo-1-none": {"photo": 3.94e-08, "photo_g_rgb": 0.00e+00},
    "photo-1-w": {"photo": 3.94e-08, "photo_g_rgb": 5.96e-08},
    "photo-1-w_mean": {"photo": 3.23e-08, "photo_g_rgb": 2.41e-08},
    "photo-5-none": {"photo": 1.41e-08, "photo_g_rgb": 1.49e-08},
    "photo-5-w": {"photo": 1.34e-08, "photo_g_rgb": 2.85e-08},
    "photo-5-w_mean": {"photo": 2.73e-08, "photo_g_rgb": 4.71e-08},
    "photo-341-none": {"photo": 3.65e-10, "photo_g_rgb": 9.31e-10},
    "photo-341-w": {"photo": 2.28e-08, "photo_g_rgb": 5.99e-08},
    "photo-341-w_mean": {"photo": 9.44e-08, "photo_g_rgb": 4.74e-08},
    "photo-1023-none": {"photo": 2.38e-08, "photo_g_rgb": 9.31e-10},
    "photo-1023-w": {"photo": 9.94e-09, "photo_g_rgb": 1.10e-07},
    "photo-1023-w_mean": {"photo": 1.82e-08, "photo_g_rgb": 6.96e-08},
    "photo-1024-none": {"photo": 1.70e-08, "photo_g_rgb": 0.00e+00},
    "photo-1024-w": {"photo": 1.65e-08, "photo_g_rgb": 1.56e-07},
    "photo-1024-w_mean": {"photo": 7.36e-08, "photo_g_rgb": 6.22e-08},
    "photo-1025-none": {"photo": 6.97e-08, "photo_g_rgb": 9.31e-10},
    "photo-1025-w": {"photo": 1.04e-09, "photo_g_rgb": 5.09e-08},
    "photo-1025-w_mean": {"photo": 2.87e-08, "photo_g_rgb": 3.92e-08},
    "photo-4096-none": {"photo": 2.61e-08, "photo_g_rgb": 0.00e+00},
    "photo-4096-w": {"photo": 3.13e-08, "photo_g_rgb": 6.64e-08},
    "photo-4096-w_mean": {"photo": 2.38e-09, "photo_g_rgb": 6.21e-08},
    "rows": {"rows_g_src": 3.44e-08},
    "combine-eight-s": {"combine": 5.34e-08, "combine_g": 4.39e-08},
    "combine-eight-none": {"combine": 7.35e-09, "combine_g": 5.96e-09},
    "combine-single": {"combine": 3.68e-08, "combine_g": 3.48e-08},
}
