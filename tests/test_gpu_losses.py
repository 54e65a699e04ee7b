"""The loss kernels of csrc/lrf_losses.inl on the GPU at the batch shapes and edge inputs of tests/losses_cases.py, held to its
float64 references: views drawn with replacement, one and two frames, the forward-mask rule with a starting frame, rays per
view either side of a power of two and of the 1024-thread stride, masked views and exact ties at the clip threshold, depths
at, below and beyond the clamp, quantiles 0, 0.5 and 1; the photometric loss below and off multiples of 1024 rays; the gathers
past one block; `combine` with all eight terms.

Tolerances: K.tolerance(K.E32[case][quantity]) -- 4 x the error of the float32 CPU chain against float64, not below 8 roundings,
not above the 1e-5 / 2e-6 / 1e-4 of tests/test_gpu_training.py; tests/test_losses_host.py keeps E32 current and checks the
conditions under which zero clip flips can be demanded.  Every case runs twice and must return the same bits.  The direct
calls of the entry points run on tensors carved out of a sentinel pool (util.Pool)."""
import ctypes as C

import numpy as np
import pytest
import torch

import losses_cases as K
from localrf_amd import _native as N
from localrf_amd import losses
from localrf_amd.scene_ops import rows_gather
from util import PAD, Pool

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNWRITTEN = 0x7FD5A5A5                # a NaN no kernel computes: an output element still holding it was not written


def _host(t):
    return t.detach().cpu().numpy()


def _report(tag, rows):
    """rows: (quantity, error, e32, tolerance).  Every figure is printed before anything is asserted."""
    for q, err, e32, tol in rows:
        print(f"[{tag}] {q:14s} e32 {e32:.2e}  tolerance {tol:.2e}  kernel {err:.2e}")
    over = [(q, err, tol) for q, err, e32, tol in rows if not err <= tol]
    assert not over, (tag, over)


# ------------------------------------------------------------------------------------------------------- geometric losses
def _run_geo(c, form, frozen=False):
    """The case through localrf_amd.losses -> {quantity: float32 array}.  mean: view ids on the host (one staged upload);
    per_view: view ids on the device, the sums through `combine` with the weights of K.per_view_coef."""
    leaf = lambda t, grad=True: t.to(DEV).clone().requires_grad_(grad)
    L = dict(depth_map=leaf(c["depth"]), directions=leaf(c["dirs"]), cam2world=leaf(c["c2w"]),
             focal=leaf(c["focal"], not frozen), center=leaf(c["center"], not frozen))
    kw = dict(ij=c["ij"].to(DEV), view_ids=c["view_ids"] if form == "mean" else c["view_ids"].to(DEV), starting_frame_id=c["start"],
              fwd_flow=c["fwd_flow"].to(DEV), fwd_mask=c["fwd_mask"].to(DEV), bwd_flow=c["bwd_flow"].to(DEV), bwd_mask=c["bwd_mask"].to(DEV))
    pv = form == "per_view"
    fl, farr = losses.flow_loss(return_arr=True, per_view=pv, quantile=c["q_flow"], **L, **kw)
    out = {"flow": fl, "flow_arr": farr}
    with_depth = c["n"] > 1
    if with_depth:
        d2 = leaf(c["depth"])
        dl, darr = losses.depth_loss(d2, c["invdepths"].to(DEV), c["V"], quantile=c["q_depth"], return_arr=True, per_view=pv)
        out.update(depth=dl, depth_arr=darr)
    wrt = [v for v in L.values() if v.requires_grad]
    if pv:
        assert fl.shape == (c["V"],)
        (af, bf), (ad, bd) = K.per_view_coef(c)
        total = losses.combine([(fl, af, bf)] + ([(dl, ad, bd)] if with_depth else []), torch.tensor(K.S_REG, device=DEV))
        out["total"] = total
        gf = torch.autograd.grad(total, wrt + ([d2] if with_depth else []), allow_unused=True)
    else:
        gf = torch.autograd.grad(fl, wrt, allow_unused=True) + (torch.autograd.grad(dl, [d2]) if with_depth else ())
    names = ["flow_g_depth", "flow_g_dirs", "flow_g_c2w"] + ([] if frozen else ["flow_g_focal", "flow_g_center"]) + ["depth_g_depth"]
    out.update(zip(names, gf))
    torch.cuda.synchronize()
    return {k: _host(v) for k, v in out.items()}


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", K.GEO_CASES)
def test_geometric_losses_against_float64(name, form):
    """flow_loss and depth_loss (value or per-view sums, clipped array, every gradient; per_view: the total of `combine` too)
    against K.geo_ref, zero clip flips, two runs bit-identical.  masked: the gradients of the fully masked view and of the view
    whose threshold is exactly 0 are exactly zero.

    Measured on an MI355X: docs/LOSS_KERNEL_FIGURES.md lists e32 and the kernels' error per case, form and quantity (the test
    prints them).  The closest any quantity comes to its tolerance is 0.94 of it (flow_g_depth of pow2_edges-3, per_view: 4.5e-7 under the floor of 4.8e-7)."""
    c, ref = K.geo_case(name), K.geo_ref(name, form)
    a, b = _run_geo(c, form), _run_geo(c, form)
    assert set(a) == set(K.quantities(c, form))
    for q in a:
        assert np.array_equal(a[q].view(np.int32), b[q].view(np.int32)), (q, "differs between two runs")
        assert np.isfinite(a[q]).all(), q
    e32 = K.E32[f"{name}/{form}"]
    for arr in ("flow_arr", "depth_arr"):
        if arr in a:
            flips = K.clip_flips(a[arr].reshape(ref[arr].shape), ref[arr])
            print(f"[{name}/{form}] {arr} clip flips {flips}")
            assert flips == 0, arr
    if name == "masked":
        for v in (0, 1):
            assert not a["flow_arr"].reshape(c["V"], -1)[v].any() and not a["flow_g_depth"].reshape(c["V"], -1)[v].any()
            assert not a["flow_g_dirs"].reshape(c["V"], -1)[v].any()
        assert a["flow_arr"].reshape(c["V"], -1)[2].any() and a["flow_g_depth"].reshape(c["V"], -1)[2].any()
    _report(f"{name}/{form}", [(q, K.geo_err(c, q, a[q], ref), e32[q], K.tolerance(e32[q], q)) for q in K.quantities(c, form)])


def test_single_ray_depth_loss_is_not_a_number():
    """n = 1: the reference divides 0 by 0 (the mean absolute deviation of one value); so does the kernel."""
    c = K.geo_case("single_ray")
    val = losses.depth_loss(c["depth"].to(DEV), c["invdepths"].to(DEV), c["V"])
    assert bool(torch.isnan(val))


def test_frozen_intrinsics_take_the_branch_without_their_gradients():
    """focal and center without a tape (LocalTensorfs.freeze_intrinsics): no gradient for them, the others bit-identical to the
    run with intrinsic leaves and within the tolerances of the float64 reference."""
    c = K.geo_case("dup_views")
    a, f = _run_geo(c, "mean"), _run_geo(c, "mean", frozen=True)
    ref = K.geo_run(c, torch.float64, "mean", frozen=True)
    assert "flow_g_focal" not in f and "flow_g_center" not in f and "flow_g_focal" not in ref
    e32 = K.E32["dup_views/mean"]
    for q in f:
        assert np.array_equal(a[q].view(np.int32), f[q].view(np.int32)), q
    _report("dup_views/frozen", [(q, K.geo_err(c, q, f[q], ref), e32[q], K.tolerance(e32[q], q)) for q in f])


# ------------------------------------------------------------------------------------------------------- direct calls
class _Carver:
    """Inputs and outputs of a direct call, carved out of one sentinel pool.  Outputs are pre-filled with UNWRITTEN."""

    def __init__(self, floats):
        self.pool = Pool(floats)
        self.outs = {}

    def f32(self, t):
        return self.pool.take(_host(t).astype(np.float32))

    def ints(self, t, dtype):
        t = t.to(dtype).contiguous()
        v = self.pool.take(np.zeros(t.numel() * t.element_size() // 4)).view(dtype)
        v.copy_(t.reshape(-1))
        return v.view(t.shape)

    def out(self, name, *shape):
        v = self.pool.take(np.zeros(shape))
        v.view(torch.int32).fill_(UNWRITTEN)
        self.outs[name] = v
        return v

    def check(self, tag, only=None):
        """Every element of every output written and no NaN in it, the bytes between the views untouched."""
        torch.cuda.synchronize()
        for name, v in self.outs.items():
            if only is None or name in only:
                assert not bool((v.view(torch.int32) == UNWRITTEN).any()), (tag, name, "an element was not written")
                assert not bool(torch.isnan(v).any()), (tag, name, "NaN: a read past an input")
        assert self.pool.intact(), (tag, "a write outside the views")


def _room(*counts):
    return sum(int(k) + 2 * PAD + 4 for k in counts) + PAD


DIRECT_GEO = ["pow2_edges-3", "pow2_edges-65", "pow2_edges-1025", "pow2_edges-4096", "dup_views"]


@pytest.mark.parametrize("name", DIRECT_GEO)
def test_direct_geometric_calls_in_a_sentinel_pool(name):
    """lrf_flow_loss_fwd/_bwd and lrf_depth_loss_fwd/_bwd through N.launch with every input and output inside a sentinel pool:
    arr, vsum, stats, g_depth, g_dirs, g_cam2world, g_intr and the V x 36 workspace fully written, no NaN picked up from beyond
    an input, nothing written between the views; arrays and depth gradients bit-identical to the autograd path."""
    c = K.geo_case(name)
    V, n, F = c["V"], c["n"], c["F"]
    Vn = V * n
    P = _Carver(_room(*([Vn * 3, Vn, Vn * 4] + [Vn * 2] * 2 + [Vn] * 3 + [F * 12, 2 * V, 2 * V, 1, 2, 1]       # inputs (ij: int64)
                        + [Vn, V, Vn, Vn * 3, F * 12, V * 3, V * 36] + [Vn, V * 6, V, Vn])))                    # outputs
    keep = dict(cam2world=P.f32(c["c2w"]), frame=P.ints(c["frames"], torch.int32),
                fwd_off=P.ints(c["view_ids"] == F - 1, torch.int32), dirs=P.f32(c["dirs"]), depth=P.f32(c["depth"]),
                ij=P.ints(c["ij"], torch.int64), fwd_flow=P.f32(c["fwd_flow"]), fwd_mask=P.f32(c["fwd_mask"]),
                bwd_flow=P.f32(c["bwd_flow"]), bwd_mask=P.f32(c["bwd_mask"]), focal=P.f32(c["focal"]), center=P.f32(c["center"]))
    inv, one = P.f32(c["invdepths"]), P.f32(torch.ones(1))
    a = N.LrfFlowLoss()
    for k, t in keep.items():
        setattr(a, k, t.data_ptr())
    a.F, a.V, a.n, a.quantile = F, V, n, c["q_flow"]
    dev = torch.device(DEV)
    arr, vsum = P.out("arr", V, n), P.out("vsum", V)
    N.launch("lrf_flow_loss_fwd", dev, C.byref(a), N.ptr(arr), N.ptr(vsum))
    P.check((name, "flow fwd"), only={"arr", "vsum"})
    g_depth, g_dirs, g_c2w = P.out("g_depth", V, n), P.out("g_dirs", V, n, 3), P.out("g_cam2world", F, 3, 4)
    g_intr, ws = P.out("g_intr", V, 3), P.out("workspace", V * 36)
    N.launch("lrf_flow_loss_bwd", dev, C.byref(a), N.ptr(arr), N.ptr(one), 1.0 / Vn, N.ptr(g_depth), N.ptr(g_dirs), N.ptr(g_c2w),
             N.ptr(g_intr), N.ptr(ws))
    P.check((name, "flow bwd"))
    darr, stats, dsum, dg = P.out("depth arr", V, n), P.out("stats", V, 6), P.out("depth vsum", V), P.out("depth g_depth", V, n)
    N.launch("lrf_depth_loss_fwd", dev, N.ptr(keep["depth"]), N.ptr(inv), V, n, c["q_depth"], N.ptr(darr), N.ptr(stats), N.ptr(dsum))
    P.check((name, "depth fwd"), only={"depth arr", "stats", "depth vsum"})
    N.launch("lrf_depth_loss_bwd", dev, N.ptr(keep["depth"]), N.ptr(inv), V, n, N.ptr(darr), N.ptr(stats), N.ptr(one), 1.0 / Vn, N.ptr(dg))
    P.check((name, "depth bwd"))
    for k, t in keep.items():                                   # the inputs are as they were
        src = {"frame": c["frames"].int(), "fwd_off": (c["view_ids"] == F - 1).int(), "cam2world": c["c2w"]}.get(k, c.get(k))
        assert torch.equal(t.cpu().reshape(-1), src.reshape(-1)), k
    auto = _run_geo(c, "mean")
    for q, t in (("flow_arr", arr), ("flow_g_depth", g_depth), ("flow_g_dirs", g_dirs), ("flow_g_c2w", g_c2w), ("depth_arr", darr),
                 ("depth_g_depth", dg)):
        assert np.array_equal(_host(t).reshape(-1).view(np.int32), auto[q].reshape(-1).view(np.int32)), q
    assert np.array_equal(_host(stats)[:, 5].view(np.int32), _median_index(c)), "the median's index"


def _median_index(c):
    """Per view the index of the lower median of 1 / clamp(depth) in float32 (unique: tests/test_losses_host.py)."""
    x = np.float32(1) / np.maximum(c["depth"].numpy(), np.float32(1e-6))
    return np.argsort(x, axis=1, kind="stable")[:, (c["n"] - 1) // 2].astype(np.int32)


# ------------------------------------------------------------------------------------------------------- photometric loss
@pytest.mark.parametrize("R", K.PHOTO_SIZES)
def test_photometric_loss_against_float64(R):
    """lrf_photo_loss_fwd/_bwd at ray counts below, at and off multiples of its 1024 threads: without weights, with [R] weights
    and this batch's mean, with [R,1] weights and a supplied mean.  Value and d / d rgb against float64, rows with
    rgb == target exactly zero, two runs bit-identical; then the same launches inside a sentinel pool."""
    p = K.photo_case(R)
    rows = []
    for mode in K.PHOTO_MODES:
        ref, e32 = K.photo_run(p, mode, torch.float64), K.E32[f"photo-{R}-{mode}"]
        w, wm = K.photo_args(p, mode)
        res = []
        for _ in range(2):
            rgb = p["rgb"].to(DEV).requires_grad_(True)
            val = losses.photometric_loss(rgb, p["tgt"].to(DEV), None if w is None else w.to(DEV), None if wm is None else wm.to(DEV))
            (g,) = torch.autograd.grad(val * K.PHOTO_UP, rgb)
            res.append({"photo": _host(val), "photo_g_rgb": _host(g)})
        for q in ref:
            assert np.array_equal(res[0][q].view(np.int32), res[1][q].view(np.int32)), (mode, q)
            rows.append((f"{mode} {q}", K.rel_err(res[0][q], ref[q]), e32[q], K.tolerance(e32[q], q)))
        assert not res[0]["photo_g_rgb"][:p["equal"]].any() and res[0]["photo_g_rgb"][p["equal"]:].all()
    _report(f"photo-{R}", rows)
    P = _Carver(_room(3 * R, 3 * R, R, 1, 1, 1, 1, 3 * R))
    rgb, tgt, w, wm, up = P.f32(p["rgb"]), P.f32(p["tgt"]), P.f32(p["w"]), P.f32(p["wm"].reshape(1)), P.f32(torch.tensor([K.PHOTO_UP]))
    loss, aux, g_rgb = P.out("loss", 1), P.out("aux", 1), P.out("g_rgb", R, 3)
    for wp, mp in ((None, None), (w, None), (w, wm)):
        for t in P.outs.values():
            t.view(torch.int32).fill_(UNWRITTEN)
        N.launch("lrf_photo_loss_fwd", torch.device(DEV), N.ptr(rgb), N.ptr(tgt), N.ptr(wp), N.ptr(mp), R, N.ptr(loss), N.ptr(aux))
        N.launch("lrf_photo_loss_bwd", torch.device(DEV), N.ptr(rgb), N.ptr(tgt), N.ptr(wp), N.ptr(aux), N.ptr(up), R, N.ptr(g_rgb))
        P.check(("photo", R, wp is not None, mp is not None))


# ------------------------------------------------------------------------------------------------------- gathers
@pytest.mark.parametrize("shape", K.GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_gather_is_tensor_indexing(shape):
    """lrf_batch_gather over more than one block (V n = 300 and 4096), negative view ids, pixel ids 0 and HW - 1: every output
    bit-identical to tensor indexing; a call with only `invdepths`; the launch inside a sentinel pool."""
    g = K.gather_case(shape)
    V, n, HW, F = shape
    views, pix = g["views"].to(DEV), g["pix"].to(DEV)
    src = {k: g[k].to(DEV) for k in ("images", "fwd", "bwd", "inv")}
    rows = losses.batch_gather(views, pix, images=src["images"], fwd_flow=src["fwd"], bwd_flow=src["bwd"], invdepths=src["inv"])
    va = (g["views"] % F)[:, None]
    want = {"target": g["images"][va, g["pix"]].reshape(-1, 3), "fwd_flow": g["fwd"][va, g["pix"]].reshape(-1, 2),
            "bwd_flow": g["bwd"][va, g["pix"]].reshape(-1, 2), "invdepths": g["inv"][va, g["pix"]].reshape(-1),
            "fwd_mask": (va < F - 1).float().expand(V, n).reshape(-1), "bwd_mask": (va > 0).float().expand(V, n).reshape(-1)}
    assert set(rows) == set(want)
    for k in want:
        assert torch.equal(rows[k].cpu(), want[k]), k
    only = losses.batch_gather(views, pix, invdepths=src["inv"])
    assert set(only) == {"invdepths"} and torch.equal(only["invdepths"].cpu(), want["invdepths"])
    Vn = V * n
    P = _Carver(_room(F * HW * 3, F * HW * 2, F * HW * 2, F * HW, 2 * V, 2 * Vn, Vn * 3, Vn * 2, Vn, Vn * 2, Vn, Vn))
    a = N.LrfBatchGather()
    keep = [P.f32(g["images"]), P.f32(g["fwd"]), P.f32(g["bwd"]), P.f32(g["inv"]), P.ints(g["views"], torch.int64), P.ints(g["pix"], torch.int64)]
    a.images, a.fwd_flow, a.bwd_flow, a.invdepths, a.view_ids, a.pix = (t.data_ptr() for t in keep)
    a.V, a.n, a.HW, a.n_images = V, n, HW, F
    outs = [P.out("target", Vn, 3), P.out("fwd_flow", Vn, 2), P.out("fwd_mask", Vn), P.out("bwd_flow", Vn, 2), P.out("bwd_mask", Vn),
            P.out("invdepths", Vn)]
    N.launch("lrf_batch_gather", torch.device(DEV), C.byref(a), *[N.ptr(t) for t in outs])
    P.check(("batch_gather", shape))
    for k, t in P.outs.items():
        assert torch.equal(t.cpu(), want[k]), k


def test_rows_gather_forward_is_indexing_and_backward_matches_float64():
    """lrf_rows_gather / _bwd at F = 70, K = 12, V = 30 (V K and F K past one block of 256): repeated and negative ids, a frame
    nobody names (its gradient row is exactly zero).  Forward bit-identical to indexing; backward against float64, two runs
    bit-identical; both launches inside a sentinel pool."""
    r = K.rows_case()
    F, Kk, V = r["F"], r["K"], r["V"]
    ref, e32 = K.rows_run(r, torch.float64), K.E32["rows"]
    idx, up = r["idx"].to(DEV), r["up"].to(DEV)
    res = []
    for _ in range(2):
        src = r["src"].to(DEV).requires_grad_(True)
        out = rows_gather(src, idx)
        assert torch.equal(out.cpu(), r["src"][r["idx"]])
        (g,) = torch.autograd.grad((out * up).sum(), src)
        res.append(_host(g))
    assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)) and not res[0][r["unnamed"]].any()
    _report("rows", [("rows_g_src", K.rel_err(res[0], ref["rows_g_src"]), e32["rows_g_src"], K.tolerance(e32["rows_g_src"], "rows_g_src"))])
    P = _Carver(_room(F * Kk, 2 * V, V * Kk, V * Kk, F * Kk))
    src, ids, upp = P.f32(r["src"]), P.ints(r["idx"], torch.int64), P.f32(r["up"])
    out, g_src = P.out("out", V, Kk), P.out("g_src", F, Kk)
    N.launch("lrf_rows_gather", torch.device(DEV), N.ptr(src), ids.data_ptr(), V, Kk, F, N.ptr(out))
    N.launch("lrf_rows_gather_bwd", torch.device(DEV), N.ptr(upp), ids.data_ptr(), V, Kk, F, N.ptr(g_src))
    P.check("rows_gather")
    assert torch.equal(out.cpu(), r["src"][r["idx"]]) and np.array_equal(_host(g_src).view(np.int32), res[0].view(np.int32))


# ------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("name", K.COMBINE_CASES)
def test_combine_against_float64(name):
    """lrf_loss_combine_fwd/_bwd with LRF_LOSS_TERMS_MAX terms (scalars and length-16 vectors, with s and with s = None) and
    with one term: total and every term's gradient against float64, two runs bit-identical, the launches inside a sentinel pool."""
    xs, coef, s = K.combine_case(name)
    assert len(xs) in (1, N.LRF_LOSS_TERMS_MAX)
    ref, e32 = K.combine_run(name, torch.float64), K.E32[f"combine-{name}"]
    res = []
    for _ in range(2):
        ys = [x.to(DEV).requires_grad_(True) for x in xs]
        total = losses.combine([(y, a, b) for y, (a, b) in zip(ys, coef)], None if s is None else s.to(DEV))
        gs = torch.autograd.grad(total * K.COMBINE_UP, ys)
        assert all(g.shape == y.shape for g, y in zip(gs, ys))
        res.append({"combine": _host(total), "combine_g": np.concatenate([_host(g).reshape(-1) for g in gs])})
    for q in ref:
        assert np.array_equal(res[0][q].view(np.int32), res[1][q].view(np.int32)), q
    _report(f"combine-{name}", [(q, K.rel_err(res[0][q], ref[q]), e32[q], K.tolerance(e32[q], q)) for q in ref])
    k = len(xs)
    P = _Carver(_room(*([x.numel() for x in xs] + [1, 1, 1, k, k])))
    t = N.LrfLossTerms()
    keep = [P.f32(x.reshape(-1)) for x in xs]
    for i, (x, (a, b)) in enumerate(zip(keep, coef)):
        t.x[i], t.n[i], t.a[i], t.b[i] = x.data_ptr(), x.numel(), a, b
    t.count = k
    sv = None if s is None else P.f32(s.reshape(1))
    t.s = None if sv is None else sv.data_ptr()
    up = P.f32(torch.tensor([K.COMBINE_UP]))
    total, w_out, g = P.out("total", 1), P.out("w_out", k), P.out("g", k)
    N.launch("lrf_loss_combine_fwd", torch.device(DEV), C.byref(t), N.ptr(total), N.ptr(w_out))
    N.launch("lrf_loss_combine_bwd", torch.device(DEV), N.ptr(w_out), N.ptr(up), k, N.ptr(g))
    P.check(("combine", name))
    assert np.array_equal(_host(total).view(np.int32).reshape(-1), res[0]["combine"].view(np.int32).reshape(-1))
