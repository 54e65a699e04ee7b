"""The field-upkeep kernels on the GPU -- k_upsample_bilinear (csrc/lrf_losses.inl), k_dense_alpha / k_alpha_pool with
alpha_mask_sample (csrc/lrf_mask.inl, lrf_common.h), k_density_feature / k_app_feature / k_sample_ray_aabb / k_sample_contracted
(csrc/lrf_render.hip) -- at the shapes and edge inputs of tests/upkeep_cases.py, held to its float64 references: line-shaped,
one-row, one-output, identity and shrinking resizes, 255 / 256 / 257 outputs and one launch above the 65535 x 4 block cap;
lattices with an axis of 1 or 2, three different lengths, values on, below and above the threshold and through the clamp;
dense alpha with and without a previous mask, on the previous mask's own lattice planes, above softplus's threshold of 20 and
with relu; feature lookups at -1, +1, +-1.5, on texel centres and on a one-texel grid at P either side of a block; aabb rays
with zero components, misses, both clamps and N = 1; contracted points with an infinity norm of exactly 1.

Tolerances: K.tolerance(K.E32[case][quantity], quantity) -- 4 x the error of the float32 CPU evaluation against float64, not
below 8 roundings, not above the 1e-6 / 2e-6 the suite demands already; tests/test_upkeep_host.py keeps E32 current.  Binary
outputs (mask cells, `inside` flags) are asserted exactly on the sets float64 decides (K.mask_sets, K.flag_sets) and counted
elsewhere.  The pool kernel is an exact function of its input: bit for bit.  Every case runs twice and must return the same
bits; the direct calls run on tensors carved out of a sentinel pool (util.Pool), 16-byte aligned and one float past that.

Measured on an MI355X: docs/FIELD_UPKEEP_FIGURES.md lists e32, tolerance and the kernels' error per case and quantity (the
tests print them).  No defect found.  The closest any quantity comes to its tolerance is 0.37 of it (`xc` of the contracted
case `3x85`: 2.9e-7 under 7.6e-7).  Undecidable mask cells: at most 1.8 % (`B/rebuild`, 143 of 7920) outside the
coincident-lattice case, which has 35 of 4641; there the kernel differs from float64 on 2 cells and from the float32 ATen
evaluation on 9, all of them undecidable.  Undecidable `inside` flags: 5 of 3200 in `64x50/eval`, none elsewhere; the kernel
flips no flag.  Seven temporarily wrong kernels each fail the cases written for them; one (no 1e-6 for a zero direction
component) passed everything until the `graze` ray was added."""
import ctypes as C

import numpy as np
import pytest
import torch

import upkeep_cases as K
from localrf_amd import AlphaGridMask
from localrf_amd import _native as N
from oracle import vm_render_torch as ot
from util import PAD, Pool, make_field, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNWRITTEN = 0x7FD5A5A5                # a NaN no kernel computes: an output element still holding it was not written
MIS = [0, 1]


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _report(tag, rows):
    """rows: (quantity, error, e32, tolerance).  Every figure is printed before anything is asserted."""
    for q, err, e32, tol in rows:
        print(f"[{tag}] {q:6s} e32 {e32:.2e}  tolerance {tol:.2e}  kernel {err:.2e}")
    over = [(q, err, tol) for q, err, e32, tol in rows if not err <= tol]
    assert not over, (tag, over)


def _row(key, q, err):
    e32 = K.E32[key][q]
    return (q, err, e32, K.tolerance(e32, q))


class _Carver:
    """Inputs and outputs of a direct call, carved out of one sentinel pool: 16-byte aligned (mis = 0) or one float past that
    (mis = 1); outputs pre-filled with UNWRITTEN."""

    def __init__(self, mis, *counts):
        self.pool, self.mis, self.outs = Pool(sum(int(k) + 2 * PAD + 8 for k in counts) + PAD), mis, {}

    def f32(self, a):
        return self.pool.take(np.asarray(a, np.float32), mis=self.mis)

    def out(self, name, *shape):
        v = self.pool.take(np.zeros(shape), mis=self.mis)
        v.view(torch.int32).fill_(UNWRITTEN)
        self.outs[name] = v
        return v

    def check(self, tag):
        torch.cuda.synchronize()
        for name, v in self.outs.items():
            assert not bool((v.view(torch.int32) == UNWRITTEN).any()), (tag, name, "an element was not written")
            assert not bool(torch.isnan(v).any()), (tag, name, "NaN: a read past an input")
        assert self.pool.intact(), (tag, "a write outside the views")


def _dev():
    return torch.device(DEV)


# ------------------------------------------------------------------------------------------------------------------ upsample
def _resize(src, dst, H2, W2):
    C_, H, W = src.shape
    N.launch("lrf_upsample_bilinear", _dev(), N.ptr(src), C_, H, W, N.ptr(dst), H2, W2)


@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("name", K.UP_CASES[:-1])
def test_upsample_direct_against_float64(name, mis):
    """lrf_upsample_bilinear inside a sentinel pool against ATen's align_corners=True formula in float64: every output written,
    nothing else touched, two runs the same bits; the identity resize returns its input bit for bit."""
    src, H2, W2, idx = K.up_case(name)
    P = _Carver(mis, src.size, idx.size, idx.size)
    s = P.f32(src)
    a, b = P.out("dst", src.shape[0], H2, W2), P.out("again", src.shape[0], H2, W2)
    _resize(s, a, H2, W2)
    _resize(s, b, H2, W2)
    P.check(name)
    assert np.array_equal(_host(s), src), "the source was changed"
    got = _host(a)
    assert np.array_equal(_bits(got), _bits(_host(b)))
    if name == K.UP_IDENTITY:
        assert np.array_equal(_bits(got), _bits(src))
    _report(f"up:{name}", [_row(f"up:{name}", "up", K.abs_err(got.reshape(-1), K.up_ref(name)))])


def test_upsample_above_the_launch_cap():
    """67 415 424 outputs: 307 584 more than the 65535 x 4 blocks of 256 threads cover, so the stride loop runs a second time.
    Every 61st element and the last 4096 against float64; no element left unwritten."""
    src, H2, W2, idx = K.up_case(K.UP_BIG)
    s = torch.from_numpy(src).to(DEV)
    dst = torch.full((src.shape[0], H2, W2), float("nan"), device=DEV)
    _resize(s, dst, H2, W2)
    torch.cuda.synchronize()
    assert dst.numel() > K.LAUNCH_CAP and not bool(torch.isnan(dst).any()), "an element was not written"
    got = _host(dst.reshape(-1)[torch.from_numpy(idx).to(DEV)])
    tail = idx >= K.LAUNCH_CAP
    print(f"[up:{K.UP_BIG}] second trip alone: kernel {K.abs_err(got[tail], K.up_ref(K.UP_BIG)[tail]):.2e} on {int(tail.sum())} elements")
    _report(f"up:{K.UP_BIG}", [_row(f"up:{K.UP_BIG}", "up", K.abs_err(got, K.up_ref(K.UP_BIG)))])


def test_upsample_through_the_field():
    """upsample_volume_grid (5,7,9) -> (12,8,10): the twelve tensors against float64, stepSize and nSamples against the
    reference's expressions (tensorBase.py:317-330), new Parameter objects, two runs the same bits."""
    cpu = K.upfield_field()
    ref, step, ns = K.upfield_ref(cpu)
    runs = []
    for _ in range(2):
        f = K.upfield_field().to(DEV)
        before = list(f._param_list()[:12])                      # kept alive: a new tensor cannot take an old one's address
        f.upsample_volume_grid(list(K.UPFIELD[1]))
        torch.cuda.synchronize()
        assert not {p.data_ptr() for p in before} & {p.data_ptr() for p in f._param_list()[:12]}
        runs.append({k: _host(v) for k, v in f.state_dict().items() if k in ref})
    assert set(runs[0]) == set(ref) and len(ref) == 12
    err = 0.0
    for k, v in ref.items():
        assert runs[0][k].shape == v.shape and np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
        err = max(err, K.abs_err(runs[0][k], v))
    print(f"[upfield] stepSize {float(f.stepSize):.9g} against {step:.9g}, nSamples {f.nSamples} against floor({ns:.6f}) + 1")
    assert abs(float(f.stepSize) - step) <= 4 * 2.0 ** -24 * step and f.nSamples == int(ns) + 1
    assert f.gridSize.tolist() == list(K.UPFIELD[1]) and f.layout.grid == K.UPFIELD[1]
    _report("upfield:5x7x9-12x8x10", [_row("upfield:5x7x9-12x8x10", "up", err)])


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("lat", K.POOL_LATTICES, ids=lambda l: "x".join(map(str, l)))
def test_alpha_pool_threshold_bit_for_bit(lat, mis):
    """lrf_alpha_pool_threshold inside a sentinel pool against the numpy max-pool over the same floats, bit for bit: random
    alpha, a single 1 at each corner (kept: exactly the clipped 2x2x2 block), -0.5 and 1.5 through the clamp, thres and its two
    neighbours alone in a field of zeros, thres = 0."""
    gx, gy, gz = lat
    for name, alpha, thres, expect in K.pool_inputs(lat):
        P = _Carver(mis, alpha.size, alpha.size)
        a, out = P.f32(alpha), P.out("mask", gz, gy, gx)
        N.launch("lrf_alpha_pool_threshold", _dev(), N.ptr(a), gx, gy, gz, float(thres), N.ptr(out))
        P.check((lat, name))
        got = _host(out)
        assert np.array_equal(_host(a), alpha), "the input was changed"
        assert np.array_equal(_bits(got), _bits(K.pool_ref(alpha, thres))), (lat, name, int((got != K.pool_ref(alpha, thres)).sum()))
        assert expect is None or np.array_equal(got, expect), (lat, name)


# ------------------------------------------------------------------------------------------------------------------ mask
def _mask_field(name):
    f = K.mask_field(name, DEV)
    prev = K.mask_prev(name)
    if prev is not None:
        f.alphaMask = AlphaGridMask(_dev(), torch.from_numpy(prev[1]).to(DEV), torch.from_numpy(prev[0]).to(DEV))
    return f


def _run_mask(name):
    lat = K.MASK_CASES[name][3]
    f = _mask_field(name)
    dense = f.getDenseAlpha(lat)
    assert tuple(dense.shape) == tuple(lat)
    dense = _host(dense)                                         # [X][Y][Z], as the reference indexes it
    f.updateAlphaMask(lat)
    torch.cuda.synchronize()
    return f, dense, _host(f.alphaMask.alpha_volume[0, 0])


@pytest.mark.parametrize("name", list(K.MASK_CASES))
def test_dense_alpha_and_mask_against_float64(name):
    """getDenseAlpha and updateAlphaMask against K.mask_ref: alpha within the tolerance at every lattice point whose validity
    float64 decides (within it of 0 or of the unmasked value at the others), read through the returned [X][Y][Z] view; the
    mask equal on every decidable cell, 0.0 or 1.0 everywhere; two runs the same bits.  The coincident-lattice case also
    against the float32 ATen evaluation: both counts of differing cells are printed, every one on an undecidable cell."""
    lat, ref = K.MASK_CASES[name][3], K.mask_ref(name)
    f, dense, mask = _run_mask(name)
    _, dense2, mask2 = _run_mask(name)
    assert np.array_equal(_bits(dense), _bits(dense2)) and np.array_equal(_bits(mask), _bits(mask2))
    assert mask.shape == lat[::-1] and f.alphaMask.gridSize.tolist() == list(lat) and np.isin(mask, (0.0, 1.0)).all()
    assert np.array_equal(_host(f.alphaMask.aabb), _host(f.aabb))
    tol = K.tolerance(K.E32[f"mask:{name}"]["alpha"], "alpha")
    m64, keep, drop = K.mask_sets(ref, tol)
    dec = keep | drop
    diff = mask != m64
    print(f"[mask:{name}] kept {mask.mean():.3f}, undecidable cells {int((~dec).sum())} of {dec.size}, the kernel differs from float64 "
          f"on {int(diff.sum())} cells, {int((diff & dec).sum())} of them decidable")
    if name == K.COINCIDENT:
        fld = dict(K.mask_field(name).state_dict())
        prev = K.mask_prev(name)
        fld["alphaMask.alpha_volume"], fld["alphaMask.aabb"] = torch.from_numpy(prev[0])[None, None], torch.from_numpy(prev[1])
        aten = ot.update_alpha_mask(fld, lat, float(f.stepSize), float(K.THRES), float(f.density_shift)).numpy()
        d2 = mask != aten
        print(f"[mask:{name}] the kernel differs from the float32 ATen evaluation on {int(d2.sum())} cells, {int((d2 & dec).sum())} of them "
              f"decidable; ATen from float64 on {int((aten != m64).sum())}")
        assert not (d2 & dec).any()
    rows = [_row(f"mask:{name}", "alpha", K.alpha_err(dense.transpose(2, 1, 0), ref))]
    _report(f"mask:{name}", rows)
    assert not (diff & dec).any()


def test_render_through_the_rebuilt_noncubic_mask():
    """64 rays through the 33x31x17 mask the kernels rebuilt through a 20x18x22 one (k_march's alpha_mask_sample on a mask whose
    three lengths differ), against oracle.render_field in float64 with the same mask, at the bars of test_gpu_parity._check_rays."""
    f, _, mask = _run_mask(K.RENDER_CASE)
    rays = torch.from_numpy(K.render_rays()).to(DEV)
    with torch.no_grad():
        rgb, depth = f(rays, white_bg=True, is_train=False, N_samples=K.RENDER_NS)
    want_rgb, want_depth, _ = K.render_ref(K.mask_field(K.RENDER_CASE), mask)
    for q, got, ref in (("rgb", _host(rgb), want_rgb), ("depth", _host(depth), want_depth)):
        err = (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).reshape(len(ref), -1).max(-1)
        print(f"[mask:{K.RENDER_CASE}] render {q}: worst ray {err.max():.2e} against 1e-4")
        assert (err <= 1e-4).all(), q


# ------------------------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("name", K.FEAT_CASES)
def test_feature_kernels_against_float64(name, mis):
    """lrf_density_feature and lrf_app_feature inside a sentinel pool against oracle.density_feature / app_feature in float64, at
    the coordinates of K.feat_coords; two runs the same bits, the bits of compute_densityfeature / compute_appfeature."""
    grid, u = K.feat_case(name)
    f = K.feat_field(grid, DEV)
    P_ = len(u)
    P = _Carver(mis, u.size, P_, P_, 27 * P_, 27 * P_)
    uu = P.f32(u)
    sig, sig2, app, app2 = P.out("sig", P_), P.out("sig2", P_), P.out("app", P_, 27), P.out("app2", P_, 27)
    f._ensure_cache()
    cf = f._c_field()
    for s, a in ((sig, app), (sig2, app2)):
        N.launch("lrf_density_feature", _dev(), C.byref(cf), N.ptr(uu), P_, N.ptr(s))
        N.launch("lrf_app_feature", _dev(), C.byref(cf), N.ptr(uu), P_, N.ptr(a))
    P.check(name)
    assert np.array_equal(_host(uu), u), "the coordinates were changed"
    got = {"sig": _host(sig), "app": _host(app)}
    assert np.array_equal(_bits(got["sig"]), _bits(_host(sig2))) and np.array_equal(_bits(got["app"]), _bits(_host(app2)))
    ud = torch.from_numpy(u).to(DEV)
    assert np.array_equal(_bits(got["sig"]), _bits(_host(f.compute_densityfeature(ud))))
    assert np.array_equal(_bits(got["app"]), _bits(_host(f.compute_appfeature(ud))))
    ref = K.feat_ref(name)
    _report(f"feat:{name}", [_row(f"feat:{name}", q, K.abs_err(got[q], ref[q])) for q in ("sig", "app")])


# ------------------------------------------------------------------------------------------------------------------ rays
def _flags_view(P, n):
    v = P.pool.take(np.zeros((n + 3) // 4))
    b = v.view(torch.uint8)
    b.fill_(0xA5)
    return b


@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("name", K.RAY_CASES)
def test_sample_ray_aabb_against_float64(name, mis):
    """lrf_sample_ray_aabb inside a sentinel pool against oracle.sample_ray_aabb in float64: t and pts within the tolerance,
    `inside` 0 or 1 and exact on every flag float64 decides, the bytes behind the flags untouched; two runs the same bits."""
    rays, n, jit = K.ray_case(name)
    R = len(rays)
    P = _Carver(mis, rays.size, R, 3 * R * n, R * n, 3 * R * n, R * n, R * n, R * n)
    r, j = P.f32(rays), (None if jit is None else P.f32(jit))
    aabb = (C.c_float * 6)(*K.AABB.reshape(-1).tolist())
    outs = []
    for k in range(2):
        pts, t, ins = P.out(f"pts{k}", R, n, 3), P.out(f"t{k}", R, n), _flags_view(P, R * n)
        N.launch("lrf_sample_ray_aabb", _dev(), N.ptr(r), aabb, K.STEP, K.NEAR_FAR[0], K.NEAR_FAR[1], N.ptr(j), R, n, N.ptr(pts), N.ptr(t), ins.data_ptr())
        outs.append((pts, t, ins))
    P.check(name)
    assert np.array_equal(_host(r), rays), "the rays were changed"
    (pts, t, ins), again = [tuple(_host(x) for x in o) for o in outs]
    for x, y in zip((pts, t), again):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.array_equal(ins, again[2]) and (ins[R * n:] == 0xA5).all() and np.isin(ins[:R * n], (0, 1)).all()
    ref = K.ray_ref(name)
    rows = [_row(f"ray:{name}", "t", K.rel1_err(t, ref["t"])), _row(f"ray:{name}", "pts", K.rel1_err(pts, ref["pts"]))]
    inside, outside = K.flag_sets(ref["pts"], rows[1][3])
    dec = inside | outside
    diff = ins[:R * n].reshape(R, n).astype(bool) != ref["inside"]
    print(f"[ray:{name}] undecidable flags {int((~dec).sum())} of {dec.size}, the kernel differs from float64 on {int(diff.sum())}, "
          f"{int((diff & dec).sum())} of them decidable")
    _report(f"ray:{name}", rows)
    assert not (diff & dec).any()


@pytest.mark.parametrize("mode", ["eval", "jit"])
def test_sample_ray_method_returns_the_kernel_s_bits(mode):
    """TensorBase.sample_ray on a 32^3 field (64 rays x 50 samples): the step K.STEP stands for, the direct call's values."""
    rays, n, jit = K.ray_case(f"64x50/{mode}")
    f = quiet(make_field, K.RAY_GRID, "cpu", seed=5).to(DEV)
    assert float(f.stepSize) == K.STEP and np.array_equal(_host(f.aabb), K.AABB) and tuple(f.near_far) == K.NEAR_FAR
    r = torch.from_numpy(rays).to(DEV)
    pts, t, inside = f.sample_ray(r[:, :3], r[:, 3:], is_train=jit is not None, N_samples=n, jitter=None if jit is None else torch.from_numpy(jit))
    ref = K.ray_ref(f"64x50/{mode}")
    rows = [_row(f"ray:64x50/{mode}", "t", K.rel1_err(_host(t), ref["t"])), _row(f"ray:64x50/{mode}", "pts", K.rel1_err(_host(pts), ref["pts"]))]
    ins, out = K.flag_sets(ref["pts"], rows[1][3])
    _report(f"ray:64x50/{mode} (method)", rows)
    assert inside.dtype == torch.bool and np.array_equal(_host(inside)[ins | out], ref["inside"][ins | out])


@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("name", K.CON_CASES)
def test_sample_ray_contracted_against_float64(name, mis):
    """lrf_sample_ray_contracted inside a sentinel pool against oracle.sample_ray_contracted in float64: origins whose infinity
    norm is exactly 1 (returned bit for bit), the float above 1, below 1e-6; the far end of the schedule; two runs the same bits."""
    o, d, z = K.con_case(name)
    R, S = len(o), len(z)
    P = _Carver(mis, o.size, d.size, S, 3 * R * S, 3 * R * S)
    oo, dd, zz = P.f32(o), P.f32(d), P.f32(z)
    a, b = P.out("pts", R, S, 3), P.out("again", R, S, 3)
    for out in (a, b):
        N.launch("lrf_sample_ray_contracted", _dev(), N.ptr(oo), N.ptr(dd), N.ptr(zz), R, S, N.ptr(out))
    P.check(name)
    got = _host(a)
    assert np.array_equal(_bits(got), _bits(_host(b)))
    for k in range(R):
        if not d[k].any() and np.abs(o[k]).max() <= 1:
            assert np.array_equal(_bits(got[k]), _bits(np.broadcast_to(o[k], (S, 3)))), k
    _report(f"con:{name}", [_row(f"con:{name}", "xc", K.abs_err(got, K.con_ref(name)["xc"]))])
