"""k_march after its pass B was split in two (the in-chunk scans of up to eight 64-sample chunks side by side, then the
ordered walk with `carry`) and the sample schedule moved into LDS: parity with the ATen port
(oracle/vm_render_torch.py) at the shapes where the grouping can go wrong, the phase clocks of the TIMED kernel, and one
training forward with its gradients.

Shapes: R in {1, 5, 17} (never a multiple of the 4 / 8 / 16 rays of a workgroup), S in {2, 63, 64, 65, 130, 512, 513,
1100}: a partial last chunk, exactly one chunk, one chunk plus one sample, exactly one group of eight chunks (512), one
group plus one chunk (513), more than two groups (1100: 18 chunks = 8 + 8 + 2).  Odd S does not come out of the
reference's schedule (2 * (N // 6) samples): the next even schedule is built and the last sample of its linear half
dropped, which keeps it increasing.

Tolerances are the ones tests/test_gpu_parity.py uses: rgb and depth 1e-4 relative (denominator floor 1e-3), weights
2e-6 absolute, acc 1e-5 absolute.  The shading mask (w > weight_thres) is discontinuous, so a ray with a port weight within
2e-6 of the threshold is left out of the shaded-set and colour comparison; at most 1 % of a case's rays may be (of the 23
rays of a case: none).  The rays of every case were chosen on the CPU, with the port alone (RAY_DRAW): no weight within
4e-6 of the threshold, twice the tolerance, since the port's own weights move by ~1e-7 between host and device;
test_port_alone_stays_clear_of_the_threshold repeats that check without a GPU."""
import ctypes as C

import pytest
import torch

from util import capture_train_ws, check_grads, kernel_relu_masks, make_field, make_rays, port_gradients, quiet

DEV = "cuda:0"
TOL = 1e-4                     # rgb, depth (tests/test_gpu_parity.py)
W_TOL, ACC_TOL = 2e-6, 1e-5    # weights, acc (test_weights_and_acc_vs_oracle)
RS = (1, 5, 17)
SS = (2, 63, 64, 65, 130, 512, 513, 1100)
GRID = [18, 22, 24]
VARIANTS = ("plain", "floater", "early_term", "mask", "no_lds_lines")
FLOATER = 0.25
SEED = {"plain": 11, "floater": 12, "early_term": 13, "mask": 14, "no_lds_lines": 15}


def schedule(S):
    """S increasing sample distances: the reference's schedule for even S, one sample fewer for odd S."""
    from oracle import vm_render_torch as ot
    h = (S + 1) // 2
    z = ot.z_schedule(6 * h)[0]
    if S % 2:
        z = torch.cat([z[:h - 1], z[h:]])
    assert z.numel() == S and bool((z[1:] > z[:-1]).all())
    return z.contiguous()


ALL_SHELLS = (0.9, -0.9, 0.45, -0.45, 1.5, -1.5)
MASK_GRID = (40, 44, 36)


def shells_field(seed, centres, height, width, shift):
    """Near-empty space (density_shift `shift`: sigma ~ 1e-5 and less between the walls, so that no weight there comes near
    the shading threshold) and nested box-shaped shells of dense walls at |x|, |y|, |z| = centres (1.5 lies in the
    contracted region): one rank-1 component per centre and plane (plane = 1, line = a bump).  A ray crosses several walls,
    the weights rise and fall through the threshold within a few samples, and the transmittance that reaches the later
    chunks -- and the forced last sample -- depends on every chunk before them.
    The bumps are kept as low and wide as that allows: a line that rises by h per cell turns the ~1e-6 rounding of a
    sample's cell coordinate into h * 1e-6 of density feature, and alpha = 1 - exp(-sigma * 25 * dist) multiplies it by
    25 * dist, which is 0.8 at S = 63 -- the weights' 2e-6 has no room for walls that are steeper than they need to be."""
    f = quiet(make_field, GRID, "cpu", seed=seed, density_shift=shift)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(0.05)
        for p in range(3):
            L = f.density_line[p].shape[2]
            c = torch.linspace(-2, 2, L)
            for comp, centre in enumerate(centres):
                f.density_plane[p][0, comp].fill_(1.0)
                f.density_line[p][0, comp, :, 0] = height * torch.exp(-((c - centre) / width) ** 2)
    return f


def variant_field(variant, S=0):
    """The CPU field of a case (the mask of "mask" is rebuilt later, on the device).
    Short schedules: a random, semi-transparent field; "early_term" and "mask" need walls (an optical depth above 21 for
    T < 1e-9, empty space for the mask to cut) and get low, wide ones.
    From S = 512 on every variant gets steep shells: in a smooth field sampled 512 times and more, consecutive weights differ
    by ~1e-5 where they cross the threshold, and no choice of rays keeps 23 of them clear of it.
    "mask" has two shells only: a rebuilt mask that cuts about half of the volume."""
    centres = ALL_SHELLS[:2] if variant == "mask" else ALL_SHELLS
    if S >= 512:
        return shells_field(SEED[variant], centres, 20.0, 0.2, -12.0)
    if variant in ("early_term", "mask"):
        return shells_field(SEED[variant], centres, 12.0, 0.35, -9.0)
    f = quiet(make_field, GRID, "cpu", seed=SEED[variant])
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(4.0)
    return f


# (variant, S, R) -> which draw of rays the case uses, where it is not the first: the first one whose port weights, on the
# CPU, all stay 4e-6 (twice the tolerance) clear of the shading threshold
RAY_DRAW = {("plain", 513, 5): 2, ("plain", 513, 17): 2, ("plain", 1100, 5): 3, ("floater", 512, 17): 3, ("floater", 513, 17): 7,
            ("floater", 1100, 5): 3, ("floater", 1100, 17): 5, ("early_term", 512, 17): 1, ("early_term", 513, 5): 2,
            ("mask", 130, 5): 1, ("mask", 513, 5): 1, ("mask", 513, 17): 1, ("mask", 1100, 17): 1, ("no_lds_lines", 512, 17): 1,
            ("no_lds_lines", 513, 17): 3, ("no_lds_lines", 1100, 1): 1, ("no_lds_lines", 1100, 5): 2, ("no_lds_lines", 1100, 17): 1}


def variant_rays(variant, R, S, draw=None):
    draw = RAY_DRAW.get((variant, S, R), 0) if draw is None else draw
    return make_rays(R, 1000 * SEED[variant] + 10 * S + R + 100000 * draw, pinhole=True)


def port_render(fld, rays, z, floater, weight_thres, density_shift=-5.0):
    """rgb, depth from the port's render_field; weights and acc from the same op chain (its lines up to alpha2weights:
    render_field does not return them)."""
    from oracle import vm_render_torch as ot
    import torch.nn.functional as F
    rgb, depth = ot.render_field(fld, rays, z[None], True, floater, density_shift=density_shift, weight_thres=weight_thres)
    o, d = rays[:, :3], rays[:, 3:6]
    dh = d / torch.norm(d, dim=-1, keepdim=True)
    x = o[:, None, :] + dh[:, None, :] * z[None, :, None]
    m = x.abs().amax(dim=-1, keepdim=True).clamp(min=1e-6)
    x = torch.where(m <= 1, x, ((2 * m - 1) / (m ** 2)) * x)
    dists = torch.cat([z[1:] - z[:-1], torch.zeros_like(z[:1])], -1)[None]
    valid = torch.ones(x.shape[:2], dtype=torch.bool, device=x.device)
    aabb = fld["aabb"]
    if fld.get("alphaMask.alpha_volume") is not None:
        maabb = fld.get("alphaMask.aabb", aabb)
        pm = (x.reshape(-1, 3) - maabb[0]) * (1.0 / (maabb[1] - maabb[0]) * 2) - 1
        a = F.grid_sample(fld["alphaMask.alpha_volume"], pm.view(1, -1, 1, 1, 3), align_corners=True).view(-1)
        valid &= (a > 0).view(valid.shape)
    valid[:, -1] = False
    u = (x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1
    sigma = torch.zeros(x.shape[:2], device=x.device)
    if valid.any():
        sigma[valid] = F.softplus(ot.density_feature(fld, u[valid]) + density_shift)
    alpha = 1.0 - torch.exp(-sigma * dists * 25.0)
    w = ot.alpha2weights(alpha)
    acc = w.sum(-1)
    if floater > 0:
        k = torch.arange(alpha.shape[1], device=x.device)[None]
        alpha[k < (w * k).sum(-1, keepdim=True) * floater] = 0
        w = ot.alpha2weights(alpha)
    return rgb, depth, w, acc


def case_floater(variant):
    return FLOATER if variant == "floater" else 0.0


def test_port_alone_stays_clear_of_the_threshold():
    """On the CPU: no port weight of any case within 4e-6 of the shading threshold, so the 1 % cap on excluded rays (0 of
    a case's 23) is the port's own before any kernel runs.  The "mask" cases use the port's update_alpha_mask here."""
    from oracle import vm_render_torch as ot
    for v in VARIANTS:
        for S in SS:
            f = variant_field(v, S)
            fld = {k: t.detach().clone() for k, t in f.state_dict().items()}
            if v == "mask":
                vol = ot.update_alpha_mask(fld, MASK_GRID, float(f.stepSize), density_shift=float(f.density_shift))
                assert 0.02 < float(vol.mean()) < 0.98
                fld["alphaMask.alpha_volume"], fld["alphaMask.aabb"] = vol[None, None], fld["aabb"]
            thres = float(f.rayMarch_weight_thres)
            for R in RS:
                with torch.no_grad():
                    _, _, w, _ = port_render(fld, variant_rays(v, R, S), schedule(S), case_floater(v), thres, float(f.density_shift))
                assert float((w - thres).abs().min()) >= 4e-6, (v, S, R)
                assert int((w[:, :-1] > thres).sum()) >= (R if S > 2 else 0), (v, S, R)      # something is shaded in front of the forced last sample


@pytest.fixture(scope="module")
def fields(built_lib):
    """The device fields, built once: per variant the one of the short schedules and the one of S >= 512; "mask" gets its
    alpha mask rebuilt on the device."""
    out = {}
    for v in VARIANTS:
        for S in (0, 512):
            f = variant_field(v, S).to(DEV)
            if v == "early_term":
                f.early_term_T = 1e-9
            if v == "mask":
                quiet(f.updateAlphaMask, MASK_GRID)
                assert 0.02 < float(f.alphaMask.alpha_volume.mean()) < 0.98      # a mask that cuts, and not everything
            out[v, S] = f
    return out


def _rel(got, ref):
    return ((got - ref).abs() / ref.abs().clamp(min=1e-3)).reshape(got.shape[0], -1).amax(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_parity_with_the_aten_port(built_lib, fields, variant, S):
    f = fields[variant, 512 if S >= 512 else 0]
    z = schedule(S).to(DEV)
    floater = case_floater(variant)
    thres = float(f.rayMarch_weight_thres)
    fld = dict(f.state_dict())
    n_rays = n_excluded = 0
    f.z_override = z
    if variant == "no_lds_lines":
        built_lib.lrf_debug_set_lds_lines(0)
    try:
        for R in RS:
            rays = variant_rays(variant, R, S).to(DEV)
            with torch.no_grad():
                rgb, depth, w, acc, zz = f.render_weights(rays, floater_thresh=floater)
                assert zz.numel() == S and tuple(w.shape) == (R, S)
                rgb_p, depth_p, w_p, acc_p = port_render(fld, rays, z, floater, thres, float(f.density_shift))
            e_w, e_acc = float((w - w_p).abs().max()), float((acc - acc_p).abs().max())
            e_dep, e_rgb = _rel(depth, depth_p), _rel(rgb, rgb_p)
            near = ((w_p - thres).abs() < W_TOL).any(-1)                       # rays the shading threshold may flip
            print(variant, "S", S, "R", R, "w", e_w, "acc", e_acc, "depth", float(e_dep.max()), "rgb", float(e_rgb.max()),
                  "near", int(near.sum()), "shaded", int((w_p > thres).sum()))
            assert e_w < W_TOL, (R, e_w)
            assert e_acc < ACC_TOL, (R, e_acc)
            assert float(e_dep.max()) < TOL, (R, float(e_dep.max()))
            keep = ~near
            assert bool(((w > thres) == (w_p > thres))[keep].all()), R         # the shaded lists (w is the very float the kernel compares)
            assert float(e_rgb[keep].max() if keep.any() else 0.0) < TOL, (R, float(e_rgb.max()))
            n_rays += R
            n_excluded += int(near.sum())
    finally:
        f.z_override = None
        if variant == "no_lds_lines":
            built_lib.lrf_debug_set_lds_lines(1)
    assert n_excluded <= int(0.01 * n_rays), (n_excluded, n_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("lds_lines", [1, 0])
@pytest.mark.parametrize("S", [65, 513])
def test_phase_clocks(built_lib, fields, S, lds_lines):
    """k_march_timed: four non-zero phase totals per ray, and the very outputs of the production kernel."""
    f = fields["plain", 0]
    R = 17
    rays = variant_rays("plain", R, S).to(DEV)
    f.z_override = schedule(S).to(DEV)
    dump = torch.zeros(R, 4, dtype=torch.int64, device=DEV)
    try:
        built_lib.lrf_debug_set_lds_lines(lds_lines)
        with torch.no_grad():
            rgb0, depth0, w0, acc0, _ = f.render_weights(rays)
            torch.cuda.synchronize()
            built_lib.lrf_debug_march_phases(C.c_void_p(dump.data_ptr()))
            rgb1, depth1, w1, acc1, _ = f.render_weights(rays)
            torch.cuda.synchronize()
    finally:
        built_lib.lrf_debug_march_phases(None)
        built_lib.lrf_debug_set_lds_lines(1)
        f.z_override = None
    print("phases (cycles, mean over rays)", dump.double().mean(0).tolist())
    assert bool((dump > 0).all()), dump
    assert torch.equal(rgb0, rgb1) and torch.equal(depth0, depth1) and torch.equal(w0, w1) and torch.equal(acc0, acc1)


@pytest.mark.gpu
def test_training_forward_and_gradients(built_lib):
    """is_train=True with a jittered schedule, 64 rays x 130 samples (three chunks, the last one partial), through the
    row-saving forward: outputs against the port, every gradient within check_grads' 1e-4."""
    from oracle import vm_render_torch as ot
    R, N = 64, 390
    f = variant_field("plain").to(DEV)
    gen = torch.Generator().manual_seed(77)
    jit = (torch.rand(N // 6, generator=gen), torch.rand(N // 6, generator=gen))
    z = ot.z_schedule(N, jitter=jit)[0].contiguous()
    assert z.numel() == 130
    rays = make_rays(R, 256, pinhole=True).to(DEV).requires_grad_(True)      # (the first seed from 78 on with every port weight 4e-6 clear of the threshold)
    g_rgb = torch.randn(R, 3, generator=gen).to(DEV)
    g_depth = torch.randn(R, generator=gen).to(DEV)
    f.z_override = z.clone()
    try:
        with capture_train_ws(f) as cap:
            rgb, depth = f(rays, white_bg=True, is_train=True, N_samples=N)
            ((rgb * g_rgb).sum() + (depth * g_depth).sum()).backward()
            torch.cuda.synchronize()
            masks = kernel_relu_masks(f, rays, z.to(DEV), cap.ws)
    finally:
        f.z_override = None
    mine = {n: p.grad.clone() for n, p in f.named_parameters() if p.grad is not None}
    mine["rays"] = rays.grad.clone()
    ref, info = port_gradients(f, rays.detach(), z.to(DEV), g_rgb, g_depth, True, masks, list(mine))
    assert info.get("n_forced", 0) >= 0.98 * masks[3], (info, masks[3])
    with torch.no_grad():
        rgb_p, depth_p = ot.render_field(dict(f.state_dict()), rays.detach(), z.to(DEV)[None], True, 0.0,
                                         weight_thres=f.rayMarch_weight_thres)
    assert float(_rel(depth.detach(), depth_p).max()) < TOL and float(_rel(rgb.detach(), rgb_p).max()) < TOL
    worst = check_grads(mine, ref)
    print("training forward: worst gradient error", max(worst.values()))
