"""k_shade3 after its tail left the LDS pipe (join_halves32 / half_sum32) and its header stopped waiting for the sample index
(the aligned dword of the 16-bit list, taken apart at the use): small fields through the public forward.

Cases: R in {5, 64, 300} x S in {65, 128} x two wall fields.  R = 5 leaves most of the 256 workgroups without a ray; S = 65 makes
R * S odd for odd R, so the last index dword of the list is the half-used one.  "walls" shades with the default threshold
(weights > 1e-3), "faint" with 0.03, under which whole rays shade nothing.  The seeds were chosen on the CPU with
oracle/vm_render_torch.py (weights no closer than 2e-5 to the threshold) so that the per-ray shaded counts of the R = 300 cases
include 0, 1, 31, 32, 33 and counts >= 65: an empty ray, a one-sample tile, a tile one short of full, a full tile, a tile
and one sample, three tiles.  test_shaded_counts_cover_the_edges asserts that from the kernel's own weights.

Per case: the default engine against the exact-fp32 engine (3e-5, colours in [0, 1]); tile offsets built in the kernel
against global offsets (lrf_debug_set_lds_toff(0)), bit for bit; the training forward's rgb against the eval's, bit for bit;
two consecutive calls, bit for bit.  One-field lrf_scene_fwd against the single-field call, bit for bit."""
import pytest
import torch

from util import make_field, make_rays, quiet

DEV = "cuda:0"
GRID = [28, 24, 32]
RS = (5, 64, 300)
SS = (65, 128)
THRES = {"walls": 1e-3, "faint": 0.03}


def wall_field(thres):
    f = quiet(make_field, GRID, "cpu", seed=6, density_shift=-9.0, rayMarch_weight_thres=thres)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(0.05)
        for p in range(3):
            L = f.density_line[p].shape[2]
            c = torch.linspace(-2, 2, L)
            for comp, centre in enumerate((0.9, -0.9)):
                f.density_plane[p][0, comp].fill_(1.0)
                f.density_line[p][0, comp, :, 0] = 6.0 * torch.exp(-((c - centre) / 0.25) ** 2)
    return f.to(DEV)


@pytest.fixture(scope="module")
def fields(built_lib):
    return {name: wall_field(t) for name, t in THRES.items()}


def schedule(f, S):
    """S sample distances: the field's own schedule of S (or S + 1) samples, cut to S."""
    f.z_override = None
    z = f.z_schedule(False, 3 * (S + (S & 1)), torch.device(DEV))
    return z.view(-1)[:S].clone()


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("name", tuple(THRES))
def test_case(built_lib, fields, name, R, S):
    f = fields[name]
    rays = make_rays(R, 100, pinhole=True).to(DEV)
    f.z_override = schedule(f, S)
    try:
        with torch.no_grad():
            rgb, depth, w, acc, z = f.render_weights(rays)
            assert z.numel() == S
            first = (rgb.clone(), depth.clone(), acc.clone())
            again = [t.clone() for t in f.render_weights(rays)[:2]]
            f.mlp_engine = "f32"
            exact = f.render_weights(rays)[0].clone()
            f.mlp_engine = "bf16x3"
            built_lib.lrf_debug_set_lds_toff(0)
            g_rgb, g_depth, _, g_acc, _ = f.render_weights(rays)
            glob = (g_rgb.clone(), g_depth.clone(), g_acc.clone())
            built_lib.lrf_debug_set_lds_toff(1)
            ev = [t.clone() for t in f(rays, white_bg=True, is_train=False, N_samples=-1)]
        tr = [t.detach().clone() for t in f(rays, white_bg=True, is_train=True, N_samples=-1)]
        torch.cuda.synchronize()
    finally:
        f.mlp_engine = "bf16x3"
        built_lib.lrf_debug_set_lds_toff(1)
        f.z_override = None
    n = (w > f.rayMarch_weight_thres).sum(-1)
    print(name, "R", R, "S", S, "shaded per ray: min", int(n.min()), "max", int(n.max()), "rays without a sample", int((n == 0).sum()))
    assert bool(torch.isfinite(rgb).all()) and (name != "walls" or int(n.sum()) > R)
    err = float((rgb - exact).abs().max())
    print("max |rgb - rgb(f32 engine)|", err)
    assert err < 3e-5, err
    for a, b, what in zip(first, glob, ("rgb", "depth", "acc")):
        assert torch.equal(a, b), ("LDS offsets against global offsets", what)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two consecutive calls"
    assert torch.equal(ev[0], first[0]) and torch.equal(ev[1], first[1]), "forward() against render_weights()"
    assert torch.equal(tr[0], ev[0]), ("training forward rgb against eval", float((tr[0] - ev[0]).abs().max()))


@pytest.mark.gpu
def test_shaded_counts_cover_the_edges(built_lib, fields):
    """The R = 300 cases, from the kernel's own weights against the field's threshold: every edge count occurs."""
    import numpy as np
    seen = []
    for name, f in fields.items():
        for S in SS:
            f.z_override = schedule(f, S)
            try:
                with torch.no_grad():
                    w = f.render_weights(make_rays(300, 100, pinhole=True).to(DEV))[2]
            finally:
                f.z_override = None
            n = (w > f.rayMarch_weight_thres).sum(-1).cpu().numpy()
            print(name, "S", S, "counts", np.unique(n))
            seen.append(n)
    have = np.unique(np.concatenate(seen))
    for c in (0, 1, 31, 32, 33):
        assert c in have, (c, have)
    assert have.max() >= 65, have


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
def test_one_field_scene_forward_equals_the_field_call(built_lib, fields, S):
    """lrf_scene_fwd with one field (its per-field path: k_march -> k_shade3 on the rays it forms, blend with weight 1, clamp)
    against the same field called on those rays."""
    from localrf_amd.scene_ops import scene_forward, scene_rays
    f = fields["walls"]
    W, H, R = 24, 18, 300
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, W * H, (R,), generator=gen).to(DEV)
    c2w = torch.eye(4)[None, :3, :].clone()
    c2w[0, :, 3] = torch.tensor([0.05, -0.03, 0.02])
    c2w = c2w.to(DEV)
    w2rf = torch.zeros(1, 3, device=DEV)
    focal, center = torch.tensor([14.0], device=DEV), torch.tensor([W / 2.0, H / 2.0], device=DEV)
    bw = torch.ones(1, 1, device=DEV)
    f.z_override = schedule(f, S)
    try:
        with torch.no_grad():
            rgbs, depth, _, _ = scene_forward(ids, c2w, w2rf, focal, center, R, W, H, False, [f], True, 0.0, 4096, bw, None)
            rays, _, _ = scene_rays(ids, c2w, w2rf, focal, center, R, W, H, False)
            rgb1, depth1, w, _, _ = f.render_weights(rays[0].contiguous())
        torch.cuda.synchronize()
    finally:
        f.z_override = None
    assert int((w > f.rayMarch_weight_thres).sum()) > R
    assert torch.equal(depth, depth1)
    assert torch.equal(rgbs, rgb1.clamp(0.0, 1.0)), float((rgbs - rgb1.clamp(0.0, 1.0)).abs().max())
