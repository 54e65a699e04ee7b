"""The colour kernel's tile offsets from k_march's group sums (tile_range_fill / tile_range_finish, csrc/lrf_shade3.inl) instead of a scan of
every ray's count in every workgroup.

1. Partition: lrf_debug_tile_ranges runs the prologue's device function in a kernel of its own; per workgroup its rays
   [ra, rb), tiles [T0, T1), and the offsets / counts it holds for those rays must be numpy's integers (cumsum of
   ceil(n / 32), searchsorted(side="left"), last workgroup -> R).  Synthetic counts, the smallest that can go wrong.
2. Two implementations: the same batch through the in-kernel offsets and through k_scan_tiles_n + global offsets
   (lrf_debug_set_lds_toff(0)): rgb, depth and acc bit for bit, at every rays-per-workgroup value of k_march (the group size).
3. Training rows: one forward + backward, toff16, tileinfo and the 19 gradients bit-identical with the two offset paths."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import capture_train_ws, make_field, make_rays, quiet

DEV = "cuda:0"
NB = 256
RS = (1, 3, 4, 5, 255, 256, 257, 1023, 4096, 4099)
GROUPS = (4, 8, 16)
PATTERNS = ("zeros", "one_ray", "one_ray_few_tiles", "small", "few_tiles", "zero_run", "zero_tail")


def counts(pattern, R, seed):
    """Shaded-sample counts per ray (what k_march leaves in ncomp; at most 65535: k_shade3 keeps them as 16-bit)."""
    rng = np.random.RandomState(seed)
    n = np.zeros(R, dtype=np.int32)
    if pattern == "one_ray":                      # all tiles in one ray, more tiles than workgroups
        n[R // 2] = 40000
    elif pattern == "one_ray_few_tiles":          # ... and fewer (T < nb)
        n[R - 1] = 97
    elif pattern == "small":
        n = rng.choice(np.array([0, 1, 31, 32, 33], dtype=np.int32), size=R)
    elif pattern == "few_tiles":                  # T < nb: most workgroups get an empty range
        idx = rng.choice(R, size=min(R, 20), replace=False)
        n[idx] = rng.randint(1, 34, size=idx.size)
    elif pattern == "zero_run":                   # zero-tile runs that straddle the boundaries of groups of 4, 8 and 16
        n = rng.randint(1, 200, size=R).astype(np.int32)
        n[13:19] = 0
        n[max(0, R // 2 - 3):R // 2 + 2] = 0
        if R > 64:
            n[61:83] = 0
    elif pattern == "zero_tail":                  # the last workgroup's range runs over many rays without a tile
        n = rng.randint(0, 70, size=R).astype(np.int32)
        n[R // 3:] = 0
    return n


def numpy_ranges(n, nb):
    R = n.size
    toff = np.concatenate([[0], np.cumsum((n.astype(np.int64) + 31) // 32)])
    T = int(toff[R])
    b = np.arange(nb, dtype=np.int64)
    ra = np.minimum(np.searchsorted(toff, b * T // nb, side="left"), R)
    rb = np.minimum(np.searchsorted(toff, (b + 1) * T // nb, side="left"), R)
    rb[nb - 1] = R
    return toff, ra, rb


@pytest.mark.gpu
@pytest.mark.parametrize("G", GROUPS)
def test_partition_matches_numpy(built_lib, G):
    for R in RS:
        r = np.arange(R + 1)[None, :]
        for pi, pattern in enumerate(PATTERNS):
            n = counts(pattern, R, 1000 * G + 10 * R + pi)
            toff, ra, rb = numpy_ranges(n, NB)
            d_n = torch.from_numpy(n).to(DEV)
            gsum = torch.zeros((R + G - 1) // G, dtype=torch.int32, device=DEV)
            ranges = torch.full((NB, 4), -1, dtype=torch.int32, device=DEV)
            toff_out = torch.full((NB, R + 1), -1, dtype=torch.int32, device=DEV)
            nc_out = torch.full((NB, R), -1, dtype=torch.int32, device=DEV)
            rc = built_lib.lrf_debug_tile_ranges(d_n.data_ptr(), R, G, NB, gsum.data_ptr(), ranges.data_ptr(), toff_out.data_ptr(),
                                                 nc_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            want = np.stack([ra, rb, toff[ra], toff[rb]], 1)
            got = ranges.cpu().numpy()
            assert np.array_equal(got, want), (R, pattern, np.nonzero((got != want).any(1))[0][:4], got[:4], want[:4])
            inside = (r >= ra[:, None]) & (r <= rb[:, None])
            assert np.array_equal(toff_out.cpu().numpy(), np.where(inside, toff[None, :], -1)), (R, pattern)
            inside = (r[:, :R] >= ra[:, None]) & (r[:, :R] < rb[:, None])
            assert np.array_equal(nc_out.cpu().numpy(), np.where(inside, n[None, :], -1)), (R, pattern)


GRID = [48, 48, 48]
N_SAMPLES = 288          # 96 samples per ray


def random_field():
    f = quiet(make_field, GRID, "cpu", seed=5)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(4.0)
    return f.to(DEV)


def walls_field():
    """Nearly empty space between nested box-shaped shells of dense walls, an alpha mask rebuilt from it and early
    termination: rays end behind different numbers of walls, the shaded counts differ widely between rays."""
    f = quiet(make_field, GRID, "cpu", seed=6, density_shift=-9.0)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(0.05)
        for p in range(3):
            L = f.density_line[p].shape[2]
            c = torch.linspace(-2, 2, L)
            for comp, centre in enumerate((0.9, -0.9, 0.45, -0.45, 1.5, -1.5)):
                f.density_plane[p][0, comp].fill_(1.0)
                f.density_line[p][0, comp, :, 0] = 12.0 * torch.exp(-((c - centre) / 0.35) ** 2)
    f = f.to(DEV)
    quiet(f.updateAlphaMask, (40, 44, 36))
    f.early_term_T = 1e-9
    return f


@pytest.fixture(scope="module")
def fields(built_lib):
    return {"random": random_field(), "walls": walls_field()}


@pytest.mark.gpu
@pytest.mark.parametrize("R", (1, 5, 257, 1000))
@pytest.mark.parametrize("name", ("random", "walls"))
def test_two_offset_paths_agree(built_lib, fields, name, R):
    f = fields[name]
    rays = make_rays(R, 40 + R, pinhole=True).to(DEV)
    first = None
    try:
        for march_rays in GROUPS:
            built_lib.lrf_debug_set_march_rays(march_rays)
            out = []
            for lds_toff in (1, 0):
                built_lib.lrf_debug_set_lds_toff(lds_toff)
                with torch.no_grad():
                    rgb, depth, w, acc, _ = f.render_weights(rays, N_samples=N_SAMPLES)
                torch.cuda.synchronize()
                out.append((rgb.clone(), depth.clone(), acc.clone(), int((w > f.rayMarch_weight_thres).sum())))
            a, b = out
            print(name, "R", R, "rays per march workgroup", march_rays, "shaded", a[3])
            assert a[3] > 0
            for x, y, what in zip(a[:3], b[:3], ("rgb", "depth", "acc")):
                assert torch.equal(x, y), (what, march_rays)
            if first is None:
                first = a
            for x, y, what in zip(a[:3], first[:3], ("rgb", "depth", "acc")):      # per-ray results do not depend on the workgroup size
                assert torch.equal(x, y), (what, march_rays, "against 4 rays per workgroup")
    finally:
        built_lib.lrf_debug_set_march_rays(0)
        built_lib.lrf_debug_set_lds_toff(1)
    shaded = (w > f.rayMarch_weight_thres).sum(-1)
    print(name, "R", R, "shaded samples per ray: min", int(shaded.min()), "max", int(shaded.max()))


@pytest.mark.gpu
def test_largest_sample_count(built_lib, fields):
    """S = 4096, the most lrf_render_fwd accepts: no k_march workgroup with the density lines in LDS fits, so k_march<false>
    runs with four alpha slices of 16 KB -- 64 KB of LDS -- and the combine word of the group sums behind them.  Both offset
    paths, bit for bit; weights that sum to acc."""
    f = fields["random"]
    R, N = 5, 6 * 2048
    rays = make_rays(R, 77, pinhole=True).to(DEV)
    out = []
    try:
        for lds_toff in (1, 0):
            built_lib.lrf_debug_set_lds_toff(lds_toff)
            with torch.no_grad():
                rgb, depth, w, acc, z = f.render_weights(rays, N_samples=N)
            torch.cuda.synchronize()
            assert z.numel() == 4096 and tuple(w.shape) == (R, 4096)
            out.append((rgb.clone(), depth.clone(), acc.clone(), w.clone()))
    finally:
        built_lib.lrf_debug_set_lds_toff(1)
    a, b = out
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    assert int((a[3] > f.rayMarch_weight_thres).sum()) > R
    assert float((a[3].sum(-1) - a[2]).abs().max()) < 1e-4             # (4096 fp32 terms of at most 1, summed in another order)
    assert float(a[0].min()) >= 0.0 and float(a[0].max()) <= 1.0 + 1e-5 and float(a[1].min()) > 0.0


def _up256(x):
    return (x + 255) & ~255


@pytest.mark.gpu
def test_training_rows_agree(built_lib):
    """toff16, tileinfo (workspace of lrf_render_fwd_train: tileinfo follows the mask bits, csrc/lrf_backward.inl carve_bwd) and
    every gradient, deterministic backward."""
    from localrf_amd import _native as N
    R, S = 257, 96
    f = random_field()
    f.deterministic = True
    rays = make_rays(R, 91, pinhole=True).to(DEV)
    gen = torch.Generator().manual_seed(3)
    g_rgb, g_depth = torch.randn(R, 3, generator=gen).to(DEV), torch.randn(R, generator=gen).to(DEV)
    z = f.z_schedule(False, N_SAMPLES, torch.device(DEV)).clone()
    assert z.numel() == S
    lay = (C.c_uint64 * 9)()
    N.lib().lrf_workspace_layout_bwd(R, S, (C.c_int32 * 3)(*f.layout.grid), lay)
    toff_off, bits_off = int(lay[3]), int(lay[6])
    tiles_max = R * 2 * ((S + 31) // 32)
    ti_off = bits_off + _up256(tiles_max * 128 * 4)
    res = []
    f.z_override = z
    try:
        for lds_toff in (1, 0):
            built_lib.lrf_debug_set_lds_toff(lds_toff)
            f.zero_grad(set_to_none=True)
            with capture_train_ws(f) as cap:
                rgb, depth = f(rays, white_bg=True, is_train=True, N_samples=N_SAMPLES)
                ((rgb * g_rgb).sum() + (depth * g_depth).sum()).backward()
                torch.cuda.synchronize()
            ws = cap.ws
            toff16 = ws[toff_off:toff_off + 4 * (R + 1)].view(torch.int32).clone()
            tiles = int(toff16[R])
            tileinfo = ws[ti_off:ti_off + 16 * tiles].view(torch.int32).clone()
            grads = {n: p.grad.clone() for n, p in f.named_parameters() if p.grad is not None}
            res.append((toff16, tileinfo, grads, rgb.detach().clone(), depth.detach().clone()))
    finally:
        built_lib.lrf_debug_set_lds_toff(1)
        f.z_override = None
    a, b = res
    assert int(a[0][R]) > 2 * R and len(a[2]) == 19, (int(a[0][R]), len(a[2]))
    assert bool((a[0][1:] >= a[0][:-1]).all())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
