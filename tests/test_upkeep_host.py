"""The cases of tests/upkeep_cases.py checked on the CPU, from the references alone: the recorded table E32 against a fresh
measurement; the conditions tests/test_gpu_upkeep.py relies on (no tolerance at its cap, at most 2 % undecidable mask cells and
10 % decided on either side, at most 0.2 % undecidable `inside` flags with decided ones on both sides, no decidable cell or flag
flipped by the float32 evaluation); the edges every case is there to hold; the float64 references against what the reference
recorded (upsample_grid, alpha_mask_rebuild, sample_ray).  No GPU."""
import numpy as np
import pytest
import torch

import upkeep_cases as K
from losses_cases import _not_stale
from oracle import vm_render_np as onp
from oracle import vm_render_torch as ot
from util import field_from_seed, load_golden


@pytest.mark.parametrize("family,name", [(f, n) for f, (names, _) in K.CHECKS.items() for n in names])
def test_case_meets_its_conditions_and_E32_is_current(family, name):
    bad, e32 = K.CHECKS[family][1](name)
    assert not bad, bad
    _not_stale(K.E32[f"{family}:{name}"], e32, f"{family}:{name}")


def test_every_case_has_a_row_and_a_seed():
    assert set(K.E32) == {f"{f}:{n}" for f, (names, _) in K.CHECKS.items() for n in names}
    assert set(K.MASK_CASES) | set(K.RAY_CASES) <= set(K.SEEDS)
    assert set(K.UP_AMP) <= set(K.UP_CASES)


def test_tolerance_rule():
    """The three regimes: the floor, 4 e32, the cap of the quantity; dense alpha has no cap."""
    assert K.tolerance(0.0, "up") == K.tolerance(1e-8, "alpha") == K.FLOOR == 8 * 2.0 ** -24
    assert K.tolerance(2e-7, "up") == K.tolerance(2e-7, "sig") == K.tolerance(2e-7, "alpha") == 8e-7
    assert K.tolerance(1.0, "up") == 1e-6 and K.tolerance(1.0, "alpha") == 4.0
    for q in ("sig", "app", "t", "pts", "xc"):
        assert K.tolerance(1.0, q) == 2e-6


# ------------------------------------------------------------------------------------------------------------------ upsample
def test_upsample_cases_hold_their_edges():
    n = {name: K.UP_SHAPES[i][0] * K.UP_SHAPES[i][3] * K.UP_SHAPES[i][4] for i, name in enumerate(K.UP_CASES)}
    assert sorted(n[k] for k in ("3x4x6-5x17", "4x5x3-8x8", "1x9x1-257x1")) == [255, 256, 257]
    assert n[K.UP_BIG] == 67415424 > K.LAUNCH_CAP == 67107840 and K.up_case(K.UP_BIG)[3][-1] == n[K.UP_BIG] - 1
    assert (K.up_case(K.UP_BIG)[3] >= K.LAUNCH_CAP).sum() > 4096         # elements only the second trip of the stride loop writes
    src, H2, W2, idx = K.up_case(K.UP_IDENTITY)
    assert (H2, W2) == src.shape[1:] and np.array_equal(K.up_ref(K.UP_IDENTITY).reshape(src.shape), src.astype(np.float64))
    src, H2, W2, _ = K.up_case("8x6x5-1x1")                              # one output: the first texel, as ATen takes it
    assert np.array_equal(K.up_ref("8x6x5-1x1"), src[:, 0, 0].astype(np.float64))
    src, H2, W2, _ = K.up_case("8x1x6-5x6")                              # H = 1 and W2 = W: every row is the source row
    assert np.array_equal(K.up_ref("8x1x6-5x6").reshape(8, 5, 6), np.repeat(src.astype(np.float64), 5, 1))
    src, H2, W2, _ = K.up_case("8x2x2-257x3")                            # in = 2: corners kept, the middle column their mean
    r = K.up_ref("8x2x2-257x3").reshape(8, 257, 3)
    assert np.array_equal(r[:, [0, 256]][:, :, [0, 2]], src.astype(np.float64)) and np.allclose(r[:, 0, 1], src[:, 0].mean(-1), atol=1e-12)
    for name in K.UP_CASES[:-1]:                                          # the float64 formula against ATen's own in float64
        src, H2, W2, idx = K.up_case(name)
        want = torch.nn.functional.interpolate(torch.from_numpy(src).double()[None], size=(H2, W2), mode="bilinear", align_corners=True)
        assert np.abs(want[0].numpy().reshape(-1) - K.up_ref(name)).max() <= 1e-15, name


def test_float64_resize_reproduces_the_recorded_upsample():
    """tests/golden/upsample_grid.npz: the twelve tensors the reference's upsample_volume_grid left, within the 1e-6 the suite
    holds the kernel to against the same file."""
    g = load_golden("upsample_grid")
    f = field_from_seed(g)
    tgt, n = [int(v) for v in g["target"]], 0
    for k, v in f.state_dict().items():
        if "plane" in k or "line" in k:
            want = g["up." + k]
            got = K.resize64_at(v.numpy()[0], want.shape[2], want.shape[3], np.arange(want[0].size)).reshape(want.shape)
            assert np.abs(got - want).max() <= 1e-6, k
            n += 1
    assert n == 12 and len(tgt) == 3


def test_upfield_reference():
    f = K.upfield_field()
    ref, step, ns = K.upfield_ref(f)
    assert len(ref) == 12 and ref["density_plane.0"].shape == (1, 8, 8, 12) and ref["app_line.0"].shape == (1, 24, 10, 1)
    up = ot.upsample_vm({k: v.detach() for k, v in f.state_dict().items()}, K.UPFIELD[1])
    for k, v in ref.items():
        assert np.abs(up[k].numpy() - v).max() <= K.tolerance(K.E32["upfield:5x7x9-12x8x10"]["up"], "up"), k


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("lat", K.POOL_LATTICES, ids=lambda l: "x".join(map(str, l)))
def test_pool_reference_and_its_inputs(lat):
    """The numpy max-pool against F.max_pool3d on the same floats, and against what each crafted input is there to decide."""
    seen = {}
    for name, alpha, thres, expect in K.pool_inputs(lat):
        got = K.pool_ref(alpha, thres)
        a = torch.from_numpy(alpha).clamp(0, 1)[None, None]
        want = (torch.nn.functional.max_pool3d(a, kernel_size=3, padding=1, stride=1)[0, 0] >= float(thres)).float().numpy()
        assert np.array_equal(got, want), name
        if expect is not None:
            assert np.array_equal(got, expect), name
        seen[name] = got
    assert alpha.shape == lat[::-1]
    assert seen["thres-at"].sum() == seen["thres-above"].sum() >= 1 and seen["thres-below"].sum() == 0
    if min(lat) >= 3:                                       # a swapped axis moves a corner's block
        assert len({seen[f"corner-{k}"].tobytes() for k in range(8)}) == 8 and seen["corner-0"].sum() == 8
    if np.prod(lat) >= 255:
        assert 0.02 < seen["random"].mean() < 0.98


# ------------------------------------------------------------------------------------------------------------------ mask
@pytest.mark.parametrize("name", list(K.MASK_CASES))
def test_mask_case_figures(name):
    bad, e32, fig = K.mask_check(name)
    print(f"[mask:{name}] e32 {e32['alpha']:.2e}  kept {fig['kept']:.3f}  undecidable cells {fig['undecidable']} of {fig['cells']}  "
          f"points of undecided validity {fig['undecided_validity']}  cells float32 flips {fig['flips32']}")
    assert not bad, bad
    grid, _, _, lat, prev, act = K.MASK_CASES[name]
    ref = K.mask_ref(name)
    assert ref["alpha"].shape == lat[::-1] and (prev is None) == bool(ref["valid"].all())
    if prev is not None:
        assert (~ref["valid"]).mean() > 0.01 and (ref["free"][~ref["valid"]] > 1e-5).sum() > 10   # zeroed points a kernel that ignored the mask would miss by 20 tolerances
        assert not (ref["sure_valid"] & ~ref["valid"]).any() and not (ref["sure_invalid"] & ref["valid"]).any()
    if name == K.COINCIDENT:
        assert fig["undecided_validity"] > 50                # the case sits on the old mask's lattice planes
    elif prev is not None:
        assert len(set(lat)) == 3 and len(set(prev)) == 3 and all((a - 1) % (b - 1) for a, b in zip(lat, prev))


def test_coincident_lattice_against_the_float32_aten_evaluation():
    """Every difference between oracle.vm_render_torch.update_alpha_mask (float32, ATen) and the float64 mask falls on an
    undecidable cell; the same for the non-coincident rebuilds, where there is none."""
    for name in (K.COINCIDENT, "A/rebuild", "A/20x18x22"):
        f = K.mask_field(name)
        fld = dict(f.state_dict())
        prev = K.mask_prev(name)
        if prev is not None:
            fld["alphaMask.alpha_volume"] = torch.from_numpy(prev[0])[None, None]
            fld["alphaMask.aabb"] = torch.from_numpy(prev[1])
        with K.one_thread():
            aten = ot.update_alpha_mask(fld, K.MASK_CASES[name][3], float(f.stepSize), float(K.THRES), float(f.density_shift)).numpy()
        m64, keep, drop = K.mask_sets(K.mask_ref(name), K.tolerance(K.E32[f"mask:{name}"]["alpha"], "alpha"))
        diff = aten != m64
        print(f"[mask:{name}] float32 ATen differs from float64 on {int(diff.sum())} cells, {int((diff & (keep | drop)).sum())} of them decidable")
        assert not (diff & (keep | drop)).any(), name


def test_float64_mask_reproduces_the_recorded_rebuild():
    """tests/golden/alpha_mask_rebuild.npz: the reference's two binary volumes (a 20x18x22 lattice, then 30x27x33 through the
    first) agree with the float64 reference on every decidable cell."""
    g = load_golden("alpha_mask_rebuild")
    f = field_from_seed(g)
    prev = None
    for k in ("1", "2"):
        lat = tuple(int(v) for v in g["g" + k])
        want = np.unpackbits(g["m" + k])[:int(np.prod(g[f"m{k}_shape"]))].reshape(g[f"m{k}_shape"])
        ref, r32 = K.mask_eval(f, lat, np.float64, prev), K.mask_eval(f, lat, np.float32, prev)
        m64, keep, drop = K.mask_sets(ref, K.tolerance(K.alpha_err(r32["alpha"], ref), "alpha"))
        assert want.shape == m64.shape and (keep | drop).mean() > 0.97
        assert np.array_equal(want[keep | drop], m64[keep | drop]), k
        prev = (want.astype(np.float32), f.aabb.detach().numpy())


def test_render_through_the_rebuilt_mask_is_well_conditioned():
    """The 64 rays of the GPU test's render through the float64 mask of RENDER_CASE: the float32 oracle meets the bars of
    test_gpu_parity._check_rays against float64, and the mask blocks samples that carry weight without it."""
    f = K.mask_field(K.RENDER_CASE)
    m64 = K.mask_sets(K.mask_ref(K.RENDER_CASE), K.FLOOR)[0]
    rgb, depth, ex = K.render_ref(f, m64)
    r32, d32, _ = K.render_ref(f, m64, np.float32)
    for got, ref in ((r32, rgb), (d32, depth)):
        assert (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)).max() <= 1e-4
    free = K.render_ref(f, np.ones_like(m64))
    assert np.abs(free[0] - rgb).max() > 1e-3 and 0.05 < ex["acc"].mean()                  # ten times the bar: the mask matters


# ------------------------------------------------------------------------------------------------------------------ features
def test_feature_coordinates_hold_their_edges():
    assert K.FEAT_GRIDS[-1] == (1, 1, 1)
    one = np.float32(1)
    for grid in K.FEAT_GRIDS:
        u = K.feat_coords(grid)
        assert u.shape == (257, 3) and u.dtype == np.float32
        combos = {tuple(p) for p in u[:27].tolist()}
        assert combos == {(a, b, c) for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0) for c in (-1.0, 0.0, 1.0)}
        for a in range(3):
            for v in (-1.5, 1.5, float(np.nextafter(one, np.float32(0))), float(np.nextafter(-one, np.float32(0)))):
                assert (u[:, a] == np.float32(v)).any(), (grid, a, v)
            ix = (u[:, a].astype(np.float64) + 1) / 2 * (grid[a] - 1)
            centres = {int(round(i)) for i in ix[np.abs(ix - np.round(ix)) < 1e-5]}
            assert centres >= set(range(grid[a])), (grid, a)
    r = K.feat_ref("5x7x9/P257")
    f = K.feat_field((5, 7, 9))
    sig15 = K.feat_run(f, np.clip(K.feat_coords((5, 7, 9)), -1, 1), np.float64)["sig"]
    assert np.array_equal(r["sig"], sig15)                  # the border clamp: +-1.5 reads what +-1 reads
    assert 0.05 < np.abs(r["sig"]).max() < 5 and r["app"].shape == (257, 27)


# ------------------------------------------------------------------------------------------------------------------ rays
@pytest.mark.parametrize("shape", [f"{r}x{n}" for r, n in K.RAY_SHAPES])
def test_ray_cases_decide_flags_on_both_sides(shape):
    ins = out = 0
    for mode in ("eval", "jit"):
        bad, e32, fig = K.ray_check(f"{shape}/{mode}")
        print(f"[ray:{shape}/{mode}] undecidable flags {fig['undecidable']} of {fig['flags']}, decided inside {fig['inside']}, outside {fig['outside']}")
        assert not bad, bad
        ins, out = ins + fig["inside"], out + fig["outside"]
    assert ins > 0 and out > 0


def test_ray_cases_hold_their_edges():
    rays, N, jit = K.ray_case("64x50/eval")
    d, o = rays[:, 3:], rays[:, :3]
    for a in range(3):
        assert ((d[:, a] == 0) & (np.abs(d).min(-1) == 0) & ((d == 0).sum(-1) == 1)).any(), a
    assert ((d == 0).sum(-1) == 2).any() and (d < 0).all(-1).any() and (np.abs(o) > 2).any(-1).any() and jit is None
    t = K.ray_ref("64x50/eval")["t"]
    assert (t[:, 0] == np.float64(np.float32(1e3))).any() and (t[:, 0] == 0.1).any()                             # far and near clamps
    assert ((t[:, 0] > 0.2) & (t[:, 0] < 999)).any()                                                            # and neither
    assert ((t[:, 0] > 499.9) & (t[:, 0] < 500.1)).any()             # a zero component 5e-4 outside its slab: 5e-4 / 1e-6
    ref = K.ray_ref("64x50/eval")
    miss = ~ref["inside"].any(-1)
    assert miss.sum() >= 10 and (ref["inside"].any(-1) & ~ref["inside"].all(-1)).sum() >= 10         # rays that miss, rays that leave
    assert K.ray_case("64x50/jit")[2].shape == (64,) and abs(K.STEP - 0.5 * 4 / 31) < 1e-8
    assert [r * n for r, n in K.RAY_SHAPES] == [1, 255, 256, 255, 257, 3200]


def test_contracted_cases_hold_their_edges():
    one = np.float32(1)
    o, d, z = K.con_case("64x50")
    m = np.abs(o[:3]).max(-1)
    assert not d[:3].any() and m[0] == np.nextafter(one, np.float32(2)) and m[1] == one and m[2] < 1e-6
    x = K.con_ref("64x50")["xc"]
    assert np.array_equal(x[1, 0], o[1].astype(np.float64)) and np.array_equal(x[2, 0], o[2].astype(np.float64))      # not contracted
    assert 0 < np.float64(o[0, 0]) - x[0, 0, 0] < 1e-13                                        # (2m - 1) / m^2 = 1 - ulp^2
    assert z[-1] == np.float32(1000.1) and (np.diff(z) > 0).all() and np.abs(x[:, -1]).max() > 1.99
    assert np.abs(x).max() < 2 and K.con_case("1x1")[0][0, 0] == np.nextafter(one, np.float32(2))


def test_float64_sample_ray_reproduces_the_recorded_rays():
    """tests/golden/sample_ray.npz (eval, and train with the recorded jitter): t and pts within the float32 error, every
    decidable flag equal; the flags that differ from the reference's are counted."""
    g = load_golden("sample_ray")
    assert np.array_equal(g["aabb"], K.AABB) and abs(float(g["stepSize"]) - K.STEP) < 1e-9
    r = g["rays"].astype(np.float64)
    nf = [float(v) for v in g["near_far"]]
    for jit, sfx in ((None, ""), (g["U"], "_j")):
        pts, t, inside = onp.sample_ray_aabb(r[:, :3], r[:, 3:], K.AABB.astype(np.float64), float(g["stepSize"]), int(g["N_samples"]), nf,
                                             None if jit is None else jit.astype(np.float64))
        p32, t32, _ = onp.sample_ray_aabb(g["rays"][:, :3], g["rays"][:, 3:], K.AABB, float(g["stepSize"]), int(g["N_samples"]), nf, jit)
        e_t, e_p = K.rel1_err(t32, t), K.rel1_err(p32, pts)
        assert K.rel1_err(g["t" + sfx], t) <= K.tolerance(e_t, "t") and K.rel1_err(g["pts" + sfx], pts) <= K.tolerance(e_p, "pts")
        ins, out = K.flag_sets(pts, K.tolerance(e_p, "pts"))
        dec = ins | out
        print(f"[golden sample_ray{sfx}] undecidable {int((~dec).sum())} of {dec.size}, the recorded flags differ from float64 on "
              f"{int((g['inside' + sfx] != inside).sum())}")
        assert np.array_equal(g["inside" + sfx][dec], inside[dec]) and (~dec).mean() <= 0.02
