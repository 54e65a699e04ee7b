"""The references of tests/optim_reg_cases.py checked on the CPU: adam_step_ref against torch.optim.Adam in float64,
density_l1_ref and tv_ref against autograd over the reference's expressions in float64, and the condition that the
constructed density-L1 inputs are built to meet.  No GPU."""
import numpy as np
import pytest
import torch

import optim_reg_cases as K


def test_adam_step_ref_is_torch_adam_in_float64():
    """25 steps with lr decay and several magnitudes of gradient.

    With the host scalars kept in double the reference IS torch.optim.Adam: 1e-13 of the tensor's size, double roundoff
    over 25 steps.  Rounding them to float32 as the ABI does moves one step by no more than 3 u |p' - p|: step_size and
    bc2_sqrt move by u each, and the betas and eps given to torch are the rounded ones already."""
    b1, b2, eps = (K.f32(x) for x in (*K.ADAM_BETAS, K.ADAM_EPS))
    r = np.random.default_rng(3)
    p0 = r.standard_normal(301)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=0.02, betas=(b1, b2), eps=eps)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for it in range(25):
        g = r.standard_normal(301) * 10.0 ** (it % 5 - 3)
        pt.grad = torch.from_numpy(g.copy())
        lr = opt.param_groups[0]["lr"]
        step_size, bc2 = K.adam_scalars(lr, b1, b2, it + 1)
        pr, mr, vr, E_p, _, _ = K.adam_step_ref(p, g, m, v, step_size, bc2, b1, b2, eps)
        p1, m1, v1, _, _, _ = K.adam_step_ref(p, g, m, v, step_size, bc2, b1, b2, eps, round_scalars=False)
        assert (np.abs(pr - p1) <= 3 * K.U * np.abs(p1 - p) + 1e-300).all()
        assert np.array_equal(mr, m1) and np.array_equal(vr, v1)
        assert (E_p > 0).all()
        opt.step()
        p, m, v = p1, m1, v1
        st = opt.state[pt]
        for mine, ref in ((p, pt.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            assert (np.abs(mine - ref) <= 1e-13 * np.abs(ref).max()).all(), it
        opt.param_groups[0]["lr"] *= 0.97


def test_adam_bound_is_a_few_roundings_of_the_step():
    """The derived bound is element-wise and tight enough to tell a systematic one-ulp difference.

    It stays below 16 u of max(|p'|, |p' - p|): the ten operations' roundings, those of v halved by the root, those of m
    and d carried by the quotient.  A float32 evaluation of the update in numpy lies inside it.  The same evaluation moved
    by one ulp lies outside it for a large share of the elements."""
    b1, b2 = K.ADAM_BETAS
    p, g, m, v = K.adam_arrays(5000, 1)
    step_size, bc2 = K.adam_scalars(0.02, b1, b2, 7)
    pr, mr, vr, E_p, E_m, E_v = K.adam_step_ref(p, g, m, v, step_size, bc2, b1, b2, K.ADAM_EPS)
    assert (E_p <= 16 * K.U * np.maximum(np.abs(pr), np.abs(pr - p)) + 2 * K.TINY).all()
    F = np.float32
    f1, f2, fe, fs, fb = F(b1), F(b2), F(K.ADAM_EPS), F(step_size), F(bc2)
    m32 = ((g - m).astype(np.float64) * np.float64(F(1) - f1) + m).astype(F)       # fma: the product is exact in double
    t = ((F(1) - f2) * g) * g
    v32 = (v.astype(np.float64) * np.float64(f2) + t).astype(F)
    den = np.sqrt(v32) / fb + fe
    p32 = (-np.float64(fs) * np.float64(m32 / den) + p).astype(F)
    assert (np.abs(m32 - mr) <= E_m).all() and (np.abs(v32 - vr) <= E_v).all() and (np.abs(p32 - pr) <= E_p).all()
    # one ulp more on every element is outside it for a large share of them: a systematic difference cannot hide in a tensor
    off = np.nextafter(p32, F(np.inf))
    assert (np.abs(off - pr) > E_p).mean() > 0.25


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("grid", K.L1_SMALL_GRIDS + ((7, 6, 5),))
def test_density_l1_ref_is_the_reference_expression(grid, relu):
    planes, lines = K.l1_inputs(grid, relu, seed=11)
    val, grads, sums = K.density_l1_ref(planes, lines, K.L1_SHIFT, relu)
    tval, tgrads = K.density_l1_torch(planes, lines, K.L1_SHIFT, relu, torch.float64)
    assert abs(val - tval) <= 1e-13 * abs(tval)
    for g, t, a in zip(grads, tgrads, sums):
        assert g.shape == t.shape == a.shape
        assert K.normalised_error(g, t, a) <= 1e-12
        assert (np.abs(g) <= a * (1 + 1e-12)).all() and a.max() > 0


def test_density_l1_ref_keeps_the_three_flattening_orders():
    """On a non-cubic grid, flattening plane 1 like plane 0 (a swapped order) changes the value: the reference is sensitive to
    what the kernel must reproduce."""
    planes, lines = K.l1_inputs((7, 6, 5), False, seed=2)
    val, _, _ = K.density_l1_ref(planes, lines, K.L1_SHIFT, False)
    feat = K.l1_features(planes, lines)
    P, L = np.float64(planes[1]).reshape(8, -1), np.float64(lines[1]).reshape(8, -1)
    swapped = feat - np.einsum("cq,cr->qr", P, L).reshape(-1) + np.einsum("cq,cr->rq", P, L).reshape(-1)
    sig, _ = K._sigma(swapped, K.L1_SHIFT, False)
    assert abs(np.sqrt(np.maximum(sig, 1e-5)).mean() - val) > 1e-6 * val


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("grid", K.L1_SMALL_GRIDS + (K.L1_LARGE_GRID_256CU,))
def test_constructed_l1_inputs_meet_their_condition(grid, relu):
    """No lattice point with sig in [0.5e-5, 2e-5] (relu: |feat| < 1e-3), each of the three bands holds >= 10 % of the points,
    in float64 on the float32 inputs."""
    assert K.l1_large_grid(256) == K.L1_LARGE_GRID_256CU
    planes, lines = K.l1_inputs(grid, relu, seed=11)
    assert all(a.dtype == np.float32 for a in planes + lines)
    fractions, forbidden = K.l1_bands(planes, lines, K.L1_SHIFT, relu)
    assert forbidden == 0
    assert min(fractions) >= 0.10 and abs(sum(fractions) - 1.0) < 1e-12, fractions


@pytest.mark.parametrize("name", sorted(K.TV_TABLES))
def test_tv_ref_is_the_reference_module(name):
    xs = K.tv_inputs(K.TV_TABLES[name], seed=4)
    val, grads, sums = K.tv_ref(xs, K.TV_WEIGHT)
    tval, tgrads = K.tv_torch(xs, K.TV_WEIGHT, torch.float64)
    assert abs(val - tval) <= 1e-13 * abs(tval)
    for g, t, a in zip(grads, tgrads, sums):
        assert K.normalised_error(g, t, a) <= 1e-12
        assert (np.abs(g) <= a * (1 + 1e-12)).all()
    if name == "single":
        assert val == 0.0 and not grads[0].any() and not sums[0].any()
    else:
        assert val > 0


def test_tv_tables_are_what_they_claim():
    assert len(K.TV_TABLES["sixteen"]) == K.TV_MAX == len(set(K.TV_TABLES["sixteen"]))
    sizes = [int(np.prod(s)) for s in K.TV_TABLES["blocks"]]
    assert sizes[2] == 3 * 4096 and sizes[3] % 4096 and (37 * 41) % 4096 and 4096 % 41      # whole blocks; mid-channel, mid-row ends
    assert K.tv_scales(5) == [1e-2, 1e-2, 1e-2, 1e-3, 1e-3]
