"""The cases of tests/losses_cases.py checked on the CPU: each case's float64 reference against the same chain in float32, the
conditions tests/test_gpu_losses.py relies on (zero clip flips, a clip margin, a unique median, tolerances under the caps) and
the recorded table E32 against a fresh measurement.  No GPU."""
import numpy as np
import pytest
import torch

import losses_cases as K
from losses_cases import _not_stale
from oracle import vm_render_torch as ot


@pytest.mark.parametrize("name", K.GEO_CASES)
def test_geometric_case_meets_the_conditions_and_E32_is_current(name):
    """K.geo_check: the case holds what it is there for; in every view no entry of the float64 arrays lies within 16 d32 of the
    threshold; the float32 chain clips exactly the entries the float64 chain clips; the median of 1 / clamp(depth) is unique
    and the same element in both precisions; 4 e32 stays under the cap for every quantity in both forms.  Then E32 against
    what was just measured."""
    bad, e32 = K.geo_check(name)
    assert not bad, bad
    for form in K.FORMS:
        _not_stale(K.E32[f"{name}/{form}"], e32[form], f"{name}/{form}")


def test_a_seed_with_a_near_tie_or_a_cancellation_is_refused():
    """Seeds the search passed over, for the reasons it passed them over: pow2_edges-3 seed 1 (two depth-loss entries within
    2e-6 of the threshold: the float32 chain clips another entry), pow2_edges-4096 seed 1 (a ray reprojected almost into the
    neighbour's image plane: its float32 error of 9 px is the view's d32), depth_edges seed 6 (a gradient of the turned view
    lost to cancellation: 4 e32 = 4.7e-4), pow2_edges-4095 seed 1 (the recorded float32 error of the depth gradient is a lucky one:
    with the rays in another order the same chain errs by more than half the tolerance it would give)."""
    for name, seed, what in (("pow2_edges-3", 1, "clip flips"), ("pow2_edges-4096", 1, "within 16 d32"), ("depth_edges", 6, "over the cap"),
                             ("pow2_edges-4095", 1, "another order")):
        bad, _ = K.geo_check(name, seed)
        assert any(what in b for b in bad), (name, seed, bad)


def test_the_forward_mask_rule_is_the_absolute_id_rule():
    """pow2_edges, dup_views: a non-last frame whose absolute id is F - 1 loses its forward term, the last frame (absolute id
    F - 1 + start) keeps its own -- against its clamped neighbour, itself.  "The last frame" would give other arrays."""
    for name in ("pow2_edges-65", "dup_views"):
        c = K.geo_case(name)
        assert c["start"] > 0
        raw = K.geo_raw(c, torch.float64)["flow"][0]
        off = dict(c, fwd_mask=torch.zeros_like(c["fwd_mask"]))
        only_bwd = K.geo_raw(off, torch.float64)["flow"][0]
        for v, fr in enumerate(c["frames"].tolist()):
            if fr + c["start"] == c["F"] - 1:
                assert fr != c["F"] - 1 and np.array_equal(raw[v], only_bwd[v])
            else:
                assert not np.array_equal(raw[v], only_bwd[v])
        assert c["F"] - 1 in c["frames"].tolist() and c["F"] - 1 - c["start"] in c["frames"].tolist()


def test_single_ray_depth_reference_is_not_a_number():
    c = K.geo_case("single_ray")
    val, arr = ot.depth_loss(c["depth"].double(), c["invdepths"].double())
    assert torch.isnan(val) and torch.isnan(arr).all()
    assert "depth" not in K.geo_ref("single_ray", "mean") and np.isfinite(K.geo_ref("single_ray", "mean")["flow_g_c2w"]).all()


def test_one_frame_depth_gradient_is_normalised_by_the_terms_that_cancel():
    """In float64 the gradient is a few roundings of the terms' size, not zero: the normalised form measures those roundings,
    max|x| would not."""
    c, ref = K.geo_case("one_frame"), K.geo_ref("one_frame", "mean")
    scale = K.one_frame_scale(c, ref)
    kept = ref["flow_arr"] != 0
    assert (scale[kept] > 0).all() and (scale[~kept] == 0).all() and (ref["flow_g_depth"][~kept] == 0).all()
    assert np.abs(ref["flow_g_depth"][kept] / scale[kept]).max() <= 16 * 2.0 ** -53
    assert K.geo_err(c, "flow_g_depth", ref["flow_g_depth"], ref) == 0.0
    moved = ref["flow_g_depth"].copy()
    moved[~kept] = 1e-30
    assert K.geo_err(c, "flow_g_depth", moved, ref) == float("inf")


def test_the_other_cases_E32_is_current_and_under_the_caps():
    measured = K.other_e32()
    for key, e in measured.items():
        _not_stale(K.E32[key], e, key)
        for q, v in e.items():
            assert 4 * v <= K.cap_of(q), (key, q, v)
    assert set(K.E32) == set(measured) | {f"{n}/{f}" for n in K.GEO_CASES for f in K.FORMS}


def test_tolerance_rule():
    assert K.tolerance(0.0, "flow") == K.FLOOR == 8 * 2.0 ** -24
    assert K.tolerance(1e-6, "flow_arr") == 4e-6 and K.tolerance(1e-6, "flow_g_c2w") == 4e-6
    assert K.tolerance(1.0, "flow") == K.tolerance(1.0, "total") == 1e-5 and K.tolerance(1.0, "photo_g_rgb") == 2e-6
    assert K.tolerance(1.0, "depth_g_depth") == K.tolerance(1.0, "rows_g_src") == K.tolerance(1.0, "combine_g") == 1e-4


def test_gather_and_rows_cases_hold_their_edges():
    for shape in K.GATHER_SHAPES:
        g = K.gather_case(shape)
        assert (g["views"] < 0).any() and int(g["pix"].min()) == 0 and int(g["pix"].max()) == g["HW"] - 1
        assert int(g["views"].min()) >= -g["n_images"] and int(g["views"].max()) < g["n_images"]
    assert K.GATHER_SHAPES[0][0] * K.GATHER_SHAPES[0][1] > 256                       # more than one block of k_batch_gather
    r = K.rows_case()
    named = (r["idx"] % r["F"]).tolist()
    assert r["unnamed"] not in named and (r["idx"] < 0).any() and named.count(5) >= 3 and r["V"] * r["K"] > 256 and r["F"] * r["K"] > 256
    assert (K.rows_run(r, torch.float64)["rows_g_src"][r["unnamed"]] == 0).all()
