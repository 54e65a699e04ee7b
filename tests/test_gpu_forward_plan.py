"""The forward render on both sides of every branch of its launch plan (csrc/lrf_forward.inl: plan_march, plan_shade3,
pipe_chunks), bit for bit against the commit before the plan existed.

tests/golden/forward_plan_parent.json holds util.tensor_digest of every output, recorded on the MI355X from that commit's
library by tests/golden/make_golden_forward_plan.py (which renders each case twice and refuses one whose runs differ: the
forward has no atomics, and the deterministic backward is bit-reproducible by its own tests).  The sample counts are where
the plan of a 48^3 grid flips (tests/test_forward_plan_host.py pins the same numbers by name): z leaves LDS at S = 1766 | 1767,
4 -> 8 rays per march workgroup at 2208 | 2209, 8 -> 16 at 2352 | 2353, the lines leave LDS at 2424 | 2425, z leaves again at
3276 | 3277; 96^3: 4 -> 8 rays at 1920 | 1921.  S is even (two halves of N_samples // 6), so the far side is S + 2.  The ray
counts, at S = 64: 11399 | 11400, where the colour kernel's tile offsets leave LDS (image + z + 6 R + 84 bytes against 160 KB -
256); 16384 | 16388, 4096 | 4097 groups of 4 rays, the other bound on those offsets (the LDS bound comes first at every S, so
both sides run behind k_scan_tiles_n); 32764 | 32768, one pass against two chunks over two streams."""
import json
import os

import pytest
import torch

from test_forward_fixed_cost import random_field, walls_field
from util import make_field, make_rays, quiet, tensor_digest

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_plan_parent.json")

S_EDGES = (1766, 1768, 2208, 2210, 2352, 2354, 2424, 2426, 3276, 3278)
R_EDGES = (11399, 11400, 16384, 16388, 32764, 32768)
FIELDS = ("random", "walls")

# (kind, field, R, S)
CASES = ([("weights", f, R, S) for f in FIELDS for R in (5, 33) for S in S_EDGES]
         + [("weights", f, R, 64) for f in FIELDS for R in R_EDGES]
         + [(kind, f, 5, S) for kind in ("normals", "quantiles") for f in FIELDS for S in (1766, 1768)]
         + [("train", f, R, S) for f in FIELDS for R in (5, 17) for S in (1766, 1768)]
         + [("train", "random96", R, S) for R in (5, 17) for S in (1920, 1922)])


def case_id(case):
    return "-".join(str(x) for x in case)


def random_field_96():
    f = quiet(make_field, [96, 96, 96], "cpu", seed=5)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(4.0)
    return f.to(DEV)


def make_fields():
    return {"random": random_field(), "walls": walls_field(), "random96": random_field_96()}


def _train(f, rays, N_samples, drop_workspace):
    """rgb, depth of the taped forward and every gradient of a deterministic backward; drop_workspace: the backward is not
    handed the forward's saved rows, so lrf_render_bwd runs the forward once more itself."""
    f.zero_grad(set_to_none=True)
    rays = rays.clone().requires_grad_(True)
    if drop_workspace:
        orig = f._native_backward
        f._native_backward = lambda *a, saved_ws=None: orig(*a, saved_ws=None)
    try:
        rgb, depth = f(rays, white_bg=True, is_train=True, N_samples=N_samples)
        gen = torch.Generator().manual_seed(3)
        g_rgb, g_depth = torch.randn(rgb.shape, generator=gen).to(DEV), torch.randn(depth.shape, generator=gen).to(DEV)
        ((rgb * g_rgb).sum() + (depth * g_depth).sum()).backward()
        torch.cuda.synchronize()
    finally:
        if drop_workspace:
            del f._native_backward
    out = {"rgb": rgb, "depth": depth, "g_rays": rays.grad}
    grads = {n: p.grad for n, p in f.named_parameters() if p.grad is not None}
    assert len(grads) == 19, sorted(grads)
    out.update({"g." + n: g for n, g in grads.items()})
    return out


def run_case(fields, case):
    """{output name: tensor_digest} of one case."""
    kind, name, R, S = case
    f = fields[name]
    N_samples = 3 * S
    rays = make_rays(R, 40 + R, pinhole=True).to(DEV)
    if kind == "train":
        f.deterministic = True
        f.z_override = f.z_schedule(False, N_samples, torch.device(DEV)).clone()
        try:
            assert f.z_override.numel() == S
            saved = _train(f, rays, N_samples, False)
            rerun = _train(f, rays, N_samples, True)
        finally:
            f.z_override = None
            f.deterministic = None
            f.zero_grad(set_to_none=True)
        out = {"saved." + k: v for k, v in saved.items()}
        out.update({"rerun." + k: v for k, v in rerun.items()})
    else:
        with torch.no_grad():
            if kind == "weights":
                rgb, depth, w, acc, z = f.render_weights(rays, N_samples=N_samples)
                out = {"rgb": rgb, "depth": depth, "acc": acc, "weights": w}
            elif kind == "normals":
                normals, acc = f.render_normals(rays, N_samples=N_samples)
                z = f.z_schedule(False, N_samples, rays.device)
                out = {"normals": normals, "acc": acc}
            else:
                depth, acc, index = f.render_depth_quantiles(rays, q=(0.25, 0.5, 0.9), N_samples=N_samples, return_index=True)
                z = f.z_schedule(False, N_samples, rays.device)
                out = {"depth": depth, "acc": acc, "index": index}
        torch.cuda.synchronize()
        assert z.numel() == S
    return {k: tensor_digest(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fields(built_lib):
    return make_fields()


def test_every_case_is_recorded(golden):
    assert set(golden) == {case_id(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_outputs_are_the_parents(built_lib, fields, golden, case):
    want = golden[case_id(case)]
    got = run_case(fields, case)
    assert set(got) == set(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong
