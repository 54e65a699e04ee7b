"""The forward's launch plan (csrc/lrf_forward.inl: plan_march, plan_shade3, pipe_chunks) through lrf_debug_forward_plan, and the
host side that moved with it.  No GPU: the plan is arithmetic, a size is arithmetic, and every recorded refusal comes before
the library's first HIP call.

1. The plan equals the restatement of the previous commit's launch code (forward_plan_cases.restate) for every sample count,
   over grids, ray counts and every combination of the switches.
2. Each threshold of the plan, by name, on both sides, at 48^3 (and the first one of 96^3).
3. Workspace sizes and refusals equal the values recorded from the previous commit (tests/golden/forward_plan_host_parent.json,
   written by tests/golden/make_golden_forward_plan_host.py); the refusals include lrf_scene_fwd's fuse decision, one
   condition at a time."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import forward_plan_cases as F
from localrf_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_plan_host_parent.json")

GRIDS = [(g, g, g) for g in (32, 48, 64, 96, 128, 300, 500, 640, 900, 1000)] + [(48, 64, 96), (300, 200, 640), (1000, 31, 7)]
RS = (1, 4, 5, 11399, 11400, 16383, 16384, 16385, 32767, 32768, 65536, 65537)
SWITCHES = list(itertools.product((True, False), (True, False), (0, 4, 8, 16)))     # lines, toff, forced march rays
G48, G96 = (48, 48, 48), (96, 96, 96)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_plan_is_the_restated_rules(grid):
    lib = N.lib()
    S = np.arange(2, 4097)
    seen = set()
    for R in RS:
        for lines, toff, rays in SWITCHES:
            got = F.plan_sweep(lib, grid, R, F.switches(lines, toff, rays))
            want = F.restate(grid, R, S, lines, toff, rays)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, (grid, R, lines, toff, rays, int(S[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())
            # every LDS size within what lds_opt_in asks for its kernel
            assert (got[:, 5] <= got[:, 10]).all() and (got[:, 7] <= got[:, 11]).all(), (grid, R, lines, toff, rays)
            seen.update(map(tuple, np.unique(got[:, [0, 2, 6]], axis=0).tolist()))
    assert {(0, 0, 0), (0, 1, 1)} <= seen                       # (lines off reaches both z forms at every grid)


def test_switches_below_zero_read_the_hooks():
    lib = N.lib()
    try:
        for lines, toff, rays in SWITCHES:
            lib.lrf_debug_set_lds_lines(int(lines))
            lib.lrf_debug_set_lds_toff(int(toff))
            lib.lrf_debug_set_march_rays(rays)
            for R, S in ((5, 64), (16385, 64), (33, 2300), (40000, 3000)):
                assert F.plan(lib, G48, R, S, -1) == F.plan(lib, G48, R, S, F.switches(lines, toff, rays)), (lines, toff, rays, R, S)
        lib.lrf_debug_set_pipe_chunk(100)
        assert [F.plan(lib, G48, R, 64, -1)["pipe_chunks"] for R in (199, 200, 201, 1000)] == [1, 2, 3, 10]
        lib.lrf_debug_set_pipe_chunk(0)
        assert F.plan(lib, G48, 1 << 20, 64, -1)["pipe_chunks"] == 1
    finally:
        lib.lrf_debug_set_lds_lines(1)
        lib.lrf_debug_set_lds_toff(1)
        lib.lrf_debug_set_march_rays(0)
        lib.lrf_debug_set_pipe_chunk(16384)


def test_bad_arguments():
    lib = N.lib()
    out = (C.c_int64 * 12)()
    ll = (C.c_int32 * 3)(48, 48, 48)
    assert lib.lrf_debug_forward_plan(ll, 5, 64, 3, out) == 0
    for R, S, sw in ((0, 64, 3), (5, 1, 3), (5, 4097, 3), (5, 64, 3 | (5 << 2)), (5, 64, 3 | (32 << 2))):
        assert lib.lrf_debug_forward_plan(ll, R, S, sw, out) == -1, (R, S, sw)
    assert lib.lrf_debug_forward_plan((C.c_int32 * 3)(48, 0, 48), 5, 64, 3, out) == -1
    assert lib.lrf_debug_forward_plan(None, 5, 64, 3, out) == -1 and lib.lrf_debug_forward_plan(ll, 5, 64, 3, None) == -1


# (grid, S below, S above, the fields that flip: name -> (below, above)); lds_l = 144 * 32 = 4608 B at 48^3, 9216 B at 96^3
THRESHOLDS = [
    ("z leaves LDS: (5 S 4 + 4608) 4 <= 159744", G48, 1766, 1767, dict(zlds=(1, 0), nw=(4, 4))),
    ("4 -> 8 rays: (4 S 4 + 4608) 4 <= 159744", G48, 2208, 2209, dict(nw=(4, 8), group=(4, 8), march_block=(256, 512), zlds=(0, 0))),
    ("8 -> 16 rays: (8 S 4 + 4608) 2 <= 159744", G48, 2352, 2353, dict(nw=(8, 16), group=(8, 16), march_block=(512, 1024), zlds=(0, 0))),
    ("lines leave LDS, z returns: 16 S 4 + 4608 <= 159744", G48, 2424, 2425,
     dict(nw=(16, 0), group=(16, 4), march_block=(1024, 256), zlds=(0, 1), march_opt_in=(160 * 1024, 64 * 1024 + 16))),
    ("z leaves again: 5 S 4 <= 65536", G48, 3276, 3277, dict(nw=(0, 0), zlds=(1, 0))),
    ("96^3, 4 -> 8 rays: (4 S 4 + 9216) 4 <= 159744", G96, 1920, 1921, dict(nw=(4, 8), group=(4, 8), zlds=(0, 1))),
]


@pytest.mark.parametrize("what, grid, lo, hi, flips", THRESHOLDS, ids=[t[0].split(":")[0] for t in THRESHOLDS])
def test_named_thresholds_of_the_march(what, grid, lo, hi, flips):
    lib = N.lib()
    for R in (5, 33):
        a, b = F.plan(lib, grid, R, lo, F.switches()), F.plan(lib, grid, R, hi, F.switches())
        for name, (below, above) in flips.items():
            assert (a[name], b[name]) == (below, above), (what, name, a, b)
        for p, S in ((a, lo), (b, hi)):
            lds_l = sum(grid) * 32
            assert p["march_lds"] == p["group"] * S * 4 + (lds_l if p["nw"] else 0) + (S * 4 if p["zlds"] else 0) + 16
            assert p["march_grid"] == -(-R // p["group"]) and p["march_lds"] <= p["march_opt_in"]
        assert a == dict(zip(F.NAMES, F.restate(grid, R, lo).tolist())) and b == dict(zip(F.NAMES, F.restate(grid, R, hi).tolist()))


def test_named_thresholds_of_the_colour_kernel():
    lib = N.lib()
    image = 5928 * 16
    # The LDS bound, image + z + 6 R + 20 + 64 <= 160 KB - 256, is the one that flips the plan at every group size: 11399 | 11400
    # rays at S = 64.  The other bound, 512 threads x 8 group sums (16384 rays for a group of 4), lies beyond it for every S.
    for rays, S in ((0, 64), (4, 64), (8, 64), (16, 64), (16, 512), (4, 2000), (0, 4096), (0, 2)):
        R_max = (160 * 1024 - 256 - 64 - 20 - image - S * 4) // 6
        assert R_max < 512 * 8 * 4 and (S != 64 or R_max == 11399)
        a, b = F.plan(lib, G48, R_max, S, F.switches(rays=rays)), F.plan(lib, G48, R_max + 1, S, F.switches(rays=rays))
        assert a["group"] == b["group"] and (S > 64 or a["group"] == max(rays, 4)), (rays, S, a)
        assert (a["in_lds"], a["scan_tiles"], b["in_lds"], b["scan_tiles"]) == (1, 0, 0, 1), (rays, S, R_max, a, b)
        assert a["shade3_lds"] == image + S * 4 + (R_max + 1) * 4 + R_max * 2 + 16 and b["shade3_lds"] == image + S * 4
        assert a["shade3_lds"] + 64 <= a["shade3_opt_in"] < a["shade3_lds"] + 64 + 6
    for R in (16384, 16385):
        assert F.plan(lib, G48, R, 64, F.switches())["in_lds"] == 0
    # the switch
    off = F.plan(lib, G48, 5, 64, F.switches(toff=False))
    assert (off["in_lds"], off["scan_tiles"], off["shade3_lds"]) == (0, 1, image + 64 * 4)
    # two pipe chunks
    assert [F.plan(lib, G48, R, 64, F.switches())["pipe_chunks"] for R in (32767, 32768, 32769, 65536, 65537)] == [1, 2, 3, 4, 5]


def test_sizes_are_the_parents(golden):
    got, want = F.sizes(N.lib()), golden["sizes"]
    assert set(got) == set(want) and len(want) == 7 * len(F.SHAPES)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert want["lrf_workspace_bytes(32768,64)"] >= 2 * want["lrf_workspace_bytes(16384,64)"]   # (two chunks, a workspace each)


def test_refusals_are_the_parents(golden):
    want = golden["refusals"]
    got = F.refusals(N.lib())
    calls, _ = F.refusal_calls()
    assert set(want) == set(got) == {key for key, _, _ in calls}   # nothing was dropped when the golden file was recorded
    assert {name for _, name, _ in calls} == {"lrf_render_fwd", "lrf_render_fwd_train", "lrf_render_normals",
                                              "lrf_render_depth_quantiles", "lrf_scene_fwd"}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    fused = {k for k, v in want.items() if v[1] == "lrf_scene_fwd: scene workspace too small"}
    assert fused == {"scene fused", "scene fused four", "scene fused chunk 0", "scene fused ragged tail", "scene fused 640"}
    assert "scene 2000 no lines" in want
    by_field = {k for k, v in want.items() if v[1].startswith("lrf_scene_rays")}
    assert len(by_field) == 16, sorted(by_field)
