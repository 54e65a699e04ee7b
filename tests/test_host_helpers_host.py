"""The host side of the entry points after it moved onto the shared helpers of csrc/lrf_host.inl (refuse, launch, misaligned,
Carver): every workspace size and every refusal recorded from the commit before the move (tests/golden/host_helpers_parent.json,
written by tests/golden/make_golden_host_helpers.py) comes out the same, byte for byte.  No GPU: a size is arithmetic and every
recorded refusal comes before the library's first HIP call."""
import json
import os

import pytest

import host_helpers_cases as H
from localrf_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_helpers_parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_workspace_sizes_are_the_parents(golden):
    got = H.sizes(N.lib())
    want = golden["sizes"]
    assert set(got) == set(want)
    symbols = {k.split("(")[0] for k in want}
    assert symbols >= {"lrf_workspace_bytes", "lrf_workspace_bytes_bwd", "lrf_workspace_bytes_bwd_cfg", "lrf_workspace_layout_bwd",
                       "lrf_normals_workspace_bytes", "lrf_quantile_workspace_bytes", "lrf_select_workspace_bytes",
                       "lrf_flow_comparison_workspace_bytes", "lrf_depth_comparison_workspace_bytes",
                       "lrf_image_metrics_workspace_bytes", "lrf_frame_sharpness_workspace_bytes", "lrf_encode_frames_workspace_bytes"}
    for s in symbols - {"lrf_workspace_bytes", "lrf_workspace_bytes_bwd", "lrf_workspace_bytes_bwd_cfg", "lrf_workspace_layout_bwd",
                        "lrf_frame_sharpness_workspace_bytes"}:           # (these four take any shape; the fifth takes none)
        assert any(v == 0 for k, v in want.items() if k.startswith(s + "(")), f"{s}: no refused shape in the table"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_refusals_are_the_parents(golden):
    want = golden["refusals"]
    got = H.refusals(N.lib())
    assert len(want) >= 100 and set(want) <= set(got)
    entry_points = {name for key, name, _ in H.refusal_calls() if key in want}
    assert len(entry_points) == 40                                        # every entry point of the twelve converted files
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
