"""Deterministic backward (LRF_FLAG_DETERMINISTIC), the host side: the ABI bit, the scatter-partition knob, the flag word
TensorVMSplit builds (its own setting or torch.use_deterministic_algorithms) and the workspace the mode needs.  No GPU."""
import ctypes as C
import os
import re

import torch

from util import make_field, quiet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    hdr = open(os.path.join(ROOT, "include", "lrf.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+(\d+)u", hdr)
    assert m, name
    return int(m[1])


def test_header_and_binding_define_the_flag():
    from localrf_amd import _native as N
    assert _define("LRF_FLAG_DETERMINISTIC") == 256 and _define("LRF_FLAG_ALL") == 511
    assert N.LRF_FLAG_DETERMINISTIC == 256 and N.LRF_FLAG_ALL == 511


def test_scatter_workgroup_knob_is_exported(built_lib):
    from localrf_amd import _native as N
    assert "lrf_debug_set_scatter_wgs" in N.SYMBOLS
    assert "lrf_debug_set_scatter_wgs" in open(os.path.join(ROOT, "include", "lrf_debug.h")).read()
    built_lib.lrf_debug_set_scatter_wgs(0)          # (the default; process-wide)


def test_flags_follow_the_field_and_torch():
    from localrf_amd import _native as N
    f = quiet(make_field, [16, 16, 16], "cpu", seed=0)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert f.deterministic is None and not f._flags(True) & N.LRF_FLAG_DETERMINISTIC
        f.deterministic = True
        assert f._flags(True) & N.LRF_FLAG_DETERMINISTIC and f._flags(False) & N.LRF_FLAG_DETERMINISTIC
        f.deterministic = None
        torch.use_deterministic_algorithms(True)
        assert f._flags(True) & N.LRF_FLAG_DETERMINISTIC
        f.deterministic = False                      # forced off whatever torch says
        assert not f._flags(True) & N.LRF_FLAG_DETERMINISTIC
    finally:
        torch.use_deterministic_algorithms(was)


def test_workspace_grows_only_with_the_flag(built_lib):
    from localrf_amd import _native as N
    for g3 in ((300, 300, 300), (64, 48, 40)):
        grid = (C.c_int32 * 3)(*g3)
        plain = built_lib.lrf_workspace_bytes_bwd_cfg(4096, 512, grid, 0, 0, 128, 0)
        assert plain == built_lib.lrf_workspace_bytes_bwd(4096, 512, grid)
        det = built_lib.lrf_workspace_bytes_bwd_cfg(4096, 512, grid, 0, 0, 128, N.LRF_FLAG_DETERMINISTIC)
        x, y, z = g3
        elems = (8 + 24) * (x * y + x * z + y * z + x + y + z)          # every plane and line gradient element, 8 bytes each
        assert det - plain >= 8 * elems and det - plain <= 8 * elems + 12 * 256, (g3, det - plain, 8 * elems)
