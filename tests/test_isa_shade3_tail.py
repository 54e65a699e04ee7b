"""Static checks on the tile loop of the colour kernel (k_shade3 / k_shade3m, csrc/lrf_shade3_kernel.inl), on the gfx950 assembly
of the library compiled as __graft_entry__.build() compiles it (no GPU needed; as tests/test_isa_checks.py).

The tile loop is the innermost backward branch that encloses every v_mfma of the kernel.

1. The tail moves lanes in the VALU: between the loop's last v_mfma and its back edge there is no ds_bpermute_b32 (six dependent
   LDS round trips per tile stood there), and the 15 DPP instructions and 6 lane swaps of join_halves32 / half_sum32 are there.
2. The next tile's header is not waited for where it is issued.  Pattern: H = the last three vector loads of the loop in front
   of its first global_load_dwordx4 (the first gather of the current tile).  Asserted: they are global_load_dword (the aligned
   dword that holds the 16-bit sample index), global_load_dword (the compositing weight) and global_load_dwordx3 (the ray's
   direction), and the loop holds no global_load_ushort (its zero extension was the use that forced the wait); between the
   first load of H and that first gather no s_waitcnt names vmcnt -- such a wait could only be satisfied by the loads of H,
   the only vector-memory operations issued behind it.  (With global tile offsets the walk to the tile's ray, in front of
   H, reads an offset and waits for it: that is the walk's own load, step d of the round-trip work, not taken.)
"""
import re

import pytest

from isa_util import device_asm, kernels

KERNELS = r"k_shade3m?ILi8ELb[01]ELb0ELb[01]EE"  # the four k_shade3 instantiations of the render paths and k_shade3m


@pytest.fixture(scope="module")
def loops():
    found = {name: _tile_loop(body) for name, body in kernels(device_asm()).items() if re.search(KERNELS, name)}
    assert len(found) == 5, sorted(found)
    return found


def _tile_loop(body):
    """(instructions of the tile loop, index of its last v_mfma)."""
    lines = body.splitlines()
    labels = {m[1]: i for i, ln in enumerate(lines) if (m := re.match(r"(\.LBB\d+_\d+):", ln))}
    mf = [i for i, ln in enumerate(lines) if "v_mfma" in ln]
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_(?:cbranch_\w+|branch) (\.LBB\d+_\d+)", ln)
        if m and m[1] in labels and labels[m[1]] < mf[0] and i > mf[-1] and (best is None or i - labels[m[1]] < best[1] - best[0]):
            best = (labels[m[1]], i)
    assert best is not None, "no backward branch around the MFMAs"
    ins = [ln.split(";")[0].strip() for ln in lines[best[0]:best[1] + 1]]
    ins = [s for s in ins if s and not s.endswith(":") and not s.startswith(".")]
    last = max(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    assert sum(s.startswith("v_mfma_f32_32x32x16_bf16") for s in ins) == 135
    return ins, last


def test_tail_has_no_lds_lane_moves(loops):
    for name, (ins, last) in loops.items():
        tail = ins[last:]
        assert not any(s.startswith("ds_bpermute_b32") for s in tail), name
        assert not any(s.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")) for s in ins), name     # nor anywhere else in the loop
        assert sum(s.startswith("v_permlane32_swap") for s in tail) == 3, name                              # o0, o1, o2
        assert sum(s.startswith("v_permlane16_swap") for s in tail) == 3, name                              # r, g, b
        assert sum("_dpp" in s.split()[0] for s in tail) == 15, name                                        # 3 x (xor 1, 2, 4 (two moves), 8)


def test_next_header_is_not_awaited_where_it_is_issued(loops):
    for name, (ins, last) in loops.items():
        first_gather = next(i for i, s in enumerate(ins) if s.startswith("global_load_dwordx4"))
        loads = [i for i, s in enumerate(ins[:first_gather]) if s.startswith(("global_load", "buffer_load"))]
        header = loads[-3:]
        assert [ins[i].split()[0] for i in header] == ["global_load_dword", "global_load_dword", "global_load_dwordx3"], (name, [ins[i] for i in loads])
        assert not any(s.startswith("global_load_ushort") for s in ins), name
        waits = [s for s in ins[header[0]:first_gather] if s.startswith("s_waitcnt") and "vmcnt" in s]
        assert not waits, (name, waits)
