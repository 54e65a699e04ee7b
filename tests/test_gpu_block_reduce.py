"""The order of the workgroup reductions (csrc/lrf_common.h: wave butterfly 32 -> 1, then the waves in index order from wave
0's value), bit for bit: lrf_debug_block_reduce runs block_sum / block_sum0 in fp32 and fp64 and the unsigned minimum and
maximum on the rows of block_reduce_cases.py, at one, four and sixteen waves and in both flavours (result in every thread,
result in thread 0), against the numpy restatement that tests/test_block_reduce_host.py shows to be sensitive to the order."""
import numpy as np
import pytest
import torch

from block_reduce_cases import NTS, ROWS, expected, rows

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("every_thread", [0, 1])
@pytest.mark.parametrize("nt", NTS)
def test_block_reductions_match_the_stated_order_bitwise(built_lib, nt, every_thread):
    v = rows(nt)
    B = len(v)
    d_in = torch.from_numpy(v).to(DEV)
    d_s32 = torch.full((B,), 7.0, device=DEV)
    d_s64 = torch.full((B,), 7.0, device=DEV, dtype=torch.float64)
    d_lo, d_hi = torch.full((B,), 7, device=DEV, dtype=torch.int32), torch.full((B,), 7, device=DEV, dtype=torch.int32)
    rc = built_lib.lrf_debug_block_reduce(d_in.data_ptr(), B, nt, every_thread, d_s32.data_ptr(), d_s64.data_ptr(), d_lo.data_ptr(),
                                          d_hi.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = (d_s32.cpu().numpy().view(np.uint32), d_s64.cpu().numpy().view(np.uint64), d_lo.cpu().numpy().view(np.uint32),
           d_hi.cpu().numpy().view(np.uint32))
    want = expected(v)
    want = (want[0].view(np.uint32), want[1].view(np.uint64), want[2], want[3])
    for what, g, w in zip(("fp32 sum", "fp64 sum", "min of bits", "max of bits"), got, want):
        print(nt, every_thread, what, [hex(x) for x in g], [hex(x) for x in w])
        assert (g == w).all(), (what, dict(zip(ROWS, zip(g, w))))


@pytest.mark.gpu
def test_refusals(built_lib):
    x = torch.zeros(3 * 128, device=DEV)
    o = torch.zeros(8, device=DEV, dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    assert built_lib.lrf_debug_block_reduce(x.data_ptr(), 3, 128, 0, o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), st) != 0
    assert built_lib.lrf_debug_block_reduce(x.data_ptr(), 0, 64, 0, o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), st) != 0
    assert built_lib.lrf_debug_block_reduce(None, 3, 64, 0, o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), st) != 0
