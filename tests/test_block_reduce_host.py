"""The numpy restatement that tests/test_gpu_block_reduce.py pins the workgroup reductions to is sensitive to the order it
states: on the mixed rows of block_reduce_cases.py, a butterfly run 1 -> 32, the waves folded from the last, and np.sum each
give other bits.  Without this the GPU pin could pass under a wrong order.  No GPU."""
import numpy as np
import pytest

from block_reduce_cases import OFFSETS, block_reduce, expected, rows


@pytest.mark.parametrize("nt", [256, 1024])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_stated_order_differs_from_its_neighbours(nt, dtype):
    mixed = rows(nt)[0].astype(dtype)
    bits = {np.float32: np.uint32, np.float64: np.uint64}[dtype]
    stated = block_reduce(mixed, np.add)
    others = {"butterfly 1 -> 32": block_reduce(mixed, np.add, offsets=OFFSETS[::-1]),
              "waves from the last": block_reduce(mixed, np.add, reverse_waves=True),
              "np.sum": np.sum(mixed, dtype=dtype)}
    for what, other in others.items():
        assert np.isfinite(other) and stated.view(bits) != dtype(other).view(bits), (what, stated, other)


def test_rows_and_expected_values():
    for nt in (64, 256, 1024):
        v = rows(nt)
        s32, s64, lo, hi = expected(v)
        assert (s32.dtype, s64.dtype, lo.dtype, hi.dtype) == (np.float32, np.float64, np.uint32, np.uint32)
        assert np.abs(np.log2(np.abs(v[0]))).max() <= 21 and (v[0] > 0).any() and (v[0] < 0).any()
        assert s32[1].view(np.uint32) == 0 and s64[1].view(np.uint64) == 0              # +0.0, not -0.0
        assert np.isnan(v[2]).sum() == 1 and np.isposinf(v[2]).sum() == 1 and not np.isneginf(v[2]).any()
        assert s32[2].view(np.uint32) == 0x7FC00000 and s64[2].view(np.uint64) == 0x7FF8000000000000   # the input's NaN
        assert (lo == v.view(np.uint32).min(1)).all() and (hi == v.view(np.uint32).max(1)).all()
