"""Inputs and the numpy restatement for the workgroup reductions of csrc/lrf_common.h (block_sum, block_sum0, block_min0,
block_max0), shared by tests/test_gpu_block_reduce.py and tests/test_block_reduce_host.py.

The order every kernel outside the render hot path promises: an xor butterfly over each wave's 64 lanes with offsets
32, 16, ... 1, then the waves' values folded in wave-index order starting from wave 0's, ((w0 o w1) o w2) o ..."""
import numpy as np

NTS = (64, 256, 1024)                      # one wave (the fold is the identity), four waves, sixteen
ROWS = ("mixed", "zeros", "nan_inf")
SEED = 14                                  # test_block_reduce_host.py shows that the mixed rows tell the orders apart
LANE = np.arange(64)
OFFSETS = (32, 16, 8, 4, 2, 1)


def rows(nt):
    """[3][nt] float32: mixed signs and magnitudes across 2^-20 .. 2^20; all +0.0; values with one NaN and one +Inf (no -Inf:
    the only NaN of the sums is then the input's own quiet NaN, propagated, and its bits are defined)."""
    rng = np.random.RandomState(SEED)
    mixed = (rng.choice([-1.0, 1.0], nt) * rng.uniform(1.0, 2.0, nt) * np.exp2(rng.uniform(-20.0, 20.0, nt))).astype(np.float32)
    special = rng.standard_normal(nt).astype(np.float32)
    special[(5 * nt) // 8 + 3] = np.float32(np.nan)
    special[nt // 8 + 1] = np.float32(np.inf)
    v = np.stack([mixed, np.zeros(nt, np.float32), special])
    assert v.dtype == np.float32 and not np.signbit(v[1]).any()
    return v


def block_reduce(row, op, offsets=OFFSETS, reverse_waves=False):
    """row [nt] of any dtype -> the workgroup's value in that dtype: per wave the butterfly (every lane ends with the same
    bits; lane 0's are stored), then the waves folded from the first."""
    v = row.reshape(-1, 64)
    with np.errstate(all="ignore"):
        for d in offsets:
            v = op(v, v[:, LANE ^ d])
        w = v[:, 0][::-1] if reverse_waves else v[:, 0]
        s = w[0]
        for k in range(1, len(w)):
            s = op(s, w[k])
    assert s.dtype == row.dtype
    return s


def expected(v):
    """rows [B][nt] float32 -> (fp32 sums, fp64 sums of the widened values, uint32 min and max of the bit patterns)"""
    bits = v.view(np.uint32)
    return (np.array([block_reduce(r, np.add) for r in v]),
            np.array([block_reduce(r.astype(np.float64), np.add) for r in v]),
            np.array([block_reduce(r, np.minimum) for r in bits]),
            np.array([block_reduce(r, np.maximum) for r in bits]))
