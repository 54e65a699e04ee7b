"""The two lane sums of k_shade3's tail (join_halves32, half_sum32, csrc/lrf_shade3.inl: lane swaps and DPP adds) against the
__shfl_xor butterflies they replaced, bit for bit in all 64 lanes.

lrf_debug_tile_reduce runs both helpers on a caller's [T][64] rows, one wave per row.  The reference is the old code in numpy
float32: join = v + v[lane ^ 32]; sum = the ladder v += v[lane ^ d], d = 1, 2, 4, 8, 16.  Rows: random normal x exp(3 normal)
(a wide dynamic range: the rounding of every level matters), denormals, signed zeros, one huge lane.  No NaNs: payload
propagation is not part of the contract."""
import numpy as np
import pytest
import torch

DEV = "cuda:0"
T = 64
LANE = np.arange(64)


def rows():
    rng = np.random.RandomState(24)
    v = (rng.standard_normal((T, 64)) * np.exp(3.0 * rng.standard_normal((T, 64)))).astype(np.float32)
    tiny = np.float32(1.4e-45)
    v[48:52] = (rng.randint(-200, 200, size=(4, 64)).astype(np.float32) * tiny)                  # denormals (and a few zeros)
    v[52] = 0.0
    v[53] = -0.0
    v[54] = np.where(rng.rand(64) < 0.5, np.float32(0.0), np.float32(-0.0))
    v[55] = np.where(rng.rand(64) < 0.5, v[55], np.float32(-0.0))                                 # zeros of either sign among values
    v[56:60, :] = rng.standard_normal((4, 64)).astype(np.float32)
    for i, lane in enumerate((0, 31, 32, 63)):                                                   # one huge lane
        v[56 + i, lane] = np.float32((-1) ** i * 3.0e38)
    v[60:64] = rng.standard_normal((4, 64)).astype(np.float32) * np.float32(1e-30)
    v[60:64, ::7] = np.float32(1e30)                                                             # sums that cancel nothing, lanes that vanish
    assert np.isfinite(v).all()
    return v


def butterflies(v):
    """What the tail computed before: every lane of v + shfl_xor(v, 32) and of the five-step ladder, in float32."""
    join = v + v[:, LANE ^ 32]
    s = v.copy()
    with np.errstate(over="ignore"):
        for d in (1, 2, 4, 8, 16):
            s = s + s[:, LANE ^ d]
    assert join.dtype == np.float32 and s.dtype == np.float32
    return join, s


@pytest.mark.gpu
def test_lane_sums_match_the_butterflies_bitwise(built_lib):
    v = rows()
    want_join, want_sum = butterflies(v)
    finite = np.isfinite(want_sum).all(1) & np.isfinite(want_join).all(1)                          # (a row that overflows to inf - inf is a NaN row)
    assert finite.sum() >= T - 4, finite
    d_in = torch.from_numpy(v).to(DEV)
    d_join, d_sum = torch.full_like(d_in, 7.0), torch.full_like(d_in, 7.0)
    rc = built_lib.lrf_debug_tile_reduce(d_in.data_ptr(), T, d_join.data_ptr(), d_sum.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got_join, got_sum = d_join.cpu().numpy(), d_sum.cpu().numpy()
    for what, got, want in (("join_halves32", got_join, want_join), ("half_sum32", got_sum, want_sum)):
        bad = got.view(np.uint32)[finite] != want.view(np.uint32)[finite]
        assert not bad.any(), (what, np.argwhere(bad)[:8], got[finite][bad][:4], want[finite][bad][:4])
    # the two halves of a row are summed apart, and every lane of a half holds its sum
    assert (got_sum.view(np.uint32)[finite][:, :32] == got_sum.view(np.uint32)[finite][:, :1]).all()
    assert (got_sum.view(np.uint32)[finite][:, 32:] == got_sum.view(np.uint32)[finite][:, 32:33]).all()

