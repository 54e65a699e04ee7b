"""Depth quantiles without a GPU: the fp32 restatement of the kernel against the fp64 oracle of the definition, the properties
of the definition, the cap on the rays the GPU comparison may exclude, the exported symbols and every refusal that comes
before a launch.

Tolerance (also the GPU test's): on the rays the oracle does not flag the index is equal and |depth - depth64| <=
max(4 e, 1e-6 max z / dn), e = max |restatement with a sequential fp32 prefix sum - fp64| over the same rays: the same fp32
arithmetic in another summation order.  The flagged share (a C_i within 1e-5 of q, or w_{i*} < 1e-4) is capped at 2 %."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from abi_util import FAKE, declared_exported_bound, refused
import quantile_cases as Q
from localrf_amd import NativeError, depth_quantiles, mesh, pointcloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.5, 0.1, 0.9, 0.25)                                              # unsorted


@pytest.mark.parametrize("S", [2, 63, 64, 65, 129, 512])
def test_restatement_against_the_fp64_oracle(S):
    w, z, rays = Q.synthetic(300, S, seed=100 + S)
    depth, index = Q.restate(w, z, rays, QS)
    assert depth.dtype == np.float32 and index.dtype == np.int32 and depth.shape == (4, 300)
    Q.compare(f"synthetic S={S}", w, z, rays, QS, depth, index)
    assert ((index >= 0) & (index < S - 1)).any() or S == 2             # crossings before the forced last sample
    if S > 64:
        assert (index >= 64).any() and ((index >= 0) & (index < 64)).any()          # in the first step and beyond it


def test_properties_of_the_definition():
    w, z, rays = Q.synthetic(200, 129, seed=7)
    qs = (0.1, 0.25, 0.5, 0.9)
    depth, index = Q.restate(w, z, rays, qs)
    found = index >= 0
    for a in range(3):                                                  # q1 < q2: index and depth do not decrease
        both = found[a] & found[a + 1]
        assert (index[a][both] <= index[a + 1][both]).all() and (depth[a][both] <= depth[a + 1][both]).all()
        assert not (found[a + 1] & ~found[a]).any()
    dn = Q.ray_norm32(rays)
    for j in (0, 63, 64, 128):                                          # the whole weight in sample j
        one = np.zeros((200, 129), np.float32)
        one[:, j] = 0.8
        d, i = Q.restate(one, z, rays, (0.2, 0.8, 0.81))
        assert (i[:2] == j).all() and (i[2] == -1).all() and (d[2] == 0).all()
        z1 = z[min(j + 1, 128)]
        assert np.array_equal(d[1], ((z[j] + np.float32(1) * (z1 - z[j])) / dn).astype(np.float32))       # t = 1: the far end
    sub = w * np.float32(0.3)                                           # acc <= 0.3 + rounding < q
    d, i = Q.restate(sub, z, rays, (0.5,))
    assert (i == -1).all() and (d == 0).all() and not np.signbit(d).any()
    d, i = Q.restate(np.zeros((5, 129), np.float32), z, rays[:5], (0.5, 1.0))
    assert (i == -1).all() and (d == 0).all()
    for S in (2, 65, 129):
        wa, labels = Q.adversarial(S)
        ra = np.resize(rays, (wa.shape[0], 6)).astype(np.float32)
        za = z[:S]
        d, i = Q.restate(wa, za, ra, (0.5, 0.9))
        for r, (kind, j) in enumerate(labels):
            if kind in ("at", "tie"):
                assert i[0, r] == j and d[0, r] > 0, (S, kind, j)
            elif kind == "late nan":                                    # crossed before the NaN: kept; after it: none
                assert i[0, r] == 0 and i[1, r] == -1 and d[1, r] == 0
            else:
                assert i[0, r] == -1 and d[0, r] == 0 and i[1, r] == -1, (S, kind, j)
        d64, i64, _ = Q.oracle64(wa, za, ra, (0.5, 0.9))
        assert np.array_equal(i64, i)                                   # the oracle follows the same rule, NaN included


@pytest.mark.parametrize("case", [c for c in Q.FIELD_CASES if c != "alpha_mask"])
def test_flagged_share_of_the_field_cases(case):
    """The cap on the fields the GPU test uses, from the CPU oracle's weights (alpha_mask's mask is built on the GPU: its
    count is asserted there)."""
    f, rays, floater, n = Q.case_field(case, "cpu")
    w, z = Q.oracle_weights(f, rays, n, floater)
    q = (0.25, 0.5, 0.75)
    depth, index = Q.restate(w, z, rays.numpy(), q)
    Q.compare(case, w, z, rays.numpy(), q, depth, index)


def test_quantile_symbols_declared_exported_and_checked(built_lib):
    from localrf_amd import _native as N
    header = declared_exported_bound(built_lib, ("lrf_quantile_workspace_bytes", "lrf_render_depth_quantiles"))
    debug = open(os.path.join(ROOT, "include", "lrf_debug.h")).read()
    assert "lrf_depth_quantiles_from_weights" in N.SYMBOLS and "lrf_depth_quantiles_from_weights(" in debug
    getattr(built_lib, "lrf_depth_quantiles_from_weights")
    assert built_lib.lrf_abi_version() == 7 and "#define LRF_ABI_VERSION 7" in header
    ws = built_lib.lrf_quantile_workspace_bytes
    assert ws(0, 64) == 0 and ws(16, 1) == 0 and ws(16, 4097) == 0
    for R, S in ((1, 2), (200, 88), (4096, 512)):
        assert ws(R, S) >= built_lib.lrf_workspace_bytes(R, S) + 4 * R * S + 20 * R
        assert ws(R, S) <= built_lib.lrf_workspace_bytes(R, S) + 4 * R * S + 20 * R + 5 * 256
    fake = C.c_void_p(FAKE)
    fld = N.LrfField()
    fld.cache = FAKE
    fld.grid[:] = [20, 24, 28]
    half = (C.c_float * 4)(0.5, 0.25, 0.75, 1.0)


    def dq(f=C.byref(fld), rays=fake, z=fake, R=8, S=64, flags=1, q=half, K=1, bw=None, per_view=1, accumulate=0, depth=fake,
           wsum=None, index=None, acc=None, wsp=fake):
        return refused(built_lib, built_lib.lrf_render_depth_quantiles(f, rays, z, R, S, flags, 0.0, q, K, bw, per_view, accumulate, depth,
                                                                         wsum, index, acc, wsp, None))
    for bad in (dict(f=None), dict(rays=None), dict(z=None), dict(q=None), dict(depth=None), dict(wsp=None)):
        assert dq(**bad) == "lrf_render_depth_quantiles: null argument", bad
    for bad in (dict(R=0), dict(R=-3), dict(S=1), dict(S=4097)):
        assert "need R > 0 and 2 <= S <= 4096" in dq(**bad), bad
    for bad in (dict(K=0), dict(K=5), dict(K=-1)):
        assert "1 <= K <= 4" in dq(**bad), bad
    for v in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert "(0, 1]" in dq(q=(C.c_float * 2)(0.5, v), K=2), v
    assert "(0, 1]" not in dq(q=(C.c_float * 2)(0.5, 7.0), K=1, wsp=None)           # beyond K: not read
    assert "unknown flag bits" in dq(flags=1 << 12)
    assert "per_view" in dq(bw=fake, wsum=fake, per_view=0)
    assert "accumulate must be 0 or 1" in dq(accumulate=2) and "accumulate must be 0 or 1" in dq(accumulate=-1)
    assert "accumulate = 1 needs index = NULL" in dq(accumulate=1, index=fake)
    assert "blend_w needs wsum" in dq(bw=fake)
    for bad in (dict(depth=C.c_void_p(0x10002)), dict(wsum=C.c_void_p(0x10001)), dict(index=C.c_void_p(0x10002)),
                dict(acc=C.c_void_p(0x10003)), dict(rays=C.c_void_p(0x10002)), dict(bw=C.c_void_p(0x10002), wsum=fake)):
        assert "4-byte aligned" in dq(**bad), bad
    assert "256-byte aligned" in dq(wsp=C.c_void_p(0x10010))

    def fw(w=fake, z=fake, rays=fake, R=8, S=64, q=half, K=1, depth=fake, index=None):
        return refused(built_lib, built_lib.lrf_depth_quantiles_from_weights(w, z, rays, R, S, q, K, depth, index, None))
    for bad in (dict(w=None), dict(z=None), dict(rays=None), dict(q=None), dict(depth=None)):
        assert fw(**bad) == "lrf_depth_quantiles_from_weights: null argument", bad
    assert "2 <= S <= 4096" in fw(S=1) and "2 <= S <= 4096" in fw(R=0) and "1 <= K <= 4" in fw(K=5)
    assert "(0, 1]" in fw(q=(C.c_float * 1)(0.0)) and "4-byte aligned" in fw(index=C.c_void_p(0x10002))


def test_python_refusals_before_any_launch():
    from normals_cases import field
    from novel_views_cases import scene
    lt, g = scene("cpu")
    W, H = int(g["W"]), int(g["H"])
    poses = torch.from_numpy(g["poses"])
    f = field("cpu", 1)
    with pytest.raises(NativeError, match="no CPU fallback"):
        f.render_depth_quantiles(torch.zeros(4, 6))
    with pytest.raises(TypeError):
        f.render_depth_quantiles([[0.0] * 6])
    for bad in ((), (0.1, 0.2, 0.3, 0.4, 0.5), (0.0,), (1.5,), (float("nan"),), (0.5, -1.0)):
        with pytest.raises(ValueError, match="q must"):
            f.render_depth_quantiles(torch.zeros(4, 6), q=bad)
        with pytest.raises(ValueError, match="q must"):
            depth_quantiles.render_depth_quantiles(lt, poses, W, H, q=bad)
    with pytest.raises(NativeError):
        depth_quantiles.render_depth_quantiles(lt, poses, W, H)
    with pytest.raises(NativeError):
        depth_quantiles.median_depth(lt, poses, W, H)
    with pytest.raises(ValueError, match="poses"):
        depth_quantiles.render_depth_quantiles(lt, torch.zeros(3, 2, 4), W, H)
    with pytest.raises(ValueError, match="chunk"):
        depth_quantiles.median_depth(lt, poses, W, H, chunk=0)
    # the fusion entry points: a bad depth=, max_spread without "median" -- before the scene's device is even looked at
    for fn, args in ((pointcloud.scene_point_cloud, (lt, W, H)), (mesh.scene_mesh, (lt, W, H, 0.1))):
        with pytest.raises(ValueError, match="'expected' or 'median'"):
            fn(*args, depth="mean")
        with pytest.raises(ValueError, match="'expected' or 'median'"):
            fn(*args, depth=None)
        with pytest.raises(ValueError, match="max_spread needs depth='median'"):
            fn(*args, max_spread=0.1)
        with pytest.raises(ValueError, match="max_spread needs depth='median'"):
            fn(*args, depth="expected", max_spread=0.1)
        with pytest.raises(ValueError, match="max_spread must be"):
            fn(*args, depth="median", max_spread=-1.0)
        with pytest.raises(NativeError):                                 # valid arguments, CPU scene
            fn(*args, depth="median", max_spread=0.2, **({"bounds": ((-1, -1, -1), (1, 1, 1))} if fn is mesh.scene_mesh else {}))


def test_spread_filter_is_the_stated_expression():
    d25 = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 2.0])
    d50 = torch.tensor([2.0, 2.0, 2.0, 0.0, 2.0, 2.0])
    d75 = torch.tensor([2.2, 3.5, 3.0, 3.0, 0.0, 2.0])
    got = depth_quantiles.spread_filter(d25, d50, d75, 0.75)
    assert got.tolist() == [2.0, 0.0, 0.0, 0.0, 0.0, 2.0]               # 1.2 <= 1.5 kept; 2.5 > 1.5; three with one missing; 0 spread
