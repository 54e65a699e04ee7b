"""The device frame store (localrf_amd.frames, csrc/lrf_frames.inl) without a GPU: the exports, the C ABI's refusals (every
call here is refused before any launch: the pointers are never dereferenced), sample_ids against a numpy restatement of
LocalRFDataset.sample() (dataLoader/localrf_dataset.py:273-313) under the same seeds, the numpy facts the kernels rely on,
and DeviceFrames' refusals that come before any device allocation."""
import ctypes as C
import random
import sys
import os

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_cases as fc  # noqa: E402
from abi_util import filled  # noqa: E402
from localrf_amd import frames  # noqa: E402
from localrf_amd import _native as N  # noqa: E402

FAKE = 1 << 40          # a non-null address that is never dereferenced: every call below is refused first


def _window(**over):
    planes = ("rgb", "loss_weight", "invdepth", "fwd_flow", "fwd_mask", "bwd_flow", "bwd_mask", "slot_of", "status")
    return filled(N.LrfFrameWindow, dict(dict.fromkeys(planes, FAKE), capacity=4, n_px=12, num_images=10), **over)


def test_library_exports_the_frame_store(built_lib):
    for name in ("lrf_frames_gather", "lrf_decode_flow", "lrf_frame_sharpness", "lrf_frame_sharpness_workspace_bytes"):
        assert name in N.SYMBOLS and getattr(built_lib, name) is not None
    assert built_lib.lrf_frame_sharpness_workspace_bytes() > 0
    assert built_lib.lrf_abi_version() == 7


def _err(lib):
    return lib.lrf_last_error().decode()


def test_c_abi_refuses_bad_windows_before_any_launch(built_lib):
    lib = built_lib
    ids = C.c_void_p(FAKE)
    out = [C.c_void_p(FAKE)] + [None] * 6
    assert lib.lrf_frames_gather(None, ids, ids, 2, 3, *out, None) != 0 and "null window" in _err(lib)
    for bad in (dict(capacity=0), dict(n_px=0), dict(num_images=0), dict(capacity=-3)):
        w = _window(**bad)
        assert lib.lrf_frames_gather(C.byref(w), ids, ids, 2, 3, *out, None) != 0 and "positive" in _err(lib)
        assert lib.lrf_decode_flow(C.byref(w), 0, 0, ids, 3, 4, 1.0, None) != 0
        assert lib.lrf_frame_sharpness(C.byref(w), 0, 3, 4, None, ids, None) != 0
    for k in ("rgb", "loss_weight", "slot_of", "status"):
        w = _window(**{k: None})
        assert lib.lrf_frames_gather(C.byref(w), ids, ids, 2, 3, *out, None) != 0 and "required" in _err(lib)
    w = _window(fwd_mask=None)
    assert lib.lrf_frames_gather(C.byref(w), ids, ids, 2, 3, *out, None) != 0 and "mask plane" in _err(lib)


def test_c_abi_refuses_bad_views_ids_and_outputs(built_lib):
    lib = built_lib
    ids = C.c_void_p(FAKE)
    out = [C.c_void_p(FAKE)] * 7
    w = _window()
    for V, n in ((0, 3), (-1, 3), (2, 0), (1 << 20, 1 << 10)):
        assert lib.lrf_frames_gather(C.byref(w), ids, ids, V, n, *out, None) != 0 and "V > 0" in _err(lib)
    assert lib.lrf_frames_gather(C.byref(w), None, ids, 2, 3, *out, None) != 0 and "null ids" in _err(lib)
    assert lib.lrf_frames_gather(C.byref(w), ids, None, 2, 3, *out, None) != 0 and "null ids" in _err(lib)
    w = _window(invdepth=None)
    assert lib.lrf_frames_gather(C.byref(w), ids, ids, 2, 3, *out, None) != 0 and "does not hold" in _err(lib)
    w = _window(fwd_flow=None, fwd_mask=None)
    outs = [None] * 4 + [C.c_void_p(FAKE)] + [None] * 2                     # fwd_mask alone
    assert lib.lrf_frames_gather(C.byref(w), ids, ids, 2, 3, *outs, None) != 0 and "does not hold" in _err(lib)


def test_c_abi_refuses_bad_decode_and_sharpness_arguments(built_lib):
    lib = built_lib
    p = C.c_void_p(FAKE)
    w = _window()                                                               # n_px = 12
    assert lib.lrf_decode_flow(C.byref(w), 0, 0, p, 3, 5, 1.0, None) != 0 and "n_px" in _err(lib)
    assert lib.lrf_decode_flow(C.byref(w), 4, 0, p, 3, 4, 1.0, None) != 0 and "slot" in _err(lib)
    assert lib.lrf_decode_flow(C.byref(w), -1, 1, p, 3, 4, 1.0, None) != 0 and "slot" in _err(lib)
    assert lib.lrf_decode_flow(C.byref(w), 0, 0, None, 3, 4, 1.0, None) != 0 and "null" in _err(lib)
    assert lib.lrf_decode_flow(C.byref(w), 0, 0, p, 3, 4, float("inf"), None) != 0 and "finite" in _err(lib)
    assert lib.lrf_decode_flow(C.byref(w), 0, 0, p, 3, 4, 1e300, None) != 0 and "finite" in _err(lib)
    nf = _window(fwd_flow=None, fwd_mask=None, bwd_flow=None, bwd_mask=None)
    assert lib.lrf_decode_flow(C.byref(nf), 0, 1, p, 3, 4, 1.0, None) != 0 and "no flow" in _err(lib)
    assert lib.lrf_frame_sharpness(C.byref(w), 0, 4, 4, None, p, None) != 0 and "n_px" in _err(lib)
    assert lib.lrf_frame_sharpness(C.byref(w), 4, 3, 4, None, p, None) != 0 and "slot" in _err(lib)
    assert lib.lrf_frame_sharpness(C.byref(w), 0, 3, 4, None, None, None) != 0 and "workspace" in _err(lib)
    big = _window(n_px=(1 << 21) + 1, capacity=1)
    assert lib.lrf_frame_sharpness(C.byref(big), 0, 1, (1 << 21) + 1, None, p, None) != 0 and "2^21" in _err(lib)


def _case_windows():
    """(fbases, test_frame_every, bounds): windows with and without test frames, and windows after deactivate_frames."""
    num = [f"{i:05d}" for i in range(40)]
    named = [f"frame_{i}" for i in range(30)]
    return [(num, 10, (0, 7)), (num, 10, (0, 23)), (num, 10, (12, 31)), (num, 10, (20, 24)), (num, 10, (33, 40)),
            (num, 0, (5, 17)), (named, 4, (3, 11)), (num, 10, (9, 12)), (num, 10, (0, 3))]


@pytest.mark.parametrize("case", range(9))
@pytest.mark.parametrize("is_refining", [False, True])
@pytest.mark.parametrize("optimize_poses", [False, True])
def test_sample_ids_matches_the_reference_sample(case, is_refining, optimize_poses):
    fbases, every, bounds = _case_windows()[case]
    mask = fc.mask_of_fbases(fbases, every)
    n_px, batch = 6 * 5, 16 * 8
    n_active = bounds[1] - bounds[0]
    all_x = {"rgbs": np.arange(n_active * n_px * 3, dtype=np.float32).reshape(-1, 3)}
    seen_ttp = set()
    for seed in range(12):
        random.seed(seed); np.random.seed(seed)
        ref = fc.reference_sample(mask, bounds, n_px, all_x, batch, is_refining, optimize_poses)
        r_state, n_state = random.random(), np.random.random()
        random.seed(seed); np.random.seed(seed)
        views, idx, ttp = frames.sample_ids(mask, list(bounds), n_px, batch, is_refining, optimize_poses)
        assert (random.random(), np.random.random()) == (r_state, n_state)            # the same draws were consumed
        assert views.dtype == np.int64 and idx.dtype == np.int64 and idx.shape == (batch,)
        np.testing.assert_array_equal(views, ref["view_ids"])
        np.testing.assert_array_equal(idx, ref["idx"])
        assert bool(ttp) == bool(ref["train_test_poses"])
        assert (views >= bounds[0]).all() and (views < bounds[1]).all()
        np.testing.assert_array_equal(all_x["rgbs"][idx - bounds[0] * n_px], ref["rgbs"])
        seen_ttp.add(bool(ttp))
        if not is_refining and (1 - mask[bounds[0]:bounds[1]]).sum() > 4 and not ttp:     # the forced last views
            cand = np.arange(*bounds)[mask[bounds[0]:bounds[1]] == 0]
            assert list(views[:6]) == [cand[-1], cand[-1], cand[-2], cand[-2], cand[-3], cand[-4]]
    if not optimize_poses:
        assert seen_ttp == {False}


def test_test_mask_follows_fbases():
    fb = ["00000", "00007", "00010", "x", "00020", "y"]
    assert list(fc.mask_of_fbases(fb, 10)) == [1, 0, 1, 0, 1, 0]
    assert list(fc.mask_of_fbases(["a", "b", "c"], 2)) == [1, 0, 1]               # non-numeric stems: their index


def test_numpy_rounds_the_flow_scale_to_fp32_before_the_multiply():
    """localrf_dataset.py:193-194: `fwd_flow * flow_scale` with a float32 array and a Python float is a float32 product of the
    float rounded to fp32 (what k_decode_flow computes), which is not the fp64 product rounded once."""
    enc = np.stack(np.meshgrid(np.arange(0, 65536, 97, dtype=np.int64), np.arange(3), indexing="ij"), -1)
    enc = np.concatenate([enc[..., :1], enc[..., :1], np.full_like(enc[..., :1], 32769)], -1)[:, 0].astype(np.uint16)
    flow = enc[..., :2].astype(np.float32)
    flow -= 2 ** 15
    flow /= 2 ** 8
    scale = 540 / 271                                                            # a non-integer Python float
    got = flow * scale
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, flow * np.float32(scale))
    assert not np.array_equal(got, (flow.astype(np.float64) * scale).astype(np.float32))
    f, m = fc.decode_flow_scaled(np.array([[0, 32768, 32768], [65535, 32769, 32769], [1, 1, 65535]], dtype=np.uint16), 1.0)
    np.testing.assert_array_equal(f, np.array([[-128.0, 0.0], [127.99609375, 0.00390625], [-127.99609375, -127.99609375]], np.float32))
    np.testing.assert_array_equal(m, np.array([0.0, 1.0, 1.0], np.float32))


def test_grey_uses_truncation_and_opencv_constants():
    k = np.arange(256, dtype=np.float32)
    np.testing.assert_array_equal(((k / np.float32(255)) * np.float32(255)).astype(np.uint8), k.astype(np.uint8))   # 8-bit values survive
    area = np.array([[[0.5, 0.5, 0.5]]], np.float32)                             # an INTER_AREA average is not an 8-bit value:
    assert fc.grey_u8(area)[0, 0] == 127                                         # 127.5 truncates (rounding would give 128)
    prim = np.eye(3, dtype=np.float32)[None]                                     # pure red, green, blue
    assert list(fc.grey_u8(prim)[0]) == [76, 150, 29]                            # OpenCV's RGB2GRAY of (255,0,0) etc.
    assert fc.grey_u8(np.ones((1, 1, 3), np.float32))[0, 0] == 255


@pytest.mark.parametrize("H,W", [(37, 53), (1, 9), (8, 1), (2, 2), (61, 3)])
def test_exact_sharpness_is_numpys_float32_variance(H, W):
    img = fc.make_frame(3, H, W)["img"]
    a, b = fc.sharpness_exact(img), fc.sharpness_numpy_f32(img)
    lap = fc.laplacian(fc.grey_u8(img)).astype(np.float64)
    assert a == np.float32(lap.var())                                            # the fp64 variance of the same integers
    assert abs(float(a) - float(b)) <= 2e-6 * max(abs(float(b)), 1e-30)


def _reader(H=6, W=5, **kw):
    return lambda i: fc.make_frame(i, H, W, **kw)


def test_device_frames_refuses_bad_readers_and_capacity_before_any_allocation():
    dev = "cuda:0"                                                               # never allocated: every call refuses first
    with pytest.raises(ValueError, match="capacity"):
        frames.DeviceFrames(_reader(), 10, capacity=3, n_init_frames=5, device=dev)
    with pytest.raises(ValueError, match="positive"):
        frames.DeviceFrames(_reader(), 10, capacity=0, device=dev)
    bad = [("img", lambda d: d["img"].astype(np.float64)), ("img", lambda d: d["img"][..., :2]),
           ("invdepth", lambda d: d["invdepth"][:, :-1]), ("invdepth", lambda d: d["invdepth"].astype(np.float16)),
           ("encoded_fwd_flow", lambda d: d["encoded_fwd_flow"].astype(np.int32)),
           ("encoded_bwd_flow", lambda d: d["encoded_bwd_flow"][..., :2]),
           ("mask", lambda d: d["mask"].astype(np.float32)), ("mask", lambda d: d["mask"][:-1])]
    for key, f in bad:
        def reader(i, key=key, f=f):
            d = fc.make_frame(i, 6, 5)
            d[key] = f(d)
            return d
        with pytest.raises(ValueError, match=key):
            frames.DeviceFrames(reader, 10, capacity=8, n_init_frames=2, device=dev)

    def no_scale(i):
        d = fc.make_frame(i, 6, 5)
        d["flow_scale"] = None
        return d
    with pytest.raises(ValueError, match="flow_scale"):
        frames.DeviceFrames(no_scale, 10, capacity=8, n_init_frames=2, device=dev)

    def decoded_bad(i):
        d = fc.make_frame(i, 6, 5, encoded=False)
        d["fwd_mask"] = d["fwd_mask"].astype(np.int64)
        return d
    with pytest.raises(ValueError, match="fwd_mask"):
        frames.DeviceFrames(decoded_bad, 10, capacity=8, n_init_frames=2, device=dev)
    with pytest.raises(TypeError):
        frames.DeviceFrames(lambda i: [1, 2], 10, capacity=8, device=dev)
    with pytest.raises(ValueError, match="fbases"):
        frames.DeviceFrames(_reader(), 10, capacity=8, fbases=["a"], device=dev)
    with pytest.raises(N.NativeError):
        frames.DeviceFrames(_reader(), 10, capacity=8, device="cpu")


def test_frame_store_kernels_use_no_scratch():
    import re
    from isa_util import device_asm, scratch_bytes
    asm = device_asm()
    for k in ("k_frames_gather", "k_decode_flow", "k_frame_sharpness", "k_frame_weight"):
        names = [m for m in re.findall(r"^(_Z\w+):", asm, re.M) if k + "E" in m or re.search(k + r"[A-Z]", m)]
        assert names, k
        for name in names:
            assert scratch_bytes(asm, name) == 0, (name, scratch_bytes(asm, name))
