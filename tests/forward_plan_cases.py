"""What tests/test_forward_plan_host.py compares the forward's launch plan (csrc/lrf_forward.inl) with.

1. restate(): the launch rules of k_march and k_shade3 in plain Python, written from the host code of the commit BEFORE the
   plan existed (march_lds_rays, march_lds_z, launch_march, launch_shade3, pipe_chunks of csrc/lrf_render.hip there), not from
   plan_march / plan_shade3.
2. sizes() / refusals(): the calls behind tests/golden/forward_plan_host_parent.json -- workspace sizes over a table of shapes,
   and every refusal of the forward's entry points that comes before the library touches HIP -- which
   tests/golden/make_golden_forward_plan_host.py records from a build of that commit.  Pointers are made-up addresses (A is
   256-byte aligned); what the host dereferences (LrfField, LrfSceneField) is real ctypes memory."""
import ctypes as C

import numpy as np

from localrf_amd import _native as N

# ---------------------------------------------------------------------------------------------------------- 1. the rules
LRF_CD = 8                      # density channels per line cell
MARCH_LDS_TAIL = 16
W32_ALL_U4 = 5928               # the colour network's weight image, in 16-byte words (csrc/lrf_common.h)
TILE_GPT = 8
PIPE_CHUNK = 16384
KB = 1024

LINES, TOFF = 1, 2              # lrf_debug_forward_plan's switch bits; forced march rays above them


def switches(lines=True, toff=True, rays=0):
    return (LINES if lines else 0) | (TOFF if toff else 0) | (rays << 2)


def restate(ll, R, S, lines=True, toff=True, rays=0):
    """The twelve numbers of lrf_debug_forward_plan; S an integer or an integer array (then one row per S)."""
    S = np.asarray(S, dtype=np.int64)
    lds_l = sum(ll) * LRF_CD * 4
    fits = {cand: (cand * S * 4 + lds_l) * (16 // cand) <= 156 * KB for cand in (4, 8, 16)}      # march_lds_rays:
    nw = np.where(fits[4], 4, np.where(fits[8], 8, np.where(fits[16], 16, 0)))                    # the smallest that fits,
    if rays in fits:
        nw = np.where(fits[rays], rays, nw)                                                       # or the hook's where it fits;
    if not lines:
        nw = 0 * nw                                                                               # none with the lines switched off
    group = np.where(nw > 0, nw, 4)                                                               # march_group_rays
    zlds = np.where(nw > 0, ((nw + 1) * S * 4 + lds_l) * (16 // group) <= 156 * KB, 5 * S * 4 <= 64 * KB)   # march_lds_z
    grid = (R + group - 1) // group                                                               # launch_march
    block = 64 * group
    lds = group * S * 4 + np.where(nw > 0, lds_l, 0) + np.where(zlds, S * 4, 0) + MARCH_LDS_TAIL
    lds_base = W32_ALL_U4 * 16 + S * 4                                                            # launch_shade3
    lds_toff = (R + 1) * 4 + R * 2 + 16
    in_lds = (lds_base + lds_toff + 64 <= 160 * KB - 256) & ((R + group - 1) // group <= 512 * TILE_GPT) & bool(toff)
    chunks = (R + PIPE_CHUNK - 1) // PIPE_CHUNK if R >= 2 * PIPE_CHUNK else 1                     # pipe_chunks
    cols = [nw, group, zlds, grid, block, lds, in_lds, lds_base + np.where(in_lds, lds_toff, 0), ~in_lds, chunks + 0 * S,
            np.where(nw > 0, 160 * KB, 64 * KB + MARCH_LDS_TAIL), 160 * KB - 256 + 0 * S]         # lds_opt_in's rows
    return np.stack([np.asarray(c, dtype=np.int64) for c in cols], axis=-1)


NAMES = ("nw", "group", "zlds", "march_grid", "march_block", "march_lds", "in_lds", "shade3_lds", "scan_tiles", "pipe_chunks",
         "march_opt_in", "shade3_opt_in")


def plan(lib, ll, R, S, sw):
    out = (C.c_int64 * 12)()
    rc = lib.lrf_debug_forward_plan((C.c_int32 * 3)(*ll), R, S, sw, out)
    assert rc == 0, (ll, R, S, sw, rc)
    return dict(zip(NAMES, (int(v) for v in out)))


def plan_sweep(lib, ll, R, sw, S_lo=2, S_hi=4096):
    """lrf_debug_forward_plan for every S in S_lo .. S_hi -> int64 [S_hi - S_lo + 1, 12]"""
    n = S_hi - S_lo + 1
    buf = (C.c_int64 * (12 * n))()
    c_ll, fn = (C.c_int32 * 3)(*ll), lib.lrf_debug_forward_plan
    base, ptr = C.addressof(buf), C.POINTER(C.c_int64)
    for i in range(n):
        if fn(c_ll, R, S_lo + i, sw, C.cast(base + 96 * i, ptr)):
            raise AssertionError((ll, R, S_lo + i, sw))
    return np.frombuffer(buf, dtype=np.int64).reshape(n, 12).copy()


# ------------------------------------------------------------------------------------------- 2. sizes and refusals
A = 0x10000
DET = N.LRF_FLAG_DETERMINISTIC

# (R, S, grid): smallest, odd, the sample counts of tests/test_gpu_forward_plan.py, bench.py's, R on both sides of the tile-offset
# bound and of two pipe chunks, beyond the sort limit
SHAPES = [(1, 2, (1, 1, 1)), (3, 5, (5, 7, 9)), (5, 1766, (48, 48, 48)), (33, 1768, (48, 48, 48)), (17, 1920, (96, 96, 96)),
          (4096, 512, (300, 300, 300)), (11399, 64, (48, 48, 48)), (11400, 64, (48, 48, 48)), (16384, 64, (48, 48, 48)), (32767, 64, (48, 48, 48)),
          (32768, 64, (48, 48, 48)), (40000, 96, (128, 128, 128)), (65537, 7, (64, 48, 32))]


def _i3(a, b, c):
    return (C.c_int32 * 3)(a, b, c)


def sizes(lib):
    out = {}
    for R, S, g in SHAPES:
        out[f"lrf_workspace_bytes({R},{S})"] = lib.lrf_workspace_bytes(R, S)
        out[f"lrf_normals_workspace_bytes({R},{S})"] = lib.lrf_normals_workspace_bytes(R, S)
        out[f"lrf_quantile_workspace_bytes({R},{S})"] = lib.lrf_quantile_workspace_bytes(R, S)
        for cfg in [(0, 0, 0, 0), (0, 0, 0, DET), (2, 2, 64, 0)]:
            out[f"lrf_workspace_bytes_bwd_cfg({R},{S},{g},{cfg})"] = lib.lrf_workspace_bytes_bwd_cfg(R, S, _i3(*g), *cfg)
        o = (C.c_uint64 * 9)()
        lib.lrf_workspace_layout_bwd(R, S, _i3(*g), o)
        out[f"lrf_workspace_layout_bwd({R},{S},{g})"] = [int(v) for v in o]
    return out


def _field(grid=(48, 48, 48), **kw):
    f = N.LrfField(cache=A, grid=_i3(*grid), weight_thres=1e-3, term_T=0.0)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


_WEIGHTS = dict(basis=A, w1=A, b1=A, w2=A, b2=A, w3=A, b3=A)


def _scene(fields, R=32, per_view=8, n_rf=None, floater=0.0, chunk=16, ws=A, ws_bytes=1, ray_ids=None, blend_w=A):
    """An lrf_scene_fwd call.  With the fused form chosen it is refused for its one-byte scene workspace; otherwise it goes on to
    lrf_scene_rays, which refuses the null ray_ids: either way before the first HIP call, and the text tells which."""
    keep = [f for f, _, _ in fields]
    arr = (N.LrfSceneField * len(fields))(*[N.LrfSceneField(C.pointer(f) if f is not None else None, A, S, flags, A)
                                            for f, S, flags in fields])
    n = len(fields) if n_rf is None else n_rf
    return (ray_ids, R, per_view, A, A, n, A, A, 64, 64, 0, arr, floater, chunk, blend_w, None, A, A, A, A, A, A, A, ws, ws_bytes, None), keep


def refusal_calls():
    """[(key, symbol, args)]"""
    Z = None
    q = (C.c_float * 1)(0.5)
    fwd = lambda f=None, R=4, S=8, flags=0, **kw: (C.byref(f if f is not None else _field(**kw)), A, A, R, S, flags, 0.0, A, A, Z, Z, A, Z)  # noqa: E731
    train = lambda R=4, S=8, flags=0, **kw: (C.byref(_field(**kw)), A, A, R, S, flags, A, A, A, Z)  # noqa: E731
    nrm = lambda R=4, S=8, flags=0, **kw: (C.byref(_field(**kw)), A, A, R, S, flags, 0.0, Z, 0, 0, A, Z, A, Z)  # noqa: E731
    qnt = lambda R=4, S=8, flags=0, **kw: (C.byref(_field(**kw)), A, A, R, S, flags, 0.0, q, 1, Z, 0, 0, A, Z, Z, Z, A, Z)  # noqa: E731
    c = [
        ("fwd null", "lrf_render_fwd", (Z, Z, Z, 0, 0, 0, 0.0, Z, Z, Z, Z, Z, Z)),
        ("fwd cache", "lrf_render_fwd", fwd(cache=None)),
        ("fwd R", "lrf_render_fwd", fwd(R=0)),
        ("fwd S low", "lrf_render_fwd", fwd(S=1)),
        ("fwd S high", "lrf_render_fwd", fwd(S=4097)),
        ("fwd flags", "lrf_render_fwd", fwd(flags=1 << 20)),
        ("fwd rows saved", "lrf_render_fwd", fwd(flags=N.LRF_FLAG_ROWS_SAVED)),
        ("fwd plane events", "lrf_render_fwd", fwd(flags=N.LRF_FLAG_PLANE_EVENTS)),
        ("fwd network", "lrf_render_fwd", fwd(fea_pe=7)),
        ("fwd featureC", "lrf_render_fwd", fwd(feature_c=257)),
        ("fwd weights", "lrf_render_fwd", fwd(fea_pe=2)),
        ("fwd f32 engine", "lrf_render_fwd", fwd(flags=N.LRF_FLAG_MLP_F32, fea_pe=2, **_WEIGHTS)),
        ("train null", "lrf_render_fwd_train", (Z, Z, Z, 0, 0, 0, Z, Z, Z, Z)),
        ("train R", "lrf_render_fwd_train", train(R=0)),
        ("train S", "lrf_render_fwd_train", train(S=2049)),
        ("train valu", "lrf_render_fwd_train", train(flags=N.LRF_FLAG_MLP_VALU)),
        ("train f32", "lrf_render_fwd_train", train(flags=N.LRF_FLAG_MLP_F32)),
        ("train flags", "lrf_render_fwd_train", train(flags=1 << 20)),
        ("train network", "lrf_render_fwd_train", train(view_pe=-1)),
        ("train weights", "lrf_render_fwd_train", train(view_pe=3)),
        ("normals null", "lrf_render_normals", (Z, Z, Z, 0, 0, 0, 0.0, Z, 0, 0, Z, Z, Z, Z)),
        ("normals S", "lrf_render_normals", nrm(S=4097)),
        ("normals flags", "lrf_render_normals", nrm(flags=1 << 20)),
        ("normals rows saved", "lrf_render_normals", nrm(flags=N.LRF_FLAG_ROWS_SAVED)),
        ("normals network", "lrf_render_normals", nrm(fea_pe=7)),
        ("normals weights", "lrf_render_normals", nrm(fea_pe=1)),
        ("quantiles null", "lrf_render_depth_quantiles", (Z, Z, Z, 0, 0, 0, 0.0, Z, 0, Z, 0, 0, Z, Z, Z, Z, Z, Z)),
        ("quantiles S", "lrf_render_depth_quantiles", qnt(S=1)),
        ("quantiles flags", "lrf_render_depth_quantiles", qnt(flags=1 << 20)),
        ("quantiles network", "lrf_render_depth_quantiles", qnt(feature_c=300)),
        ("quantiles f32 engine", "lrf_render_depth_quantiles", qnt(flags=N.LRF_FLAG_MLP_F32, view_pe=2, **_WEIGHTS)),
    ]
    two = lambda **kw: [(_field(**kw), 64, 0), (_field(**kw), 64, 0)]  # noqa: E731
    scene = [
        ("scene null", (Z, 0, 0, Z, Z, 0, Z, Z, 0, 0, 0, Z, 0.0, 0, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, 0, Z), None),
        ("scene n_rf 0", *_scene(two(), n_rf=0)),
        ("scene n_rf 65", *_scene(two(), n_rf=65)),
        ("scene per_view", *_scene(two(), R=33)),
        ("scene per_view 0", *_scene(two(), per_view=0)),
        ("scene field null", *_scene([(_field(), 64, 0), (None, 64, 0)])),
        ("scene field S", *_scene([(_field(), 64, 0), (_field(), 1, 0)])),
        ("scene field flags", *_scene([(_field(), 64, 1 << 20), (_field(), 64, 0)])),
        ("scene field network", *_scene([(_field(), 64, 0), (_field(fea_pe=9), 64, 0)])),
        # the fuse decision, one condition at a time: "scene workspace too small" = fused, lrf_scene_rays' refusal = field by field
        ("scene fused", *_scene(two())),
        ("scene fused four", *_scene(two() + two())),
        ("scene fused chunk 0", *_scene(two(), chunk=0)),
        ("scene fused ragged tail", *_scene(two(), R=40, chunk=16)),
        ("scene fused 640", *_scene(two(grid=(640, 640, 640)))),
        ("scene one field", *_scene(two()[:1])),
        ("scene no workspace", *_scene(two(), ws=None)),
        ("scene chunk 24", *_scene(two(), R=48, chunk=24)),
        ("scene R 0", *_scene(two(), R=0)),
        ("scene floater", *_scene(two(), floater=0.5)),
        ("scene S differs", *_scene([(_field(), 64, 0), (_field(), 66, 0)])),
        ("scene flags differ", *_scene([(_field(), 64, 0), (_field(), 64, N.LRF_FLAG_WHITE_BG)])),
        ("scene sorted", *_scene([(_field(), 64, N.LRF_FLAG_SORT_RAYS), (_field(), 64, N.LRF_FLAG_SORT_RAYS)])),
        ("scene valu", *_scene([(_field(), 64, N.LRF_FLAG_MLP_VALU), (_field(), 64, N.LRF_FLAG_MLP_VALU)])),
        ("scene generic network", *_scene([(_field(), 64, 0), (_field(fea_pe=2, **_WEIGHTS), 64, 0)])),
        ("scene grid differs", *_scene([(_field(), 64, 0), (_field(grid=(48, 48, 49)), 64, 0)])),
        ("scene weight_thres differs", *_scene([(_field(), 64, 0), (_field(weight_thres=2e-3), 64, 0)])),
        ("scene term_T differs", *_scene([(_field(), 64, 0), (_field(term_T=1e-4), 64, 0)])),
        ("scene 2000 no lines", *_scene(two(grid=(2000, 2000, 2000)))),
        ("scene 48 S 4096 no lines", *_scene([(_field(), 4096, 0), (_field(), 4096, 0)])),
        ("scene workspace fits", *_scene(two(), ws_bytes=1 << 40)),
    ]
    return c + [(key, "lrf_scene_fwd", args) for key, args, _keep in scene], [k for _, _, k in scene]


def refusals(lib):
    """{key: [return code, lrf_last_error text]}"""
    out = {}
    calls, keep = refusal_calls()
    for key, name, args in calls:
        C.memset(lib.lrf_error_slot(), 0, 1)
        rc = getattr(lib, name)(*args)
        out[key] = [int(rc), lib.lrf_last_error().decode()]
    del keep
    return out
