"""The calls behind tests/golden/host_helpers_parent.json: workspace sizes over a table of shapes and the refusals of the entry
points whose host side uses the shared helpers of csrc/lrf_host.inl.  tests/golden/make_golden_host_helpers.py records them
from a build of the commit before the helpers moved; tests/test_host_helpers_host.py replays them on the current build.

Every refusal here happens before the library touches HIP, so the pointers are made-up addresses: A is aligned to 256 bytes,
A + 1 to nothing.  What is dereferenced on the host (structs, pointer tables, length arrays) is real ctypes memory."""
import ctypes as C

from localrf_amd import _native as N

A = 0x10000
DET = N.LRF_FLAG_DETERMINISTIC


def _i3(a, b, c):
    return (C.c_int32 * 3)(a, b, c)


def sizes(lib):
    """{key: bytes}: every *_workspace_bytes whose layout goes through a Carver, and lrf_workspace_layout_bwd's offsets."""
    out = {}
    # (R, S): smallest legal, odd R * S (cidx ends off a dword, pieces off 256 bytes), bench.py's, a pipelined batch, refused / degenerate
    rs = [(1, 2), (3, 5), (7, 129), (4096, 512), (40000, 64), (0, 2), (1, 1), (1, 4097)]
    grids = [(1, 1, 1), (5, 7, 9), (300, 300, 300)]
    for R, S in rs:
        out[f"lrf_workspace_bytes({R},{S})"] = lib.lrf_workspace_bytes(R, S)
        out[f"lrf_normals_workspace_bytes({R},{S})"] = lib.lrf_normals_workspace_bytes(R, S)
        out[f"lrf_quantile_workspace_bytes({R},{S})"] = lib.lrf_quantile_workspace_bytes(R, S)
    for R, S in rs[:4]:
        for g in grids:
            out[f"lrf_workspace_bytes_bwd({R},{S},{g})"] = lib.lrf_workspace_bytes_bwd(R, S, _i3(*g))
            for cfg in [(0, 0, 0, 0), (0, 0, 0, DET), (2, 2, 64, 0), (2, 2, 64, DET), (0, 0, 128, N.LRF_FLAG_MLP_VALU), (6, 6, 256, DET)]:
                out[f"lrf_workspace_bytes_bwd_cfg({R},{S},{g},{cfg})"] = lib.lrf_workspace_bytes_bwd_cfg(R, S, _i3(*g), *cfg)
    for R, S, g in [(3, 5, (5, 7, 9)), (4096, 512, (300, 300, 300))]:
        o = (C.c_uint64 * 9)()
        lib.lrf_workspace_layout_bwd(R, S, _i3(*g), o)
        out[f"lrf_workspace_layout_bwd({R},{S},{g})"] = [int(v) for v in o]
    for B, n in [(1, 1), (3, 7), (5, 1000), (256, 1 << 20), (65535, 1), (0, 1), (65536, 1), (1, 0), (1, 1 << 31)]:
        out[f"lrf_select_workspace_bytes({B},{n})"] = lib.lrf_select_workspace_bytes(B, n)
    # (V, H, W): smallest, H * W = 1 with V = 1, odd, a frame of several chunks, the view limits, refused
    for V, H, W in [(1, 1, 1), (1, 3, 5), (3, 17, 31), (2, 270, 480), (64, 9, 9), (65, 9, 9), (32767, 1, 1), (0, 4, 4), (1, 0, 4), (1, 40000, 40000)]:
        out[f"lrf_flow_comparison_workspace_bytes({V},{H},{W})"] = lib.lrf_flow_comparison_workspace_bytes(V, H, W)
        out[f"lrf_depth_comparison_workspace_bytes({V},{H},{W})"] = lib.lrf_depth_comparison_workspace_bytes(V, H, W)
    for B, H, W, fs in [(1, 1, 1, 1), (1, 11, 11, 11), (3, 17, 31, 11), (2, 270, 480, 11), (1, 100, 100, 31), (0, 11, 11, 11), (1, 10, 11, 11), (1, 40, 40, 32),
                        (1, 20000, 20000, 11)]:
        out[f"lrf_image_metrics_workspace_bytes({B},{H},{W},{fs})"] = lib.lrf_image_metrics_workspace_bytes(B, H, W, fs)
    out["lrf_frame_sharpness_workspace_bytes()"] = lib.lrf_frame_sharpness_workspace_bytes()
    for V in [1, 3, 120, 1 << 24, 0, (1 << 24) + 1]:
        out[f"lrf_encode_frames_workspace_bytes({V})"] = lib.lrf_encode_frames_workspace_bytes(V)
    segs = (N.LrfTvSeg * 3)(N.LrfTvSeg(A, A, 1, 1, 1, 1.0), N.LrfTvSeg(A, A, 16, 97, 97, 1.0), N.LrfTvSeg(A, A, 48, 300, 1, 1.0))
    for count in (1, 2, 3, 0):
        out[f"lrf_tv_workspace({count})"] = lib.lrf_tv_workspace(segs, count)
    return out


def _window(**kw):
    w = N.LrfFrameWindow(rgb=A, loss_weight=A, slot_of=A, status=A, capacity=4, n_px=12, num_images=9)
    for k, v in kw.items():
        setattr(w, k, v)
    return C.byref(w)


def _metrics(**kw):
    m = N.LrfImageMetrics(img0=A, img1=A, B=1, H=16, W=16, filter_size=11, max_val=1.0, filter_sigma=1.5, k1=0.01, k2=0.03)
    for k, v in kw.items():
        setattr(m, k, v)
    return C.byref(m)


def _flowcmp(**kw):
    c = N.LrfFlowComparison(cam2world=A, depth=A, dirs=A, ij=A, fwd_flow=A, fwd_mask=A, bwd_flow=A, bwd_mask=A, focal=A, center=A,
                            F=4, V=2, H=3, W=5)
    for k, v in kw.items():
        setattr(c, k, v)
    return C.byref(c)


def _field(cache=A):
    return C.byref(N.LrfField(cache=cache))


def _ptrs(*v):
    return (N._f * len(v))(*v)


def _n64(*v):
    return (C.c_int64 * len(v))(*v)


def _f32(*v):
    return (C.c_float * len(v))(*v)


def _adam(*t):
    return (N.LrfAdamTensor * len(t))(*[N.LrfAdamTensor(*x) for x in t])


def refusal_calls():
    """[(key, symbol, args)]: for every entry point its all-null / all-zero call, then one call per further class of check
    (size, pairing, alignment, flag) where the refusal still comes before the first HIP call."""
    Z = None
    P3, T3 = _ptrs(A, A, A), _ptrs(A, A, A)
    tv1 = (N.LrfTvSeg * 1)(N.LrfTvSeg(A, None, 1, 2, 2, 1.0))
    terms = N.LrfLossTerms(count=1)
    q_ok, q_bad = _f32(0.5), _f32(0.0)
    c = [
        # lrf_scene.inl
        ("scene_rays null", "lrf_scene_rays", (Z, 0, 0, Z, Z, 0, Z, Z, 0, 0, 0, Z, Z, Z, Z)),
        ("scene_rays pinhole", "lrf_scene_rays", (A, 4, 2, A, A, 1, Z, Z, 4, 4, 0, A, A, A, Z)),
        ("scene_rays sizes", "lrf_scene_rays", (A, 4, 0, A, A, 1, A, A, 4, 4, 0, A, A, A, Z)),
        ("scene_rays multiple", "lrf_scene_rays", (A, 5, 2, A, A, 1, A, A, 4, 4, 0, A, A, A, Z)),
        ("scene_rays_bwd null", "lrf_scene_rays_bwd", (Z, 0, 0, Z, 0, Z, Z, 0, 0, 0, Z, Z, Z, Z, Z, Z)),
        ("scene_rays_bwd pinhole", "lrf_scene_rays_bwd", (A, 4, 2, A, 1, Z, A, 4, 4, 0, A, A, A, A, A, Z)),
        ("scene_rays_bwd sizes", "lrf_scene_rays_bwd", (A, 5, 2, A, 1, A, A, 4, 4, 0, A, A, A, A, A, Z)),
        ("scene_blend null", "lrf_scene_blend", (Z, Z, Z, Z, 0, 0, 0, Z, Z, Z, Z)),
        ("scene_blend sizes", "lrf_scene_blend", (A, A, A, Z, 5, 2, 1, A, A, Z, Z)),
        ("scene_blend_bwd null", "lrf_scene_blend_bwd", (Z, Z, Z, Z, Z, 0, 0, 0, Z, Z, Z, Z)),
        ("scene_blend_bwd sizes", "lrf_scene_blend_bwd", (A, A, A, A, Z, 4, 2, 0, A, A, Z, Z)),
        ("pose_assemble null", "lrf_pose_assemble", (Z, Z, 0, 0, Z, Z)),
        ("pose_assemble V", "lrf_pose_assemble", (P3, T3, 65, 0, A, Z)),
        ("pose_assemble row", "lrf_pose_assemble", (_ptrs(A, None, A), T3, 3, 0, A, Z)),
        ("pose_assemble cross", "lrf_pose_assemble", (P3, T3, 2, 1, A, Z)),
        ("pose_assemble_bwd null", "lrf_pose_assemble_bwd", (Z, 0, 0, Z, Z, Z, Z)),
        ("pose_assemble_bwd cross", "lrf_pose_assemble_bwd", (P3, 2, 1, A, A, A, Z)),
        # lrf_adam.inl
        ("adam_step count", "lrf_adam_step", (Z, -1, 0.9, 0.99, 1e-8, Z)),
        ("adam_step null", "lrf_adam_step", (Z, 1, 0.9, 0.99, 1e-8, Z)),
        ("adam_step tensor", "lrf_adam_step", (_adam((A, A, None, A, 4, 0.0, 0.0)), 1, 0.9, 0.99, 1e-8, Z)),
        ("adam_step large", "lrf_adam_step", (_adam((A, A, A, A, 2000000001, 0.0, 0.0)), 1, 0.9, 0.99, 1e-8, Z)),
        ("adam_step_dev null", "lrf_adam_step_dev", (Z, 0, Z, 0.9, 0.99, 1e-8, Z)),
        ("adam_step_dev count", "lrf_adam_step_dev", (Z, 65, A, 0.9, 0.99, 1e-8, Z)),
        ("adam_step_pack count", "lrf_adam_step_pack", (Z, -1, Z, 0.9, 0.99, 1e-8, Z, Z, Z)),
        ("adam_step_pack null", "lrf_adam_step_pack", (Z, 0, Z, 0.9, 0.99, 1e-8, Z, Z, Z)),
        # lrf_losses.inl
        ("upsample_bilinear", "lrf_upsample_bilinear", (Z, 0, 0, 0, Z, 0, 0, Z)),
        ("flow_loss_fwd", "lrf_flow_loss_fwd", (Z, Z, Z, Z)),
        ("flow_loss_bwd", "lrf_flow_loss_bwd", (Z, Z, Z, 0.0, Z, Z, Z, Z, Z, Z)),
        ("depth_loss_fwd", "lrf_depth_loss_fwd", (Z, Z, 0, 0, 0.0, Z, Z, Z, Z)),
        ("depth_loss_fwd per view", "lrf_depth_loss_fwd", (A, A, 2, 4097, 0.5, A, A, A, Z)),
        ("depth_loss_bwd", "lrf_depth_loss_bwd", (Z, Z, 0, 0, Z, Z, Z, 0.0, Z, Z)),
        ("photo_loss_fwd", "lrf_photo_loss_fwd", (Z, Z, Z, Z, 0, Z, Z, Z)),
        ("photo_loss_bwd", "lrf_photo_loss_bwd", (Z, Z, Z, Z, Z, 0, Z, Z)),
        ("rows_gather", "lrf_rows_gather", (Z, Z, 0, 0, 0, Z, Z)),
        ("rows_gather_bwd", "lrf_rows_gather_bwd", (Z, Z, 0, 0, 0, Z, Z)),
        ("batch_gather", "lrf_batch_gather", (Z, Z, Z, Z, Z, Z, Z, Z)),
        ("loss_combine_fwd", "lrf_loss_combine_fwd", (Z, Z, Z, Z)),
        ("loss_combine_fwd term", "lrf_loss_combine_fwd", (C.byref(terms), A, A, Z)),
        ("loss_combine_bwd", "lrf_loss_combine_bwd", (Z, Z, 0, Z, Z)),
        ("loss_combine_bwd count", "lrf_loss_combine_bwd", (A, A, 9, A, Z)),
        # lrf_metrics.inl
        ("image_metrics null", "lrf_image_metrics", (Z, Z, Z, Z, Z, Z)),
        ("image_metrics B", "lrf_image_metrics", (_metrics(B=65536), Z, A, A, A, Z)),
        ("image_metrics large", "lrf_image_metrics", (_metrics(H=20000, W=20000), Z, A, A, A, Z)),
        ("image_metrics fs", "lrf_image_metrics", (_metrics(filter_size=32, H=64, W=64), Z, A, A, A, Z)),
        ("image_metrics small", "lrf_image_metrics", (_metrics(H=10), Z, A, A, A, Z)),
        ("image_metrics sigma", "lrf_image_metrics", (_metrics(filter_sigma=0.0), Z, A, A, A, Z)),
        ("image_metrics finite", "lrf_image_metrics", (_metrics(k1=float("inf")), Z, A, A, A, Z)),
        ("image_metrics members", "lrf_image_metrics", (_metrics(img1=None), Z, A, A, A, Z)),
        ("image_metrics vanishing", "lrf_image_metrics", (_metrics(filter_size=2, filter_sigma=1e-200), Z, A, A, A, Z)),
        # lrf_frames.inl
        ("frames_gather null", "lrf_frames_gather", (Z, Z, Z, 0, 0, Z, Z, Z, Z, Z, Z, Z, Z)),
        ("frames_gather window", "lrf_frames_gather", (_window(capacity=0), A, A, 1, 1, A, A, Z, Z, Z, Z, Z, Z)),
        ("frames_gather planes", "lrf_frames_gather", (_window(fwd_flow=A), A, A, 1, 1, A, A, Z, Z, Z, Z, Z, Z)),
        ("frames_gather sizes", "lrf_frames_gather", (_window(), A, A, 0, 1, A, A, Z, Z, Z, Z, Z, Z)),
        ("frames_gather ids", "lrf_frames_gather", (_window(), Z, A, 1, 1, A, A, Z, Z, Z, Z, Z, Z)),
        ("frames_gather absent", "lrf_frames_gather", (_window(), A, A, 1, 1, A, A, A, Z, Z, Z, Z, Z)),
        ("decode_flow null", "lrf_decode_flow", (Z, 0, 0, Z, 0, 0, 0.0, Z)),
        ("decode_flow slot", "lrf_decode_flow", (_window(), 4, 0, A, 3, 4, 1.0, Z)),
        ("decode_flow shape", "lrf_decode_flow", (_window(), 0, 0, A, 3, 5, 1.0, Z)),
        ("decode_flow encoded", "lrf_decode_flow", (_window(), 0, 0, Z, 3, 4, 1.0, Z)),
        ("decode_flow planes", "lrf_decode_flow", (_window(), 0, 1, A, 3, 4, 1.0, Z)),
        ("decode_flow scale", "lrf_decode_flow", (_window(fwd_flow=A, fwd_mask=A), 0, 0, A, 3, 4, 1e300, Z)),
        ("frame_sharpness null", "lrf_frame_sharpness", (Z, 0, 0, 0, Z, Z, Z)),
        ("frame_sharpness slot", "lrf_frame_sharpness", (_window(), -1, 3, 4, Z, A, Z)),
        ("frame_sharpness shape", "lrf_frame_sharpness", (_window(), 0, 4, 4, Z, A, Z)),
        ("frame_sharpness pixels", "lrf_frame_sharpness", (_window(n_px=(1 << 21) + 1, capacity=1), 0, 1, (1 << 21) + 1, Z, A, Z)),
        ("frame_sharpness workspace", "lrf_frame_sharpness", (_window(), 0, 3, 4, Z, Z, Z)),
        # lrf_select.inl
        ("select null", "lrf_select", (Z, 0, Z, 0, 0, 0, 0.0, Z, Z, Z)),
        ("select B", "lrf_select", (A, 8, _n64(8), 1, 65536, 0, 0.5, A, A, Z)),
        ("select n_count", "lrf_select", (A, 8, _n64(8, 8), 2, 3, 0, 0.5, A, A, Z)),
        ("select rows", "lrf_select", (A, 8, _n64(*([8] * 257)), 257, 257, 0, 0.5, A, A, Z)),
        ("select n", "lrf_select", (A, 8, _n64(8, 0), 2, 2, 0, 0.5, A, A, Z)),
        ("select stride", "lrf_select", (A, -1, _n64(8), 1, 2, 0, 0.5, A, A, Z)),
        ("select mode", "lrf_select", (A, 8, _n64(8), 1, 2, 2, 0.5, A, A, Z)),
        ("select q", "lrf_select", (A, 8, _n64(8), 1, 2, 0, 1.5, A, A, Z)),
        # lrf_evalgeo.inl
        ("flow_comparison null", "lrf_flow_comparison", (Z, Z, Z, Z, Z, Z, Z, Z)),
        ("flow_comparison V", "lrf_flow_comparison", (_flowcmp(V=65), A, A, Z, Z, A, A, Z)),
        ("flow_comparison frame", "lrf_flow_comparison", (_flowcmp(H=0), A, A, Z, Z, A, A, Z)),
        ("flow_comparison F", "lrf_flow_comparison", (_flowcmp(F=0), A, A, Z, Z, A, A, Z)),
        ("flow_comparison idx", "lrf_flow_comparison", (_flowcmp(F=1, idx=(C.c_int32 * 64)(0, 1)), A, A, Z, Z, A, A, Z)),
        ("flow_comparison members", "lrf_flow_comparison", (_flowcmp(dirs=None), A, A, Z, Z, A, A, Z)),
        ("flow_comparison workspace", "lrf_flow_comparison", (_flowcmp(), A, A, Z, Z, A, Z, Z)),
        ("flow_comparison raw", "lrf_flow_comparison", (_flowcmp(), A, A, A, Z, A, A, Z)),
        ("depth_comparison zero", "lrf_depth_comparison", (Z, Z, 0, 0, 0, Z, Z, Z, Z)),
        ("depth_comparison frame", "lrf_depth_comparison", (A, A, 1, 40000, 40000, A, A, A, Z)),
        ("depth_comparison null", "lrf_depth_comparison", (A, Z, 1, 3, 5, A, A, A, Z)),
        # lrf_encode.inl
        ("encode_frames zero", "lrf_encode_frames", (Z, Z, 0, 0, 0, Z, Z, Z, Z, Z, Z, Z, Z)),
        ("encode_frames null", "lrf_encode_frames", (Z, A, 1, 2, 2, Z, Z, Z, A, Z, Z, A, Z)),
        ("encode_frames rgb", "lrf_encode_frames", (A, A, 1, 2, 2, A, Z, Z, A, Z, Z, A, Z)),
        ("encode_frames workspace", "lrf_encode_frames", (Z, A, 1, 2, 2, A, Z, Z, A, Z, Z, Z, Z)),
        ("encode_frames V", "lrf_encode_frames", (Z, A, (1 << 24) + 1, 1, 1, A, Z, Z, A, Z, Z, A, Z)),
        ("encode_frames align 16", "lrf_encode_frames", (Z, A + 4, 1, 2, 2, A, Z, Z, A, Z, Z, A, Z)),
        ("encode_frames align 4", "lrf_encode_frames", (Z, A, 1, 2, 2, A, Z, Z, A + 2, Z, Z, A, Z)),
        ("encode_frames align ws", "lrf_encode_frames", (Z, A, 1, 2, 2, A, Z, Z, A, Z, Z, A + 1, Z)),
        # lrf_reg.inl
        ("density_l1_fwd null", "lrf_density_l1_fwd", (Z, Z, Z, Z, 0.0, 0, Z, Z, Z)),
        ("density_l1_fwd lattice", "lrf_density_l1_fwd", (P3, T3, _i3(4, 6, 8), _i3(6, 4, 4), 0.0, 0, A, A, Z)),
        ("density_l1_bwd null", "lrf_density_l1_bwd", (Z, Z, Z, Z, Z, Z, Z, Z, Z)),
        ("density_l1_bwd lattice", "lrf_density_l1_bwd", (P3, T3, _i3(4, 6, 8), _i3(6, 4, 0), A, A, P3, T3, Z)),
        ("density_l1_bwd_acc null", "lrf_density_l1_bwd_acc", (Z, Z, Z, Z, Z, Z, Z, Z, Z)),
        ("tv_loss_fwd null", "lrf_tv_loss_fwd", (Z, 0, 0.0, Z, Z, Z)),
        ("tv_loss_fwd workspace", "lrf_tv_loss_fwd", (tv1, 1, 1.0, Z, A, Z)),
        ("tv_loss_bwd null", "lrf_tv_loss_bwd", (Z, 0, 0.0, Z, Z)),
        ("tv_loss_bwd gradient", "lrf_tv_loss_bwd", (tv1, 1, 1.0, A, Z)),
        # lrf_mask.inl
        ("dense_alpha null", "lrf_dense_alpha", (Z, Z, Z, Z, 0, 0, 0, 0.0, 0, Z, Z)),
        ("dense_alpha cache", "lrf_dense_alpha", (_field(None), A, A, A, 2, 2, 2, 1.0, 0, A, Z)),
        ("dense_alpha lattice", "lrf_dense_alpha", (_field(), A, A, A, 2, 0, 2, 1.0, 0, A, Z)),
        ("alpha_pool_threshold null", "lrf_alpha_pool_threshold", (Z, 0, 0, 0, 0.0, Z, Z)),
        ("alpha_pool_threshold lattice", "lrf_alpha_pool_threshold", (A, 2, 2, -1, 0.5, A, Z)),
        # lrf_normals.inl
        ("density_gradient null", "lrf_density_gradient", (Z, Z, 0, Z, Z, Z)),
        ("density_gradient P", "lrf_density_gradient", (_field(), A, -1, A, Z, Z)),
        ("density_gradient arrays", "lrf_density_gradient", (_field(), Z, 4, A, Z, Z)),
        ("density_gradient align", "lrf_density_gradient", (_field(), A, 4, A, A + 2, Z)),
        ("render_normals null", "lrf_render_normals", (Z, Z, Z, 0, 0, 0, 0.0, Z, 0, 0, Z, Z, Z, Z)),
        ("render_normals sizes", "lrf_render_normals", (_field(), A, A, 4, 1, 0, 0.0, Z, 0, 0, A, Z, A, Z)),
        ("render_normals per_view", "lrf_render_normals", (_field(), A, A, 4, 8, 0, 0.0, A, 0, 0, A, Z, A, Z)),
        ("render_normals accumulate", "lrf_render_normals", (_field(), A, A, 4, 8, 0, 0.0, Z, 0, 2, A, Z, A, Z)),
        ("render_normals align", "lrf_render_normals", (_field(), A, A, 4, 8, 0, 0.0, Z, 0, 0, A + 1, Z, A, Z)),
        ("render_normals align ws", "lrf_render_normals", (_field(), A, A, 4, 8, 0, 0.0, Z, 0, 0, A, Z, A + 128, Z)),
        ("render_normals flags", "lrf_render_normals", (_field(), A, A, 4, 8, 1 << 20, 0.0, Z, 0, 0, A, Z, A, Z)),
        # lrf_quantile.inl
        ("render_depth_quantiles null", "lrf_render_depth_quantiles", (Z, Z, Z, 0, 0, 0, 0.0, Z, 0, Z, 0, 0, Z, Z, Z, Z, Z, Z)),
        ("render_depth_quantiles sizes", "lrf_render_depth_quantiles", (_field(), A, A, 4, 4097, 0, 0.0, q_ok, 1, Z, 0, 0, A, Z, Z, Z, A, Z)),
        ("render_depth_quantiles K", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 5, Z, 0, 0, A, Z, Z, Z, A, Z)),
        ("render_depth_quantiles q", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_bad, 1, Z, 0, 0, A, Z, Z, Z, A, Z)),
        ("render_depth_quantiles per_view", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, A, 0, 0, A, A, Z, Z, A, Z)),
        ("render_depth_quantiles accumulate", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, Z, 0, 3, A, Z, Z, Z, A, Z)),
        ("render_depth_quantiles index", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, Z, 0, 1, A, Z, A, Z, A, Z)),
        ("render_depth_quantiles wsum", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, A, 2, 0, A, Z, Z, Z, A, Z)),
        ("render_depth_quantiles align", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, Z, 0, 0, A, Z, A + 2, Z, A, Z)),
        ("render_depth_quantiles align ws", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 0, 0.0, q_ok, 1, Z, 0, 0, A, Z, Z, Z, A + 64, Z)),
        ("render_depth_quantiles flags", "lrf_render_depth_quantiles", (_field(), A, A, 4, 8, 1 << 20, 0.0, q_ok, 1, Z, 0, 0, A, Z, Z, Z, A, Z)),
        ("depth_quantiles_from_weights null", "lrf_depth_quantiles_from_weights", (Z, Z, Z, 0, 0, Z, 0, Z, Z, Z)),
        ("depth_quantiles_from_weights sizes", "lrf_depth_quantiles_from_weights", (A, A, A, 0, 8, q_ok, 1, A, Z, Z)),
        ("depth_quantiles_from_weights K", "lrf_depth_quantiles_from_weights", (A, A, A, 4, 8, q_ok, 0, A, Z, Z)),
        ("depth_quantiles_from_weights q", "lrf_depth_quantiles_from_weights", (A, A, A, 4, 8, q_bad, 1, A, Z, Z)),
        ("depth_quantiles_from_weights align", "lrf_depth_quantiles_from_weights", (A, A, A + 3, 4, 8, q_ok, 1, A, Z, Z)),
    ]
    return c


# Left out, because the commit the golden file was recorded from does not refuse them on the host:
#   lrf_adam_step(count = 0), lrf_scene_*(R = 0), lrf_density_gradient(P = 0): return 0 without a launch;
#   lrf_adam_step_pack's per-tensor checks, lrf_density_l1_bwd's "null gradient pointer" and lrf_density_l1_workspace: reached
#   only behind make_layout / device_cus(), which asks HIP for the device.
def refusals(lib):
    """{key: [return code, lrf_last_error text]}"""
    out = {}
    for key, name, args in refusal_calls():
        C.memset(lib.lrf_error_slot(), 0, 1)
        rc = getattr(lib, name)(*args)
        out[key] = [int(rc), lib.lrf_last_error().decode()]
    return out
