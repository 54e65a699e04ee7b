"""Shared pieces of the novel-view tests: numpy restatements of the frame encoding (cv2.imwrite's byte conversion and the
index image of utils/utils.py:visualize_depth in numpy 2.2's float32 arithmetic), the scene of tests/golden/novel_views.npz
and edge-case frames."""
import numpy as np
import torch

from util import FIELD_KW, load_golden


def rgb8_host(rgb):
    """cv2.imwrite(255 * rgb): saturate_cast<uchar>(fp32(255 * x)) = clip(rint(.), 0, 255), ties to even; NaN -> 0."""
    v = np.float32(255) * np.asarray(rgb, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), 0, np.clip(np.rint(v), 0, 255)).astype(np.uint8)


def depth_idx_host(depth, minmax):
    """The uint8 image visualize_depth hands to cv2.applyColorMap, for one frame [H, W] (numpy 2.2, float32):
    x = nan_to_num(d); minmax None: mi = min(x[x > 0]) (ValueError when empty), ma = max(x), D = fp32(fp32(ma - mi) + 1e-8);
    else D = fp32(fp64(ma - mi) + 1e-8) and mi rounded to fp32; uint8(fp32(255 * clip(fp32(x - mi) / D, 0, 1))), NaN -> 0.
    Returns (idx, (mi, ma))."""
    x = np.nan_to_num(np.asarray(depth, np.float32))
    if minmax is None:
        pos = x[x > 0]
        if pos.size == 0:
            raise ValueError("no positive depth")
        mi, ma = np.float32(pos.min()), np.float32(x.max())
        D = np.float32(np.float32(ma - mi) + np.float32(1e-8))
    else:
        mi, ma = np.float32(minmax[0]), np.float32(minmax[1])
        D = np.float32(float(minmax[1]) - float(minmax[0]) + 1e-8)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - mi) / D
        s = np.float32(255) * np.clip(t, np.float32(0), np.float32(1))
        idx = np.where(np.isnan(s), 0, s).astype(np.uint8)
    return idx, (mi, ma)


def depth_idx_frames(depth, minmax):
    """depth_idx_host over frames [V, H, W] -> (idx [V,H,W], ranges [V,2])."""
    out = [depth_idx_host(d, minmax) for d in np.asarray(depth, np.float32)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float32)


def edge_depths(rng, V, H, W):
    """Frames with NaN, +-inf, zeros, negatives, exact ties of the [0, 5] mapping, and huge values."""
    d = rng.uniform(-0.5, 6.0, (V, H, W)).astype(np.float32)
    flat = d.reshape(V, -1)
    n = flat.shape[1]
    for v in range(V):
        k = rng.permutation(n)[:max(8, n // 10)]
        specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5.0, 2.5, np.float32(5.0) * np.float32(100.5 / 255),
                             3e38, -3e38, 1e-40, 5.0 / 255], np.float32)
        flat[v, k] = specials[rng.integers(0, specials.size, k.size)]
    return d


def edge_rgbs(rng, V, H, W):
    """Colours in and around [0, 1] with NaN, +-inf and exact .5 ties of 255 x."""
    x = rng.uniform(-0.2, 1.2, (V, H, W, 3)).astype(np.float32)
    flat = x.reshape(-1)
    k = rng.permutation(flat.size)[:flat.size // 5]
    ties = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    specials = np.concatenate([ties, np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1e9, -1e9], np.float32)])
    flat[k] = specials[rng.integers(0, specials.size, k.size)]
    return x


def golden():
    return load_golden("novel_views")


def gap_case(device):
    """scene(device) with the blending weights of two training frames overwritten so that their active fields are not
    adjacent, (0, 2) and (1, 3), and three poses through them: the two frames' own and the first shifted by 0.05.
    Returns (lt, poses [3,3,4], views, W, H, test frames)."""
    lt, g = scene(device)
    views = [2, 6, 2]
    with torch.no_grad():                                       # in place: _version moves and the host mirror refreshes
        lt.blending_weights[2] = torch.tensor([0.25, 0.0, 0.75, 0.0])
        lt.blending_weights[6] = torch.tensor([0.0, 0.5, 0.0, 0.5])
        poses = lt.get_cam2world().detach()[views].clone()
    poses[2, :, 3] += 0.05
    assert [tuple(torch.nonzero(lt._blending_host()[v])[:, 0].tolist()) for v in views] == [(0, 2), (1, 3), (0, 2)]
    return lt, poses, views, 24, 16, g["test_frames"].tolist()


def scene(device):
    """Our LocalTensorfs holding the golden's scene (make_golden_geometry.build_scene, lr_exposure_init > 0): the four fields
    regenerated from the seed (3 x (3 frames, 1 field), density planes x 3) and checked against the reference's checksum,
    then the recorded poses, exposures, blending weights and world2rf loaded on top."""
    from localrf_amd import LocalTensorfs
    from util import quiet, state_checksum
    g = golden()
    torch.manual_seed(int(g["seed"]))
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    lt = quiet(LocalTensorfs, fov=85.6, n_init_frames=5, n_overlap=3, WH=tuple(int(v) for v in g["scene_WH"]),
               n_iters_per_frame=600, n_iters_reg=100, lr_R_init=5e-3, lr_t_init=5e-4,
               lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
               lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[],
               camera_prior=None, device="cpu", lr_upsample_reset=True,
               aabb=aabb, gridSize=[16, 16, 16], **FIELD_KW)
    for _ in range(3):
        for _ in range(3):
            quiet(lt.append_frame)
        quiet(lt.append_rf, 3)
    sd = lt.state_dict()
    small = {k[3:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items() if k.startswith("lt.")}
    assert sorted(small) == sorted(k for k in sd if not k.startswith("tensorfs.")), "scene layout differs from the golden's"
    with torch.no_grad():
        for k, v in small.items():
            assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
            sd[k].copy_(v)
        for f in lt.tensorfs:
            for p in f.density_plane:
                p.mul_(3.0)
    got = state_checksum({k: v for k, v in lt.state_dict().items() if k.startswith("tensorfs.")})
    want = float(g["field_sum"][0])
    assert abs(got - want) <= 1e-6 * want, ("seeded fields differ from the reference's", got, want)
    if str(device) != "cpu":
        lt = lt.to(device)
        lt.device = torch.device(device)
        for f in lt.tensorfs:
            f.to(device)
    return lt, g
