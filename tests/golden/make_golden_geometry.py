"""Generate tests/golden/eval_geometry.npz: the reference's own test-view geometry diagnostics -- the flow and depth
comparison images renderer.render(test=True) returns (renderer.py:79-124) -- on a small seeded blended LocalTensorfs on
the CPU.  Runs only where the reference tree is present (make_golden.import_reference); the file it writes is what travels.
Usage:  python tests/golden/make_golden_geometry.py

The reference's renderer.render runs unchanged with minimal stand-in datasets whose flows, masks, inverse depths and
images are already at W x H, so cv2.resize is an identity.  visualize_depth and draw_poses (not part of this diagnostic)
and imageio (never called: no video) are stubbed.  LocalTensorfs.forward is wrapped to record depth_map, directions and ij
of each rendered view.  Stored per view k (keys "v{k}."): idx, depth [HW], dirs [HW,3], ij [HW,2] (int32: pixel coordinates),
fwd_flow / bwd_flow [H,W,2], fwd_mask / bwd_mask [H,W], invdepth [H,W] and the reference's fwd_cmp / bwd_cmp [3H,2W] and
depth_cmp [3H,W]; shared: cam2world [F,3,4], focal, center, W, H.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

W, H = 64, 48
SEED = 31


def build_scene(LocalTensorfs):
    """case_local's blended scene at 64 x 48: 14 frames over 4 fields, poses and exposures perturbed."""
    torch.manual_seed(SEED)
    aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    lt = make_golden.quiet(LocalTensorfs, fov=85.6, n_init_frames=5, n_overlap=3, WH=(W, H),
                           n_iters_per_frame=600, n_iters_reg=100, lr_R_init=5e-3, lr_t_init=5e-4,
                           lr_i_init=0, lr_exposure_init=1e-3, rf_lr_init=0.02, rf_lr_basis=1e-3,
                           lr_decay_target_ratio=0.1, N_voxel_list={}, update_AlphaMask_list=[],
                           camera_prior=None, device="cpu", lr_upsample_reset=True,
                           aabb=aabb, gridSize=[16, 16, 16], **make_golden.FIELD_KW)
    g = torch.Generator().manual_seed(SEED + 1)
    for _ in range(3):
        for _ in range(3):
            make_golden.quiet(lt.append_frame)
            with torch.no_grad():
                lt.t_c2w[-1].add_(0.05 * torch.randn(3, generator=g))
                lt.r_c2w[-1].add_(0.05 * torch.randn(3, 2, generator=g))
                lt.exposure[-1].add_(0.05 * torch.randn(3, 3, generator=g))
        make_golden.quiet(lt.append_rf, 3)
    with torch.no_grad():
        for f in lt.tensorfs:
            for p in f.density_plane:
                p.mul_(3.0)
    return lt


class _Train:
    def __init__(self, F):
        self.all_fbases = {f"{i:06d}": i for i in range(F)}

    def get_frame_fbase(self, idx):
        return f"{idx:06d}"


class _Test:
    """The test split at W x H: rgbs, flows (pixels), 0/1 masks and inverse depths from a seeded generator."""
    def __init__(self, ids, seed):
        rng = np.random.default_rng(seed)
        n = len(ids)
        self.all_fbases = {f"{i:06d}": k for k, i in enumerate(ids)}
        self.all_rgbs = rng.random((n, H, W, 3), dtype=np.float32)
        self.all_fwd_flow = (3.0 * rng.standard_normal((n, H, W, 2))).astype(np.float32)
        self.all_bwd_flow = (3.0 * rng.standard_normal((n, H, W, 2))).astype(np.float32)
        self.all_fwd_mask = (rng.random((n, H, W)) < 0.8).astype(np.float32)
        self.all_bwd_mask = (rng.random((n, H, W)) < 0.8).astype(np.float32)
        self.all_invdepths = (0.2 + rng.random((n, H, W))).astype(np.float32)


def main():
    _, _, LocalTensorfs = make_golden.import_reference()
    sys.modules["imageio"] = types.ModuleType("imageio")
    cv2 = sys.modules["cv2"]
    cv2.INTER_NEAREST = 0
    cv2.resize = lambda img, size, interpolation=None: img          # every input is already at W x H
    import renderer                                                    # the reference's own module
    renderer.visualize_depth = lambda depth, minmax=None: (torch.zeros(3, *depth.shape), None)
    renderer.draw_poses = lambda poses, colours: np.zeros((H, W, 3), np.uint8)

    lt = build_scene(LocalTensorfs)
    F = len(lt.r_c2w)
    test_ids = [3, 8, F - 1]                                           # the last frame: its forward neighbour clamps
    test = _Test(test_ids, SEED + 2)
    rec, calls = {}, []
    fwd = lt.forward

    def recording_forward(*a, **k):
        out = fwd(*a, **k)
        calls.append([t.detach().clone() for t in out[1:]])
        return out
    lt.forward = recording_forward
    args = types.SimpleNamespace(batch_size=4096, device="cpu")
    poses = lt.get_cam2world().detach()
    with torch.no_grad():
        _, _, _, fwd_tb, bwd_tb, depth_tb, _ = renderer.render(test, poses, lt, args, W=W, H=H, test=True,
                                                                 train_dataset=_Train(F), add_frame_to_list=True)
    assert len(calls) == len(test_ids) == len(fwd_tb) == len(depth_tb)
    for k, idx in enumerate(test_ids):
        depth, dirs, ij = calls[k]
        rec[f"v{k}.idx"] = np.int64(idx)
        rec[f"v{k}.depth"] = depth.numpy().astype(np.float32)
        rec[f"v{k}.dirs"] = dirs.numpy().astype(np.float32)
        assert int(ij.abs().max()) < 2 ** 31
        rec[f"v{k}.ij"] = ij.numpy().astype(np.int32)
        rec[f"v{k}.fwd_flow"], rec[f"v{k}.bwd_flow"] = test.all_fwd_flow[k], test.all_bwd_flow[k]
        rec[f"v{k}.fwd_mask"], rec[f"v{k}.bwd_mask"] = test.all_fwd_mask[k], test.all_bwd_mask[k]
        rec[f"v{k}.invdepth"] = test.all_invdepths[k]
        rec[f"v{k}.fwd_cmp"] = fwd_tb[k].numpy()
        rec[f"v{k}.bwd_cmp"] = bwd_tb[k].numpy()
        rec[f"v{k}.depth_cmp"] = depth_tb[k].numpy()
        print(f"view {idx}: fwd_cmp {tuple(fwd_tb[k].shape)} {fwd_tb[k].dtype} depth_cmp {tuple(depth_tb[k].shape)}")
    rec["views"] = np.int64(len(test_ids))
    rec["cam2world"] = poses.numpy()
    rec["focal"] = np.float32(lt.focal(W).detach().reshape(-1)[0])
    rec["center"] = lt.center(W, H).detach().reshape(-1).numpy().astype(np.float32)
    rec["W"], rec["H"] = np.int64(W), np.int64(H)
    rec["meta"] = np.array(f"reference renderer.render(test=True); numpy {np.__version__}; torch {torch.__version__}; seed {SEED}")
    path = os.path.join(HERE, "eval_geometry.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
