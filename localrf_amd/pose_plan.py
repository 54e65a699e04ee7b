"""The one owner of a render along a list of camera poses: which training frame each pose borrows its blending weights from,
which consecutive frames share an active set and render together, and what a group of them hands to the field kernels.

  check_poses(poses)                    [N, 3, 4] (or [N, 4, 4]) camera-to-world matrices -> [N, 3, 4]
  nearest_frames(local_tensorfs, poses) the training frame each pose borrows its blending weights from (renderer.py:47-53)
  PosePlan(local_tensorfs, poses, ...)  the frames, their groups and the inputs of every group

A new pose-path map builds a PosePlan (host only: every argument is checked and nothing is launched), calls on_device(),
allocates its outputs and loops over plan.calls, taking a group's inputs from group_inputs or its per-field calls from
group_spans.  novel_views.render_poses, normals.render_normals and depth_quantiles.render_depth_quantiles are that loop.
Cited lines are relative to the reference's localTensoRF directory.
"""
import numpy as np
import torch

from . import _native as N
from .scene_ops import scene_forward, scene_rays


def check_poses(poses):
    if not torch.is_tensor(poses):
        poses = torch.as_tensor(np.asarray(poses, dtype=np.float32))
    if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
        raise ValueError(f"poses must be [N, 3, 4] (or [N, 4, 4]) camera-to-world matrices, got {tuple(poses.shape)}")
    if not poses.is_floating_point():
        raise ValueError(f"poses must hold floating-point values, got {poses.dtype}")
    return poses[:, :3, :]


def nearest_frames(local_tensorfs, poses):
    """renderer.py:47-53 for all N poses at once: LongTensor [N], argmin_f |t_c2w[f] - pose[:, 3]| (first index on ties; a
    NaN distance wins, as torch.argmin has it), on the scene's device.  No read-back."""
    poses = check_poses(poses)
    t = torch.stack([p.detach() for p in local_tensorfs.t_c2w], dim=0)
    if poses.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=t.device)
    dist = torch.norm(t[None] - poses.to(device=t.device, dtype=t.dtype)[:, None, :, 3], dim=-1)
    return torch.argmin(dist, dim=1)


class PosePlan:
    """Construction checks everything on the host and launches nothing, on a CPU scene too:
      lt, W, H, chunk   as given (W, H, chunk as ints)
      poses [n, 3, 4]   the poses of the rendered frames, where the caller keeps them
      views, is_test    per frame, lists: its nearest training frame and whether that frame is a test frame
      groups            [(i0, i1, active)]: consecutive frames with one active set, at most frames_per_call of them
      n                 the number of frames
    start is the reference's (novel_views.render_poses describes it).  on_device() adds dev, cam2world [n, 3, 4] and vids [n]
    on the scene's device, calls (groups cut to what the scene's max_untaped_workspace allows) and, when asked, exposure."""

    def __init__(self, local_tensorfs, poses, W, H, test_frames=(), frame_indices=None, start=0, frames_per_call=None, chunk=4096):
        if int(chunk) < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        W, H = int(W), int(H)
        if W <= 0 or H <= 0:
            raise ValueError(f"need W, H > 0, got {W} x {H}")
        if frames_per_call is not None and int(frames_per_call) < 1:
            raise ValueError(f"frames_per_call must be >= 1, got {frames_per_call}")
        start = int(start)
        if start < 0:
            raise ValueError(f"start must be >= 0, got {start}")
        poses = check_poses(poses)[start:]                          # renderer.py:45: poses_mtx = poses_mtx[start:]
        n = max(0, int(poses.shape[0]) - start)                     # renderer.py:46: idxs = range(start, len(poses_mtx))
        F = len(local_tensorfs.r_c2w)
        if frame_indices is None:
            frame_indices = nearest_frames(local_tensorfs, poses) if n else []
        fi = frame_indices.tolist() if hasattr(frame_indices, "tolist") else list(frame_indices)   # one read-back per path
        if n and len(fi) < start + n:
            raise ValueError(f"frame_indices holds {len(fi)} entries; frame i uses frame_indices[start + i] up to {start + n - 1}")
        views = [int(v) for v in fi[start:start + n]]               # renderer.py:60-63: view_ids = frame_indices[idx]
        for i, v in enumerate(views):
            if not 0 <= v < F:
                raise ValueError(f"frame {i}: frame index {v} lies outside [0, {F})")
        tests = set(int(t) for t in test_frames)
        bw = local_tensorfs._blending_host()
        groups = []
        for i, v in enumerate(views):
            active = tuple(torch.nonzero(bw[v])[:, 0].tolist())
            if not active:                                          # the reference's forward returns a 5-tuple there and
                raise ValueError(f"frame {i}: its nearest frame {v} has no active field (no blending weight)")   # renderer.py:65 fails
            if groups and groups[-1][2] == active and (frames_per_call is None or i - groups[-1][0] < int(frames_per_call)):
                groups[-1][1] = i + 1
            else:
                groups.append([i, i + 1, active])
        self.lt, self.W, self.H, self.chunk, self.n = local_tensorfs, W, H, int(chunk), n
        self.poses, self.views, self.groups = poses[:n], views, groups
        self.is_test = [v in tests for v in views]                  # renderer.py:47,74: is_test_id[view_ids.item()]

    def on_device(self, exposure=False):
        """The device half: refuses a CPU scene, cuts the groups to the workspace cap and uploads poses and view ids; with
        exposure, each frame's own 3x3 colour transform or -- for a test frame -- its neighbours' mean (local_tensorfs.py:
        481-496, test_id chosen per frame).  Returns self."""
        lt, W, H = self.lt, self.W, self.H
        N.require_gpu(lt.blending_weights, "the scene", "rendering")
        self.dev = dev = lt.blending_weights.device
        # frames per call: bounded by frames_per_call (in groups) and by the scene's max_untaped_workspace over the per-call ray
        # buffers of lrf_scene_fwd (rays, per-field colour and depth, directions, ij, blended colour and depth: 40 n_rf + 44 B)
        cap = max(1, int(lt.max_untaped_workspace) // (W * H * (40 * max(len(g[2]) for g in self.groups) + 44))) if self.groups else 1
        self.calls = [(j, min(i1, j + cap), active) for i0, i1, active in self.groups for j in range(i0, i1, cap)]
        self.cam2world = self.poses.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.vids = torch.tensor(self.views, dtype=torch.int64).to(dev, non_blocking=True)
        self.exposure = None
        if exposure and lt.lr_exposure_init > 0 and self.views:
            with torch.no_grad():
                own = lt._exposure_for(self.vids, False)
                borrowed = lt._exposure_for(self.vids, True)
                mask = torch.tensor(self.is_test, dtype=torch.bool).to(dev, non_blocking=True)
                self.exposure = torch.where(mask[:, None, None], borrowed, own).contiguous()
        return self

    def group_inputs(self, i0, i1, active):
        """What frames i0..i1 (one active set) hand to the kernels: (fields, resident on the scene's device; shifts [n_active, 3];
        focal; center; fov360; ray_ids [V H W]; blend_w [V, n_active])."""
        lt, W, H = self.lt, self.W, self.H
        fields = [lt.tensorfs[rf] for rf in active]
        for f in fields:
            if f.device != self.dev:
                f.to(self.dev)
        pinhole = lt.fov != 360
        ray_ids = torch.arange((i1 - i0) * W * H, dtype=torch.int64, device=self.dev)
        return (fields, lt._shifts(lt.world2rf, list(active)), lt.focal(W) if pinhole else None,
                lt.center(W, H) if pinhole else None, not pinhole, ray_ids,
                lt._active_columns(lt.blending_weights[self.vids[i0:i1]], list(active)))

    def render_colour(self, i0, i1, active, floater_thresh):
        """Frames i0..i1 (one active set) in one lrf_scene_fwd call: what LocalTensorfs.forward(ray_ids, [view], W, H,
        is_train=False, cam2world=pose[None], test_id=...) computes for each of them -> (rgb [V H W, 3], depth [V H W])."""
        lt, W, H = self.lt, self.W, self.H
        fields, shifts, focal, center, fov360, ray_ids, bw = self.group_inputs(i0, i1, active)
        per_field = max(1, self.chunk // len(active))
        return scene_forward(ray_ids, self.cam2world[i0:i1], shifts, focal, center, W * H, W, H, fov360, fields, True, floater_thresh,
                             lt._untaped_chunk(per_field, fields), bw, None if self.exposure is None else self.exposure[i0:i1],
                             refine=lt.is_refining)[:2]

    def group_spans(self, i0, i1, active):
        """The per-field calls of frames i0..i1 (one active set): yields (r0, r1, calls) per span of rays, calls = [(f, z, flags,
        rays [r1 - r0, 6], blend_w)] over the active fields in the reference's field order, blend_w being the field's weights
        from the span's first view on (per_view = H W).  A span holds whole views when chunk covers one, else part of a single
        view."""
        V, HW, chunk = i1 - i0, self.W * self.H, self.chunk
        fields, shifts, focal, center, fov360, ray_ids, bw = self.group_inputs(i0, i1, active)
        rays, _, _ = scene_rays(ray_ids, self.cam2world[i0:i1], shifts, focal, center, HW, self.W, self.H, fov360)
        bw = N.conform(bw.t())                                      # [n_active, V]: a field's weights are one contiguous row
        per_field = []
        for f in fields:
            z = f.z_schedule(False, -1, self.dev).detach().contiguous().float().view(-1)
            flags = f._flags(True) | (N.LRF_FLAG_PE_OFF if (f.fea_pe > 0 and not self.lt.is_refining) else 0)
            per_field.append((f, z, flags))
        if chunk >= HW:                                             # whole views per call
            step = (chunk // HW) * HW
            spans = [(r0, min(V * HW, r0 + step)) for r0 in range(0, V * HW, step)]
        else:                                                       # a call never crosses a view: one blend weight per call
            spans = [(v * HW + r0, v * HW + min(HW, r0 + chunk)) for v in range(V) for r0 in range(0, HW, chunk)]
        for r0, r1 in spans:
            yield r0, r1, [(f, z, flags, rays[k, r0:r1], bw[k, r0 // HW:]) for k, (f, z, flags) in enumerate(per_field)]
