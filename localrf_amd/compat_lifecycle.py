"""Lifecycle of a LocalTensorfs scene, call-for-call compatible with the reference.

ATTRIBUTION.  This module restates, method by method, the host-side control flow of
`localTensoRF/local_tensorfs.py` of facebookresearch/localrf (MIT License, Copyright (c) Meta Platforms, Inc. and
affiliates): constructor state, `append_frame`, `append_rf`, `optimizer_step`, `optimizer_step_poses_only`,
`get_kwargs` / `save` / `load`, `get_dist_to_last_rf`, `get_reg_loss`.  A drop-in has to make the same decisions at the same
iteration counts and keep the same attribute and checkpoint names, so these methods follow the reference's structure
closely on purpose; each cites the lines it mirrors (relative to /root/reference/localTensoRF), and
`tests/test_gpu_training.py::test_trajectory_replay_vs_reference_golden` replays 30 iterations recorded from the reference
through them.  What is NOT here -- and shares nothing with the reference -- is everything that computes: the render
entry point (`scene.py`), the kernels behind it (`csrc/`), the fused optimiser (`optim.py`).

MI355X-first differences (results identical): finished fields stay resident in HBM (288 GB) instead of being parked
on the host (local_tensorfs.py:132); every per-frame Adam of one step runs in a single `lrf_adam_step` launch.
"""
import re

import math

import torch

from .field import AlphaGridMask, TensorVMSplit
from .optim import FusedAdam
from .rays import N_to_reso, mtx_to_sixD, sixD_to_mtx

_ADAM_BETAS = (0.9, 0.99)

# constructor arguments of local_tensorfs.LocalTensorfs that are kept verbatim, and the attribute each one is stored under
# (checkpoints written by get_kwargs / save round-trip through the same table)
_CTOR_ATTRS = (
    ("fov", "fov"), ("n_init_frames", "n_init_frames"), ("n_overlap", "n_overlap"),
    ("n_iters_per_frame", "n_iters_per_frame"), ("n_iters_reg", "n_iters_reg_per_frame"),
    ("lr_R_init", "lr_R_init"), ("lr_t_init", "lr_t_init"), ("lr_i_init", "lr_i_init"), ("lr_exposure_init", "lr_exposure_init"),
    ("rf_lr_init", "rf_lr_init"), ("rf_lr_basis", "rf_lr_basis"), ("lr_decay_target_ratio", "lr_decay_target_ratio"),
    ("N_voxel_list", "N_voxel_per_frame_list"), ("update_AlphaMask_list", "update_AlphaMask_per_frame_list"),
    ("lr_upsample_reset", "lr_upsample_reset"),
)


class SceneLifecycle(torch.nn.Module):
    def __init__(self, fov, n_init_frames, n_overlap, WH, n_iters_per_frame, n_iters_reg,
                 lr_R_init, lr_t_init, lr_i_init, lr_exposure_init, rf_lr_init, rf_lr_basis,
                 lr_decay_target_ratio, N_voxel_list, update_AlphaMask_list, camera_prior,
                 device, lr_upsample_reset, **tensorf_args):
        super().__init__()
        given = dict(locals())
        for arg, attr in _CTOR_ATTRS:                           # constructor argument -> attribute of the reference's name
            setattr(self, attr, given[arg])
        self.W, self.H = WH
        self.device = torch.device(device)
        self.camera_prior = camera_prior
        self.tensorf_args = tensorf_args
        self.is_refining = False
        # utils/utils.py:386 calls torch.cross without `dim`, which picks the FIRST axis of size 3:
        # for a batch of exactly 3 views that is the view axis, not xyz.  True reproduces the
        # reference result (checked against a reference-recorded golden); False = the cross product
        # the reference meant.  Only batches of exactly 3 views differ.
        self.reference_cross = True
        # data-parallel hook (localrf_amd/dist.py): called between backward and the optimiser steps of
        # optimizer_step with this module; None = single process, as the reference
        self.grad_sync = None
        # extension: True = focal() / center() are computed without a tape (the intrinsics' .grad is left alone).  The
        # reference always differentiates through them and reads the result only while it tunes the intrinsics
        # (local_tensorfs.py:218-222); a captured iteration sets this when they are not tuned
        self.freeze_intrinsics = False
        # lower bound of the rays per field call in forward (see there); 1 = chunk exactly as the reference
        self.min_chunk = 65536
        self.max_untaped_workspace = 1 << 30                    # ... unless that call's workspace would exceed this many bytes (scene.py)

        # schedule state until optimizer_step rescales it by the number of training frames (local_tensorfs.py:77-82)
        self.lr_factor, self.regularize = 1, True
        self.n_iters, self.n_iters_reg = n_iters_per_frame, n_iters_reg
        self.N_voxel_list, self.update_AlphaMask_list = N_voxel_list, update_AlphaMask_list

        # per-frame pose / exposure parameters, each with its own Adam (local_tensorfs.py:88-97)
        self.r_c2w = torch.nn.ParameterList()
        self.t_c2w = torch.nn.ParameterList()
        self.exposure = torch.nn.ParameterList()
        self.r_optimizers, self.t_optimizers, self.exp_optimizers = [], [], []
        self.pose_linked_rf = []
        self.blending_weights = torch.nn.Parameter(
            torch.ones([1, 1], device=self.device), requires_grad=False)
        for _ in range(n_init_frames):
            self.append_frame()

        if self.camera_prior is not None:                       # :99-104
            focal = self.camera_prior["transforms"]["fl_x"]
            focal *= self.W / self.camera_prior["transforms"]["w"]
        else:
            focal = self.W / math.tan(fov * math.pi / 180 / 2) / 2
        self.init_focal = torch.nn.Parameter(torch.Tensor([focal]).to(self.device))
        self.focal_offset = torch.nn.Parameter(torch.ones(1, device=device))
        self.center_rel = torch.nn.Parameter(0.5 * torch.ones(2, device=device))
        if lr_i_init > 0:
            self.intrinsic_optimizer = FusedAdam(
                [self.focal_offset, self.center_rel], betas=_ADAM_BETAS, lr=self.lr_i_init)

        self.tensorfs = torch.nn.ParameterList()
        self.rf_iter = []
        self.world2rf = torch.nn.ParameterList()
        self.append_rf()

    # ----------------------------------------------------------------- field / frame lifecycle
    def append_rf(self, n_added_frames=1):
        """Start a new local field centred on the last camera (local_tensorfs.py:116-146)."""
        self.is_refining = False
        if len(self.tensorfs) > 0:
            n_ov = min(n_added_frames, self.n_overlap, self.blending_weights.shape[0] - 1)
            ramp = 1 / n_ov + torch.arange(0, 1, 1 / n_ov)
            self.blending_weights.requires_grad = False
            self.blending_weights[-n_ov:, -1] = 1 - ramp
            fresh = torch.zeros_like(self.blending_weights[:, 0:1])
            fresh[-n_ov:, 0] = ramp
            self.blending_weights = torch.nn.Parameter(
                torch.cat([self.blending_weights, fresh], dim=1), requires_grad=False)
            world2rf = -self.t_c2w[-1].clone().detach()
            # reference parks the finished field on the CPU here (:132); with 288 GB of HBM it
            # stays resident.  Its optimiser is gone: drop its gradients (35-96 MB) with it.
            for p in self.tensorfs[-1].parameters():
                p.grad = None
            self.tensorfs[-1].drop_grads()
        else:
            world2rf = torch.zeros(3, device=self.device)
        self.tensorfs.append(TensorVMSplit(device=self.device, **self.tensorf_args))
        self.world2rf.append(world2rf.clone().detach())
        self.rf_iter.append(0)
        self.rf_optimizer = FusedAdam(
            self.tensorfs[-1].get_optparam_groups(self.rf_lr_init, self.rf_lr_basis), betas=_ADAM_BETAS,
            pack_field=self.tensorfs[-1])                        # the step refreshes the field's layout cache itself (lrf_adam_step_pack)

    def append_frame(self):
        """New frame initialised from the previous pose (local_tensorfs.py:148-177)."""
        if len(self.r_c2w) == 0:
            self.r_c2w.append(torch.eye(3, 2, device=self.device))
            self.t_c2w.append(torch.zeros(3, device=self.device))
            self.pose_linked_rf.append(0)
        else:
            self.r_c2w.append(mtx_to_sixD(sixD_to_mtx(self.r_c2w[-1].clone().detach()[None]))[0])
            self.t_c2w.append(self.t_c2w[-1].clone().detach())
            self.blending_weights = torch.nn.Parameter(
                torch.cat([self.blending_weights, self.blending_weights[-1:, :]], dim=0),
                requires_grad=False)
            self.pose_linked_rf.append(int(torch.nonzero(self.blending_weights[-1, :])[0]))
        self.exposure.append(torch.eye(3, 3, device=self.device))
        if self.camera_prior is not None:
            idx = len(self.r_c2w) - 1
            rel = self.camera_prior["rel_poses"][idx]
            last_r = sixD_to_mtx(self.r_c2w[-1].clone().detach()[None])[0]
            self.r_c2w[-1] = last_r @ rel[:3, :3]
            self.t_c2w[-1].data += last_r @ rel[:3, 3]
        self.r_optimizers.append(FusedAdam([self.r_c2w[-1]], betas=_ADAM_BETAS, lr=self.lr_R_init))
        self.t_optimizers.append(FusedAdam([self.t_c2w[-1]], betas=_ADAM_BETAS, lr=self.lr_t_init))
        self.exp_optimizers.append(
            FusedAdam([self.exposure[-1]], betas=_ADAM_BETAS, lr=self.lr_exposure_init))

    # ----------------------------------------------------------------- optimisation
    def _active_pose_ids(self):
        last = len(self.rf_iter) - 1
        if self.rf_iter[-1] >= self.n_iters:
            return []
        return [i for i, rf in enumerate(self.pose_linked_rf) if rf == last]

    def optimizer_step_poses_only(self, loss):
        """local_tensorfs.py:179-191."""
        ids = self._active_pose_ids()
        for i in ids:
            self.r_optimizers[i].zero_grad()
            self.t_optimizers[i].zero_grad()
        loss.backward()
        if ids:
            FusedAdam.step_many([o for i in ids for o in (self.r_optimizers[i], self.t_optimizers[i])])

    def optimizer_step(self, loss, optimize_poses):
        """One optimisation step of the current field, its linked poses/exposures and the
        intrinsics, plus the scheduled upsample / alpha-mask rebuild (local_tensorfs.py:193-290).  In three parts so that
        a captured iteration (localrf_amd/graph_step.py) can run the device work of the middle as one graph replay."""
        pose_ids, tune_intrinsics = self.step_begin(optimize_poses)
        loss.backward()
        if self.grad_sync is not None:          # data parallel: localrf_amd.dist.allreduce_grads(self)
            self.grad_sync(self)
        self.rf_optimizer.step()
        self.step_schedule()
        small = self.small_optimizers(pose_ids, optimize_poses, tune_intrinsics)
        if small:
            FusedAdam.step_many(small)          # :229-249, one launch for all of them
        return self.step_finish()

    def step_begin(self, optimize_poses, zero_grad=True):
        """The schedule bookkeeping and learning-rate decays ahead of the backward (local_tensorfs.py:193-228)."""
        it = self.rf_iter[-1]
        if it == 0:
            self.lr_factor = 1
            self.n_iters = self.n_iters_per_frame
            self.n_iters_reg = self.n_iters_reg_per_frame
        elif it == 1:
            n_train = (self.blending_weights[:, -1] > 0).sum()
            self.n_iters = int(self.n_iters_per_frame * n_train)
            self.n_iters_reg = int(self.n_iters_reg_per_frame * n_train)
            self.lr_factor = self.lr_decay_target_ratio ** (1 / self.n_iters)
            self.N_voxel_list = {int(k * n_train): v for k, v in self.N_voxel_per_frame_list.items()}
            self.update_AlphaMask_list = [int(u * n_train) for u in self.update_AlphaMask_per_frame_list]
        self.regularize = self.rf_iter[-1] < self.n_iters_reg

        def decay(opt):
            for grp in opt.param_groups:
                grp["lr"] *= self.lr_factor

        pose_ids = self._active_pose_ids()
        for i in pose_ids:
            if optimize_poses:
                decay(self.r_optimizers[i]); decay(self.t_optimizers[i])
                if zero_grad:
                    self.r_optimizers[i].zero_grad(); self.t_optimizers[i].zero_grad()
            if self.lr_exposure_init > 0:
                decay(self.exp_optimizers[i])
                if zero_grad:
                    self.exp_optimizers[i].zero_grad()
        tune_intrinsics = (self.lr_i_init > 0 and self.blending_weights.shape[1] == 1
                           and self.is_refining)
        if tune_intrinsics:
            decay(self.intrinsic_optimizer)
            if zero_grad:
                self.intrinsic_optimizer.zero_grad()
        if zero_grad:
            self.rf_optimizer.zero_grad()
        return pose_ids, tune_intrinsics

    def step_schedule(self):
        """Behind the field's Adam step: its decay while refining, the scheduled upsample and alpha-mask rebuild
        (local_tensorfs.py:245-266)."""
        if self.is_refining:
            for grp in self.rf_optimizer.param_groups:
                grp["lr"] *= self.lr_factor
        if self.rf_iter[-1] in self.N_voxel_list:               # :251-261
            reso = N_to_reso(self.N_voxel_list[self.rf_iter[-1]], self.tensorfs[-1].aabb)
            self.tensorfs[-1].upsample_volume_grid(reso)
            if self.lr_upsample_reset:
                self.rf_optimizer = FusedAdam(
                    self.tensorfs[-1].get_optparam_groups(self.rf_lr_init, self.rf_lr_basis),
                    betas=_ADAM_BETAS, pack_field=self.tensorfs[-1])
        if self.rf_iter[-1] in self.update_AlphaMask_list:      # :264-266
            self.tensorfs[-1].updateAlphaMask(tuple((self.tensorfs[-1].gridSize / 2).int().tolist()))

    def small_optimizers(self, pose_ids, optimize_poses, tune_intrinsics):
        small = []
        for i in pose_ids:
            if optimize_poses:
                small += [self.r_optimizers[i], self.t_optimizers[i]]
            if self.lr_exposure_init > 0:
                small.append(self.exp_optimizers[i])
        if tune_intrinsics:
            small.append(self.intrinsic_optimizer)
        return small

    def step_finish(self):
        if self.is_refining:
            self.rf_iter[-1] += 1
        return self.rf_iter[-1] >= self.n_iters - 1             # can_add_rf

    def get_kwargs(self):
        """local_tensorfs.py:301-324."""
        kw = {arg: getattr(self, attr) for arg, attr in _CTOR_ATTRS}
        kw.update(camera_prior=None, WH=(self.W, self.H))
        kw.update(self.tensorfs[0].get_kwargs())
        return kw

    def save(self, path):
        torch.save({"kwargs": self.get_kwargs(), "state_dict": self.state_dict()}, path)

    def load(self, state_dict):
        """Re-grow fields/frames to match a checkpoint, then load it (local_tensorfs.py:331-356)."""
        n_frames = 0
        for key in state_dict:
            if re.fullmatch(r"r_c2w.[0-9]*", key):
                n_frames += 1
            if re.fullmatch(r"tensorfs.[1-9][0-9]*.density_plane.0", key):
                pl = state_dict[key]
                ln = state_dict[f"{key[:-15]}density_line.0"]
                self.tensorf_args["gridSize"] = [pl.shape[2], pl.shape[3], ln.shape[2]]
                self.append_rf()
        for i in range(len(self.tensorfs)):
            if f"tensorfs.{i}.alphaMask.aabb" in state_dict:
                vol = state_dict[f"tensorfs.{i}.alphaMask.alpha_volume"].to(self.device)
                aabb = state_dict[f"tensorfs.{i}.alphaMask.aabb"].to(self.device)
                self.tensorfs[i].alphaMask = AlphaGridMask(self.device, aabb, vol)
        for _ in range(n_frames - len(self.r_c2w)):
            self.append_frame()
        self.blending_weights = torch.nn.Parameter(
            torch.ones_like(state_dict["blending_weights"]), requires_grad=False)
        self.load_state_dict(state_dict)

    def get_dist_to_last_rf(self):
        return torch.norm(self.t_c2w[-1] + self.world2rf[-1])

    def get_reg_loss(self, tvreg, TV_weight_density, TV_weight_app, L1_weight_inital):
        """local_tensorfs.py:361-375."""
        tv_loss, l1_loss = 0, 0
        if self.rf_iter[-1] < self.n_iters:
            sched = self.lr_factor ** self.rf_iter[-1]
            if TV_weight_density > 0:
                tv_loss += self.tensorfs[-1].TV_loss_density(tvreg).mean() * TV_weight_density * sched
            if TV_weight_app > 0:
                tv_loss += self.tensorfs[-1].TV_loss_app(tvreg).mean() * TV_weight_app * sched
            if L1_weight_inital > 0:
                l1_loss += self.tensorfs[-1].density_L1() * L1_weight_inital
        return tv_loss, l1_loss

