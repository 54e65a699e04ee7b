"""A device-resident frame window: the train split of LocalRFDataset (dataLoader/localrf_dataset.py) for the fast loop.

  DeviceFrames(reader, num_images, capacity, ...)   the frames [bounds[0], bounds[1]) live in `capacity` device slots
  .activate_frames(n) / .deactivate_frames(first) / .has_left_frames()    localrf_dataset.py:125-151, the same bounds
  .sample(batch_size, is_refining, optimize_poses, n_views=16)           localrf_dataset.py:273-313, device tensors out
  .sample_ids(...)                                  the host half of sample(): view ids, global ray ids, train_test_poses
                                                    (also a module function, testable without a GPU)
  .gather(view_ids, ray_ids, want=...)              the rows of the dataset tensors, one launch, safe under graph capture
  .errors()                                         the sticky status bits of the gathers so far (synchronises)

The package reads no files.  `reader(i)` returns frame i's arrays at the frame's size -- what read_image of
localrf_dataset.py:155-223 builds, minus cv2.imread and the resizes:
  "img"        float32 [H,W,3] in [0, 1], RGB
  "invdepth"   float32 [H,W] (optional: depth loss)
  flows (optional): "encoded_fwd_flow" / "encoded_bwd_flow" uint16 [H,W,3] and "flow_scale" (decoded on the device,
               utils/utils.py:67-71), or decoded "fwd_flow" / "bwd_flow" float32 [H,W,2] with "fwd_mask" / "bwd_mask" [H,W]
  "mask"       bool / uint8 [H,W] motion mask (optional; the loss weight is zero where it is false)
Every frame must provide the same set.  Per frame: one pinned staging block, one host->device copy, then HIP kernels
(csrc/lrf_frames.inl) write the slot: the flow decode, and the loss weight var(Laplacian(grey)) x mask of
localrf_dataset.py:229-235.  Nothing here synchronises the device except errors().

Shapes follow the reference's `self.all_X[idx_sample]`: rgbs [B,3], flows [B,2], loss_weights / invdepths / masks [B,1].
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _native as N
from ._native import NativeError

KEYS = ("rgbs", "loss_weights", "invdepths", "fwd_flow", "fwd_mask", "bwd_flow", "bwd_mask")
_WIDTH = {"rgbs": 3, "loss_weights": 1, "invdepths": 1, "fwd_flow": 2, "fwd_mask": 1, "bwd_flow": 2, "bwd_mask": 1}


def _align(n):
    return (n + 255) // 256 * 256


def sample_ids(test_mask, active_frames_bounds, n_px_per_frame, batch_size, is_refining, optimize_poses, n_views=16):
    """The host half of LocalRFDataset.sample() (localrf_dataset.py:273-301), drawing from Python's `random` and numpy's
    global generator with the same calls in the same order: the same seeds give the same batch.  Returns (view_ids int64
    [n_views], idx int64 [batch_size] -- global ray ids view * n_px + pixel --, train_test_poses)."""
    lo, hi = active_frames_bounds
    in_window_test = np.asarray(test_mask)[lo:hi]
    train_test_poses = in_window_test.mean() > random.uniform(0, 1) if optimize_poses else False
    keep = in_window_test if train_test_poses else 1 - in_window_test
    candidates = np.arange(lo, hi, dtype=np.int64)[keep == 1]
    n_cand = keep.sum()
    picks = np.random.randint(0, n_cand, n_views, dtype=np.int64)
    if not is_refining and n_cand > 4:                                           # the newest views, always, while coarse
        picks[:2] = n_cand - 1
        picks[2:4] = n_cand - 2
        picks[4] = n_cand - 3
        picks[5] = n_cand - 4
    view_ids = candidates[picks]
    pix = np.random.randint(0, n_px_per_frame, batch_size, dtype=np.int64).reshape(n_views, -1)
    idx = (pix + view_ids[:, None] * n_px_per_frame).reshape(-1)
    return view_ids, idx, train_test_poses


class DeviceFrames:
    """A drop-in for LocalRFDataset(split="train") whose frames live on the GPU.  `capacity` slots are allocated once;
    activating more frames than that refuses before any upload.  fbases: the frames' file stems (test_mask follows
    localrf_dataset.py:81-90: a numeric stem is its own index); default "0", "1", ..."""

    def __init__(self, reader, num_images, capacity, n_init_frames=7, fbases=None, test_frame_every=10, device=None):
        self.reader = reader
        self.num_images = int(num_images)
        self.capacity = int(capacity)
        if self.num_images <= 0 or self.capacity <= 0:
            raise ValueError("num_images and capacity must be positive")
        self.device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
        if self.device.type != "cuda":
            raise NativeError("localrf_amd.frames: the frame store lives on an AMD GPU (HIP kernels); there is no CPU fallback")
        fbases = [str(i) for i in range(self.num_images)] if fbases is None else [str(f) for f in fbases]
        if len(fbases) != self.num_images:
            raise ValueError(f"{len(fbases)} fbases for {self.num_images} images")
        index = [int(f) if f.isnumeric() else i for i, f in enumerate(fbases)]
        self.test_mask = np.array([1 if test_frame_every > 0 and k % test_frame_every == 0 else 0 for k in index])
        self.all_fbases = {f: i for i, f in enumerate(fbases)}
        self.white_bg = False
        self.near_far = [0.1, 1e3]
        self.scene_bbox = 2 * torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])

        if min(int(n_init_frames), self.num_images) > self.capacity:
            raise ValueError(f"n_init_frames {n_init_frames} exceeds the capacity {self.capacity}")
        first = self._check(0, reader(0))
        self._first, self._keys = first, set(first)
        H, W = first["img"].shape[:2]
        self.img_wh = [W, H]
        self.n_px_per_frame = H * W
        self.load_depth = "invdepth" in first
        self.flow_kind = "encoded" if "encoded_fwd_flow" in first else ("decoded" if "fwd_flow" in first else None)
        self.load_flow = self.flow_kind is not None
        self.has_motion_mask = "mask" in first

        n, cap, dev = self.n_px_per_frame, self.capacity, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(cap, n, 3, **f32)
        self.loss_weight = torch.zeros(cap, n, **f32)
        self.invdepth = torch.zeros(cap, n, **f32) if self.load_depth else None
        if self.load_flow:
            self.fwd_flow, self.bwd_flow = torch.zeros(cap, n, 2, **f32), torch.zeros(cap, n, 2, **f32)
            self.fwd_mask, self.bwd_mask = torch.zeros(cap, n, **f32), torch.zeros(cap, n, **f32)
        else:
            self.fwd_flow = self.bwd_flow = self.fwd_mask = self.bwd_mask = None
        self.slot_of = torch.full((self.num_images,), -1, dtype=torch.int32, device=dev)    # fixed addresses: a captured gather
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)                         # keeps reading the live table
        self._slot_host = np.full(self.num_images, -1, dtype=np.int32)
        self._free = list(range(cap))
        self._win = N.LrfFrameWindow()
        w = self._win
        w.rgb, w.loss_weight = self.rgb.data_ptr(), self.loss_weight.data_ptr()
        if self.load_depth:
            w.invdepth = self.invdepth.data_ptr()
        if self.load_flow:
            w.fwd_flow, w.fwd_mask = self.fwd_flow.data_ptr(), self.fwd_mask.data_ptr()
            w.bwd_flow, w.bwd_mask = self.bwd_flow.data_ptr(), self.bwd_mask.data_ptr()
        w.slot_of, w.status = self.slot_of.data_ptr(), self.status.data_ptr()
        w.capacity, w.n_px, w.num_images = cap, n, self.num_images

        # staging layout of one frame (the same for every frame): name -> (byte offset, numpy dtype, shape)
        parts = [("img", np.float32, (n, 3))]
        if self.load_depth:
            parts.append(("invdepth", np.float32, (n,)))
        if self.flow_kind == "encoded":
            parts += [("encoded_fwd_flow", np.uint16, (n, 3)), ("encoded_bwd_flow", np.uint16, (n, 3))]
        elif self.flow_kind == "decoded":
            parts += [("fwd_flow", np.float32, (n, 2)), ("bwd_flow", np.float32, (n, 2)),
                      ("fwd_mask", np.float32, (n,)), ("bwd_mask", np.float32, (n,))]
        if self.has_motion_mask:
            parts.append(("mask", np.uint8, (n,)))
        self._layout, off = {}, 0
        for name, dt, shape in parts:
            self._layout[name] = (off, dt, shape)
            off += _align(int(np.prod(shape)) * np.dtype(dt).itemsize)
        self._stage_bytes = off
        self._upload = torch.empty(off, dtype=torch.uint8, device=dev)                     # device side of the staging block
        self._ws = torch.empty(max(int(N.lib().lrf_frame_sharpness_workspace_bytes()), 8), dtype=torch.uint8, device=dev)

        self.active_frames_bounds = [0, 0]
        self.activate_frames(n_init_frames)

    # ------------------------------------------------------------------ frames
    def _check(self, i, d):
        """Frame i's reader output, validated (shapes and dtypes against frame 0's) -> {name: contiguous array}."""
        if not isinstance(d, dict) or "img" not in d:
            raise TypeError(f"reader({i}) must return a dict with 'img'")
        img = np.asarray(d["img"])
        if img.dtype != np.float32 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"reader({i})['img'] must be float32 [H,W,3], got {img.dtype} {img.shape}")
        H, W = img.shape[:2]
        out = {"img": img}

        def take(name, dtypes, shape):
            a = np.asarray(d[name])
            if a.dtype not in dtypes or a.shape != shape:
                raise ValueError(f"reader({i})['{name}'] must be {'/'.join(np.dtype(t).name for t in dtypes)} {list(shape)}, "
                                 f"got {a.dtype} {list(a.shape)}")
            return a

        if d.get("invdepth") is not None:
            out["invdepth"] = take("invdepth", (np.float32,), (H, W))
        if d.get("encoded_fwd_flow") is not None or d.get("encoded_bwd_flow") is not None:
            out["encoded_fwd_flow"] = take("encoded_fwd_flow", (np.uint16,), (H, W, 3))
            out["encoded_bwd_flow"] = take("encoded_bwd_flow", (np.uint16,), (H, W, 3))
            scale = d.get("flow_scale")
            if scale is None or not np.isfinite(float(scale)):
                raise ValueError(f"reader({i}): encoded flows need a finite 'flow_scale'")
            out["flow_scale"] = float(scale)
        elif d.get("fwd_flow") is not None or d.get("bwd_flow") is not None:
            out["fwd_flow"] = take("fwd_flow", (np.float32,), (H, W, 2))
            out["bwd_flow"] = take("bwd_flow", (np.float32,), (H, W, 2))
            out["fwd_mask"] = take("fwd_mask", (np.float32, np.bool_), (H, W))
            out["bwd_mask"] = take("bwd_mask", (np.float32, np.bool_), (H, W))
        if d.get("mask") is not None:
            out["mask"] = take("mask", (np.bool_, np.uint8), (H, W))
        if i > 0:
            if list(img.shape[1::-1]) != self.img_wh:
                raise ValueError(f"reader({i}): image {W}x{H}, the window holds {self.img_wh[0]}x{self.img_wh[1]}")
            if set(out) != self._keys:
                raise ValueError(f"reader({i}) provides {sorted(out)}, frame 0 provided {sorted(self._keys)}")
        return out

    def _push_table(self):
        stage = torch.from_numpy(self._slot_host.copy()).pin_memory()
        self.slot_of.copy_(stage, non_blocking=True)

    def _upload_frame(self, i, d, slot):
        stage = torch.empty(self._stage_bytes, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        for name, (off, dt, shape) in self._layout.items():
            cnt = int(np.prod(shape))
            host[off:off + cnt * np.dtype(dt).itemsize].view(dt).reshape(shape)[...] = d[name].reshape(shape)
        up = self._upload
        up.copy_(stage, non_blocking=True)                                        # the frame's one host->device copy

        def dev_view(name, width):
            off, dt, shape = self._layout[name]
            cnt = int(np.prod(shape))
            return up[off:off + cnt * 4].view(torch.float32).view(-1, width) if width > 1 else up[off:off + cnt * 4].view(torch.float32)

        self.rgb[slot].copy_(dev_view("img", 3))
        if self.load_depth:
            self.invdepth[slot].copy_(dev_view("invdepth", 1))
        H, W = self.img_wh[1], self.img_wh[0]
        if self.flow_kind == "encoded":
            for back, name in ((0, "encoded_fwd_flow"), (1, "encoded_bwd_flow")):
                N.launch("lrf_decode_flow", self.device, C.byref(self._win), slot, back, up.data_ptr() + self._layout[name][0],
                         H, W, d["flow_scale"])
        elif self.flow_kind == "decoded":
            self.fwd_flow[slot].copy_(dev_view("fwd_flow", 2))
            self.bwd_flow[slot].copy_(dev_view("bwd_flow", 2))
            self.fwd_mask[slot].copy_(dev_view("fwd_mask", 1))
            self.bwd_mask[slot].copy_(dev_view("bwd_mask", 1))
        mask_ptr = up.data_ptr() + self._layout["mask"][0] if self.has_motion_mask else None
        N.launch("lrf_frame_sharpness", self.device, C.byref(self._win), slot, H, W, mask_ptr, self._ws.data_ptr())

    def _prepare(self, i, d):
        """Reader output -> the staging dtypes (masks as float32 / uint8)."""
        d = dict(d)
        for k in ("fwd_mask", "bwd_mask"):
            if k in d:
                d[k] = d[k].astype(np.float32, copy=False)
        if "mask" in d:
            d["mask"] = d["mask"].astype(np.uint8, copy=False)
        return d

    def activate_frames(self, n_frames=1):
        """localrf_dataset.py:125-132: extend the window by n_frames (clamped to num_images) and upload the new frames."""
        lo, hi = self.active_frames_bounds
        new_hi = min(hi + int(n_frames), self.num_images)
        if new_hi - lo > self.capacity:
            raise ValueError(f"activating frames {hi}..{new_hi - 1} would hold {new_hi - lo} frames in a window of capacity "
                             f"{self.capacity}")
        if new_hi <= hi:
            self.active_frames_bounds[1] = new_hi
            return
        frames = [(i, self._first if i == 0 and self._first is not None else self._check(i, self.reader(i))) for i in range(hi, new_hi)]
        with torch.cuda.device(self.device):
            for i, d in frames:
                slot = self._free.pop(0)
                self._upload_frame(i, self._prepare(i, d), slot)
                self._slot_host[i] = slot
            self._push_table()
        self._first = None                                                        # (frame 0 was read once, by __init__)
        self.active_frames_bounds[1] = new_hi

    def has_left_frames(self):
        return self.active_frames_bounds[1] < self.num_images

    def deactivate_frames(self, first_frame):
        """localrf_dataset.py:138-151: frames before first_frame leave the window; their slots are freed, nothing is copied."""
        lo, hi = self.active_frames_bounds
        first_frame = int(first_frame)
        if not lo <= first_frame <= hi:
            raise ValueError(f"first_frame {first_frame} outside the active window [{lo}, {hi}]")
        if first_frame == lo:
            return
        for i in range(lo, first_frame):
            self._free.append(int(self._slot_host[i]))
            self._slot_host[i] = -1
        with torch.cuda.device(self.device):
            self._push_table()
        self.active_frames_bounds[0] = first_frame

    def get_frame_fbase(self, view_id):
        return list(self.all_fbases.keys())[view_id]

    # ------------------------------------------------------------------ batches
    def sample_ids(self, batch_size, is_refining, optimize_poses, n_views=16):
        """The host half of sample(): see the module function sample_ids."""
        return sample_ids(self.test_mask, self.active_frames_bounds, self.n_px_per_frame, batch_size, is_refining, optimize_poses, n_views)

    def sample(self, batch_size, is_refining, optimize_poses, n_views=16):
        """localrf_dataset.py:273-313 with device tensors: the reference's keys (rgbs, loss_weights, invdepths, fwd_flow,
        fwd_mask, bwd_flow, bwd_mask -- None when not loaded --, idx, view_ids: int64 on the device, train_test_poses).
        One host->device copy of the ids, one gather launch."""
        view_ids, idx, ttp = self.sample_ids(batch_size, is_refining, optimize_poses, n_views)
        V = view_ids.shape[0]
        stage = torch.empty(V + idx.shape[0], dtype=torch.int64, pin_memory=True)
        stage.numpy()[:V] = view_ids
        stage.numpy()[V:] = idx
        ids = stage.to(self.device, non_blocking=True)
        rows = self.gather(ids[:V], ids[V:], want=self.available())
        out = {k: rows.get(k) for k in KEYS}
        out.update(idx=ids[V:], view_ids=ids[:V], train_test_poses=ttp)
        return out

    def available(self):
        """The gather outputs this store holds."""
        return tuple(k for k in KEYS if not ((k == "invdepths" and not self.load_depth) or (k.endswith(("flow", "mask")) and not self.load_flow)))

    def gather(self, view_ids, ray_ids, want=KEYS):
        """Rows of the dataset tensors for V views x n rays in one launch: view_ids int64 [V], ray_ids int64 [V*n] or [V,n]
        (global ids view * n_px + pix, or per-view pixel ids), both on this device.  want: the keys to return (see KEYS).
        No host synchronisation and no host read: safe inside a graph capture.  A view that is not resident gives NaN rows
        and sets bit N.LRF_FRAMES_ERR_NOT_RESIDENT of errors()."""
        if not (torch.is_tensor(view_ids) and torch.is_tensor(ray_ids)) or view_ids.device != self.device or ray_ids.device != self.device:
            raise ValueError(f"view_ids and ray_ids must be tensors on {self.device}")
        if view_ids.dtype != torch.int64 or ray_ids.dtype != torch.int64:
            raise ValueError("view_ids and ray_ids must be int64")
        V, B = int(view_ids.numel()), int(ray_ids.numel())
        if V == 0 or B % V:
            raise ValueError(f"{B} ray ids do not split into {V} views")
        bad = [k for k in want if k not in KEYS]
        if bad:
            raise ValueError(f"unknown keys {bad}; known: {KEYS}")
        missing = [k for k in want if k not in self.available()]
        if missing:
            raise ValueError(f"the store holds no {missing}")
        vi, ri = view_ids.reshape(-1).contiguous(), ray_ids.reshape(-1).contiguous()
        out = {k: torch.empty(B, _WIDTH[k], dtype=torch.float32, device=self.device) for k in want}
        N.launch("lrf_frames_gather", self.device, C.byref(self._win), vi.data_ptr(), ri.data_ptr(), V, B // V,
                 *[N.ptr(out.get(k)) for k in KEYS], guard=True)
        return out

    def errors(self, clear=False):
        """The status bits of every gather so far (N.LRF_FRAMES_ERR_NOT_RESIDENT: a view was not in the window).  Reads
        the device word: this synchronises.  clear: reset it afterwards (stream-ordered)."""
        v = int(self.status.item())
        if clear:
            self.status.zero_()
        return v
