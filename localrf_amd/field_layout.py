"""FieldLayout -- what a TensorVMSplit keeps on the native side of lrf_render_*: the packed parameter cache and the rule that
says when it is stale, the LrfField struct built from it, the host copies of the grid and the box, and the workspaces.

All of it is derived from the field's parameters and rebuilt by the call that needs it; none of it is registered with the
module, so nothing reaches state_dict().  The field makes a new one in _reset_native_state() (__init__ and to()) and hands
itself to every call: the layout keeps no reference to the field.
"""
import ctypes as C

import torch

from . import _native as N


def point_at(st, tensors, planes=True):
    """Write the addresses of 19 tensors in the order of TensorVMSplit._param_list() into the density_plane ... b3 members of
    `st` (LrfParams, LrfGrads); planes=False for LrfField, which has the seven network members only."""
    a = [t.data_ptr() for t in tensors]
    if planes:
        st.density_plane[:], st.density_line[:], st.app_plane[:], st.app_line[:] = a[0:3], a[3:6], a[6:9], a[9:12]
    st.basis, st.w1, st.b1, st.w2, st.b2, st.w3, st.b3 = a[12:]


class FieldLayout:
    def __init__(self, grid=None):
        self.grid = grid                         # host copies of gridSize and aabb (tuples), so that no render call
        self.box = self._box_of = None           # synchronises to read them back; _box_of: (data_ptr, _version) of aabb
        self.cache = self.key = None             # channel-last / fragment-ordered image of the parameters (lrf_pack_field)
        self._cfield = self._cfield_key = None   # LrfField of the current cache / alpha mask
        self._mask_box = (None, None)            # (id, data_ptr, _version of the alpha mask and its box), its host copy
        self.release_workspaces()                # ws: eval-forward workspace per stream; ws_bwd: the recomputing backward's

    # ------------------------------------------------------------------ host copies
    def refresh_host(self, field, grid=None):
        """The one read-back of the box: when aabb is another tensor or was written (load_state_dict, to()) -- the kernels
        read it live, as normalize_coord does (tensorBase.py:342-345).  `grid`: the new gridSize (update_stepSize)."""
        if grid is not None:
            self.grid = tuple(int(g) for g in grid)
        aabb = field.aabb
        at = (aabb.data_ptr(), aabb._version)
        if at != self._box_of:
            self.box, self._box_of = tuple(float(v) for v in aabb.detach().reshape(-1).tolist()), at
        return self.box

    # ------------------------------------------------------------------ the packed cache
    def current_key(self, field):
        """What the cache is valid for: every parameter's (data_ptr, _version), the grid and the box."""
        return field._param_versions() + self.grid + self.refresh_host(field)

    def is_fresh(self, field):
        return self.key == self.current_key(field)

    def invalidate(self):
        """The next ensure() packs, and the next c_field() builds its struct, whatever the key says."""
        self.key = self._cfield_key = None

    def mark_fresh(self, field):
        """The cache was just rewritten from the parameters as they are now (lrf_adam_step_pack)."""
        self.key = self.current_key(field)

    def _fits(self, nbytes, dev):
        return self.cache is not None and self.cache.numel() * 4 == nbytes and self.cache.device == dev

    def ensure(self, field):
        """(Re)pack the cache when any parameter changed (optimizer step, upsample tensoRF.py:224-233, load_state_dict)."""
        key = self.current_key(field)
        if key == self.key:
            return
        lib = N.lib()
        cp, ps = field._c_params()
        nbytes, dev = lib.lrf_cache_bytes(cp.grid), ps[0].device
        if not self._fits(nbytes, dev):
            self.cache = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        N.launch("lrf_pack_field", dev, C.byref(cp), self.cache.data_ptr())
        self.key = key

    def step_target(self, field):
        """(LrfParams, parameter list, cache) for lrf_adam_step_pack -- the optimiser step that leaves the cache holding the
        stepped values (localrf_amd.optim.FusedAdam(pack_field=...)) -- or None while no packed cache of the current grid's
        size exists (the first forward, after an upsample / a device move): the step then runs alone, the next forward packs."""
        if self.key is None:
            return None
        cp, ps = field._c_params()
        return (cp, ps, self.cache) if self._fits(N.lib().lrf_cache_bytes(cp.grid), ps[0].device) else None

    # ------------------------------------------------------------------ the struct the kernels take
    def c_field(self, field):
        """LrfField for the current cache / alpha mask, rebuilt only when one of them, a scalar or the box changed."""
        mask = field.alphaMask
        scalars = (float(field.density_shift), float(field.distance_scale), float(field.rayMarch_weight_thres),
                   float(field.early_term_T))
        key = (self.cache.data_ptr(), self.key, id(mask), None if mask is None else mask.alpha_volume.data_ptr(), scalars, self.box)
        if self._cfield_key == key:
            return self._cfield
        f = N.LrfField(cache=self.cache.data_ptr())
        f.aabb[:] = f.alpha_aabb[:] = self.box   # (no mask: alpha_vol NULL and alpha_dim 0, as the struct starts)
        f.grid[:] = self.grid
        if mask is not None:
            vol = mask.alpha_volume.detach()
            f.alpha_vol = vol.data_ptr()
            f.alpha_dim[:] = [vol.shape[-1], vol.shape[-2], vol.shape[-3]]
            mk = (id(mask), mask.aabb.data_ptr(), mask.aabb._version)
            if self._mask_box[0] != mk:          # read back once per mask (a rebuild makes a new mask): c_field can then run
                self._mask_box = (mk, tuple(float(v) for v in mask.aabb.detach().reshape(-1).tolist()))   # inside a capture
            f.alpha_aabb[:] = self._mask_box[1]
        f.density_shift, f.distance_scale, f.weight_thres, f.term_T = scalars
        point_at(f, field._param_list(), planes=False)
        f.fea_pe, f.view_pe, f.feature_c = int(field.fea_pe), int(field.view_pe), int(field.featureC)
        self._cfield, self._cfield_key = f, key
        return f

    # ------------------------------------------------------------------ workspaces
    def workspace(self, R, S, dev):
        """One eval-forward workspace per stream that renders through this field: two streams may run eval forwards of the
        same field side by side (k_march of one batch beside k_shade3 of another: 4096-ray batches alternating over two
        streams 0.164 -> 0.145 ms per batch, scripts/two_stream_fwd_probe.py); the cache they read is shared."""
        nbytes = N.lib().lrf_workspace_bytes(R, S)
        st = N.stream(dev)
        ws = self.ws.get(st)
        if ws is None or ws.numel() < nbytes or ws.device != dev:
            ws = self.ws[st] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws

    def workspace_bwd(self, nbytes, dev):
        if self.ws_bwd is None or self.ws_bwd.numel() < nbytes or self.ws_bwd.device != dev:
            self.ws_bwd = None                   # drop the old buffer before the larger one is allocated
            self.ws_bwd = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self.ws_bwd

    def release_workspaces(self):
        self.ws, self.ws_bwd = {}, None
