"""GradBucket -- the ONE flat fp32 buffer a field's backward leaves its parameter gradients in, and what is known about it.

lrf_render_bwd writes the gradients of all parameter tensors of a TensorVMSplit (and d/d rays [R, 6] behind them) into views
of one buffer, every view 64 floats (256 bytes) aligned.  The data-parallel exchange (localrf_amd.dist) sums that buffer
across ranks in place, piece by piece, behind the events the backward records.  The field owns one GradBucket per backward
(TensorVMSplit._grads); localrf_amd.dist and the captured iteration (localrf_amd.graph_step) speak to it and to nothing else.
"""
import torch


class GradBucket:
    """params: the parameter tensors in the order of the buffer, in three branches -- density = params[:first_app],
    appearance = params[first_app:first_net] (its first three tensors are the planes), network = params[first_net:].
    R: rays of the batch (the [R, 6] ray-gradient tail lies behind the parameter part and is rank-local).

    fresh: written by THIS backward and not yet reduced (localrf_amd.dist reduces fresh buckets only and clears it; a
      replayed graph sets it again, because the backward's Python does not run in a replay).
    events: the bucket events of lrf_render_bwd_wait belong to the backward that filled the buffer -- not for an empty
      batch, and not inside a stream capture (a captured event cannot be waited for from outside the graph).
    plane_events: that backward ran its appearance scatter as one pass per plane (LRF_FLAG_PLANE_EVENTS)."""

    def __init__(self, params, R, dev, first_app, first_net, plane_events=False, events=False):
        if plane_events and first_net - first_app < 3:
            raise ValueError("plane_events needs the three appearance planes")
        offs = [0]
        for n in [p.numel() for p in params] + [R * 6]:
            offs.append(offs[-1] + (n + 63) // 64 * 64)
        # lrf_render_bwd clears the whole buffer itself (LrfGrads.zero_base / zero_floats, with the launch that clears its
        # bins; the offsets are multiples of 64 floats: so is the total) -- except for an empty batch, where it is not called
        self.flat = (torch.empty if R > 0 else torch.zeros)(offs[-1], dtype=torch.float32, device=dev)
        self.params, self.offs, self.n_param, self.R = params, offs[:len(params)], offs[-2], R
        self.dens, self.app, self.net = (0, offs[first_app]), (offs[first_app], offs[first_net]), (offs[first_net], offs[-2])
        self.app_planes = tuple(offs[first_app:first_app + 3])
        self.fresh, self.events, self.plane_events = True, bool(events), bool(plane_events)

    def views(self):
        """(gradient view per parameter, d/d rays [R, 6]): what LrfGrads points to and what autograd is handed.  They are
        NOT kept here: autograd adopts an incoming gradient as .grad without a copy only while nobody else holds a
        reference to it."""
        flat = self.flat
        g_rays = flat[self.n_param:self.n_param + self.R * 6].view(self.R, 6)
        return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offs)], g_rays

    def release(self):
        """Give the buffer up (35-96 MB; the field's optimiser is gone).  The bucket stays with its field as the mark that
        the field's gradients come from lrf_render_bwd and that it sat the last backward out: held(), rebucket() and chunks()
        are None from now on."""
        self.flat, self.fresh, self.events = None, False, False

    def held(self):
        """(flat[:n_param], params that require grad) if .grad of every one of them is still a view of the buffer (autograd
        adopts the views when .grad was None, i.e. after zero_grad(set_to_none=True) -- what the optimisers here do):
        localrf_amd.dist.allreduce_grads then reduces the buffer in place, no copies.  None when (some of) the gradients
        were accumulated elsewhere (rebucket() brings them back) or the buffer was released."""
        if self.flat is None:
            return None
        base = self.flat.untyped_storage().data_ptr()
        ps = [p for p in self.params if p.requires_grad]
        for p in ps:
            if p.grad is None or p.grad.untyped_storage().data_ptr() != base:
                return None
        return self.flat[:self.n_param], ps          # the parameter part: the d/d rays tail behind it is rank-local

    def rebucket(self):
        """Bring the gradients back into the buffer when autograd put (some of) them elsewhere: it sums the contributions
        to a parameter BEFORE it writes .grad, so with a regulariser in the loss (density_L1 / TV,
        local_tensorfs.py:316-330: their node runs first) .grad of the density tensors is the regulariser's tensor with the
        render gradient added to it, not the view lrf_render_bwd wrote.  One multi-tensor copy (device to device, the size
        of the strays) and .grad re-pointed to the views -- instead of a concatenation of the whole field and a host
        read-back on the data-parallel path.  Returns held()."""
        if self.flat is None:
            return None
        base = self.flat.untyped_storage().data_ptr()
        src, dst, who = [], [], []
        for p, o in zip(self.params, self.offs):
            if not p.requires_grad:
                continue
            if p.grad is None:                       # (no gradient reached it: nothing to bring back, nothing is invented)
                return None
            if p.grad.untyped_storage().data_ptr() != base:
                v = self.flat[o:o + p.numel()].view(p.shape)
                if p.grad.shape != v.shape or p.grad.dtype != v.dtype or p.grad.device != v.device:
                    return None
                src.append(p.grad)
                dst.append(v)
                who.append(p)
        if src:
            torch._foreach_copy_(dst, src)
            for p, v in zip(who, dst):
                p.grad = v
            self.events = False                      # the bucket events of lrf_render_bwd are behind these copies
        return self.held()

    def chunks(self):
        """[(bucket, start, end)] in the order the backward finishes them: the pieces localrf_amd.dist all-reduces one by
        one, each behind lrf_render_bwd_wait(bucket).  Density planes + lines (bucket 0: the per-ray branch ends early),
        colour network (1), then the appearance tensors -- as ONE piece (2), or, when the backward ran its appearance
        scatter per plane (plane_events: a process group with more than one rank exists), plane 0 (3), plane 1 (4) and
        plane 2 with the three lines (2), so that only the last ~ third of the 26 MB (300^3) is exposed behind the backward."""
        if self.flat is None:
            return None
        out = [(0,) + self.dens, (1,) + self.net]
        if self.plane_events:
            a0, a1, a2 = self.app_planes
            out += [(3, a0, a1), (4, a1, a2), (2, a2, self.app[1])]
        else:
            out.append((2,) + self.app)
        return out
