"""Deterministic backward (LRF_FLAG_DETERMINISTIC / TensorVMSplit.deterministic / torch.use_deterministic_algorithms) on the
MI355X: the same inputs give the same gradient BITS -- all 19 parameter tensors and d/d rays -- from run to run, whatever the
number of scatter workgroups (lrf_debug_set_scatter_wgs), on one stream or two, captured or eager, with or without the
per-plane passes of LRF_FLAG_PLANE_EVENTS; the results stay within 2e-6 of each tensor's maximum of the default mode's, and
the density tensors meet the reference-recorded gradients at 1e-4.  Training runs under torch.use_deterministic_algorithms
repeat bit for bit.  Every test that flips a global restores it."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import vm_render_np as oracle
from util import (FIELD_KW, check_grads, field_from_golden, field_from_seed, golden_field_dict, load_golden, make_field,
                  quiet)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grads(f, rays_np, z, g_rgb, g_depth):
    """Row-saving forward + backward through autograd; gradients by name (+ "rays")."""
    f.z_override = z.clone()
    for p in f.parameters():
        p.grad = None
    rays = torch.as_tensor(rays_np).to(DEV).clone().requires_grad_(True)
    rgb, depth = f(rays, white_bg=True, is_train=False, N_samples=-1)
    ((rgb * g_rgb).sum() + (depth * g_depth).sum()).backward()
    torch.cuda.synchronize()
    f.z_override = None
    out = {n: p.grad.clone() for n, p in f.named_parameters() if p.grad is not None}
    out["rays"] = rays.grad.clone()
    return out


def _setup(name):
    g = load_golden(name)
    f = quiet(field_from_golden, g, DEV) if name == "field_small_train_grad" else field_from_seed(g, DEV)
    ns = int(g["N_samples"]) if "N_samples" in g else int(g["nSamples"])
    z = torch.from_numpy(oracle.z_schedule(ns, np.float32, jitter=(g["U"], g["U2"])))
    gr, gd = torch.from_numpy(g["g_rgb"]).to(DEV), torch.from_numpy(g["g_depth"]).to(DEV)
    return g, f, z, gr, gd


def _same(a, b, what):
    assert set(a) == set(b)
    bad = [n for n in a if not torch.equal(a[n], b[n])]
    assert not bad, (what, bad)


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


@pytest.mark.parametrize("name", ["field_small_train_grad", "field_128_train_grad", "field_500_train_grad", "field_640_train_grad"])
def test_field_gradients_are_bit_identical(built_lib, name):
    g, f, z, gr, gd = _setup(name)
    f.deterministic = False
    default = _grads(f, g["rays"], z, gr, gd)
    f.deterministic = True
    runs = {}
    try:
        for key, wgs, overlap in (("a", 0, 1), ("b", 0, 1), ("c", 0, 1), ("wgs7", 7, 1), ("wgs4cus", 4 * _cus(), 1), ("one_stream", 0, 0)):
            built_lib.lrf_debug_set_scatter_wgs(wgs)
            built_lib.lrf_debug_set_bwd_overlap(overlap)
            runs[key] = _grads(f, g["rays"], z, gr, gd)
    finally:
        built_lib.lrf_debug_set_scatter_wgs(0)
        built_lib.lrf_debug_set_bwd_overlap(1)
    assert len(runs["a"]) == 20
    for key in runs:
        _same(runs["a"], runs[key], key)
    det = runs["a"]
    worst = {}
    for n, v in det.items():
        den = float(default[n].abs().max())
        err = float((v - default[n]).abs().max()) / max(den, 1e-30)
        worst[n] = err
        if n == "rays":
            continue
        assert err <= 2e-6, (n, err)           # plane / line tensors: other sums of the same products; weights: the same kernels
    print(name, "deterministic vs default, max error / max:", {n: "%.1e" % e for n, e in sorted(worst.items(), key=lambda t: -t[1])[:5]})
    dens = {n: v for n, v in det.items() if n.startswith("density_")}
    names = [n for n in dens]
    subset = {n: torch.from_numpy(g["gidx." + n]).to(DEV) for n in names if ("gidx." + n) in g}
    gmax = {n: float(g["gmax." + n]) for n in names} if "gmax.density_plane.0" in g else None
    check_grads(dens, {n: torch.from_numpy(g["grad." + n]).to(DEV) for n in dens}, 1e-4, subset=subset or None, gmax=gmax)


def _native_bwd(f, rays, z, gr, gd, flags):
    g_rays, grads = f._native_backward(rays, z, flags, gr, gd)
    return [g_rays.clone()] + [t.clone() for t in grads]


def test_captured_backward_equals_eager(built_lib):
    g, f, z, gr, gd = _setup("field_128_train_grad")
    f.deterministic = True
    rays = torch.as_tensor(g["rays"]).to(DEV)
    zz = z.to(DEV)
    flags = f._flags(True)
    eager = _native_bwd(f, rays, zz, gr, gd, flags)           # two streams
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _native_bwd(f, rays, zz, gr, gd, flags)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_rays, grads = f._native_backward(rays, zz, flags, gr, gd)       # one stream inside the capture
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        captured = [g_rays] + list(grads)
        assert len(captured) == len(eager)
        for i, (a, b) in enumerate(zip(eager, captured)):
            assert torch.equal(a, b), i
    eager2 = _native_bwd(f, rays, zz, gr, gd, flags)
    for a, b in zip(eager, eager2):
        assert torch.equal(a, b)


def test_plane_events_give_the_same_bits(built_lib, monkeypatch):
    from localrf_amd import _native as N
    from localrf_amd import dist
    g, f, z, gr, gd = _setup("field_128_train_grad")
    f.deterministic = True
    rays = torch.as_tensor(g["rays"]).to(DEV)
    zz = z.to(DEV)
    plain = _native_bwd(f, rays, zz, gr, gd, f._flags(True))
    monkeypatch.setattr(dist, "active", lambda: True)
    g_rays, grads = f._native_backward(rays, zz, f._flags(True), gr, gd)
    assert f._grads.plane_events
    st = torch.cuda.current_stream(DEV).cuda_stream
    for bucket in (3, 4, 0, 1, 2):
        N.check(N.lib().lrf_render_bwd_wait(bucket, st), "lrf_render_bwd_wait")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(plain, [g_rays] + list(grads))):
        assert torch.equal(a, b), i


def test_other_engines(built_lib):
    from localrf_amd._native import NativeError
    g, f, z, gr, gd = _setup("field_small_train_grad")
    f.mlp_engine = "f32"                                    # exact-fp32 colour network (the backward's kernels are the default ones)
    f.deterministic = True
    runs = []
    try:
        for wgs in (0, 0, 7):
            built_lib.lrf_debug_set_scatter_wgs(wgs)
            runs.append(_grads(f, g["rays"], z, gr, gd))
    finally:
        built_lib.lrf_debug_set_scatter_wgs(0)
    for r in runs[1:]:
        _same(runs[0], r, "f32")
    # the generic engine (a non-default network) is not covered: refused by name, never silently non-deterministic
    gp = load_golden("field_pe_2_3_64")
    cfg = dict(fea_pe=int(gp["fea_pe"]), view_pe=int(gp["view_pe"]), featureC=int(gp["featureC"]))
    fp = quiet(make_field, [int(v) for v in gp["grid"]], "cpu", **cfg)
    fp.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in golden_field_dict(gp).items()})
    fp = fp.to(DEV)
    fp.deterministic = True
    rays = torch.from_numpy(gp["rays"]).to(DEV).requires_grad_(True)
    rgb, depth = fp(rays, white_bg=True, is_train=False, N_samples=int(gp["N_samples"]))
    with pytest.raises(NativeError, match="LRF_FLAG_DETERMINISTIC does not cover the generic engine"):
        (rgb.sum() + depth.sum()).backward()


def _train_synth():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_synth
    return train_synth


def test_training_runs_are_reproducible():
    train_synth = _train_synth()
    kw = dict(frames=9, final=80, iters_per_frame=30, n_max_frames=5, dev=DEV, geo_every=5, record_all=True, max_iters=150)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        g1 = train_synth.run(graph=True, **kw)
        g2 = train_synth.run(graph=True, **kw)
        e1 = train_synth.run(graph=False, **kw)
        e2 = train_synth.run(graph=False, **kw)
    finally:
        torch.use_deterministic_algorithms(was)
    a, b = np.array(g1["all_losses"]), np.array(g2["all_losses"])
    assert a.shape == b.shape and len(a) > 100 and np.array_equal(a, b)
    c, d = np.array(e1["all_losses"]), np.array(e2["all_losses"])
    assert c.shape == d.shape and np.array_equal(c, d)
    n = min(len(a), len(c))
    print("deterministic training: eager vs captured, max |loss difference| over %d iterations: %.3e" % (n, float(np.abs(a[:n] - c[:n]).max())))


def test_trajectory_replay_is_reproducible():
    from localrf_amd import LocalTensorfs
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import trajectory as tj
    g = load_golden("trajectory_30it")

    def one():
        kw = dict(FIELD_KW)
        kw.update(tj.FIELD_OVER)
        aabb = 2 * torch.tensor([[-1.0, -1, -1], [1, 1, 1]]).to(DEV)
        scene_kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in tj.SCENE_KW.items()}
        lt = quiet(LocalTensorfs, device=DEV, aabb=aabb, gridSize=list(tj.GRID), **scene_kw, **kw)
        quiet(lt.load, {k[5:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items() if k.startswith("init.")})
        lt = lt.to(DEV)

        def before_forward(scene, it):
            scene.tensorfs[-1].z_override = torch.from_numpy(g[f"z.{it}"]).to(DEV)

        def after_append_rf(scene):
            sd = {k[4:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items() if k.startswith("rf1.")}
            scene.tensorfs[-1].load_state_dict(sd)
        log = quiet(tj.run, lt, g["view_u"], g["ray_ids"], tj.targets(), DEV, before_forward=before_forward,
                    after_append_rf=after_append_rf)
        return log, {k: v.detach().cpu().numpy() for k, v in lt.state_dict().items()}

    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        log1, s1 = one()
        log2, s2 = one()
    finally:
        torch.use_deterministic_algorithms(was)
    assert set(s1) == set(s2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    photo = np.array([r["photo"] for r in log1])
    assert (np.abs(photo - g["photo"]) / g["photo"]).max() < 1e-4
    want = {k[6:]: v for k, v in g.items() if k.startswith("final.")}
    worst = 0.0
    for k, w in want.items():
        if w.dtype.kind != "f" or not np.abs(w).max() > 0 or k.endswith("alpha_volume"):
            continue
        l2 = float(np.linalg.norm(s1[k] - w) / np.linalg.norm(w))
        worst = max(worst, l2)
        assert l2 < 3e-3, (k, l2)
    print("deterministic trajectory: worst relative L2 of the final parameters against the reference golden %.2e" % worst)
