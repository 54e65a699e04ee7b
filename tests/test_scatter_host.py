"""The gradient scatter's reference side, without a GPU (tests/scatter_cases.py holds the restatement and the case list):
  * the float64 restatement equals float64 autograd through the reference's op chain on all twelve tensors, per cell;
  * every case covers what it is meant to cover -- proven from the reference alone, so that no GPU test passes vacuously;
  * the reference's own fp32 scatter against float64, kappa_ref per case (docs/SCATTER_FIGURES.md), which sets the GPU bar;
  * lrf_render_bwd's engine choice, pinned on either side of every threshold through lrf_debug_scatter_plan."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from abi_util import FAKE, refused  # noqa: E402
import scatter_cases as sc                       # noqa: E402
from oracle import vm_render_torch as ot         # noqa: E402


# ------------------------------------------------------------------ the float64 port with its upstream kept
def port_float64(case):
    """render_field in float64 on the case's field, with retain_grad on the density feature and on the appearance product
    rows.  Returns fld (numpy, state-dict names), rays, z, gf [R S], lin [n], dX [n,3,24], grads {name: float64 array}."""
    f = sc.case_field(case)
    rays, z = sc.case_rays(case), sc.case_z(case)
    g_rgb, g_depth = sc.case_upstream(case)
    kept = {}
    orig_d, orig_a = ot.density_feature, ot.app_feature

    def dens(fld, u):
        out = orig_d(fld, u)
        out.retain_grad()
        kept["df"] = out
        return out

    def app(fld, u):                                  # app_feature with its product rows x [n,72] kept
        pp, ll = ot._vm_lookup([fld[f"app_plane.{i}"] for i in range(3)], [fld[f"app_line.{i}"] for i in range(3)], u)
        x = (torch.cat(pp) * torch.cat(ll)).T
        x.retain_grad()
        kept["x"] = x
        return torch.nn.functional.linear(x, fld["basis_mat.weight"])

    torch.set_default_dtype(torch.float64)
    try:
        ot.density_feature, ot.app_feature = dens, app
        fld = {k: v.detach().clone().double() for k, v in f.state_dict().items()}
        leaves = {n: fld[n].clone().requires_grad_(True) for n in sc.NAMES}
        info = {"want_masks": True}
        rgb, depth = ot.render_field({**fld, **leaves}, torch.from_numpy(rays).double(), torch.from_numpy(z).double()[None], True, 0.0,
                                     density_shift=float(f.density_shift), weight_thres=float(f.rayMarch_weight_thres), info=info)
        ((rgb * torch.from_numpy(g_rgb).double()).sum() + (depth * torch.from_numpy(g_depth).double()).sum()).backward()
    finally:
        ot.density_feature, ot.app_feature = orig_d, orig_a
        torch.set_default_dtype(torch.float32)
    R, S = case.R, case.S
    gf = np.zeros(R * S)
    if "df" in kept:                                  # every sample but a ray's last (no case mixes a mask with live samples)
        valid = np.ones((R, S), bool)
        valid[:, -1] = False
        gf[valid.reshape(-1)] = kept["df"].grad.numpy()
    lin = info["own_lin"].numpy() if "x" in kept else np.zeros(0, np.int64)
    dX = kept["x"].grad.numpy().reshape(-1, 3, 24) if "x" in kept else np.zeros((0, 3, 24))
    grads = {n: (leaves[n].grad.numpy() if leaves[n].grad is not None else np.zeros(tuple(leaves[n].shape))) for n in sc.NAMES}
    fld_np = {k: v.detach().numpy() for k, v in f.state_dict().items()}
    return fld_np, rays, z, gf, lin, dX, grads


_PORT = {}


def port_case(case):
    """port_float64 and the restatement on its fp32-rounded upstream (what a kernel would be handed), once per case."""
    if case.name not in _PORT:
        fld, rays, z, gf, lin, dX, grads = port_float64(case)
        gf32, dX32 = gf.astype(np.float32), dX.astype(np.float32)
        ref, info = sc.scatter_ref(fld, rays, z, gf32, lin, dX32, case.unit)
        _PORT[case.name] = dict(fld=fld, rays=rays, z=z, gf=gf, lin=lin, dX=dX, grads=grads, gf32=gf32, dX32=dX32, ref=ref, info=info)
    return _PORT[case.name]


# ------------------------------------------------------------------ 1. the restatement is the reference's autograd
@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_restatement_equals_float64_autograd(case):
    """G within 1e-12 A of the float64 port's autograd gradient, every cell of all twelve tensors; exactly zero where A = 0."""
    pc = port_case(case)
    ref, _ = sc.scatter_ref(pc["fld"], pc["rays"], pc["z"], pc["gf"], pc["lin"], pc["dX"], case.unit)       # the unrounded upstream
    for name in sc.NAMES:
        G, A, m = ref[name]
        over, stray, worst, _ = sc.cell_errors(pc["grads"][name], G, A, m, 1e-12, 0.0)
        assert over == 0 and stray == 0, (case.name, name, over, stray, worst)
        assert G.shape == pc["grads"][name].shape


# ------------------------------------------------------------------ 2. the cases cover what they are meant to cover
def _tiles_with_entries(u, p, grid):
    W, H = grid[sc.MAT_MODE[p][0]], grid[sc.MAT_MODE[p][1]]
    x0 = sc.tap(u[:, sc.MAT_MODE[p][0]], W)[0]
    y0 = sc.tap(u[:, sc.MAT_MODE[p][1]], H)[0]
    tx, ty = (W + sc.BTILE - 1) // sc.BTILE, (H + sc.BTILE - 1) // sc.BTILE
    return np.bincount((y0 // sc.BTILE) * tx + x0 // sc.BTILE, minlength=tx * ty)


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_cases_cover_their_edges(case):
    pc = port_case(case)
    ref, grid = pc["ref"], case.grid
    kinds = ("density", "app") if "edges" in case.expect else ("density",) if "edges_d" in case.expect else ()
    for kind in kinds:
        for p in range(3):
            A = ref[f"{kind}_plane.{p}"][1][0].max(0)                     # [H,W]: any channel
            for what, v in (("first row", A[0]), ("last row", A[-1]), ("first column", A[:, 0]), ("last column", A[:, -1])):
                assert v.max() > 0, (case.name, kind, p, what)
            Al = ref[f"{kind}_line.{p}"][1][0, :, :, 0].max(0)
            assert Al[0] > 0 and Al[-1] > 0, (case.name, kind, p, "line ends")
    if "borders" in case.expect:
        borders = 0
        for kind in ("density", "app"):
            for p in range(3):
                A = ref[f"{kind}_plane.{p}"][1][0].max(0)
                for x in range(sc.BTILE, A.shape[1], sc.BTILE):
                    assert A[:, x].max() > 0, (case.name, kind, p, "x", x)
                    borders += 1
                for y in range(sc.BTILE, A.shape[0], sc.BTILE):
                    assert A[y].max() > 0, (case.name, kind, p, "y", y)
                    borders += 1
        assert borders > 0, case.name
    u = sc.positions(pc["rays"], pc["z"], pc["fld"]["aabb"])
    for ent in (np.nonzero(pc["gf32"])[0], pc["lin"]):
        if case.masked and ent is not pc["lin"]:
            continue                                                      # (no density entry at all)
        cnt = [_tiles_with_entries(u[ent], p, grid) for p in range(3)]
        full = [p for p in range(3) if cnt[p].size > 1 and cnt[p].min() > 0]
        holes = [p for p in range(3) if cnt[p].min() == 0]
        if "tiles_full" in case.expect:
            assert full, (case.name, [c.tolist() for c in cnt])
        if "tiles_empty" in case.expect:
            assert holes, (case.name, [c.tolist() for c in cnt])
    if "run17" in case.expect:
        ent = np.zeros(case.R * case.S, bool)
        ent[np.nonzero(pc["gf32"])[0]] = True
        best = 0
        for p in range(3):
            W, H = grid[sc.MAT_MODE[p][0]], grid[sc.MAT_MODE[p][1]]
            x0, x1 = sc.tap(u[:, sc.MAT_MODE[p][0]], W)[:2]
            y0, y1 = sc.tap(u[:, sc.MAT_MODE[p][1]], H)[:2]
            key = (((y0 * W + x0) * 2 + (x1 - x0)) * 2 + (y1 - y0)).reshape(case.R, case.S)
            for r in range(case.R):
                run = 0
                for k in range(case.S):
                    same = k > 0 and ent[r * case.S + k] and ent[r * case.S + k - 1] and key[r, k] == key[r, k - 1]
                    run = run + 1 if same else 1
                    best = max(best, run)
        assert best >= 17, (case.name, best)
    if "corner17" in case.expect:
        W, H = grid[0], grid[1]
        assert W % sc.BTILE == 1 and H % sc.BTILE == 1
        x0, x1 = sc.tap(u[:, 0], W)[:2]
        y0, y1 = sc.tap(u[:, 1], H)[:2]
        corner = ((x0 == W - 1) & (x1 == W - 1) & (y0 == H - 1) & (y1 == H - 1) & (pc["gf32"] != 0)).reshape(case.R, case.S)
        best = 0
        for r in range(case.R):
            run = 0
            for k in range(case.S):
                run = run + 1 if corner[r, k] else 0
                best = max(best, run)
        assert best >= 17, (case.name, best)
    if "long90" in case.expect:
        p_long = [p for p in range(3) if grid[sc.VEC_MODE[p]] == max(grid)][0]
        for kind in ("density", "app"):
            Al = ref[f"{kind}_line.{p_long}"][1][0, :, :, 0].max(0)
            assert np.count_nonzero(Al) >= 0.9 * Al.size, (case.name, kind, np.count_nonzero(Al), Al.size)
            long_axis = sc.VEC_MODE[p_long]
            for q in range(3):                                            # ... and along the long side of the two planes that have it
                if q == p_long:
                    continue
                A = ref[f"{kind}_plane.{q}"][1][0].max(0)
                along = A.max(0) if sc.MAT_MODE[q][0] == long_axis else A.max(1)
                assert np.count_nonzero(along) >= 0.9 * along.size, (case.name, kind, q)
    if case.masked:
        assert not pc["gf32"].any()
    assert pc["info"]["n_app"] > 0, case.name                             # every case shades something


# ------------------------------------------------------------------ 3. the reference's own fp32 error
def reference_float32(pc):
    """The same scatter the way the reference does it: fp32 positions (render_field's expressions), then F.grid_sample's
    backward through the port's _vm_lookup, handed the same fp32 upstream."""
    fld = pc["fld"]
    rays, z = torch.from_numpy(pc["rays"]), torch.from_numpy(pc["z"])[None]
    o, d = rays[:, :3], rays[:, 3:6]
    dh = d / torch.norm(d, dim=-1, keepdim=True)
    x = o[:, None, :] + dh[:, None, :] * z[..., None]
    m = x.abs().amax(dim=-1, keepdim=True).clamp(min=1e-6)
    x = torch.where(m <= 1, x, ((2 * m - 1) / (m ** 2)) * x)
    aabb = torch.from_numpy(fld["aabb"])
    u = ((x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1).reshape(-1, 3)
    out = {}
    ent = torch.from_numpy(np.nonzero(pc["gf32"])[0])
    for kind, Cn in sc.KINDS:
        planes = [torch.from_numpy(fld[f"{kind}_plane.{p}"]).clone().requires_grad_(True) for p in range(3)]
        lines = [torch.from_numpy(fld[f"{kind}_line.{p}"]).clone().requires_grad_(True) for p in range(3)]
        if kind == "density":
            uu = u[ent]
            up = [torch.from_numpy(pc["gf32"])[ent][None].expand(Cn, -1)] * 3
        else:
            uu = u[torch.from_numpy(pc["lin"])]
            dX = torch.from_numpy(pc["dX32"])
            up = [dX[:, p, :].T for p in range(3)]
        if uu.shape[0]:
            pp, ll = ot._vm_lookup(planes, lines, uu)
            sum((a * b * g).sum() for a, b, g in zip(pp, ll, up)).backward()
        for p in range(3):
            for what, t in (("plane", planes[p]), ("line", lines[p])):
                out[f"{kind}_{what}.{p}"] = t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32)
    return out


_KAPPA = {}


def kappa_ref(case):
    """max over the cells with A > 0 of all twelve tensors of |g32 - G| / A, and the number of non-zero cells where A = 0."""
    if case.name not in _KAPPA:
        pc = port_case(case)
        g32 = reference_float32(pc)
        worst, strays = 0.0, 0
        for name in sc.NAMES:
            G, A, m = pc["ref"][name]
            _, stray, w, _ = sc.cell_errors(g32[name], G, A, m, 0.0, 0.0)
            worst, strays = max(worst, w), strays + stray
        _KAPPA[case.name] = (worst, strays)
    return _KAPPA[case.name]


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_reference_float32_scatter_error(case):
    """kappa_ref per case (docs/SCATTER_FIGURES.md), under a loose sanity bound: an fp32 position is ~1e-7 of the axis off,
    1e-4 of a cell at 1440 cells; a wrong tap would give ~1."""
    worst, strays = kappa_ref(case)
    info = port_case(case)["info"]
    print("kappa_ref %-16s %.3e   entries: density %d, appearance %d" % (case.name, worst, info["n_density"], info["n_app"]))
    assert strays == 0, (case.name, strays)               # POS_SLACK holds for the reference's own fp32 positions
    assert worst <= 2 * sc.KAPPA_REF_MAX, (case.name, worst)


def test_kappa_constant_is_the_measured_maximum():
    """sc.KAPPA_REF_MAX, which sets the GPU bar, is the largest kappa_ref over the case list (1.9529e-4) to four digits: the
    measurement is never above it and at most 3 % below."""
    worst = max(kappa_ref(c)[0] for c in sc.CASES)
    assert 0.97 * sc.KAPPA_REF_MAX <= worst <= sc.KAPPA_REF_MAX, worst
    assert sc.KAPPA_MARGIN == 4.0


# ------------------------------------------------------------------ 4. the engine choice
DET, FIX, CAS_FUSED, CAS_SPLIT = 0, 1, 2, 3
LDS_LIMIT = 160 * 1024
TILE = 33 * 33


def plan(lib, ll_max, det=0, bits=1):
    out = (C.c_int64 * 8)()
    rc = lib.lrf_debug_scatter_plan(ll_max, det, bits, out)
    return rc, [int(v) for v in out]


@pytest.mark.parametrize("bits,ll,dens,app,app_ch", [
    (1, 479, FIX, FIX, 8), (1, 480, FIX, FIX, 4), (1, 661, FIX, FIX, 4), (1, 662, FIX, CAS_SPLIT, 8),
    (1, 1439, FIX, CAS_SPLIT, 8), (1, 1440, CAS_SPLIT, CAS_SPLIT, 8),
    (17, 596, CAS_FUSED, CAS_FUSED, 8), (17, 597, CAS_FUSED, CAS_SPLIT, 8), (17, 959, CAS_FUSED, CAS_SPLIT, 8),
    (17, 960, CAS_SPLIT, CAS_SPLIT, 8)])
def test_engine_thresholds(built_lib, bits, ll, dens, app, app_ch):
    rc, o = plan(built_lib, ll, 0, bits)
    assert rc == 0 and o[:4] == [dens, app, 8, app_ch], (ll, o)
    # the LDS each kernel is launched with: derived here from the accumulators' sizes, not read back from the library
    want_d = {FIX: 2 * 4 * 8 * (TILE + ll), CAS_FUSED: 4 * 8 * (TILE + ll), CAS_SPLIT: 4 * 8 * TILE}[dens]
    want_a = {FIX: 8 * (app_ch * TILE + 24 * ll), CAS_FUSED: 4 * 24 * (TILE + ll), CAS_SPLIT: 4 * 24 * TILE}[app]
    assert o[4:] == [want_d, want_a, 4 * 8 * ll, 4 * 24 * ll], (ll, o)
    assert max(o[4:]) <= LDS_LIMIT


def test_engine_choice_elsewhere(built_lib):
    """Engine 25 keeps the lines apart at every size; 257 is fixed point for the density only; 1025 has no four-channel sweeps;
    the deterministic mode takes the int64 image whatever the switches say, up to 640 cells, and refuses from 641 on -- what
    lrf_render_bwd's refusal says; bad arguments are refused; a negative engine reads the process's own switch."""
    assert plan(built_lib, 64, 0, 25)[1][:2] == [CAS_SPLIT, CAS_SPLIT]
    assert plan(built_lib, 64, 0, 257)[1][:2] == [FIX, CAS_FUSED]
    assert plan(built_lib, 480, 0, 1025)[1][:4] == [FIX, CAS_FUSED, 8, 8] and plan(built_lib, 479, 0, 1025)[1][:4] == [FIX, FIX, 8, 8]
    for bits in (1, 17, 25):
        assert plan(built_lib, 479, 1, bits) == (0, plan(built_lib, 479, 1, 1)[1])
        assert plan(built_lib, 479, 1, bits)[1][:4] == [DET, DET, 8, 8]
        assert plan(built_lib, 480, 1, bits)[1][:4] == [DET, DET, 8, 4]
        assert plan(built_lib, 640, 1, bits)[0] == 0 and plan(built_lib, 641, 1, bits)[0] == 1
    assert max(plan(built_lib, 640, 1, 1)[1][4:6]) <= LDS_LIMIT
    assert plan(built_lib, 0, 0, 1)[0] == -1 and built_lib.lrf_debug_scatter_plan(64, 0, 1, None) == -1
    try:
        built_lib.lrf_debug_set_train_fwd_engine(17)
        assert plan(built_lib, 64, 0, -1)[1][:2] == [CAS_FUSED, CAS_FUSED]
    finally:
        built_lib.lrf_debug_set_train_fwd_engine(1)
    assert plan(built_lib, 64, 0, -1)[1][:2] == [FIX, FIX]


def test_debug_entries_are_declared():
    from localrf_amd import _native as N
    assert "lrf_debug_scatter_plan" in N.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "lrf_debug.h")).read()
    assert "lrf_debug_scatter_plan(" in hdr
    assert "lrf_debug_workspace_vmax_bwd" in N.SYMBOLS and "lrf_debug_workspace_vmax_bwd(" in hdr


def test_deterministic_refusal_names_its_first_refused_length(built_lib):
    """LRF_FLAG_DETERMINISTIC accepts every line the reference reaches (640 cells) and refuses 641, with the text that says so.
    Fake device pointers: the refusal comes before any HIP call."""
    from localrf_amd import _native as N
    fake = C.c_void_p(FAKE)

    def bwd(n):
        f = N.LrfField(cache=fake, feature_c=128)
        f.grid[:] = [n, 17, 19]
        return built_lib.lrf_render_bwd(C.byref(f), C.byref(N.LrfParams()), fake, fake, 64, 64, N.LRF_FLAG_DETERMINISTIC, fake, fake,
                                        C.byref(N.LrfGrads()), fake, fake, None)
    assert "DETERMINISTIC covers lines up to 640 cells" in refused(built_lib, bwd(641))
    assert "line too long" in refused(built_lib, bwd(2000))
    # (640 itself is accepted: test_engine_choice_elsewhere, and on the device tests/test_gpu_scatter.py runs it)
