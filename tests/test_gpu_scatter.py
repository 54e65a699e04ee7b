"""The gradient scatter of lrf_render_bwd on the MI355X, cell by cell against float64 (tests/scatter_cases.py).

Each run is an ordinary row-saving forward and backward() of a TensorVMSplit.  The kernels' own upstream is then read out of
the training workspace -- the per-sample density-feature gradient k_bwd_ray leaves in the `feat` buffer (it overwrites the
forward's feature there: csrc/lrf_backward.inl, "consumed by the binned scatter kernels"), rowinfo and the dX blocks of the
gradient rows -- and handed to the float64 restatement: both sides sum the same fp32 upstream values, so the comparison is of
the counting sort, the scatter kernels, k_det_convert and the engine choice alone, not of the colour network or the per-ray
backward.  Every cell of all twelve tensors must satisfy

    |kernel - G| <= kappa A + floor,    exactly 0.0 where A = 0

kappa = 4 x the reference's own fp32-against-float64 error (sc.KAPPA_REF_MAX, measured in tests/test_scatter_host.py); floor =
(m / 2 + 1) quanta for the fixed-point engines (sc.fixed_point_quantum), 0 for the compare-and-swap engines.  The figures each
run prints are collected in docs/SCATTER_FIGURES.md.  Every test that flips a process-wide debug switch restores it."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scatter_cases as sc                       # noqa: E402
from util import capture_train_ws                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KAPPA = sc.KAPPA_MARGIN * sc.KAPPA_REF_MAX
DET, FIX, CAS_FUSED, CAS_SPLIT = 0, 1, 2, 3
ENGINE_NAME = {DET: "int64 image", FIX: "fixed point", CAS_FUSED: "compare-and-swap, lines fused", CAS_SPLIT: "compare-and-swap, lines apart"}


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _plan(lib, grid, det):
    """(density engine, appearance engine, appearance channels per sweep) as lrf_render_bwd picks them right now."""
    out = (C.c_int64 * 8)()
    assert lib.lrf_debug_scatter_plan(max(grid), 1 if det else 0, -1, out) == 0
    return int(out[0]), int(out[1]), int(out[3])


_DX_INDEX = {}


def _dx_index(lib, buffer):
    """[16,72] float offsets of (row, 24 plane + channel) of the dX block inside a gradient tile, in the row-major order
    (buffer 1) or the groups order (buffer 3) of lrf_debug_saved_row_offset."""
    if buffer not in _DX_INDEX:
        base = 48 if buffer == 1 else 0
        _DX_INDEX[buffer] = np.array([[lib.lrf_debug_saved_row_offset(buffer, r, base + c) for c in range(72)] for r in range(16)], np.int64)
    return _DX_INDEX[buffer]


class Setup:
    """A case's field on the device with its rays, schedule and output gradients."""

    def __init__(self, case, scale=1.0):
        self.case = case
        self.f = sc.case_field(case, DEV)
        self.rays, self.z = sc.case_rays(case), sc.case_z(case)
        g_rgb, g_depth = sc.case_upstream(case)
        self.g_rgb, self.g_depth = torch.from_numpy(g_rgb * np.float32(scale)).to(DEV), torch.from_numpy(g_depth * np.float32(scale)).to(DEV)
        self.fld = {k: v.detach().cpu().numpy() for k, v in self.f.state_dict().items()}


def _read_upstream(lib, su, ws, app_engine):
    """gf [R S], lin [n], dX [n,3,24] as the backward left them in workspace `ws`."""
    case, f = su.case, su.f
    R, S = case.R, case.S
    out = (C.c_uint64 * 9)()
    lib.lrf_workspace_layout_bwd(R, S, (C.c_int32 * 3)(*f.layout.grid), out)
    _, grd_off, ri_off, toff_off, _, grd_ld, _, _, feat_off = [int(v) for v in out]
    tiles = int(ws[toff_off:toff_off + 4 * (R + 1)].view(torch.int32)[R])
    rows = tiles * 16
    gf = ws[feat_off:feat_off + 4 * R * S].view(torch.float32).cpu().numpy().copy()
    rowinfo = ws[ri_off:ri_off + 4 * rows].view(torch.int32).cpu().numpy()
    valid = rowinfo >= 0
    grd = ws[grd_off:grd_off + 4 * rows * grd_ld].view(torch.float32).cpu().numpy().reshape(tiles, 16 * grd_ld)
    idx = _dx_index(lib, 3 if app_engine in (DET, FIX) else 1)
    dX = grd[:, idx].reshape(rows, 3, 24)[valid]
    vm = (C.c_uint64 * 2)()
    lib.lrf_debug_workspace_vmax_bwd(R, S, (C.c_int32 * 3)(*f.layout.grid), vm)
    vmax = [float(ws[int(o):int(o) + 4].view(torch.float32).cpu()[0]) for o in vm]      # the largest-contribution words, as floats
    return gf, rowinfo[valid].astype(np.int64), dX, vmax


def run(lib, su, det=False, plane_events=False, monkeypatch=None):
    """One forward + backward; returns the twelve gradients (numpy), the upstream the kernels scattered and the engines."""
    f, case = su.f, su.case
    f.deterministic = det
    dens_eng, app_eng, app_ch = _plan(lib, case.grid, det)
    z = torch.from_numpy(su.z)
    if plane_events:                                  # the data-parallel form: one appearance pass per plane (LRF_FLAG_PLANE_EVENTS)
        from localrf_amd import _native as N
        from localrf_amd import dist
        rays, zz = torch.from_numpy(su.rays).to(DEV), z.to(DEV)
        flags = f._flags(True)
        _, _, ws, _ = f._native_forward_train(rays, zz, flags)
        monkeypatch.setattr(dist, "active", lambda: True)
        try:
            _, grads = f._native_backward(rays, zz, flags, su.g_rgb, su.g_depth, saved_ws=ws)
            assert f._grads.plane_events
            st = torch.cuda.current_stream(DEV).cuda_stream
            for bucket in (3, 4, 0, 1, 2):
                N.check(lib.lrf_render_bwd_wait(bucket, st), "lrf_render_bwd_wait")
            torch.cuda.synchronize()
        finally:
            monkeypatch.undo()
        got = {n: g.detach().cpu().numpy().reshape(su.fld[n].shape) for n, g in zip(
            [f"{k}_{w}.{p}" for k in ("density", "app") for w in ("plane", "line") for p in range(3)], grads[:12])}
    else:
        f.z_override = z.clone()
        for p in f.parameters():
            p.grad = None
        rays = torch.from_numpy(su.rays).to(DEV).clone().requires_grad_(True)
        with capture_train_ws(f) as cap:
            rgb, depth = f(rays, white_bg=True, is_train=False, N_samples=-1)
            ((rgb * su.g_rgb).sum() + (depth * su.g_depth).sum()).backward()
            torch.cuda.synchronize()
            ws = cap.ws
        f.z_override = None
        named = dict(f.named_parameters())
        got = {n: named[n].grad.detach().cpu().numpy() for n in sc.NAMES}
    gf, lin, dX, vmax = _read_upstream(lib, su, ws, app_eng)
    return dict(got=got, gf=gf, lin=lin, dX=dX, vmax=vmax, engines=(dens_eng, app_eng, app_ch))


_REF = {}


def reference(su, r):
    """The float64 restatement for the upstream of run r (one evaluation per distinct upstream)."""
    h = hashlib.sha256()
    for a in (r["gf"], r["lin"], r["dX"]):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (su.case.name, h.hexdigest())
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()
        _REF[key] = sc.scatter_ref(su.fld, su.rays, su.z, r["gf"], r["lin"], r["dX"], su.case.unit)
    return _REF[key]


def check(su, r, what=""):
    """The per-cell bar on all twelve tensors; prints the figures of docs/SCATTER_FIGURES.md."""
    ref, info = reference(su, r)
    worst = {"density": (0.0, 0.0), "app": (0.0, 0.0)}
    quanta = {}
    for kind, eng in (("density", r["engines"][0]), ("app", r["engines"][1])):
        quanta[kind] = sc.fixed_point_quantum(info[f"vmax_{kind}"], info[f"n_{kind}"]) if eng in (DET, FIX) else 0.0
    # the kernels' largest-contribution word (the fp32 maximum of the same products) is what the floor's binade stands for:
    # within a factor of two of the float64 maximum wherever the group has entries and runs on fixed point
    for q, (kind, eng) in enumerate((("density", r["engines"][0]), ("app", r["engines"][1]))):
        if eng in (DET, FIX) and info[f"n_{kind}"]:
            assert 0.5 * info[f"vmax_{kind}"] <= r["vmax"][q] <= 2.0 * info[f"vmax_{kind}"], (su.case.name, kind, r["vmax"][q], info[f"vmax_{kind}"])
    bad = []
    for name in sc.NAMES:
        kind = name.split("_")[0]
        G, A, m = ref[name]
        over, stray, w, share = sc.cell_errors(r["got"][name], G, A, m, KAPPA, quanta[kind])
        worst[kind] = (max(worst[kind][0], w), max(worst[kind][1], share))
        if over or stray:
            bad.append((name, over, stray, w, share))
    print("scatter %-16s %-10s density [%s, %d entries, quantum %.1e]: worst |err|/A %.2e, err/bar %.2e;  appearance [%s x%d, %d entries, "
          "quantum %.1e]: worst |err|/A %.2e, err/bar %.2e" % (
              su.case.name, what, ENGINE_NAME[r["engines"][0]], info["n_density"], quanta["density"], worst["density"][0], worst["density"][1],
              ENGINE_NAME[r["engines"][1]], r["engines"][2], info["n_app"], quanta["app"], worst["app"][0], worst["app"][1]))
    assert not bad, (su.case.name, what, bad)
    return info


def _with_engine(lib, bits, fn):
    try:
        lib.lrf_debug_set_train_fwd_engine(bits)
        return fn()
    finally:
        lib.lrf_debug_set_train_fwd_engine(1)


# ------------------------------------------------------------------ tile edges, line thresholds, entry counts
TILE_RUNS = [(c.name, e) for c in sc.TILE_CASES for e in (1, 17)] + [("tile_33_32_65", 25)]


@pytest.mark.parametrize("name,engine", TILE_RUNS, ids=lambda v: str(v))
def test_tile_edges(built_lib, name, engine):
    """Plane sides of 32, 33, 34, 64 and 65 cells as x and as y of a plane, and the 2^3 grid whose runs are 64 lanes long:
    fixed point (1), compare-and-swap with the lines fused (17) and apart (25)."""
    su = Setup(sc.BY_NAME[name])
    r = _with_engine(built_lib, engine, lambda: run(built_lib, su))
    assert r["engines"][:2] == {1: (FIX, FIX), 17: (CAS_FUSED, CAS_FUSED), 25: (CAS_SPLIT, CAS_SPLIT)}[engine]
    info = check(su, r, "engine %d" % engine)
    assert info["n_density"] > 0 and info["n_app"] > 0


LINE_ENGINES = {"line_479": (FIX, FIX, 8), "line_480": (FIX, FIX, 4), "line_661": (FIX, FIX, 4), "line_662": (FIX, CAS_SPLIT, 8),
                "line_1439": (FIX, CAS_SPLIT, 8), "line_1440": (CAS_SPLIT, CAS_SPLIT, 8), "line_640": (FIX, FIX, 4),
                "line_596_cas": (CAS_FUSED, CAS_FUSED, 8), "line_597_cas": (CAS_FUSED, CAS_SPLIT, 8),
                "line_959_cas": (CAS_FUSED, CAS_SPLIT, 8), "line_960_cas": (CAS_SPLIT, CAS_SPLIT, 8),
                "line_480_mid": (FIX, FIX, 4), "line_480_last": (FIX, FIX, 4)}


@pytest.mark.parametrize("case", sc.LINE_CASES, ids=repr)
def test_line_thresholds(built_lib, case):
    """Either side of every length at which lrf_render_bwd changes engine, and 480 cells along each of the three axes."""
    su = Setup(case)
    r = _with_engine(built_lib, case.engine, lambda: run(built_lib, su))
    assert r["engines"] == LINE_ENGINES[case.name]
    check(su, r, "engine %d" % case.engine)


@pytest.mark.parametrize("case", sc.COUNT_CASES, ids=repr)
def test_entry_counts_around_a_fill_block(built_lib, case):
    """R S = 4032, 4096 and 4160 entries (k_bin_fill takes 4096 per block) and the smallest batch, one ray of two samples."""
    su = Setup(case)
    r = run(built_lib, su)
    info = check(su, r)
    if case.R == 1:
        assert info["n_density"] == 1 and info["n_app"] >= 1


def test_only_the_last_sample_of_each_ray_is_shaded(built_lib):
    """density_shift = -30: the appearance rows are the forced last samples alone, one per ray, in tiles of one row."""
    su = Setup(sc.BY_NAME["rows_last_only"])
    r = run(built_lib, su)
    assert r["lin"].size == su.case.R and np.all(r["lin"] % su.case.S == su.case.S - 1)
    check(su, r)


def test_fully_masked_field(built_lib):
    """An all-zero alpha mask: no density entry at all, the six density gradients exactly zero.  (The reference still shades
    every ray's last sample, whose alpha is forced to 1 behind the mask: the appearance tensors stay under the per-cell bar.)"""
    su = Setup(sc.BY_NAME["masked"])
    r = run(built_lib, su)
    assert not r["gf"].any()
    for n in sc.NAMES[:6]:
        assert not r["got"][n].any(), n
    check(su, r)


def test_zero_upstream(built_lib):
    """g_rgb = g_depth = 0: every plane and line gradient is exactly zero and both largest-contribution words are zero, on the
    fixed-point, compare-and-swap and deterministic engines.  A run with the case's own upstream goes first through the same
    workspace size, and its words are not zero: a word k_clear_bins left alone would show."""
    case = sc.BY_NAME["tile_64_34_33"]
    live = run(built_lib, Setup(case))
    assert live["vmax"][0] > 0 and live["vmax"][1] > 0, live["vmax"]
    su = Setup(case, scale=0.0)
    for engine in (1, 17):
        r = _with_engine(built_lib, engine, lambda: run(built_lib, su))
        assert not r["gf"].any() and not r["dX"].any()
        assert r["vmax"] == [0.0, 0.0], (engine, r["vmax"])
        for n in sc.NAMES:
            assert not r["got"][n].any(), (engine, n)
    r = run(built_lib, su, det=True)
    assert r["vmax"] == [0.0, 0.0], ("deterministic", r["vmax"])
    for n in sc.NAMES:
        assert not r["got"][n].any(), ("deterministic", n)


# ------------------------------------------------------------------ shares
@pytest.mark.parametrize("name", ["tile_64_34_33", "line_480"])
def test_shares(built_lib, name, monkeypatch):
    """1, 2, 7, the default and 4 x CUs workgroups: with one, flush_line runs between planes; with 4 x CUs most shares are empty.
    The multi-tile case once more as three per-plane passes."""
    su = Setup(sc.BY_NAME[name])
    try:
        for wgs in (1, 2, 7, 0, 4 * _cus()):
            built_lib.lrf_debug_set_scatter_wgs(wgs)
            check(su, run(built_lib, su), "wgs %d" % wgs)
        built_lib.lrf_debug_set_scatter_wgs(0)
        if name == "tile_64_34_33":
            check(su, run(built_lib, su, plane_events=True, monkeypatch=monkeypatch), "per plane")
    finally:
        built_lib.lrf_debug_set_scatter_wgs(0)


# ------------------------------------------------------------------ deterministic mode
def _same_bits(a, b, what):
    bad = [n for n in sc.NAMES if a[n].tobytes() != b[n].tobytes()]
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", [c.name for c in sc.TILE_CASES] + ["line_480", "line_640"])
def test_deterministic_mode(built_lib, name):
    """LRF_FLAG_DETERMINISTIC: the per-cell bar, and the same bits whatever the number of workgroups."""
    su = Setup(sc.BY_NAME[name])
    runs = {}
    try:
        for wgs in (0, 1, 2, 7, 4 * _cus()):
            built_lib.lrf_debug_set_scatter_wgs(wgs)
            runs[wgs] = run(built_lib, su, det=True)
    finally:
        built_lib.lrf_debug_set_scatter_wgs(0)
    assert runs[0]["engines"][:2] == (DET, DET)
    check(su, runs[0], "det")
    for wgs, r in runs.items():
        _same_bits(runs[0]["got"], r["got"], (name, wgs))


@pytest.mark.parametrize("name", ["tile_33_32_65", "line_480"])
def test_power_of_two_scaling_in_deterministic_mode(built_lib, name):
    """g_rgb and g_depth scaled by 2^-40 and 2^40, the gradients scaled back: the same bits as unscaled -- the chain is linear
    and the fixed-point scale follows the binade of the largest contribution."""
    case = sc.BY_NAME[name]
    base = run(built_lib, Setup(case), det=True)["got"]
    for k in (-40, 40):
        got = run(built_lib, Setup(case, scale=2.0 ** k), det=True)["got"]
        back = {n: (got[n].astype(np.float64) * 2.0 ** -k).astype(np.float32) for n in sc.NAMES}
        for n in sc.NAMES:
            assert np.isfinite(got[n]).all(), (k, n)
            assert np.array_equal(got[n].astype(np.float64) * 2.0 ** -k, back[n].astype(np.float64)), (k, n, "scaling back is exact")
        _same_bits(base, back, (name, k))
