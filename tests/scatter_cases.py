"""The gradient scatter as an operation: a float64 restatement in plain numpy, the case list and the per-cell bar that
tests/test_scatter_host.py (no GPU) and tests/test_gpu_scatter.py (MI355X) share.

The scatter turns per-sample upstream gradients into the gradients of the twelve plane and line tensors: for plane p, entry s
and channel c, plane cell (y, x) receives dx * L * w (L: the line value interpolated at the sample, w: the bilinear weight of
the tap) and line cell l receives dx * P * wl (P: the plane value interpolated at the sample).  Positions follow
oracle/vm_render_torch.py::render_field (unit direction, o + dhat z, the contraction, the aabb normalisation), taps follow
ATen's align_corners=True border clamp (tap1d in csrc/lrf_common.h).  No torch autograd in here.

Per tensor the restatement returns
  G  the signed float64 sum,
  A  the incoming magnitude: the sum of |dx * L| (planes) or |dx * P| (lines) over the entries that touch the cell, NOT
     weighted by the tap weight -- a rounding of the position moves a weight by an absolute amount, so this is the unit an
     error is measured in,
  m  the number of contributions.
An entry "touches" the two (line) or four (plane) cells of its taps, and -- for A and m only -- the next cell over when its
float64 position lies within POS_SLACK of a cell boundary: an fp32 evaluation of the same position may land on the other side
of the boundary and add a contribution of weight ~1e-7 there, so such a cell cannot be required to stay exactly zero.
POS_SLACK = 2^-20 of the axis (1e-6 (size - 1) cells): the fp32 position is a handful of roundings of values up to 2 away
from its float64 value, 2^-22 of the axis at most.  Such a cell is not exempt: the entry's whole |dx * L| is in its A, so what a
kernel writes there must stay under kappa times it -- a weight of 8e-4 at most -- and a cell no entry comes that near must hold
exactly 0.0.

A is a sound unit of error only while the interpolated values L and P carry no cancellation of their own: where a line's two
taps have opposite signs, L can be 1e-5 of either term, an fp32 (or float64) evaluation of L is then off by 1e-2 (1e-11) of L,
and so is every contribution through it, whatever the scatter does.  The cases' fields therefore hold the magnitudes of the
reference's 0.1 randn initialisation: planes and lines are non-negative, the upstream gradients keep both signs, and every
sum the scatter itself forms still cancels.  One case, signed_33_32_65, keeps the signed initialisation, so that negative
plane and line values pass through the kernels' products and fixed-point conversion; its A is in the unit "terms": |dx| times
the interpolation of the taps' magnitudes, which no cancellation shrinks (and which equals |dx * L| on a non-negative field).
"""
import numpy as np

MAT_MODE = ((0, 1), (0, 2), (1, 2))
VEC_MODE = (2, 1, 0)
BTILE = 32
POS_SLACK = 2.0 ** -20
KINDS = (("density", 8), ("app", 24))
NAMES = tuple(f"{kind}_{what}.{p}" for kind, _ in KINDS for what in ("plane", "line") for p in range(3))
AABB = np.array([[-2.0, -2, -2], [2, 2, 2]])


# ------------------------------------------------------------------ the restatement
def positions(rays, z, aabb):
    """Normalised sample coordinates u [R * S, 3], float64 (render_field's formulas)."""
    rays, z, aabb = np.asarray(rays, np.float64), np.asarray(z, np.float64).reshape(-1), np.asarray(aabb, np.float64)
    o, d = rays[:, :3], rays[:, 3:6]
    dh = d / np.sqrt((d * d).sum(-1, keepdims=True))
    x = o[:, None, :] + dh[:, None, :] * z[None, :, None]
    m = np.maximum(np.abs(x).max(-1, keepdims=True), 1e-6)
    x = np.where(m <= 1, x, ((2 * m - 1) / (m * m)) * x)
    u = (x - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1
    return u.reshape(-1, 3)


def tap(u, size):
    """ATen's unnormalize (align_corners=True) + border clip: base tap, clamped +1 tap, fractional weight, and the range of
    cells [lo, hi] the entry can touch when its position moves by POS_SLACK of the axis."""
    ix = np.clip(((u + 1.0) * 0.5) * (size - 1), 0.0, size - 1.0)
    i0 = np.floor(ix).astype(np.int64)
    t = ix - i0
    i1 = np.minimum(i0 + 1, size - 1)
    d = POS_SLACK * (size - 1)
    lo = np.floor(np.clip(ix - d, 0.0, size - 1.0)).astype(np.int64)
    hi = np.minimum(np.floor(np.clip(ix + d, 0.0, size - 1.0)).astype(np.int64) + 1, size - 1)
    return i0, i1, t, lo, hi


def _sum_into(ncell, idx, vals):
    """[C, ncell]: out[c, idx[j]] += vals[c, j]."""
    return np.stack([np.bincount(idx, weights=v, minlength=ncell) for v in vals])


def scatter_group(planes, lines, u, dx, unit="value"):
    """One tensor group.  planes[p] [1,C,H,W], lines[p] [1,C,L,1] (any float dtype); u [n,3] float64; dx [n,3,C] upstream per
    entry, plane and channel.  Returns ({"plane.p" / "line.p": (G, A, m)}, vmax): G, A shaped like the tensor, m [H,W] / [L];
    vmax = the largest |dx * L| or |dx * P| of the group (what the kernels' largest-contribution word bounds).
    unit "terms": A counts |dx| times the interpolation of the taps' MAGNITUDES (|a| (1 - t) + |b| t for L, the bilinear sum of
    the four |taps| for P) instead of |dx * L|, |dx * P|: the unit for a field with both signs (module docstring)."""
    out, vmax = {}, 0.0
    n = u.shape[0]
    dx = np.asarray(dx, np.float64).reshape(n, 3, planes[0].shape[1])
    for p in range(3):
        Pl = np.asarray(planes[p], np.float64)[0]                       # [C,H,W]
        Ln = np.asarray(lines[p], np.float64)[0, :, :, 0]               # [C,L]
        C, H, W = Pl.shape
        L = Ln.shape[1]
        x0, x1, tx, xlo, xhi = tap(u[:, MAT_MODE[p][0]], W)
        y0, y1, ty, ylo, yhi = tap(u[:, MAT_MODE[p][1]], H)
        l0, l1, tl, llo, lhi = tap(u[:, VEC_MODE[p]], L)
        d = dx[:, p, :].T                                               # [C,n]
        Lv = Ln[:, l0] * (1 - tl) + Ln[:, l1] * tl
        ws = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
        cells = (y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1)
        Pf = Pl.reshape(C, -1)
        Pv = sum(Pf[:, c] * w for c, w in zip(cells, ws))
        dP, dL = d * Lv, d * Pv
        if unit == "terms":
            aP = np.abs(d) * (np.abs(Ln[:, l0]) * (1 - tl) + np.abs(Ln[:, l1]) * tl)
            aL = np.abs(d) * sum(np.abs(Pf[:, c]) * w for c, w in zip(cells, ws))
        else:
            aP, aL = np.abs(dP), np.abs(dL)
        if n:
            vmax = max(vmax, float(np.abs(dP).max()), float(np.abs(dL).max()))
        G = sum(_sum_into(H * W, c, dP * w) for c, w in zip(cells, ws)) if n else np.zeros((C, H * W))
        A, m = np.zeros((C, H * W)), np.zeros(H * W)
        for dy in range(3):
            for dxo in range(3):
                on = (ylo + dy <= yhi) & (xlo + dxo <= xhi)
                if on.any():
                    idx = ((ylo + dy) * W + xlo + dxo)[on]
                    A += _sum_into(H * W, idx, aP[:, on])
                    m += np.bincount(idx, minlength=H * W)
        out[f"plane.{p}"] = (G.reshape(1, C, H, W), A.reshape(1, C, H, W), m.reshape(H, W))
        G = (_sum_into(L, l0, dL * (1 - tl)) + _sum_into(L, l1, dL * tl)) if n else np.zeros((C, L))
        A, m = np.zeros((C, L)), np.zeros(L)
        for dl in range(3):
            on = llo + dl <= lhi
            if on.any():
                A += _sum_into(L, (llo + dl)[on], aL[:, on])
                m += np.bincount((llo + dl)[on], minlength=L)
        out[f"line.{p}"] = (G.reshape(1, C, L, 1), A.reshape(1, C, L, 1), m)
    return out, vmax


def scatter_ref(fld, rays, z, gf, lin, dX, unit="value"):
    """The whole scatter.  fld: the field's twelve tensors and "aabb" by state-dict name (numpy); rays [R,6]; z [S]; gf [R * S]
    the density group's upstream per sample (0 = no entry); lin [n] = ray * S + k of the shaded samples and dX [n,3,24] their
    appearance upstream rows.  Returns {tensor name: (G, A, m)} for the twelve tensors and info = {"vmax_density",
    "vmax_app", "n_density", "n_app"} (entry counts: every plane of a group holds the same entries)."""
    u = positions(rays, z, fld["aabb"])
    gf = np.asarray(gf, np.float64).reshape(-1)
    ent = np.nonzero(gf)[0]
    res, info = {}, {}
    for kind, C in KINDS:
        planes = [fld[f"{kind}_plane.{p}"] for p in range(3)]
        lines = [fld[f"{kind}_line.{p}"] for p in range(3)]
        if kind == "density":
            uu, dx = u[ent], np.broadcast_to(gf[ent][:, None, None], (ent.size, 3, C))
        else:
            lin = np.asarray(lin, np.int64).reshape(-1)
            uu, dx = u[lin], np.asarray(dX, np.float64).reshape(lin.size, 3, C)
        grp, vmax = scatter_group(planes, lines, uu, dx, unit)
        for k, v in grp.items():
            res[f"{kind}_{k}"] = v
        info[f"vmax_{kind}"], info[f"n_{kind}"] = vmax, int(uu.shape[0])
    return res, info


# ------------------------------------------------------------------ the bar
def fixed_point_quantum(vmax, n_p):
    """The quantum of the fixed-point engines for a group whose largest |contribution| is at most vmax and whose planes hold n_p
    entries each: 2^(vex - min(46, 62 - bits(4 n_p))), vex the binade above vmax plus one (the kernels' own word holds the fp32
    maximum of the same products; one binade covers its rounding).  This is the bound the comment above det_shift
    (csrc/lrf_backward.inl) derives; the non-deterministic kernel scales by a workgroup's segment, never coarser."""
    if vmax <= 0.0 or n_p == 0:
        return 0.0
    vex = int(np.frexp(vmax)[1]) + 1
    return float(np.ldexp(1.0, vex - min(46, 62 - int(4 * n_p).bit_length())))


def cell_errors(got, G, A, m, kappa, quantum):
    """The per-cell bar |got - G| <= kappa A + floor, floor = (m / 2 + 1) quantum (0 for the compare-and-swap engines), and
    exactly 0.0 where A = 0.  Returns (number of cells over the bar, number of non-zero cells where A = 0, worst |err| / A
    over the cells with A > 0, worst err / bar)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - G)
    floor = (np.asarray(m, np.float64).reshape((1, 1) + A.shape[2:]) / 2 + 1) * quantum
    bar = kappa * A + floor
    hit = A > 0
    stray = int(np.count_nonzero(got[~hit]))
    over = int(np.count_nonzero(err[hit] > bar[hit]))
    worst = float((err[hit] / A[hit]).max()) if hit.any() else 0.0
    barred = hit & (bar > 0)
    share = float((err[barred] / bar[barred]).max()) if barred.any() else 0.0
    return over, stray, worst, share


# ------------------------------------------------------------------ the cases
class Case:
    """grid, R rays of S samples, seeds; engine: lrf_debug_set_train_fwd_engine bits; field: TensorVMSplit keyword overrides;
    masked: an all-zero alpha mask; expect: the coverage conditions tests/test_scatter_host.py proves from the reference alone
      edges    A > 0 in the first and last row, column and line cell of every plane and line (density and appearance)
      edges_d  the same for the density tensors only
      borders  A > 0 at a cell on every shared tile border (x or y a multiple of 32) of every plane
      tiles_full   every tile of a plane of more than one tile holds entries (density and appearance)
      tiles_empty  some tile of a plane holds no entry
               An entry is binned by its base tap, and a base tap never lies in a plane's last cell unless the sample is
               clamped there; so a side of 33 or 65 cells leaves its last tile empty and no plane with such a side is ever full,
               and where no side is 1 mod 32 (32 x 64 x 34, the line cases) or the aabb clamps (clamp_33_33_17) rays in every
               direction fill every tile.  Only tile_64_34_33 has both: planes of 64 x 34 (full) and of 64 x 33, 34 x 33.
      run17    17 or more consecutive samples of a ray share a plane cell (the run crosses a 16-lane row)
      long90   at least 90 % of the cells of the longest line have A > 0 (density and appearance)
      corner17 17 or more consecutive samples of a ray are clamped onto the last cell of plane 0, which is the first cell of its
               tile: the one run whose key in k_scatter_fix's seg_run is 0, what a lane shift reads past the start of a row
    half: the aabb is [-half, half]^3 (2: the contraction's range, nothing is clamped)
    unit: "value" = non-negative planes and lines, A in |dx * L|; "terms" = the signed initialisation, A in |dx| x the taps' magnitudes"""

    def __init__(self, name, grid, R, S, engine=1, expect=("edges",), field=None, masked=False, seed=0, half=2.0, unit="value"):
        self.name, self.grid, self.R, self.S, self.engine, self.half, self.unit = name, list(grid), R, S, engine, half, unit
        self.expect, self.field, self.masked, self.seed = frozenset(expect), dict(field or {}), masked, seed

    def __repr__(self):
        return self.name


# Far samples (z up to 1e3) contract to within 1e-3 of the aabb's faces: a ray along +-axis reaches the first and last cell
# of that axis.  With the reference's density_shift -5 the transmittance is spent by z ~ 40 and nothing behind is shaded; the
# long-line cases take density_shift -10 and a weight threshold of 1e-7, so that every sample of a ray is shaded and the
# appearance entries reach both ends of a 1440-cell line.
THIN = dict(density_shift=-10, rayMarch_weight_thres=1e-7)
TILE_CASES = [
    Case("tile_33_32_65", [33, 32, 65], 96, 96, expect=("edges", "borders", "tiles_empty"), field=THIN),
    Case("tile_64_34_33", [64, 34, 33], 96, 96, expect=("edges", "borders", "tiles_full", "tiles_empty"), field=THIN),
    Case("tile_65_65_17", [65, 65, 17], 96, 96, expect=("edges", "borders", "tiles_empty"), field=THIN),
    Case("tile_32_64_34", [32, 64, 34], 96, 96, expect=("edges", "borders", "tiles_full"), field=THIN),
    Case("tiny_2_2_2", [2, 2, 2], 16, 128, expect=("edges", "run17")),
    Case("signed_33_32_65", [33, 32, 65], 96, 96, expect=("edges", "borders", "tiles_empty"), field=THIN, unit="terms"),
    # an aabb inside the contraction's range: every sample beyond it is clamped onto the border cells (both taps on one cell)
    Case("clamp_33_33_17", [33, 33, 17], 96, 96, expect=("edges", "borders", "tiles_full", "run17", "corner17"), field=THIN, half=1.0),
]
LINE_CASES = (
    [Case(f"line_{n}", [n, 17, 19], 128, 128, expect=("edges", "borders", "tiles_full", "long90"), field=THIN) for n in (479, 480, 661, 662, 1439, 1440)]
    + [Case(f"line_{n}_cas", [n, 19, 17], 128, 128, engine=17, expect=("edges", "borders", "tiles_full", "long90"), field=THIN) for n in (596, 597, 959, 960)]
    + [Case("line_640", [640, 17, 19], 128, 128, expect=("edges", "borders", "tiles_full", "long90"), field=THIN),   # the deterministic mode's longest line
       Case("line_480_mid", [21, 480, 18], 128, 128, expect=("edges", "borders", "tiles_full", "long90"), field=THIN),
       Case("line_480_last", [18, 23, 480], 128, 128, expect=("edges", "borders", "tiles_full", "long90"), field=THIN)]
)
COUNT_CASES = [
    Case("count_4032", [20, 24, 28], 63, 64),
    Case("count_4096", [20, 24, 28], 64, 64),
    Case("count_4160", [20, 24, 28], 65, 64),
    Case("count_2", [20, 24, 28], 1, 2, expect=()),
]
ROW_CASES = [
    Case("rows_last_only", [33, 32, 65], 96, 96, expect=("edges_d", "tiles_empty"), field=dict(density_shift=-30)),
    Case("masked", [33, 32, 65], 96, 96, expect=("tiles_empty",), masked=True),
]
CASES = TILE_CASES + LINE_CASES + COUNT_CASES + ROW_CASES
BY_NAME = {c.name: c for c in CASES}
# kappa of the GPU bar: KAPPA_MARGIN x the largest kappa_ref over CASES, the reference's own fp32 scatter against float64 as
# tests/test_scatter_host.py measures it: 1.9529e-4, at line_1439 (docs/SCATTER_FIGURES.md).  The constant is that measurement
# to four digits; the host test fails when its own measurement is above it or more than 3 % below.  Nothing measured on a kernel
# enters.
KAPPA_REF_MAX = 1.953e-4
KAPPA_MARGIN = 4.0


def case_rays(case):
    """[R,6] float32: origins near the centre, the first six directions along +-x, +-y, +-z (slightly off axis), two along +-(x + y), the rest uniform
    on the sphere and not normalised to length 1 (the kernels divide)."""
    g = np.random.default_rng(1000 + case.seed + 7 * case.R + case.S)
    o = 0.05 * g.standard_normal((case.R, 3))
    d = g.standard_normal((case.R, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    for i in range(min(6, case.R)):
        d[i] = 0.02 * g.standard_normal(3)
        d[i, i // 2] = 1.0 if i % 2 == 0 else -1.0
    if case.R >= 8:                      # ... and two along the diagonal of plane 0
        d[6] = (1.0, 1.0, 0.01)
        d[7] = (-1.0, -1.0, -0.01)
    d *= g.uniform(0.5, 2.0, (case.R, 1))
    return np.concatenate([o, d], -1).astype(np.float32)


def case_z(case):
    """[S] float32: the reference's eval schedule with S samples (half linear in [0.1, 1.1), half inverse depth), its last three
    distances moved out to 400, 650 and 1000: the schedule's own last step ends near z = 60, which contracts to 0.4 % short of
    the aabb's face -- more than a cell of the long lines -- and a ray's last sample is never a density entry."""
    from oracle import vm_render_np as onp
    z = onp.z_schedule(3 * case.S, np.float32).reshape(-1).copy()
    assert z.size == case.S
    if case.S >= 16:
        z[-3:] = (400.0, 650.0, 1000.0)
    return z


def case_upstream(case):
    """g_rgb [R,3], g_depth [R] float32."""
    g = np.random.default_rng(2000 + case.seed + case.R)
    return g.standard_normal((case.R, 3)).astype(np.float32), g.standard_normal(case.R).astype(np.float32)


def case_field(case, device="cpu"):
    """The TensorVMSplit of a case, parameters drawn on the CPU generator (the same on every machine)."""
    import torch
    from util import make_field, quiet
    from localrf_amd import AlphaGridMask
    f = quiet(make_field, case.grid, "cpu", seed=300 + case.seed, **case.field)
    if case.half != 2.0:                 # (make_field's aabb is [-2, 2]^3)
        from localrf_amd import TensorVMSplit
        from util import FIELD_KW
        torch.manual_seed(300 + case.seed)
        aabb = case.half * torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
        f = quiet(TensorVMSplit, torch.device("cpu"), aabb, list(case.grid), **{**FIELD_KW, **case.field})
    with torch.no_grad():                # no cancellation inside an interpolated plane or line value: see A in the module's docstring
        for n, p in f.named_parameters():
            if n in NAMES and case.unit == "value":
                p.abs_()
    if case.masked:
        f.alphaMask = AlphaGridMask(torch.device("cpu"), f.aabb.detach().clone(), torch.zeros(8, 8, 8))
    return f if str(device) == "cpu" else f.to(device)
