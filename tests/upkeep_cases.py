"""Shared pieces of the field-upkeep kernel tests: the kernels that run between iterations and rebuild the field itself --
k_upsample_bilinear (csrc/lrf_losses.inl), k_dense_alpha / k_alpha_pool (csrc/lrf_mask.inl, with alpha_mask_sample of
lrf_common.h), k_density_feature / k_app_feature / k_sample_ray_aabb / k_sample_contracted (csrc/lrf_render.hip).  The cases, their
float64 references (oracle/vm_render_np.py in np.float64 plus a few lines of numpy here) and the measured error of the float32
CPU evaluation of the same expressions, from which the GPU tolerances follow.

  up_case / up_ref / up_check                ATen's align_corners=True bilinear formula in float64; e32 from F.interpolate
  upfield_*                                  the same through TensorVMSplit.upsample_volume_grid: twelve tensors, stepSize, nSamples
  pool_inputs / pool_ref                     clamp(0, 1), 3x3x3 max with -inf padding, >= thres: exact, no tolerance
  MASK_CASES / mask_field / mask_eval / mask_sets / mask_check
                                             getDenseAlpha + updateAlphaMask, optionally through a previous mask, and the
                                             decidable sets of the binary result
  feat_*                                     density_feature / app_feature at edge coordinates
  ray_* / con_*                              sample_ray (aabb march) and sample_ray_contracted
  tolerance, E32, SEEDS                      min(max(4 e32, FLOOR), cap); the recorded float32-CPU errors; the seeds

Decidable sets.  A binary output is asserted exactly where float64 decides it and nowhere else:
  * the validity of a lattice point under a previous mask is decidably valid when the taps with float64 weight >= W_MIN already
    sum to more than 0, decidably invalid when no in-range voxel of its closed 2x2x2 neighbourhood (the taps of every base
    index a coordinate within NEAR_PLANE of a lattice plane could floor to) holds a 1;
  * a pooled cell is decidably kept when the pooled alpha with every undecided point taken as 0 exceeds float32(thres) by more
    than the alpha tolerance, decidably dropped when the pooled alpha with every undecided point taken as valid stays further
    than the tolerance below it;
  * an `inside` flag is decidable when the float64 point is further than the pts tolerance from the surface of the box
    (inside: from every face plane; outside: beyond some face plane by more than it).

Every e32 is arithmetic on the references alone, never on a kernel's output.  Nothing here touches a GPU or the HIP library.
Cited lines are relative to the reference's localTensoRF directory."""
import functools
import zlib

import numpy as np
import torch

from losses_cases import FLOOR, one_thread  # noqa: F401  (re-exported)
from oracle import vm_render_np as onp
from util import make_field, quiet

# what the suite demands today: 1e-6 absolute on resized tensors (test_upsample_*), 2e-6 absolute on the two feature kernels
# (test_feature_kernels_vs_reference_golden), 2e-6 relative on t and pts (test_sample_ray_aabb_vs_reference_golden), 2e-6
# absolute on contracted positions; dense alpha has no bar of its own in the suite: 4 e32 with the floor
CAP = {"up": 1e-6, "sig": 2e-6, "app": 2e-6, "t": 2e-6, "pts": 2e-6, "xc": 2e-6, "alpha": None}
W_MIN = 1e-5                            # a tap below this float64 weight decides nothing
NEAR_PLANE = 1e-4                       # voxel units: this close to a lattice plane float32 may floor to either side
UNDECIDABLE_MASK, DECIDED_EACH_SIDE, UNDECIDABLE_FLAGS = 0.02, 0.10, 0.002


def tolerance(e32, quantity):
    """4 x the float32-CPU error, not below 8 roundings, not above what the suite demands already."""
    t = max(4.0 * e32, FLOOR)
    return t if CAP[quantity] is None else min(t, CAP[quantity])


def abs_err(x, ref):
    return float(np.abs(np.asarray(x, np.float64).reshape(np.shape(ref)) - ref).max()) if np.size(ref) else 0.0


def rel1_err(x, ref):
    """max |x - ref| / max(|ref|, 1) per element: the measure test_sample_ray_aabb_vs_reference_golden uses for pts."""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(x, np.float64).reshape(ref.shape) - ref) / np.maximum(np.abs(ref), 1.0)).max())


def _rng(name, seed=0):
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


# ------------------------------------------------------------------------------------------------------------------ upsample
UP_SHAPES = ([(8, 5, 7, 9, 6), (24, 20, 28, 27, 31), (8, 27, 30, 16, 12), (8, 2, 2, 257, 3), (8, 1, 6, 5, 6), (8, 6, 5, 1, 1)]   # planes
             + [(8, 16, 1, 101, 1), (24, 64, 1, 101, 1)]                                    # lines: W = W2 = 1
             + [(3, 4, 6, 5, 17), (4, 5, 3, 8, 8), (1, 9, 1, 257, 1)]                        # 255, 256, 257 output elements
             + [(24, 13, 11, 13, 11)]                                                       # the identity
             + [(24, 8, 8, 1676, 1676)])                                                    # above the launch cap
UP_CASES = ["{}x{}x{}-{}x{}".format(*s) for s in UP_SHAPES]
UP_BIG, UP_IDENTITY = UP_CASES[-1], UP_CASES[-2]
LAUNCH_CAP = 65535 * 4 * 256            # threads of the largest launch: above this many outputs the stride loop repeats
# The sources are white noise of the parameters' initial scale, 0.1 randn.  The float32 formula rounds the source index (scale x
# index, ~1e-7 relative), which costs index x slope: at the larger sizes ATen's own float32 result is further than a quarter
# of the suite's 1e-6 from float64.  There the amplitude is halved until 4 e32 fits under the cap (a power of two scales every
# figure exactly), so that the tolerance stays 4 e32 and the cap decides nothing; up_check refuses a case that needs its cap.
UP_AMP = {"24x20x28-27x31": 0.025, "8x27x30-16x12": 0.025, "24x64x1-101x1": 0.0125, "24x8x8-1676x1676": 0.05}


def up_case(name):
    """(src [C,H,W] float32, H2, W2, idx): idx the flat output elements that are checked (all, or for the case above the launch
    cap every 61st plus the last 4096)."""
    C, H, W, H2, W2 = UP_SHAPES[UP_CASES.index(name)]
    src = (UP_AMP.get(name, 0.1) * _rng(name).standard_normal((C, H, W))).astype(np.float32)
    n = C * H2 * W2
    idx = np.arange(n) if n <= LAUNCH_CAP else np.concatenate([np.arange(0, n, 61), np.arange(n - 4096, n)])
    return src, H2, W2, idx


def resize64_at(src, H2, W2, idx):
    """ATen upsample_bilinear2d, align_corners=True (UpSample.h area_pixel_compute_scale / compute_source_index), in float64
    at the flat output elements idx: source index = dst * (in - 1) / (out - 1) (0 for out = 1), the +1 tap clamped."""
    C, H, W = src.shape
    s = src.astype(np.float64)
    x2, y2, c = idx % W2, (idx // W2) % H2, idx // (W2 * H2)
    fy = y2 * ((H - 1) / (H2 - 1) if H2 > 1 else 0.0)
    fx = x2 * ((W - 1) / (W2 - 1) if W2 > 1 else 0.0)
    y0, x0 = np.minimum(np.floor(fy).astype(np.int64), H - 1), np.minimum(np.floor(fx).astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = fy - y0, fx - x0
    return (1 - ly) * ((1 - lx) * s[c, y0, x0] + lx * s[c, y0, x1]) + ly * ((1 - lx) * s[c, y1, x0] + lx * s[c, y1, x1])


def resize32(src, H2, W2):
    with one_thread():
        return torch.nn.functional.interpolate(torch.from_numpy(src)[None], size=(H2, W2), mode="bilinear", align_corners=True)[0].numpy()


@functools.lru_cache(maxsize=None)
def up_ref(name):
    src, H2, W2, idx = up_case(name)
    return resize64_at(src, H2, W2, idx)


def up_check(name):
    src, H2, W2, idx = up_case(name)
    e32 = {"up": abs_err(resize32(src, H2, W2).reshape(-1)[idx], up_ref(name))}
    return _over_cap(e32), e32


UPFIELD = ((5, 7, 9), (12, 8, 10))      # grid -> target: three different sizes either way, one axis shrinks nowhere


def upfield_field(device="cpu"):
    return quiet(make_field, UPFIELD[0], device, seed=SEEDS["upfield"])


def upfield_ref(f):
    """f: the field before the resize (CPU) -> ({state-dict name: float64 tensor}, stepSize, nSamples) of
    tensoRF.py:198-233 and tensorBase.py:317-330 in float64."""
    tgt = UPFIELD[1]
    sd = {k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}
    out = {}
    for kind in ("density", "app"):
        for i in range(3):
            m0, m1 = onp.MAT_MODE[i]
            for key, (h2, w2) in ((f"{kind}_plane.{i}", (tgt[m1], tgt[m0])), (f"{kind}_line.{i}", (tgt[onp.VEC_MODE[i]], 1))):
                src = sd[key][0]
                out[key] = resize64_at(src, h2, w2, np.arange(src.shape[0] * h2 * w2)).reshape(1, src.shape[0], h2, w2)
    size = (sd["aabb"][1] - sd["aabb"][0]).astype(np.float64)
    step = float(np.mean(size / (np.asarray(tgt, np.float64) - 1)) * f.step_ratio)
    return out, step, np.sqrt((size ** 2).sum()) / step


def upfield_check():
    f = upfield_field()
    ref, step, ns = upfield_ref(f)
    bad = [] if abs(ns - round(ns)) > 1e-3 else ["nSamples sits on an integer"]
    e32 = {"up": max(abs_err(resize32(f.state_dict()[k].numpy()[0], *v.shape[2:]), v[0]) for k, v in ref.items())}
    return bad + _over_cap(e32), e32


# ------------------------------------------------------------------------------------------------------------------ pool
POOL_LATTICES = ((1, 1, 1), (1, 5, 1), (2, 2, 2), (5, 7, 9), (4, 8, 8), (3, 5, 17), (257, 1, 1), (20, 18, 22))     # (gx, gy, gz)
THRES = np.float32(1e-4)                # alphaMask_thres as the float the kernel is handed


def pool_values(alpha):
    """clamp(0, 1) then the 3x3x3 max with -inf padding (tensorBase.py:523-527) of alpha [gz,gy,gx], in alpha's dtype."""
    a = np.clip(alpha, 0, 1)
    gz, gy, gx = a.shape
    pad = np.full((gz + 2, gy + 2, gx + 2), -np.inf, a.dtype)
    pad[1:-1, 1:-1, 1:-1] = a
    m = np.full(a.shape, -np.inf, a.dtype)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                m = np.maximum(m, pad[dz:dz + gz, dy:dy + gy, dx:dx + gx])
    return m


def pool_ref(alpha, thres):
    return (pool_values(alpha) >= thres).astype(np.float32)


def block(lat, cell):
    """Ones on the 3x3x3 window around cell = (ix, iy, iz) clipped to the lattice (gx, gy, gz), as [gz,gy,gx]."""
    out = np.zeros(lat[::-1], np.float32)
    (x, y, z) = cell
    out[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 1
    return out


def pool_inputs(lat):
    """[(name, alpha [gz,gy,gx] float32, thres, expected or None)]: random alpha around the threshold, a single 1 at each
    corner (kept: exactly the clipped 2x2x2 block), -0.5 and 1.5 through the clamp, thres / the float below / the float above
    alone in a field of zeros, thres = 0."""
    gx, gy, gz = lat
    rng = _rng("pool-{}x{}x{}".format(*lat))
    shape = (gz, gy, gx)
    rand = (1e-4 * np.exp(2 * rng.standard_normal(shape) - 4)).astype(np.float32)
    out = [("random", rand, THRES, None), ("random-thres0", rand - np.float32(2e-5), np.float32(0), np.ones(shape, np.float32))]
    for k in range(8):
        cell = tuple((g - 1) * ((k >> a) & 1) for a, g in enumerate(lat))
        a = np.zeros(shape, np.float32)
        a[cell[2], cell[1], cell[0]] = 1
        out.append((f"corner-{k}", a, THRES, block(lat, cell)))
    mix = np.where(rng.random(shape) < 0.5, np.float32(-0.5), np.float32(1.5)).astype(np.float32)
    out.append(("clamp-hi", mix, np.float32(1.25), np.zeros(shape, np.float32)))          # 1.5 clamps to 1, under 1.25
    out.append(("clamp-lo", np.full(shape, -0.5, np.float32), np.float32(0), np.ones(shape, np.float32)))   # -0.5 clamps to 0, at 0
    cell = tuple(int(rng.integers(0, g)) for g in lat)
    for tag, v in (("at", THRES), ("below", np.nextafter(THRES, np.float32(0))), ("above", np.nextafter(THRES, np.float32(1)))):
        a = np.zeros(shape, np.float32)
        a[cell[2], cell[1], cell[0]] = v
        out.append((f"thres-{tag}", a, THRES, np.zeros(shape, np.float32) if tag == "below" else block(lat, cell)))
    return out


# ------------------------------------------------------------------------------------------------------------------ mask
GRID_A, GRID_B = (13, 9, 11), (20, 24, 28)
MASK_CASES = {                          # grid, scale of the density planes, offset, new lattice, previous mask's lattice, activation
    "A/7x5x6": (GRID_A, 60, -2.0, (7, 5, 6), None, "softplus"),                   # so coarse a lattice keeps nearly all without it
    "A/20x18x22": (GRID_A, 60, 0, (20, 18, 22), None, "softplus"),
    "A/33x31x17": (GRID_A, 60, 0, (33, 31, 17), None, "softplus"),
    "A/1x3x2": (GRID_A, 60, 0, (1, 3, 2), None, "softplus"),
    "B/20x18x22": (GRID_B, 60, 0, (20, 18, 22), None, "softplus"),
    "A/rebuild": (GRID_A, 60, 0, (33, 31, 17), (20, 18, 22), "softplus"),
    "B/rebuild": (GRID_B, 60, 0, (20, 18, 22), (10, 12, 14), "softplus"),
    "A/coincident": (GRID_A, 60, 0, (17, 13, 21), (9, 7, 11), "softplus"),
    "A/softplus20": (GRID_A, 1500, -40.0, (20, 18, 22), None, "softplus"),      # feature + shift from far below 0 to above 20
    "A/relu": (GRID_A, 60, -2.0, (20, 18, 22), None, "relu"),                   # relu(feature): mostly negative, so that cells drop
}
COINCIDENT = "A/coincident"
# offset: component 0 of plane 0 is set to 1 and of line 0 to the offset, which adds it to every feature
RENDER_CASE, RENDER_RAYS, RENDER_NS = "A/rebuild", 64, 96


def mask_field(name, device="cpu", seed=None):
    grid, scale, offset, _, _, act = MASK_CASES[name]
    f = quiet(make_field, grid, "cpu", seed=SEEDS[name] if seed is None else seed, density_shift=-10, fea2denseAct=act)
    with torch.no_grad():
        for p in f.density_plane:
            p.mul_(float(scale))
        if offset:
            f.density_plane[0][0, 0].fill_(1.0)
            f.density_line[0][0, 0].fill_(offset)
    return f.to(device) if str(device) != "cpu" else f


def field_dict(f, dt):
    fld = {k: v.detach().cpu().numpy().astype(dt) for k, v in f.state_dict().items() if v.dtype.is_floating_point}
    fld.update(density_shift=float(f.density_shift), fea2denseAct=f.fea2denseAct)
    return fld


def lattice_points(aabb, lat, dt):
    """tensorBase.py:504-509 in [gz,gy,gx] order: torch.linspace(0, 1, g) in float32 (what the kernel is handed), cast to
    dt, then aabb[0] * (1 - t) + aabb[1] * t -> [gz * gy * gx, 3]."""
    lin = [torch.linspace(0, 1, int(g)).numpy().astype(dt) for g in lat]
    Z, Y, X = np.meshgrid(lin[2], lin[1], lin[0], indexing="ij")
    t = np.stack([X, Y, Z], -1).reshape(-1, 3)
    one = np.asarray(1, dt)
    return (aabb[0] * (one - t) + aabb[1] * t).astype(dt)


def mask_validity(vol, maabb, x):
    """x [P,3] float64 under the mask vol [Z,Y,X] of box maabb -> (valid, decidably valid, decidably invalid)."""
    Z, Y, X = vol.shape
    p = onp.normalize_coord(x, maabb)
    valid = onp.trilerp_zeros(vol, p) > 0
    size = (X, Y, Z)
    ix = [((p[:, a] + 1.0) / 2.0) * (size[a] - 1) for a in range(3)]
    b0 = [np.floor(i).astype(np.int64) for i in ix]
    t = [i - b for i, b in zip(ix, b0)]
    sure = np.zeros(len(x))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi, zi = b0[0] + dx, b0[1] + dy, b0[2] + dz
                ok = (xi >= 0) & (xi < X) & (yi >= 0) & (yi < Y) & (zi >= 0) & (zi < Z)
                w = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                v = vol[np.clip(zi, 0, Z - 1), np.clip(yi, 0, Y - 1), np.clip(xi, 0, X - 1)]
                sure += np.where(ok & (w >= W_MIN), v * w, 0.0)
    lo = [np.floor(i - NEAR_PLANE).astype(np.int64) for i in ix]
    hi = [np.floor(i + NEAR_PLANE).astype(np.int64) + 1 for i in ix]
    any_one = np.zeros(len(x), bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                xi, yi, zi = lo[0] + dx, lo[1] + dy, lo[2] + dz
                ok = ((xi <= hi[0]) & (yi <= hi[1]) & (zi <= hi[2])
                      & (xi >= 0) & (xi < X) & (yi >= 0) & (yi < Y) & (zi >= 0) & (zi < Z))
                any_one |= ok & (vol[np.clip(zi, 0, Z - 1), np.clip(yi, 0, Y - 1), np.clip(xi, 0, X - 1)] > 0)
    return valid, sure > 0, ~any_one


def mask_eval(f, lat, dt, prev=None):
    """getDenseAlpha (tensorBase.py:501-516, 538-558) of the CPU field f on the lattice (gx, gy, gz) in dt, through the mask
    prev = (vol [Z,Y,X], aabb) if given -> dict(alpha [gz,gy,gx]; free: the same without the mask; valid; y = feature + shift;
    and in float64 sure_valid, sure_invalid)."""
    fld = field_dict(f, dt)
    x = lattice_points(fld["aabb"], lat, dt)
    step = np.asarray(float(f.stepSize), dt)
    feat = onp.density_feature(fld, onp.normalize_coord(x, fld["aabb"]))
    free = (np.asarray(1, dt) - np.exp(-onp.feature2density(fld, feat) * step)).astype(dt)
    shape = tuple(lat)[::-1]
    out = dict(free=free.reshape(shape), y=(feat + np.asarray(fld["density_shift"], dt)).reshape(shape))
    if prev is None:
        valid = np.ones(len(x), bool)
        sv, si = valid, ~valid
    else:
        vol, maabb = prev
        valid = onp.trilerp_zeros(vol.astype(dt), onp.normalize_coord(x, maabb.astype(dt))) > 0
        _, sv, si = mask_validity(vol.astype(np.float64), maabb.astype(np.float64), x.astype(np.float64))
    out.update(alpha=np.where(valid, free, np.asarray(0, dt)).reshape(shape), valid=valid.reshape(shape),
               sure_valid=sv.reshape(shape), sure_invalid=si.reshape(shape))
    return out


@functools.lru_cache(maxsize=None)
def mask_prev(name, seed=None):
    """The previous mask of a case: the float64 reference's own mask of the same field on the previous lattice, with the
    field's box -> (vol [Z,Y,X] float32 of 0 / 1, aabb [2,3] float32), or None."""
    prev = MASK_CASES[name][4]
    if prev is None:
        return None
    f = mask_field(name, seed=seed)
    vol = (pool_values(mask_eval(f, prev, np.float64)["alpha"]) >= np.float64(THRES)).astype(np.float32)
    return vol, f.aabb.detach().numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def mask_ref(name, seed=None):
    return mask_eval(mask_field(name, seed=seed), MASK_CASES[name][3], np.float64, mask_prev(name, seed))


def mask_sets(ref, tol):
    """ref: mask_eval in float64 -> (mask [gz,gy,gx] of 0 / 1, decidably kept, decidably dropped)."""
    lo = pool_values(np.where(ref["sure_valid"], ref["free"], 0.0))
    hi = pool_values(np.where(ref["sure_invalid"], 0.0, ref["free"]))
    th = np.float64(THRES)
    return (pool_values(ref["alpha"]) >= th).astype(np.float32), lo - th > tol, th - hi > tol


def alpha_err(alpha, ref):
    """max |alpha - alpha64| over the lattice points whose validity float64 decides; at the others alpha has to be within the
    same distance of 0 or of the unmasked value."""
    a = np.asarray(alpha, np.float64).reshape(ref["alpha"].shape)
    dec = ref["sure_valid"] | ref["sure_invalid"]
    e = np.where(dec, np.abs(a - ref["alpha"]), np.minimum(np.abs(a), np.abs(a - ref["free"])))
    return float(e.max())


def mask_check(name, seed=None):
    """-> (violations, e32, figures): the float32 oracle against float64; the undecidable share; decided cells on both sides;
    no decided cell flipped by float32."""
    f, lat = mask_field(name, seed=seed), MASK_CASES[name][3]
    ref = mask_ref(name, seed)
    r32 = mask_eval(f, lat, np.float32, mask_prev(name, seed))
    e32 = {"alpha": alpha_err(r32["alpha"], ref)}
    tol = tolerance(e32["alpha"], "alpha")
    m64, keep, drop = mask_sets(ref, tol)
    m32 = pool_ref(r32["alpha"], THRES)
    und = 1.0 - float((keep | drop).mean())
    fig = dict(kept=float(m64.mean()), undecidable=int((~(keep | drop)).sum()), cells=int(m64.size), flips32=int((m32 != m64).sum()),
               undecided_validity=int((~(ref["sure_valid"] | ref["sure_invalid"])).sum()))
    bad = []
    if ((m32 != m64) & (keep | drop)).any():
        bad.append("float32 flips a decidable cell")
    if (keep & (m64 == 0)).any() or (drop & (m64 == 1)).any():
        bad.append("a decidable set disagrees with float64")
    if name != COINCIDENT:
        if und > UNDECIDABLE_MASK:
            bad.append(f"undecidable share {und:.4f}")
        if keep.mean() < DECIDED_EACH_SIDE or drop.mean() < DECIDED_EACH_SIDE:
            bad.append(f"decided kept {keep.mean():.3f}, dropped {drop.mean():.3f}")
    if name == "A/softplus20" and not ((ref["y"] > 20).sum() >= 20 and (ref["y"] < 20).sum() >= 20):
        bad.append("softplus branch above 20 not reached on both sides")
    return bad, e32, fig


def render_rays():
    from util import make_rays
    return make_rays(RENDER_RAYS, SEEDS["render"]).numpy()


def render_ref(f, vol, dt=np.float64):
    """64 rays through the field of RENDER_CASE with the mask vol [Z,Y,X] -> (rgb, depth, extras) of oracle.render_field."""
    fld = field_dict(f, dt)
    fld["alphaMask.alpha_volume"] = vol.astype(dt)[None, None]
    fld["alphaMask.aabb"] = fld["aabb"]
    for k, v in dict(distance_scale=f.distance_scale, rayMarch_weight_thres=f.rayMarch_weight_thres).items():
        fld[k] = float(v)
    return onp.render_field(fld, render_rays().astype(dt), onp.z_schedule(RENDER_NS, dt), True, 0.0, return_extras=True)


# ------------------------------------------------------------------------------------------------------------------ features
FEAT_GRIDS = ((5, 7, 9), (20, 24, 28), (1, 1, 1))       # (1,1,1): make_layout has no lower bound, a one-texel grid is the smallest
FEAT_P = (1, 127, 128, 129, 255, 256, 257)              # either side of the 128-thread (app) and 256-thread (density) blocks
FEAT_CASES = ["{}x{}x{}/P{}".format(*g, p) for g in FEAT_GRIDS for p in FEAT_P]
FEAT_SCALE = 3.0                        # planes x 3, as smoke() scales them: 4 e32 of the 28-texel grid stays under the 2e-6 cap


def feat_field(grid, device="cpu"):
    f = quiet(make_field, grid, "cpu", seed=SEEDS["feat"])
    with torch.no_grad():
        for p in list(f.density_plane) + list(f.app_plane):
            p.mul_(FEAT_SCALE)
    return f.to(device) if str(device) != "cpu" else f


@functools.lru_cache(maxsize=None)
def feat_coords(grid):
    """[257,3] float32 normalised coordinates: the 27 combinations of {-1, 0, +1}; +-1.5 and nextafter(+-1, 0) on each axis
    with the other two random; every texel centre along each axis with the other two random; uniform in [-1, 1]."""
    rng = _rng("feat-{}x{}x{}".format(*grid))
    u = [np.array([a, b, c], np.float32) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    one = np.float32(1)
    for a in range(3):
        for v in (np.float32(-1.5), np.float32(1.5), np.nextafter(-one, np.float32(0)), np.nextafter(one, np.float32(0))):
            p = rng.uniform(-1, 1, 3).astype(np.float32)
            p[a] = v
            u.append(p)
        for i in range(grid[a]):
            p = rng.uniform(-1, 1, 3).astype(np.float32)
            p[a] = np.float32(-1.0 + 2.0 * i / max(grid[a] - 1, 1))
            u.append(p)
    u = np.stack(u)
    assert len(u) <= 257
    return np.concatenate([u, rng.uniform(-1, 1, (257 - len(u), 3)).astype(np.float32)])


def feat_case(name):
    g, p = name.split("/P")
    grid = tuple(int(v) for v in g.split("x"))
    return grid, feat_coords(grid)[:int(p)]


def feat_run(f, u, dt):
    fld = field_dict(f, dt)
    return {"sig": onp.density_feature(fld, u.astype(dt)).astype(np.float64), "app": onp.app_feature(fld, u.astype(dt))[0].astype(np.float64)}


@functools.lru_cache(maxsize=None)
def feat_ref(name):
    grid, u = feat_case(name)
    return feat_run(feat_field(grid), u, np.float64)


def feat_check(name):
    grid, u = feat_case(name)
    r32 = feat_run(feat_field(grid), u, np.float32)
    e32 = {q: abs_err(r32[q], feat_ref(name)[q]) for q in ("sig", "app")}
    return _over_cap(e32), e32


# ------------------------------------------------------------------------------------------------------------------ sample_ray
RAY_SHAPES = ((1, 1), (5, 51), (4, 64), (3, 85), (257, 1), (64, 50))      # R x N: 255, 256, 255, 257 either side of one block
RAY_CASES = [f"{r}x{n}/{m}" for r, n in RAY_SHAPES for m in ("eval", "jit")]
CON_CASES = [f"{r}x{n}" for r, n in RAY_SHAPES]
RAY_GRID = (32, 32, 32)
AABB = np.array([[-2.0, -2, -2], [2, 2, 2]], np.float32)
NEAR_FAR = (0.1, 1e3)
STEP = float((torch.tensor([4.0, 4.0, 4.0]) / (torch.tensor(RAY_GRID) - 1)).mean() * 0.5)     # update_stepSize at step_ratio 0.5
KINDS = ("zero0", "inside", "far0", "zero1", "miss", "zero2", "zero01", "negative", "outside_hit", "far1", "tiny", "graze")


def _one_ray(kind, rng, hit_ok):
    o = rng.uniform(-1.5, 1.5, 3)
    d = rng.standard_normal(3)
    d /= np.linalg.norm(d)
    d = np.where(np.abs(d) < 0.05, 0.05, d)
    if kind.startswith("zero"):                             # a zero component on one axis, on two axes: the 1e-6 substitution
        for a in kind[4:]:
            d[int(a)] = 0.0
    elif kind.startswith("far"):                            # zero component and an origin below the slab: t_min = 1e6, the far clamp
        a = int(kind[3])
        d[a], o[a] = 0.0, -3.0
    elif kind == "graze":                                   # zero component, origin 5e-4 below the slab: 5e-4 / 1e-6 = 500, under the
        d[0], o[0] = 0.0, -2.0005                           # far clamp -- the one place the VALUE of the substitute shows (1 / 0 clamps too)
    elif kind == "tiny":                                    # 1 / 1e-4 = 1e4: the far clamp without the substitution
        d[2], o[2] = 1e-4, -3.0
    elif kind == "miss":                                    # enters the y slab on its face plane at x = 4: outside, decidably
        o = np.array([3.0, 3.0, 0.0]) + 0.1 * rng.standard_normal(3)
        d = np.array([1.0, -1.0, 0.2]) + 0.05 * rng.standard_normal(3)
    elif kind == "negative":
        d = -np.abs(d)
    elif kind == "outside_hit" and hit_ok:                  # the first sample of an eval ray lies ON the entry face: undecidable
        o = np.array([-3.5, 0.4, -0.3]) + 0.2 * rng.standard_normal(3)
        d = np.array([1.0, 0.0, 0.0]) + 0.1 * rng.standard_normal(3)
    return np.concatenate([o, d])


@functools.lru_cache(maxsize=None)
def ray_case(name, seed=None):
    """-> (rays [R,6] float32, N, jitter [R] float32 or None).  Rays that enter the box from outside put their first eval
    sample on a face, so they are drawn only with jitter or where 0.2 % of the flags leaves room for them (64 x 50)."""
    shape, mode = name.split("/")
    R, N = (int(v) for v in shape.split("x"))
    rng = _rng("ray-" + name, SEEDS[name] if seed is None else seed)
    if R == 1:      # inside at t = near, outside one jittered step further; zero components on two axes
        rays = np.array([[1.85, 0.3, -0.2, 1.0, 0.0, 0.0]])
        jit = np.array([0.9])
    else:
        hit_ok = mode == "jit" or R * N >= 3200
        rays = np.stack([_one_ray(KINDS[r % len(KINDS)], rng, hit_ok) for r in range(R)])
        jit = rng.uniform(0.05, 1.0, R)
    return rays.astype(np.float32), N, (jit.astype(np.float32) if mode == "jit" else None)


def ray_run(name, dt, seed=None):
    rays, N, jit = ray_case(name, seed)
    r = rays.astype(dt)
    pts, t, inside = onp.sample_ray_aabb(r[:, :3], r[:, 3:], AABB.astype(dt), STEP, N, NEAR_FAR, None if jit is None else jit.astype(dt))
    return {"pts": pts.astype(np.float64), "t": t.astype(np.float64), "inside": inside}


@functools.lru_cache(maxsize=None)
def ray_ref(name):
    return ray_run(name, np.float64)


def flag_sets(pts, tol):
    """-> (decidably inside, decidably outside) of float64 points against AABB, distances on the scale of the pts measure."""
    m = tol * np.maximum(np.abs(pts), 1.0)
    lo, hi = AABB[0].astype(np.float64), AABB[1].astype(np.float64)
    return ((pts - lo > m) & (hi - pts > m)).all(-1), ((lo - pts > m) | (pts - hi > m)).any(-1)


def ray_check(name, seed=None):
    ref = ray_ref(name) if seed is None else ray_run(name, np.float64, seed)
    r32 = ray_run(name, np.float32, seed)
    e32 = {q: rel1_err(r32[q], ref[q]) for q in ("t", "pts")}
    ins, out = flag_sets(ref["pts"], tolerance(e32["pts"], "pts"))
    bad = []
    if 1.0 - (ins | out).mean() > UNDECIDABLE_FLAGS:
        bad.append(f"{int((~(ins | out)).sum())} of {ins.size} flags undecidable")
    if (r32["inside"] != ref["inside"])[ins | out].any() or (ins & ~ref["inside"]).any() or (out & ref["inside"]).any():
        bad.append("float32 flips a decidable flag")
    return bad + _over_cap(e32), e32, dict(undecidable=int((~(ins | out)).sum()), flags=int(ins.size), inside=int(ins.sum()), outside=int(out.sum()))


@functools.lru_cache(maxsize=None)
def con_case(name):
    """-> (o [R,3], d [R,3] unit, z [S]) float32.  The first rays have d = 0 and an origin whose infinity norm is exactly 1, the
    float above 1, below 1e-6; z is drawn from the 128-sample eval schedule and ends at z = 1000.1."""
    R, S = (int(v) for v in name.split("x"))
    rng = _rng("con-" + name)
    o = (0.5 * rng.standard_normal((R, 3))).astype(np.float32)
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    one = np.float32(1)
    special = np.array([[np.nextafter(one, np.float32(2)), 0.3, -0.2], [-0.4, 1.0, 0.9], [5e-7, -3e-7, 1e-7]], np.float32)
    k = 3 if R >= 4 else 1
    o[:k], d[:k] = special[:k], 0
    zs = onp.z_schedule(384)
    z = zs[np.round(np.linspace(0, len(zs) - 1, S)).astype(int)].astype(np.float32)
    z[-1] = np.float32(1000.1)                              # far + 0.1: where the jittered schedule ends (tensorBase.py:431-436)
    return o, d, z


def con_run(name, dt):
    o, d, z = con_case(name)
    return {"xc": onp.sample_ray_contracted(o.astype(dt), d.astype(dt), z.astype(dt)).astype(np.float64)}


@functools.lru_cache(maxsize=None)
def con_ref(name):
    return con_run(name, np.float64)


def con_check(name):
    e32 = {"xc": abs_err(con_run(name, np.float32)["xc"], con_ref(name)["xc"])}
    return _over_cap(e32), e32


def _over_cap(e32):
    return [f"{q}: 4 e32 = {4 * e:.3e} over the cap {CAP[q]:.0e}" for q, e in e32.items() if CAP[q] is not None and not 4 * e <= CAP[q]]


# ------------------------------------------------------------------------------------------------------------------ seeds, E32
CHECKS = {"up": (UP_CASES, up_check), "upfield": (["5x7x9-12x8x10"], lambda name: upfield_check()),
          "mask": (list(MASK_CASES), lambda name: mask_check(name)[:2]), "feat": (FEAT_CASES, feat_check),
          "ray": (RAY_CASES, lambda name: ray_check(name)[:2]), "con": (CON_CASES, con_check)}

# Seeds: the first from 1 upwards with which the case meets its conditions on the CPU (mask_check, ray_check).  A changed seed
# has to pass tests/test_upkeep_host.py.
SEEDS = {"upfield": 3, "feat": 11, "render": 1}
SEEDS.update({name: 1 for name in MASK_CASES})
SEEDS.update({"A/1x3x2": 2, "A/softplus20": 2})
SEEDS.update({name: 1 for name in RAY_CASES})

# E32["<family>:<case>"][quantity]: the float32 CPU evaluation's error against float64 (absolute; t and pts: |x - x64| / max(|x64|,
# 1)).  tests/test_upkeep_host.py recomputes it.
E32 = {
    "up:8x5x7-9x6": {"up": 5.81e-08},
    "up:24x20x28-27x31": {"up": 1.40e-07},
    "up:8x27x30-16x12": {"up": 1.63e-07},
    "up:8x2x2-257x3": {"up": 1.49e-08},
    "up:8x1x6-5x6": {"up": 0.00e+00},
    "up:8x6x5-1x1": {"up": 0.00e+00},
    "up:8x16x1-101x1": {"up": 2.35e-07},
    "up:24x64x1-101x1": {"up": 1.58e-07},
    "up:3x4x6-5x17": {"up": 1.14e-08},
    "up:4x5x3-8x8": {"up": 9.34e-08},
    "up:1x9x1-257x1": {"up": 9.78e-09},
    "up:24x13x11-13x11": {"up": 0.00e+00},
    "up:24x8x8-1676x1676": {"up": 1.79e-07},
    "upfield:5x7x9-12x8x10": {"up": 1.09e-07},
    "mask:A/7x5x6": {"alpha": 7.66e-08},
    "mask:A/20x18x22": {"alpha": 1.95e-07},
    "mask:A/33x31x17": {"alpha": 1.03e-07},
    "mask:A/1x3x2": {"alpha": 6.73e-08},
    "mask:B/20x18x22": {"alpha": 2.62e-07},
    "mask:A/rebuild": {"alpha": 1.03e-07},
    "mask:B/rebuild": {"alpha": 2.62e-07},
    "mask:A/coincident": {"alpha": 9.68e-08},
    "mask:A/softplus20": {"alpha": 1.41e-05},
    "mask:A/relu": {"alpha": 1.30e-06},
    "feat:5x7x9/P1": {"sig": 2.91e-09, "app": 3.74e-09},
    "feat:5x7x9/P127": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:5x7x9/P128": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:5x7x9/P129": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:5x7x9/P255": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:5x7x9/P256": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:5x7x9/P257": {"sig": 2.67e-07, "app": 2.15e-08},
    "feat:20x24x28/P1": {"sig": 1.17e-08, "app": 4.56e-09},
    "feat:20x24x28/P127": {"sig": 3.48e-07, "app": 9.94e-08},
    "feat:20x24x28/P128": {"sig": 3.48e-07, "app": 9.94e-08},
    "feat:20x24x28/P129": {"sig": 3.48e-07, "app": 9.94e-08},
    "feat:20x24x28/P255": {"sig": 3.97e-07, "app": 1.32e-07},
    "feat:20x24x28/P256": {"sig": 3.97e-07, "app": 1.32e-07},
    "feat:20x24x28/P257": {"sig": 3.97e-07, "app": 1.32e-07},
    "feat:1x1x1/P1": {"sig": 5.96e-09, "app": 4.15e-09},
    "feat:1x1x1/P127": {"sig": 5.96e-09, "app": 7.43e-09},
    "feat:1x1x1/P128": {"sig": 5.96e-09, "app": 7.43e-09},
    "feat:1x1x1/P129": {"sig": 5.96e-09, "app": 7.43e-09},
    "feat:1x1x1/P255": {"sig": 5.96e-09, "app": 7.43e-09},
    "feat:1x1x1/P256": {"sig": 5.96e-09, "app": 7.43e-09},
    "feat:1x1x1/P257": {"sig": 5.96e-09, "app": 7.43e-09},
    "ray:1x1/eval": {"t": 1.49e-09, "pts": 1.22e-08},
    "ray:1x1/jit": {"t": 1.54e-09, "pts": 1.41e-08},
    "ray:5x51/eval": {"t": 9.36e-08, "pts": 4.48e-07},
    "ray:5x51/jit": {"t": 1.25e-07, "pts": 3.35e-07},
    "ray:4x64/eval": {"t": 9.36e-08, "pts": 1.68e-07},
    "ray:4x64/jit": {"t": 7.70e-08, "pts": 1.13e-07},
    "ray:3x85/eval": {"t": 9.36e-08, "pts": 2.27e-07},
    "ray:3x85/jit": {"t": 1.10e-07, "pts": 2.09e-07},
    "ray:257x1/eval": {"t": 5.26e-08, "pts": 9.12e-08},
    "ray:257x1/jit": {"t": 1.01e-07, "pts": 1.24e-07},
    "ray:64x50/eval": {"t": 1.03e-07, "pts": 4.95e-07},
    "ray:64x50/jit": {"t": 1.27e-07, "pts": 4.44e-07},
    "con:1x1": {"xc": 1.42e-14},
    "con:5x51": {"xc": 1.82e-07},
    "con:4x64": {"xc": 1.68e-07},
    "con:3x85": {"xc": 1.91e-07},
    "con:257x1": {"xc": 3.38e-07},
    "con:64x50": {"xc": 2.65e-07},
}
