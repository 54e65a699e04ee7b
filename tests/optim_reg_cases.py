"""Shared pieces of the optimiser / regulariser tests: plain float64 references of the fused Adam step (csrc/lrf_adam.inl),
the density-L1 regulariser and the TV regulariser (csrc/lrf_reg.inl), the constructed inputs, and the case tables.

  adam_step_ref(p, g, m, v, step_size, bc2_sqrt, b1, b2, eps)   one step in float64 + element-wise float32 error bounds
  adam_scalars(lr, b1, b2, step)                                (step_size, bc2_sqrt) as FusedAdam forms them on the host
  density_l1_ref(planes, lines, shift, relu)                    value, six gradients, their absolute-term sums (float64)
  density_l1_expression(planes, lines, feature2density)         the reference method's arithmetic on torch tensors
  density_l1_torch(planes, lines, shift, relu, dtype)           that expression through autograd, in `dtype`
  l1_inputs(grid, relu, seed) / l1_bands(...)                   the banded lattice features and the condition they meet
  tv_ref(tensors, weight)                                       value, gradients, absolute-term sums (float64)
  TVLoss / tv_expression(planes, lines, reg)                    the reference module and how a field applies it
  tv_torch(tensors, weight, dtype)                              the module through autograd, in `dtype`
  normalised_error(got, ref, abs_sum)                           max_i |got_i - ref_i| / abs_sum_i

Cited lines are relative to the reference's localTensoRF directory (models/tensoRF.py, utils/utils.py)."""
import math

import numpy as np
import torch

U = 2.0 ** -24                    # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -149                # absolute error of an operation whose result is subnormal
F32 = np.float32


def gam(k):
    """(1 + u)^k - 1 <= k u / (1 - k u): the relative error of k correctly rounded operations in a row."""
    return k * U / (1.0 - k * U)


def f32(x):
    """The float32 nearest to x, as a float64 (what a `float` argument of the ABI holds)."""
    return float(F32(x))


# --------------------------------------------------------------------------------------------------------------- Adam
def adam_scalars(lr, b1, b2, step):
    """(step_size, bc2_sqrt) of a parameter at its `step`-th step, in double as FusedAdam._entries / torch.optim.Adam form them."""
    return lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def adam_step_ref(p, g, m, v, step_size, bc2_sqrt, b1, b2, eps, round_scalars=True):
    """The three update lines at the head of csrc/lrf_adam.inl in float64 on the given (float32-valued) arrays:

        m' = m + (g - m)(1 - b1);   v' = v b2 + (1 - b2) g g;   p' = p - step_size * m' / (sqrt(v') / bc2_sqrt + eps)

    with step_size, bc2_sqrt, b1, b2 and eps first rounded to float32 (the ABI passes them as `float`; round_scalars=False
    keeps the doubles: that is torch.optim.Adam in float64).  Returns (p', m', v', E_p, E_m, E_v): E_* bound, element by
    element, |kernel - reference| for a kernel that evaluates adam1() with correctly rounded float32 operations
    (sub, fma, mul, mul, fma, sqrt, div, add, div, fma), each of which returns x (1 + d), |d| <= u = 2^-24.  With
    gam(k) = k u / (1 - k u) >= (1 + u)^k - 1:

      m:  fl(g - m) and fl(1 - b1) carry one rounding each, the fma one more on the sum
            E_m = gam(2) |g - m| (1 - b1) (1 + u) + u |m'|
      v:  fl(1 - b2), the two multiplications by g, then the fma
            E_v = gam(3) (1 - b2) g^2 (1 + u) + u |v'|
      s = sqrt(v'):  |sqrt(v^) - sqrt(v')| <= min(E_v / sqrt(v'), sqrt(E_v)) =: e0 (0 where v' = 0: then E_v = 0), one rounding
            E_s = e0 + u (s + e0)
      q = s / bc2_sqrt:       E_q = (E_s + u (s + E_s)) / bc2_sqrt
      d = q + eps:            E_d = E_q + u (d + E_q)
      r = m' / d:  m^/d^ - m'/d = ((m^ - m') + r (d - d^)) / d^
            e1 = (E_m + |r| E_d) / (d - E_d),   E_r = e1 + u (|r| + e1)
      p:  one fma            E_p = step_size E_r + u (|p'| + step_size E_r)

    plus 2^-149 on each for a subnormal result.  Nothing is normalised by a tensor maximum."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if round_scalars:
        step_size, bc2_sqrt, b1, b2, eps = (f32(x) for x in (step_size, bc2_sqrt, b1, b2, eps))
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = m + (g - m) * c1
    v1 = v * b2 + c2 * g * g
    s = np.sqrt(v1)
    d = s / bc2_sqrt + eps
    r = m1 / d
    p1 = p - step_size * r
    E_m = gam(2) * np.abs(g - m) * c1 * (1 + U) + U * np.abs(m1) + TINY
    E_v = gam(3) * c2 * g * g * (1 + U) + U * np.abs(v1) + TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        e0 = np.where(v1 > 0, np.minimum(E_v / np.where(v1 > 0, s, 1.0), np.sqrt(E_v)), np.sqrt(E_v))
    E_s = e0 + U * (s + e0)
    E_q = (E_s + U * (s + E_s)) / bc2_sqrt
    E_d = E_q + U * (d + E_q)
    assert (d > 2 * E_d).all(), "the bound needs a denominator that its own error cannot reach"
    e1 = (E_m + np.abs(r) * E_d) / (d - E_d)
    E_r = e1 + U * (np.abs(r) + e1)
    E_p = step_size * E_r + U * (np.abs(p1) + step_size * E_r) + TINY
    return p1, m1, v1, E_p, E_m, E_v


ADAM_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193, 3 * 4096 + 2)      # below / at / above one vector, one block, three blocks
ADAM_BETAS = (0.9, 0.99)
ADAM_EPS = 1e-8


def adam_arrays(n, seed, zero_grad=False):
    """float32 (p, g, m, v) of one tensor: gradients over 1e-6 .. 1e3 in magnitude, random state with v >= 0.  zero_grad:
    g = 0 and v = 0 everywhere, so that the denominator is eps alone (m is tiny: the step stays finite)."""
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(F32)
    if zero_grad:
        return p, np.zeros(n, F32), (1e-9 * r.standard_normal(n)).astype(F32), np.zeros(n, F32)
    g = (np.sign(r.standard_normal(n)) * 10.0 ** r.uniform(-6, 3, n)).astype(F32)
    m = (r.standard_normal(n) * 10.0 ** r.uniform(-6, 3, n)).astype(F32)
    v = (r.standard_normal(n) ** 2 * 10.0 ** r.uniform(-12, 6, n)).astype(F32)
    return p, g, m, v


# --------------------------------------------------------------------------------------------------------- density L1
MAT_MODE = ((0, 1), (0, 2), (1, 2))
VEC_MODE = (2, 1, 0)
L1_C = 8
L1_SHIFT = -5.0
L1_SMALL_GRIDS = ((300, 20, 12), (33, 17, 9), (5, 3, 2))
L1_LARGE_GRID_256CU = (112, 104, 96)      # n = 1 118 208 = 1.066 x 4096 x 256


def l1_large_grid(cus):
    """A (112, 104, g2) grid whose lattice has about 1.07 x 4096 x cus points: k_l1_fwd's grid-stride loop takes a second
    iteration for some threads, and every plane has more than 4096 texels."""
    return (112, 104, int(1.07 * 4096 * cus / (112 * 104)))


def l1_shapes(grid):
    """The six tensor shapes of a field of this grid (tensoRF.py:27-41): planes [1,8,g[m1],g[m0]], lines [1,8,g[v],1]."""
    planes = [(1, L1_C, grid[MAT_MODE[i][1]], grid[MAT_MODE[i][0]]) for i in range(3)]
    lines = [(1, L1_C, grid[VEC_MODE[i]], 1) for i in range(3)]
    return planes, lines


def l1_inputs(grid, relu, seed):
    """Six float32 density tensors whose lattice features keep away from the clamp at 1e-5 (relu: from zero), so that the
    float32 gradient does not hinge on the summation order of a single feature.  Component 0 of plane 0 times line 0 is
    dominant: each texel of plane 0 belongs to one of three bands (clamped / active / above the softplus threshold 20), its
    line lies in [0.9, 1.1]; the other 23 components add noise of amplitude <= 23 x 0.2 x 0.2 < 1."""
    r = np.random.default_rng(seed)
    ps, ls = l1_shapes(grid)
    planes = [r.uniform(-0.2, 0.2, s) for s in ps]
    lines = [r.uniform(-0.2, 0.2, s) for s in ls]
    hw0 = ps[0][2] * ps[0][3]
    band = r.permutation(np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 2])[np.arange(hw0) % 10])
    lo, hi = np.array([-25.0, 7.5, 30.0])[band], np.array([-11.0, 20.0, 40.0])[band]
    # feat = a b + noise: <= -8.9 | in [5.75, 23] | >= 26; with the shift of -5: <= -13.9 | [0.75, 18] | >= 21
    planes[0][0, 0] = r.uniform(lo, hi).reshape(ps[0][2:])
    lines[0][0, 0] = r.uniform(0.9, 1.1, ls[0][2:])
    return [a.astype(F32) for a in planes], [a.astype(F32) for a in lines]


def l1_features(planes, lines):
    """feat [n] float64 in the reference's index arithmetic: every plane flattens the lattice plane-major with its own line
    fastest, and the three are added element by element in those three different orders (tensoRF.py:84-89)."""
    feat = 0.0
    for pl, ln in zip(planes, lines):
        P = np.asarray(pl, np.float64).reshape(L1_C, -1)
        L = np.asarray(ln, np.float64).reshape(L1_C, -1)
        feat = feat + np.einsum("cq,cr->qr", P, L).reshape(-1)
    return feat


def _sigma(feat, shift, relu):
    if relu:
        return np.maximum(feat, 0.0), (feat > 0).astype(np.float64)
    x = feat + shift
    xs = np.minimum(x, 20.0)
    return np.where(x > 20.0, x, np.log1p(np.exp(xs))), np.where(x > 20.0, 1.0, 1.0 / (1.0 + np.exp(-xs)))


def l1_bands(planes, lines, shift, relu):
    """(fractions of the lattice in the clamped / active / high band, number of points in the forbidden zone): the zone is
    sig in [0.5e-5, 2e-5] (relu: |feat| < 1e-3); high is feat + shift > 20."""
    feat = l1_features(planes, lines)
    sig, _ = _sigma(feat, shift, relu)
    bad = (np.abs(feat) < 1e-3) if relu else ((sig >= 0.5e-5) & (sig <= 2e-5))
    high = feat + shift > 20.0
    low = sig < 1e-5
    mid = ~low & ~high
    return (low.mean(), mid.mean(), high.mean()), int(bad.sum())


def density_l1_ref(planes, lines, shift, relu):
    """TensorVMSplit.density_L1 (tensoRF.py:83-92) in float64 numpy: mean_i sqrt(clamp(feature2density(feat_i), 1e-5)), softplus
    with threshold 20 (F.softplus) or relu, clamp(min) passing the gradient where sig >= 1e-5.
    Returns (value, grads, abs_sums): grads = the six gradients (3 planes, 3 lines, shaped as the inputs), abs_sums = for
    every gradient element the sum of the absolute values of the terms it is made of (sum |dfeat_i x other factor|)."""
    feat = l1_features(planes, lines)
    n = feat.size
    sig, dsig = _sigma(feat, shift, relu)
    y = np.sqrt(np.maximum(sig, 1e-5))
    dfeat = np.where(sig >= 1e-5, 0.5 / y * dsig, 0.0) / n
    gp, gl, ap, al = [], [], [], []
    for pl, ln in zip(planes, lines):
        P = np.asarray(pl, np.float64).reshape(L1_C, -1)
        L = np.asarray(ln, np.float64).reshape(L1_C, -1)
        D = dfeat.reshape(P.shape[1], L.shape[1])
        gp.append((L @ D.T).reshape(np.shape(pl)))
        ap.append((np.abs(L) @ np.abs(D).T).reshape(np.shape(pl)))
        gl.append((P @ D).reshape(np.shape(ln)))
        al.append((np.abs(P) @ np.abs(D)).reshape(np.shape(ln)))
    return float(y.mean()), gp + gl, ap + al


def density_l1_expression(planes, lines, feature2density):
    """The arithmetic of the reference's TensorVMSplit.density_L1 (tensoRF.py:83-92), verbatim, on three torch planes
    [1,C,H,W] and their three lines [1,C,L,1]: the materialised outer products, summed in the three planes' own orders."""
    n = int(planes[0].shape[2] * planes[0].shape[3] * lines[0].shape[2])
    feat = planes[0].new_zeros((n,))
    for pl, ln in zip(planes, lines):
        pl = pl.view(-1, int(pl.shape[2] * pl.shape[3]))
        ln = ln.view(-1, int(ln.shape[2]))
        feat = feat + torch.sum(torch.bmm(pl[..., None], ln[:, None]).view(-1, n), dim=0)
    return torch.sqrt(feature2density(feat).clamp(1e-5)).mean()


def density_l1_torch(planes, lines, shift, relu, dtype, g_up=1.0):
    """density_l1_expression through autograd on the CPU, in `dtype`, differentiated with the upstream gradient g_up.
    -> (value, six gradients) as float64 numpy."""
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True) for a in list(planes) + list(lines)]
    act = torch.relu if relu else (lambda feat: torch.nn.functional.softplus(feat + shift))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' grouping, and with it a measured float32 error, must not depend
    try:                                          # on how many cores the machine has
        out = density_l1_expression(ts[:3], ts[3:], act)
        (out * g_up).backward()
    finally:
        torch.set_num_threads(threads)
    return float(out.detach().double()), [t.grad.double().numpy() for t in ts]


def normalised_error(got, ref, abs_sum):
    """max_i |got_i - ref_i| / abs_sum_i over the elements with abs_sum_i > 0; where abs_sum_i == 0 every term of the element
    is zero and got_i must be exactly zero (inf otherwise)."""
    got, ref, abs_sum = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, abs_sum))
    err = np.abs(got - ref)
    nz = abs_sum > 0
    if (err[~nz] != 0).any():
        return math.inf
    return float((err[nz] / abs_sum[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ TV
TV_WEIGHT = 0.7
TV_MAX = 16
TV_TABLES = {
    "single": [(1, 1, 1, 1)],
    # an H = 1 and a W = 1 tensor, one of exactly three 4096-element blocks, blocks that end mid-row and mid-channel
    # (24 x 37 x 41 = 8.9 blocks, rows of 41), differences across a block boundary along W (4097 x 1 row) and along H
    "blocks": [(1, 8, 1, 7), (1, 8, 9, 1), (1, 3, 64, 64), (1, 24, 37, 41), (1, 1, 1, 4097), (1, 1, 4097, 1)],
    "sixteen": [(1, 1 + k % 3, 2 + k, 19 - k) for k in range(TV_MAX)],
}


def tv_inputs(shapes, seed):
    r = np.random.default_rng(seed)
    return [r.standard_normal(s).astype(F32) for s in shapes]


def tv_scales(count):
    """1e-2 for the first three tensors (the planes), 1e-3 for the rest: _TVLossFn._table, for a table of any length."""
    return [1e-2 if i < 3 else 1e-3 for i in range(count)]


def tv_ref(tensors, weight):
    """TVLoss (utils/utils.py:293-309) applied tensor by tensor as tensoRF.py:94-110 in float64 numpy, x [1,C,H,W]:
        tv(x) = 2 w (mean (x[y+1] - x[y])^2 [H > 1] + mean (x[,x+1] - x[,x])^2 [W > 1]),  loss = sum_k scale_k tv(x_k)
    weight and the scales are first rounded to float32 (the ABI passes them as `float`).
    Returns (value, grads, abs_sums): abs_sums = per element the sum |coefficient x difference| over the (up to four)
    differences that its gradient is made of."""
    w = f32(weight)
    value, grads, sums = 0.0, [], []
    for x, sc in zip(tensors, tv_scales(len(tensors))):
        x = np.asarray(x, np.float64)
        _, C, H, W = x.shape
        s = f32(sc) * w * 2.0
        g, a = np.zeros_like(x), np.zeros_like(x)
        if H > 1:
            d = x[:, :, 1:, :] - x[:, :, :-1, :]
            ch = 2.0 / (C * (H - 1) * W)
            value += s * (d ** 2).mean()
            g[:, :, 1:, :] += s * ch * d
            g[:, :, :-1, :] -= s * ch * d
            a[:, :, 1:, :] += s * ch * np.abs(d)
            a[:, :, :-1, :] += s * ch * np.abs(d)
        if W > 1:
            d = x[:, :, :, 1:] - x[:, :, :, :-1]
            cw = 2.0 / (C * H * (W - 1))
            value += s * (d ** 2).mean()
            g[:, :, :, 1:] += s * cw * d
            g[:, :, :, :-1] -= s * cw * d
            a[:, :, :, 1:] += s * cw * np.abs(d)
            a[:, :, :, :-1] += s * cw * np.abs(d)
        grads.append(g)
        sums.append(a)
    return float(value), grads, sums


class TVLoss(torch.nn.Module):
    """The reference module (utils/utils.py:293-309), verbatim arithmetic."""

    def __init__(self, TVLoss_weight=1):
        super().__init__()
        self.TVLoss_weight = TVLoss_weight

    def forward(self, x):
        h_x, w_x = x.size()[2], x.size()[3]
        tv = 0
        if h_x > 1:
            tv += torch.pow((x[:, :, 1:, :] - x[:, :, :h_x - 1, :]), 2).mean()
        if w_x > 1:
            tv += torch.pow((x[:, :, :, 1:] - x[:, :, :, :w_x - 1]), 2).mean()
        return self.TVLoss_weight * 2 * tv


def tv_expression(planes, lines, reg):
    """TV_loss_density / TV_loss_app of the reference (tensoRF.py:94-110) on a field's planes and lines."""
    total = 0
    for i in range(3):
        total = total + reg(planes[i].transpose(0, 1)) * 1e-2 + reg(lines[i].transpose(0, 1)) * 1e-3
    return total


def tv_torch(tensors, weight, dtype, g_up=1.0, want_grads=True):
    """TVLoss applied tensor by tensor on the CPU, in `dtype`, with tv_ref's scales for a table of any length (weight and
    scales rounded to float32 as there), differentiated with the upstream gradient g_up unless want_grads is False.
    -> (value, gradients or None) as float64 numpy."""
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(want_grads) for a in tensors]
    reg = TVLoss(f32(weight))
    total = torch.zeros((), dtype=dtype)
    for x, sc in zip(ts, tv_scales(len(ts))):
        total = total + reg(x) * f32(sc)
    if not want_grads:
        return float(total.double()), None
    if total.requires_grad:                       # (a table of single elements has no difference to differentiate)
        (total * g_up).backward()
    return float(total.detach().double()), [np.zeros(t.shape) if t.grad is None else t.grad.double().numpy() for t in ts]
