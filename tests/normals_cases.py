"""Shared pieces of the normals tests: the oracle.  The density function g(x) = density_feature(u(contract(x))) is the
CPU oracle's own (oracle.vm_render_torch.density_feature: F.grid_sample, bilinear, align_corners, border), differentiated
with torch.autograd.grad in fp64 -- an independent restatement of what csrc/lrf_normals.inl derives by hand -- and the same
chain in fp32, whose distance from fp64 is the yardstick of the tolerance.  Samples on a kink of g (a cell boundary, a tie of
the contraction's argmax, the contraction's own boundary) are reported, from the oracle's numbers alone."""
import numpy as np
import torch

from oracle import vm_render_torch as O
from util import make_field

GRID = (20, 24, 28)          # non-cubic: an axis mix-up shows
CELL_TOL = 1e-4              # grid units from a cell boundary
TIE_TOL = 1e-5               # two largest |x| components (m > 1), and |m - 1|
MAX_FLAGGED_POINTS = 0.005
MAX_FLAGGED_RAYS = 0.02


def field(device, seed, grid=GRID, **over):
    """A field whose density planes and lines are 0.3 randn (seeded on the host), aabb +-2, everything else as constructed."""
    f = make_field(grid, "cpu", seed=seed, **over)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in list(f.density_plane) + list(f.density_line):
            p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    return f.to(device) if str(device) != "cpu" else f


def field_dict(f, dtype):
    """The oracle's `fld` of a field's density tensors and aabb, on the host in dtype."""
    sd = f.state_dict()
    keys = [f"density_plane.{i}" for i in range(3)] + [f"density_line.{i}" for i in range(3)]
    fld = {k: sd[k].detach().cpu().to(dtype) for k in keys}
    fld["aabb"] = f.aabb.detach().cpu().to(dtype)
    return fld


def grid_of(fld):
    """(gx, gy, gz) from the tensors: plane 0 is [1,C,gy,gx], line 0 is [1,C,gz,1]."""
    return (fld["density_plane.0"].shape[3], fld["density_plane.0"].shape[2], fld["density_line.0"].shape[2])


def contract(x):
    m = x.abs().amax(dim=-1, keepdim=True).clamp(min=1e-6)              # utils/ray_utils.py:9-12
    return torch.where(m <= 1, x, ((2 * m - 1) / (m ** 2)) * x)


def normalise(fld, xc):
    aabb = fld["aabb"]
    return (xc - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1


def density_of_x(fld, x):
    return O.density_feature(fld, normalise(fld, contract(x)))


def grad_u(fld, u):
    """d density_feature / du at u [P,3] (in fld's dtype) -> (grad [P,3], feature [P])."""
    u = u.detach().clone().requires_grad_(True)
    df = O.density_feature(fld, u)
    (g,) = torch.autograd.grad(df.sum(), u)
    return g.detach(), df.detach()


def grad_x(fld, x):
    """d g / dx at x [P,3] (in fld's dtype)."""
    x = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(density_of_x(fld, x).sum(), x)
    return g.detach()


def flag_u(u, grid):
    """[P] bool: a coordinate within CELL_TOL grid units of a cell boundary of the lattice (its two ends included)."""
    u = u.double()
    flagged = torch.zeros(u.shape[0], dtype=torch.bool)
    for a in range(3):
        ix = (u[:, a] + 1) / 2 * (grid[a] - 1)
        near = (ix - torch.round(ix)).abs() < CELL_TOL
        flagged |= near & (ix > -CELL_TOL) & (ix < grid[a] - 1 + CELL_TOL)
    return flagged


def flag_x(fld64, x):
    """[P] bool: the kinks of g at x [P,3] fp64 -> (flagged, contraction ties among them)."""
    ax = x.abs().sort(dim=-1, descending=True).values
    m = ax[:, 0]
    tie = (m > 1) & ((ax[:, 0] - ax[:, 1]) < TIE_TOL)
    edge = (m - 1).abs() < TIE_TOL
    cell = flag_u(normalise(fld64, contract(x)), grid_of(fld64))
    return tie | edge | cell, tie


def sample_positions(rays, z, dtype):
    """rays [R,6], z [S] -> x [R,S,3] = o + d / |d| z in dtype (tensorBase.py:578-580,438-440)."""
    rays, z = rays.detach().cpu().to(dtype), z.detach().cpu().to(dtype).view(-1)
    o, d = rays[:, :3], rays[:, 3:6]
    dh = d / torch.norm(d, dim=-1, keepdim=True)
    return o[:, None, :] + dh[:, None, :] * z[None, :, None]


def ray_normals(f, rays, z, weights, dtype):
    """The ray normals of the oracle in dtype, composited with the GIVEN weights [R,S] (fp32, as render_weights returned
    them): N = sum over w > thres of w n, n = -grad g / max(|grad g|, 1e-8).  -> (N [R,3], shaded [R,S] bool, x [R,S,3])."""
    fld = field_dict(f, dtype)
    x = sample_positions(rays, z, dtype)
    R, S = x.shape[:2]
    w = weights.detach().cpu()
    shaded = w > float(f.rayMarch_weight_thres)
    n = torch.zeros(R, S, 3, dtype=dtype)
    if shaded.any():
        g = grad_x(fld, x[shaded])
        n[shaded] = -g / torch.norm(g, dim=-1, keepdim=True).clamp(min=1e-8)
    N = (w.to(dtype)[..., None] * n * shaded[..., None]).sum(1)
    return N, shaded, x


def ray_case(f, rays, z, weights):
    """Everything a composite comparison needs: the fp64 oracle, e = max |fp32 - fp64| over the rays that stay, and the
    excluded rays (one of their shaded samples is flagged) -- all from the oracle alone."""
    N64, shaded, x64 = ray_normals(f, rays, z, weights, torch.float64)
    N32, _, _ = ray_normals(f, rays, z, weights, torch.float32)
    fld64 = field_dict(f, torch.float64)
    R, S = shaded.shape
    flagged, tie = flag_x(fld64, x64.reshape(-1, 3))
    flagged, tie = flagged.view(R, S), tie.view(R, S)
    excluded = (flagged & shaded).any(1)
    keep = ~excluded
    e = float((N32.double() - N64)[keep].abs().max()) if keep.any() else 0.0
    return {"N64": N64, "keep": keep, "excluded": int(excluded.sum()), "e": e, "shaded": shaded,
            "flagged_samples": int(flagged.sum()), "ties": int(tie.sum())}


def point_queries(seed, n=4096):
    """u [n + 14, 3] fp32: n points uniform in [-1.2, 1.2]^3, the eight corners, the six points +-1 on the axes."""
    gen = torch.Generator().manual_seed(seed)
    u = (torch.rand(n, 3, generator=gen) * 2.4 - 1.2).float()
    corners = torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    return torch.cat([u, corners, axes]).contiguous()


def test_rays(R, seed):
    """Origins 0.2 randn, directions randn: samples on both sides of the contraction."""
    gen = torch.Generator().manual_seed(seed)
    return torch.cat([0.2 * torch.randn(R, 3, generator=gen), torch.randn(R, 3, generator=gen)], -1)


test_rays.__test__ = False


def encode_normals_host(normal):
    """numpy restatement of normals.encode_normals: fp32 0.5 N / max(|N|, 1e-8) + 0.5, then novel_views_cases.rgb8_host."""
    from novel_views_cases import rgb8_host
    n = np.asarray(normal, np.float32)
    length = np.sqrt((n * n).sum(-1, dtype=np.float32), dtype=np.float32)
    unit = n / np.maximum(length, np.float32(1e-8))[..., None]
    return rgb8_host(np.float32(0.5) * unit + np.float32(0.5))
