"""Shared pieces of the mesh tests: the numpy fp32 restatement of csrc/lrf_mesh.inl (k_tsdf_integrate and the marching
tetrahedra of k_mesh_count / k_mesh_emit, same operation order), the analytic fields and the topology helpers.  Everything is
float32 arithmetic on float32 arrays; Python numbers only appear as weak scalars."""
import numpy as np

from novel_views_cases import rgb8_host
from points_cases import reproject

F32 = np.float32


# ------------------------------------------------------------------------------------------------ integration
def new_volume(dims, colours=True):
    Nx, Ny, Nz = dims
    return {"tsdf": np.ones((Nz, Ny, Nx), F32), "weight": np.zeros((Nz, Ny, Nx), F32),
            "rgb": np.zeros((Nz, Ny, Nx, 3), F32) if colours else None}


def lattice(origin, voxel, dims):
    """[Nz,Ny,Nx,3]: origin + (float)(ix, iy, iz) * voxel, one multiply and one add per axis."""
    Nx, Ny, Nz = dims
    o, h = np.asarray(origin, F32), F32(voxel)
    x = o[0] + np.arange(Nx, dtype=F32) * h
    y = o[1] + np.arange(Ny, dtype=F32) * h
    z = o[2] + np.arange(Nz, dtype=F32) * h
    out = np.empty((Nz, Ny, Nx, 3), F32)
    out[..., 0], out[..., 1], out[..., 2] = x[None, None, :], y[None, :, None], z[:, None, None]
    return out


def integrate_host(vol, origin, voxel, trunc, depth, rgb8, c2w, f, cx, cy, depth_range=(0.0, np.inf)):
    """k_tsdf_integrate on the host, in place on vol (new_volume's dict); frames in order.  -> vol"""
    depth, c2w = np.asarray(depth, F32), np.asarray(c2w, F32)
    V, H, W = depth.shape
    Nz, Ny, Nx = vol["tsdf"].shape
    pw = lattice(origin, voxel, (Nx, Ny, Nz))
    lo, hi, tr = F32(depth_range[0]), F32(depth_range[1]), F32(trunc)
    t, wt, col = vol["tsdf"], vol["weight"], vol["rgb"]
    assert (col is None) == (rgb8 is None)
    for v in range(V):
        nz, u, w = reproject(pw, c2w[v], f, cx, cy)
        with np.errstate(all="ignore"):
            ru, rw = np.rint(u), np.rint(w)
            ok = (nz > 0) & (ru >= 0) & (ru < F32(2147483648.0)) & (rw >= 0) & (rw < F32(2147483648.0))
            iu = np.where(ok, ru, 0).astype(np.int64)
            iw = np.where(ok, rw, 0).astype(np.int64)
            ok &= (iu < W) & (iw < H)
            iu, iw = np.where(ok, iu, 0), np.where(ok, iw, 0)
            dn = depth[v][iw, iu]
            ok &= np.isfinite(dn) & (dn > 0) & (dn >= lo) & (dn <= hi)
            sdf = (dn - nz).astype(F32)
            ok &= ~(sdf < -tr)
            s = np.minimum(F32(1), sdf / tr).astype(F32)
            w1 = (wt + F32(1)).astype(F32)
            t[...] = np.where(ok, (t * wt + s) / w1, t)
            if col is not None:
                c = np.asarray(rgb8, np.uint8)[v][iw, iu].astype(F32) / F32(255)
                col[...] = np.where(ok[..., None], (col * wt[..., None] + c) / w1[..., None], col)
            wt[...] = np.where(ok, w1, wt)
    return vol


# ------------------------------------------------------------------------------------------------ the case tables
def _tet_edge(i, j):
    i, j = min(i, j), max(i, j)
    return j - 1 if i == 0 else i + j


_ONE = [(0, 1, 2, 3), (1, 0, 3, 2), (2, 0, 1, 3), (3, 0, 2, 1)]       # even permutations with a corner first
_TWO = [(0, 1, 2, 3), (0, 2, 3, 1), (0, 3, 1, 2), (1, 2, 0, 3), (1, 3, 2, 0), (2, 3, 0, 1)]   # ... with a pair first
_PERM = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
_ODD = [0, 1, 1, 0, 0, 1]


def tet_case(m):
    """Inside mask of a positively oriented tetrahedron -> list of triangles, each three tetrahedron edges (0..5)."""
    ins = [k for k in range(4) if (m >> k) & 1]
    if len(ins) in (1, 3):
        i = ins[0] if len(ins) == 1 else [k for k in range(4) if k not in ins][0]
        _, j, k, l = _ONE[i]
        ij, ik, il = _tet_edge(i, j), _tet_edge(i, k), _tet_edge(i, l)
        return [(ij, ik, il)] if len(ins) == 1 else [(ij, il, ik)]
    if len(ins) == 2:
        i, j, k, l = [q for q in _TWO if set(q[:2]) == set(ins)][0]
        return [(_tet_edge(i, k), _tet_edge(i, l), _tet_edge(j, l)), (_tet_edge(i, k), _tet_edge(j, l), _tet_edge(j, k))]
    return []


def tet_corners(t):
    """The four corners of tetrahedron t as offset bits (bit 0 = x), positively oriented."""
    a, b, _ = _PERM[t]
    c1, c2 = 1 << a, (1 << a) | (1 << b)
    return (0, c2, c1, 7) if _ODD[t] else (0, c1, c2, 7)


_EA, _EB = (0, 0, 0, 1, 1, 2), (1, 2, 3, 2, 3, 3)
CASE_N = np.array([len(tet_case(m)) for m in range(16)], np.int64)
CASE_E = np.zeros((16, 2, 3), np.int64)
for _m in range(16):
    for _j, _tri in enumerate(tet_case(_m)):
        CASE_E[_m, _j] = _tri
TET_LO = np.array([[tet_corners(t)[_EA[k]] & tet_corners(t)[_EB[k]] for k in range(6)] for t in range(6)], np.int64)
TET_D = np.array([[tet_corners(t)[_EA[k]] ^ tet_corners(t)[_EB[k]] for k in range(6)] for t in range(6)], np.int64)


# ------------------------------------------------------------------------------------------------ extraction
def _shift(a, d, fill):
    """a[iz + dz, iy + dy, ix + dx] for offset bits d (d > 0 axes shifted by +1), `fill` beyond the lattice."""
    out = np.full_like(a, fill)
    sx, sy, sz = d & 1, (d >> 1) & 1, (d >> 2) & 1
    Nz, Ny, Nx = a.shape[:3]
    out[:Nz - sz, :Ny - sy, :Nx - sx] = a[sz:, sy:, sx:]
    return out


def _shift_back(a, s, fill):
    """a[iz - sz, iy - sy, ix - sx] for offset bits s, `fill` beyond the lattice."""
    out = np.full_like(a, fill)
    sx, sy, sz = s & 1, (s >> 1) & 1, (s >> 2) & 1
    Nz, Ny, Nx = a.shape[:3]
    out[sz:, sy:, sx:] = a[:Nz - sz, :Ny - sy, :Nx - sx]
    return out


def extract_host(value, origin, voxel, level=0.0, weight=None, rgb=None, min_weight=1.0):
    """lrf_mesh_extract on the host -> dict(vertices [Nv,3] fp32, faces [Nf,3] int32, rgb8 [Nv,3] uint8 or None, counts)."""
    value = np.asarray(value, F32)
    Nz, Ny, Nx = value.shape
    lev = F32(level)
    with np.errstate(invalid="ignore"):
        inside = value < lev
        okpt = np.ones(value.shape, bool) if weight is None else np.asarray(weight, F32) >= F32(min_weight)
    cell = okpt.copy()                                              # cell[P]: the cell whose lowest corner is P is valid
    for d in range(1, 8):
        cell &= _shift(okpt, d, False)
    exist = np.zeros((Nz, Ny, Nx, 7), bool)
    for e in range(7):
        d = e + 1
        free = ~d & 7
        anyc = np.zeros(value.shape, bool)
        for s in range(8):
            if s & ~free:
                continue
            anyc |= _shift_back(cell, s, False)
        exist[..., e] = (inside != _shift(inside, d, False)) & _shift(np.ones(value.shape, bool), d, False) & anyc
    vid = (np.cumsum(exist.reshape(-1)) - 1).reshape(exist.shape)
    iz, iy, ix, e = np.nonzero(exist)                               # C order: (z, y, x, edge)
    d = e + 1
    pts = lattice(origin, voxel, (Nx + 1, Ny + 1, Nz + 1))
    pa = pts[iz, iy, ix]
    jz, jy, jx = iz + ((d >> 2) & 1), iy + ((d >> 1) & 1), ix + (d & 1)
    pb = pts[jz, jy, jx]
    va, vb = value[iz, iy, ix], value[jz, jy, jx]
    with np.errstate(all="ignore"):
        t = ((lev - va) / (vb - va)).astype(F32)
        verts = (pa + t[:, None] * (pb - pa)).astype(F32)
        rgb8 = None
        if rgb is not None:
            rgb = np.asarray(rgb, F32)
            ca, cb = rgb[iz, iy, ix], rgb[jz, jy, jx]
            rgb8 = rgb8_host((ca + t[:, None] * (cb - ca)).astype(F32)).reshape(-1, 3)
    # faces: per cell (lattice order), tetrahedron, triangle
    bits = np.zeros(value.shape, np.int64)
    for c in range(8):
        bits |= _shift(inside, c, False).astype(np.int64) << c
    cz, cy_, cx_ = np.nonzero(cell)
    cm = bits[cz, cy_, cx_]
    out = np.full((cm.size, 6, 2, 3), -1, np.int64)
    for tt in range(6):
        cs = tet_corners(tt)
        m = sum(((cm >> cs[k]) & 1) << k for k in range(4))
        for j in range(2):
            has = CASE_N[m] > j
            for k in range(3):
                ek = CASE_E[m, j, k]
                lo, dd = TET_LO[tt][ek], TET_D[tt][ek]
                oz, oy, ox = cz + ((lo >> 2) & 1), cy_ + ((lo >> 1) & 1), cx_ + (lo & 1)
                out[:, tt, j, k] = np.where(has, vid[oz, oy, ox, dd - 1], -1)
                assert exist[oz, oy, ox, dd - 1][has].all()
    faces = out.reshape(-1, 3)
    faces = faces[faces[:, 0] >= 0].astype(np.int32)
    return {"vertices": verts, "faces": faces, "rgb8": rgb8, "counts": (int(verts.shape[0]), int(faces.shape[0]))}


# ------------------------------------------------------------------------------------------------ analytic fields, topology
N_ANALYTIC = 24
H_ANALYTIC = 1.0 / 23
SPHERE_C, SPHERE_R = (0.5130, 0.4870, 0.5070), 0.35
TORUS_C, TORUS_R, TORUS_r = (0.5070, 0.4930, 0.5110), 0.27, 0.11


def analytic_lattice():
    return lattice((0.0, 0.0, 0.0), H_ANALYTIC, (N_ANALYTIC,) * 3).astype(np.float64)


def sphere_field():
    """|x - c| - r on the 24^3 lattice of the unit cube, fp32."""
    p = analytic_lattice() - np.array(SPHERE_C)
    return (np.sqrt((p * p).sum(-1)) - SPHERE_R).astype(F32)


def torus_field():
    """Signed distance to a torus with axis z, fp32."""
    p = analytic_lattice() - np.array(TORUS_C)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - TORUS_R
    return (np.sqrt(q * q + p[..., 2] ** 2) - TORUS_r).astype(F32)


def directed_edges(faces):
    """dict (a, b) -> how many faces run the edge a -> b."""
    f = np.asarray(faces, np.int64)
    out = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        out[(a, b)] = out.get((a, b), 0) + 1
    return out


def boundary_edges(faces):
    """Directed edges whose reverse no face runs."""
    de = directed_edges(faces)
    return [k for k in de if (k[1], k[0]) not in de]


def closed_manifold_euler(mesh):
    """Asserts: indices in range, every vertex used, every undirected edge in exactly two faces, once per direction.
    -> V - E + F"""
    v, f = mesh["vertices"], mesh["faces"]
    assert f.min() >= 0 and f.max() < v.shape[0]
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))
    de = directed_edges(f)
    assert all(n == 1 for n in de.values())
    assert all((b, a) in de for a, b in de)
    assert len(de) == 3 * f.shape[0]
    return v.shape[0] - len(de) // 2 + f.shape[0]


def signed_volume(mesh):
    v = mesh["vertices"].astype(np.float64)
    a, b, c = (v[mesh["faces"][:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)
