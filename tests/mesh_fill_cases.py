"""Shared pieces of the hole-filling tests: the numpy restatement of csrc/lrf_mesh_fill.inl by another algorithm -- np.unique
with counts on a Nv + b keys for the boundary test (as tests/mesh_smooth_cases.py has it), the boundary loops traced one after
the other on the host with a visited set, the same integer arithmetic for the means -- and the cases: meshes of
tests/mesh_clean_cases.py and tests/mesh_smooth_cases.py with faces taken out, and hand-made ones for the edges of the rules.

A case is (mesh, max_edges, closable): closable says that the filled mesh must be closed.  fan 3 has no "max_edges = n - 1"
case: 2 lies outside [3, 4096] and is refused (tests/test_mesh_fill_host.py checks that refusal)."""
import functools

import numpy as np

from mesh_cases import F32, extract_host, lattice
from mesh_clean_cases import base_meshes, fan
from mesh_smooth_cases import FAR, TETRAHEDRON, moved
from mesh_smooth_cases import cases as smooth_cases
from mesh_simplify_cases import SHIFT

HOLE_KEYS = ("boundary_edges", "nonmanifold_edges", "degenerate_faces", "loops", "loop_edges", "longest_loop", "open_edges")


# ------------------------------------------------------------------------------------------------ the restatement
def boundary_host(mesh):
    """-> (tails a and heads b of the directed edges by id 3 f + k, the boundary mask, the non-manifold count, the degenerate
    face count)."""
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    nv = mesh["vertices"].shape[0]
    assert ((f >= 0) & (f < nv)).all(), "a bad face index: every call raises"
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    a, b = f.reshape(-1), f[:, (1, 2, 0)].reshape(-1)
    valid = np.repeat(~degenerate, 3)
    if not valid.any():
        return a, b, np.zeros(a.size, bool), 0, int(degenerate.sum())
    keys, counts = np.unique(a[valid] * nv + b[valid], return_counts=True)

    def count_of(k):
        at = np.minimum(np.searchsorted(keys, k), keys.size - 1)
        return np.where(keys[at] == k, counts[at], 0)
    same, opp = count_of(a * nv + b) - 1, count_of(b * nv + a)
    boundary = valid & (opp == 0)
    nonmanifold = valid & ((same > 0) | (opp > 1))
    return a, b, boundary, int(nonmanifold.sum()), int(degenerate.sum())


def loops_host(mesh, max_edges):
    """Items 1-3 -> (the fillable loops, each the list of its edge ids from its leader on, ordered by leader; the counts)."""
    a, b, boundary, nonmanifold, degenerate = boundary_host(mesh)
    nv = mesh["vertices"].shape[0]
    ids = np.nonzero(boundary)[0]
    n_out, n_in = np.bincount(a[ids], minlength=nv), np.bincount(b[ids], minlength=nv)
    first = {}
    for e in ids.tolist():                                          # ascending: the smallest edge that leaves each vertex
        first.setdefault(int(a[e]), e)
    nxt = {e: first[int(b[e])] if n_in[b[e]] == 1 and n_out[b[e]] == 1 else None for e in ids.tolist()}
    seen, loops = set(), []
    for e in ids.tolist():
        if e in seen:
            continue
        chain, cur = [e], nxt[e]
        seen.add(e)
        while cur is not None and cur not in seen:
            chain.append(cur)
            seen.add(cur)
            cur = nxt[cur]
        if cur == e and 3 <= len(chain) <= max_edges:               # a cycle, and e its smallest edge: all below it were seen
            loops.append(chain)
    x = np.ascontiguousarray(mesh["vertices"], F32)
    if nv == 0 or float((x.max(0).astype(np.float64) - x.min(0).astype(np.float64)).max()) == 0.0:
        loops = []                                                  # a box of zero extent fills nothing
    edges = sum(len(c) for c in loops)
    counts = {"boundary_edges": int(ids.size), "nonmanifold_edges": nonmanifold, "degenerate_faces": degenerate, "loops": len(loops),
              "loop_edges": edges, "longest_loop": max([len(c) for c in loops], default=0), "open_edges": int(ids.size) - edges}
    return loops, counts


def fill_host(mesh, max_edges):
    """Item 4 -> the filled mesh dict with "fill": the counts of loops_host and added_vertices, added_faces."""
    loops, counts = loops_host(mesh, max_edges)
    x = np.ascontiguousarray(mesh["vertices"], F32)
    f = np.ascontiguousarray(mesh["faces"], np.int32).reshape(-1, 3)
    c = mesh["rgb8"]
    nv, nf = x.shape[0], f.shape[0]
    out = dict(mesh, fill=dict(counts, added_vertices=len(loops), added_faces=counts["loop_edges"]))
    if not loops:
        return out
    assert np.isfinite(x).all()
    lo = (x.min(0) + F32(0.0)).astype(np.float64)                   # -0 becomes +0
    extent = float((x.max(0).astype(np.float64) - lo).max())
    s = 36 - int(np.frexp(extent)[1])
    q = np.rint(np.ldexp(x.astype(np.float64) - lo, s)).astype(np.int64)
    tail = f.reshape(-1).astype(np.int64)
    head = f[:, (1, 2, 0)].reshape(-1).astype(np.int64)
    new_v, new_c, rank = np.zeros((len(loops), 3), F32), np.zeros((len(loops), 3), np.uint8), {}
    for r, loop in enumerate(loops):
        L = len(loop)
        at = tail[loop]
        assert np.unique(at).size == L
        S = q[at].sum(0)
        m = S.astype(np.float64) / np.float64(L)
        new_v[r] = (lo + np.ldexp(m, -s)).astype(F32)
        if c is not None:
            C = c[at].astype(np.int64).sum(0)
            new_c[r] = (2 * C + L) // (2 * L)
        rank.update((e, r) for e in loop)
    new_f = np.array([(head[e], tail[e], nv + rank[e]) for e in sorted(rank)], np.int32).reshape(-1, 3)
    out.update(vertices=np.concatenate([x, new_v]), faces=np.concatenate([f, new_f]), rgb8=None if c is None else np.concatenate([c, new_c]),
               counts=(nv + len(loops), nf + new_f.shape[0]))
    return out


# ------------------------------------------------------------------------------------------------ the meshes
def without_faces(mesh, drop):
    keep = np.ones(mesh["faces"].shape[0], bool)
    keep[np.asarray(sorted(drop), np.int64)] = False
    f = np.ascontiguousarray(mesh["faces"][keep])
    return dict(mesh, faces=f, counts=(int(mesh["vertices"].shape[0]), int(f.shape[0])))


def apart_faces(mesh, n, seed):
    """n faces no two of which share a vertex, found in a seeded order."""
    f = np.asarray(mesh["faces"], np.int64)
    used, out = np.zeros(mesh["vertices"].shape[0], bool), []
    for i in np.random.default_rng(seed).permutation(f.shape[0]).tolist():
        if not used[f[i]].any():
            used[f[i]] = True
            out.append(i)
            if len(out) == n:
                return out
    raise AssertionError("the mesh has too few faces")


def cap_faces(mesh, seed_face, rim, allowed):
    """A disc of rim - 2 faces around seed_face whose border is one simple loop of `rim` edges: every added face shares
    exactly one edge with the disc and brings a vertex the disc does not hold, so the border grows by one edge and stays
    simple.  Only faces whose three vertices are `allowed` are taken."""
    f = np.asarray(mesh["faces"], np.int64)
    by_edge = {}
    for i, (p, q, r) in enumerate(f.tolist()):
        for u, w in ((p, q), (q, r), (r, p)):
            by_edge[(u, w)] = i
    disc, held = [seed_face], set(f[seed_face].tolist())
    border = [(int(f[seed_face][k]), int(f[seed_face][(k + 1) % 3])) for k in range(3)]
    assert all(allowed[v] for v in held)
    while len(disc) < rim - 2:
        for at, (u, w) in enumerate(border):                        # the first border edge whose far face qualifies
            g = by_edge.get((w, u))
            if g is None or g in disc:
                continue
            third = [v for v in f[g].tolist() if v not in (u, w)][0]
            if third in held or not allowed[third]:
                continue
            disc.append(g)
            held.add(third)
            border[at:at + 1] = [(u, third), (third, w)]
            break
        else:
            raise AssertionError("the disc cannot grow")
    return disc


def sphere_caps(rim):
    """The sphere with two discs taken out, in its lower and its upper part: one border of `rim` edges, one of rim + 1."""
    m = base_meshes()["sphere"]
    z = m["vertices"][:, 2]
    f = np.asarray(m["faces"], np.int64)
    low, high = z < 0.45, z > 0.56
    seed_low = int(np.nonzero(low[f].all(1))[0][0])
    seed_high = int(np.nonzero(high[f].all(1))[0][-1])
    return without_faces(m, cap_faces(m, seed_low, rim, low) + cap_faces(m, seed_high, rim + 1, high))


def bow_tie():
    """The sphere without two faces that share one vertex and no edge: two holes that touch."""
    m = base_meshes()["sphere"]
    f = np.asarray(m["faces"], np.int64)
    for v in range(m["vertices"].shape[0]):
        around = np.nonzero((f == v).any(1))[0].tolist()
        for i in around:
            for j in around:
                if len(set(f[i].tolist()) & set(f[j].tolist())) == 1:
                    return without_faces(m, [i, j])
    raise AssertionError("no such pair")


def _made(vertices, faces, rgb8=None):
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return {"vertices": v, "faces": f, "rgb8": None if rgb8 is None else np.ascontiguousarray(rgb8, dtype=np.uint8).reshape(-1, 3),
            "counts": (int(v.shape[0]), int(f.shape[0]))}


def colour_halves():
    """A square hole whose colour sums are 2, 3 and 1019 over 4: 0.5 rounds up to 1, 0.75 to 1, 254.75 to 255; and a triangle
    hole with sums 1, 2, 4 over 3: 0, 1, 1."""
    v = [[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, 0.2], [3, 0, 0], [4, 0, 0.3], [3, 1, 0.1]]
    c = [[0, 1, 255], [0, 0, 255], [1, 1, 255], [1, 1, 254], [0, 1, 2], [1, 0, 1], [0, 1, 1]]
    return _made(v, [(0, 1, 2), (0, 2, 3), (4, 5, 6)], c)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (mesh, max_edges, closable), in a fixed order."""
    sphere = base_meshes()["sphere"]
    minus20 = without_faces(sphere, apart_faces(sphere, 20, 71))
    tet = _made(TETRAHEDRON[0], TETRAHEDRON[1][:3])
    out = {
        "tetrahedron minus one face": (tet, 64, True),
        "sphere minus 20": (minus20, 64, True),
        "sphere minus 90": (without_faces(sphere, apart_faces(sphere, 90, 72)), 64, True),
        "sphere minus 20 / no colours": (dict(minus20, rgb8=None), 64, True),
        "sphere minus 20 / shifted": (moved(minus20, SHIFT), 64, True),
        "sphere minus 20 / far": (moved(minus20, -FAR), 64, True),
    }
    for rim in (3, 64, 65):
        out[f"sphere caps {rim}"] = (sphere_caps(rim), rim, False)
    for n, most in ((3, 3), (65, 65), (65, 4096), (1025, 1025), (65, 64), (1025, 1024)):
        out[f"fan {n} / max_edges {most}"] = (fan(n, seed=n % 97), most, most >= n)
    out["bow tie"] = (bow_tie(), 64, False)
    for name in ("three triangles on one edge", "strip", "a degenerate face", "one point"):
        out[name] = (smooth_cases()[name], 64, name == "a degenerate face")     # its three valid faces leave one loop of 5
    stray = _made(np.concatenate([[[5.0, -3.0, 2.0]], tet["vertices"], [[-1.0, 7.0, 0.5]]]), tet["faces"] + 1)
    out["an unreferenced vertex"] = (stray, 64, True)
    out["sphere"] = (sphere, 64, True)
    out["colour halves"] = (colour_halves(), 64, True)
    return out


CASE_NAMES = ("tetrahedron minus one face", "sphere minus 20", "sphere minus 90", "sphere minus 20 / no colours",
              "sphere minus 20 / shifted", "sphere minus 20 / far", "sphere caps 3", "sphere caps 64", "sphere caps 65",
              "fan 3 / max_edges 3", "fan 65 / max_edges 65", "fan 65 / max_edges 4096", "fan 1025 / max_edges 1025",
              "fan 65 / max_edges 64", "fan 1025 / max_edges 1024", "bow tie", "three triangles on one edge", "strip",
              "a degenerate face", "one point", "an unreferenced vertex", "sphere", "colour halves")
UNCHANGED = ("fan 65 / max_edges 64", "fan 1025 / max_edges 1024", "bow tie", "three triangles on one edge", "strip", "one point", "sphere")
CLOSABLE = tuple(n for n in CASE_NAMES if n not in UNCHANGED[:-1] + ("sphere caps 3", "sphere caps 64", "sphere caps 65"))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's fill of cases()[name], computed once and shared."""
    m, max_edges, _ = cases()[name]
    return fill_host(m, max_edges)


# ------------------------------------------------------------------------------------------------ the end-to-end volume
E2E_N = 32
E2E_H = 1.0 / 31
E2E_C, E2E_R = (0.5130, 0.4870, 0.5070), 0.35                      # mesh_cases.SPHERE_C, SPHERE_R
# the centre (ix, iy, iz) of the 3 x 3 x 3 block of lattice points whose weights are zeroed: on the surface, on the +x side.
# tests/test_mesh_fill_host.py checks on the host that the rim it leaves is one simple loop of at most 64 edges.
E2E_BLOCK = (27, 15, 16)


def e2e_volume(block=E2E_BLOCK):
    """(tsdf, weight) [32,32,32] fp32: the sphere's distance field, weight 1 but for the block."""
    p = lattice((0.0, 0.0, 0.0), E2E_H, (E2E_N,) * 3).astype(np.float64) - np.array(E2E_C)
    fld = (np.sqrt((p * p).sum(-1)) - E2E_R).astype(F32)
    w = np.ones_like(fld)
    ix, iy, iz = block
    w[iz - 1:iz + 2, iy - 1:iy + 2, ix - 1:ix + 2] = 0
    return fld, w


def e2e_mesh_host(block=E2E_BLOCK):
    fld, w = e2e_volume(block)
    return extract_host(fld, (0.0, 0.0, 0.0), E2E_H, weight=w)
