// lrf_mesh.inl -- rendered depth fused into a truncated signed-distance (TSDF) volume, and a triangle mesh extracted from a
// scalar volume (included by lrf_render.hip after lrf_encode.inl and lrf_points.inl, whose enc_rgb_byte, pts_finite_pos and
// reproject it shares; the scans are lrf_compact.inl's, the host helpers lrf_host.inl's).  The fusion and the extraction are each written once, here, for the dense volume
// of this file and for the block-sparse one of lrf_tsdf_blocks.inl: the two differ only in where a lattice point is stored.
//
// A lattice has Nx x Ny x Nz points at origin + (ix, iy, iz) * voxel.  Per point: tsdf (starts at 1), weight (starts at 0), rgb
// in [0, 1] (3 floats, nullable, starts at 0).  The dense volume stores every point, x fastest: [Nz,Ny,Nx] and [Nz,Ny,Nx,3].
//
// Fusion (tsdf_fuse_point): one lane per stored point.  The point's tsdf, weight and rgb are read once, kept in registers over
// the frame loop and written once.  Per frame v in frame order, in fp32 with contraction off so that a numpy restatement
// matches bit for bit:
//   0. p = origin + (float)(ix, iy, iz) * voxel, one multiply and one add per axis (the kernel's part);
//   1. reproject (lrf_points.inl): q = R_v^T (p - t_v), nz = -q.z; skipped behind the camera or outside the image;
//   2. dn = depth[v,iw,iu]; skipped unless finite, positive and d_min <= dn <= d_max;
//   3. sdf = dn - nz (both in units of the un-normalised direction whose z is -1); skipped if sdf < -trunc;
//      s = min(1, sdf / trunc) (IEEE division);
//   4. tsdf = (tsdf * weight + s) / (weight + 1); rgb[c] = (rgb[c] * weight + (float)rgb8[v,iw,iu,c] / 255) / (weight + 1);
//      weight = weight + 1.
// The frame's camera-to-world matrix is addressed by the loop counter alone, so it is read with scalar loads into scalar
// registers.  No atomics; integrating frames k..V on the state frames 0..k left gives the bits of one call over 0..V.
// k_tsdf_integrate: a wave covers 64 consecutive x of one (z, y) row, so its reprojections land on neighbouring pixels.
//
// Extraction: marching tetrahedra on the Kuhn split of each cell.  Corners of a cell are numbered by their offset bits
// (bit 0 = x, bit 1 = y, bit 2 = z).  Tetrahedron t = 0..5 is the monotone path 000 -> 111 of the t-th permutation (a, b, c)
// of the axes in lexicographic order: corners 0, 1<<a, 1<<a | 1<<b, 7; the middle two are swapped for an odd permutation so
// that every tetrahedron is positively oriented.  The split is translation invariant: the face diagonals of neighbouring
// cells coincide, so the mesh has no cracks, and a tetrahedron has no ambiguous case.
// Every mesh vertex lies on one of the seven lattice edges a lattice point P owns: edge e = 0..6 runs from P to P + d with
// d = e + 1 read as offset bits -- (1,0,0), (0,1,0), (1,1,0), (0,0,1), (1,0,1), (0,1,1), (1,1,1).  A tetrahedron's edge between
// corners A and B (nested bit sets) is edge (A ^ B) - 1 of the point at corner A & B.
//   inside   value < level (strict)
//   valid    a cell whose eight corners have weight >= min_weight (every cell when weight is null)
//   vertex   on an owned edge whose ends straddle the level and that at least one valid cell contains (the cells at P - s
//            for the subsets s of the axes d leaves out); position pa + t * (pb - pa), t = (level - a) / (b - a), always
//            from the owning end a, so every cell that uses it sees the same bits; colour enc_rgb_byte(ca + t * (cb - ca))
//   faces    per valid cell, tetrahedron by tetrahedron: one inside corner i -> (ij, ik, il) for the even permutation
//            (i, j, k, l); three inside -> the outside corner's triangle reversed; two inside i, j -> (ik, il, jl) and
//            (ik, jl, jk).  The normal points towards value > level.
// The rules read the lattice through a view (MeshArgs here, BlocksMeshArgs in lrf_tsdf_blocks.inl) that maps storage to it:
//   point(p)               storage point p -> MeshPoint: its storage index and lattice coordinates
//   beside(q, dx, dy, dz)  offsets in -1..1 -> the neighbour's storage index; -2 beyond the lattice, -1 on the lattice but
//                          not stored (never from the dense view)
//   corner(q, d)           beside() for the corner d of the cell at q, for a cell known to be valid (the dense view skips the
//                          bounds checks)
//   stored(o)              o >= 0; val(o), passes(o), colour(o, c): the value, weight >= min_weight and rgb at o, where -1
//                          reads as value 1, weight 0, rgb 0.  A negative index is never dereferenced nor owns a vertex.
// Three launches, no atomics, no host synchronisation; storage order is (z, y, x) for the dense view:
//   count (mesh_count_body)  per storage point the 7-bit mask of its vertices, the triangles of its cell and the vertices
//                 before it in its workgroup -> info; per workgroup the vertex and face totals
//   k_points_scan two workgroups: exclusive vertex and face bases per workgroup, the true totals in counts[0..1]
//   emit (mesh_emit_body)  vertices in (storage point, edge) order, faces in (cell, tetrahedron, triangle) order; a face's
//                 vertex index is its owner's base + popcount(owner's mask below the edge).  Rows at or beyond capacity are
//                 not written.
namespace lrf {

constexpr int TSDF_NT = 256;
constexpr int MESH_NT = 256;                                        // lattice points per workgroup (info keeps 11 bits of prefix)
constexpr unsigned MESH_CELL = 0x361Bu;                             // the 8 corners of a cell in the 3x3x3 neighbourhood mask

struct TsdfArgs {
  float* tsdf; float* weight; float* rgb;
  int Nx, Ny, Nz, nxc;                                              // nxc: 64-point chunks per row
  long long n_items;                                                // Nz Ny nxc wave items
  float ox, oy, oz, voxel, trunc;
  int V, H, W;
  float d_min, d_max;
};

// steps 1..4 over the V frames for the point at pw whose state is stored at index p
__device__ __forceinline__ void tsdf_fuse_point(size_t p, const float (&pw)[3], float* tsdf, float* weight, float* rgb, float trunc,
                                                const float* __restrict__ depth, const uint8_t* __restrict__ rgb8,
                                                const float* __restrict__ c2w, const float* __restrict__ focal,
                                                const float* __restrict__ center, int V, int H, int W, float d_min, float d_max) {
#pragma clang fp contract(off)
  const float f = focal[0], cx = center[0], cy = center[1];
  float t = tsdf[p], wt = weight[p];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (rgb) { c0 = rgb[3 * p]; c1 = rgb[3 * p + 1]; c2 = rgb[3 * p + 2]; }
  for (int v = 0; v < V; ++v) {
    float nz;
    int iu, iw;
    if (!reproject(c2w + (size_t)v * 12, pw, f, cx, cy, W, H, nz, iu, iw)) continue;
    const size_t px = (size_t)v * H * W + (size_t)iw * W + iu;
    const float dn = depth[px];
    if (!(pts_finite_pos(dn) && dn >= d_min && dn <= d_max)) continue;
    const float sdf = dn - nz;
    if (sdf < -trunc) continue;
    const float s = fminf(1.0f, sdf / trunc);
    const float w1 = wt + 1.0f;
    t = (t * wt + s) / w1;
    if (rgb) {
      const uint8_t* c = rgb8 + 3 * px;
      c0 = (c0 * wt + (float)c[0] / 255.0f) / w1;
      c1 = (c1 * wt + (float)c[1] / 255.0f) / w1;
      c2 = (c2 * wt + (float)c[2] / 255.0f) / w1;
    }
    wt = w1;
  }
  tsdf[p] = t; weight[p] = wt;
  if (rgb) { rgb[3 * p] = c0; rgb[3 * p + 1] = c1; rgb[3 * p + 2] = c2; }
}

__global__ __launch_bounds__(TSDF_NT) void k_tsdf_integrate(TsdfArgs a, const float* __restrict__ depth,
                                                            const uint8_t* __restrict__ rgb8, const float* __restrict__ c2w,
                                                            const float* __restrict__ focal, const float* __restrict__ center) {
#pragma clang fp contract(off)
  const long long item = (long long)blockIdx.x * (TSDF_NT / 64) + (threadIdx.x >> 6);
  if (item >= a.n_items) return;
  const int xc = (int)(item % a.nxc);
  const long long row = item / a.nxc;
  const int iy = (int)(row % a.Ny), iz = (int)(row / a.Ny);
  const int ix = xc * 64 + (threadIdx.x & 63);
  if (ix >= a.Nx) return;
  const float pw[3] = {a.ox + (float)ix * a.voxel, a.oy + (float)iy * a.voxel, a.oz + (float)iz * a.voxel};
  tsdf_fuse_point((size_t)row * a.Nx + ix, pw, a.tsdf, a.weight, a.rgb, a.trunc, depth, rgb8, c2w, focal, center, a.V, a.H, a.W,
                  a.d_min, a.d_max);
}

// ------------------------------------------------------------------------------------------------ the case tables, in code
constexpr int mt_popc4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
// the edge of a tetrahedron between its corners i and j: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) -> 0..5
constexpr int mt_edge(int i, int j) { return i > j ? mt_edge(j, i) : (i == 0 ? j - 1 : i + j); }
constexpr unsigned mt_tri(int a, int b, int c, int slot) {
  return ((unsigned)a | (unsigned)b << 3 | (unsigned)c << 6) << (2 + 9 * slot);
}
// inside mask m of a positively oriented tetrahedron -> triangles | edge triples << 2 (three bits per edge, nine per triangle)
constexpr unsigned mt_case(int m) {
  // even permutations (i, j, k, l) of the corners that put a corner, or a pair, first: they keep the orientation
  constexpr int one[4][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {2, 0, 1, 3}, {3, 0, 2, 1}};
  constexpr int two[6][4] = {{0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {1, 2, 0, 3}, {1, 3, 2, 0}, {2, 3, 0, 1}};
  const int pc = mt_popc4(m);
  if (pc == 1 || pc == 3) {
    const int bit = pc == 1 ? m : (~m & 15);
    const int i = bit == 1 ? 0 : bit == 2 ? 1 : bit == 4 ? 2 : 3;
    const int ij = mt_edge(one[i][0], one[i][1]), ik = mt_edge(one[i][0], one[i][2]), il = mt_edge(one[i][0], one[i][3]);
    return 1u | (pc == 1 ? mt_tri(ij, ik, il, 0) : mt_tri(ij, il, ik, 0));
  }
  if (pc == 2) {
    for (int r = 0; r < 6; ++r) {
      if (((1 << two[r][0]) | (1 << two[r][1])) != m) continue;
      const int i = two[r][0], j = two[r][1], k = two[r][2], l = two[r][3];
      return 2u | mt_tri(mt_edge(i, k), mt_edge(i, l), mt_edge(j, l), 0) | mt_tri(mt_edge(i, k), mt_edge(j, l), mt_edge(j, k), 1);
    }
  }
  return 0u;
}
// corner k of tetrahedron t as offset bits
constexpr int mt_corner(int t, int k) {
  constexpr int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  constexpr int odd[6] = {0, 1, 1, 0, 0, 1};
  const int c1 = 1 << perm[t][0], c2 = c1 | 1 << perm[t][1];
  return k == 0 ? 0 : k == 3 ? 7 : ((k == 1) != (odd[t] != 0)) ? c1 : c2;
}
// the six edges of tetrahedron t, six bits each: owner corner | direction << 3
constexpr unsigned long long mt_tet_edges(int t) {
  constexpr int ea[6] = {0, 0, 0, 1, 1, 2}, eb[6] = {1, 2, 3, 2, 3, 3};
  unsigned long long out = 0;
  for (int k = 0; k < 6; ++k) {
    const int A = mt_corner(t, ea[k]), B = mt_corner(t, eb[k]);
    out |= (unsigned long long)((A & B) | (A ^ B) << 3) << (6 * k);
  }
  return out;
}
__constant__ unsigned MT_CASE[16] = {mt_case(0), mt_case(1), mt_case(2), mt_case(3), mt_case(4), mt_case(5), mt_case(6), mt_case(7),
                                     mt_case(8), mt_case(9), mt_case(10), mt_case(11), mt_case(12), mt_case(13), mt_case(14),
                                     mt_case(15)};

// a lattice point: its storage index and its lattice coordinates
struct MeshPoint { int p, x, y, z; };

// the dense view: storage index = (z Ny + y) Nx + x
struct MeshArgs {
  const float* value; const float* weight; const float* rgb;        // weight, rgb nullable
  int Nx, Ny, Nz, n;                                                // n = Nx Ny Nz < 2^31
  float ox, oy, oz, voxel, level, min_weight;

  __device__ __forceinline__ MeshPoint point(int p) const {
    const int r = p / Nx;
    return {p, p % Nx, r % Ny, r / Ny};
  }
  __device__ __forceinline__ int offset(int dx, int dy, int dz) const {
    return (int)(dx + (long long)dy * Nx + (long long)dz * Nx * Ny);
  }
  // q lies on the lattice, so an axis can only be left on the side its offset points to
  __device__ __forceinline__ int beside(const MeshPoint& q, int dx, int dy, int dz) const {
    if ((dx < 0 && q.x == 0) || (dx > 0 && q.x + 1 >= Nx) || (dy < 0 && q.y == 0) || (dy > 0 && q.y + 1 >= Ny) ||
        (dz < 0 && q.z == 0) || (dz > 0 && q.z + 1 >= Nz))
      return -2;
    return q.p + offset(dx, dy, dz);
  }
  __device__ __forceinline__ int corner(const MeshPoint& q, int d) const { return q.p + offset(d & 1, (d >> 1) & 1, (d >> 2) & 1); }
  __device__ __forceinline__ bool stored(int) const { return true; }
  __device__ __forceinline__ float val(int o) const { return value[o]; }
  __device__ __forceinline__ bool passes(int o) const { return !weight || weight[o] >= min_weight; }
  __device__ __forceinline__ float colour(int o, int c) const { return rgb[3 * (size_t)o + c]; }
};

// the inside bits of tetrahedron T's four corners, from the cell's eight
template <int T>
__device__ __forceinline__ unsigned mesh_tet_mask(unsigned cm) {
  return ((cm >> mt_corner(T, 0)) & 1u) | ((cm >> mt_corner(T, 1)) & 1u) << 1 | ((cm >> mt_corner(T, 2)) & 1u) << 2 |
         ((cm >> mt_corner(T, 3)) & 1u) << 3;
}
__device__ __forceinline__ unsigned mesh_tet_tris(unsigned m) {
  const unsigned pc = __popc(m);
  return pc == 2 ? 2u : (pc == 1 || pc == 3) ? 1u : 0u;
}

// info[p] = vertex mask | triangles of the cell << 7 | vertices before p in its workgroup << 11; part: MESH_NT / 64 words of LDS
template <class View>
__device__ __forceinline__ void mesh_count_body(const View& a, unsigned* part, unsigned* __restrict__ info,
                                                unsigned* __restrict__ wgv, unsigned* __restrict__ wgf) {
  const long long pl = (long long)blockIdx.x * MESH_NT + threadIdx.x;
  unsigned mask = 0, ntri = 0;
  if (pl < a.n) {
    const MeshPoint q = a.point((int)pl);
    const bool ina = a.val(q.p) < a.level;
    unsigned cm = ina ? 1u : 0u, present = 1u, strad = 0u;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
      const int o = a.beside(q, d & 1, (d >> 1) & 1, (d >> 2) & 1);
      if (o == -2) continue;
      const bool inb = a.val(o) < a.level;
      present |= 1u << d;
      cm |= (inb ? 1u : 0u) << d;
      if (inb != ina) strad |= 1u << (d - 1);
    }
    if (strad) {
      unsigned ok = 0;                                              // bit (dz+1) 9 + (dy+1) 3 + (dx+1): that neighbour can be a cell's corner
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        const int o = a.beside(q, k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1);
        if (o != -2 && a.passes(o)) ok |= 1u << k;
      }
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        const int d = e + 1, fr = ~d & 7;
        bool any = false;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          if (s & ~fr) continue;                                    // s: the axes along which the cell starts one point before P
          const int shift = 13 - (s & 1) - 3 * ((s >> 1) & 1) - 9 * ((s >> 2) & 1);
          any = any || ((ok >> shift) & MESH_CELL) == MESH_CELL;
        }
        if (((strad >> e) & 1u) && any) mask |= 1u << e;
      }
      if (present == 0xFFu && ((ok >> 13) & MESH_CELL) == MESH_CELL)
        ntri = mesh_tet_tris(mesh_tet_mask<0>(cm)) + mesh_tet_tris(mesh_tet_mask<1>(cm)) + mesh_tet_tris(mesh_tet_mask<2>(cm)) +
               mesh_tet_tris(mesh_tet_mask<3>(cm)) + mesh_tet_tris(mesh_tet_mask<4>(cm)) + mesh_tet_tris(mesh_tet_mask<5>(cm));
    }
  }
  unsigned vtot, ftot;
  const unsigned vpre = block_scan_excl<MESH_NT>(__popc(mask), part, vtot);
  block_scan_excl<MESH_NT>(ntri, part, ftot);
  if (pl < a.n) info[pl] = mask | ntri << 7 | vpre << 11;
  if (threadIdx.x == 0) { wgv[blockIdx.x] = vtot; wgf[blockIdx.x] = ftot; }
}

// the faces of tetrahedron T of the valid cell at q; a vertex is indexed through the point that owns its edge
template <int T, class View>
__device__ __forceinline__ void mesh_tet_faces(const View& a, const unsigned* __restrict__ info, const unsigned* __restrict__ wgv,
                                               const MeshPoint& q, unsigned cm, long long& row, long long max_faces,
                                               int* __restrict__ faces) {
  constexpr unsigned long long edges = mt_tet_edges(T);
  const unsigned m = mesh_tet_mask<T>(cm);
  if (m == 0u || m == 15u) return;
  const unsigned cs = MT_CASE[m];
  const int nt = (int)(cs & 3u);
  for (int j = 0; j < nt; ++j, ++row) {
    if (row >= max_faces) continue;
    for (int k = 0; k < 3; ++k) {
      const unsigned ek = (cs >> (2 + 9 * j + 3 * k)) & 7u;
      const unsigned code = (unsigned)(edges >> (6 * ek)) & 63u;    // owner corner | direction << 3
      const int o = a.corner(q, (int)(code & 7u));
      if (!a.stored(o)) continue;                                   // only under a block table that does not match the pools
      const unsigned oi = info[o];
      faces[3 * row + k] = (int)(wgv[(unsigned)o / MESH_NT] + (oi >> 11) + __popc(oi & ((1u << ((code >> 3) - 1u)) - 1u)));
    }
  }
}

template <class View>
__device__ __forceinline__ void mesh_emit_body(const View& a, unsigned* part, const unsigned* __restrict__ info,
                                               const unsigned* __restrict__ wgv, const unsigned* __restrict__ wgf,
                                               long long max_vertices, long long max_faces, float* __restrict__ vertices,
                                               uint8_t* __restrict__ rgb8_out, int* __restrict__ faces) {
#pragma clang fp contract(off)
  const long long pl = (long long)blockIdx.x * MESH_NT + threadIdx.x;
  const unsigned me = pl < a.n ? info[pl] : 0u;
  const unsigned mask = me & 127u, ntri = (me >> 7) & 15u;
  unsigned ftot;
  const unsigned fpre = block_scan_excl<MESH_NT>(ntri, part, ftot);
  if (!(mask | ntri)) return;
  const MeshPoint q = a.point((int)pl);
  if (mask) {
    long long row = (long long)wgv[blockIdx.x] + (me >> 11);
    const float va = a.val(q.p);
    const float pa[3] = {a.ox + (float)q.x * a.voxel, a.oy + (float)q.y * a.voxel, a.oz + (float)q.z * a.voxel};
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      if (!((mask >> e) & 1u)) continue;
      const int d = e + 1;
      if (row < max_vertices) {
        const int o = a.corner(q, d);                               // an edge of a valid cell: both ends are stored
        const float vb = a.val(o);
        const float t = (a.level - va) / (vb - va);
        const float pb[3] = {a.ox + (float)(q.x + (d & 1)) * a.voxel, a.oy + (float)(q.y + ((d >> 1) & 1)) * a.voxel,
                             a.oz + (float)(q.z + ((d >> 2) & 1)) * a.voxel};
        for (int c = 0; c < 3; ++c) vertices[3 * row + c] = pa[c] + t * (pb[c] - pa[c]);
        if (rgb8_out) {
          for (int c = 0; c < 3; ++c) {
            const float ca = a.colour(q.p, c), cb = a.colour(o, c);
            rgb8_out[3 * row + c] = (uint8_t)enc_rgb_byte(ca + t * (cb - ca));
          }
        }
      }
      ++row;
    }
  }
  if (ntri) {                                                       // the cell at q is valid: its eight corners are stored
    unsigned cm = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) cm |= (a.val(a.corner(q, d)) < a.level ? 1u : 0u) << d;
    long long row = (long long)wgf[blockIdx.x] + fpre;
    mesh_tet_faces<0>(a, info, wgv, q, cm, row, max_faces, faces);
    mesh_tet_faces<1>(a, info, wgv, q, cm, row, max_faces, faces);
    mesh_tet_faces<2>(a, info, wgv, q, cm, row, max_faces, faces);
    mesh_tet_faces<3>(a, info, wgv, q, cm, row, max_faces, faces);
    mesh_tet_faces<4>(a, info, wgv, q, cm, row, max_faces, faces);
    mesh_tet_faces<5>(a, info, wgv, q, cm, row, max_faces, faces);
  }
}

__global__ __launch_bounds__(MESH_NT) void k_mesh_count(MeshArgs a, unsigned* __restrict__ info, unsigned* __restrict__ wgv,
                                                        unsigned* __restrict__ wgf) {
  __shared__ unsigned part[MESH_NT / 64];
  mesh_count_body(a, part, info, wgv, wgf);
}

__global__ __launch_bounds__(MESH_NT) void k_mesh_emit(MeshArgs a, const unsigned* __restrict__ info,
                                                       const unsigned* __restrict__ wgv, const unsigned* __restrict__ wgf,
                                                       long long max_vertices, long long max_faces, float* __restrict__ vertices,
                                                       uint8_t* __restrict__ rgb8_out, int* __restrict__ faces) {
  __shared__ unsigned part[MESH_NT / 64];
  mesh_emit_body(a, part, info, wgv, wgf, max_vertices, max_faces, vertices, rgb8_out, faces);
}

// lattice points of a shape, or 0 when the entry points refuse it
static long long mesh_points(int Nx, int Ny, int Nz) {
  if (Nx < 1 || Ny < 1 || Nz < 1) return 0;
  const long long n = (long long)Nx * Ny;                            // < 2^62
  return n >= (1ll << 31) || n * Nz >= (1ll << 31) ? 0 : n * Nz;
}

// the checks of the frames every fusion entry point takes (dense and block-sparse); 0 when they pass
static int tsdf_check_frames(const char* who, const float* depth, const float* c2w, const float* focal, const float* center, int V,
                             int H, int W, float d_min, float d_max) {
  if (V < 1 || H < 1 || W < 1 || (long long)V * H * W >= (1ll << 31)) return refuse(who, "need V, H, W >= 1 and V H W < 2^31");
  if (!depth || !c2w || !focal || !center) return refuse(who, "null argument");
  if (!(d_min <= d_max)) return refuse(who, "need d_min <= d_max");
  if (misaligned(3, depth, c2w, focal, center)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  return 0;
}

// the checks of the level, the gate and the outputs both extract entry points take; 0 when they pass
static int mesh_check_outputs(const char* who, bool has_rgb, float level, bool gated, float min_weight, int64_t max_vertices,
                              int64_t max_faces, const float* vertices, const uint8_t* rgb8_out, const int32_t* faces,
                              const int64_t* counts, const void* workspace) {
  if (!vertices || !faces || !counts || !workspace) return refuse(who, "null argument");
  if (has_rgb != !!rgb8_out) return refuse(who, "rgb and rgb8_out go together");
  if (level != level) return refuse(who, "level must not be NaN");
  if (gated && !(min_weight > 0.0f)) return refuse(who, "min_weight must be > 0");
  if (max_vertices < 0 || max_faces < 0 || max_vertices >= (1ll << 31) || max_faces >= (1ll << 31))
    return refuse(who, "max_vertices and max_faces must lie in [0, 2^31)");
  if (misaligned(3, vertices, faces, workspace)) return refuse(who, "float and int32 arrays and the workspace must be 4-byte aligned");
  if (misaligned(7, counts)) return refuse(who, "counts must be 8-byte aligned");
  return 0;
}

// the workspace of an extraction over n storage points (dense and block-sparse): info, then the vertex and the face counts of
// the n_wg workgroups, one array of two rows for the scan; pad: a byte that keeps the size above 0 for an empty pool
struct MeshWs { int n_wg; unsigned* info; unsigned* wgv; unsigned* wgf; size_t bytes; };
static MeshWs mesh_carve(void* workspace, long long n, size_t pad) {
  Carver c(workspace);
  MeshWs w;
  w.n_wg = (int)blocks_for(n, MESH_NT);
  w.info = c.take<unsigned>((size_t)n);
  w.wgv = c.take<unsigned>(w.n_wg);
  w.wgf = c.take<unsigned>(w.n_wg);
  c.take<char>(pad);
  w.bytes = c.bytes();
  return w;
}

}  // namespace lrf

extern "C" int lrf_tsdf_integrate(const LrfTsdfVolume* vol, const float* depth, const uint8_t* rgb8, const float* cam2world,
                                  const float* focal, const float* center, int32_t V, int32_t H, int32_t W, float d_min,
                                  float d_max, void* stream) {
  using namespace lrf;
  if (!vol) return set_err("lrf_tsdf_integrate: null argument");
  const long long n = mesh_points(vol->Nx, vol->Ny, vol->Nz);
  if (!n) return set_err("lrf_tsdf_integrate: need Nx, Ny, Nz >= 1 and Nx Ny Nz < 2^31");
  if (!vol->tsdf || !vol->weight) return set_err("lrf_tsdf_integrate: null argument");
  if (tsdf_check_frames("lrf_tsdf_integrate", depth, cam2world, focal, center, V, H, W, d_min, d_max)) return 1;
  if (!vol->rgb != !rgb8) return set_err("lrf_tsdf_integrate: the volume's rgb and the frames' rgb8 go together");
  if (!(vol->voxel > 0.0f)) return set_err("lrf_tsdf_integrate: voxel must be > 0");
  if (!(vol->trunc > 0.0f)) return set_err("lrf_tsdf_integrate: trunc must be > 0");
  if (misaligned(3, vol->tsdf, vol->weight, vol->rgb)) return set_err("lrf_tsdf_integrate: float arrays must be 4-byte aligned");
  TsdfArgs a;
  memset(&a, 0, sizeof(a));
  a.tsdf = vol->tsdf; a.weight = vol->weight; a.rgb = vol->rgb;
  a.Nx = vol->Nx; a.Ny = vol->Ny; a.Nz = vol->Nz; a.nxc = (vol->Nx + 63) / 64;
  a.n_items = (long long)vol->Nz * vol->Ny * a.nxc;
  a.ox = vol->origin[0]; a.oy = vol->origin[1]; a.oz = vol->origin[2]; a.voxel = vol->voxel; a.trunc = vol->trunc;
  a.V = V; a.H = H; a.W = W; a.d_min = d_min; a.d_max = d_max;
  return launch(k_tsdf_integrate, blocks_for(a.n_items, TSDF_NT / 64), TSDF_NT, reinterpret_cast<hipStream_t>(stream), a, depth, rgb8,
                cam2world, focal, center);                          // <= 2^31 / 4 workgroups
}

extern "C" size_t lrf_mesh_workspace_bytes(int32_t Nx, int32_t Ny, int32_t Nz) {
  using namespace lrf;
  const long long n = mesh_points(Nx, Ny, Nz);
  return n ? mesh_carve(nullptr, n, 0).bytes : 0;
}

extern "C" int lrf_mesh_extract(const LrfMeshExtract* m, int64_t max_vertices, int64_t max_faces, float* vertices,
                                uint8_t* rgb8_out, int32_t* faces, int64_t* counts, void* workspace, void* stream) {
  using namespace lrf;
  if (!m) return set_err("lrf_mesh_extract: null argument");
  const long long n = mesh_points(m->Nx, m->Ny, m->Nz);
  if (!n) return set_err("lrf_mesh_extract: need Nx, Ny, Nz >= 1 and Nx Ny Nz < 2^31");
  if (!m->value) return set_err("lrf_mesh_extract: null argument");
  if (!(m->voxel > 0.0f)) return set_err("lrf_mesh_extract: voxel must be > 0");
  if (misaligned(3, m->value, m->weight, m->rgb)) return set_err("lrf_mesh_extract: float arrays must be 4-byte aligned");
  if (mesh_check_outputs("lrf_mesh_extract", m->rgb != nullptr, m->level, m->weight != nullptr, m->min_weight, max_vertices,
                         max_faces, vertices, rgb8_out, faces, counts, workspace))
    return 1;
  MeshArgs a;
  memset(&a, 0, sizeof(a));
  a.value = m->value; a.weight = m->weight; a.rgb = m->rgb;
  a.Nx = m->Nx; a.Ny = m->Ny; a.Nz = m->Nz; a.n = (int)n;
  a.ox = m->origin[0]; a.oy = m->origin[1]; a.oz = m->origin[2]; a.voxel = m->voxel;
  a.level = m->level; a.min_weight = m->min_weight;
  const MeshWs w = mesh_carve(workspace, n, 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_mesh_count, w.n_wg, MESH_NT, st, a, w.info, w.wgv, w.wgf));
  LRF_TRY(launch(k_points_scan, 2, PTS_SCAN_NT, st, w.wgv, w.n_wg, reinterpret_cast<long long*>(counts)));
  if (max_vertices == 0 && max_faces == 0) return 0;                 // a counting call: no row could be written
  return launch(k_mesh_emit, w.n_wg, MESH_NT, st, a, w.info, w.wgv, w.wgf, max_vertices, max_faces, vertices, rgb8_out, faces);
}
