// lrf_mesh_simplify.inl -- an indexed triangle mesh simplified by uniform vertex clustering (Rossignac-Borrel): every vertex
// falls into a cell of a uniform grid, the vertices of a cell become one vertex at their mean, faces follow their vertices
// (included by lrf_render.hip; the keep lists and their scans are lrf_compact.inl's, the host helpers lrf_host.inl's; lrf_mesh_clean.inl's
// mf_workgroups sizes the face lists).
// The output bytes are a fixed function of the input: integer sums, fp64 operations that are each rounded on their own, and a
// choice among duplicate faces that does not depend on the order of arrival.  No sort, no floating-point atomics.
//
// A mesh is vertices [Nv,3] fp32, rgb8 [Nv,3] uint8 (nullable) and faces [Nf,3] int32.  cell > 0 is the cell edge and origin
// the grid's anchor, both doubles.
//   1. Cell of a vertex, per axis k: t = ((double)v[k] - origin[k]) / cell, i = floor(t), q = (uint64)((t - i) * 2^32).  A
//      vertex is bad when a coordinate is not finite or |i| >= 2^30 on an axis; a bad vertex is never used as an index.
//   2. Box: lo, hi = the per-axis minimum and maximum of i (int32 atomicMin / atomicMax), dims = hi - lo + 1, the linear cell
//      index has x fastest, then y, then z; cells = dx dy dz < 2^31.
//   3. Clusters: every cell that holds a vertex, numbered in increasing linear cell index: one bit per cell (atomicOr), the
//      popcounts per word and per 16 words, one ordered scan (k_points_scan).  There is no hash here.
//   4. Representative, per cluster: S[k] = sum of q (uint64), n (uint32), C[c] = sum of rgb8 (uint32), all integer atomicAdd.
//      x[k] = (float)(origin[k] + ((double)i[k] + ((double)S[k] / (double)n) * 2^-32) * cell), every operation rounded on its
//      own (the functions that hold them switch contraction off: no multiply and add become an FMA); colour (2 C[c] + n) / (2 n) in integers.
//      (uint32 colour sums hold 2^24 vertices per cluster.)
//   5. Faces: every index becomes its vertex's cluster; a face with two equal clusters is degenerate and dropped; the others
//      are rotated so that the smallest cluster comes first (the winding stays; the triple is the face's key).  With dedupe,
//      among faces of equal keys the one with the smallest input index survives.  Survivors keep their input order.
//   6. Vertices out: the clusters that a surviving face holds, in cluster order; a cluster's row is the number of such
//      clusters before it.  A mesh without faces simplifies to the empty mesh.
//
// Duplicate faces without a sort: an open-addressing table of int32 FACE INDICES (not keys), a power of two >= 2 Nf and >= 64
// slots, all -1 at the start.  The keys lie in tri [Nf,3], written by the launch before (-1 for a dropped face).
//   insert  one lane per face f with a key, probing linearly from hash(key): old = atomicCAS(&slot, -1, f); old == -1: done;
//           key(old) == key(f): atomicMin(&slot, f), done; else the next slot.  Only faces of equal key ever replace a slot's
//           value, so the key of a claimed slot never changes and comparing against the returned old is sound.
//   keep    a later launch probes read-only: f stays iff the slot that holds its key holds f.
// No waiting: one compare-and-swap per visited slot and no retry of it, so the probe loop is bounded by the capacity -- the
// table is never more than half full -- and cannot spin; no lane, wave or workgroup waits on another, every other loop is
// bounded by a constant, and a kernel is a fixed sequence: like lrf_mesh_clean.inl it cannot deadlock under any scheduling.
// Per key the minimum index survives, whatever the hash function and whatever the scheduling.  Data moves between lanes
// inside a launch only through the values atomics return; everything else a lane reads was written by an earlier launch.
//
// lrf_mesh_simplify_bounds, two launches:
//   k_ms_bounds_init   lo = INT_MAX, hi = INT_MIN, flag = 0
//   k_ms_bounds        one lane per vertex: its cell; per wave a shuffle reduction and six atomicMin / atomicMax; a bad vertex
//                      sets bit 0 of the flag and enters neither
// lrf_mesh_simplify, twelve launches (eleven without dedupe, five without faces):
//   k_ms_zero          cell bits, referenced-cluster bits, face keep bits, accumulators, flag and counts = 0; the table = -1
//   k_ms_mark          one lane per vertex: atomicOr of its cell's bit (one per run of equal cells in a wave); a vertex that is
//                      bad or outside the box given sets bit 1 of the flag and is skipped
//   k_ms_count_words   one lane per word: the set bits before it within its group of 16 words, and the group's total
//   k_points_scan      exclusive bases of the groups; counts[2] = occupied cells
//   k_ms_accumulate    one lane per vertex: cluster = rank of its cell's bit; the atomicAdds of 4., one set per run of equal
//                      clusters in a wave (a segmented scan sums the run first: integers, so the same sums); cluster_of[v],
//                      cell_of[cluster]
//   k_ms_faces_map     one lane per face: tri[f] = its canonical key or -1.  A face with an index outside [0, Nv) is never
//                      dereferenced and sets bit 0 of the flag, as k_cc_hook does.  counts[3] += degenerate faces
//   k_ms_faces_insert  (dedupe only) the insert above
//   k_ms_faces_keep    one lane per face: kept or not (the ballot is the keep word); a kept face ORs the bits of its three
//                      clusters into the referenced words; counts[4] += duplicate faces
//   k_ms_count_words   the referenced and the face words (blockIdx.y)
//   k_points_scan      two workgroups: counts[0] = vertices out, counts[1] = faces out
//   k_ms_write         a referenced cluster's position and colour to its row; a kept face's three clusters, as rows, to its row
//   k_ms_finish        flag bit 0: counts[1] = -1 (a bad face index); bit 1: counts[0] = -1 (a vertex outside the box)
// With Nf = 0 no face kernel runs: zero, mark, count, scan, finish.
//
// Quadric placement (lrf_mesh_simplify_quadric): items 1, 2, 3, 5 and 6 as above and item 4's colour; item 4's position becomes
// the minimum of the cluster's summed plane quadric (Lindstrom, out-of-core simplification), inside the cluster's closed cell.
// i_c is the integer cell of cluster c; i_v, q_v are item 1's cell and fraction of vertex v.
//   a. Contributions.  A face contributes once to each DISTINCT cluster among its three corners, whether it survives or not.
//      In the frame of cluster c, in cell units: u_j = (double)(i_vj - i_c) + (double)q_vj * 2^-32; n = (u_1 - u_0) x (u_2 - u_0)
//      (each component one product minus another); d = -((n_x u_0x + n_y u_0y) + n_z u_0z); the nine coefficients n_x^2, n_y^2,
//      n_z^2, n_x n_y, n_x n_z, n_y n_z, -d n_x, -d n_y, -d n_z.  Every operation rounded on its own.  n is not normalised: a face
//      weighs by its squared area, and there is no square root and no division.  g = max(n_x^2, n_y^2, n_z^2, d^2); a
//      contribution with g == 0 (a face without area, a repeated index) or g not finite is skipped.
//   b. One exponent per cluster.  E_c = the maximum of ilogb(g) over the cluster's contributions (int32 atomicMax).  A
//      contribution adds llrint(ldexp(coef, 40 - E_c)), of magnitude <= 2^41, to nine int64 sums and 1 to the uint32 count m_c
//      (integer atomicAdd: no order).  The sums are exact for m_c < 2^21; a cluster with m_c >= 2^21 keeps the mean.
//   c. Solve (the common scale cancels).  A, b = the sums as doubles; mu = item 4's mean fraction ((double)S / (double)n) * 2^-32;
//      tr = (A00 + A11) + A22, l = regularize * tr, M = A + l I, r = b + l mu.  x = adj(M) r / det(M) by cofactors in this order:
//        c00 = M11 M22 - M12 M12   c01 = M02 M12 - M01 M22   c02 = M01 M12 - M02 M11
//        c11 = M00 M22 - M02 M02   c12 = M01 M02 - M00 M12   c22 = M00 M11 - M01 M01
//        det = (M00 c00 + M01 c01) + M02 c02
//        x_0 = ((c00 r_0 + c01 r_1) + c02 r_2) / det, x_1 with (c01, c11, c12), x_2 with (c02, c12, c22)
//      The cluster keeps the mean when m_c == 0, tr <= 0, det <= 0 or an x_k is not finite; else every x_k is clamped to [0, 1].
//      The regulariser decides the position inside a plane and along a crease.
//   d. Position: (float)(origin[k] + ((double)i_c[k] + x_k) * cell), item 4's expression with x in place of the mean fraction.
// The bytes depend on neither the vertex order, the face order nor the scheduling.  No waiting, as above: single atomics whose
// results nobody reads, never retried; constant trip counts; no scratch.
// lrf_mesh_simplify_quadric, sixteen launches (fifteen without dedupe, six without faces): k_ms_quadric_zero first (the sums and
// counts = 0, E = INT_MIN, counts[5], counts[6] = 0), the launches of lrf_mesh_simplify up to k_ms_write, which leaves the
// mean in every row, then
//   k_ms_quadric_exponent    one lane per face: rule a's g per distinct cluster, the atomicMax of b.  Corner 0's maximum is
//                            taken over each run of equal clusters in the wave first (a segmented scan)
//   k_ms_quadric_accumulate  one lane per face: rule a again, the ten atomicAdds of b per distinct cluster; corner 0's ten
//                            values are summed over each run of equal clusters in the wave first, as k_ms_accumulate does
//   k_ms_quadric_place       one lane per cluster: an emitted cluster that solves (c) overwrites its row's position (d); the
//                            others keep k_ms_write's bytes.  counts[5] += emitted clusters left at the mean, counts[6] +=
//                            emitted clusters with an x_k outside [0, 1]
// and k_ms_finish.
namespace lrf {

constexpr int MS_NT = 256;
constexpr int MS_ZERO_BLOCKS = 4096;                                // k_ms_zero strides over its words
constexpr double MS_I_LIMIT = 1073741824.0;                         // 2^30
constexpr double MS_Q_ONE = 4294967296.0;                           // 2^32

struct MsGrid { double origin[3]; double cell; int lo[3]; int dims[3]; };

// item 1 -> false for a bad vertex
__device__ __forceinline__ bool ms_cell(const float* __restrict__ v, const double* origin, double cell, int* i,
                                        unsigned long long* q) {
#pragma clang fp contract(off)
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t = ((double)v[k] - origin[k]) / cell;
    const double fl = floor(t);
    if (!(fabs(fl) < MS_I_LIMIT)) { ok = false; i[k] = 0; q[k] = 0; continue; }       // NaN fails too
    i[k] = (int)fl;
    q[k] = (unsigned long long)((t - fl) * MS_Q_ONE);
  }
  return ok;
}

// the linear cell of a vertex inside the box, or -1
__device__ __forceinline__ long long ms_linear(const MsGrid& g, const int* i) {
  long long c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = (long long)i[k] - g.lo[k];
    if (c[k] < 0 || c[k] >= g.dims[k]) return -1;
  }
  return (c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0];
}

__global__ __launch_bounds__(64) void k_ms_bounds_init(int* __restrict__ out) {
  const int t = threadIdx.x;
  if (t < 3) out[t] = 0x7fffffff;
  else if (t < 6) out[t] = -0x7fffffff - 1;
  else if (t == 6) out[t] = 0;
}

__global__ __launch_bounds__(MS_NT) void k_ms_bounds(const float* __restrict__ vertices, int Nv, MsGrid g, int* out) {
  const long long v = (long long)blockIdx.x * MS_NT + threadIdx.x;
  int i[3] = {0, 0, 0};
  unsigned long long q[3];
  const bool have = v < Nv;
  const bool ok = have && ms_cell(vertices + 3 * v, g.origin, g.cell, i, q);
  const unsigned long long good = __ballot(ok);
  int lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_min(ok ? i[k] : 0x7fffffff);
    hi[k] = wave_max(ok ? i[k] : -0x7fffffff - 1);
  }
  if ((threadIdx.x & 63) == 0 && good) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMin(&out[k], lo[k]); atomicMax(&out[3 + k], hi[k]); }
  }
  wave_or(&out[6], have && !ok, 1);
}

__global__ __launch_bounds__(MS_NT) void k_ms_zero(unsigned long long* __restrict__ zero, size_t n_zero,
                                                   unsigned long long* __restrict__ table, size_t n_table,
                                                   long long* __restrict__ counts) {
  const size_t stride = (size_t)gridDim.x * MS_NT;
  const size_t t0 = (size_t)blockIdx.x * MS_NT + threadIdx.x;
  for (size_t i = t0; i < n_zero; i += stride) zero[i] = 0ull;
  for (size_t i = t0; i < n_table; i += stride) table[i] = ~0ull;   // two slots of -1
  if (t0 < 5) counts[t0] = 0;
}

__global__ __launch_bounds__(MS_NT) void k_ms_mark(const float* __restrict__ vertices, int Nv, MsGrid g,
                                                   unsigned long long* cell_bits, int* flag) {
  const long long v = (long long)blockIdx.x * MS_NT + threadIdx.x;
  int i[3];
  unsigned long long q[3];
  long long lin = -1;
  const bool have = v < Nv;
  if (have && ms_cell(vertices + 3 * v, g.origin, g.cell, i, q)) lin = ms_linear(g, i);
  // a mesh in extraction order has runs of one cell: the first lane of a run of equal cells speaks for it
  const long long before = __shfl_up(lin, 1, 64);
  if (lin >= 0 && ((threadIdx.x & 63) == 0 || before != lin)) atomicOr(&cell_bits[lin >> 6], 1ull << (lin & 63));
  wave_or(flag, have && lin < 0, 2);
}

// the pre and wg of gridDim.y stacked keep lists (KeepList::pick) from their bits; words is a multiple of KEEP_GROUP
__global__ __launch_bounds__(MS_NT) void k_ms_count_words(const unsigned long long* __restrict__ bits, unsigned* __restrict__ pre,
                                                          unsigned* __restrict__ wg, long long words) {
  const long long w = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const size_t at = (size_t)blockIdx.y * words;
  const unsigned c = w < words ? (unsigned)__popcll(bits[at + w]) : 0u;
  const unsigned s = wave_scan_incl<KEEP_GROUP>(c);
  if (w < words) {
    pre[at + w] = s - c;
    if ((threadIdx.x & (KEEP_GROUP - 1)) == KEEP_GROUP - 1) wg[(size_t)blockIdx.y * (words / KEEP_GROUP) + w / KEEP_GROUP] = s;
  }
}

__global__ __launch_bounds__(MS_NT) void k_ms_accumulate(const float* __restrict__ vertices, const uint8_t* __restrict__ rgb8, int Nv,
                                                         MsGrid g, const unsigned long long* __restrict__ cell_bits,
                                                         const unsigned* __restrict__ pre, const unsigned* __restrict__ wg,
                                                         unsigned long long* S, unsigned* nC, int* __restrict__ cell_of,
                                                         int* __restrict__ cluster_of) {
  const long long v = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int i[3];
  unsigned long long s[3] = {0ull, 0ull, 0ull};
  unsigned n[4] = {1u, 0u, 0u, 0u};                                 // the vertex count and the colour sums
  long long lin = -1;
  int cl = -1;
  if (v < Nv) {
    if (ms_cell(vertices + 3 * v, g.origin, g.cell, i, s)) lin = ms_linear(g, i);
    if (lin >= 0) cl = (int)KeepList{cell_bits, pre, wg}.rank(lin);
    if (!in_range(cl, Nv)) cl = -1;                                    // cannot happen after k_ms_mark of the same vertices
    if (cl >= 0 && rgb8) {
#pragma unroll
      for (int c = 0; c < 3; ++c) n[1 + c] = rgb8[3 * v + c];
    }
    cluster_of[v] = cl;
  }
  // a mesh in extraction order has runs of one cluster: a segmented inclusive scan over the wave's lanes (six steps, every
  // lane takes part) leaves each run's integer sums in its last lane, which adds them: the same sums as one add per vertex
  const int cl_before = __shfl_up(cl, 1, 64), cl_after = __shfl_down(cl, 1, 64);      // every lane takes part in both
  bool head = lane == 0 || cl_before != cl;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned long long ts[3];
    unsigned tn[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) ts[k] = __shfl_up(s[k], off, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) tn[k] = __shfl_up(n[k], off, 64);
    const int th = __shfl_up((int)head, off, 64);
    if (lane >= off && !head) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += ts[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) n[k] += tn[k];
      head = th != 0;
    }
  }
  const bool tail = lane == 63 || cl_after != cl;
  if (cl < 0 || !tail) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd(&S[3 * (size_t)cl + k], s[k]);
  atomicAdd(&nC[4 * (size_t)cl], n[0]);
  if (rgb8) {
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(&nC[4 * (size_t)cl + 1 + c], n[1 + c]);
  }
  cell_of[cl] = (int)lin;                                           // every run of the cluster stores the same value
}

__global__ __launch_bounds__(MS_NT) void k_ms_faces_map(const int* __restrict__ faces, int Nf, int Nv,
                                                        const int* __restrict__ cluster_of, int* __restrict__ tri, int* flag,
                                                        unsigned long long* counts) {
  const long long f = (long long)blockIdx.x * MS_NT + threadIdx.x;
  bool bad = false, degenerate = false;
  if (f < Nf) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int k0 = -1, k1 = -1, k2 = -1;
    if (!(in_range(a, Nv) && in_range(b, Nv) && in_range(c, Nv))) {
      bad = true;
    } else {
      const int ca = cluster_of[a], cb = cluster_of[b], cc = cluster_of[c];
      if (ca < 0 || cb < 0 || cc < 0) {
        // a vertex outside the box: k_ms_mark has set the flag
      } else if (ca == cb || cb == cc || ca == cc) {
        degenerate = true;
      } else if (ca < cb && ca < cc) {
        k0 = ca; k1 = cb; k2 = cc;
      } else if (cb < ca && cb < cc) {
        k0 = cb; k1 = cc; k2 = ca;
      } else {
        k0 = cc; k1 = ca; k2 = cb;
      }
    }
    tri[3 * f] = k0; tri[3 * f + 1] = k1; tri[3 * f + 2] = k2;
  }
  wave_or(flag, bad, 1);
  wave_count(&counts[3], degenerate);
}

__device__ __forceinline__ unsigned long long ms_hash(int k0, int k1, int k2) {
  unsigned long long h = (unsigned long long)(unsigned)k0 * 0x9E3779B97F4A7C15ull;
  h ^= (((unsigned long long)(unsigned)k1 << 32) | (unsigned)k2) * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  return h ^ (h >> 32);
}

__global__ __launch_bounds__(MS_NT) void k_ms_faces_insert(const int* __restrict__ tri, int Nf, int* table, unsigned long long mask) {
  const long long f = (long long)blockIdx.x * MS_NT + threadIdx.x;
  if (f >= Nf) return;
  const int k0 = tri[3 * f];
  if (k0 < 0) return;
  const int k1 = tri[3 * f + 1], k2 = tri[3 * f + 2];
  unsigned long long slot = ms_hash(k0, k1, k2) & mask;
  // one compare-and-swap per visited slot, at most capacity slots: at most Nf <= capacity / 2 of them are ever claimed
  for (unsigned long long step = 0; step <= mask; ++step) {
    const int old = atomicCAS(&table[slot], -1, (int)f);
    if (old == -1) return;
    if (!in_range(old, Nf)) return;                                    // not a table of k_ms_zero
    if (tri[3 * (size_t)old] == k0 && tri[3 * (size_t)old + 1] == k1 && tri[3 * (size_t)old + 2] == k2) {
      atomicMin(&table[slot], (int)f);
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// the grid covers words * 64 faces: every keep word is written
__global__ __launch_bounds__(MS_NT) void k_ms_faces_keep(const int* __restrict__ tri, int Nf, int n_clusters_max,
                                                         const int* __restrict__ table, unsigned long long mask, int dedupe,
                                                         unsigned long long* __restrict__ face_bits, unsigned long long* ref_bits,
                                                         unsigned long long* counts) {
  const long long f = (long long)blockIdx.x * MS_NT + threadIdx.x;
  bool keyed = false, keep = false;
  int k0 = -1, k1 = -1, k2 = -1;
  if (f < Nf) {
    k0 = tri[3 * f]; k1 = tri[3 * f + 1]; k2 = tri[3 * f + 2];
    keyed = in_range(k0, n_clusters_max) && in_range(k1, n_clusters_max) && in_range(k2, n_clusters_max);
  }
  if (keyed) {
    if (!dedupe) {
      keep = true;
    } else {
      unsigned long long slot = ms_hash(k0, k1, k2) & mask;
      for (unsigned long long step = 0; step <= mask; ++step) {     // read-only: the table is the launch before's
        const int s = table[slot];
        if (!in_range(s, Nf)) break;                                   // an empty slot: cannot happen for an inserted key
        if (tri[3 * (size_t)s] == k0 && tri[3 * (size_t)s + 1] == k1 && tri[3 * (size_t)s + 2] == k2) { keep = s == (int)f; break; }
        slot = (slot + 1) & mask;
      }
    }
  }
  if (keep) {
    atomicOr(&ref_bits[k0 >> 6], 1ull << (k0 & 63));
    atomicOr(&ref_bits[k1 >> 6], 1ull << (k1 & 63));
    atomicOr(&ref_bits[k2 >> 6], 1ull << (k2 & 63));
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) face_bits[f >> 6] = m;
  wave_count(&counts[4], keyed && !keep);
}

// item 4's position from the fraction of the cell, and the mean fraction: every operation is rounded on its own
__device__ __forceinline__ float ms_position_at(double origin, double cell, int i, double frac) {
#pragma clang fp contract(off)
  const double t = (double)i + frac;
  const double x = t * cell;
  return (float)(origin + x);
}
__device__ __forceinline__ double ms_mean_fraction(unsigned long long S, unsigned n) {
#pragma clang fp contract(off)
  const double mean = (double)S / (double)n;
  return mean * (1.0 / MS_Q_ONE);
}
__device__ __forceinline__ float ms_position(double origin, double cell, int i, unsigned long long S, unsigned n) {
  return ms_position_at(origin, cell, i, ms_mean_fraction(S, n));
}

// bits, pre, wg: two stacked keep lists of `words` words each (referenced clusters, faces), scanned
__global__ __launch_bounds__(MS_NT) void k_ms_write(MsGrid g, const unsigned long long* __restrict__ S, const unsigned* __restrict__ nC,
                                                    const int* __restrict__ cell_of, const int* __restrict__ tri,
                                                    const unsigned long long* __restrict__ bits, const unsigned* __restrict__ pre,
                                                    const unsigned* __restrict__ wg, long long words, float* __restrict__ vertices_out,
                                                    uint8_t* __restrict__ rgb8_out, int* __restrict__ faces_out) {
  const long long i = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const int which = blockIdx.y;
  if (i >= words * 64) return;
  const KeepList clusters{bits, pre, wg}, mine = clusters.pick(which, (size_t)words);
  if (!mine.kept(i)) return;                                        // a set bit: the cluster has vertices, the face has a key
  const size_t row = (size_t)(int)mine.rank(i);
  if (!which) {
    const int lin = cell_of[i];
    const int c[3] = {lin % g.dims[0], (lin / g.dims[0]) % g.dims[1], lin / g.dims[0] / g.dims[1]};
    const unsigned n = nC[4 * i];
#pragma unroll
    for (int k = 0; k < 3; ++k) vertices_out[3 * row + k] = ms_position(g.origin[k], g.cell, g.lo[k] + c[k], S[3 * i + k], n);
    if (rgb8_out) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        rgb8_out[3 * row + k] = (uint8_t)((2ull * nC[4 * i + 1 + k] + n) / (2ull * n));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) faces_out[3 * row + k] = (int)clusters.rank((long long)tri[3 * i + k]);
  }
}

// ---------------------------------------------------------------------------------------------- quadric placement (rules a-d)
constexpr unsigned MS_Q_CAP = 1u << 21;                             // the cap of rule b: below it the nine sums are exact
constexpr int MS_Q_BITS = 40;                                       // a scaled coefficient has magnitude <= 2^41
constexpr int MS_Q_NONE = -0x7fffffff - 1;                          // E of a cluster without a contribution

// the corners of face f: clusters, cells, fractions -> false for a face that contributes nowhere (past Nf, an index outside
// [0, Nv), which is never dereferenced, or a corner without a cluster)
__device__ __forceinline__ bool ms_quadric_face(const float* __restrict__ vertices, const int* __restrict__ faces, long long f, int Nf,
                                                int Nv, const MsGrid& g, const int* __restrict__ cluster_of, int* cl, int (*i)[3],
                                                unsigned long long (*q)[3]) {
  if (f >= Nf) return false;
  int at[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) at[j] = faces[3 * f + j];
  if (!(in_range(at[0], Nv) && in_range(at[1], Nv) && in_range(at[2], Nv))) return false;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    cl[j] = cluster_of[at[j]];
    ok = ok && in_range(cl[j], Nv);
  }
  if (!ok) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) ok = ms_cell(vertices + 3 * (size_t)at[j], g.origin, g.cell, i[j], q[j]) && ok;
  return ok;
}

// corner j speaks for its cluster unless an earlier corner has the same one: once per distinct cluster of the face
__device__ __forceinline__ bool ms_quadric_speaks(const int* cl, int j) {
  return j == 0 || (cl[j] != cl[0] && (j == 1 || cl[j] != cl[1]));
}

// rule a: the nine coefficients of the face's plane in the frame of corner j's cell -> g; every operation rounded on its own
__device__ __forceinline__ double ms_quadric_coefs(const int (*i)[3], const unsigned long long (*q)[3], int j, double* coef) {
#pragma clang fp contract(off)
  double u[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double frac = (double)q[c][k] * (1.0 / MS_Q_ONE);
      u[c][k] = (double)(i[c][k] - i[j][k]) + frac;                 // |i| < 2^30: the difference is an int
    }
  }
  double a[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = u[1][k] - u[0][k]; b[k] = u[2][k] - u[0][k]; }
  const double y0 = a[1] * b[2], z0 = a[2] * b[1], y1 = a[2] * b[0], z1 = a[0] * b[2], y2 = a[0] * b[1], z2 = a[1] * b[0];
  const double nx = y0 - z0, ny = y1 - z1, nz = y2 - z2;
  const double px = nx * u[0][0], py = ny * u[0][1], pz = nz * u[0][2];
  const double pxy = px + py;
  const double d = -(pxy + pz);
  const double md = -d;
  coef[0] = nx * nx; coef[1] = ny * ny; coef[2] = nz * nz;
  coef[3] = nx * ny; coef[4] = nx * nz; coef[5] = ny * nz;
  coef[6] = md * nx; coef[7] = md * ny; coef[8] = md * nz;
  const double dd = d * d;
  return fmax(fmax(coef[0], coef[1]), fmax(coef[2], dd));           // all four are finite: |u| < 2^32
}
// a contribution counts when g is positive and finite
__device__ __forceinline__ bool ms_quadric_counts(double g) { return g > 0.0 && g < __builtin_inf(); }

__global__ __launch_bounds__(MS_NT) void k_ms_quadric_zero(long long* __restrict__ Q, unsigned* __restrict__ m, int* __restrict__ E,
                                                           size_t n_clusters, long long* __restrict__ counts) {
  const size_t stride = (size_t)gridDim.x * MS_NT;
  const size_t t0 = (size_t)blockIdx.x * MS_NT + threadIdx.x;
  for (size_t i = t0; i < 9 * n_clusters; i += stride) Q[i] = 0;
  for (size_t i = t0; i < n_clusters; i += stride) { m[i] = 0u; E[i] = MS_Q_NONE; }
  if (t0 < 2) counts[5 + t0] = 0;
}

// rule b, the exponent: one lane per face, atomicMax of ilogb(g) per distinct cluster.  Corner 0's maxima are taken over the
// runs of equal clusters in the wave first (a segmented scan, every lane takes part), as k_ms_accumulate sums its runs.
__global__ __launch_bounds__(MS_NT) void k_ms_quadric_exponent(const float* __restrict__ vertices, const int* __restrict__ faces, int Nf,
                                                               int Nv, MsGrid g, const int* __restrict__ cluster_of, int* E) {
  const long long f = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int cl[3] = {-1, -1, -1}, i[3][3];
  unsigned long long q[3][3];
  int e[3] = {MS_Q_NONE, MS_Q_NONE, MS_Q_NONE};
  if (ms_quadric_face(vertices, faces, f, Nf, Nv, g, cluster_of, cl, i, q)) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!ms_quadric_speaks(cl, j)) continue;
      double coef[9];
      const double gg = ms_quadric_coefs(i, q, j, coef);
      if (ms_quadric_counts(gg)) e[j] = ilogb(gg);
    }
  } else {
    cl[0] = -1;
  }
#pragma unroll
  for (int j = 1; j < 3; ++j)
    if (e[j] != MS_Q_NONE) atomicMax(&E[cl[j]], e[j]);
  const int key = cl[0];
  const int key_before = __shfl_up(key, 1, 64), key_after = __shfl_down(key, 1, 64);
  bool head = lane == 0 || key_before != key;
  int top = e[0];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int tt = __shfl_up(top, off, 64);
    const int th = __shfl_up((int)head, off, 64);
    if (lane >= off && !head) {
      top = tt > top ? tt : top;
      head = th != 0;
    }
  }
  const bool tail = lane == 63 || key_after != key;
  if (key >= 0 && tail && top != MS_Q_NONE) atomicMax(&E[key], top);
}

// rule b, the sums: one lane per face; per distinct cluster nine int64 atomicAdds of llrint(ldexp(coef, 40 - E)) and one of the
// count.  Corner 0's ten values are summed over the runs of equal clusters in the wave first: integers, so the same sums.
__global__ __launch_bounds__(MS_NT) void k_ms_quadric_accumulate(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                 int Nf, int Nv, MsGrid g, const int* __restrict__ cluster_of,
                                                                 const int* __restrict__ E, unsigned long long* Q, unsigned* m) {
  const long long f = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int cl[3] = {-1, -1, -1}, i[3][3];
  unsigned long long q[3][3];
  unsigned long long s[9] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};     // corner 0's, two's complement
  unsigned n = 0u;
  if (ms_quadric_face(vertices, faces, f, Nf, Nv, g, cluster_of, cl, i, q)) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!ms_quadric_speaks(cl, j)) continue;
      double coef[9];
      const double gg = ms_quadric_coefs(i, q, j, coef);
      if (!ms_quadric_counts(gg)) continue;
      const int ec = E[cl[j]];
      if (ec < ilogb(gg)) continue;                                 // not the E of k_ms_quadric_exponent over these faces
      const int shift = MS_Q_BITS - ec;
      if (j == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = (unsigned long long)llrint(ldexp(coef[k], shift));
        n = 1u;
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) atomicAdd(&Q[9 * (size_t)cl[j] + k], (unsigned long long)llrint(ldexp(coef[k], shift)));
        atomicAdd(&m[cl[j]], 1u);
      }
    }
  } else {
    cl[0] = -1;
  }
  const int key = cl[0];
  const int key_before = __shfl_up(key, 1, 64), key_after = __shfl_down(key, 1, 64);
  bool head = lane == 0 || key_before != key;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned long long ts[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ts[k] = __shfl_up(s[k], off, 64);
    const unsigned tn = __shfl_up(n, off, 64);
    const int th = __shfl_up((int)head, off, 64);
    if (lane >= off && !head) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s[k] += ts[k];
      n += tn;
      head = th != 0;
    }
  }
  const bool tail = lane == 63 || key_after != key;
  if (key < 0 || !tail || n == 0u) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) atomicAdd(&Q[9 * (size_t)key + k], s[k]);
  atomicAdd(&m[key], n);
}

// rule c in the fixed order: M = A + l I, r = b + l mu, x = adj(M) r / det(M) by cofactors -> false where the mean stands
__device__ __forceinline__ bool ms_quadric_solve(const long long* __restrict__ Q, const double* mu, double regularize, double* x) {
#pragma clang fp contract(off)
  const double A00 = (double)Q[0], A11 = (double)Q[1], A22 = (double)Q[2];
  const double M01 = (double)Q[3], M02 = (double)Q[4], M12 = (double)Q[5];
  const double tr = (A00 + A11) + A22;
  if (!(tr > 0.0)) return false;
  const double l = regularize * tr;
  const double M00 = A00 + l, M11 = A11 + l, M22 = A22 + l;
  double r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lm = l * mu[k];
    r[k] = (double)Q[6 + k] + lm;
  }
  const double p0 = M11 * M22, p1 = M12 * M12, p2 = M02 * M12, p3 = M01 * M22, p4 = M01 * M12, p5 = M02 * M11;
  const double p6 = M00 * M22, p7 = M02 * M02, p8 = M01 * M02, p9 = M00 * M12, p10 = M00 * M11, p11 = M01 * M01;
  const double c00 = p0 - p1, c01 = p2 - p3, c02 = p4 - p5, c11 = p6 - p7, c12 = p8 - p9, c22 = p10 - p11;
  const double d0 = M00 * c00, d1 = M01 * c01, d2 = M02 * c02;
  const double d01 = d0 + d1;
  const double det = d01 + d2;
  if (!(det > 0.0)) return false;
  const double row[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t0 = row[k][0] * r[0], t1 = row[k][1] * r[1], t2 = row[k][2] * r[2];
    const double t01 = t0 + t1;
    const double num = t01 + t2;
    x[k] = num / det;
    ok = ok && is_finite(x[k]);
  }
  return ok;
}

// rules c and d, after k_ms_write: one lane per cluster; an emitted cluster whose quadric solves takes the solved position in its
// row, every other row keeps k_ms_write's mean.  counts[5] += emitted clusters left at the mean, counts[6] += clamped ones.
// bits, pre, wg: the referenced clusters' keep list, scanned
__global__ __launch_bounds__(MS_NT) void k_ms_quadric_place(MsGrid g, double regularize, const unsigned long long* __restrict__ S,
                                                            const unsigned* __restrict__ nC, const int* __restrict__ cell_of,
                                                            const long long* __restrict__ Q, const unsigned* __restrict__ m,
                                                            const unsigned long long* __restrict__ bits, const unsigned* __restrict__ pre,
                                                            const unsigned* __restrict__ wg, long long words,
                                                            float* __restrict__ vertices_out, unsigned long long* counts) {
  const long long i = (long long)blockIdx.x * MS_NT + threadIdx.x;
  const KeepList clusters{bits, pre, wg};
  const bool live = i < words * 64 && clusters.kept(i);
  bool solved = false, clamped = false;
  if (live) {
    const unsigned mc = m[i];
    double mu[3], x[3];
    const unsigned n = nC[4 * i];
#pragma unroll
    for (int k = 0; k < 3; ++k) mu[k] = ms_mean_fraction(S[3 * i + k], n);
    solved = mc > 0u && mc < MS_Q_CAP && ms_quadric_solve(Q + 9 * i, mu, regularize, x);
    if (solved) {
      const size_t row = (size_t)(int)clusters.rank(i);
      const int lin = cell_of[i];
      const int c[3] = {lin % g.dims[0], (lin / g.dims[0]) % g.dims[1], lin / g.dims[0] / g.dims[1]};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        clamped = clamped || x[k] < 0.0 || x[k] > 1.0;
        const double xk = fmin(fmax(x[k], 0.0), 1.0);
        vertices_out[3 * row + k] = ms_position_at(g.origin[k], g.cell, g.lo[k] + c[k], xk);
      }
    }
  }
  wave_count(&counts[5], live && !solved);
  wave_count(&counts[6], clamped);
}

__global__ __launch_bounds__(64) void k_ms_finish(const int* __restrict__ flag, long long* __restrict__ counts) {
  if (threadIdx.x) return;
  const int bits = *flag;
  if (bits & 1) counts[1] = -1;
  if (bits & 2) counts[0] = -1;
}

static bool ms_shape(long long Nv, long long Nf, long long cells) {
  return mesh_shape(Nv, Nf) && cells >= 1 && cells < (1ll << 31);
}
static size_t ms_capacity(long long Nf) {
  size_t cap = 64;
  while (cap < 2 * (size_t)Nf) cap <<= 1;
  return cap;
}

// the workspace, 8-byte words first: [zeroed: flag | cell bits | referenced bits, face bits | S | n, C] [table], then the 4-byte
// arrays.  words_c, words_2: the keep words of the cells / of the clusters and of the faces (each); n_zero: the 8-byte words
// k_ms_zero clears; cap: the table's slots
struct MsWs {
  size_t words_c, words_2, n_zero, cap, bytes;
  int* flag; unsigned long long* cell_bits; unsigned long long* bits_2; unsigned long long* S; unsigned* nC; int* table;
  unsigned* pre_c; unsigned* pre_2; unsigned* wg_c; unsigned* wg_2; int* cell_of; int* cluster_of; int* tri;
};
static MsWs ms_carve(void* workspace, long long Nv, long long Nf, long long cells) {
  Carver c(workspace);
  MsWs w;
  w.words_c = round_up(((size_t)cells + 63) / 64, KEEP_GROUP);
  w.words_2 = (size_t)mf_workgroups(Nv, Nf) * KEEP_GROUP;
  w.cap = ms_capacity(Nf);
  w.flag = c.take<int>(2);
  w.cell_bits = c.take<unsigned long long>(w.words_c);
  w.bits_2 = c.take<unsigned long long>(2 * w.words_2);
  w.S = c.take<unsigned long long>(3 * (size_t)Nv);
  w.nC = c.take<unsigned>(4 * (size_t)Nv);
  w.n_zero = c.at / 8;
  w.table = c.take<int>(w.cap);
  w.pre_c = c.take<unsigned>(w.words_c);
  w.pre_2 = c.take<unsigned>(2 * w.words_2);
  w.wg_c = c.take<unsigned>(w.words_c / KEEP_GROUP);
  w.wg_2 = c.take<unsigned>(2 * (w.words_2 / KEEP_GROUP));
  w.cell_of = c.take<int>((size_t)Nv);
  w.cluster_of = c.take<int>((size_t)Nv);
  w.tri = c.take<int>(3 * (size_t)Nf);
  w.bytes = c.bytes();
  return w;
}

// the quadric workspace: the layout above as one piece, then per cluster (at most Nv) the nine sums, the count and the exponent
struct MsQuadricWs { MsWs mean; long long* Q; unsigned* m; int* E; size_t bytes; };
static MsQuadricWs ms_quadric_carve(void* workspace, long long Nv, long long Nf, long long cells) {
  Carver c(workspace);
  MsQuadricWs w;
  w.mean = ms_carve(workspace, Nv, Nf, cells);
  c.take<char>(w.mean.bytes);
  w.Q = c.take<long long>(9 * (size_t)Nv);
  w.m = c.take<unsigned>((size_t)Nv);
  w.E = c.take<int>((size_t)Nv);
  w.bytes = c.bytes();
  return w;
}

// the refusals that both entry points share, under the caller's name -> 0 and the cells of the box
static int ms_check(const char* who, const LrfMeshSimplify* m, const float* vertices_out, const uint8_t* rgb8_out,
                    const int32_t* faces_out, const int64_t* counts, const void* workspace, long long* cells_out) {
  if (!mesh_shape(m->Nv, m->Nf)) return refuse(who, "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (!m->vertices || !vertices_out || !counts || !workspace || (m->Nf && (!m->faces || !faces_out))) return refuse(who, "null argument");
  if (!m->rgb8 != !rgb8_out) return refuse(who, "rgb8 and rgb8_out go together");
  long long cells = 1;
  for (int k = 0; k < 3; ++k) {
    if (m->dims[k] < 1 || cells >= (1ll << 31)) return refuse(who, "need dims >= 1 and 1 <= cells < 2^31");
    cells *= m->dims[k];
  }
  if (cells >= (1ll << 31)) return refuse(who, "need dims >= 1 and 1 <= cells < 2^31");
  for (int k = 0; k < 3; ++k)
    if (m->lo[k] <= -(1 << 30) || (long long)m->lo[k] + m->dims[k] > (1 << 30)) return refuse(who, "the box must lie inside (-2^30, 2^30)");
  if (!(is_finite(m->origin[0]) && is_finite(m->origin[1]) && is_finite(m->origin[2]))) return refuse(who, "origin must hold 3 finite values");
  if (!(m->cell > 0.0 && is_finite(m->cell))) return refuse(who, "cell must be finite and > 0");
  if (misaligned(3, m->vertices, m->faces, vertices_out, faces_out)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, counts, workspace)) return refuse(who, "counts and workspace must be 8-byte aligned");
  *cells_out = cells;
  return 0;
}

static MsGrid ms_grid(const LrfMeshSimplify* m) {
  MsGrid g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < 3; ++k) { g.origin[k] = m->origin[k]; g.lo[k] = m->lo[k]; g.dims[k] = m->dims[k]; }
  g.cell = m->cell;
  return g;
}

// every launch of the mean placement but the last, k_ms_finish
static int ms_enqueue(const LrfMeshSimplify* m, const MsWs& w, const MsGrid& g, float* vertices_out, uint8_t* rgb8_out,
                      int32_t* faces_out, int64_t* counts, void* workspace, hipStream_t st) {
  const int Nv = (int)m->Nv, Nf = (int)m->Nf;
  long long* cnt = reinterpret_cast<long long*>(counts);
  unsigned long long* ucnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned long long mask = w.cap - 1;
  const bool dedupe = m->dedupe != 0 && Nf > 0;
  const size_t n_table = dedupe ? w.cap / 2 : 0;                    // 8-byte words
  const size_t most = w.n_zero > n_table ? w.n_zero : n_table;
  const size_t zero_blocks = (most + MS_NT - 1) / MS_NT;
  const unsigned nbv = blocks_for(Nv, MS_NT), nbf = blocks_for(Nf, MS_NT);
  LRF_TRY(launch(k_ms_zero, (unsigned)(zero_blocks < MS_ZERO_BLOCKS ? zero_blocks : MS_ZERO_BLOCKS), MS_NT, st,
                 static_cast<unsigned long long*>(workspace), w.n_zero, reinterpret_cast<unsigned long long*>(w.table), n_table, cnt));
  LRF_TRY(launch(k_ms_mark, nbv, MS_NT, st, m->vertices, Nv, g, w.cell_bits, w.flag));
  LRF_TRY(launch(k_ms_count_words, blocks_for((long long)w.words_c, MS_NT), MS_NT, st, w.cell_bits, w.pre_c, w.wg_c, w.words_c));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.wg_c, w.words_c / KEEP_GROUP, cnt + 2));
  if (Nf) {
    const long long words = (long long)w.words_2;
    LRF_TRY(launch(k_ms_accumulate, nbv, MS_NT, st, m->vertices, m->rgb8, Nv, g, w.cell_bits, w.pre_c, w.wg_c, w.S, w.nC, w.cell_of,
                   w.cluster_of));
    LRF_TRY(launch(k_ms_faces_map, nbf, MS_NT, st, m->faces, Nf, Nv, w.cluster_of, w.tri, w.flag, ucnt));
    if (dedupe) LRF_TRY(launch(k_ms_faces_insert, nbf, MS_NT, st, w.tri, Nf, w.table, mask));
    LRF_TRY(launch(k_ms_faces_keep, blocks_for(words * 64, MS_NT), MS_NT, st, w.tri, Nf, Nv, w.table, mask, dedupe ? 1 : 0,
                   w.bits_2 + words, w.bits_2, ucnt));
    LRF_TRY(launch(k_ms_count_words, dim3(blocks_for(words, MS_NT), 2), MS_NT, st, w.bits_2, w.pre_2, w.wg_2, words));
    LRF_TRY(launch(k_points_scan, 2, PTS_SCAN_NT, st, w.wg_2, words / KEEP_GROUP, cnt));
    LRF_TRY(launch(k_ms_write, dim3(blocks_for(words * 64, MS_NT), 2), MS_NT, st, g, w.S, w.nC, w.cell_of, w.tri, w.bits_2, w.pre_2,
                   w.wg_2, words, vertices_out, rgb8_out, faces_out));
  }
  return 0;
}

}  // namespace lrf

extern "C" int lrf_mesh_simplify_bounds(const float* vertices, int64_t Nv, const double* origin, double cell, int32_t* out,
                                        void* stream) {
  using namespace lrf;
  if (!mesh_shape(Nv, 0)) return set_err("lrf_mesh_simplify_bounds: need 1 <= Nv < 2^31");
  if (!vertices || !origin || !out) return set_err("lrf_mesh_simplify_bounds: null argument");
  if (!(is_finite(origin[0]) && is_finite(origin[1]) && is_finite(origin[2])))
    return set_err("lrf_mesh_simplify_bounds: origin must hold 3 finite values");
  if (!(cell > 0.0 && is_finite(cell))) return set_err("lrf_mesh_simplify_bounds: cell must be finite and > 0");
  if (misaligned(3, vertices, out)) return set_err("lrf_mesh_simplify_bounds: float and int32 arrays must be 4-byte aligned");
  MsGrid g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < 3; ++k) g.origin[k] = origin[k];
  g.cell = cell;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_ms_bounds_init, 1, 64, st, out));
  return launch(k_ms_bounds, blocks_for(Nv, MS_NT), MS_NT, st, vertices, Nv, g, out);
}

extern "C" size_t lrf_mesh_simplify_workspace_bytes(int64_t Nv, int64_t Nf, int64_t cells) {
  using namespace lrf;
  return ms_shape(Nv, Nf, cells) ? ms_carve(nullptr, Nv, Nf, cells).bytes : 0;
}

extern "C" int lrf_mesh_simplify(const LrfMeshSimplify* m, float* vertices_out, uint8_t* rgb8_out, int32_t* faces_out,
                                 int64_t* counts, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_simplify";
  if (!m) return refuse(who, "null argument");
  long long cells = 0;
  LRF_TRY(ms_check(who, m, vertices_out, rgb8_out, faces_out, counts, workspace, &cells));
  const MsWs w = ms_carve(workspace, m->Nv, m->Nf, cells);
  const MsGrid g = ms_grid(m);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(ms_enqueue(m, w, g, vertices_out, rgb8_out, faces_out, counts, workspace, st));
  return launch(k_ms_finish, 1, 64, st, w.flag, reinterpret_cast<long long*>(counts));
}

extern "C" size_t lrf_mesh_simplify_quadric_workspace_bytes(int64_t Nv, int64_t Nf, int64_t cells) {
  using namespace lrf;
  return ms_shape(Nv, Nf, cells) ? ms_quadric_carve(nullptr, Nv, Nf, cells).bytes : 0;
}

extern "C" int lrf_mesh_simplify_quadric(const LrfMeshSimplifyQuadric* q, float* vertices_out, uint8_t* rgb8_out, int32_t* faces_out,
                                         int64_t* counts, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_simplify_quadric";
  if (!q) return refuse(who, "null argument");
  const LrfMeshSimplify* m = &q->mesh;
  long long cells = 0;
  LRF_TRY(ms_check(who, m, vertices_out, rgb8_out, faces_out, counts, workspace, &cells));
  if (!(q->regularize > 0.0 && q->regularize <= 1.0)) return refuse(who, "regularize must lie in (0, 1]");      // NaN fails
  const int Nv = (int)m->Nv, Nf = (int)m->Nf;
  const MsQuadricWs w = ms_quadric_carve(workspace, m->Nv, m->Nf, cells);
  const MsGrid g = ms_grid(m);
  long long* cnt = reinterpret_cast<long long*>(counts);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t zero_blocks = (9 * (size_t)Nv + MS_NT - 1) / MS_NT;
  LRF_TRY(launch(k_ms_quadric_zero, (unsigned)(zero_blocks < MS_ZERO_BLOCKS ? zero_blocks : MS_ZERO_BLOCKS), MS_NT, st, w.Q, w.m, w.E,
                 (size_t)Nv, cnt));
  LRF_TRY(ms_enqueue(m, w.mean, g, vertices_out, rgb8_out, faces_out, counts, workspace, st));
  if (Nf) {
    const long long words = (long long)w.mean.words_2;
    const unsigned nbf = blocks_for(Nf, MS_NT);
    LRF_TRY(launch(k_ms_quadric_exponent, nbf, MS_NT, st, m->vertices, m->faces, Nf, Nv, g, w.mean.cluster_of, w.E));
    LRF_TRY(launch(k_ms_quadric_accumulate, nbf, MS_NT, st, m->vertices, m->faces, Nf, Nv, g, w.mean.cluster_of, w.E,
                   reinterpret_cast<unsigned long long*>(w.Q), w.m));
    LRF_TRY(launch(k_ms_quadric_place, blocks_for(words * 64, MS_NT), MS_NT, st, g, q->regularize, w.mean.S, w.mean.nC, w.mean.cell_of,
                   w.Q, w.m, w.mean.bits_2, w.mean.pre_2, w.mean.wg_2, words, vertices_out, reinterpret_cast<unsigned long long*>(counts)));
  }
  return launch(k_ms_finish, 1, 64, st, w.mean.flag, cnt);
}
