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

// item 4's position: every operation is rounded on its own
__device__ __forceinline__ float ms_position(double origin, double cell, int i, unsigned long long S, unsigned n) {
#pragma clang fp contract(off)
  const double mean = (double)S / (double)n;
  const double frac = mean * (1.0 / MS_Q_ONE);
  const double t = (double)i + frac;
  const double x = t * cell;
  return (float)(origin + x);
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
  if (!m) return set_err("lrf_mesh_simplify: null argument");
  if (!mesh_shape(m->Nv, m->Nf)) return set_err("lrf_mesh_simplify: need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (!m->vertices || !vertices_out || !counts || !workspace || (m->Nf && (!m->faces || !faces_out)))
    return set_err("lrf_mesh_simplify: null argument");
  if (!m->rgb8 != !rgb8_out) return set_err("lrf_mesh_simplify: rgb8 and rgb8_out go together");
  long long cells = 1;
  for (int k = 0; k < 3; ++k) {
    if (m->dims[k] < 1 || cells >= (1ll << 31)) return set_err("lrf_mesh_simplify: need dims >= 1 and 1 <= cells < 2^31");
    cells *= m->dims[k];
  }
  if (cells >= (1ll << 31)) return set_err("lrf_mesh_simplify: need dims >= 1 and 1 <= cells < 2^31");
  for (int k = 0; k < 3; ++k)
    if (m->lo[k] <= -(1 << 30) || (long long)m->lo[k] + m->dims[k] > (1 << 30))
      return set_err("lrf_mesh_simplify: the box must lie inside (-2^30, 2^30)");
  if (!(is_finite(m->origin[0]) && is_finite(m->origin[1]) && is_finite(m->origin[2])))
    return set_err("lrf_mesh_simplify: origin must hold 3 finite values");
  if (!(m->cell > 0.0 && is_finite(m->cell))) return set_err("lrf_mesh_simplify: cell must be finite and > 0");
  if (misaligned(3, m->vertices, m->faces, vertices_out, faces_out))
    return set_err("lrf_mesh_simplify: float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, counts, workspace)) return set_err("lrf_mesh_simplify: counts and workspace must be 8-byte aligned");
  const int Nv = (int)m->Nv, Nf = (int)m->Nf;
  const MsWs w = ms_carve(workspace, m->Nv, m->Nf, cells);
  MsGrid g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < 3; ++k) { g.origin[k] = m->origin[k]; g.lo[k] = m->lo[k]; g.dims[k] = m->dims[k]; }
  g.cell = m->cell;
  long long* cnt = reinterpret_cast<long long*>(counts);
  unsigned long long* ucnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned long long mask = w.cap - 1;
  const bool dedupe = m->dedupe != 0 && Nf > 0;
  const size_t n_table = dedupe ? w.cap / 2 : 0;                    // 8-byte words
  const size_t most = w.n_zero > n_table ? w.n_zero : n_table;
  const size_t zero_blocks = (most + MS_NT - 1) / MS_NT;
  const unsigned nbv = blocks_for(Nv, MS_NT), nbf = blocks_for(Nf, MS_NT);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
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
  return launch(k_ms_finish, 1, 64, st, w.flag, cnt);
}
